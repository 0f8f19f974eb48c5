#!/usr/bin/env python3
"""Phoenix frame times (fr_render_phoenix), with the Mandelbrot path on the same geometries as the yardstick.

    python tools/phoenix_time.py [--reps N]

Device time from the context's "timing" event pair, median of N renders after warm-up.  For Phoenix it also reports
sum(iter): updates executed per frame, (i + 1) for a sample that escaped at loop index i, max_iter for one that did not,
read from the iter plane (aa = 1), and the op rate at 16 ops per update as written (8 mul + 8 add: the two squares of
an update are those of the previous test), as a fraction of the non-FMA VALU peak of the precision (fp64 39.3 T/s; fp32
78.6 T/s, which counts packed / dual-issued fp32: a scalar fp32 loop tops out at half of it).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import fractalrenderer_amd as fr  # noqa: E402

PEAK = {"f64": 39.3e12, "f32": 78.6e12}
OPS_PER_UPDATE = 16
CASES = (("f64", 4096, 4096, 1024), ("f32", 4096, 4096, 1024), ("f32", 1700, 900, 256))


def timed(fn, r, reps):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(reps):
        fn()
        ms.append(r.last_kernel_ms())
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    r = fr.Renderer(0)
    for prec_name, W, H, mi in CASES:
        prec = fr.Precision.F64 if prec_name == "f64" else fr.Precision.F32
        rgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        it = torch.empty((H, W), dtype=torch.int32, device=dev)
        st = fr.FractalState(max_iterations=mi)
        r.render_phoenix(st, W, H, precision=prec, iter=it)
        updates = int(torch.where(it < mi, it.to(torch.int64) + 1, torch.full_like(it, mi, dtype=torch.int64)).sum())
        med, lo, hi = timed(lambda: r.render_phoenix(st, W, H, precision=prec, rgba=rgba), r, args.reps)
        grid = r.last_grid()
        rate = updates * OPS_PER_UPDATE / (med * 1e-3)
        line = {"kernel": "phoenix", "precision": prec_name, "W": W, "H": H, "max_iter": mi, "ms": round(med, 4),
                "ms_min": round(lo, 4), "ms_max": round(hi, 4), "mpix_s": round(W * H / med / 1e3, 1), "sum_iter": updates,
                "interior": round(float((it == mi).float().mean()), 4), "ops_per_s": round(rate / 1e12, 3),
                "frac_of_valu_peak": round(rate / PEAK[prec_name], 3), "grid": grid}
        print(json.dumps(line), flush=True)
        med, lo, hi = timed(lambda: r.render(st, W, H, precision=prec, rgba=rgba), r, args.reps)
        print(json.dumps({"kernel": "mandelbrot", "precision": prec_name, "W": W, "H": H, "max_iter": mi, "ms": round(med, 4),
                          "ms_min": round(lo, 4), "ms_max": round(hi, 4), "mpix_s": round(W * H / med / 1e3, 1)}), flush=True)
    r.close()


if __name__ == "__main__":
    main()
