#!/usr/bin/env python3
"""Mandelbulb frame times (fr_render_mandelbulb) and the march / shade split A/B.

    python tools/mandelbulb_time.py [--reps N] [--de-calls N]
    python tools/mandelbulb_time.py --count-de        (host only: the DE calls of the 1700x900 aa 1 frame)

Default view (FractalState and MandelbulbParams initialisers: power 8, max_iter 256, time 0), post-chained rgba plane.
Device time from the context's "timing" event pair, median of N renders after warm-up, at 1700x900 (the reference's
window), 1920x1080 and 4096^2, aa 1 and 2.  Each frame is timed with the march / shade split (the default,
"mandelbulb_split" 0) and with in-loop shading ("mandelbulb_split" 1), alternating, so that clock drift hits both alike.
DE calls per frame are counted on the host by tests/mandelbulb_ref.py (one per march step, 12 per hit); --de-calls
passes that count for the 1700x900 aa 1 frame and the DE call rate is reported for it.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CASES = ((1700, 900, 1), (1920, 1080, 1), (4096, 4096, 1), (1700, 900, 2), (1920, 1080, 2), (4096, 4096, 2))


def count_de():
    import mandelbulb_ref
    W, H = 1700, 900
    total = 0
    for r0 in range(0, H, 50):
        mandelbulb_ref.render(W, H, rows=(r0, min(H, r0 + 50)))
        total += mandelbulb_ref.de_calls
    print(json.dumps({"W": W, "H": H, "aa": 1, "de_calls": total, "per_pixel": round(total / (W * H), 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--de-calls", type=int, default=0)
    ap.add_argument("--count-de", action="store_true")
    args = ap.parse_args()
    if args.count_de:
        return count_de()
    import torch
    import fractalrenderer_amd as fr
    dev = torch.device("cuda:0")
    r = fr.Renderer(0)
    r.set_option("timing", 1)
    st0, mb = fr.FractalState(), fr.MandelbulbParams()
    for W, H, aa in CASES:
        st = fr.FractalState(antialiasing_samples=aa)
        rgba = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        ms = {0: [], 1: []}
        for split in (0, 1):                                  # warm-up, both variants
            r.set_option("mandelbulb_split", split)
            for _ in range(2):
                r.render_mandelbulb(st, W, H, mb, post_chain=True, rgba=rgba)
        for _ in range(args.reps):
            for split in (0, 1):
                r.set_option("mandelbulb_split", split)
                r.render_mandelbulb(st, W, H, mb, post_chain=True, rgba=rgba)
                ms[split].append(r.last_kernel_ms())
        r.set_option("mandelbulb_split", 0)
        med = {k: statistics.median(v) for k, v in ms.items()}
        line = {"kernel": "mandelbulb", "W": W, "H": H, "aa": aa, "max_iter": st0.max_iterations, "ms": round(med[0], 4),
                "ms_min": round(min(ms[0]), 4), "ms_max": round(max(ms[0]), 4), "mpix_s": round(W * H / med[0] / 1e3, 1),
                "ms_in_loop_shading": round(med[1], 4), "split_speedup": round(med[1] / med[0], 3), "grid": r.last_grid()}
        if args.de_calls and (W, H, aa) == (1700, 900, 1):
            line["de_calls"] = args.de_calls
            line["de_calls_per_s"] = round(args.de_calls / (med[0] * 1e-3) / 1e9, 3)   # G/s
        print(json.dumps(line), flush=True)
    r.close()


if __name__ == "__main__":
    main()
