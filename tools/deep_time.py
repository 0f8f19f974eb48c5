#!/usr/bin/env python3
"""Device time of fr_render_deep (profiles/deep_time.txt): the default view at 1024^2 / max_iter 1024 next to fr_render fp64
on the same view, the tests' 1e-30 and 1e-100 views at 4096^2, and the host's reference orbit as a figure of its own.

Lane-updates are counted from the iter plane, as the perturbation step executes them: i + 1 for a sample that escaped
at loop index i, max_iter for one that did not (fr_render runs with "periodicity" off, so it executes the same count).
usage: deep_time.py [out.txt]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fractalrenderer_amd as fr  # noqa: E402
import deep_ref as R  # noqa: E402

REPS = 7


def updates(it, max_iter):
    it = it.astype(np.int64)
    return int(np.where(it < max_iter, it + 1, max_iter).sum())


def timed(r, fn):
    fn()                                                     # warm-up (and, for a deep view, its reference orbit)
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        fn()
        ms.append(r.last_kernel_ms())
    return statistics.median(ms), min(ms)


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    say(f"# fr_render_deep, one GPU; median (min) of {REPS} renders after a warm-up, device time from the context's event "
        f"pair; G lane-updates/s = updates / median")
    with fr.Renderer(0) as r:
        r.set_option("periodicity", -1)
        cases = [("default view", R.SHALLOW | {"max_iter": 1024}, 1024, True),
                 ("view A (1e-30)", R.VIEW_A, 4096, False), ("view B (1e-100)", R.VIEW_B, 4096, False)]
        for label, v, n, with_fp64 in cases:
            st = fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"])
            view = fr.DeepView(v["cx"], v["cy"])
            it = torch.empty((n, n), dtype=torch.int32, device=dev)
            rgba = torch.empty((n, n, 4), dtype=torch.float32, device=dev)
            med, lo = timed(r, lambda: r.render_deep(st, n, n, view, rgba=rgba, iter=it))
            u = updates(it.cpu().numpy(), v["max_iter"])
            say(f"{label:16s} {n}^2 max_iter {v['max_iter']:5d} deep    {med:9.3f} ms ({lo:.3f})  {u / 1e9:8.3f} G updates  "
                f"{u / med / 1e6:7.1f} G lane-updates/s  grid {r.last_grid() & 0xffff}")
            if with_fp64:
                st64 = fr.FractalState(center_x=float(v["cx"]), center_y=float(v["cy"]), zoom=v["zoom"],
                                       max_iterations=v["max_iter"])
                med, lo = timed(r, lambda: r.render(st64, n, n, precision=fr.Precision.F64, rgba=rgba, iter=it))
                u = updates(it.cpu().numpy(), v["max_iter"])
                say(f"{label:16s} {n}^2 max_iter {v['max_iter']:5d} fr_render fp64 {med:9.3f} ms ({lo:.3f})  {u / 1e9:8.3f} G updates  "
                    f"{u / med / 1e6:7.1f} G lane-updates/s")
    say("# host reference orbit (fr_deep_reference_orbit, one CPU thread): wall time of one call")
    for label, view, zoom, it in [("view A", fr.DeepView(R.VIEW_A["cx"], R.VIEW_A["cy"]), R.VIEW_A["zoom"], R.VIEW_A["max_iter"]),
                                  ("view B", fr.DeepView(R.VIEW_B["cx"], R.VIEW_B["cy"]), R.VIEW_B["zoom"], R.VIEW_B["max_iter"]),
                                  ("interior, 1e-30", fr.DeepView("-0.5", "0"), 1e-30, 200000),
                                  ("interior, 1e-100", fr.DeepView("-0.5", "0"), 1e-100, 200000),
                                  ("interior, 1e-290", fr.DeepView("-0.5", "0"), 1e-290, 200000)]:
        t = time.perf_counter()
        orb = fr.deep_reference_orbit(view, zoom, it)
        dt = time.perf_counter() - t
        say(f"{label:18s} F = {fr.deep_frac_bits(zoom):4d}  {len(orb) - 1:7d} iterations  {dt * 1e3:9.2f} ms  "
            f"{dt / max(len(orb) - 1, 1) * 1e6 * 1e3:8.1f} ms per 10^6 iterations")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
