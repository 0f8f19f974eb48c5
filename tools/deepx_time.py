#!/usr/bin/env python3
"""Device time of fr_render_deepx (profiles/deepx_time.txt): view B (1e-100) through fr_render_deep and through
fr_render_deepx (the same arithmetic after each sample's first step), views D (1e-400) and E (1e-1000) of
tests/golden/deepx_views.json, all at 4096^2, and the host's reference orbit for D and E.

Lane-updates are counted from the iter plane as in deep_time.py: i + 1 for a sample that escaped at loop index i,
max_iter for one that did not.
usage: deepx_time.py [out.txt]"""
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
import deepx_ref as X  # noqa: E402

REPS = 7
N = 4096


def updates(it, max_iter):
    it = it.astype(np.int64)
    return int(np.where(it < max_iter, it + 1, max_iter).sum())


def timed(r, fn):
    fn()                                                     # warm-up (and the view's reference orbit)
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
    V = X.views()
    B = R.VIEW_B
    say(f"# fr_render_deepx, one GPU; median (min) of {REPS} renders after a warm-up, device time from the context's event "
        f"pair; G lane-updates/s = updates / median")
    it = torch.empty((N, N), dtype=torch.int32, device=dev)
    rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
    with fr.Renderer(0) as r:
        cases = [("view B (1e-100)", "deep ", fr.FractalState(zoom=B["zoom"], max_iterations=B["max_iter"]),
                  fr.DeepView(B["cx"], B["cy"]), B["max_iter"]),
                 ("view B (1e-100)", "deepx", fr.FractalState(max_iterations=B["max_iter"]),
                  fr.DeepView(B["cx"], B["cy"], zoom=repr(B["zoom"])), B["max_iter"])]
        for name, label in (("D", "view D (1e-400)"), ("E", "view E (1e-1000)")):
            v = V[name]
            cases.append((label, "deepx", fr.FractalState(max_iterations=v["max_iter"]),
                          fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]), v["max_iter"]))
        for label, entry, st, view, max_iter in cases:
            med, lo = timed(r, lambda: r.render_deep(st, N, N, view, rgba=rgba, iter=it))
            u = updates(it.cpu().numpy(), max_iter)
            say(f"{label:17s} {N}^2 max_iter {max_iter:5d} {entry}  {med:9.3f} ms ({lo:.3f})  {u / 1e9:8.3f} G updates  "
                f"{u / med / 1e6:7.1f} G lane-updates/s  grid {r.last_grid() & 0xffff}")
    say("# host reference orbit (fr_deepx_reference_orbit, one CPU thread): wall time of one call")
    for name in ("D", "E"):
        v = V[name]
        t = time.perf_counter()
        _, e = fr.deepx_reference_orbit(fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"]), v["max_iter"])
        dt = time.perf_counter() - t
        say(f"view {name}             F = {fr.deepx_frac_bits(v['zoom']):4d}  {len(e) - 1:7d} iterations  {dt * 1e3:9.2f} ms  "
            f"{dt / max(len(e) - 1, 1) * 1e6 * 1e3:8.1f} ms per 10^6 iterations")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
