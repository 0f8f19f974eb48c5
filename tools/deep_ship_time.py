#!/usr/bin/env python3
"""Device time of fr_render_deep_ship (profiles/deep_ship_time.txt): the tests' 1e-30 and 1e-100 Burning Ship views at
4096^2, next to fr_render_deep on its own 1e-30 and 1e-100 views from the same session for scale.

"timing" = 1; the time is fr_ctx_last_kernel_ms (the context's event pair), all three planes on the device.  Lane-updates
are counted from the iter plane, as the perturbation step executes them: i + 1 for a sample that escaped at loop index i,
max_iter for one that did not.
usage: deep_ship_time.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fractalrenderer_amd as fr  # noqa: E402
import deep_ref as R  # noqa: E402
import deep_ship_ref as S  # noqa: E402

REPS, WARM, N = 7, 3, 4096


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
    nu = torch.empty((N, N), dtype=torch.float64, device=dev)
    it = torch.empty((N, N), dtype=torch.int32, device=dev)
    say(f"# fr_render_deep_ship next to fr_render_deep, one GPU, {N}^2, aa 1, rgba + nu + iter on the device; median (min) of "
        f"{REPS} renders after {WARM} warm-ups, device time from the context's event pair (\"timing\" = 1); "
        f"G lane-updates/s = updates / median")
    with fr.Renderer(0) as r:
        r.set_option("timing", 1)
        for label, v, ship in (("ship A (1e-30)", S.SHIP_A, True), ("ship B (1e-100)", S.SHIP_B, True),
                               ("view A (1e-30)", R.VIEW_A, False), ("view B (1e-100)", R.VIEW_B, False)):
            st = fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"])
            view = fr.DeepView(v["cx"], v["cy"])
            fn = r.render_deep_ship if ship else r.render_deep
            ms = []
            for k in range(WARM + REPS):
                fn(st, N, N, view, rgba=rgba, nu=nu, iter=it)
                if k >= WARM:
                    ms.append(r.last_kernel_ms())
            torch.cuda.synchronize()
            i = it.cpu().numpy().astype(np.int64)
            u = int(np.where(i < v["max_iter"], i + 1, v["max_iter"]).sum())
            med, lo = statistics.median(ms), min(ms)
            say(f"{label:16s} {N}^2 max_iter {v['max_iter']:5d} {'fr_render_deep_ship' if ship else 'fr_render_deep':20s} "
                f"{med:9.3f} ms ({lo:.3f})  {u / 1e9:8.3f} G updates  {u / med / 1e6:7.1f} G lane-updates/s  "
                f"escaped {float((i < v['max_iter']).mean()):.3f}  grid {r.last_grid() & 0xffff}")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
