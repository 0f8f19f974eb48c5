#!/usr/bin/env python3
"""Device time of fr_render_deep_phoenix (profiles/deep_phoenix_time.txt): the tests' Phoenix views PA30 (1e-30), PA and PB
(1e-100) at 4096^2, next to fr_render_deep on its own 1e-30 and 1e-100 views and fr_render_deep_ship on SHIP_A and SHIP_B, from
the same session and interleaved: every round renders each case once, so drift of the device's clocks falls on all alike.

"timing" = 1; the time is fr_ctx_last_kernel_ms (the context's event pair), all three planes on the device.  Lane-updates
are counted from the iter plane, as the perturbation step executes them: i + 1 for a sample that escaped at loop index i,
max_iter for one that did not.  The three Phoenix views share one orbit slot, so every Phoenix render of a round computes its
orbit on the host first; that is host time in front of the launch and no part of the event pair.
usage: deep_phoenix_time.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fractalrenderer_amd as fr  # noqa: E402
import deep_phoenix_ref as D  # noqa: E402
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
    say(f"# fr_render_deep_phoenix next to fr_render_deep and fr_render_deep_ship, one GPU, {N}^2, aa 1, rgba + nu + iter on the "
        f"device; median (min) of {REPS} renders after {WARM} warm-ups, the cases interleaved round by round, device time from the "
        f"context's event pair (\"timing\" = 1); G lane-updates/s = updates / median")
    cases = [("phoenix PA30 (1e-30)", D.PA30, "phoenix"), ("phoenix PA (1e-100)", D.PA, "phoenix"),
             ("phoenix PB (1e-100)", D.PB, "phoenix"), ("ship A (1e-30)", S.SHIP_A, "ship"), ("ship B (1e-100)", S.SHIP_B, "ship"),
             ("view A (1e-30)", R.VIEW_A, "deep"), ("view B (1e-100)", R.VIEW_B, "deep")]
    names = {"phoenix": "fr_render_deep_phoenix", "ship": "fr_render_deep_ship", "deep": "fr_render_deep"}
    with fr.Renderer(0) as r:
        r.set_option("timing", 1)

        def render(v, kind):
            # Phoenix's flow stripes off, as the other two paths render without theirs
            st = fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], stripe_density=0.0)
            view = fr.DeepView(v["cx"], v["cy"])
            if kind == "phoenix":
                r.render_deep_phoenix(st, N, N, view, fr.PhoenixParams(phoenix_p=v["p"], phoenix_r=v["r"]), rgba=rgba, nu=nu, iter=it)
            else:
                (r.render_deep_ship if kind == "ship" else r.render_deep)(st, N, N, view, rgba=rgba, nu=nu, iter=it)
            return r.last_kernel_ms()

        ms = {label: [] for label, _, _ in cases}
        grids = {}
        for k in range(WARM + REPS):
            for label, v, kind in cases:
                t = render(v, kind)
                grids[label] = r.last_grid() & 0xffff
                if k >= WARM:
                    ms[label].append(t)
        for label, v, kind in cases:
            render(v, kind)
            torch.cuda.synchronize()
            i = it.cpu().numpy().astype(np.int64)
            u = int(np.where(i < v["max_iter"], i + 1, v["max_iter"]).sum())
            med, lo = statistics.median(ms[label]), min(ms[label])
            say(f"{label:21s} {N}^2 max_iter {v['max_iter']:5d} {names[kind]:23s} {med:9.3f} ms ({lo:.3f})  {u / 1e9:8.3f} G updates  "
                f"{u / med / 1e6:7.1f} G lane-updates/s  escaped {float((i < v['max_iter']).mean()):.3f}  grid {grids[label]}")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
