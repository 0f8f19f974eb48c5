#!/usr/bin/env python3
"""Device time of fr_render_deepx_phoenix (profiles/deepx_phoenix_time.txt): the tests' views PX310, PX400A, PX400B and TIP1000 at
4096^2; PA and PB (1e-100) through both Phoenix entry points; fr_render_deepx on view D and fr_render_deepx_ship on S400 (both
1e-400) for scale -- one session, interleaved: every round renders each case once, so drift of the device's clocks falls on all
alike.

"timing" = 1; the time is fr_ctx_last_kernel_ms (the context's event pair), all three planes on the device.  Lane-updates are
counted from the iter plane, as the perturbation step executes them: i + 1 for a sample that escaped at loop index i, max_iter
for one that did not.  Views that share an orbit slot recompute their orbit on the host in every round; that is host time in
front of the launch and no part of the event pair.
usage: deepx_phoenix_time.py [out.txt]"""
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
import deepx_phoenix_ref as PX  # noqa: E402
import deepx_ref as X  # noqa: E402
import deepx_ship_ref as SX  # noqa: E402

REPS, WARM, N = 5, 2, 4096


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
    nu = torch.empty((N, N), dtype=torch.float64, device=dev)
    it = torch.empty((N, N), dtype=torch.int32, device=dev)
    say(f"# fr_render_deepx_phoenix, one GPU, {N}^2, aa 1, rgba + nu + iter on the device; median (min) of {REPS} renders after "
        f"{WARM} warm-ups, the cases interleaved round by round, device time from the context's event pair (\"timing\" = 1); "
        f"G lane-updates/s = updates / median")
    cases = [(name, v, "xphoenix") for name, v in PX.NEW_VIEWS.items()]
    cases += [("PA (1e-100)", PX.OLD_VIEWS["PA"], "xphoenix"), ("PA (1e-100)", D.PA, "phoenix"),
              ("PB (1e-100)", PX.OLD_VIEWS["PB"], "xphoenix"), ("PB (1e-100)", D.PB, "phoenix"),
              ("view D (1e-400)", X.views()["D"], "deepx"), ("ship S400 (1e-400)", SX.views()["S400"], "xship")]
    names = {"xphoenix": "fr_render_deepx_phoenix", "phoenix": "fr_render_deep_phoenix", "deepx": "fr_render_deepx",
             "xship": "fr_render_deepx_ship"}
    with fr.Renderer(0) as r:
        r.set_option("timing", 1)

        def render(v, kind):
            # Phoenix's flow stripes off, as the other paths render without theirs
            if kind == "phoenix":
                st = fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"], stripe_density=0.0)
                r.render_deep_phoenix(st, N, N, fr.DeepView(v["cx"], v["cy"]), fr.PhoenixParams(phoenix_p=v["p"], phoenix_r=v["r"]),
                                      rgba=rgba, nu=nu, iter=it)
                return r.last_kernel_ms()
            st = fr.FractalState(max_iterations=v["max_iter"], stripe_density=0.0)
            view = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"])
            if kind == "xphoenix":
                r.render_deepx_phoenix(st, N, N, view, fr.PhoenixParams(phoenix_p=v["p"], phoenix_r=v["r"]), rgba=rgba, nu=nu, iter=it)
            else:
                (r.render_deepx_ship if kind == "xship" else r.render_deep)(st, N, N, view, rgba=rgba, nu=nu, iter=it)   # a zoom string: fr_render_deepx
            return r.last_kernel_ms()

        ms = {(label, kind): [] for label, _, kind in cases}
        grids = {}
        for k in range(WARM + REPS):
            for label, v, kind in cases:
                t = render(v, kind)
                grids[(label, kind)] = r.last_grid() & 0xffff
                if k >= WARM:
                    ms[(label, kind)].append(t)
        for label, v, kind in cases:
            render(v, kind)
            torch.cuda.synchronize()
            i = it.cpu().numpy().astype(np.int64)
            u = int(np.where(i < v["max_iter"], i + 1, v["max_iter"]).sum())
            med, lo = statistics.median(ms[(label, kind)]), min(ms[(label, kind)])
            say(f"{label:19s} {N}^2 max_iter {v['max_iter']:5d} {names[kind]:24s} {med:9.3f} ms ({lo:.3f})  {u / 1e9:8.3f} G updates  "
                f"{u / med / 1e6:7.1f} G lane-updates/s  escaped {float((i < v['max_iter']).mean()):.3f}  grid {grids[(label, kind)]}")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
