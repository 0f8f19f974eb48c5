#!/usr/bin/env python3
"""Device time of fr_render_deep_ship_de / fr_render_deepx_ship_de next to fr_render_deep_ship / fr_render_deepx_ship
(profiles/deep_ship_de_time.txt), on one context at 4096^2: SHIP_A (1e-30) and SHIP_B (1e-100) with fp64 deltas, S400 (1e-400)
and TIP1000 (1e-1000) with extended deltas, each with its BLA flag off and on.

Per view and flag the two entry points are interleaved: after a warm-up of each (orbit, table, the occupancy queries), REPS
rounds of one plain render (rgba, iter) and one distance render (rgba, iter, de, deriv; shade off), device time from the
context's event pair; median (min) of each, the ratio DE / plain of the medians, and the lane-updates per second of both (the
updates of sample (0,0) of every pixel, min(iter + 1, max_iter), from the iter plane).
usage: deep_ship_de_time.py [out.txt]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fractalrenderer_amd as fr  # noqa: E402
import deep_ship_ref as S  # noqa: E402
import deepx_ship_ref as XS  # noqa: E402

REPS = 7
N = 4096


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    say(f"# plain (rgba, iter) and distance (rgba, iter, de, deriv; shade 0) renders interleaved, one GPU, one context; median (min) "
        f"of {REPS} renders each after a warm-up, device time from the context's event pair; G/s = lane-updates per second")
    with fr.Renderer(0) as r:
        r.set_option("timing", 1)
        rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
        it = torch.empty((N, N), dtype=torch.int32, device=dev)
        de = torch.empty((N, N), dtype=torch.float64, device=dev)
        deriv = torch.empty((N, N, 4), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def ship(label, v):
            ext = isinstance(v["zoom"], str)
            if ext:
                st = fr.FractalState(max_iterations=v["max_iter"])
                view = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"])
                plain, names = r.render_deepx_ship, ("fr_render_deepx_ship", "fr_render_deepx_ship_de")
            else:
                st = fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"])
                view = fr.DeepView(v["cx"], v["cy"])
                plain, names = r.render_deep_ship, ("fr_render_deep_ship", "fr_render_deep_ship_de")
            return (label, v["max_iter"], names,
                    lambda bla: plain(st, N, N, view, rgba=rgba, iter=it, bla=bla),
                    lambda bla: r.render_deep_ship_de(st, N, N, view, rgba=rgba, iter=it, de=de, deriv=deriv, bla=bla))

        xv = XS.views()
        cases = [ship("SHIP_A (1e-30)", S.SHIP_A), ship("SHIP_B (1e-100)", S.SHIP_B), ship("S400 (1e-400)", xv["S400"]),
                 ship("TIP1000 (1e-1000)", xv["TIP1000"])]
        for label, max_iter, names, plain, dist in cases:
            for bla in (False, True):
                runs = [("plain", names[0], plain), ("de", names[1], dist)]
                for _, _, f in runs:                              # warm-up: orbit, table, the occupancy queries
                    f(bla)
                updates = int(torch.clamp(it.to(torch.int64) + 1, max=max_iter).sum().item())
                ms = {key: [] for key, _, _ in runs}
                for _ in range(REPS):
                    for key, _, f in runs:
                        f(bla)
                        ms[key].append(r.last_kernel_ms())
                med = {key: statistics.median(t) for key, t in ms.items()}
                for key, name, _ in runs:
                    say(f"{label:17s} {N}^2 max_iter {max_iter:5d} BLA {'on ' if bla else 'off'} {name:24s} "
                        f"{med[key]:9.3f} ms ({min(ms[key]):.3f}) {updates / med[key] / 1e6:7.1f} G/s")
                say(f"{label:17s} BLA {'on ' if bla else 'off'} DE / plain = {med['de'] / med['plain']:.3f}")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
