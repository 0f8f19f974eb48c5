#!/usr/bin/env python3
"""Device time of fr_render_deep_de next to fr_render_deep (profiles/deep_de_time.txt), on one context: the default view,
view B (1e-100) and view C (1e-50, next to a minibrot) at 4096^2, each with FR_FLAG_DEEP_BLA off and on.

Per view and flag the two entry points are interleaved in one session: after a warm-up of both (orbit, table), REPS rounds of
one fr_render_deep (rgba, iter) and one fr_render_deep_de (rgba, iter, de, deriv; shade off), device time from the context's
event pair; median (min) of each and the ratio DE / plain of the medians.
usage: deep_de_time.py [out.txt]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fractalrenderer_amd as fr  # noqa: E402
import deep_bla_ref as BR  # noqa: E402
import deep_ref as R  # noqa: E402

REPS = 7
N = 4096


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    say(f"# fr_render_deep (rgba, iter) and fr_render_deep_de (rgba, iter, de, deriv; shade 0) interleaved, one GPU, one context; "
        f"median (min) of {REPS} renders each after a warm-up, device time from the context's event pair")
    with fr.Renderer(0) as r:
        r.set_option("timing", 1)
        rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
        it = torch.empty((N, N), dtype=torch.int32, device=dev)
        de = torch.empty((N, N), dtype=torch.float64, device=dev)
        deriv = torch.empty((N, N, 2), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        cases = [("default view", R.SHALLOW | {"max_iter": 1024}), ("view B (1e-100)", R.VIEW_B), ("view C (1e-50)", BR.VIEW_C)]
        for label, v in cases:
            view = fr.DeepView(v["cx"], v["cy"])
            st = fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"])
            for bla in (False, True):
                def plain():
                    r.render_deep(st, N, N, view, rgba=rgba, iter=it, bla=bla)
                    return r.last_kernel_ms()

                def dist():
                    r.render_deep_de(st, N, N, view, rgba=rgba, iter=it, de=de, deriv=deriv, bla=bla)
                    return r.last_kernel_ms()

                plain(); dist()                                   # warm-up: orbit, table, both occupancy queries
                ms = {"plain": [], "de": []}
                for _ in range(REPS):
                    ms["plain"].append(plain())
                    ms["de"].append(dist())
                mp, md = statistics.median(ms["plain"]), statistics.median(ms["de"])
                for key, name in (("plain", "fr_render_deep   "), ("de", "fr_render_deep_de")):
                    say(f"{label:16s} {N}^2 max_iter {v['max_iter']:5d} BLA {'on ' if bla else 'off'} {name} "
                        f"{statistics.median(ms[key]):9.3f} ms ({min(ms[key]):.3f})")
                say(f"{label:16s} BLA {'on ' if bla else 'off'} DE / plain = {md / mp:.3f}")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
