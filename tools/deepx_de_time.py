#!/usr/bin/env python3
"""Device time of fr_render_deepx_de next to fr_render_deepx (profiles/deepx_de_time.txt), on one context: view D (1e-400),
view E (1e-1000) and view B (1e-100) as an extended view at 4096^2, each with FR_FLAG_DEEPX_BLA off and on; on view B also
fr_render_deep_de, whose D is a plain double2 -- what the always-extended D costs where fp64 would do.

Per view and flag the entry points are interleaved in one session: after a warm-up of each (orbit, table), REPS rounds of one
fr_render_deepx (rgba, iter) and one fr_render_deepx_de (rgba, iter, de, deriv; shade off), device time from the context's
event pair; median (min) of each and the ratio DE / plain of the medians.
usage: deepx_de_time.py [out.txt]"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fractalrenderer_amd as fr  # noqa: E402
import deep_ref as R  # noqa: E402
import deepx_ref as X  # noqa: E402

REPS = 7
N = 4096


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    V = X.views()
    say(f"# fr_render_deepx (rgba, iter) and fr_render_deepx_de (rgba, iter, de, deriv; shade 0) interleaved, one GPU, one context; "
        f"median (min) of {REPS} renders each after a warm-up, device time from the context's event pair")
    with fr.Renderer(0) as r:
        r.set_option("timing", 1)
        rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
        it = torch.empty((N, N), dtype=torch.int32, device=dev)
        de = torch.empty((N, N), dtype=torch.float64, device=dev)
        deriv = torch.empty((N, N, 2), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        cases = [("view D (1e-400)", V["D"], None), ("view E (1e-1000)", V["E"], None),
                 ("view B (1e-100)", dict(R.VIEW_B, zoom="1e-100"), R.VIEW_B)]
        for label, v, v64 in cases:
            view = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"])
            st = fr.FractalState(max_iterations=v["max_iter"])
            for bla in (False, True):
                def plain():
                    r.render_deep(st, N, N, view, rgba=rgba, iter=it, xbla=bla)
                    return r.last_kernel_ms()

                def dist():
                    r.render_deepx_de(st, N, N, view, rgba=rgba, iter=it, de=de, deriv=deriv, bla=bla)
                    return r.last_kernel_ms()

                def dist64():                                     # the fp64 entry point on the same view
                    r.render_deep_de(fr.FractalState(zoom=v64["zoom"], max_iterations=v64["max_iter"]), N, N,
                                     fr.DeepView(v64["cx"], v64["cy"]), rgba=rgba, iter=it, de=de, deriv=deriv, bla=bla)
                    return r.last_kernel_ms()

                runs = [("plain", "fr_render_deepx   ", plain), ("de", "fr_render_deepx_de", dist)]
                if v64 is not None:
                    runs.append(("de64", "fr_render_deep_de ", dist64))
                for _, _, f in runs:                              # warm-up: orbit, table, the occupancy queries
                    f()
                ms = {key: [] for key, _, _ in runs}
                for _ in range(REPS):
                    for key, _, f in runs:
                        ms[key].append(f())
                med = {key: statistics.median(t) for key, t in ms.items()}
                for key, name, _ in runs:
                    say(f"{label:17s} {N}^2 max_iter {v['max_iter']:5d} BLA {'on ' if bla else 'off'} {name} "
                        f"{med[key]:9.3f} ms ({min(ms[key]):.3f})")
                say(f"{label:17s} BLA {'on ' if bla else 'off'} DE / plain = {med['de'] / med['plain']:.3f}")
                if v64 is not None:
                    say(f"{label:17s} BLA {'on ' if bla else 'off'} fr_render_deepx_de / fr_render_deep_de = {med['de'] / med['de64']:.3f}")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
