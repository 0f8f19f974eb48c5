#!/usr/bin/env python3
"""Device time of fr_render_deepx with and without FR_FLAG_DEEPX_BLA (profiles/deepx_bla_time.txt), on one context: view B
(1e-100), views D (1e-400) and E (1e-1000) of tests/golden/deepx_views.json, all at 4096^2.

Per view: median (min) kernel time of REPS renders after a warm-up, flag off then on; lane-updates executed (single steps
+ BLA steps, from fr_ctx_last_deepx_steps) next to the updates they represent (single steps + updates skipped); and the
table build on its own: stream time of renders that rebuild the table (the zoom string alternates between two values whose
53-bit mantissas differ, so dcmax changes and the orbit stays cached) less their kernel time.
usage: deepx_bla_time.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fractalrenderer_amd as fr  # noqa: E402
import deep_bla_ref as BR  # noqa: E402
import deep_ref as R  # noqa: E402
import deepx_ref as X  # noqa: E402

REPS = 7
N = 4096


def updates(it, max_iter):
    it = it.astype(np.int64)
    return int(np.where(it < max_iter, it + 1, max_iter).sum())


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    V = X.views()
    B = R.VIEW_B
    say(f"# fr_render_deepx, FR_FLAG_DEEPX_BLA off / on, one GPU, one context; median (min) of {REPS} renders after a warm-up, "
        f"device time from the context's event pair")
    say("# executed = lane-updates the kernel ran (off: every update; on: single + BLA steps); represented = updates the "
        "frame stands for")
    it = torch.empty((N, N), dtype=torch.int32, device=dev)
    rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
    cases = [("view B (1e-100)", dict(cx=B["cx"], cy=B["cy"], zoom=repr(B["zoom"]), max_iter=B["max_iter"]), "1.0000001e-100"),
             ("view D (1e-400)", V["D"], "1.0000001e-400"), ("view E (1e-1000)", V["E"], "1.0000001e-1000")]
    with fr.Renderer(0) as r:
        r.set_option("timing", 1)
        for label, v, zoom2 in cases:
            view = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"])
            st = fr.FractalState(max_iterations=v["max_iter"])
            res = {}
            for bla in (False, True):
                r.render_deep(st, N, N, view, rgba=rgba, iter=it, xbla=bla)          # warm-up: orbit, table
                torch.cuda.synchronize()
                ms = []
                for _ in range(REPS):
                    r.render_deep(st, N, N, view, rgba=rgba, iter=it, xbla=bla)
                    ms.append(r.last_kernel_ms())
                u = updates(it.cpu().numpy(), v["max_iter"])
                if bla:
                    s = r.last_deepx_steps()
                    execd, rep = s.plain + s.bla, s.plain + s.skipped
                    assert rep == u
                    extra = f"  single {s.plain / 1e9:.3f} G  BLA {s.bla / 1e9:.4f} G  skipped {s.skipped / 1e9:.3f} G"
                else:
                    execd, rep, extra = u, u, ""
                res[bla] = statistics.median(ms)
                say(f"{label:17s} {N}^2 max_iter {v['max_iter']:5d} BLA {'on ' if bla else 'off'} {statistics.median(ms):9.3f} ms "
                    f"({min(ms):.3f})  executed {execd / 1e9:8.3f} G  represented {rep / 1e9:8.3f} G  "
                    f"{rep / statistics.median(ms) / 1e6:8.1f} G updates/s{extra}")
            say(f"{label:17s} off / on = {res[False] / res[True]:.2f}x")
            # table build: renders that rebuild it (dcmax alternates), stream time less kernel time
            views = [view, fr.DeepView(v["cx"], v["cy"], zoom=zoom2, frac_bits=fr.deepx_frac_bits(v["zoom"]))]
            s0 = torch.cuda.Stream()
            tb = []
            for rep in range(REPS + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(s0)
                r.render_deep(st, N, N, views[rep % 2], rgba=rgba, iter=it, xbla=True, stream=s0.cuda_stream, sync=False)
                e1.record(s0)
                s0.synchronize()
                if rep:
                    tb.append(e0.elapsed_time(e1) - r.last_kernel_ms())
            n_ref = len(fr.deepx_reference_orbit(view, v["max_iter"])[1]) - 1
            say(f"{label:17s} table build (N = {n_ref}, K = {BR.levels(n_ref)}, {(n_ref - 1) - bin(n_ref - 1).count('1')} entries): "
                f"{statistics.median(tb):.3f} ms median ({min(tb):.3f}) -- stream time of a rebuilding render less its kernel")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
