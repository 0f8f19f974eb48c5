#!/usr/bin/env python3
"""Device time of fr_render_deep with and without FR_FLAG_DEEP_BLA (profiles/deep_bla_time.txt), on one context: the
default view at 1024^2, view B (1e-100) and view C (1e-50, next to a minibrot) at 4096^2.

Per view: median (min) kernel time of REPS renders after a warm-up, flag off then on; lane-updates executed (plain steps
+ BLA steps, from fr_ctx_last_deep_steps) next to the updates they represent (plain steps + updates skipped); and the
table build on its own: stream time of renders that rebuild the table (the zoom alternates between two neighbouring
doubles, so dcmax changes and the orbit stays cached) less their kernel time.
usage: deep_bla_time.py [out.txt]"""
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

REPS = 7


def updates(it, max_iter):
    it = it.astype(np.int64)
    return int(np.where(it < max_iter, it + 1, max_iter).sum())


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    say(f"# fr_render_deep, FR_FLAG_DEEP_BLA off / on, one GPU, one context; median (min) of {REPS} renders after a warm-up, "
        f"device time from the context's event pair")
    say("# executed = lane-updates the kernel ran (off: every update; on: plain + BLA steps); represented = updates the "
        "frame stands for")
    with fr.Renderer(0) as r:
        r.set_option("timing", 1)
        cases = [("default view", R.SHALLOW | {"max_iter": 1024}, 1024), ("view B (1e-100)", R.VIEW_B, 4096),
                 ("view C (1e-50)", BR.VIEW_C, 4096)]
        for label, v, n in cases:
            view = fr.DeepView(v["cx"], v["cy"])
            it = torch.empty((n, n), dtype=torch.int32, device=dev)
            rgba = torch.empty((n, n, 4), dtype=torch.float32, device=dev)
            res = {}
            for bla in (False, True):
                st = fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"])
                r.render_deep(st, n, n, view, rgba=rgba, iter=it, bla=bla)          # warm-up: orbit, table
                torch.cuda.synchronize()
                ms = []
                for _ in range(REPS):
                    r.render_deep(st, n, n, view, rgba=rgba, iter=it, bla=bla)
                    ms.append(r.last_kernel_ms())
                u = updates(it.cpu().numpy(), v["max_iter"])
                if bla:
                    s = r.last_deep_steps()
                    execd, rep = s.plain + s.bla, s.plain + s.skipped
                    assert rep == u
                    extra = f"  plain {s.plain / 1e9:.3f} G  BLA {s.bla / 1e9:.4f} G  skipped {s.skipped / 1e9:.3f} G"
                else:
                    execd, rep, extra = u, u, ""
                res[bla] = statistics.median(ms)
                say(f"{label:16s} {n}^2 max_iter {v['max_iter']:5d} BLA {'on ' if bla else 'off'} {statistics.median(ms):9.3f} ms "
                    f"({min(ms):.3f})  executed {execd / 1e9:8.3f} G  represented {rep / 1e9:8.3f} G  "
                    f"{rep / statistics.median(ms) / 1e6:8.1f} G updates/s{extra}")
            say(f"{label:16s} off / on = {res[False] / res[True]:.2f}x")
            # table build: renders that rebuild it (dcmax alternates), stream time less kernel time
            zs = [v["zoom"], float(np.nextafter(v["zoom"], 1.0))]
            s0 = torch.cuda.Stream()
            tb = []
            for rep in range(REPS + 1):
                st = fr.FractalState(zoom=zs[rep % 2], max_iterations=v["max_iter"])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(s0)
                r.render_deep(st, n, n, view, rgba=rgba, iter=it, bla=True, stream=s0.cuda_stream, sync=False)
                e1.record(s0)
                s0.synchronize()
                if rep:
                    tb.append(e0.elapsed_time(e1) - r.last_kernel_ms())
            N = len(R.reference_orbit(v["cx"], v["cy"], v["zoom"], v["max_iter"])) - 1
            say(f"{label:16s} table build (N = {N}, K = {BR.levels(N)}, {(N - 1) - bin(N - 1).count('1')} entries): "
                f"{statistics.median(tb):.3f} ms median ({min(tb):.3f}) -- stream time of a rebuilding render less its kernel")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
