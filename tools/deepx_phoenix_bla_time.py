#!/usr/bin/env python3
"""Device time of fr_render_deepx_phoenix with and without FR_FLAG_DEEPX_PHOENIX_BLA (profiles/deepx_phoenix_bla_time.txt), on one
context: the tests' PX310 (1e-310), PX400A and PX400B (1e-400), TIP1000 and NUC201X (1e-1000) views, and PA (1e-100) passed as an
extended view, where the lanes run in the plain mode, at 4096^2, all three planes on the device.

Per view: WARM renders of each form first, then REPS rounds of one unflagged and one flagged render, alternating, so both
see the same clocks and neighbours; median (min, max) kernel time of each form (fr_ctx_last_kernel_ms, "timing" = 1);
lane-updates executed (single + BLA steps, from fr_ctx_last_deepx_phoenix_steps) next to the updates they represent (single
steps + updates skipped); the share of pixels whose iter equals the unflagged render's; and the table build on its own: stream
time of renders that rebuild the table (the zoom alternates between two strings 1e-15 apart at pinned fraction bits, so dcmax
changes and the orbit stays cached) less their kernel time.  The unflagged render is the yardstick: deep_phoenix_x_kernel.
The last case is the shallow view as an extended one, where no lane passes the pre-filter and the flag can only cost.
usage: deepx_phoenix_bla_time.py [out.txt [view ...]]   (views by name: a subset of the cases)"""
import os
import statistics
import sys
from decimal import Decimal

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fractalrenderer_amd as fr  # noqa: E402
import deepx_phoenix_bla_ref as XB  # noqa: E402
import deepx_phoenix_ref as PX  # noqa: E402

REPS, WARM, N = 7, 2, 4096


def updates(it, max_iter):
    it = it.astype(np.int64)
    return int(np.where(it < max_iter, it + 1, max_iter).sum())


def main(out_path, only=()):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
    nu = torch.empty((N, N), dtype=torch.float64, device=dev)
    it = torch.empty((N, N), dtype=torch.int32, device=dev)
    say(f"# fr_render_deepx_phoenix, FR_FLAG_DEEPX_PHOENIX_BLA off / on, one GPU, one context, {N}^2, aa 1, rgba + nu + iter on the "
        f"device; {WARM} warm-ups of each form, then {REPS} rounds of off, on alternating; median (min, max), device time from the "
        f"context's event pair (\"timing\" = 1)")
    say("# executed = lane-updates the kernel ran (off: every update; on: single + BLA steps); represented = updates the "
        "frame stands for")
    cases = [(k, XB.VIEWS[k]) for k in ("PX310", "PX400A", "PX400B", "TIP1000", "NUC201X")]
    cases += [(k + " as extended", PX.OLD_VIEWS[k]) for k in ("PA", "shallowA")]
    if only:
        cases = [c for c in cases if c[0].split()[0] in only]
    with fr.Renderer(0) as r:
        r.set_option("timing", 1)
        for name, v in cases:
            label = f"{name} ({v['zoom']})"
            bits = PX.frac_bits_of(v)
            view = fr.DeepView(v["cx"], v["cy"], bits, zoom=v["zoom"])
            ph = fr.PhoenixParams(phoenix_p=v["p"], phoenix_r=v["r"])
            st = fr.FractalState(max_iterations=v["max_iter"])
            for _ in range(WARM):
                for bla in (False, True):
                    r.render_deepx_phoenix(st, N, N, view, ph, rgba=rgba, nu=nu, iter=it, xbla=bla)
            ms = {False: [], True: []}
            its = {}
            for k in range(REPS):
                for bla in (False, True):
                    r.render_deepx_phoenix(st, N, N, view, ph, rgba=rgba, nu=nu, iter=it, xbla=bla)
                    ms[bla].append(r.last_kernel_ms())
                    if k == REPS - 1:
                        torch.cuda.synchronize()
                        its[bla] = it.cpu().numpy()
            s = r.last_deepx_phoenix_steps()
            for bla in (False, True):
                u = updates(its[bla], v["max_iter"])
                if bla:
                    execd, rep = s.plain + s.bla, s.plain + s.skipped
                    extra = f"  single {s.plain / 1e9:.3f} G  BLA {s.bla / 1e9:.4f} G  skipped {s.skipped / 1e9:.3f} G"
                    if rep != u:
                        extra += f"  (updates of its own iter plane: {u / 1e9:.3f} G)"
                else:
                    execd, rep, extra = u, u, ""
                med = statistics.median(ms[bla])
                say(f"{label:24s} {N}^2 max_iter {v['max_iter']:5d} BLA {'on ' if bla else 'off'} {med:9.3f} ms "
                    f"({min(ms[bla]):.3f}, {max(ms[bla]):.3f})  executed {execd / 1e9:8.3f} G  represented {rep / 1e9:8.3f} G  "
                    f"{rep / med / 1e6:8.1f} G updates/s  {execd / med / 1e6:8.1f} G trips/s{extra}")
            say(f"{label:24s} off / on = {statistics.median(ms[False]) / statistics.median(ms[True]):.2f}x   "
                f"trips off / on = {updates(its[False], v['max_iter']) / (s.plain + s.bla):.2f}x   "
                f"iter equal to the unflagged render's on {float((its[True] == its[False]).mean()):.6f} of the pixels   "
                f"grid {r.last_grid() & 0xffff}")
            # table build: renders that rebuild it (dcmax alternates), stream time less kernel time
            zs = [v["zoom"], format(Decimal(v["zoom"]) * Decimal("1.000000000000001"), "e")]
            s0 = torch.cuda.Stream()
            tb = []
            for rep in range(REPS + 1):
                vz = fr.DeepView(v["cx"], v["cy"], bits, zoom=zs[rep % 2])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(s0)
                r.render_deepx_phoenix(st, N, N, vz, ph, rgba=rgba, nu=nu, iter=it, xbla=True, stream=s0.cuda_stream, sync=False)
                e1.record(s0)
                s0.synchronize()
                if rep:
                    tb.append(e0.elapsed_time(e1) - r.last_kernel_ms())
            n_ref = len(PX.orbit_of(v)[1]) - 1
            say(f"{label:24s} table build (N = {n_ref}, K = {(n_ref - 1).bit_length() - 1}, "
                f"{(n_ref - 1) - bin(n_ref - 1).count('1')} entries of 112 bytes): {statistics.median(tb):.3f} ms median "
                f"({min(tb):.3f}) -- stream time of a rebuilding render less its kernel")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None, tuple(sys.argv[2:]))
