#!/usr/bin/env python3
"""Device time of fr_render_deepx_ship with and without FR_FLAG_DEEPX_SHIP_BLA (profiles/deepx_ship_bla_time.txt) at 4096^2, all
three planes on the device: S400 and S310 (the structured views the flag is for), TIP1000 (the tip of the needle: Y = 0 on
the whole orbit, no step ever qualifies -- the price of the flag where it cannot help) and the tests' 1e-100 ship view B as
an extended view (plain-mode lanes).

Every view is measured by a child process of its own under `timeout`, one context each; the first child that fails ends the
run.  Per view: WARM renders of each form first, then REPS rounds of one unflagged and one flagged render, alternating, so
both see the same clocks and neighbours; median (min, max) kernel time of each form (fr_ctx_last_kernel_ms, "timing" = 1);
lane-updates executed (single + BLA steps, from fr_ctx_last_deepx_ship_steps) next to the updates they represent (single
steps + updates skipped); the share of pixels whose iter equals the unflagged render's; and the table build on its own:
stream time of renders that rebuild the table (the zoom string alternates between two values whose 53-bit mantissas differ,
so dcmax changes and the orbit stays cached) less their kernel time.  The parent, which never opens the GPU, adds the step
counts of the numpy restatement at 128 x 96.
usage: deepx_ship_bla_time.py [out.txt]        (deepx_ship_bla_time.py --view NAME is the child)"""
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deep_ship_ref as S  # noqa: E402
import deepx_ship_ref as SX  # noqa: E402

REPS, WARM, N = 7, 2, 4096
CHILD_LIMIT = 240                        # seconds per view; S400 is about 5 s of device time
RESTATED = (("S400", 128, 96), ("S310", 128, 96), ("NUC546", 128, 96), ("TIPY300", 48, 36))


def cases():
    V = SX.views()
    b = SX.as_x_view(S.SHIP_B)
    return {"S400": ("ship S400 (1e-400)", V["S400"], "1.0000001e-400"),
            "S310": ("ship S310 (1e-310)", V["S310"], "1.0000001e-310"),
            "TIP1000": ("tip (1e-1000)", V["TIP1000"], "1.0000001e-1000"),
            "B": ("ship B (1e-100)", b, "1.0000001e-100")}


def updates(it, max_iter):
    it = it.astype(np.int64)
    return int(np.where(it < max_iter, it + 1, max_iter).sum())


def child(name):
    import torch

    import fractalrenderer_amd as fr

    label, v, zoom2 = cases()[name]
    dev = torch.device("cuda:0")
    rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
    nu = torch.empty((N, N), dtype=torch.float64, device=dev)
    it = torch.empty((N, N), dtype=torch.int32, device=dev)

    def say(s):
        print(s, flush=True)

    with fr.Renderer(0) as r:
        r.set_option("timing", 1)
        view = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"])
        st = fr.FractalState(max_iterations=v["max_iter"])
        for _ in range(WARM):
            for bla in (False, True):
                r.render_deepx_ship(st, N, N, view, rgba=rgba, nu=nu, iter=it, bla=bla)
        ms = {False: [], True: []}
        its = {}
        for k in range(REPS):
            for bla in (False, True):
                r.render_deepx_ship(st, N, N, view, rgba=rgba, nu=nu, iter=it, bla=bla)
                ms[bla].append(r.last_kernel_ms())
                if k == REPS - 1:
                    torch.cuda.synchronize()
                    its[bla] = it.cpu().numpy()
        s = r.last_deepx_ship_steps()
        for bla in (False, True):
            u = updates(its[bla], v["max_iter"])
            if bla:
                execd, rep = s.plain + s.bla, s.plain + s.skipped
                assert rep == u
                extra = f"  single {s.plain / 1e9:.3f} G  BLA {s.bla / 1e9:.4f} G  skipped {s.skipped / 1e9:.3f} G"
            else:
                execd, rep, extra = u, u, ""
            med = statistics.median(ms[bla])
            say(f"{label:18s} {N}^2 max_iter {v['max_iter']:5d} BLA {'on ' if bla else 'off'} {med:9.3f} ms "
                f"({min(ms[bla]):.3f}, {max(ms[bla]):.3f})  executed {execd / 1e9:8.3f} G  represented {rep / 1e9:8.3f} G  "
                f"{rep / med / 1e6:8.1f} G updates/s  {execd / med / 1e6:8.1f} G trips/s{extra}")
        say(f"{label:18s} off / on = {statistics.median(ms[False]) / statistics.median(ms[True]):.2f}x   "
            f"trips off / on = {updates(its[False], v['max_iter']) / (s.plain + s.bla):.2f}x   "
            f"iter equal to the unflagged render's on {float((its[True] == its[False]).mean()):.6f} of the pixels   "
            f"grid {r.last_grid() & 0xffff}")
        # table build: renders that rebuild it (dcmax alternates), stream time less kernel time
        views = [view, fr.DeepView(v["cx"], v["cy"], zoom=zoom2, frac_bits=fr.deepx_frac_bits(v["zoom"]))]
        s0 = torch.cuda.Stream()
        tb = []
        for rep in range(REPS + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(s0)
            r.render_deepx_ship(st, N, N, views[rep % 2], rgba=rgba, nu=nu, iter=it, bla=True, stream=s0.cuda_stream, sync=False)
            e1.record(s0)
            s0.synchronize()
            if rep:
                tb.append(e0.elapsed_time(e1) - r.last_kernel_ms())
        n_ref = len(fr.deepx_ship_reference_orbit(view, v["max_iter"])[1]) - 1
        say(f"{label:18s} table build (N = {n_ref}, K = {(n_ref - 1).bit_length() - 1}, "
            f"{(n_ref - 1) - bin(n_ref - 1).count('1')} entries of 80 bytes): {statistics.median(tb):.3f} ms median "
            f"({min(tb):.3f}) -- stream time of a rebuilding render less its kernel")


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# fr_render_deepx_ship, FR_FLAG_DEEPX_SHIP_BLA off / on, one GPU, one context per view, {N}^2, aa 1, rgba + nu + iter on "
        f"the device; {WARM} warm-ups of each form, then {REPS} rounds of off, on alternating; median (min, max), device time "
        f"from the context's event pair (\"timing\" = 1)")
    say("# executed = lane-updates the kernel ran (off: every update; on: single + BLA steps); represented = updates the "
        "frame stands for")
    failed = False
    for name in cases():
        p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--view", name],
                           capture_output=True, text=True)
        for line in p.stdout.splitlines():
            say(line)
        if p.returncode != 0:                                      # nothing more is started on the GPU after a failure
            say(f"# {name}: the child ended with status {p.returncode}; the run stops here")
            sys.stderr.write(p.stderr[-3000:])
            failed = True
            break
    if not failed:
        import deepx_ship_bla_ref as XB
        say("# the restatement's step counts (tests/deepx_ship_bla_ref.py, aa 1): single steps / BLA steps / updates skipped, "
            "and the iter values equal to the unflagged restatement's")
        V = SX.views()
        for name, w, h in RESTATED:
            orbit = SX.orbit_of(V[name])
            samples, c = XB.restate_ship_x_bla(V[name], w, h, orbit=orbit)
            plain = SX.restate_ship_x(V[name], w, h, orbit=orbit)
            eq = int((samples[0][0] == plain[0][0]).sum())
            say(f"# {name:8s} {w:3d} x {h:<3d} N {len(orbit[1]) - 1:5d}  {c[0]:9d} / {c[1]:7d} / {c[2]:10d}   "
                f"{c[2] / (c[0] + c[2]):.4f} of the updates skipped, {(c[0] + c[2]) / (c[0] + c[1]):6.2f}x fewer trips, "
                f"iter equal on {eq} of {w * h}")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--view":
        child(sys.argv[2])
    else:
        sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else None))
