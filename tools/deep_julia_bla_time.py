#!/usr/bin/env python3
"""Device time of fr_render_deep_julia / fr_render_deepx_julia with and without their BLA flags
(profiles/deep_julia_bla_time.txt): RABBIT30, DENDRITE100 and PRECRIT60 through fr_render_deep_julia, DENDRITE400 and PRECRIT60
through fr_render_deepx_julia, and a c = 0 view where no probe passes (the price of the probe), at 4096^2.

"timing" = 1; the time is fr_ctx_last_kernel_ms (the context's event pair), all three planes on the device.  One round renders
every case once, unflagged then flagged, in turn; the medians are over the rounds after the warm-up rounds.  The tables are keyed
by the orbits alone, so only a view's first flagged render builds them; that render's time is printed apart.
FR_TREE in the environment names another tree to import the package from;
--unflagged-only: the unflagged renders alone, for a tree without the flags (the parent commit's times).
usage: deep_julia_bla_time.py [--unflagged-only] [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.environ.get("FR_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "tests"))
import fractalrenderer_amd as fr  # noqa: E402
import deep_julia_bla_ref as JB  # noqa: E402

REPS, WARM, N = 7, 2, 4096
C0 = dict(name="C0", c=(0.0, 0.0), cx="0.5", cy="0.25", zoom=1e-30, zoom_s="1e-30", max_iter=1000)


def main(out_path, unflagged_only):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
    nu = torch.empty((N, N), dtype=torch.float64, device=dev)
    it = torch.empty((N, N), dtype=torch.int32, device=dev)
    planes = dict(rgba=rgba, nu=nu, iter=it)
    say(f"# fr_render_deep_julia / fr_render_deepx_julia {'without' if unflagged_only else 'with and without'} their BLA flags, one "
        f"GPU ({torch.cuda.get_device_name(0)}), {N}^2, aa 1, rgba + nu + iter on the device; the cases interleaved (one render of "
        f"each per round), median (min) of {REPS} rounds after {WARM} warm-up rounds, device time from the context's event pair "
        f"(\"timing\" = 1)")
    say("# command: python tools/deep_julia_bla_time.py" + (" --unflagged-only" if unflagged_only else "") +
        " profiles/deep_julia_bla_time.txt")

    def call(v, extended, bla):
        st = fr.FractalState(zoom=2.5 if extended else v["zoom"], max_iterations=v["max_iter"], julia_c_real=v["c"][0],
                             julia_c_imag=v["c"][1])
        view = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom_s"] if extended else None)
        kw = dict(bla=True) if bla else {}
        return lambda r: r.render_deep_julia(st, N, N, view, **planes, **kw)

    views = [(JB.view("RABBIT30"), False), (JB.view("DENDRITE100"), False), (JB.view("PRECRIT60"), False),
             (JB.view("DENDRITE400"), True), (JB.view("PRECRIT60"), True), (C0, False), (C0, True)]
    cases = []
    for v, extended in views:
        for bla in ((False,) if unflagged_only else (False, True)):
            cases.append((v, extended, bla, call(v, extended, bla)))
    ms = [[] for _ in cases]
    first = [None] * len(cases)
    steps = [None] * len(cases)
    iters = [None] * len(cases)
    with fr.Renderer(0) as r:
        r.set_option("timing", 1)
        for k in range(WARM + REPS):
            for c, (v, extended, bla, fn) in enumerate(cases):
                fn(r)
                if k == 0:
                    first[c] = r.last_kernel_ms()
                    torch.cuda.synchronize()
                    iters[c] = it.cpu().numpy().copy()
                    if bla:
                        steps[c] = tuple(r.last_deepx_julia_steps() if extended else r.last_deep_julia_steps())
                if k >= WARM:
                    ms[c].append(r.last_kernel_ms())
    med = [statistics.median(m) for m in ms]
    for c, (v, extended, bla, _) in enumerate(cases):
        entry = "fr_render_deepx_julia" if extended else "fr_render_deep_julia"
        upd = int(np.minimum(iters[c].astype(np.int64) + 1, v["max_iter"]).sum())
        s = f"{v['name']:12s} max_iter {v['max_iter']:5d} {entry:22s} {'BLA ' if bla else 'plain'} {med[c]:9.3f} ms ({min(ms[c]):.3f})"
        if bla:
            single, nbla, skipped = steps[c]
            equal = float((iters[c] == iters[c - 1]).mean())
            s += (f"  {med[c - 1] / med[c]:6.2f}x of plain  skipped {skipped / (single + skipped):.4f} of {upd / 1e9:.3f} G updates  "
                  f"BLA steps {nbla / 1e6:.2f} M  equal iter {equal:.6f}  first flagged render {first[c]:.3f} ms")
        else:
            s += f"  {upd / 1e9:8.3f} G updates  {upd / med[c] / 1e6:7.1f} G lane-updates/s"
        say(s)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--unflagged-only"]
    main(args[0] if args else None, "--unflagged-only" in sys.argv[1:])
