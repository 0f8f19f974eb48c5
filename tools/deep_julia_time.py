#!/usr/bin/env python3
"""Device time of fr_render_deep_julia and fr_render_deepx_julia (profiles/deep_julia_time.txt): RABBIT30, DENDRITE100 and the
1e-400 dendrite of tests/deep_julia_ref.py at 4096^2, interleaved in one session with their Mandelbrot counterparts --
fr_render_deep on its view B (1e-100) and fr_render_deepx on its view D (1e-400).

"timing" = 1; the time is fr_ctx_last_kernel_ms (the context's event pair), all three planes on the device.  Lane-updates =
the sum of min(iter + 1, max_iter) over the frame's iter plane.  One round renders every case once, in turn; the medians are
over the rounds after the warm-up rounds.
usage: deep_julia_time.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fractalrenderer_amd as fr  # noqa: E402
import deep_julia_ref as J  # noqa: E402
import deep_ref as R  # noqa: E402
import deepx_ref as X  # noqa: E402

REPS, WARM, N = 7, 2, 4096


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
    nu = torch.empty((N, N), dtype=torch.float64, device=dev)
    it = torch.empty((N, N), dtype=torch.int32, device=dev)
    planes = dict(rgba=rgba, nu=nu, iter=it)
    say(f"# fr_render_deep_julia / fr_render_deepx_julia next to fr_render_deep / fr_render_deepx, one GPU "
        f"({torch.cuda.get_device_name(0)}), {N}^2, aa 1, rgba + nu + iter on the device; the cases interleaved (one render of "
        f"each per round), median (min) of {REPS} rounds after {WARM} warm-up rounds, device time from the context's event pair "
        f"(\"timing\" = 1); lane-updates = sum of min(iter + 1, max_iter); G lane-updates/s = updates / median")
    say("# command: python tools/deep_julia_time.py profiles/deep_julia_time.txt")

    def julia(v, extended):
        st = fr.FractalState(zoom=v["zoom"] or 1.0, max_iterations=v["max_iter"], julia_c_real=v["c"][0], julia_c_imag=v["c"][1])
        view = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom_s"] if extended else None)
        return lambda r: r.render_deep_julia(st, N, N, view, **planes)

    def mandel(v, extended):
        st = fr.FractalState(zoom=1.0 if extended else v["zoom"], max_iterations=v["max_iter"])
        view = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"] if extended else None)
        return lambda r: r.render_deep(st, N, N, view, **planes)

    vb, vd = R.VIEW_B, X.views()["D"]
    cases = [
        ("julia RABBIT30 (1e-30)", "fr_render_deep_julia", J.view("RABBIT30")["max_iter"], julia(J.view("RABBIT30"), False)),
        ("julia DENDRITE100 (1e-100)", "fr_render_deep_julia", J.view("DENDRITE100")["max_iter"], julia(J.view("DENDRITE100"), False)),
        ("mandelbrot view B (1e-100)", "fr_render_deep", vb["max_iter"], mandel(vb, False)),
        ("julia DENDRITE400 (1e-400)", "fr_render_deepx_julia", J.view("DENDRITE400")["max_iter"], julia(J.view("DENDRITE400"), True)),
        ("mandelbrot view D (1e-400)", "fr_render_deepx", vd["max_iter"], mandel(vd, True)),
    ]
    ms = [[] for _ in cases]
    upd = [None] * len(cases)
    with fr.Renderer(0) as r:
        r.set_option("timing", 1)
        for k in range(WARM + REPS):
            for c, (_, _, max_iter, call) in enumerate(cases):
                call(r)
                if k >= WARM:
                    ms[c].append(r.last_kernel_ms())
                if k == 0:
                    torch.cuda.synchronize()
                    i = it.cpu().numpy().astype(np.int64)
                    upd[c] = (int(np.minimum(i + 1, max_iter).sum()), float((i < max_iter).mean()), r.last_grid() & 0xffff)
    rate = {}
    for c, (label, entry, max_iter, _) in enumerate(cases):
        med, lo = statistics.median(ms[c]), min(ms[c])
        u, esc, grid = upd[c]
        rate[label] = u / med / 1e6
        say(f"{label:28s} max_iter {max_iter:5d} {entry:22s} {med:9.3f} ms ({lo:.3f})  {u / 1e9:8.3f} G updates  "
            f"{rate[label]:7.1f} G lane-updates/s  escaped {esc:.3f}  grid {grid}")
    b, d = rate["mandelbrot view B (1e-100)"], rate["mandelbrot view D (1e-400)"]
    say(f"# rate against the Mandelbrot counterpart of the session: RABBIT30 {rate['julia RABBIT30 (1e-30)'] / b:.3f}, "
        f"DENDRITE100 {rate['julia DENDRITE100 (1e-100)'] / b:.3f} of fr_render_deep on view B; "
        f"DENDRITE400 {rate['julia DENDRITE400 (1e-400)'] / d:.3f} of fr_render_deepx on view D")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
