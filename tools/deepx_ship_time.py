#!/usr/bin/env python3
"""Device time of fr_render_deepx_ship (profiles/deepx_ship_time.txt): the structured 1e-400 view and the tip view at 1e-1000
of tests/golden/deepx_ship_views.json at 4096^2, and in the same session the two rates it sits between -- fr_render_deep_ship
on its view B (1e-100) and fr_render_deepx on its view D (1e-400) -- then a Burning Ship sequence walk in both modes.

"timing" = 1; the time is fr_ctx_last_kernel_ms (the context's event pair), all three planes on the device.  Lane-updates of
the extended ship views are counted by the numpy restatement at 256 x 192 (extended + plain steps) and scaled by the pixel
ratio; those of the two neighbours from the iter plane, as their own tools count them.
usage: deepx_ship_time.py [out.txt]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fractalrenderer_amd as fr  # noqa: E402
import deep_ship_ref as S  # noqa: E402
import deepx_ref as X  # noqa: E402
import deepx_ship_ref as SX  # noqa: E402

REPS, WARM, N = 7, 2, 4096
CW, CH = 256, 192
SEQ_FIRST, SEQ_LAST, SEQ_FRAMES, SEQ_N = "1e-310", "6.25e-312", 41, 1024      # four octaves, ten frames per octave


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
    nu = torch.empty((N, N), dtype=torch.float64, device=dev)
    it = torch.empty((N, N), dtype=torch.int32, device=dev)
    V, XV = SX.views(), X.views()
    say(f"# fr_render_deepx_ship between fr_render_deep_ship and fr_render_deepx, one GPU ({torch.cuda.get_device_name(0)}), {N}^2, "
        f"aa 1, rgba + nu + iter on the device; median (min) of {REPS} renders after {WARM} warm-ups, device time from the "
        f"context's event pair (\"timing\" = 1); G lane-updates/s = updates / median")
    say("# command: python tools/deepx_ship_time.py profiles/deepx_ship_time.txt")

    def timed(r, call, max_iter):
        ms = []
        for k in range(WARM + REPS):
            call()
            if k >= WARM:
                ms.append(r.last_kernel_ms())
        torch.cuda.synchronize()
        i = it.cpu().numpy().astype(np.int64)
        return statistics.median(ms), min(ms), int(np.where(i < max_iter, i + 1, max_iter).sum()), float((i < max_iter).mean())

    with fr.Renderer(0) as r:
        r.set_option("timing", 1)
        v = S.SHIP_B
        st = fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"])
        med, lo, u, esc = timed(r, lambda: r.render_deep_ship(st, N, N, fr.DeepView(v["cx"], v["cy"]), rgba=rgba, nu=nu, iter=it),
                                v["max_iter"])
        say(f"{'ship B (1e-100)':18s} max_iter {v['max_iter']:5d} {'fr_render_deep_ship':21s} {med:9.3f} ms ({lo:.3f})  "
            f"{u / 1e9:8.3f} G updates  {u / med / 1e6:7.1f} G lane-updates/s  escaped {esc:.3f}  grid {r.last_grid() & 0xffff}")
        for label, name in (("ship S400 (1e-400)", "S400"), ("tip (1e-1000)", "TIP1000")):
            v = V[name]
            st = fr.FractalState(max_iterations=v["max_iter"])
            view = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"])
            med, lo, u_iter, esc = timed(r, lambda: r.render_deepx_ship(st, N, N, view, rgba=rgba, nu=nu, iter=it), v["max_iter"])
            t0 = time.perf_counter()
            stats = {}
            SX.restate_ship_x(v, CW, CH, stats=stats)
            u = (stats["ext_steps"] + stats["plain_steps"]) * (N * N) / (CW * CH)
            say(f"{label:18s} max_iter {v['max_iter']:5d} {'fr_render_deepx_ship':21s} {med:9.3f} ms ({lo:.3f})  "
                f"{u / 1e9:8.3f} G updates  {u / med / 1e6:7.1f} G lane-updates/s  escaped {esc:.3f}  grid {r.last_grid() & 0xffff}  "
                f"(restatement {CW}x{CH}: {stats['ext_steps'] / (stats['ext_steps'] + stats['plain_steps']):.3f} of the updates "
                f"extended, {stats['flipped_ext']} flipped extended steps, {time.perf_counter() - t0:.0f} s; from the {N}^2 iter "
                f"plane {u_iter / 1e9:.3f} G updates)")
            t0 = time.perf_counter()
            orbit = fr.deepx_ship_reference_orbit(view, v["max_iter"])
            say(f"{'':18s} host orbit: F = {fr.deepx_frac_bits(v['zoom'])}, {len(orbit[1]) - 1} updates, "
                f"{(time.perf_counter() - t0) * 1e3:.2f} ms")
        v = XV["D"]
        st = fr.FractalState(max_iterations=v["max_iter"])
        view = fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"])
        med, lo, u, esc = timed(r, lambda: r.render_deep(st, N, N, view, rgba=rgba, nu=nu, iter=it), v["max_iter"])
        say(f"{'view D (1e-400)':18s} max_iter {v['max_iter']:5d} {'fr_render_deepx':21s} {med:9.3f} ms ({lo:.3f})  "
            f"{u / 1e9:8.3f} G updates  {u / med / 1e6:7.1f} G lane-updates/s  escaped {esc:.3f}  grid {r.last_grid() & 0xffff}")

    # a ship sequence walk, both modes, a fresh context per walk (so every walk computes its orbit)
    v = V["S310"]
    st = fr.FractalState(max_iterations=v["max_iter"])
    out = torch.empty((SEQ_N, SEQ_N, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    say(f"# ship sequence: S310's centre {SEQ_FIRST} -> {SEQ_LAST} (four octaves), {SEQ_FRAMES} frames, {SEQ_N}^2, max_iter "
        f"{v['max_iter']}, rgba on the device")
    for rnd in range(2):
        for mode in (0, 1):
            with fr.Renderer(0) as r:
                r.set_option("timing", 1)
                with fr.DeepZoomSequence(r, st, v["cx"], v["cy"], SEQ_FIRST, SEQ_LAST, SEQ_FRAMES, SEQ_N, SEQ_N,
                                         keyframes=bool(mode), formula="ship") as s:
                    t0 = time.perf_counter()
                    dev_ms = 0.0
                    for f in range(SEQ_FRAMES):
                        s.render(f, rgba=out)
                        dev_ms += r.last_kernel_ms()
                    wall = time.perf_counter() - t0
                    say(f"mode {mode} walk, round {rnd}: wall {wall * 1e3:9.1f} ms  device {dev_ms:9.1f} ms  "
                        f"stats (exact, resampled, orbits) = {s.stats()}  F = {s.plan(0).frac_bits}")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
