#!/usr/bin/env python3
"""Deep zoom sequences (fr_deep_sequence) timed on one GPU (profiles/deep_sequence_time.txt).

The walk: view T110's centre (tests/golden/deepx_views.json) from "1e-110" down ten octaves, 30 frames per octave (301
frames), 1024^2, max_iter 905, device planes.
- the two modes: wall and device time of the whole walk in mode 0 (every frame exact) and mode 1 (octave keyframes +
  resampling), interleaved, each walk on a context of its own; the host time of the one orbit;
- the caller's loop: the same 301 zooms as decimal strings through fr_render_deepx with automatic frac_bits, the only way
  to render the walk without the sequence object;
- the resampling kernel alone at 1024^2 and 4096^2 (keyframes cached: the frame's event pair holds that one launch),
  next to a device-to-device copy of one rgba plane in the same run;
- quality: PSNR of mode 1 against mode 0 on the 8-bit export, over the 290 frames off the keyframe grid.
usage: deep_sequence_time.py [out.txt]"""
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fractalrenderer_amd as fr  # noqa: E402
import deepx_ref as X  # noqa: E402

FIRST, LAST, FRAMES, N, MAX_ITER = "1e-110", "9.765625e-114", 301, 1024, 905
ROUNDS = 2
REPS = 20


def pair_string(mant, exp2):
    """the exact decimal string of mant 2^exp2 (exp2 < 52)"""
    k = 52 - exp2
    return f"{int(mant * (1 << 52)) * 5 ** k}e-{k}"


def main(out_path):
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    v = X.views()["T110"]
    st = fr.FractalState(max_iterations=MAX_ITER)
    rgba = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def seq(r, mode, n=N, first=FIRST, last=LAST, frames=FRAMES, post=False):
        return fr.DeepZoomSequence(r, st, v["cx"], v["cy"], first, last, frames, n, n, keyframes=bool(mode), post_chain=post)

    say(f"# fr_deep_sequence: {v['cx'][:24]}... {FIRST} -> {LAST} (ten octaves), {FRAMES} frames, {N}^2, max_iter {MAX_ITER}, one GPU")
    say(f"# command: python tools/deep_sequence_time.py profiles/deep_sequence_time.txt   (GPU: {torch.cuda.get_device_name(0)})")

    # the two modes, interleaved, a fresh context per walk (so every walk computes its orbit)
    walks = {0: [], 1: []}
    for rnd in range(ROUNDS):
        for mode in (0, 1):
            with fr.Renderer(0) as r, seq(r, mode) as s:
                t0 = time.perf_counter()
                dev_ms = 0.0
                for f in range(FRAMES):
                    s.render(f, rgba=rgba)
                    dev_ms += r.last_kernel_ms()
                wall = time.perf_counter() - t0
                stats = s.stats()
                F = s.plan(0).frac_bits
            walks[mode].append((wall, dev_ms))
            say(f"mode {mode} walk, round {rnd}: wall {wall * 1e3:9.1f} ms  device {dev_ms:9.1f} ms  "
                f"stats (exact, resampled, orbits) = {stats}  F = {F}")
    best = {m: min(w for w, _ in walks[m]) for m in walks}
    bdev = {m: min(d for _, d in walks[m]) for m in walks}
    say(f"mode 1 / mode 0: wall {best[1] / best[0]:.3f}  device {bdev[1] / bdev[0]:.3f}   (best of {ROUNDS}; 11 of 301 frames "
        f"exact = {11 / 301:.3f})")
    t0 = time.perf_counter()
    orbit = fr.deepx_reference_orbit(fr.DeepView(v["cx"], v["cy"], frac_bits=F, zoom=FIRST), MAX_ITER)
    say(f"the one orbit on the host (F = {F}, {len(orbit[1]) - 1} updates): {(time.perf_counter() - t0) * 1e3:.2f} ms")

    # the caller's loop: the same zooms through fr_render_deepx, automatic frac_bits
    with fr.Renderer(0) as r, seq(r, 0) as s:
        plans = [s.plan(f) for f in range(FRAMES)]
    zooms = [pair_string(p.zoom_mant, p.zoom_exp2) for p in plans]
    assert all(fr.deepx_zoom(z) == (p.zoom_mant, p.zoom_exp2) for z, p in zip(zooms, plans))
    bits = [fr.deepx_frac_bits(z) for z in zooms]
    changes = 1 + sum(1 for a, b in zip(bits, bits[1:]) if a != b)
    loops = []
    for rnd in range(ROUNDS):
        with fr.Renderer(0) as r:
            t0 = time.perf_counter()
            dev_ms = 0.0
            for z in zooms:
                r.render_deep(st, N, N, fr.DeepView(v["cx"], v["cy"], zoom=z), rgba=rgba)
                dev_ms += r.last_kernel_ms()
            loops.append((time.perf_counter() - t0, dev_ms))
        say(f"fr_render_deepx loop, round {rnd}: wall {loops[-1][0] * 1e3:9.1f} ms  device {loops[-1][1]:9.1f} ms  "
            f"orbits {changes} (automatic F {min(bits)} .. {max(bits)})")
    lbest = min(w for w, _ in loops)
    say(f"mode 0 / fr_render_deepx loop: wall {best[0] / lbest:.3f}   mode 1 / fr_render_deepx loop: wall {best[1] / lbest:.3f}")

    # the resampling kernel alone, and a device-to-device copy of one rgba plane
    for n in (1024, 4096):
        out = torch.empty((n, n, 4), dtype=torch.float32, device=dev)
        dst = torch.empty_like(out)
        torch.cuda.synchronize()
        with fr.Renderer(0) as r, seq(r, 1, n, FIRST, "5e-111", 3) as s:
            assert s.plan(1).resampled
            s.render(1, rgba=out)                                     # the two keyframes
            ms = []
            for _ in range(REPS):
                s.render(1, rgba=out)
                ms.append(r.last_kernel_ms())
            assert s.stats()[:2] == (2, REPS + 1)
        cp = []
        for _ in range(REPS + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(out)
            e1.record()
            torch.cuda.synchronize()
            cp.append(e0.elapsed_time(e1))
        cp = cp[1:]
        px = n * n
        k, c = statistics.median(ms), statistics.median(cp)
        say(f"deep_resample_kernel {n}^2: {k:.4f} ms median ({min(ms):.4f} min) = {px * 16 / k / 1e6:.0f} GB/s of stores "
            f"({px * 32 / k / 1e6:.0f} GB/s with one read of each pixel's taps);  D2D copy of one rgba plane {c:.4f} ms "
            f"({min(cp):.4f}) = {px * 32 / c / 1e6:.0f} GB/s read + write;  kernel / copy = {k / c:.2f}")
        del out, dst

    # quality on the 8-bit export
    a = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
    b = torch.empty((N, N, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    psnr = []
    with fr.Renderer(0) as r, seq(r, 0, post=True) as s0, seq(r, 1, post=True) as s1:
        for f in range(FRAMES):
            if not s1.plan(f).resampled:
                continue
            s0.render(f, rgba=a)
            s1.render(f, rgba=b)
            pa = r.export_rgb8(a, N, N, through_half=True).to(torch.float32)
            pb = r.export_rgb8(b, N, N, through_half=True).to(torch.float32)
            mse = float(((pa - pb) ** 2).mean())
            psnr.append(math.inf if mse == 0.0 else 10.0 * math.log10(255.0 ** 2 / mse))
    finite = [x for x in psnr if x != math.inf]
    say(f"mode 1 against mode 0 on the 8-bit export, {len(psnr)} frames off the grid: PSNR worst {min(psnr):.2f} dB, mean "
        f"{statistics.fmean(finite):.2f} dB over the {len(finite)} frames that differ ({len(psnr) - len(finite)} frames are "
        f"identical byte for byte: with max_iter fixed the deepest octaves show little but interior)")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
