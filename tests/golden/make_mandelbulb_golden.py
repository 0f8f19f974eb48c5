"""Generates tests/golden/mandelbulb_spv_frames.npz by executing the reference's compiled Mandelbulb shader.

    python tests/golden/make_mandelbulb_golden.py [case ...]

Reads /root/reference/FractalRenderer/shaders/mandelbulb.comp.spv at generation time (the binary is never copied), runs one
interpreter invocation per pixel (tests/golden/spirv_interp_ext.py: spirv_interp.py plus the opcodes this shader needs)
and stores:
  <case>/rgba    float32 (H, W, 4)  the texel the invocation wrote with OpImageWrite (post-chained, as the shader writes it)
  <case>/lin     float32 (H, W, 3)  the sample's colour as raymarch returned it (main's `color`; aa == 1 cases only)
  <case>/iter    int32   (H, W)     raymarch's step index i of a hit, -1 for a ray that hits nothing (aa == 1 cases only)
  <case>/t       float32 (H, W)     raymarch's t where the march stopped (aa == 1 cases only)
  __meta__       JSON: every case's parameters, frame size and packed push constants, the sha256 of the shader binary,
                 numpy version
Push constants are packed here from the case parameters in the order of ComputeEffect::update_from_state's Mandelbulb case
(src/compute_effect_manager.h:173-199); tests/test_mandelbulb_host.py pins the library's packing to the same floats.
The interpreter propagates NaN through clamp(); where the shader's colour is NaN the fixture holds NaN.
"""
import hashlib
import json
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]

from spirv_interp_ext import F32, Cell, Invocation, Module   # noqa: E402

SPV = "/root/reference/FractalRenderer/shaders/mandelbulb.comp.spv"
PROBES = ("raymarch:i", "raymarch:t", "raymarch:normal", "main:color")

# name -> (W, H, parameters); parameters default to the FractalState initialisers (src/fractal_state.h:24-33,68)
CASES = {
    "default": (48, 36, dict()),
    "front": (32, 24, dict(max_iterations=64)),
    "side": (32, 24, dict(max_iterations=64, rotation_y=1.5708)),
    "closeup": (32, 24, dict(max_iterations=64, camera_distance=1.5, rotation_y=0.785)),
    "power2": (32, 24, dict(max_iterations=32, mandelbulb_power=2.0, palette_mode=1)),
    "power4": (32, 24, dict(max_iterations=32, mandelbulb_power=4.0, palette_mode=2)),
    "power12": (32, 24, dict(max_iterations=32, mandelbulb_power=12.0, palette_mode=3)),
    "power16": (32, 24, dict(max_iterations=32, mandelbulb_power=16.0, palette_mode=4)),
    "time": (32, 24, dict(max_iterations=48, time=2.75, palette_mode=5, color_offset=0.3, color_scale=2.5)),
    "rotation_speed0": (32, 24, dict(max_iterations=48, rotation_speed=0.0, time=1.5)),
    "aa2": (20, 15, dict(max_iterations=32, aa=2)),
    "aa3": (16, 12, dict(max_iterations=24, aa=3, time=0.8)),
    "clamp_low": (24, 18, dict(max_iterations=1, fov=0.05, color_scale=0.01, palette_mode=-3)),
    "clamp_high": (16, 12, dict(max_iterations=5000, mandelbulb_power=40.0, fov=7.0, palette_mode=9)),
    "camera_inside": (24, 18, dict(max_iterations=24, camera_distance=0.05)),
    "post_floors": (24, 18, dict(max_iterations=32, color_brightness=0.02, color_saturation=-1.0, color_contrast=0.0)),
    "ragged": (37, 13, dict(max_iterations=40, rotation_y=0.4, time=0.3)),
    "tall": (12, 40, dict(max_iterations=40, fov=1.6)),
}

DEFAULTS = dict(camera_distance=3.0, rotation_y=0.0, fov=1.0, mandelbulb_power=8.0, rotation_speed=0.5, time=0.0,
                max_iterations=256, aa=1, palette_mode=0, color_offset=0.0, color_scale=1.0, color_brightness=1.0,
                color_saturation=1.0, color_contrast=1.0)


def params(name):
    W, H, kw = CASES[name]
    p = dict(DEFAULTS)
    p.update(kw)
    return W, H, p


def pack(p):
    """src/compute_effect_manager.h:173-199, every field static_cast<float>"""
    f = lambda v: float(np.float32(v))   # noqa: E731
    return [f(p["camera_distance"]), f(p["rotation_y"]), f(p["mandelbulb_power"]), f(p["max_iterations"]),
            f(p["color_offset"]), f(p["color_scale"]), 0.0, f(p["palette_mode"]),
            f(p["time"]), f(p["fov"]), f(p["aa"]), f(p["color_brightness"]),
            f(p["rotation_speed"]), f(p["color_saturation"]), f(p["color_contrast"]), 0.0,
            0.0, 0.0, 0.0, 0.0]


def run_case(name):
    W, H, p = params(name)
    m = Module(SPV)
    pc = pack(p)
    gid = m.global_named("gl_GlobalInvocationID")
    push = next(g for g, s in m.global_storage.items() if s == 9)
    image = next(g for g, s in m.global_storage.items() if s == 0)
    rgba = np.zeros((H, W, 4), np.float32)
    lin = np.zeros((H, W, 3), np.float32)
    it = np.full((H, W), -1, np.int32)
    tt = np.full((H, W), np.nan, np.float32)
    t0 = time.time()
    for y in range(H):
        for x in range(W):
            g = {gid: Cell([x, y, 0]), image: Cell(None),
                 push: Cell([[F32(v) for v in pc[4 * k:4 * k + 4]] for k in range(4)])}   # the shader declares data1-4
            inv = Invocation(m, g, (W, H), probe=PROBES).run()
            assert len(inv.stores) == 1 and inv.stores[0][1] == [x, y]
            rgba[y, x] = inv.stores[0][2]
            lin[y, x] = inv.probes["main:color"]
            if PROBES[2] in inv.probes:                  # the hit branch computed a normal
                it[y, x] = inv.probes[PROBES[0]]
            tt[y, x] = inv.probes[PROBES[1]]
    print("%-16s %3dx%-3d  %.1f s" % (name, W, H, time.time() - t0), flush=True)
    return name, rgba, lin, it, tt


def main(argv):
    names = argv or list(CASES)
    path = os.path.join(HERE, "mandelbulb_spv_frames.npz")
    out = dict(np.load(path)) if argv and os.path.exists(path) else {}
    jobs = int(os.environ.get("JOBS", "8"))
    with multiprocessing.Pool(jobs) as pool:
        for name, rgba, lin, it, tt in pool.imap_unordered(run_case, names):
            out[name + "/rgba"] = rgba
            if params(name)[2]["aa"] <= 1:
                out[name + "/lin"] = lin
                out[name + "/iter"] = it
                out[name + "/t"] = tt
    meta = json.loads(str(out["__meta__"])) if "__meta__" in out else {"cases": {}}
    for name in names:
        W, H, p = params(name)
        meta["cases"][name] = {"W": W, "H": H, "params": p, "push_constants": pack(p)}
    with open(SPV, "rb") as f:
        meta["sha256"] = {"mandelbulb.comp.spv": hashlib.sha256(f.read()).hexdigest()}
    meta["numpy"] = np.__version__
    out["__meta__"] = np.array(json.dumps(meta, sort_keys=True))
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
