"""Generates tests/golden/phoenix_spv_frames.npz by executing the reference's compiled Phoenix shader.

    python tests/golden/make_phoenix_golden.py [case ...]

Reads /root/reference/FractalRenderer/shaders/phoenix.comp.spv at generation time (the binary is never copied), runs one
interpreter invocation per pixel (tests/golden/spirv_interp.py, as make_spv_golden.py does) and stores:
  <case>/rgba    float32 (H, W, 4)  the texel the invocation wrote with OpImageWrite (post-chained, as the shader writes it)
  <case>/iter    int32   (H, W)     phoenix_iter's loop index i (aa == 1 cases only)
  <case>/smooth  float32 (H, W)     sample_phoenix's smooth_iter (aa == 1 cases only)
  __meta__       JSON: every case's parameters and frame size, the sha256 of the shader binary, numpy version
Push constants are packed here from the case parameters in the order of ComputeEffect::update_from_state's Phoenix case
(src/compute_effect_manager.h:201-224); tests/test_phoenix_host.py pins the library's packing to the same layout.
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

from spirv_interp import F32, Cell, Invocation, Module   # noqa: E402

SPV = "/root/reference/FractalRenderer/shaders/phoenix.comp.spv"
PROBES = ("phoenix_iter:i", "sample_phoenix:smooth_iter")
JC = (float(np.float32(-0.7)), float(np.float32(0.27015)))

# name -> (W, H, parameters); parameters default to the FractalState initialisers (src/fractal_state.h)
CASES = {
    "classic": (64, 48, dict(max_iterations=128)),
    "swirl": (48, 36, dict(max_iterations=96, phoenix_p=0.2, phoenix_r=-0.3)),
    "tendrils": (48, 36, dict(max_iterations=96, phoenix_p=-0.1, phoenix_r=-0.8)),
    "chaos": (48, 36, dict(max_iterations=96, phoenix_p=0.3, phoenix_r=-0.6)),
    "stripes_below": (40, 30, dict(max_iterations=96, stripe_density=0.005)),
    "stripes_off": (40, 30, dict(max_iterations=96, stripe_density=0.0)),
    "stripes_dense": (40, 30, dict(max_iterations=96, stripe_density=17.5, center_x=-0.2, zoom=1.5)),
    "julia_mode": (24, 16, dict(max_iterations=64, use_julia_set=1, julia_c_real=0.25, julia_c_imag=0.1)),
    "julia_mode_escapes": (16, 12, dict(max_iterations=64, use_julia_set=1, julia_c_real=0.6, julia_c_imag=0.55)),
    "aa2": (24, 16, dict(max_iterations=64, aa=2)),
    "aa3": (16, 12, dict(max_iterations=48, aa=3, phoenix_p=0.2, phoenix_r=-0.3)),
    "palette3": (32, 24, dict(max_iterations=64, palette_mode=3)),
    "zoomed_out": (48, 32, dict(max_iterations=64, zoom=14.0)),
    "max_iter1": (40, 30, dict(max_iterations=1, zoom=6.0)),
    "max_iter2": (40, 30, dict(max_iterations=2, zoom=6.0)),
    "ragged": (70, 21, dict(max_iterations=80, center_x=-0.3, center_y=0.2, zoom=2.2)),
    "tall": (20, 52, dict(max_iterations=80)),
    "interior": (40, 30, dict(max_iterations=128, center_x=0.0, center_y=0.0, zoom=0.6)),
    "post": (32, 24, dict(max_iterations=64, color_brightness=1.2, color_saturation=0.8, color_contrast=1.1)),
    "post_floors": (32, 24, dict(max_iterations=64, color_brightness=0.02, color_saturation=-1.0, color_contrast=0.0)),
    # one full block of 16 updates (two) and a tail of one: escapes at i = 16 (7 samples) and at i = 32 (4 samples; the
    # centre of tail_17 has only 2 of them at this size, so tail_33 sits 1.1 pixels left and half a pixel up)
    "tail_17": (24, 16, dict(max_iterations=17, center_x=-0.45, center_y=0.55, zoom=0.4)),
    "tail_33": (24, 16, dict(max_iterations=33, center_x=-0.4775, center_y=0.5375, zoom=0.4)),
}

DEFAULTS = dict(center_x=-0.5, center_y=0.0, zoom=3.0, max_iterations=256, julia_c_real=JC[0], julia_c_imag=JC[1],
                phoenix_p=0.0, phoenix_r=-0.5, use_julia_set=0, aa=1, color_scale=1.0, color_brightness=1.0,
                color_saturation=1.0, color_contrast=1.0, palette_mode=0, stripe_density=10.0)


def params(name):
    W, H, kw = CASES[name]
    p = dict(DEFAULTS)
    p.update(kw)
    return W, H, p


def pack(p):
    """src/compute_effect_manager.h:201-224, every field static_cast<float>"""
    f = lambda v: float(np.float32(v))   # noqa: E731
    return [f(p["center_x"]), f(p["center_y"]), f(p["zoom"]), f(p["max_iterations"]),
            f(p["julia_c_real"]), f(p["julia_c_imag"]), f(p["phoenix_p"]), f(p["phoenix_r"]),
            f(p["aa"]), f(p["color_scale"]), f(p["color_brightness"]), f(p["color_saturation"]),
            f(p["color_contrast"]), f(p["palette_mode"]), f(p["stripe_density"]), 1.0 if p["use_julia_set"] else 0.0,
            0.0, 0.0, 0.0, 0.0]


def run_case(name):
    W, H, p = params(name)
    m = Module(SPV)
    pc = pack(p)
    gid = m.global_named("gl_GlobalInvocationID")
    push = next(g for g, s in m.global_storage.items() if s == 9)
    image = next(g for g, s in m.global_storage.items() if s == 0)
    rgba = np.zeros((H, W, 4), np.float32)
    it = np.full((H, W), -1, np.int32)
    sm = np.full((H, W), np.nan, np.float32)
    t = time.time()
    for y in range(H):
        for x in range(W):
            g = {gid: Cell([x, y, 0]), image: Cell(None),
                 push: Cell([[F32(v) for v in pc[4 * k:4 * k + 4]] for k in range(5)])}
            inv = Invocation(m, g, (W, H), probe=PROBES).run()
            assert len(inv.stores) == 1 and inv.stores[0][1] == [x, y]
            rgba[y, x] = inv.stores[0][2]
            it[y, x] = inv.probes.get(PROBES[0], -1)
            sm[y, x] = inv.probes.get(PROBES[1], np.nan)
    print("%-20s %3dx%-3d  %.1f s" % (name, W, H, time.time() - t), flush=True)
    return name, rgba, it, sm


def main(argv):
    names = argv or list(CASES)
    path = os.path.join(HERE, "phoenix_spv_frames.npz")
    out = dict(np.load(path)) if argv and os.path.exists(path) else {}
    jobs = int(os.environ.get("JOBS", "8"))
    with multiprocessing.Pool(jobs) as pool:
        for name, rgba, it, sm in pool.imap_unordered(run_case, names):
            out[name + "/rgba"] = rgba
            if params(name)[2]["aa"] <= 1:
                out[name + "/iter"] = it
                out[name + "/smooth"] = sm
    meta = json.loads(str(out["__meta__"])) if "__meta__" in out else {"cases": {}}
    for name in names:
        W, H, p = params(name)
        meta["cases"][name] = {"W": W, "H": H, "params": p}
    with open(SPV, "rb") as f:
        meta["sha256"] = {"phoenix.comp.spv": hashlib.sha256(f.read()).hexdigest()}
    meta["numpy"] = np.__version__
    out["__meta__"] = np.array(json.dumps(meta, sort_keys=True))
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
