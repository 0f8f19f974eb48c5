"""Mandelbulb (fr_render_mandelbulb): the parts that need no GPU -- ABI layout, defaults, push-constant packing, validation,
the numpy restatement against the executed shader, the interpreter extension, and the kernel's register budget."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mandelbulb_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "mandelbulb_spv_frames.npz")
SPV_SHA256 = "mandelbulb.comp.spv"


@pytest.fixture(scope="module")
def mbx():
    """the executed-shader fixture: {name: (W, H, params, push_constants, rgba, lin | None, iter | None, t | None)}"""
    z = np.load(FIXTURE)
    meta = json.loads(str(z["__meta__"]))
    out = {}
    for name, c in meta["cases"].items():
        g = lambda k: z[name + "/" + k] if name + "/" + k in z else None   # noqa: E731
        out[name] = (c["W"], c["H"], c["params"], c["push_constants"], z[name + "/rgba"], g("lin"), g("iter"), g("t"))
    return out


def params_of(fr, p):
    """(FractalState, MandelbulbParams) of a fixture case"""
    st = fr.FractalState(max_iterations=p["max_iterations"], antialiasing_samples=p["aa"], palette_mode=p["palette_mode"],
                         color_offset=p["color_offset"], color_scale=p["color_scale"],
                         color_brightness=p["color_brightness"], color_saturation=p["color_saturation"],
                         color_contrast=p["color_contrast"])
    mb = fr.MandelbulbParams(p["camera_distance"], p["rotation_y"], p["fov"], p["mandelbulb_power"], p["rotation_speed"],
                             p["time"])
    return st, mb


def _c(fr, st, mb):
    return st.to_params(fr.FractalType.Mandelbulb, fr.Precision.F32), mb.to_c()


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_mandelbulb_params_layout_matches_the_header(fr, tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("gcc not available")
    mirror = fr._capi.fr_mandelbulb_params
    lines = ['printf("sizeof %zu\\n", sizeof(fr_mandelbulb_params));']
    for fname, _ in mirror._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(fr_mandelbulb_params, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"fractalrenderer_amd.h\"\n"
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run([gcc, "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(mirror) == 32
    for fname, _ in mirror._fields_:
        assert int(got[fname]) == getattr(mirror, fname).offset, fname


def test_feature_macro_and_symbols(fr):
    hdr = open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")).read()
    assert re.search(r"#define FR_HAS_MANDELBULB 1\b", hdr)
    lib = fr.lib()
    for sym in ("fr_mandelbulb_params_default", "fr_pack_push_constants_mandelbulb", "fr_render_mandelbulb",
                "fr_render_mandelbulb_async"):
        assert hasattr(lib, sym), sym


def test_defaults(fr):
    mb = fr._capi.fr_mandelbulb_params()
    C.memset(C.byref(mb), 0x5A, C.sizeof(mb))
    assert fr.lib().fr_mandelbulb_params_default(C.byref(mb)) == 0
    assert (mb.camera_distance, mb.rotation_y, mb.fov, mb.mandelbulb_power, mb.rotation_speed, mb.time) == \
        (3.0, 0.0, 1.0, 8.0, 0.5, 0.0)
    assert list(mb.reserved) == [0, 0]
    d = fr.MandelbulbParams().to_c()
    assert bytes(d) == bytes(mb)
    assert fr.lib().fr_mandelbulb_params_default(None) == fr._capi.FR_ERR_INVALID_ARG


def test_presets():
    import fractalrenderer_amd as fr
    P = fr.MANDELBULB_PRESETS
    assert [P[k].mandelbulb_power for k in ("Classic (8)", "Smooth (4)", "Spiky (12)", "Extreme (16)")] == [8, 4, 12, 16]
    assert (P["Side View"].camera_distance, P["Side View"].rotation_y) == (3.0, float(np.float32(1.5708)))
    assert (P["Close-up Detail"].camera_distance, P["Close-up Detail"].rotation_y) == (1.5, float(np.float32(0.785)))


def test_packing_matches_the_fixture_bit_for_bit(fr, mbx):
    for name, (W, H, p, pc, *_rest) in mbx.items():
        st, mb = params_of(fr, p)
        got = fr.pack_push_constants_mandelbulb(st, mb)
        assert got.view(np.uint32).tolist() == np.array(pc, np.float32).view(np.uint32).tolist(), name


# ---- validation ------------------------------------------------------------------------------------------------------
def _validate(fr, p, mb, W=64, H=48):
    lib = fr.lib()
    out = (C.c_float * 20)()
    st = lib.fr_pack_push_constants_mandelbulb(C.byref(p), C.byref(mb), out)
    msg = lib.fr_last_error().decode() if st else ""
    return st, msg


def test_validation_codes_and_messages(fr):
    E = fr._capi
    st0, mb0 = _c(fr, fr.FractalState(), fr.MandelbulbParams())
    assert _validate(fr, st0, mb0)[0] == E.FR_OK

    def case(mut_p=None, mut_mb=None):
        p, mb = _c(fr, fr.FractalState(), fr.MandelbulbParams())
        if mut_p:
            mut_p(p)
        if mut_mb:
            mut_mb(mb)
        return _validate(fr, p, mb)

    st, msg = case(lambda p: setattr(p, "fractal_type", 4))
    assert st == E.FR_ERR_INVALID_ARG and "FR_FRACTAL_MANDELBULB" in msg
    st, msg = case(lambda p: setattr(p, "precision", 1))
    assert st == E.FR_ERR_UNSUPPORTED and "F32 only" in msg
    st, msg = case(lambda p: setattr(p, "precision", 7))
    assert st == E.FR_ERR_INVALID_ARG and "unknown precision" in msg
    for bad in (0, -3, (1 << 24) + 1):
        st, msg = case(lambda p: setattr(p, "max_iterations", bad))
        assert st == E.FR_ERR_INVALID_ARG and "max_iterations" in msg
    assert case(lambda p: setattr(p, "max_iterations", 5000))[0] == E.FR_OK        # clamped to 1024, as the shader
    st, msg = case(lambda p: setattr(p, "antialiasing_samples", 17))
    assert st == E.FR_ERR_INVALID_ARG and "antialiasing_samples" in msg
    for f in ("camera_distance", "rotation_y", "fov", "mandelbulb_power", "rotation_speed", "time"):
        for v in (float("nan"), float("inf")):
            st, msg = case(mut_mb=lambda mb: setattr(mb, f, v))
            assert st == E.FR_ERR_INVALID_ARG and "must be finite" in msg, f
    for k in (0, 1):
        def set_res(mb, k=k):
            mb.reserved[k] = 1
        st, msg = case(mut_mb=set_res)
        assert st == E.FR_ERR_INVALID_ARG and "reserved must be 0" in msg
    # what Mandelbulb does not read is not checked
    def unread(p):
        p.zoom = 0.0
        p.center_x = float("nan")
        p.bailout = -1.0
        p.julia_c_real = float("inf")
    assert case(unread)[0] == E.FR_OK
    # frame size rules of fr_render_mandelbulb (no context needed: validation runs first)
    p, mb = _c(fr, fr.FractalState(), fr.MandelbulbParams())
    o = fr._capi.fr_output()
    assert fr.lib().fr_render_mandelbulb(None, C.byref(p), C.byref(mb), 64, 48, None, C.byref(o)) == E.FR_ERR_INVALID_ARG
    lib = fr.lib()
    assert lib.fr_pack_push_constants_mandelbulb(C.byref(p), None, (C.c_float * 20)()) == E.FR_ERR_INVALID_ARG


def test_fr_params_paths_still_refuse_mandelbulb(fr):
    E = fr._capi
    p = fr.FractalState().to_params(fr.FractalType.Mandelbulb, fr.Precision.F32)
    assert fr.lib().fr_params_validate(C.byref(p), 64, 48) == E.FR_ERR_UNSUPPORTED
    assert fr.lib().fr_pack_push_constants(C.byref(p), (C.c_float * 20)()) == E.FR_ERR_UNSUPPORTED


# ---- the restatement and the fixture -------------------------------------------------------------------------------
def test_fixture_metadata(mbx):
    z = np.load(FIXTURE)
    meta = json.loads(str(z["__meta__"]))
    assert re.fullmatch(r"[0-9a-f]{64}", meta["sha256"][SPV_SHA256])
    assert len(mbx) >= 10
    assert os.path.getsize(FIXTURE) < 1 << 20


def test_restatement_reproduces_the_executed_shader_bitwise(mbx):
    """Measured when the fixture was made: on the host that ran the interpreter, every plane of every case is bitwise
    equal (the restatement calls the same numpy float32 functions in the same order).  Another host's numpy may round
    a transcendental differently, so the bar here leaves a little room: hit / miss and step index may differ on 0.5 %
    of the pixels (a silhouette ray that flips), colours elsewhere within 2e-3."""
    nan_px = hit_px = 0
    for name, (W, H, p, pc, rgba, lin, it, t) in mbx.items():
        r_it, r_t, r_lin = mandelbulb_ref.render(W, H, **p)
        post = mandelbulb_ref.post_chain_as_interpreted(r_lin, p["color_brightness"], p["color_saturation"],
                                                        p["color_contrast"])
        n = W * H
        bad_nan = np.isnan(post).any(-1) != np.isnan(rgba[..., :3]).any(-1)
        close = np.abs(np.nan_to_num(post) - np.nan_to_num(rgba[..., :3])).max(-1) <= 2e-3
        assert int((bad_nan | ~close).sum()) <= max(2, int(0.005 * n)), name
        if it is not None:
            assert int((r_it != it).sum()) <= max(2, int(0.005 * n)), name
            hit_px += int((it >= 0).sum())
            nan_px += int(np.isnan(lin).any(-1).sum())
    # the NaN policy's frequency: most hit points of the power-8 surface lie inside the unit sphere
    assert hit_px > 0 and 0.4 < nan_px / hit_px < 0.75, (nan_px, hit_px)


def test_ao_loop_runs_eight_times_in_float():
    k, n = np.float32(0.01), 0
    while k < np.float32(0.15):
        k, n = np.float32(k + np.float32(0.02)), n + 1
    assert n == 8


# ---- the kernel's resources ------------------------------------------------------------------------------------------
def test_mandelbulb_kernel_has_no_scratch(fr):
    """Recompiles the device code with resource remarks.  Both instantiations (march / shade split and in-loop shading)
    keep the orbit, ray and shading state in registers: no scratch, no VGPR spills.  Measured when the kernel was
    written: 131 VGPRs (3 waves per SIMD) and 60-62 SGPRs spilled -- to VGPR lanes (v_writelane), not memory: the
    inlined OCML routines' constants are hoisted out of the loops.  The bounds below hold those numbers with a small
    margin, so a change that grows them shows up here."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "fractalrenderer_amd", "csrc")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                          "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-c", os.path.join(csrc, "fr_device.hip"),
                          "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    usage, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    names = [n for n in usage if n.startswith("_ZN2fr17mandelbulb_kernel")]
    assert len(names) == 2, names
    for n in names:
        u = usage[n]
        assert u["ScratchSize [bytes/lane]"] == 0, (n, u)
        assert u["VGPRs Spill"] == 0, (n, u)
        assert u["VGPRs"] <= 136, (n, u)
        assert u["SGPRs Spill"] <= 72, (n, u)
