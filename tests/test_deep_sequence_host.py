"""Deep zoom sequences (fr_deep_sequence): the parts that need no GPU -- the ABI (macro, prototypes, struct layouts), the
plan of the standard sequence S and of sequences with unequal mantissas against the restatement (tests/deep_seq_ref.py),
the automatic F, every rejected descriptor, and the restated resampler on a linear ramp."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import deep_seq_ref as Q
import deepx_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T110 = X.views()["T110"]
S = Q.S


def _desc(fr, zoom_first=S["zoom_first"], zoom_last=S["zoom_last"], frames=S["frames"], frac_bits=0, mode=0, reserved=0,
          cx=T110["cx"], cy=T110["cy"]):
    enc = lambda s: s.encode() if isinstance(s, str) else s
    return fr._capi.fr_deep_sequence_desc(enc(cx), enc(cy), enc(zoom_first), enc(zoom_last), frames, frac_bits, mode, reserved)


def _plan(fr, d, f):
    out = fr._capi.fr_deep_sequence_frame()
    st = fr.lib().fr_deep_sequence_plan(C.byref(d), f, C.byref(out))
    return st if st else out


def _log2_pair(m, e):
    return math.log2(m) + e


# ---- ABI -----------------------------------------------------------------------------------------------------------
NAMES = ("fr_deep_sequence_plan", "fr_deep_sequence_create", "fr_deep_sequence_destroy", "fr_deep_sequence_render",
         "fr_deep_sequence_render_png", "fr_deep_sequence_stats")


def test_header_macro_prototypes_and_layouts(fr, tmp_path):
    for n in NAMES:
        assert n in fr._capi.SIGNATURES and getattr(fr.lib(), n) is not None, n
    assert "fr_deepseq_resolve" in fr._capi.INTERNAL_SIGNATURES
    desc, frame = fr._capi.fr_deep_sequence_desc, fr._capi.fr_deep_sequence_frame
    assert C.sizeof(desc) == 48 and C.sizeof(frame) == 32
    assert callable(fr.DeepZoomSequence) and fr.DeepSequenceFrame._fields == tuple(n for n, _ in frame._fields_)
    with open(os.path.join(ROOT, "include", "fractalrenderer_amd.h")) as f:
        header = f.read()
    for n in NAMES:
        assert header.count(n + "(") == 1, n
    gcc = shutil.which("gcc")
    if not gcc:
        return
    lines = ['printf("desc %zu\\n", sizeof(fr_deep_sequence_desc));', 'printf("frame %zu\\n", sizeof(fr_deep_sequence_frame));']
    for st, mirror in (("fr_deep_sequence_desc", desc), ("fr_deep_sequence_frame", frame)):
        for fname, _ in mirror._fields_:
            lines.append(f'printf("{st}.{fname} %zu\\n", offsetof({st}, {fname}));')
    proto = tmp_path / "proto.c"                       # the macro, and the prototypes as a C compiler reads them
    proto.write_text("#include \"fractalrenderer_amd.h\"\n"
                     "#if !defined(FR_HAS_DEEP_SEQUENCE) || FR_HAS_DEEP_SEQUENCE != 1\n#error FR_HAS_DEEP_SEQUENCE\n#endif\n"
                     "int (*a)(const fr_deep_sequence_desc*, int32_t, fr_deep_sequence_frame*) = fr_deep_sequence_plan;\n"
                     "int (*b)(fr_ctx*, const fr_params*, const fr_deep_sequence_desc*, uint32_t, uint32_t, fr_deep_sequence**)\n"
                     "    = fr_deep_sequence_create;\n"
                     "void (*c)(fr_deep_sequence*) = fr_deep_sequence_destroy;\n"
                     "int (*d)(fr_deep_sequence*, int32_t, const fr_output*) = fr_deep_sequence_render;\n"
                     "int (*e)(fr_deep_sequence*, int32_t, const char*) = fr_deep_sequence_render_png;\n"
                     "int (*f)(const fr_deep_sequence*, uint64_t*) = fr_deep_sequence_stats;\n")
    subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", str(proto), "-o",
                    str(tmp_path / "proto.o")], check=True)
    src = tmp_path / "seq.c"
    src.write_text("#include <stddef.h>\n#include <stdio.h>\n#include \"fractalrenderer_amd.h\"\n"
                   "int main(void) {\n" + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "seq"
    subprocess.run([gcc, "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if line)
    assert int(got["desc"]) == 48 and int(got["frame"]) == 32
    for st, mirror in (("fr_deep_sequence_desc", desc), ("fr_deep_sequence_frame", frame)):
        for fname, _ in mirror._fields_:
            assert int(got[f"{st}.{fname}"]) == getattr(mirror, fname).offset, (st, fname)


# ---- the plan ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_plan_of_the_standard_sequence(fr, mode):
    zm0, ze0 = X.zoom_pair(S["zoom_first"])
    d = _desc(fr, mode=mode)
    prev = None
    for f in range(S["frames"]):
        p = _plan(fr, d, f)
        want = Q.plan(S["zoom_first"], S["zoom_last"], S["frames"], f, mode)
        L = want["L"]
        assert L == -0.25 * f
        assert 1.0 <= p.zoom_mant < 2.0
        assert abs(_log2_pair(p.zoom_mant, p.zoom_exp2) - (_log2_pair(zm0, ze0) + L)) < 1e-12
        assert p.keyframe == math.floor(-L) == want["keyframe"] and p.frac_bits == Q.auto_frac_bits(S["zoom_first"], S["zoom_last"])
        assert (p.zoom_mant, p.zoom_exp2) == (want["zoom_mant"], want["zoom_exp2"])
        if f in Q.S_GRID:
            assert (p.zoom_mant, p.zoom_exp2) == (zm0, ze0 - f // 4) == X.zoom_pair(Q.S_GRID[f])
            assert p.u == 1.0 and p.resampled == 0
        else:
            assert 0.5 < p.u < 1.0 and p.resampled == mode
            assert abs(p.u - 2.0 ** -(-L - p.keyframe)) < 1e-15 and abs(p.u - want["u"]) < 1e-15
        z = _log2_pair(p.zoom_mant, p.zoom_exp2)
        assert prev is None or z < prev                               # strictly monotone
        prev = z
    E = fr._capi.FR_ERR_INVALID_ARG
    assert _plan(fr, d, -1) == E and _plan(fr, d, S["frames"]) == E
    assert fr.lib().fr_deep_sequence_plan(C.byref(d), 0, None) == E
    assert fr.lib().fr_deep_sequence_plan(None, 0, C.byref(fr._capi.fr_deep_sequence_frame())) == E


def test_unequal_mantissas_keep_the_endpoints_and_stay_monotone(fr):
    first, last, n = "3e-20", "7e-25", 50
    d = _desc(fr, first, last, n, mode=1)
    zm0, ze0, zm1, ze1, D = Q.walk(first, last)
    assert zm0 != zm1 and D != math.floor(D)
    p0, p1 = _plan(fr, d, 0), _plan(fr, d, n - 1)
    assert (p0.zoom_mant, p0.zoom_exp2) == (zm0, ze0) == X.zoom_pair(first) and p0.u == 1.0 and p0.keyframe == 0
    assert (p1.zoom_mant, p1.zoom_exp2) == (zm1, ze1) == X.zoom_pair(last)
    assert p1.keyframe == math.floor(-D) and p1.resampled == 1 and 0.5 < p1.u < 1.0
    prev = None
    for f in range(n):
        p = _plan(fr, d, f)
        L = 0.0 if f == 0 else D if f == n - 1 else (D * f) / (n - 1)
        z = _log2_pair(p.zoom_mant, p.zoom_exp2)
        assert 1.0 <= p.zoom_mant < 2.0 and abs(z - (_log2_pair(zm0, ze0) + L)) < 1e-12
        assert p.keyframe == math.floor(-L) and (f == 0 or 0.5 < p.u < 1.0)
        assert prev is None or z < prev
        prev = z


@pytest.mark.parametrize("mode", [0, 1])
def test_reversed_sequence_plans_the_mirrored_zooms(fr, mode):
    n = S["frames"]
    fwd, rev = _desc(fr, mode=mode), _desc(fr, S["zoom_last"], S["zoom_first"], mode=mode)
    for f in range(n):
        a, b = _plan(fr, rev, f), _plan(fr, fwd, n - 1 - f)
        assert (a.zoom_mant, a.zoom_exp2, a.u, a.resampled, a.frac_bits) == (b.zoom_mant, b.zoom_exp2, b.u, b.resampled, b.frac_bits)
        # keyframe j of the reversed sequence is (zm0', ze0' - j) with ze0' = ze0 - 2: the same view as keyframe j + 2 of S
        assert a.keyframe + 2 == b.keyframe and a.keyframe <= 0


def test_automatic_frac_bits(fr):
    for first, last in ((S["zoom_first"], S["zoom_last"]), (S["zoom_last"], S["zoom_first"]), ("1e-300", "2.5e-301"),
                        ("3", "1e-400"), ("1e-999", "2e-1000"), ("1e-20", "1e-20")):
        want = Q.auto_frac_bits(first, last)
        for mode in (0, 1):
            assert _plan(fr, _desc(fr, first, last, 7, mode=mode), 3).frac_bits == want, (first, last)
    assert Q.auto_frac_bits(S["zoom_first"], S["zoom_last"]) == X.frac_bits_x("1.25e-111")
    assert _plan(fr, _desc(fr, frac_bits=640), 1).frac_bits == 640


# ---- validation ----------------------------------------------------------------------------------------------------
def test_every_rejected_descriptor(fr):
    E, U = fr._capi.FR_ERR_INVALID_ARG, fr._capi.FR_ERR_UNSUPPORTED
    ok = lambda d: not isinstance(_plan(fr, d, 0), int)
    assert ok(_desc(fr)) and ok(_desc(fr, mode=1)) and ok(_desc(fr, frames=2))
    for frames in (1, 0, -3):
        assert _plan(fr, _desc(fr, frames=frames), 0) == E, frames
    for mode in (-1, 2, 7):
        assert _plan(fr, _desc(fr, mode=mode), 0) == E, mode
    assert _plan(fr, _desc(fr, reserved=1), 0) == E
    for fb in (-1, 1, 127, 4097):
        assert _plan(fr, _desc(fr, frac_bits=fb), 0) == E, fb
    assert ok(_desc(fr, frac_bits=128)) and ok(_desc(fr, frac_bits=4096))
    for z in ("1e-1001", "1e4", "0", "-3", "x", "", None, "1e-110 "):
        assert _plan(fr, _desc(fr, zoom_first=z), 0) == E, z
        assert _plan(fr, _desc(fr, zoom_last=z), 0) == E, z
    for kw in (dict(cx=None), dict(cy=None), dict(cx="1e"), dict(cy="5e9")):
        assert _plan(fr, _desc(fr, **kw), 0) == E, kw
    # mode 1: a keyframe the walk needs outside [1e-1000, 1e3]; mode 0 renders the same descriptors
    for first, last, frames in (("1.5e-1000", "1e-1000", 3), ("3e-1000", "1e-1000", 4), ("600", "1000", 3)):
        assert ok(_desc(fr, first, last, frames, mode=0)), (first, last)
        assert _plan(fr, _desc(fr, first, last, frames, mode=1), 0) == E, (first, last)
    # ... and walks that end exactly on the last keyframe the range holds are accepted
    assert ok(_desc(fr, "4e-1000", "1e-1000", 9, mode=1)) and ok(_desc(fr, "2e-1000", "1e-1000", 3, mode=1))
    assert ok(_desc(fr, "250", "1000", 5, mode=1))
    # the rules for p (fr_render_deepx's), with no device: through the resolver the create call runs first
    L = fr.lib()
    walk = (C.c_char * 64)()

    def resolve(d, w=64, h=48, **kw):
        st = fr.FractalState(max_iterations=S["max_iter"])
        p = st.to_params(kw.pop("fractal", fr.FractalType.Mandelbrot), kw.pop("precision", fr.Precision.F64), False)
        for k, v in kw.items():
            setattr(p, k, v)
        return L.fr_deepseq_resolve(C.byref(p), C.byref(d), w, h, walk)

    d = _desc(fr, mode=1)
    assert resolve(d) == 0
    assert resolve(d, flags=fr.FR_FLAG_DEEPX_BLA) == 0 and resolve(d, flags=fr.FR_FLAG_DEEPX_BLA | fr._capi.FR_FLAG_POST_CHAIN) == 0
    assert resolve(d, flags=fr.FR_FLAG_DEEP_BLA) == U
    assert resolve(d, fractal=fr.FractalType.JuliaSet) == U and resolve(d, precision=fr.Precision.F32) == U
    assert resolve(d, orbit_trap_enabled=1) == U and resolve(d, stripe_enabled=1) == U and resolve(d, interior_style=2) == U
    assert resolve(d, max_iterations=0) == E and resolve(d, bailout=0.0) == E and resolve(d, w=0, h=48) == E
    assert resolve(_desc(fr, frames=1)) == E
    # the entry points check their arguments before they touch a device
    p = fr.FractalState().to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, False)
    h = C.c_void_p()
    o = fr._capi.fr_output(None, None, None, fr._capi.FR_MEM_HOST, 0)
    assert L.fr_deep_sequence_create(None, C.byref(p), C.byref(d), 64, 48, C.byref(h)) == E and not h.value
    assert L.fr_deep_sequence_render(None, 0, C.byref(o)) == E
    assert L.fr_deep_sequence_render_png(None, 0, b"x.png") == E
    assert L.fr_deep_sequence_stats(None, (C.c_uint64 * 3)()) == E
    L.fr_deep_sequence_destroy(None)


# ---- the restated resampler -----------------------------------------------------------------------------------------
def _ramp_keys(W, H, coef, quant=None):
    """two keyframes of a colour that is linear in the view's coordinate: keyframe k + 1 shows the middle half of keyframe k"""
    def key(scale):
        wx = (np.arange(W, dtype=np.float64) - 0.5 * W)[None, :] * scale
        wy = (np.arange(H, dtype=np.float64) - 0.5 * H)[:, None] * scale
        img = np.empty((H, W, 4), np.float64)
        for ch, (c0, a, b) in enumerate(coef):
            img[..., ch] = c0 + a * wx + b * wy
        img[..., 3] = 1.0
        return img
    return key(1.0), key(0.5)


def _ramp_at(W, H, coef, u):
    wx = (np.arange(W, dtype=np.float64) - 0.5 * W)[None, :] * u
    wy = (np.arange(H, dtype=np.float64) - 0.5 * H)[:, None] * u
    return np.stack([c0 + a * wx + b * wy for c0, a, b in coef], axis=2)


def _ulps(got, want):
    return np.abs(got[..., :3].astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64)


def _ramp13(W, H):
    """a ramp of 13-bit values inside one binade, [0.5, 1): both keyframes hold it exactly in float32"""
    g = lambda v: round(v * 4096) / 4096
    coef = [(0.75, g(0.12 / W), g(0.08 / H)), (0.75, -g(0.1 / W), g(0.1 / H)), (0.8125, g(0.15 / W), -g(0.02 / H))]
    k0, k1 = _ramp_keys(W, H, coef)
    assert all(np.array_equal(k.astype(np.float32).astype(np.float64), k) and k[..., :3].min() >= 0.5 and k.max() <= 1.0
               for k in (k0, k1))
    return coef, k0.astype(np.float32), k1.astype(np.float32)


@pytest.mark.parametrize("W,H", [(64, 48), (17, 9), (203, 117)])
def test_restated_resampler_reproduces_a_linear_ramp(W, H):
    """Bilinear interpolation of a linear function is that function; what is left is rounding.  With u a multiple of 2^-9
    the read points are multiples of 2^-10, the weights and their complements are exact, and a product of a 13-bit value
    and a 10-bit weight fits a float32: 2 ulps hold with room (the error is 0)."""
    coef, k0, k1 = _ramp13(W, H)
    for u in (0.75, 0.625, 0.875, 0.5 + 2.0 ** -9, 1.0 - 2.0 ** -9, 0.5 + 189 * 2.0 ** -9):
        got = Q.resample(k0, k1, u)
        ulps = _ulps(got, _ramp_at(W, H, coef, u))
        print(W, H, u, "max error in fp32 ulps", float(ulps.max()))
        assert ulps.max() <= 2.0
        assert np.all(got[..., 3] == 1.0)


@pytest.mark.parametrize("W,H", [(64, 48), (203, 117)])
def test_restated_resampler_rounding_at_the_zooms_of_a_real_walk(W, H):
    """u = 2^-0.25, 2^-0.5, 2^-0.75 (the frames of S) and values next to the ends of (0.5, 1): nothing is exact any more.
    The bound is that of the arithmetic as the header writes it, in ulps of the binade [0.5, 1): each complement 1.0f - w
    is rounded once, so cx + wx and cy + wy each miss 1 by at most 2^-25 (0.5 ulp of a value below 1, together 1 ulp);
    each interpolation stage is two products and a sum, at most 0.5 ulp for the products together with room and 0.5 for
    the sum (1 ulp a stage, 2 together): 3 ulps.  Measured: 2.2 - 2.5."""
    coef, k0, k1 = _ramp13(W, H)
    for u in (2.0 ** -0.25, 2.0 ** -0.5, 2.0 ** -0.75, 0.999, 0.5000001):
        ulps = _ulps(Q.resample(k0, k1, u), _ramp_at(W, H, coef, u))
        print(W, H, u, "max error in fp32 ulps", float(ulps.max()), "mean", float(ulps.mean()))
        assert ulps.max() <= 3.0


def test_restated_resampler_with_u2_one_returns_the_deeper_keyframe():
    rng = np.random.default_rng(11)
    for W, H in ((64, 48), (7, 5), (1, 1)):
        k0 = rng.random((H, W, 4), dtype=np.float32)
        k1 = rng.random((H, W, 4), dtype=np.float32)
        k1[..., 3] = 1.0
        got = Q.resample(k0, k1, 0.5)                                # u2 == 1: qx == x, every weight 0
        assert np.array_equal(got.view(np.uint32), k1.view(np.uint32))


def test_restated_resampler_reads_keyframe_k_outside_the_deeper_one():
    """dyadic u and a ramp of few bits: every product and sum is exact, so the frame IS the ramp, and the pixels outside
    the deeper keyframe's reach come from keyframe k"""
    W, H, u = 16, 12, 0.75
    coef = [(0.5, 1.0 / 64, 1.0 / 128), (0.5, -1.0 / 64, 1.0 / 64), (0.25, 1.0 / 128, 0.0)]
    k0, k1 = (k.astype(np.float32) for k in _ramp_keys(W, H, coef))
    got = Q.resample(k0, k1, u)
    assert np.array_equal(got[..., :3].astype(np.float64), _ramp_at(W, H, coef, u))
    marked = k0.copy()
    marked[..., :3] += np.float32(1.0)                               # keyframe k moved by 1: where is it read?
    from_k0 = Q.resample(marked, k1, u)[..., 0] != got[..., 0]
    qx = 0.5 * W + (np.arange(W) - 0.5 * W) * 2 * u
    qy = 0.5 * H + (np.arange(H) - 0.5 * H) * 2 * u
    inside = ((qx >= 0) & (qx <= W - 1))[None, :] & ((qy >= 0) & (qy <= H - 1))[:, None]
    assert np.array_equal(from_k0, ~inside) and 0 < inside.sum() < W * H
