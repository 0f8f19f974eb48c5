"""Store footprint of every kernel that writes through a caller's pointer: each render below goes into guard-banded,
pattern-filled planes (tests/guarded.py) and gets three verdicts --
  (a) the guard bands before and after every plane still hold the pattern;
  (b) no payload element the call owns still holds the pattern, and under FR_LAYOUT_FRAME the rows of the other parts do;
  (c) the values equal the CPU reference of that path (never another GPU render), under the bars of the path's own suite:
      check_against (test_gpu_parity) for fr_render, _ulp_ok / _few / RGB_TOL / NU_TOL_F64 (test_phoenix_gpu), MAX_FLIP /
      RGB_TOL / _post_policy (test_mandelbulb_gpu, whose _few carries MAX_FLIP), NU_TOL / RGB_TOL / _few of test_deep_gpu
      for the deep views with its colour stage in the form test_deepx_gpu keeps (_expected_rgba there: the same stage for
      any frame size; test_deep_gpu's own is written for 256x192), + the three step counts of FR_FLAG_DEEP_BLA against
      last_deep_steps().

The matrix (W x H; "small" = 1x1, 1x70, 70x1, 7x9, 9x7, 63x65, 65x63, 131x67; "big" = 257x129, 520x504):

  path (id)                                                     whole frame   layouts (131x67, 7x9)   big
  ------------------------------------------------------------  ------------  ----------------------  -----------------------
  fr_render Mandelbrot fp64, staging 1     (mandel_staging1)    small         all                     -
  fr_render Mandelbrot fp64, staging 3     (mandel_staging3)    small         all                     auto + forced options
  fr_render Mandelbrot fp64, tile_kernel 1 (mandel_general)     small         all                     -
  fr_render Julia fp32                     (julia_f32)          small         all                     -
  fr_render Burning Ship, orbit trap       (ship_trap)          small         all                     -
  fr_render Mandelbrot aa 2, automatic     (mandel_aa2)         small         all                     -
  fr_render Mandelbrot aa 2, banded        (mandel_aa2_banded)  small         all                     -
  fr_render Deep_Zoom, use_perturbation    (deep_zoom)          small         all                     auto + forced options
  fr_render_phoenix fp32 / fp64            (phoenix_f32/_f64)   small         all                     auto + forced options
  fr_render_phoenix fp32 / fp64, aa 2      (phoenix_*_aa2)      small         all                     -
  fr_render_mandelbulb, split 0 / 1        (mandelbulb_split*)  small         all                     -
  fr_render_deep, VIEW_A                   (deep)               small         all                     -
  fr_render_deep + FR_FLAG_DEEP_BLA        (deep_bla)           small         all                     -
  fr_render_deepx, 1e-110 / 1e-320         (deepx_above/below)  small         all                     -

  layouts "all": whole frame in FR_MEM_HOST planes; packed shards (1,3,5), (2,3,8), (0,2,1), (7,8,4) and the part that owns
  the short last strip, each against the reference's rows; FR_LAYOUT_FRAME, one part alone and then the others, for the
  shardings (3,5), (2,1), (8,4); the plane subsets iter / nu / rgba + iter; a part with no rows (packed and whole-frame).
  forced options: "shards" 8 and 64, "probes" 1 and 2 (Phoenix at max_iter 64 is a moderate launch: 257x129 is a grid of
  71 workgroups, 8 shards, home shard only; 520x504 a grid of 256 or more, 64 shards, home + a neighbour -- asserted).
  fr_export_rgb8 / fr_export_rgb16: widths 1, 3, 4, 5, 61, 64 x heights 1, 5, 37, output offsets 0..3, device and host.
  fr_colorize_async: 7x9 and 131x67, Mandelbrot fp64 and Julia fp32.
  staging 1 / 3: last_stages() is asserted after every render (1 / 2), so a planning change cannot quietly turn these cases
  into something else.  mandel_aa2_banded: bands of 8 pixel rows apply to whole packed frames taller than 8 rows; its
  shards and FR_LAYOUT_FRAME parts take the sample loop, its frames of up to 8 rows the unbanded staged form.

Frames of fewer than 2000 pixels can use the exception caps (max(2, 0.1 %) palette-wrap / pre-gamma pixels, MAX_FLIP) only
through their floor of 2.  On those frames the fr_render references are shown on the CPU to need no exception: the fp64
cases cannot take the palette-wrap exception at all and run without the post chain (no pre-gamma exception), and no
reference pixel of the fp32 cases (julia_f32, deep_zoom) lies within 1e-4 of a palette wrap (asserted in
_OraclePath.compute_reference).  Phoenix, Mandelbulb and the deep views lean on the floor at every "small" size below
131x67 (on 1x1 the colour check of Mandelbulb cannot fail; its guards and its footprint still can): whether the GPU's libm
moves a colour across a palette knot there cannot be told on the CPU.

What the FR_MEM_HOST cases can and cannot see: the copy back rewrites every element of the caller's planes from the
library's staging planes, so verdict (b) holds there whatever the kernel stored; a dropped or misplaced store shows only in
(c), as whatever the staging planes held, and (a) pins the copy's length.  (Two deliberately wrong builds of walk_subtiles,
last column never stored / one column too many, fail every one-pass case in device planes; in host planes they fail
through (c) and the BLA counts, except Mandelbulb at 131x67, where a 67-pixel column is within MAX_FLIP.)
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import deep_bla_ref as BR
import deep_ref as R
import deepx_ref as X
import mandelbulb_ref
import phoenix_ref
from guarded import Guarded, GuardedPlanes
from oracle import oracle as O
from test_deep_gpu import NU_TOL as DEEP_NU_TOL, RGB_TOL as DEEP_RGB_TOL, _few as deep_few
from test_deepx_gpu import _expected_rgba as deep_expected_rgba
from test_gpu_parity import RGB_TOL as PARITY_RGB_TOL, check_against, to_state
from test_mandelbulb_gpu import RGB_TOL as BULB_RGB_TOL, _few as bulb_few, _post_policy
from test_phoenix_gpu import NU_TOL_F64, RGB_TOL as PHOENIX_RGB_TOL, _few as phoenix_few, _ulp_ok

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (1, 70), (70, 1), (7, 9), (9, 7), (63, 65), (65, 63), (131, 67)]
BIG = [(257, 129), (520, 504)]
LAYOUT_GEOMS = [(131, 67), (7, 9)]
SHARDS = [(1, 3, 5), (2, 3, 8), (0, 2, 1), (7, 8, 4)]
FRAME_SHARDINGS = [(3, 5), (2, 1), (8, 4)]          # (nparts, rows per strip); part 1 renders alone first
FORCED = [{}, {"shards": 8}, {"shards": 64}, {"probes": 1}, {"probes": 2}]


def _gid(g):
    return "%dx%d" % g


def _fid(f):
    return "auto" if not f else "_".join("%s%d" % kv for kv in f.items())


@contextlib.contextmanager
def _options(r, opts):
    try:
        for k, v in opts.items():
            r.set_option(k, v)
        yield
    finally:
        for k in opts:
            r.set_option(k, 0)


def _last_strip_shard(H):
    """the part (of 2, strips of 5 rows) that owns the short last strip of an H-row frame"""
    assert H % 5 != 0
    return ((H // 5) % 2, 2, 5)


# ---- the paths: how to render one (Renderer method and raw C ABI), its CPU reference, its checker ----------------------
class _Path:
    f64 = False                      # the nu plane's type
    name = None                      # its key in _paths()

    def options(self, W):
        return {}

    def reference(self, oracle, W, H):
        return _cached_reference(self.name, W, H)

    def after(self, r, W, H, rows):
        """what else the call must have left behind (the BLA step counts), for the frame rows it rendered"""


class _OraclePath(_Path):
    """fr_render against oracle.render through check_against"""

    def __init__(self, p, options=None, stages=None):
        self.p, self.f64, self._opts, self.stages = p, p.precision == 1, options or (lambda W: {}), stages

    def options(self, W):
        return self._opts(W)

    def after(self, r, W, H, rows):
        if self.stages is not None:
            assert r.last_stages() == self.stages, (r.last_stages(), W, H)      # the forced schedule was the one taken

    def _args(self, fr):
        prec = fr.Precision.F64 if self.p.precision == 1 else fr.Precision.F32
        return to_state(fr, self.p), fr.FractalType(self.p.fractal), prec

    def render(self, fr, r, W, H, shard, planes):
        st, ft, prec = self._args(fr)
        r.render(st, W, H, fractal_type=ft, precision=prec, post_chain=bool(self.p.post_chain), shard=shard, **planes)

    def raw(self, fr, r, W, H, sh, out):
        st, ft, prec = self._args(fr)
        cp = st.to_params(ft, prec, bool(self.p.post_chain))
        return fr.lib().fr_render_shard(r._ctx, C.byref(cp), W, H, C.byref(sh), C.byref(out))

    def _near_wrap(self, nu):
        """check_against's palette-wrap neighbourhood, on the reference's own nu"""
        p = self.p
        scale, off, mi, nu32 = np.float32(p.color_scale), np.float32(p.color_offset), np.float32(p.max_iterations), nu.astype(np.float32)
        if p.fractal == 5:
            t = (nu32 * scale + off) * np.float32({0: 0.05, 1: 0.03, 2: 0.04}.get(p.palette_mode, 0.02))
        else:
            t = (np.clip(nu32 / mi * scale, 0, 1) + off) if p.fractal == 0 else (off + nu32 / mi * scale)
        u = t - np.floor(t)
        return int((np.minimum(u, 1 - u) < 1e-4).sum())

    def compute_reference(self, oracle, W, H):
        ref = oracle.render(self.p, W, H)
        if W * H < 2000:
            # the tiny frames lean on no tolerance exception: fp64 cannot take the wrap exception and runs without the
            # post chain; fp32 has no reference pixel near a wrap
            assert (self.p.precision == 1 and not self.p.post_chain) or self._near_wrap(ref.nu) == 0, (W, H)
        return ref

    def check(self, oracle, W, H, rows, rgba, nu, it):
        ref = self.reference(oracle, W, H)
        e_rgba, e_nu, e_it = ref.rgba[rows], ref.nu[rows], ref.iter[rows]
        # an absent plane stands in with the reference's own: the present ones are held to check_against's bars
        check_against(self.p, e_it, e_nu, e_rgba, e_rgba if rgba is None else rgba, e_nu if nu is None else nu,
                      e_it if it is None else it)


class _PhoenixPath(_Path):
    MAX_ITER = 64

    def __init__(self, f64, aa=1):
        self.f64, self.aa = f64, aa

    def _args(self, fr):
        return (fr.FractalState(max_iterations=self.MAX_ITER, antialiasing_samples=self.aa), fr.PhoenixParams(),
                fr.Precision.F64 if self.f64 else fr.Precision.F32)

    def render(self, fr, r, W, H, shard, planes):
        st, ph, prec = self._args(fr)
        r.render_phoenix(st, W, H, ph, precision=prec, shard=shard, **planes)

    def raw(self, fr, r, W, H, sh, out):
        st, ph, prec = self._args(fr)
        cp, cph = st.to_params(fr.FractalType.Phoenix, prec), ph.to_c()
        return fr.lib().fr_render_phoenix(r._ctx, C.byref(cp), C.byref(cph), W, H, C.byref(sh), C.byref(out))

    def compute_reference(self, oracle, W, H):
        return phoenix_ref.render(W, H, max_iterations=self.MAX_ITER, f64=self.f64, aa=self.aa)

    def check(self, oracle, W, H, rows, rgba, nu, it):
        r_it, r_sm, r_rgb = (a[rows] for a in self.reference(oracle, W, H))
        if it is not None:
            assert np.array_equal(it, r_it), "escape indices differ: %d pixels" % int((it != r_it).sum())
        if nu is not None:
            assert (np.abs(nu - r_sm).max() <= NU_TOL_F64) if self.f64 else np.all(_ulp_ok(nu, r_sm))
        if rgba is not None:
            assert np.all(rgba[..., 3] == 1.0)
            bad = np.abs(rgba[..., :3] - r_rgb).max(axis=2) > PHOENIX_RGB_TOL
            assert phoenix_few(bad, r_it.size), int(bad.sum())


class _MandelbulbPath(_Path):
    KW = dict(max_iterations=32, time=1.25)

    def __init__(self, split):
        self.split = split

    def options(self, W):
        return {"mandelbulb_split": self.split}

    def _args(self, fr):
        return fr.FractalState(max_iterations=self.KW["max_iterations"]), fr.MandelbulbParams(time=self.KW["time"])

    def render(self, fr, r, W, H, shard, planes):
        st, mb = self._args(fr)
        r.render_mandelbulb(st, W, H, mb, post_chain=True, shard=shard, **planes)

    def raw(self, fr, r, W, H, sh, out):
        st, mb = self._args(fr)
        cp, cmb = st.to_params(fr.FractalType.Mandelbulb, fr.Precision.F32, True), mb.to_c()
        return fr.lib().fr_render_mandelbulb(r._ctx, C.byref(cp), C.byref(cmb), W, H, C.byref(sh), C.byref(out))

    def compute_reference(self, oracle, W, H):
        assert W * H <= 131 * 67                     # whole-frame references of this path stay small
        r_it, r_t, r_lin = mandelbulb_ref.render(W, H, **self.KW)
        return r_it, r_t, _post_policy(mandelbulb_ref.post_chain(r_lin))

    def check(self, oracle, W, H, rows, rgba, nu, it):
        r_it, r_t, r_rgb = (a[rows] for a in self.reference(oracle, W, H))
        n = r_it.size
        if it is not None:
            assert bulb_few((it >= 0) != (r_it >= 0), n) and bulb_few(it != r_it, n), int((it != r_it).sum())
        if nu is not None:
            assert bulb_few(~np.isclose(nu, r_t, 1e-4, 1e-5), n)
        if rgba is not None:
            assert not np.isnan(rgba).any() and np.all(rgba[..., 3] == 1.0)
            bad = np.abs(rgba[..., :3] - r_rgb).max(-1) > BULB_RGB_TOL
            assert bulb_few(bad, n), int(bad.sum())


class _DeepPath(_Path):
    """fr_render_deep (VIEW_A), plain or with FR_FLAG_DEEP_BLA, and fr_render_deepx (a view of deepx_views.json)"""
    f64 = True

    def __init__(self, kind, view):
        self.kind, self.v = kind, view

    def _args(self, fr):
        v = self.v
        if self.kind == "deepx":
            return fr.FractalState(max_iterations=v["max_iter"]), fr.DeepView(v["cx"], v["cy"], zoom=v["zoom"])
        return fr.FractalState(zoom=v["zoom"], max_iterations=v["max_iter"]), fr.DeepView(v["cx"], v["cy"])

    def render(self, fr, r, W, H, shard, planes):
        st, view = self._args(fr)
        r.render_deep(st, W, H, view, shard=shard, bla=self.kind == "bla", **planes)

    def raw(self, fr, r, W, H, sh, out):
        st, view = self._args(fr)
        cp = st.to_params(fr.FractalType.Mandelbrot, fr.Precision.F64, False)
        if self.kind == "deepx":
            cv = view.to_cx()
            return fr.lib().fr_render_deepx(r._ctx, C.byref(cp), C.byref(cv), W, H, C.byref(sh), C.byref(out))
        if self.kind == "bla":
            cp.flags |= fr.FR_FLAG_DEEP_BLA
        cv = view.to_c()
        return fr.lib().fr_render_deep(r._ctx, C.byref(cp), C.byref(cv), W, H, C.byref(sh), C.byref(out))

    def compute_reference(self, oracle, W, H):
        if self.kind == "deepx":
            return X.restate_x(self.v, W, H)
        return (BR.restate_bla if self.kind == "bla" else R.restate)(self.v, W, H)[0]

    def after(self, r, W, H, rows):
        if self.kind == "bla":
            # every table radius and every level choice of the kernel over the pixels of THIS call, summed: equal
            counts = BR.restate_bla(self.v, W, H, rows=rows)[1]
            assert tuple(r.last_deep_steps()) == tuple(counts), (tuple(r.last_deep_steps()), tuple(counts))

    def check(self, oracle, W, H, rows, rgba, nu, it):
        v = self.v
        samples = [(a[rows], b[rows]) for a, b in self.reference(oracle, W, H)]
        r_it, r_r2 = samples[0]
        if it is not None:
            assert np.array_equal(it, r_it), "escape indices differ: %d pixels" % int((it != r_it).sum())
        if nu is not None:
            assert np.abs(nu - R.smooth(r_it, r_r2, v["max_iter"])).max() <= DEEP_NU_TOL
        if rgba is not None:
            assert np.all(rgba[..., 3] == 1.0)
            bad = np.abs(rgba[..., :3] - deep_expected_rgba(oracle, v, samples, 1, False)).max(axis=2) > DEEP_RGB_TOL
            assert deep_few(bad, r_it.size), int(bad.sum())


@functools.lru_cache(maxsize=None)
def _paths():
    O.build()
    P = O.OracleParams
    mandel = dict(max_iterations=200, center_x=-0.75, zoom=2.0)
    paths = {
        "mandel_staging1": _OraclePath(P(**mandel), lambda W: {"staging": 1}, stages=1),
        "mandel_staging3": _OraclePath(P(**mandel), lambda W: {"staging": 3}, stages=2),
        "mandel_general": _OraclePath(P(**mandel), lambda W: {"tile_kernel": 1}),
        "julia_f32": _OraclePath(P(fractal=1, precision=0, center_x=0.0, julia_c_real=0.4, julia_c_imag=0.4, max_iterations=200)),
        "ship_trap": _OraclePath(P(fractal=2, center_x=-0.5, center_y=-0.5, zoom=3.5, max_iterations=160, orbit_trap_enabled=1,
                                   orbit_trap_radius=0.6, interior_style=1, palette_mode=3)),
        "mandel_aa2": _OraclePath(P(aa=2, max_iterations=100, center_x=-0.75, zoom=2.0)),
        # bands of 8 pixel rows: every frame taller than 8 rows goes through the scratch band by band
        "mandel_aa2_banded": _OraclePath(P(aa=2, max_iterations=100, center_x=-0.75, zoom=2.0),
                                         lambda W: {"ssaa_band_samples": W * 4 * 8}),
        "deep_zoom": _OraclePath(P(fractal=5, precision=0, center_x=-0.75, center_y=0.1, zoom=100.0, max_iterations=300,
                                   use_perturbation=1, palette_mode=1, color_scale=2.0, color_offset=0.5)),
        "phoenix_f32": _PhoenixPath(False), "phoenix_f64": _PhoenixPath(True),
        "phoenix_f32_aa2": _PhoenixPath(False, 2), "phoenix_f64_aa2": _PhoenixPath(True, 2),
        "mandelbulb_split0": _MandelbulbPath(0), "mandelbulb_split1": _MandelbulbPath(1),
        "deep": _DeepPath("plain", R.VIEW_A), "deep_bla": _DeepPath("bla", R.VIEW_A),
        "deepx_above": _DeepPath("deepx", X.views()["T110"]),       # 1e-110: plain steps, the double range holds the deltas
        "deepx_below": _DeepPath("deepx", X.views()["T320"]),       # 1e-320: below the double range, extended steps
    }
    assert sorted(paths) == sorted(PATH_NAMES)
    for name, p in paths.items():
        p.name = name
    return paths


@functools.lru_cache(maxsize=None)
def _cached_reference(name, W, H):
    """the CPU reference of a path at a size: computed once, shared by every test, never changed"""
    return _paths()[name].compute_reference(O, W, H)


PATH_NAMES = ["mandel_staging1", "mandel_staging3", "mandel_general", "julia_f32", "ship_trap", "mandel_aa2",
              "mandel_aa2_banded", "deep_zoom", "phoenix_f32", "phoenix_f64", "phoenix_f32_aa2", "phoenix_f64_aa2",
              "mandelbulb_split0", "mandelbulb_split1", "deep", "deep_bla", "deepx_above", "deepx_below"]


def _by_path(names=PATH_NAMES):
    return pytest.mark.parametrize("name", names)


# ---- the three verdicts -----------------------------------------------------------------------------------------------
def _render_packed(fr, r, oracle, path, W, H, *, shard=None, backend="device", planes=GuardedPlanes.NAMES, forced=None):
    """one render through the Renderer into packed guarded planes, and its verdicts; returns the planes"""
    rows = shard.rows(H) if shard else H
    assert rows > 0
    g = shard.global_rows(H) if shard else np.arange(H)
    gp = GuardedPlanes(rows, W, f64=path.f64, backend=backend, planes=planes)
    with _options(r, dict(path.options(W), **(forced or {}))):
        path.render(fr, r, W, H, shard, gp.kwargs())
        path.after(r, W, H, g)
    assert gp.guards_intact(), gp.guard_hits()                              # (a)
    assert gp.unwritten() == 0, {k: p.unwritten() for k, p in gp.present()}   # (b)
    path.check(oracle, W, H, g, *gp.values())                               # (c)
    return gp


def _empty_part(fr, r, path, W, H, shard, layout):
    """a part that owns no rows stores nothing anywhere: raw C ABI, planes of a whole frame, all of it still the pattern"""
    assert shard.rows(H) == 0
    gp = GuardedPlanes(H, W, f64=path.f64, backend="device")
    with _options(r, path.options(W)):
        assert path.raw(fr, r, W, H, shard.to_c(), gp.output(fr._capi, layout)) == fr._capi.FR_OK
    assert gp.guards_intact(), gp.guard_hits()
    assert gp.untouched(np.ones(H, bool)) and gp.unwritten() == H * W * 6


@pytest.mark.parametrize("geom", SMALL, ids=_gid)
@_by_path()
def test_whole_frame_in_device_planes(fr, renderer, oracle, name, geom):
    path = _paths()[name]
    _render_packed(fr, renderer, oracle, path, *geom)


@pytest.mark.parametrize("geom", LAYOUT_GEOMS, ids=_gid)
@_by_path()
def test_whole_frame_in_host_planes(fr, renderer, oracle, name, geom):
    """FR_MEM_HOST: the guards are host memory, the copy back is what is held to them"""
    path = _paths()[name]
    _render_packed(fr, renderer, oracle, path, *geom, backend="host")


@pytest.mark.parametrize("geom", LAYOUT_GEOMS, ids=_gid)
@_by_path()
def test_packed_shards(fr, renderer, oracle, name, geom):
    """partial strips, strips that are no whole sub-tile rows, the short last strip: each against the reference's rows
    (at 7x9 the parts (2,3,8) and (7,8,4) own no rows: they must leave everything alone)"""
    path = _paths()[name]
    W, H = geom
    last = _last_strip_shard(H)
    assert H - 1 in fr.Shard(*last).global_rows(H) and fr.Shard(*last).rows(H) % 5 != 0
    for s in SHARDS + [last]:
        shard = fr.Shard(*s)
        if shard.rows(H) == 0:
            _empty_part(fr, renderer, path, W, H, shard, fr._capi.FR_LAYOUT_PACKED)
        else:
            _render_packed(fr, renderer, oracle, path, W, H, shard=shard)
    _render_packed(fr, renderer, oracle, path, W, H, shard=fr.Shard(*SHARDS[0]), backend="host")


@pytest.mark.parametrize("geom", LAYOUT_GEOMS, ids=_gid)
@_by_path()
def test_frame_layout_one_part_alone_then_the_others(fr, renderer, oracle, name, geom):
    """FR_LAYOUT_FRAME through the raw C ABI: part 1 alone into pattern-filled whole-frame planes -- its rows equal the
    reference's, every other row is untouched, the guards are intact -- then the remaining parts, and the whole frame"""
    path = _paths()[name]
    W, H = geom
    E = fr._capi
    for nparts, R_ in FRAME_SHARDINGS:
        gp = GuardedPlanes(H, W, f64=path.f64, backend="device")
        out = gp.output(E, E.FR_LAYOUT_FRAME)
        with _options(renderer, path.options(W)):
            for part in [1] + [k for k in range(nparts) if k != 1]:
                shard = fr.Shard(part, nparts, R_)
                g = shard.global_rows(H)
                assert path.raw(fr, renderer, W, H, shard.to_c(), out) == E.FR_OK, (nparts, R_, part)
                if len(g):
                    path.after(renderer, W, H, g)
                if part == 1:
                    mine = np.zeros(H, bool)
                    mine[g] = True
                    assert mine.any() and not mine.all()
                    assert gp.guards_intact(), (nparts, R_, gp.guard_hits())
                    assert gp.unwritten(mine) == 0, (nparts, R_)
                    assert gp.untouched(~mine), (nparts, R_)
                    path.check(oracle, W, H, g, *(p[g] for p in gp.values()))
        assert gp.guards_intact(), (nparts, R_, gp.guard_hits())
        assert gp.unwritten() == 0, (nparts, R_)
        path.check(oracle, W, H, np.arange(H), *gp.values())


@pytest.mark.parametrize("geom", LAYOUT_GEOMS, ids=_gid)
@_by_path()
def test_plane_subsets(fr, renderer, oracle, name, geom):
    """the library accepts any non-empty subset of planes: the absent ones are None, the present ones guarded and complete"""
    path = _paths()[name]
    for planes in (("iter",), ("nu",), ("rgba", "iter")):
        gp = _render_packed(fr, renderer, oracle, path, *geom, planes=planes)
        assert [k for k, _ in gp.present()] == [k for k in GuardedPlanes.NAMES if k in planes]


@_by_path()
def test_a_part_with_no_rows_stores_nothing(fr, renderer, name):
    path = _paths()[name]
    W, H = 131, 67
    for layout in (fr._capi.FR_LAYOUT_PACKED, fr._capi.FR_LAYOUT_FRAME):
        _empty_part(fr, renderer, path, W, H, fr.Shard(2, 3, 64), layout)


# ---- the queue regimes of a moderate launch, and the forced ones --------------------------------------------------------
@pytest.mark.parametrize("forced", FORCED, ids=_fid)
@pytest.mark.parametrize("geom", BIG, ids=_gid)
@_by_path(["phoenix_f32", "phoenix_f64", "mandel_staging3", "deep_zoom"])
def test_queue_regimes(fr, renderer, oracle, name, geom, forced):
    """257x129: 561 sub-tiles, a grid of 71 workgroups (8 shards, waves stop at the home shard taken from the workgroup
    index); 520x504: 4095 sub-tiles in 256 blocks, a grid of 256 workgroups or more (64 shards, home + a neighbour).
    Asserted for Phoenix, whose launch at max_iter 64 is moderate: a later planning change that moves these frames into
    another regime fails here instead of testing something else.  Then "shards" and "probes" by force: a sub-tile that no
    wave visits is an unwritten pixel.  (deep_zoom_kernel ignores the probe limit; its frame must still be complete.)"""
    path = _paths()[name]
    _render_packed(fr, renderer, oracle, path, *geom, forced=forced)
    if isinstance(path, _PhoenixPath) and not forced:
        grid = renderer.last_grid()
        assert (64 <= grid < 256) if geom == BIG[0] else grid >= 256, grid


# ---- the other kernels that store through a caller's pointer ------------------------------------------------------------
def _export_source(rng, h, w):
    """test_export_rgb8's random planes: out-of-range, negative and huge values included"""
    x = rng.random((h, w, 4), dtype=np.float32)
    x[..., :3] *= rng.choice(np.array([1.0, 1.0, 0.05, 3.0, 40.0], np.float32), size=(h, w, 3))
    x[rng.random((h, w)) < 0.02] = -0.25
    return np.ascontiguousarray(x)


def _export_footprint(src, w, h, backend, dtype, patterns, export, expected):
    import torch
    source = torch.from_numpy(src).cuda() if backend == "device" else src
    for off in range(4):                                     # bytes (rgb8) / elements (rgb16) past a 4-element boundary
        half = bool(off & 1)
        left = np.ones(h * w * 3, bool)
        for pattern in patterns:
            g = Guarded(h * w * 3, dtype, pattern, 4096 + 16, backend, offset=off)
            assert g.address() % (4 * g.dtype.itemsize) == off * g.dtype.itemsize
            export(source, w, h, out=g.payload((h, w, 3)), through_half=half)
            assert g.guards_intact(), (w, h, off, backend, g.guard_hits())                                    # (a)
            assert np.array_equal(g.values((h, w, 3)), expected(src, half)), (w, h, off, backend)            # (c)
            left &= g.still_pattern()
        # (b): a byte that holds the pattern under BOTH fills was never stored (a stored byte can equal one fill, not two)
        assert not left.any(), (w, h, off, backend, int(left.sum()))


@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("w", [1, 3, 4, 5, 61, 64])
def test_export_rgb8_footprint(fr, renderer, oracle, w, backend):
    """the four-pixel and the one-pixel form and their tails all end a buffer; output views 0..3 bytes past a dword"""
    rng = np.random.default_rng(80 + w)
    for h in (1, 5, 37):
        _export_footprint(_export_source(rng, h, w), w, h, backend, np.uint8, (0xA5, 0x5A), renderer.export_rgb8,
                          lambda s, half: oracle.export_rgb8(s, through_half=half))


@pytest.mark.parametrize("backend", ["device", "host"])
@pytest.mark.parametrize("w", [1, 3, 4, 5, 61, 64])
def test_export_rgb16_footprint(fr, renderer, w, backend):
    def expected(s, half):                                   # test_export_rgb16's expression (src/vk_engine.cpp:2058-2069)
        c = s[::-1, :, :3].astype(np.float16).astype(np.float32) if half else s[::-1, :, :3]
        return (np.clip(c, 0.0, 1.0) * np.float32(65535.0)).astype(np.uint16)

    rng = np.random.default_rng(160 + w)
    for h in (1, 5, 37):
        src = _export_source(rng, h, w)
        src[..., :3] = np.minimum(src[..., :3], np.float32(60000.0))            # inside fp16's range for the rounding
        _export_footprint(src, w, h, backend, np.uint16, (0xA5A5, 0x5A5A), renderer.export_rgb16, expected)


@pytest.mark.parametrize("geom", LAYOUT_GEOMS, ids=_gid)
@_by_path(["mandel_staging1", "julia_f32"])
def test_colorize_footprint(fr, renderer, oracle, name, geom):
    """fr_colorize_async with n no multiple of the block size: guarded rgba, against oracle.colorize and bit-equal to the
    colour the render itself stored"""
    path = _paths()[name]
    import torch
    W, H = geom
    gp = _render_packed(fr, renderer, oracle, path, W, H, planes=("rgba", "nu"))
    st, ft, prec = path._args(fr)
    assert renderer.colorize_supported(st, ft, prec)
    again = GuardedPlanes(H, W, f64=path.f64, backend="device", planes=("rgba",))
    renderer.colorize(st, gp["nu"].payload(), again["rgba"].payload(), fractal_type=ft, precision=prec)
    torch.cuda.synchronize()
    assert again.guards_intact(), again.guard_hits()
    assert again.unwritten() == 0
    assert np.array_equal(again["rgba"].payload_bits(), gp["rgba"].payload_bits())
    ref = oracle.colorize(path.p, gp.values()[1].astype(np.float64))
    assert np.abs(again.values()[0] - ref).max() <= PARITY_RGB_TOL
