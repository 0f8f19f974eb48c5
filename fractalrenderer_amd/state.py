"""Host-side mirror of the reference's viewport type for the hot path.

FractalState / FractalType / Presets follow src/fractal_state.h (same field names,
same defaults), restricted to the fields the Mandelbrot and Julia compute path reads
(the union packed by ComputeEffect::update_from_state, src/compute_effect_manager.h:84-140).
"""
from __future__ import annotations

import enum
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np

from . import _capi


class FractalType(enum.IntEnum):
    """src/fractal_state.h:6-14.  Mandelbrot and JuliaSet are the hot path; BurningShip and Deep_Zoom are
    its variants (section 8 f1/f4).  Phoenix renders through Renderer.render_phoenix (fr_render_phoenix: its p, r and
    Julia-mode flag travel in PhoenixParams, which fr_params has no room for); Renderer.render and the other fr_params
    entry points reject it with FR_ERR_UNSUPPORTED, as they reject Mandelbulb, which renders through
    Renderer.render_mandelbulb (fr_render_mandelbulb, with MandelbulbParams)."""
    Mandelbrot = 0
    JuliaSet = 1
    BurningShip = 2
    Mandelbulb = 3
    Phoenix = 4
    Deep_Zoom = 5


class Precision(enum.IntEnum):
    F32 = _capi.FR_PRECISION_F32   # what the reference's shaders compute in
    F64 = _capi.FR_PRECISION_F64


_F32 = lambda v: float(np.float32(v))  # noqa: E731  (the reference stores these as float)


@dataclass
class FractalState:
    """src/fractal_state.h:16-91 (hot-path fields, reference defaults)."""
    center_x: float = -0.5                      # :18
    center_y: float = 0.0                       # :19
    zoom: float = 3.0                           # :20
    max_iterations: int = 256                   # :21
    julia_c_real: float = _F32(-0.7)            # :29
    julia_c_imag: float = _F32(0.27015)         # :30
    bailout: float = 4.0                        # :36
    antialiasing_samples: int = 1               # :37
    palette_mode: int = 0                       # :40
    color_offset: float = 0.0                   # :41
    color_scale: float = 1.0                    # :42
    interior_style: int = 0                     # :47
    orbit_trap_enabled: bool = False            # :48
    orbit_trap_radius: float = 0.5              # :49
    stripe_enabled: bool = False                # :50
    stripe_density: float = 10.0                # :51
    color_brightness: float = 1.0               # :77
    color_saturation: float = 1.0               # :78
    color_contrast: float = 1.0                 # :79
    use_perturbation: bool = False              # :86  (Deep_Zoom: compute and use the fp64 reference orbit)

    def reset(self) -> None:
        """FractalState::reset(), src/fractal_state.h:135-153 (note zoom 1.5, not 3.0)."""
        self.center_x, self.center_y, self.zoom, self.max_iterations = -0.5, 0.0, 1.5, 256
        self.color_brightness = self.color_saturation = self.color_contrast = 1.0

    # -- C ABI conversion ---------------------------------------------------------------
    def to_params(self, fractal_type: FractalType = FractalType.Mandelbrot,
                  precision: Precision = Precision.F64, post_chain: bool = False) -> _capi.fr_params:
        p = _capi.fr_params()
        p.fractal_type = int(fractal_type)
        p.precision = int(precision)
        for f in fields(self):
            v = getattr(self, f.name)
            setattr(p, f.name, int(v) if isinstance(v, bool) else v)
        p.flags = _capi.FR_FLAG_POST_CHAIN if post_chain else 0
        return p

    @classmethod
    def from_params(cls, p: _capi.fr_params) -> "FractalState":
        kw = {}
        for f in fields(cls):
            v = getattr(p, f.name)
            kw[f.name] = bool(v) if f.type == "bool" else v
        return cls(**kw)


@dataclass(frozen=True)
class Preset:
    name: str
    type: FractalType
    center_x: float
    center_y: float
    zoom: float
    iterations: int


# Presets::MANDELBROT_PRESETS, src/fractal_state.h:171-180
MANDELBROT_PRESETS = (
    Preset("Overview", FractalType.Mandelbrot, -0.5, 0.0, 2.5, 256),
    Preset("Seahorse Valley", FractalType.Mandelbrot, -0.743643887037151, 0.13182590420533, 0.008, 1024),
    Preset("Elephant Valley", FractalType.Mandelbrot, 0.257, 0.0, 0.015, 768),
    Preset("Triple Spiral", FractalType.Mandelbrot, -0.088, 0.654, 0.02, 512),
    Preset("Mini Mandelbrot", FractalType.Mandelbrot, -1.7497, 0.00001, 0.0005, 1024),
    Preset("Spiral Galaxy", FractalType.Mandelbrot, -0.7453, 0.1127, 0.01, 768),
)

# DeepZoomPresets::createSeahorseZoom, src/deep_zoom_system.cpp:576-583 (the C4 benchmark view)
SEAHORSE_DEEP = Preset("Seahorse deep", FractalType.Mandelbrot, -0.743643887037151, 0.13182590420533, 1e-6, 16384)


def pack_push_constants(state: FractalState, fractal_type: FractalType) -> np.ndarray:
    """ComputeEffect::update_from_state (src/compute_effect_manager.h:84-140): the 80-byte
    ComputePushConstants block as 20 float32."""
    out = (_capi.C.c_float * 20)()
    p = state.to_params(fractal_type)
    _capi.check(_capi.lib().fr_pack_push_constants(_capi.C.byref(p), out))
    return np.array(out[:], dtype=np.float32)


@dataclass
class PhoenixParams:
    """FractalState's Phoenix fields, src/fractal_state.h:82-84 (fr_phoenix_params).  p and r are float in the reference."""
    phoenix_p: float = 0.0                      # :82  damping
    phoenix_r: float = -0.5                     # :83  feedback / memory
    use_julia_set: bool = False                 # :84  C = julia_c for every pixel (which still starts from z = 0)

    def to_c(self) -> _capi.fr_phoenix_params:
        return _capi.fr_phoenix_params(_F32(self.phoenix_p), _F32(self.phoenix_r), int(self.use_julia_set), 0)


# the preset buttons of UIManager::draw_phoenix_controls, src/ui_manager.cpp:1405-1409: name -> PhoenixParams
PHOENIX_PRESETS = {
    "Classic Phoenix": PhoenixParams(_F32(0.0), _F32(-0.5)),
    "Swirl": PhoenixParams(_F32(0.2), _F32(-0.3)),
    "Tendrils": PhoenixParams(_F32(-0.1), _F32(-0.8)),
    "Chaos": PhoenixParams(_F32(0.3), _F32(-0.6)),
}


def pack_push_constants_phoenix(state: FractalState, phoenix: PhoenixParams = None) -> np.ndarray:
    """ComputeEffect::update_from_state, Phoenix case (src/compute_effect_manager.h:201-224): 20 float32."""
    out = (_capi.C.c_float * 20)()
    p = state.to_params(FractalType.Phoenix)
    ph = (phoenix or PhoenixParams()).to_c()
    _capi.check(_capi.lib().fr_pack_push_constants_phoenix(_capi.C.byref(p), _capi.C.byref(ph), out))
    return np.array(out[:], dtype=np.float32)


@dataclass
class MandelbulbParams:
    """FractalState's 3-D fields, src/fractal_state.h:24-26,33,68, and the frame time (fr_mandelbulb_params).  The
    shader animates with `time` (ImGui::GetTime(), src/vk_engine.cpp:336): the caller supplies it."""
    camera_distance: float = 3.0                # :24
    rotation_y: float = 0.0                     # :25  radians
    fov: float = 1.0                            # :26
    mandelbulb_power: float = 8.0               # :33
    rotation_speed: float = 0.5                 # :68  (0 means 0.3 in the shader)
    time: float = 0.0                           # seconds

    def to_c(self) -> _capi.fr_mandelbulb_params:
        return _capi.fr_mandelbulb_params(_F32(self.camera_distance), _F32(self.rotation_y), _F32(self.fov),
                                          _F32(self.mandelbulb_power), _F32(self.rotation_speed), _F32(self.time))


# UIManager's Mandelbulb buttons: the power presets (src/ui_manager.cpp:1319-1324) and the views (:1476-1480) as
# name -> MandelbulbParams (the other fields keep their defaults)
MANDELBULB_PRESETS = {
    "Classic (8)": MandelbulbParams(mandelbulb_power=8.0),
    "Smooth (4)": MandelbulbParams(mandelbulb_power=4.0),
    "Spiky (12)": MandelbulbParams(mandelbulb_power=12.0),
    "Extreme (16)": MandelbulbParams(mandelbulb_power=16.0),
    "Front View": MandelbulbParams(camera_distance=3.0, rotation_y=0.0, mandelbulb_power=8.0),
    "Side View": MandelbulbParams(camera_distance=3.0, rotation_y=_F32(1.5708), mandelbulb_power=8.0),
    "Close-up Detail": MandelbulbParams(camera_distance=1.5, rotation_y=_F32(0.785), mandelbulb_power=8.0),
}


def pack_push_constants_mandelbulb(state: FractalState, mandelbulb: MandelbulbParams = None) -> np.ndarray:
    """ComputeEffect::update_from_state, Mandelbulb case (src/compute_effect_manager.h:173-199): 20 float32."""
    out = (_capi.C.c_float * 20)()
    p = state.to_params(FractalType.Mandelbulb, Precision.F32)
    mb = (mandelbulb or MandelbulbParams()).to_c()
    _capi.check(_capi.lib().fr_pack_push_constants_mandelbulb(_capi.C.byref(p), _capi.C.byref(mb), out))
    return np.array(out[:], dtype=np.float32)


@dataclass(frozen=True)
class DeepView:
    """The centre of a view deeper than double precision (fr_deep_view): decimal strings, [+-]digits[.digits][(e|E)[+-]digits]
    of at most 4096 characters, or Decimals (written out with str()).  frac_bits: fraction bits of the host's fixed-point
    reference orbit, 0 = automatic (deep_frac_bits(zoom)).  The zoom is FractalState.zoom; its centre is not read.
    zoom: None, or the view height as a decimal string (or Decimal) in [1e-1000, 1e3] -- then the view is an fr_deepx_view,
    rendered with extended-exponent deltas (fr_render_deepx, fr_render_deepx_ship), and FractalState.zoom is not read either."""
    center_x: object = "-0.5"
    center_y: object = "0"
    frac_bits: int = 0
    zoom: object = None

    def to_c(self) -> _capi.fr_deep_view:
        return _capi.fr_deep_view(str(self.center_x).encode("ascii"), str(self.center_y).encode("ascii"),
                                  int(self.frac_bits), 0)

    def to_cx(self) -> _capi.fr_deepx_view:
        return _capi.fr_deepx_view(str(self.center_x).encode("ascii"), str(self.center_y).encode("ascii"),
                                   str(self.zoom).encode("ascii"), int(self.frac_bits), 0)


def deep_frac_bits(zoom: float) -> int:
    """fr_deep_frac_bits: the automatic fraction bits of a deep view at this zoom."""
    n = int(_capi.lib().fr_deep_frac_bits(float(zoom)))
    _capi.check(min(n, 0))
    return n


def deep_reference_orbit(view: DeepView, zoom: float, max_iterations: int, bailout: float = 4.0) -> np.ndarray:
    """fr_deep_reference_orbit: Z_0 .. Z_N of the view as an (N + 1, 2) float64 array (host only)."""
    buf = np.empty((int(max_iterations) + 1, 2), np.float64)
    n = _capi.C.c_int32()
    v = view.to_c()
    _capi.check(_capi.lib().fr_deep_reference_orbit(_capi.C.byref(v), float(zoom), int(max_iterations), _F32(bailout),
                                                    buf.ctypes.data, _capi.C.byref(n)))
    return buf[:n.value].copy()


def deep_ship_reference_orbit(view: DeepView, zoom: float, max_iterations: int, bailout: float = 4.0) -> np.ndarray:
    """fr_deep_ship_reference_orbit: Z_0 .. Z_N of the Burning Ship recurrence at the view's centre, as deep_reference_orbit."""
    buf = np.empty((int(max_iterations) + 1, 2), np.float64)
    n = _capi.C.c_int32()
    v = view.to_c()
    _capi.check(_capi.lib().fr_deep_ship_reference_orbit(_capi.C.byref(v), float(zoom), int(max_iterations), _F32(bailout),
                                                         buf.ctypes.data, _capi.C.byref(n)))
    return buf[:n.value].copy()


def deep_phoenix_reference_orbit(view: DeepView, zoom: float, max_iterations: int,
                                 phoenix: Optional[PhoenixParams] = None) -> np.ndarray:
    """fr_deep_phoenix_reference_orbit: Z_0 .. Z_N of z' = z^2 + c + r z_prev + p z at the view's centre (the shader's fixed
    bailout 2), as deep_reference_orbit; `phoenix` carries p and r (default: the reference's initialisers)."""
    buf = np.empty((int(max_iterations) + 1, 2), np.float64)
    n = _capi.C.c_int32()
    v = view.to_c()
    ph = (phoenix or PhoenixParams()).to_c()
    _capi.check(_capi.lib().fr_deep_phoenix_reference_orbit(_capi.C.byref(v), _capi.C.byref(ph), float(zoom), int(max_iterations),
                                                            buf.ctypes.data, _capi.C.byref(n)))
    return buf[:n.value].copy()


def deepx_zoom(zoom) -> tuple:
    """fr_deepx_zoom: a decimal zoom string as (zm, ze), zoom = zm 2^ze, zm in [1, 2) correctly rounded."""
    zm, ze = _capi.C.c_double(), _capi.C.c_int32()
    _capi.check(_capi.lib().fr_deepx_zoom(str(zoom).encode("ascii"), _capi.C.byref(zm), _capi.C.byref(ze)))
    return zm.value, ze.value


def deepx_frac_bits(zoom) -> int:
    """fr_deepx_frac_bits: the automatic fraction bits of an extended view at this zoom (a decimal string)."""
    n = int(_capi.lib().fr_deepx_frac_bits(str(zoom).encode("ascii")))
    _capi.check(min(n, 0))
    return n


def deepx_reference_orbit(view: DeepView, max_iterations: int, bailout: float = 4.0) -> tuple:
    """fr_deepx_reference_orbit: Z_0 .. Z_N of an extended view (view.zoom set) as ((N + 1, 2) float64 mantissas,
    (N + 1,) int32 exponents): point n is mantissas[n] * 2^exponents[n] (host only)."""
    mant = np.empty((int(max_iterations) + 1, 2), np.float64)
    exp2 = np.empty(int(max_iterations) + 1, np.int32)
    n = _capi.C.c_int32()
    v = view.to_cx()
    _capi.check(_capi.lib().fr_deepx_reference_orbit(_capi.C.byref(v), int(max_iterations), _F32(bailout), mant.ctypes.data,
                                                     exp2.ctypes.data, _capi.C.byref(n)))
    return mant[:n.value].copy(), exp2[:n.value].copy()


def deepx_ship_reference_orbit(view: DeepView, max_iterations: int, bailout: float = 4.0) -> tuple:
    """fr_deepx_ship_reference_orbit: deepx_reference_orbit for the Burning Ship recurrence (points signed)."""
    mant = np.empty((int(max_iterations) + 1, 2), np.float64)
    exp2 = np.empty(int(max_iterations) + 1, np.int32)
    n = _capi.C.c_int32()
    v = view.to_cx()
    _capi.check(_capi.lib().fr_deepx_ship_reference_orbit(_capi.C.byref(v), int(max_iterations), _F32(bailout), mant.ctypes.data,
                                                          exp2.ctypes.data, _capi.C.byref(n)))
    return mant[:n.value].copy(), exp2[:n.value].copy()


def deepx_phoenix_reference_orbit(view: DeepView, max_iterations: int, phoenix: Optional[PhoenixParams] = None) -> tuple:
    """fr_deepx_phoenix_reference_orbit: deep_phoenix_reference_orbit's orbit of a view with a zoom string, in the extended
    storage: (mant, exp2) as deepx_reference_orbit returns them."""
    mant = np.empty((int(max_iterations) + 1, 2), np.float64)
    exp2 = np.empty(int(max_iterations) + 1, np.int32)
    n = _capi.C.c_int32()
    v = view.to_cx()
    ph = (phoenix or PhoenixParams()).to_c()
    _capi.check(_capi.lib().fr_deepx_phoenix_reference_orbit(_capi.C.byref(v), _capi.C.byref(ph), int(max_iterations),
                                                             mant.ctypes.data, exp2.ctypes.data, _capi.C.byref(n)))
    return mant[:n.value].copy(), exp2[:n.value].copy()


def deep_julia_reference_orbits(view: DeepView, c, max_iterations: int, bailout: float = 4.0, zoom: float = 1.0) -> tuple:
    """fr_deep_julia_reference_orbits / fr_deepx_julia_reference_orbits: the two orbits of a deep Julia view (host only).
    c = (c_re, c_im), doubles.  P starts at the view's centre, Q at 0.  A view without a zoom string gives
    (P, Q) as (N_P + 1, 2) and (N_Q + 1, 2) float64 arrays, F taken from `zoom`; a view with one gives the extended storage,
    ((P mantissas, P exponents), (Q mantissas, Q exponents)) as deepx_reference_orbit does, and `zoom` is not read."""
    n = int(max_iterations) + 1
    np_, nq = _capi.C.c_int32(), _capi.C.c_int32()
    pm, qm = np.empty((n, 2), np.float64), np.empty((n, 2), np.float64)
    if view.zoom is None:
        v = view.to_c()
        _capi.check(_capi.lib().fr_deep_julia_reference_orbits(_capi.C.byref(v), float(c[0]), float(c[1]), float(zoom),
                                                               int(max_iterations), _F32(bailout), pm.ctypes.data,
                                                               _capi.C.byref(np_), qm.ctypes.data, _capi.C.byref(nq)))
        return pm[:np_.value].copy(), qm[:nq.value].copy()
    pe, qe = np.empty(n, np.int32), np.empty(n, np.int32)
    vx = view.to_cx()
    _capi.check(_capi.lib().fr_deepx_julia_reference_orbits(_capi.C.byref(vx), float(c[0]), float(c[1]), int(max_iterations),
                                                            _F32(bailout), pm.ctypes.data, pe.ctypes.data, _capi.C.byref(np_),
                                                            qm.ctypes.data, qe.ctypes.data, _capi.C.byref(nq)))
    return (pm[:np_.value].copy(), pe[:np_.value].copy()), (qm[:nq.value].copy(), qe[:nq.value].copy())
