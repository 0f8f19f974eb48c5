"""Renderer: the Python face of the C-ABI render entry points.

Mirrors the reference's compute boundary for the hot path:
  ComputeEffectManager::dispatch(cmd, type, state, time, desc_set, extent)
      src/compute_effect_manager.h:435-468
  AnimationRenderer::RenderFrameCallback  bool(const FractalState&, width, height, path)
      src/animation_renderer.h:41-48
PyTorch is used only for device memory and streams; every pixel is computed by the HIP
kernels behind libfractalrenderer_amd.so.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np

from . import _capi
from .state import DeepView, FractalState, FractalType, MandelbulbParams, PhoenixParams, Precision


DEEP_DE_EDGE_PX = 1.8     # fr_deep_de_default's edge_px: 0.005 c-plane units at zoom 3.0 on 1080 rows


class DeepSteps(NamedTuple):
    """fr_ctx_last_deep_steps: the steps of a deep render with BLA"""
    plain: int          # plain perturbation steps
    bla: int            # BLA steps
    skipped: int        # updates the BLA steps stood for (sum of 2^k)


@dataclass(frozen=True)
class Shard:
    """Row-strip sharding of one frame (fr_shard): strips of rows_per_strip rows dealt
    round-robin to nparts parts; this part renders only its own strips, packed."""
    part: int = 0
    nparts: int = 1
    rows_per_strip: int = 0

    def to_c(self) -> _capi.fr_shard:
        return _capi.fr_shard(self.part, self.nparts, self.rows_per_strip)

    def rows(self, height: int) -> int:
        s = self.to_c()
        return int(_capi.lib().fr_shard_rows(C.byref(s), height))

    def global_rows(self, height: int) -> np.ndarray:
        """frame row index of every packed local row of this part"""
        s = self.to_c()
        n = self.rows(height)
        L = _capi.lib()
        return np.array([L.fr_shard_global_row(C.byref(s), height, r) for r in range(n)], dtype=np.int64)


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


class Renderer:
    """One fr_ctx bound to one HIP device."""

    def __init__(self, device: int = 0, timing: bool = True):
        """timing: option "timing" -- the event pair around every render that last_kernel_ms() reads.  The C library's
        default is OFF (two timed event records cost a frame ~4.7 us); this wrapper, which tests and tools measure with,
        switches it on unless told otherwise (bench.py's timed contexts are told otherwise)."""
        self._lib = _capi.lib()
        h = C.c_void_p()
        _capi.check(self._lib.fr_ctx_create(int(device), C.byref(h)))
        self._ctx = h
        self.device = int(device)
        if timing:
            self.set_option("timing", 1)

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.fr_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def compute_units(self) -> int:
        return _capi.check(self._lib.fr_ctx_compute_units(self._ctx))

    def set_option(self, name: str, value: int) -> None:
        """fr_ctx_set_option (the public names), or fr_ctx_set_tuning for the internal queue / stream tuning names of
        csrc/fr_tuning.h (tests, tools, A/B measurements); 0 = automatic."""
        if name in _capi.TUNING_NAMES:
            _capi.check(self._lib.fr_ctx_set_tuning(self._ctx, name.encode(), int(value)))
        else:
            _capi.check(self._lib.fr_ctx_set_option(self._ctx, name.encode(), int(value)))

    def set_tuning(self, workgroups_per_cu: int = 0, subtiles_per_dequeue: int = 0, shape: int = 0,
                   run_min: int = 0, shift_bias: int = 0) -> None:
        """All queue knobs at once; 0 = automatic everywhere (see fr_ctx_set_option)."""
        for k, v in (("workgroups_per_cu", workgroups_per_cu), ("run_max", subtiles_per_dequeue),
                     ("subtile_shape", shape), ("run_min", run_min), ("shift_bias", shift_bias)):
            self.set_option(k, v)

    def reserve(self, state: FractalState, width: int, height: int, *, fractal_type: FractalType = FractalType.Mandelbrot,
                precision: Precision = Precision.F64, shard: Optional[Shard] = None) -> None:
        """fr_ctx_reserve: size the context's scratch for this geometry now, so that later sync=False renders of it
        (or of anything smaller) are launch-only."""
        p = state.to_params(fractal_type, precision)
        sh = shard.to_c() if shard else None
        _capi.check(self._lib.fr_ctx_reserve(self._ctx, C.byref(p), width, height, C.byref(sh) if sh is not None else None))

    def check(self) -> None:
        """fr_ctx_check: raises if a render that completed on this context lost pixels (after the caller's own sync)."""
        _capi.check(self._lib.fr_ctx_check(self._ctx))

    def last_grid(self) -> int:
        return _capi.check(self._lib.fr_ctx_last_grid(self._ctx)) & 0xFFFF

    def last_stages(self) -> int:
        return _capi.check(self._lib.fr_ctx_last_grid(self._ctx)) >> 16

    def _last_steps(self, symbol: str) -> DeepSteps:
        """the three counters behind one of the fr_ctx_last_*_steps entry points"""
        out = (C.c_uint64 * 3)()
        _capi.check(getattr(self._lib, symbol)(self._ctx, out))
        return DeepSteps(int(out[0]), int(out[1]), int(out[2]))

    def last_deep_steps(self) -> DeepSteps:
        """fr_ctx_last_deep_steps: (plain steps, BLA steps, updates skipped) of the most recent render_deep(bla=True) on
        this context, over every sub-sample of its pixels (after the caller's own sync for sync=False)."""
        return self._last_steps("fr_ctx_last_deep_steps")

    def last_deepx_steps(self) -> DeepSteps:
        """fr_ctx_last_deepx_steps: (single steps of both modes, BLA steps, updates skipped) of the most recent
        render_deep(xbla=True) on this context, as last_deep_steps()."""
        return self._last_steps("fr_ctx_last_deepx_steps")

    def last_deep_ship_steps(self) -> DeepSteps:
        """fr_ctx_last_deep_ship_steps: (plain steps, BLA steps, updates skipped) of the most recent
        render_deep_ship(bla=True) on this context, as last_deep_steps()."""
        return self._last_steps("fr_ctx_last_deep_ship_steps")

    def last_deep_phoenix_steps(self) -> DeepSteps:
        """fr_ctx_last_deep_phoenix_steps: (plain steps, BLA steps, updates skipped) of the most recent
        render_deep_phoenix(bla=True) on this context, as last_deep_steps()."""
        return self._last_steps("fr_ctx_last_deep_phoenix_steps")

    def last_deepx_phoenix_steps(self) -> DeepSteps:
        """fr_ctx_last_deepx_phoenix_steps: (single steps of both modes, BLA steps, updates skipped) of the most recent
        render_deepx_phoenix(xbla=True) on this context, as last_deep_steps()."""
        return self._last_steps("fr_ctx_last_deepx_phoenix_steps")

    def last_deepx_ship_steps(self) -> DeepSteps:
        """fr_ctx_last_deepx_ship_steps: (single steps of both modes, BLA steps, updates skipped) of the most recent
        render_deepx_ship(bla=True) or ship-sequence render with bla=True on this context, as last_deep_steps()."""
        return self._last_steps("fr_ctx_last_deepx_ship_steps")

    def last_deep_julia_steps(self) -> DeepSteps:
        """fr_ctx_last_deep_julia_steps: (single steps, BLA steps, updates skipped) of the most recent render_deep_julia(bla=True)
        of a view without a zoom string on this context, both orbits counted together, as last_deep_steps()."""
        return self._last_steps("fr_ctx_last_deep_julia_steps")

    def last_deepx_julia_steps(self) -> DeepSteps:
        """fr_ctx_last_deepx_julia_steps: the same for the most recent render_deep_julia(bla=True) of a view with a zoom
        string (single steps of both modes)."""
        return self._last_steps("fr_ctx_last_deepx_julia_steps")

    def last_kernel_ms(self) -> float:
        return float(self._lib.fr_ctx_last_kernel_ms(self._ctx))

    def last_pool_closing(self) -> int:
        """internal (fr_tuning.h): 1 / 0 = the lane pool of the most recent render looked / did not look for cycles, -1 = none"""
        return int(self._lib.fr_ctx_last_pool_closing(self._ctx))

    def last_whole_blocks(self) -> tuple[int, int, int]:
        """internal (fr_tuning.h): of the most recent render's survivor stream (waits for it) -- whole blocks written, whole
        blocks that turned dirty in the lane pool, records that went through the ring; zeros where it kept one class"""
        out = (C.c_uint64 * 3)()
        _capi.check(self._lib.fr_ctx_last_whole_blocks(self._ctx, out))
        return int(out[0]), int(out[1]), int(out[2])

    def last_fold(self) -> int:
        """internal (fr_tuning.h): rows the most recent render rendered as a folded render (a Mandelbrot frame with
        center_y == 0: the rows below the real axis are mirrored stores), 0 where it rendered every row itself"""
        return int(self._lib.fr_ctx_last_fold(self._ctx))

    # -- plane plumbing ------------------------------------------------------------------
    @staticmethod
    def _ptr(x, want_dtype: str, nelem: int, what: str):
        if x is None:
            return None, None
        if _is_torch(x):
            if not x.is_contiguous():
                raise ValueError(f"{what}: tensor must be contiguous")
            if str(x.dtype).replace("torch.", "") != want_dtype:
                raise ValueError(f"{what}: dtype {x.dtype}, expected {want_dtype}")
            if x.numel() != nelem:
                raise ValueError(f"{what}: {x.numel()} elements, expected {nelem}")
            return x.data_ptr(), ("device" if x.is_cuda else "host")
        a = x
        if not isinstance(a, np.ndarray) or not a.flags["C_CONTIGUOUS"]:
            raise ValueError(f"{what}: need a C-contiguous numpy array or torch tensor")
        if a.dtype != np.dtype(want_dtype):
            raise ValueError(f"{what}: dtype {a.dtype}, expected {want_dtype}")
        if a.size != nelem:
            raise ValueError(f"{what}: {a.size} elements, expected {nelem}")
        return a.ctypes.data, "host"

    def _output(self, precision: Precision, rows: int, width: int, rgba, nu, it, extra=()) -> _capi.fr_output:
        # (also called with self = None by Node.render: uses nothing of the instance)
        # extra: planes beyond fr_output's three as (struct, field, array, dtype, elements per pixel); their pointers go into the
        # struct's field and their memory kind has to be that of the others
        npx = rows * width
        nu_dtype = "float64" if precision == Precision.F64 else "float32"   # Deep_Zoom callers pass Precision.F32
        kinds = set()
        o = _capi.fr_output()
        planes = [(o, "rgba", rgba, "float32", 4), (o, "nu", nu, nu_dtype, 1), (o, "iter", it, "int32", 1)]
        for struct, name, x, dt, per_px in planes + list(extra):
            p, kind = Renderer._ptr(x, dt, npx * per_px, name)
            setattr(struct, name, p)
            if kind:
                kinds.add(kind)
        if len(kinds) > 1:
            raise ValueError("output planes must all be host or all be device memory")
        o.memory = _capi.FR_MEM_DEVICE if kinds == {"device"} else _capi.FR_MEM_HOST
        return o

    # -- render ----------------------------------------------------------------------------
    def render(self, state: FractalState, width: int, height: int, *,
               fractal_type: FractalType = FractalType.Mandelbrot,
               precision: Precision = Precision.F64, post_chain: bool = False,
               rgba=None, nu=None, iter=None, shard: Optional[Shard] = None,
               stream: Optional[int] = None, sync: bool = True) -> None:
        """The reference's render(viewport, max_iter, out_buffer) surface.

        rgba: rows*W*4 float32, nu: rows*W float64 (F64) / float32 (F32), iter: rows*W int32;
        numpy arrays (host, PCIe-inclusive path) or torch CUDA tensors (device, no copies).
        sync=False enqueues on `stream` (a raw hipStream_t handle, e.g.
        torch.cuda.current_stream().cuda_stream) and returns at once (device planes only).
        """
        p = state.to_params(fractal_type, precision, post_chain)
        rows = shard.rows(height) if shard else height
        if rows == 0:
            _capi.check(self._lib.fr_params_validate(C.byref(p), width, height))
            return                                   # this part owns no rows of the frame
        self._render_call(self._lib.fr_render_shard, self._lib.fr_render_shard_async, (C.byref(p),), width, height,
                          precision, rows, rgba, nu, iter, shard, stream, sync)

    def render_phoenix(self, state: FractalState, width: int, height: int, phoenix: Optional[PhoenixParams] = None, *,
                       precision: Precision = Precision.F32, post_chain: bool = False,
                       rgba=None, nu=None, iter=None, shard: Optional[Shard] = None,
                       stream: Optional[int] = None, sync: bool = True) -> None:
        """fr_render_phoenix / fr_render_phoenix_async: a frame of shaders/phoenix.comp.  `phoenix` carries FractalState's
        phoenix_p, phoenix_r and use_julia_set (default: the reference's initialisers, the "Classic Phoenix" preset).
        Planes, shard, stream and sync as for render(); precision defaults to F32, what the shader computes in."""
        p = state.to_params(FractalType.Phoenix, precision, post_chain)
        ph = (phoenix or PhoenixParams()).to_c()
        rows = shard.rows(height) if shard else height
        self._render_call(self._lib.fr_render_phoenix, self._lib.fr_render_phoenix_async, (C.byref(p), C.byref(ph)), width,
                          height, precision, rows, rgba, nu, iter, shard, stream, sync)

    def render_mandelbulb(self, state: FractalState, width: int, height: int, mandelbulb: Optional[MandelbulbParams] = None,
                          *, post_chain: bool = False, rgba=None, nu=None, iter=None, shard: Optional[Shard] = None,
                          stream: Optional[int] = None, sync: bool = True) -> None:
        """fr_render_mandelbulb / fr_render_mandelbulb_async: a frame of shaders/mandelbulb.comp, in fp32 (the only
        precision).  `mandelbulb` carries the camera, the power and the frame time (default: FractalState's initialisers,
        time 0).  rgba: the linear colour (NaN where the shader's is, see the header) or, with post_chain, the shader's
        output; nu (float32): sample (0,0)'s ray parameter t where its march stopped; iter: its hit step, -1 for a miss.
        Planes, shard, stream and sync as for render()."""
        p = state.to_params(FractalType.Mandelbulb, Precision.F32, post_chain)
        mb = (mandelbulb or MandelbulbParams()).to_c()
        rows = shard.rows(height) if shard else height
        self._render_call(self._lib.fr_render_mandelbulb, self._lib.fr_render_mandelbulb_async, (C.byref(p), C.byref(mb)),
                          width, height, Precision.F32, rows, rgba, nu, iter, shard, stream, sync)

    def render_deep(self, state: FractalState, width: int, height: int, view: Optional[DeepView] = None, *,
                    post_chain: bool = False, rgba=None, nu=None, iter=None, shard: Optional[Shard] = None,
                    stream: Optional[int] = None, sync: bool = True, bla: bool = False, xbla: bool = False) -> None:
        """fr_render_deep / fr_render_deep_async: a Mandelbrot view deeper than double precision, by perturbation around one
        reference orbit computed on the host.  `view` carries the centre as decimal strings (default: "-0.5", "0"); the
        zoom and every other field come from `state` (its double centre is not read).  Always fp64: nu is float64.
        Planes, shard, stream and sync as for render().  A new view computes its orbit on the host first, also with
        sync=False; a render of the view the context holds is launch-only.  bla=True sets FR_FLAG_DEEP_BLA: iteration
        skipping by bilinear approximation (the header's rules; last_deep_steps() reports what it skipped).
        A view with a zoom string (DeepView(..., zoom="1e-400")) goes to fr_render_deepx / fr_render_deepx_async:
        extended-exponent deltas, zooms down to 1e-1000, state.zoom not read.  bla=True raises there (its table is fp64);
        xbla=True sets FR_FLAG_DEEPX_BLA, BLA in the extended arithmetic (last_deepx_steps() reports what it skipped), and
        is a ValueError for a view without a zoom string."""
        if xbla and (view is None or view.zoom is None):
            raise ValueError("xbla=True needs a view with a zoom string (DeepView(..., zoom=\"1e-400\")); bla=True is the "
                             "flag of views without one")
        p = state.to_params(FractalType.Mandelbrot, Precision.F64, post_chain)
        if bla:
            p.flags |= _capi.FR_FLAG_DEEP_BLA
        if xbla:
            p.flags |= _capi.FR_FLAG_DEEPX_BLA
        rows = shard.rows(height) if shard else height
        if view is not None and view.zoom is not None:
            vx = view.to_cx()
            self._render_call(self._lib.fr_render_deepx, self._lib.fr_render_deepx_async, (C.byref(p), C.byref(vx)), width,
                              height, Precision.F64, rows, rgba, nu, iter, shard, stream, sync)
            return
        v = (view or DeepView()).to_c()
        self._render_call(self._lib.fr_render_deep, self._lib.fr_render_deep_async, (C.byref(p), C.byref(v)), width, height,
                          Precision.F64, rows, rgba, nu, iter, shard, stream, sync)

    def render_deep_de(self, state: FractalState, width: int, height: int, view: Optional[DeepView] = None, *,
                       post_chain: bool = False, rgba=None, nu=None, iter=None, de=None, deriv=None, shade: bool = False,
                       edge_px: float = DEEP_DE_EDGE_PX, shard: Optional[Shard] = None, stream: Optional[int] = None,
                       sync: bool = True, bla: bool = False) -> None:
        """fr_render_deep_de / fr_render_deep_de_async: render_deep() with the derivative dz/dc carried through the
        perturbation loop and two planes more.  de: rows*W float64, the exterior distance estimate of sample (0,0) in pixel
        spacings of the whole frame (0 for interior); deriv: rows*W*2 float64, (D.x, D.y) = dz/dc * (zoom / H) at the escaping
        update.  Any one of the five planes is enough; all of them are host or all device memory.  shade=True applies the
        debug shader's distance shading to every escaped sub-sample (edge_px: the smoothstep's upper edge in pixel spacings);
        without it rgba is render_deep()'s.  iter, nu and last_deep_steps() are render_deep()'s, and the context's orbit and
        BLA table are shared with it.  bla=True sets FR_FLAG_DEEP_BLA.  A view with a zoom string is a ValueError: below
        1e-290 the derivative needs an exponent of its own, and render_deepx_de() carries one."""
        if view is not None and view.zoom is not None:
            raise ValueError("render_deep_de takes the zoom from the state: extended views (a zoom string) go to render_deepx_de")
        p = state.to_params(FractalType.Mandelbrot, Precision.F64, post_chain)
        if bla:
            p.flags |= _capi.FR_FLAG_DEEP_BLA
        v = (view or DeepView()).to_c()
        rows = shard.rows(height) if shard else height
        e = _capi.fr_deep_de(None, None, 1 if shade else 0, float(edge_px))
        # (through the class: tests call this method on a stand-in for the renderer that has _lib, _ctx and _output only)
        Renderer._render_call(self, self._lib.fr_render_deep_de, self._lib.fr_render_deep_de_async,
                              (C.byref(p), C.byref(v), C.byref(e)), width, height, Precision.F64, rows, rgba, nu, iter, shard,
                              stream, sync, extra=((e, "de", de, "float64", 1), (e, "deriv", deriv, "float64", 2)))

    def render_deepx_de(self, state: FractalState, width: int, height: int, view: DeepView, *, post_chain: bool = False,
                        rgba=None, nu=None, iter=None, de=None, deriv=None, shade: bool = False,
                        edge_px: float = DEEP_DE_EDGE_PX, shard: Optional[Shard] = None, stream: Optional[int] = None,
                        sync: bool = True, bla: bool = False) -> None:
        """fr_render_deepx_de / fr_render_deepx_de_async: render_deep_de() for a view with a zoom string
        (DeepView(..., zoom="1e-400")), zooms down to 1e-1000: the derivative is carried with an exponent of its own through
        both modes of the extended loop.  A view without a zoom string is a ValueError (render_deep_de() takes those).
        de, deriv, shade and edge_px as for render_deep_de(): de stays finite at any depth, deriv saturates outside a
        double's range.  iter, nu and rgba without shade are render_deep()'s of the same view, and the context's extended
        orbit and table are shared with it.  bla=True sets FR_FLAG_DEEPX_BLA (last_deepx_steps() reports what it skipped)."""
        if view is None or view.zoom is None:
            raise ValueError("render_deepx_de needs a view with a zoom string (DeepView(..., zoom=\"1e-400\")); "
                             "render_deep_de renders views without one")
        p = state.to_params(FractalType.Mandelbrot, Precision.F64, post_chain)
        if bla:
            p.flags |= _capi.FR_FLAG_DEEPX_BLA
        vx = view.to_cx()
        rows = shard.rows(height) if shard else height
        e = _capi.fr_deep_de(None, None, 1 if shade else 0, float(edge_px))
        # (through the class, as render_deep_de)
        Renderer._render_call(self, self._lib.fr_render_deepx_de, self._lib.fr_render_deepx_de_async,
                              (C.byref(p), C.byref(vx), C.byref(e)), width, height, Precision.F64, rows, rgba, nu, iter, shard,
                              stream, sync, extra=((e, "de", de, "float64", 1), (e, "deriv", deriv, "float64", 2)))

    def render_deep_ship(self, state: FractalState, width: int, height: int, view: Optional[DeepView] = None, *,
                         post_chain: bool = False, rgba=None, nu=None, iter=None, shard: Optional[Shard] = None,
                         stream: Optional[int] = None, sync: bool = True, bla: bool = False) -> None:
        """fr_render_deep_ship / fr_render_deep_ship_async: a Burning Ship view deeper than double precision, by perturbation
        around one reference orbit of the ship's recurrence computed on the host.  `view` carries the centre as decimal
        strings (a view with a zoom string is a ValueError: it goes to render_deepx_ship()); the zoom, in
        [1e-290, 1e3], and every other field come from `state` (its double centre is not read).  Always fp64: nu is float64.
        Planes, shard, stream and sync as for render_deep(); the context keeps the ship's orbit next to render_deep's.
        bla=True sets FR_FLAG_DEEP_SHIP_BLA: iteration skipping by bilinear approximation with the ship's real 2x2 maps (the
        header's rules; last_deep_ship_steps() reports what it skipped)."""
        if view is not None and view.zoom is not None:
            raise ValueError("render_deep_ship takes the zoom from the state: extended views (a zoom string) are Mandelbrot only")
        p = state.to_params(FractalType.BurningShip, Precision.F64, post_chain)
        if bla:
            p.flags |= _capi.FR_FLAG_DEEP_SHIP_BLA
        v = (view or DeepView()).to_c()
        rows = shard.rows(height) if shard else height
        self._render_call(self._lib.fr_render_deep_ship, self._lib.fr_render_deep_ship_async, (C.byref(p), C.byref(v)), width,
                          height, Precision.F64, rows, rgba, nu, iter, shard, stream, sync)

    def render_deep_phoenix(self, state: FractalState, width: int, height: int, view: Optional[DeepView] = None,
                            phoenix: Optional[PhoenixParams] = None, *, post_chain: bool = False, rgba=None, nu=None, iter=None,
                            shard: Optional[Shard] = None, stream: Optional[int] = None, sync: bool = True,
                            bla: bool = False) -> None:
        """fr_render_deep_phoenix / fr_render_deep_phoenix_async: a Phoenix view deeper than double precision, by perturbation
        around one reference orbit of the second-order recurrence computed on the host.  `view` carries the centre as decimal
        strings; `phoenix` carries phoenix_p and phoenix_r as for render_phoenix() (use_julia_set must stay off: a Julia-mode
        Phoenix frame is one colour).  The zoom, in [1e-290, 1e3], and every other field come from `state` (its double centre
        is not read).  Always fp64: nu is float64.  Planes, shard, stream and sync as for render_deep_ship(); the context keeps
        the Phoenix orbit in a slot of its own.  A view with a zoom string is a ValueError (render_deepx_phoenix() takes
        those); there is no distance estimate on this path.
        bla=True sets FR_FLAG_DEEP_PHOENIX_BLA: iteration skipping by bilinear approximation on the pair of deltas, with complex
        2x2 maps (the header's rules; last_deep_phoenix_steps() reports what it skipped)."""
        if view is not None and view.zoom is not None:
            raise ValueError("render_deep_phoenix takes the zoom from the state: render_deepx_phoenix renders views with a zoom "
                             "string")
        p = state.to_params(FractalType.Phoenix, Precision.F64, post_chain)
        if bla:
            p.flags |= _capi.FR_FLAG_DEEP_PHOENIX_BLA
        ph = (phoenix or PhoenixParams()).to_c()
        v = (view or DeepView()).to_c()
        rows = shard.rows(height) if shard else height
        self._render_call(self._lib.fr_render_deep_phoenix, self._lib.fr_render_deep_phoenix_async,
                          (C.byref(p), C.byref(ph), C.byref(v)), width, height, Precision.F64, rows, rgba, nu, iter, shard, stream,
                          sync)

    def render_deepx_phoenix(self, state: FractalState, width: int, height: int, view: DeepView,
                             phoenix: Optional[PhoenixParams] = None, *, post_chain: bool = False, rgba=None, nu=None, iter=None,
                             shard: Optional[Shard] = None, stream: Optional[int] = None, sync: bool = True,
                             xbla: bool = False) -> None:
        """fr_render_deepx_phoenix / fr_render_deepx_phoenix_async: a Phoenix view with extended-exponent deltas, zooms down to
        1e-1000.  `view` carries the centre and the zoom as decimal strings (DeepView(..., zoom="1e-400")); a view without a
        zoom string is a ValueError (render_deep_phoenix() takes those).  state.zoom and its double centre are not read;
        `phoenix` and every other argument as for render_deep_phoenix().  The context keeps this path's orbit in a slot of its
        own.  xbla=True sets FR_FLAG_DEEPX_PHOENIX_BLA (the keyword of render_deep()'s extended flag): iteration skipping on the
        pair of deltas with complex 2x2 maps in extended arithmetic (the header's rules; last_deepx_phoenix_steps() reports what
        it skipped)."""
        if view is None or view.zoom is None:
            raise ValueError("render_deepx_phoenix needs a view with a zoom string (DeepView(..., zoom=\"1e-400\")); "
                             "render_deep_phoenix renders views without one")
        p = state.to_params(FractalType.Phoenix, Precision.F64, post_chain)
        if xbla:
            p.flags |= _capi.FR_FLAG_DEEPX_PHOENIX_BLA
        ph = (phoenix or PhoenixParams()).to_c()
        vx = view.to_cx()
        rows = shard.rows(height) if shard else height
        self._render_call(self._lib.fr_render_deepx_phoenix, self._lib.fr_render_deepx_phoenix_async,
                          (C.byref(p), C.byref(ph), C.byref(vx)), width, height, Precision.F64, rows, rgba, nu, iter, shard, stream,
                          sync)

    def render_deepx_ship(self, state: FractalState, width: int, height: int, view: DeepView, *, post_chain: bool = False,
                          rgba=None, nu=None, iter=None, shard: Optional[Shard] = None, stream: Optional[int] = None,
                          sync: bool = True, bla: bool = False) -> None:
        """fr_render_deepx_ship / fr_render_deepx_ship_async: a Burning Ship view with extended-exponent deltas, zooms down to
        1e-1000.  `view` carries the centre and the zoom as decimal strings (DeepView(..., zoom="1e-400")); a view without a
        zoom string is a ValueError (render_deep_ship() takes those).  state.zoom and its double centre are not read; every
        other field comes from `state`.  Planes, shard, stream and sync as for render_deep_ship(); the context keeps this
        path's orbit in a slot of its own.  bla=True sets FR_FLAG_DEEPX_SHIP_BLA: iteration skipping with the ship's 2x2 maps in
        extended arithmetic (the header's rules; last_deepx_ship_steps() reports what it skipped)."""
        if view is None or view.zoom is None:
            raise ValueError("render_deepx_ship needs a view with a zoom string (DeepView(..., zoom=\"1e-400\")); "
                             "render_deep_ship renders views without one")
        p = state.to_params(FractalType.BurningShip, Precision.F64, post_chain)
        if bla:
            p.flags |= _capi.FR_FLAG_DEEPX_SHIP_BLA
        vx = view.to_cx()
        rows = shard.rows(height) if shard else height
        self._render_call(self._lib.fr_render_deepx_ship, self._lib.fr_render_deepx_ship_async, (C.byref(p), C.byref(vx)), width,
                          height, Precision.F64, rows, rgba, nu, iter, shard, stream, sync)

    def render_deep_julia(self, state: FractalState, width: int, height: int, view: Optional[DeepView] = None, *,
                          post_chain: bool = False, rgba=None, nu=None, iter=None, shard: Optional[Shard] = None,
                          stream: Optional[int] = None, sync: bool = True, bla: bool = False) -> None:
        """fr_render_deep_julia / fr_render_deep_julia_async: a Julia set view deeper than double precision, by perturbation
        around two reference orbits computed on the host (the orbit of the centre, and the critical orbit samples rebase
        onto).  c = (state.julia_c_real, state.julia_c_imag); `view` carries the centre as decimal strings (default "0",
        "0"), the zoom and every other field come from `state` (its double centre is not read).  A view with a zoom string
        (DeepView(..., zoom="1e-400")) goes to fr_render_deepx_julia / fr_render_deepx_julia_async: extended-exponent deltas,
        zooms down to 1e-1000, state.zoom not read.  Always fp64; planes, shard, stream and sync as for render_deep().
        bla=True sets the flag that fits the view, FR_FLAG_DEEPX_JULIA_BLA with a zoom string and FR_FLAG_DEEP_JULIA_BLA
        without: iteration skipping by bilinear approximation on both orbits (the header's rules; last_deepx_julia_steps() /
        last_deep_julia_steps() report what it skipped)."""
        p = state.to_params(FractalType.JuliaSet, Precision.F64, post_chain)
        rows = shard.rows(height) if shard else height
        if view is not None and view.zoom is not None:
            if bla:
                p.flags |= _capi.FR_FLAG_DEEPX_JULIA_BLA
            vx = view.to_cx()
            self._render_call(self._lib.fr_render_deepx_julia, self._lib.fr_render_deepx_julia_async, (C.byref(p), C.byref(vx)),
                              width, height, Precision.F64, rows, rgba, nu, iter, shard, stream, sync)
            return
        if bla:
            p.flags |= _capi.FR_FLAG_DEEP_JULIA_BLA
        v = (view or DeepView("0", "0")).to_c()
        self._render_call(self._lib.fr_render_deep_julia, self._lib.fr_render_deep_julia_async, (C.byref(p), C.byref(v)), width,
                          height, Precision.F64, rows, rgba, nu, iter, shard, stream, sync)

    def render_deep_julia_de(self, state: FractalState, width: int, height: int, view: Optional[DeepView] = None, *,
                             post_chain: bool = False, rgba=None, nu=None, iter=None, de=None, deriv=None, shade: bool = False,
                             edge_px: float = DEEP_DE_EDGE_PX, shard: Optional[Shard] = None, stream: Optional[int] = None,
                             sync: bool = True, bla: bool = False) -> None:
        """fr_render_deep_julia_de / fr_render_deepx_julia_de and their _async forms: render_deep_julia() with the derivative
        of a sample's point with respect to its own starting point carried through the perturbation loop, and two planes
        more.  de: rows*W float64, the exterior distance estimate of sample (0,0) in pixel spacings of the whole frame (0 for
        interior); deriv: rows*W*2 float64, (D.x, D.y) = dz_n/dz_0 * (zoom / H) at the escaping update.  Any one of the five
        planes is enough; all of them are host or all device memory.  shade and edge_px as for render_deep_de().  The view
        dispatches exactly as in render_deep_julia(): with a zoom string it goes to the extended entry point (de stays finite
        at any depth, deriv saturates outside a double's range), without one to the fp64 entry point.  iter, nu, rgba without
        shade and the step counts are render_deep_julia()'s, and the context's orbits and tables are shared with it.
        bla=True sets the flag that fits the view."""
        p = state.to_params(FractalType.JuliaSet, Precision.F64, post_chain)
        rows = shard.rows(height) if shard else height
        e = _capi.fr_deep_de(None, None, 1 if shade else 0, float(edge_px))
        extra = ((e, "de", de, "float64", 1), (e, "deriv", deriv, "float64", 2))
        # (through the class, as render_deep_de)
        if view is not None and view.zoom is not None:
            if bla:
                p.flags |= _capi.FR_FLAG_DEEPX_JULIA_BLA
            vx = view.to_cx()
            Renderer._render_call(self, self._lib.fr_render_deepx_julia_de, self._lib.fr_render_deepx_julia_de_async,
                                  (C.byref(p), C.byref(vx), C.byref(e)), width, height, Precision.F64, rows, rgba, nu, iter,
                                  shard, stream, sync, extra=extra)
            return
        if bla:
            p.flags |= _capi.FR_FLAG_DEEP_JULIA_BLA
        v = (view or DeepView("0", "0")).to_c()
        Renderer._render_call(self, self._lib.fr_render_deep_julia_de, self._lib.fr_render_deep_julia_de_async,
                              (C.byref(p), C.byref(v), C.byref(e)), width, height, Precision.F64, rows, rgba, nu, iter, shard,
                              stream, sync, extra=extra)

    def render_deep_ship_de(self, state: FractalState, width: int, height: int, view: Optional[DeepView] = None, *,
                            post_chain: bool = False, rgba=None, nu=None, iter=None, de=None, deriv=None, shade: bool = False,
                            edge_px: float = DEEP_DE_EDGE_PX, shard: Optional[Shard] = None, stream: Optional[int] = None,
                            sync: bool = True, bla: bool = False) -> None:
        """fr_render_deep_ship_de / fr_render_deepx_ship_de and their _async forms: render_deep_ship() / render_deepx_ship()
        with the real 2x2 Jacobian of a sample's point with respect to c carried through the perturbation loop, and two planes
        more.  de: rows*W float64, the exterior distance estimate of sample (0,0) in pixel spacings of the whole frame (0 for
        interior), |z| log|z| over the length of the gradient of |z|; deriv: rows*W*4 float64, (J11, J12, J21, J22) =
        dz/dc * (zoom / H) at the escaping update.  Any one of the five planes is enough; all of them are host or all device
        memory.  shade and edge_px as for render_deep_de().  The view dispatches as in render_deep_julia_de(): with a zoom
        string it goes to the extended entry point (de stays finite at any depth, deriv saturates outside a double's range),
        without one to the fp64 entry point.  iter, nu, rgba without shade and the step counts are the plain ship call's, and
        the context's orbit and table are shared with it.  bla=True sets the flag that fits the view."""
        p = state.to_params(FractalType.BurningShip, Precision.F64, post_chain)
        rows = shard.rows(height) if shard else height
        e = _capi.fr_deep_de(None, None, 1 if shade else 0, float(edge_px))
        extra = ((e, "de", de, "float64", 1), (e, "deriv", deriv, "float64", 4))
        # (through the class, as render_deep_de)
        if view is not None and view.zoom is not None:
            if bla:
                p.flags |= _capi.FR_FLAG_DEEPX_SHIP_BLA
            vx = view.to_cx()
            Renderer._render_call(self, self._lib.fr_render_deepx_ship_de, self._lib.fr_render_deepx_ship_de_async,
                                  (C.byref(p), C.byref(vx), C.byref(e)), width, height, Precision.F64, rows, rgba, nu, iter,
                                  shard, stream, sync, extra=extra)
            return
        if bla:
            p.flags |= _capi.FR_FLAG_DEEP_SHIP_BLA
        v = (view or DeepView()).to_c()
        Renderer._render_call(self, self._lib.fr_render_deep_ship_de, self._lib.fr_render_deep_ship_de_async,
                              (C.byref(p), C.byref(v), C.byref(e)), width, height, Precision.F64, rows, rgba, nu, iter, shard,
                              stream, sync, extra=extra)

    def _render_call(self, fn_sync, fn_async, params: tuple, width: int, height: int, precision: Precision, rows: int,
                     rgba, nu, it, shard: Optional[Shard], stream: Optional[int], sync: bool, extra=()) -> None:
        """the planes, the shard and the sync / async entry of render(), render_phoenix(), render_mandelbulb(), render_deep(),
        render_deep_de(), render_deep_ship(), render_deepx_ship(), render_deep_julia() and render_deep_phoenix(); params: the entry's arguments between
        the context and the frame size; extra: the planes it writes beyond rgba, nu and iter (_output)"""
        out = self._output(precision, rows, width, rgba, nu, it, extra)
        sh = shard.to_c() if shard else None
        shp = C.byref(sh) if sh is not None else None
        if sync:
            if stream is not None:
                raise ValueError("stream is only meaningful with sync=False")
            _capi.check(fn_sync(self._ctx, *params, width, height, shp, C.byref(out)))
        else:
            _capi.check(fn_async(self._ctx, *params, width, height, shp, C.byref(out), C.c_void_p(stream or 0)))

    def dispatch(self, fractal_type: FractalType, state: FractalState, extent: tuple, **kw) -> None:
        """Name-for-name mirror of ComputeEffectManager::dispatch (type, state, extent);
        the Vulkan command buffer / descriptor set arguments become the output planes."""
        self.render(state, int(extent[0]), int(extent[1]), fractal_type=fractal_type, **kw)

    def render_frame(self, state: FractalState, width: int, height: int, path: str,
                     fractal_type: FractalType = FractalType.Mandelbrot,
                     precision: Precision = Precision.F32) -> bool:
        """The RenderFrameCallback itself: bool(const FractalState&, width, height, path)
        (src/animation_renderer.h:41-48): render, 8-bit export, PNG -- all behind fr_render_frame_png.
        Returns False on failure, as the reference's callback does."""
        p = state.to_params(fractal_type, precision)
        return self._lib.fr_render_frame_png(self._ctx, C.byref(p), width, height, os.fsencode(path)) == _capi.FR_OK

    @staticmethod
    def colorize_supported(state: FractalState, fractal_type: FractalType = FractalType.Mandelbrot,
                           precision: Precision = Precision.F64) -> bool:
        """fr_colorize_supported: the colour plane is a function of the smooth-count plane alone."""
        p = state.to_params(fractal_type, precision)
        return bool(_capi.lib().fr_colorize_supported(C.byref(p)))

    def colorize(self, state: FractalState, nu, rgba, *, fractal_type: FractalType = FractalType.Mandelbrot,
                 precision: Precision = Precision.F64, post_chain: bool = False,
                 stream: Optional[int] = None) -> None:
        """fr_colorize_async: device nu plane (float64 for F64, float32 for F32) -> device RGBA f32 plane,
        bit-identical to the rgba plane render() writes.  Enqueued on `stream` (raw hipStream_t), no sync."""
        p = state.to_params(fractal_type, precision, post_chain)
        n = nu.numel()
        p_nu, k1 = self._ptr(nu, "float64" if precision == Precision.F64 else "float32", n, "nu")
        p_rgba, k2 = self._ptr(rgba, "float32", n * 4, "rgba")
        if k1 != "device" or k2 != "device":
            raise ValueError("colorize needs device tensors")
        _capi.check(self._lib.fr_colorize_async(self._ctx, C.byref(p), n, p_nu, p_rgba, C.c_void_p(stream or 0)))

    def export_rgb16(self, rgba, width: int, height: int, out=None, through_half: bool = False, stream: Optional[int] = None):
        """16-bit export of export_print_quality (src/vk_engine.cpp:2054-2073): clamp, *65535, flip.
        stream (raw hipStream_t, device tensors only): enqueue there and return without waiting (fr_export_rgb16_async)."""
        p_in, kind_in = self._ptr(rgba, "float32", width * height * 4, "rgba")
        if out is None:
            if kind_in == "device":
                import torch
                out = torch.empty((height, width, 3), dtype=torch.int16, device=rgba.device)   # torch has no uint16 math: raw bits
            else:
                out = np.empty((height, width, 3), np.uint16)
        want = "int16" if _is_torch(out) else "uint16"
        p_out, kind_out = self._ptr(out, want, width * height * 3, "rgb16")
        if kind_in != kind_out:
            raise ValueError("rgba and rgb16 must live in the same memory kind")
        mem = _capi.FR_MEM_DEVICE if kind_in == "device" else _capi.FR_MEM_HOST
        if stream is not None:
            if kind_in != "device":
                raise ValueError("stream is only meaningful for device tensors")
            _capi.check(self._lib.fr_export_rgb16_async(self._ctx, p_in, width, height, p_out, int(through_half), C.c_void_p(stream)))
        else:
            _capi.check(self._lib.fr_export_rgb16(self._ctx, p_in, width, height, p_out, mem, int(through_half)))
        return out

    def export_rgb8(self, rgba, width: int, height: int, out=None, through_half: bool = False, stream: Optional[int] = None):
        """8-bit export of VulkanEngine::render_animation_frame (src/vk_engine.cpp:1344-1371):
        second ACES + gamma, u8 truncation, vertical flip.
        stream (raw hipStream_t, device tensors only): enqueue there and return without waiting (fr_export_rgb8_async)."""
        p_in, kind_in = self._ptr(rgba, "float32", width * height * 4, "rgba")
        if out is None:
            if kind_in == "device":
                import torch
                out = torch.empty((height, width, 3), dtype=torch.uint8, device=rgba.device)
            else:
                out = np.empty((height, width, 3), np.uint8)
        p_out, kind_out = self._ptr(out, "uint8", width * height * 3, "rgb8")
        if kind_in != kind_out:
            raise ValueError("rgba and rgb8 must live in the same memory kind")
        mem = _capi.FR_MEM_DEVICE if kind_in == "device" else _capi.FR_MEM_HOST
        if stream is not None:
            if kind_in != "device":
                raise ValueError("stream is only meaningful for device tensors")
            _capi.check(self._lib.fr_export_rgb8_async(self._ctx, p_in, width, height, p_out, int(through_half), C.c_void_p(stream)))
        else:
            _capi.check(self._lib.fr_export_rgb8(self._ctx, p_in, width, height, p_out, mem, int(through_half)))
        return out


class Node:
    """fr_node: one frame over the GPUs of a node behind the C ABI -- one process, one render context, stream and host
    worker thread per device, parts rendered concurrently, the frame assembled on devices[root] by in-place peer stores
    or by an RCCL gather (include/fractalrenderer_amd.h).  `devices` may repeat an ordinal (render lanes on one card)."""

    def __init__(self, devices):
        self._lib = _capi.lib()
        devs = [int(d) for d in devices]
        arr = (C.c_int * len(devs))(*devs)
        h = C.c_void_p()
        _capi.check(self._lib.fr_node_create(arr, len(devs), C.byref(h)))
        self._node = h
        self.devices = devs

    def close(self) -> None:
        if getattr(self, "_node", None):
            self._lib.fr_node_destroy(self._node)
            self._node = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_option(self, name: str, value: int) -> None:
        _capi.check(self._lib.fr_node_set_option(self._node, name.encode(), int(value)))

    def set_tuning(self, name: str, value: int) -> None:
        """fr_node_set_tuning (internal, csrc/fr_tuning.h): fault injection, the one-card RCCL loopback, context tuning."""
        _capi.check(self._lib.fr_node_set_tuning(self._node, name.encode(), int(value)))

    def render(self, state: FractalState, width: int, height: int, *, root: int = 0,
               fractal_type: FractalType = FractalType.Mandelbrot, precision: Precision = Precision.F64,
               post_chain: bool = False, rgba=None, nu=None, iter=None, sync: bool = True) -> None:
        """fr_node_render (sync=False: fr_node_render_async; call wait())."""
        p = state.to_params(fractal_type, precision, post_chain)
        out = Renderer._output(None, precision, height, width, rgba, nu, iter)
        fn = self._lib.fr_node_render if sync else self._lib.fr_node_render_async
        _capi.check(fn(self._node, C.byref(p), width, height, int(root), C.byref(out)))

    def submit(self, state: FractalState, width: int, height: int, *, root: int = 0,
               fractal_type: FractalType = FractalType.Mandelbrot, precision: Precision = Precision.F64,
               post_chain: bool = False, rgba=None, nu=None, iter=None) -> int:
        """fr_node_submit: hands one frame to the node and returns its ticket without waiting; up to "slots" frames are in
        flight.  The planes must stay alive until wait_frame(ticket) / wait()."""
        p = state.to_params(fractal_type, precision, post_chain)
        out = Renderer._output(None, precision, height, width, rgba, nu, iter)
        t = C.c_uint64(0)
        _capi.check(self._lib.fr_node_submit(self._node, C.byref(p), width, height, int(root), C.byref(out), C.byref(t)))
        return int(t.value)

    def wait_frame(self, ticket: int) -> None:
        _capi.check(self._lib.fr_node_wait_frame(self._node, int(ticket)))

    def wait(self) -> None:
        _capi.check(self._lib.fr_node_wait(self._node))

    def in_flight(self) -> int:
        return int(self._lib.fr_node_in_flight(self._node))

    def render_animation(self, anim, output_folder: Optional[str], *, base: Optional[FractalState] = None,
                         fractal_type: FractalType = FractalType.Mandelbrot, precision: Precision = Precision.F32,
                         width: int = 0, height: int = 0, first_frame: int = 0, frame_count: int = 0, frame_step: int = 0,
                         max_iterations: int = 0, on_frame_complete=None, raw_fd: int = 0) -> int:
        """fr_node_render_animation: AnimationRenderer::start_render (src/animation_renderer.cpp:26-152) over the node's
        devices, end to end (render -> 8-bit export on the frame's root -> PNG).  `anim`: an AnimationSystem.  Returns the
        number of frames written; on_frame_complete(frame, total) returning True cancels.  raw_fd > 0: packed RGB24 frames to
        that file descriptor (an encoder's stdin) instead of PNG files; output_folder may then be None."""
        p = (base if base is not None else anim.fractal_state).to_params(fractal_type, precision)
        cb = _capi.FR_FRAME_CALLBACK((lambda f, t, _u: 1 if on_frame_complete(f, t) else 0) if on_frame_complete else 0)
        o = _capi.fr_anim_render_options(int(width), int(height), int(first_frame), int(frame_count), int(frame_step),
                                         int(max_iterations), 0, cb, None, int(raw_fd), 0)
        n = C.c_int32(0)
        folder = os.fsencode(output_folder) if output_folder is not None else None
        _capi.check(self._lib.fr_node_render_animation(self._node, anim._h, C.byref(p), C.byref(o), folder, C.byref(n)))
        return int(n.value)

    def rccl_usable(self) -> bool:
        return bool(self._lib.fr_node_rccl_usable(self._node))

    def last_gather(self) -> int:
        return int(self._lib.fr_node_last_gather(self._node))

    def last_kernel_ms(self, part: int) -> float:
        return float(self._lib.fr_node_last_kernel_ms(self._node, int(part)))


def rccl_selftest(device: int = 0, nbytes: int = 1 << 20) -> int:
    """fr_node_rccl_selftest (internal): plugin load, one-rank communicator, a grouped ncclSend / ncclRecv pair on a stream,
    compared on the host.  Returns ncclGetVersion()."""
    v = C.c_int(0)
    _capi.check(_capi.lib().fr_node_rccl_selftest(int(device), int(nbytes), C.byref(v)))
    return int(v.value)


def mapped_runtimes() -> list:
    """fr_node_mapped_runtimes (internal): the librccl / libamdhip64 / libfractalrenderer_amd files this process has mapped."""
    buf = C.create_string_buffer(1 << 16)
    _capi.check(_capi.lib().fr_node_mapped_runtimes(buf, len(buf)))
    return [ln for ln in buf.value.decode().split("\n") if ln]


def export8_thresholds(host_powf: bool = False) -> np.ndarray:
    """fr_export8_thresholds (internal): t[b] = the smallest float32 a of [0, 1] with (uint8)(powf(a, 1/2.2f) * 255) >= b,
    b = 0..255, and t[256] = inf -- the table the 8-bit export kernel corrects its gamma estimate against: baked in, from the
    correctly rounded single-precision power (tools/gen_export8_table.py).  host_powf: the same by bisection with this host's libm."""
    t = (C.c_float * 257)()
    (_capi.lib().fr_export8_thresholds_host_powf if host_powf else _capi.lib().fr_export8_thresholds)(t)
    return np.frombuffer(t, dtype=np.float32).copy()


def write_png(path: str, rgb: np.ndarray, texts=None, print_metadata: bool = False) -> None:
    """fr_write_png: (H, W, 3) uint8 or uint16 -> PNG (8-bit: the animation frames, src/vk_engine.cpp:1374-1381;
    16-bit + print_metadata: the print export, src/vk_engine.cpp:2114-2208)."""
    a = np.ascontiguousarray(rgb)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype not in (np.uint8, np.uint16):
        raise ValueError("rgb must be (H, W, 3) uint8 or uint16")
    items = list((texts or {}).items())
    arr = (_capi.fr_png_text * max(1, len(items)))()
    keep = []
    for k, (key, val) in enumerate(items):
        kb, vb = key.encode("latin-1"), val.encode("latin-1", "replace")
        keep += [kb, vb]
        arr[k].key, arr[k].text = kb, vb
    _capi.check(_capi.lib().fr_write_png(os.fsencode(path), a.shape[1], a.shape[0], 8 * a.dtype.itemsize,
                                         a.ctypes.data, arr, len(items), int(print_metadata)))


def write_raw_rgb24(fd: int, rgb8: np.ndarray) -> None:
    """fr_write_raw_rgb24: one packed RGB24 frame to a file descriptor (an encoder's stdin pipe)."""
    a = np.ascontiguousarray(rgb8, np.uint8)
    _capi.check(_capi.lib().fr_write_raw_rgb24(fd, a.ctypes.data, a.shape[1], a.shape[0]))


def frame_path(folder: str, frame: int) -> str:
    """frame_%06d.png naming of AnimationRenderer::start_render (src/animation_renderer.cpp:86-88)."""
    buf = C.create_string_buffer(4096)
    _capi.check(_capi.lib().fr_frame_path(os.fsencode(folder), frame, buf, len(buf)))
    return os.fsdecode(buf.value)
