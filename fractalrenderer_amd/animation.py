"""Mirror of the reference's animation model for the hot path's callers.

  AnimationSystem   src/animation_system.{h,cpp}  (keyframes, interpolate, .franim I/O)
  AnimationRenderer src/animation_renderer.{h,cpp} (the frame loop that invokes the
                    RenderFrameCallback plug-in point once per frame)
All arithmetic (JSON parsing, easing, interpolation, frame timing) lives in the C library
(fractalrenderer_amd/csrc/fr_franim.c); these classes only hold handles.
"""
from __future__ import annotations

import ctypes as C
import enum
import os
from dataclasses import dataclass
from typing import Callable, List, NamedTuple, Optional

from . import _capi
from .renderer import Renderer, frame_path
from .state import FractalState, FractalType, Precision


class InterpolationType(enum.IntEnum):
    """src/animation_system.h:8-14"""
    Linear = 0
    EaseInOut = 1
    EaseIn = 2
    EaseOut = 3
    Exponential = 4


@dataclass
class Keyframe:
    """src/animation_system.h:16-22"""
    time: float
    state: FractalState
    interp_type: InterpolationType = InterpolationType.EaseInOut


class AnimationSystem:
    """src/animation_system.h:37-83.  `fractal_state` plays the role of the reference's
    FractalState& member: it is what interpolate() returns when there are no keyframes."""

    def __init__(self, fractal_state: Optional[FractalState] = None):
        self._lib = _capi.lib()
        self.fractal_state = fractal_state if fractal_state is not None else FractalState()
        h = C.c_void_p()
        _capi.check(self._lib.fr_anim_create(C.byref(h)))
        self._h = h

    def _replace(self, h: C.c_void_p) -> None:
        if self._h:
            self._lib.fr_anim_free(self._h)
        self._h = h

    def __del__(self):
        try:
            if self._h:
                self._lib.fr_anim_free(self._h)
                self._h = None
        except Exception:
            pass

    # -- Save/Load (src/animation_system.cpp:221-313) -----------------------------------
    def load_from_file(self, filename: str) -> bool:
        h = C.c_void_p()
        st = self._lib.fr_anim_load(os.fsencode(filename), C.byref(h))
        if st != _capi.FR_OK:
            return False                      # the reference returns false and logs
        self._replace(h)
        return True

    def loads(self, text: str) -> None:
        raw = text.encode("utf-8")
        h = C.c_void_p()
        _capi.check(self._lib.fr_anim_parse(raw, len(raw), C.byref(h)))
        self._replace(h)

    def save_to_file(self, filename: str) -> bool:
        return self._lib.fr_anim_save(self._h, os.fsencode(filename)) == _capi.FR_OK

    # -- keyframes ----------------------------------------------------------------------
    def add_keyframe(self, time: float, state: FractalState,
                     interp_type: InterpolationType = InterpolationType.EaseInOut) -> None:
        p = state.to_params()
        _capi.check(self._lib.fr_anim_add_keyframe(self._h, time, C.byref(p), int(interp_type)))

    def get_keyframes(self) -> List[Keyframe]:
        out = []
        for i in range(self.info.keyframe_count):
            k = _capi.fr_keyframe()
            _capi.check(self._lib.fr_anim_get_keyframe(self._h, i, C.byref(k)))
            out.append(Keyframe(k.time, FractalState.from_params(k.state), InterpolationType(k.interp_type)))
        return out

    @property
    def info(self) -> _capi.fr_anim_info:
        i = _capi.fr_anim_info()
        _capi.check(self._lib.fr_anim_get_info(self._h, C.byref(i)))
        return i

    def get_duration(self) -> float:
        return float(self.info.duration)

    @property
    def name(self) -> str:
        return self._lib.fr_anim_name(self._h).decode("utf-8")

    @property
    def description(self) -> str:
        return self._lib.fr_anim_description(self._h).decode("utf-8")

    # -- interpolation (src/animation_system.cpp:82-181) ---------------------------------
    def interpolate(self, time: float) -> FractalState:
        base = self.fractal_state.to_params()
        out = _capi.fr_params()
        _capi.check(self._lib.fr_anim_state_at(self._h, time, C.byref(base), C.byref(out)))
        return FractalState.from_params(out)

    # -- frame arithmetic (src/animation_renderer.cpp:48,80) -------------------------------
    def frame_count(self) -> int:
        return int(self._lib.fr_anim_frame_count(self._h))

    def frame_time(self, frame: int) -> float:
        return float(self._lib.fr_anim_frame_time(self._h, frame))


# bool(const FractalState&, uint32_t width, uint32_t height, const std::string& path)
RenderFrameCallback = Callable[[FractalState, int, int, str], bool]


class AnimationRenderer:
    """The frame loop of AnimationRenderer::start_render (src/animation_renderer.cpp:26-152):
    for frame in range(int(duration*fps)): state = interpolate(frame/float(fps));
    render_frame_callback(state, export_width, export_height, "<folder>/frame_%06d.png")."""

    def __init__(self, render_frame_callback: Optional[RenderFrameCallback] = None):
        self.render_frame_callback = render_frame_callback
        self.current_frame = 0
        self.total_frames = 0
        self.on_frame_complete: Optional[Callable[[int, int], None]] = None

    def start_render(self, anim_system: AnimationSystem, output_folder: str = "animation_frames",
                     frames: Optional[range] = None, width: Optional[int] = None,
                     height: Optional[int] = None) -> bool:
        if self.render_frame_callback is None:
            return False                                           # :207-210 "No render callback set"
        info = anim_system.info
        if info.keyframe_count < 2:
            return False                                           # :35-42 "Need at least 2 keyframes"
        self.total_frames = anim_system.frame_count()              # :48
        w = width or info.export_width
        h = height or info.export_height
        for frame in (frames if frames is not None else range(self.total_frames)):
            if frame >= self.total_frames:
                break
            self.current_frame = frame
            time = anim_system.frame_time(frame)                   # :80
            state = anim_system.interpolate(time)                  # :83
            path = frame_path(output_folder, frame)                # :86-88
            if not self.render_frame_callback(state, w, h, path):  # :100-107 -> :216
                return False
            if self.on_frame_complete:
                self.on_frame_complete(frame, self.total_frames)   # :124-126
        return True


@dataclass
class ZoomKeyframe:
    """src/deep_zoom_system.h:84-89 (centre / zoom are the reference's double-backed ArbitraryFloat)"""
    center_x: float = 0.0
    center_y: float = 0.0
    zoom: float = 1.0
    duration: float = 0.0


class DeepZoomPath:
    """The zoom-path animation of DeepZoomManager (src/deep_zoom_system.cpp:454-556): playZoomPath, zoomTo,
    update_animation.  `state` is the FractalState it moves (the reference's DeepZoomState centre / zoom).
    All arithmetic is in the C library (fractalrenderer_amd/csrc/fr_zoompath.c)."""

    PRESETS = ("Seahorse", "Elephant", "MiniMandelbrot")        # DeepZoomPresets, :575-601

    def __init__(self, state: Optional[FractalState] = None):
        self._lib = _capi.lib()
        self.state = state if state is not None else FractalState()
        self.zoom_animating = False
        self.zoom_progress = 0.0
        h = C.c_void_p()
        _capi.check(self._lib.fr_zoom_path_create(C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if self._h:
                self._lib.fr_zoom_path_free(self._h)
                self._h = None
        except Exception:
            pass

    @staticmethod
    def preset(which) -> ZoomKeyframe:
        idx = DeepZoomPath.PRESETS.index(which) if isinstance(which, str) else int(which)
        k = _capi.fr_zoom_keyframe()
        _capi.check(_capi.lib().fr_zoom_preset(idx, C.byref(k)))
        return ZoomKeyframe(k.center_x, k.center_y, k.zoom, k.duration)

    def play_zoom_path(self, path: List[ZoomKeyframe]) -> None:
        arr = (_capi.fr_zoom_keyframe * max(1, len(path)))()
        for i, k in enumerate(path):
            arr[i].center_x, arr[i].center_y, arr[i].zoom, arr[i].duration = k.center_x, k.center_y, k.zoom, k.duration
        _capi.check(self._lib.fr_zoom_path_play(self._h, arr, len(path)))
        self.zoom_animating, self.zoom_progress = bool(path), 0.0

    def zoom_to(self, target_x: float, target_y: float, target_zoom: float, duration: float) -> None:
        p = self.state.to_params()
        _capi.check(self._lib.fr_zoom_path_zoom_to(self._h, C.byref(p), target_x, target_y, target_zoom, duration))
        self.zoom_animating, self.zoom_progress = True, 0.0

    def update_animation(self, delta_time: float) -> bool:
        """Advances the path; returns True where the reference recomputes its reference orbit (a keyframe was reached)."""
        p = self.state.to_params()
        anim, dirty, prog = C.c_int32(), C.c_int32(), C.c_float()
        _capi.check(self._lib.fr_zoom_path_update(self._h, delta_time, C.byref(p), C.byref(anim), C.byref(prog), C.byref(dirty)))
        self.state.center_x, self.state.center_y, self.state.zoom = p.center_x, p.center_y, p.zoom
        self.zoom_animating, self.zoom_progress = bool(anim.value), float(prog.value)
        return bool(dirty.value)


class DeepSequenceFrame(NamedTuple):
    """fr_deep_sequence_frame: what one frame of a DeepZoomSequence is"""
    zoom_mant: float        # the frame's view height is zoom_mant 2^zoom_exp2, zoom_mant in [1, 2)
    zoom_exp2: int
    frac_bits: int          # the sequence's F
    keyframe: int           # k = floor(-log2(zoom / zoom_first)); may be negative
    resampled: bool         # keyframes=True and the frame is not a keyframe itself
    u: float                # 1.0 on a keyframe, else in (0.5, 1): the frame's height over keyframe k's


class DeepZoomSequence:
    """fr_deep_sequence: a zoom into one deep centre, frame after frame, around one reference orbit.  The zoom runs from
    zoom_first to zoom_last (decimal strings, fr_deepx_view's range) in equal steps of log(zoom) over `frames` frames.
    keyframes=False renders every frame exactly (fr_render_deepx's kernels); keyframes=True renders one keyframe per octave
    and resamples the frames in between from their two neighbouring keyframes on the GPU (rgba only).  xbla sets
    FR_FLAG_DEEPX_BLA for every exact render; post_chain as for Renderer.render_deep.  formula="ship" walks into a Burning
    Ship centre instead (fr_deep_ship_sequence_create: every exact render is fr_render_deepx_ship's; bla=True sets
    FR_FLAG_DEEPX_SHIP_BLA for each of them, and xbla=True is a ValueError there, as bla=True is for the Mandelbrot formula).
    The renderer must outlive the sequence; the rules are in include/fractalrenderer_amd.h."""

    def __init__(self, renderer: Renderer, state: FractalState, cx, cy, zoom_first, zoom_last, frames: int, width: int,
                 height: int, *, keyframes: bool = False, frac_bits: int = 0, xbla: bool = False, post_chain: bool = False,
                 formula: str = "mandelbrot", bla: bool = False):
        if formula not in ("mandelbrot", "ship"):
            raise ValueError(f"formula {formula!r} is neither \"mandelbrot\" nor \"ship\"")
        ship = formula == "ship"
        if ship and xbla:
            raise ValueError("xbla=True is not available with formula=\"ship\": the flag of extended Burning Ship views is "
                             "bla=True")
        if bla and not ship:
            raise ValueError("bla=True is the Burning Ship formula's flag: the Mandelbrot formula takes xbla=True")
        self._lib = _capi.lib()
        self._h = None
        self.renderer, self.frames, self.width, self.height = renderer, int(frames), int(width), int(height)
        self._desc = _capi.fr_deep_sequence_desc(str(cx).encode("ascii"), str(cy).encode("ascii"),
                                                 str(zoom_first).encode("ascii"), str(zoom_last).encode("ascii"),
                                                 int(frames), int(frac_bits), 1 if keyframes else 0, 0)
        p = state.to_params(FractalType.BurningShip if ship else FractalType.Mandelbrot, Precision.F64, post_chain)
        if xbla:
            p.flags |= _capi.FR_FLAG_DEEPX_BLA
        if bla:
            p.flags |= _capi.FR_FLAG_DEEPX_SHIP_BLA
        h = C.c_void_p()
        create = self._lib.fr_deep_ship_sequence_create if ship else self._lib.fr_deep_sequence_create
        _capi.check(create(renderer._ctx, C.byref(p), C.byref(self._desc), self.width, self.height, C.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.fr_deep_sequence_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def plan(self, frame: int) -> DeepSequenceFrame:
        """fr_deep_sequence_plan: host arithmetic only"""
        f = _capi.fr_deep_sequence_frame()
        _capi.check(self._lib.fr_deep_sequence_plan(C.byref(self._desc), int(frame), C.byref(f)))
        return DeepSequenceFrame(f.zoom_mant, f.zoom_exp2, f.frac_bits, f.keyframe, bool(f.resampled), f.u)

    def render(self, frame: int, *, rgba=None, nu=None, iter=None) -> None:
        """fr_deep_sequence_render: the frame into the given planes, Renderer.render_deep's conventions (numpy arrays or torch
        CUDA tensors; nu is float64); a resampled frame has an rgba plane only.  Returns when the planes are written."""
        out = Renderer._output(None, Precision.F64, self.height, self.width, rgba, nu, iter)
        _capi.check(self._lib.fr_deep_sequence_render(self._h, int(frame), C.byref(out)))

    def render_png(self, frame: int, path: str) -> None:
        """fr_deep_sequence_render_png: the post-chained frame through the 8-bit export into a PNG"""
        _capi.check(self._lib.fr_deep_sequence_render_png(self._h, int(frame), os.fsencode(path)))

    def render_to_folder(self, folder: str, on_frame: Optional[Callable[[int, int], object]] = None) -> int:
        """Every frame as frame_%06d.png (fr_frame_path) in `folder`, in order.  on_frame(frame, frames) is called behind
        each file; a truthy return cancels the run.  Returns the number of files written."""
        os.makedirs(folder, exist_ok=True)
        for f in range(self.frames):
            self.render_png(f, frame_path(folder, f))
            if on_frame is not None and on_frame(f, self.frames):
                return f + 1
        return self.frames

    def stats(self) -> tuple:
        """fr_deep_sequence_stats: (exact renders enqueued, frames resampled, reference orbits computed)"""
        out = (C.c_uint64 * 3)()
        _capi.check(self._lib.fr_deep_sequence_stats(self._h, out))
        return int(out[0]), int(out[1]), int(out[2])
