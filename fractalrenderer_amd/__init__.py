"""fractalrenderer_amd -- MI355X-native escape-time renderer (Mandelbrot/Julia hot path).

The product is libfractalrenderer_amd.so (C ABI: include/fractalrenderer_amd.h; HIP kernels:
fractalrenderer_amd/csrc/).  This package is the thin host-side mirror of the reference's
interface for that path.  Importing it loads the library and fails loudly if it is absent.
"""
from . import _capi
from ._capi import (FR_FLAG_DEEP_BLA, FR_FLAG_DEEPX_BLA, FR_FLAG_DEEP_SHIP_BLA, FR_FLAG_DEEPX_SHIP_BLA, FR_FLAG_DEEP_JULIA_BLA,
                    FR_FLAG_DEEPX_JULIA_BLA, FR_FLAG_DEEP_PHOENIX_BLA, FR_FLAG_DEEPX_PHOENIX_BLA, FractalRendererError, lib)
from .state import (FractalState, FractalType, Precision, Preset, MANDELBROT_PRESETS,
                    SEAHORSE_DEEP, pack_push_constants, PhoenixParams, PHOENIX_PRESETS, pack_push_constants_phoenix,
                    MandelbulbParams, MANDELBULB_PRESETS, pack_push_constants_mandelbulb, DeepView, deep_frac_bits,
                    deep_reference_orbit, deep_ship_reference_orbit, deepx_zoom, deepx_frac_bits, deepx_reference_orbit,
                    deepx_ship_reference_orbit, deep_julia_reference_orbits, deep_phoenix_reference_orbit,
                    deepx_phoenix_reference_orbit)
from .renderer import (Renderer, DeepSteps, DEEP_DE_EDGE_PX, Node, Shard, write_png, write_raw_rgb24, frame_path, export8_thresholds, rccl_selftest,
                       mapped_runtimes)
from .animation import (AnimationSystem, AnimationRenderer, InterpolationType, Keyframe, DeepZoomPath, ZoomKeyframe,
                        DeepZoomSequence, DeepSequenceFrame)

lib()  # no silent fallback: a missing/incomplete library is an import error

__all__ = [
    "FractalRendererError", "lib", "FractalState", "FractalType", "Precision", "Preset",
    "MANDELBROT_PRESETS", "SEAHORSE_DEEP", "pack_push_constants", "PhoenixParams", "PHOENIX_PRESETS",
    "pack_push_constants_phoenix", "MandelbulbParams", "MANDELBULB_PRESETS", "pack_push_constants_mandelbulb", "DeepView",
    "deep_frac_bits", "deep_reference_orbit", "deep_ship_reference_orbit", "deepx_zoom", "deepx_frac_bits", "deepx_reference_orbit", "deepx_ship_reference_orbit", "deep_julia_reference_orbits", "deep_phoenix_reference_orbit", "deepx_phoenix_reference_orbit", "FR_FLAG_DEEP_BLA", "FR_FLAG_DEEPX_BLA", "FR_FLAG_DEEP_SHIP_BLA", "FR_FLAG_DEEPX_SHIP_BLA", "FR_FLAG_DEEP_JULIA_BLA", "FR_FLAG_DEEPX_JULIA_BLA", "FR_FLAG_DEEP_PHOENIX_BLA", "FR_FLAG_DEEPX_PHOENIX_BLA", "DeepSteps", "DEEP_DE_EDGE_PX", "Renderer", "Node", "Shard",
    "write_png", "write_raw_rgb24", "frame_path", "export8_thresholds", "rccl_selftest", "mapped_runtimes",
    "AnimationSystem", "AnimationRenderer", "InterpolationType", "Keyframe", "DeepZoomPath", "ZoomKeyframe",
    "DeepZoomSequence", "DeepSequenceFrame",
]
