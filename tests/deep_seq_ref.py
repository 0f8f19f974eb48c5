"""Deep zoom sequences (fr_deep_sequence): the plan and the resampling restated with numpy, operation for operation as
the header writes them.

- plan(zoom_first, zoom_last, frames, f, mode): what frame f is -- (zoom_mant, zoom_exp2, keyframe, resampled, u, L);
- auto_frac_bits: the sequence's automatic F (fr_deepx_frac_bits' rule on half the smaller zoom);
- resample(key0, key1, u): a frame between keyframes k (key0) and k + 1 (key1), coordinates in float64 and colour in
  float32, one rounding per operation (numpy never contracts a multiply and an add).

The standard sequence S of the tests is view T110 of tests/golden/deepx_views.json from "1e-110" to "2.5e-111" in 9 frames.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import deepx_ref as X

S = dict(view="T110", zoom_first="1e-110", zoom_last="2.5e-111", frames=9, max_iter=905)
S_GRID = {0: "1e-110", 4: "5e-111", 8: "2.5e-111"}          # the frames of S that are keyframes, and their zoom strings


def walk(zoom_first: str, zoom_last: str):
    zm0, ze0 = X.zoom_pair(zoom_first)
    zm1, ze1 = X.zoom_pair(zoom_last)
    D = float(ze1 - ze0) + (math.log2(zm1) - math.log2(zm0))
    return zm0, ze0, zm1, ze1, D


def plan(zoom_first: str, zoom_last: str, frames: int, f: int, mode: int = 0):
    zm0, ze0, zm1, ze1, D = walk(zoom_first, zoom_last)
    if f == 0:
        L, m, e = 0.0, zm0, ze0
    elif f == frames - 1:
        L, m, e = D, zm1, ze1
    else:
        L = (D * f) / (frames - 1)
        q = math.floor(L)
        r = L - q
        m = zm0 * float(np.exp2(np.float64(r)))
        if m >= 2.0:
            m, q = m / 2.0, q + 1
        e = ze0 + q
    s = -L
    k = math.floor(s)
    on_grid = s == k
    u = 1.0 if on_grid else float(np.exp2(np.float64(-(s - k))))
    return dict(zoom_mant=m, zoom_exp2=e, keyframe=k, resampled=int(mode == 1 and not on_grid), u=u, L=L)


def auto_frac_bits(zoom_first: str, zoom_last: str) -> int:
    """frac_bits_x of half the smaller of the two zooms (as a decimal string of the exact half)"""
    q = min(Fraction(zoom_first), Fraction(zoom_last)) / 2
    # an exact decimal string of q: its denominator divides a power of ten
    k = 0
    while (q * 10 ** k).denominator != 1:
        k += 1
    return X.frac_bits_x(f"{(q * 10 ** k).numerator}e-{k}")


def _tap(s: np.ndarray, n: int):
    i0 = np.clip(np.floor(s), 0, n - 1).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    w = (s - i0.astype(np.float64)).astype(np.float32)
    return i0, i1, w


def resample(key0: np.ndarray, key1: np.ndarray, u: float) -> np.ndarray:
    """key0 / key1: (H, W, 4) float32 planes of keyframes k / k + 1; returns the (H, W, 4) float32 frame"""
    H, W = key0.shape[:2]
    assert key0.dtype == np.float32 and key1.dtype == np.float32 and key1.shape == key0.shape
    u = np.float64(u)
    hw, hh = np.float64(0.5) * np.float64(W), np.float64(0.5) * np.float64(H)
    dx = (np.arange(W, dtype=np.float64) - hw)[None, :]
    dy = (np.arange(H, dtype=np.float64) - hh)[:, None]
    u2 = u + u
    qx = np.broadcast_to(hw + dx * u2, (H, W))
    qy = np.broadcast_to(hh + dy * u2, (H, W))
    deeper = (qx >= 0.0) & (qx <= W - 1) & (qy >= 0.0) & (qy <= H - 1)
    sx = np.where(deeper, qx, np.broadcast_to(hw + dx * u, (H, W)))
    sy = np.where(deeper, qy, np.broadcast_to(hh + dy * u, (H, W)))
    x0, x1, wx = _tap(sx, W)
    y0, y1, wy = _tap(sy, H)
    one = np.float32(1.0)
    cx, cy = one - wx, one - wy
    out = np.empty((H, W, 4), np.float32)
    for ch in range(3):
        a, b = key0[..., ch], key1[..., ch]
        v00 = np.where(deeper, b[y0, x0], a[y0, x0])
        v01 = np.where(deeper, b[y0, x1], a[y0, x1])
        v10 = np.where(deeper, b[y1, x0], a[y1, x0])
        v11 = np.where(deeper, b[y1, x1], a[y1, x1])
        top = v00 * cx + v01 * wx
        bot = v10 * cx + v11 * wx
        out[..., ch] = top * cy + bot * wy
    out[..., 3] = one
    return out
