/*
 * fr_deepseq.hip.h -- the resampling kernel of deep zoom sequences (fr_deep_sequence, mode 1; the arithmetic is in the
 * header).  A frame between two octave keyframes is read from the deeper keyframe k+1 where that one covers the pixel
 * and from keyframe k elsewhere, bilinearly: coordinates in fp64, colour in fp32, every operation one rounding.
 *
 * Memory-bound: four 16-byte taps and one 16-byte store per pixel, one pixel per lane in row-major order, so a wave
 * stores 1 KiB of consecutive bytes and its taps fall into two rows of at most 65 pixels of one keyframe each.
 */
#pragma once
#include "fr_kernels.hip.h"

namespace fr {

struct ResampleArgs {
    const float4* key0;                  /* keyframe k, W x H packed */
    const float4* key1;                  /* keyframe k + 1 */
    float4* out;                         /* the caller's plane, W x H packed */
    int32_t W, H;
    double u;                            /* in (0.5, 1]: the frame's height over keyframe k's */
};

/* floor(s) clamped to [0, n - 1], its right / lower neighbour, and the weight of that neighbour */
__device__ __forceinline__ void resample_tap(const double s, const int32_t n, int32_t& i0, int32_t& i1, float& w)
{
    const double f = floor(s);
    i0 = !(f >= 0.0) ? 0 : (f > (double)(n - 1) ? n - 1 : (int32_t)f);    /* (a NaN cannot arise; it would read pixel 0) */
    i1 = min(i0 + 1, n - 1);
    w = (float)(s - (double)i0);
}

__global__ void __launch_bounds__(kBlockThreads) deep_resample_kernel(const ResampleArgs a)
{
    const uint32_t npx = (uint32_t)a.W * (uint32_t)a.H;               /* < 2^31 (the caller checks) */
    const uint32_t i = blockIdx.x * (uint32_t)kBlockThreads + threadIdx.x;
    if (i >= npx) return;
    const uint32_t y = i / (uint32_t)a.W, x = i - y * (uint32_t)a.W;
    const double hw = 0.5 * (double)a.W, hh = 0.5 * (double)a.H;
    const double dx = (double)x - hw, dy = (double)y - hh;
    const double u2 = a.u + a.u;
    const double qx = hw + dx * u2, qy = hh + dy * u2;
    const bool deeper = qx >= 0.0 && qx <= (double)(a.W - 1) && qy >= 0.0 && qy <= (double)(a.H - 1);
    const float4* __restrict__ src = deeper ? a.key1 : a.key0;
    const double sx = deeper ? qx : hw + dx * a.u;
    const double sy = deeper ? qy : hh + dy * a.u;
    int32_t x0, x1, y0, y1;
    float wx, wy;
    resample_tap(sx, a.W, x0, x1, wx);
    resample_tap(sy, a.H, y0, y1, wy);
    const float cx = 1.0f - wx, cy = 1.0f - wy;
    const size_t r0 = (size_t)y0 * (size_t)a.W, r1 = (size_t)y1 * (size_t)a.W;
    const float4 v00 = src[r0 + x0], v01 = src[r0 + x1], v10 = src[r1 + x0], v11 = src[r1 + x1];
    float4 o;
    o.x = (v00.x * cx + v01.x * wx) * cy + (v10.x * cx + v11.x * wx) * wy;
    o.y = (v00.y * cx + v01.y * wx) * cy + (v10.y * cx + v11.y * wx) * wy;
    o.z = (v00.z * cx + v01.z * wx) * cy + (v10.z * cx + v11.z * wx) * wy;
    o.w = 1.0f;
    a.out[i] = o;
}

}  // namespace fr
