/*
 * fr_phoenix.hip.h -- the Phoenix fractal of shaders/phoenix.comp on gfx950 (fr_render_phoenix).
 *
 *   z' = z^2 + C + r * z_prev + p * z,  z = z_prev = 0 at the start, update then test |z|^2 > 4 (:63-78)
 *
 * restated operation for operation in fp32 (what the shader computes in) or fp64, one rounding per operation, no
 * contraction (the file is built with -ffp-contract=off).  How it runs:
 *   - a persistent grid of the resident set pulls runs of 8x8 sub-tiles from the sharded WaveQueue (8 or 64 shards);
 *   - one lane per sample; the aa x aa samples of a pixel run one after the other in the lane (:101-146);
 *   - the orbit (z, z_prev, C and the two squares of z) stays in registers.  Blocks of 16 updates run UNCHECKED, keeping
 *     only the running maximum of |z|^2; a block in which some lane went past 4 is rolled back (z and z_prev at its
 *     start) and replayed with the test after every update.  A lane that escapes records (i, z) and is parked at the
 *     fixed point z = z_prev = C = 0, which every later update maps to itself; the wave leaves as soon as none of its
 *     64 lanes is live.  Escape is not absorbing here (|C| may exceed 2, and z_prev feeds back), so the unchecked block
 *     keeps the maximum rather than testing its last |z|^2 only: an orbit that leaves the disc and comes back inside a
 *     block is still caught, and the first non-finite |z|^2 of an orbit is always preceded (or accompanied) by a finite
 *     or infinite one above 4, which the maximum keeps;
 *   - smooth count, palette and flow stripes after the loop (:79-146), post chain at the store (:160-166).
 */
#pragma once
#include "fr_kernels.hip.h"

namespace fr {

/* Kernel argument block of phoenix_kernel (its own: LaunchArgs is shared by the escape-time kernels and stays as it is). */
struct PhoenixArgs {
    double center_x, center_y, zoom;     /* fp64 map; the fp32 kernel reads the float narrowings below (data1.xyz) */
    double julia_cx, julia_cy;
    float center_x_f, center_y_f, zoom_f, julia_cx_f, julia_cy_f;
    float p, r;                          /* data2.zw: float in FractalState (src/fractal_state.h:82-83) */
    float stripe_density;                /* data4.z */
    float brightness, saturation, contrast;
    int32_t max_iter, aa, use_julia;
    uint32_t flags;
    TileGeom g;
    float4* rgba;
    void* nu;
    int32_t* iter;
    QueueArgs q;
};

constexpr int kPhoenixBlock = 16;        /* updates per unchecked block */

/* One update, phoenix_step + the test of phoenix_iter (:63-66, :74-77) as written:
 *   x = (((zx*zx - zy*zy) + C.x) + r*prev.x) + p*zx,   y = ((((2*zx)*zy) + C.y) + r*prev.y) + p*zy
 * sx, sy hold zx*zx and zy*zy: the squares of the test are those of the next update.  Returns dot(z, z). */
template <typename T>
__device__ __forceinline__ T phoenix_step(T& zx, T& zy, T& qx, T& qy, T& sx, T& sy, const T cx, const T cy, const T p,
                                          const T r)
{
    const T x = (((sx - sy) + cx) + r * qx) + p * zx;
    const T y = ((((T)2 * zx) * zy + cy) + r * qy) + p * zy;
    qx = zx; qy = zy;
    zx = x; zy = y;
    sx = x * x; sy = y * y;
    return sx + sy;
}

/* phoenix_iter's loop (:69-79) for the wave's 64 samples.  live = false: a lane without a sample (outside the frame).
 * esc = the loop index i of the escaping update (max_iter if none), (ezx, ezy) = lastZ. */
template <typename T>
__device__ __forceinline__ void phoenix_orbit(T cx, T cy, const T p, const T r, const int max_iter, bool live, int& esc,
                                              T& ezx, T& ezy)
{
    T zx = (T)0, zy = (T)0, qx = (T)0, qy = (T)0, sx = (T)0, sy = (T)0;
    if (!live) { cx = (T)0; cy = (T)0; }
    esc = max_iter;
    ezx = (T)0; ezy = (T)0;
    auto park = [&]() { zx = zy = qx = qy = sx = sy = cx = cy = (T)0; };
    int i = 0;
    for (; i + kPhoenixBlock <= max_iter; i += kPhoenixBlock) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        const T zx0 = zx, zy0 = zy, qx0 = qx, qy0 = qy;
        T m = (T)0;
#pragma unroll
        for (int k = 0; k < kPhoenixBlock; ++k) {
            const T d = phoenix_step(zx, zy, qx, qy, sx, sy, cx, cy, p, r);
            m = m < d ? d : m;                                   /* (NaN d keeps m: see the file comment) */
        }
        if (__builtin_amdgcn_ballot_w64(m > (T)4) != 0ull) {
            cold_path();
            zx = zx0; zy = zy0; qx = qx0; qy = qy0;
            sx = zx * zx; sy = zy * zy;
            for (int k = 0; k < kPhoenixBlock; ++k) {
                const T d = phoenix_step(zx, zy, qx, qy, sx, sy, cx, cy, p, r);
                if (d > (T)4) { esc = i + k; ezx = zx; ezy = zy; live = false; park(); }
            }
        }
    }
    for (; i < max_iter; ++i) {                                  /* the last max_iter % 16 updates, tested */
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        const T d = phoenix_step(zx, zy, qx, qy, sx, sy, cx, cy, p, r);
        if (d > (T)4) { esc = i; ezx = zx; ezy = zy; live = false; park(); }
    }
    if (live) { ezx = zx; ezy = zy; }                            /* lastZ of a sample that never escaped */
}

/* smooth count, :80-83: float(i) + 1 - log(log(dot(z,z))/2 / log 2) / log 2; interior: float(max_iter) */
template <typename T>
__device__ __forceinline__ T phoenix_smooth(const int esc, const T ezx, const T ezy, const int max_iter)
{
    if (esc >= max_iter) return (T)max_iter;
    const T log_zn = Real<T>::log(ezx * ezx + ezy * ezy) / (T)2;
    const T nu = Real<T>::log(log_zn / Real<T>::ln2()) / Real<T>::ln2();
    return ((T)esc + (T)1) - nu;
}

/* get_palette_color -> palette_ultra_fire (:18-43): palette_mode is ignored.  NaN t fails every comparison: c5. */
__device__ __forceinline__ void phoenix_fire(float t, float rgb[3])
{
    t = t - floorf(t);                                           /* fract */
    t = pow01(t, 0.7f);
    const float c1[3] = {0.0f, 0.0f, 0.1f}, c2[3] = {0.8f, 0.0f, 0.0f}, c3[3] = {1.0f, 0.3f, 0.0f};
    const float c4[3] = {1.0f, 0.9f, 0.0f}, c5[3] = {1.0f, 1.0f, 0.95f};
    const float *a = c5, *b = c5;
    float w = 0.0f;
    if (t < 0.2f)      { a = c1; b = c2; w = t * 5.0f; }
    else if (t < 0.4f) { a = c2; b = c3; w = (t - 0.2f) * 5.0f; }
    else if (t < 0.6f) { a = c3; b = c4; w = (t - 0.4f) * 5.0f; }
    else if (t < 0.8f) { a = c4; b = c5; w = (t - 0.6f) * 5.0f; }
    else { rgb[0] = c5[0]; rgb[1] = c5[1]; rgb[2] = c5[2]; return; }
    for (int k = 0; k < 3; ++k) rgb[k] = a[k] * (1.0f - w) + b[k] * w;     /* GLSL mix */
}

/* colour of one sample, :119-140, in float as written.  The fp64 kernel hands it t = smooth / max_iter divided in double
 * and narrowed (as the fp64 Julia path narrows its palette argument), the smooth count and lastZ narrowed: past the
 * smooth count the shader's arithmetic is a colour, and in double its transcendentals (pow, exp, atan2, sin) held the
 * kernel at 136 VGPRs = 3 waves per SIMD. */
__device__ __forceinline__ void phoenix_colour(float t, const float smooth, const float ezx, const float ezy,
                                               const float density, float rgb[3])
{
    t = pow01(t, 0.8f);                                                    /* NaN for a negative smooth count */
    const float dens = density < 0.0f ? 0.0f : density;                    /* max(data4.z, 0) */
    if (!(dens > 0.01f)) { phoenix_fire(t, rgb); return; }
    const float amp = clamp01(dens * 0.05f);                               /* :99 */
    const float angle = atan2f(ezy, ezx);
    const float mod = 0.5f + 0.5f * sinf(angle * dens + smooth * 0.25f);
    const float adaptive = amp * (1.0f - expf(-0.004f * smooth * smooth));
    float t2 = t + 0.1f * mod;
    t2 = t2 - floorf(t2);                                                  /* fract */
    float base[3], stripe[3];
    phoenix_fire(t, base);
    phoenix_fire(t2, stripe);
    const float w = adaptive * mod;
    for (int k = 0; k < 3; ++k) rgb[k] = base[k] * (1.0f - w) + stripe[k] * w;
}

template <typename T>
__global__ void __launch_bounds__(kBlockThreads)
phoenix_kernel(const PhoenixArgs A)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const int W = A.g.W, H = A.g.H, max_iter = A.max_iter;
    const int aa = A.aa > 1 ? A.aa : 1;                                     /* max(int(data3.x), 1), :91 */
    constexpr bool f64 = std::is_same<T, double>::value;
    const T p = (T)A.p, r = (T)A.r;
    const T ctr_x = f64 ? (T)A.center_x : (T)A.center_x_f, ctr_y = f64 ? (T)A.center_y : (T)A.center_y_f;
    const T zoom = f64 ? (T)A.zoom : (T)A.zoom_f;
    const T jcx = f64 ? (T)A.julia_cx : (T)A.julia_cx_f, jcy = f64 ? (T)A.julia_cy : (T)A.julia_cy_f;
    const T sizex = (T)W, sizey = (T)H;
    const T aspect = sizex / sizey;                                         /* :106 */
    const T sample_offset = ((T)1 / sizex) / (T)aa;                         /* :93-94 */
    const T centre_off = sample_offset * (T)(aa - 1) * (T)0.5;              /* :103, second term */

    walk_subtiles<3, true>(A.q, A.g, lane, [&](const int px, const int py, const int lrow, const bool inside) {
        const T base_u = (T)px / sizex, base_v = (T)py / sizey;        /* :157 */
        float acc[3] = {0.0f, 0.0f, 0.0f};
        T nu0 = (T)0;
        int it0 = 0;
        for (int sx = 0; sx < aa; ++sx) {
            for (int sy = 0; sy < aa; ++sy) {
                const T ox = (T)sx * sample_offset - centre_off, oy = (T)sy * sample_offset - centre_off;   /* :103 */
                const T u = base_u + ox / sizex, v = base_v + oy / sizey;                               /* :104 */
                T cx = ctr_x + ((u - (T)0.5) * zoom) * aspect;                                          /* :107-110 */
                T cy = ctr_y + (v - (T)0.5) * zoom;
                if (A.use_julia) { cx = jcx; cy = jcy; }                                                /* :64-65 */
                int esc;
                T ezx, ezy;
                phoenix_orbit<T>(cx, cy, p, r, max_iter, inside, esc, ezx, ezy);
                const T smooth = phoenix_smooth<T>(esc, ezx, ezy, max_iter);
                if (sx == 0 && sy == 0) { nu0 = smooth; it0 = esc; }
                if (A.rgba) {
                    float rgb[3];
                    phoenix_colour((float)(smooth / (T)max_iter), (float)smooth, (float)ezx, (float)ezy,
                                   A.stripe_density, rgb);
                    acc[0] = acc[0] + rgb[0]; acc[1] = acc[1] + rgb[1]; acc[2] = acc[2] + rgb[2];   /* :142 */
                }
            }
        }
        if (!inside) return;
        const size_t o = plane_index(A.g, px, py, lrow);
        if (A.rgba) {
            const float n = (float)(aa * aa);
            float rgb[3] = {acc[0] / n, acc[1] / n, acc[2] / n};                                      /* :146 */
            if (A.flags & FR_FLAG_POST_CHAIN) post_chain(rgb, A.brightness, A.saturation, A.contrast, true);
            A.rgba[o] = make_float4(rgb[0], rgb[1], rgb[2], 1.0f);
        }
        if (A.nu) static_cast<T*>(A.nu)[o] = nu0;
        if (A.iter) A.iter[o] = it0;
    });
}

}  // namespace fr
