/*
 * fr_mandelbulb.hip.h -- the Mandelbulb ray marcher of shaders/mandelbulb.comp on gfx950 (fr_render_mandelbulb).
 *
 * Restated operation for operation in fp32, one rounding per operation, no contraction (the file is built with
 * -ffp-contract=off), with the accurate OCML acosf, atan2f, powf, sinf, cosf, expf, logf and a correctly rounded
 * sqrtf and divide: the host-side restatement (tests/mandelbulb_ref.py) and the SPIR-V interpreter evaluate the same
 * operations, so the planes agree to the few ulps by which the transcendentals differ.  How it runs:
 *   - a persistent grid of the resident set pulls runs of 8x8 sub-tiles from the sharded WaveQueue, as Phoenix does;
 *     sky rays end in a few steps, surface rays take tens to over a hundred, so the dynamic tiles balance the waves;
 *   - one lane per sample; the aa x aa samples of a pixel run one after the other in the lane (:201-213);
 *   - march / shade split: a wave's lanes march (one DE call per step) until the ballot of marching lanes is empty;
 *     only then do the lanes that hit shade together (12 more DE calls: 4 for the normal, 8 for the ambient
 *     occlusion).  Shading at the hit, as the shader's control flow reads, would run those 12 calls for one or a few
 *     lanes while the others wait.  Each lane's arithmetic is the same in both orders ("mandelbulb_split" = 1 in
 *     fr_ctx_set_tuning selects the in-loop order, for A/B measurements and the tests that compare the two bitwise);
 *   - the DE's own loop leaves per lane on escape (r > 2) and per wave once no lane is left in it;
 *   - orbit, ray and shading state stay in registers (no scratch: tests/test_mandelbulb_host.py checks it).
 * NaN policy (include/fractalrenderer_amd.h): the linear colour keeps the shader's NaN (log(log|pos|) of a hit inside
 * the unit sphere); the post chain's clamp maps NaN to 0 as IEEE maxNum / minNum do.
 */
#pragma once
#include "fr_kernels.hip.h"

namespace fr {

/* Kernel argument block of mandelbulb_kernel (its own: LaunchArgs is shared by the escape-time kernels). The clamps of
 * main (:177-190) are applied by the host. */
struct MandelbulbArgs {
    float camera_distance, rotation_y, power, time, fov, rotation_speed;
    float color_offset, color_scale;
    float brightness, saturation, contrast;
    int32_t max_iter, palette_mode, aa;
    uint32_t flags;
    TileGeom g;
    float4* rgba;
    float* nu;
    int32_t* iter;
    QueueArgs q;
};

constexpr int kMbMaxSteps = 200;
constexpr float kMbMaxDist = 10.0f;

/* GLSL max and clamp in the operand order of FMax (x < y ? y : x) and FClamp (min(max(x, lo), hi)), which keep a NaN x:
 * the linear colour carries the shader's NaN.  Only the post chain clamps with maxNum / minNum (mb_post_chain). */
__device__ __forceinline__ float mb_max(float x, float y) { return x < y ? y : x; }
__device__ __forceinline__ float mb_clamp(float x, float lo, float hi)
{
    const float m = lo > x ? lo : x;
    return hi < m ? hi : m;
}
__device__ __forceinline__ float mb_fract(float x) { return x - floorf(x); }
__device__ __forceinline__ float mb_mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }

/* mandelbulb_de, :96-108 */
__device__ __forceinline__ float mb_de(const float px, const float py, const float pz, const float power, const int max_iter,
                                       float& escape_iter)
{
    float zx = px, zy = py, zz = pz, dr = 1.0f, r = 0.0f;
    escape_iter = (float)max_iter;
    for (int i = 0; i < max_iter; ++i) {
        r = sqrtf((zx * zx + zy * zy) + zz * zz);
        if (r > 2.0f) { escape_iter = (float)i; break; }
        if (r < 0.0001f) break;
        float theta = acosf(mb_clamp(zz / r, -1.0f, 1.0f));
        float phi = atan2f(zy, zx);
        const float r_pow = powf(r, power - 1.0f);
        dr = (r_pow * power) * dr + 1.0f;
        const float zr = powf(r, power);
        theta = theta * power;
        phi = phi * power;
        const float st = sinf(theta), ct = cosf(theta), sp = sinf(phi), cp = cosf(phi);
        zx = (st * cp) * zr + px;
        zy = (sp * st) * zr + py;
        zz = ct * zr + pz;
    }
    if (r < 0.0001f || dr < 0.0001f) return 0.0f;
    return ((0.5f * logf(r)) * r) / dr;
}

/* hash / noise, :25-32 */
__device__ __forceinline__ float mb_hash(float x, float y)
{
    return mb_fract(sinf(x * 127.1f + y * 311.7f) * 43758.5453123f);
}

__device__ __forceinline__ float mb_noise(float px, float py)
{
    const float ix = floorf(px), iy = floorf(py);
    const float fx = mb_fract(px), fy = mb_fract(py);
    const float a = mb_hash(ix, iy), b = mb_hash(ix + 1.0f, iy + 0.0f);
    const float c = mb_hash(ix + 0.0f, iy + 1.0f), d = mb_hash(ix + 1.0f, iy + 1.0f);
    const float ux = (fx * fx) * (3.0f - 2.0f * fx), uy = (fy * fy) * (3.0f - 2.0f * fy);
    return (mb_mix(a, b, ux) + ((c - a) * uy) * (1.0f - ux)) + ((d - b) * ux) * uy;
}

/* hsv2rgb, :17-20 */
__device__ __forceinline__ void mb_hsv2rgb(float h, float s, float v, float rgb[3])
{
    const float off[3] = {0.0f, 4.0f, 2.0f};
    for (int k = 0; k < 3; ++k) {
        const float x = h * 6.0f + off[k];
        const float m = x - 6.0f * floorf(x / 6.0f);                           /* mod(x, 6) */
        const float c = mb_clamp(fabsf(m - 3.0f) - 1.0f, 0.0f, 1.0f);
        rgb[k] = mb_mix(1.0f, c, s) * v;
    }
}

__device__ __forceinline__ void mb_dynamic(float t, float rgb[3])                /* :34-39 */
{
    const float hue = mb_fract(t + 0.3f * sinf(t * 12.0f));
    const float sat = 0.6f + 0.4f * sinf(t * 7.0f);
    mb_hsv2rgb(hue, sat, powf(t, 0.4f), rgb);
}

__device__ __forceinline__ void mb_fire_ice(float t, float rgb[3])               /* :41-46 */
{
    const float s = mb_clamp((t - 0.0f) / (1.0f - 0.0f), 0.0f, 1.0f);
    const float blend = (s * s) * (3.0f - 2.0f * s);
    const float f = mb_fract(t * 3.0f);
    rgb[0] = mb_mix(powf(blend, 2.0f), 0.0f, f);
    rgb[1] = mb_mix(blend * 0.5f, 0.5f + 0.5f * blend, f);
    rgb[2] = mb_mix(0.0f, 1.0f, f);
}

__device__ __forceinline__ void mb_lava(float t, float rgb[3])                   /* :48-55 */
{
    /* knots c1..c5 as selects (an array indexed by the segment would live in scratch) */
    float a0, a1, a2, b0, b1, b2, w;
    if (t < 0.25f)      { a0 = 0.1f; a1 = 0.0f; a2 = 0.0f; b0 = 0.8f; b1 = 0.1f; b2 = 0.0f; w = t * 4.0f; }
    else if (t < 0.5f)  { a0 = 0.8f; a1 = 0.1f; a2 = 0.0f; b0 = 1.0f; b1 = 0.5f; b2 = 0.0f; w = (t - 0.25f) * 4.0f; }
    else if (t < 0.75f) { a0 = 1.0f; a1 = 0.5f; a2 = 0.0f; b0 = 1.0f; b1 = 0.9f; b2 = 0.3f; w = (t - 0.5f) * 4.0f; }
    else                { a0 = 1.0f; a1 = 0.9f; a2 = 0.3f; b0 = 1.0f; b1 = 1.0f; b2 = 0.8f; w = (t - 0.75f) * 4.0f; }
    rgb[0] = mb_mix(a0, b0, w); rgb[1] = mb_mix(a1, b1, w); rgb[2] = mb_mix(a2, b2, w);
}

__device__ __forceinline__ void mb_neon(float t, float rgb[3])                   /* :57-61 */
{
    const float c1[3] = {0.0f, 0.0f, 0.1f}, c2[3] = {0.0f, 0.2f, 0.6f}, c3[3] = {0.0f, 0.8f, 1.0f}, c4[3] = {0.5f, 1.0f, 1.0f};
    const float w = powf(t, 2.0f);
    for (int k = 0; k < 3; ++k) rgb[k] = mb_mix(mb_mix(c1[k], c2[k], t), mb_mix(c3[k], c4[k], t), w);
}

/* get_palette_color, :63-75 (mode already in [0, 5]) */
__device__ __forceinline__ void mb_palette(float t, int mode, float rgb[3])
{
    t = mb_fract(t);
    const float n = mb_noise(t * 100.0f, t * 57.0f) * 0.02f;
    /* modes 4 and 5 warp t first; the four ramps each have one call site */
    const float u = mode == 4 ? powf(t, 0.5f) : (mode == 5 ? powf(t, 0.6f) : t);
    const float x = u + n;
    if (mode == 0 || mode == 4) mb_dynamic(x, rgb);
    else if (mode == 1 || mode == 5) mb_fire_ice(x, rgb);
    else if (mode == 2) mb_lava(x, rgb);
    else mb_neon(x, rgb);
}

/* the hit branch of raymarch, :142-160: normal (4 DE calls, :113-124), lighting, palette, ambient occlusion (8 DE calls:
 * k = 0.01, 0.03, ... accumulated in float while k < 0.15), fog.  The 12 DE calls go through one call site. */
__device__ __forceinline__ void mb_shade(const MandelbulbArgs& A, const float power, const int max_iter, const float px,
                                         const float py, const float pz, const float rdx, const float rdy, const float rdz,
                                         const float t, const float d, const float escape_iter, const float mix_w,
                                         float rgb[3])
{
    constexpr float eps = 0.001f;
    float d0 = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f, ao = 0.0f, k = 0.01f, dummy;
#pragma unroll 1
    for (int j = 0; j < 12; ++j) {
        float qx = px, qy = py, qz = pz;
        if (j == 1)      { qx = px + eps; qy = py + 0.0f; qz = pz + 0.0f; }
        else if (j == 2) { qx = px + 0.0f; qy = py + eps; qz = pz + 0.0f; }
        else if (j == 3) { qx = px + 0.0f; qy = py + 0.0f; qz = pz + eps; }
        else if (j >= 4) { qx = nx * k + px; qy = ny * k + py; qz = nz * k + pz; }
        const float e = mb_de(qx, qy, qz, power, max_iter, dummy);
        if (j == 0) d0 = e;
        else if (j == 1) nx = e - d0;
        else if (j == 2) ny = e - d0;
        else if (j == 3) {
            nz = e - d0;
            const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
            if (len < 0.0001f) { nx = 0.0f; ny = 1.0f; nz = 0.0f; }
            else { nx = nx / len; ny = ny / len; nz = nz / len; }
        } else {
            ao = ao + expf(-10.0f * e);
            k = k + 0.02f;
        }
    }
    const float lx = __builtin_bit_cast(float, 0x3f1d8e9fu), lz = __builtin_bit_cast(float, 0x3efc1764u);   /* normalize */
    const float ly = lx;                                           /* (vec3(1, 1, 0.8)) as the shader's module holds it */
    const float diffuse = mb_max((nx * lx + ny * ly) + nz * lz, 0.0f);
    const float vx = -rdx, vy = -rdy, vz = -rdz;
    const float ix = -lx, iy = -ly, iz = -lz;                      /* reflect(-light_dir, normal) = I - 2 dot(N, I) N */
    const float k2 = 2.0f * ((nx * ix + ny * iy) + nz * iz);
    const float fx = ix - k2 * nx, fy = iy - k2 * ny, fz = iz - k2 * nz;
    const float spec = powf(mb_max((vx * fx + vy * fy) + vz * fz, 0.0f), 64.0f);
    const float rim = powf(1.0f - mb_max((nx * vx + ny * vy) + nz * vz, 0.0f), 2.0f);
    const float glow = expf(-8.0f * d), filament_glow = expf(-30.0f * d);
    const float lp = sqrtf((px * px + py * py) + pz * pz);
    float iter_t = (escape_iter + 1.0f) - logf(logf(lp)) / logf(power + 0.0001f);
    iter_t = iter_t / (float)max_iter;
    iter_t = mb_fract(A.color_offset + powf(iter_t, 0.6f) * A.color_scale);
    float base[3], alt[3];
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {                                  /* one palette call site for base and alt */
        float col[3];
        mb_palette(j == 0 ? iter_t : mb_fract(iter_t + 0.33f), j == 0 ? A.palette_mode : (A.palette_mode + 1) % 6, col);
        for (int c = 0; c < 3; ++c) { if (j == 0) base[c] = col[c]; else alt[c] = col[c]; }
    }
    const float light = 0.15f + diffuse * 0.9f;
    const float fg[3] = {1.0f, 0.8f, 0.5f};
    ao = 1.0f - ao / 8.0f;
    const float occl = ao * 0.8f + 0.2f;
    const float fog = mb_clamp(t / kMbMaxDist, 0.0f, 1.0f) * 0.6f;
    const float sky_fog[3] = {0.0f, 0.0f, 0.1f};
    for (int c = 0; c < 3; ++c) {
        float v = mb_mix(base[c], alt[c], mix_w);
        v = v * light;
        v = v + spec * 0.5f;
        v = v + rim * 0.25f;
        v = v + glow * 0.5f;
        v = v + (fg[c] * filament_glow) * 0.5f;
        v = v * occl;
        rgb[c] = mb_mix(v, sky_fog[c], fog);
    }
}

/* the sky of a miss, :165-166 */
__device__ __forceinline__ void mb_sky(const float rdy, float rgb[3])
{
    const float sky = mb_clamp(rdy * 0.5f + 0.5f, 0.0f, 1.0f);
    const float lo[3] = {0.02f, 0.02f, 0.05f}, hi[3] = {0.5f, 0.6f, 0.8f};
    for (int c = 0; c < 3; ++c) rgb[c] = mb_mix(lo[c], hi[c], sky);
}

/* enhance_color -> aces_tonemap -> pow(1/2.2), :85-91, :80-83, :216-218; the clamp of enhance_color maps NaN to 0
 * (maxNum / minNum).  The floors of :187-190 are applied by the host. */
__device__ __forceinline__ void mb_post_chain(float rgb[3], float brightness, float saturation, float contrast)
{
    float c[3];
    for (int k = 0; k < 3; ++k) c[k] = rgb[k] * brightness;
    for (int k = 0; k < 3; ++k) c[k] = (c[k] - 0.5f) * contrast + 0.5f;
    const float gray = (c[0] * 0.299f + c[1] * 0.587f) + c[2] * 0.114f;
    for (int k = 0; k < 3; ++k) c[k] = fminf(fmaxf(mb_mix(gray, c[k], saturation), 0.0f), 1.0f);   /* NaN -> 0 */
    const float g = __builtin_bit_cast(float, 0x3ee8ba2fu);       /* 1.0 / 2.2 as the shader's module holds it */
    for (int k = 0; k < 3; ++k) rgb[k] = powf(aces(c[k]), g);
}

template <bool kSplit>
__global__ void __launch_bounds__(kBlockThreads)
mandelbulb_kernel(const MandelbulbArgs A)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const int W = A.g.W, H = A.g.H, max_iter = A.max_iter, aa = A.aa;

    /* the camera, :192-209 (wave-uniform) */
    const float rotation = A.rotation_y + A.rotation_speed * A.time;
    const float dist = A.camera_distance * (1.0f + 0.3f * sinf(A.time * 0.5f));
    const float cr = cosf(rotation), sr = sinf(rotation);
    /* rot * vec3(0, 0, dist), columns (c, 0, s), (0, 1, 0), (-s, 0, c), summed over the columns in order */
    const float rox = (cr * 0.0f + 0.0f * 0.0f) + (-sr) * dist;
    const float roy = (0.0f * 0.0f + 1.0f * 0.0f) + 0.0f * dist;
    const float roz = (sr * 0.0f + 0.0f * 0.0f) + cr * dist;
    const float power = A.power + 0.5f * sinf(A.time * 0.7f);
    float fwx = -rox, fwy = -roy, fwz = -roz;
    {
        const float l = sqrtf((fwx * fwx + fwy * fwy) + fwz * fwz);
        fwx = fwx / l; fwy = fwy / l; fwz = fwz / l;
    }
    /* right = normalize(cross((0, 1, 0), forward)), up = cross(forward, right) */
    float rtx = 1.0f * fwz - fwy * 0.0f, rty = 0.0f * fwx - fwz * 0.0f, rtz = 0.0f * fwy - fwx * 1.0f;
    {
        const float l = sqrtf((rtx * rtx + rty * rty) + rtz * rtz);
        rtx = rtx / l; rty = rty / l; rtz = rtz / l;
    }
    const float upx = fwy * rtz - rty * fwz, upy = fwz * rtx - rtz * fwx, upz = fwx * rty - rtx * fwy;
    const float mix_w = 0.3f + 0.3f * sinf(A.time * 0.5f);
    const float faa = (float)aa, half_w = (float)W * 0.5f, half_h = (float)H * 0.5f, fh = (float)H;

    walk_subtiles<3, true>(A.q, A.g, lane, [&](const int px, const int py, const int lrow, const bool inside) {
        float acc[3] = {0.0f, 0.0f, 0.0f};
        float t0 = 0.0f;
        int step0 = -1;
        for (int sy = 0; sy < aa; ++sy) {
            for (int sx = 0; sx < aa; ++sx) {
                const float ux = (((float)px + (float)sx / faa) - half_w) / fh;     /* :203-205 */
                const float uy = (((float)py + (float)sy / faa) - half_h) / fh;
                float rdx = (fwx + (rtx * ux) * A.fov) + (upx * uy) * A.fov;           /* :209 */
                float rdy = (fwy + (rty * ux) * A.fov) + (upy * uy) * A.fov;
                float rdz = (fwz + (rtz * ux) * A.fov) + (upz * uy) * A.fov;
                {
                    const float l = sqrtf((rdx * rdx + rdy * rdy) + rdz * rdz);
                    rdx = rdx / l; rdy = rdy / l; rdz = rdz / l;
                }
                /* raymarch, :133-167 */
                float t = 0.001f, d = 0.0f, escape_iter = 0.0f, pxh = 0.0f, pyh = 0.0f, pzh = 0.0f;
                float rgb[3];
                int step = -1;
                bool marching = inside;
                bool hit = false;
                for (int i = 0; i < kMbMaxSteps; ++i) {
                    if (__builtin_amdgcn_ballot_w64(marching) == 0ull) break;
                    if (!marching) continue;
                    pxh = rdx * t + rox; pyh = rdy * t + roy; pzh = rdz * t + roz;
                    d = mb_de(pxh, pyh, pzh, power, max_iter, escape_iter);
                    if (isnan(d) || isinf(d)) { marching = false; continue; }
                    const float threshold = mb_max(0.0001f, 0.001f * t);
                    if (d < threshold) {
                        marching = false; hit = true; step = i;
                        if (!kSplit)
                            mb_shade(A, power, max_iter, pxh, pyh, pzh, rdx, rdy, rdz, t, d, escape_iter, mix_w, rgb);
                        continue;
                    }
                    if (t > kMbMaxDist || d > kMbMaxDist) { marching = false; continue; }
                    t = t + mb_max(d * 0.5f, 0.0005f);
                }
                if (kSplit && hit) mb_shade(A, power, max_iter, pxh, pyh, pzh, rdx, rdy, rdz, t, d, escape_iter, mix_w, rgb);
                if (!hit) mb_sky(rdy, rgb);
                if (sx == 0 && sy == 0) { t0 = t; step0 = step; }
                acc[0] = acc[0] + rgb[0]; acc[1] = acc[1] + rgb[1]; acc[2] = acc[2] + rgb[2];   /* :211 */
            }
        }
        if (!inside) return;
        const size_t o = plane_index(A.g, px, py, lrow);
        if (A.rgba) {
            const float n = (float)(aa * aa);
            float rgb[3] = {acc[0] / n, acc[1] / n, acc[2] / n};                     /* :215 */
            if (A.flags & FR_FLAG_POST_CHAIN) mb_post_chain(rgb, A.brightness, A.saturation, A.contrast);
            A.rgba[o] = make_float4(rgb[0], rgb[1], rgb[2], 1.0f);
        }
        if (A.nu) A.nu[o] = t0;
        if (A.iter) A.iter[o] = step0;
    });
}

}  // namespace fr
