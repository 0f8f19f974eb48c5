/*
 * fr_deep.hip.h -- Mandelbrot views deeper than double precision on gfx950 (fr_render_deep): perturbation around one
 * reference orbit with rebasing.
 *
 * The reference orbit Z_0 .. Z_N (fr_deep.c: fixed point on the host, stored as doubles) sits in HBM; every sample
 * iterates its fp64 delta dz = z - Z_m from it, dc being its offset from the centre:
 *   t = (Z_m + Z_m) + dz;  dz' = (t.x dz.x - t.y dz.y, t.x dz.y + t.y dz.x) + dc;  m += 1;  z = Z_m + dz';  r2 = |z|^2
 *   r2 > B2: escaped at this loop index;  r2 < |dz'|^2 or m == N: rebase, dz = z, m = 0;  else dz = dz'
 * one rounding per operation as written (the file is built with -ffp-contract=off).  The rebase restarts the sample on the
 * orbit's start whenever its delta has outgrown the orbit (|z| < |dz|) or the orbit ends, so one reference serves every
 * sample and no glitch can form.  How it runs (as the Phoenix kernel):
 *   - a persistent grid of the resident set pulls runs of 8x8 sub-tiles from the sharded WaveQueue with unlimited
 *     stealing (deep views have very uneven iteration counts);
 *   - one lane per sample; the aa x aa samples of a pixel run one after the other in the lane (mandelbrot.comp:219-230);
 *   - dz, dc, m and the loop index stay in registers.  Z_m and Z_{m+1} are in registers too, and Z_{m+2} is loaded one
 *     step ahead; Z_1 is loaded once, so a rebase (Z_m = Z_0 = 0, Z_{m+1} = Z_1) waits for no load.  While no lane of a
 *     wave has rebased, all 64 lanes read the same orbit point; after that they gather from different m;
 *   - smooth count, palette, interior style and the post chain are those of the fp64 Mandelbrot path: shade() and
 *     post_chain() of fr_kernels.hip.h on (i, r2).
 */
#pragma once
#include "fr_kernels.hip.h"

namespace fr {

/* Kernel argument block of deep_kernel (its own: LaunchArgs is shared by the escape-time kernels and stays as it is).
 * The colour fields carry the names shade() / colour_of() read. */
struct DeepArgs {
    const double2* orbit;                /* Z_0 .. Z_N */
    int32_t n_ref;                       /* N >= 1 */
    int32_t max_iter, aa;
    double zoom, B2;
    int32_t W, H, rows_local, part, nparts, rows_per_strip, out_frame;
    uint32_t flags;
    /* colour stage (fill_params's values for the same fr_params) */
    int32_t interior_style, lib_log;
    double inv_max_iter, inv_log2_bailout, color_scale_d, color_offset_d;
    float brightness, saturation, contrast;
    fr_palette_table pal;
    const double2* log2_tab;
    float4* rgba;
    double* nu;
    int32_t* iter;
    QueueArgs q;
};

/* The wave's 64 samples, one per lane.  live = false: a lane without a sample (outside the frame).  esc = the loop index
 * of the escaping update (max_iter if none), r2 = |z|^2 there. */
__device__ __forceinline__ void deep_orbit(const DeepArgs& A, const double dcx, const double dcy, const double2 z1,
                                           bool live, int& esc, double& er2)
{
    const double2* __restrict__ orbit = A.orbit;
    const int N = A.n_ref, max_iter = A.max_iter;
    const double B2 = A.B2;
    double dzx = 0.0, dzy = 0.0;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m */
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    int m = 0;
    esc = max_iter;
    er2 = 0.0;
    for (int i = 0; i < max_iter; ++i) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const double2 Znn = orbit[m + 2 <= N ? m + 2 : N];      /* Z_{m+2}, for the next step (m + 1 < N) */
        const double tx = (Zx + Zx) + dzx, ty = (Zy + Zy) + dzy;
        const double nx = (tx * dzx - ty * dzy) + dcx;
        const double ny = (tx * dzy + ty * dzx) + dcy;
        ++m;
        const double zx = Znx + nx, zy = Zny + ny;
        const double r2 = zx * zx + zy * zy;
        if (r2 > B2) {
            esc = i; er2 = r2; live = false;
        } else if (r2 < nx * nx + ny * ny || m == N) {           /* rebase */
            dzx = zx; dzy = zy; m = 0;
            Zx = 0.0; Zy = 0.0; Znx = z1.x; Zny = z1.y;
        } else {
            dzx = nx; dzy = ny;
            Zx = Znx; Zy = Zny; Znx = Znn.x; Zny = Znn.y;
        }
    }
}

__global__ void __launch_bounds__(kBlockThreads)
deep_kernel(const DeepArgs A)
{
    __shared__ LdsBlock S;
    __shared__ double2 log2_lds[kLog2Entries];
    if (threadIdx.x == 0) S.pal = A.pal;
    reinterpret_cast<double*>(log2_lds)[threadIdx.x] = reinterpret_cast<const double*>(A.log2_tab)[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {                                       /* the colour of interior samples, once per workgroup */
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        colour_of<double, 0>(A, S, (double)A.max_iter, true, rgb);
        S.interior_rgb[0] = rgb[0]; S.interior_rgb[1] = rgb[1]; S.interior_rgb[2] = rgb[2];
    }
    __syncthreads();
    const LogTab<double> lg{log2_lds};

    const uint32_t lane = threadIdx.x & (kWave - 1);
    const int lx = (int)(lane & 7u), ly = (int)(lane >> 3);
    const int W = A.W, H = A.H;
    const int aa = A.aa > 1 ? A.aa : 1;
    const double resx = (double)W, resy = (double)H, zoom = A.zoom;
    const double2 z1 = A.orbit[1];
    const bool want_rgb = A.rgba != nullptr;
    const bool want_nu = want_rgb || A.nu != nullptr;

    WaveQueue q;
    q.init(A.q.heads, A.q.n_blk, (uint32_t)kShardBlock, A.q.run_shift, A.q.run_min, A.q.run_max, lane, A.q.ns_log2);
    q.set_probes(A.q.flags);
    uint32_t begin, count, cur_shard;
    while (q.next(begin, count, cur_shard)) {
        for (uint32_t j = begin; j < begin + count; ++j) {
            const uint32_t blk = WaveQueue::block_of(j / kShardBlock, cur_shard, A.q.ns_log2);
            if (blk >= A.q.n_blk) continue;
            const uint32_t sid = blk * kShardBlock + (j % kShardBlock);
            if (sid >= A.q.n_items) continue;
            const uint32_t sty = sid / A.q.nsx, stx = sid - sty * A.q.nsx;
            const int px = (int)stx * 8 + lx;
            const int lrow = (int)sty * 8 + ly;
            const bool inside = px < W && lrow < A.rows_local;
            int py = lrow;
            if (A.nparts != 1) {
                const int strip = lrow / A.rows_per_strip;
                py = (strip * A.nparts + A.part) * A.rows_per_strip + (lrow - strip * A.rows_per_strip);
            }
            float acc[3] = {0.0f, 0.0f, 0.0f};
            double nu0 = 0.0;
            int it0 = 0;
            const int nsamp = aa * aa;
            for (int s = 0; s < nsamp; ++s) {
                const int sy = s / aa, sx = s - sy * aa;                                   /* mandelbrot.comp:219-230 */
                const double pxs = (double)px + (double)sx / (double)aa;
                const double pys = (double)py + (double)sy / (double)aa;
                const double dcx = ((pxs - 0.5 * resx) / resy) * zoom;                     /* :149-151, less the centre */
                const double dcy = ((pys - 0.5 * resy) / resy) * zoom;
                int esc;
                double r2;
                deep_orbit(A, inside ? dcx : 0.0, inside ? dcy : 0.0, z1, inside, esc, r2);
                double nu;
                float rgb[3];
                shade<double, 0>(A, S, lg, esc, r2, want_nu, want_rgb, nu, rgb);
                if (s == 0) { nu0 = nu; it0 = esc; }
                acc[0] += rgb[0]; acc[1] += rgb[1]; acc[2] += rgb[2];
            }
            if (aa > 1) {
                const float n = (float)(aa * aa);
                acc[0] /= n; acc[1] /= n; acc[2] /= n;
            }
            if (want_rgb && (A.flags & FR_FLAG_POST_CHAIN)) post_chain(acc, A.brightness, A.saturation, A.contrast, false);
            if (!inside) continue;
            const size_t o = (size_t)(A.out_frame ? py : lrow) * (size_t)W + (size_t)px;
            if (A.rgba) A.rgba[o] = make_float4(acc[0], acc[1], acc[2], 1.0f);
            if (A.nu) A.nu[o] = nu0;
            if (A.iter) A.iter[o] = it0;
        }
    }
}

}  // namespace fr
