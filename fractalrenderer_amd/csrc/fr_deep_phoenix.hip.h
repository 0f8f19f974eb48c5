/*
 * fr_deep_phoenix.hip.h -- Phoenix views deeper than double precision on gfx950 (fr_render_deep_phoenix): perturbation around
 * one reference orbit with rebasing, for the second-order recurrence of shaders/phoenix.comp,
 *
 *   z' = z^2 + c + r z_prev + p z,   z = z_prev = 0 at the start, update then test |z|^2 > 4.
 *
 * The reference orbit Z_0 .. Z_N (fr_deep.c: fixed point on the host, stored as doubles, Z_{-1} = Z_0 = 0) sits in HBM.  A
 * sample carries TWO deltas, dz = z - Z_m and dq = z_prev - Z_{m-1}, and its offset dc from the centre.  Subtracting the
 * orbit's recurrence from the sample's leaves
 *   dz' = (2 Z_m + dz + p) dz + r dq + dc,   dq' = dz
 * which the step below performs, one fp64 rounding per operation as written (the file is built with -ffp-contract=off):
 *   t   = (((Z_m.x + Z_m.x) + dz.x) + p,  (Z_m.y + Z_m.y) + dz.y)
 *   dz' = (((t.x dz.x - t.y dz.y) + r dq.x) + dc.x,  ((t.x dz.y + t.y dz.x) + r dq.y) + dc.y)
 *   dq' = dz;  m += 1;  z = Z_m + dz';  q = Z_{m-1} + dq';  r2 = |z|^2
 *   r2 > 4: escaped at this loop index, lastZ = z
 *   r2 + r^2 |q|^2 < |dz'|^2 + r^2 |dq'|^2  or  m == N: rebase, dz = z, dq = q, m = 0
 *   else dz = dz', dq = dq'
 * A rebase restores the PAIR (z, z_prev) as the two deltas from Z_0 = Z_{-1} = 0, so the step at m = 0 is the recurrence
 * itself.  The rule weighs the previous point by |r|, its weight in the next update: at r = 0 it is deep_orbit's rule
 * (fr_deep.hip.h); for r of order 1 the whole pair has to be smaller than the pair of deltas, so that a rebase never puts an
 * O(1) term r q next to pixel-dependent terms many orders below it.  The rule is empirical (the header says on which views it
 * was checked against the exact iteration), not a theorem.
 *
 * A kernel and a loop of its own rather than a fourth policy of deep_orbit<F>: the state is two deltas, the orbit is read at
 * two indices, and the rebase is another rule.  How it runs is deep_kernel's way:
 *   - a persistent grid of the resident set pulls runs of 8x8 sub-tiles from the sharded WaveQueue with unlimited stealing; one
 *     lane per sample, the aa x aa samples of a pixel one after the other in the lane (sx outer: the ship's viewport map, which
 *     is Phoenix's less the centre); the wave leaves a sample's loop when no lane is live;
 *   - Z_m and Z_{m+1} are in registers and Z_{m+2} is loaded one step ahead, as in deep_orbit; behind m += 1 the register that
 *     held Z_m is Z_{m-1}, so q is formed from the registers and no update gathers twice.  Z_1 is loaded once, so a rebase
 *     (Z_m = Z_0 = 0, Z_{m+1} = Z_1) waits for no load;
 *   - the colour stage is phoenix_kernel<double>'s: phoenix_smooth on (i, lastZ) in double, phoenix_colour on
 *     (smooth / max_iter, smooth, lastZ) narrowed to float, the aa x aa average, post_chain with Phoenix's floors.  lastZ of a
 *     sample that never escaped is Z_m + dz of its final state, the z of its last update.
 */
#pragma once
#include "fr_deep.hip.h"
#include "fr_phoenix.hip.h"

namespace fr {

/* Kernel argument block of deep_phoenix_kernel */
struct DeepPhoenixArgs {
    const double2* orbit;                /* Z_0 .. Z_N */
    int32_t n_ref;                       /* N >= 1 */
    int32_t max_iter, aa;
    double zoom;
    double p, r;                         /* the floats of fr_phoenix_params, widened */
    float stripe_density;
    float brightness, saturation, contrast;
    uint32_t flags;
    TileGeom g;
    float4* rgba;
    double* nu;
    int32_t* iter;
    QueueArgs q;
};

/* The wave's 64 samples, one per lane.  live = false: a lane without a sample (outside the frame).  esc = the loop index of
 * the escaping update (max_iter if none), (ezx, ezy) = lastZ. */
__device__ __forceinline__ void deep_phoenix_orbit(const DeepPhoenixArgs& A, const double dcx, const double dcy, const double2 z1,
                                                   bool live, int& esc, double& ezx, double& ezy)
{
    const double2* __restrict__ orbit = A.orbit;
    const int max_iter = A.max_iter, N = A.n_ref;
    const double p = A.p, r = A.r;
    const double rr = r * r;
    double dzx = 0.0, dzy = 0.0, dqx = 0.0, dqy = 0.0;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m */
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    int m = 0;
    esc = max_iter;
    ezx = 0.0; ezy = 0.0;
    for (int i = 0; i < max_iter; ++i) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const double2 Znn = orbit[m + 2 <= N ? m + 2 : N];       /* Z_{m+2}, for the next step (m + 1 < N) */
        const double tx = ((Zx + Zx) + dzx) + p, ty = (Zy + Zy) + dzy;
        const double nx = ((tx * dzx - ty * dzy) + r * dqx) + dcx;
        const double ny = ((tx * dzy + ty * dzx) + r * dqy) + dcy;
        ++m;                                                     /* (Zx, Zy) is Z_{m-1} from here, (dzx, dzy) is dq' */
        const double zx = Znx + nx, zy = Zny + ny;
        const double qx = Zx + dzx, qy = Zy + dzy;
        const double r2 = zx * zx + zy * zy;
        if (r2 > 4.0) {
            esc = i; ezx = zx; ezy = zy; live = false;
        } else if (r2 + rr * (qx * qx + qy * qy) < (nx * nx + ny * ny) + rr * (dzx * dzx + dzy * dzy) || m == N) {   /* rebase */
            dzx = zx; dzy = zy; dqx = qx; dqy = qy; m = 0;
            Zx = 0.0; Zy = 0.0; Znx = z1.x; Zny = z1.y;
        } else {
            dqx = dzx; dqy = dzy; dzx = nx; dzy = ny;
            Zx = Znx; Zy = Zny; Znx = Znn.x; Zny = Znn.y;
        }
    }
    if (live) { ezx = Zx + dzx; ezy = Zy + dzy; }                /* lastZ of a sample that never escaped */
}

/* The smooth count and the linear colour of one sample.  A function of its own, as deep_de_of is (fr_deep.hip.h): inlined, the
 * colour stage's transcendentals hold the kernel at 104 VGPRs = 4 waves per SIMD; this way it is 83 = 5, and the struct
 * returns in registers (scratch stays 0). */
struct PhoenixShade {
    double smooth;
    float r, g, b;
};

__device__ __attribute__((noinline)) PhoenixShade deep_phoenix_shade(const int esc, const double ezx, const double ezy,
                                                                     const int max_iter, const float density, const bool want_rgb)
{
    PhoenixShade o;
    o.smooth = phoenix_smooth<double>(esc, ezx, ezy, max_iter);
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    if (want_rgb) phoenix_colour((float)(o.smooth / (double)max_iter), (float)o.smooth, (float)ezx, (float)ezy, density, rgb);
    o.r = rgb[0]; o.g = rgb[1]; o.b = rgb[2];
    return o;
}

__global__ void __launch_bounds__(kBlockThreads)
deep_phoenix_kernel(const DeepPhoenixArgs A)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const int W = A.g.W, H = A.g.H, max_iter = A.max_iter;
    const int aa = A.aa > 1 ? A.aa : 1;
    const double resx = (double)W, resy = (double)H;
    const double2 z1 = A.orbit[1];

    walk_subtiles<3, true>(A.q, A.g, lane, [&](const int px, const int py, const int lrow, const bool inside) {
        float acc[3] = {0.0f, 0.0f, 0.0f};
        double nu0 = 0.0;
        int it0 = 0;
        const int nsamp = aa * aa;
        for (int s = 0; s < nsamp; ++s) {
            const double2 dc = ShipFormula::dc(px, py, s, aa, resx, resy, A.zoom);
            const double cx = inside ? dc.x : 0.0, cy = inside ? dc.y : 0.0;
            int esc;
            double ezx, ezy;
            deep_phoenix_orbit(A, cx, cy, z1, inside, esc, ezx, ezy);
            const PhoenixShade sh = deep_phoenix_shade(esc, ezx, ezy, max_iter, A.stripe_density, A.rgba != nullptr);
            if (s == 0) { nu0 = sh.smooth; it0 = esc; }
            if (A.rgba) { acc[0] = acc[0] + sh.r; acc[1] = acc[1] + sh.g; acc[2] = acc[2] + sh.b; }
        }
        if (!inside) return;
        const size_t o = plane_index(A.g, px, py, lrow);
        if (A.rgba) {
            const float n = (float)(aa * aa);
            float rgb[3] = {acc[0] / n, acc[1] / n, acc[2] / n};
            if (A.flags & FR_FLAG_POST_CHAIN) post_chain(rgb, A.brightness, A.saturation, A.contrast, true);
            A.rgba[o] = make_float4(rgb[0], rgb[1], rgb[2], 1.0f);
        }
        if (A.nu) A.nu[o] = nu0;
        if (A.iter) A.iter[o] = it0;
    });
}

}  // namespace fr
