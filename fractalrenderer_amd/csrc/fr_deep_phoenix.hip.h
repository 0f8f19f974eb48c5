/*
 * fr_deep_phoenix.hip.h -- Phoenix views deeper than double precision on gfx950 (fr_render_deep_phoenix, and below 1e-290
 * fr_render_deepx_phoenix: the second half of the file): perturbation around one reference orbit with rebasing, for the
 * second-order recurrence of shaders/phoenix.comp,
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
 * Loops and a kernel body of their own rather than a fourth policy of deep_orbit<F>: the state is two deltas, the orbit is read
 * at two indices, and the rebase is another rule.  There are four loops -- fp64 or extended-exponent deltas, each plain or with
 * iteration skipping -- and one body around them, deep_phoenix_kernel_body<DeepPhoenixBlock<X, BLA>> at the end of the file: the
 * block's two switches pick how dc is formed, which loop runs and whether the step counts exist.  How it runs is deep_kernel's way:
 *   - a persistent grid of the resident set pulls runs of 8x8 sub-tiles from the sharded WaveQueue with unlimited stealing; one
 *     lane per sample, the aa x aa samples of a pixel one after the other in the lane (sx outer: the ship's viewport map, which
 *     is Phoenix's less the centre); the wave leaves a sample's loop when no lane is live;
 *   - Z_m and Z_{m+1} are in registers and Z_{m+2} is loaded one step ahead, as in deep_orbit; behind m += 1 the register that
 *     held Z_m is Z_{m-1}, so q is formed from the registers and no update gathers twice.  Z_1 is loaded once, so a rebase
 *     (Z_m = Z_0 = 0, Z_{m+1} = Z_1) waits for no load;
 *   - the colour stage is phoenix_kernel<double>'s: phoenix_smooth on (i, lastZ) in double, phoenix_colour on
 *     (smooth / max_iter, smooth, lastZ) narrowed to float, the aa x aa average, post_chain with Phoenix's floors.  lastZ of a
 *     sample that never escaped is Z_m + dz of its final state, the z of its last update.
 * Behind the fp64 loop and the colour stage: iteration skipping for this path (FR_FLAG_DEEP_PHOENIX_BLA) -- the table's level
 * kernel and the flagged loop; then the extended half, its iteration skipping (FR_FLAG_DEEPX_PHOENIX_BLA), and the kernels.
 */
#pragma once
#include "fr_deep.hip.h"
#include "fr_phoenix.hip.h"

namespace fr {

/* What every deep Phoenix kernel reads: the whole argument block of deep_phoenix_kernel */
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

/* The argument block of the four kernels, composed as DeepBlock is (fr_deep.hip.h): DeepPhoenixArgs, then with X the orbit's
 * extended storage (orbit holds the plain doubles and zoom is not read), then with BLA the table of that storage.  A part that is
 * off is an empty base and takes no room. */
template <bool X, bool BLA = false>
struct DeepPhoenixBlock : DeepPhoenixArgs, std::conditional_t<X, DeepXOrbit, NoPart<0>> {
    static constexpr bool kX = X, kBla = false;
};

template <bool X>
struct DeepPhoenixBlock<X, true> : DeepPhoenixBlock<X> {
    static constexpr bool kBla = true;
    std::conditional_t<X, BlaXTable, BlaTable> t;
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

/* ---- iteration skipping (FR_FLAG_DEEP_PHOENIX_BLA; the header's section is the contract) ----------------------------------------
 * The linear part of the step acts on the PAIR (dz, dq): an entry of the table is a complex 2 x 2 matrix M = (M11, M12, M21, M22),
 * a complex 2-vector B = (B1, B2) and a radius that bounds |dz|^2 + |dq|^2.  Levels, coverage and entry count are those of the
 * other fp64 tables (bla_offset, bla_top_level of fr_deep.hip.h); the storage is BlaTable's, r in an array of its own and six
 * double2 per entry in ab: M's four, then B's two. */
constexpr int kPhoenixMbPerEntry = 6;

struct PhoenixLin {
    double2 m[4];                        /* M11, M12, M21, M22 */
    double2 b[2];                        /* B1, B2 */
    double r;
};

__device__ __forceinline__ double2 pc_mul(const double2 a, const double2 b)
{
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 pc_add(const double2 a, const double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double pc_n2(const double2 c) { return c.x * c.x + c.y * c.y; }

/* the single step at Z_m, 1 <= m <= N - 1: dz' = (2 Z_m + p) dz + r dq + dc, dq' = dz, valid while the dropped dz^2 stays below
 * one rounding of a dz */
__device__ __forceinline__ PhoenixLin phoenix_single(const double2 Z, const double p, const double r)
{
    PhoenixLin s;
    const double ax = (Z.x + Z.x) + p, ay = Z.y + Z.y;
    s.m[0] = make_double2(ax, ay); s.m[1] = make_double2(r, 0.0);
    s.m[2] = make_double2(1.0, 0.0); s.m[3] = make_double2(0.0, 0.0);
    s.b[0] = make_double2(1.0, 0.0); s.b[1] = make_double2(0.0, 0.0);
    s.r = 0x1p-54 * bla_abs(ax, ay);
    return s;
}

/* Level k of the table, as bla_level builds the others': entry j merges x (level k - 1, entry 2j) and y (entry 2j + 1), level 0
 * being the single steps from the orbit.  M = M_y M_x, B = M_y B_x + B_y,
 * r = min(r_x, max(0, (r_y - |B_x| dcmax) / |M_x|)) with the Frobenius norm of M_x, 0 when an element is not finite. */
__global__ void __launch_bounds__(kBlockThreads)
phoenix_bla_level_kernel(const double2* __restrict__ orbit, const int32_t n_ref, const int32_t k, const double dcmax,
                              const double p, const double r, double* __restrict__ rad, double2* __restrict__ mb)
{
    constexpr int S = kPhoenixMbPerEntry;
    const uint32_t n1 = (uint32_t)(n_ref - 1);
    const uint32_t cnt = n1 >> k;
    const uint32_t off = bla_offset(n1, k);
    const uint32_t offp = k > 1 ? bla_offset(n1, k - 1) : 0u;
    for (uint32_t j = blockIdx.x * kBlockThreads + threadIdx.x; j < cnt; j += gridDim.x * kBlockThreads) {
        PhoenixLin x, y;
        if (k == 1) {
            x = phoenix_single(orbit[1 + 2 * j], p, r);
            y = phoenix_single(orbit[2 + 2 * j], p, r);
        } else {
            const uint32_t ex = offp + 2 * j, ey = ex + 1;
            for (int i = 0; i < 4; ++i) { x.m[i] = mb[S * ex + i]; y.m[i] = mb[S * ey + i]; }
            for (int i = 0; i < 2; ++i) { x.b[i] = mb[S * ex + 4 + i]; y.b[i] = mb[S * ey + 4 + i]; }
            x.r = rad[ex]; y.r = rad[ey];
        }
        double2 m[4], b[2];
        bool finite = true;
        for (int i = 0; i < 2; ++i) {
            for (int c = 0; c < 2; ++c) m[2 * i + c] = pc_add(pc_mul(y.m[2 * i], x.m[c]), pc_mul(y.m[2 * i + 1], x.m[2 + c]));
            b[i] = pc_add(pc_add(pc_mul(y.m[2 * i], x.b[0]), pc_mul(y.m[2 * i + 1], x.b[1])), y.b[i]);
        }
        for (int i = 0; i < 4; ++i) finite = finite && __builtin_isfinite(m[i].x) && __builtin_isfinite(m[i].y);
        for (int i = 0; i < 2; ++i) finite = finite && __builtin_isfinite(b[i].x) && __builtin_isfinite(b[i].y);
        const double nm = sqrt((pc_n2(x.m[0]) + pc_n2(x.m[1])) + (pc_n2(x.m[2]) + pc_n2(x.m[3])));
        const double nb = sqrt(pc_n2(x.b[0]) + pc_n2(x.b[1]));
        const double t = (y.r - nb * dcmax) / nm;
        double rr = t > 0.0 ? t : 0.0;                           /* NaN: 0 */
        rr = rr < x.r ? rr : x.r;
        if (!finite) rr = 0.0;
        const uint32_t e = off + j;
        rad[e] = rr;
        for (int i = 0; i < 4; ++i) mb[S * e + i] = m[i];
        for (int i = 0; i < 2; ++i) mb[S * e + 4 + i] = b[i];
    }
}

/* deep_phoenix_orbit with BLA: u replaces the loop index.  A lane at m >= 1 probes the levels top down from bla_top_level (radii
 * are monotone in k) and takes the first whose radius admits the pair, else the plain step, operation for operation
 * deep_phoenix_orbit's; BLA and plain lanes of a wave take their steps in the same trip.  No level's radius exceeds the single
 * step's 2^-54 |2 Z_m + p| <= 2^-54 (4 + |p|), so a lane whose pair has |dz|^2 + |dq|^2 >= 2^-104 (4 + |p|)^2 (a bound sixteen
 * times above, with room for every rounding, and one compare against a wave-uniform constant) cannot pass a probe and gathers
 * nothing.  A BLA lane loads Z_m and Z_{m-1} at its new m, and Z_{m+1} if it goes on from there (the Z_{m+2} prefetch is for the
 * plain step).  nplain / nbla: the steps this sample took. */
__device__ __forceinline__ void deep_phoenix_orbit_bla(const DeepPhoenixArgs& A, const BlaTable& T, const double dcx,
                                                       const double dcy, const double2 z1, bool live, int& esc, double& ezx,
                                                       double& ezy, uint32_t& nplain, uint32_t& nbla)
{
    const double2* __restrict__ orbit = A.orbit;
    const double* __restrict__ tr = T.r;
    const double2* __restrict__ tmb = T.ab;
    const int max_iter = A.max_iter, N = A.n_ref, K = T.levels;
    const uint32_t n1 = (uint32_t)(N - 1);
    const double p = A.p, r = A.r;
    const double rr = r * r;
    double dzx = 0.0, dzy = 0.0, dqx = 0.0, dqy = 0.0;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m */
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    /* |dz|^2 + |dq|^2 of a lane at m >= 1, (dz.x dz.x + dz.y dz.y) + (dq.x dq.x + dq.y dq.y): the two sums are those of the
     * rebase test that let the lane go on from its last step, so the probe's operand costs one addition.  (A rebased lane is at
     * m = 0 and probes nothing before its next step.) */
    double v2 = 0.0;
    const double amax = 4.0 + fabs(p);                           /* |2 Z_m + p| <= 4 + |p| for m < N, where |Z_m| <= 2 */
    const double vmax = 0x1p-104 * (amax * amax);
    int m = 0, u = 0;
    esc = max_iter;
    ezx = 0.0; ezy = 0.0;
    nplain = 0u; nbla = 0u;
    for (;;) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const double2 Znn = orbit[m + 2 <= N ? m + 2 : N];       /* Z_{m+2}, for a plain step */
        int k = 0;
        uint32_t e = 0u;
        if (m >= 1 && v2 < vmax) {
            const uint32_t mm = (uint32_t)(m - 1);
            for (int kk = bla_top_level(mm, K, N, m, max_iter, u); kk >= 1; --kk) {
                const uint32_t ek = bla_offset(n1, kk) + (mm >> kk);
                const double rad = tr[ek];
                if (v2 < rad * rad) { k = kk; e = ek; break; }
            }
        }
        double nx, ny, nqx, nqy;                                 /* dz', dq' */
        double Zmx, Zmy, Zpx, Zpy;                               /* Z_m and Z_{m-1} behind the step */
        if (k > 0) {
            const double2* __restrict__ E = tmb + (size_t)kPhoenixMbPerEntry * e;
            const double2 dz = make_double2(dzx, dzy), dq = make_double2(dqx, dqy), dc = make_double2(dcx, dcy);
            const double2 nz = pc_add(pc_add(pc_mul(E[0], dz), pc_mul(E[1], dq)), pc_mul(E[4], dc));
            const double2 nq = pc_add(pc_add(pc_mul(E[2], dz), pc_mul(E[3], dq)), pc_mul(E[5], dc));
            nx = nz.x; ny = nz.y; nqx = nq.x; nqy = nq.y;
            m += 1 << k;
            u += 1 << k;
            ++nbla;
            const double2 Zm = orbit[m], Zp = orbit[m - 1];
            Zmx = Zm.x; Zmy = Zm.y; Zpx = Zp.x; Zpy = Zp.y;
        } else {
            const double tx = ((Zx + Zx) + dzx) + p, ty = (Zy + Zy) + dzy;
            nx = ((tx * dzx - ty * dzy) + r * dqx) + dcx;
            ny = ((tx * dzy + ty * dzx) + r * dqy) + dcy;
            nqx = dzx; nqy = dzy;
            ++m;
            ++u;
            ++nplain;
            Zmx = Znx; Zmy = Zny; Zpx = Zx; Zpy = Zy;
        }
        const double zx = Zmx + nx, zy = Zmy + ny;
        const double qx = Zpx + nqx, qy = Zpy + nqy;
        const double r2 = zx * zx + zy * zy;
        const double n2 = nx * nx + ny * ny, nq2 = nqx * nqx + nqy * nqy;
        if (r2 > 4.0) {
            esc = u - 1; ezx = zx; ezy = zy; live = false;       /* the last update the step covered */
        } else if (r2 + rr * (qx * qx + qy * qy) < n2 + rr * nq2 || m == N) {   /* rebase */
            dzx = zx; dzy = zy; dqx = qx; dqy = qy; m = 0;
            Zx = 0.0; Zy = 0.0; Znx = z1.x; Zny = z1.y;
        } else {
            dzx = nx; dzy = ny; dqx = nqx; dqy = nqy;
            v2 = n2 + nq2;
            Zx = Zmx; Zy = Zmy;
            if (k > 0) {                                          /* m < N here */
                const double2 Zn = orbit[m + 1];
                Znx = Zn.x; Zny = Zn.y;
            } else {
                Znx = Znn.x; Zny = Znn.y;
            }
        }
        if (u >= max_iter) live = false;                          /* esc stays max_iter */
    }
    if (esc == max_iter) { ezx = Zx + dzx; ezy = Zy + dzy; }     /* lastZ of a sample that never escaped */
}

/* ---- below 1e-290: extended-exponent deltas (fr_render_deepx_phoenix) ---------------------------------------------------------
 * deep_phoenix_orbit in the two modes of deep_orbit_x (fr_deep.hip.h; norm, (+), ldexp and the storage are the header's).  The
 * orbit is in the extended storage: mantissa pairs and int32 exponents for the extended mode, the plain doubles for the plain
 * one.  dc = norm(fx zm, fy zm, ze) as in deep_kernel, dcp = x_plain(dc).  A lane starts EXTENDED with dz = dq = the zero, m = 0.
 *
 * EXTENDED step.  Z_m = (X, Y, eZ), Z_{m+1} = (Xn, Yn, eZn), dz = (a, b, ed) normalised, dq = (c, d, eq) with |c|, |d| <= 2 (not
 * normalised: it is a copy of an earlier dz, or a q), dc = (cx, cy, ec).  pe = 0, or FR_DEEPX_ZERO_EXP when p == 0; the exponent of
 * the r dq term is er = eq, or FR_DEEPX_ZERO_EXP when r == 0: a term that is exactly zero never raises a common exponent.
 *   eu = max(eZ + 1, ed);   u = (ldexp(X, eZ + 1 - eu) + ldexp(a, ed - eu),  ldexp(Y, eZ + 1 - eu) + ldexp(b, ed - eu))
 *   et = max(eu, pe);       t = (ldexp(u.x, eu - et) + ldexp(p, pe - et),  ldexp(u.y, eu - et))
 *   P = (t.x a - t.y b,  t.x b + t.y a) at eP = et + ed
 *   e1 = max(eP, er);       s = (ldexp(P.x, eP - e1) + ldexp(r c, er - e1),  ldexp(P.y, eP - e1) + ldexp(r d, er - e1))
 *   en = max(e1, ec);       n = (ldexp(s.x, e1 - en) + ldexp(cx, ec - en),  ldexp(s.y, e1 - en) + ldexp(cy, ec - en))
 *   m += 1
 *   ez = max(eZn, en);      z = (ldexp(Xn, eZn - ez) + ldexp(n.x, en - ez),  ldexp(Yn, eZn - ez) + ldexp(n.y, en - ez))
 *   eq' = max(eZ, ed);      q = (ldexp(X, eZ - eq') + ldexp(a, ed - eq'),  ldexp(Y, eZ - eq') + ldexp(b, ed - eq'))
 *   r2 = z.x z.x + z.y z.y;   escaped at i if ldexp(r2, 2 ez) > 4, lastZ = (ldexp(z.x, ez), ldexp(z.y, ez))
 *   rebase if  r2 + ldexp((r r)(q.x q.x + q.y q.y), 2 (eq' - ez))  <  ldexp(n.x n.x + n.y n.y, 2 (en - ez)) + ldexp((r r)(a a + b b), 2 (ed - ez))
 *           or m == N:   dz = norm(z, ez), dq = (q, eq') with FR_DEEPX_ZERO_EXP for q = 0, m = 0
 *   else:                dz = norm(n, en), dq = (a, b, ed) -- a copy, no rounding and no second normalisation
 *   dz.e > -400: the lane turns PLAIN with dz = ldexp(dz, dz.e), dq = ldexp(dq, dq.e) (which may flush).
 * On operands a double holds every ldexp is exact, so the step performs the roundings of the PLAIN step in its order; from
 * dz = dq = 0 it gives n = dc exactly.
 *
 * PLAIN step: deep_phoenix_orbit's step and rule, operation for operation, on the plain doubles of the orbit and dcp.  If
 * afterwards max(|dz.x|, |dz.y|) < 2^-400 the lane turns EXTENDED with dz = norm(dz, 0), dq = norm(dq, 0).
 *
 * The mode depends on the new dz alone.  In the plain mode |dz| >= 2^-400, so t dz is at least 2^-800 unless t itself is down at
 * its rounding error; an r dq or a dc that a double cannot hold (below 2^-1074) is then more than 2^200 below the sum it enters.
 * lastZ of a lane that never escaped is Z_m (+) dz of its final state as a double.
 *
 * Registers across a step as in deep_phoenix_orbit: Z_{m+2} is loaded one step ahead, Z_1 is kept for the rebase, q comes from
 * the register that held Z_m; a lane that changes mode reloads Z_m and Z_{m+1} from the new mode's arrays. */
__device__ __forceinline__ void deep_phoenix_orbit_x(const DeepPhoenixBlock<true>& A, const double cx, const double cy, const int ec,
                                                     bool live, int& esc, double& ezx, double& ezy)
{
    const double2* __restrict__ orbit = A.orbit;
    const double2* __restrict__ mant = A.mant;
    const int32_t* __restrict__ exp2 = A.exp2;
    const int max_iter = A.max_iter, N = A.n_ref;
    const double p = A.p, r = A.r;
    const double rr = r * r;
    const int pe = p == 0.0 ? kXZero : 0;
    const bool rzero = r == 0.0;
    const double cpx = x_plain(cx, ec), cpy = x_plain(cy, ec);   /* the plain mode's dc */
    double dzx = 0.0, dzy = 0.0, dqx = 0.0, dqy = 0.0;           /* plain: dz, dq; extended: their mantissas */
    int ed = kXZero, eq = kXZero;
    bool ext = true;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m, in the lane's mode */
    int eZ = kXZero;
    const double2 z1 = mant[1];
    const int ez1 = exp2[1];
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    int eZn = ez1;
    int m = 0;
    esc = max_iter;
    ezx = 0.0; ezy = 0.0;
    for (int i = 0; i < max_iter; ++i) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const int mn = m + 2 <= N ? m + 2 : N;                   /* Z_{m+2}, for the next step (m + 1 < N) */
        if (ext) {
            const double2 Znn = mant[mn];
            const int eZnn = exp2[mn];
            const int eu = eZ + 1 > ed ? eZ + 1 : ed;
            const double ux = __builtin_ldexp(Zx, eZ + 1 - eu) + __builtin_ldexp(dzx, ed - eu);
            const double uy = __builtin_ldexp(Zy, eZ + 1 - eu) + __builtin_ldexp(dzy, ed - eu);
            const int et = eu > pe ? eu : pe;
            const double tx = __builtin_ldexp(ux, eu - et) + __builtin_ldexp(p, pe - et);
            const double ty = __builtin_ldexp(uy, eu - et);
            const double px = tx * dzx - ty * dzy;
            const double py = tx * dzy + ty * dzx;
            const int ep = et + ed;
            const int er = rzero ? kXZero : eq;
            const int e1 = ep > er ? ep : er;
            const double sx = __builtin_ldexp(px, ep - e1) + __builtin_ldexp(r * dqx, er - e1);
            const double sy = __builtin_ldexp(py, ep - e1) + __builtin_ldexp(r * dqy, er - e1);
            const int en = e1 > ec ? e1 : ec;
            const double nx = __builtin_ldexp(sx, e1 - en) + __builtin_ldexp(cx, ec - en);
            const double ny = __builtin_ldexp(sy, e1 - en) + __builtin_ldexp(cy, ec - en);
            ++m;                                                 /* (Zx, Zy, eZ) is Z_{m-1} from here, (dzx, dzy, ed) is dq' */
            const int ez = eZn > en ? eZn : en;
            const double zx = __builtin_ldexp(Znx, eZn - ez) + __builtin_ldexp(nx, en - ez);
            const double zy = __builtin_ldexp(Zny, eZn - ez) + __builtin_ldexp(ny, en - ez);
            const int eqq = eZ > ed ? eZ : ed;
            const double qx = __builtin_ldexp(Zx, eZ - eqq) + __builtin_ldexp(dzx, ed - eqq);
            const double qy = __builtin_ldexp(Zy, eZ - eqq) + __builtin_ldexp(dzy, ed - eqq);
            const double r2 = zx * zx + zy * zy;
            if (__builtin_ldexp(r2, 2 * ez) > 4.0) {
                esc = i; ezx = __builtin_ldexp(zx, ez); ezy = __builtin_ldexp(zy, ez); live = false;
                continue;
            }
            const double lhs = r2 + __builtin_ldexp(rr * (qx * qx + qy * qy), 2 * (eqq - ez));
            const double rhs = __builtin_ldexp(nx * nx + ny * ny, 2 * (en - ez)) +
                               __builtin_ldexp(rr * (dzx * dzx + dzy * dzy), 2 * (ed - ez));
            const bool reb = lhs < rhs || m == N;
            double ax = reb ? zx : nx, ay = reb ? zy : ny;
            int ea = reb ? ez : en;
            x_norm(ax, ay, ea);
            dqx = reb ? qx : dzx; dqy = reb ? qy : dzy;
            eq = reb ? ((qx == 0.0 && qy == 0.0) ? kXZero : eqq) : ed;
            if (reb) m = 0;
            if (ea <= kXThr) {                                    /* stays extended */
                dzx = ax; dzy = ay; ed = ea;
                if (reb) {
                    Zx = 0.0; Zy = 0.0; eZ = kXZero; Znx = z1.x; Zny = z1.y; eZn = ez1;
                } else {
                    Zx = Znx; Zy = Zny; eZ = eZn; Znx = Znn.x; Zny = Znn.y; eZn = eZnn;
                }
                continue;
            }
            dzx = __builtin_ldexp(ax, ea); dzy = __builtin_ldexp(ay, ea);
            dqx = __builtin_ldexp(dqx, eq); dqy = __builtin_ldexp(dqy, eq);
            ext = false;
        } else {
            const double2 Znn = orbit[mn];
            const double tx = ((Zx + Zx) + dzx) + p, ty = (Zy + Zy) + dzy;
            const double nx = ((tx * dzx - ty * dzy) + r * dqx) + cpx;
            const double ny = ((tx * dzy + ty * dzx) + r * dqy) + cpy;
            ++m;
            const double zx = Znx + nx, zy = Zny + ny;
            const double qx = Zx + dzx, qy = Zy + dzy;
            const double r2 = zx * zx + zy * zy;
            if (r2 > 4.0) {
                esc = i; ezx = zx; ezy = zy; live = false;
                continue;
            }
            const bool reb = r2 + rr * (qx * qx + qy * qy) < (nx * nx + ny * ny) + rr * (dzx * dzx + dzy * dzy) || m == N;
            double ax = reb ? zx : nx, ay = reb ? zy : ny;
            dqx = reb ? qx : dzx; dqy = reb ? qy : dzy;
            if (reb) m = 0;
            if (!(fmax(fabs(ax), fabs(ay)) < 0x1p-400)) {         /* stays plain */
                dzx = ax; dzy = ay;
                if (reb) {
                    const double2 p1 = orbit[1];
                    Zx = 0.0; Zy = 0.0; Znx = p1.x; Zny = p1.y;
                } else {
                    Zx = Znx; Zy = Zny; Znx = Znn.x; Zny = Znn.y;
                }
                continue;
            }
            int ea = 0;
            x_norm(ax, ay, ea);
            dzx = ax; dzy = ay; ed = ea;
            eq = 0;
            x_norm(dqx, dqy, eq);
            ext = true;
        }
        /* the lane changed its mode: Z_m and Z_{m+1} (m < N here) from the new mode's arrays */
        if (ext) {
            const double2 a = mant[m], b = mant[m + 1];
            Zx = a.x; Zy = a.y; eZ = exp2[m]; Znx = b.x; Zny = b.y; eZn = exp2[m + 1];
        } else {
            const double2 a = orbit[m], b = orbit[m + 1];
            Zx = a.x; Zy = a.y; Znx = b.x; Zny = b.y;
        }
    }
    if (live) {                                                  /* lastZ of a sample that never escaped */
        if (ext) {
            const int ez = eZ > ed ? eZ : ed;
            ezx = __builtin_ldexp(__builtin_ldexp(Zx, eZ - ez) + __builtin_ldexp(dzx, ed - ez), ez);
            ezy = __builtin_ldexp(__builtin_ldexp(Zy, eZ - ez) + __builtin_ldexp(dzy, ed - ez), ez);
        } else {
            ezx = Zx + dzx; ezy = Zy + dzy;
        }
    }
}

/* ---- iteration skipping below 1e-290 (FR_FLAG_DEEPX_PHOENIX_BLA; the header's section is the contract) ---------------------------
 * FR_FLAG_DEEP_PHOENIX_BLA's maps of the pair (dz, dq) in the extended arithmetic of BlaXTable: M's eight mantissas share one
 * int32 exponent, B's four another, the radius is an XRad.  The storage is the extended tables': r in an array of its own, six
 * double2 per entry in ab (M's four, then B's two), (M.e, B.e) in abe. */
struct PhoenixLinX {
    double2 m[4];                        /* mantissas of M11, M12, M21, M22 */
    double2 b[2];                        /* ... of B1, B2 */
    int em, eb;
    double rv;
    int re;
};

/* norm of the header on M's eight mantissas: the largest into [0.5, 1), the zero matrix gets FR_DEEPX_ZERO_EXP */
__device__ __forceinline__ void x_norm8(double2* m, int& e)
{
    const double mx = fmax(fmax(fmax(fabs(m[0].x), fabs(m[0].y)), fmax(fabs(m[1].x), fabs(m[1].y))),
                           fmax(fmax(fabs(m[2].x), fabs(m[2].y)), fmax(fabs(m[3].x), fabs(m[3].y))));
    const int k = __builtin_amdgcn_frexp_exp(mx);
    for (int i = 0; i < 4; ++i) { m[i].x = __builtin_ldexp(m[i].x, -k); m[i].y = __builtin_ldexp(m[i].y, -k); }
    e = mx == 0.0 ? kXZero : e + k;
}

/* the single step at Z_m = (Z, eZ), 1 <= m <= N - 1, from the extended storage: a = (Z, eZ + 1) (+) (p, pe), the doubling in the
 * exponent; M = norm(a, (r, 0), (1, 0), 0) on the common exponent max(a.e, 0), B = norm((1, 0), 0), rad = 2^-54 |norm(a)| with the
 * factor in the exponent */
__device__ __forceinline__ PhoenixLinX phoenix_single_x(const double2 Z, const int eZ, const double p, const int pe, const double r)
{
    PhoenixLinX s;
    const int ea = eZ + 1 > pe ? eZ + 1 : pe;
    const double ax = __builtin_ldexp(Z.x, eZ + 1 - ea) + __builtin_ldexp(p, pe - ea);
    const double ay = __builtin_ldexp(Z.y, eZ + 1 - ea);
    const int em = ea > 0 ? ea : 0;
    s.m[0] = make_double2(__builtin_ldexp(ax, ea - em), __builtin_ldexp(ay, ea - em));
    s.m[1] = make_double2(__builtin_ldexp(r, -em), 0.0);
    s.m[2] = make_double2(__builtin_ldexp(1.0, -em), 0.0);
    s.m[3] = make_double2(0.0, 0.0);
    s.em = em;
    x_norm8(s.m, s.em);
    s.b[0] = make_double2(0.5, 0.0); s.b[1] = make_double2(0.0, 0.0);
    s.eb = 1;
    double nx = ax, ny = ay;
    int ne = ea;
    x_norm(nx, ny, ne);
    double rv = bla_abs(nx, ny);
    int re = ne;
    x_norm1(rv, re);
    if (rv != 0.0) re -= 54;
    s.rv = rv; s.re = re;
    return s;
}

/* Level k of the extended table: phoenix_bla_level_kernel's merge with bla_level_x's exponents, radius, void rule and 24-bit cut */
__global__ void __launch_bounds__(kBlockThreads)
phoenix_x_bla_level_kernel(const double2* __restrict__ mant, const int32_t* __restrict__ exp2, const int32_t n_ref, const int32_t k,
                           const double dcv, const int32_t dce, const double p, const double r, XRad* __restrict__ rad,
                           double2* __restrict__ mb, int2* __restrict__ mbe)
{
    constexpr int S = kPhoenixMbPerEntry;
    const uint32_t n1 = (uint32_t)(n_ref - 1);
    const uint32_t cnt = n1 >> k;
    const uint32_t off = bla_offset(n1, k);
    const uint32_t offp = k > 1 ? bla_offset(n1, k - 1) : 0u;
    const int pe = p == 0.0 ? kXZero : 0;
    for (uint32_t j = blockIdx.x * kBlockThreads + threadIdx.x; j < cnt; j += gridDim.x * kBlockThreads) {
        PhoenixLinX x, y;
        if (k == 1) {
            x = phoenix_single_x(mant[1 + 2 * j], exp2[1 + 2 * j], p, pe, r);
            y = phoenix_single_x(mant[2 + 2 * j], exp2[2 + 2 * j], p, pe, r);
        } else {
            const uint32_t ex = offp + 2 * j, ey = ex + 1;
            const XRad rx = rad[ex], ry = rad[ey];
            const int2 eex = mbe[ex], eey = mbe[ey];
            for (int i = 0; i < 4; ++i) { x.m[i] = mb[S * ex + i]; y.m[i] = mb[S * ey + i]; }
            for (int i = 0; i < 2; ++i) { x.b[i] = mb[S * ex + 4 + i]; y.b[i] = mb[S * ey + 4 + i]; }
            x.em = eex.x; x.eb = eex.y; y.em = eey.x; y.eb = eey.y;
            x.rv = (double)rx.v; x.re = rx.e;
            y.rv = (double)ry.v; y.re = ry.e;
        }
        double2 m[4], q[2], b[2];
        for (int i = 0; i < 2; ++i) {
            for (int c = 0; c < 2; ++c) m[2 * i + c] = pc_add(pc_mul(y.m[2 * i], x.m[c]), pc_mul(y.m[2 * i + 1], x.m[2 + c]));
            q[i] = pc_add(pc_mul(y.m[2 * i], x.b[0]), pc_mul(y.m[2 * i + 1], x.b[1]));
        }
        int em = y.em + x.em;
        x_norm8(m, em);
        const int e1 = y.em + x.eb;
        int eb = e1 > y.eb ? e1 : y.eb;
        for (int i = 0; i < 2; ++i)
            b[i] = make_double2(__builtin_ldexp(q[i].x, e1 - eb) + __builtin_ldexp(y.b[i].x, y.eb - eb),
                                __builtin_ldexp(q[i].y, e1 - eb) + __builtin_ldexp(y.b[i].y, y.eb - eb));
        x_norm4(b[0], b[1], eb);
        double av = sqrt((pc_n2(x.m[0]) + pc_n2(x.m[1])) + (pc_n2(x.m[2]) + pc_n2(x.m[3])));
        int ae = x.em;
        x_norm1(av, ae);
        double bv = sqrt(pc_n2(x.b[0]) + pc_n2(x.b[1]));
        int be = x.eb;
        x_norm1(bv, be);
        const double pv = bv * dcv;
        const int pve = be + dce;
        const int et = y.re > pve ? y.re : pve;
        const double num = __builtin_ldexp(y.rv, y.re - et) - __builtin_ldexp(pv, pve - et);
        const double t = num / av;
        double rv = (t > 0.0 && __builtin_isfinite(t)) ? t : 0.0;    /* NaN: 0 */
        int re = et - ae;
        x_norm1(rv, re);
        /* M_x the zero matrix (an a more than 2^1074 below the 1 of M21 has no mantissa left next to it): t = +inf, rad = rad_x */
        const bool keep_x = av == 0.0 && num > 0.0;
        if (keep_x || !x_less(rv, re, x.rv, x.re)) { rv = x.rv; re = x.re; }
        const int lm = em < 0 ? -em : em, lb = eb < 0 ? -eb : eb;
        if ((lm > kXBlaExpLim && em != kXZero) || lb > kXBlaExpLim) {   /* void; the zero matrix is a map like any other */
            rv = 0.0; re = kXZero;
            for (int i = 0; i < 4; ++i) m[i] = make_double2(0.0, 0.0);
            for (int i = 0; i < 2; ++i) b[i] = make_double2(0.0, 0.0);
            em = kXZero; eb = kXZero;
        }
        const uint32_t e = off + j;
        XRad out;
        out.v = (float)x_trunc24(rv); out.e = re;
        rad[e] = out;
        for (int i = 0; i < 4; ++i) mb[S * e + i] = m[i];
        for (int i = 0; i < 2; ++i) mb[S * e + 4 + i] = b[i];
        mbe[e] = make_int2(em, eb);
    }
}

/* a term of a BLA step, a product of mantissas at the exponent e: exactly zero, it has FR_DEEPX_ZERO_EXP and raises no common
 * exponent (M12 = M22 = 0 at r = 0 must not shift M11 dz out of a double next to a dq 2^1100 above dz) */
__device__ __forceinline__ int px_term_exp(const double2 t, const int e) { return (t.x == 0.0 && t.y == 0.0) ? kXZero : e; }

/* (a, ea) (+) (b, eb) per component, at e = max(ea, eb) */
__device__ __forceinline__ double2 px_add(const double2 a, const int ea, const double2 b, const int eb, int& e)
{
    e = ea > eb ? ea : eb;
    return make_double2(__builtin_ldexp(a.x, ea - e) + __builtin_ldexp(b.x, eb - e),
                        __builtin_ldexp(a.y, ea - e) + __builtin_ldexp(b.y, eb - e));
}

/* deep_phoenix_orbit_x with BLA: u replaces the loop index.  A lane at m >= 1, in either mode, probes the levels top down from
 * bla_top_level on its pair as two normalised extended numbers at their common exponent (a plain lane forms norm(dz, 0) and
 * norm(dq, 0)); a BLA step is taken in extended arithmetic whatever the lane's mode, and ends in the EXTENDED step's tail -- z,
 * q = Z_{m-1} (+) dq', the escape test, the pair rebase rule, norm and the mode rule -- which the extended single step shares.
 * dq' of a BLA step is computed, not copied: it is normalised where the step stores it (dq = norm(q) or norm(dq')), so that at
 * m >= 1 both deltas of an extended lane are normalised.  The single steps are deep_phoenix_orbit_x's, operation for operation.
 * The pre-filter: no level's radius exceeds 2^-54 (4 + |p|) < 2^(E - 54), E the frexp exponent of 4 + |p|, and a normalised pair
 * has |v| >= 2^(max(dz.e, dq.e) - 1): an extended lane with max(dz.e, dq.e) + 53 >= E, or a plain lane whose
 * |dz|^2 + |dq|^2 >= 2^-104 (4 + |p|)^2 (deep_phoenix_orbit_bla's compare; no underflow, |dz| >= 2^-400), cannot pass a probe and
 * gathers nothing.  A BLA lane loads Z_m and Z_{m-1} at its new m from the extended storage, and Z_{m+1} from the arrays of the
 * mode it goes on in.  nsingle / nbla: the steps this sample took. */
__device__ __forceinline__ void deep_phoenix_orbit_x_bla(const DeepPhoenixBlock<true>& A, const BlaXTable& T, const double cx,
                                                         const double cy, const int ec, bool live, int& esc, double& ezx,
                                                         double& ezy, uint32_t& nsingle, uint32_t& nbla)
{
    const double2* __restrict__ orbit = A.orbit;
    const double2* __restrict__ mant = A.mant;
    const int32_t* __restrict__ exp2 = A.exp2;
    const XRad* __restrict__ tr = T.r;
    const double2* __restrict__ tmb = T.ab;
    const int2* __restrict__ tme = T.abe;
    const int max_iter = A.max_iter, N = A.n_ref, K = T.levels;
    const uint32_t n1 = (uint32_t)(N - 1);
    const double p = A.p, r = A.r;
    const double rr = r * r;
    const int pe = p == 0.0 ? kXZero : 0;
    const bool rzero = r == 0.0;
    const double amax = 4.0 + fabs(p);                           /* |2 Z_m + p| <= 4 + |p| for m < N, where |Z_m| <= 2 */
    const double vmax = 0x1p-104 * (amax * amax);
    const int eamax = __builtin_amdgcn_frexp_exp(amax);
    const double cpx = x_plain(cx, ec), cpy = x_plain(cy, ec);   /* the plain mode's dc */
    double dzx = 0.0, dzy = 0.0, dqx = 0.0, dqy = 0.0;           /* plain: dz, dq; extended: their mantissas */
    int ed = kXZero, eq = kXZero;
    bool ext = true;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m, in the lane's mode */
    int eZ = kXZero;
    const double2 z1 = mant[1];
    const int ez1 = exp2[1];
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    int eZn = ez1;
    int m = 0, u = 0;
    esc = max_iter;
    ezx = 0.0; ezy = 0.0;
    nsingle = 0u; nbla = 0u;
    for (;;) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const int mn = m + 2 <= N ? m + 2 : N;                   /* Z_{m+2}, for the single step after this one */
        int k = 0;
        uint32_t e = 0u;
        double vzx = dzx, vzy = dzy, vqx = dqx, vqy = dqy;       /* the pair, extended and normalised */
        int vze = ed, vqe = eq;
        if (m >= 1) {
            bool cand;
            if (ext) {
                cand = (ed > eq ? ed : eq) + 53 < eamax;
            } else {
                cand = (dzx * dzx + dzy * dzy) + (dqx * dqx + dqy * dqy) < vmax;
                if (cand) {
                    vze = 0; x_norm(vzx, vzy, vze);
                    vqe = 0; x_norm(vqx, vqy, vqe);
                }
            }
            if (cand) {
                const int ev = vze > vqe ? vze : vqe;
                const double a = __builtin_ldexp(vzx, vze - ev), b = __builtin_ldexp(vzy, vze - ev);
                const double c = __builtin_ldexp(vqx, vqe - ev), d = __builtin_ldexp(vqy, vqe - ev);
                const double v2 = (a * a + b * b) + (c * c + d * d);
                const uint32_t mm = (uint32_t)(m - 1);
                for (int kk = bla_top_level(mm, K, N, m, max_iter, u); kk >= 1; --kk) {
                    const uint32_t ek = bla_offset(n1, kk) + (mm >> kk);
                    const XRad rd = tr[ek];
                    const double rv = (double)rd.v;
                    if (v2 < __builtin_ldexp(rv * rv, 2 * (rd.e - ev))) { k = kk; e = ek; break; }
                }
            }
        }
        if (k > 0 || ext) {
            double nx, ny, nqx, nqy;                             /* dz' and dq' */
            double Wx, Wy, Px, Py;                               /* Z_m and Z_{m-1} behind the step */
            int en, enq, eW, eP, eZnn = 0;
            double2 Znn = make_double2(0.0, 0.0);
            if (k > 0) {
                const double2* __restrict__ E = tmb + (size_t)kPhoenixMbPerEntry * e;
                const int2 ee = tme[e];
                const double2 dz = make_double2(vzx, vzy), dq = make_double2(vqx, vqy), dc = make_double2(cx, cy);
                const double2 t1 = pc_mul(E[0], dz), t2 = pc_mul(E[1], dq), t3 = pc_mul(E[4], dc);
                const double2 s1 = pc_mul(E[2], dz), s2 = pc_mul(E[3], dq), s3 = pc_mul(E[5], dc);
                const int ez_ = ee.x + vze, eq_ = ee.x + vqe, ec_ = ee.y + ec;
                int e12;
                const double2 t12 = px_add(t1, px_term_exp(t1, ez_), t2, px_term_exp(t2, eq_), e12);
                const double2 nz = px_add(t12, e12, t3, px_term_exp(t3, ec_), en);
                const double2 s12 = px_add(s1, px_term_exp(s1, ez_), s2, px_term_exp(s2, eq_), e12);
                const double2 nq = px_add(s12, e12, s3, px_term_exp(s3, ec_), enq);
                nx = nz.x; ny = nz.y; nqx = nq.x; nqy = nq.y;
                m += 1 << k;
                u += 1 << k;
                ++nbla;
                const double2 Wm = mant[m], Pm = mant[m - 1];
                Wx = Wm.x; Wy = Wm.y; eW = exp2[m];
                Px = Pm.x; Py = Pm.y; eP = exp2[m - 1];
            } else {
                Znn = mant[mn];
                eZnn = exp2[mn];
                const int eu = eZ + 1 > ed ? eZ + 1 : ed;
                const double ux = __builtin_ldexp(Zx, eZ + 1 - eu) + __builtin_ldexp(dzx, ed - eu);
                const double uy = __builtin_ldexp(Zy, eZ + 1 - eu) + __builtin_ldexp(dzy, ed - eu);
                const int et = eu > pe ? eu : pe;
                const double tx = __builtin_ldexp(ux, eu - et) + __builtin_ldexp(p, pe - et);
                const double ty = __builtin_ldexp(uy, eu - et);
                const double px = tx * dzx - ty * dzy;
                const double py = tx * dzy + ty * dzx;
                const int ep = et + ed;
                const int er = rzero ? kXZero : eq;
                const int e1 = ep > er ? ep : er;
                const double sx = __builtin_ldexp(px, ep - e1) + __builtin_ldexp(r * dqx, er - e1);
                const double sy = __builtin_ldexp(py, ep - e1) + __builtin_ldexp(r * dqy, er - e1);
                en = e1 > ec ? e1 : ec;
                nx = __builtin_ldexp(sx, e1 - en) + __builtin_ldexp(cx, ec - en);
                ny = __builtin_ldexp(sy, e1 - en) + __builtin_ldexp(cy, ec - en);
                nqx = dzx; nqy = dzy; enq = ed;                  /* dq' = dz, a copy */
                ++m;
                ++u;
                ++nsingle;
                Wx = Znx; Wy = Zny; eW = eZn;
                Px = Zx; Py = Zy; eP = eZ;
            }
            const int ez = eW > en ? eW : en;
            const double zx = __builtin_ldexp(Wx, eW - ez) + __builtin_ldexp(nx, en - ez);
            const double zy = __builtin_ldexp(Wy, eW - ez) + __builtin_ldexp(ny, en - ez);
            const int eqq = eP > enq ? eP : enq;
            const double qx = __builtin_ldexp(Px, eP - eqq) + __builtin_ldexp(nqx, enq - eqq);
            const double qy = __builtin_ldexp(Py, eP - eqq) + __builtin_ldexp(nqy, enq - eqq);
            const double r2 = zx * zx + zy * zy;
            if (__builtin_ldexp(r2, 2 * ez) > 4.0) {
                esc = u - 1; ezx = __builtin_ldexp(zx, ez); ezy = __builtin_ldexp(zy, ez); live = false;   /* the last update covered */
                continue;
            }
            const double lhs = r2 + __builtin_ldexp(rr * (qx * qx + qy * qy), 2 * (eqq - ez));
            const double rhs = __builtin_ldexp(nx * nx + ny * ny, 2 * (en - ez)) +
                               __builtin_ldexp(rr * (nqx * nqx + nqy * nqy), 2 * (enq - ez));
            const bool reb = lhs < rhs || m == N;
            double ax = reb ? zx : nx, ay = reb ? zy : ny;
            int ea = reb ? ez : en;
            x_norm(ax, ay, ea);
            dqx = reb ? qx : nqx; dqy = reb ? qy : nqy;
            eq = reb ? ((qx == 0.0 && qy == 0.0) ? kXZero : eqq) : enq;
            if (k > 0) x_norm(dqx, dqy, eq);                      /* a BLA step's dq: normalised here */
            if (reb) m = 0;
            if (ea <= kXThr) {                                    /* extended from here */
                dzx = ax; dzy = ay; ed = ea;
                ext = true;
                if (reb) {
                    Zx = 0.0; Zy = 0.0; eZ = kXZero; Znx = z1.x; Zny = z1.y; eZn = ez1;
                } else if (k == 0) {
                    Zx = Znx; Zy = Zny; eZ = eZn; Znx = Znn.x; Zny = Znn.y; eZn = eZnn;
                } else {                                          /* m < N here */
                    const double2 b = mant[m + 1];
                    Zx = Wx; Zy = Wy; eZ = eW; Znx = b.x; Zny = b.y; eZn = exp2[m + 1];
                }
            } else {                                              /* plain from here (m < N) */
                const double2 a = orbit[m], b = orbit[m + 1];
                dzx = __builtin_ldexp(ax, ea); dzy = __builtin_ldexp(ay, ea);
                dqx = __builtin_ldexp(dqx, eq); dqy = __builtin_ldexp(dqy, eq);
                ext = false;
                Zx = a.x; Zy = a.y; Znx = b.x; Zny = b.y;
            }
        } else {
            const double2 Znn = orbit[mn];
            const double tx = ((Zx + Zx) + dzx) + p, ty = (Zy + Zy) + dzy;
            const double nx = ((tx * dzx - ty * dzy) + r * dqx) + cpx;
            const double ny = ((tx * dzy + ty * dzx) + r * dqy) + cpy;
            ++m;
            ++u;
            ++nsingle;
            const double zx = Znx + nx, zy = Zny + ny;
            const double qx = Zx + dzx, qy = Zy + dzy;
            const double r2 = zx * zx + zy * zy;
            if (r2 > 4.0) {
                esc = u - 1; ezx = zx; ezy = zy; live = false;
                continue;
            }
            const bool reb = r2 + rr * (qx * qx + qy * qy) < (nx * nx + ny * ny) + rr * (dzx * dzx + dzy * dzy) || m == N;
            double ax = reb ? zx : nx, ay = reb ? zy : ny;
            dqx = reb ? qx : dzx; dqy = reb ? qy : dzy;
            if (reb) m = 0;
            if (!(fmax(fabs(ax), fabs(ay)) < 0x1p-400)) {         /* stays plain */
                dzx = ax; dzy = ay;
                if (reb) {
                    const double2 p1 = orbit[1];
                    Zx = 0.0; Zy = 0.0; Znx = p1.x; Zny = p1.y;
                } else {
                    Zx = Znx; Zy = Zny; Znx = Znn.x; Zny = Znn.y;
                }
            } else {                                              /* turns extended (m < N) */
                const double2 a = mant[m], b = mant[m + 1];
                int ea = 0;
                x_norm(ax, ay, ea);
                dzx = ax; dzy = ay; ed = ea;
                eq = 0;
                x_norm(dqx, dqy, eq);
                ext = true;
                Zx = a.x; Zy = a.y; eZ = exp2[m]; Znx = b.x; Zny = b.y; eZn = exp2[m + 1];
            }
        }
        if (u >= max_iter) live = false;                          /* esc stays max_iter */
    }
    if (esc == max_iter) {                                       /* lastZ of a sample that never escaped */
        if (ext) {
            const int ez = eZ > ed ? eZ : ed;
            ezx = __builtin_ldexp(__builtin_ldexp(Zx, eZ - ez) + __builtin_ldexp(dzx, ed - ez), ez);
            ezy = __builtin_ldexp(__builtin_ldexp(Zy, eZ - ez) + __builtin_ldexp(dzy, ed - ez), ez);
        } else {
            ezx = Zx + dzx; ezy = Zy + dzy;
        }
    }
}

/* ---- the kernels ---------------------------------------------------------------------------------------------------------------
 * One body for the four, ARGS = DeepPhoenixBlock<X, BLA>.  X: dc is formed on the zoom's mantissa and normalised with the zoom's
 * exponent, and the loops are the extended ones.  BLA: the flagged loop, and the step counts -- each lane sums its samples' steps
 * and updates; a wave adds its three totals to the table's counters with one atomic each (updates skipped = updates - plain or
 * single steps).  The four named __global__ wrappers below are the kernels.  The block comes by value for the instruction
 * streams' sake, which are those of the time when each kernel had this body written into it: taken by reference, all four kernels
 * are scheduled differently. */
template <class ARGS>
__device__ __forceinline__ void deep_phoenix_kernel_body(const ARGS A)
{
    constexpr bool X = ARGS::kX, BLA = ARGS::kBla;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const int W = A.g.W, H = A.g.H, max_iter = A.max_iter;
    const int aa = A.aa > 1 ? A.aa : 1;
    const double resx = (double)W, resy = (double)H;
    const double2 z1 = X ? make_double2(0.0, 0.0) : A.orbit[1];  /* fp64: Z_1 for the rebase; the extended loops load their own */
    unsigned long long n_plain = 0ull, n_bla = 0ull, n_upd = 0ull;   /* BLA: this lane's steps and updates */

    walk_subtiles<3, true>(A.q, A.g, lane, [&](const int px, const int py, const int lrow, const bool inside) {
        float acc[3] = {0.0f, 0.0f, 0.0f};
        double nu0 = 0.0;
        int it0 = 0;
        const int nsamp = aa * aa;
        for (int s = 0; s < nsamp; ++s) {
            double zs;                                           /* extended: the zoom's mantissa; its exponent is dc.e */
            if constexpr (X) zs = A.zm;
            else zs = A.zoom;
            const double2 dc = ShipFormula::dc(px, py, s, aa, resx, resy, zs);
            double cx = inside ? dc.x : 0.0, cy = inside ? dc.y : 0.0;
            int ec = 0;
            if constexpr (X) { ec = A.ze; x_norm(cx, cy, ec); }
            int esc;
            double ezx, ezy;
            uint32_t np, nb;
            if constexpr (X) {
                if constexpr (BLA) deep_phoenix_orbit_x_bla(A, A.t, cx, cy, ec, inside, esc, ezx, ezy, np, nb);
                else deep_phoenix_orbit_x(A, cx, cy, ec, inside, esc, ezx, ezy);
            } else {
                if constexpr (BLA) deep_phoenix_orbit_bla(A, A.t, cx, cy, z1, inside, esc, ezx, ezy, np, nb);
                else deep_phoenix_orbit(A, cx, cy, z1, inside, esc, ezx, ezy);
            }
            if constexpr (BLA) {
                if (inside) {
                    n_plain += np; n_bla += nb;
                    n_upd += (unsigned long long)(esc < max_iter ? esc + 1 : max_iter);
                }
            }
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
    if constexpr (BLA) {
        unsigned long long v[3] = {n_plain, n_bla, n_upd - n_plain};
        for (int c = 0; c < 3; ++c) {
            for (int o = kWave / 2; o > 0; o >>= 1) v[c] += __shfl_xor(v[c], o, kWave);
            if (lane == 0) atomicAdd(A.t.steps + c, v[c]);
        }
    }
}

__global__ void __launch_bounds__(kBlockThreads)
deep_phoenix_kernel(const DeepPhoenixBlock<false> A) { deep_phoenix_kernel_body(A); }
__global__ void __launch_bounds__(kBlockThreads)
deep_phoenix_bla_kernel(const DeepPhoenixBlock<false, true> A) { deep_phoenix_kernel_body(A); }
__global__ void __launch_bounds__(kBlockThreads)
deep_phoenix_x_kernel(const DeepPhoenixBlock<true> A) { deep_phoenix_kernel_body(A); }
__global__ void __launch_bounds__(kBlockThreads)
deep_phoenix_x_bla_kernel(const DeepPhoenixBlock<true, true> A) { deep_phoenix_kernel_body(A); }

}  // namespace fr
