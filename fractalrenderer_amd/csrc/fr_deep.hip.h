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
 *
 * Bilinear approximation (FR_FLAG_DEEP_BLA; the semantics are in the header): deep_bla_level_kernel builds the table from the
 * device orbit, one launch per level, and deep_kernel<DeepBlaArgs> runs deep_orbit_bla as its per-sample loop.  The
 * table stores, level after level (level k from entry offset bla_offset(N - 1, k)), the radius r of every entry in an
 * array of doubles of its own and (A, B) in an array of double2 pairs: a probe gathers 8 bytes, only the chosen level's
 * 32 bytes of (A, B) are loaded.
 *
 * Extended-exponent deltas (fr_render_deepx; the arithmetic is in the header): deep_kernel<DeepXArgs> runs deep_orbit_x as
 * its per-sample loop.  A lane is in one of two modes.  Plain: deep_orbit's step on the plain doubles of the orbit.
 * Extended (max(|dz.x|, |dz.y|) < 2^-400): dz is two double mantissas and one int32 exponent, the orbit points come from
 * the mantissa and exponent arrays, alignment is v_ldexp_f64, and the one normalisation per step takes its exponent with
 * v_frexp_exp_i32_f64 off max(|x|, |y|); the mode test is an integer compare.  Z_m and Z_{m+1} stay in registers in the
 * lane's mode and Z_{m+2} is fetched one step ahead from that mode's arrays; a lane that changes mode reloads both.
 *
 * BLA for extended views (FR_FLAG_DEEPX_BLA; the semantics are in the header): deepx_bla_level_kernel builds a table whose
 * (A, B, r) carry int32 exponents from the extended orbit arrays, one launch per level, and deep_kernel<DeepXBlaArgs> runs
 * deep_orbit_x_bla: deep_orbit_x whose lanes, in either mode, probe the table as deep_orbit_bla does and take a BLA step in
 * extended arithmetic.  A probe gathers 8 bytes (r as a float mantissa and an int32 exponent); the chosen level's A and B
 * are 32 bytes of mantissas and 8 bytes of exponents in arrays of their own.
 *
 * Deep Burning Ship views (fr_render_deep_ship; the step is in the header): deep_kernel<DeepShipArgs> runs deep_orbit_ship as
 * its per-sample loop -- deep_orbit on (|Z_m|, fold(Z_m, dz)), the fold a pair of compares and selects, with deep_orbit's
 * registers and prefetch.  The orbit is the ship's own (fr_deep.c), dc is the Burning Ship shader's viewport map less the
 * centre (sx outer), and the colour stage is that of the fp64 Burning Ship path: shade<double, 2>, interior samples
 * black, the post chain with the Julia / Burning Ship floors.
 *
 * BLA for the ship (FR_FLAG_DEEP_SHIP_BLA; the semantics are in the header): while no fold flips a sign the ship's step less
 * its square term is a real 2x2 map, 2 |Z_m| times a rotation or reflection.  deep_ship_bla_level_kernel builds the table
 * from the ship's device orbit, one launch per level -- r in an array of doubles of its own, the eight doubles of (A, B) as
 * four double2 per entry -- and deep_kernel<DeepShipBlaArgs> runs deep_orbit_ship_bla: deep_orbit_ship whose lanes probe
 * the table as deep_orbit_bla does.  A probe gathers 8 bytes, only the chosen level's 64 bytes of (A, B) are loaded.
 *
 * Extended Burning Ship views (fr_render_deepx_ship; the step is in the header): deep_kernel<DeepShipXArgs> runs
 * deep_orbit_ship_x -- deep_orbit_x's two modes, registers, prefetch and mode changes around the ship's step.  The plain mode
 * is deep_orbit_ship's step; the extended mode takes the fold in the delta's frame (ship_fold_x: the orbit coordinate brought
 * to the delta's exponent by v_ldexp_f64, the same compares and selects), so a coordinate far below its partner, or exactly 0
 * on the real axis, still folds the delta it meets.  The viewport map and the colour stage are the ship's.
 *
 * BLA for extended ship views (FR_FLAG_DEEPX_SHIP_BLA; the semantics are in the header): the ship's real 2x2 maps carried as
 * four mantissas with one shared int32 exponent.  deepx_ship_bla_level_kernel builds the table from the ship's extended
 * orbit, one launch per level -- r as an XRad in an array of its own, the eight mantissas of (A, B) as four double2 and their
 * two exponents as an int2 per entry -- and deep_kernel<DeepShipXBlaArgs> runs deep_orbit_ship_x_bla: deep_orbit_ship_x whose
 * lanes, in either mode, probe the table as deep_orbit_x_bla does and take a BLA step in extended arithmetic.  A probe
 * gathers 8 bytes; the chosen level's 72 bytes of (A, B) are loaded inside the taken-step branch only.
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
    TileGeom g;
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

/* The BLA table of the cached orbit (deep_kernel<DeepBlaArgs> only) */
struct BlaTable {
    const double* r;                     /* r of every entry, level 1 first */
    const double2* ab;                   /* A, B of every entry: ab[2 e], ab[2 e + 1] */
    int32_t levels;                      /* K = floor(log2(N - 1)), 0 = no table */
    unsigned long long* steps;           /* plain steps, BLA steps, updates skipped: one atomic add each per wave */
};

struct DeepBlaArgs {
    DeepArgs d;
    BlaTable t;
};

/* Entries before level k (>= 1) of a table over n1 = N - 1 single steps: sum_{i=1}^{k-1} (n1 >> i).  With
 * S(x) = sum_{i>=1} (x >> i) = x - popcount(x) that is S(n1) - S(n1 >> (k - 1)). */
__device__ __forceinline__ uint32_t bla_offset(const uint32_t n1, const int k)
{
    const uint32_t t = n1 >> (k - 1);
    return (n1 - (uint32_t)__popc(n1)) - (t - (uint32_t)__popc(t));
}

/* |w| as the header writes it: sqrt(w.x*w.x + w.y*w.y).  On gfx950 sqrt(double) is LLVM's expansion of llvm.sqrt.f64:
 * scaling of small arguments, v_rsq_f64, two Newton-Raphson refinements of the root and half-reciprocal root, and a final
 * correction from the fma residual x - s*s -- the correctly rounded OCML sequence (tests/test_deep_bla_gpu.py compares
 * every radius of device-built tables with numpy's bit for bit). */
__device__ __forceinline__ double bla_abs(const double x, const double y) { return sqrt(x * x + y * y); }

/* Level k of the table: entry j merges x (level k - 1, entry 2j) and y (level k - 1, entry 2j + 1); level 0 is the single
 * step at m = 1 + i (A = 2 Z_m, B = 1, r = 2^-53 |Z_m|), computed from the orbit and never stored. */
__global__ void __launch_bounds__(kBlockThreads)
deep_bla_level_kernel(const double2* __restrict__ orbit, const int32_t n_ref, const int32_t k, const double dcmax,
                      double* __restrict__ r, double2* __restrict__ ab)
{
    const uint32_t n1 = (uint32_t)(n_ref - 1);
    const uint32_t cnt = n1 >> k;
    const uint32_t off = bla_offset(n1, k);
    const uint32_t offp = k > 1 ? bla_offset(n1, k - 1) : 0u;
    for (uint32_t j = blockIdx.x * kBlockThreads + threadIdx.x; j < cnt; j += gridDim.x * kBlockThreads) {
        double2 ax, bx, ay, by;
        double rx, ry;
        if (k == 1) {
            const double2 zx = orbit[1 + 2 * j], zy = orbit[2 + 2 * j];
            ax = make_double2(zx.x + zx.x, zx.y + zx.y); bx = make_double2(1.0, 0.0); rx = 0x1p-53 * bla_abs(zx.x, zx.y);
            ay = make_double2(zy.x + zy.x, zy.y + zy.y); by = make_double2(1.0, 0.0); ry = 0x1p-53 * bla_abs(zy.x, zy.y);
        } else {
            const uint32_t ex = offp + 2 * j, ey = ex + 1;
            ax = ab[2 * ex]; bx = ab[2 * ex + 1]; rx = r[ex];
            ay = ab[2 * ey]; by = ab[2 * ey + 1]; ry = r[ey];
        }
        const double2 a = make_double2(ay.x * ax.x - ay.y * ax.y, ay.x * ax.y + ay.y * ax.x);
        const double2 b = make_double2((ay.x * bx.x - ay.y * bx.y) + by.x, (ay.x * bx.y + ay.y * bx.x) + by.y);
        const double t = (ry - bla_abs(bx.x, bx.y) * dcmax) / bla_abs(ax.x, ax.y);
        double rr = t > 0.0 ? t : 0.0;                           /* NaN: 0 */
        rr = rr < rx ? rr : rx;
        if (!(__builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(b.x) && __builtin_isfinite(b.y)))
            rr = 0.0;
        const uint32_t e = off + j;
        r[e] = rr;
        ab[2 * e] = a;
        ab[2 * e + 1] = b;
    }
}

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

/* fr_render_deep_ship: d.orbit holds the Burning Ship orbit of the centre */
struct DeepShipArgs {
    DeepArgs d;
    double log_bailout;                  /* log(bailout), for shade<double, 2> at bailout <= 1 (LaunchArgs::log_bailout) */
};

/* |X + a| - |X| without the cancelling sum: the signs of X and of w = X + a (exact: an IEEE sum is zero only when it is
 * exactly zero) pick a, -a or +-(2X + a).  X2 = X + X.  Compares and selects, no branch. */
__device__ __forceinline__ double ship_fold(const double X, const double X2, const double a)
{
    const double w = X + a, d = X2 + a;
    const double up = w >= 0.0 ? a : -d;
    const double dn = w > 0.0 ? d : -a;
    return X >= 0.0 ? up : dn;
}

/* deep_orbit for z <- (|x| + i |y|)^2 + c: the same step on U = (|Z_m.x|, |Z_m.y|) and f = (fold(Z_m.x, dz.x),
 * fold(Z_m.y, dz.y)); z = Z_{m+1} + dz' with the signed orbit point, escape and rebase as there (Z_0 = 0: at m = 0 the
 * step is (|dz.x| + i |dz.y|)^2 + dc). */
__device__ __forceinline__ void deep_orbit_ship(const DeepArgs& A, const double dcx, const double dcy, const double2 z1,
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
        const double X2 = Zx + Zx, Y2 = Zy + Zy;
        const double fx = ship_fold(Zx, X2, dzx), fy = ship_fold(Zy, Y2, dzy);
        const double tx = fabs(X2) + fx, ty = fabs(Y2) + fy;     /* |X| + |X| = |X + X| */
        const double nx = (tx * fx - ty * fy) + dcx;
        const double ny = (tx * fy + ty * fx) + dcy;
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

/* deep_orbit with BLA: u replaces the loop index.  A lane at m >= 1 probes the levels top down from
 * min(ctz(m - 1), K, floor(log2(N - m)), floor(log2(max_iter - u))) and takes the first k with |dz|^2 < r^2.  No level's
 * r exceeds the single step's 2^-53 |Z_m| (r only ever shrinks in the merge), so a lane with
 * |dz|^2 2^104 >= |Z_m|^2 (a bound above 2^-106 |Z_m|^2 with room for every rounding) cannot pass a probe and gathers
 * nothing.  A BLA lane loads Z_m and Z_{m+1} at its new m (the Z_{m+2} prefetch is for the plain step); BLA and plain
 * lanes of a wave take their steps in the same trip.  nplain / nbla: the steps this sample took. */
__device__ __forceinline__ void deep_orbit_bla(const DeepArgs& A, const BlaTable& T, const double dcx, const double dcy,
                                               const double2 z1, bool live, int& esc, double& er2, uint32_t& nplain,
                                               uint32_t& nbla)
{
    const double2* __restrict__ orbit = A.orbit;
    const double* __restrict__ tr = T.r;
    const int N = A.n_ref, max_iter = A.max_iter, K = T.levels;
    const uint32_t n1 = (uint32_t)(N - 1);
    const double B2 = A.B2;
    double dzx = 0.0, dzy = 0.0;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m */
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    int m = 0, u = 0;
    esc = max_iter;
    er2 = 0.0;
    nplain = 0u; nbla = 0u;
    for (;;) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const double2 Znn = orbit[m + 2 <= N ? m + 2 : N];      /* Z_{m+2}, for a plain step */
        const double dz2 = dzx * dzx + dzy * dzy;
        int k = 0;
        uint32_t e = 0u;
        if (m >= 1 && dz2 * 0x1p104 < Zx * Zx + Zy * Zy) {
            const uint32_t mm = (uint32_t)(m - 1);
            int kk = mm ? __builtin_ctz(mm) : K;
            kk = kk < K ? kk : K;
            const int kn = 31 - __builtin_clz((uint32_t)(N - m));
            const int ki = 31 - __builtin_clz((uint32_t)(max_iter - u));
            kk = kk < kn ? kk : kn;
            kk = kk < ki ? kk : ki;
            for (; kk >= 1; --kk) {
                const uint32_t ek = bla_offset(n1, kk) + (mm >> kk);
                const double r = tr[ek];
                if (dz2 < r * r) { k = kk; e = ek; break; }
            }
        }
        double nx, ny, Zmx, Zmy;
        int step;
        if (k > 0) {
            const double2 a = T.ab[2 * e], b = T.ab[2 * e + 1];
            nx = (a.x * dzx - a.y * dzy) + (b.x * dcx - b.y * dcy);
            ny = (a.x * dzy + a.y * dzx) + (b.x * dcy + b.y * dcx);
            step = 1 << k;
            ++nbla;
            m += step;
            const double2 Zm = orbit[m];
            Zmx = Zm.x; Zmy = Zm.y;
        } else {
            const double tx = (Zx + Zx) + dzx, ty = (Zy + Zy) + dzy;
            nx = (tx * dzx - ty * dzy) + dcx;
            ny = (tx * dzy + ty * dzx) + dcy;
            step = 1;
            ++nplain;
            m += 1;
            Zmx = Znx; Zmy = Zny;
        }
        u += step;
        const double zx = Zmx + nx, zy = Zmy + ny;
        const double r2 = zx * zx + zy * zy;
        if (r2 > B2) {
            esc = u - 1; er2 = r2; live = false;                 /* the last update the step covered */
        } else if (r2 < nx * nx + ny * ny || m == N) {           /* rebase */
            dzx = zx; dzy = zy; m = 0;
            Zx = 0.0; Zy = 0.0; Znx = z1.x; Zny = z1.y;
        } else {
            dzx = nx; dzy = ny;
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
}

/* ---- BLA for the ship (FR_FLAG_DEEP_SHIP_BLA; the semantics are in the header) --------------------------------------------
 * The table of the ship's cached orbit: levels and offsets are those of the Mandelbrot table, an entry is r and the real
 * matrices A = (a11, a12, a21, a22), B = (b11, b12, b21, b22). */
struct ShipBlaTable {
    const double* r;                     /* r of every entry, level 1 first */
    const double2* ab;                   /* ab[4 e .. 4 e + 3] = (a11, a12), (a21, a22), (b11, b12), (b21, b22) */
    int32_t levels;                      /* K = floor(log2(N - 1)), 0 = no table */
    unsigned long long* steps;           /* plain steps, BLA steps, updates skipped: one atomic add each per wave */
};

struct DeepShipBlaArgs {
    DeepShipArgs s;
    ShipBlaTable t;
};

/* one entry while it is being merged: the rows of A and of B, and r */
struct ShipLin {
    double2 a1, a2, b1, b2;
    double r;
};

/* The single step at orbit point Z = (X, Y): A = [[2X, -2Y], [2|Y| sgn X, 2|X| sgn Y]], B = 1, r = 2^-53 |Z| capped by |X|
 * and |Y| (the fold conditions: below them no fold flips a sign). */
__device__ __forceinline__ ShipLin ship_single(const double2 Z)
{
    const double ax = fabs(Z.x), ay = fabs(Z.y);
    const double sx = Z.x >= 0.0 ? 1.0 : -1.0, sy = Z.y >= 0.0 ? 1.0 : -1.0;
    ShipLin s;
    s.a1 = make_double2(Z.x + Z.x, -(Z.y + Z.y));
    s.a2 = make_double2((ay + ay) * sx, (ax + ax) * sy);
    s.b1 = make_double2(1.0, 0.0);
    s.b2 = make_double2(0.0, 1.0);
    double r = 0x1p-53 * bla_abs(Z.x, Z.y);
    r = r < ax ? r : ax;
    r = r < ay ? r : ay;
    s.r = r;
    return s;
}

/* Level k of the ship's table: deep_bla_level_kernel with the real 2x2 products.  |A_x| is the length of A_x's first column
 * (A_x is a scaled orthogonal matrix: its operator norm), |B_x| the Frobenius norm. */
__global__ void __launch_bounds__(kBlockThreads)
deep_ship_bla_level_kernel(const double2* __restrict__ orbit, const int32_t n_ref, const int32_t k, const double dcmax,
                           double* __restrict__ r, double2* __restrict__ ab)
{
    const uint32_t n1 = (uint32_t)(n_ref - 1);
    const uint32_t cnt = n1 >> k;
    const uint32_t off = bla_offset(n1, k);
    const uint32_t offp = k > 1 ? bla_offset(n1, k - 1) : 0u;
    for (uint32_t j = blockIdx.x * kBlockThreads + threadIdx.x; j < cnt; j += gridDim.x * kBlockThreads) {
        ShipLin x, y;
        if (k == 1) {
            x = ship_single(orbit[1 + 2 * j]);
            y = ship_single(orbit[2 + 2 * j]);
        } else {
            const uint32_t ex = offp + 2 * j, ey = ex + 1;
            x.a1 = ab[4 * ex]; x.a2 = ab[4 * ex + 1]; x.b1 = ab[4 * ex + 2]; x.b2 = ab[4 * ex + 3]; x.r = r[ex];
            y.a1 = ab[4 * ey]; y.a2 = ab[4 * ey + 1]; y.b1 = ab[4 * ey + 2]; y.b2 = ab[4 * ey + 3]; y.r = r[ey];
        }
        const double2 a1 = make_double2(y.a1.x * x.a1.x + y.a1.y * x.a2.x, y.a1.x * x.a1.y + y.a1.y * x.a2.y);
        const double2 a2 = make_double2(y.a2.x * x.a1.x + y.a2.y * x.a2.x, y.a2.x * x.a1.y + y.a2.y * x.a2.y);
        const double2 b1 = make_double2((y.a1.x * x.b1.x + y.a1.y * x.b2.x) + y.b1.x, (y.a1.x * x.b1.y + y.a1.y * x.b2.y) + y.b1.y);
        const double2 b2 = make_double2((y.a2.x * x.b1.x + y.a2.y * x.b2.x) + y.b2.x, (y.a2.x * x.b1.y + y.a2.y * x.b2.y) + y.b2.y);
        const double nb = sqrt((x.b1.x * x.b1.x + x.b1.y * x.b1.y) + (x.b2.x * x.b2.x + x.b2.y * x.b2.y));
        const double t = (y.r - nb * dcmax) / bla_abs(x.a1.x, x.a2.x);
        double rr = t > 0.0 ? t : 0.0;                           /* NaN: 0 */
        rr = rr < x.r ? rr : x.r;
        if (!(__builtin_isfinite(a1.x) && __builtin_isfinite(a1.y) && __builtin_isfinite(a2.x) && __builtin_isfinite(a2.y) &&
              __builtin_isfinite(b1.x) && __builtin_isfinite(b1.y) && __builtin_isfinite(b2.x) && __builtin_isfinite(b2.y)))
            rr = 0.0;
        const uint32_t e = off + j;
        r[e] = rr;
        ab[4 * e] = a1;
        ab[4 * e + 1] = a2;
        ab[4 * e + 2] = b1;
        ab[4 * e + 3] = b2;
    }
}

/* deep_orbit_ship with BLA: u replaces the loop index, the probe is deep_orbit_bla's (no level's r exceeds the single step's
 * 2^-53 |Z_m|, so the same pre-filter holds).  The BLA branch loads the entry's eight doubles and Z_m, Z_{m+1} at its new
 * m; the plain branch is deep_orbit_ship's step with its Z_{m+2} prefetch. */
__device__ __forceinline__ void deep_orbit_ship_bla(const DeepArgs& A, const ShipBlaTable& T, const double dcx,
                                                    const double dcy, const double2 z1, bool live, int& esc, double& er2,
                                                    uint32_t& nplain, uint32_t& nbla)
{
    const double2* __restrict__ orbit = A.orbit;
    const double* __restrict__ tr = T.r;
    const double2* __restrict__ tab = T.ab;
    const int N = A.n_ref, max_iter = A.max_iter, K = T.levels;
    const uint32_t n1 = (uint32_t)(N - 1);
    const double B2 = A.B2;
    double dzx = 0.0, dzy = 0.0;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m */
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    int m = 0, u = 0;
    esc = max_iter;
    er2 = 0.0;
    nplain = 0u; nbla = 0u;
    for (;;) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const double2 Znn = orbit[m + 2 <= N ? m + 2 : N];      /* Z_{m+2}, for a plain step */
        const double dz2 = dzx * dzx + dzy * dzy;
        int k = 0;
        uint32_t e = 0u;
        if (m >= 1 && dz2 * 0x1p104 < Zx * Zx + Zy * Zy) {
            const uint32_t mm = (uint32_t)(m - 1);
            int kk = mm ? __builtin_ctz(mm) : K;
            kk = kk < K ? kk : K;
            const int kn = 31 - __builtin_clz((uint32_t)(N - m));
            const int ki = 31 - __builtin_clz((uint32_t)(max_iter - u));
            kk = kk < kn ? kk : kn;
            kk = kk < ki ? kk : ki;
            for (; kk >= 1; --kk) {
                const uint32_t ek = bla_offset(n1, kk) + (mm >> kk);
                const double r = tr[ek];
                if (dz2 < r * r) { k = kk; e = ek; break; }
            }
        }
        double nx, ny, Zmx, Zmy;
        int step;
        if (k > 0) {
            const double2 a1 = tab[4 * e], a2 = tab[4 * e + 1], b1 = tab[4 * e + 2], b2 = tab[4 * e + 3];
            nx = (a1.x * dzx + a1.y * dzy) + (b1.x * dcx + b1.y * dcy);
            ny = (a2.x * dzx + a2.y * dzy) + (b2.x * dcx + b2.y * dcy);
            step = 1 << k;
            ++nbla;
            m += step;
            const double2 Zm = orbit[m];
            Zmx = Zm.x; Zmy = Zm.y;
        } else {
            const double X2 = Zx + Zx, Y2 = Zy + Zy;
            const double fx = ship_fold(Zx, X2, dzx), fy = ship_fold(Zy, Y2, dzy);
            const double tx = fabs(X2) + fx, ty = fabs(Y2) + fy;     /* |X| + |X| = |X + X| */
            nx = (tx * fx - ty * fy) + dcx;
            ny = (tx * fy + ty * fx) + dcy;
            step = 1;
            ++nplain;
            m += 1;
            Zmx = Znx; Zmy = Zny;
        }
        u += step;
        const double zx = Zmx + nx, zy = Zmy + ny;
        const double r2 = zx * zx + zy * zy;
        if (r2 > B2) {
            esc = u - 1; er2 = r2; live = false;                 /* the last update the step covered */
        } else if (r2 < nx * nx + ny * ny || m == N) {           /* rebase */
            dzx = zx; dzy = zy; m = 0;
            Zx = 0.0; Zy = 0.0; Znx = z1.x; Zny = z1.y;
        } else {
            dzx = nx; dzy = ny;
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
}

/* fr_render_deepx: d.orbit holds the plain doubles P_n, d.zoom is not read */
struct DeepXArgs {
    DeepArgs d;
    const double2* mant;                 /* (mx, my) of Z_0 .. Z_N */
    const int32_t* exp2;                 /* e of Z_0 .. Z_N */
    double zm;                           /* zoom = zm 2^ze */
    int32_t ze;
};

constexpr int kXZero = FR_DEEPX_ZERO_EXP;
constexpr int kXThr = -400;              /* extended while the normalised dz.e <= kXThr */

/* norm(x, y, e) of the header */
__device__ __forceinline__ void x_norm(double& x, double& y, int& e)
{
    const double mx = fmax(fabs(x), fabs(y));
    const int k = __builtin_amdgcn_frexp_exp(mx);
    x = __builtin_ldexp(x, -k);
    y = __builtin_ldexp(y, -k);
    e = mx == 0.0 ? kXZero : e + k;
}

/* deep_orbit in two modes (the header's EXTENDED and PLAIN steps).  (cx, cy, ec) = dc, normalised. */
__device__ __forceinline__ void deep_orbit_x(const DeepXArgs& AA, const double cx, const double cy, const int ec, bool live,
                                             int& esc, double& er2)
{
    const DeepArgs& A = AA.d;
    const double2* __restrict__ orbit = A.orbit;
    const double2* __restrict__ mant = AA.mant;
    const int32_t* __restrict__ exp2 = AA.exp2;
    const int N = A.n_ref, max_iter = A.max_iter;
    const double B2 = A.B2;
    /* the plain mode's dc: a component below 2^-1022 is 0 */
    const double cpx = (cx != 0.0 && __builtin_amdgcn_frexp_exp(cx) + ec > -1022) ? __builtin_ldexp(cx, ec) : 0.0;
    const double cpy = (cy != 0.0 && __builtin_amdgcn_frexp_exp(cy) + ec > -1022) ? __builtin_ldexp(cy, ec) : 0.0;
    double dzx = 0.0, dzy = 0.0;                                 /* plain: dz; extended: its mantissas */
    int ed = kXZero;
    bool ext = true;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m, in the lane's mode */
    int eZ = kXZero;
    const double2 z1 = mant[1];
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    int eZn = exp2[1];
    int m = 0;
    esc = max_iter;
    er2 = 0.0;
    for (int i = 0; i < max_iter; ++i) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const int mn = m + 2 <= N ? m + 2 : N;                   /* Z_{m+2}, for the next step (m + 1 < N) */
        double ax, ay;                                           /* the next dz */
        int ea = 0;
        bool reb;
        if (ext) {
            const double2 Znn = mant[mn];
            const int eZnn = exp2[mn];
            const int et = eZ + 1 > ed ? eZ + 1 : ed;
            const double tx = __builtin_ldexp(Zx, eZ + 1 - et) + __builtin_ldexp(dzx, ed - et);
            const double ty = __builtin_ldexp(Zy, eZ + 1 - et) + __builtin_ldexp(dzy, ed - et);
            const double px = tx * dzx - ty * dzy;
            const double py = tx * dzy + ty * dzx;
            const int ep = et + ed;
            const int en = ep > ec ? ep : ec;
            const double nx = __builtin_ldexp(px, ep - en) + __builtin_ldexp(cx, ec - en);
            const double ny = __builtin_ldexp(py, ep - en) + __builtin_ldexp(cy, ec - en);
            ++m;
            const int ez = eZn > en ? eZn : en;
            const double zx = __builtin_ldexp(Znx, eZn - ez) + __builtin_ldexp(nx, en - ez);
            const double zy = __builtin_ldexp(Zny, eZn - ez) + __builtin_ldexp(ny, en - ez);
            const double r2 = zx * zx + zy * zy;
            const double r2d = __builtin_ldexp(r2, 2 * ez);
            if (r2d > B2) {
                esc = i; er2 = r2d; live = false;
                continue;
            }
            reb = r2 < __builtin_ldexp(nx * nx + ny * ny, 2 * (en - ez)) || m == N;
            ax = reb ? zx : nx; ay = reb ? zy : ny; ea = reb ? ez : en;
            x_norm(ax, ay, ea);
            if (reb) m = 0;
            if (ea <= kXThr) {                                    /* stays extended */
                dzx = ax; dzy = ay; ed = ea;
                if (reb) {
                    Zx = 0.0; Zy = 0.0; eZ = kXZero; Znx = z1.x; Zny = z1.y; eZn = exp2[1];
                } else {
                    Zx = Znx; Zy = Zny; eZ = eZn; Znx = Znn.x; Zny = Znn.y; eZn = eZnn;
                }
                continue;
            }
            dzx = __builtin_ldexp(ax, ea); dzy = __builtin_ldexp(ay, ea);
            ext = false;
        } else {
            const double2 Znn = orbit[mn];
            const double tx = (Zx + Zx) + dzx, ty = (Zy + Zy) + dzy;
            const double nx = (tx * dzx - ty * dzy) + cpx;
            const double ny = (tx * dzy + ty * dzx) + cpy;
            ++m;
            const double zx = Znx + nx, zy = Zny + ny;
            const double r2 = zx * zx + zy * zy;
            if (r2 > B2) {
                esc = i; er2 = r2; live = false;
                continue;
            }
            reb = r2 < nx * nx + ny * ny || m == N;
            ax = reb ? zx : nx; ay = reb ? zy : ny;
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
            x_norm(ax, ay, ea);
            dzx = ax; dzy = ay; ed = ea;
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
}

/* fr_render_deepx_ship: x.d.orbit holds the plain doubles P_n of the ship's orbit, x.mant / x.exp2 its extended storage */
struct DeepShipXArgs {
    DeepXArgs x;
    double log_bailout;                  /* as DeepShipArgs */
};

/* fold_x of the header: ship_fold on an orbit mantissa X at exponent eZ and a delta mantissa a at exponent ed, s = eZ - ed,
 * taken in the delta's frame -- the result is a mantissa at ed.  X far above the delta: the ldexp may give +-inf, w has X's
 * sign, the select returns +-a and drops the infinite d.  X far below: Xs is 0 or a subnormal, below half an ulp of a. */
__device__ __forceinline__ double ship_fold_x(const double X, const int s, const double a)
{
    const double Xs = __builtin_ldexp(X, s), X2s = __builtin_ldexp(X, s + 1);
    const double w = Xs + a, d = X2s + a;
    const double up = w >= 0.0 ? a : -d;
    const double dn = w > 0.0 ? d : -a;
    return X >= 0.0 ? up : dn;
}

/* deep_orbit_x for z <- (|x| + i |y|)^2 + c (the header's EXTENDED and PLAIN steps of fr_render_deepx_ship): the extended
 * step on U = (|Z_m.x|, |Z_m.y|, Z_m.e + 1) and f = (fold_x, fold_x, dz.e), the plain step deep_orbit_ship's; z = Z_{m+1} (+) n
 * with the signed orbit point, escape, rebase, norm and the mode rule as in deep_orbit_x.  (cx, cy, ec) = dc, normalised. */
__device__ __forceinline__ void deep_orbit_ship_x(const DeepXArgs& AA, const double cx, const double cy, const int ec,
                                                  bool live, int& esc, double& er2)
{
    const DeepArgs& A = AA.d;
    const double2* __restrict__ orbit = A.orbit;
    const double2* __restrict__ mant = AA.mant;
    const int32_t* __restrict__ exp2 = AA.exp2;
    const int N = A.n_ref, max_iter = A.max_iter;
    const double B2 = A.B2;
    /* the plain mode's dc: a component below 2^-1022 is 0 */
    const double cpx = (cx != 0.0 && __builtin_amdgcn_frexp_exp(cx) + ec > -1022) ? __builtin_ldexp(cx, ec) : 0.0;
    const double cpy = (cy != 0.0 && __builtin_amdgcn_frexp_exp(cy) + ec > -1022) ? __builtin_ldexp(cy, ec) : 0.0;
    double dzx = 0.0, dzy = 0.0;                                 /* plain: dz; extended: its mantissas */
    int ed = kXZero;
    bool ext = true;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m, in the lane's mode */
    int eZ = kXZero;
    const double2 z1 = mant[1];
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    int eZn = exp2[1];
    int m = 0;
    esc = max_iter;
    er2 = 0.0;
    for (int i = 0; i < max_iter; ++i) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const int mn = m + 2 <= N ? m + 2 : N;                   /* Z_{m+2}, for the next step (m + 1 < N) */
        double ax, ay;                                           /* the next dz */
        int ea = 0;
        bool reb;
        if (ext) {
            const double2 Znn = mant[mn];
            const int eZnn = exp2[mn];
            const double fx = ship_fold_x(Zx, eZ - ed, dzx), fy = ship_fold_x(Zy, eZ - ed, dzy);
            const int et = eZ + 1 > ed ? eZ + 1 : ed;
            const double tx = __builtin_ldexp(fabs(Zx), eZ + 1 - et) + __builtin_ldexp(fx, ed - et);
            const double ty = __builtin_ldexp(fabs(Zy), eZ + 1 - et) + __builtin_ldexp(fy, ed - et);
            const double px = tx * fx - ty * fy;
            const double py = tx * fy + ty * fx;
            const int ep = et + ed;
            const int en = ep > ec ? ep : ec;
            const double nx = __builtin_ldexp(px, ep - en) + __builtin_ldexp(cx, ec - en);
            const double ny = __builtin_ldexp(py, ep - en) + __builtin_ldexp(cy, ec - en);
            ++m;
            const int ez = eZn > en ? eZn : en;
            const double zx = __builtin_ldexp(Znx, eZn - ez) + __builtin_ldexp(nx, en - ez);
            const double zy = __builtin_ldexp(Zny, eZn - ez) + __builtin_ldexp(ny, en - ez);
            const double r2 = zx * zx + zy * zy;
            const double r2d = __builtin_ldexp(r2, 2 * ez);
            if (r2d > B2) {
                esc = i; er2 = r2d; live = false;
                continue;
            }
            reb = r2 < __builtin_ldexp(nx * nx + ny * ny, 2 * (en - ez)) || m == N;
            ax = reb ? zx : nx; ay = reb ? zy : ny; ea = reb ? ez : en;
            x_norm(ax, ay, ea);
            if (reb) m = 0;
            if (ea <= kXThr) {                                    /* stays extended */
                dzx = ax; dzy = ay; ed = ea;
                if (reb) {
                    Zx = 0.0; Zy = 0.0; eZ = kXZero; Znx = z1.x; Zny = z1.y; eZn = exp2[1];
                } else {
                    Zx = Znx; Zy = Zny; eZ = eZn; Znx = Znn.x; Zny = Znn.y; eZn = eZnn;
                }
                continue;
            }
            dzx = __builtin_ldexp(ax, ea); dzy = __builtin_ldexp(ay, ea);
            ext = false;
        } else {
            const double2 Znn = orbit[mn];
            const double X2 = Zx + Zx, Y2 = Zy + Zy;
            const double fx = ship_fold(Zx, X2, dzx), fy = ship_fold(Zy, Y2, dzy);
            const double tx = fabs(X2) + fx, ty = fabs(Y2) + fy;     /* |X| + |X| = |X + X| */
            const double nx = (tx * fx - ty * fy) + cpx;
            const double ny = (tx * fy + ty * fx) + cpy;
            ++m;
            const double zx = Znx + nx, zy = Zny + ny;
            const double r2 = zx * zx + zy * zy;
            if (r2 > B2) {
                esc = i; er2 = r2; live = false;
                continue;
            }
            reb = r2 < nx * nx + ny * ny || m == N;
            ax = reb ? zx : nx; ay = reb ? zy : ny;
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
            x_norm(ax, ay, ea);
            dzx = ax; dzy = ay; ed = ea;
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
}

/* ---- BLA for extended views (FR_FLAG_DEEPX_BLA; the semantics are in the header) -----------------------------------------
 * The table of the extended orbit: per entry the radius r as 8 bytes (XRad: the top 24 bits of its mantissa as a float and
 * its int32 exponent -- what a probe gathers), and apart from it (A, B) as two double2 of normalised mantissas with their
 * two exponents in an int2, loaded for the chosen level only.  Levels and offsets are those of the fp64 table. */
struct XRad {
    float v;                             /* mantissa in [0.5, 1), 0 for r = 0 */
    int32_t e;                           /* FR_DEEPX_ZERO_EXP for r = 0 */
};

struct BlaXTable {
    const XRad* r;                       /* r of every entry, level 1 first */
    const double2* ab;                   /* mantissas of A, B: ab[2 e], ab[2 e + 1] */
    const int2* abe;                     /* (A.e, B.e) */
    int32_t levels;                      /* K = floor(log2(N - 1)), 0 = no table */
    unsigned long long* steps;           /* single steps, BLA steps, updates skipped: one atomic add each per wave */
};

struct DeepXBlaArgs {
    DeepXArgs x;
    BlaXTable t;
};

constexpr int kXBlaExpLim = 1 << 27;     /* an entry whose A.e or B.e leaves [-2^27, 2^27] is void */

/* an extended real normalised: v into [0.5, 1), zero gets FR_DEEPX_ZERO_EXP */
__device__ __forceinline__ void x_norm1(double& v, int& e)
{
    const int k = __builtin_amdgcn_frexp_exp(v);
    e = v == 0.0 ? kXZero : e + k;
    v = __builtin_ldexp(v, -k);
}

/* the top 24 bits of a mantissa in [0.5, 1) (toward zero): exactly a float */
__device__ __forceinline__ double x_trunc24(const double v)
{
    return __longlong_as_double(__double_as_longlong(v) & ~((1ll << 29) - 1));
}

/* Level k of the extended table.  Level 0 is the single step at m = 1 + i (A = norm(Z_m.x, Z_m.y, Z_m.e + 1), B = norm(1, 0, 0),
 * r = 2^-53 |Z_m|), computed from the orbit and never stored. */
__global__ void __launch_bounds__(kBlockThreads)
deepx_bla_level_kernel(const double2* __restrict__ mant, const int32_t* __restrict__ exp2, const int32_t n_ref, const int32_t k,
                       const double dcv, const int32_t dce, XRad* __restrict__ r, double2* __restrict__ ab,
                       int2* __restrict__ abe)
{
    const uint32_t n1 = (uint32_t)(n_ref - 1);
    const uint32_t cnt = n1 >> k;
    const uint32_t off = bla_offset(n1, k);
    const uint32_t offp = k > 1 ? bla_offset(n1, k - 1) : 0u;
    for (uint32_t j = blockIdx.x * kBlockThreads + threadIdx.x; j < cnt; j += gridDim.x * kBlockThreads) {
        double2 A[2], B[2];                                      /* x, y */
        int eA[2], eB[2], eR[2];
        double R[2];
        if (k == 1) {
            for (int s = 0; s < 2; ++s) {
                const double2 z = mant[1 + s + 2 * j];
                const int ez = exp2[1 + s + 2 * j];
                A[s] = z; eA[s] = ez + 1;
                x_norm(A[s].x, A[s].y, eA[s]);
                B[s] = make_double2(0.5, 0.0); eB[s] = 1;
                double nx = z.x, ny = z.y;
                int ne = ez;
                x_norm(nx, ny, ne);
                R[s] = bla_abs(nx, ny); eR[s] = ne;
                x_norm1(R[s], eR[s]);
                if (R[s] != 0.0) eR[s] -= 53;
            }
        } else {
            for (int s = 0; s < 2; ++s) {
                const uint32_t e = offp + 2 * j + s;
                const int2 ee = abe[e];
                const XRad rr = r[e];
                A[s] = ab[2 * e]; B[s] = ab[2 * e + 1]; eA[s] = ee.x; eB[s] = ee.y;
                R[s] = (double)rr.v; eR[s] = rr.e;
            }
        }
        double2 a = make_double2(A[1].x * A[0].x - A[1].y * A[0].y, A[1].x * A[0].y + A[1].y * A[0].x);
        int ea = eA[1] + eA[0];
        x_norm(a.x, a.y, ea);
        const double px = A[1].x * B[0].x - A[1].y * B[0].y, py = A[1].x * B[0].y + A[1].y * B[0].x;
        const int e1 = eA[1] + eB[0];
        int eb = e1 > eB[1] ? e1 : eB[1];
        double2 b = make_double2(__builtin_ldexp(px, e1 - eb) + __builtin_ldexp(B[1].x, eB[1] - eb),
                                 __builtin_ldexp(py, e1 - eb) + __builtin_ldexp(B[1].y, eB[1] - eb));
        x_norm(b.x, b.y, eb);
        double bv = bla_abs(B[0].x, B[0].y), av = bla_abs(A[0].x, A[0].y);
        int be = eB[0], ae = eA[0];
        x_norm1(bv, be);
        x_norm1(av, ae);
        const double pv = bv * dcv;
        const int pe = be + dce;
        const int et = eR[1] > pe ? eR[1] : pe;
        const double t = (__builtin_ldexp(R[1], eR[1] - et) - __builtin_ldexp(pv, pe - et)) / av;
        double rv = (t > 0.0 && __builtin_isfinite(t)) ? t : 0.0;    /* NaN: 0 */
        int re = et - ae;
        x_norm1(rv, re);
        if (!(re < eR[0] || (re == eR[0] && rv < R[0]))) { rv = R[0]; re = eR[0]; }
        const int la = ea < 0 ? -ea : ea, lb = eb < 0 ? -eb : eb;
        if (la > kXBlaExpLim || lb > kXBlaExpLim) {
            rv = 0.0; re = kXZero;
            a = make_double2(0.0, 0.0); ea = kXZero;
            b = make_double2(0.0, 0.0); eb = kXZero;
        }
        const uint32_t e = off + j;
        XRad out;
        out.v = (float)x_trunc24(rv); out.e = re;
        r[e] = out;
        ab[2 * e] = a;
        ab[2 * e + 1] = b;
        abe[e] = make_int2(ea, eb);
    }
}

/* deep_orbit_x with BLA: u replaces the loop index.  A lane at m >= 1, in either mode, probes the levels top down as
 * deep_orbit_bla does, on its dz as a normalised extended number (a plain lane forms norm(dz.x, dz.y, 0)), and takes the
 * first k with |dz|^2 < r^2; the step is then taken in extended arithmetic whatever the lane's mode, and the lane reloads
 * Z_m, Z_{m+1} in the mode the step leaves it in.  No level's r exceeds 2^-53 |Z_m| < 2^(E - 52.5), E the exponent of Z_m's
 * larger component normalised, and |dz| >= 2^(dz.e - 1): a lane with dz.e + 51 >= E cannot pass a probe and gathers nothing
 * (E from the lane's own copy of Z_m: for a point below 2^-1022 the plain double's exponent is never below the true one).
 * BLA lanes and single-step lanes of a wave take their steps in the same trip.  nsingle / nbla: the steps this sample took. */
__device__ __forceinline__ void deep_orbit_x_bla(const DeepXArgs& AA, const BlaXTable& T, const double cx, const double cy,
                                                 const int ec, bool live, int& esc, double& er2, uint32_t& nsingle,
                                                 uint32_t& nbla)
{
    const DeepArgs& A = AA.d;
    const double2* __restrict__ orbit = A.orbit;
    const double2* __restrict__ mant = AA.mant;
    const int32_t* __restrict__ exp2 = AA.exp2;
    const XRad* __restrict__ tr = T.r;
    const int N = A.n_ref, max_iter = A.max_iter, K = T.levels;
    const uint32_t n1 = (uint32_t)(N - 1);
    const double B2 = A.B2;
    const double cpx = (cx != 0.0 && __builtin_amdgcn_frexp_exp(cx) + ec > -1022) ? __builtin_ldexp(cx, ec) : 0.0;
    const double cpy = (cy != 0.0 && __builtin_amdgcn_frexp_exp(cy) + ec > -1022) ? __builtin_ldexp(cy, ec) : 0.0;
    double dzx = 0.0, dzy = 0.0;                                 /* plain: dz; extended: its mantissas */
    int ed = kXZero;
    bool ext = true;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m, in the lane's mode */
    int eZ = kXZero;
    const double2 z1 = mant[1];
    const int e1 = exp2[1];
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    int eZn = e1;
    int m = 0, u = 0;
    esc = max_iter;
    er2 = 0.0;
    nsingle = 0u; nbla = 0u;
    for (;;) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const int mn = m + 2 <= N ? m + 2 : N;                   /* Z_{m+2}, for the single step after this one */
        int k = 0;
        uint32_t e = 0u;
        double qx = dzx, qy = dzy;                               /* dz, extended and normalised */
        int qe = ed;
        if (m >= 1) {
            if (!ext) { qe = 0; x_norm(qx, qy, qe); }
            const int eZm = (ext ? eZ : 0) + __builtin_amdgcn_frexp_exp(fmax(fabs(Zx), fabs(Zy)));
            if (qe + 51 < eZm) {
                const double dz2 = qx * qx + qy * qy;
                const uint32_t mm = (uint32_t)(m - 1);
                int kk = mm ? __builtin_ctz(mm) : K;
                kk = kk < K ? kk : K;
                const int kn = 31 - __builtin_clz((uint32_t)(N - m));
                const int ki = 31 - __builtin_clz((uint32_t)(max_iter - u));
                kk = kk < kn ? kk : kn;
                kk = kk < ki ? kk : ki;
                for (; kk >= 1; --kk) {
                    const uint32_t ek = bla_offset(n1, kk) + (mm >> kk);
                    const XRad r = tr[ek];
                    const double rv = (double)r.v;
                    if (dz2 < __builtin_ldexp(rv * rv, 2 * (r.e - qe))) { k = kk; e = ek; break; }
                }
            }
        }
        double ax, ay;                                           /* the next dz */
        int ea = 0;
        bool reb;
        if (k > 0 || ext) {
            double nx, ny, Wx, Wy;                               /* n and Z at the new m */
            int en, eW, eZnn = 0;
            double2 Znn = make_double2(0.0, 0.0);
            if (k > 0) {
                const double2 a = T.ab[2 * e], b = T.ab[2 * e + 1];
                const int2 ee = T.abe[e];
                const double px = a.x * qx - a.y * qy, py = a.x * qy + a.y * qx;
                const double sx = b.x * cx - b.y * cy, sy = b.x * cy + b.y * cx;
                const int ep = ee.x + qe, es = ee.y + ec;
                en = ep > es ? ep : es;
                nx = __builtin_ldexp(px, ep - en) + __builtin_ldexp(sx, es - en);
                ny = __builtin_ldexp(py, ep - en) + __builtin_ldexp(sy, es - en);
                m += 1 << k;
                u += 1 << k;
                ++nbla;
                const double2 Wm = mant[m];
                Wx = Wm.x; Wy = Wm.y; eW = exp2[m];
            } else {
                Znn = mant[mn];
                eZnn = exp2[mn];
                const int et = eZ + 1 > ed ? eZ + 1 : ed;
                const double tx = __builtin_ldexp(Zx, eZ + 1 - et) + __builtin_ldexp(dzx, ed - et);
                const double ty = __builtin_ldexp(Zy, eZ + 1 - et) + __builtin_ldexp(dzy, ed - et);
                const double px = tx * dzx - ty * dzy;
                const double py = tx * dzy + ty * dzx;
                const int ep = et + ed;
                en = ep > ec ? ep : ec;
                nx = __builtin_ldexp(px, ep - en) + __builtin_ldexp(cx, ec - en);
                ny = __builtin_ldexp(py, ep - en) + __builtin_ldexp(cy, ec - en);
                ++m;
                ++u;
                ++nsingle;
                Wx = Znx; Wy = Zny; eW = eZn;
            }
            const int ez = eW > en ? eW : en;
            const double zx = __builtin_ldexp(Wx, eW - ez) + __builtin_ldexp(nx, en - ez);
            const double zy = __builtin_ldexp(Wy, eW - ez) + __builtin_ldexp(ny, en - ez);
            const double r2 = zx * zx + zy * zy;
            const double r2d = __builtin_ldexp(r2, 2 * ez);
            if (r2d > B2) {
                esc = u - 1; er2 = r2d; live = false;             /* the last update the step covered */
                continue;
            }
            reb = r2 < __builtin_ldexp(nx * nx + ny * ny, 2 * (en - ez)) || m == N;
            ax = reb ? zx : nx; ay = reb ? zy : ny; ea = reb ? ez : en;
            x_norm(ax, ay, ea);
            if (reb) m = 0;
            if (ea <= kXThr) {                                    /* extended from here */
                dzx = ax; dzy = ay; ed = ea;
                ext = true;
                if (reb) {
                    Zx = 0.0; Zy = 0.0; eZ = kXZero; Znx = z1.x; Zny = z1.y; eZn = e1;
                } else if (k == 0) {
                    Zx = Znx; Zy = Zny; eZ = eZn; Znx = Znn.x; Zny = Znn.y; eZn = eZnn;
                } else {                                          /* m < N here */
                    const double2 b = mant[m + 1];
                    Zx = Wx; Zy = Wy; eZ = eW; Znx = b.x; Zny = b.y; eZn = exp2[m + 1];
                }
            } else {                                              /* plain from here (m < N) */
                const double2 a = orbit[m], b = orbit[m + 1];
                dzx = __builtin_ldexp(ax, ea); dzy = __builtin_ldexp(ay, ea);
                ext = false;
                Zx = a.x; Zy = a.y; Znx = b.x; Zny = b.y;
            }
        } else {
            const double2 Znn = orbit[mn];
            const double tx = (Zx + Zx) + dzx, ty = (Zy + Zy) + dzy;
            const double nx = (tx * dzx - ty * dzy) + cpx;
            const double ny = (tx * dzy + ty * dzx) + cpy;
            ++m;
            ++u;
            ++nsingle;
            const double zx = Znx + nx, zy = Zny + ny;
            const double r2 = zx * zx + zy * zy;
            if (r2 > B2) {
                esc = u - 1; er2 = r2; live = false;
                continue;
            }
            reb = r2 < nx * nx + ny * ny || m == N;
            ax = reb ? zx : nx; ay = reb ? zy : ny;
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
                x_norm(ax, ay, ea);
                dzx = ax; dzy = ay; ed = ea;
                ext = true;
                Zx = a.x; Zy = a.y; eZ = exp2[m]; Znx = b.x; Zny = b.y; eZn = exp2[m + 1];
            }
        }
        if (u >= max_iter) live = false;                          /* esc stays max_iter */
    }
}

/* ---- BLA for extended ship views (FR_FLAG_DEEPX_SHIP_BLA; the semantics are in the header) ---------------------------------
 * The table of the ship's extended orbit: per entry the radius as an XRad (what a probe gathers), and apart from it the real
 * matrices A and B as four double2 of mantissas -- (a11, a12), (a21, a22), (b11, b12), (b21, b22), each matrix normalised on
 * its largest element -- with their two shared exponents in an int2, loaded for the chosen level only.  Levels and offsets
 * are those of the fp64 table. */
struct ShipXBlaTable {
    const XRad* r;                       /* r of every entry, level 1 first */
    const double2* ab;                   /* ab[4 e .. 4 e + 3]: the rows of A and of B, mantissas */
    const int2* abe;                     /* (A.e, B.e) */
    int32_t levels;                      /* K = floor(log2(N - 1)), 0 = no table */
    unsigned long long* steps;           /* single steps, BLA steps, updates skipped: one atomic add each per wave */
};

struct DeepShipXBlaArgs {
    DeepShipXArgs s;
    ShipXBlaTable t;
};

/* norm4 of the header: a matrix's four mantissas normalised on the largest of them */
__device__ __forceinline__ void x_norm4(double2& r1, double2& r2, int& e)
{
    const double mx = fmax(fmax(fabs(r1.x), fabs(r1.y)), fmax(fabs(r2.x), fabs(r2.y)));
    const int k = __builtin_amdgcn_frexp_exp(mx);
    r1.x = __builtin_ldexp(r1.x, -k); r1.y = __builtin_ldexp(r1.y, -k);
    r2.x = __builtin_ldexp(r2.x, -k); r2.y = __builtin_ldexp(r2.y, -k);
    e = mx == 0.0 ? kXZero : e + k;
}

/* one entry while it is being merged: the rows of A and of B with their exponents, and r */
struct ShipXLin {
    double2 a1, a2, b1, b2;
    int ea, eb;
    double rv;
    int re;
};

/* (v, e) < (w, f) on normalised extended reals; the zero's exponent FR_DEEPX_ZERO_EXP is below every other */
__device__ __forceinline__ bool x_less(const double v, const int e, const double w, const int f)
{
    return e < f || (e == f && v < w);
}

/* The single step at the extended orbit point Z = (X, Y) 2^eZ: ship_single with the doubling in A's exponent, r = 2^-53 |norm(Z)|
 * capped by |X| and |Y| as extended reals (a coordinate stored as 0 gives r = 0). */
__device__ __forceinline__ ShipXLin shipx_single(const double2 Z, const int eZ)
{
    const double ax = fabs(Z.x), ay = fabs(Z.y);
    const double sx = Z.x >= 0.0 ? 1.0 : -1.0, sy = Z.y >= 0.0 ? 1.0 : -1.0;
    ShipXLin s;
    s.a1 = make_double2(Z.x, -Z.y);
    s.a2 = make_double2(ay * sx, ax * sy);
    s.ea = eZ + 1;
    x_norm4(s.a1, s.a2, s.ea);
    s.b1 = make_double2(0.5, 0.0);
    s.b2 = make_double2(0.0, 0.5);
    s.eb = 1;
    double nx = Z.x, ny = Z.y;
    int ne = eZ;
    x_norm(nx, ny, ne);
    double rv = bla_abs(nx, ny);
    int re = ne;
    x_norm1(rv, re);
    if (rv != 0.0) re -= 53;
    double cv = ax;
    int ce = eZ;
    x_norm1(cv, ce);
    if (!x_less(rv, re, cv, ce)) { rv = cv; re = ce; }
    cv = ay; ce = eZ;
    x_norm1(cv, ce);
    if (!x_less(rv, re, cv, ce)) { rv = cv; re = ce; }
    s.rv = rv; s.re = re;
    return s;
}

/* Level k of the extended ship table: deep_ship_bla_level_kernel's products and norms in deepx_bla_level_kernel's arithmetic
 * (t, the r < r_x rule, the void rule and the 24-bit cut of the stored radius are that kernel's). */
__global__ void __launch_bounds__(kBlockThreads)
deepx_ship_bla_level_kernel(const double2* __restrict__ mant, const int32_t* __restrict__ exp2, const int32_t n_ref,
                            const int32_t k, const double dcv, const int32_t dce, XRad* __restrict__ r,
                            double2* __restrict__ ab, int2* __restrict__ abe)
{
    const uint32_t n1 = (uint32_t)(n_ref - 1);
    const uint32_t cnt = n1 >> k;
    const uint32_t off = bla_offset(n1, k);
    const uint32_t offp = k > 1 ? bla_offset(n1, k - 1) : 0u;
    for (uint32_t j = blockIdx.x * kBlockThreads + threadIdx.x; j < cnt; j += gridDim.x * kBlockThreads) {
        ShipXLin x, y;
        if (k == 1) {
            x = shipx_single(mant[1 + 2 * j], exp2[1 + 2 * j]);
            y = shipx_single(mant[2 + 2 * j], exp2[2 + 2 * j]);
        } else {
            const uint32_t ex = offp + 2 * j, ey = ex + 1;
            const int2 eex = abe[ex], eey = abe[ey];
            const XRad rx = r[ex], ry = r[ey];
            x.a1 = ab[4 * ex]; x.a2 = ab[4 * ex + 1]; x.b1 = ab[4 * ex + 2]; x.b2 = ab[4 * ex + 3];
            x.ea = eex.x; x.eb = eex.y; x.rv = (double)rx.v; x.re = rx.e;
            y.a1 = ab[4 * ey]; y.a2 = ab[4 * ey + 1]; y.b1 = ab[4 * ey + 2]; y.b2 = ab[4 * ey + 3];
            y.ea = eey.x; y.eb = eey.y; y.rv = (double)ry.v; y.re = ry.e;
        }
        double2 a1 = make_double2(y.a1.x * x.a1.x + y.a1.y * x.a2.x, y.a1.x * x.a1.y + y.a1.y * x.a2.y);
        double2 a2 = make_double2(y.a2.x * x.a1.x + y.a2.y * x.a2.x, y.a2.x * x.a1.y + y.a2.y * x.a2.y);
        int ea = y.ea + x.ea;
        x_norm4(a1, a2, ea);
        const double2 p1 = make_double2(y.a1.x * x.b1.x + y.a1.y * x.b2.x, y.a1.x * x.b1.y + y.a1.y * x.b2.y);
        const double2 p2 = make_double2(y.a2.x * x.b1.x + y.a2.y * x.b2.x, y.a2.x * x.b1.y + y.a2.y * x.b2.y);
        const int e1 = y.ea + x.eb;
        int eb = e1 > y.eb ? e1 : y.eb;
        double2 b1 = make_double2(__builtin_ldexp(p1.x, e1 - eb) + __builtin_ldexp(y.b1.x, y.eb - eb),
                                  __builtin_ldexp(p1.y, e1 - eb) + __builtin_ldexp(y.b1.y, y.eb - eb));
        double2 b2 = make_double2(__builtin_ldexp(p2.x, e1 - eb) + __builtin_ldexp(y.b2.x, y.eb - eb),
                                  __builtin_ldexp(p2.y, e1 - eb) + __builtin_ldexp(y.b2.y, y.eb - eb));
        x_norm4(b1, b2, eb);
        double bv = sqrt((x.b1.x * x.b1.x + x.b1.y * x.b1.y) + (x.b2.x * x.b2.x + x.b2.y * x.b2.y));
        double av = bla_abs(x.a1.x, x.a2.x);
        int be = x.eb, ae = x.ea;
        x_norm1(bv, be);
        x_norm1(av, ae);
        const double pv = bv * dcv;
        const int pe = be + dce;
        const int et = y.re > pe ? y.re : pe;
        const double t = (__builtin_ldexp(y.rv, y.re - et) - __builtin_ldexp(pv, pe - et)) / av;
        double rv = (t > 0.0 && __builtin_isfinite(t)) ? t : 0.0;    /* NaN: 0 */
        int re = et - ae;
        x_norm1(rv, re);
        if (!x_less(rv, re, x.rv, x.re)) { rv = x.rv; re = x.re; }
        const int la = ea < 0 ? -ea : ea, lb = eb < 0 ? -eb : eb;
        if (la > kXBlaExpLim || lb > kXBlaExpLim) {
            rv = 0.0; re = kXZero;
            a1 = make_double2(0.0, 0.0); a2 = a1; ea = kXZero;
            b1 = a1; b2 = a1; eb = kXZero;
        }
        const uint32_t e = off + j;
        XRad out;
        out.v = (float)x_trunc24(rv); out.e = re;
        r[e] = out;
        ab[4 * e] = a1;
        ab[4 * e + 1] = a2;
        ab[4 * e + 2] = b1;
        ab[4 * e + 3] = b2;
        abe[e] = make_int2(ea, eb);
    }
}

/* deep_orbit_ship_x with BLA: deep_orbit_x_bla's loop -- u for the loop index, its probe on the 8-byte radius with the
 * pre-filter dz.e + 51 < E (no level's r exceeds the single step's 2^-53 |Z_m|: the fold caps only lower it), its reload of
 * Z_m, Z_{m+1} in the mode a step leaves the lane in -- around the ship's steps: the BLA step is the real 2x2 map in extended
 * arithmetic, its nine loads inside the taken branch; the single steps are deep_orbit_ship_x's, operation for operation. */
__device__ __forceinline__ void deep_orbit_ship_x_bla(const DeepXArgs& AA, const ShipXBlaTable& T, const double cx,
                                                      const double cy, const int ec, bool live, int& esc, double& er2,
                                                      uint32_t& nsingle, uint32_t& nbla)
{
    const DeepArgs& A = AA.d;
    const double2* __restrict__ orbit = A.orbit;
    const double2* __restrict__ mant = AA.mant;
    const int32_t* __restrict__ exp2 = AA.exp2;
    const XRad* __restrict__ tr = T.r;
    const int N = A.n_ref, max_iter = A.max_iter, K = T.levels;
    const uint32_t n1 = (uint32_t)(N - 1);
    const double B2 = A.B2;
    const double cpx = (cx != 0.0 && __builtin_amdgcn_frexp_exp(cx) + ec > -1022) ? __builtin_ldexp(cx, ec) : 0.0;
    const double cpy = (cy != 0.0 && __builtin_amdgcn_frexp_exp(cy) + ec > -1022) ? __builtin_ldexp(cy, ec) : 0.0;
    double dzx = 0.0, dzy = 0.0;                                 /* plain: dz; extended: its mantissas */
    int ed = kXZero;
    bool ext = true;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m, in the lane's mode */
    int eZ = kXZero;
    const double2 z1 = mant[1];
    const int e1 = exp2[1];
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    int eZn = e1;
    int m = 0, u = 0;
    esc = max_iter;
    er2 = 0.0;
    nsingle = 0u; nbla = 0u;
    for (;;) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const int mn = m + 2 <= N ? m + 2 : N;                   /* Z_{m+2}, for the single step after this one */
        int k = 0;
        uint32_t e = 0u;
        double qx = dzx, qy = dzy;                               /* dz, extended and normalised */
        int qe = ed;
        if (m >= 1) {
            if (!ext) { qe = 0; x_norm(qx, qy, qe); }
            const int eZm = (ext ? eZ : 0) + __builtin_amdgcn_frexp_exp(fmax(fabs(Zx), fabs(Zy)));
            if (qe + 51 < eZm) {
                const double dz2 = qx * qx + qy * qy;
                const uint32_t mm = (uint32_t)(m - 1);
                int kk = mm ? __builtin_ctz(mm) : K;
                kk = kk < K ? kk : K;
                const int kn = 31 - __builtin_clz((uint32_t)(N - m));
                const int ki = 31 - __builtin_clz((uint32_t)(max_iter - u));
                kk = kk < kn ? kk : kn;
                kk = kk < ki ? kk : ki;
                for (; kk >= 1; --kk) {
                    const uint32_t ek = bla_offset(n1, kk) + (mm >> kk);
                    const XRad r = tr[ek];
                    const double rv = (double)r.v;
                    if (dz2 < __builtin_ldexp(rv * rv, 2 * (r.e - qe))) { k = kk; e = ek; break; }
                }
            }
        }
        double ax, ay;                                           /* the next dz */
        int ea = 0;
        bool reb;
        if (k > 0 || ext) {
            double nx, ny, Wx, Wy;                               /* n and Z at the new m */
            int en, eW, eZnn = 0;
            double2 Znn = make_double2(0.0, 0.0);
            if (k > 0) {
                const double2 a1 = T.ab[4 * e], a2 = T.ab[4 * e + 1], b1 = T.ab[4 * e + 2], b2 = T.ab[4 * e + 3];
                const int2 ee = T.abe[e];
                const double px = a1.x * qx + a1.y * qy, py = a2.x * qx + a2.y * qy;
                const double sx = b1.x * cx + b1.y * cy, sy = b2.x * cx + b2.y * cy;
                const int ep = ee.x + qe, es = ee.y + ec;
                en = ep > es ? ep : es;
                nx = __builtin_ldexp(px, ep - en) + __builtin_ldexp(sx, es - en);
                ny = __builtin_ldexp(py, ep - en) + __builtin_ldexp(sy, es - en);
                m += 1 << k;
                u += 1 << k;
                ++nbla;
                const double2 Wm = mant[m];
                Wx = Wm.x; Wy = Wm.y; eW = exp2[m];
            } else {
                Znn = mant[mn];
                eZnn = exp2[mn];
                const double fx = ship_fold_x(Zx, eZ - ed, dzx), fy = ship_fold_x(Zy, eZ - ed, dzy);
                const int et = eZ + 1 > ed ? eZ + 1 : ed;
                const double tx = __builtin_ldexp(fabs(Zx), eZ + 1 - et) + __builtin_ldexp(fx, ed - et);
                const double ty = __builtin_ldexp(fabs(Zy), eZ + 1 - et) + __builtin_ldexp(fy, ed - et);
                const double px = tx * fx - ty * fy;
                const double py = tx * fy + ty * fx;
                const int ep = et + ed;
                en = ep > ec ? ep : ec;
                nx = __builtin_ldexp(px, ep - en) + __builtin_ldexp(cx, ec - en);
                ny = __builtin_ldexp(py, ep - en) + __builtin_ldexp(cy, ec - en);
                ++m;
                ++u;
                ++nsingle;
                Wx = Znx; Wy = Zny; eW = eZn;
            }
            const int ez = eW > en ? eW : en;
            const double zx = __builtin_ldexp(Wx, eW - ez) + __builtin_ldexp(nx, en - ez);
            const double zy = __builtin_ldexp(Wy, eW - ez) + __builtin_ldexp(ny, en - ez);
            const double r2 = zx * zx + zy * zy;
            const double r2d = __builtin_ldexp(r2, 2 * ez);
            if (r2d > B2) {
                esc = u - 1; er2 = r2d; live = false;             /* the last update the step covered */
                continue;
            }
            reb = r2 < __builtin_ldexp(nx * nx + ny * ny, 2 * (en - ez)) || m == N;
            ax = reb ? zx : nx; ay = reb ? zy : ny; ea = reb ? ez : en;
            x_norm(ax, ay, ea);
            if (reb) m = 0;
            if (ea <= kXThr) {                                    /* extended from here */
                dzx = ax; dzy = ay; ed = ea;
                ext = true;
                if (reb) {
                    Zx = 0.0; Zy = 0.0; eZ = kXZero; Znx = z1.x; Zny = z1.y; eZn = e1;
                } else if (k == 0) {
                    Zx = Znx; Zy = Zny; eZ = eZn; Znx = Znn.x; Zny = Znn.y; eZn = eZnn;
                } else {                                          /* m < N here */
                    const double2 b = mant[m + 1];
                    Zx = Wx; Zy = Wy; eZ = eW; Znx = b.x; Zny = b.y; eZn = exp2[m + 1];
                }
            } else {                                              /* plain from here (m < N) */
                const double2 a = orbit[m], b = orbit[m + 1];
                dzx = __builtin_ldexp(ax, ea); dzy = __builtin_ldexp(ay, ea);
                ext = false;
                Zx = a.x; Zy = a.y; Znx = b.x; Zny = b.y;
            }
        } else {
            const double2 Znn = orbit[mn];
            const double X2 = Zx + Zx, Y2 = Zy + Zy;
            const double fx = ship_fold(Zx, X2, dzx), fy = ship_fold(Zy, Y2, dzy);
            const double tx = fabs(X2) + fx, ty = fabs(Y2) + fy;     /* |X| + |X| = |X + X| */
            const double nx = (tx * fx - ty * fy) + cpx;
            const double ny = (tx * fy + ty * fx) + cpy;
            ++m;
            ++u;
            ++nsingle;
            const double zx = Znx + nx, zy = Zny + ny;
            const double r2 = zx * zx + zy * zy;
            if (r2 > B2) {
                esc = u - 1; er2 = r2; live = false;
                continue;
            }
            reb = r2 < nx * nx + ny * ny || m == N;
            ax = reb ? zx : nx; ay = reb ? zy : ny;
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
                x_norm(ax, ay, ea);
                dzx = ax; dzy = ay; ed = ea;
                ext = true;
                Zx = a.x; Zy = a.y; eZ = exp2[m]; Znx = b.x; Zny = b.y; eZn = exp2[m + 1];
            }
        }
        if (u >= max_iter) live = false;                          /* esc stays max_iter */
    }
}

__device__ __forceinline__ const DeepArgs& deep_args(const DeepArgs& A) { return A; }
__device__ __forceinline__ const DeepArgs& deep_args(const DeepXArgs& A) { return A.d; }
__device__ __forceinline__ const DeepArgs& deep_args(const DeepBlaArgs& A) { return A.d; }
__device__ __forceinline__ const DeepArgs& deep_args(const DeepXBlaArgs& A) { return A.x.d; }
__device__ __forceinline__ const DeepArgs& deep_args(const DeepShipArgs& A) { return A.d; }
__device__ __forceinline__ const DeepArgs& deep_args(const DeepShipBlaArgs& A) { return A.s.d; }
__device__ __forceinline__ const DeepArgs& deep_args(const DeepShipXArgs& A) { return A.x.d; }
__device__ __forceinline__ const DeepArgs& deep_args(const DeepShipXBlaArgs& A) { return A.s.x.d; }
__device__ __forceinline__ const DeepXArgs& deepx_args(const DeepXArgs& A) { return A; }
__device__ __forceinline__ const DeepXArgs& deepx_args(const DeepXBlaArgs& A) { return A.x; }
__device__ __forceinline__ const DeepXArgs& deepx_args(const DeepShipXArgs& A) { return A.x; }
__device__ __forceinline__ const DeepXArgs& deepx_args(const DeepShipXBlaArgs& A) { return A.s.x; }
__device__ __forceinline__ double ship_log_bailout(const DeepShipArgs& A) { return A.log_bailout; }
__device__ __forceinline__ double ship_log_bailout(const DeepShipBlaArgs& A) { return A.s.log_bailout; }
__device__ __forceinline__ double ship_log_bailout(const DeepShipXArgs& A) { return A.log_bailout; }
__device__ __forceinline__ double ship_log_bailout(const DeepShipXBlaArgs& A) { return A.s.log_bailout; }

/* deep_kernel<DeepArgs>: the plain step; deep_kernel<DeepBlaArgs>: with BLA (deep_orbit_bla, the step counts);
 * deep_kernel<DeepXArgs>: extended-exponent deltas (deep_orbit_x); deep_kernel<DeepXBlaArgs>: those with BLA
 * (deep_orbit_x_bla, the step counts); deep_kernel<DeepShipArgs>: the Burning Ship (deep_orbit_ship, its viewport map and
 * colour stage); deep_kernel<DeepShipBlaArgs>: the ship with BLA (deep_orbit_ship_bla, the step counts);
 * deep_kernel<DeepShipXArgs>: the ship with extended-exponent deltas (deep_orbit_ship_x, the ship's map and colour stage);
 * deep_kernel<DeepShipXBlaArgs>: those with BLA (deep_orbit_ship_x_bla, the step counts) */
template <class ARGS>
__global__ void __launch_bounds__(kBlockThreads)
deep_kernel(const ARGS AA)
{
    constexpr bool XBLA = std::is_same<ARGS, DeepXBlaArgs>::value;
    constexpr bool SHIPBLA = std::is_same<ARGS, DeepShipBlaArgs>::value;
    constexpr bool SHIPXBLA = std::is_same<ARGS, DeepShipXBlaArgs>::value;
    constexpr bool BLA = std::is_same<ARGS, DeepBlaArgs>::value || XBLA || SHIPBLA || SHIPXBLA;
    constexpr bool X = std::is_same<ARGS, DeepXArgs>::value || XBLA;
    constexpr bool SHIPX = std::is_same<ARGS, DeepShipXArgs>::value || SHIPXBLA;
    constexpr bool SHIP = std::is_same<ARGS, DeepShipArgs>::value || SHIPBLA || SHIPX;
    constexpr int FRACTAL = SHIP ? 2 : 0;                         /* the colour stage: shade() / colour_of() */
    const DeepArgs& A = deep_args(AA);
    __shared__ LdsBlock S;
    __shared__ double2 log2_lds[kLog2Entries];
    if (threadIdx.x == 0) S.pal = A.pal;
    if constexpr (SHIP) {
        if (threadIdx.x == 0) S.log_bailout = ship_log_bailout(AA);
    }
    reinterpret_cast<double*>(log2_lds)[threadIdx.x] = reinterpret_cast<const double*>(A.log2_tab)[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {                                       /* the colour of interior samples, once per workgroup */
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        colour_of<double, FRACTAL>(A, S, (double)A.max_iter, true, rgb);
        S.interior_rgb[0] = rgb[0]; S.interior_rgb[1] = rgb[1]; S.interior_rgb[2] = rgb[2];
    }
    __syncthreads();
    const LogTab<double> lg{log2_lds};

    const uint32_t lane = threadIdx.x & (kWave - 1);
    const int W = A.g.W, H = A.g.H;
    const int aa = A.aa > 1 ? A.aa : 1;
    const double resx = (double)W, resy = (double)H, zoom = A.zoom;
    const double2 z1 = A.orbit[1];
    const bool want_rgb = A.rgba != nullptr;
    const bool want_nu = want_rgb || A.nu != nullptr;

    unsigned long long n_plain = 0ull, n_bla = 0ull, n_upd = 0ull;   /* BLA: this lane's steps and updates */
    walk_subtiles<3, true>(A.q, A.g, lane, [&](const int px, const int py, const int lrow, const bool inside) {
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
            if constexpr (SHIP) {                                 /* the map of tile_kernel's Burning Ship path, less the centre */
                const int ux = s / aa, uy = s - ux * aa;          /* burning_ship.comp:337-344: sx outer */
                double uvx = (double)px / resx, uvy = (double)py / resy;
                if (aa > 1) {
                    const double pixel_size = 1.0 / resx;
                    const double sample_offset = pixel_size / (double)aa;
                    const double centre = sample_offset * (double)(aa - 1) * 0.5;
                    uvx = uvx + ((double)ux * sample_offset - centre) / resx;
                    uvy = uvy + ((double)uy * sample_offset - centre) / resy;
                }
                double zs = zoom;                                 /* extended: the zoom's mantissa, its exponent goes to dc.e */
                if constexpr (SHIPX) zs = deepx_args(AA).zm;
                const double sdx = (uvx - 0.5) * zs * (resx / resy);
                const double sdy = (uvy - 0.5) * zs;
                if constexpr (SHIPX) {
                    double cx = inside ? sdx : 0.0, cy = inside ? sdy : 0.0;
                    int ec = deepx_args(AA).ze;
                    x_norm(cx, cy, ec);
                    if constexpr (SHIPXBLA) {
                        uint32_t np, nb;
                        deep_orbit_ship_x_bla(deepx_args(AA), AA.t, cx, cy, ec, inside, esc, r2, np, nb);
                        if (inside) {
                            n_plain += np; n_bla += nb;
                            n_upd += (unsigned long long)(esc < A.max_iter ? esc + 1 : A.max_iter);
                        }
                    } else {
                        deep_orbit_ship_x(deepx_args(AA), cx, cy, ec, inside, esc, r2);
                    }
                } else if constexpr (SHIPBLA) {
                    uint32_t np, nb;
                    deep_orbit_ship_bla(A, AA.t, inside ? sdx : 0.0, inside ? sdy : 0.0, z1, inside, esc, r2, np, nb);
                    if (inside) {
                        n_plain += np; n_bla += nb;
                        n_upd += (unsigned long long)(esc < A.max_iter ? esc + 1 : A.max_iter);
                    }
                } else {
                    deep_orbit_ship(A, inside ? sdx : 0.0, inside ? sdy : 0.0, z1, inside, esc, r2);
                }
            } else if constexpr (X) {
                const DeepXArgs& XA = deepx_args(AA);
                double cx = ((pxs - 0.5 * resx) / resy) * XA.zm, cy = ((pys - 0.5 * resy) / resy) * XA.zm;
                int ec = XA.ze;
                if (!inside) { cx = 0.0; cy = 0.0; }
                x_norm(cx, cy, ec);
                if constexpr (XBLA) {
                    uint32_t np, nb;
                    deep_orbit_x_bla(XA, AA.t, cx, cy, ec, inside, esc, r2, np, nb);
                    if (inside) {
                        n_plain += np; n_bla += nb;
                        n_upd += (unsigned long long)(esc < A.max_iter ? esc + 1 : A.max_iter);
                    }
                } else {
                    deep_orbit_x(XA, cx, cy, ec, inside, esc, r2);
                }
            } else if constexpr (BLA) {
                uint32_t np, nb;
                deep_orbit_bla(A, AA.t, inside ? dcx : 0.0, inside ? dcy : 0.0, z1, inside, esc, r2, np, nb);
                if (inside) {
                    n_plain += np; n_bla += nb;
                    n_upd += (unsigned long long)(esc < A.max_iter ? esc + 1 : A.max_iter);
                }
            } else {
                deep_orbit(A, inside ? dcx : 0.0, inside ? dcy : 0.0, z1, inside, esc, r2);
            }
            double nu;
            float rgb[3];
            shade<double, FRACTAL>(A, S, lg, esc, r2, want_nu, want_rgb, nu, rgb);
            if (s == 0) { nu0 = nu; it0 = esc; }
            acc[0] += rgb[0]; acc[1] += rgb[1]; acc[2] += rgb[2];
        }
        if (aa > 1) {
            const float n = (float)(aa * aa);
            acc[0] /= n; acc[1] /= n; acc[2] /= n;
        }
        if (want_rgb && (A.flags & FR_FLAG_POST_CHAIN)) post_chain(acc, A.brightness, A.saturation, A.contrast, SHIP);
        if (!inside) return;
        const size_t o = plane_index(A.g, px, py, lrow);
        if (A.rgba) A.rgba[o] = make_float4(acc[0], acc[1], acc[2], 1.0f);
        if (A.nu) A.nu[o] = nu0;
        if (A.iter) A.iter[o] = it0;
    });
    if constexpr (BLA) {                                          /* updates skipped = updates - plain steps */
        unsigned long long v[3] = {n_plain, n_bla, n_upd - n_plain};
        for (int c = 0; c < 3; ++c) {
            for (int o = kWave / 2; o > 0; o >>= 1) v[c] += __shfl_xor(v[c], o, kWave);
            if (lane == 0) atomicAdd(AA.t.steps + c, v[c]);
        }
    }
}

}  // namespace fr
