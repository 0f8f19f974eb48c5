/*
 * fr_deep.hip.h -- views deeper than double precision on gfx950: perturbation around one reference orbit with rebasing, for
 * the Mandelbrot set (fr_render_deep, fr_render_deepx), the Burning Ship (fr_render_deep_ship, fr_render_deepx_ship) and, around
 * two orbits, Julia sets (fr_render_deep_julia, fr_render_deepx_julia).
 *
 * The reference orbit Z_0 .. Z_N (fr_deep.c: fixed point on the host, stored as doubles) sits in HBM; every sample
 * iterates its delta dz = z - Z_m from it, dc being its offset from the centre.  The Mandelbrot step:
 *   t = (Z_m + Z_m) + dz;  dz' = (t.x dz.x - t.y dz.y, t.x dz.y + t.y dz.x) + dc;  m += 1;  z = Z_m + dz';  r2 = |z|^2
 *   r2 > B2: escaped at this loop index;  r2 < |dz'|^2 or m == N: rebase, dz = z, m = 0;  else dz = dz'
 * one rounding per operation as written (the file is built with -ffp-contract=off).  The rebase restarts the sample on the
 * orbit's start whenever its delta has outgrown the orbit (|z| < |dz|) or the orbit ends, so one reference serves every
 * sample and no glitch can form.
 *
 * The shape of the file:
 *   - two formula policies, MandelFormula and ShipFormula, hold everything that differs between the two recurrences and
 *     nothing else: the linear part of the plain step (t, f) and of the extended step (U, f), the BLA step in fp64 and in
 *     extended arithmetic with the loads of its own entry, the viewport map of a sample, the colour stage's index, and for
 *     the table build the single step, the merge products, the two norms and the load and store of an entry.  The ship's
 *     step is the Mandelbrot step on U = (|Z_m.x|, |Z_m.y|) and f = (fold(Z_m.x, dz.x), fold(Z_m.y, dz.y)), the fold a pair
 *     of compares and selects; its BLA step is a real 2x2 map where Mandelbrot's is a complex product.
 *   - a third policy, JuliaFormula: Mandelbrot's linear part, the ship's viewport map, no dc term (the sample's offset is its
 *     first delta) and kTwoOrbits -- a lane starts on the orbit P of the view's centre, stored behind the critical orbit Q in
 *     the same buffers, and its first rebase moves it onto Q (Q_0 = 0 keeps the rebase exact) for good.  A lane carries its
 *     orbit's base and N; the extended loops flush a delta whose exponent runs below -2^27 to zero.  Its BLA is Mandelbrot's
 *     with kHasB = false: no dc, so an entry is (r, A) and a step one complex product; there is one table per orbit, Q's
 *     first in the same buffers, and a BLA lane also carries its table's entry base, n1 and K.
 *   - four per-sample loops, each templated on the formula: deep_orbit (fp64 deltas), deep_orbit_bla (those with BLA),
 *     deep_orbit_x (extended-exponent deltas, fr_render_deepx*), deep_orbit_x_bla (those with BLA).  The BLA loops count the
 *     updates u a sample has covered, the others the loop index.  In all of them dz, dc, m and the count stay in registers;
 *     Z_m and Z_{m+1} are in registers too and Z_{m+2} is loaded one step ahead; Z_1 is loaded once, so a rebase
 *     (Z_m = Z_0 = 0, Z_{m+1} = Z_1) waits for no load.  While no lane of a wave has rebased, all 64 lanes read the same
 *     orbit point; after that they gather from different m.
 *   - extended-exponent deltas (the arithmetic is in the header): a lane is in one of two modes.  Plain: the fp64 step on
 *     the plain doubles of the orbit.  Extended (max(|dz.x|, |dz.y|) < 2^-400): dz is two double mantissas and one int32
 *     exponent, the orbit points come from the mantissa and exponent arrays, alignment is v_ldexp_f64, and the one
 *     normalisation per step takes its exponent with v_frexp_exp_i32_f64 off max(|x|, |y|); the mode test is an integer
 *     compare.  A lane that changes mode reloads Z_m and Z_{m+1} from the new mode's arrays.  The ship's extended step
 *     takes the fold in the delta's frame (ship_fold_x).
 *   - two level probes, bla_probe on the fp64 table and bla_probe_x on the extended one, each used by its BLA loop for both
 *     formulas: top down from bla_top_level, the first level whose radius admits |dz|, behind a pre-filter that lets a lane
 *     which cannot pass gather nothing.  A probe gathers 8 bytes; the chosen level's (A, B) are loaded inside the
 *     taken-step branch only.
 *   - two table builds, bla_level (fp64) and bla_level_x (extended), one launch per level: entry j of level k merges entries
 *     2j and 2j + 1 of level k - 1, level 0 being the single steps, computed from the orbit and never stored.  The six
 *     __global__ level kernels are these two with a formula (Julia's: one orbit and its part of the buffers per launch).  The table stores, level after level (level k from entry
 *     offset bla_offset(N - 1, k)), the radius r of every entry in an array of its own -- a double, or an XRad -- and
 *     (A, B) as F::kAbPerEntry double2 per entry (2: complex A, B; 4: the rows of the ship's real matrices; 1: Julia's A), the
 *     extended tables with their two exponents in an int2 (Julia: A's in an int32).
 *   - deep_kernel<ARGS>, ARGS = DeepBlock<F, X, DE, BLA>: one argument-block template over the four switches -- DeepArgs and
 *     the parts they turn on -- and one kernel for its twenty instantiations, which reads the switches from the block.  A
 *     persistent grid of the resident set pulls runs of 8x8 sub-tiles from the sharded WaveQueue with unlimited stealing (deep
 *     views have very uneven iteration counts); one lane per sample, the aa x aa samples of a pixel one after the other in the
 *     lane; dc through the formula's viewport map, one dispatch on (X, DE, BLA) to the loop, then the colour stage of the
 *     formula's fp64 path: shade() and post_chain() of fr_kernels.hip.h on (i, r2).
 *   - the distance estimate (fr_render_deep_de): a compile-time option DE of deep_orbit and deep_orbit_bla carries
 *     D = dz/dc * s, s = zoom / H one pixel spacing, next to the delta -- D' = 2 z D + s in a plain step, D' = A D + B s in a
 *     BLA step, nothing in a rebase -- and feeds nothing back: (i, r2) and the step counts are those of the loops without it.
 *     Four live VGPRs and, per plain update, 11 fp64 operations.  The kernel turns (r2, D) of an escaped sample into
 *     |z| log|z| / |D| and, on request, the debug shader's distance shading.
 *   - the same below 1e-290 (fr_render_deepx_de): the option DE of deep_orbit_x and deep_orbit_x_bla, with D an extended
 *     complex number (XDeriv: two mantissas, one int32 exponent) whatever mode the lane's delta is in, normalised after every
 *     update; s = (sm, es) stays in SGPRs.  Five live VGPRs.
 *   - the distance estimate of Julia views (fr_render_deep_julia_de, fr_render_deepx_julia_de): the option DE for a formula
 *     without a dc term (kHasB == false).  D = dz_n/dz_0 * s starts at s, not at 0; an update is one complex product,
 *     D' = 2 z D or D' = A D, and nothing is added (the overloads of deep_step_d, deep_step_xd, deep_step_pd and deepx_d_set
 *     without s); the extended D is flushed to the zero below 2^-2^27 as the delta is.  Four and five live VGPRs.
 *   - the distance estimate of ship views (fr_render_deep_ship_de, fr_render_deepx_ship_de): the option DE for a formula with
 *     kRealJacobian.  The ship's map is not conformal, so the derivative is a real 2x2 matrix J = dz/dc * s (Jac; XJac: four
 *     mantissas, one int32 exponent, norm4 after every update): J' = L J + s I in a single step, L the derivative of
 *     (|x| + i |y|)^2 at the sample's point (ship_lj), J' = A J + B s in a BLA step, nothing in a rebase.  An escaping lane keeps
 *     z in its dz registers, and the kernel turns (J, z) into the gradient of |z|, g = J^T z / |z|, which deep_de_of takes as D.
 *     Eight and nine live VGPRs.  The four kernels are instantiations of deep_ship_de_kernel, a __global__ template of their
 *     own around the same body.
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

/* The fp64 BLA table of a cached orbit (FR_FLAG_DEEP_BLA, FR_FLAG_DEEP_SHIP_BLA) */
struct BlaTable {
    const double* r;                     /* r of every entry, level 1 first */
    const double2* ab;                   /* (A, B) of every entry: ab[n e .. n e + n - 1], n = F::kAbPerEntry */
    int32_t levels;                      /* K = floor(log2(N - 1)), 0 = no table */
    unsigned long long* steps;           /* plain steps, BLA steps, updates skipped: one atomic add each per wave */
};

/* The radius of an extended table's entry: the top 24 bits of its mantissa as a float and its int32 exponent -- the 8 bytes
 * a probe gathers */
struct XRad {
    float v;                             /* mantissa in [0.5, 1), 0 for r = 0 */
    int32_t e;                           /* FR_DEEPX_ZERO_EXP for r = 0 */
};

/* The extended BLA table of a cached extended orbit (FR_FLAG_DEEPX_BLA, FR_FLAG_DEEPX_SHIP_BLA): BlaTable with normalised
 * mantissas in ab and the exponents apart */
struct BlaXTable {
    const XRad* r;                       /* r of every entry, level 1 first */
    const double2* ab;                   /* mantissas of (A, B), laid out as BlaTable::ab */
    const int2* abe;                     /* (A.e, B.e) */
    int32_t levels;                      /* K = floor(log2(N - 1)), 0 = no table */
    unsigned long long* steps;           /* single steps, BLA steps, updates skipped: one atomic add each per wave */
};

/* A Julia view's second orbit: orbit / n_ref (and mant, exp2) are Q, the critical orbit a rebase lands on, so
 * z1 = Q_1; P, the orbit of the centre every sample starts on, sits p_off points behind Q in the same buffers */
struct JuliaStart {
    int32_t p_off;
    int32_t n_p;                         /* N_P >= 1 */
};

/* A Julia view's tables (FR_FLAG_DEEP_JULIA_BLA, FR_FLAG_DEEPX_JULIA_BLA): q is the table of Q = orbit; P's entries start
 * base_p entries behind Q's in the same arrays */
template <class TAB>
struct JuliaTab {
    TAB q;
    int32_t levels_p;                    /* K of P's table, 0 = none */
    uint32_t base_p;                     /* the entries of Q's table */
};

/* ---- the argument blocks -----------------------------------------------------------------------------------------------
 * DeepBlock<F, X, DE, BLA> is the argument block of deep_kernel for the formula policy F (below), extended-exponent deltas X,
 * the distance estimate DE and a BLA table: DeepArgs, then the parts its switches turn on, in this order.  A part that is off
 * is an empty base and takes no room. */
struct MandelFormula;
struct ShipFormula;
struct JuliaFormula;
template <int> struct NoPart {};

/* X: the orbit's extended storage; DeepArgs::orbit holds the plain doubles P_n and DeepArgs::zoom is not read */
struct DeepXOrbit {
    const double2* mant;                 /* (mx, my) of Z_0 .. Z_N */
    const int32_t* exp2;                 /* e of Z_0 .. Z_N */
    double zm;                           /* zoom = zm 2^ze */
    int32_t ze;
};

/* what the formula adds: nothing for Mandelbrot */
template <class F> struct DeepFormulaPart {};
template <> struct DeepFormulaPart<ShipFormula> {
    double log_bailout;                  /* log(bailout), for shade<double, 2> at bailout <= 1 (LaunchArgs::log_bailout) */
};
template <> struct DeepFormulaPart<JuliaFormula> {
    double log_bailout;
    JuliaStart j;
};

/* DE: the scaled derivative D = dz/dc * s (Julia: dz_n/dz_0 * s) carried next to the delta, s = zoom / H of the whole frame, one
 * pixel spacing: a double, or with X an extended real s = sm 2^es, sm in [0.5, 1), as D is an extended complex number there */
struct DeepSpacing { double s; };
struct DeepXSpacing { double sm; int32_t es; };
template <bool X>
struct DeepDePart : std::conditional_t<X, DeepXSpacing, DeepSpacing> {
    double* de;                          /* distance estimate of sample (0,0), in pixel spacings */
    double* deriv;                       /* (D.x, D.y) of sample (0,0) at its escaping update: two doubles per pixel, a caller's
                                          * plane with no more than a double's alignment; the ship: (J11, J12, J21, J22), four */
    int32_t shade;                       /* 1: the debug shader's distance shading on every escaped sub-sample */
    float edge_px;                       /* ... its smoothstep's upper edge, in pixel spacings */
};

template <class F, bool X, bool DE, bool BLA = false>
struct DeepBlock : DeepArgs, std::conditional_t<X, DeepXOrbit, NoPart<0>>, DeepFormulaPart<F>,
                   std::conditional_t<DE, DeepDePart<X>, NoPart<1>> {
    using Formula = F;
    static constexpr bool kX = X, kDe = DE, kBla = false;
};

/* BLA: the block without it, then the table of its storage -- the two tables of a formula with two orbits */
template <class F, bool X, bool DE>
struct DeepBlock<F, X, DE, true> : DeepBlock<F, X, DE> {
    static constexpr bool kBla = true;
    using Table = std::conditional_t<X, BlaXTable, BlaTable>;
    std::conditional_t<F::kTwoOrbits, JuliaTab<Table>, Table> t;
};

/* a block's table: Q's where there are two */
template <class B>
__host__ __device__ __forceinline__ auto& bla_table(B& b)
{
    if constexpr (B::Formula::kTwoOrbits) return b.t.q;
    else return b.t;
}

constexpr int kXZero = FR_DEEPX_ZERO_EXP;
constexpr int kXThr = -400;              /* extended while the normalised dz.e <= kXThr */
constexpr int kXBlaExpLim = 1 << 27;     /* an entry whose A.e or B.e leaves [-2^27, 2^27] is void */
constexpr int kXFlushExp = -(1 << 27);   /* Julia: a normalised dz, or D, with e below this becomes the zero (the header's FLUSH) */

/* ---- extended reals ----------------------------------------------------------------------------------------------------
 * norm(x, y, e) of the header */
__device__ __forceinline__ void x_norm(double& x, double& y, int& e)
{
    const double mx = fmax(fabs(x), fabs(y));
    const int k = __builtin_amdgcn_frexp_exp(mx);
    x = __builtin_ldexp(x, -k);
    y = __builtin_ldexp(y, -k);
    e = mx == 0.0 ? kXZero : e + k;
}

/* an extended real normalised: v into [0.5, 1), zero gets FR_DEEPX_ZERO_EXP */
__device__ __forceinline__ void x_norm1(double& v, int& e)
{
    const int k = __builtin_amdgcn_frexp_exp(v);
    e = v == 0.0 ? kXZero : e + k;
    v = __builtin_ldexp(v, -k);
}

/* norm4 of the header: a matrix's four mantissas normalised on the largest of them */
__device__ __forceinline__ void x_norm4(double2& r1, double2& r2, int& e)
{
    const double mx = fmax(fmax(fabs(r1.x), fabs(r1.y)), fmax(fabs(r2.x), fabs(r2.y)));
    const int k = __builtin_amdgcn_frexp_exp(mx);
    r1.x = __builtin_ldexp(r1.x, -k); r1.y = __builtin_ldexp(r1.y, -k);
    r2.x = __builtin_ldexp(r2.x, -k); r2.y = __builtin_ldexp(r2.y, -k);
    e = mx == 0.0 ? kXZero : e + k;
}

/* (v, e) < (w, f) on normalised extended reals; the zero's exponent FR_DEEPX_ZERO_EXP is below every other */
__device__ __forceinline__ bool x_less(const double v, const int e, const double w, const int f)
{
    return e < f || (e == f && v < w);
}

/* the top 24 bits of a mantissa in [0.5, 1) (toward zero): exactly a float */
__device__ __forceinline__ double x_trunc24(const double v)
{
    return __longlong_as_double(__double_as_longlong(v) & ~((1ll << 29) - 1));
}

/* a component of the normalised dc = (cx, cy, ec) as the plain mode's double: below 2^-1022 it is 0 */
__device__ __forceinline__ double x_plain(const double c, const int ec)
{
    return (c != 0.0 && __builtin_amdgcn_frexp_exp(c) + ec > -1022) ? __builtin_ldexp(c, ec) : 0.0;
}

/* |w| as the header writes it: sqrt(w.x*w.x + w.y*w.y).  On gfx950 sqrt(double) is LLVM's expansion of llvm.sqrt.f64:
 * scaling of small arguments, v_rsq_f64, two Newton-Raphson refinements of the root and half-reciprocal root, and a final
 * correction from the fma residual x - s*s -- the correctly rounded OCML sequence (tests/test_deep_bla_gpu.py compares
 * every radius of device-built tables with numpy's bit for bit). */
__device__ __forceinline__ double bla_abs(const double x, const double y) { return sqrt(x * x + y * y); }

/* |X + a| - |X| without the cancelling sum: the signs of X and of w = X + a (exact: an IEEE sum is zero only when it is
 * exactly zero) pick a, -a or +-(2X + a).  X2 = X + X.  Compares and selects, no branch. */
__device__ __forceinline__ double ship_fold(const double X, const double X2, const double a)
{
    const double w = X + a, d = X2 + a;
    const double up = w >= 0.0 ? a : -d;
    const double dn = w > 0.0 ? d : -a;
    return X >= 0.0 ? up : dn;
}

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

/* fr_render_deep_de: D' stays where the step forms it.  Left alone the compiler sinks the whole update behind the trip's
 * escape and rebase branches (nothing in them reads D) and keeps the old dz and Z_m alive, in eight registers of their own, to
 * form it there. */
__device__ __forceinline__ void deep_pin_d(double2& D) { asm volatile("" : "+v"(D.x), "+v"(D.y)); }

/* fr_render_deepx_de: D = dz/dc * s as an extended complex number, normalised after every update in either mode of the lane's
 * delta; the zero has FR_DEEPX_ZERO_EXP */
struct XDeriv {
    double x, y;
    int e;
};

/* D' = norm(p (+) q) of the header: p at ep the step's linear part applied to D, q at eq its dc term applied to s.  Pinned as
 * deep_pin_d pins the fp64 D. */
__device__ __forceinline__ void deepx_d_set(XDeriv& D, const double px, const double py, const int ep, const double qx,
                                            const double qy, const int eq)
{
    const int e = ep > eq ? ep : eq;
    D.x = __builtin_ldexp(px, ep - e) + __builtin_ldexp(qx, eq - e);
    D.y = __builtin_ldexp(py, ep - e) + __builtin_ldexp(qy, eq - e);
    D.e = e;
    x_norm(D.x, D.y, D.e);
    asm volatile("" : "+v"(D.x), "+v"(D.y), "+v"(D.e));
}

/* ... with q = (sm, 0, es), a single step's: nothing is added to the imaginary part */
__device__ __forceinline__ void deepx_d_set(XDeriv& D, const double px, const double py, const int ep, const double sm,
                                            const int es)
{
    const int e = ep > es ? ep : es;
    D.x = __builtin_ldexp(px, ep - e) + __builtin_ldexp(sm, es - e);
    D.y = __builtin_ldexp(py, ep - e);
    D.e = e;
    x_norm(D.x, D.y, D.e);
    asm volatile("" : "+v"(D.x), "+v"(D.y), "+v"(D.e));
}

/* ... without q, a formula without a dc term (Julia): D' = norm(p), then the header's FLUSH of D -- below 2^-2^27 it becomes
 * the zero and stays it (a product with the zero is the zero) */
__device__ __forceinline__ void deepx_d_set(XDeriv& D, const double px, const double py, const int ep)
{
    D.x = px; D.y = py; D.e = ep;
    x_norm(D.x, D.y, D.e);
    if (D.e < kXFlushExp) { D.x = 0.0; D.y = 0.0; D.e = kXZero; }
    asm volatile("" : "+v"(D.x), "+v"(D.y), "+v"(D.e));
}

/* fr_render_deep_ship_de: the ship's map is not conformal, so its derivative is a real 2x2 matrix,
 * J = [[dx/dcx, dx/dcy], [dy/dcx, dy/dcy]] * s, carried by rows; z is the sample's point at its escaping update, which the
 * loops hand back in the escaped lane's dz */
struct Jac {
    double2 r1, r2;                      /* (J11, J12), (J21, J22) */
    double2 z;
};

/* fr_render_deepx_ship_de: J as four mantissas and one shared int32 exponent, normalised with norm4 after every update */
struct XJac {
    double2 r1, r2;
    int e;
    double2 z;                           /* plain doubles: |z| > bailout there */
};

/* deep_pin_d for the four entries of J */
__device__ __forceinline__ void deep_pin_j(double2& r1, double2& r2)
{
    asm volatile("" : "+v"(r1.x), "+v"(r1.y), "+v"(r2.x), "+v"(r2.y));
}

/* J' = norm4(p (+) q) of the header: the rows p1, p2 at ep the step's linear part applied to J, q1, q2 at eq its dc term applied
 * to s */
__device__ __forceinline__ void deepx_j_set(XJac& J, const double2 p1, const double2 p2, const int ep, const double2 q1,
                                            const double2 q2, const int eq)
{
    const int e = ep > eq ? ep : eq;
    J.r1 = make_double2(__builtin_ldexp(p1.x, ep - e) + __builtin_ldexp(q1.x, eq - e),
                        __builtin_ldexp(p1.y, ep - e) + __builtin_ldexp(q1.y, eq - e));
    J.r2 = make_double2(__builtin_ldexp(p2.x, ep - e) + __builtin_ldexp(q2.x, eq - e),
                        __builtin_ldexp(p2.y, ep - e) + __builtin_ldexp(q2.y, eq - e));
    J.e = e;
    x_norm4(J.r1, J.r2, J.e);
    asm volatile("" : "+v"(J.r1.x), "+v"(J.r1.y), "+v"(J.r2.x), "+v"(J.r2.y), "+v"(J.e));
}

/* ... with q = (sm I, es), a single step's: nothing is added off the diagonal */
__device__ __forceinline__ void deepx_j_set(XJac& J, const double2 p1, const double2 p2, const int ep, const double sm,
                                            const int es)
{
    const int e = ep > es ? ep : es;
    const double q = __builtin_ldexp(sm, es - e);
    J.r1 = make_double2(__builtin_ldexp(p1.x, ep - e) + q, __builtin_ldexp(p1.y, ep - e));
    J.r2 = make_double2(__builtin_ldexp(p2.x, ep - e), __builtin_ldexp(p2.y, ep - e) + q);
    J.e = e;
    x_norm4(J.r1, J.r2, J.e);
    asm volatile("" : "+v"(J.r1.x), "+v"(J.r1.y), "+v"(J.r2.x), "+v"(J.r2.y), "+v"(J.e));
}

/* L J of the ship at the point (x, y), doubling apart: L = [[x, -y], [|y| sgn sx, |x| sgn sy]], sgn v = v >= 0 ? 1 : -1; (sx, sy)
 * carries the signs of the point's coordinates ((x, y) itself in fp64) */
__device__ __forceinline__ void ship_lj(const double x, const double y, const double sx, const double sy, const double2 j1,
                                        const double2 j2, double2& p1, double2& p2)
{
    const double l12 = -y;
    const double l21 = sx >= 0.0 ? fabs(y) : -fabs(y), l22 = sy >= 0.0 ? fabs(x) : -fabs(x);
    p1 = make_double2(x * j1.x + l12 * j2.x, x * j1.y + l12 * j2.y);
    p2 = make_double2(l21 * j1.x + l22 * j2.x, l21 * j1.y + l22 * j2.y);
}

/* ---- the formula policies ------------------------------------------------------------------------------------------------
 * What a policy hands to the shared code, all by value (small structs in registers). */
struct StepLin { double tx, ty, fx, fy; };          /* the plain step: dz' = t * f + dc, a complex product */
struct StepLinX { double ux, uy, fx, fy; };         /* the extended step: t = (U, Z_m.e + 1) (+) (f, dz.e), dz' = t * f (+) dc */
struct BlaStepX { double px, py, sx, sy; int ea, eb; };   /* a BLA step's A dz and B dc as mantissas, and (A.e, B.e) */

/* an entry of a table while it is being merged: F::kAbPerEntry / 2 double2 each of A and of B, and r */
template <int ROWS>
struct BlaLin {
    double2 a[ROWS], b[ROWS];
    double r;
};
template <int ROWS>
struct BlaLinX {
    double2 a[ROWS], b[ROWS];
    int ea, eb;
    double rv;
    int re;
};

/* z <- z^2 + c */
struct MandelFormula {
    static constexpr int kFractal = 0;                /* the colour stage: shade() / colour_of() */
    static constexpr bool kLogBailoutLds = false;
    static constexpr bool kTwoOrbits = false;         /* one orbit from 0, a dc term in every step */
    static constexpr bool kHasB = true;
    static constexpr bool kRealJacobian = false;      /* conformal: the derivative is a complex number */
    static constexpr int kAbPerEntry = 2;             /* complex A, B */
    using Lin = BlaLin<1>;
    using LinX = BlaLinX<1>;

    static __device__ __forceinline__ StepLin lin(const double Zx, const double Zy, const double dzx, const double dzy)
    {
        return {(Zx + Zx) + dzx, (Zy + Zy) + dzy, dzx, dzy};
    }
    static __device__ __forceinline__ StepLinX lin_x(const double Zx, const double Zy, const int eZ, const double dzx,
                                                     const double dzy, const int ed)
    {
        return {Zx, Zy, dzx, dzy};
    }
    /* dz' = A dz + B dc, complex products */
    static __device__ __forceinline__ double2 bla(const BlaTable& T, const uint32_t e, const double dzx,
                                                  const double dzy, const double dcx, const double dcy)
    {
        const double2 a = T.ab[2 * e], b = T.ab[2 * e + 1];
        return make_double2((a.x * dzx - a.y * dzy) + (b.x * dcx - b.y * dcy), (a.x * dzy + a.y * dzx) + (b.x * dcy + b.y * dcx));
    }
    /* bla() with the derivative of the map it applies, from the one load of (A, B): D' = A D + B s */
    static __device__ __forceinline__ double2 bla_d(const BlaTable& T, const uint32_t e, const double dzx, const double dzy,
                                                    const double dcx, const double dcy, const double s, double2& D)
    {
        const double2 a = T.ab[2 * e], b = T.ab[2 * e + 1];
        D = make_double2((a.x * D.x - a.y * D.y) + b.x * s, (a.x * D.y + a.y * D.x) + b.y * s);
        deep_pin_d(D);
        return make_double2((a.x * dzx - a.y * dzy) + (b.x * dcx - b.y * dcy), (a.x * dzy + a.y * dzx) + (b.x * dcy + b.y * dcx));
    }
    static __device__ __forceinline__ BlaStepX bla_x(const BlaXTable& T, const uint32_t e, const double qx, const double qy,
                                                     const double cx, const double cy)
    {
        const double2 a = T.ab[2 * e], b = T.ab[2 * e + 1];
        const int2 ee = T.abe[e];
        return {a.x * qx - a.y * qy, a.x * qy + a.y * qx, b.x * cx - b.y * cy, b.x * cy + b.y * cx, ee.x, ee.y};
    }
    /* bla_x() with the derivative of the map it applies, from the one load of the entry:
     * D' = norm((A D, A.e + D.e) (+) (B (sm, 0), B.e + es)) */
    static __device__ __forceinline__ BlaStepX bla_x_d(const BlaXTable& T, const uint32_t e, const double qx, const double qy,
                                                       const double cx, const double cy, const double sm, const int es, XDeriv& D)
    {
        const double2 a = T.ab[2 * e], b = T.ab[2 * e + 1];
        const int2 ee = T.abe[e];
        deepx_d_set(D, a.x * D.x - a.y * D.y, a.x * D.y + a.y * D.x, ee.x + D.e, b.x * sm, b.y * sm, ee.y + es);
        return {a.x * qx - a.y * qy, a.x * qy + a.y * qx, b.x * cx - b.y * cy, b.x * cy + b.y * cx, ee.x, ee.y};
    }
    /* mandelbrot.comp:219-230 (sy outer) and :149-151, less the centre; zs = the zoom or its mantissa */
    static __device__ __forceinline__ double2 dc(const int px, const int py, const int s, const int aa, const double resx,
                                                 const double resy, const double zs)
    {
        const int sy = s / aa, sx = s - sy * aa;
        const double pxs = (double)px + (double)sx / (double)aa;
        const double pys = (double)py + (double)sy / (double)aa;
        return make_double2(((pxs - 0.5 * resx) / resy) * zs, ((pys - 0.5 * resy) / resy) * zs);
    }

    /* the table build.  The single step at Z_m: A = 2 Z_m, B = 1, r = 2^-53 |Z_m| */
    static __device__ __forceinline__ Lin single(const double2 Z)
    {
        Lin s;
        s.a[0] = make_double2(Z.x + Z.x, Z.y + Z.y);
        s.b[0] = make_double2(1.0, 0.0);
        s.r = 0x1p-53 * bla_abs(Z.x, Z.y);
        return s;
    }
    /* A = norm(Z_m.x, Z_m.y, Z_m.e + 1), B = norm(1, 0, 0), r = 2^-53 |Z_m| */
    static __device__ __forceinline__ LinX single_x(const double2 Z, const int eZ)
    {
        LinX s;
        s.a[0] = Z; s.ea = eZ + 1;
        x_norm(s.a[0].x, s.a[0].y, s.ea);
        s.b[0] = make_double2(0.5, 0.0); s.eb = 1;
        double nx = Z.x, ny = Z.y;
        int ne = eZ;
        x_norm(nx, ny, ne);
        s.rv = bla_abs(nx, ny); s.re = ne;
        x_norm1(s.rv, s.re);
        if (s.rv != 0.0) s.re -= 53;
        return s;
    }
    /* A_y A_x and A_y B_x (the caller adds B_y) */
    template <class L>
    static __device__ __forceinline__ void mul_a(const L& y, const L& x, double2* a)
    {
        a[0] = make_double2(y.a[0].x * x.a[0].x - y.a[0].y * x.a[0].y, y.a[0].x * x.a[0].y + y.a[0].y * x.a[0].x);
    }
    template <class L>
    static __device__ __forceinline__ void mul_b(const L& y, const L& x, double2* p)
    {
        p[0] = make_double2(y.a[0].x * x.b[0].x - y.a[0].y * x.b[0].y, y.a[0].x * x.b[0].y + y.a[0].y * x.b[0].x);
    }
    template <class L>
    static __device__ __forceinline__ double norm_a(const L& x) { return bla_abs(x.a[0].x, x.a[0].y); }
    template <class L>
    static __device__ __forceinline__ double norm_b(const L& x) { return bla_abs(x.b[0].x, x.b[0].y); }
    static __device__ __forceinline__ void norm_rows(double2* m, int& e) { x_norm(m[0].x, m[0].y, e); }
};

/* z <- (|x| + i |y|)^2 + c */
struct ShipFormula {
    static constexpr int kFractal = 2;
    static constexpr bool kLogBailoutLds = true;      /* shade<double, 2> at bailout <= 1 */
    static constexpr bool kTwoOrbits = false;
    static constexpr bool kHasB = true;
    static constexpr bool kRealJacobian = true;       /* the derivative is a real 2x2 matrix (Jac, XJac) */
    static constexpr int kAbPerEntry = 4;             /* the rows (a11, a12), (a21, a22), (b11, b12), (b21, b22) */
    using Lin = BlaLin<2>;
    using LinX = BlaLinX<2>;

    static __device__ __forceinline__ StepLin lin(const double Zx, const double Zy, const double dzx, const double dzy)
    {
        const double X2 = Zx + Zx, Y2 = Zy + Zy;
        const double fx = ship_fold(Zx, X2, dzx), fy = ship_fold(Zy, Y2, dzy);
        return {fabs(X2) + fx, fabs(Y2) + fy, fx, fy};       /* |X| + |X| = |X + X| */
    }
    static __device__ __forceinline__ StepLinX lin_x(const double Zx, const double Zy, const int eZ, const double dzx,
                                                     const double dzy, const int ed)
    {
        const double fx = ship_fold_x(Zx, eZ - ed, dzx), fy = ship_fold_x(Zy, eZ - ed, dzy);
        return {fabs(Zx), fabs(Zy), fx, fy};
    }
    /* dz' = A dz + B dc, real 2x2 maps: valid while no fold flips a sign, which the radius guarantees */
    static __device__ __forceinline__ double2 bla(const BlaTable& T, const uint32_t e, const double dzx,
                                                  const double dzy, const double dcx, const double dcy)
    {
        const double2 a1 = T.ab[4 * e], a2 = T.ab[4 * e + 1], b1 = T.ab[4 * e + 2], b2 = T.ab[4 * e + 3];
        return make_double2((a1.x * dzx + a1.y * dzy) + (b1.x * dcx + b1.y * dcy), (a2.x * dzx + a2.y * dzy) + (b2.x * dcx + b2.y * dcy));
    }
    /* bla() with the derivative of the map it applies, from the one load of (A, B): J' = A J + B s, real 2x2 products */
    static __device__ __forceinline__ double2 bla_d(const BlaTable& T, const uint32_t e, const double dzx, const double dzy,
                                                    const double dcx, const double dcy, const double s, Jac& J)
    {
        const double2 a1 = T.ab[4 * e], a2 = T.ab[4 * e + 1], b1 = T.ab[4 * e + 2], b2 = T.ab[4 * e + 3];
        const double2 j1 = J.r1, j2 = J.r2;
        J.r1 = make_double2((a1.x * j1.x + a1.y * j2.x) + b1.x * s, (a1.x * j1.y + a1.y * j2.y) + b1.y * s);
        J.r2 = make_double2((a2.x * j1.x + a2.y * j2.x) + b2.x * s, (a2.x * j1.y + a2.y * j2.y) + b2.y * s);
        deep_pin_j(J.r1, J.r2);
        return make_double2((a1.x * dzx + a1.y * dzy) + (b1.x * dcx + b1.y * dcy), (a2.x * dzx + a2.y * dzy) + (b2.x * dcx + b2.y * dcy));
    }
    static __device__ __forceinline__ BlaStepX bla_x(const BlaXTable& T, const uint32_t e, const double qx, const double qy,
                                                     const double cx, const double cy)
    {
        const double2 a1 = T.ab[4 * e], a2 = T.ab[4 * e + 1], b1 = T.ab[4 * e + 2], b2 = T.ab[4 * e + 3];
        const int2 ee = T.abe[e];
        return {a1.x * qx + a1.y * qy, a2.x * qx + a2.y * qy, b1.x * cx + b1.y * cy, b2.x * cx + b2.y * cy, ee.x, ee.y};
    }
    /* bla_x() with the derivative of the map it applies, from the one load of the entry:
     * J' = norm4((A J, A.e + J.e) (+) (B sm, B.e + es)) */
    static __device__ __forceinline__ BlaStepX bla_x_d(const BlaXTable& T, const uint32_t e, const double qx, const double qy,
                                                       const double cx, const double cy, const double sm, const int es, XJac& J)
    {
        const double2 a1 = T.ab[4 * e], a2 = T.ab[4 * e + 1], b1 = T.ab[4 * e + 2], b2 = T.ab[4 * e + 3];
        const int2 ee = T.abe[e];
        const double2 j1 = J.r1, j2 = J.r2;
        deepx_j_set(J, make_double2(a1.x * j1.x + a1.y * j2.x, a1.x * j1.y + a1.y * j2.y),
                    make_double2(a2.x * j1.x + a2.y * j2.x, a2.x * j1.y + a2.y * j2.y), ee.x + J.e,
                    make_double2(b1.x * sm, b1.y * sm), make_double2(b2.x * sm, b2.y * sm), ee.y + es);
        return {a1.x * qx + a1.y * qy, a2.x * qx + a2.y * qy, b1.x * cx + b1.y * cy, b2.x * cx + b2.y * cy, ee.x, ee.y};
    }
    /* the map of tile_kernel's Burning Ship path, less the centre (burning_ship.comp:337-344: sx outer) */
    static __device__ __forceinline__ double2 dc(const int px, const int py, const int s, const int aa, const double resx,
                                                 const double resy, const double zs)
    {
        const int ux = s / aa, uy = s - ux * aa;
        double uvx = (double)px / resx, uvy = (double)py / resy;
        if (aa > 1) {
            const double pixel_size = 1.0 / resx;
            const double sample_offset = pixel_size / (double)aa;
            const double centre = sample_offset * (double)(aa - 1) * 0.5;
            uvx = uvx + ((double)ux * sample_offset - centre) / resx;
            uvy = uvy + ((double)uy * sample_offset - centre) / resy;
        }
        return make_double2((uvx - 0.5) * zs * (resx / resy), (uvy - 0.5) * zs);
    }

    /* the table build.  The single step at Z = (X, Y): A = [[2X, -2Y], [2|Y| sgn X, 2|X| sgn Y]], B = 1, r = 2^-53 |Z| capped
     * by |X| and |Y| (the fold conditions: below them no fold flips a sign) */
    static __device__ __forceinline__ Lin single(const double2 Z)
    {
        const double ax = fabs(Z.x), ay = fabs(Z.y);
        const double sx = Z.x >= 0.0 ? 1.0 : -1.0, sy = Z.y >= 0.0 ? 1.0 : -1.0;
        Lin s;
        s.a[0] = make_double2(Z.x + Z.x, -(Z.y + Z.y));
        s.a[1] = make_double2((ay + ay) * sx, (ax + ax) * sy);
        s.b[0] = make_double2(1.0, 0.0);
        s.b[1] = make_double2(0.0, 1.0);
        double r = 0x1p-53 * bla_abs(Z.x, Z.y);
        r = r < ax ? r : ax;
        r = r < ay ? r : ay;
        s.r = r;
        return s;
    }
    /* single() with the doubling in A's exponent, r = 2^-53 |norm(Z)| capped by |X| and |Y| as extended reals (a coordinate
     * stored as 0 gives r = 0) */
    static __device__ __forceinline__ LinX single_x(const double2 Z, const int eZ)
    {
        const double ax = fabs(Z.x), ay = fabs(Z.y);
        const double sx = Z.x >= 0.0 ? 1.0 : -1.0, sy = Z.y >= 0.0 ? 1.0 : -1.0;
        LinX s;
        s.a[0] = make_double2(Z.x, -Z.y);
        s.a[1] = make_double2(ay * sx, ax * sy);
        s.ea = eZ + 1;
        x_norm4(s.a[0], s.a[1], s.ea);
        s.b[0] = make_double2(0.5, 0.0);
        s.b[1] = make_double2(0.0, 0.5);
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
    /* A_y A_x and A_y B_x (the caller adds B_y), real 2x2 products */
    template <class L>
    static __device__ __forceinline__ void mul_a(const L& y, const L& x, double2* a)
    {
        a[0] = make_double2(y.a[0].x * x.a[0].x + y.a[0].y * x.a[1].x, y.a[0].x * x.a[0].y + y.a[0].y * x.a[1].y);
        a[1] = make_double2(y.a[1].x * x.a[0].x + y.a[1].y * x.a[1].x, y.a[1].x * x.a[0].y + y.a[1].y * x.a[1].y);
    }
    template <class L>
    static __device__ __forceinline__ void mul_b(const L& y, const L& x, double2* p)
    {
        p[0] = make_double2(y.a[0].x * x.b[0].x + y.a[0].y * x.b[1].x, y.a[0].x * x.b[0].y + y.a[0].y * x.b[1].y);
        p[1] = make_double2(y.a[1].x * x.b[0].x + y.a[1].y * x.b[1].x, y.a[1].x * x.b[0].y + y.a[1].y * x.b[1].y);
    }
    /* |A_x| is the length of A_x's first column (A_x is a scaled orthogonal matrix: its operator norm), |B_x| the Frobenius
     * norm */
    template <class L>
    static __device__ __forceinline__ double norm_a(const L& x) { return bla_abs(x.a[0].x, x.a[1].x); }
    template <class L>
    static __device__ __forceinline__ double norm_b(const L& x)
    {
        return sqrt((x.b[0].x * x.b[0].x + x.b[0].y * x.b[0].y) + (x.b[1].x * x.b[1].x + x.b[1].y * x.b[1].y));
    }
    static __device__ __forceinline__ void norm_rows(double2* m, int& e) { x_norm4(m[0], m[1], e); }
};

/* z <- z^2 + c with c fixed and the sample's offset in z_0 (Julia): Mandelbrot's linear part, the ship's viewport map (the
 * two shaders share it), no dc term, and two orbits -- a sample starts with dz = its offset on the orbit of the centre and
 * rebases onto the critical orbit.  BLA: Mandelbrot's single step and merge without B, dz' = A dz. */
struct JuliaFormula {
    static constexpr int kFractal = 1;
    static constexpr bool kLogBailoutLds = true;      /* shade<double, 1> at bailout <= 1 */
    static constexpr bool kTwoOrbits = true;
    static constexpr bool kHasB = false;              /* no dc term: an entry is (r, A) */
    static constexpr bool kRealJacobian = false;
    static constexpr int kAbPerEntry = 1;             /* complex A */
    using Lin = BlaLin<1>;                            /* b stays unused */
    using LinX = BlaLinX<1>;

    static __device__ __forceinline__ StepLin lin(const double Zx, const double Zy, const double dzx, const double dzy)
    {
        return MandelFormula::lin(Zx, Zy, dzx, dzy);
    }
    static __device__ __forceinline__ StepLinX lin_x(const double Zx, const double Zy, const int eZ, const double dzx,
                                                     const double dzy, const int ed)
    {
        return MandelFormula::lin_x(Zx, Zy, eZ, dzx, dzy, ed);
    }
    /* julia.comp:221-225, :253-264, less the centre: the sample's first delta */
    static __device__ __forceinline__ double2 dc(const int px, const int py, const int s, const int aa, const double resx,
                                                 const double resy, const double zs)
    {
        return ShipFormula::dc(px, py, s, aa, resx, resy, zs);
    }
    /* dz' = A dz, a complex product */
    static __device__ __forceinline__ double2 bla(const BlaTable& T, const uint32_t e, const double dzx,
                                                  const double dzy, const double, const double)
    {
        const double2 a = T.ab[e];
        return make_double2(a.x * dzx - a.y * dzy, a.x * dzy + a.y * dzx);
    }
    /* bla() with the derivative of the map it applies, from the one load of A: D' = A D, nothing added */
    static __device__ __forceinline__ double2 bla_d(const BlaTable& T, const uint32_t e, const double dzx, const double dzy,
                                                    const double, const double, const double, double2& D)
    {
        const double2 a = T.ab[e];
        D = make_double2(a.x * D.x - a.y * D.y, a.x * D.y + a.y * D.x);
        deep_pin_d(D);
        return make_double2(a.x * dzx - a.y * dzy, a.x * dzy + a.y * dzx);
    }
    static __device__ __forceinline__ BlaStepX bla_x(const BlaXTable& T, const uint32_t e, const double qx, const double qy,
                                                     const double, const double)
    {
        const double2 a = T.ab[e];
        return {a.x * qx - a.y * qy, a.x * qy + a.y * qx, 0.0, 0.0, reinterpret_cast<const int32_t*>(T.abe)[e], 0};
    }
    /* bla_x() with the derivative of the map it applies, from the one load of the entry: D' = norm(A D, A.e + D.e), flushed */
    static __device__ __forceinline__ BlaStepX bla_x_d(const BlaXTable& T, const uint32_t e, const double qx, const double qy,
                                                       const double, const double, const double, const int, XDeriv& D)
    {
        const double2 a = T.ab[e];
        const int ea = reinterpret_cast<const int32_t*>(T.abe)[e];
        deepx_d_set(D, a.x * D.x - a.y * D.y, a.x * D.y + a.y * D.x, ea + D.e);
        return {a.x * qx - a.y * qy, a.x * qy + a.y * qx, 0.0, 0.0, ea, 0};
    }

    /* the table build: Mandelbrot's, B never read */
    static __device__ __forceinline__ Lin single(const double2 Z) { return MandelFormula::single(Z); }
    static __device__ __forceinline__ LinX single_x(const double2 Z, const int eZ) { return MandelFormula::single_x(Z, eZ); }
    template <class L>
    static __device__ __forceinline__ void mul_a(const L& y, const L& x, double2* a) { MandelFormula::mul_a(y, x, a); }
    template <class L>
    static __device__ __forceinline__ double norm_a(const L& x) { return MandelFormula::norm_a(x); }
    static __device__ __forceinline__ void norm_rows(double2* m, int& e) { MandelFormula::norm_rows(m, e); }
};

/* ---- the steps ---------------------------------------------------------------------------------------------------------
 * The plain step: dz' from (Z_m, dz, dc) */
template <class F>
__device__ __forceinline__ double2 deep_step(const double Zx, const double Zy, const double dzx, const double dzy,
                                             const double dcx, const double dcy)
{
    const StepLin l = F::lin(Zx, Zy, dzx, dzy);
    if constexpr (F::kTwoOrbits) return make_double2(l.tx * l.fx - l.ty * l.fy, l.tx * l.fy + l.ty * l.fx);
    else return make_double2((l.tx * l.fx - l.ty * l.fy) + dcx, (l.tx * l.fy + l.ty * l.fx) + dcy);
}

/* The derivative's plain step (fr_render_deep_de), at the sample's point before the update: z = Z_m + dz is the sum the previous
 * trip's escape test formed (0 at the start, dz itself behind a rebase: Z_0 = 0), formed again here so that it is not live
 * across the trip; w = z + z; D' = ((w.x D.x - w.y D.y) + s, w.x D.y + w.y D.x) */
__device__ __forceinline__ void deep_step_d(const double Zx, const double Zy, const double dzx, const double dzy, const double s,
                                            double2& D)
{
    const double zx = Zx + dzx, zy = Zy + dzy;
    const double wx = zx + zx, wy = zy + zy;
    D = make_double2((wx * D.x - wy * D.y) + s, wx * D.y + wy * D.x);
    deep_pin_d(D);
}

/* ... of a formula without a dc term (fr_render_deep_julia_de): D' = (w.x D.x - w.y D.y, w.x D.y + w.y D.x), nothing added (adding
 * 0.0 would change the sign of a zero) */
__device__ __forceinline__ void deep_step_d(const double Zx, const double Zy, const double dzx, const double dzy, double2& D)
{
    const double zx = Zx + dzx, zy = Zy + dzy;
    const double wx = zx + zx, wy = zy + zy;
    D = make_double2(wx * D.x - wy * D.y, wx * D.y + wy * D.x);
    deep_pin_d(D);
}

/* The ship's (fr_render_deep_ship_de): L = [[w.x, -w.y], [|w.y| sgn x, |w.x| sgn y]] at the same point (x, y) = Z_m + dz, the
 * derivative of (|x| + i |y|)^2 on the piece the sample's own orbit is on; J' = L J + s I, s added behind each diagonal sum */
__device__ __forceinline__ void deep_step_d(const double Zx, const double Zy, const double dzx, const double dzy, const double s,
                                            Jac& J)
{
    const double x = Zx + dzx, y = Zy + dzy;
    double2 p1, p2;
    ship_lj(x + x, y + y, x, y, J.r1, J.r2, p1, p2);
    J.r1 = make_double2(p1.x + s, p1.y);
    J.r2 = make_double2(p2.x, p2.y + s);
    deep_pin_j(J.r1, J.r2);
}

/* The extended step (the header's EXTENDED step): dz' = (n.x, n.y, en), not normalised */
template <class F>
__device__ __forceinline__ double2 deep_step_x(const double Zx, const double Zy, const int eZ, const double dzx,
                                               const double dzy, const int ed, const double cx, const double cy, const int ec,
                                               int& en)
{
    const StepLinX l = F::lin_x(Zx, Zy, eZ, dzx, dzy, ed);
    const int et = eZ + 1 > ed ? eZ + 1 : ed;
    const double tx = __builtin_ldexp(l.ux, eZ + 1 - et) + __builtin_ldexp(l.fx, ed - et);
    const double ty = __builtin_ldexp(l.uy, eZ + 1 - et) + __builtin_ldexp(l.fy, ed - et);
    const double px = tx * l.fx - ty * l.fy;
    const double py = tx * l.fy + ty * l.fx;
    const int ep = et + ed;
    if constexpr (F::kTwoOrbits) {                                /* n = p */
        en = ep;
        return make_double2(px, py);
    } else {
        en = ep > ec ? ep : ec;
        return make_double2(__builtin_ldexp(px, ep - en) + __builtin_ldexp(cx, ec - en),
                            __builtin_ldexp(py, ep - en) + __builtin_ldexp(cy, ec - en));
    }
}

/* The derivative's extended step (fr_render_deepx_de), at the sample's point before the update: b = (Z_m, eZ) (+) (dz, ed) at
 * eb = max(eZ, ed), the doubling of w = 2 b in the exponent; D' = norm((b D, eb + 1 + D.e) (+) (sm, 0, es)) */
__device__ __forceinline__ void deep_step_xd(const double Zx, const double Zy, const int eZ, const double dzx, const double dzy,
                                             const int ed, const double sm, const int es, XDeriv& D)
{
    const int eb = eZ > ed ? eZ : ed;
    const double bx = __builtin_ldexp(Zx, eZ - eb) + __builtin_ldexp(dzx, ed - eb);
    const double by = __builtin_ldexp(Zy, eZ - eb) + __builtin_ldexp(dzy, ed - eb);
    deepx_d_set(D, bx * D.x - by * D.y, bx * D.y + by * D.x, eb + 1 + D.e, sm, es);
}

/* ... and its plain step on the extended D: deep_step_d's w = 2 (Z_m + dz) on the plain doubles, the product at D.e */
__device__ __forceinline__ void deep_step_pd(const double Zx, const double Zy, const double dzx, const double dzy, const double sm,
                                             const int es, XDeriv& D)
{
    const double zx = Zx + dzx, zy = Zy + dzy;
    const double wx = zx + zx, wy = zy + zy;
    deepx_d_set(D, wx * D.x - wy * D.y, wx * D.y + wy * D.x, D.e, sm, es);
}

/* The ship's two (fr_render_deepx_ship_de): the magnitudes of L from b's mantissas, J' = norm4((L J, eb + 1 + J.e) (+) (sm I, es)).
 * Its signs cannot come from b: aligned to eb, a coordinate far below the other is 0 there and has lost its sign (the tip of the
 * needle: Y = 0 exactly and y = dz.y, 2^-1330 below x).  They are those of fold_x's w, the sum taken in the delta's frame, the
 * same expressions ship_fold_x forms in this trip.  And in the plain mode L from w = 2 (Z_m + dz) on the plain doubles, the
 * product at J.e */
__device__ __forceinline__ void deep_step_xd(const double Zx, const double Zy, const int eZ, const double dzx, const double dzy,
                                             const int ed, const double sm, const int es, XJac& J)
{
    const int eb = eZ > ed ? eZ : ed;
    const double bx = __builtin_ldexp(Zx, eZ - eb) + __builtin_ldexp(dzx, ed - eb);
    const double by = __builtin_ldexp(Zy, eZ - eb) + __builtin_ldexp(dzy, ed - eb);
    const double wx = __builtin_ldexp(Zx, eZ - ed) + dzx, wy = __builtin_ldexp(Zy, eZ - ed) + dzy;
    double2 p1, p2;
    ship_lj(bx, by, wx, wy, J.r1, J.r2, p1, p2);
    deepx_j_set(J, p1, p2, eb + 1 + J.e, sm, es);
}

__device__ __forceinline__ void deep_step_pd(const double Zx, const double Zy, const double dzx, const double dzy, const double sm,
                                             const int es, XJac& J)
{
    const double x = Zx + dzx, y = Zy + dzy;
    double2 p1, p2;
    ship_lj(x + x, y + y, x, y, J.r1, J.r2, p1, p2);
    deepx_j_set(J, p1, p2, J.e, sm, es);
}

/* ... and the two of a formula without a dc term (fr_render_deepx_julia_de): D' = norm(b D, eb + 1 + D.e) and D' = norm(w D, D.e),
 * each flushed */
__device__ __forceinline__ void deep_step_xd(const double Zx, const double Zy, const int eZ, const double dzx, const double dzy,
                                             const int ed, XDeriv& D)
{
    const int eb = eZ > ed ? eZ : ed;
    const double bx = __builtin_ldexp(Zx, eZ - eb) + __builtin_ldexp(dzx, ed - eb);
    const double by = __builtin_ldexp(Zy, eZ - eb) + __builtin_ldexp(dzy, ed - eb);
    deepx_d_set(D, bx * D.x - by * D.y, bx * D.y + by * D.x, eb + 1 + D.e);
}

__device__ __forceinline__ void deep_step_pd(const double Zx, const double Zy, const double dzx, const double dzy, XDeriv& D)
{
    const double zx = Zx + dzx, zy = Zy + dzy;
    const double wx = zx + zx, wy = zy + zy;
    deepx_d_set(D, wx * D.x - wy * D.y, wx * D.y + wy * D.x, D.e);
}

/* ---- the tables --------------------------------------------------------------------------------------------------------
 * Entries before level k (>= 1) of a table over n1 = N - 1 single steps: sum_{i=1}^{k-1} (n1 >> i).  With
 * S(x) = sum_{i>=1} (x >> i) = x - popcount(x) that is S(n1) - S(n1 >> (k - 1)). */
__device__ __forceinline__ uint32_t bla_offset(const uint32_t n1, const int k)
{
    const uint32_t t = n1 >> (k - 1);
    return (n1 - (uint32_t)__popc(n1)) - (t - (uint32_t)__popc(t));
}

/* Level k of an fp64 table: entry j merges x (level k - 1, entry 2j) and y (level k - 1, entry 2j + 1); level 0 is the single
 * step at m = 1 + i, computed from the orbit and never stored.  A = A_y A_x, B = A_y B_x + B_y,
 * r = min(r_x, max(0, (r_y - |B_x| dcmax) / |A_x|)), 0 when an element is not finite.  A formula without B (Julia) has
 * neither B nor dcmax: r = min(r_x, max(0, r_y / |A_x|)). */
template <class F>
__device__ __forceinline__ void bla_level(const double2* __restrict__ orbit, const int32_t n_ref, const int32_t k,
                                          const double dcmax, double* __restrict__ r, double2* __restrict__ ab)
{
    constexpr int S = F::kAbPerEntry;                            /* double2 per entry: A's rows, then B's */
    constexpr int R = F::kHasB ? S / 2 : S;
    const uint32_t n1 = (uint32_t)(n_ref - 1);
    const uint32_t cnt = n1 >> k;
    const uint32_t off = bla_offset(n1, k);
    const uint32_t offp = k > 1 ? bla_offset(n1, k - 1) : 0u;
    for (uint32_t j = blockIdx.x * kBlockThreads + threadIdx.x; j < cnt; j += gridDim.x * kBlockThreads) {
        typename F::Lin x, y;
        if (k == 1) {
            x = F::single(orbit[1 + 2 * j]);
            y = F::single(orbit[2 + 2 * j]);
        } else {
            const uint32_t ex = offp + 2 * j, ey = ex + 1;
            for (int i = 0; i < R; ++i) {
                x.a[i] = ab[S * ex + i];
                if constexpr (F::kHasB) x.b[i] = ab[S * ex + R + i];
            }
            x.r = r[ex];
            for (int i = 0; i < R; ++i) {
                y.a[i] = ab[S * ey + i];
                if constexpr (F::kHasB) y.b[i] = ab[S * ey + R + i];
            }
            y.r = r[ey];
        }
        double2 a[R], b[R];
        F::mul_a(y, x, a);
        if constexpr (F::kHasB) F::mul_b(y, x, b);
        bool finite = true;
        for (int i = 0; i < R; ++i) {
            if constexpr (F::kHasB) {
                b[i] = make_double2(b[i].x + y.b[i].x, b[i].y + y.b[i].y);
                finite = finite && __builtin_isfinite(a[i].x) && __builtin_isfinite(a[i].y) && __builtin_isfinite(b[i].x) &&
                         __builtin_isfinite(b[i].y);
            } else {
                finite = finite && __builtin_isfinite(a[i].x) && __builtin_isfinite(a[i].y);
            }
        }
        double t;
        if constexpr (F::kHasB) t = (y.r - F::norm_b(x) * dcmax) / F::norm_a(x);
        else t = y.r / F::norm_a(x);
        double rr = t > 0.0 ? t : 0.0;                           /* NaN: 0 */
        rr = rr < x.r ? rr : x.r;
        if (!finite) rr = 0.0;
        const uint32_t e = off + j;
        r[e] = rr;
        for (int i = 0; i < R; ++i) {
            ab[S * e + i] = a[i];
            if constexpr (F::kHasB) ab[S * e + R + i] = b[i];
        }
    }
}

/* Level k of an extended table: bla_level with (A, B, r) carrying int32 exponents, from the extended orbit arrays.  An entry
 * whose A.e or B.e leaves [-2^27, 2^27] is void (all zero); the stored radius is cut to 24 bits.  A formula without B (Julia)
 * stores A.e alone, an int32 per entry in abe, and has t = r_y (/) |A_x|. */
template <class F>
__device__ __forceinline__ void bla_level_x(const double2* __restrict__ mant, const int32_t* __restrict__ exp2,
                                            const int32_t n_ref, const int32_t k, const double dcv, const int32_t dce,
                                            XRad* __restrict__ r, double2* __restrict__ ab, int2* __restrict__ abe)
{
    constexpr int S = F::kAbPerEntry;                            /* double2 per entry: A's rows, then B's */
    constexpr int R = F::kHasB ? S / 2 : S;
    int32_t* __restrict__ const ae1 = reinterpret_cast<int32_t*>(abe);   /* without B: A.e of every entry */
    const uint32_t n1 = (uint32_t)(n_ref - 1);
    const uint32_t cnt = n1 >> k;
    const uint32_t off = bla_offset(n1, k);
    const uint32_t offp = k > 1 ? bla_offset(n1, k - 1) : 0u;
    for (uint32_t j = blockIdx.x * kBlockThreads + threadIdx.x; j < cnt; j += gridDim.x * kBlockThreads) {
        typename F::LinX x, y;
        if (k == 1) {
            x = F::single_x(mant[1 + 2 * j], exp2[1 + 2 * j]);
            y = F::single_x(mant[2 + 2 * j], exp2[2 + 2 * j]);
        } else {
            const uint32_t ex = offp + 2 * j, ey = ex + 1;
            const XRad rx = r[ex], ry = r[ey];
            if constexpr (F::kHasB) {
                const int2 eex = abe[ex], eey = abe[ey];
                for (int i = 0; i < R; ++i) { x.a[i] = ab[S * ex + i]; x.b[i] = ab[S * ex + R + i]; }
                x.ea = eex.x; x.eb = eex.y;
                for (int i = 0; i < R; ++i) { y.a[i] = ab[S * ey + i]; y.b[i] = ab[S * ey + R + i]; }
                y.ea = eey.x; y.eb = eey.y;
            } else {
                for (int i = 0; i < R; ++i) { x.a[i] = ab[S * ex + i]; y.a[i] = ab[S * ey + i]; }
                x.ea = ae1[ex]; y.ea = ae1[ey];
            }
            x.rv = (double)rx.v; x.re = rx.e;
            y.rv = (double)ry.v; y.re = ry.e;
        }
        double2 a[R], p[R], b[R];
        F::mul_a(y, x, a);
        int ea = y.ea + x.ea;
        F::norm_rows(a, ea);
        int eb = 0;
        double av = F::norm_a(x);
        int ae = x.ea;
        x_norm1(av, ae);
        double t;
        int et;
        if constexpr (F::kHasB) {
            F::mul_b(y, x, p);
            const int e1 = y.ea + x.eb;
            eb = e1 > y.eb ? e1 : y.eb;
            for (int i = 0; i < R; ++i)
                b[i] = make_double2(__builtin_ldexp(p[i].x, e1 - eb) + __builtin_ldexp(y.b[i].x, y.eb - eb),
                                    __builtin_ldexp(p[i].y, e1 - eb) + __builtin_ldexp(y.b[i].y, y.eb - eb));
            F::norm_rows(b, eb);
            double bv = F::norm_b(x);
            int be = x.eb;
            x_norm1(bv, be);
            const double pv = bv * dcv;
            const int pe = be + dce;
            et = y.re > pe ? y.re : pe;
            t = (__builtin_ldexp(y.rv, y.re - et) - __builtin_ldexp(pv, pe - et)) / av;
        } else {
            et = y.re;
            t = y.rv / av;
        }
        double rv = (t > 0.0 && __builtin_isfinite(t)) ? t : 0.0;    /* NaN: 0 */
        int re = et - ae;
        x_norm1(rv, re);
        if (!x_less(rv, re, x.rv, x.re)) { rv = x.rv; re = x.re; }
        const int la = ea < 0 ? -ea : ea, lb = eb < 0 ? -eb : eb;
        if (la > kXBlaExpLim || lb > kXBlaExpLim) {
            rv = 0.0; re = kXZero;
            for (int i = 0; i < R; ++i) { a[i] = make_double2(0.0, 0.0); b[i] = make_double2(0.0, 0.0); }
            ea = kXZero; eb = kXZero;
        }
        const uint32_t e = off + j;
        XRad out;
        out.v = (float)x_trunc24(rv); out.e = re;
        r[e] = out;
        if constexpr (F::kHasB) {
            for (int i = 0; i < R; ++i) { ab[S * e + i] = a[i]; ab[S * e + R + i] = b[i]; }
            abe[e] = make_int2(ea, eb);
        } else {
            for (int i = 0; i < R; ++i) ab[S * e + i] = a[i];
            ae1[e] = ea;
        }
    }
}

__global__ void __launch_bounds__(kBlockThreads)
deep_bla_level_kernel(const double2* __restrict__ orbit, const int32_t n_ref, const int32_t k, const double dcmax,
                      double* __restrict__ r, double2* __restrict__ ab)
{
    bla_level<MandelFormula>(orbit, n_ref, k, dcmax, r, ab);
}

__global__ void __launch_bounds__(kBlockThreads)
deep_ship_bla_level_kernel(const double2* __restrict__ orbit, const int32_t n_ref, const int32_t k, const double dcmax,
                           double* __restrict__ r, double2* __restrict__ ab)
{
    bla_level<ShipFormula>(orbit, n_ref, k, dcmax, r, ab);
}

__global__ void __launch_bounds__(kBlockThreads)
deepx_bla_level_kernel(const double2* __restrict__ mant, const int32_t* __restrict__ exp2, const int32_t n_ref, const int32_t k,
                       const double dcv, const int32_t dce, XRad* __restrict__ r, double2* __restrict__ ab,
                       int2* __restrict__ abe)
{
    bla_level_x<MandelFormula>(mant, exp2, n_ref, k, dcv, dce, r, ab, abe);
}

__global__ void __launch_bounds__(kBlockThreads)
deepx_ship_bla_level_kernel(const double2* __restrict__ mant, const int32_t* __restrict__ exp2, const int32_t n_ref,
                            const int32_t k, const double dcv, const int32_t dce, XRad* __restrict__ r,
                            double2* __restrict__ ab, int2* __restrict__ abe)
{
    bla_level_x<ShipFormula>(mant, exp2, n_ref, k, dcv, dce, r, ab, abe);
}

/* Julia: one launch per level and orbit.  orbit / mant / exp2 point at the orbit's point 0 (Q's, or P's behind it), r / ab / ae
 * at the first entry of that orbit's table */
__global__ void __launch_bounds__(kBlockThreads)
deep_julia_bla_level_kernel(const double2* __restrict__ orbit, const int32_t n_ref, const int32_t k, double* __restrict__ r,
                            double2* __restrict__ ab)
{
    bla_level<JuliaFormula>(orbit, n_ref, k, 0.0, r, ab);
}

__global__ void __launch_bounds__(kBlockThreads)
deepx_julia_bla_level_kernel(const double2* __restrict__ mant, const int32_t* __restrict__ exp2, const int32_t n_ref,
                             const int32_t k, XRad* __restrict__ r, double2* __restrict__ ab, int32_t* __restrict__ ae)
{
    bla_level_x<JuliaFormula>(mant, exp2, n_ref, k, 0.0, 0, r, ab, reinterpret_cast<int2*>(ae));
}

/* ---- the level probes --------------------------------------------------------------------------------------------------
 * The level a lane at m >= 1 with u updates behind it probes first: min(ctz(m - 1), K, floor(log2(N - m)),
 * floor(log2(max_iter - u))) */
__device__ __forceinline__ int bla_top_level(const uint32_t mm, const int K, const int N, const int m, const int max_iter,
                                             const int u)
{
    int kk = mm ? __builtin_ctz(mm) : K;
    kk = kk < K ? kk : K;
    const int kn = 31 - __builtin_clz((uint32_t)(N - m));
    const int ki = 31 - __builtin_clz((uint32_t)(max_iter - u));
    kk = kk < kn ? kk : kn;
    kk = kk < ki ? kk : ki;
    return kk;
}

struct BlaHit {
    int k;                               /* the level taken, 0 = none */
    uint32_t e;                          /* its entry */
};

/* The fp64 probe: the levels top down, the first k with |dz|^2 < r^2.  No level's r exceeds the single step's 2^-53 |Z_m| (r
 * only ever shrinks in the merge, the ship's fold caps only lower it), so a lane with |dz|^2 2^104 >= |Z_m|^2 (a bound above
 * 2^-106 |Z_m|^2 with room for every rounding) cannot pass a probe and gathers nothing. */
__device__ __forceinline__ BlaHit bla_probe(const double* tr, const uint32_t n1, const int K, const int N,
                                            const int max_iter, const int m, const int u, const double dz2, const double Zx,
                                            const double Zy)
{
    BlaHit h = {0, 0u};
    if (m >= 1 && dz2 * 0x1p104 < Zx * Zx + Zy * Zy) {
        const uint32_t mm = (uint32_t)(m - 1);
        for (int kk = bla_top_level(mm, K, N, m, max_iter, u); kk >= 1; --kk) {
            const uint32_t ek = bla_offset(n1, kk) + (mm >> kk);
            const double r = tr[ek];
            if (dz2 < r * r) { h.k = kk; h.e = ek; break; }
        }
    }
    return h;
}

struct BlaHitX {
    int k;
    uint32_t e;
    double qx, qy;                       /* dz, extended and normalised */
    int qe;
};

/* The extended probe, for a lane in either mode: on its dz as a normalised extended number (a plain lane forms
 * norm(dz.x, dz.y, 0)).  No level's r exceeds 2^-53 |Z_m| < 2^(E - 52.5), E the exponent of Z_m's larger component normalised,
 * and |dz| >= 2^(dz.e - 1): a lane with dz.e + 51 >= E cannot pass a probe and gathers nothing (E from the lane's own copy of
 * Z_m: for a point below 2^-1022 the plain double's exponent is never below the true one). */
__device__ __forceinline__ BlaHitX bla_probe_x(const XRad* tr, const uint32_t n1, const int K, const int N,
                                               const int max_iter, const int m, const int u, const bool ext, const double dzx,
                                               const double dzy, const int ed, const double Zx, const double Zy, const int eZ)
{
    BlaHitX h = {0, 0u, dzx, dzy, ed};
    if (m >= 1) {
        if (!ext) { h.qe = 0; x_norm(h.qx, h.qy, h.qe); }
        const int eZm = (ext ? eZ : 0) + __builtin_amdgcn_frexp_exp(fmax(fabs(Zx), fabs(Zy)));
        if (h.qe + 51 < eZm) {
            const double dz2 = h.qx * h.qx + h.qy * h.qy;
            const uint32_t mm = (uint32_t)(m - 1);
            for (int kk = bla_top_level(mm, K, N, m, max_iter, u); kk >= 1; --kk) {
                const uint32_t ek = bla_offset(n1, kk) + (mm >> kk);
                const XRad r = tr[ek];
                const double rv = (double)r.v;
                if (dz2 < __builtin_ldexp(rv * rv, 2 * (r.e - h.qe))) { h.k = kk; h.e = ek; break; }
            }
        }
    }
    return h;
}

/* the derivative a loop carries for a formula: a complex number, or the ship's matrix */
template <class F> using DeepD = std::conditional_t<F::kRealJacobian, Jac, double2>;
template <class F> using DeepXD = std::conditional_t<F::kRealJacobian, XJac, XDeriv>;

/* ---- the per-sample loops ----------------------------------------------------------------------------------------------
 * The wave's 64 samples, one per lane.  live = false: a lane without a sample (outside the frame).  esc = the loop index
 * of the escaping update (max_iter if none), r2 = |z|^2 there.  z = Z_{m+1} + dz' with the signed orbit point for either
 * formula (Z_0 = 0: at m = 0 the ship's step is (|dz.x| + i |dz.y|)^2 + dc). */
template <class F, bool DE = false>
__device__ __forceinline__ void deep_orbit(const DeepArgs& A, const JuliaStart J, const double dcx, const double dcy,
                                           const double2 z1, bool live, int& esc, double& er2, const double s = 0.0,
                                           DeepD<F>* const Dout = nullptr)
{
    const double2* __restrict__ orbit = A.orbit;
    const int max_iter = A.max_iter;
    int N = A.n_ref;                                             /* of the lane's orbit: Julia's lanes start on P */
    int base = 0;                                                /* where that orbit starts in `orbit` */
    const double B2 = A.B2;
    double dzx = 0.0, dzy = 0.0;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m */
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    if constexpr (F::kTwoOrbits) {                               /* dz = the sample's offset, on P: one point for all lanes */
        base = J.p_off; N = J.n_p;
        const double2 p0 = orbit[base], p1 = orbit[base + 1];
        dzx = dcx; dzy = dcy;
        Zx = p0.x; Zy = p0.y; Znx = p1.x; Zny = p1.y;
    }
    int m = 0;
    esc = max_iter;
    er2 = 0.0;
    DeepD<F> D;                                                  /* DE: dz/dc * s, through the escaping update */
    if constexpr (F::kRealJacobian) D.r1 = D.r2 = D.z = make_double2(0.0, 0.0);
    else D = make_double2(0.0, 0.0);
    if constexpr (DE && !F::kHasB) D.x = s;                      /* ... without a dc term dz_n/dz_0 * s: (s, +0.0) at the start */
    for (int i = 0; i < max_iter; ++i) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const double2 Znn = orbit[base + (m + 2 <= N ? m + 2 : N)];   /* Z_{m+2}, for the next step (m + 1 < N) */
        if constexpr (DE && F::kHasB) deep_step_d(Zx, Zy, dzx, dzy, s, D);
        else if constexpr (DE) deep_step_d(Zx, Zy, dzx, dzy, D);
        const double2 n = deep_step<F>(Zx, Zy, dzx, dzy, dcx, dcy);
        const double nx = n.x, ny = n.y;
        ++m;
        const double zx = Znx + nx, zy = Zny + ny;
        const double r2 = zx * zx + zy * zy;
        if (r2 > B2) {
            esc = i; er2 = r2; live = false;
            if constexpr (DE && F::kRealJacobian) { dzx = zx; dzy = zy; }   /* z, for the gradient of |z| */
        } else if (r2 < nx * nx + ny * ny || m == N) {           /* rebase */
            dzx = zx; dzy = zy; m = 0;
            Zx = 0.0; Zy = 0.0; Znx = z1.x; Zny = z1.y;
            if constexpr (F::kTwoOrbits) { base = 0; N = A.n_ref; }   /* onto Q, for good */
        } else {
            dzx = nx; dzy = ny;
            Zx = Znx; Zy = Zny; Znx = Znn.x; Zny = Znn.y;
        }
    }
    if constexpr (DE && F::kRealJacobian) D.z = make_double2(dzx, dzy);
    if constexpr (DE) *Dout = D;
}

/* deep_orbit with BLA: u replaces the loop index.  A lane probes the table (bla_probe) and takes the level it finds, else
 * the plain step.  A BLA lane loads Z_m and Z_{m+1} at its new m (the Z_{m+2} prefetch is for the plain step); BLA and plain
 * lanes of a wave take their steps in the same trip.  nplain / nbla: the steps this sample took.  Two orbits (J, levels_p and
 * base_p of P's table): the lane's orbit base, N, and its table's entry base, n1 and K are P's until the first rebase.
 * DE: a BLA step takes D through the derivative of the linear map it applies, from the (A, B) it loads anyway (F::bla_d). */
template <class F, bool DE = false>
__device__ __forceinline__ void deep_orbit_bla(const DeepArgs& A, const BlaTable& T, const JuliaStart J, const int levels_p,
                                               const uint32_t base_p, const double dcx, const double dcy, const double2 z1,
                                               bool live, int& esc, double& er2, uint32_t& nplain, uint32_t& nbla,
                                               const double s = 0.0, DeepD<F>* const Dout = nullptr)
{
    const double2* __restrict__ orbit = A.orbit;
    const double* __restrict__ tr = T.r;
    const int max_iter = A.max_iter;
    int N = A.n_ref, K = T.levels;
    uint32_t n1 = (uint32_t)(N - 1);
    int base = 0;                                                /* where the lane's orbit starts in `orbit` */
    uint32_t tb = 0u;                                            /* ... and its table in tr / T.ab */
    const double B2 = A.B2;
    double dzx = 0.0, dzy = 0.0;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m */
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    if constexpr (F::kTwoOrbits) {                               /* dz = the sample's offset, on P: one point for all lanes */
        base = J.p_off; N = J.n_p; K = levels_p; n1 = (uint32_t)(N - 1); tb = base_p;
        const double2 p0 = orbit[base], p1 = orbit[base + 1];
        dzx = dcx; dzy = dcy;
        Zx = p0.x; Zy = p0.y; Znx = p1.x; Zny = p1.y;
    }
    int m = 0, u = 0;
    esc = max_iter;
    er2 = 0.0;
    nplain = 0u; nbla = 0u;
    DeepD<F> D;                                                  /* DE: dz/dc * s, through the escaping update */
    if constexpr (F::kRealJacobian) D.r1 = D.r2 = D.z = make_double2(0.0, 0.0);
    else D = make_double2(0.0, 0.0);
    if constexpr (DE && !F::kHasB) D.x = s;                      /* ... without a dc term dz_n/dz_0 * s: (s, +0.0) at the start */
    for (;;) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const double2 Znn = orbit[base + (m + 2 <= N ? m + 2 : N)];   /* Z_{m+2}, for a plain step */
        const double dz2 = dzx * dzx + dzy * dzy;
        const BlaHit h = bla_probe(tr + tb, n1, K, N, max_iter, m, u, dz2, Zx, Zy);
        const int k = h.k;
        double2 n;
        double Zmx, Zmy;
        int step;
        if (k > 0) {
            if constexpr (DE) n = F::bla_d(T, tb + h.e, dzx, dzy, dcx, dcy, s, D);
            else n = F::bla(T, tb + h.e, dzx, dzy, dcx, dcy);
            step = 1 << k;
            ++nbla;
            m += step;
            const double2 Zm = orbit[base + m];
            Zmx = Zm.x; Zmy = Zm.y;
        } else {
            if constexpr (DE && F::kHasB) deep_step_d(Zx, Zy, dzx, dzy, s, D);
            else if constexpr (DE) deep_step_d(Zx, Zy, dzx, dzy, D);
            n = deep_step<F>(Zx, Zy, dzx, dzy, dcx, dcy);
            step = 1;
            ++nplain;
            m += 1;
            Zmx = Znx; Zmy = Zny;
        }
        u += step;
        const double nx = n.x, ny = n.y;
        const double zx = Zmx + nx, zy = Zmy + ny;
        const double r2 = zx * zx + zy * zy;
        if (r2 > B2) {
            esc = u - 1; er2 = r2; live = false;                 /* the last update the step covered */
            if constexpr (DE && F::kRealJacobian) { dzx = zx; dzy = zy; }   /* z, for the gradient of |z| */
        } else if (r2 < nx * nx + ny * ny || m == N) {           /* rebase */
            dzx = zx; dzy = zy; m = 0;
            Zx = 0.0; Zy = 0.0; Znx = z1.x; Zny = z1.y;
            if constexpr (F::kTwoOrbits) {                        /* onto Q and its table, for good */
                base = 0; N = A.n_ref; K = T.levels; n1 = (uint32_t)(N - 1); tb = 0u;
            }
        } else {
            dzx = nx; dzy = ny;
            Zx = Zmx; Zy = Zmy;
            if (k > 0) {                                          /* m < N here */
                const double2 Zn = orbit[base + m + 1];
                Znx = Zn.x; Zny = Zn.y;
            } else {
                Znx = Znn.x; Zny = Znn.y;
            }
        }
        if (u >= max_iter) live = false;                          /* esc stays max_iter */
    }
    if constexpr (DE && F::kRealJacobian) D.z = make_double2(dzx, dzy);
    if constexpr (DE) *Dout = D;
}

/* deep_orbit in two modes (the header's EXTENDED and PLAIN steps).  (cx, cy, ec) = dc, normalised.  z = Z_{m+1} (+) n with the
 * signed orbit point; escape, rebase, norm and the mode rule are the same for either formula. */
template <class F, bool DE = false>
__device__ __forceinline__ void deep_orbit_x(const DeepArgs& A, const DeepXOrbit& AX, const JuliaStart J, const double cx,
                                             const double cy, const int ec, bool live, int& esc, double& er2,
                                             const double sm = 0.0, const int es = 0, DeepXD<F>* const Dout = nullptr)
{
    const double2* __restrict__ orbit = A.orbit;
    const double2* __restrict__ mant = AX.mant;
    const int32_t* __restrict__ exp2 = AX.exp2;
    const int max_iter = A.max_iter;
    int N = A.n_ref;                                             /* of the lane's orbit, which starts at `base` in the arrays */
    int base = 0;
    const double B2 = A.B2;
    const double cpx = x_plain(cx, ec), cpy = x_plain(cy, ec);   /* the plain mode's dc */
    double dzx = 0.0, dzy = 0.0;                                 /* plain: dz; extended: its mantissas */
    int ed = kXZero;
    bool ext = true;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m, in the lane's mode */
    int eZ = kXZero;
    const double2 z1 = mant[1];
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    int eZn = exp2[1];
    if constexpr (F::kTwoOrbits) {                               /* dz = the sample's offset (cx, cy, ec), on P, in its mode */
        base = J.p_off; N = J.n_p;
        ext = ec <= kXThr;
        if (ext) {
            const double2 a = mant[base], b = mant[base + 1];
            dzx = cx; dzy = cy; ed = ec;
            Zx = a.x; Zy = a.y; eZ = exp2[base]; Znx = b.x; Zny = b.y; eZn = exp2[base + 1];
        } else {
            const double2 a = orbit[base], b = orbit[base + 1];
            dzx = __builtin_ldexp(cx, ec); dzy = __builtin_ldexp(cy, ec);
            Zx = a.x; Zy = a.y; Znx = b.x; Zny = b.y;
        }
    }
    int m = 0;
    esc = max_iter;
    er2 = 0.0;
    DeepXD<F> D;                                                 /* DE: dz/dc * s, through the escaping update */
    if constexpr (F::kRealJacobian) { D.r1 = D.r2 = D.z = make_double2(0.0, 0.0); D.e = kXZero; }
    else D = XDeriv{0.0, 0.0, kXZero};
    if constexpr (DE && !F::kHasB) { D.x = sm; D.e = es; }       /* ... without a dc term dz_n/dz_0 * s: (sm, +0.0, es) at first */
    for (int i = 0; i < max_iter; ++i) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const int mn = base + (m + 2 <= N ? m + 2 : N);          /* Z_{m+2}, for the next step (m + 1 < N) */
        double ax, ay;                                           /* the next dz */
        int ea = 0;
        bool reb;
        if (ext) {
            const double2 Znn = mant[mn];
            const int eZnn = exp2[mn];
            int en;
            if constexpr (DE && F::kHasB) deep_step_xd(Zx, Zy, eZ, dzx, dzy, ed, sm, es, D);
            else if constexpr (DE) deep_step_xd(Zx, Zy, eZ, dzx, dzy, ed, D);
            const double2 n = deep_step_x<F>(Zx, Zy, eZ, dzx, dzy, ed, cx, cy, ec, en);
            const double nx = n.x, ny = n.y;
            ++m;
            const int ez = eZn > en ? eZn : en;
            const double zx = __builtin_ldexp(Znx, eZn - ez) + __builtin_ldexp(nx, en - ez);
            const double zy = __builtin_ldexp(Zny, eZn - ez) + __builtin_ldexp(ny, en - ez);
            const double r2 = zx * zx + zy * zy;
            const double r2d = __builtin_ldexp(r2, 2 * ez);
            if (r2d > B2) {
                esc = i; er2 = r2d; live = false;
                if constexpr (DE && F::kRealJacobian) { dzx = __builtin_ldexp(zx, ez); dzy = __builtin_ldexp(zy, ez); }   /* z */
                continue;
            }
            reb = r2 < __builtin_ldexp(nx * nx + ny * ny, 2 * (en - ez)) || m == N;
            ax = reb ? zx : nx; ay = reb ? zy : ny; ea = reb ? ez : en;
            x_norm(ax, ay, ea);
            if constexpr (F::kTwoOrbits) {
                if (ea < kXFlushExp) { ax = 0.0; ay = 0.0; ea = kXZero; }   /* FLUSH */
                if (reb) { base = 0; N = A.n_ref; }               /* onto Q, for good */
            }
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
            if constexpr (DE && F::kHasB) deep_step_pd(Zx, Zy, dzx, dzy, sm, es, D);
            else if constexpr (DE) deep_step_pd(Zx, Zy, dzx, dzy, D);
            const double2 n = deep_step<F>(Zx, Zy, dzx, dzy, cpx, cpy);
            const double nx = n.x, ny = n.y;
            ++m;
            const double zx = Znx + nx, zy = Zny + ny;
            const double r2 = zx * zx + zy * zy;
            if (r2 > B2) {
                esc = i; er2 = r2; live = false;
                if constexpr (DE && F::kRealJacobian) { dzx = zx; dzy = zy; }   /* z, for the gradient of |z| */
                continue;
            }
            reb = r2 < nx * nx + ny * ny || m == N;
            ax = reb ? zx : nx; ay = reb ? zy : ny;
            if (reb) m = 0;
            if constexpr (F::kTwoOrbits) {
                if (reb) { base = 0; N = A.n_ref; }
            }
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
            const double2 a = mant[base + m], b = mant[base + m + 1];
            Zx = a.x; Zy = a.y; eZ = exp2[base + m]; Znx = b.x; Zny = b.y; eZn = exp2[base + m + 1];
        } else {
            const double2 a = orbit[base + m], b = orbit[base + m + 1];
            Zx = a.x; Zy = a.y; Znx = b.x; Zny = b.y;
        }
    }
    if constexpr (DE && F::kRealJacobian) D.z = make_double2(dzx, dzy);
    if constexpr (DE) *Dout = D;
}

/* deep_orbit_x with BLA: u replaces the loop index.  A lane, in either mode, probes the table (bla_probe_x); a BLA step is
 * taken in extended arithmetic whatever the lane's mode, its loads inside the taken branch, and the lane reloads Z_m, Z_{m+1}
 * in the mode the step leaves it in.  The single steps are deep_orbit_x's, operation for operation.  BLA lanes and
 * single-step lanes of a wave take their steps in the same trip.  nsingle / nbla: the steps this sample took.  Two orbits: as
 * deep_orbit_bla, and a BLA step ends with the flush of deep_orbit_x. */
template <class F, bool DE = false>
__device__ __forceinline__ void deep_orbit_x_bla(const DeepArgs& A, const DeepXOrbit& AX, const BlaXTable& T, const JuliaStart J,
                                                 const int levels_p, const uint32_t base_p, const double cx, const double cy,
                                                 const int ec, bool live, int& esc, double& er2, uint32_t& nsingle,
                                                 uint32_t& nbla, const double sm = 0.0, const int es = 0,
                                                 DeepXD<F>* const Dout = nullptr)
{
    const double2* __restrict__ orbit = A.orbit;
    const double2* __restrict__ mant = AX.mant;
    const int32_t* __restrict__ exp2 = AX.exp2;
    const XRad* __restrict__ tr = T.r;
    const int max_iter = A.max_iter;
    int N = A.n_ref, K = T.levels;
    uint32_t n1 = (uint32_t)(N - 1);
    int base = 0;                                                /* where the lane's orbit starts in the arrays */
    uint32_t tb = 0u;                                            /* ... and its table in tr / T.ab / T.abe */
    const double B2 = A.B2;
    const double cpx = x_plain(cx, ec), cpy = x_plain(cy, ec);   /* the plain mode's dc */
    double dzx = 0.0, dzy = 0.0;                                 /* plain: dz; extended: its mantissas */
    int ed = kXZero;
    bool ext = true;
    double Zx = 0.0, Zy = 0.0;                                   /* Z_m, in the lane's mode */
    int eZ = kXZero;
    const double2 z1 = mant[1];
    const int e1 = exp2[1];
    double Znx = z1.x, Zny = z1.y;                               /* Z_{m+1} */
    int eZn = e1;
    if constexpr (F::kTwoOrbits) {                               /* dz = the sample's offset (cx, cy, ec), on P, in its mode */
        base = J.p_off; N = J.n_p; K = levels_p; n1 = (uint32_t)(N - 1); tb = base_p;
        ext = ec <= kXThr;
        if (ext) {
            const double2 a = mant[base], b = mant[base + 1];
            dzx = cx; dzy = cy; ed = ec;
            Zx = a.x; Zy = a.y; eZ = exp2[base]; Znx = b.x; Zny = b.y; eZn = exp2[base + 1];
        } else {
            const double2 a = orbit[base], b = orbit[base + 1];
            dzx = __builtin_ldexp(cx, ec); dzy = __builtin_ldexp(cy, ec);
            Zx = a.x; Zy = a.y; Znx = b.x; Zny = b.y;
        }
    }
    int m = 0, u = 0;
    esc = max_iter;
    er2 = 0.0;
    nsingle = 0u; nbla = 0u;
    DeepXD<F> D;                                                 /* DE: dz/dc * s, through the escaping update */
    if constexpr (F::kRealJacobian) { D.r1 = D.r2 = D.z = make_double2(0.0, 0.0); D.e = kXZero; }
    else D = XDeriv{0.0, 0.0, kXZero};
    if constexpr (DE && !F::kHasB) { D.x = sm; D.e = es; }       /* ... without a dc term dz_n/dz_0 * s: (sm, +0.0, es) at first */
    for (;;) {
        if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
        if (!live) continue;
        const int mn = base + (m + 2 <= N ? m + 2 : N);          /* Z_{m+2}, for the single step after this one */
        const BlaHitX h = bla_probe_x(tr + tb, n1, K, N, max_iter, m, u, ext, dzx, dzy, ed, Zx, Zy, eZ);
        const int k = h.k;
        double ax, ay;                                           /* the next dz */
        int ea = 0;
        bool reb;
        if (k > 0 || ext) {
            double nx, ny, Wx, Wy;                               /* n and Z at the new m */
            int en, eW, eZnn = 0;
            double2 Znn = make_double2(0.0, 0.0);
            if (k > 0) {
                BlaStepX s;
                if constexpr (DE) s = F::bla_x_d(T, tb + h.e, h.qx, h.qy, cx, cy, sm, es, D);
                else s = F::bla_x(T, tb + h.e, h.qx, h.qy, cx, cy);
                const int ep = s.ea + h.qe;
                if constexpr (F::kHasB) {
                    const int eq = s.eb + ec;
                    en = ep > eq ? ep : eq;
                    nx = __builtin_ldexp(s.px, ep - en) + __builtin_ldexp(s.sx, eq - en);
                    ny = __builtin_ldexp(s.py, ep - en) + __builtin_ldexp(s.sy, eq - en);
                } else {                                          /* n = A (x) dz */
                    en = ep;
                    nx = s.px; ny = s.py;
                }
                m += 1 << k;
                u += 1 << k;
                ++nbla;
                const double2 Wm = mant[base + m];
                Wx = Wm.x; Wy = Wm.y; eW = exp2[base + m];
            } else {
                Znn = mant[mn];
                eZnn = exp2[mn];
                if constexpr (DE && F::kHasB) deep_step_xd(Zx, Zy, eZ, dzx, dzy, ed, sm, es, D);
                else if constexpr (DE) deep_step_xd(Zx, Zy, eZ, dzx, dzy, ed, D);
                const double2 n = deep_step_x<F>(Zx, Zy, eZ, dzx, dzy, ed, cx, cy, ec, en);
                nx = n.x; ny = n.y;
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
                if constexpr (DE && F::kRealJacobian) { dzx = __builtin_ldexp(zx, ez); dzy = __builtin_ldexp(zy, ez); }   /* z */
                continue;
            }
            reb = r2 < __builtin_ldexp(nx * nx + ny * ny, 2 * (en - ez)) || m == N;
            ax = reb ? zx : nx; ay = reb ? zy : ny; ea = reb ? ez : en;
            x_norm(ax, ay, ea);
            if (reb) m = 0;
            if constexpr (F::kTwoOrbits) {
                if (ea < kXFlushExp) { ax = 0.0; ay = 0.0; ea = kXZero; }   /* FLUSH */
                if (reb) {                                        /* onto Q and its table, for good */
                    base = 0; N = A.n_ref; K = T.levels; n1 = (uint32_t)(N - 1); tb = 0u;
                }
            }
            if (ea <= kXThr) {                                    /* extended from here */
                dzx = ax; dzy = ay; ed = ea;
                ext = true;
                if (reb) {
                    Zx = 0.0; Zy = 0.0; eZ = kXZero; Znx = z1.x; Zny = z1.y; eZn = e1;
                } else if (k == 0) {
                    Zx = Znx; Zy = Zny; eZ = eZn; Znx = Znn.x; Zny = Znn.y; eZn = eZnn;
                } else {                                          /* m < N here */
                    const double2 b = mant[base + m + 1];
                    Zx = Wx; Zy = Wy; eZ = eW; Znx = b.x; Zny = b.y; eZn = exp2[base + m + 1];
                }
            } else {                                              /* plain from here (m < N) */
                const double2 a = orbit[base + m], b = orbit[base + m + 1];
                dzx = __builtin_ldexp(ax, ea); dzy = __builtin_ldexp(ay, ea);
                ext = false;
                Zx = a.x; Zy = a.y; Znx = b.x; Zny = b.y;
            }
        } else {
            const double2 Znn = orbit[mn];
            if constexpr (DE && F::kHasB) deep_step_pd(Zx, Zy, dzx, dzy, sm, es, D);
            else if constexpr (DE) deep_step_pd(Zx, Zy, dzx, dzy, D);
            const double2 n = deep_step<F>(Zx, Zy, dzx, dzy, cpx, cpy);
            const double nx = n.x, ny = n.y;
            ++m;
            ++u;
            ++nsingle;
            const double zx = Znx + nx, zy = Zny + ny;
            const double r2 = zx * zx + zy * zy;
            if (r2 > B2) {
                esc = u - 1; er2 = r2; live = false;
                if constexpr (DE && F::kRealJacobian) { dzx = zx; dzy = zy; }   /* z, for the gradient of |z| */
                continue;
            }
            reb = r2 < nx * nx + ny * ny || m == N;
            ax = reb ? zx : nx; ay = reb ? zy : ny;
            if (reb) m = 0;
            if constexpr (F::kTwoOrbits) {
                if (reb) { base = 0; N = A.n_ref; K = T.levels; n1 = (uint32_t)(N - 1); tb = 0u; }
            }
            if (!(fmax(fabs(ax), fabs(ay)) < 0x1p-400)) {         /* stays plain */
                dzx = ax; dzy = ay;
                if (reb) {
                    const double2 p1 = orbit[1];
                    Zx = 0.0; Zy = 0.0; Znx = p1.x; Zny = p1.y;
                } else {
                    Zx = Znx; Zy = Zny; Znx = Znn.x; Zny = Znn.y;
                }
            } else {                                              /* turns extended (m < N) */
                const double2 a = mant[base + m], b = mant[base + m + 1];
                x_norm(ax, ay, ea);
                dzx = ax; dzy = ay; ed = ea;
                ext = true;
                Zx = a.x; Zy = a.y; eZ = exp2[base + m]; Znx = b.x; Zny = b.y; eZn = exp2[base + m + 1];
            }
        }
        if (u >= max_iter) live = false;                          /* esc stays max_iter */
    }
    if constexpr (DE && F::kRealJacobian) D.z = make_double2(dzx, dzy);
    if constexpr (DE) *Dout = D;
}

/* ---- the kernel --------------------------------------------------------------------------------------------------------
 * The distance estimate of a sample that escaped with r2 and D (fr_render_deep_de): |z| log|z| / |D|, in pixel spacings since D
 * carries s.  |D| overflowing gives 0 by the division; NaN (D not finite, 0 / 0) becomes 0.  A function of its own, once per
 * escaped sample: inlined, the library log's polynomial coefficients are hoisted out of every loop of the kernel into twelve
 * VGPRs that stay live through the orbit loop (107 and 136 VGPRs, a wave per SIMD less in either kernel, against 94 and 123
 * this way; it uses 21 itself and no stack). */
__device__ __attribute__((noinline)) double deep_de_of(const double r2, const double2 D)
{
    const double dl = sqrt(D.x * D.x + D.y * D.y);
    const double zl = sqrt(r2);
    const double de = (zl * log(zl)) / dl;
    return de != de ? 0.0 : de;
}

/* mandelbrot_debug.comp:196-197 on a sample's linear rgb, the smoothstep's edge in pixel spacings; fp32 */
__device__ __forceinline__ void deep_de_shade(float rgb[3], const double de, const float edge_px)
{
    const float x = fminf(fmaxf((float)de / edge_px, 0.0f), 1.0f);
    const float sm = x * x * (3.0f - 2.0f * x);
    const float t = (1.0f - sm) * 0.3f;
    for (int c = 0; c < 3; ++c) rgb[c] = rgb[c] * (1.0f - t) + (rgb[c] * 0.7f) * t;
}

/* The block's switches name the loop: its formula, extended-exponent deltas, the distance estimate (the derivative and its two
 * planes), BLA (with the step counts).  Two things here are as they are for the instruction streams' sake, which are those of
 * the time when every block was a struct of its own: the body is a function apart from the one __global__ template below (written
 * into it, all twenty kernels are scheduled differently), and Julia's j is read per sample, where the loops are called (read
 * once in front of the walk, Julia's eight kernels differ). */
template <class ARGS>
__device__ __forceinline__ void deep_kernel_body(const ARGS& AA)
{
    using F = typename ARGS::Formula;
    constexpr bool X = ARGS::kX, DE = ARGS::kDe, BLA = ARGS::kBla;
    constexpr int FRACTAL = F::kFractal;
    const DeepArgs& A = AA;
    __shared__ LdsBlock S;
    __shared__ double2 log2_lds[kLog2Entries];
    if (threadIdx.x == 0) S.pal = A.pal;
    if constexpr (F::kLogBailoutLds) {
        if (threadIdx.x == 0) S.log_bailout = AA.log_bailout;
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
    const double resx = (double)W, resy = (double)H;
    double zs = A.zoom;                                           /* extended: the zoom's mantissa, its exponent goes to dc.e */
    if constexpr (X) zs = AA.zm;
    const double2 z1 = A.orbit[1];
    const bool want_rgb = A.rgba != nullptr;
    const bool want_nu = want_rgb || A.nu != nullptr;
    double de_s = 0.0;                                            /* DE: one pixel spacing, wave-uniform; extended: its mantissa */
    int de_es = 0;                                                /* ... and exponent */
    bool de_shade = false;
    if constexpr (DE) {
        if constexpr (X) { de_s = AA.sm; de_es = AA.es; }
        else de_s = AA.s;
        de_shade = want_rgb && AA.shade != 0;
    }

    unsigned long long n_plain = 0ull, n_bla = 0ull, n_upd = 0ull;   /* BLA: this lane's steps and updates */
    int levels_p = 0;                                             /* BLA on two orbits: P's table */
    uint32_t base_p = 0u;
    if constexpr (F::kTwoOrbits && BLA) { levels_p = AA.t.levels_p; base_p = AA.t.base_p; }
    walk_subtiles<3, true>(A.q, A.g, lane, [&](const int px, const int py, const int lrow, const bool inside) {
        float acc[3] = {0.0f, 0.0f, 0.0f};
        double nu0 = 0.0;
        int it0 = 0;
        const int nsamp = aa * aa;
        for (int s = 0; s < nsamp; ++s) {
            int esc;
            double r2;
            const double2 dc = F::dc(px, py, s, aa, resx, resy, zs);
            double cx = inside ? dc.x : 0.0, cy = inside ? dc.y : 0.0;
            uint32_t np = 0u, nb = 0u;
            JuliaStart J = {0, 0};                                /* two orbits: where a sample starts, P */
            if constexpr (F::kTwoOrbits) J = AA.j;
            double2 D = make_double2(0.0, 0.0);
            /* DE, extended: D = (D.x, D.y) 2^eD.  The loop's XDeriv is unpacked into these two so that the planes and
             * deep_de_of(r2, D) below are one code path with the fp64 derivative's, the exponent applied behind them */
            int eD = 0;
            Jac Jm;                                               /* ... and the ship's matrix, its mantissas with X */
            if constexpr (DE && X) {
                int ec = AA.ze;
                x_norm(cx, cy, ec);
                DeepXD<F> Dx;
                if constexpr (BLA)
                    deep_orbit_x_bla<F, true>(A, AA, bla_table(AA), J, levels_p, base_p, cx, cy, ec, inside, esc, r2, np, nb,
                                              de_s, de_es, &Dx);
                else deep_orbit_x<F, true>(A, AA, J, cx, cy, ec, inside, esc, r2, de_s, de_es, &Dx);
                if constexpr (F::kRealJacobian) { Jm.r1 = Dx.r1; Jm.r2 = Dx.r2; Jm.z = Dx.z; }
                else D = make_double2(Dx.x, Dx.y);
                eD = Dx.e;
            } else if constexpr (DE) {
                DeepD<F>* Dp;
                if constexpr (F::kRealJacobian) Dp = &Jm;
                else Dp = &D;
                if constexpr (BLA)
                    deep_orbit_bla<F, true>(A, bla_table(AA), J, levels_p, base_p, cx, cy, z1, inside, esc, r2, np, nb, de_s, Dp);
                else deep_orbit<F, true>(A, J, cx, cy, z1, inside, esc, r2, de_s, Dp);
            } else if constexpr (X) {
                int ec = AA.ze;
                x_norm(cx, cy, ec);
                if constexpr (BLA)
                    deep_orbit_x_bla<F>(A, AA, bla_table(AA), J, levels_p, base_p, cx, cy, ec, inside, esc, r2, np, nb);
                else deep_orbit_x<F>(A, AA, J, cx, cy, ec, inside, esc, r2);
            } else {
                if constexpr (BLA)
                    deep_orbit_bla<F>(A, bla_table(AA), J, levels_p, base_p, cx, cy, z1, inside, esc, r2, np, nb);
                else deep_orbit<F>(A, J, cx, cy, z1, inside, esc, r2);
            }
            if (BLA && inside) {
                n_plain += np; n_bla += nb;
                n_upd += (unsigned long long)(esc < A.max_iter ? esc + 1 : A.max_iter);
            }
            /* DE: the planes of sample (0,0) at once and in front of the colour stage, deriv first: nothing of them stays live
             * through the colour stage or the samples that follow */
            double de = 0.0;
            if constexpr (DE) {
                const bool escaped = esc < A.max_iter;            /* interior: 0 and (0, 0) */
                const bool first = s == 0 && inside;
                if constexpr (F::kRealJacobian) {                 /* four doubles: (J11, J12, J21, J22) */
                    if (first && AA.deriv) {
                        double* const dst = AA.deriv + 4 * plane_index(A.g, px, py, lrow);
                        const double j[4] = {Jm.r1.x, Jm.r1.y, Jm.r2.x, Jm.r2.y};
                        for (int c = 0; c < 4; ++c) {
                            if constexpr (X) dst[c] = escaped ? __builtin_ldexp(j[c], eD) : 0.0;
                            else dst[c] = escaped ? j[c] : 0.0;
                        }
                    }
                    /* the gradient of |z| with respect to c, J^T z / |z|: the D of deep_de_of */
                    if (escaped && (s == 0 || de_shade)) {
                        const double zl = sqrt(r2);
                        const double ux = Jm.z.x / zl, uy = Jm.z.y / zl;
                        D = make_double2(Jm.r1.x * ux + Jm.r2.x * uy, Jm.r1.y * ux + Jm.r2.y * uy);
                    }
                } else if (first && AA.deriv) {
                    double* const dst = AA.deriv + 2 * plane_index(A.g, px, py, lrow);
                    if constexpr (X) {                            /* saturates outside a double's range */
                        dst[0] = escaped ? __builtin_ldexp(D.x, eD) : 0.0; dst[1] = escaped ? __builtin_ldexp(D.y, eD) : 0.0;
                    } else {
                        dst[0] = escaped ? D.x : 0.0; dst[1] = escaped ? D.y : 0.0;
                    }
                }
                if (escaped && (s == 0 || de_shade)) {
                    de = deep_de_of(r2, D);                       /* extended: of the mantissas, so |D| cannot overflow */
                    if constexpr (X) de = __builtin_ldexp(de, -eD);
                }
                if (first && AA.de) AA.de[plane_index(A.g, px, py, lrow)] = de;
            }
            double nu;
            float rgb[3];
            shade<double, FRACTAL>(A, S, lg, esc, r2, want_nu, want_rgb, nu, rgb);
            if (s == 0) { nu0 = nu; it0 = esc; }
            if constexpr (DE) {
                if (de_shade && esc < A.max_iter) deep_de_shade(rgb, de, AA.edge_px);
            }
            acc[0] += rgb[0]; acc[1] += rgb[1]; acc[2] += rgb[2];
        }
        if (aa > 1) {
            const float n = (float)(aa * aa);
            acc[0] /= n; acc[1] /= n; acc[2] /= n;
        }
        if (want_rgb && (A.flags & FR_FLAG_POST_CHAIN)) post_chain(acc, A.brightness, A.saturation, A.contrast, FRACTAL != 0);
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
            if (lane == 0) atomicAdd(bla_table(AA).steps + c, v[c]);
        }
    }
}

template <class ARGS>
__global__ void __launch_bounds__(kBlockThreads)
deep_kernel(const ARGS AA)
{
    deep_kernel_body(AA);
}

/* The four kernels of the ship's distance estimate, DeepBlock<ShipFormula, X, true, BLA>: the same body under a __global__
 * template of their own (kShipDe picks it in the launch) */
template <class ARGS>
__global__ void __launch_bounds__(kBlockThreads)
deep_ship_de_kernel(const ARGS AA)
{
    deep_kernel_body(AA);
}

}  // namespace fr
