/*
 * fr_deep.c -- host side of the deep Mandelbrot views (fr_render_deep, include/fractalrenderer_amd.h): the decimal
 * parser, the fixed-point reference orbit and the validation of a deep view.  Plain C11 with unsigned __int128 products.
 *
 * Fixed point: a value v is the integer X = v 2^F in L = ceil(F / 64) + 1 limbs of 64 bits, little-endian two's
 * complement -- F fraction bits and at least 64 integer bits.  Centres are limited to |c| < 2^32, so an orbit point that
 * has not escaped (|Z|^2 <= bailout^2 <= 2^32) is below 2^16, the escaping one below 2^33, and the squares of the escape
 * test (< 2^(2F + 66)) fit in the 2L limbs of a product.
 *
 * Extended views (fr_render_deepx): the zoom string becomes (zm, ze) through the same parser (its truncated integer, the
 * inexact flag of its divisions, one rounding to 53 bits), and the orbit is stored as doubles plus a side array of
 * exponents -- 0 for every point a normal double holds, so those points are the doubles of fr_deep_reference_orbit and the
 * kernel's plain mode loads 16 bytes per point; only a point below 2^-1022 carries mantissas and a non-zero exponent.
 *
 * Deep Burning Ship views (fr_render_deep_ship): the same loop with Im = floor(2 |Zr| |Zi| / 2^F) + Ci (orbit_formula), and
 * fr_deep_validate's rules for FR_FRACTAL_BURNING_SHIP (fr_deep_ship_validate).
 *
 * Extended Burning Ship views (fr_render_deepx_ship): the ship's recurrence through the extended storage, and the ship's
 * rules with the zoom taken from the view's string (fr_deepx_ship_validate).
 *
 * Deep Julia views (fr_render_deep_julia, fr_render_deepx_julia): Mandelbrot's recurrence with c from a pair of doubles, twice --
 * from the view's centre (orbit_loop's start point) and from 0 -- in either storage, and the two validators.
 *
 * The six paths share one host side: what their validators ask is a row of kRules read by validate_params, either view struct
 * goes through resolve_view, and the six reference-orbit entry points start with orbit_request.
 *
 * Deep Phoenix views (fr_render_deep_phoenix): a second-order recurrence, Z' = Z^2 + C + r Z_prev + p Z, as one more formula of
 * the same loop (kOrbitPhoenix: two products more per component and the previous point kept), p and r from floats
 * (phoenix_terms); its validator stands apart from kRules, since it reads fr_phoenix_params and Phoenix's own field rules
 * (fr_phoenix_validate), and goes through resolve_view like the others.  |p|, |r| < 2^32 keeps the escaping point below 2^36.
 */
#include "fr_internal.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

enum {
    kMaxChars = 4096,                          /* longest centre string */
    kMaxFracBits = 4096,
    kMaxLimbs = kMaxFracBits / 64 + 1,         /* L at F = 4096 */
    /* the parser's working integer: up to 4096 decimal digits (13607 bits) shifted left by F (4096) */
    kWorkLimbs = 280
};

typedef struct { int F, L; } fx_fmt;

/* ---- multi-limb magnitudes ---------------------------------------------------------------------------------------- */
static int top_limb(const uint64_t* a, int n)             /* index of the highest non-zero limb, -1 for zero */
{
    for (int i = n - 1; i >= 0; --i)
        if (a[i]) return i;
    return -1;
}

static void shl_bits(uint64_t* a, int n, int s)           /* a <<= s in n limbs (bits shifted out are lost) */
{
    const int w = s / 64, b = s % 64;
    for (int i = n - 1; i >= 0; --i) {
        uint64_t v = 0;
        if (i - w >= 0) {
            v = a[i - w] << b;
            if (b && i - w - 1 >= 0) v |= a[i - w - 1] >> (64 - b);
        }
        a[i] = v;
    }
}

/* r = a >> s (r has rn limbs, a has an limbs); returns 1 when a bit shifted out was set */
static int shr_bits(uint64_t* r, int rn, const uint64_t* a, int an, int s)
{
    const int w = s / 64, b = s % 64;
    int lost = 0;
    for (int i = 0; i < w && i < an; ++i) lost |= a[i] != 0;
    if (b && w < an) lost |= (a[w] & ((1ull << b) - 1)) != 0;
    for (int i = 0; i < rn; ++i) {
        uint64_t v = 0;
        if (i + w < an) {
            v = a[i + w] >> b;
            if (b && i + w + 1 < an) v |= a[i + w + 1] << (64 - b);
        }
        r[i] = v;
    }
    return lost;
}

static int bit_of(const uint64_t* a, int n, long k)      /* bit k of a, 0 outside */
{
    if (k < 0 || k >= 64L * n) return 0;
    return (int)((a[k / 64] >> (k % 64)) & 1u);
}

static int any_below(const uint64_t* a, int n, long k)    /* some bit below bit k of a is set */
{
    for (long i = 0; i < n && 64 * i < k; ++i) {
        const long lo = 64 * i;
        const uint64_t m = k - lo >= 64 ? ~0ull : ((1ull << (k - lo)) - 1);
        if (a[i] & m) return 1;
    }
    return 0;
}

static void add_one(uint64_t* a, int n)
{
    for (int i = 0; i < n; ++i)
        if (++a[i] != 0) return;
}

static void negate(uint64_t* a, int n)                    /* two's complement */
{
    for (int i = 0; i < n; ++i) a[i] = ~a[i];
    add_one(a, n);
}

static int is_negative(const uint64_t* a, int n) { return (int)(a[n - 1] >> 63); }

/* r = a + b (n limbs, modular) */
static void add_n(uint64_t* r, const uint64_t* a, const uint64_t* b, int n)
{
    unsigned __int128 c = 0;
    for (int i = 0; i < n; ++i) {
        c += (unsigned __int128)a[i] + b[i];
        r[i] = (uint64_t)c;
        c >>= 64;
    }
}

/* r = a - b (n limbs, modular) */
static void sub_n(uint64_t* r, const uint64_t* a, const uint64_t* b, int n)
{
    uint64_t borrow = 0;
    for (int i = 0; i < n; ++i) {
        const uint64_t ai = a[i], bi = b[i];
        const uint64_t d = ai - bi - borrow;
        borrow = (ai < bi) || (ai - bi < borrow);
        r[i] = d;
    }
}

static int cmp_n(const uint64_t* a, const uint64_t* b, int n)   /* unsigned compare */
{
    for (int i = n - 1; i >= 0; --i)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}

/* r[0 .. 2n) = a * b, magnitudes of n limbs */
static void mul_mag(uint64_t* r, const uint64_t* a, const uint64_t* b, int n)
{
    memset(r, 0, sizeof(uint64_t) * 2 * (size_t)n);
    const int ta = top_limb(a, n), tb = top_limb(b, n);
    for (int i = 0; i <= ta; ++i) {
        unsigned __int128 c = 0;
        const uint64_t ai = a[i];
        if (!ai) continue;
        for (int j = 0; j <= tb; ++j) {
            c += (unsigned __int128)ai * b[j] + r[i + j];
            r[i + j] = (uint64_t)c;
            c >>= 64;
        }
        for (int k = i + tb + 1; c; ++k) {
            c += r[k];
            r[k] = (uint64_t)c;
            c >>= 64;
        }
    }
}

static uint64_t mul_small(uint64_t* a, int n, uint64_t m)      /* a *= m; returns the carry out */
{
    unsigned __int128 c = 0;
    for (int i = 0; i < n; ++i) {
        c += (unsigned __int128)a[i] * m;
        a[i] = (uint64_t)c;
        c >>= 64;
    }
    return (uint64_t)c;
}

static void add_small(uint64_t* a, int n, uint64_t v)          /* a += v */
{
    for (int i = 0; i < n && v; ++i) {
        a[i] += v;
        v = a[i] < v;
    }
}

static uint64_t div_small(uint64_t* a, int n, uint64_t d)      /* a /= d (floor); returns the remainder */
{
    unsigned __int128 rem = 0;
    for (int i = n - 1; i >= 0; --i) {
        const unsigned __int128 cur = (rem << 64) | a[i];
        a[i] = (uint64_t)(cur / d);
        rem = cur % d;
    }
    return (uint64_t)rem;
}

/* ---- decimal parser -------------------------------------------------------------------------------------------------
 * [+-]digits[.digits][(e|E)[+-]digits] -> round_half_even(value 2^F) in fmt.L limbs.  The digits are built into one big
 * integer D (value = D 10^net), shifted left by F, then multiplied by 10 (net > 0) or divided by 10 once per digit of
 * the negative exponent; the last division's remainder and a sticky bit of the earlier ones round to nearest, ties to
 * even.  Returns 0, or -1 for a malformed string, -2 for |value| >= 2^32. */
/* The scan and the scaling of both parsers: A = floor(|value| 2^F) in kWorkLimbs limbs, *neg the sign, *rem the remainder
 * of the last division by 10 and *sticky whether an earlier one left any (both 0 when no division took place).  Returns 0;
 * 1 for a value that is zero or far below 2^-F (A is not set); -1 for a malformed string; -2 for |value| >= 2^32. */
static int parse_scaled(const char* s, int F, uint64_t* A, int* neg_out, uint64_t* rem, int* sticky_out)
{
    size_t len = 0;
    while (len <= (size_t)kMaxChars && s[len]) ++len;
    if (len == 0 || len > (size_t)kMaxChars) return -1;
    size_t i = 0;
    int neg = 0;
    if (s[i] == '+' || s[i] == '-') neg = s[i++] == '-';
    memset(A, 0, sizeof(uint64_t) * kWorkLimbs);
    long ndig = 0, nfrac = 0;
    for (; s[i] >= '0' && s[i] <= '9'; ++i, ++ndig) {
        mul_small(A, kWorkLimbs, 10);
        add_small(A, kWorkLimbs, (uint64_t)(s[i] - '0'));
    }
    if (ndig == 0) return -1;
    if (s[i] == '.') {
        ++i;
        for (; s[i] >= '0' && s[i] <= '9'; ++i, ++nfrac) {
            mul_small(A, kWorkLimbs, 10);
            add_small(A, kWorkLimbs, (uint64_t)(s[i] - '0'));
        }
        if (nfrac == 0) return -1;
    }
    long ex = 0;
    if (s[i] == 'e' || s[i] == 'E') {
        ++i;
        int eneg = 0;
        if (s[i] == '+' || s[i] == '-') eneg = s[i++] == '-';
        long nex = 0;
        for (; s[i] >= '0' && s[i] <= '9'; ++i, ++nex)
            if (ex < 1000000) ex = ex * 10 + (s[i] - '0');      /* saturates: anything past it is 0 or too large */
        if (nex == 0) return -1;
        if (eneg) ex = -ex;
    }
    if (s[i] != '\0') return -1;

    *neg_out = neg; *rem = 0; *sticky_out = 0;
    if (top_limb(A, kWorkLimbs) < 0) return 1;                   /* zero, whatever its sign */
    const long net = ex - nfrac;
    if (net >= 0) {
        if (net > 10) return -2;                                 /* D >= 1: >= 1e11 > 2^32 */
        for (long k = 0; k < net; ++k) mul_small(A, kWorkLimbs, 10);
        if (top_limb(A, kWorkLimbs) > 0 || A[0] >= (1ull << 32)) return -2;
        shl_bits(A, kWorkLimbs, F);
    } else {
        const long k = -net;
        /* D < 10^4096 and 2^F <= 2^4096 < 10^1234: past 10^5331 the value is below 1/2 and rounds to 0 */
        if (k > 5400) return 1;
        shl_bits(A, kWorkLimbs, F);
        int n = top_limb(A, kWorkLimbs) + 1, sticky = 0;
        for (long d = 0; d + 1 < k; ++d) {
            sticky |= div_small(A, n, 10) != 0;
            while (n > 1 && A[n - 1] == 0) --n;
        }
        *rem = div_small(A, n, 10);
        *sticky_out = sticky;
    }
    return 0;
}

static int parse_fixed(const char* s, fx_fmt fmt, uint64_t* out)
{
    uint64_t A[kWorkLimbs];
    int neg = 0, sticky = 0;
    uint64_t r = 0;
    const int st = parse_scaled(s, fmt.F, A, &neg, &r, &sticky);
    if (st == -1) return -1;
    memset(out, 0, sizeof(uint64_t) * (size_t)fmt.L);
    if (st != 0) return st == 1 ? 0 : st;
    if (r > 5 || (r == 5 && (sticky || (A[0] & 1u)))) add_one(A, kWorkLimbs);   /* the last digit decides the rounding */
    const long lim = (long)fmt.F + 32;                           /* |X| < 2^(F + 32) */
    for (int j = 0; j < kWorkLimbs; ++j) {
        const long lo = 64L * j;
        if (lo + 64 <= lim) continue;
        const uint64_t m = lo >= lim ? ~0ull : ~((1ull << (lim - lo)) - 1);
        if (A[j] & m) return -2;
    }
    memcpy(out, A, sizeof(uint64_t) * (size_t)fmt.L);
    if (neg) negate(out, fmt.L);
    return 0;
}

/* ---- fixed point -> double --------------------------------------------------------------------------------------------
 * X 2^-F rounded to nearest, ties to even, subnormals included (what float(Fraction(X, 2**F)) is): the top p bits of |X|,
 * p = 53 or fewer where the result is subnormal, the next bit and a sticky bit below it. */
static double fixed_to_double(const uint64_t* x, fx_fmt fmt)
{
    uint64_t m[kMaxLimbs];
    memcpy(m, x, sizeof(uint64_t) * (size_t)fmt.L);
    const int neg = is_negative(m, fmt.L);
    if (neg) negate(m, fmt.L);
    const int t = top_limb(m, fmt.L);
    if (t < 0) return 0.0;
    const long b = 64L * t + 63 - __builtin_clzll(m[t]);        /* highest set bit */
    const long e = b - fmt.F;                                     /* 2^e <= |v| < 2^(e+1) */
    long p = 53;
    if (e < -1022) p = 53 - (-1022 - e);
    const long shift = b + 1 - p;                                 /* bits below the kept ones */
    double r;
    if (shift <= 0) {
        r = ldexp((double)m[0], -fmt.F);                          /* b < p <= 53: exact */
    } else {
        uint64_t v = 0;
        for (long k = 0; k < 64 && k < p; ++k) v |= (uint64_t)bit_of(m, fmt.L, shift + k) << k;
        const int half = bit_of(m, fmt.L, shift - 1), sticky = any_below(m, fmt.L, shift - 1);
        if (half && (sticky || (v & 1u))) ++v;
        r = ldexp((double)v, (int)(shift - fmt.F));
    }
    return neg ? -r : r;
}

/* ---- the reference orbit ------------------------------------------------------------------------------------------------ */

/* floor(sign * P / 2^s) into r (L limbs, two's complement); P a 2L-limb magnitude */
static void floor_shift(uint64_t* r, const uint64_t* P, int s, int negative, fx_fmt fmt)
{
    const int lost = shr_bits(r, fmt.L, P, 2 * fmt.L, s);
    if (negative) {
        if (lost) add_one(r, fmt.L);
        negate(r, fmt.L);
    }
}

/* Extended storage of one orbit point (fr_deepx_reference_orbit): (mx, my) 2^e.  A point whose larger component is a
 * normal double keeps e = 0 and the doubles fixed_to_double gives; a smaller one gets e = the exponent that puts its larger
 * mantissa into [0.5, 1), each mantissa rounded once from the fixed-point value; zero gets FR_DEEPX_ZERO_EXP. */
static void store_extended(const uint64_t* zr, const uint64_t* zi, fx_fmt fmt, double* mxy, int32_t* e)
{
    long top = -1;
    const uint64_t* z[2] = {zr, zi};
    for (int k = 0; k < 2; ++k) {
        uint64_t m[kMaxLimbs];
        memcpy(m, z[k], sizeof(uint64_t) * (size_t)fmt.L);
        if (is_negative(m, fmt.L)) negate(m, fmt.L);
        const int t = top_limb(m, fmt.L);
        if (t < 0) continue;
        const long b = 64L * t + 63 - __builtin_clzll(m[t]);
        if (b > top) top = b;
    }
    if (top < 0) { mxy[0] = 0.0; mxy[1] = 0.0; *e = FR_DEEPX_ZERO_EXP; return; }
    const long b = top - fmt.F;                                   /* 2^b <= larger component < 2^(b + 1) */
    fx_fmt f = fmt;
    *e = 0;
    if (b < -1022) { *e = (int32_t)(b + 1); f.F = fmt.F + (int)(b + 1); }
    mxy[0] = fixed_to_double(zr, f);
    mxy[1] = fixed_to_double(zi, f);
}

/* The recurrence: kOrbitMandelbrot Z^2 + C; kOrbitShip (|Zr| + i |Zi|)^2 + C, whose imaginary product is never negative
 * (fr_render_deep_ship). */
typedef enum { kOrbitMandelbrot = 0, kOrbitShip = 1, kOrbitPhoenix = 2 } orbit_formula;

/* kOrbitPhoenix: Z' = Z^2 + C + r Q + p Z with Q the point before Z (fr_render_deep_phoenix); P = floor(p 2^F), R = floor(r 2^F) */
typedef struct { uint64_t p[kMaxLimbs], r[kMaxLimbs]; } phoenix_terms;

/* acc += floor(a b / 2^F): a, b and acc signed values of L limbs */
static void add_mul_floor(uint64_t* acc, const uint64_t* a, const uint64_t* b, fx_fmt fmt)
{
    uint64_t ma[kMaxLimbs], mb[kMaxLimbs], pr[2 * kMaxLimbs], t[kMaxLimbs];
    memcpy(ma, a, sizeof(uint64_t) * (size_t)fmt.L);
    memcpy(mb, b, sizeof(uint64_t) * (size_t)fmt.L);
    const int na = is_negative(ma, fmt.L), nb = is_negative(mb, fmt.L);
    if (na) negate(ma, fmt.L);
    if (nb) negate(mb, fmt.L);
    mul_mag(pr, ma, mb, fmt.L);
    floor_shift(t, pr, fmt.F, na != nb, fmt);
    add_n(acc, acc, t, fmt.L);
}

/* T = floor(bailout^2 2^(2F)) in 2L + 1 limbs: |Z|^2 2^(2F) = Zr^2 + Zi^2 is an integer, so "> bailout^2" is "> T" exactly */
static void bailout_threshold(uint64_t* T, fx_fmt fmt, float bailout)
{
    const int L2 = 2 * fmt.L;
    memset(T, 0, sizeof(uint64_t) * (size_t)(L2 + 1));
    const double b2 = (double)bailout * (double)bailout;          /* exact: a float squared */
    int ex = 0;
    const double mant = frexp(b2, &ex);
    const uint64_t mi = (uint64_t)ldexp(mant, 53);
    const long ts = (long)ex - 53 + 2L * fmt.F;
    T[0] = mi;
    if (ts >= 0) shl_bits(T, L2 + 1, (int)ts);
    else T[0] = -ts >= 64 ? 0 : mi >> -ts;
}

/* out_exp NULL: Z_n as doubles; else the extended storage.  (sr0, si0) the orbit's first point, NULL for 0 (the Julia views'
 * primary orbit starts at the view's centre, fr_render_deep_julia).  ph: kOrbitPhoenix's P and R, NULL for the other formulas. */
static int orbit_loop(const uint64_t* cr, const uint64_t* ci, const uint64_t* sr0, const uint64_t* si0, fx_fmt fmt,
                      orbit_formula formula, const phoenix_terms* ph, int32_t max_iter, float bailout, double* out_xy,
                      int32_t* out_exp, int32_t* out_len)
{
    const int L = fmt.L, L2 = 2 * fmt.L;
    uint64_t zr[kMaxLimbs], zi[kMaxLimbs], ar[kMaxLimbs], ai[kMaxLimbs], t0[kMaxLimbs], t1[kMaxLimbs];
    uint64_t qr[kMaxLimbs], qi[kMaxLimbs], wr[kMaxLimbs], wi[kMaxLimbs];   /* Phoenix: Z_{n-1}, and Z_n while Z_{n+1} is formed */
    memset(qr, 0, sizeof qr); memset(qi, 0, sizeof qi);
    uint64_t sr[2 * kMaxLimbs + 1], si[2 * kMaxLimbs + 1], pr[2 * kMaxLimbs], ssum[2 * kMaxLimbs + 1], T[2 * kMaxLimbs + 1];
    memset(zr, 0, sizeof zr); memset(zi, 0, sizeof zi);
    memset(sr, 0, sizeof sr); memset(si, 0, sizeof si);
    bailout_threshold(T, fmt, bailout);

    out_xy[0] = 0.0; out_xy[1] = 0.0;
    if (out_exp) out_exp[0] = FR_DEEPX_ZERO_EXP;
    if (sr0 && si0) {
        memcpy(zr, sr0, sizeof(uint64_t) * (size_t)L);
        memcpy(zi, si0, sizeof(uint64_t) * (size_t)L);
        if (out_exp) {
            store_extended(zr, zi, fmt, out_xy, out_exp);
        } else {
            out_xy[0] = fixed_to_double(zr, fmt);
            out_xy[1] = fixed_to_double(zi, fmt);
        }
    }
    int32_t n = 0;
    for (;; ++n) {
        if (n == max_iter) break;
        /* magnitudes of Zr, Zi */
        memcpy(ar, zr, sizeof(uint64_t) * (size_t)L);
        memcpy(ai, zi, sizeof(uint64_t) * (size_t)L);
        const int nr = is_negative(ar, L), ni = is_negative(ai, L);
        if (nr) negate(ar, L);
        if (ni) negate(ai, L);
        mul_mag(sr, ar, ar, L);
        mul_mag(si, ai, ai, L);
        sr[L2] = si[L2] = 0;
        add_n(ssum, sr, si, L2 + 1);
        if (cmp_n(ssum, T, L2 + 1) > 0) break;                     /* |Z_n|^2 > bailout^2 */
        mul_mag(pr, ar, ai, L);
        if (formula == kOrbitPhoenix) {
            memcpy(wr, zr, sizeof(uint64_t) * (size_t)L);
            memcpy(wi, zi, sizeof(uint64_t) * (size_t)L);
        }
        /* Re = floor(Zr^2 / 2^F) - floor(Zi^2 / 2^F) + Cr,  Im = floor(2 Zr Zi / 2^F) + Ci (the ship: 2 |Zr| |Zi|) */
        floor_shift(t0, sr, fmt.F, 0, fmt);
        floor_shift(t1, si, fmt.F, 0, fmt);
        sub_n(zr, t0, t1, L);
        add_n(zr, zr, cr, L);
        floor_shift(t0, pr, fmt.F - 1, formula == kOrbitShip ? 0 : nr != ni, fmt);
        add_n(zi, t0, ci, L);
        if (formula == kOrbitPhoenix) {     /* ... + floor(R Q / 2^F) + floor(P Z / 2^F) per component, then Q = Z_n */
            add_mul_floor(zr, ph->r, qr, fmt);
            add_mul_floor(zr, ph->p, wr, fmt);
            add_mul_floor(zi, ph->r, qi, fmt);
            add_mul_floor(zi, ph->p, wi, fmt);
            memcpy(qr, wr, sizeof(uint64_t) * (size_t)L);
            memcpy(qi, wi, sizeof(uint64_t) * (size_t)L);
        }
        if (out_exp) {
            store_extended(zr, zi, fmt, out_xy + 2 * (n + 1), out_exp + n + 1);
        } else {
            out_xy[2 * (n + 1)] = fixed_to_double(zr, fmt);
            out_xy[2 * (n + 1) + 1] = fixed_to_double(zi, fmt);
        }
    }
    *out_len = n + 1;
    return FR_OK;
}

/* ---- public entry points ------------------------------------------------------------------------------------------------ */

int fr_deep_view_default(fr_deep_view* v)
{
    if (!v) return fr_set_error(FR_ERR_INVALID_ARG, "deep view is NULL");
    v->center_x = "-0.5";
    v->center_y = "0";
    v->frac_bits = 0;
    v->reserved = 0;
    return FR_OK;
}

int fr_deepx_view_default(fr_deepx_view* v)
{
    if (!v) return fr_set_error(FR_ERR_INVALID_ARG, "deep view is NULL");
    v->center_x = "-0.5";
    v->center_y = "0";
    v->zoom = "3";
    v->frac_bits = 0;
    v->reserved = 0;
    return FR_OK;
}

int fr_deep_frac_bits(double zoom)
{
    if (!isfinite(zoom) || !(zoom > 0.0))
        return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_frac_bits: zoom must be finite and > 0");
    double want = 64.0 + (double)(int)(-log10(zoom) * 3.32) + 64.0;   /* src/deep_zoom_system.cpp:209-260 */
    if (want < 128.0) want = 128.0;
    if (want > (double)kMaxFracBits) want = kMaxFracBits;
    const int bits = (int)want;
    return (bits + 63) / 64 * 64;
}

static int check_zoom(double zoom)
{
    if (!isfinite(zoom) || !(zoom >= 1e-290) || !(zoom <= 1e3))
        return fr_set_error(FR_ERR_INVALID_ARG, "deep zoom %g outside [1e-290, 1e3]", zoom);
    return FR_OK;
}

static int check_bailout(float bailout)
{
    if (!isfinite(bailout) || !(bailout > 0.0f) || !(bailout <= 65536.0f))
        return fr_set_error(FR_ERR_INVALID_ARG, "deep bailout must be finite, > 0 and <= 2^16");
    return FR_OK;
}

static int check_julia_c(double c_re, double c_im)
{
    if (!isfinite(c_re) || !isfinite(c_im) || !(fabs(c_re) < 4294967296.0) || !(fabs(c_im) < 4294967296.0))
        return fr_set_error(FR_ERR_INVALID_ARG, "deep Julia views need a finite c with |c_re|, |c_im| < 2^32");
    return FR_OK;
}

/* both centre strings in fixed point; FR_OK or FR_ERR_INVALID_ARG */
static int parse_centre(const char* center_x, const char* center_y, fx_fmt fmt, uint64_t* cr, uint64_t* ci)
{
    const char* which[2] = {"center_x", "center_y"};
    const char* str[2] = {center_x, center_y};
    uint64_t* dst[2] = {cr, ci};
    for (int k = 0; k < 2; ++k) {
        const int st = parse_fixed(str[k], fmt, dst[k]);
        if (st == -1)
            return fr_set_error(FR_ERR_INVALID_ARG, "deep view %s is not [+-]digits[.digits][(e|E)[+-]digits] of at most 4096 "
                                "characters", which[k]);
        if (st == -2) return fr_set_error(FR_ERR_INVALID_ARG, "deep view %s: |centre| must be < 2^32", which[k]);
    }
    return FR_OK;
}

int fr_deepx_check_centre(const char* center_x, const char* center_y, int32_t frac_bits)
{
    uint64_t cr[kMaxLimbs], ci[kMaxLimbs];
    const fx_fmt fmt = {frac_bits, (frac_bits + 63) / 64 + 1};
    return parse_centre(center_x, center_y, fmt, cr, ci);
}

int fr_deep_parse_fixed(const char* s, int32_t frac_bits, uint64_t* out, int32_t nlimbs)
{
    if (!s || !out) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_parse_fixed: NULL argument");
    if (frac_bits < 128 || frac_bits > kMaxFracBits)
        return fr_set_error(FR_ERR_INVALID_ARG, "frac_bits %d outside [128, 4096]", frac_bits);
    const fx_fmt fmt = {frac_bits, (frac_bits + 63) / 64 + 1};
    if (nlimbs < fmt.L) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_parse_fixed: %d limbs, %d needed", nlimbs, fmt.L);
    uint64_t x[kMaxLimbs], unused[kMaxLimbs];
    const int st = parse_centre(s, "0", fmt, x, unused);
    if (st != FR_OK) return st;
    memcpy(out, x, sizeof(uint64_t) * (size_t)fmt.L);
    return fmt.L;
}

/* ---- the zoom of an extended view ---------------------------------------------------------------------------------------------
 * The zoom is a decimal string: parsed like a centre into floor(value 2^kZoomBits) with the inexact flag of the divisions,
 * its top 53 bits rounded to nearest, ties to even -- one rounding from the decimal value. */
enum { kZoomBits = 3520 };                    /* 1e-1000 2^3520 is about 2^198: far more than 54 bits */

static int zoom_pair(const char* s, double* zm, int32_t* ze)
{
    if (!s) return fr_set_error(FR_ERR_INVALID_ARG, "deep zoom string is NULL");
    uint64_t A[kWorkLimbs];
    int neg = 0, sticky = 0;
    uint64_t rem = 0;
    const int st = parse_scaled(s, kZoomBits, A, &neg, &rem, &sticky);
    if (st == -1)
        return fr_set_error(FR_ERR_INVALID_ARG, "deep zoom is not [+-]digits[.digits][(e|E)[+-]digits] of at most 4096 characters");
    const int t = st == 0 ? top_limb(A, kWorkLimbs) : -1;
    const long b = t < 0 ? -1 : 64L * t + 63 - __builtin_clzll(A[t]);
    if (st != 0 || neg || b < 64) return fr_set_error(FR_ERR_INVALID_ARG, "deep zoom outside [1e-1000, 1e3]");
    uint64_t v = 0;
    for (int k = 0; k < 53; ++k) v |= (uint64_t)bit_of(A, kWorkLimbs, b - 52 + k) << k;
    const int half = bit_of(A, kWorkLimbs, b - 53);
    const int below = any_below(A, kWorkLimbs, b - 53) || rem != 0 || sticky;
    if (half && (below || (v & 1u))) ++v;
    long e = b - kZoomBits;
    if (v == (1ull << 53)) { v >>= 1; ++e; }
    const double m = ldexp((double)v, -52);
    /* the range, on the rounded pair: 1e-1000 = 1.0511037747648835 2^-3322, 1e3 = 1.953125 2^9 */
    if (e < -3322 || (e == -3322 && m < 1.0511037747648835) || e > 9 || (e == 9 && m > 1.953125))
        return fr_set_error(FR_ERR_INVALID_ARG, "deep zoom outside [1e-1000, 1e3]");
    *zm = m;
    *ze = (int32_t)e;
    return FR_OK;
}

int fr_deepx_zoom(const char* zoom, double* mant, int32_t* exp2)
{
    if (!mant || !exp2) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deepx_zoom: out is NULL");
    return zoom_pair(zoom, mant, exp2);
}

int fr_deepx_frac_bits_pair(double zm, int32_t ze)
{
    if (ze >= -1000) {
        const double z = ldexp(zm, ze);                          /* exact: a normal double */
        if (z >= 1e-290) return fr_deep_frac_bits(z);
    }
    double want = 64.0 + (double)(int)(-(log10(zm) + (double)ze * log10(2.0)) * 3.32) + 64.0;
    if (want < 128.0) want = 128.0;
    if (want > (double)kMaxFracBits) want = kMaxFracBits;
    const int bits = (int)want;
    return (bits + 63) / 64 * 64;
}

int fr_deepx_frac_bits(const char* zoom)
{
    double zm;
    int32_t ze;
    const int st = zoom_pair(zoom, &zm, &ze);
    return st != FR_OK ? st : fr_deepx_frac_bits_pair(zm, ze);
}

/* ---- a view resolved --------------------------------------------------------------------------------------------------------
 * Either view struct (v: the zoom is the caller's double; x: the view's string) checked in one order -- reserved, frac_bits, the
 * centre strings, the zoom string -- and turned into the fixed-point format, the zoom pair (v: (zoom, 0)) and, with `centre`,
 * both centre strings parsed.  Every validator and every reference orbit goes through here. */
typedef struct {
    fx_fmt fmt;
    uint64_t cr[kMaxLimbs], ci[kMaxLimbs];
    double zm;
    int32_t ze;
} deep_resolved;

static int resolve_view(const fr_deep_view* v, const fr_deepx_view* x, double zoom, int centre, deep_resolved* r)
{
    if (!v && !x) return fr_set_error(FR_ERR_INVALID_ARG, "deep view is NULL");
    const char* cx = x ? x->center_x : v->center_x;
    const char* cy = x ? x->center_y : v->center_y;
    const int32_t bits = x ? x->frac_bits : v->frac_bits;
    if ((x ? x->reserved : v->reserved) != 0)
        return fr_set_error(FR_ERR_INVALID_ARG, "%s.reserved must be 0", x ? "fr_deepx_view" : "fr_deep_view");
    if (bits != 0 && (bits < 128 || bits > kMaxFracBits))
        return fr_set_error(FR_ERR_INVALID_ARG, "frac_bits %d outside {0} U [128, 4096]", bits);
    if (!cx || !cy) return fr_set_error(FR_ERR_INVALID_ARG, "deep view centre string is NULL");
    r->zm = zoom;
    r->ze = 0;
    int st;
    if (x && (st = zoom_pair(x->zoom, &r->zm, &r->ze)) != FR_OK) return st;
    const int F = bits ? bits : x ? fr_deepx_frac_bits_pair(r->zm, r->ze) : fr_deep_frac_bits(zoom);
    if (F < 0) return F;
    r->fmt.F = F;
    r->fmt.L = (F + 63) / 64 + 1;
    return centre ? parse_centre(cx, cy, r->fmt, r->cr, r->ci) : FR_OK;
}

int fr_deepx_resolve(const fr_deepx_view* v, double* zm, int32_t* ze, int32_t* frac_bits)
{
    deep_resolved r;
    const int st = resolve_view(NULL, v, 0.0, 0, &r);
    if (st != FR_OK) return st;
    *zm = r.zm;
    *ze = r.ze;
    *frac_bits = r.fmt.F;
    return FR_OK;
}

/* ---- the rules of the six paths -----------------------------------------------------------------------------------------------
 * What differs between the validators: one row per (formula, storage).  validate_params checks in this order: the fractal
 * type, the precision, fr_params_validate (the double centre, and the zoom where the view's string carries it, not read), the
 * zoom, the bailout, Julia's c, the whole-orbit rule, the foreign BLA flags. */
typedef enum { kWholeNone = 0, kWholeMandel, kWholeShip } whole_orbit_rule;

typedef struct {
    const char* who;                 /* the entry point, as the messages name it */
    int32_t fractal;
    const char* fractal_name;
    int zoom_in_params;              /* the zoom is p->zoom; else the view's string */
    int julia;                       /* c is checked, and the centre has to lie inside the bailout radius */
    whole_orbit_rule whole;          /* which colourings need the whole orbit: Mandelbrot's list, the ship's, none */
    struct { uint32_t mask; const char* msg; } foreign[2];   /* BLA flags of other paths, in the order they are refused */
} deep_rules;

#define JULIA_FLAGS (FR_FLAG_DEEP_JULIA_BLA | FR_FLAG_DEEPX_JULIA_BLA)
#define JULIA_FLAGS_MSG "FR_FLAG_DEEP_JULIA_BLA / FR_FLAG_DEEPX_JULIA_BLA are not available (their tables belong to the Julia paths)"
#define OTHER_FLAGS (FR_FLAG_DEEP_BLA | FR_FLAG_DEEPX_BLA | FR_FLAG_DEEP_SHIP_BLA | FR_FLAG_DEEPX_SHIP_BLA)
#define OTHER_FLAGS_MSG "the BLA flags are not available (their tables belong to the Mandelbrot and Burning Ship paths)"

#define XPHOENIX_FLAG_MSG "FR_FLAG_DEEPX_PHOENIX_BLA is not available (its BLA table belongs to fr_render_deepx_phoenix)"

enum { kDeep, kDeepX, kDeepShip, kDeepXShip, kDeepJulia, kDeepXJulia };

static const deep_rules kRules[6] = {
    [kDeep] = {"fr_render_deep", FR_FRACTAL_MANDELBROT, "FR_FRACTAL_MANDELBROT", 1, 0, kWholeMandel,
               {{JULIA_FLAGS, JULIA_FLAGS_MSG}, {0, NULL}}},
    [kDeepX] = {"fr_render_deepx", FR_FRACTAL_MANDELBROT, "FR_FRACTAL_MANDELBROT", 0, 0, kWholeMandel,
                {{FR_FLAG_DEEP_BLA, "FR_FLAG_DEEP_BLA is not available (its table is fp64): the flag of extended views is "
                                    "FR_FLAG_DEEPX_BLA"},
                 {JULIA_FLAGS, JULIA_FLAGS_MSG}}},
    [kDeepShip] = {"fr_render_deep_ship", FR_FRACTAL_BURNING_SHIP, "FR_FRACTAL_BURNING_SHIP", 1, 0, kWholeShip,
                   {{FR_FLAG_DEEP_BLA | FR_FLAG_DEEPX_BLA,
                     "FR_FLAG_DEEP_BLA / FR_FLAG_DEEPX_BLA are not available (their tables are Mandelbrot's): the flag of the ship "
                     "is FR_FLAG_DEEP_SHIP_BLA"},
                    {JULIA_FLAGS, JULIA_FLAGS_MSG}}},
    [kDeepXShip] = {"fr_render_deepx_ship", FR_FRACTAL_BURNING_SHIP, "FR_FRACTAL_BURNING_SHIP", 0, 0, kWholeShip,
                    {{FR_FLAG_DEEP_BLA | FR_FLAG_DEEPX_BLA | FR_FLAG_DEEP_SHIP_BLA,
                      "FR_FLAG_DEEP_BLA / FR_FLAG_DEEPX_BLA / FR_FLAG_DEEP_SHIP_BLA are not available (their tables belong to the "
                      "other deep paths): the flag of extended Burning Ship views is FR_FLAG_DEEPX_SHIP_BLA"},
                     {JULIA_FLAGS, JULIA_FLAGS_MSG}}},
    [kDeepJulia] = {"fr_render_deep_julia", FR_FRACTAL_JULIA, "FR_FRACTAL_JULIA", 1, 1, kWholeNone,
                    {{OTHER_FLAGS, OTHER_FLAGS_MSG},
                     {FR_FLAG_DEEPX_JULIA_BLA, "FR_FLAG_DEEPX_JULIA_BLA is not available (its table is extended): the flag of this "
                                               "entry point is FR_FLAG_DEEP_JULIA_BLA"}}},
    [kDeepXJulia] = {"fr_render_deepx_julia", FR_FRACTAL_JULIA, "FR_FRACTAL_JULIA", 0, 1, kWholeNone,
                     {{OTHER_FLAGS, OTHER_FLAGS_MSG},
                      {FR_FLAG_DEEP_JULIA_BLA, "FR_FLAG_DEEP_JULIA_BLA is not available (its table is fp64): the flag of this entry "
                                               "point is FR_FLAG_DEEPX_JULIA_BLA"}}},
};

static int validate_params(const deep_rules* k, const fr_params* p, uint32_t width, uint32_t height)
{
    if (!p) return fr_set_error(FR_ERR_INVALID_ARG, "params/deep view is NULL");
    if (p->fractal_type != k->fractal)
        return fr_set_error(FR_ERR_UNSUPPORTED, "%s renders %s only (got %d)", k->who, k->fractal_name, p->fractal_type);
    if (p->precision != FR_PRECISION_F64)
        return fr_set_error(FR_ERR_UNSUPPORTED, "%s needs FR_PRECISION_F64 (got %d)", k->who, p->precision);
    fr_params q = *p;                                            /* the double centre (and a string's zoom) is not read */
    q.center_x = 0.0; q.center_y = 0.0;
    if (!k->zoom_in_params) q.zoom = 1.0;
    int st = fr_params_validate(&q, width, height);
    if (st != FR_OK) return st;
    if (k->zoom_in_params && (st = check_zoom(p->zoom)) != FR_OK) return st;
    if ((st = check_bailout(p->bailout)) != FR_OK) return st;
    if (k->julia && (st = check_julia_c(p->julia_c_real, p->julia_c_imag)) != FR_OK) return st;
    if (k->whole == kWholeMandel && (p->orbit_trap_enabled || p->stripe_enabled || p->interior_style == 2))
        return fr_set_error(FR_ERR_UNSUPPORTED, "%s: the orbit trap, stripes and interior_style 2 need the whole orbit and are "
                            "not available", k->who);
    if (k->whole == kWholeShip &&
        (p->orbit_trap_enabled || (p->stripe_enabled && p->interior_style == 2) || p->interior_style == 3))
        return fr_set_error(FR_ERR_UNSUPPORTED, "%s: the orbit trap, stripes with interior_style 2 and interior_style 3 need the "
                            "whole orbit and are not available", k->who);
    for (int i = 0; i < 2; ++i)
        if (p->flags & k->foreign[i].mask) return fr_set_error(FR_ERR_UNSUPPORTED, "%s: %s", k->who, k->foreign[i].msg);
    if (p->flags & FR_FLAG_DEEPX_PHOENIX_BLA) return fr_set_error(FR_ERR_UNSUPPORTED, "%s: %s", k->who, XPHOENIX_FLAG_MSG);
    return FR_OK;
}

/* the centre rule of the Julia views: |P_0|^2 <= bailout^2, compared exactly */
static int check_julia_centre(const uint64_t* cr, const uint64_t* ci, fx_fmt fmt, float bailout)
{
    const int L = fmt.L, L2 = 2 * fmt.L;
    uint64_t ar[kMaxLimbs], ai[kMaxLimbs];
    uint64_t sr[2 * kMaxLimbs + 1], si[2 * kMaxLimbs + 1], ssum[2 * kMaxLimbs + 1], T[2 * kMaxLimbs + 1];
    memcpy(ar, cr, sizeof(uint64_t) * (size_t)L);
    memcpy(ai, ci, sizeof(uint64_t) * (size_t)L);
    if (is_negative(ar, L)) negate(ar, L);
    if (is_negative(ai, L)) negate(ai, L);
    mul_mag(sr, ar, ar, L);
    mul_mag(si, ai, ai, L);
    sr[L2] = si[L2] = 0;
    add_n(ssum, sr, si, L2 + 1);
    bailout_threshold(T, fmt, bailout);
    if (cmp_n(ssum, T, L2 + 1) > 0)
        return fr_set_error(FR_ERR_INVALID_ARG, "deep Julia view: the centre lies outside the bailout radius (|centre|^2 > bailout^2)");
    return FR_OK;
}

/* a validator with its view: the row's rules for p, then the view resolved and its centre parsed (v or x, as resolve_view) */
static int validate_view(const deep_rules* k, const fr_params* p, const fr_deep_view* v, const fr_deepx_view* x, uint32_t width,
                         uint32_t height)
{
    if (!p || (!v && !x)) return fr_set_error(FR_ERR_INVALID_ARG, "params/deep view is NULL");
    int st = validate_params(k, p, width, height);
    if (st != FR_OK) return st;
    deep_resolved r;
    if ((st = resolve_view(v, x, p->zoom, 1, &r)) != FR_OK) return st;
    return k->julia ? check_julia_centre(r.cr, r.ci, r.fmt, p->bailout) : FR_OK;
}

int fr_deep_validate(const fr_params* p, const fr_deep_view* v, uint32_t width, uint32_t height)
{
    return validate_view(&kRules[kDeep], p, v, NULL, width, height);
}

int fr_deep_ship_validate(const fr_params* p, const fr_deep_view* v, uint32_t width, uint32_t height)
{
    return validate_view(&kRules[kDeepShip], p, v, NULL, width, height);
}

int fr_deepx_validate_params(const fr_params* p, uint32_t width, uint32_t height)
{
    return validate_params(&kRules[kDeepX], p, width, height);
}

int fr_deepx_validate(const fr_params* p, const fr_deepx_view* v, uint32_t width, uint32_t height)
{
    return validate_view(&kRules[kDeepX], p, NULL, v, width, height);
}

int fr_deepx_ship_validate_params(const fr_params* p, uint32_t width, uint32_t height)
{
    return validate_params(&kRules[kDeepXShip], p, width, height);
}

int fr_deepx_ship_validate(const fr_params* p, const fr_deepx_view* v, uint32_t width, uint32_t height)
{
    return validate_view(&kRules[kDeepXShip], p, NULL, v, width, height);
}

int fr_deep_julia_validate(const fr_params* p, const fr_deep_view* v, uint32_t width, uint32_t height)
{
    return validate_view(&kRules[kDeepJulia], p, v, NULL, width, height);
}

int fr_deepx_julia_validate(const fr_params* p, const fr_deepx_view* v, uint32_t width, uint32_t height)
{
    return validate_view(&kRules[kDeepXJulia], p, NULL, v, width, height);
}

int fr_deep_de_default(fr_deep_de* e)
{
    if (!e) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_de is NULL");
    e->de = NULL;
    e->deriv = NULL;
    e->shade = 0;
    e->edge_px = 1.8f;                           /* 0.005 c-plane units (mandelbrot_debug.comp:196) at zoom 3.0 on 1080 rows */
    return FR_OK;
}

/* the rules of the distance block itself, behind the view's */
static int check_de_block(const fr_deep_de* e)
{
    if (e->shade != 0 && e->shade != 1) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_de.shade %d is neither 0 nor 1", e->shade);
    if (e->shade == 1 && (!isfinite(e->edge_px) || !(e->edge_px > 0.0f)))
        return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_de.edge_px must be finite and > 0 with shade 1");
    return FR_OK;
}

int fr_deep_de_validate(const fr_params* p, const fr_deep_view* v, const fr_deep_de* e, uint32_t width, uint32_t height)
{
    if (!e) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_de is NULL");
    const int st = fr_deep_validate(p, v, width, height);
    return st != FR_OK ? st : check_de_block(e);
}

int fr_deepx_de_validate(const fr_params* p, const fr_deepx_view* v, const fr_deep_de* e, uint32_t width, uint32_t height)
{
    if (!e) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_de is NULL");
    const int st = fr_deepx_validate(p, v, width, height);
    if (st != FR_OK) return st;
    if (p->flags & (FR_FLAG_DEEP_SHIP_BLA | FR_FLAG_DEEPX_SHIP_BLA))     /* (fr_render_deepx does not read them) */
        return fr_set_error(FR_ERR_UNSUPPORTED, "fr_render_deepx_de: FR_FLAG_DEEP_SHIP_BLA / FR_FLAG_DEEPX_SHIP_BLA are not "
                            "available (their tables are the Burning Ship's): the flag of this entry point is FR_FLAG_DEEPX_BLA");
    return check_de_block(e);
}

int fr_deep_julia_de_validate(const fr_params* p, const fr_deep_view* v, const fr_deep_de* e, uint32_t width, uint32_t height)
{
    if (!e) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_de is NULL");
    const int st = fr_deep_julia_validate(p, v, width, height);
    return st != FR_OK ? st : check_de_block(e);
}

int fr_deepx_julia_de_validate(const fr_params* p, const fr_deepx_view* v, const fr_deep_de* e, uint32_t width, uint32_t height)
{
    if (!e) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_de is NULL");
    const int st = fr_deepx_julia_validate(p, v, width, height);
    return st != FR_OK ? st : check_de_block(e);
}

int fr_deep_ship_de_validate(const fr_params* p, const fr_deep_view* v, const fr_deep_de* e, uint32_t width, uint32_t height)
{
    if (!e) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_de is NULL");
    const int st = fr_deep_ship_validate(p, v, width, height);
    return st != FR_OK ? st : check_de_block(e);
}

int fr_deepx_ship_de_validate(const fr_params* p, const fr_deepx_view* v, const fr_deep_de* e, uint32_t width, uint32_t height)
{
    if (!e) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_de is NULL");
    const int st = fr_deepx_ship_validate(p, v, width, height);
    return st != FR_OK ? st : check_de_block(e);
}

/* ---- the reference orbits -----------------------------------------------------------------------------------------------------
 * What the six entry points ask before they iterate, in this order: the out pointers (have_out), max_iter, the zoom (the entry's
 * double; NULL for an extended entry, whose view carries a string), the bailout, Julia's c (julia_c, NULL elsewhere), then
 * the view resolved with its centre -- v or x, whichever the entry takes; a NULL view is resolve_view's to refuse. */
static int orbit_request(const char* who, int have_out, const fr_deep_view* v, const fr_deepx_view* x, const double* zoom,
                         int32_t max_iter, float bailout, const double* julia_c, deep_resolved* r)
{
    if (!have_out) return fr_set_error(FR_ERR_INVALID_ARG, "%s: out is NULL", who);
    if (max_iter < 1 || max_iter > (1 << 24))
        return fr_set_error(FR_ERR_INVALID_ARG, "max_iterations %d outside [1, 2^24]", max_iter);
    int st;
    if (zoom && (st = check_zoom(*zoom)) != FR_OK) return st;
    if ((st = check_bailout(bailout)) != FR_OK) return st;
    if (julia_c && (st = check_julia_c(julia_c[0], julia_c[1])) != FR_OK) return st;
    return resolve_view(v, x, zoom ? *zoom : 0.0, 1, r);
}

int fr_deep_reference_orbit(const fr_deep_view* v, double zoom, int32_t max_iter, float bailout, double* out_xy,
                            int32_t* out_len)
{
    deep_resolved r;
    const int st = orbit_request("fr_deep_reference_orbit", out_xy && out_len, v, NULL, &zoom, max_iter, bailout, NULL, &r);
    if (st != FR_OK) return st;
    return orbit_loop(r.cr, r.ci, NULL, NULL, r.fmt, kOrbitMandelbrot, NULL, max_iter, bailout, out_xy, NULL, out_len);
}

int fr_deep_ship_reference_orbit(const fr_deep_view* v, double zoom, int32_t max_iter, float bailout, double* out_xy,
                                 int32_t* out_len)
{
    deep_resolved r;
    const int st = orbit_request("fr_deep_ship_reference_orbit", out_xy && out_len, v, NULL, &zoom, max_iter, bailout, NULL, &r);
    if (st != FR_OK) return st;
    return orbit_loop(r.cr, r.ci, NULL, NULL, r.fmt, kOrbitShip, NULL, max_iter, bailout, out_xy, NULL, out_len);
}

int fr_deepx_reference_orbit(const fr_deepx_view* v, int32_t max_iter, float bailout, double* out_mant_xy, int32_t* out_exp2,
                             int32_t* out_len)
{
    deep_resolved r;
    const int st = orbit_request("fr_deepx_reference_orbit", out_mant_xy && out_exp2 && out_len, NULL, v, NULL, max_iter, bailout,
                                 NULL, &r);
    if (st != FR_OK) return st;
    return orbit_loop(r.cr, r.ci, NULL, NULL, r.fmt, kOrbitMandelbrot, NULL, max_iter, bailout, out_mant_xy, out_exp2, out_len);
}

int fr_deepx_ship_reference_orbit(const fr_deepx_view* v, int32_t max_iter, float bailout, double* out_mant_xy,
                                  int32_t* out_exp2, int32_t* out_len)
{
    deep_resolved r;
    const int st = orbit_request("fr_deepx_ship_reference_orbit", out_mant_xy && out_exp2 && out_len, NULL, v, NULL, max_iter,
                                 bailout, NULL, &r);
    if (st != FR_OK) return st;
    return orbit_loop(r.cr, r.ci, NULL, NULL, r.fmt, kOrbitShip, NULL, max_iter, bailout, out_mant_xy, out_exp2, out_len);
}

/* ---- deep Julia views (fr_render_deep_julia, fr_render_deepx_julia) -----------------------------------------------------------
 * c is a pair of doubles: round_half_even(c 2^F), exact wherever F holds the double's last bit (every c but a tiny one). */
static void double_to_fixed(double c, fx_fmt fmt, uint64_t* out)
{
    memset(out, 0, sizeof(uint64_t) * (size_t)fmt.L);
    if (c == 0.0) return;
    int ex = 0;
    const double mant = frexp(fabs(c), &ex);
    const uint64_t mi = (uint64_t)ldexp(mant, 53);               /* |c| = mi 2^(ex - 53) */
    const long s = (long)ex - 53 + fmt.F;
    if (s >= 0) {
        out[0] = mi;
        shl_bits(out, fmt.L, (int)s);                            /* |c| < 2^32: below 2^(F + 32) */
    } else if (-s < 64) {
        const int k = (int)-s;
        const uint64_t q = mi >> k, rem = mi & ((1ull << k) - 1), half = 1ull << (k - 1);
        out[0] = q + (rem > half || (rem == half && (q & 1u)));
    }                                                            /* else below 2^-11 of a unit: 0 */
    if (c < 0.0) negate(out, fmt.L);
}

/* P (from the centre) and Q (from 0) of z <- z^2 + c in one storage; the view resolved, its centre z */
static int julia_orbits(const deep_resolved* z, const double* c, int32_t max_iter, float bailout, double* p_xy, int32_t* p_exp,
                        int32_t* p_len, double* q_xy, int32_t* q_exp, int32_t* q_len)
{
    int st;
    if ((st = check_julia_centre(z->cr, z->ci, z->fmt, bailout)) != FR_OK) return st;
    uint64_t cr[kMaxLimbs], ci[kMaxLimbs];
    double_to_fixed(c[0], z->fmt, cr);
    double_to_fixed(c[1], z->fmt, ci);
    if ((st = orbit_loop(cr, ci, z->cr, z->ci, z->fmt, kOrbitMandelbrot, NULL, max_iter, bailout, p_xy, p_exp, p_len)) != FR_OK) return st;
    return orbit_loop(cr, ci, NULL, NULL, z->fmt, kOrbitMandelbrot, NULL, max_iter, bailout, q_xy, q_exp, q_len);
}

int fr_deep_julia_reference_orbits(const fr_deep_view* v, double c_re, double c_im, double zoom, int32_t max_iter, float bailout,
                                   double* out_p_xy, int32_t* out_p_len, double* out_q_xy, int32_t* out_q_len)
{
    const double c[2] = {c_re, c_im};
    deep_resolved r;
    const int st = orbit_request("fr_deep_julia_reference_orbits", out_p_xy && out_p_len && out_q_xy && out_q_len, v, NULL, &zoom,
                                 max_iter, bailout, c, &r);
    if (st != FR_OK) return st;
    return julia_orbits(&r, c, max_iter, bailout, out_p_xy, NULL, out_p_len, out_q_xy, NULL, out_q_len);
}

int fr_deepx_julia_reference_orbits(const fr_deepx_view* v, double c_re, double c_im, int32_t max_iter, float bailout,
                                    double* out_p_mant_xy, int32_t* out_p_exp2, int32_t* out_p_len, double* out_q_mant_xy,
                                    int32_t* out_q_exp2, int32_t* out_q_len)
{
    const double c[2] = {c_re, c_im};
    deep_resolved r;
    const int st = orbit_request("fr_deepx_julia_reference_orbits",
                                 out_p_mant_xy && out_p_exp2 && out_p_len && out_q_mant_xy && out_q_exp2 && out_q_len, NULL, v, NULL,
                                 max_iter, bailout, c, &r);
    if (st != FR_OK) return st;
    return julia_orbits(&r, c, max_iter, bailout, out_p_mant_xy, out_p_exp2, out_p_len, out_q_mant_xy, out_q_exp2, out_q_len);
}

/* ---- deep Phoenix views (fr_render_deep_phoenix) ------------------------------------------------------------------------------
 * p and r are floats: floor(v 2^F) of the float's exact value (an integer already wherever F holds the float's last bit). */
static void float_to_fixed_floor(float f, fx_fmt fmt, uint64_t* out)
{
    memset(out, 0, sizeof(uint64_t) * (size_t)fmt.L);
    if (f == 0.0f) return;
    int ex = 0;
    const double mant = frexp(fabs((double)f), &ex);
    const uint64_t mi = (uint64_t)ldexp(mant, 53);               /* |f| = mi 2^(ex - 53) */
    const long s = (long)ex - 53 + fmt.F;
    int lost = 0;
    if (s >= 0) {
        out[0] = mi;
        shl_bits(out, fmt.L, (int)s);                            /* |f| < 2^32: below 2^(F + 32) */
    } else if (-s < 64) {
        out[0] = mi >> -s;
        lost = (mi & ((1ull << -s) - 1)) != 0;
    } else {
        lost = 1;
    }
    if (f < 0.0f) {                                              /* floor of a negative value: away from zero */
        if (lost) add_one(out, fmt.L);
        negate(out, fmt.L);
    }
}

/* the rule both entry points put on p and r beyond fr_phoenix_validate's: inside the fixed point's range, as a centre is */
static int check_phoenix_terms(const fr_phoenix_params* ph)
{
    if (!isfinite(ph->phoenix_p) || !isfinite(ph->phoenix_r) || !(fabsf(ph->phoenix_p) < 4294967296.0f) ||
        !(fabsf(ph->phoenix_r) < 4294967296.0f))
        return fr_set_error(FR_ERR_INVALID_ARG, "deep Phoenix views need finite p and r with |p|, |r| < 2^32");
    return FR_OK;
}

/* The rules of the two entry points, in one order: `entry` with the fp64 view v checks p->zoom and resolves with it; with the
 * extended view x the zoom is the view's string, p->zoom is not read, and the view is checked as fr_deepx_validate checks its own
 * (resolve_view: reserved, frac_bits, the centre strings, the zoom string and its range).  flag: the entry's own BLA flag; other /
 * other_flag / other_table: the other Phoenix entry's, its name and what its table is. */
static int phoenix_view_validate(const char* entry, const char* flag, uint32_t other, const char* other_flag, const char* other_table,
                                 const fr_params* p, const fr_phoenix_params* ph, const fr_deep_view* v, const fr_deepx_view* x,
                                 uint32_t width, uint32_t height)
{
    if (!p || !ph || (!v && !x)) return fr_set_error(FR_ERR_INVALID_ARG, "params/phoenix params/deep view is NULL");
    if (p->fractal_type != FR_FRACTAL_PHOENIX)
        return fr_set_error(FR_ERR_UNSUPPORTED, "%s renders FR_FRACTAL_PHOENIX only (got %d)", entry, p->fractal_type);
    if (p->precision != FR_PRECISION_F64)
        return fr_set_error(FR_ERR_UNSUPPORTED, "%s needs FR_PRECISION_F64 (got %d)", entry, p->precision);
    if (width == 0 || height == 0)
        return fr_set_error(FR_ERR_INVALID_ARG, "width and height must be > 0 (got %ux%u)", width, height);
    fr_params q = *p;                                            /* the double centre is not read, nor an extended view's double zoom */
    q.center_x = 0.0; q.center_y = 0.0;
    if (x) q.zoom = 1.0;
    int st = fr_phoenix_validate(&q, ph, width, height);
    if (st != FR_OK) return st;
    if ((st = check_phoenix_terms(ph)) != FR_OK) return st;
    if (ph->use_julia_set)
        return fr_set_error(FR_ERR_UNSUPPORTED, "%s: use_julia_set is not available (a Julia-mode Phoenix frame "
                            "starts every pixel from z = 0 with the same c, so it is one colour at any depth)", entry);
    if (v && (st = check_zoom(p->zoom)) != FR_OK) return st;
    if (p->flags & (OTHER_FLAGS | JULIA_FLAGS))
        return fr_set_error(FR_ERR_UNSUPPORTED, "%s: the BLA flags of the other paths are not available (their "
                            "tables belong to the Mandelbrot, Burning Ship and Julia paths): the flag of this entry point is "
                            "%s", entry, flag);
    if (p->flags & other)
        return fr_set_error(FR_ERR_UNSUPPORTED, "%s: %s is not available (its BLA table is %s): the flag of this entry point is %s",
                            entry, other_flag, other_table, flag);
    deep_resolved r;
    return resolve_view(v, x, v ? p->zoom : 0.0, 1, &r);
}

int fr_deep_phoenix_validate(const fr_params* p, const fr_phoenix_params* ph, const fr_deep_view* v, uint32_t width, uint32_t height)
{
    return phoenix_view_validate("fr_render_deep_phoenix", "FR_FLAG_DEEP_PHOENIX_BLA", FR_FLAG_DEEPX_PHOENIX_BLA,
                                 "FR_FLAG_DEEPX_PHOENIX_BLA", "extended, fr_render_deepx_phoenix's", p, ph, v, NULL, width, height);
}

/* the shared tail of the two reference orbits: p and r in the resolved view's fixed point, then the Phoenix recurrence; out_exp2
 * with the extended storage */
static int phoenix_orbit_tail(const deep_resolved* r, const fr_phoenix_params* ph, int32_t max_iter, double* out_xy, int32_t* out_exp2,
                              int32_t* out_len)
{
    const int st = check_phoenix_terms(ph);
    if (st != FR_OK) return st;
    phoenix_terms t;
    float_to_fixed_floor(ph->phoenix_p, r->fmt, t.p);
    float_to_fixed_floor(ph->phoenix_r, r->fmt, t.r);
    return orbit_loop(r->cr, r->ci, NULL, NULL, r->fmt, kOrbitPhoenix, &t, max_iter, 2.0f, out_xy, out_exp2, out_len);
}

int fr_deep_phoenix_reference_orbit(const fr_deep_view* v, const fr_phoenix_params* ph, double zoom, int32_t max_iter, double* out_xy,
                                    int32_t* out_len)
{
    if (!ph) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_phoenix_reference_orbit: phoenix params is NULL");
    deep_resolved r;
    int st = orbit_request("fr_deep_phoenix_reference_orbit", out_xy && out_len, v, NULL, &zoom, max_iter, 2.0f, NULL, &r);
    if (st != FR_OK) return st;
    return phoenix_orbit_tail(&r, ph, max_iter, out_xy, NULL, out_len);
}

/* ---- deep Phoenix views below 1e-290 (fr_render_deepx_phoenix): fr_deep_phoenix_validate's rules with the zoom in the view's
 * string ---------------------------------------------------------------------------------------------------------------------- */
int fr_deepx_phoenix_validate(const fr_params* p, const fr_phoenix_params* ph, const fr_deepx_view* v, uint32_t width, uint32_t height)
{
    return phoenix_view_validate("fr_render_deepx_phoenix", "FR_FLAG_DEEPX_PHOENIX_BLA", FR_FLAG_DEEP_PHOENIX_BLA,
                                 "FR_FLAG_DEEP_PHOENIX_BLA", "fp64, fr_render_deep_phoenix's", p, ph, NULL, v, width, height);
}

int fr_deepx_phoenix_reference_orbit(const fr_deepx_view* v, const fr_phoenix_params* ph, int32_t max_iter, double* out_mant_xy,
                                     int32_t* out_exp2, int32_t* out_len)
{
    if (!ph) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deepx_phoenix_reference_orbit: phoenix params is NULL");
    deep_resolved r;
    int st = orbit_request("fr_deepx_phoenix_reference_orbit", out_mant_xy && out_exp2 && out_len, NULL, v, NULL, max_iter, 2.0f,
                           NULL, &r);
    if (st != FR_OK) return st;
    return phoenix_orbit_tail(&r, ph, max_iter, out_mant_xy, out_exp2, out_len);
}
