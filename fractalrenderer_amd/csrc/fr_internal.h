/*
 * fr_internal.h -- declarations shared by the C host side (fr_host.c, fr_franim.c)
 * and the HIP side (fr_device.hip).  Not installed; the public ABI is
 * include/fractalrenderer_amd.h.
 */
#ifndef FR_INTERNAL_H
#define FR_INTERNAL_H

#include "fractalrenderer_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* thread-local last-error message (fr_host.c) */
int fr_set_error(int status, const char* fmt, ...)
#if defined(__GNUC__)
    __attribute__((format(printf, 2, 3)))
#endif
    ;

int32_t fr_deep_zoom_reference_length(const fr_params* p);
/* a shard with its defaults filled in (fr_host.c): NULL = the whole frame, nparts 0 = one part, rows_per_strip 0 = the whole
 * frame for one part and single rows for several */
fr_shard fr_shard_normalise(const fr_shard* s, uint32_t height);
/* the validation of fr_render_phoenix (fr_host.c); width == height == 0 skips the frame-size rules */
int fr_phoenix_validate(const fr_params* p, const fr_phoenix_params* ph, uint32_t width, uint32_t height);
/* the validation of fr_render_mandelbulb (fr_host.c); width == height == 0 skips the frame-size rules */
int fr_mandelbulb_validate(const fr_params* p, const fr_mandelbulb_params* mb, uint32_t width, uint32_t height);
/* the validation of fr_render_deep (fr_deep.c), the centre strings parsed included */
int fr_deep_validate(const fr_params* p, const fr_deep_view* v, uint32_t width, uint32_t height);
/* the validation of fr_render_deep_ship (fr_deep.c): fr_deep_validate's rules for FR_FRACTAL_BURNING_SHIP */
int fr_deep_ship_validate(const fr_params* p, const fr_deep_view* v, uint32_t width, uint32_t height);
/* the validation of fr_render_deepx (fr_deep.c), and its view resolved: the zoom pair and the fraction bits */
int fr_deepx_validate(const fr_params* p, const fr_deepx_view* v, uint32_t width, uint32_t height);
int fr_deepx_resolve(const fr_deepx_view* v, double* zm, int32_t* ze, int32_t* frac_bits);
/* the parts of fr_deepx_validate that a caller with a resolved view shares (fr_deepseq.c): the rules for p, the centre
 * strings parsed at frac_bits, and fr_deepx_frac_bits' rule on a zoom pair */
int fr_deepx_validate_params(const fr_params* p, uint32_t width, uint32_t height);
int fr_deepx_check_centre(const char* center_x, const char* center_y, int32_t frac_bits);
int fr_deepx_frac_bits_pair(double zm, int32_t ze);
/* the validation of fr_render_deepx_ship (fr_deep.c): fr_deep_ship_validate's rules with the zoom from the view's string and
 * no BLA flag but the path's own, FR_FLAG_DEEPX_SHIP_BLA; _params is the part a caller with a resolved view shares */
int fr_deepx_ship_validate(const fr_params* p, const fr_deepx_view* v, uint32_t width, uint32_t height);
int fr_deepx_ship_validate_params(const fr_params* p, uint32_t width, uint32_t height);

/* fr_deep_sequence (fr_deepseq.c): a descriptor resolved -- the two zoom pairs, D = log2(last / first), the one F -- and
 * what frame f is.  fr_deepseq_resolve performs every check of the descriptor; p may be NULL (fr_deep_sequence_plan has
 * none), width == height == 0 skips the frame-size rules as fr_params_validate does. */
typedef struct fr_deepseq_walk {
    double  zm0, zm1, D;
    int32_t ze0, ze1, frames, frac_bits, mode;
} fr_deepseq_walk;
int  fr_deepseq_resolve(const fr_params* p, const fr_deep_sequence_desc* d, uint32_t width, uint32_t height, fr_deepseq_walk* w);
/* fr_deepseq_resolve with p checked by the formula's rules: ship = 0 fr_render_deepx's, 1 fr_render_deepx_ship's */
int  fr_deepseq_resolve_formula(const fr_params* p, const fr_deep_sequence_desc* d, uint32_t width, uint32_t height, int ship,
                                fr_deepseq_walk* w);
void fr_deepseq_frame(const fr_deepseq_walk* w, int32_t frame, fr_deep_sequence_frame* out);
/* tests: a centre string in the fixed point of the reference orbit (fr_deep.c): ceil(frac_bits / 64) + 1 little-endian
 * two's-complement limbs into out[0 .. nlimbs); returns that number of limbs or an error */
int fr_deep_parse_fixed(const char* s, int32_t frac_bits, uint64_t* out, int32_t nlimbs);
/* tests: the context's BLA table (fr_device.hip), copied to the host after a sync of the context's stream: r[0 .. n) and
 * ab[0 .. 4n) (A.x, A.y, B.x, B.y per entry), level after level.  Returns the entries it holds, 0 for none. */
int64_t fr_deep_bla_table(fr_ctx* ctx, double* r, double* ab, int64_t n);
/* tests: the extended BLA table of the context (FR_FLAG_DEEPX_BLA), level 1 first: r receives n entries of 8 bytes (the
 * mantissa as a float, the int32 exponent), ab 4 n doubles (the mantissas of A, B), ab_exp 2 n int32 (their exponents);
 * NULL skips a part.  Returns the number of entries the table has (0: none). */
int64_t fr_deepx_bla_table(fr_ctx* ctx, void* r, double* ab, int32_t* ab_exp, int64_t n);
/* tests: the ship's BLA table of the context (FR_FLAG_DEEP_SHIP_BLA), as fr_deep_bla_table: r[0 .. n) and ab[0 .. 8n)
 * (a11, a12, a21, a22, b11, b12, b21, b22 per entry), level after level.  Returns the entries it holds, 0 for none. */
int64_t fr_deep_ship_bla_table(fr_ctx* ctx, double* r, double* ab, int64_t n);
/* tests: the Phoenix BLA table of the context (FR_FLAG_DEEP_PHOENIX_BLA), as fr_deep_bla_table: r[0 .. n) and mb[0 .. 12n)
 * (M11, M12, M21, M22, B1, B2 per entry, each as x, y), level after level.  Returns the entries it holds, 0 for none. */
int64_t fr_deep_phoenix_bla_table(fr_ctx* ctx, double* r, double* mb, int64_t n);
/* tests: the extended ship BLA table of the context (FR_FLAG_DEEPX_SHIP_BLA), as fr_deepx_bla_table: r receives n entries of 8
 * bytes, ab 8 n doubles (the mantissas a11, a12, a21, a22, b11, b12, b21, b22 per entry), ab_exp 2 n int32 (A.e, B.e);
 * NULL skips a part.  Returns the number of entries the table has (0: none). */
int64_t fr_deepx_ship_bla_table(fr_ctx* ctx, void* r, double* ab, int32_t* ab_exp, int64_t n);
/* tests: the extended Phoenix BLA table of the context (FR_FLAG_DEEPX_PHOENIX_BLA), as fr_deepx_ship_bla_table: r receives n
 * entries of 8 bytes, mb 12 n doubles (the mantissas of M11, M12, M21, M22, B1, B2 per entry, each as x, y), mb_exp 2 n int32
 * (M.e, B.e); NULL skips a part.  Returns the number of entries the table has (0: none). */
int64_t fr_deepx_phoenix_bla_table(fr_ctx* ctx, void* r, double* mb, int32_t* mb_exp, int64_t n);
/* tests: how often the context has built the BLA table of a path: extended 0 / 1, formula 0 Mandelbrot, 1 Burning Ship, 2 Julia,
 * 3 Phoenix (fp64: FR_FLAG_DEEP_PHOENIX_BLA's table, extended: FR_FLAG_DEEPX_PHOENIX_BLA's; a cached table serves a render
 * without a build) */
int64_t fr_deep_bla_builds(fr_ctx* ctx, int extended, int formula);
/* tests: how often the orbit slot of a path has received another orbit (a render of the view it holds leaves it unchanged):
 * extended 0 / 1, formula as above and 3 Phoenix (fr_render_deep_phoenix, fr_render_deepx_phoenix) */
int64_t fr_deep_orbit_generation(fr_ctx* ctx, int extended, int formula);

/* the context's own stream (hipStream_t) and device ordinal: fr_node.cpp orders RCCL transfers behind the renders */
void* fr_ctx_stream_handle(fr_ctx* ctx);
int   fr_ctx_device(const fr_ctx* ctx);

/* thresholds of the 8-bit export (fr_host.c): t[b] = smallest float a in [0, 1] with (uint8)(powf(a, 1/2.2f) * 255) >= b, powf
 * being the correctly rounded single-precision power (a baked table: the same on every host); _host_powf: the same by
 * bisection with the deployment host's libm, for the tests to report where a host's powf differs */
void fr_export8_thresholds(float t[257]);
void fr_export8_thresholds_host_powf(float t[257]);

/* ---- palette knot table: what the kernels stage into LDS ------------------------------
 * Every palette of the two shaders is "warp t, then a 5-knot piece-wise linear ramp"
 * (shaders/mandelbrot.comp:60-141, shaders/julia.comp:20-181).  The table holds the ramp
 * exactly as written (break points, the per-segment multiply/divide constant, the knots),
 * so the device evaluation performs the shader's own float operations. */
enum {
    FR_WARP_NONE       = 0,   /* w = t                        */
    FR_WARP_POW        = 1,   /* w = pow(t, e)                */
    FR_WARP_SMOOTHSTEP = 2,   /* w = smoothstep(0, 1, t)      */
    FR_WARP_GRAY       = 3    /* colour = vec3(t), no ramp    */
};

typedef struct fr_palette_table {
    int32_t warp;
    float   warp_exp;
    int32_t nseg;            /* 4 or 5                                              */
    int32_t last_const;      /* 1: last segment returns knot[4] (fire-style ramps)  */
    float   seg_lo[5];       /* segment k covers w in [seg_lo[k], seg_lo[k+1])      */
    float   seg_k[5];        /* mix factor = (w - seg_lo[k]) * seg_k[k]  or / seg_k[k] */
    int32_t seg_div[5];      /* 1: divide by seg_k, 0: multiply                      */
    int32_t any_div;         /* some segment divides (lets the kernels skip the divide otherwise) */
    float   knot[6][4];      /* RGB knots (4th lane padding); knot[k], knot[k+1] bound segment k */
} fr_palette_table;

/* shader: 0 = shaders/mandelbrot.comp numbering, 1 = shaders/julia.comp numbering */
void fr_palette_table_build(int shader, int palette_mode, fr_palette_table* out);

#ifdef __cplusplus
}
#endif
#endif
