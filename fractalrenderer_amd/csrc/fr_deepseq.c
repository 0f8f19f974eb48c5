/*
 * fr_deepseq.c -- host planning of deep zoom sequences (fr_deep_sequence; the rules are in the header): the descriptor
 * resolved into the two zoom pairs, D and the one F, and what frame f is.  Plain C, no device; the device glue is next
 * to the fr_render_deepx code in fr_device.hip.
 */
#include <math.h>
#include <stddef.h>

#include "fr_internal.h"

/* zoom_pair's range rule (fr_deep.c) on a pair: 1e-1000 = 1.0511037747648835 2^-3322, 1e3 = 1.953125 2^9 */
static int pair_in_range(double m, int64_t e)
{
    return !(e < -3322 || (e == -3322 && m < 1.0511037747648835) || e > 9 || (e == 9 && m > 1.953125));
}

/* L of frame f (0 < f < frames - 1 takes the division), and s = -L, k = floor(s) */
static double frame_L(const fr_deepseq_walk* w, int32_t f)
{
    if (f == 0) return 0.0;
    if (f == w->frames - 1) return w->D;
    return (w->D * (double)f) / (double)(w->frames - 1);
}

void fr_deepseq_frame(const fr_deepseq_walk* w, int32_t f, fr_deep_sequence_frame* out)
{
    const double L = frame_L(w, f);
    if (f == 0) {
        out->zoom_mant = w->zm0;
        out->zoom_exp2 = w->ze0;
    } else if (f == w->frames - 1) {
        out->zoom_mant = w->zm1;
        out->zoom_exp2 = w->ze1;
    } else {
        double q = floor(L);
        const double r = L - q;
        double m = w->zm0 * exp2(r);
        if (m >= 2.0) { m = m / 2.0; q = q + 1.0; }
        out->zoom_mant = m;
        out->zoom_exp2 = w->ze0 + (int32_t)q;
    }
    const double s = -L;
    const double k = floor(s);
    const int on_grid = s == k;
    out->frac_bits = w->frac_bits;
    out->keyframe = (int32_t)k;
    out->resampled = (w->mode == 1 && !on_grid) ? 1 : 0;
    out->u = on_grid ? 1.0 : exp2(-(s - k));
}

int fr_deepseq_resolve(const fr_params* p, const fr_deep_sequence_desc* d, uint32_t width, uint32_t height, fr_deepseq_walk* w)
{
    return fr_deepseq_resolve_formula(p, d, width, height, 0, w);
}

int fr_deepseq_resolve_formula(const fr_params* p, const fr_deep_sequence_desc* d, uint32_t width, uint32_t height, int ship,
                               fr_deepseq_walk* w)
{
    if (!d || !w) return fr_set_error(FR_ERR_INVALID_ARG, "deep sequence descriptor is NULL");
    int st;
    if (p && (st = ship ? fr_deepx_ship_validate_params(p, width, height) : fr_deepx_validate_params(p, width, height)) != FR_OK)
        return st;
    if (d->reserved != 0) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_sequence_desc.reserved must be 0");
    if (d->frames < 2) return fr_set_error(FR_ERR_INVALID_ARG, "a deep sequence has at least 2 frames (got %d)", d->frames);
    if (d->mode != 0 && d->mode != 1) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_sequence_desc.mode %d outside {0, 1}", d->mode);
    if (d->frac_bits != 0 && (d->frac_bits < 128 || d->frac_bits > 4096))
        return fr_set_error(FR_ERR_INVALID_ARG, "frac_bits %d outside {0} U [128, 4096]", d->frac_bits);
    if (!d->center_x || !d->center_y) return fr_set_error(FR_ERR_INVALID_ARG, "deep view centre string is NULL");
    if ((st = fr_deepx_zoom(d->zoom_first, &w->zm0, &w->ze0)) != FR_OK) return st;
    if ((st = fr_deepx_zoom(d->zoom_last, &w->zm1, &w->ze1)) != FR_OK) return st;
    w->D = (double)(w->ze1 - w->ze0) + (log2(w->zm1) - log2(w->zm0));
    w->frames = d->frames;
    w->mode = d->mode;
    const int first_smaller = w->ze0 < w->ze1 || (w->ze0 == w->ze1 && w->zm0 < w->zm1);
    w->frac_bits = d->frac_bits ? d->frac_bits
                                : fr_deepx_frac_bits_pair(first_smaller ? w->zm0 : w->zm1, (first_smaller ? w->ze0 : w->ze1) - 1);
    if ((st = fr_deepx_check_centre(d->center_x, d->center_y, w->frac_bits)) != FR_OK) return st;
    if (d->mode == 1) {
        /* s is monotone in f, so the keyframes needed at the two ends of the walk bound all of them: k of frames 0 and
         * frames-1, and k + 1 of the off-grid frames next to them */
        const int32_t probe[4] = {0, 1, d->frames - 2, d->frames - 1};
        for (int i = 0; i < 4; ++i) {
            fr_deep_sequence_frame fp;
            fr_deepseq_frame(w, probe[i], &fp);
            for (int j = 0; j <= fp.resampled; ++j)
                if (!pair_in_range(w->zm0, (int64_t)w->ze0 - ((int64_t)fp.keyframe + j)))
                    return fr_set_error(FR_ERR_INVALID_ARG, "deep sequence: keyframe %d of frame %d lies outside [1e-1000, 1e3]",
                                        fp.keyframe + j, probe[i]);
        }
    }
    return FR_OK;
}

int fr_deep_sequence_plan(const fr_deep_sequence_desc* desc, int32_t frame, fr_deep_sequence_frame* out)
{
    if (!out) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_sequence_plan: out is NULL");
    fr_deepseq_walk w;
    const int st = fr_deepseq_resolve(NULL, desc, 0, 0, &w);
    if (st != FR_OK) return st;
    if (frame < 0 || frame >= w.frames)
        return fr_set_error(FR_ERR_INVALID_ARG, "frame %d outside [0, %d)", frame, w.frames);
    fr_deepseq_frame(&w, frame, out);
    return FR_OK;
}
