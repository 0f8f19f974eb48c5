/*
 * fr_plan.h -- internal, host code: the tuning knobs of a context and the schedule of a render as a value.
 *
 * plan_render() decides everything about a Mandelbrot / Julia / Burning Ship render that is decided before its first
 * launch -- route, kernel family, one pass or two, budgets, grids, queue geometry, buffer sizes -- from the tunings, the
 * compute-unit count and the request alone: no HIP call, no context.  None of it can change a pixel, so the GPU tests pass
 * whichever schedule is chosen; tests/test_render_plan_host.py pins it instead (fr_plan_describe, fr_tuning.h).
 * Not self-contained: fr_device.hip includes it behind fr_kernels.hip.h, whose QueueArgs and queue constants (kShards,
 * kMaxShards, kShardBlock, kFastBlock, kQueueProbeShift) it uses.
 */
#ifndef FR_PLAN_H
#define FR_PLAN_H

#include <stdint.h>
#include <string.h>

#include "fr_internal.h"

namespace fr {

/* fr_ctx_set_tuning / fr_ctx_set_option by name; 0 = the automatic choice unless said otherwise */
struct Tuning {
    int32_t periodicity;        /* cycle closing: -1 off, 0 automatic (on, first window 128), else the first snapshot window in iterations */
    uint32_t staging;           /* 0 = automatic, 1 = single pass, 3 = tile pass + lane-pool pass whatever max_iter is */
    uint32_t stage_first;       /* iteration budget b0 of the tile pass */
    uint32_t shards;            /* 8 or 64: queue shards / stream regions of a render */
    uint32_t regions;           /* (= shards), 8 or 64: regions of the survivor streams */
    uint32_t tile_kernel;       /* 0 = the lean tile kernel where it applies, 1 = the general tile_kernel */
    uint32_t shape;             /* else FPW_LOG2 (3, 4, 6) */
    uint32_t wg_per_cu, run_max, run_min;
    int32_t shift_bias;         /* added to the guided-run shift */
    uint32_t probes;            /* tile pass: shards a wave probes before exiting */
    uint32_t stream_run_max, stream_run_min, stream_wg_per_cu;
    uint32_t stream_probes;     /* same for the stream / lane-pool passes */
    uint32_t stream_rotate;     /* 0 automatic, 1 regions by XCD, 2 writers rotate over the regions */
    uint32_t pool_refill;       /* lane pool: idle lanes that trigger a refill (0 = 24, fp64 16) */
    uint32_t pool_items_per_wg; /* lane pool grid: at most one workgroup per this many sub-tiles of the frame (0 = 32) */
    uint32_t stripes;           /* the Mandelbrot shader's effects (stripes, orbit trap, trap-coloured interior): 0 = automatic (lean tile
                                   pass + lane pool, kernel code FRACTAL = 3), 1 = the effects variant of the general tile kernel */
    uint32_t ssaa;              /* SSAA: 0 = automatic, 1 = the sample loop of the general tile kernel, 2 = staged (sample grid
                                 * through tile pass + lane pool, then ssaa_reduce_kernel) wherever it applies */
    uint32_t ssaa_band;         /* staged SSAA: samples per band of a whole frame whose sample grid is larger (0 = automatic: 2^29) */
    uint32_t tile_pixels;       /* lean tile kernel: sub-tiles (pixels per lane) per trip, 0 = automatic (2), 1 or 2 */
    uint32_t tile_exit;         /* lean tile pass, staged: occupancy exit -- 0 = automatic, 1 = off, else the per-record cost of the
                                   lane pool in updates that the exit rule assumes (escape_run_lean) */
    uint32_t tile_exit_from;    /* ... and the updates a trip runs before it may leave (0 = automatic) */
    uint32_t prepare;           /* 0 = automatic (the tile pass prepares its own control block and tables, except on a capturing
                                   stream), 1 = prepare_kernel in a launch of its own */
    uint32_t whole_blocks;      /* survivor stream in two classes (whole blocks beside the ring's records): 0 = automatic (plan_render: large
                                   fp64 frames), 1 = off, 2 = on wherever whole_blocks_apply */
    uint32_t mandelbulb_split;  /* 0 = automatic (march / shade split), 1 = shade at the hit, inside the march loop */
    uint32_t fold;              /* folded render of a real-axis-symmetric Mandelbrot frame (plan_fold): 0 = automatic (frames of at least
                                   kFoldAutoPixels pixels), 1 = off, 2 = on wherever the frame qualifies */
    uint32_t debug_region_blocks; /* tests only: cap the capacity of a survivor-stream region, to provoke an overflow */
};

constexpr int kNotMine = 1;     /* tuning_set / option_set: the name is somebody else's */

/* fr_ctx_set_tuning's names that are one unsigned member: accepted are [0, hi] (hi < 0: anything), or 0 and the values of `set` */
struct TuningRow { const char* name; uint32_t Tuning::*member; int64_t hi, set[3]; const char* error; };
static const TuningRow kTuningRows[] = {
    {"workgroups_per_cu", &Tuning::wg_per_cu, 16, {}, "workgroups_per_cu must be in [0,16]"},
    {"run_max", &Tuning::run_max, 1024, {}, "run_max must be in [0,1024]"},
    {"run_min", &Tuning::run_min, 1024, {}, "run_min must be in [0,1024]"},
    {"subtile_shape", &Tuning::shape, 0, {3, 4, 6}, "subtile_shape must be 0, 3 (8x8), 4 (16x4) or 6 (64x1)"},
    {"pool_refill_at", &Tuning::pool_refill, 64, {}, "pool_refill_at must be in [0,64]"},
    {"stage_first", &Tuning::stage_first, 1 << 24, {}, "stage_first out of range"},
    {"stream_run_max", &Tuning::stream_run_max, 1024, {}, "stream_run_max must be in [0,1024]"},
    {"stream_run_min", &Tuning::stream_run_min, 1024, {}, "stream_run_min must be in [0,1024]"},
    {"stream_workgroups_per_cu", &Tuning::stream_wg_per_cu, 8, {}, "stream_workgroups_per_cu must be in [0,8]"},
    {"stream_rotate", &Tuning::stream_rotate, -1, {}, ""},
    {"regions", &Tuning::regions, 0, {8, 64}, "regions must be 0 (automatic), 8 or 64"},
    {"tile_pixels", &Tuning::tile_pixels, 2, {}, "tile_pixels must be 0 (automatic), 1 or 2"},
    {"prepare", &Tuning::prepare, 1, {}, "prepare must be 0 (automatic: inside the lean tile pass) or 1 (a launch of its own)"},
    {"tile_exit", &Tuning::tile_exit, 4096, {}, "tile_exit must be 0 (automatic), 1 (off) or a cost in updates up to 4096"},
    {"tile_exit_from", &Tuning::tile_exit_from, 1 << 24, {}, "tile_exit_from out of range"},
    {"ssaa", &Tuning::ssaa, 2, {}, "ssaa must be 0 (automatic), 1 (sample loop of the general tile kernel) or 2 (staged)"},
    {"stripes", &Tuning::stripes, 1, {}, "stripes must be 0 (automatic) or 1 (Mandelbrot effects by the effects variant of the general tile kernel)"},
    {"ssaa_band_samples", &Tuning::ssaa_band, 1ll << 30, {}, "ssaa_band_samples must be 0 (automatic: 2^29) or up to 2^30"},
    {"pool_items_per_wg", &Tuning::pool_items_per_wg, 4096, {}, "pool_items_per_wg must be in [0,4096]"},
    {"whole_blocks", &Tuning::whole_blocks, 2, {}, "whole_blocks must be 0 (automatic), 1 (off) or 2 (on wherever the lane pool has the loop for them)"},
    {"mandelbulb_split", &Tuning::mandelbulb_split, 1, {}, "mandelbulb_split must be 0 (automatic: march / shade split) or 1 (shade inside the march loop)"},
    {"debug_region_blocks", &Tuning::debug_region_blocks, -1, {}, ""},   /* tests only (overflow reporting); 0 = the real capacity */
};

/* one name of fr_ctx_set_tuning: FR_OK, an error, or kNotMine */
inline int tuning_set(Tuning& t, const char* name, int64_t value)
{
    for (const TuningRow& r : kTuningRows) {
        if (strcmp(name, r.name)) continue;
        bool ok = r.set[0] ? value == 0 : (r.hi < 0 || (value >= 0 && value <= r.hi));
        for (const int64_t v : r.set) ok = ok || (v != 0 && value == v);
        if (!ok) return fr_set_error(FR_ERR_INVALID_ARG, "%s", r.error);
        t.*r.member = (uint32_t)value;
        return FR_OK;
    }
    if (!strcmp(name, "shift_bias")) {                /* the one signed knob */
        if (value < -16 || value > 16) return fr_set_error(FR_ERR_INVALID_ARG, "shift_bias must be in [-16,16]");
        t.shift_bias = (int32_t)value;
    } else if (!strcmp(name, "probes") || !strcmp(name, "stream_probes")) {
        (name[0] == 's' ? t.stream_probes : t.probes) = (uint32_t)value & 0xFu;
    } else {
        return kNotMine;
    }
    return FR_OK;
}

/* the names of fr_ctx_set_option that are tunings: FR_OK, an error, or kNotMine */
inline int option_set(Tuning& t, const char* name, int64_t value)
{
    if (!strcmp(name, "periodicity")) {
        if (value < -1 || value > (1 << 20)) return fr_set_error(FR_ERR_INVALID_ARG, "periodicity must be -1 (off), 0 (automatic: on), 1 (on) or a first snapshot window in iterations");
        t.periodicity = value <= 0 ? (int32_t)value : (value == 1 ? 128 : (int32_t)((value + 15) / 16 * 16));
    } else if (!strcmp(name, "staging")) {
        /* 2 (block stream passes) and 4 (fused launch) were measured dead ends and left the library in 1.0: accepted,
         * they select the automatic schedule */
        if (value < 0 || value > 4) return fr_set_error(FR_ERR_INVALID_ARG, "staging must be 0 (automatic), 1 (single pass) or 3 (tile pass + lane-pool pass)");
        t.staging = (value == 2 || value == 4) ? 0u : (uint32_t)value;
    } else if (!strcmp(name, "shards")) {
        if (value != 0 && value != 8 && value != 64) return fr_set_error(FR_ERR_INVALID_ARG, "shards must be 0 (automatic), 8 or 64");
        t.shards = (uint32_t)value;
    } else if (!strcmp(name, "tile_kernel")) {
        if (value < 0 || value > 1) return fr_set_error(FR_ERR_INVALID_ARG, "tile_kernel must be 0 (automatic: lean where it applies) or 1 (general)");
        t.tile_kernel = (uint32_t)value;
    } else if (!strcmp(name, "fold")) {
        if (value < 0 || value > 2) return fr_set_error(FR_ERR_INVALID_ARG, "fold must be 0 (automatic), 1 (off) or 2 (on wherever the frame qualifies)");
        t.fold = (uint32_t)value;
    } else {
        return kNotMine;
    }
    return FR_OK;
}

/* the smallest b with 2^b >= v, at most 31 */
inline uint32_t ceil_log2(uint32_t v) { return v <= 1u ? 0u : (v > (1u << 31) ? 31u : 32u - (uint32_t)__builtin_clz(v - 1u)); }

/* run_shift of a guided queue: log2 of the divisor, moved by "shift_bias" */
inline uint32_t clamp_shift(const Tuning& t, int v) { v += t.shift_bias; return (uint32_t)(v < 0 ? 0 : (v > 31 ? 31 : v)); }

/* Cycle closing ("periodicity"): on unless switched off.  Where it takes effect: the lane-pool pass (PERIOD
 * instantiation), the tile kernel when it runs samples to max_iter with 8x8 sub-tiles -- a one-pass frame (PERIOD
 * instantiation) and SSAA (always compiled in).  Where it does not: the effects variants, one-pass frames with 16x4 /
 * 64x1 sub-tiles and Deep_Zoom -- those iterate every sample to max_iter, as the reference does. */
inline uint32_t period_window(const Tuning& t) { return t.periodicity < 0 ? 0u : (t.periodicity == 0 ? 128u : (uint32_t)t.periodicity); }

/* colourings that need more of the orbit than (escape index, |z|^2): the as-written effects loops */
inline bool needs_effects(const fr_params* p)
{
    switch (p->fractal_type) {
    case FR_FRACTAL_MANDELBROT:   return p->orbit_trap_enabled || p->stripe_enabled || p->interior_style == 2;
    case FR_FRACTAL_BURNING_SHIP: return p->orbit_trap_enabled || (p->stripe_enabled && p->interior_style == 2) ||
                                         p->interior_style == 3;
    default: return false;
    }
}

/* The lean tile kernel serves 8x8 sub-tiles whose row strips (if sharded) are whole sub-tile rows; "tile_kernel" = 1 keeps
 * the general kernel (tests compare the two bitwise).  row_multiple: 1, or aa when the question is about the sample grid
 * of a strip (its rows are rows_per_strip x aa samples high).  What else a caller needs -- one sample per pixel, no
 * effects variant -- it asks itself. */
inline bool lean_applies(const Tuning& t, const fr_shard& shard, uint32_t row_multiple)
{
    return t.tile_kernel != 1u && (t.shape == 0u || t.shape == 3u) && (shard.nparts == 1 || (shard.rows_per_strip * row_multiple) % 8u == 0u);
}

/* ---- folded render ------------------------------------------------------------------------------------
 * The Mandelbrot viewport map is cy(py) = center_y + ((py - 0.5 H) / H) zoom (write_coordinate_tables, MAP == 0): with
 * center_y == 0 rows r and H - r get exactly negated cy, for even and odd H, in either precision.  The update negates Yd and
 * changes nothing else -- products and round-to-nearest are sign-symmetric; x2, y2d and 4|z|^2 are even in Yd -- so the two
 * orbits are conjugates bit for bit: same escape index, same |z|^2, and the plain colour stage is a function of those two
 * alone.  Such a frame renders rows [0, R) and every store of a pixel in row r also stores the same values at row H - r.
 * R = floor(H / 2) + 1 rounded up to whole sub-tile rows; the mirrored store happens iff r >= 1 and H - r >= R, so a mirror
 * never lands on a row that is rendered itself (row 0 has no partner, row H / 2 is its own).
 * Qualifies: Mandelbrot by the lean family without effects (stripes read the sign of z), one sample per pixel (the SSAA
 * sample offsets are anchored top-left and do not mirror), a whole frame (no shard, not a sample grid), (T)center_y == 0 in
 * the kernels' precision, R < H.  "fold" = 2 never overrides any of these; automatic folds frames of at least
 * kFoldAutoPixels pixels (below that the frame is one pass and ramp-bound: halving its rows buys little). */
constexpr size_t kFoldAutoPixels = (size_t)1 << 20;

inline uint32_t fold_rows(uint32_t H) { return (uint32_t)(((uint64_t)H / 2u + 1u + 7u) & ~(uint64_t)7u); }

/* rows the folded render of this request renders, or 0: not folded */
inline uint32_t plan_fold(const Tuning& t, const fr_params* p, uint32_t W, uint32_t H, const fr_shard& norm, int ssaa_of)
{
    if (t.fold == 1u || p->fractal_type != FR_FRACTAL_MANDELBROT) return 0u;
    if (needs_effects(p) || p->antialiasing_samples > 1 || ssaa_of > 1) return 0u;
    if (norm.nparts != 1u || !lean_applies(t, norm, 1)) return 0u;
    const bool zero = p->precision == FR_PRECISION_F64 ? (double)p->center_y == 0.0 : (float)p->center_y == 0.0f;
    if (!zero) return 0u;
    const uint32_t R = fold_rows(H);
    if (R >= H) return 0u;
    if (t.fold == 0u && (size_t)W * H < kFoldAutoPixels) return 0u;
    return R;
}

/* The lane pool's records carry a pixel's index in the planes and nothing else: its row is index / W, as one multiplication
 * and one shift.  With l = ceil(log2 W), s = 31 + l and m = floor(2^s / W) + 1 (< 2^32):  index m / 2^s = index / W + index e / 2^s
 * with 0 < e <= 1, and index e / 2^s < 2^31 / 2^s = 2^-l <= 1 / W for every index < 2^31 -- less than what the fraction of
 * index / W lacks to the next integer -- so floor(index m / 2^s) == floor(index / W) for every index a legal frame has.
 * fold_div_ok evaluates the kernel's expression at both ends of every row of the frame (the expression is monotonic in the
 * index): the same kind of check exact_division_ok makes for the viewport map. */
struct FoldDiv { uint32_t magic, shift; };
inline FoldDiv fold_div(uint32_t W)
{
    FoldDiv d;
    d.shift = 31u + ceil_log2(W);
    d.magic = (uint32_t)((((uint64_t)1 << d.shift) / W) + 1u);
    return d;
}
inline uint32_t fold_div_apply(const FoldDiv& d, uint32_t index) { return (uint32_t)(((uint64_t)index * d.magic) >> d.shift); }
/* exact for every index in [0, n)?  (n <= 2^31) */
inline bool fold_div_ok(uint32_t W, const FoldDiv& d, uint64_t n)
{
    if (W == 0u || n > ((uint64_t)1 << 31)) return false;
    for (uint64_t first = 0, row = 0; first < n; first += W, ++row) {
        const uint64_t last = first + W - 1u < n - 1u ? first + W - 1u : n - 1u;
        if (fold_div_apply(d, (uint32_t)first) != row || fold_div_apply(d, (uint32_t)last) != row) return false;
    }
    return true;
}

/* ---- geometry of the tile pass ----------------------------------------------------------------------
 * Sub-tiles of 64 pixels (2^shape wide) in blocks of 16 dealt round by round to the 8 or 64 shards, a shard's place
 * rotating with the round (WaveQueue::block_of; blocks >= n_blk are skipped by the kernels); a persistent grid of
 * exactly the resident set (wg_per_cu workgroups per CU unless "workgroups_per_cu" says otherwise); run lengths and
 * probe limit of the queue.  The Deep_Zoom and Phoenix kernels take the same queue as an unbounded pass on 8x8 sub-tiles.
 * (The caller sets heads.) */
inline QueueArgs plan_tile_queue(const Tuning& t, int compute_units, uint32_t W, uint32_t rows_local, int shape, bool bounded,
                                 bool moderate, uint32_t wg_per_cu, uint32_t* grid_out)
{
    const uint32_t fpw = 1u << shape, fph = 64u >> shape;
    QueueArgs tq = {};
    tq.nsx = (W + fpw - 1) / fpw;
    tq.nsx_shift = -1;
    for (int b = 0; b < 31; ++b)
        if (tq.nsx == (1u << b)) tq.nsx_shift = b;
    const uint32_t nsy = (rows_local + fph - 1) / fph;
    tq.n_items = tq.nsx * nsy;
    tq.n_blk = (tq.n_items + kShardBlock - 1) / kShardBlock;

    uint32_t grid = (uint32_t)compute_units * (t.wg_per_cu ? t.wg_per_cu : wg_per_cu);
    /* never more waves than the shortest runs can feed: a wave takes at least run_min sub-tiles per dequeue (4 when
     * bounded, 2 otherwise), and waves that find nothing still cost their launch and their exit probes -- at 512^2
     * a grid of one wave per sub-tile left 3 of 4 waves without work: 0.083 ms per frame against 0.048 ms */
    const uint32_t per_wave = t.run_min ? t.run_min : (bounded ? 4u : 2u);
    const uint32_t max_grid = (tq.n_items + 4u * per_wave - 1u) / (4u * per_wave);
    if (grid > max_grid) grid = max_grid < 1 ? 1 : max_grid;
    /* Shards: 64 (8 per XCD) where waves stop at their home shard(s) and the frame has work for them -- 64 queue heads
     * (and 64 block counters of the survivor stream) instead of 8 take the same claims at 8x the rate (kMaxShards);
     * launches with unlimited stealing keep 8: a wave probes every shard before it exits. */
    const bool limited = (bounded || moderate) && grid >= 64u;
    /* (from 4 blocks per shard and 256 workgroups: a 512^2 frame -- 256 blocks -- measured -6 % with 64 shards, end of round 4;
     * the rule had asked for 8 blocks per shard and 512 workgroups) */
    uint32_t ns = (limited && grid >= 256u && tq.n_blk >= 4u * (uint32_t)kMaxShards) ? (uint32_t)kMaxShards : (uint32_t)kShards;
    if (t.shards) ns = t.shards;
    tq.ns_log2 = ns == (uint32_t)kMaxShards ? 6u : 3u;
    const uint32_t waves_per_shard = (grid * 4u + ns - 1) / ns;
    /* Run length of a dequeue = clamp(remaining >> run_shift, run_min, run_max).
     *  - unbounded items (single pass, measured on C2, profiles/r01_sweep_c2.txt): sub-tile cost varies 100x,
     *    so long runs leave a tail of waves holding several max_iter sub-tiles while single sub-tile claims
     *    saturate the queue words (~88 dequeues/us each: a 0.44 ms floor): short runs of 2..8;
     *  - bounded items (staged tile pass: at most b0 iterations each): long runs are safe and hide the
     *    dequeue latency that dominates cheap sub-tiles. */
    if (bounded) {
        /* 64 shards: runs a quarter as long again (remaining / (8 waves' worth)) -- with waves that stop at their home
         * shards the last runs of a shard are its tail, and at 80 waves per shard a run of 16 sub-tiles inside the set is
         * 20 us on a chip that is otherwise done: C2 tile pass 114 -> 105 us, C3 125 -> 112 us, C5 1639 -> 1593 us
         * (a view where every sub-tile costs the same pays for the extra claims: 76 -> 85 us) */
        tq.run_shift = clamp_shift(t, (int)ceil_log2(2u * waves_per_shard) + (ns == (uint32_t)kMaxShards ? 2 : 0));
        tq.run_max = t.run_max ? t.run_max : 32u;
        tq.run_min = t.run_min ? t.run_min : 4u;
    } else {
        tq.run_shift = clamp_shift(t, (int)ceil_log2(16u * waves_per_shard));
        tq.run_max = t.run_max ? t.run_max : 8u;
        tq.run_min = t.run_min ? t.run_min : 2u;
    }
    if (tq.run_min > tq.run_max) tq.run_min = tq.run_max;
    tq.flags = 0u;
    /* Bounded items are dealt evenly to the shards, so a wave whose home shard is dry exits instead of
     * probing the other 7 (measured: the exit storm of 4096 waves x 8 serialized atomics costs 31 us of the
     * 260 us tile pass of C2 and 36 of the 74 us of a 1/8 shard, profiles/r01_probe_limit.txt).  Unbounded
     * passes keep full stealing; so do grids with fewer workgroups than shards. */
    /* Passes whose items are long (SSAA: aa^2 samples to max_iter per pixel; effects; a forced single pass) keep full
     * stealing: with home + one neighbour the C5 view at 2x2 samples takes 9.96 ms instead of 8.12 ms. */
    /* 64 shards: home + the next one of the same XCD (80 waves per shard: a second look evens out the ends) */
    uint32_t probes = t.probes ? t.probes : (limited ? (ns == (uint32_t)kMaxShards ? 2u : 1u) : 0u);
    if (grid < ns) probes = 0;
    tq.flags |= probes << kQueueProbeShift;
    *grid_out = grid;
    return tq;
}

/* ---- stage schedule ----------------------------------------------------------------------------------
 * Two passes -- the tile pass runs [0, b0), the lane pool [b0, max_iter) -- or one.  Not staged: SSAA (samples of a pixel
 * must meet again to be averaged), the effects variants (accumulators along the whole orbit), short max_iter.
 * plan_stages returns the number of passes and *b0 = upper iteration bound of the first (max_iter when it is the only
 * one).  (Block stream passes with x4 budgets and a fused one-launch schedule were built and measured slower everywhere:
 * DESIGN.md section 7.) */
inline int staging_threshold(const fr_params* p, size_t npx)
{
    const bool big = npx > ((size_t)1 << 23);
    if (p->fractal_type == FR_FRACTAL_JULIA) return npx <= ((size_t)1 << 20) ? 512 : 256;   /* (small frames: 256^2 ... 1024x768 at 256, the
                                                                                              * dust 55 -> 36 us in one pass, a filled set 50 -> 23) */
    /* Small frames (end of round 4, profiles/r04_small_frame_staging.txt): the second launch and the lane pool's ramp and
     * run-out are ~45-60 us whatever the frame, which a frame of half a megapixel does not win back before max_iter 1024-2048
     * (256^2 at 512, fp64: 74 -> 49 us in one pass; 512^2 at 1024, fp32: 92 -> 72; but the Seahorse view at 2048: 129 against
     * 168-190 in one pass): up to 2^19 pixels fp32 stages from 1536, fp64 from 1024 -- from 1536 up to 2^18 pixels; a Julia set from 512 up to 2^20 pixels. */
    if (npx <= ((size_t)1 << 19)) return p->precision == FR_PRECISION_F64 ? (npx <= ((size_t)1 << 18) ? 1536 : 1024) : 1536;
    return p->precision == FR_PRECISION_F64 ? (big ? 384 : 512) : (big ? 512 : 768);
}

inline int plan_stages(const Tuning& t, const fr_params* p, bool effects, size_t npx, bool pool_runs_everything, int* b0)
{
    const int max_iter = p->max_iterations;
    const bool allow = !effects && p->antialiasing_samples <= 1 && t.staging != 1u;
    /* tile-pass budget: ~max_iter/28 rounded to the unchecked block, within [32, 192] (measured best:
     * 32 at max_iter 1024, 64 at 2048, 128-192 at 4096, flat at 16384) */
    int auto_first = ((max_iter / 28 + kFastBlock / 2) / kFastBlock) * kFastBlock;
    auto_first = auto_first < 32 ? 32 : (auto_first > 192 ? 192 : auto_first);
    /* fp64 frames of 2^24 pixels and more whose lane pool runs every survivor to max_iter (cycle closing off, or skipped
     * because it closed nothing lately): ~max_iter/11 within [96, 192].  Round 3's sweeps with the lean tile kernel
     * (profiles/r03_b0_and_pool_tuning.txt): C2 (4096^2, 1024) 96 against 32: -1.8 %, C5 (8192^2, 4096) 192 against 144:
     * -0.5 %; a 1080p frame at 1024 keeps 32 (96: +8 %), the fp32 Julia dust its 80 (96-128 within noise, 256: +8 %).
     * A pool that closes cycles makes a survivor cheap, and the long tile pass only costs: C2 with cycle closing
     * 0.517 ms at 32, 0.583 ms at 96. */
    if (pool_runs_everything && p->precision == FR_PRECISION_F64 && npx >= ((size_t)1 << 24)) {
        int big = ((max_iter / 11 + kFastBlock / 2) / kFastBlock) * kFastBlock;
        big = big < 96 ? 96 : (big > 192 ? 192 : big);
        if (big > auto_first) auto_first = big;
    }
    const int first = t.stage_first ? (int)t.stage_first : auto_first;
    /* The second pass pays off where orbits are long.  Rounds 1-3: below max_iter ~768 (~384 on frames above 4K) ONE pass
     * whose waves stop at their home shard was faster -- 1080p at max_iter 256: 0.061 ms against 0.109 ms -- and above it
     * the two passes won by up to 35 % (profiles/r01_staging_crossover.txt).  Round 4's lane pool (deferred escapes) moved
     * the crossover down where escapes are spread out (profiles/r04_staging_crossover.txt, 168 cells): a Julia set wins
     * with two passes from max_iter 256 (-5 to -12 %; 384: -15 to -30 %; 512: -23 to -36 %), an fp64 Mandelbrot view
     * from 512 at every size up to 4K (-6 to -13 %; 384 on frames above 2^23 pixels as before: the default view loses 5-9 %
     * there, the Seahorse view wins 15-28 %), an fp32 one stays at 768 (512 above 2^23 pixels, where 384 lost 7-11 %).
     * An explicit "staging" or "stage_first" stages whenever there is room for two budgets. */
    const int auto_min = staging_threshold(p, npx);
    const bool forced = t.staging != 0 || t.stage_first != 0;
    *b0 = max_iter;
    if (allow && (forced ? max_iter >= 2 * first : max_iter >= auto_min)) {
        int b = first - first % kFastBlock;                      /* the budget is a multiple of the unchecked block */
        if (b < kFastBlock) b = kFastBlock;
        if (b < max_iter) *b0 = b;
    }
    return *b0 < max_iter ? 2 : 1;
}

/* occupancy exit of the lean tile pass (escape_run_lean): what a record costs the lane pool, in updates, and the updates a
 * trip runs before it may leave */
constexpr uint32_t kTileExitCost = 48u, kTileExitFrom = 32u;

constexpr uint32_t kWholeBlocksPerWave = 16u;     /* automatic "whole_blocks": blocks of the frame per lane-pool wave, at least */

enum Route { kRouteDirect = 1, kRouteDeepZoom, kRouteSsaaStaged, kRouteSsaaBanded };
enum Family { kGeneral, kGeneralEffects, kGeneralSampleLoop, kLean, kLeanStripes };

/* What enqueue_render decides before its first launch.  Of the SSAA routes and Deep_Zoom only the route part is filled:
 * their renders plan themselves (the sample grid as a direct render of its own, Deep_Zoom in launch_one_pass). */
struct RenderPlan {
    int route, family;
    uint32_t nbands, band_rows; /* kRouteSsaaBanded: bands of band_rows pixel rows (whole sub-tile rows), the last one shorter */
    int shape, tile_pixels;     /* FPW_LOG2 of the sub-tiles; lean kernels: sub-tiles per trip */
    int nstages, nstages_all;   /* 2: tile pass + lane pool; _all: what plan_stages answers for a pool that runs everything out */
    uint32_t wg_per_cu, grid, sgrid;   /* resident workgroups per CU of the tile kernel; workgroups of the tile pass / the lane-pool pass */
    uint32_t nregions, rotate_regions, region_blocks;   /* survivor stream: regions, blocks per region */
    size_t stream_bytes, coord_bytes;   /* the survivor stream; the coordinate tables of the lean kernels */
    /* the stream's second class (WholeRef, fr_kernels.hip.h): whether this render may write one -- whole_blocks_apply() has the
     * last word, it knows what the pool does -- and its buffer: every record goes to exactly one class, so the whole blocks
     * of a frame are at most its pixels / 64; a region that is full sends its trips through the ring, which holds them all */
    bool whole_may;
    uint32_t whole_region_blocks;
    size_t whole_bytes;
    bool f64, bounded, moderate;
    /* b0 and what follows from it, [0] for a pool that runs every survivor to max_iter, [1] for a pool that looks for cycles.
     * Whether it looks is the context's to say (pool_wants_cycle_closing, stateful), and only where pool_may_look. */
    bool pool_may_look;
    int b0[2];
    int32_t exit_from[2];
    uint32_t exit_cost, pool_refill_at, tile_period_window;   /* window != 0: the tile pass runs its samples to max_iter and closes cycles */
    QueueArgs tq, pq;           /* tile queue, pool queue (heads: the caller's) */

    bool staged() const { return nstages > 1; }
    bool lean() const { return family == kLean || family == kLeanStripes; }
    bool stripes() const { return family == kLeanStripes; }
    /* Whole blocks are written and read by the instantiations that hold the clean run -- the staged lean tile pass in front
     * of a lane pool that neither looks for cycles (pool_looks) nor shades stripes -- and by those alone: the others have no
     * loop that reads the class.  Row-strip shards and the sample grid of a staged SSAA frame are renders like any other here:
     * a record carries its pixel's place in the planes, and the conditions of a whole trip (full, inside the frame) are the
     * trip's own. */
    bool whole_blocks_apply(bool pool_looks) const { return whole_may && !pool_looks; }
};

inline RenderPlan plan_render(const Tuning& t, int compute_units, const fr_params* p, uint32_t W, uint32_t H, const fr_shard& norm,
                              uint32_t rows_local, int ssaa_of, bool out_frame = false)
{
    RenderPlan r = {};
    const bool julia = p->fractal_type == FR_FRACTAL_JULIA;
    const bool f64 = r.f64 = p->precision == FR_PRECISION_F64;
    const bool one_sample = p->antialiasing_samples <= 1;
    /* The Mandelbrot shader's effects need nothing along the orbit: stripe shading reads the z of the sample's last update, and
     * the orbit trap's minimum is the constant 0 (see shade_stripes: the first update makes z = c, and distToC is part of
     * the minimum).  Such frames take the lean tile pass and the lane pool in their code-3 instantiations instead of the
     * effects variant's lockstep run to max_iter with four running minima -- 8x8 sub-tiles, two per trip.  (Burning Ship's
     * trap and stripe sums are real accumulators: the effects variant keeps them.) */
    const bool stripes_lean = p->fractal_type == FR_FRACTAL_MANDELBROT && needs_effects(p) && t.stripes != 1u && t.tile_pixels != 1u;
    /* ssaa_of > 1: this IS the sample grid of a supersampled frame (direct, lean kernels only) */
    r.route = p->fractal_type == FR_FRACTAL_DEEP_ZOOM ? kRouteDeepZoom : kRouteDirect;
    if (r.route == kRouteDeepZoom) return r;
    /* SSAA.  The sample loop of the general tile kernel runs a pixel's aa x aa samples one after the other, each to max_iter
     * in lockstep with the 63 other pixels of its sub-tile: no compaction, no lane pool -- on escape-dense views a sample
     * costs 1.6-1.8x what a pixel of the same view costs without SSAA (profiles/r04_ssaa_staged.txt).  Staged: the sample
     * grid is a frame of W aa x H aa "pixels" whose coordinates are the samples' (prepare_kernel writes them into the lean
     * kernels' tables), rendered through tile pass + lane pool into scratch planes, and ssaa_reduce_kernel averages.  Same
     * arithmetic per sample, same summation order: bit-identical planes.  Applies where the lean kernels do (no effects,
     * 8x8 sub-tiles, strips of whole sub-tile rows in sample space) and the sample grid is a legal frame (< 2^31 samples). */
    if (ssaa_of <= 1 && !one_sample && (!needs_effects(p) || stripes_lean) && t.ssaa != 1u && lean_applies(t, norm, (uint32_t)p->antialiasing_samples)) {   /* (striped
                                                      sample grids too: their samples take the stripe instantiations) */
        const uint32_t aa = (uint32_t)p->antialiasing_samples;
        const uint64_t nsamples = (uint64_t)W * aa * (uint64_t)H * aa;
        /* (measured: -32 to -61 % on every view and size but the C2 frame with cycle closing off, +-2 %; also where the sample
         * grid takes ONE pass -- 1080p at max_iter 256: -38 % -- because the lean kernel beats the general one.  The sample
         * planes and the survivor stream of the sample grid are context scratch: 16 B + up to 60 B per sample; above 2^29
         * samples -- 8192^2 at aa 3 -- the sample loop stays.) */
        const uint64_t band_cap = t.ssaa_band ? t.ssaa_band : (1ull << 29);
        const bool fits = nsamples <= band_cap || (t.ssaa == 2u && !t.ssaa_band);
        if (fits && nsamples < (1ull << 31) && (uint64_t)norm.rows_per_strip * aa <= 0xFFFFFFFFull) { r.route = kRouteSsaaStaged; return r; }
        /* A WHOLE frame whose sample grid is larger (a print export: 8192^2 at aa 3 is 6e8 samples, 46 GB of sample planes and
         * survivor stream) goes through the same scratch band by band: contiguous bands of whole sub-tile rows, each rendered as
         * the one strip of "part b of B" straight into the caller's planes (FR_LAYOUT_FRAME addressing), one after the other on
         * the stream.  Same samples, same sums: bit-identical (test_staged_ssaa_is_bit_identical_to_the_sample_loop).  Row-strip shards keep the sample
         * loop above the cap: a band of a shard is not a shard. */
        if (!fits && norm.nparts == 1 && !out_frame && (uint64_t)W * aa * 8u * aa <= band_cap) {
            const uint64_t per_row = (uint64_t)W * aa * aa;                     /* samples per pixel row */
            r.band_rows = (uint32_t)(band_cap / per_row) & ~7u;                  /* whole sub-tile rows, >= 8 by the test above */
            if (r.band_rows > H) r.band_rows = (H + 7u) & ~7u;
            r.nbands = (H + r.band_rows - 1u) / r.band_rows;
            r.route = kRouteSsaaBanded;
            return r;
        }
    }

    const bool stripes = stripes_lean && one_sample && lean_applies(t, norm, 1);
    const bool effects = needs_effects(p) && !stripes;
    /* the lean tile kernel: every one-sample render without effects where lean_applies */
    const bool lean = !effects && one_sample && lean_applies(t, norm, 1);
    r.family = effects ? kGeneralEffects : stripes ? kLeanStripes : lean ? kLean : one_sample ? kGeneral : kGeneralSampleLoop;
    r.shape = t.shape ? (int)t.shape : 3;
    r.tile_pixels = !lean ? 0 : (stripes || t.tile_pixels != 1u) ? 2 : 1;
    const int max_iter = p->max_iterations;
    const size_t npx = (size_t)rows_local * W;
    r.nstages = plan_stages(t, p, effects, npx, false, &r.b0[1]);
    r.nstages_all = plan_stages(t, p, effects, npx, true, &r.b0[0]);
    const bool staged = r.staged();
    r.pool_may_look = staged && !stripes;                         /* (a closed cycle has no z after max_iter updates) */
    /* a pass that runs its samples to max_iter closes cycles in escape_run: SSAA (any shape; always compiled in) and
     * the one-sample kernel with 8x8 sub-tiles (its PERIOD instantiation, launch_tile); a staged tile pass hands its
     * survivors on */
    r.tile_period_window = !effects && !staged && !stripes ? period_window(t) : 0u;
    /* survivor-stream writers move to the next region after every block: the regions come out equally
     * long with the same mix of blocks, so the reading pass is balanced with little stealing (measured,
     * profiles/r01_region_rotation.txt: C2 0.883 -> 0.831 ms, C3 0.598 -> 0.539 ms; regions by XCD = 1) */
    r.rotate_regions = t.stream_rotate == 1u ? 0u : 1u;

    /* bounded, cheap items: the staged tile pass, and an unstaged pass whose samples run at most 128 updates
     * (measured at max_iter <= 32: 0.31 ms with short runs -- the queue words saturate -- 0.17 ms with long) */
    const int aa1 = one_sample ? 1 : p->antialiasing_samples;
    r.bounded = staged || (!effects && (long long)max_iter * aa1 * aa1 <= 128);
    /* items of moderate cost (an unstaged pass below the staging threshold): short runs as for unbounded items, but
     * the waves stop at their home shard -- the blocks of 16 sub-tiles dealt round-robin keep the shards level */
    r.moderate = !staged && !effects && (long long)max_iter * aa1 * aa1 < 768;
    /* The fp64 tile kernel holds 5 workgroups of 256 threads per CU (the per-wave timeline of the diag buffer
     * shows workgroups beyond the resident set only start when resident ones exit, and find the queue dry):
     * launch exactly the resident set.  Measured 5 vs 4: C2 +1.9 %, C3 +5.6 %, C5 +1.7 %; 6-8 (the one-sample
     * kernel fits 7 at 69 VGPRs) within 1 %. */
    /* the staged lean tile kernel in fp32 (52 VGPRs, 8.5 KB of LDS) holds 6: C3 -1.4 %
     * (fp32 only: the fp64 instantiation's 82 VGPRs leave room for 5 waves per SIMD) */
    r.wg_per_cu = !f64 && staged && lean ? 6u : 5u;
    r.tq = plan_tile_queue(t, compute_units, W, rows_local, r.shape, r.bounded, r.moderate, r.wg_per_cu, &r.grid);
    r.coord_bytes = lean ? ((size_t)W + H) * sizeof(double) : 0;
    if (!staged) return r;

    /* ---- lane-pool pass over the survivor stream ---------------------------------------------------- */
    /* the pool / stream kernels hold 6 workgroups per CU; their blocks are latency bound (dequeue -> record
     * loads -> iterate -> scattered stores), so run all of them */
    r.sgrid = (uint32_t)compute_units * (t.stream_wg_per_cu ? t.stream_wg_per_cu : 6u);
    {   /* small frames: at most one wave per 8 sub-tiles of the frame (every survivor block holds 64 records, and
         * a frame rarely leaves more than a quarter of its pixels alive after the tile pass: ~2 blocks per wave;
         * 1080p at max_iter 1024: 0.144 ms with 6 workgroups per CU, 0.128 ms with the 4 this cap gives) */
        const uint32_t per_wg = t.pool_items_per_wg ? t.pool_items_per_wg : 32u;
        const uint32_t cap = (r.tq.n_items + per_wg - 1u) / per_wg;
        if (r.sgrid > cap) r.sgrid = cap < 1u ? 1u : cap;
    }
    /* the survivor streams have as many regions as the tile queue has shards ("regions" overrides) */
    r.nregions = t.regions ? t.regions : (1u << r.tq.ns_log2);
    /* Survivor stream: blocks of 64 records {pixel u32, iterations done u32, nfields x T}.  Worst case: every
     * sample survives (npx/64 full blocks) + one partial block per writer wave; the regions of the stream hold
     * 1.5x that, so a region that fills up can spill into its neighbours. */
    const size_t block_bytes = 2 * 64 * 4 + (julia ? 2 : 4) * 64 * (f64 ? 8 : 4);
    const uint32_t worst_blocks = (uint32_t)((npx + 63) / 64) + (r.grid > r.sgrid ? r.grid : r.sgrid) * 4u + 16u;
    r.region_blocks = (worst_blocks * 3u / 2u + r.nregions - 1) / r.nregions + 1u;
    r.stream_bytes = (size_t)r.region_blocks * r.nregions * block_bytes;
    if (t.debug_region_blocks && t.debug_region_blocks < r.region_blocks) r.region_blocks = t.debug_region_blocks;
    /* Automatic: where it was measured to pay and never to cost (profiles/pool_whole_blocks.txt) -- fp64 frames with at least
     * kWholeBlocksPerWave blocks of 64 pixels per wave of the pool's grid.  A whole block is a coarse item: its wave runs all the
     * updates it has left before it claims again, so a frame that gives a wave only a block or two ends on a few waves that
     * hold one more than the others (1080p at max_iter 1024: 8 blocks of frame per wave, +37 %; 3840 x 2160: 21, -4.5 %;
     * C2: 42, -2.5 %); fp32 views were measured on the C3 dust alone (+1.9 %) and stay with one class. */
    const bool whole_auto = f64 && (npx + 63) / 64 >= (size_t)kWholeBlocksPerWave * r.sgrid * 4u;
    r.whole_may = lean && !stripes && (t.whole_blocks == 2u || (t.whole_blocks == 0u && whole_auto));
    if (r.whole_may) {
        r.whole_region_blocks = (((uint32_t)((npx + 63) / 64) + r.nregions - 1) / r.nregions + 3u) & ~1u;   /* even: claims are pairs */
        r.whole_bytes = (size_t)r.whole_region_blocks * r.nregions * block_bytes;
        if (t.debug_region_blocks && t.debug_region_blocks < r.whole_region_blocks) r.whole_region_blocks = t.debug_region_blocks & ~1u;
    }
    if (lean && t.tile_exit != 1u) {
        r.exit_cost = t.tile_exit ? t.tile_exit : kTileExitCost;
        for (int k = 0; k < 2; ++k) {
            /* not in the first half of the budget (C5, b0 192: 4.22 -> 4.09 ms leaving from 64, 4.06 from 96; C2, b0 96: +-0.3 %
             * whatever the rule -- profiles/r04_tile_occupancy_exit.txt) */
            const uint32_t half = ((uint32_t)r.b0[k] / 2u + 15u) / 16u * 16u;
            r.exit_from[k] = (int32_t)(t.tile_exit_from ? t.tile_exit_from : (half > kTileExitFrom ? half : kTileExitFrom));
        }
    }
    r.pq.ns_log2 = r.nregions == (uint32_t)kMaxShards ? 6u : 3u;   /* region r of the input stream is shard r of this queue */
    const uint32_t swps = (r.sgrid * 4u + r.nregions - 1) / r.nregions;
    r.pq.run_shift = clamp_shift(t, (int)ceil_log2(2u * swps));
    /* a lane-pool wave holds its claimed blocks as a private reserve and only stalls for a dequeue
     * once per reserve, so claim little and never ahead: what a wave has reserved when the queue
     * runs dry is exactly the tail of the pass (measured: 1-3 block runs + one run prefetched left
     * a 315 us drain on C2; a block of 64 interior records is ~60 us of work at 5 waves/SIMD).
     * ONE block per claim since round 3 (runs of 1-2 before): C2 -3.1 %, 1080p/1024 -0.9 %, C3 / C5 / C4 within
     * +-1 % (profiles/r03_b0_and_pool_tuning.txt) */
    r.pq.run_min = t.stream_run_min ? t.stream_run_min : 1u;
    r.pq.run_max = t.stream_run_max ? t.stream_run_max : 1u;
    if (r.pq.run_min > r.pq.run_max) r.pq.run_min = r.pq.run_max;
    uint32_t probes = t.stream_probes ? t.stream_probes : (r.rotate_regions ? 4u : 0u);
    if (r.sgrid < 64u || r.sgrid < r.nregions) probes = 0;
    r.pq.flags = probes << kQueueProbeShift;
    /* finished lanes wait until this many are idle: 24 in fp32, 16 in fp64 (where a retire + refill round is cheaper
     * relative to an update: C5 -1.5 %, 1080p/1024 -1.8 %, C2 / C4 unchanged; the fp32 dust +1.5 % with 16) */
    r.pool_refill_at = t.pool_refill ? t.pool_refill : (f64 ? 16u : 24u);
    if (r.pool_refill_at > 64u) r.pool_refill_at = 64u;
    return r;
}

}  /* namespace fr */
#endif /* FR_PLAN_H */
