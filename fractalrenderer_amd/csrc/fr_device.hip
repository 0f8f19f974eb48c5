/*
 * fr_device.hip -- context, launch logic and the render entry points of the C ABI
 * (include/fractalrenderer_amd.h).  The kernels are in fr_kernels.hip.h.
 *
 * Replaces, for the hot path only:
 *   ComputeEffectManager::dispatch          src/compute_effect_manager.h:435-468
 *   VulkanEngine::render_animation_frame    src/vk_engine.cpp:1181-1418 (render + readback part)
 * There is no CPU fallback in this file: without a HIP device every call fails.
 */
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>

#include "fr_kernels.hip.h"
#include "fr_phoenix.hip.h"
#include "fr_mandelbulb.hip.h"
#include "fr_deep.hip.h"
#include "fr_deep_phoenix.hip.h"
#include "fr_deepseq.hip.h"
#include "fr_tuning.h"
#include "fr_plan.h"

using namespace fr;

static constexpr int kMaxStages = 2;            /* tile pass (+ lane-pool pass) */
static constexpr size_t kStageWords = (size_t)2 * kMaxShards * kShardStrideWords;   /* one stage: its queue heads, then its stream counters */
/* behind the stages, in their layout: the second class of the survivor stream (WholeRef) -- its queue heads and block counters,
 * then its two groups of read-out words; zeroed with the stages in front of every render that writes the class */
static constexpr int kWholeStage = kMaxStages, kWholeStages = 2;
static constexpr size_t kCtrlWords = (size_t)(kMaxStages + kWholeStages) * kStageWords;
static constexpr size_t kReadyWord = kCtrlWords + (size_t)(kFeedbackShards + 1) * kShardStrideWords;   /* LaunchArgs::pro_ready */
static constexpr size_t kFeedbackWord = kCtrlWords;            /* behind the stages: Feedback::dev_flag (kFeedbackShards words, 128 B apart) */
static constexpr uint32_t kProbeEvery = 16;                     /* frames between two looks of a view that closed nothing */

/* what a cached reference orbit was computed for (orbit_key_matches / orbit_key_store) */
struct OrbitKey {
    bool valid;                 /* the key describes the orbit on the device */
    char* x;                    /* centre strings (malloc'd copies) */
    char* y;
    int32_t bits, max_iter;
    float bailout;              /* compared by its bits */
    uint64_t c_bits[2];         /* Julia: the bits of c; Phoenix: the bits of its floats p and r (0 in the other formulas' slots) */
};

/* the formula of a deep view: the index of its cache slots */
enum { kMandel = 0, kShip = 1, kJulia = 2, kPhoenix = 3, kFormulas = 4 };

/* One cache slot of reference orbits of deep views: the buffers and what they hold */
struct DeepOrbit {
    char* host;                 /* pinned upload buffer, cap points */
    char* dev;
    size_t cap;
    int32_t len;                /* N + 1 (a Julia slot: of Q, at point 0; P lies cap / 2 points behind it) */
    int32_t len_p;              /* a Julia slot: N_P + 1 */
    OrbitKey key;               /* of dev */
    uint64_t gen;               /* bumped whenever dev receives another orbit */
};

/* One BLA table of a cached orbit, and the step counts of the most recent render with its flag */
struct BlaSlot {
    void* r;                    /* r of every entry (cap): doubles, or XRad in an extended table */
    double2* ab;                /* (A, B) of every entry (the formula's kAbPerEntry times cap); extended: their mantissas */
    int2* abe;                  /* extended: their exponents (cap); a Julia slot: A's alone, an int32 per entry */
    size_t cap;                 /* entries (a Julia slot: of both tables, Q's first) */
    bool valid;                 /* the key below describes the table */
    uint64_t key_gen, key_dcv;  /* gen of its orbit; bits of dcmax, extended: of dcmax's mantissa (a Julia slot: 0, no dcmax) */
    int32_t key_dce;            /* extended: dcmax's exponent */
    uint64_t builds;            /* how often the table has been built (tests: fr_deep_bla_builds) */
    unsigned long long* steps_dev;     /* the kernel's three counters */
    unsigned long long* steps_host;    /* pinned: their copy behind the most recent render with the flag */
    bool have_steps;
    hipEvent_t ev;              /* recorded behind every render with the flag (not while capturing): rebuilds wait for it */
    bool ev_valid;
};

/* What the context keeps for one deep path, a (storage, formula) pair: its most recent reference orbit(s), their BLA table, and
 * the resident workgroups per CU of the deep_kernel instantiations that read them (0 = not asked yet): [0] the path's own pair,
 * [1] the distance entry point's that shares the slot -- fr_render_deep_de's the fp64 Mandelbrot slot, fr_render_deepx_de's the
 * extended one, fr_render_deep_julia_de's and fr_render_deepx_julia_de's the two Julia slots, fr_render_deep_ship_de's and
 * fr_render_deepx_ship_de's the two ship slots;
 * [.][0] the unflagged kernel, [.][1] the flagged one */
struct DeepSlot {
    DeepOrbit o;
    BlaSlot t;
    int wg_per_cu[2][2];
};

struct fr_ctx {
    int device;
    int compute_units;
    hipStream_t stream;
    hipEvent_t ev_begin, ev_end;
    bool have_timing;           /* ev_begin / ev_end hold the most recent render (only recorded with "timing" on) */
    bool timing;                /* option "timing": record the event pair around every render (fr_ctx_last_kernel_ms).  Off by
                                 * default since 1.1: two timed event records cost a frame ~4.7 us (C2 0.6 %, C3 1.8 %, a 1080p
                                 * frame at max_iter 256 10 %: profiles/r04_timing_events.txt) */
    bool have_render;           /* a render has been enqueued: last_stream is where */
    hipStream_t last_stream;    /* the stream of the most recent render */
    hipEvent_t ev_order;        /* no timing: recorded on last_stream when somebody has to wait for that render */
    uint32_t* d_ctrl;           /* queue heads + stream counters of every stage (kCtrlWords) */
    void* frame_buf;            /* fr_render_frame_png: RGBA f32 frame + RGB8 */
    size_t frame_bytes;
    void* orbit_host;           /* Deep_Zoom: pinned staging (fp64 orbit + its float narrowing) */
    float* orbit_dev;           /* Deep_Zoom: reference orbit as float pairs */
    size_t orbit_cap;           /* capacity in scalars (2 per orbit point) */
    void* stream_buf;           /* survivor stream (tile pass -> lane pool) */
    size_t stream_bytes;
    void* whole_buf;            /* its second class: whole blocks (WholeRef) */
    size_t whole_bytes;
    uint32_t last_whole_cap;    /* the most recent render wrote that class, in regions of this many blocks (0: it did not) */
    Tuning tune;                /* fr_ctx_set_tuning and the scheduling names of fr_ctx_set_option (fr_plan.h) */
    size_t diag_stride;         /* words between the diag regions of consecutive stages */
    int last_stages;
    uint64_t* diag;             /* optional device buffer for per-wave timelines */
    uint32_t last_grid;
    void* scratch;              /* device staging for FR_MEM_HOST outputs */
    size_t scratch_bytes;
    double2* log2_tab;          /* device copy of the log2 table of the fp64 smooth-count epilogue (log2_tab()) */
    float* export8_thr;         /* device: 256 x {t[b], t[b + 1]}, the byte thresholds of the 8-bit export (fr_export8_thresholds) */
    void* coord_buf;            /* lean tile pass: W + H coordinates of the frame being rendered (prepare_kernel) */
    size_t coord_bytes;
    void* ssaa_buf;             /* staged SSAA: the sample planes (colour [+ nu] [+ iter]), grow-only */
    size_t ssaa_bytes;
    uint32_t* overflow_host;    /* pinned, device-mapped word: a survivor stream ran out of blocks (see StreamRef::overflow) */
    uint32_t* overflow_dev;     /* the same word as the kernels address it */
    bool render_on_user_stream; /* the most recent render was enqueued on a caller's stream: ev_end orders the context's
                                 * own stream (exports, colorize) behind it */
    /* automatic cycle closing of the lane pool (pool_wants_cycle_closing) */
    uint32_t render_seq;        /* renders enqueued on this context */
    uint32_t prologue_epoch;    /* lean tile passes launched with the in-kernel prologue (lean_prologue): 28 bits */
    uint64_t probe_key;         /* what the context renders (fractal, precision, max_iter, geometry, coarse view) */
    int probe_mode;             /* 0 LOOK: every render's pool looks; 1 SKIP: none does, skip_left to go; 2 WAIT: one look is in
                                 * flight (render probe_seq), nobody else looks until its verdict is back */
    uint32_t probe_first;       /* LOOK: first render of the run of looks; WAIT: the one look */
    uint32_t skip_left;
    int last_pool_closing;      /* the most recent render's lane pool looked for cycles (1) / did not (0) / there was none (-1) */
    struct DivCheck { bool valid, julia, f64, ok; uint32_t W, H; };
    DivCheck div_cache[8];      /* exact_division_ok() results */
    uint32_t div_next;
    uint32_t fold_div_w, fold_div_rows;   /* fold_div_ok() held for frames this wide of up to this many rendered rows */
    uint32_t last_fold;         /* rows the most recent render rendered as a folded render (fr_plan.h: plan_fold); 0: it was not one */
    int phoenix_wg_per_cu[2];   /* resident workgroups per CU of phoenix_kernel<float> / <double> (0 = not asked yet) */
    int mandelbulb_wg_per_cu[2];  /* ... of mandelbulb_kernel<false> / <true> (0 = not asked yet) */
    /* deep views: one slot per path, deep[storage][formula] (deep_slot()).  Storage 0, plain doubles Z_0 .. Z_N in one pinned and
     * one device block of cap double2: fr_render_deep (and fr_render_deep_de), fr_render_deep_ship, fr_render_deep_julia with
     * the tables of FR_FLAG_DEEP_BLA, FR_FLAG_DEEP_SHIP_BLA, FR_FLAG_DEEP_JULIA_BLA.  Storage 1, the extended storage, one
     * pinned and one device block of cap points each -- the plain doubles, the mantissa pairs, the exponents, in this order:
     * fr_render_deepx, fr_render_deepx_ship, fr_render_deepx_julia and the sequences, with the tables of FR_FLAG_DEEPX_BLA,
     * FR_FLAG_DEEPX_SHIP_BLA, FR_FLAG_DEEPX_JULIA_BLA.  The six paths share nothing.  A Julia slot holds two orbits: Q in the
     * first half of every array, P in the second.  A seventh slot, deep[0][kPhoenix], is fr_render_deep_phoenix's: plain doubles,
     * with the table of FR_FLAG_DEEP_PHOENIX_BLA; an eighth, deep[1][kPhoenix], is fr_render_deepx_phoenix's: the extended
     * storage, with the table of FR_FLAG_DEEPX_PHOENIX_BLA. */
    DeepSlot deep[2][kFormulas];
};

static DeepSlot& deep_slot(fr_ctx* c, bool ext, int f) { return c->deep[ext ? 1 : 0][f]; }

#define FR_HIP_TRY(expr)                                                               \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fr_set_error(FR_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

extern "C" int fr_ctx_create(int device_ordinal, fr_ctx** out)
{
    if (!out) return fr_set_error(FR_ERR_INVALID_ARG, "fr_ctx_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fr_set_error(FR_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                            e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device_ordinal < 0 || device_ordinal >= ndev)
        return fr_set_error(FR_ERR_NO_DEVICE, "device ordinal %d out of range [0,%d)", device_ordinal, ndev);
    FR_HIP_TRY(hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    FR_HIP_TRY(hipGetDeviceProperties(&prop, device_ordinal));

    fr_ctx* c = (fr_ctx*)calloc(1, sizeof(fr_ctx));
    if (!c) return fr_set_error(FR_ERR_NOMEM, "out of host memory");
    c->device = device_ordinal;
    c->compute_units = prop.multiProcessorCount;
    /* log2 table: bin i of [0.5, 1) has midpoint m_i = 0.5 + (i + 0.5) / 256; entry = {y_i = RN(1 / m_i), -log2(y_i)}.
     * The logarithm is taken of the ROUNDED reciprocal (in 64-bit long double), so that m = (1 + r) / y_i holds for
     * the r the kernels compute and the table contributes no error of its own beyond its final rounding. */
    double tab[2 * kLog2Entries];
    for (int i = 0; i < kLog2Entries; ++i) {
        const double m = 0.5 + ((double)i + 0.5) / (2.0 * kLog2Entries);
        const double y = 1.0 / m;
        tab[2 * i] = y;
        tab[2 * i + 1] = (double)(-log2l((long double)y));
    }
    /* byte thresholds of the 8-bit export as the pairs the kernel reads: {t[b], t[b + 1]} */
    float t8[257], pairs[512];
    fr_export8_thresholds(t8);
    for (int b = 0; b < 256; ++b) { pairs[2 * b] = t8[b]; pairs[2 * b + 1] = t8[b + 1]; }
    auto slot_events = [c] {                     /* the event of every deep slot's table (BlaSlot::ev) */
        for (auto& storage : c->deep)
            for (DeepSlot& s : storage) {
                const hipError_t e = hipEventCreateWithFlags(&s.t.ev, hipEventDisableTiming);
                if (e != hipSuccess) return e;
            }
        return hipSuccess;
    };
    hipError_t e2;
    if ((e2 = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e2 = hipEventCreate(&c->ev_begin)) != hipSuccess ||
        (e2 = hipEventCreate(&c->ev_end)) != hipSuccess ||
        (e2 = hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming)) != hipSuccess ||
        (e2 = slot_events()) != hipSuccess ||
        (e2 = hipMalloc((void**)&c->d_ctrl, (kCtrlWords + (size_t)(kFeedbackShards + 2) * kShardStrideWords) * sizeof(uint32_t))) != hipSuccess ||
        (e2 = hipMemset(c->d_ctrl, 0, (kCtrlWords + (size_t)(kFeedbackShards + 2) * kShardStrideWords) * sizeof(uint32_t))) != hipSuccess ||
        (e2 = hipHostMalloc((void**)&c->overflow_host, 64, hipHostMallocMapped)) != hipSuccess ||
        (e2 = hipHostGetDevicePointer((void**)&c->overflow_dev, c->overflow_host, 0)) != hipSuccess ||
        (e2 = hipMalloc((void**)&c->log2_tab, sizeof(tab))) != hipSuccess ||
        (e2 = hipMemcpy(c->log2_tab, tab, sizeof(tab), hipMemcpyHostToDevice)) != hipSuccess ||
        (e2 = hipMalloc((void**)&c->export8_thr, sizeof(pairs))) != hipSuccess ||
        (e2 = hipMemcpy(c->export8_thr, pairs, sizeof(pairs), hipMemcpyHostToDevice)) != hipSuccess) {
        fr_ctx_destroy(c);                       /* releases whatever was created */
        return fr_set_error(FR_ERR_HIP, "context setup failed: %s", hipGetErrorString(e2));
    }
    c->overflow_host[0] = 0u;
    c->overflow_host[1] = 0u;                    /* the feedback word (Feedback::host_word) */
    *out = c;
    return FR_OK;
}

/* Also the unwinding path of a failed fr_ctx_create: every member may still be NULL. */
extern "C" void fr_ctx_destroy(fr_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();                /* renders of this context may have been enqueued on callers' streams */
    if (c->scratch) (void)hipFree(c->scratch);
    if (c->d_ctrl) (void)hipFree(c->d_ctrl);
    if (c->overflow_host) (void)hipHostFree(c->overflow_host);
    if (c->log2_tab) (void)hipFree(c->log2_tab);
    if (c->export8_thr) (void)hipFree(c->export8_thr);
    if (c->coord_buf) (void)hipFree(c->coord_buf);
    if (c->ssaa_buf) (void)hipFree(c->ssaa_buf);
    if (c->stream_buf) (void)hipFree(c->stream_buf);
    if (c->whole_buf) (void)hipFree(c->whole_buf);
    if (c->frame_buf) (void)hipFree(c->frame_buf);
    if (c->orbit_host) (void)hipHostFree(c->orbit_host);
    if (c->orbit_dev) (void)hipFree(c->orbit_dev);
    for (auto& storage : c->deep)
        for (DeepSlot& s : storage) {
            if (s.o.host) (void)hipHostFree(s.o.host);
            if (s.o.dev) (void)hipFree(s.o.dev);
            free(s.o.key.x);
            free(s.o.key.y);
            if (s.t.r) (void)hipFree(s.t.r);
            if (s.t.ab) (void)hipFree(s.t.ab);
            if (s.t.abe) (void)hipFree(s.t.abe);
            if (s.t.steps_dev) (void)hipFree(s.t.steps_dev);
            if (s.t.steps_host) (void)hipHostFree(s.t.steps_host);
            if (s.t.ev) (void)hipEventDestroy(s.t.ev);
        }
    if (c->ev_begin) (void)hipEventDestroy(c->ev_begin);
    if (c->ev_end) (void)hipEventDestroy(c->ev_end);
    if (c->ev_order) (void)hipEventDestroy(c->ev_order);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    free(c);
}

extern "C" int fr_ctx_compute_units(fr_ctx* c)
{
    if (!c) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL");
    return c->compute_units;
}

/* Options a caller needs, by name; value 0 restores the automatic choice (include/fractalrenderer_amd.h). */
extern "C" int fr_ctx_set_option(fr_ctx* c, const char* name, int64_t value)
{
    if (!c || !name) return fr_set_error(FR_ERR_INVALID_ARG, "ctx/name is NULL");
    const int st = option_set(c->tune, name, value);
    if (st != kNotMine) return st;               /* periodicity, staging, shards, tile_kernel */
    if (!strcmp(name, "timing")) {
        if (value < 0 || value > 1) return fr_set_error(FR_ERR_INVALID_ARG, "timing must be 0 (off) or 1 (an event pair around every render: fr_ctx_last_kernel_ms)");
        c->timing = value != 0;
        if (!c->timing) c->have_timing = false;
    } else if (!strcmp(name, "diag_buffer")) {
        c->diag = (uint64_t*)(uintptr_t)value;        /* device pointer, 4 x u64 per wave of the grid; 0 = off */
    } else if (!strcmp(name, "diag_stride")) {
        c->diag_stride = (size_t)value;               /* u64 words between the diag regions of consecutive stages */
    } else if (!strcmp(name, "pool") || !strcmp(name, "stage_ratio") || !strcmp(name, "pool_evict_at") ||
               !strcmp(name, "pool_passes") || !strcmp(name, "queue_flags")) {
        /* retired with the schedules they steered (fresh-pixel pool, block stages, eviction passes): accepted, ignored */
    } else {
        return fr_set_error(FR_ERR_INVALID_ARG, "unknown option '%s' (queue / stream tuning names moved to fr_ctx_set_tuning, "
                                                "fractalrenderer_amd/csrc/fr_tuning.h)", name);
    }
    return FR_OK;
}

/* Tuning knobs of the persistent queues and the survivor stream (fr_tuning.h: tests, tools/ and A/B measurements; not part
 * of the public header).  None of them can change a pixel. */
extern "C" int fr_ctx_set_tuning(fr_ctx* c, const char* name, int64_t value)
{
    if (!c || !name) return fr_set_error(FR_ERR_INVALID_ARG, "ctx/name is NULL");
    if (!strcmp(name, "debug_prologue_epoch")) {
        if (value < 0 || value > 0x0FFFFFFF) return fr_set_error(FR_ERR_INVALID_ARG, "debug_prologue_epoch: 28 bits");
        c->prologue_epoch = (uint32_t)value;          /* tests only: the epoch of the next in-kernel prologue is this + 1 */
    }
    const int st = strcmp(name, "debug_prologue_epoch") ? tuning_set(c->tune, name, value) : FR_OK;
    return st == kNotMine ? fr_set_error(FR_ERR_INVALID_ARG, "unknown tuning name '%s'", name) : st;
}

/* workgroups of 256 threads per launch of the most recent render; bits 16.. = number of stages */
extern "C" int fr_ctx_last_grid(fr_ctx* c)
{
    if (!c) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL");
    return (int)(c->last_grid | ((uint32_t)c->last_stages << 16));
}

extern "C" float fr_ctx_last_kernel_ms(fr_ctx* c)
{
    if (!c || !c->have_timing) return -1.0f;
    if (hipSetDevice(c->device) != hipSuccess) return -1.0f;
    if (hipEventSynchronize(c->ev_end) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, c->ev_begin, c->ev_end) != hipSuccess) return -1.0f;
    return ms;
}

/* ---- launch ---------------------------------------------------------------------------------- */

/* The kernels map pixel -> plane coordinate with  q' = fma(a - b*RN(a*y) , y, RN(a*y)),  y = RN(1/b)
 * instead of the as-written IEEE divide a / b (Markstein's correction step).  That is the
 * correctly rounded quotient in all but exotic cases; rather than rely on the theorem's side
 * conditions, evaluate the identical expression here for EVERY numerator the frame uses (one per
 * column, one per row) and allow the divide-free path only if all of them equal a / b.
 * Result cached per (W, H, fractal, precision). */
template <typename T>
static bool quotients_exact(uint32_t W, uint32_t H, bool julia)
{
    const T resx = (T)W, resy = (T)H;
    const T inv_w = (T)1 / resx, inv_h = (T)1 / resy;
    auto same = [](T a, T b, T rb) {
        const T q = a * rb;
        const T r = std::fma(-q, b, a);
        return std::fma(r, rb, q) == a / b;
    };
    if (julia) {                                   /* shaders/julia.comp:325  uv = pix / size */
        for (uint32_t x = 0; x < W; ++x) if (!same((T)x, resx, inv_w)) return false;
        for (uint32_t y = 0; y < H; ++y) if (!same((T)y, resy, inv_h)) return false;
    } else {                                       /* shaders/mandelbrot.comp:150  (pix - 0.5 res) / res.y */
        for (uint32_t x = 0; x < W; ++x) if (!same((T)x - (T)0.5 * resx, resy, inv_h)) return false;
        for (uint32_t y = 0; y < H; ++y) if (!same((T)y - (T)0.5 * resy, resy, inv_h)) return false;
    }
    return true;
}

static bool exact_division_ok(fr_ctx* c, uint32_t W, uint32_t H, bool julia, bool f64)
{
    for (int k = 0; k < 8; ++k) {
        const fr_ctx::DivCheck& d = c->div_cache[k];
        if (d.valid && d.W == W && d.H == H && d.julia == julia && d.f64 == f64) return d.ok;
    }
    const bool ok = f64 ? quotients_exact<double>(W, H, julia) : quotients_exact<float>(W, H, julia);
    fr_ctx::DivCheck& slot = c->div_cache[c->div_next++ & 7];
    slot.valid = true; slot.W = W; slot.H = H; slot.julia = julia; slot.f64 = f64; slot.ok = ok;
    return ok;
}

template <typename T, int FRACTAL, bool EFFECTS, bool SSAA>
static hipError_t launch_tile_aa(int shape, dim3 grid, hipStream_t s, const LaunchArgs& a)
{
    switch (shape) {
    case 6: hipLaunchKernelGGL((tile_kernel<T, FRACTAL, 6, EFFECTS, SSAA>), grid, dim3(kBlockThreads), 0, s, a); break;
    case 4: hipLaunchKernelGGL((tile_kernel<T, FRACTAL, 4, EFFECTS, SSAA>), grid, dim3(kBlockThreads), 0, s, a); break;
    default: hipLaunchKernelGGL((tile_kernel<T, FRACTAL, 3, EFFECTS, SSAA>), grid, dim3(kBlockThreads), 0, s, a); break;
    }
    return hipGetLastError();
}

template <typename T, int FRACTAL, bool EFFECTS>
static hipError_t launch_tile(int shape, dim3 grid, hipStream_t s, const LaunchArgs& a)
{
    if constexpr (!EFFECTS) {
        /* one-sample pass run to max_iter with cycle closing on: its own variant (8x8 sub-tiles only), so that the
         * default kernel does not carry the snapshot registers */
        if (a.aa <= 1 && a.period_window && shape == 3) {
            hipLaunchKernelGGL((tile_kernel<T, FRACTAL, 3, false, false, true>), grid, dim3(kBlockThreads), 0, s, a);
            return hipGetLastError();
        }
    }
    return a.aa > 1 ? launch_tile_aa<T, FRACTAL, EFFECTS, true>(shape, grid, s, a)
                    : launch_tile_aa<T, FRACTAL, EFFECTS, false>(shape, grid, s, a);
}

template <typename T, int FRACTAL>
static hipError_t launch_tile_lean(int np, dim3 grid, hipStream_t s, const LaunchArgs& a)
{
    if constexpr (FRACTAL == 0) {
        if (a.fold_rows) {                       /* a folded render (plan_fold): the same kernels with the mirrored stores */
            const bool w = a.whole.base != nullptr, pw = a.period_window != 0u;
            if (w && np == 2) hipLaunchKernelGGL((tile_lean_kernel<T, 0, false, 2 + kWholeTrips + kFoldTrips>), grid, dim3(kBlockThreads), 0, s, a);
            else if (w) hipLaunchKernelGGL((tile_lean_kernel<T, 0, false, 1 + kWholeTrips + kFoldTrips>), grid, dim3(kBlockThreads), 0, s, a);
            else if (np == 2 && pw) hipLaunchKernelGGL((tile_lean_kernel<T, 0, true, 2 + kFoldTrips>), grid, dim3(kBlockThreads), 0, s, a);
            else if (np == 2) hipLaunchKernelGGL((tile_lean_kernel<T, 0, false, 2 + kFoldTrips>), grid, dim3(kBlockThreads), 0, s, a);
            else if (pw) hipLaunchKernelGGL((tile_lean_kernel<T, 0, true, 1 + kFoldTrips>), grid, dim3(kBlockThreads), 0, s, a);
            else hipLaunchKernelGGL((tile_lean_kernel<T, 0, false, 1 + kFoldTrips>), grid, dim3(kBlockThreads), 0, s, a);
            return hipGetLastError();
        }
    }
    if (a.whole.base) {                         /* (staged, no cycle closing in the tile pass: plan_render) */
        if (np == 2) hipLaunchKernelGGL((tile_lean_kernel<T, FRACTAL, false, 2 + kWholeTrips>), grid, dim3(kBlockThreads), 0, s, a);
        else hipLaunchKernelGGL((tile_lean_kernel<T, FRACTAL, false, 1 + kWholeTrips>), grid, dim3(kBlockThreads), 0, s, a);
    } else if (np == 2) {
        if (a.period_window)
            hipLaunchKernelGGL((tile_lean_kernel<T, FRACTAL, true, 2>), grid, dim3(kBlockThreads), 0, s, a);
        else
            hipLaunchKernelGGL((tile_lean_kernel<T, FRACTAL, false, 2>), grid, dim3(kBlockThreads), 0, s, a);
    } else {
        if (a.period_window)
            hipLaunchKernelGGL((tile_lean_kernel<T, FRACTAL, true, 1>), grid, dim3(kBlockThreads), 0, s, a);
        else
            hipLaunchKernelGGL((tile_lean_kernel<T, FRACTAL, false, 1>), grid, dim3(kBlockThreads), 0, s, a);
    }
    return hipGetLastError();
}

/* the Mandelbrot shader's effects through the lean kernels (kernel code FRACTAL = 3, shade_stripes): two sub-tiles per trip, no cycle closing */
template <typename T>
static hipError_t launch_tile_lean_stripes(dim3 grid, hipStream_t s, const LaunchArgs& a)
{
    hipLaunchKernelGGL((tile_lean_kernel<T, 3, false, 2>), grid, dim3(kBlockThreads), 0, s, a);
    return hipGetLastError();
}
template <typename T>
static hipError_t launch_pool_stripes(dim3 grid, hipStream_t s, const LaunchArgs& a)
{
    hipLaunchKernelGGL((pool_kernel<T, 3, false>), grid, dim3(kBlockThreads), 0, s, a);
    return hipGetLastError();
}

/* control block + coordinate tables of a lean render (prepare_kernel) */
template <typename T, int FRACTAL>
static hipError_t launch_prepare(hipStream_t s, const LaunchArgs& a, uint32_t* ctrl, uint32_t n_ctrl, const Feedback& fb)
{
    const uint32_t n = (uint32_t)(a.W + a.H) > n_ctrl ? (uint32_t)(a.W + a.H) : n_ctrl;
    const dim3 grid((n + kBlockThreads - 1) / kBlockThreads);
    hipLaunchKernelGGL((prepare_kernel<T, FRACTAL == 0 ? 0 : 1>), grid, dim3(kBlockThreads), 0, s, a, ctrl, n_ctrl, fb);
    return hipGetLastError();
}

template <typename T, int FRACTAL>
static hipError_t launch_stream_pool(dim3 grid, hipStream_t s, const LaunchArgs& a)
{
    if constexpr (FRACTAL == 0) {
        if (a.fold_rows) {                       /* a folded render (plan_fold): the same kernels with the mirrored stores */
            if (a.period_window) hipLaunchKernelGGL((pool_kernel<T, kFoldPool, true>), grid, dim3(kBlockThreads), 0, s, a);
            else if (a.whole.base) hipLaunchKernelGGL((pool_kernel<T, kWholePool + kFoldPool, false>), grid, dim3(kBlockThreads), 0, s, a);
            else hipLaunchKernelGGL((pool_kernel<T, kFoldPool, false>), grid, dim3(kBlockThreads), 0, s, a);
            return hipGetLastError();
        }
    }
    if (a.period_window)
        hipLaunchKernelGGL((pool_kernel<T, FRACTAL, true>), grid, dim3(kBlockThreads), 0, s, a);
    else if (a.whole.base)                       /* the stream has two classes (plan_render: never with cycle closing) */
        hipLaunchKernelGGL((pool_kernel<T, FRACTAL + kWholePool, false>), grid, dim3(kBlockThreads), 0, s, a);
    else
        hipLaunchKernelGGL((pool_kernel<T, FRACTAL, false>), grid, dim3(kBlockThreads), 0, s, a);
    return hipGetLastError();
}

/* run fn(T{}, integral_constant<int, FRACTAL>{}) for the runtime (fractal, precision) */
template <class Fn>
static hipError_t by_variant(int fractal, bool f64, Fn&& fn)
{
    using std::integral_constant;
    switch (fractal) {
    case FR_FRACTAL_JULIA:        return f64 ? fn(double{}, integral_constant<int, 1>{}) : fn(float{}, integral_constant<int, 1>{});
    case FR_FRACTAL_BURNING_SHIP: return f64 ? fn(double{}, integral_constant<int, 2>{}) : fn(float{}, integral_constant<int, 2>{});
    default:                      return f64 ? fn(double{}, integral_constant<int, 0>{}) : fn(float{}, integral_constant<int, 0>{});
    }
}

/* control block in device memory, zeroed by ONE memset per render:
 *   words [s * kStageWords, + kMaxShards * 32): the (8 or 64) queue heads of stage s, 128 B apart
 *   the next kMaxShards * 32 words: the (8 or 64) region counters of the survivor stream written by stage s */
static uint32_t* stage_heads(fr_ctx* c, int s) { return c->d_ctrl + (size_t)s * kStageWords; }
static uint32_t* stage_counter(fr_ctx* c, int s) { return c->d_ctrl + (size_t)s * kStageWords + (size_t)kMaxShards * kShardStrideWords; }

/* A survivor stream that ran out of blocks (StreamRef::overflow) loses pixels: report it as a failed render at the
 * next point where the host knows the kernels are done.  Sticky until reported. */
static int check_overflow(fr_ctx* c)
{
    if (__atomic_load_n(c->overflow_host, __ATOMIC_RELAXED) == 0u) return FR_OK;
    __atomic_store_n(c->overflow_host, 0u, __ATOMIC_RELAXED);
    return fr_set_error(FR_ERR_INTERNAL, "a kernel reported an internal error (a survivor stream overflowed, or a lane-pool wave "
                                         "gave up on a stretch that would not end): the frame of the last render on this context "
                                         "is incomplete, please report the parameters");
}

/* what the first launch of a render forwards from the previous one (see Feedback) */
static Feedback feedback_of(fr_ctx* c)
{
    Feedback fb;
    fb.dev_flag = c->d_ctrl + kFeedbackWord;
    fb.host_word = c->overflow_dev + 1;
    fb.prev_seq = c->render_seq;                 /* the caller increments render_seq after its launches */
    return fb;
}

/* Automatic cycle closing ("periodicity" = 0) of the lane pool.  Its PERIOD instantiation costs a frame in which nothing
 * ever closes -- a Julia dust, the C5 view -- 7 % / 3.5 % (profiles/r03_periodicity_cost.txt: the comparisons were made
 * all but free in round 3, the rest would not yield), and frames come in sequences of similar views.  So a context that
 * has looked and closed NOTHING renders its next kProbeEvery - 1 frames of the same kind (fractal, precision, max_iter,
 * geometry) with the plain instantiation, then looks again.  What the pool found travels back without a synchronisation
 * (Feedback), so the verdict on frame n is known when frame n + 2 is planned -- or later, if the host runs ahead of the
 * device: until then the pool keeps looking.  A view whose pools close cycles always looks.  Nothing a pixel depends on. */
static bool pool_wants_cycle_closing(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t rows)
{
    if (c->tune.periodicity != 0) return c->tune.periodicity > 0;          /* explicit: on (any window) or off */
    uint64_t key = 1469598103934665603ull;
    /* ... and WHERE it looks, coarsely: the octave of the zoom, the centre in units of that octave's view height, the Julia
     * constant to 1/64 -- a sequence that leaves a dust for an interior-heavy view (or pans by a view, or zooms by 2x) starts
     * looking again at once instead of finishing its 14 frames of not looking */
    int zexp = 0;
    (void)frexp(fabs(p->zoom), &zexp);
    const double cell = ldexp(1.0, zexp);
    const uint64_t parts[10] = {(uint64_t)p->fractal_type, (uint64_t)p->precision, (uint64_t)p->max_iterations, W, rows,
                                (uint64_t)(int64_t)zexp, (uint64_t)(int64_t)floor(p->center_x / cell), (uint64_t)(int64_t)floor(p->center_y / cell),
                                (uint64_t)(int64_t)floor(p->julia_c_real * 64.0), (uint64_t)(int64_t)floor(p->julia_c_imag * 64.0)};
    for (uint64_t v : parts) key = (key ^ v) * 1099511628211ull;
    if (key != c->probe_key) { c->probe_key = key; c->probe_mode = 0; c->probe_first = 0; }
    /* the verdict the device forwarded last: (render number << 1) | "closing cycles paid" (an eighth of the pool's records
     * and more were retired by a closed cycle), of a render whose pool looked */
    const uint32_t word = __atomic_load_n(c->overflow_host + 1, __ATOMIC_RELAXED);
    const uint32_t seq = word >> 1;
    const bool nothing_closed = (word & 1u) == 0u;
    const uint32_t mine = c->render_seq + 1;                                /* this render's number */
    switch (c->probe_mode) {
    case 0:      /* LOOK: only renders whose pools looked are forwarded, and from probe_first on those are renders of this key:
                  * any of their verdicts counts (a host that runs ahead of the device may never see the one of a particular
                  * render) */
        if (c->probe_first != 0 && seq >= c->probe_first && seq <= c->render_seq && nothing_closed) {
            c->probe_mode = 1; c->skip_left = kProbeEvery - 2;
            return false;
        }
        if (c->probe_first == 0) c->probe_first = mine;
        return true;
    case 1:      /* SKIP */
        if (c->skip_left > 0) { --c->skip_left; return false; }
        c->probe_mode = 2; c->probe_first = mine;                           /* the one look */
        return true;
    default:     /* WAIT: the host may be many frames ahead of the device; one look in flight is enough */
        if (seq == c->probe_first) {
            if (nothing_closed) { c->probe_mode = 1; c->skip_left = kProbeEvery - 2; return false; }
            c->probe_mode = 0; c->probe_first = mine;                       /* the view closes cycles now: look again */
            return true;
        }
        return false;
    }
}

/* zero the queue heads and stream counters of the next render (a kernel, not a memset node: see clear_words_kernel) */
/* (whole: the words of the survivor stream's second class too -- they lie behind the last stage) */
static hipError_t clear_control_block(fr_ctx* c, hipStream_t stream, int nstages, bool whole = false)
{
    const uint32_t n = (uint32_t)((size_t)(whole ? kWholeStage + kWholeStages : nstages) * kStageWords);
    hipLaunchKernelGGL(clear_words_kernel, dim3((n + 4 * kBlockThreads - 1) / (4 * kBlockThreads)), dim3(kBlockThreads), 0, stream, c->d_ctrl, n,
                       feedback_of(c));
    return hipGetLastError();
}

/* Work on the context's own stream (exports, colorize without a stream argument) must see the planes of a render that
 * was enqueued on a CALLER's stream: ev_end was recorded there behind the last launch. */
static hipError_t order_after_last_render(fr_ctx* c, hipStream_t s)
{
    if (!c->render_on_user_stream || !c->have_render || c->last_stream == s) return hipSuccess;
    /* recorded NOW, on the stream that render went to: behind it (and behind whatever the caller has enqueued there since) --
     * the renders themselves record nothing for this */
    const hipError_t e = hipEventRecord(c->ev_order, c->last_stream);
    if (e != hipSuccess) return e;
    return hipStreamWaitEvent(s, c->ev_order, 0);
}

/* the caller's shard with its defaults filled in, and the rows it owns (0: nothing to do) */
static int normalise_shard(const fr_shard* shard, uint32_t H, fr_shard* norm, uint32_t* rows_local)
{
    *norm = fr_shard_normalise(shard, H);
    if (norm->part >= norm->nparts)
        return fr_set_error(FR_ERR_INVALID_ARG, "shard part %u >= nparts %u", norm->part, norm->nparts);
    *rows_local = fr_shard_rows(norm, H);
    return FR_OK;
}

/* behind the last launch of a render: its end event, and where and in how many stages it went */
static int finish_render(fr_ctx* c, hipStream_t stream, int nstages, uint32_t fold = 0u)
{
    c->last_fold = fold;                         /* rows a folded render rendered (fr_ctx_last_fold); 0: every row of its own */
    if (c->timing) FR_HIP_TRY(hipEventRecord(c->ev_end, stream));
    c->have_timing = c->timing;
    c->have_render = true;
    c->last_stream = stream;
    c->last_stages = nstages;
    ++c->render_seq;                             /* its first launch forwarded the previous render's verdict (Feedback) */
    return FR_OK;
}

/* the geometry part of a one-pass kernel's argument block (TileGeom, fr_kernels.hip.h) */
static TileGeom tile_geom(uint32_t W, uint32_t H, uint32_t rows_local, const fr_shard* norm, bool out_frame)
{
    TileGeom g;
    g.W = (int32_t)W; g.H = (int32_t)H; g.rows_local = (int32_t)rows_local;
    g.part = (int32_t)norm->part; g.nparts = (int32_t)norm->nparts; g.rows_per_strip = (int32_t)norm->rows_per_strip;
    g.out_frame = out_frame ? 1 : 0;
    return g;
}

/* What an entry path that takes a caller's shard does first (enqueue_render has its own, with reserve_only).
 * FR_OK with *rows_local == 0: this part owns no rows, nothing to do. */
static int begin_shard(fr_ctx* c, const fr_shard* shard, uint32_t H, fr_shard* norm, uint32_t* rows_local)
{
    const int ov = check_overflow(c);            /* of an earlier asynchronous render nobody has asked about */
    if (ov != FR_OK) return ov;
    return normalise_shard(shard, H, norm, rows_local);
}

/* ---- one-pass kernels (Deep_Zoom, Phoenix, Mandelbulb, the deep views) ----------------------------------------------
 * From "the argument block is filled" to "the render is finished".  One pass, no lane pool: a persistent grid of exactly
 * the resident set over the 8x8 sub-tiles of the WaveQueue (walk_subtiles), planned as an unstaged tile pass
 * (plan_tile_queue: short runs; waves of `moderate` launches stop at their home shard + a neighbour, with 64 shards on
 * large frames; the others steal from every shard).  The resident set is wg_per_cu workgroups per CU: the caller's cache
 * word of `kernel`, 0 = not asked yet -- then the occupancy query answers, once per context and kernel.
 * g and q are the geometry and queue members of a. */
template <class ARGS>
static int launch_one_pass(fr_ctx* c, hipStream_t stream, const char* name, void (*kernel)(ARGS), ARGS& a, const TileGeom& g,
                           QueueArgs& q, int& wg_per_cu, bool moderate)
{
    if (wg_per_cu == 0) {
        int nb = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, kBlockThreads, 0);
        if (e != hipSuccess) return fr_set_error(FR_ERR_HIP, "%s occupancy query failed: %s", name, hipGetErrorString(e));
        wg_per_cu = nb < 1 ? 1 : nb;
    }
    uint32_t grid = 0;
    q = plan_tile_queue(c->tune, c->compute_units, (uint32_t)g.W, (uint32_t)g.rows_local, 3, false, moderate, (uint32_t)wg_per_cu, &grid);
    q.heads = stage_heads(c, 0);
    c->last_grid = grid;
    c->last_pool_closing = -1;

    FR_HIP_TRY(clear_control_block(c, stream, 1));
    if (c->timing) FR_HIP_TRY(hipEventRecord(c->ev_begin, stream));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlockThreads), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fr_set_error(FR_ERR_HIP, "%s launch failed: %s", name, hipGetErrorString(e));
    return finish_render(c, stream, 1);
}

/* Deep_Zoom: what VulkanEngine::prepare_deep_zoom_rendering + dispatch do per frame
 * (src/vk_engine.cpp:215-251, src/compute_effect_manager.h:236-324): recompute the fp64 reference orbit
 * at the view centre on the host (single point, sequential), narrow it to float pairs
 * (src/deep_zoom_system.cpp:102-110), upload, launch the perturbation kernel. */
/* Deep_Zoom orbit buffers: pinned staging (fp64 orbit + its float narrowing, `cap` scalars each) + the device copy */
static int reserve_orbit(fr_ctx* c, size_t need)
{
    if (need <= c->orbit_cap) return FR_OK;
    if (c->orbit_host) { (void)hipHostFree(c->orbit_host); c->orbit_host = nullptr; }
    if (c->orbit_dev) { (void)hipFree(c->orbit_dev); c->orbit_dev = nullptr; }
    c->orbit_cap = 0;
    FR_HIP_TRY(hipHostMalloc((void**)&c->orbit_host, need * sizeof(double) + need * sizeof(float)));
    FR_HIP_TRY(hipMalloc((void**)&c->orbit_dev, need * sizeof(float)));
    c->orbit_cap = need;
    return FR_OK;
}

static int enqueue_deep_zoom(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H, const fr_shard* norm,
                             uint32_t rows_local, float* rgba, void* nu, int32_t* iter, hipStream_t stream, bool reserve_only,
                             bool out_frame)
{
    const int32_t max_iter = p->max_iterations;
    int32_t ref_iter = 0;
    if (reserve_only) return p->use_perturbation ? reserve_orbit(c, (size_t)max_iter * 2) : FR_OK;
    if (p->use_perturbation) {
        const size_t need = (size_t)max_iter * 2;
        /* the pinned staging buffer may still feed an earlier asynchronous upload */
        FR_HIP_TRY(hipStreamSynchronize(stream));
        int rs = reserve_orbit(c, need);
        if (rs != FR_OK) return rs;
        double* xy = (double*)c->orbit_host;
        float* xyf = (float*)(xy + c->orbit_cap);
        int st = fr_reference_orbit(p->center_x, p->center_y, max_iter, xy, &ref_iter);
        if (st != FR_OK) return st;
        for (int32_t i = 0; i < 2 * ref_iter; ++i) xyf[i] = (float)xy[i];
        FR_HIP_TRY(hipMemcpyAsync(c->orbit_dev, xyf, (size_t)ref_iter * 2 * sizeof(float), hipMemcpyHostToDevice, stream));
    }

    DeepZoomArgs a;
    memset(&a, 0, sizeof(a));
    a.cx_hi = (float)p->center_x; a.cx_lo = (float)(p->center_x - (double)a.cx_hi);      /* split_double, :252-257 */
    a.cy_hi = (float)p->center_y; a.cy_lo = (float)(p->center_y - (double)a.cy_hi);
    a.zoom_hi = (float)p->zoom;   a.zoom_lo = (float)(p->zoom - (double)a.zoom_hi);
    a.bailout = p->bailout; a.color_offset = p->color_offset; a.color_scale = p->color_scale;
    a.palette_mode = p->palette_mode; a.max_iter = max_iter; a.ref_iter = ref_iter;
    a.g = tile_geom(W, H, rows_local, norm, out_frame);
    a.orbit = reinterpret_cast<const float2*>(c->orbit_dev);
    a.rgba = reinterpret_cast<float4*>(rgba); a.nu = (float*)nu; a.iter = iter;

    int wg = 8;                                  /* a fixed 8 workgroups per CU: nothing is asked */
    return launch_one_pass(c, stream, "deep_zoom_kernel", deep_zoom_kernel<3>, a, a.g, a.q, wg, false);
}

/* ---- Phoenix (fr_phoenix.hip.h): one pass (launch_one_pass) ---------------------------------------------------------- */
static int enqueue_phoenix(fr_ctx* c, const fr_params* p, const fr_phoenix_params* ph, uint32_t W, uint32_t H,
                           const fr_shard* shard, float* rgba, void* nu, int32_t* iter, hipStream_t stream, bool out_frame)
{
    fr_shard norm;
    uint32_t rows_local = 0;
    const int sh = begin_shard(c, shard, H, &norm, &rows_local);
    if (sh != FR_OK || rows_local == 0) return sh;
    const bool f64 = p->precision == FR_PRECISION_F64;

    PhoenixArgs a;
    memset(&a, 0, sizeof(a));
    a.center_x = p->center_x; a.center_y = p->center_y; a.zoom = p->zoom;
    a.julia_cx = p->julia_c_real; a.julia_cy = p->julia_c_imag;
    a.center_x_f = (float)p->center_x; a.center_y_f = (float)p->center_y; a.zoom_f = (float)p->zoom;   /* data1, data2.xy */
    a.julia_cx_f = (float)p->julia_c_real; a.julia_cy_f = (float)p->julia_c_imag;
    a.p = ph->phoenix_p; a.r = ph->phoenix_r;
    a.stripe_density = p->stripe_density;
    a.brightness = p->color_brightness; a.saturation = p->color_saturation; a.contrast = p->color_contrast;
    a.max_iter = p->max_iterations; a.aa = p->antialiasing_samples; a.use_julia = ph->use_julia_set;
    a.flags = p->flags;
    a.g = tile_geom(W, H, rows_local, &norm, out_frame);
    a.rgba = reinterpret_cast<float4*>(rgba); a.nu = nu; a.iter = iter;

    /* launches of moderate cost stop at their home shard + a neighbour; long ones steal from every shard */
    const int aa1 = p->antialiasing_samples > 1 ? p->antialiasing_samples : 1;
    const bool moderate = (long long)p->max_iterations * aa1 * aa1 < 768;
    return launch_one_pass(c, stream, f64 ? "phoenix_kernel<double>" : "phoenix_kernel<float>",
                           f64 ? phoenix_kernel<double> : phoenix_kernel<float>, a, a.g, a.q, c->phoenix_wg_per_cu[f64 ? 1 : 0],
                           moderate);
}

/* ---- Mandelbulb (fr_mandelbulb.hip.h) -----------------------------------------------------------------------------
 * One pass (launch_one_pass) with unlimited stealing: ray lengths vary too much across a frame for a wave to stop at its
 * home shard.  main's clamps (:177-190) are applied here. */
static int enqueue_mandelbulb(fr_ctx* c, const fr_params* p, const fr_mandelbulb_params* mb, uint32_t W, uint32_t H,
                              const fr_shard* shard, float* rgba, void* nu, int32_t* iter, hipStream_t stream, bool out_frame)
{
    fr_shard norm;
    uint32_t rows_local = 0;
    const int sh = begin_shard(c, shard, H, &norm, &rows_local);
    if (sh != FR_OK || rows_local == 0) return sh;
    auto fmax_ = [](float x, float y) { return x < y ? y : x; };              /* GLSL max, FMax's operand order */
    auto fclamp = [&](float x, float lo, float hi) { const float m = fmax_(x, lo); return hi < m ? hi : m; };

    MandelbulbArgs a;
    memset(&a, 0, sizeof(a));
    a.camera_distance = fmax_(mb->camera_distance, 0.1f);                     /* :177 */
    a.rotation_y = mb->rotation_y;
    a.power = fclamp(mb->mandelbulb_power, 2.0f, 16.0f);                      /* :179 */
    a.max_iter = p->max_iterations < 1 ? 1 : (p->max_iterations > 1024 ? 1024 : p->max_iterations);   /* :180 */
    a.color_offset = p->color_offset;
    a.color_scale = fmax_(p->color_scale, 0.1f);                              /* :182 */
    a.palette_mode = p->palette_mode < 0 ? 0 : (p->palette_mode > 5 ? 5 : p->palette_mode);          /* :183 */
    a.time = mb->time;
    a.fov = fclamp(mb->fov, 0.1f, 3.0f);                                      /* :185 */
    a.aa = p->antialiasing_samples > 1 ? p->antialiasing_samples : 1;        /* :186 */
    a.brightness = fmax_(p->color_brightness, 0.1f);                          /* :187-190 */
    a.rotation_speed = mb->rotation_speed != 0.0f ? mb->rotation_speed : 0.3f;
    a.saturation = fmax_(p->color_saturation, 0.0f);
    a.contrast = fmax_(p->color_contrast, 0.1f);
    a.flags = p->flags;
    a.g = tile_geom(W, H, rows_local, &norm, out_frame);
    a.rgba = reinterpret_cast<float4*>(rgba); a.nu = (float*)nu; a.iter = iter;

    const bool split = c->tune.mandelbulb_split != 1u;
    return launch_one_pass(c, stream, split ? "mandelbulb_kernel<true>" : "mandelbulb_kernel<false>",
                           split ? mandelbulb_kernel<true> : mandelbulb_kernel<false>, a, a.g, a.q,
                           c->mandelbulb_wg_per_cu[split ? 1 : 0], false);
}

/* ---- deep views (fr_deep.hip.h) -------------------------------------------------------------------------------------
 * The reference orbit of the view (fr_deep.c, on the host) unless the context holds it already, then one pass
 * (launch_one_pass) with unlimited stealing. */
static char* copy_string(const char* s)
{
    const size_t n = strlen(s) + 1;
    char* d = (char*)malloc(n);
    if (d) memcpy(d, s, n);
    return d;
}

static bool orbit_key_matches(const OrbitKey& k, const char* x, const char* y, int32_t bits, int32_t max_iter, float bailout)
{
    return k.valid && k.bits == bits && k.max_iter == max_iter && memcmp(&k.bailout, &bailout, sizeof(float)) == 0 &&
           strcmp(k.x, x) == 0 && strcmp(k.y, y) == 0;
}

/* the key of the orbit that has just arrived on the device: valid once both strings are copied */
static int orbit_key_store(OrbitKey& k, const char* x, const char* y, int32_t bits, int32_t max_iter, float bailout)
{
    free(k.x); free(k.y);
    k.x = copy_string(x);
    k.y = copy_string(y);
    if (!k.x || !k.y) return fr_set_error(FR_ERR_NOMEM, "out of host memory");
    k.bits = bits; k.max_iter = max_iter; k.bailout = bailout;
    k.valid = true;
    return FR_OK;
}

/* A slot about to receive another orbit: everything that may still read its pinned or its device block has finished (an earlier
 * upload or render on this stream, the context's own or the stream of the previous render; with `t` the slot's last BLA
 * render, wherever it went), its key is void, and both blocks hold `need` points of `point_bytes` */
static int orbit_slot_prepare(fr_ctx* c, DeepOrbit& o, const BlaSlot* t, hipStream_t stream, size_t need, size_t point_bytes)
{
    FR_HIP_TRY(hipStreamSynchronize(stream));
    FR_HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->have_render && c->last_stream != stream) FR_HIP_TRY(hipStreamSynchronize(c->last_stream));
    if (t && t->ev_valid) FR_HIP_TRY(hipEventSynchronize(t->ev));
    o.key.valid = false;
    ++o.gen;
    if (need > o.cap) {
        if (o.host) { (void)hipHostFree(o.host); o.host = nullptr; }
        if (o.dev) { (void)hipFree(o.dev); o.dev = nullptr; }
        o.cap = 0;
        FR_HIP_TRY(hipHostMalloc((void**)&o.host, need * point_bytes));
        FR_HIP_TRY(hipMalloc((void**)&o.dev, need * point_bytes));
        o.cap = need;
    }
    return FR_OK;
}

/* what differs per formula on the host: the orbits a slot holds (a Julia slot: Q, then P) and the double2 per table entry */
static const struct { int orbits; size_t ab_per_entry; } kFormula[kFormulas] = {
    {1, MandelFormula::kAbPerEntry}, {1, ShipFormula::kAbPerEntry}, {2, JuliaFormula::kAbPerEntry}, {1, kPhoenixMbPerEntry}};

/* a view as the enqueue side reads it: the centre strings, the zoom as a pair (an fp64 view: (zoom, 0)) and the fraction bits of
 * its orbit; zoom: the string of an extended view, which the orbit does not depend on (nullptr: an fp64 view) */
struct DeepAt {
    const char *cx, *cy, *zoom;
    double zm;
    int32_t ze, bits;
};

/* ... of an entry point's view, validated: an fp64 view with the automatic F where frac_bits is 0; an extended view's zoom is its
 * string, resolved here with its F */
static int deep_at_of(const fr_params* p, const fr_deep_view* v, DeepAt* at)
{
    *at = {v->center_x, v->center_y, nullptr, p->zoom, 0, v->frac_bits ? v->frac_bits : fr_deep_frac_bits(p->zoom)};
    return FR_OK;
}

static int deep_at_of(const fr_params*, const fr_deepx_view* v, DeepAt* at)
{
    *at = {v->center_x, v->center_y, v->zoom, 0.0, 0, v->frac_bits};
    return fr_deepx_resolve(v, &at->zm, &at->ze, &at->bits);
}

/* The reference orbit(s) of the view in the path's slot unless the slot holds them already (keyed by the centre strings, the
 * fraction bits, max_iter, the bailout and, in a Julia slot, the bits of c).  One orbit, or Julia's Q at point 0 and P half the
 * capacity behind it (kFormula); ext: the extended storage, whose plain doubles ldexp(mantissa, exponent) are formed here.
 * Per array and orbit, what the host wrote is uploaded and nothing else: no kernel reads a point past an orbit's length.
 * The two Phoenix slots (ph): keyed by the bits of p and r where Julia's has c, and by the shader's fixed bailout 2, since
 * p->bailout is not read. */
static int deep_slot_fill(fr_ctx* c, int f, bool ext, const fr_params* p, const DeepAt& at, hipStream_t stream,
                          const fr_phoenix_params* ph = nullptr)
{
    DeepSlot& s = deep_slot(c, ext, f);
    DeepOrbit& o = s.o;
    const int32_t max_iter = p->max_iterations;
    const int norb = kFormula[f].orbits;
    uint64_t cb[2] = {0, 0};
    if (f == kJulia) {
        memcpy(&cb[0], &p->julia_c_real, sizeof(uint64_t));
        memcpy(&cb[1], &p->julia_c_imag, sizeof(uint64_t));
    }
    if (f == kPhoenix) {
        memcpy(&cb[0], &ph->phoenix_p, sizeof(float));
        memcpy(&cb[1], &ph->phoenix_r, sizeof(float));
    }
    const float bailout = f == kPhoenix ? 2.0f : p->bailout;
    if (orbit_key_matches(o.key, at.cx, at.cy, at.bits, max_iter, bailout) && o.key.c_bits[0] == cb[0] && o.key.c_bits[1] == cb[1])
        return FR_OK;
    const size_t point_bytes = ext ? 2 * sizeof(double2) + sizeof(int32_t) : sizeof(double2);
    const int ps = orbit_slot_prepare(c, o, &s.t, stream, (size_t)norb * ((size_t)max_iter + 1), point_bytes);
    if (ps != FR_OK) return ps;
    const size_t cap = o.cap, second = cap / 2;                  /* a Julia slot's capacity is even */
    double* plain = (double*)o.host;
    double* mant = ext ? plain + 2 * cap : nullptr;
    int32_t* exp2 = ext ? (int32_t*)(mant + 2 * cap) : nullptr;
    const fr_deep_view v = {at.cx, at.cy, at.bits, 0};
    const fr_deepx_view x = {at.cx, at.cy, at.zoom, at.bits, 0};
    int32_t len[2] = {0, 0};                                      /* of the orbit at point 0, of Julia's P */
    int st;
    if (f == kPhoenix)
        st = ext ? fr_deepx_phoenix_reference_orbit(&x, ph, max_iter, mant, exp2, &len[0])
                 : fr_deep_phoenix_reference_orbit(&v, ph, p->zoom, max_iter, plain, &len[0]);
    else if (f == kJulia)
        st = ext ? fr_deepx_julia_reference_orbits(&x, p->julia_c_real, p->julia_c_imag, max_iter, p->bailout, mant + 2 * second,
                                                   exp2 + second, &len[1], mant, exp2, &len[0])
                 : fr_deep_julia_reference_orbits(&v, p->julia_c_real, p->julia_c_imag, p->zoom, max_iter, p->bailout,
                                                  plain + 2 * second, &len[1], plain, &len[0]);
    else if (ext)
        st = (f == kShip ? fr_deepx_ship_reference_orbit : fr_deepx_reference_orbit)(&x, max_iter, p->bailout, mant, exp2, &len[0]);
    else
        st = (f == kShip ? fr_deep_ship_reference_orbit : fr_deep_reference_orbit)(&v, p->zoom, max_iter, p->bailout, plain, &len[0]);
    if (st != FR_OK) return st;
    for (int q = 0; q < norb; ++q) {
        const size_t b = q ? second : 0, n = (size_t)len[q];
        for (size_t i = b; ext && i < b + n; ++i) {
            plain[2 * i] = ldexp(mant[2 * i], exp2[i]);
            plain[2 * i + 1] = ldexp(mant[2 * i + 1], exp2[i]);
        }
        FR_HIP_TRY(hipMemcpyAsync(o.dev + b * sizeof(double2), o.host + b * sizeof(double2), n * sizeof(double2),
                                  hipMemcpyHostToDevice, stream));
        if (ext) {
            const size_t mo = (cap + b) * sizeof(double2), eo = 2 * cap * sizeof(double2) + b * sizeof(int32_t);
            FR_HIP_TRY(hipMemcpyAsync(o.dev + mo, o.host + mo, n * sizeof(double2), hipMemcpyHostToDevice, stream));
            FR_HIP_TRY(hipMemcpyAsync(o.dev + eo, o.host + eo, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        }
    }
    FR_HIP_TRY(hipStreamSynchronize(stream));     /* a later render of this view may go to another stream */
    const int ks = orbit_key_store(o.key, at.cx, at.cy, at.bits, max_iter, bailout);
    if (ks != FR_OK) return ks;
    o.key.c_bits[0] = cb[0]; o.key.c_bits[1] = cb[1];
    o.len = len[0]; o.len_p = len[1];
    return FR_OK;
}

/* The frame's dcmax (the whole frame's W, H; each formula's own bound, see the header); zs = the zoom or its mantissa */
static double bla_dcmax(int f, double zs, double w, double h)
{
    const double a = w / h;
    if (f == kMandel) return (1.0000001 * (0.5 * zs)) * sqrt(a * a + 1.0);
    const double hx = 0.5 + 0.5 / (w * w);
    const double hy = 0.5 + 0.5 / (w * h);
    const double ex = hx * a;
    return (1.0000001 * zs) * sqrt(ex * ex + hy * hy);
}

static int bla_levels(int32_t N) { return N > 1 ? 31 - __builtin_clz((uint32_t)(N - 1)) : 0; }   /* floor(log2(N - 1)) */
static size_t bla_entries(int32_t N)             /* sum over k >= 1 of (N - 1) >> k */
{
    const uint32_t n1 = (uint32_t)(N - 1);
    return (size_t)(n1 - (uint32_t)__builtin_popcount(n1));
}

struct JuliaTables { int32_t levels_p; uint32_t base_p; };

/* what a table build reads of the render it is for: the orbit's plain doubles, the zoom (an extended view: not read), the whole
 * frame's size, and Phoenix's p and r widened (the other formulas: not read) */
struct BlaFrame {
    const double2* orbit;
    double zoom;
    int32_t W, H;
    double p, r;
};

/* BLA: the table of the slot's cached orbit -- the extended one with x, the view's extended block -- for this frame's dcmax,
 * built on `stream` unless the slot holds it.  A rebuild overwrites the buffers in place behind the slot's last BLA render (its
 * event: the render may have gone to another stream); growing them frees the old ones, so that waits on the host first.  A
 * Julia slot (jt) holds two tables, Q's entries first and P's behind them, built from the slot's two orbits; no dcmax enters
 * them, so their key is the orbit slot's generation alone and a zoom change rebuilds nothing. */
static int bla_table_for(fr_ctx* c, DeepSlot& s, int f, const BlaFrame& d, const DeepXOrbit* x, hipStream_t stream, int* levels,
                         JuliaTables* jt)
{
    BlaSlot& t = s.t;
    const DeepOrbit& o = s.o;
    const int norb = kFormula[f].orbits;
    /* the slot's orbits as the build walks them: N, the orbit's first point, the first entry of its table */
    struct { int32_t N; size_t point, entry; } orb[2] = {{o.len - 1, 0, 0}, {f == kJulia ? o.len_p - 1 : 1, o.cap / 2, 0}};
    orb[1].entry = bla_entries(orb[0].N);
    *levels = bla_levels(orb[0].N);
    size_t need = orb[1].entry;
    if (f == kJulia) {
        jt->levels_p = bla_levels(orb[1].N);
        jt->base_p = (uint32_t)need;
        need += bla_entries(orb[1].N);
    }
    if (bla_levels(orb[0].N) == 0 && bla_levels(orb[1].N) == 0) return FR_OK;
    double dcv = 0.0;
    int32_t dce = 0;
    if (f != kJulia) {
        dcv = bla_dcmax(f, x ? x->zm : d.zoom, (double)d.W, (double)d.H);
        if (x) {                                 /* as an extended real with the zoom pair, normalised: dcv in [0.5, 1) */
            int de = 0;
            dcv = frexp(dcv, &de);
            dce = x->ze + de;
        }
    }
    uint64_t dbits;
    memcpy(&dbits, &dcv, sizeof(dbits));
    if (t.valid && t.key_gen == o.gen && t.key_dcv == dbits && t.key_dce == dce) return FR_OK;
    t.valid = false;
    const size_t nab = kFormula[f].ab_per_entry;
    if (need > t.cap) {
        FR_HIP_TRY(hipStreamSynchronize(stream));
        FR_HIP_TRY(hipStreamSynchronize(c->stream));
        if (t.ev_valid) FR_HIP_TRY(hipEventSynchronize(t.ev));
        if (t.r) { (void)hipFree(t.r); t.r = nullptr; }
        if (t.ab) { (void)hipFree(t.ab); t.ab = nullptr; }
        if (t.abe) { (void)hipFree(t.abe); t.abe = nullptr; }
        t.cap = 0;
        FR_HIP_TRY(hipMalloc(&t.r, need * (x ? sizeof(XRad) : sizeof(double))));
        FR_HIP_TRY(hipMalloc((void**)&t.ab, need * nab * sizeof(double2)));
        if (x) FR_HIP_TRY(hipMalloc((void**)&t.abe, need * (f == kJulia ? sizeof(int32_t) : sizeof(int2))));
        t.cap = need;
    } else if (t.ev_valid) {
        FR_HIP_TRY(hipStreamWaitEvent(stream, t.ev, 0));
    }
    /* level k of one orbit's table: each formula's kernel in either storage (Julia's take no dcmax and an int32 exponent plane) */
    auto launch_level = [&](dim3 grid, int32_t N, int k, size_t po, size_t eo) {
        const dim3 block(kBlockThreads);
        if (f == kJulia && x)
            hipLaunchKernelGGL(deepx_julia_bla_level_kernel, grid, block, 0, stream, x->mant + po, x->exp2 + po, N, k,
                               (XRad*)t.r + eo, t.ab + eo * nab, (int32_t*)t.abe + eo);
        else if (f == kJulia)
            hipLaunchKernelGGL(deep_julia_bla_level_kernel, grid, block, 0, stream, d.orbit + po, N, k, (double*)t.r + eo,
                               t.ab + eo * nab);
        else if (f == kPhoenix && x)
            hipLaunchKernelGGL(phoenix_x_bla_level_kernel, grid, block, 0, stream, x->mant, x->exp2, N, k, dcv, dce, d.p, d.r,
                               (XRad*)t.r, t.ab, t.abe);
        else if (f == kPhoenix)
            hipLaunchKernelGGL(phoenix_bla_level_kernel, grid, block, 0, stream, d.orbit, N, k, dcv, d.p, d.r, (double*)t.r,
                               t.ab);
        else if (x)
            hipLaunchKernelGGL(f == kShip ? deepx_ship_bla_level_kernel : deepx_bla_level_kernel, grid, block, 0, stream, x->mant,
                               x->exp2, N, k, dcv, dce, (XRad*)t.r, t.ab, t.abe);
        else
            hipLaunchKernelGGL(f == kShip ? deep_ship_bla_level_kernel : deep_bla_level_kernel, grid, block, 0, stream, d.orbit, N, k,
                               dcv, (double*)t.r, t.ab);
    };
    const uint32_t grid_cap = (uint32_t)c->compute_units * 8u;
    for (int q = 0; q < norb; ++q)
        for (int k = 1; k <= bla_levels(orb[q].N); ++k) {
            const uint32_t cnt = (uint32_t)(orb[q].N - 1) >> k;
            uint32_t grid = (cnt + kBlockThreads - 1) / kBlockThreads;
            if (grid > grid_cap) grid = grid_cap;
            launch_level(dim3(grid), orb[q].N, k, orb[q].point, orb[q].entry);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess)
                return fr_set_error(FR_ERR_HIP, "%s%sBLA table launch failed: %s", x ? "extended " : "",
                                    f == kShip ? "ship " : f == kJulia ? "Julia " : f == kPhoenix ? "Phoenix " : "", hipGetErrorString(e));
        }
    ++t.builds;
    t.key_gen = o.gen;
    t.key_dcv = dbits;
    t.key_dce = dce;
    t.valid = true;
    return FR_OK;
}

static void bla_table_args(BlaTable& a, const BlaSlot& t) { a.r = (const double*)t.r; a.ab = t.ab; }
static void bla_table_args(BlaXTable& a, const BlaSlot& t) { a.r = (const XRad*)t.r; a.ab = t.ab; a.abe = t.abe; }

/* Around a flagged kernel's launch.  In front of it: the slot's three counters, allocated on first use and cleared on the stream.
 * Behind it: their copy to pinned memory, and the slot's event unless the stream is capturing. */
static int bla_steps_begin(BlaSlot& t, hipStream_t stream, unsigned long long** steps)
{
    if (!t.steps_dev) {
        FR_HIP_TRY(hipMalloc((void**)&t.steps_dev, 3 * sizeof(unsigned long long)));
        FR_HIP_TRY(hipHostMalloc((void**)&t.steps_host, 3 * sizeof(unsigned long long)));
    }
    *steps = t.steps_dev;
    FR_HIP_TRY(hipMemsetAsync(t.steps_dev, 0, 3 * sizeof(unsigned long long), stream));
    return FR_OK;
}

static int bla_steps_end(BlaSlot& t, hipStream_t stream)
{
    FR_HIP_TRY(hipMemcpyAsync(t.steps_host, t.steps_dev, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    t.have_steps = true;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusActive; }
    t.ev_valid = false;
    if (cap == hipStreamCaptureStatusNone) {
        FR_HIP_TRY(hipEventRecord(t.ev, stream));
        t.ev_valid = true;
    }
    return FR_OK;
}

/* A flagged kernel's launch, for every path: the slot's table of formula f for the frame fr (bla_table_for: x with the extended
 * storage, jt for Julia's two), its pointers and level count into `tab`, the table inside the kernel's argument block, then
 * launch() -- the kernel on that block -- between the counters' clearing and their copy. */
template <class TAB, class Launch>
static int launch_with_bla(fr_ctx* c, hipStream_t stream, DeepSlot& s, int f, const BlaFrame& fr, const DeepXOrbit* x, TAB& tab,
                           JuliaTables* jt, Launch&& launch)
{
    int levels = 0;
    const int ts = bla_table_for(c, s, f, fr, x, stream, &levels, jt);
    if (ts != FR_OK) return ts;
    bla_table_args(tab, s.t);
    tab.levels = levels;
    const int bs = bla_steps_begin(s.t, stream, &tab.steps);
    if (bs != FR_OK) return bs;
    const int st = launch();
    if (st != FR_OK) return st;
    return bla_steps_end(s.t, stream);
}

/* The ten paths of DeepBlock, each by the block of its unflagged kernel (the flagged kernel's, with the table: DeepPath::Bla) */
using DeepMandel = DeepBlock<MandelFormula, false, false>;
using DeepMandelDe = DeepBlock<MandelFormula, false, true>;
using DeepMandelX = DeepBlock<MandelFormula, true, false>;
using DeepMandelXDe = DeepBlock<MandelFormula, true, true>;
using DeepShip = DeepBlock<ShipFormula, false, false>;
using DeepShipX = DeepBlock<ShipFormula, true, false>;
using DeepJulia = DeepBlock<JuliaFormula, false, false>;
using DeepJuliaDe = DeepBlock<JuliaFormula, false, true>;
using DeepJuliaX = DeepBlock<JuliaFormula, true, false>;
using DeepJuliaXDe = DeepBlock<JuliaFormula, true, true>;
/* ... and the ship's two distance paths, whose four kernels are deep_ship_de_kernel's */
template <bool X> using DeepShipDe = DeepBlock<ShipFormula, X, true>;

/* What launch_deep and enqueue_deep_view read of a path, BASE being the argument block of its unflagged kernel: the formula, the
 * storage, de = 1 for the blocks that carry a derivative, the flag that selects the flagged kernel and that kernel's block */
static constexpr uint32_t kDeepBlaFlag[3][2] = {{FR_FLAG_DEEP_BLA, FR_FLAG_DEEPX_BLA},
                                                {FR_FLAG_DEEP_SHIP_BLA, FR_FLAG_DEEPX_SHIP_BLA},
                                                {FR_FLAG_DEEP_JULIA_BLA, FR_FLAG_DEEPX_JULIA_BLA}};
template <class BASE>
struct DeepPath {
    using F = typename BASE::Formula;
    static constexpr int f = std::is_same<F, ShipFormula>::value ? kShip : std::is_same<F, JuliaFormula>::value ? kJulia : kMandel;
    static constexpr int de = BASE::kDe;
    static constexpr bool ext = BASE::kX;
    static constexpr uint32_t flag = kDeepBlaFlag[f][ext];
    using Bla = DeepBlock<F, BASE::kX, BASE::kDe, true>;
};

/* the __global__ template a block's kernel is an instantiation of: deep_ship_de_kernel for the ship's distance estimate */
template <class ARGS>
static constexpr bool kShipDe = std::is_same<typename ARGS::Formula, ShipFormula>::value && ARGS::kDe;
template <class ARGS>
static constexpr auto deep_kernel_of()
{
    if constexpr (kShipDe<ARGS>) return deep_ship_de_kernel<ARGS>;
    else return deep_kernel<ARGS>;
}

/* a deep kernel's name in messages, from its block's switches: deep_kernel<Julia, X, DE, BLA> */
template <class ARGS>
static const char* deep_kernel_name()
{
    static const char* const formula[3] = {"Mandel", "Ship", "Julia"};
    static const std::string name = std::string(kShipDe<ARGS> ? "deep_ship_de_kernel<" : "deep_kernel<") + formula[DeepPath<ARGS>::f] + (ARGS::kX ? ", X" : "") +
                                    (ARGS::kDe ? ", DE" : "") + (ARGS::kBla ? ", BLA" : "") + ">";
    return name.c_str();
}

/* One pass of a deep view, `base` being the argument block of its unflagged kernel: the path's kernel of BASE at the occupancy
 * cached in its slot, or with `bla` the table, then the path's flagged kernel on the same queue plan at its own occupancy, its
 * counters cleared in front of it and copied to pinned memory behind it.  The slot's event is recorded behind every such render
 * unless the stream is capturing: table rebuilds and orbit uploads wait for it. */
template <class BASE>
static int launch_deep(fr_ctx* c, hipStream_t stream, BASE& base, bool bla)
{
    using P = DeepPath<BASE>;
    using BLA = typename P::Bla;
    DeepSlot& s = deep_slot(c, P::ext, P::f);
    if (!bla)
        return launch_one_pass(c, stream, deep_kernel_name<BASE>(), deep_kernel_of<BASE>(), base, base.g, base.q, s.wg_per_cu[P::de][0],
                               false);
    BLA a;
    memset(&a, 0, sizeof(a));
    static_cast<BASE&>(a) = base;
    const DeepXOrbit* x = nullptr;
    if constexpr (P::ext) x = &a;
    JuliaTables jt = {0, 0u};
    const BlaFrame fr = {a.orbit, a.zoom, a.g.W, a.g.H, 0.0, 0.0};
    return launch_with_bla(c, stream, s, P::f, fr, x, bla_table(a), &jt, [&] {
        if constexpr (P::f == kJulia) { a.t.levels_p = jt.levels_p; a.t.base_p = jt.base_p; }
        return launch_one_pass(c, stream, deep_kernel_name<BLA>(), deep_kernel_of<BLA>(), a, a.g, a.q, s.wg_per_cu[P::de][1], false);
    });
}

/* everything of DeepArgs that does not depend on the path: the zoom and the orbit stay with enqueue_deep_view */
static void fill_deep_args(DeepArgs& a, const fr_ctx* c, const fr_params* p, const TileGeom& g, float* rgba, void* nu,
                           int32_t* iter)
{
    a.max_iter = p->max_iterations; a.aa = p->antialiasing_samples;
    a.B2 = (double)p->bailout * (double)p->bailout;
    a.g = g;
    a.flags = p->flags;
    a.interior_style = p->interior_style;
    a.lib_log = !(p->bailout > 1.0f);            /* as fill_params */
    a.inv_max_iter = 1.0 / (double)p->max_iterations;
    a.inv_log2_bailout = 1.0 / log2((double)p->bailout);
    a.color_scale_d = (double)p->color_scale; a.color_offset_d = (double)p->color_offset;
    a.brightness = p->color_brightness; a.saturation = p->color_saturation; a.contrast = p->color_contrast;
    fr_palette_table_build(p->fractal_type != FR_FRACTAL_MANDELBROT ? 1 : 0, p->palette_mode, &a.pal);   /* as fill_params */
    a.log2_tab = c->log2_tab;
    a.rgba = reinterpret_cast<float4*>(rgba); a.nu = (double*)nu; a.iter = iter;
}

/* Every deep render, BASE being the argument block of the path's unflagged kernel (DeepPath): the rows of this part, the orbit(s)
 * in the path's slot, the block filled -- the orbit, in the extended storage its mantissas, exponents and the zoom pair, Julia's
 * second orbit, log(bailout) where the block has one (as fill_params) -- then `extra` for what only one block carries
 * (fr_render_deep_de's derivative) and the launch, with the table when p carries the path's flag. */
template <class BASE, class Extra>
static int enqueue_deep_view(fr_ctx* c, const fr_params* p, const DeepAt& at, uint32_t W, uint32_t H, const fr_shard* shard,
                             float* rgba, void* nu, int32_t* iter, hipStream_t stream, bool out_frame, Extra&& extra)
{
    using P = DeepPath<BASE>;
    fr_shard norm;
    uint32_t rows_local = 0;
    const int sh = begin_shard(c, shard, H, &norm, &rows_local);
    if (sh != FR_OK || rows_local == 0) return sh;
    const int os = deep_slot_fill(c, P::f, P::ext, p, at, stream);
    if (os != FR_OK) return os;

    const DeepOrbit& o = deep_slot(c, P::ext, P::f).o;
    BASE b;
    memset(&b, 0, sizeof(b));
    b.orbit = reinterpret_cast<const double2*>(o.dev); b.n_ref = o.len - 1;
    if constexpr (P::ext) {                                      /* (zoom is not read) */
        b.mant = b.orbit + o.cap;
        b.exp2 = reinterpret_cast<const int32_t*>(b.mant + o.cap);
        b.zm = at.zm;
        b.ze = at.ze;
    } else {
        b.zoom = p->zoom;
    }
    if constexpr (P::f == kJulia) { b.j.p_off = (int32_t)(o.cap / 2); b.j.n_p = o.len_p - 1; }
    fill_deep_args(b, c, p, tile_geom(W, H, rows_local, &norm, out_frame), rgba, nu, iter);
    if constexpr (P::f != kMandel) b.log_bailout = log((double)p->bailout);
    extra(b);
    return launch_deep(c, stream, b, (p->flags & P::flag) != 0);
}

/* the extended view already resolved: v gives the centre strings (and a zoom string the orbit does not depend on), the
 * zoom is (zm, ze) and the orbit's fraction bits are `bits` -- what the frames of a fr_deep_sequence of the formula ask for */
static int enqueue_deepx_at(fr_ctx* c, int f, const fr_params* p, const fr_deepx_view* v, double zm, int32_t ze, int32_t bits,
                            uint32_t W, uint32_t H, const fr_shard* shard, float* rgba, void* nu, int32_t* iter,
                            hipStream_t stream, bool out_frame)
{
    const DeepAt at = {v->center_x, v->center_y, v->zoom, zm, ze, bits};
    if (f == kShip)
        return enqueue_deep_view<DeepShipX>(c, p, at, W, H, shard, rgba, nu, iter, stream, out_frame, [](auto&) {});
    return enqueue_deep_view<DeepMandelX>(c, p, at, W, H, shard, rgba, nu, iter, stream, out_frame, [](auto&) {});
}

/* ---- deep Phoenix views (fr_deep_phoenix.hip.h) --------------------------------------------------------------------------- */
/* the kernel of DeepPhoenixBlock<X, BLA> */
template <bool X, bool BLA>
static constexpr auto deep_phoenix_kernel_of()
{
    if constexpr (X && BLA) return deep_phoenix_x_bla_kernel;
    else if constexpr (X) return deep_phoenix_x_kernel;
    else if constexpr (BLA) return deep_phoenix_bla_kernel;
    else return deep_phoenix_kernel;
}

/* enqueue_deep_view's steps for the two paths that stand apart from DeepBlock, fr_render_deep_phoenix and with X
 * fr_render_deepx_phoenix: the rows of this part, the orbit in the Phoenix slot of the storage (deep_slot_fill), the flagged
 * kernel's block filled as enqueue_phoenix fills PhoenixArgs -- with X the extended storage and the zoom pair, else the zoom --
 * then one pass with unlimited stealing at the occupancy cached in the slot: the unflagged kernel on the block less its table, or
 * with the entry's flag the table for this frame's dcmax (the whole frame's W and H) and the flagged kernel (launch_with_bla). */
template <bool X>
static int enqueue_deep_phoenix(fr_ctx* c, const fr_params* p, const fr_phoenix_params* ph, const DeepAt& at, uint32_t W,
                                uint32_t H, const fr_shard* shard, float* rgba, void* nu, int32_t* iter, hipStream_t stream,
                                bool out_frame)
{
    fr_shard norm;
    uint32_t rows_local = 0;
    const int sh = begin_shard(c, shard, H, &norm, &rows_local);
    if (sh != FR_OK || rows_local == 0) return sh;
    const int os = deep_slot_fill(c, kPhoenix, X, p, at, stream, ph);
    if (os != FR_OK) return os;

    DeepSlot& s = deep_slot(c, X, kPhoenix);
    DeepPhoenixBlock<X, true> b;
    memset(&b, 0, sizeof(b));
    b.orbit = reinterpret_cast<const double2*>(s.o.dev); b.n_ref = s.o.len - 1;
    const DeepXOrbit* x = nullptr;
    if constexpr (X) {                                           /* (zoom is not read) */
        b.mant = b.orbit + s.o.cap;
        b.exp2 = reinterpret_cast<const int32_t*>(b.mant + s.o.cap);
        b.zm = at.zm; b.ze = at.ze;
        x = &b;
    } else {
        b.zoom = p->zoom;
    }
    b.max_iter = p->max_iterations; b.aa = p->antialiasing_samples;
    b.p = (double)ph->phoenix_p; b.r = (double)ph->phoenix_r;
    b.stripe_density = p->stripe_density;
    b.brightness = p->color_brightness; b.saturation = p->color_saturation; b.contrast = p->color_contrast;
    b.flags = p->flags;
    b.g = tile_geom(W, H, rows_local, &norm, out_frame);
    b.rgba = reinterpret_cast<float4*>(rgba); b.nu = (double*)nu; b.iter = iter;
    if (!(p->flags & (X ? FR_FLAG_DEEPX_PHOENIX_BLA : FR_FLAG_DEEP_PHOENIX_BLA))) {
        DeepPhoenixBlock<X>& a = b;
        return launch_one_pass(c, stream, X ? "deep_phoenix_x_kernel" : "deep_phoenix_kernel", deep_phoenix_kernel_of<X, false>(), a,
                               a.g, a.q, s.wg_per_cu[0][0], false);
    }
    const BlaFrame fr = {b.orbit, b.zoom, b.g.W, b.g.H, b.p, b.r};
    return launch_with_bla(c, stream, s, kPhoenix, fr, x, b.t, nullptr, [&] {
        return launch_one_pass(c, stream, X ? "deep_phoenix_x_bla_kernel" : "deep_phoenix_bla_kernel", deep_phoenix_kernel_of<X, true>(),
                               b, b.g, b.q, s.wg_per_cu[0][1], false);
    });
}

/* ---- deep zoom sequences (fr_deep_sequence; the rules are in the header, the host planning in fr_deepseq.c) ---------------
 * Every exact render is enqueue_deepx_at with the sequence's formula, around the sequence's one orbit key. Mode 1 keeps two device rgba planes: each holds one keyframe, tagged with its index and with the post-chain flag it
 * was rendered with (fr_deep_sequence_render_png
 * forces the flag), and the least recently needed one makes room. */
struct fr_deep_sequence {
    fr_ctx* c;
    fr_params p;
    bool ship;                  /* the formula: fr_deep_ship_sequence_create's sequences render through fr_render_deepx_ship's path */
    fr_deepseq_walk w;
    char* str[3];               /* copies of center_x, center_y, zoom_first */
    fr_deepx_view view;         /* the centre (the orbit key); its zoom string only has to be a valid one */
    uint32_t W, H;
    float* key[2];              /* mode 1: the keyframe planes */
    int32_t key_id[2];
    bool key_valid[2], key_post[2];
    uint64_t key_used[2], clock;
    uint64_t n_exact, n_resampled, n_orbits;
};

static int seq_exact(fr_deep_sequence* q, const fr_params* p, double zm, int32_t ze, float* rgba, void* nu, int32_t* iter,
                     hipStream_t s)
{
    const int st = enqueue_deepx_at(q->c, q->ship ? kShip : kMandel, p, &q->view, zm, ze, q->w.frac_bits, q->W, q->H, nullptr,
                                    rgba, nu, iter, s, false);
    if (st == FR_OK) ++q->n_exact;
    return st;
}

/* keyframe j in one of the two planes, rendered unless it is there -- into a free plane, else the less recently needed one,
 * but never the plane that holds keyframe *other (the frame's second one); nu / iter of it, if asked for, come from that
 * render or from one of their own */
static int seq_keyframe(fr_deep_sequence* q, const fr_params* p, int32_t j, const int32_t* other, void* nu, int32_t* iter,
                        hipStream_t s, int* slot_out)
{
    const bool post = (p->flags & FR_FLAG_POST_CHAIN) != 0;
    int slot = -1, kept = -1;
    for (int i = 0; i < 2; ++i) {
        if (!q->key_valid[i] || q->key_post[i] != post) continue;
        if (q->key_id[i] == j) slot = i;
        else if (other && q->key_id[i] == *other) kept = i;
    }
    if (slot >= 0) {
        if (nu || iter) {
            const int st = seq_exact(q, p, q->w.zm0, q->w.ze0 - j, nullptr, nu, iter, s);
            if (st != FR_OK) return st;
        }
    } else {
        slot = kept >= 0 ? 1 - kept : (!q->key_valid[0] ? 0 : (!q->key_valid[1] ? 1 : (q->key_used[0] <= q->key_used[1] ? 0 : 1)));
        q->key_valid[slot] = false;
        const int st = seq_exact(q, p, q->w.zm0, q->w.ze0 - j, q->key[slot], nu, iter, s);
        if (st != FR_OK) return st;
        q->key_id[slot] = j;
        q->key_post[slot] = post;
        q->key_valid[slot] = true;
    }
    q->key_used[slot] = ++q->clock;
    *slot_out = slot;
    return FR_OK;
}

static int seq_enqueue_frame(fr_deep_sequence* q, const fr_params* p, const fr_deep_sequence_frame& f, float* rgba, void* nu,
                             int32_t* iter, hipStream_t s)
{
    const size_t npx = (size_t)q->W * q->H;
    if (q->w.mode == 0 || (!f.resampled && !(f.zoom_mant == q->w.zm0 && f.zoom_exp2 == q->w.ze0 - f.keyframe)))
        return seq_exact(q, p, f.zoom_mant, f.zoom_exp2, rgba, nu, iter, s);
    int s0 = -1, s1 = -1;
    const int32_t k0 = f.keyframe, k1 = f.keyframe + 1;
    int st = seq_keyframe(q, p, k0, f.resampled ? &k1 : nullptr, nu, iter, s, &s0);
    if (st != FR_OK) return st;
    if (!f.resampled) {
        if (rgba) FR_HIP_TRY(hipMemcpyAsync(rgba, q->key[s0], npx * 16, hipMemcpyDeviceToDevice, s));
        return FR_OK;
    }
    st = seq_keyframe(q, p, k1, &k0, nullptr, nullptr, s, &s1);
    if (st != FR_OK) return st;
    ResampleArgs a;
    a.key0 = reinterpret_cast<const float4*>(q->key[s0]);
    a.key1 = reinterpret_cast<const float4*>(q->key[s1]);
    a.out = reinterpret_cast<float4*>(rgba);
    a.W = (int32_t)q->W; a.H = (int32_t)q->H;
    a.u = f.u;
    const uint32_t grid = (uint32_t)((npx + kBlockThreads - 1) / kBlockThreads);
    hipLaunchKernelGGL(deep_resample_kernel, dim3(grid), dim3(kBlockThreads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fr_set_error(FR_ERR_HIP, "deep_resample_kernel launch failed: %s", hipGetErrorString(e));
    ++q->n_resampled;
    return FR_OK;
}

/* one frame on `s`: one event pair around all of its launches (fr_ctx_last_kernel_ms is the frame's device time), and the
 * orbits the context computed for it counted */
static int seq_enqueue(fr_deep_sequence* q, const fr_params* p, const fr_deep_sequence_frame& f, float* rgba, void* nu,
                       int32_t* iter, hipStream_t s)
{
    fr_ctx* c = q->c;
    const uint64_t& gen = deep_slot(c, true, q->ship ? kShip : kMandel).o.gen;
    const uint64_t gen0 = gen;
    const bool timed = c->timing;
    if (timed) FR_HIP_TRY(hipEventRecord(c->ev_begin, s));
    c->timing = false;
    const int st = seq_enqueue_frame(q, p, f, rgba, nu, iter, s);
    c->timing = timed;
    q->n_orbits += gen - gen0;
    if (st != FR_OK) return st;
    if (timed) FR_HIP_TRY(hipEventRecord(c->ev_end, s));
    c->have_timing = timed;
    return FR_OK;
}

/* the parameter part of the kernel argument block (everything that does not depend on the frame geometry) */
static void fill_params(LaunchArgs& a, const fr_params* p)
{
    const bool f64 = p->precision == FR_PRECISION_F64;
    memset(&a, 0, sizeof(a));
    a.center_x = p->center_x; a.center_y = p->center_y; a.zoom = p->zoom;
    a.julia_cx = p->julia_c_real; a.julia_cy = p->julia_c_imag;
    a.bailout = p->bailout;
    a.log_bailout = f64 ? log((double)p->bailout) : (double)logf(p->bailout);
    a.max_iter = p->max_iterations;
    a.aa = p->antialiasing_samples;
    a.palette_mode = p->palette_mode;
    a.color_offset = p->color_offset; a.color_scale = p->color_scale;
    a.interior_style = p->interior_style;
    a.trap_enabled = p->orbit_trap_enabled; a.trap_radius = p->orbit_trap_radius;
    a.stripe_enabled = p->stripe_enabled; a.stripe_density = p->stripe_density;
    a.brightness = p->color_brightness; a.saturation = p->color_saturation; a.contrast = p->color_contrast;
    a.flags = p->flags;
    /* shaders/mandelbrot.comp numbering for Mandelbrot; burning_ship.comp:14-182 == julia.comp:20-181 */
    fr_palette_table_build(p->fractal_type != FR_FRACTAL_MANDELBROT ? 1 : 0, p->palette_mode, &a.pal);
    a.inv_max_iter = 1.0 / (double)p->max_iterations;
    a.inv_log2_bailout = 1.0 / log2((double)p->bailout);
    a.inv_max_iter_f = (float)a.inv_max_iter; a.inv_log2_bailout_f = (float)a.inv_log2_bailout;
    a.color_scale_d = (double)p->color_scale; a.color_offset_d = (double)p->color_offset;
    a.lib_log = !(p->bailout > 1.0f);        /* log2_pos() needs positive arguments: |z|^2 > 1 */
}

/* the grow-only device buffers of the context (growing happens on the first render of a larger geometry, not capturable) */
static int grow_device(void** buf, size_t* cap, size_t need)
{
    if (need <= *cap) return FR_OK;
    if (*buf) { (void)hipFree(*buf); *buf = nullptr; }
    *cap = 0;
    FR_HIP_TRY(hipMalloc(buf, need));
    *cap = need;
    return FR_OK;
}

/* ---- the render of a Mandelbrot / Julia / Burning Ship frame ---------------------------------------------------------
 * enqueue_render: plan (plan_render, fr_plan.h: every decision, no HIP call), route, fill_geometry, the two grow_device calls,
 * begin_frame, launch_tile_pass, launch_pool_pass, finish_render.
 * reserve_only: do everything a render of this geometry would do BEFORE its first launch -- grow the survivor streams,
 * the Deep_Zoom orbit buffers, fill the exact-division cache -- and stop (fr_ctx_reserve).
 * ssaa_of > 1: this IS the sample grid of a supersampled res_w x res_h frame (enqueue_ssaa_staged): lean kernels only, the
 * coordinate tables hold the samples' coordinates */
static int enqueue_ssaa_staged(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H, const fr_shard* norm, uint32_t rows_local,
                               float* rgba, void* nu, int32_t* iter, hipStream_t stream, bool reserve_only, bool out_frame);

/* staged SSAA of a whole frame band by band (plan_route): each band is the one strip of "part b of nbands", rendered
 * straight into the caller's planes, one after the other on the stream */
static int enqueue_ssaa_banded(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H, const RenderPlan& plan, float* rgba,
                               void* nu, int32_t* iter, hipStream_t stream, bool reserve_only)
{
    const bool timed = c->timing;
    if (timed && !reserve_only) FR_HIP_TRY(hipEventRecord(c->ev_begin, stream));
    c->timing = false;                                                   /* one event pair around all bands */
    int st = FR_OK;
    for (uint32_t b = 0; b < plan.nbands && st == FR_OK; ++b) {
        const fr_shard band = {b, plan.nbands, plan.band_rows};
        st = enqueue_ssaa_staged(c, p, W, H, &band, fr_shard_rows(&band, H), rgba, nu, iter, stream, reserve_only, true);
        if (reserve_only) break;                                         /* the first band is the largest */
    }
    c->timing = timed;
    if (st == FR_OK && timed && !reserve_only) {
        FR_HIP_TRY(hipEventRecord(c->ev_end, stream));
        c->have_timing = true;
    }
    return st;
}

/* the geometry part of the kernel argument block, and what the host prepares for the viewport map */
static void fill_geometry(LaunchArgs& a, fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H, const fr_shard& norm,
                          uint32_t rows_local, bool out_frame, int ssaa_of, uint32_t res_w, uint32_t res_h)
{
    const bool f64 = p->precision == FR_PRECISION_F64;
    a.ssaa = ssaa_of > 1 ? ssaa_of : 0;
    a.res_w = (int32_t)res_w; a.res_h = (int32_t)res_h;
    a.W = (int32_t)W; a.H = (int32_t)H; a.rows_local = (int32_t)rows_local;
    a.part = (int32_t)norm.part; a.nparts = (int32_t)norm.nparts; a.rows_per_strip = (int32_t)norm.rows_per_strip;
    a.out_frame = out_frame ? 1 : 0;
    a.log2_tab = c->log2_tab;

    /* escape is absorbing (see escape_run): bailout^2 in [4.5, 1e12], and for Julia |c| <= bailout;
     * Mandelbrot lanes with |c| > bailout retire at i = 0 inside the first, tested block */
    const double B2 = f64 ? (double)p->bailout * (double)p->bailout : (double)(p->bailout * p->bailout);
    const double c2 = a.julia_cx * a.julia_cx + a.julia_cy * a.julia_cy;
    a.fast_ok = (B2 >= 4.5 && B2 <= 1e12 && (p->fractal_type != FR_FRACTAL_JULIA || c2 <= B2)) ? 1 : 0;
    /* 4 bailout^2 as the kernels form it: B * B in the kernel's precision, times 4 (exact) */
    const float b2f = p->bailout * p->bailout;
    a.b2x4_d = 4.0 * ((double)p->bailout * (double)p->bailout);
    a.b2x4_f = 4.0f * b2f;

    /* host-prepared reciprocals; the divide-free viewport map is enabled only when verified exact */
    a.inv_w_d = 1.0 / (double)W;  a.inv_h_d = 1.0 / (double)H;
    a.inv_w_f = 1.0f / (float)W;  a.inv_h_f = 1.0f / (float)H;
    a.aspect_d = (double)W / (double)H;
    a.aspect_f = (float)W / (float)H;
    /* (the uv viewport map of julia.comp:325 / burning_ship.comp:393 has its own quotients) */
    a.exact_div_ok = exact_division_ok(c, W, H, p->fractal_type != FR_FRACTAL_MANDELBROT, f64) ? 1 : 0;
}

/* In front of the tile pass: the begin event, then a zeroed control block (and, for the lean kernels, their coordinate
 * tables) by one of three means. */
static int begin_frame(fr_ctx* c, const RenderPlan& plan, int nstages, bool whole, const fr_params* p, LaunchArgs& a, hipStream_t stream)
{
    /* (a render that writes whole blocks clears their words too: they lie behind the last stage) */
    const uint32_t ctrl_words = (uint32_t)((size_t)(whole ? kWholeStage + kWholeStages : nstages) * kStageWords);
    /* the frame's device time (fr_ctx_last_kernel_ms) includes the small launch that prepares it */
    if (c->timing) FR_HIP_TRY(hipEventRecord(c->ev_begin, stream));
    if (!plan.lean()) { FR_HIP_TRY(clear_control_block(c, stream, nstages, whole)); return FR_OK; }
    a.xs = c->coord_buf;
    a.yds = (uint8_t*)c->coord_buf + (size_t)a.W * (plan.f64 ? sizeof(double) : sizeof(float));
    /* the lean tile pass prepares its own control block and coordinate tables (lean_prologue: its first workgroups, the others
     * wait on a word keyed by a per-context epoch) -- except on a capturing stream: a replayed launch would carry a stale epoch */
    bool in_kernel_prologue = false;
    if (c->tune.prepare != 1u) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusActive; }
        in_kernel_prologue = cap == hipStreamCaptureStatusNone;
    }
    if (!in_kernel_prologue) {
        const hipError_t ep = by_variant(p->fractal_type, plan.f64, [&](auto t, auto f) {
            return launch_prepare<decltype(t), decltype(f)::value>(stream, a, c->d_ctrl, ctrl_words, feedback_of(c)); });
        if (ep != hipSuccess) return fr_set_error(FR_ERR_HIP, "prepare kernel launch failed: %s", hipGetErrorString(ep));
        return FR_OK;
    }
    if (c->prologue_epoch >= 0x0FFFFFF0u) {                 /* 28 bits: start over behind a cleared word */
        FR_HIP_TRY(hipMemsetAsync(c->d_ctrl + kReadyWord, 0, sizeof(uint32_t), stream));
        c->prologue_epoch = 0;
    }
    const Feedback fb = feedback_of(c);
    a.pro_ready = c->d_ctrl + kReadyWord;
    a.pro_epoch = ++c->prologue_epoch << 4;
    a.pro_ctrl = c->d_ctrl;
    a.pro_ctrl_words = ctrl_words;
    a.pro_fb_flag = fb.dev_flag; a.pro_fb_host = fb.host_word; a.pro_prev_seq = fb.prev_seq;
    uint32_t n = 8;
    while (n > plan.grid) n >>= 1;
    a.pro_n = n ? n : 1u;
    return FR_OK;
}

/* the tile pass: [0, b0) of a staged render, whose survivors go to the stream; else the whole render */
static int launch_tile_pass(fr_ctx* c, const RenderPlan& plan, const fr_params* p, LaunchArgs& a, bool pool_looks, hipStream_t stream)
{
    const int fractal = p->fractal_type;                      /* 0 Mandelbrot, 1 Julia, 2 Burning Ship */
    const dim3 grid(plan.grid);
    a.q = plan.tq;
    a.q.heads = stage_heads(c, 0);
    a.i1 = plan.b0[pool_looks];                                /* (from i0 = 0) */
    a.exit_cost = plan.exit_cost;
    a.exit_from = plan.exit_from[pool_looks];
    a.out.overflow = c->overflow_dev;                           /* (the prologue's timeout reports through it too) */
    if (plan.staged()) {
        a.out.base = (uint8_t*)c->stream_buf;
        a.out.n_blocks = stage_counter(c, 0);
        a.out.region_blocks = plan.region_blocks;
        a.out.rotate = plan.rotate_regions;
        a.out.nregions = plan.nregions;
    }
    memset(&a.whole, 0, sizeof(a.whole));
    c->last_whole_cap = 0;
    if (plan.whole_blocks_apply(pool_looks)) {                  /* the pool pass reads the same description */
        a.whole.base = (uint8_t*)c->whole_buf;
        a.whole.heads = stage_heads(c, kWholeStage);
        a.whole.n_blocks = stage_counter(c, kWholeStage);
        a.whole.stats = stage_heads(c, kWholeStage + 1);
        a.whole.region_blocks = c->last_whole_cap = plan.whole_region_blocks;
    }
    a.diag = c->diag;
    a.period_window = plan.tile_period_window;
    const hipError_t e =
        plan.family == kGeneralEffects ? by_variant(fractal, plan.f64, [&](auto t, auto f) {
            constexpr int F = decltype(f)::value == 1 ? 0 : decltype(f)::value;      /* Julia has no effects variant */
            return launch_tile<decltype(t), F, true>(plan.shape, grid, stream, a); })
        : plan.stripes() ? (plan.f64 ? launch_tile_lean_stripes<double>(grid, stream, a) : launch_tile_lean_stripes<float>(grid, stream, a))
        : plan.lean() ? by_variant(fractal, plan.f64, [&](auto t, auto f) {
            return launch_tile_lean<decltype(t), decltype(f)::value>(plan.tile_pixels, grid, stream, a); })
        : by_variant(fractal, plan.f64, [&](auto t, auto f) {      /* kGeneral, kGeneralSampleLoop: launch_tile looks at a.aa */
            return launch_tile<decltype(t), decltype(f)::value, false>(plan.shape, grid, stream, a); });
    if (e != hipSuccess) return fr_set_error(FR_ERR_HIP, "tile kernel launch failed: %s", hipGetErrorString(e));
    return FR_OK;
}

/* the lane-pool pass: the survivors, to max_iter */
static int launch_pool_pass(fr_ctx* c, const RenderPlan& plan, const fr_params* p, LaunchArgs& a, bool pool_looks, hipStream_t stream)
{
    const dim3 sgrid(plan.sgrid);
    a.i0 = plan.b0[pool_looks];
    a.i1 = p->max_iterations;
    a.pro_ready = nullptr;
    a.in = a.out;                                           /* what the tile pass wrote */
    a.in.n_blocks = stage_counter(c, 0);
    memset(&a.out, 0, sizeof(a.out));                       /* the pool pass runs everything out ... */
    a.out.overflow = c->overflow_dev;                       /* ... and reports a stretch loop that will not end */
    a.q = plan.pq;
    a.q.heads = stage_heads(c, 1);
    a.diag = c->diag ? c->diag + c->diag_stride : nullptr;
    a.pool_refill_at = plan.pool_refill_at;
    a.period_window = pool_looks ? period_window(c->tune) : 0u;
    c->last_pool_closing = a.period_window != 0u;
    a.closed_flag = c->d_ctrl + kFeedbackWord;
    const hipError_t e =
        plan.stripes() ? (plan.f64 ? launch_pool_stripes<double>(sgrid, stream, a) : launch_pool_stripes<float>(sgrid, stream, a))
                       : by_variant(p->fractal_type, plan.f64, [&](auto t, auto f) {
                             return launch_stream_pool<decltype(t), decltype(f)::value>(sgrid, stream, a); });
    if (e != hipSuccess) return fr_set_error(FR_ERR_HIP, "lane-pool kernel launch failed: %s", hipGetErrorString(e));
    return FR_OK;
}

static int enqueue_render(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H, const fr_shard* shard,
                          float* rgba, void* nu, int32_t* iter, hipStream_t stream, bool reserve_only = false,
                          bool out_frame = false, int ssaa_of = 0, uint32_t res_w = 0, uint32_t res_h = 0)
{
    if (!reserve_only) {
        const int ov = check_overflow(c);          /* of an earlier asynchronous render nobody has asked about */
        if (ov != FR_OK) return ov;
    }
    fr_shard norm;
    uint32_t rows_local = 0;
    const int sh = normalise_shard(shard, H, &norm, &rows_local);
    if (sh != FR_OK || rows_local == 0) return sh;           /* (rows_local 0: this part owns no rows) */
    /* FOLDED RENDER (fr_plan.h: plan_fold): decided before the plan, which is then the plan of the rows that are rendered --
     * staging, b0, shards, the whole-block rule, grids and scratch sizes all follow them.  (fr_ctx_reserve sizes for the unfolded
     * render, the larger of the two: "fold" may change between the reserve and the render.) */
    uint32_t fold = reserve_only ? 0u : plan_fold(c->tune, p, W, H, norm, ssaa_of);
    FoldDiv fdiv = {0u, 0u};
    if (fold) {
        fdiv = fold_div(W);
        if (c->fold_div_w != W || c->fold_div_rows < fold) {                /* (checked once per geometry) */
            if (fold_div_ok(W, fdiv, (uint64_t)W * fold)) { c->fold_div_w = W; c->fold_div_rows = fold; }
            else fold = 0u;                                                  /* (never seen: fold_div's bound covers every legal frame) */
        }
    }
    if (fold) rows_local = fold;
    const RenderPlan plan = plan_render(c->tune, c->compute_units, p, W, H, norm, rows_local, ssaa_of, out_frame);
    if (fold && plan.family != kLean) return fr_set_error(FR_ERR_INTERNAL, "a folded render reached a kernel family that does not mirror its stores");
    if (plan.route == kRouteDeepZoom)
        return enqueue_deep_zoom(c, p, W, H, &norm, rows_local, rgba, nu, iter, stream, reserve_only, out_frame);
    if (plan.route == kRouteSsaaStaged)
        return enqueue_ssaa_staged(c, p, W, H, &norm, rows_local, rgba, nu, iter, stream, reserve_only, out_frame);
    if (plan.route == kRouteSsaaBanded) return enqueue_ssaa_banded(c, p, W, H, plan, rgba, nu, iter, stream, reserve_only);
    if (ssaa_of > 1 && !plan.lean()) return fr_set_error(FR_ERR_INTERNAL, "staged SSAA reached a render the lean tile kernel does not serve");

    LaunchArgs a;
    fill_params(a, p);
    fill_geometry(a, c, p, W, H, norm, rows_local, out_frame, ssaa_of, res_w, res_h);
    a.rgba = reinterpret_cast<float4*>(rgba); a.nu = nu; a.iter = iter;
    a.fold_rows = fold; a.fold_magic = fdiv.magic; a.fold_shift = fdiv.shift;
    c->last_grid = plan.grid; c->last_pool_closing = -1;
    int st = grow_device(&c->stream_buf, &c->stream_bytes, plan.stream_bytes);      /* the context scratch the plan needs */
    if (st == FR_OK) st = grow_device(&c->whole_buf, &c->whole_bytes, plan.whole_bytes);
    if (st == FR_OK) st = grow_device(&c->coord_buf, &c->coord_bytes, plan.coord_bytes);
    if (st != FR_OK || reserve_only) return st;

    /* does this render's lane pool look for cycles?  (fr_ctx_reserve sizes for the pool that looks: the shorter tile pass
     * leaves more survivors.) */
    const bool pool_looks = plan.pool_may_look && pool_wants_cycle_closing(c, p, W, rows_local);
    const int nstages = plan.staged() && !pool_looks ? plan.nstages_all : plan.nstages;   /* (2 either way but for a forced schedule
                                                     with max_iter < 2 b0 of the pool that runs everything: 1, though both passes run) */
    if ((st = begin_frame(c, plan, nstages, plan.whole_blocks_apply(pool_looks), p, a, stream)) != FR_OK) return st;
    if ((st = launch_tile_pass(c, plan, p, a, pool_looks, stream)) != FR_OK) return st;
    if (plan.staged() && (st = launch_pool_pass(c, plan, p, a, pool_looks, stream)) != FR_OK) return st;
    return finish_render(c, stream, nstages, fold);
}

/* staged SSAA: the sample grid as a render of its own into context scratch, then the average */
static int enqueue_ssaa_staged(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H, const fr_shard* norm, uint32_t rows_local,
                               float* rgba, void* nu, int32_t* iter, hipStream_t stream, bool reserve_only, bool out_frame)
{
    const uint32_t aa = (uint32_t)p->antialiasing_samples;
    const uint32_t Ws = W * aa, Hs = H * aa;
    fr_params q = *p;
    q.antialiasing_samples = 1;
    q.flags &= ~FR_FLAG_POST_CHAIN;                            /* the post chain follows the average */
    const fr_shard sh = {norm->part, norm->nparts, norm->rows_per_strip * aa};
    const size_t nsamp = (size_t)rows_local * aa * Ws;
    const bool f64 = p->precision == FR_PRECISION_F64;
    const size_t nu_elt = f64 ? 8 : 4;
    /* sample planes: colour, then nu, then iter -- only those the caller's planes need */
    const size_t off_nu = rgba ? nsamp * 16 : 0, off_iter = off_nu + (nu ? nsamp * nu_elt : 0), need = off_iter + (iter ? nsamp * 4 : 0);
    int st = grow_device(&c->ssaa_buf, &c->ssaa_bytes, need);
    if (st != FR_OK) return st;
    char* base = (char*)c->ssaa_buf;
    float* s_rgba = rgba ? (float*)base : nullptr;
    void* s_nu = nu ? (void*)(base + off_nu) : nullptr;
    int32_t* s_iter = iter ? (int32_t*)(base + off_iter) : nullptr;
    st = enqueue_render(c, &q, Ws, Hs, &sh, s_rgba, s_nu, s_iter, stream, reserve_only, false, (int)aa, W, H);
    if (st != FR_OK || reserve_only) return st;
    SsaaArgs r;
    r.s_rgba = reinterpret_cast<const float4*>(s_rgba); r.s_nu = s_nu; r.s_iter = s_iter;
    r.rgba = reinterpret_cast<float4*>(rgba); r.nu = nu; r.iter = iter;
    r.W = (int32_t)W; r.rows_local = (int32_t)rows_local; r.aa = (int32_t)aa;
    r.sx_outer = p->fractal_type == FR_FRACTAL_MANDELBROT ? 0 : 1;
    r.part = (int32_t)norm->part; r.nparts = (int32_t)norm->nparts; r.rows_per_strip = (int32_t)norm->rows_per_strip; r.out_frame = out_frame ? 1 : 0;
    r.flags = p->flags; r.brightness = p->color_brightness; r.saturation = p->color_saturation; r.contrast = p->color_contrast;
    r.julia_floors = p->fractal_type != FR_FRACTAL_MANDELBROT ? 1 : 0;
    size_t blocks = ((size_t)rows_local * W + kBlockThreads - 1) / kBlockThreads;
    const size_t cap = (size_t)c->compute_units * 16;
    if (blocks > cap) blocks = cap;
    if (f64) hipLaunchKernelGGL(ssaa_reduce_kernel<double>, dim3((uint32_t)blocks), dim3(kBlockThreads), 0, stream, r);
    else hipLaunchKernelGGL(ssaa_reduce_kernel<float>, dim3((uint32_t)blocks), dim3(kBlockThreads), 0, stream, r);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fr_set_error(FR_ERR_HIP, "SSAA reduce launch failed: %s", hipGetErrorString(e));
    if (c->timing) FR_HIP_TRY(hipEventRecord(c->ev_end, stream));      /* the frame's device time includes the average */
    return FR_OK;
}

/* ---- render entry points --------------------------------------------------------------------------------------------
 * fr_render_shard, fr_render_phoenix, fr_render_mandelbulb, the twelve deep entry points of DeepBlock's paths (fr_render_deep,
 * _deep_de, _deep_ship, _deep_ship_de, _deepx, _deepx_de, _deepx_ship, _deepx_ship_de, _deep_julia, _deepx_julia, _deep_julia_de,
 * _deepx_julia_de; all through deep_entry) and the two of deep Phoenix (fr_render_deep_phoenix, _deepx_phoenix; through
 * deep_phoenix_entry), each with its _async form:
 * their parameter checks, then render_sync / render_async with the planes beyond fr_output's three (ExtraPlanes; the six
 * distance entry points alone have any) and the enqueue step as enqueue(shard, rgba, nu, iter, extra planes, stream, out_frame) */
static int check_common(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H, const fr_output* out)
{
    if (!c) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL");
    if (!p || !out) return fr_set_error(FR_ERR_INVALID_ARG, "params/out is NULL");
    return fr_params_validate(p, W, H);
}

static int check_phoenix(fr_ctx* c, const fr_params* p, const fr_phoenix_params* ph, uint32_t W, uint32_t H,
                         const fr_output* out)
{
    if (!c) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL");
    if (!p || !ph || !out) return fr_set_error(FR_ERR_INVALID_ARG, "params/phoenix params/out is NULL");
    return fr_phoenix_validate(p, ph, W, H);
}

static int check_mandelbulb(fr_ctx* c, const fr_params* p, const fr_mandelbulb_params* mb, uint32_t W, uint32_t H,
                            const fr_output* out)
{
    if (!c) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL");
    if (!p || !mb || !out) return fr_set_error(FR_ERR_INVALID_ARG, "params/mandelbulb params/out is NULL");
    return fr_mandelbulb_validate(p, mb, W, H);
}

static int check_layout(const fr_output* out)
{
    if (out->layout != FR_LAYOUT_PACKED && out->layout != FR_LAYOUT_FRAME)
        return fr_set_error(FR_ERR_INVALID_ARG, "unknown fr_output.layout %d", out->layout);
    if (out->layout == FR_LAYOUT_FRAME && out->memory != FR_MEM_DEVICE)
        return fr_set_error(FR_ERR_INVALID_ARG, "FR_LAYOUT_FRAME needs FR_MEM_DEVICE planes");
    return FR_OK;
}

/* The planes an entry point writes beyond fr_output's three (fr_render_deep_de: deriv, de): where each goes (NULL: not asked
 * for) and its bytes per pixel, a power of two.  They follow out->memory and out->layout as nu does, any one plane of the
 * render is enough, and `none` is the message of a render that has none. */
enum { kMaxExtraPlanes = 2 };
struct ExtraPlanes {
    int n = 0;
    struct { void* dst; size_t bytes; } plane[kMaxExtraPlanes] = {};
    const char* none = "fr_output has no plane to write";
};

/* 1: this part owns rows and has a plane to write; 0: it owns no rows (nothing to do); < 0: error */
static int check_planes(const fr_shard* shard, uint32_t H, const fr_output* out, const ExtraPlanes& extra)
{
    if (shard && shard->nparts && shard->part >= shard->nparts)
        return fr_set_error(FR_ERR_INVALID_ARG, "shard part %u >= nparts %u", shard->part, shard->nparts);
    if (fr_shard_rows(shard, H) == 0) return 0;
    bool any = out->rgba || out->nu || out->iter;
    for (int i = 0; i < extra.n; ++i) any = any || extra.plane[i].dst;
    if (!any) return fr_set_error(FR_ERR_INVALID_ARG, "%s", extra.none);
    return 1;
}

/* device planes only, on the caller's stream (NULL: the context's); returns once the render is enqueued */
template <class Enqueue>
static int render_async(const char* entry, fr_ctx* c, uint32_t H, const fr_shard* shard, const fr_output* out,
                        const ExtraPlanes& extra, void* hip_stream, Enqueue&& enqueue)
{
    int st = check_layout(out);
    if (st != FR_OK) return st;
    if (out->memory != FR_MEM_DEVICE)
        return fr_set_error(FR_ERR_INVALID_ARG, "%s needs FR_MEM_DEVICE outputs", entry);
    st = check_planes(shard, H, out, extra);
    if (st <= 0) return st;
    FR_HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    void* xp[kMaxExtraPlanes] = {extra.plane[0].dst, extra.plane[1].dst};
    st = enqueue(shard, out->rgba, out->nu, out->iter, xp, s, out->layout == FR_LAYOUT_FRAME);
    if (st == FR_OK) c->render_on_user_stream = s != c->stream;
    return st;
}

/* on the context's stream, waited for: device planes are written in place, host planes are staged through device scratch
 * owned by the context (PCIe-inclusive path): rgba, nu, iter at the offsets they always had, each extra plane behind them at
 * the next multiple of its element size */
template <class Enqueue>
static int render_sync(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H, const fr_shard* shard, const fr_output* out,
                       const ExtraPlanes& extra, Enqueue&& enqueue)
{
    int st = check_layout(out);
    if (st != FR_OK) return st;
    st = check_planes(shard, H, out, extra);
    if (st <= 0) return st;
    FR_HIP_TRY(hipSetDevice(c->device));
    const bool host = out->memory == FR_MEM_HOST;
    if (!host && out->memory != FR_MEM_DEVICE)
        return fr_set_error(FR_ERR_INVALID_ARG, "unknown fr_output.memory %d", out->memory);
    float* rgba = out->rgba; void* nu = out->nu; int32_t* iter = out->iter;
    const size_t npx = (size_t)fr_shard_rows(shard, H) * W;
    const size_t nu_bytes = (p->precision == FR_PRECISION_F64 && p->fractal_type != FR_FRACTAL_DEEP_ZOOM) ? 8 : 4;
    void* xp[kMaxExtraPlanes] = {extra.plane[0].dst, extra.plane[1].dst};
    if (host) {
        const size_t off_nu = npx * 16, off_iter = off_nu + npx * 8;
        size_t need = off_iter + npx * 4, off_x[kMaxExtraPlanes] = {0, 0};
        for (int i = 0; i < extra.n; ++i) {
            off_x[i] = (need + extra.plane[i].bytes - 1) / extra.plane[i].bytes * extra.plane[i].bytes;
            need = off_x[i] + npx * extra.plane[i].bytes;
        }
        const int gs = grow_device(&c->scratch, &c->scratch_bytes, need);
        if (gs != FR_OK) return gs;
        char* base = (char*)c->scratch;
        rgba = out->rgba ? (float*)base : nullptr;
        nu = out->nu ? (void*)(base + off_nu) : nullptr;
        iter = out->iter ? (int32_t*)(base + off_iter) : nullptr;
        for (int i = 0; i < extra.n; ++i) xp[i] = extra.plane[i].dst ? base + off_x[i] : nullptr;
    }
    st = enqueue(shard, rgba, nu, iter, xp, c->stream, out->layout == FR_LAYOUT_FRAME);   /* (host planes are packed) */
    if (st != FR_OK) return st;
    c->render_on_user_stream = false;
    if (host) {
        if (out->rgba) FR_HIP_TRY(hipMemcpyAsync(out->rgba, rgba, npx * 16, hipMemcpyDeviceToHost, c->stream));
        if (out->nu) FR_HIP_TRY(hipMemcpyAsync(out->nu, nu, npx * nu_bytes, hipMemcpyDeviceToHost, c->stream));
        if (out->iter) FR_HIP_TRY(hipMemcpyAsync(out->iter, iter, npx * 4, hipMemcpyDeviceToHost, c->stream));
        for (int i = 0; i < extra.n; ++i)
            if (extra.plane[i].dst)
                FR_HIP_TRY(hipMemcpyAsync(extra.plane[i].dst, xp[i], npx * extra.plane[i].bytes, hipMemcpyDeviceToHost, c->stream));
    }
    FR_HIP_TRY(hipStreamSynchronize(c->stream));
    return check_overflow(c);
}

extern "C" int fr_render_shard_async(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H,
                                     const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    const int st = check_common(c, p, W, H, out);
    if (st != FR_OK) return st;
    return render_async("fr_render_shard_async", c, H, shard, out, {}, hip_stream,
                        [&](auto sh, auto rgba, auto nu, auto iter, auto, auto s, bool out_frame) {
                            return enqueue_render(c, p, W, H, sh, rgba, nu, iter, s, false, out_frame); });
}

extern "C" int fr_ctx_reserve(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H, const fr_shard* shard)
{
    if (!c || !p) return fr_set_error(FR_ERR_INVALID_ARG, "fr_ctx_reserve: ctx/params is NULL");
    int st = fr_params_validate(p, W, H);
    if (st != FR_OK) return st;
    if (shard && shard->nparts && shard->part >= shard->nparts)
        return fr_set_error(FR_ERR_INVALID_ARG, "shard part %u >= nparts %u", shard->part, shard->nparts);
    FR_HIP_TRY(hipSetDevice(c->device));
    /* growing a buffer frees the old one, which a render still in flight may be reading: wait for the context's own
     * stream and, when the most recent render went to a caller's stream, for the event recorded behind it there */
    FR_HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->render_on_user_stream && c->have_render) FR_HIP_TRY(hipStreamSynchronize(c->last_stream));
    return enqueue_render(c, p, W, H, shard, nullptr, nullptr, nullptr, c->stream, true);
}

/* ---- fr_plan_describe (fr_tuning.h): the plan of a render as a flat record of integers, with no context and no device.
 * Of a staged or banded SSAA render the record holds the route and, from "W" on, the plan of the sample-grid render
 * (of the first band, which is the largest).  A part that owns no rows: all zero. */
static const char kPlanFields[] =
    "route nbands band_rows W H rows_local rows_per_strip family shape tile_pixels nstages nstages_all wg_per_cu grid sgrid nregions "
    "rotate_regions bounded moderate exit_cost exit_from_look exit_from_all pool_refill_at tile_period_window pool_may_look "
    "b0_look b0_all region_blocks stream_bytes coord_bytes tq_nsx tq_nsx_shift tq_n_items tq_n_blk tq_ns_log2 tq_run_shift "
    "tq_run_min tq_run_max tq_flags pq_ns_log2 pq_run_shift pq_run_min pq_run_max pq_flags";
constexpr int kPlanFieldCount = 44;

extern "C" const char* fr_plan_fields(void) { return kPlanFields; }

/* the automatic choices with n names of fr_ctx_set_tuning / fr_ctx_set_option applied in order */
static int tunings_from(Tuning& tune, const char* const* names, const int64_t* values, int n)
{
    memset(&tune, 0, sizeof(tune));
    for (int i = 0; i < n; ++i) {
        int st = tuning_set(tune, names[i], values[i]);
        if (st == kNotMine) st = option_set(tune, names[i], values[i]);
        if (st == kNotMine) return fr_set_error(FR_ERR_INVALID_ARG, "unknown tuning name '%s'", names[i]);
        if (st != FR_OK) return st;
    }
    return FR_OK;
}

/* The plan of the render that runs the kernels of a request: the request's own, or -- staged and banded SSAA -- the sample
 * grid's (of the first band, the largest), as enqueue_ssaa_staged makes it.  W, H, norm and rows_local become that render's;
 * *outer receives the request's own plan (route, nbands, band_rows). */
static int plan_of_kernels(const Tuning& tune, int compute_units, const fr_params* p, uint32_t& W, uint32_t& H, fr_shard& norm,
                           uint32_t& rows_local, RenderPlan* outer, RenderPlan* r)
{
    *r = *outer = plan_render(tune, compute_units, p, W, H, norm, rows_local, 0);
    if (outer->route != kRouteSsaaStaged && outer->route != kRouteSsaaBanded) return FR_OK;
    const fr_shard band = {0, outer->nbands, outer->band_rows};
    if (outer->route == kRouteSsaaBanded) { norm = band; rows_local = fr_shard_rows(&band, H); }
    const uint32_t aa = (uint32_t)p->antialiasing_samples;
    const fr_shard grid_shard = {norm.part, norm.nparts, norm.rows_per_strip * aa};
    fr_params q = *p;
    q.antialiasing_samples = 1;
    W *= aa; H *= aa;
    const int gs = normalise_shard(&grid_shard, H, &norm, &rows_local);
    if (gs != FR_OK) return gs;
    *r = plan_render(tune, compute_units, &q, W, H, norm, rows_local, p->antialiasing_samples);
    if (!r->lean()) return fr_set_error(FR_ERR_INTERNAL, "staged SSAA reached a render the lean tile kernel does not serve");
    return FR_OK;
}

/* fr_tuning.h: does the render of this request (of its sample grid, where SSAA is staged) write the survivor stream in two classes? */
extern "C" int fr_plan_whole_blocks(const fr_params* p, uint32_t W, uint32_t H, const fr_shard* shard, int compute_units,
                                    const char* const* names, const int64_t* values, int n_tunings, int pool_looks)
{
    if (!p || (n_tunings > 0 && (!names || !values))) return fr_set_error(FR_ERR_INVALID_ARG, "fr_plan_whole_blocks: NULL argument");
    Tuning tune;
    const int ts = tunings_from(tune, names, values, n_tunings);
    if (ts != FR_OK) return ts;
    fr_shard norm;
    uint32_t rows_local = 0;
    const int sh = normalise_shard(shard, H, &norm, &rows_local);
    if (sh != FR_OK || rows_local == 0) return sh;
    RenderPlan outer, r;
    const int st = plan_of_kernels(tune, compute_units, p, W, H, norm, rows_local, &outer, &r);
    if (st != FR_OK) return st;
    if (outer.route == kRouteDeepZoom) return 0;
    return r.whole_blocks_apply(r.pool_may_look && pool_looks != 0) ? 1 : 0;
}

/* fr_tuning.h: the fold decision of a request (plan_fold), with no context and no device */
extern "C" int fr_fold_describe(const fr_params* p, uint32_t W, uint32_t H, const fr_shard* shard, const char* const* names,
                                const int64_t* values, int n_tunings, int64_t out[2])
{
    if (!p || !out || (n_tunings > 0 && (!names || !values))) return fr_set_error(FR_ERR_INVALID_ARG, "fr_fold_describe: NULL argument");
    Tuning tune;
    const int ts = tunings_from(tune, names, values, n_tunings);
    if (ts != FR_OK) return ts;
    out[0] = out[1] = 0;
    fr_shard norm;
    uint32_t rows_local = 0;
    const int sh = normalise_shard(shard, H, &norm, &rows_local);
    if (sh != FR_OK || rows_local == 0) return sh;
    const uint32_t fold = p->fractal_type == FR_FRACTAL_DEEP_ZOOM ? 0u : plan_fold(tune, p, W, H, norm, 0);
    out[0] = fold != 0u;
    out[1] = fold ? fold : rows_local;
    return FR_OK;
}

/* fr_tuning.h: the folded render's division of a plane index by W; returns whether it is exact for every index below n_indices */
extern "C" int fr_fold_division(uint32_t W, uint64_t n_indices, uint32_t* magic, uint32_t* shift)
{
    if (W == 0u || W > (1u << 31) || !magic || !shift) return fr_set_error(FR_ERR_INVALID_ARG, "fr_fold_division: W in [1, 2^31], magic and shift not NULL");
    const FoldDiv d = fold_div(W);
    *magic = d.magic; *shift = d.shift;
    return fold_div_ok(W, d, n_indices) ? 1 : 0;
}

/* fr_tuning.h: rows the most recent render rendered as a folded render, 0: it was not one */
extern "C" int fr_ctx_last_fold(const fr_ctx* c) { return c ? (int)c->last_fold : 0; }

extern "C" int fr_plan_describe(const fr_params* p, uint32_t W, uint32_t H, const fr_shard* shard, int compute_units,
                                const char* const* names, const int64_t* values, int n_tunings, int64_t* out, int n_out)
{
    if (!p || !out || (n_tunings > 0 && (!names || !values))) return fr_set_error(FR_ERR_INVALID_ARG, "fr_plan_describe: NULL argument");
    if (n_out != kPlanFieldCount) return fr_set_error(FR_ERR_INVALID_ARG, "fr_plan_describe: the record has %d fields", kPlanFieldCount);
    Tuning tune;
    const int ts = tunings_from(tune, names, values, n_tunings);
    if (ts != FR_OK) return ts;
    memset(out, 0, sizeof(int64_t) * kPlanFieldCount);
    fr_shard norm;
    uint32_t rows_local = 0;
    const int sh = normalise_shard(shard, H, &norm, &rows_local);
    if (sh != FR_OK || rows_local == 0) return sh;
    RenderPlan outer, r;
    const int st = plan_of_kernels(tune, compute_units, p, W, H, norm, rows_local, &outer, &r);
    if (st != FR_OK) return st;
    const int route = outer.route;
    const uint32_t nbands = outer.nbands, band_rows = outer.band_rows;
    int64_t* o = out;
    *o++ = route; *o++ = nbands; *o++ = band_rows;
    if (route == kRouteDeepZoom) return FR_OK;
    const int64_t rest[] = {W, H, rows_local, norm.rows_per_strip, r.family, r.shape, r.tile_pixels, r.nstages, r.nstages_all, r.wg_per_cu, r.grid,
                            r.sgrid, r.nregions, r.rotate_regions, r.bounded, r.moderate, r.exit_cost, r.exit_from[1], r.exit_from[0],
                            r.pool_refill_at, r.tile_period_window, r.pool_may_look, r.b0[1], r.b0[0], r.region_blocks,
                            (int64_t)r.stream_bytes, (int64_t)r.coord_bytes, r.tq.nsx, r.tq.nsx_shift, r.tq.n_items, r.tq.n_blk,
                            r.tq.ns_log2, r.tq.run_shift, r.tq.run_min, r.tq.run_max, r.tq.flags, r.pq.ns_log2, r.pq.run_shift,
                            r.pq.run_min, r.pq.run_max, r.pq.flags};
    static_assert(sizeof(rest) / sizeof(rest[0]) == kPlanFieldCount - 3, "one value per name of kPlanFields");
    memcpy(o, rest, sizeof(rest));
    return FR_OK;
}

/* the step counts behind a slot's most recent render; `what` names the call and flag that fill them */
static int last_bla_steps(fr_ctx* c, bool ext, int f, const char* what, uint64_t out[3])
{
    if (!c || !out) return fr_set_error(FR_ERR_INVALID_ARG, "ctx/out is NULL");
    const BlaSlot& t = deep_slot(c, ext, f).t;
    if (!t.have_steps) return fr_set_error(FR_ERR_UNSUPPORTED, "no %s on this context yet", what);
    for (int i = 0; i < 3; ++i) out[i] = (uint64_t)t.steps_host[i];
    return FR_OK;
}

/* tests: the first n entries of a slot's table, as the device holds them; returns the entries the table has */
static int64_t read_bla_table(fr_ctx* c, bool ext, int f, void* r, double* ab, int32_t* ab_exp, int64_t n)
{
    if (!c) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL");
    const BlaSlot& t = deep_slot(c, ext, f).t;
    if (!t.valid) return 0;
    const DeepOrbit& o = deep_slot(c, ext, f).o;
    int64_t have = (int64_t)bla_entries(o.len - 1);
    if (f == kJulia) {                                            /* Q's entries, then P's; none once the slot's orbits changed */
        if (t.key_gen != o.gen) return 0;
        have += (int64_t)bla_entries(o.len_p - 1);
    }
    if (n > have) n = have;
    const size_t nab = kFormula[f].ab_per_entry;
    const size_t nexp = f == kJulia ? sizeof(int32_t) : sizeof(int2);
    FR_HIP_TRY(hipSetDevice(c->device));
    FR_HIP_TRY(hipDeviceSynchronize());
    if (n > 0 && r) FR_HIP_TRY(hipMemcpy(r, t.r, (size_t)n * (ext ? sizeof(XRad) : sizeof(double)), hipMemcpyDeviceToHost));
    if (n > 0 && ab) FR_HIP_TRY(hipMemcpy(ab, t.ab, (size_t)n * nab * sizeof(double2), hipMemcpyDeviceToHost));
    if (n > 0 && ext && ab_exp) FR_HIP_TRY(hipMemcpy(ab_exp, t.abe, (size_t)n * nexp, hipMemcpyDeviceToHost));
    return have;
}

extern "C" int fr_ctx_last_deep_steps(fr_ctx* c, uint64_t out[3])
{
    return last_bla_steps(c, false, kMandel, "fr_render_deep call with FR_FLAG_DEEP_BLA", out);
}

extern "C" int fr_ctx_last_deep_ship_steps(fr_ctx* c, uint64_t out[3])
{
    return last_bla_steps(c, false, kShip, "fr_render_deep_ship call with FR_FLAG_DEEP_SHIP_BLA", out);
}

extern "C" int fr_ctx_last_deep_phoenix_steps(fr_ctx* c, uint64_t out[3])
{
    return last_bla_steps(c, false, kPhoenix, "fr_render_deep_phoenix call with FR_FLAG_DEEP_PHOENIX_BLA", out);
}

extern "C" int fr_ctx_last_deepx_phoenix_steps(fr_ctx* c, uint64_t out[3])
{
    return last_bla_steps(c, true, kPhoenix, "fr_render_deepx_phoenix call with FR_FLAG_DEEPX_PHOENIX_BLA", out);
}

extern "C" int fr_ctx_last_deepx_steps(fr_ctx* c, uint64_t out[3])
{
    return last_bla_steps(c, true, kMandel, "fr_render_deepx call with FR_FLAG_DEEPX_BLA", out);
}

extern "C" int fr_ctx_last_deepx_ship_steps(fr_ctx* c, uint64_t out[3])
{
    return last_bla_steps(c, true, kShip, "fr_render_deepx_ship call with FR_FLAG_DEEPX_SHIP_BLA", out);
}

extern "C" int64_t fr_deep_orbit_generation(fr_ctx* c, int extended, int formula)
{
    if (!c || formula < kMandel || formula >= kFormulas) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL or no such formula");
    return (int64_t)deep_slot(c, extended != 0, formula).o.gen;
}

extern "C" int64_t fr_deep_bla_builds(fr_ctx* c, int extended, int formula)
{
    if (!c || formula < kMandel || formula >= kFormulas) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL or no such formula");
    return (int64_t)deep_slot(c, extended != 0, formula).t.builds;
}

extern "C" int fr_ctx_last_deep_julia_steps(fr_ctx* c, uint64_t out[3])
{
    return last_bla_steps(c, false, kJulia, "fr_render_deep_julia call with FR_FLAG_DEEP_JULIA_BLA", out);
}

extern "C" int fr_ctx_last_deepx_julia_steps(fr_ctx* c, uint64_t out[3])
{
    return last_bla_steps(c, true, kJulia, "fr_render_deepx_julia call with FR_FLAG_DEEPX_JULIA_BLA", out);
}

extern "C" int64_t fr_deep_julia_bla_table(fr_ctx* c, double* r, double* a, int64_t n)
{
    return read_bla_table(c, false, kJulia, r, a, nullptr, n);
}

extern "C" int64_t fr_deepx_julia_bla_table(fr_ctx* c, void* r, double* a, int32_t* a_exp, int64_t n)
{
    return read_bla_table(c, true, kJulia, r, a, a_exp, n);
}

extern "C" int64_t fr_deep_bla_table(fr_ctx* c, double* r, double* ab, int64_t n)
{
    return read_bla_table(c, false, kMandel, r, ab, nullptr, n);
}

extern "C" int64_t fr_deep_ship_bla_table(fr_ctx* c, double* r, double* ab, int64_t n)
{
    return read_bla_table(c, false, kShip, r, ab, nullptr, n);
}

extern "C" int64_t fr_deep_phoenix_bla_table(fr_ctx* c, double* r, double* mb, int64_t n)
{
    return read_bla_table(c, false, kPhoenix, r, mb, nullptr, n);
}

extern "C" int64_t fr_deepx_phoenix_bla_table(fr_ctx* c, void* r, double* mb, int32_t* mb_exp, int64_t n)
{
    return read_bla_table(c, true, kPhoenix, r, mb, mb_exp, n);
}

extern "C" int64_t fr_deepx_bla_table(fr_ctx* c, void* r, double* ab, int32_t* ab_exp, int64_t n)
{
    return read_bla_table(c, true, kMandel, r, ab, ab_exp, n);
}

extern "C" int64_t fr_deepx_ship_bla_table(fr_ctx* c, void* r, double* ab, int32_t* ab_exp, int64_t n)
{
    return read_bla_table(c, true, kShip, r, ab, ab_exp, n);
}

extern "C" int fr_ctx_check(fr_ctx* c)
{
    if (!c) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL");
    return check_overflow(c);
}

extern "C" int fr_ctx_synchronize(fr_ctx* c)
{
    if (!c) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL");
    FR_HIP_TRY(hipSetDevice(c->device));
    FR_HIP_TRY(hipStreamSynchronize(c->stream));
    return check_overflow(c);
}

/* fr_tuning.h: 1 / 0 = the lane pool of the most recent render looked / did not look for cycles, -1 = it had no lane pool */
extern "C" int fr_ctx_last_pool_closing(const fr_ctx* c) { return c ? c->last_pool_closing : -1; }

/* fr_tuning.h: the two classes of the most recent render's survivor stream, read from its control words (waits for it) */
extern "C" int fr_ctx_last_whole_blocks(fr_ctx* c, uint64_t out[3])
{
    if (!c || !out) return fr_set_error(FR_ERR_INVALID_ARG, "ctx/out is NULL");
    out[0] = out[1] = out[2] = 0;
    if (!c->have_render || c->last_whole_cap == 0u) return FR_OK;     /* one class: nothing was counted */
    FR_HIP_TRY(hipSetDevice(c->device));
    FR_HIP_TRY(hipStreamSynchronize(c->last_stream));
    const size_t bytes = (size_t)kWholeStages * kStageWords * sizeof(uint32_t);
    uint32_t* const words = (uint32_t*)malloc(bytes);
    if (!words) return fr_set_error(FR_ERR_NOMEM, "fr_ctx_last_whole_blocks: out of host memory");
    const hipError_t e = hipMemcpy(words, stage_heads(c, kWholeStage), bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { free(words); return fr_set_error(FR_ERR_HIP, "fr_ctx_last_whole_blocks: %s", hipGetErrorString(e)); }
    const size_t group = (size_t)kMaxShards * kShardStrideWords;
    for (int r = 0; r < kMaxShards; ++r) {
        const uint32_t n = words[group + (size_t)r * kShardStrideWords];             /* claims past the cap wrote nothing */
        out[0] += n < c->last_whole_cap ? n : c->last_whole_cap;
        out[1] += words[2 * group + (size_t)r * kShardStrideWords];
        out[2] += words[3 * group + (size_t)r * kShardStrideWords];
    }
    free(words);
    return FR_OK;
}

extern "C" void* fr_ctx_stream_handle(fr_ctx* c) { return c ? (void*)c->stream : nullptr; }
extern "C" int fr_ctx_device(const fr_ctx* c) { return c ? c->device : -1; }

extern "C" int fr_render_shard(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H,
                               const fr_shard* shard, const fr_output* out)
{
    const int st = check_common(c, p, W, H, out);
    if (st != FR_OK) return st;
    return render_sync(c, p, W, H, shard, out, {}, [&](auto sh, auto rgba, auto nu, auto iter, auto, auto s, bool out_frame) {
        return enqueue_render(c, p, W, H, sh, rgba, nu, iter, s, false, out_frame); });
}

extern "C" int fr_render(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H, const fr_output* out)
{
    return fr_render_shard(c, p, W, H, nullptr, out);
}

extern "C" int fr_render_phoenix_async(fr_ctx* c, const fr_params* p, const fr_phoenix_params* ph, uint32_t W, uint32_t H,
                                       const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    const int st = check_phoenix(c, p, ph, W, H, out);
    if (st != FR_OK) return st;
    return render_async("fr_render_phoenix_async", c, H, shard, out, {}, hip_stream,
                        [&](auto sh, auto rgba, auto nu, auto iter, auto, auto s, bool out_frame) {
                            return enqueue_phoenix(c, p, ph, W, H, sh, rgba, nu, iter, s, out_frame); });
}

extern "C" int fr_render_phoenix(fr_ctx* c, const fr_params* p, const fr_phoenix_params* ph, uint32_t W, uint32_t H,
                                 const fr_shard* shard, const fr_output* out)
{
    const int st = check_phoenix(c, p, ph, W, H, out);
    if (st != FR_OK) return st;
    return render_sync(c, p, W, H, shard, out, {}, [&](auto sh, auto rgba, auto nu, auto iter, auto, auto s, bool out_frame) {
        return enqueue_phoenix(c, p, ph, W, H, sh, rgba, nu, iter, s, out_frame); });
}

extern "C" int fr_render_mandelbulb_async(fr_ctx* c, const fr_params* p, const fr_mandelbulb_params* mb, uint32_t W,
                                          uint32_t H, const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    const int st = check_mandelbulb(c, p, mb, W, H, out);
    if (st != FR_OK) return st;
    return render_async("fr_render_mandelbulb_async", c, H, shard, out, {}, hip_stream,
                        [&](auto sh, auto rgba, auto nu, auto iter, auto, auto s, bool out_frame) {
                            return enqueue_mandelbulb(c, p, mb, W, H, sh, rgba, nu, iter, s, out_frame); });
}

extern "C" int fr_render_mandelbulb(fr_ctx* c, const fr_params* p, const fr_mandelbulb_params* mb, uint32_t W, uint32_t H,
                                    const fr_shard* shard, const fr_output* out)
{
    const int st = check_mandelbulb(c, p, mb, W, H, out);
    if (st != FR_OK) return st;
    return render_sync(c, p, W, H, shard, out, {}, [&](auto sh, auto rgba, auto nu, auto iter, auto, auto s, bool out_frame) {
        return enqueue_mandelbulb(c, p, mb, W, H, sh, rgba, nu, iter, s, out_frame); });
}

/* The twenty-four deep entry points of DeepBlock's paths (deep Phoenix has four more, deep_phoenix_entry below): BASE names the
 * path (DeepPath), async_entry the _async form (nullptr: the synchronous one), validate() runs the path's validator once the
 * pointers are known not to be NULL, and the enqueue step is enqueue_deep_view of the view read into a DeepAt (deep_at_of).  e: the block of the six distance entry points (fr_render_deep_de, _deepx_de, _deep_julia_de,
 * _deepx_julia_de, _deep_ship_de, _deepx_ship_de), whose two planes travel as extra planes into the derivative's fields; nullptr for every other path. */
template <class BASE, class VIEW, class Validate>
static int deep_entry(const char* async_entry, fr_ctx* c, const fr_params* p, const VIEW* v, const fr_deep_de* e, uint32_t W,
                      uint32_t H, const fr_shard* shard, const fr_output* out, void* hip_stream, Validate&& validate)
{
    constexpr bool de = DeepPath<BASE>::de != 0;
    if (!c) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL");
    if (!p || !v || !out || (de && !e))
        return fr_set_error(FR_ERR_INVALID_ARG, de ? "params/deep view/de/out is NULL" : "params/deep view/out is NULL");
    const int st = validate();
    if (st != FR_OK) return st;
    ExtraPlanes extra;
    if constexpr (de)
        extra = {2, {{e->deriv, DeepPath<BASE>::f == kShip ? 32u : 16u}, {e->de, 8}},
                 DeepPath<BASE>::f == kShip
                     ? (DeepPath<BASE>::ext ? "fr_render_deepx_ship_de: neither fr_output nor fr_deep_de has a plane to write"
                                            : "fr_render_deep_ship_de: neither fr_output nor fr_deep_de has a plane to write")
                 : DeepPath<BASE>::f == kJulia
                     ? (DeepPath<BASE>::ext ? "fr_render_deepx_julia_de: neither fr_output nor fr_deep_de has a plane to write"
                                            : "fr_render_deep_julia_de: neither fr_output nor fr_deep_de has a plane to write")
                     : (DeepPath<BASE>::ext ? "fr_render_deepx_de: neither fr_output nor fr_deep_de has a plane to write"
                                            : "fr_render_deep_de: neither fr_output nor fr_deep_de has a plane to write")};
    auto enqueue = [&](auto sh, auto rgba, auto nu, auto iter, void* const* xp, auto s, bool out_frame) {
        DeepAt at;
        const int rs = deep_at_of(p, v, &at);
        if (rs != FR_OK) return rs;
        return enqueue_deep_view<BASE>(c, p, at, W, H, sh, rgba, nu, iter, s, out_frame, [&](BASE& a) {
            if constexpr (de) {                  /* s = zoom / H of the whole frame, whatever rows this part owns */
                if constexpr (DeepPath<BASE>::ext) {     /* norm1(zm / H, ze) */
                    int k = 0;
                    a.sm = frexp(at.zm / (double)H, &k);
                    a.es = at.ze + k;
                } else {
                    a.s = p->zoom / (double)H;
                }
                a.deriv = (double*)xp[0]; a.de = (double*)xp[1];
                a.shade = e->shade; a.edge_px = e->edge_px;
            }
        });
    };
    return async_entry ? render_async(async_entry, c, H, shard, out, extra, hip_stream, enqueue)
                       : render_sync(c, p, W, H, shard, out, extra, enqueue);
}

extern "C" int fr_render_deep_async(fr_ctx* c, const fr_params* p, const fr_deep_view* v, uint32_t W, uint32_t H,
                                    const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    return deep_entry<DeepMandel>("fr_render_deep_async", c, p, v, nullptr, W, H, shard, out, hip_stream,
                                [&] { return fr_deep_validate(p, v, W, H); });
}

extern "C" int fr_render_deep(fr_ctx* c, const fr_params* p, const fr_deep_view* v, uint32_t W, uint32_t H,
                              const fr_shard* shard, const fr_output* out)
{
    return deep_entry<DeepMandel>(nullptr, c, p, v, nullptr, W, H, shard, out, nullptr,
                                [&] { return fr_deep_validate(p, v, W, H); });
}

/* fr_render_deep_de: five planes -- de and deriv follow out->memory and out->layout as nu does, and any one plane is enough */
extern "C" int fr_render_deep_de_async(fr_ctx* c, const fr_params* p, const fr_deep_view* v, const fr_deep_de* e, uint32_t W,
                                       uint32_t H, const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    return deep_entry<DeepMandelDe>("fr_render_deep_de_async", c, p, v, e, W, H, shard, out, hip_stream,
                                  [&] { return fr_deep_de_validate(p, v, e, W, H); });
}

extern "C" int fr_render_deep_de(fr_ctx* c, const fr_params* p, const fr_deep_view* v, const fr_deep_de* e, uint32_t W, uint32_t H,
                                 const fr_shard* shard, const fr_output* out)
{
    return deep_entry<DeepMandelDe>(nullptr, c, p, v, e, W, H, shard, out, nullptr,
                                  [&] { return fr_deep_de_validate(p, v, e, W, H); });
}

extern "C" int fr_render_deep_ship_async(fr_ctx* c, const fr_params* p, const fr_deep_view* v, uint32_t W, uint32_t H,
                                         const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    return deep_entry<DeepShip>("fr_render_deep_ship_async", c, p, v, nullptr, W, H, shard, out, hip_stream,
                                    [&] { return fr_deep_ship_validate(p, v, W, H); });
}

extern "C" int fr_render_deep_ship(fr_ctx* c, const fr_params* p, const fr_deep_view* v, uint32_t W, uint32_t H,
                                   const fr_shard* shard, const fr_output* out)
{
    return deep_entry<DeepShip>(nullptr, c, p, v, nullptr, W, H, shard, out, nullptr,
                                    [&] { return fr_deep_ship_validate(p, v, W, H); });
}

extern "C" int fr_render_deepx_async(fr_ctx* c, const fr_params* p, const fr_deepx_view* v, uint32_t W, uint32_t H,
                                     const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    return deep_entry<DeepMandelX>("fr_render_deepx_async", c, p, v, nullptr, W, H, shard, out, hip_stream,
                                 [&] { return fr_deepx_validate(p, v, W, H); });
}

extern "C" int fr_render_deepx(fr_ctx* c, const fr_params* p, const fr_deepx_view* v, uint32_t W, uint32_t H,
                               const fr_shard* shard, const fr_output* out)
{
    return deep_entry<DeepMandelX>(nullptr, c, p, v, nullptr, W, H, shard, out, nullptr,
                                 [&] { return fr_deepx_validate(p, v, W, H); });
}

/* fr_render_deepx_de: fr_render_deep_de's five planes on fr_render_deepx's path */
extern "C" int fr_render_deepx_de_async(fr_ctx* c, const fr_params* p, const fr_deepx_view* v, const fr_deep_de* e, uint32_t W,
                                        uint32_t H, const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    return deep_entry<DeepMandelXDe>("fr_render_deepx_de_async", c, p, v, e, W, H, shard, out, hip_stream,
                                   [&] { return fr_deepx_de_validate(p, v, e, W, H); });
}

extern "C" int fr_render_deepx_de(fr_ctx* c, const fr_params* p, const fr_deepx_view* v, const fr_deep_de* e, uint32_t W,
                                  uint32_t H, const fr_shard* shard, const fr_output* out)
{
    return deep_entry<DeepMandelXDe>(nullptr, c, p, v, e, W, H, shard, out, nullptr,
                                   [&] { return fr_deepx_de_validate(p, v, e, W, H); });
}

extern "C" int fr_render_deepx_ship_async(fr_ctx* c, const fr_params* p, const fr_deepx_view* v, uint32_t W, uint32_t H,
                                          const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    return deep_entry<DeepShipX>("fr_render_deepx_ship_async", c, p, v, nullptr, W, H, shard, out, hip_stream,
                                     [&] { return fr_deepx_ship_validate(p, v, W, H); });
}

extern "C" int fr_render_deepx_ship(fr_ctx* c, const fr_params* p, const fr_deepx_view* v, uint32_t W, uint32_t H,
                                    const fr_shard* shard, const fr_output* out)
{
    return deep_entry<DeepShipX>(nullptr, c, p, v, nullptr, W, H, shard, out, nullptr,
                                     [&] { return fr_deepx_ship_validate(p, v, W, H); });
}

extern "C" int fr_render_deep_julia_async(fr_ctx* c, const fr_params* p, const fr_deep_view* v, uint32_t W, uint32_t H,
                                          const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    return deep_entry<DeepJulia>("fr_render_deep_julia_async", c, p, v, nullptr, W, H, shard, out, hip_stream,
                                     [&] { return fr_deep_julia_validate(p, v, W, H); });
}

extern "C" int fr_render_deep_julia(fr_ctx* c, const fr_params* p, const fr_deep_view* v, uint32_t W, uint32_t H,
                                    const fr_shard* shard, const fr_output* out)
{
    return deep_entry<DeepJulia>(nullptr, c, p, v, nullptr, W, H, shard, out, nullptr,
                                     [&] { return fr_deep_julia_validate(p, v, W, H); });
}

extern "C" int fr_render_deepx_julia_async(fr_ctx* c, const fr_params* p, const fr_deepx_view* v, uint32_t W, uint32_t H,
                                           const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    return deep_entry<DeepJuliaX>("fr_render_deepx_julia_async", c, p, v, nullptr, W, H, shard, out, hip_stream,
                                      [&] { return fr_deepx_julia_validate(p, v, W, H); });
}

extern "C" int fr_render_deepx_julia(fr_ctx* c, const fr_params* p, const fr_deepx_view* v, uint32_t W, uint32_t H,
                                     const fr_shard* shard, const fr_output* out)
{
    return deep_entry<DeepJuliaX>(nullptr, c, p, v, nullptr, W, H, shard, out, nullptr,
                                      [&] { return fr_deepx_julia_validate(p, v, W, H); });
}

/* fr_render_deep_phoenix, fr_render_deepx_phoenix: fr_render_phoenix's arguments with a deep view.  deep_entry's steps with
 * the Phoenix parameters: X names the storage, validate() runs the entry's validator, the enqueue step is enqueue_deep_phoenix. */
template <bool X, class VIEW, class Validate>
static int deep_phoenix_entry(const char* async_entry, fr_ctx* c, const fr_params* p, const fr_phoenix_params* ph, const VIEW* v,
                              uint32_t W, uint32_t H, const fr_shard* shard, const fr_output* out, void* hip_stream,
                              Validate&& validate)
{
    if (!c) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL");
    if (!p || !ph || !v || !out) return fr_set_error(FR_ERR_INVALID_ARG, "params/phoenix params/deep view/out is NULL");
    const int st = validate();
    if (st != FR_OK) return st;
    auto enqueue = [&](auto sh, auto rgba, auto nu, auto iter, auto, auto s, bool out_frame) {
        DeepAt at;
        const int rs = deep_at_of(p, v, &at);
        if (rs != FR_OK) return rs;
        return enqueue_deep_phoenix<X>(c, p, ph, at, W, H, sh, rgba, nu, iter, s, out_frame);
    };
    return async_entry ? render_async(async_entry, c, H, shard, out, {}, hip_stream, enqueue)
                       : render_sync(c, p, W, H, shard, out, {}, enqueue);
}

extern "C" int fr_render_deep_phoenix_async(fr_ctx* c, const fr_params* p, const fr_phoenix_params* ph, const fr_deep_view* v,
                                            uint32_t W, uint32_t H, const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    return deep_phoenix_entry<false>("fr_render_deep_phoenix_async", c, p, ph, v, W, H, shard, out, hip_stream,
                                     [&] { return fr_deep_phoenix_validate(p, ph, v, W, H); });
}

extern "C" int fr_render_deep_phoenix(fr_ctx* c, const fr_params* p, const fr_phoenix_params* ph, const fr_deep_view* v, uint32_t W,
                                      uint32_t H, const fr_shard* shard, const fr_output* out)
{
    return deep_phoenix_entry<false>(nullptr, c, p, ph, v, W, H, shard, out, nullptr,
                                     [&] { return fr_deep_phoenix_validate(p, ph, v, W, H); });
}

extern "C" int fr_render_deepx_phoenix_async(fr_ctx* c, const fr_params* p, const fr_phoenix_params* ph, const fr_deepx_view* v,
                                             uint32_t W, uint32_t H, const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    return deep_phoenix_entry<true>("fr_render_deepx_phoenix_async", c, p, ph, v, W, H, shard, out, hip_stream,
                                    [&] { return fr_deepx_phoenix_validate(p, ph, v, W, H); });
}

extern "C" int fr_render_deepx_phoenix(fr_ctx* c, const fr_params* p, const fr_phoenix_params* ph, const fr_deepx_view* v, uint32_t W,
                                       uint32_t H, const fr_shard* shard, const fr_output* out)
{
    return deep_phoenix_entry<true>(nullptr, c, p, ph, v, W, H, shard, out, nullptr,
                                    [&] { return fr_deepx_phoenix_validate(p, ph, v, W, H); });
}

/* fr_render_deep_ship_de, fr_render_deepx_ship_de: fr_render_deep_de's five planes on the two ship paths, deriv four doubles per
 * pixel; the slots (orbit, table, step counts) are those of fr_render_deep_ship and fr_render_deepx_ship */
extern "C" int fr_render_deep_ship_de_async(fr_ctx* c, const fr_params* p, const fr_deep_view* v, const fr_deep_de* e, uint32_t W,
                                            uint32_t H, const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    return deep_entry<DeepShipDe<false>>("fr_render_deep_ship_de_async", c, p, v, e, W, H, shard, out, hip_stream,
                                         [&] { return fr_deep_ship_de_validate(p, v, e, W, H); });
}

extern "C" int fr_render_deep_ship_de(fr_ctx* c, const fr_params* p, const fr_deep_view* v, const fr_deep_de* e, uint32_t W,
                                      uint32_t H, const fr_shard* shard, const fr_output* out)
{
    return deep_entry<DeepShipDe<false>>(nullptr, c, p, v, e, W, H, shard, out, nullptr,
                                         [&] { return fr_deep_ship_de_validate(p, v, e, W, H); });
}

extern "C" int fr_render_deepx_ship_de_async(fr_ctx* c, const fr_params* p, const fr_deepx_view* v, const fr_deep_de* e,
                                             uint32_t W, uint32_t H, const fr_shard* shard, const fr_output* out,
                                             void* hip_stream)
{
    return deep_entry<DeepShipDe<true>>("fr_render_deepx_ship_de_async", c, p, v, e, W, H, shard, out, hip_stream,
                                        [&] { return fr_deepx_ship_de_validate(p, v, e, W, H); });
}

extern "C" int fr_render_deepx_ship_de(fr_ctx* c, const fr_params* p, const fr_deepx_view* v, const fr_deep_de* e, uint32_t W,
                                       uint32_t H, const fr_shard* shard, const fr_output* out)
{
    return deep_entry<DeepShipDe<true>>(nullptr, c, p, v, e, W, H, shard, out, nullptr,
                                        [&] { return fr_deepx_ship_de_validate(p, v, e, W, H); });
}

/* fr_render_deep_julia_de, fr_render_deepx_julia_de: fr_render_deep_de's five planes on the two Julia paths, whose slots (orbits,
 * tables, step counts) they share with the plain entry points */
extern "C" int fr_render_deep_julia_de_async(fr_ctx* c, const fr_params* p, const fr_deep_view* v, const fr_deep_de* e, uint32_t W,
                                             uint32_t H, const fr_shard* shard, const fr_output* out, void* hip_stream)
{
    return deep_entry<DeepJuliaDe>("fr_render_deep_julia_de_async", c, p, v, e, W, H, shard, out, hip_stream,
                                       [&] { return fr_deep_julia_de_validate(p, v, e, W, H); });
}

extern "C" int fr_render_deep_julia_de(fr_ctx* c, const fr_params* p, const fr_deep_view* v, const fr_deep_de* e, uint32_t W,
                                       uint32_t H, const fr_shard* shard, const fr_output* out)
{
    return deep_entry<DeepJuliaDe>(nullptr, c, p, v, e, W, H, shard, out, nullptr,
                                       [&] { return fr_deep_julia_de_validate(p, v, e, W, H); });
}

extern "C" int fr_render_deepx_julia_de_async(fr_ctx* c, const fr_params* p, const fr_deepx_view* v, const fr_deep_de* e,
                                              uint32_t W, uint32_t H, const fr_shard* shard, const fr_output* out,
                                              void* hip_stream)
{
    return deep_entry<DeepJuliaXDe>("fr_render_deepx_julia_de_async", c, p, v, e, W, H, shard, out, hip_stream,
                                        [&] { return fr_deepx_julia_de_validate(p, v, e, W, H); });
}

extern "C" int fr_render_deepx_julia_de(fr_ctx* c, const fr_params* p, const fr_deepx_view* v, const fr_deep_de* e, uint32_t W,
                                        uint32_t H, const fr_shard* shard, const fr_output* out)
{
    return deep_entry<DeepJuliaXDe>(nullptr, c, p, v, e, W, H, shard, out, nullptr,
                                        [&] { return fr_deepx_julia_de_validate(p, v, e, W, H); });
}

/* ---- 8-bit export ------------------------------------------------------------------------------ */
/* 1 when a frame's colour plane is a function of its smooth-count plane alone (fr_colorize_async) */
extern "C" int fr_colorize_supported(const fr_params* p)
{
    if (!p) return 0;
    if (p->fractal_type != FR_FRACTAL_MANDELBROT && p->fractal_type != FR_FRACTAL_JULIA &&
        p->fractal_type != FR_FRACTAL_BURNING_SHIP) return 0;
    if (needs_effects(p) || p->antialiasing_samples > 1) return 0;
    /* every escaped sample must have nu < max_iter, so that nu == max_iter identifies the interior:
     * Mandelbrot nu = i + 1 - log2(log2|z|) needs |z| > 2 with margin; the Julia form subtracts
     * log2(log|z|^2 / log B) > 1 for any B > 1 */
    if (p->fractal_type == FR_FRACTAL_MANDELBROT ? !(p->bailout >= 2.5f) : !(p->bailout >= 1.25f)) return 0;
    /* ... and must REPRESENT it: in fp32 a sample escaping at i = max_iter - 1 has nu = RN(max_iter - mu), mu > 0.3,
     * which rounds up to max_iter itself once the float spacing at max_iter reaches 0.5 (max_iter >= 2^23; mu can be
     * as small as ~0.3 at the smallest bailouts allowed above, so stop a binade earlier): it would be recoloured as
     * interior.  fp64 has no such limit at any max_iter the library accepts (<= 2^24). */
    if (p->precision == FR_PRECISION_F32 && p->max_iterations > (1 << 22)) return 0;
    return 1;
}

extern "C" int fr_colorize_async(fr_ctx* c, const fr_params* p, uint64_t n_pixels, const void* nu, float* rgba,
                                 void* hip_stream)
{
    if (!c || !p || !nu || !rgba) return fr_set_error(FR_ERR_INVALID_ARG, "fr_colorize_async: NULL argument");
    int st = fr_params_validate(p, 1, 1);
    if (st != FR_OK) return st;
    if (!fr_colorize_supported(p))
        return fr_set_error(FR_ERR_UNSUPPORTED, "colour is not a function of the smooth count for these parameters "
                                                "(effects, SSAA, Deep_Zoom or a small bailout)");
    if (n_pixels == 0) return FR_OK;
    FR_HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (!hip_stream) FR_HIP_TRY(order_after_last_render(c, stream));
    LaunchArgs a;
    fill_params(a, p);
    size_t blocks = ((size_t)n_pixels + kBlockThreads - 1) / kBlockThreads;
    const size_t cap = (size_t)c->compute_units * 8;
    if (blocks > cap) blocks = cap;
    const size_t n = (size_t)n_pixels;
    float4* out = reinterpret_cast<float4*>(rgba);
    hipError_t e = by_variant(p->fractal_type, p->precision == FR_PRECISION_F64, [&](auto t, auto f) {
        using T = decltype(t);
        hipLaunchKernelGGL((colorize_kernel<T, decltype(f)::value>), dim3((uint32_t)blocks), dim3(kBlockThreads), 0,
                           stream, a, reinterpret_cast<const T*>(nu), out, n);
        return hipGetLastError(); });
    if (e != hipSuccess) return fr_set_error(FR_ERR_HIP, "colorize launch failed: %s", hipGetErrorString(e));
    return FR_OK;
}

static size_t export_blocks(const fr_ctx* c, size_t npx)
{
    size_t blocks = ((npx + 3) / 4 + kBlockThreads - 1) / kBlockThreads;     /* four pixels per thread */
    const size_t cap = (size_t)c->compute_units * 8;
    return blocks > cap ? cap : (blocks < 1 ? 1 : blocks);
}

/* four pixels per thread (dword / dwordx2 stores) need a width that is a multiple of four AND an output pointer aligned
 * for those stores -- a caller may hand in a sub-buffer at any byte offset; otherwise one pixel per thread */
static hipError_t launch_export(const fr_ctx* c, const float4* in, uint8_t* out, uint32_t W, uint32_t H, int through_half,
                                hipStream_t s)
{
    const int quads_ok = (W & 3u) == 0u && ((uintptr_t)out & 3u) == 0u;
    const dim3 grid((uint32_t)export_blocks(c, (size_t)W * H));
    if (through_half)
        hipLaunchKernelGGL(export_rgb8_kernel<true>, grid, dim3(kBlockThreads), 0, s, in, out, (int)W, (int)H, quads_ok, (const float2*)c->export8_thr);
    else
        hipLaunchKernelGGL(export_rgb8_kernel<false>, grid, dim3(kBlockThreads), 0, s, in, out, (int)W, (int)H, quads_ok, (const float2*)c->export8_thr);
    return hipGetLastError();
}
static hipError_t launch_export(const fr_ctx* c, const float4* in, uint16_t* out, uint32_t W, uint32_t H, int through_half,
                                hipStream_t s)
{
    const int quads_ok = (W & 3u) == 0u && ((uintptr_t)out & 7u) == 0u;
    const dim3 grid((uint32_t)export_blocks(c, (size_t)W * H));
    if (through_half)
        hipLaunchKernelGGL(export_rgb16_kernel<true>, grid, dim3(kBlockThreads), 0, s, in, out, (int)W, (int)H, quads_ok);
    else
        hipLaunchKernelGGL(export_rgb16_kernel<false>, grid, dim3(kBlockThreads), 0, s, in, out, (int)W, (int)H, quads_ok);
    return hipGetLastError();
}

/* both export entry points: OUT = uint8_t (8-bit animation frames) or uint16_t (16-bit print export) */
template <typename OUT>
static int export_sync(fr_ctx* c, const float* rgba, uint32_t W, uint32_t H, OUT* out, int32_t memory, int32_t through_half,
                       const char* what)
{
    if (!c || !rgba || !out || W == 0 || H == 0 || (uint64_t)W * H >= (1ull << 31))
        return fr_set_error(FR_ERR_INVALID_ARG, "%s: bad argument (NULL pointer, empty frame or 2^31 pixels and more)", what);
    FR_HIP_TRY(hipSetDevice(c->device));
    const size_t npx = (size_t)W * H;
    const float4* d_in = reinterpret_cast<const float4*>(rgba);
    OUT* d_out = out;
    if (memory == FR_MEM_HOST) {
        const size_t need = npx * 16 + npx * 3 * sizeof(OUT);
        const int gs = grow_device(&c->scratch, &c->scratch_bytes, need);
        if (gs != FR_OK) return gs;
        FR_HIP_TRY(hipMemcpyAsync(c->scratch, rgba, npx * 16, hipMemcpyHostToDevice, c->stream));
        d_in = reinterpret_cast<const float4*>(c->scratch);
        d_out = reinterpret_cast<OUT*>((uint8_t*)c->scratch + npx * 16);
    } else if (memory == FR_MEM_DEVICE) {
        /* the plane may come from a render this context enqueued on a caller's stream */
        FR_HIP_TRY(order_after_last_render(c, c->stream));
    } else {
        return fr_set_error(FR_ERR_INVALID_ARG, "unknown memory kind %d", memory);
    }
    hipError_t e = launch_export(c, d_in, d_out, W, H, (int)through_half, c->stream);
    if (e != hipSuccess) return fr_set_error(FR_ERR_HIP, "export launch failed: %s", hipGetErrorString(e));
    if (memory == FR_MEM_HOST)
        FR_HIP_TRY(hipMemcpyAsync(out, d_out, npx * 3 * sizeof(OUT), hipMemcpyDeviceToHost, c->stream));
    FR_HIP_TRY(hipStreamSynchronize(c->stream));
    return check_overflow(c);
}

template <typename OUT>
static int export_async(fr_ctx* c, const float* rgba, uint32_t W, uint32_t H, OUT* out, int32_t through_half, void* hip_stream,
                        const char* what)
{
    if (!c || !rgba || !out || W == 0 || H == 0 || (uint64_t)W * H >= (1ull << 31))
        return fr_set_error(FR_ERR_INVALID_ARG, "%s: bad argument (NULL pointer, empty frame or 2^31 pixels and more)", what);
    FR_HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (!hip_stream) FR_HIP_TRY(order_after_last_render(c, s));
    hipError_t e = launch_export(c, reinterpret_cast<const float4*>(rgba), out, W, H, (int)through_half, s);
    if (e != hipSuccess) return fr_set_error(FR_ERR_HIP, "export launch failed: %s", hipGetErrorString(e));
    return FR_OK;
}

extern "C" int fr_export_rgb8(fr_ctx* c, const float* rgba, uint32_t W, uint32_t H,
                              uint8_t* rgb8, int32_t memory, int32_t through_half)
{
    return export_sync<uint8_t>(c, rgba, W, H, rgb8, memory, through_half, "fr_export_rgb8");
}

extern "C" int fr_export_rgb16(fr_ctx* c, const float* rgba, uint32_t W, uint32_t H,
                               uint16_t* rgb16, int32_t memory, int32_t through_half)
{
    return export_sync<uint16_t>(c, rgba, W, H, rgb16, memory, through_half, "fr_export_rgb16");
}

extern "C" int fr_export_rgb8_async(fr_ctx* c, const float* rgba, uint32_t W, uint32_t H, uint8_t* rgb8,
                                    int32_t through_half, void* hip_stream)
{
    return export_async<uint8_t>(c, rgba, W, H, rgb8, through_half, hip_stream, "fr_export_rgb8_async");
}

extern "C" int fr_export_rgb16_async(fr_ctx* c, const float* rgba, uint32_t W, uint32_t H, uint16_t* rgb16,
                                     int32_t through_half, void* hip_stream)
{
    return export_async<uint16_t>(c, rgba, W, H, rgb16, through_half, hip_stream, "fr_export_rgb16_async");
}

/* behind the render of a frame into frame_buf on the context's stream: fp16 round + 8-bit export + flip on the device, the
 * 3 B/pixel readback, PNG */
static int frame_png_tail(fr_ctx* c, uint32_t W, uint32_t H, const char* path)
{
    const size_t npx = (size_t)W * H;
    float* d_rgba = (float*)c->frame_buf;
    uint8_t* d_rgb8 = (uint8_t*)c->frame_buf + npx * 16;
    c->render_on_user_stream = false;
    hipError_t e = launch_export(c, reinterpret_cast<const float4*>(d_rgba), d_rgb8, W, H, 1, c->stream);
    if (e != hipSuccess) return fr_set_error(FR_ERR_HIP, "export launch failed: %s", hipGetErrorString(e));
    uint8_t* host = (uint8_t*)malloc(npx * 3);
    if (!host) return fr_set_error(FR_ERR_NOMEM, "out of host memory");
    hipError_t ce = hipMemcpyAsync(host, d_rgb8, npx * 3, hipMemcpyDeviceToHost, c->stream);
    if (ce == hipSuccess) ce = hipStreamSynchronize(c->stream);
    if (ce != hipSuccess) { free(host); return fr_set_error(FR_ERR_HIP, "readback failed: %s", hipGetErrorString(ce)); }
    int st = check_overflow(c);
    if (st == FR_OK) st = fr_write_png(path, W, H, 8, host, nullptr, 0, 0);
    free(host);
    return st;
}

/* RenderFrameCallback body: src/vk_engine.cpp:1181-1418 (render -> readback -> CPU tonemap/flip -> PNG),
 * with everything up to the 3 B/pixel readback on the GPU. */
extern "C" int fr_render_frame_png(fr_ctx* c, const fr_params* p, uint32_t W, uint32_t H, const char* path)
{
    if (!c || !p || !path) return fr_set_error(FR_ERR_INVALID_ARG, "fr_render_frame_png: NULL argument");
    int st = fr_params_validate(p, W, H);
    if (st != FR_OK) return st;
    FR_HIP_TRY(hipSetDevice(c->device));
    const size_t npx = (size_t)W * H;
    const size_t need = npx * 16 + npx * 3;
    const int gs = grow_device(&c->frame_buf, &c->frame_bytes, need);
    if (gs != FR_OK) return gs;
    fr_params q = *p;
    if (q.fractal_type != FR_FRACTAL_DEEP_ZOOM) q.flags |= FR_FLAG_POST_CHAIN;   /* the storage image holds the post-chained colour;
                                                                                     the deep-zoom shader has no post chain */
    float* d_rgba = (float*)c->frame_buf;
    st = enqueue_render(c, &q, W, H, nullptr, d_rgba, nullptr, nullptr, c->stream);
    if (st != FR_OK) return st;
    return frame_png_tail(c, W, H, path);
}

/* ---- deep zoom sequences: the entry points (the enqueue side is next to enqueue_deepx_at) --------------------------------- */
static int deep_sequence_create(const char* who, bool ship, fr_ctx* c, const fr_params* p, const fr_deep_sequence_desc* d,
                                uint32_t W, uint32_t H, fr_deep_sequence** out)
{
    if (!out) return fr_set_error(FR_ERR_INVALID_ARG, "%s: out is NULL", who);
    *out = nullptr;
    if (!c) return fr_set_error(FR_ERR_INVALID_ARG, "ctx is NULL");
    if (!p || !d) return fr_set_error(FR_ERR_INVALID_ARG, "params/deep sequence descriptor is NULL");
    fr_deepseq_walk w;
    const int st = fr_deepseq_resolve_formula(p, d, W, H, ship ? 1 : 0, &w);
    if (st != FR_OK) return st;
    if ((uint64_t)W * H >= (1ull << 31)) return fr_set_error(FR_ERR_INVALID_ARG, "a deep sequence frame has fewer than 2^31 pixels");
    fr_deep_sequence* q = (fr_deep_sequence*)calloc(1, sizeof(fr_deep_sequence));
    if (!q) return fr_set_error(FR_ERR_NOMEM, "out of host memory");
    q->c = c; q->p = *p; q->ship = ship; q->w = w; q->W = W; q->H = H;
    const char* src[3] = {d->center_x, d->center_y, d->zoom_first};
    for (int i = 0; i < 3; ++i)
        if (!(q->str[i] = strdup(src[i]))) { fr_deep_sequence_destroy(q); return fr_set_error(FR_ERR_NOMEM, "out of host memory"); }
    q->view.center_x = q->str[0]; q->view.center_y = q->str[1]; q->view.zoom = q->str[2];
    q->view.frac_bits = w.frac_bits; q->view.reserved = 0;
    if (w.mode == 1) {
        hipError_t e = hipSetDevice(c->device);
        for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipMalloc((void**)&q->key[i], (size_t)W * H * 16);
        if (e != hipSuccess) {
            fr_deep_sequence_destroy(q);
            return fr_set_error(FR_ERR_HIP, "deep sequence keyframe planes: %s", hipGetErrorString(e));
        }
    }
    *out = q;
    return FR_OK;
}

extern "C" int fr_deep_sequence_create(fr_ctx* c, const fr_params* p, const fr_deep_sequence_desc* d, uint32_t W, uint32_t H,
                                       fr_deep_sequence** out)
{
    return deep_sequence_create("fr_deep_sequence_create", false, c, p, d, W, H, out);
}

extern "C" int fr_deep_ship_sequence_create(fr_ctx* c, const fr_params* p, const fr_deep_sequence_desc* d, uint32_t W, uint32_t H,
                                            fr_deep_sequence** out)
{
    return deep_sequence_create("fr_deep_ship_sequence_create", true, c, p, d, W, H, out);
}

extern "C" void fr_deep_sequence_destroy(fr_deep_sequence* q)
{
    if (!q) return;
    if (q->key[0] || q->key[1]) {
        (void)hipSetDevice(q->c->device);
        (void)hipStreamSynchronize(q->c->stream);
        for (int i = 0; i < 2; ++i)
            if (q->key[i]) (void)hipFree(q->key[i]);
    }
    for (int i = 0; i < 3; ++i) free(q->str[i]);
    free(q);
}

extern "C" int fr_deep_sequence_render(fr_deep_sequence* q, int32_t frame, const fr_output* out)
{
    if (!q || !out) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_sequence_render: sequence/out is NULL");
    if (frame < 0 || frame >= q->w.frames) return fr_set_error(FR_ERR_INVALID_ARG, "frame %d outside [0, %d)", frame, q->w.frames);
    if (out->layout != FR_LAYOUT_PACKED) return fr_set_error(FR_ERR_INVALID_ARG, "a deep sequence writes FR_LAYOUT_PACKED whole frames");
    fr_deep_sequence_frame f;
    fr_deepseq_frame(&q->w, frame, &f);
    if (f.resampled && (out->nu || out->iter))
        return fr_set_error(FR_ERR_UNSUPPORTED, "frame %d is resampled from keyframes %d and %d: it has an rgba plane only", frame,
                            f.keyframe, f.keyframe + 1);
    return render_sync(q->c, &q->p, q->W, q->H, nullptr, out, {}, [&](auto, auto rgba, auto nu, auto iter, auto, auto s, bool) {
        return seq_enqueue(q, &q->p, f, rgba, nu, iter, s); });
}

extern "C" int fr_deep_sequence_render_png(fr_deep_sequence* q, int32_t frame, const char* path)
{
    if (!q || !path) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_sequence_render_png: NULL argument");
    if (frame < 0 || frame >= q->w.frames) return fr_set_error(FR_ERR_INVALID_ARG, "frame %d outside [0, %d)", frame, q->w.frames);
    fr_ctx* c = q->c;
    FR_HIP_TRY(hipSetDevice(c->device));
    const size_t npx = (size_t)q->W * q->H;
    const int gs = grow_device(&c->frame_buf, &c->frame_bytes, npx * 16 + npx * 3);
    if (gs != FR_OK) return gs;
    fr_params p = q->p;
    p.flags |= FR_FLAG_POST_CHAIN;
    fr_deep_sequence_frame f;
    fr_deepseq_frame(&q->w, frame, &f);
    const int st = seq_enqueue(q, &p, f, (float*)c->frame_buf, nullptr, nullptr, c->stream);
    if (st != FR_OK) return st;
    return frame_png_tail(c, q->W, q->H, path);
}

extern "C" int fr_deep_sequence_stats(const fr_deep_sequence* q, uint64_t out[3])
{
    if (!q || !out) return fr_set_error(FR_ERR_INVALID_ARG, "fr_deep_sequence_stats: sequence/out is NULL");
    out[0] = q->n_exact; out[1] = q->n_resampled; out[2] = q->n_orbits;
    return FR_OK;
}
