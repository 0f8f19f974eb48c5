/*
 * fractalrenderer_amd.h -- C ABI of the MI355X-native escape-time renderer.
 *
 * This is the drop-in boundary for the ONE hot path of franklynch/FractalRenderer:
 * the per-pixel z <- z^2 + c iteration with smooth colouring (Mandelbrot/Julia).
 * Every entry point below replaces the reference interface cited next to it.
 * Path shorthand: src/ = FractalRenderer/src/, shaders/ = FractalRenderer/shaders/.
 *
 * Conventions
 *   - plain C11, no C++ or torch types; all pointers + sizes.
 *   - every function returns an fr_status (0 = FR_OK, < 0 = error) unless noted;
 *     nothing aborts (the reference's VK_CHECK aborts, src/vk/vk_types.h:143-150).
 *     fr_last_error() returns a thread-local message for the last failure.
 *   - there is NO CPU fallback: a render call without a usable HIP device fails
 *     with FR_ERR_NO_DEVICE.
 *   - image layout: row-major, row 0 = smallest pixel y (as gl_GlobalInvocationID.y,
 *     shaders/mandelbrot.comp:215; no vertical flip), RGBA f32, alpha = 1.
 */
#ifndef FRACTALRENDERER_AMD_H
#define FRACTALRENDERER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_VERSION_MAJOR 1
#define FR_VERSION_MINOR 1   /* 1.1: frames in flight on a node (fr_node_submit, fr_node_wait_frame, "slots", "lanes") */

typedef enum fr_status {
    FR_OK               =  0,
    FR_ERR_INVALID_ARG  = -1,   /* NULL pointer, w/h == 0, max_iter outside [1, 2^24], zoom 0/non-finite ... */
    FR_ERR_NO_DEVICE    = -2,   /* no HIP device / device ordinal out of range */
    FR_ERR_HIP          = -3,   /* a HIP runtime call failed (message has the hipError string) */
    FR_ERR_UNSUPPORTED  = -4,   /* fractal type outside the hot path (Mandelbrot, JuliaSet, Deep_Zoom are in) */
    FR_ERR_IO           = -5,   /* .franim file could not be read / written */
    FR_ERR_PARSE        = -6,   /* .franim JSON malformed or a required key is missing */
    FR_ERR_NOMEM        = -7,
    FR_ERR_INTERNAL     = -8    /* the library caught itself out (a survivor stream overflowed): the frame is incomplete */
} fr_status;

/* FractalType, src/fractal_state.h:6-14 (same numeric values).  Mandelbrot and JuliaSet are the
 * hot path; BurningShip (shaders/burning_ship.comp) is the same loop with z = abs(z) before the
 * square; Deep_Zoom is the reference's perturbation shader (shaders/test_deep_zoom.comp), restated
 * with its fp32 float-float arithmetic.  Phoenix (shaders/phoenix.comp) needs three fields fr_params
 * has no room for: fr_render and the other fr_params entry points return FR_ERR_UNSUPPORTED for it, and
 * fr_render_phoenix (below) renders it.  Mandelbulb (shaders/mandelbulb.comp, a 3-D ray marcher) likewise returns
 * FR_ERR_UNSUPPORTED there and renders through fr_render_mandelbulb (below). */
typedef enum fr_fractal_type {
    FR_FRACTAL_MANDELBROT   = 0,
    FR_FRACTAL_JULIA        = 1,
    FR_FRACTAL_BURNING_SHIP = 2,
    FR_FRACTAL_MANDELBULB   = 3,
    FR_FRACTAL_PHOENIX      = 4,
    FR_FRACTAL_DEEP_ZOOM    = 5
} fr_fractal_type;

/* Arithmetic type of the iteration.  The reference computes in fp32 only
 * (shaders/mandelbrot.comp:147-170) after narrowing its double viewport
 * (src/compute_effect_manager.h:85-90); FR_PRECISION_F64 keeps the doubles. */
typedef enum fr_precision {
    FR_PRECISION_F32 = 0,
    FR_PRECISION_F64 = 1
} fr_precision;

/* fr_params.flags */
#define FR_FLAG_POST_CHAIN   0x1u  /* apply enhance_color -> aces_tonemap -> pow(1/2.2)
                                      (shaders/mandelbrot.comp:233-235, shaders/julia.comp:330-337);
                                      default is the LINEAR colour, before that chain */
#define FR_FLAG_DEEP_BLA     0x2u  /* fr_render_deep(_async) only: skip iterations by bilinear approximation (see there);
                                      every other entry point ignores it */
#define FR_FLAG_DEEPX_BLA    0x4u  /* fr_render_deepx(_async) only: the same for extended views (see there); every other
                                      entry point ignores it, fr_render_deep included */
#define FR_FLAG_DEEP_SHIP_BLA 0x8u /* fr_render_deep_ship and its _async form only: the same for deep Burning Ship views
                                      (see there); every other entry point ignores it */
#define FR_FLAG_DEEPX_SHIP_BLA 0x10u /* fr_render_deepx_ship, its _async form and fr_deep_ship_sequence_create only: the same
                                      for extended Burning Ship views (see there); every other entry point ignores it */
#define FR_FLAG_DEEP_JULIA_BLA 0x20u /* fr_render_deep_julia and its _async form only: the same for deep Julia views (see
                                      there); the other deep entry points answer FR_ERR_UNSUPPORTED */
#define FR_FLAG_DEEPX_JULIA_BLA 0x40u /* fr_render_deepx_julia and its _async form only: the same for extended Julia views (see
                                      there); the other deep entry points answer FR_ERR_UNSUPPORTED */
#define FR_FLAG_DEEP_PHOENIX_BLA 0x80u /* fr_render_deep_phoenix and its _async form only: the same for deep Phoenix views (see
                                      there); fr_deepx_phoenix_validate answers FR_ERR_UNSUPPORTED, nobody else reads it */
#define FR_FLAG_DEEPX_PHOENIX_BLA 0x100u /* fr_render_deepx_phoenix and its _async form only: the same for Phoenix views below
                                      1e-290 (see there); every other deep validator answers FR_ERR_UNSUPPORTED */

/*
 * fr_params -- the hot-path fields of FractalState (src/fractal_state.h:16-91),
 * i.e. the union of what ComputeEffect::update_from_state packs for Mandelbrot
 * (src/compute_effect_manager.h:84-113) and Julia (:115-140).  centre/zoom stay
 * double: the fp64 kernels need what the reference throws away at :86-88.
 * fr_params_default() fills the FractalState member initialisers.
 */
typedef struct fr_params {
    int32_t fractal_type;          /* fr_fractal_type                                   */
    int32_t precision;             /* fr_precision                                      */
    double  center_x;              /* src/fractal_state.h:18   default -0.5             */
    double  center_y;              /*                   :19    default  0.0             */
    double  zoom;                  /*                   :20    default  3.0  (view height in c-plane units) */
    int32_t max_iterations;        /*                   :21    default  256             */
    float   bailout;               /*                   :36    default  4.0; test is |z|^2 > bailout^2 */
    double  julia_c_real;          /*                   :29    default -0.7f  (float in the reference)  */
    double  julia_c_imag;          /*                   :30    default  0.27015f        */
    int32_t antialiasing_samples;  /*                   :37    default  1  (n -> n x n samples)         */
    int32_t palette_mode;          /*                   :40    default  0               */
    float   color_offset;          /*                   :41    default  0               */
    float   color_scale;           /*                   :42    default  1               */
    int32_t interior_style;        /*                   :47    default  0               */
    int32_t orbit_trap_enabled;    /*                   :48    default  0 (bool)        */
    float   orbit_trap_radius;     /*                   :49    default  0.5             */
    int32_t stripe_enabled;        /*                   :50    default  0 (bool)        */
    float   stripe_density;        /*                   :51    default  10              */
    float   color_brightness;      /*                   :77    default  1               */
    float   color_saturation;      /*                   :78    default  1               */
    float   color_contrast;        /*                   :79    default  1               */
    uint32_t flags;                /* FR_FLAG_*                                         */
    int32_t use_perturbation;      /*                   :86    default  0 (bool).  Deep_Zoom only: 1 = the fp64
                                      reference orbit at the centre is computed (as prepare_deep_zoom_rendering
                                      does every frame, src/vk_engine.cpp:215-251) and the shader perturbs
                                      around it; 0 = empty orbit, plain fp32 iteration                  */
} fr_params;

/* ---- parameters ------------------------------------------------------------------ */

/* FractalState{} member initialisers, src/fractal_state.h:18-51,77-79;
 * fractal_type = Mandelbrot, precision = FR_PRECISION_F64, flags = 0. */
int fr_params_default(fr_params* p);

/* FractalState::reset(), src/fractal_state.h:135-153: centre (-0.5,0), zoom 1.5 (NOT 3.0),
 * max_iterations 256, brightness/saturation/contrast 1; other fields untouched. */
int fr_params_reset(fr_params* p);

/* Validation the reference does not do (it patches or aborts, src/compute_effect_manager.h:335-345).
 * width,height > 0; width*height < 2^31; max_iterations in [1, 2^24] (ints travel as floats
 * through the push constants, exact to 2^24, shaders/mandelbrot.comp:18); zoom finite and != 0;
 * centre finite; bailout finite > 0; antialiasing_samples in [0, 16]; fractal/precision known. */
int fr_params_validate(const fr_params* p, uint32_t width, uint32_t height);

/* ComputeEffect::update_from_state, src/compute_effect_manager.h:84-113 (Mandelbrot) and
 * :115-140 (Julia): the 80-byte ComputePushConstants block (:11-17) as 20 floats,
 * bit-for-bit (every field static_cast<float>). */
int fr_pack_push_constants(const fr_params* p, float out[20]);

/* ---- context ---------------------------------------------------------------------- */

typedef struct fr_ctx fr_ctx;   /* owns the device ordinal, a stream, timing events and the
                                   tile-queue words; not re-entrant, distinct contexts may
                                   run concurrently (reference: single thread, src/vk_engine.cpp) */

/* Replaces ComputeEffectManager's constructor + init_pipelines
 * (src/compute_effect_manager.cpp:19-60,120-140): binds a HIP device; kernels are
 * precompiled for gfx950 in this library, there is nothing to load at run time. */
int  fr_ctx_create(int device_ordinal, fr_ctx** out);
void fr_ctx_destroy(fr_ctx* ctx);

/* ---- render ----------------------------------------------------------------------- */

typedef enum fr_memory {
    FR_MEM_DEVICE = 0,    /* pointers are HIP device pointers on ctx's device (no copies)   */
    FR_MEM_HOST   = 1     /* pointers are host memory; the library stages through device
                             scratch it owns and copies back (PCIe-inclusive path)          */
} fr_memory;

/* Where a part of a row-strip sharding (fr_shard) stores its rows. */
typedef enum fr_layout {
    FR_LAYOUT_PACKED = 0, /* the planes hold only this part's rows, packed densely in strip order (fr_shard_rows() rows) */
    FR_LAYOUT_FRAME  = 1  /* the planes are WHOLE-FRAME planes (height rows) and the part stores its rows in place: the parts
                             of a frame may then share one set of planes -- on one device, or on a peer device whose memory
                             is mapped (hipDeviceEnablePeerAccess): the gather of a multi-GPU frame fused into the kernels'
                             stores (fr_node_render).  FR_MEM_DEVICE only. */
} fr_layout;

/* Output planes of one render.  rgba is required unless nu or iter is given. */
typedef struct fr_output {
    float*   rgba;     /* rows*W*4 f32, linear colour (or post-chained with FR_FLAG_POST_CHAIN) */
    void*    nu;       /* rows*W smooth iteration count of sample (0,0): double for
                          FR_PRECISION_F64, float for FR_PRECISION_F32; max_iterations
                          for interior pixels.  NULL to skip                                */
    int32_t* iter;     /* rows*W index i of the escaping update (shaders/mandelbrot.comp:157-170),
                          max_iterations for interior.  NULL to skip                        */
    int32_t  memory;   /* fr_memory                                                         */
    int32_t  layout;   /* fr_layout (0 = packed part rows; occupies what was padding before 1.0) */
} fr_output;

/* Row-strip sharding of one frame over the GPUs of a node: the frame's rows are cut
 * into strips of rows_per_strip rows, dealt round-robin: strip s belongs to part
 * (s % nparts).  Part `part` renders only its strips, packed densely in strip order,
 * into its fr_output (fr_shard_rows() rows).  {0,1,0} = the whole frame. */
typedef struct fr_shard {
    uint32_t part;
    uint32_t nparts;
    uint32_t rows_per_strip;   /* 0 with nparts == 1 means "whole frame" */
} fr_shard;

/* number of rows part `part` owns / first-row table helpers (host-side arithmetic only) */
uint32_t fr_shard_rows(const fr_shard* s, uint32_t height);
/* global row index of local row `local_row` of this part; UINT32_MAX if out of range */
uint32_t fr_shard_global_row(const fr_shard* s, uint32_t height, uint32_t local_row);

/*
 * fr_render -- the reference's render(viewport, max_iter, out_buffer) surface:
 *   AnimationRenderer::RenderFrameCallback  bool(const FractalState&, uint32_t width,
 *   uint32_t height, const std::string& path)  src/animation_renderer.h:41-48, whose body
 *   VulkanEngine::render_animation_frame (src/vk_engine.cpp:1181-1418) reaches
 *   ComputeEffectManager::dispatch (src/compute_effect_manager.h:435-468) ->
 *   vkCmdDispatch(ceil(W/16), ceil(H/16), 1) of shaders/mandelbrot.comp / julia.comp.
 * Synchronous: returns after the planes are complete (reference: immediate_submit waits
 * on its fence, src/vk_engine.cpp:2319-2321).
 */
int fr_render(fr_ctx* ctx, const fr_params* p, uint32_t width, uint32_t height,
              const fr_output* out);

/* Same, restricted to one part of a row-strip sharding (multi-GPU row bands). */
int fr_render_shard(fr_ctx* ctx, const fr_params* p, uint32_t width, uint32_t height,
                    const fr_shard* shard, const fr_output* out);

/* Asynchronous form for frame pipelining: enqueues on `hip_stream` (a hipStream_t passed
 * as void*; NULL = the context's own stream) and returns without waiting.  Device memory only.
 * STEADY STATE it is launch-only (kernel launches -- a small one that clears the control block and writes the frame's
 * coordinate tables, then the render's -- + two event records: no allocation, no host synchronisation, capturable
 * into a hipGraph).  What is not steady state:
 *   - the first render of a geometry LARGER than any before it on this context grows the context's
 *     survivor-stream scratch and coordinate tables (hipFree + hipMalloc), and the first render of a new (W, H, fractal,
 *     precision) checks on the host that the divide-free viewport map is exact for every column and row
 *     (a loop over W + H numerators, cached for 8 geometries).  fr_ctx_reserve() does both ahead of time;
 *   - Deep_Zoom with use_perturbation recomputes the fp64 reference orbit on the host for every frame, as
 *     the reference does (src/vk_engine.cpp:215-251), and waits for `hip_stream` before reusing its pinned
 *     upload buffer: never launch-only.
 * A failure the device reports later (FR_ERR_INTERNAL) surfaces at the next call on the context or
 * through fr_ctx_check(). */
int fr_render_shard_async(fr_ctx* ctx, const fr_params* p, uint32_t width, uint32_t height,
                          const fr_shard* shard, const fr_output* out, void* hip_stream);

/* Pre-sizes everything a render of (params, width, height, shard) allocates or caches on first use, so
 * that later fr_render_shard_async calls of this or any smaller geometry are launch-only (see there).
 * Synchronises the context's own stream.  New design: the reference allocates its image and staging
 * buffer per call (src/vk_engine.cpp:1197-1221,1268-1272). */
int fr_ctx_reserve(fr_ctx* ctx, const fr_params* p, uint32_t width, uint32_t height, const fr_shard* shard);

/* FR_OK, or FR_ERR_INTERNAL if a render that has completed on this context since the last call lost
 * pixels (cleared by the call).  The synchronous entry points check by themselves; a caller of the
 * _async forms calls this after it has synchronised its stream. */
int fr_ctx_check(fr_ctx* ctx);

/* Device time of the most recent render's kernels on this context, from a HIP event pair recorded around its launches on
 * the launch stream (blocks until they are done).  Needs the option "timing" = 1, set BEFORE that render: the pair is not
 * recorded by default since 1.1 (two timed event records cost a frame ~4.7 us -- 0.6 % of a 4096^2 / 1024 frame, 10 % of a
 * 1080p / 256 one).  < 0 if nothing was rendered with it yet. */
float fr_ctx_last_kernel_ms(fr_ctx* ctx);

/* Options by name; value 0 restores the automatic choice (made per launch from the frame geometry).  None of them can
 * change a pixel (tests/test_gpu_parity.py::test_tuning_variants_are_bit_identical).
 * Phoenix frames (fr_render_phoenix) accept every option; "periodicity" and "staging" have no effect on them (one pass, no
 * lane pool, no cycle closing), "shards" and "timing" apply as for the other frames.
 *   "periodicity"   -1 = off, 0 = automatic (ON), 1 = on, N > 1 = on with a first snapshot window of N iterations.
 *                   Cycle closing: the kernels keep, per lane, the orbit state at the wave's last snapshot; a lane whose
 *                   state returns to it is on a cycle, can never escape, and is retired as interior at once instead of
 *                   being iterated to max_iter.  Exact, not a heuristic: the update is a deterministic function of (z, c),
 *                   so every plane stays byte-identical (tests/test_gpu_parity.py::test_periodicity_never_changes_a_pixel);
 *                   what changes is the number of iterations executed -- the reference's shaders iterate every interior
 *                   sample to max_iter (C2: 1.4x fewer, a filled Julia set 2.8x).  Automatic (0): a context whose lane pools
 *                   retired less than an eighth of their records by closed cycles -- a Julia dust -- renders its next 14
 *                   frames of the same kind without looking, then looks once more (no synchronisation: the verdict of a
 *                   frame travels with the next frame's first launch); 1 / N: always look.
 *                   Not where a sample's final z is read (stripe shading), in the Burning Ship's effects variants or Deep_Zoom.  bench.py's headline switches it OFF so that its roofline
 *                   is quoted on the reference's iteration count.
 *   "staging"       0 = automatic, 1 = single pass (every sample runs to max_iter in the tile kernel), 3 = tile pass for
 *                   the first b0 iterations + ONE lane-pool pass over the compacted survivors, whatever max_iter is.
 *                   Automatic: 3 where it applies (not with the Burning Ship's trap / stripe effects; a supersampled frame's
 *                   sample grid is rendered as a frame of its own and takes the same choice) and pays off -- a Julia set from
 *                   max_iterations 256, fp64 from 512 (384 on frames above 2^23 pixels), fp32 from 768 (512); frames of up
 *                   to 2^19 pixels: fp64 from 1024 (1536 up to 2^18 pixels), fp32 from 1536, a Julia set of up to 2^20 pixels
 *                   from 512 -- the second launch and the
 *                   pool's ramp cost a small frame more than they save (profiles/r04_staging_crossover.txt,
 *                   r04_small_frame_staging.txt).
 *   "shards"        8 or 64: shards of the work queue (each has ONE head word that its waves update with returning
 *                   atomics, ~15 ns apart).  Automatic: 64 (8 per XCD) for launches whose waves stop at their home shards
 *                   on grids of >= 256 workgroups over frames of >= 4096 sub-tiles, else 8.
 *   "tile_kernel"   1 = the general tile kernel; 0 = automatic: the LEAN tile kernel (coordinate tables written by its own
 *                   first workgroups -- by a small launch in front of it on capturing streams --, two 8x8 sub-tiles per wave
 *                   and trip) for every one-sample render (the Burning Ship's trap / stripe effects excepted) whose row
 *                   strips, if sharded, are whole sub-tile rows.
 *   "fold"          a Mandelbrot frame with center_y == 0 is symmetric about the real axis bit for bit: 0 = automatic (such a
 *                   frame of at least 2^20 pixels renders its upper floor(H / 2) + 1 rows, rounded up to 8, and stores every
 *                   finished pixel of row r at row H - r as well), 1 = off, 2 = on wherever the frame qualifies (one sample per
 *                   pixel, no stripes / orbit trap / interior style 2, a whole frame by the lean tile kernel).
 *   "timing"        1 = record a HIP event pair around every render (fr_ctx_last_kernel_ms, fr_node_last_kernel_ms); 0 = off, the
 *                   default since 1.1.
 *   "diag_buffer"   device pointer to 4 x uint64 per wave (t_start, t_end in 100 MHz ticks, items processed, dequeues);
 *                   0 disables.  "diag_stride" = uint64 words between the tile pass's and the lane pool's regions.
 * Changed in 1.0 (INTEGRATION.md lists the breaks): "periodicity" 0 means automatic = ON since 0.2 (it meant off in
 * 0.1; -1 is off); "staging" 2 / 4 and the options "pool", "stage_ratio" are accepted and ignored (the schedules they
 * selected are gone); the queue / stream tuning names moved to the internal fr_ctx_set_tuning
 * (fractalrenderer_amd/csrc/fr_tuning.h). */
int fr_ctx_set_option(fr_ctx* ctx, const char* name, int64_t value);

/* Workgroups per launch of the most recent render on this context (bits 0-15) and its number of
 * stages (bits 16-..: 1 = single pass). */
int fr_ctx_last_grid(fr_ctx* ctx);

/* Number of compute units of the context's device (hipDeviceProp_t.multiProcessorCount). */
int fr_ctx_compute_units(fr_ctx* ctx);

/* Waits for everything this context has enqueued on its OWN stream (fr_render_shard_async with a NULL stream, the
 * exports, fr_colorize_async with a NULL stream) and returns fr_ctx_check()'s verdict. */
int fr_ctx_synchronize(fr_ctx* ctx);

/* ---- Phoenix (shaders/phoenix.comp) ----------------------------------------------------------------------------------
 * z' = z^2 + C + r * z_prev + p * z from z = z_prev = 0, update then test |z|^2 > 4 (a fixed bailout), smooth count
 * i + 1 - log2(log2|z|), colour pow(smooth / max_iter, 0.8) through the ultra_fire palette (always: the shader's
 * get_palette_color ignores palette_mode, :34-43) with the flow stripes of stripe_density (on when density > 0.01,
 * whatever stripe_enabled says), in-shader aa x aa supersampling.  The viewport map is Julia's (:106-110).  C is the
 * pixel's c, or julia_c in Julia mode -- which still starts from z = 0, so EVERY pixel of a Julia-mode frame has the
 * same colour (as in the reference).  fr_params cannot express a Phoenix frame (FractalState's phoenix_p, phoenix_r and
 * use_julia_set, src/fractal_state.h:82-84, have no field there): these entry points take them in fr_phoenix_params
 * and p->fractal_type must be FR_FRACTAL_PHOENIX.  fr_render, fr_params_validate, fr_pack_push_constants keep
 * answering FR_ERR_UNSUPPORTED for Phoenix. */
#define FR_HAS_PHOENIX 1

typedef struct fr_phoenix_params {
    float   phoenix_p;             /* src/fractal_state.h:82  default  0.0   (damping)         */
    float   phoenix_r;             /*                   :83   default -0.5   (feedback/memory) */
    int32_t use_julia_set;         /*                   :84   default  0 (bool)               */
    int32_t reserved;              /* must be 0 */
} fr_phoenix_params;               /* 16 bytes */

/* FractalState's initialisers for the three fields: (0, -0.5, 0), reserved 0. */
int fr_phoenix_params_default(fr_phoenix_params* ph);

/* ComputeEffect::update_from_state's Phoenix case, src/compute_effect_manager.h:201-224, as 20 floats bit for bit:
 * data1 (cx, cy, zoom, max_iter), data2 (julia_c, p, r), data3 (aa, color_scale, brightness, saturation),
 * data4 (contrast, palette, stripe_density, use_julia ? 1 : 0), data5 = 0.  stripe_density is packed whatever
 * stripe_enabled says.  Validates as fr_render_phoenix does (no frame size). */
int fr_pack_push_constants_phoenix(const fr_params* p, const fr_phoenix_params* ph, float out[20]);

/* A Phoenix frame (or one part of a row-strip sharding of it: shard NULL = the whole frame) into `out`, synchronously.
 * Validation: fr_params_validate's rules for the fields Phoenix reads, fractal_type == FR_FRACTAL_PHOENIX, p and r
 * finite, use_julia_set 0 or 1, reserved 0; otherwise FR_ERR_INVALID_ARG.  What Phoenix does not read (bailout,
 * color_offset, interior_style, the orbit trap, stripe_enabled, use_perturbation) is ignored.
 * Planes as for fr_render (precision, FR_MEM_HOST / FR_MEM_DEVICE, FR_LAYOUT_FRAME, FR_FLAG_POST_CHAIN -- the post chain
 * with Phoenix's floors: brightness, contrast >= 0.1, saturation >= 0, :160-162): nu = smooth_iter of sample (0,0)
 * (max_iterations for interior samples), iter = the loop index i of that sample (max_iterations for interior), rgba = the
 * linear colour before enhance_color.  A sample whose smooth count is negative (a first-step escape far outside the set)
 * makes the shader's pow() NaN; every palette comparison then fails and it takes the last knot, as in the shader.
 * FR_PRECISION_F64: map, orbit and smooth count in double; t = smooth / max_iter divided in double, narrowed, and the
 * colour stage after it in float, as the shader. */
int fr_render_phoenix(fr_ctx* ctx, const fr_params* p, const fr_phoenix_params* ph, uint32_t width, uint32_t height,
                      const fr_shard* shard, const fr_output* out);

/* Asynchronous form, the fr_render_shard_async contract: device planes only, enqueued on hip_stream (NULL = the
 * context's stream), launch-only in steady state (no allocation, no host synchronisation); errors the device reports
 * later surface through fr_ctx_check.  "timing", fr_ctx_last_kernel_ms and fr_ctx_last_grid cover it. */
int fr_render_phoenix_async(fr_ctx* ctx, const fr_params* p, const fr_phoenix_params* ph, uint32_t width, uint32_t height,
                            const fr_shard* shard, const fr_output* out, void* hip_stream);

/* ---- Mandelbulb (shaders/mandelbulb.comp) ---------------------------------------------------------------------------
 * A ray marcher, one ray per sample, all in fp32 as the shader: the camera orbits the origin at camera_distance (times
 * 1 + 0.3 sin(0.5 time)), turned by rotation_y + rotation_speed * time about the y axis (rotation_speed 0 means 0.3, :188);
 * the power is mandelbulb_power + 0.5 sin(0.7 time).  Up to 200 steps of t += max(0.5 d, 0.0005) on the distance
 * estimator of the power-n bulb (escape radius 2, max_iterations clamped to [1, 1024]); a hit (d < max(1e-4, 1e-3 t))
 * is shaded with a 4-call normal, diffuse / specular / rim / glow, this shader's six palettes, 8 ambient-occlusion
 * samples and distance fog; a miss takes the sky gradient.  aa x aa samples per pixel, averaged.
 * fr_params cannot express a Mandelbulb frame (camera_distance, rotation_y, fov, mandelbulb_power, rotation_speed and
 * the frame time have no field there): these entry points take them in fr_mandelbulb_params and p->fractal_type must
 * be FR_FRACTAL_MANDELBULB.  fr_render, fr_params_validate and fr_pack_push_constants keep answering
 * FR_ERR_UNSUPPORTED for Mandelbulb.
 *
 * NaN policy.  The shader colours a hit with log(log(length(pos))), which is NaN wherever the hit point lies inside the
 * unit sphere (much of the power-8 surface).  The linear plane (rgba without FR_FLAG_POST_CHAIN) carries that NaN as
 * the shader computes it; one NaN sample makes its pixel's average NaN.  The post-chained plane follows the IEEE
 * maxNum / minNum semantics of GPU clamp(): enhance_color's clamp maps NaN to 0, so the pixel is black, finite, which
 * is what the reference shows on a GPU. */
#define FR_HAS_MANDELBULB 1

typedef struct fr_mandelbulb_params {
    float   camera_distance;       /* src/fractal_state.h:24  default 3.0                          */
    float   rotation_y;            /*                   :25   default 0.0 (radians)                */
    float   fov;                   /*                   :26   default 1.0                          */
    float   mandelbulb_power;      /*                   :33   default 8.0                          */
    float   rotation_speed;        /*                   :68   default 0.5                          */
    float   time;                  /* the frame time in seconds (ImGui::GetTime(), src/vk_engine.cpp:336); default 0 */
    int32_t reserved[2];           /* must be 0 */
} fr_mandelbulb_params;            /* 32 bytes */

/* FractalState's initialisers for the five 3-D fields, time 0, reserved 0. */
int fr_mandelbulb_params_default(fr_mandelbulb_params* mb);

/* ComputeEffect::update_from_state's Mandelbulb case, src/compute_effect_manager.h:173-199, as 20 floats bit for bit:
 * data1 (camera_distance, rotation_y, power, max_iter), data2 (color_offset, color_scale, 0, palette_mode),
 * data3 (time, fov, aa, brightness), data4 (rotation_speed, saturation, contrast, 0), data5 = 0.  Validates as
 * fr_render_mandelbulb does (no frame size). */
int fr_pack_push_constants_mandelbulb(const fr_params* p, const fr_mandelbulb_params* mb, float out[20]);

/* A Mandelbulb frame (or one part of a row-strip sharding of it: shard NULL = the whole frame) into `out`, synchronously.
 * Validation: fr_params_validate's rules for the fields Mandelbulb reads (max_iterations in [1, 2^24], clamped to 1024
 * as the shader does; antialiasing_samples in [0, 16]), fractal_type == FR_FRACTAL_MANDELBULB, every float of `mb`
 * finite, reserved 0; otherwise FR_ERR_INVALID_ARG.  FR_PRECISION_F64 answers FR_ERR_UNSUPPORTED (the shader is fp32).
 * What Mandelbulb does not read (centre, zoom, bailout, julia_c, interior style, the orbit trap, stripes,
 * use_perturbation) is ignored.
 * Planes (FR_MEM_HOST / FR_MEM_DEVICE, FR_LAYOUT_FRAME): rgba = the averaged linear colour (FR_FLAG_POST_CHAIN: the
 * shader's enhance_color -> aces_tonemap -> pow(1/2.2) with its floors: brightness, contrast >= 0.1, saturation >= 0);
 * iter = the ray-march step index of sample (0,0)'s hit, -1 for a ray that hits nothing; nu (float) = sample (0,0)'s
 * ray parameter t where its march stopped (a depth plane).  See the NaN policy above. */
int fr_render_mandelbulb(fr_ctx* ctx, const fr_params* p, const fr_mandelbulb_params* mb, uint32_t width, uint32_t height,
                         const fr_shard* shard, const fr_output* out);

/* Asynchronous form, the fr_render_shard_async contract: device planes only, enqueued on hip_stream (NULL = the
 * context's stream), launch-only in steady state; errors the device reports later surface through fr_ctx_check.
 * "timing", fr_ctx_last_kernel_ms and fr_ctx_last_grid cover it. */
int fr_render_mandelbulb_async(fr_ctx* ctx, const fr_params* p, const fr_mandelbulb_params* mb, uint32_t width,
                               uint32_t height, const fr_shard* shard, const fr_output* out, void* hip_stream);

/* ---- Mandelbrot views deeper than double precision ------------------------------------------------------------------
 * fr_params holds its centre as double, so no other path can show a view whose pixel spacing is below one ulp of the
 * centre (about 1e-13 of height near |c| ~ 1): neighbouring pixels collapse onto one c.  These entry points take the
 * centre as decimal strings and render by perturbation around ONE reference orbit:
 *   - the reference Z_n at the exact centre C is computed on the host in fixed point with frac_bits fraction bits
 *     (below) and stored as doubles;
 *   - every sample iterates its fp64 delta dz from it, dc being its offset from the centre, and is REBASED to the start
 *     of the orbit (dz = z, m = 0) whenever |z| < |dz| or the orbit ends (Zhuoran's rebasing): no glitch detection and
 *     no second reference are needed.
 * Deltas are fp64, so the zoom reaches 1e-290; fr_render_deepx (below, FR_HAS_DEEPX) carries them with an extended exponent
 * and reaches 1e-1000, and fr_deep_sequence (below it, FR_HAS_DEEP_SEQUENCE) walks a zoom into one centre through such views.
 *
 * The view: centre_x / centre_y are decimal strings, [+-]digits[.digits][(e|E)[+-]digits], at most 4096 characters,
 * |centre| < 2^32; p->center_x and p->center_y are ignored.  The zoom is p->zoom (the view height, as everywhere), finite
 * and in [1e-290, 1e3].  p->fractal_type must be FR_FRACTAL_MANDELBROT and p->precision FR_PRECISION_F64, and the orbit
 * trap, stripes and interior_style 2 are not available (they need the whole orbit): otherwise FR_ERR_UNSUPPORTED.  The
 * other fields follow fr_params_validate's rules; bailout must also be <= 2^16.  A malformed string, reserved != 0 or
 * frac_bits outside {0} U [128, 4096] is FR_ERR_INVALID_ARG.
 *
 * Reference orbit: each centre string becomes a signed fixed-point number with F = frac_bits fraction bits and at least 64
 * integer bits, rounded to nearest, ties to even.  From Z_0 = 0, Z_{n+1} = Z_n^2 + C with
 *   Re = floor(Zr Zr / 2^F) - floor(Zi Zi / 2^F) + Cr,   Im = floor(2 Zr Zi / 2^F) + Ci
 * (floor: the arithmetic shift of two's complement), up to the first N with |Z_N|^2 > bailout^2 (compared exactly) or
 * N = max_iterations.  Z_0 .. Z_N are stored as doubles, rounded to nearest.
 *
 * Per sample (x, y) and sub-sample (sx, sy) -- shaders/mandelbrot.comp:219-230's order, sy outer:
 *   dc = (((x + sx/aa) - 0.5 W) / H * zoom, ((y + sy/aa) - 0.5 H) / H * zoom), dz = 0, m = 0; then for i = 0 .. max_iter-1:
 *   t = (Z_m + Z_m) + dz;  dz' = (t.x dz.x - t.y dz.y, t.x dz.y + t.y dz.x) + dc;  m += 1;  z = Z_m + dz';  r2 = |z|^2
 *   r2 > bailout^2: escaped at i;  else if r2 < |dz'|^2 or m == N: dz = z, m = 0 (rebase);  else dz = dz'
 * each operation one fp64 rounding as written (no contraction).  The planes are those of fr_render's fp64 Mandelbrot path
 * for the same (i, r2): nu (double) = smooth count of sample (0,0), iter = its i (max_iterations for interior), rgba =
 * palette / interior_style 0-1 / aa average / FR_FLAG_POST_CHAIN exactly as there. */
#define FR_HAS_DEEP 1
#define FR_HAS_DEEP_BLA 1         /* FR_FLAG_DEEP_BLA and fr_ctx_last_deep_steps (below fr_render_deep_async) */

typedef struct fr_deep_view {
    const char* center_x;          /* decimal string (see above) */
    const char* center_y;
    int32_t     frac_bits;         /* fraction bits F of the reference orbit; 0 = automatic (fr_deep_frac_bits(zoom)) */
    int32_t     reserved;          /* must be 0 */
} fr_deep_view;                    /* 24 bytes on LP64 */

/* "-0.5", "0", 0, 0: FractalState's centre (src/fractal_state.h:18-19). */
int fr_deep_view_default(fr_deep_view* v);

/* The automatic fraction bits: 64 + (int)(-log10(zoom) * 3.32) + 64 (the reference's calculate_required_precision_bits,
 * src/deep_zoom_system.cpp:209-260), clamped to [128, 4096], rounded up to a multiple of 64.  zoom must be finite and > 0
 * (FR_ERR_INVALID_ARG otherwise). */
int fr_deep_frac_bits(double zoom);

/* The reference orbit of a view, on the host (for callers and tests): out_xy receives Z_0 .. Z_N as (re, im) doubles,
 * 2 (max_iter + 1) doubles at most; *out_len = N + 1.  Validates the view, zoom (for the automatic F), max_iter and
 * bailout as fr_render_deep does.  Takes about 3 L^2 64x64-bit products per iteration, L = ceil(F / 64) + 1 limbs. */
int fr_deep_reference_orbit(const fr_deep_view* v, double zoom, int32_t max_iter, float bailout, double* out_xy,
                            int32_t* out_len);

/* A deep view (or one part of a row-strip sharding of it: shard NULL = the whole frame) into `out`, synchronously.
 * Planes as for fr_render: FR_MEM_HOST / FR_MEM_DEVICE, FR_LAYOUT_FRAME.  Options: "shards" and "timing" apply,
 * "periodicity" and "staging" are accepted and have no effect; fr_ctx_last_kernel_ms and fr_ctx_last_grid cover it.
 * Orbit cache: the context keeps the most recent reference orbit on the device, keyed by (centre strings, F,
 * max_iterations, bailout); a render of another view computes its orbit on the host first. */
int fr_render_deep(fr_ctx* ctx, const fr_params* p, const fr_deep_view* view, uint32_t width, uint32_t height,
                   const fr_shard* shard, const fr_output* out);

/* Asynchronous form, the fr_render_shard_async contract: device planes only, enqueued on hip_stream (NULL = the
 * context's stream); errors the device reports later surface through fr_ctx_check.  A render of the view whose orbit
 * the context holds is launch-only.  A render of a NEW view computes its reference orbit on the host (the calling thread,
 * see fr_deep_reference_orbit for the cost) and waits for hip_stream -- and for the stream of the context's previous
 * render -- before it reuses its pinned upload buffer and the device orbit: never launch-only. */
int fr_render_deep_async(fr_ctx* ctx, const fr_params* p, const fr_deep_view* view, uint32_t width, uint32_t height,
                         const fr_shard* shard, const fr_output* out, void* hip_stream);

/* Bilinear approximation (BLA): iteration skipping for deep views, opt-in per call with FR_FLAG_DEEP_BLA in p->flags.
 * Only fr_render_deep and fr_render_deep_async read the flag; without it every byte they write is as above.  Near a deep
 * centre most iterations are the linear part of the step, dz' = 2 Z_m dz + dz^2 + dc with |dz| far below |Z_m|; BLA
 * replaces 2^k of them with ONE step dz' = A dz + B dc while |dz| is below a validity radius r.  (A, B, r) come from a
 * table built on the device from the cached reference orbit Z_0 .. Z_N.
 *
 * Notation: |w| = sqrt(w.x*w.x + w.y*w.y); complex products are written out as in the step above; every operation is one
 * fp64 rounding (no contraction).  sqrt is correctly rounded (on gfx950: the OCML expansion of llvm.sqrt.f64, rsq plus
 * Newton-Raphson with a final fma residual correction).
 *   - Constants: eps = 2^-53;  dcmax = (1.0000001 * (0.5 * zoom)) * sqrt((W/H)*(W/H) + 1), W/H and zoom of the WHOLE
 *     frame (never of a shard's rows), so a shard's planes equal the matching rows of the whole frame, byte for byte.
 *   - Single step at m >= 1 (never stored): A = (Z_m + Z_m), B = (1, 0), r = eps * |Z_m|.
 *   - Table: levels k = 1 .. K, K = floor(log2(N - 1)) (N <= 2: no table).  Entry j of level k covers the 2^k steps
 *     from m = 1 + j 2^k and exists iff m + 2^k <= N.  It merges x (level k-1 at m) and y (level k-1 at m + 2^(k-1)):
 *       A = A_y*A_x,  B = A_y*B_x + B_y,  t = (r_y - |B_x|*dcmax) / |A_x|,  r = (t > 0 ? t : 0) (NaN: 0),
 *       r = (r < r_x ? r : r_x),  and r = 0 if A or B is not finite.
 *     So r never exceeds r_x: validity is monotone in k.
 *   - Stepping: u (the update index) replaces the loop index i.  At each trip of a sample with m >= 1, take the largest
 *     k >= 1 with (m-1) mod 2^k == 0, m + 2^k <= N, u + 2^k <= max_iterations and dz.x*dz.x + dz.y*dz.y < r*r; then
 *       dz' = ((A.x dz.x - A.y dz.y) + (B.x dc.x - B.y dc.y), (A.x dz.y + A.y dz.x) + (B.x dc.y + B.y dc.x)),
 *       m += 2^k, u += 2^k, z = Z_m + dz', r2 = |z|^2 (as the plain step writes it);
 *     r2 > bailout^2: escaped at u - 1 (the last update the step covered); else the rebase rule of the plain step
 *     (r2 < |dz'|^2 or m == N).  If no k qualifies, or m == 0, the plain step above, unchanged: it escapes at u and then
 *     u += 1.  The planes follow from (escape index, r2) exactly as without the flag.
 * Where it differs from the plain step: a single step drops dz^2 only where |dz| / (2 |Z_m|) < 2^-54, below one rounding of
 * the kept term; merged steps differ from single ones by rounding order only.  Escapes between the first and the last
 * update of a BLA step are not looked for.
 *
 * Cost: the table has (N - 1) - popcount(N - 1) < N entries of 40 bytes (r 8, A and B 32), on the device, per context,
 * grown like the orbit buffer (about 0.67 GB at N = 2^24; an allocation failure is FR_ERR_HIP).  It is cached, keyed by the
 * orbit and the bits of dcmax: a zoom change at a fixed centre rebuilds it (K small launches on the render's stream, no
 * host work and no upload), a new view computes its orbit first as above.  A rebuild is ordered behind the context's
 * previous BLA render, whatever stream it went to. */

/* The step counts of the context's most recent fr_render_deep(_async) call made with FR_FLAG_DEEP_BLA, over every
 * sub-sample of its in-frame pixels: out[0] plain steps, out[1] BLA steps, out[2] updates skipped (the sum of 2^k over
 * the BLA steps).  A synchronous call has them on return, an asynchronous one once its stream has completed.
 * FR_ERR_UNSUPPORTED if there is no such call. */
int fr_ctx_last_deep_steps(fr_ctx* ctx, uint64_t out[3]);

/* ---- distance estimates for deep Mandelbrot views ---------------------------------------------------------------------------
 * At depth the filaments of the set are far thinner than a pixel and the smooth count of a frame is noise (view C of the tests,
 * a 1e-50 minibrot neighbourhood: the median escaped pixel lies 0.005 pixel spacings from the set).  fr_render_deep_de is
 * fr_render_deep with the derivative dz/dc carried through the perturbation loop, its rebases and its BLA steps, and two planes
 * more: the exterior distance estimate |z| log|z| / |dz/dc| of shaders/mandelbrot_debug.comp:106-148, and the derivative
 * itself.  Range, view, orbit and flags are fr_render_deep's: Mandelbrot, FR_PRECISION_F64, zoom in [1e-290, 1e3], plain or
 * with FR_FLAG_DEEP_BLA.  fr_render_deep and every other entry point are untouched.
 *
 * The arithmetic (fp64, one rounding per operation as written, no contraction), next to fr_render_deep's step above:
 *   - s = zoom / H, H the height of the WHOLE frame (never a shard's rows): one pixel spacing.  D = (0, 0) at the start.
 *     D is dz/dc * s: scaled so that it stays in range down to zoom 1e-290 (s ~ 1e-292, where dz/dc itself reaches 1e292 and
 *     more before a sample escapes) and so that |D| at escape is about 1 / de with de in pixel spacings.
 *   - Plain step: D' is formed in every trip, from the sample's point before the update,
 *       z = Z_m + dz   (the sum the previous trip's escape test formed; (0, 0) at the start; dz itself behind a rebase, Z_0 = 0)
 *       w = z + z;   D' = ((w.x D.x - w.y D.y) + s,  w.x D.y + w.y D.x)
 *   - BLA step with the entry (A, B) the sample takes: D' = ((A.x D.x - A.y D.y) + B.x s,  (A.x D.y + A.y D.x) + B.y s),
 *     the derivative of the linear map dz' = A dz + B dc that the step applies -- exact for that map, whatever the map drops.
 *   - A rebase leaves D alone: the point does not move.
 *   - Escape with r2:  zl = sqrt(r2);  dl = sqrt(D.x D.x + D.y D.y);  de = (zl * log(zl)) / dl;  a NaN de becomes 0; an
 *     overflowing |D| gives 0 by the division.  log is the device library's (within 1 ulp), sqrt is correctly rounded.
 *   - Interior samples (iter == max_iterations): de = 0, deriv = (0, 0).
 * D never feeds back: iter, nu, r2 and the three step counts are bit for bit fr_render_deep's for the same parameters.
 *
 * Shading (shade == 1), mandelbrot_debug.comp:196-197 with the edge in pixels, in fp32 on every ESCAPED sub-sample's linear rgb,
 * before the aa average and before FR_FLAG_POST_CHAIN (interior samples are not shaded: the shader returns before them):
 *   x = clamp((float)de / edge_px, 0, 1);  sm = x*x*(3 - 2x);  t = (1 - sm) * 0.3f;  rgb = rgb*(1 - t) + (rgb*0.7f)*t
 *
 * Planes: de->de and de->deriv follow out->memory and out->layout exactly as out->nu does (FR_MEM_HOST stages them like the
 * other planes).  Of the five planes rgba, nu, iter, de, deriv at least one must be given; rgba is not required.
 * Shared state: the orbit cache slot, the BLA table with its key, and fr_ctx_last_deep_steps are fr_render_deep's own -- a
 * call here after fr_render_deep of the same view computes no orbit and builds no table, and the reverse.
 * Validation: everything fr_render_deep checks; `de` NULL, shade outside {0, 1}, or shade == 1 with edge_px not finite or
 * <= 0 is FR_ERR_INVALID_ARG.
 * Cost: four live VGPRs and 11 fp64 operations per plain update on top of the step's 18 (README: measured).
 * Extended views below 1e-290, where s underflows and D needs an exponent of its own, are fr_render_deepx_de (below,
 * FR_HAS_DEEPX_DE); Julia sets are fr_render_deep_julia_de (FR_HAS_DEEP_JULIA_DE); the Burning Ship, whose derivative is a
 * real 2x2 Jacobian, is fr_render_deep_ship_de (FR_HAS_DEEP_SHIP_DE).  Out of scope: fr_deep_sequence; fr_node and .franim;
 * slope or normal lighting -- deriv is what a caller needs for it. */
#define FR_HAS_DEEP_DE 1

typedef struct fr_deep_de {
    double* de;       /* rows*W: distance estimate of sample (0,0), in PIXEL SPACINGS of the whole frame (zoom / H); 0 for
                       * interior.  NULL to skip */
    double* deriv;    /* rows*W*2: (D.x, D.y) of sample (0,0) at its escaping update, (0,0) for interior.  NULL to skip */
    int32_t shade;    /* 0: rgba exactly fr_render_deep's; 1: the debug shader's distance shading on every escaped sub-sample */
    float   edge_px;  /* shade == 1: the smoothstep's upper edge in pixel spacings, finite > 0 */
} fr_deep_de;         /* 24 bytes on LP64 */

/* NULL, NULL, 0, 1.8f  (0.005 c-plane units, mandelbrot_debug.comp:196, at zoom 3.0 on 1080 rows) */
int fr_deep_de_default(fr_deep_de* de);

/* What fr_render_deep_de checks of its arguments, the centre strings parsed included (no context needed). */
int fr_deep_de_validate(const fr_params* p, const fr_deep_view* view, const fr_deep_de* de, uint32_t width, uint32_t height);

/* fr_render_deep with the distance planes; options, timing and the orbit cache as there. */
int fr_render_deep_de(fr_ctx* ctx, const fr_params* p, const fr_deep_view* view, const fr_deep_de* de, uint32_t width,
                      uint32_t height, const fr_shard* shard, const fr_output* out);

/* Asynchronous form: fr_render_deep_async's contract, de->de and de->deriv device planes like the others. */
int fr_render_deep_de_async(fr_ctx* ctx, const fr_params* p, const fr_deep_view* view, const fr_deep_de* de, uint32_t width,
                            uint32_t height, const fr_shard* shard, const fr_output* out, void* hip_stream);

/* ---- Burning Ship views deeper than double precision ----------------------------------------------------------------------
 * fr_render_deep for z <- (|x| + i |y|)^2 + c: the same perturbation around one reference orbit with rebasing, the same view
 * (fr_deep_view, p->zoom in [1e-290, 1e3], p->center_x / p->center_y ignored), planes, shards and asynchronous rules.  The
 * mini-ships along the needle near -1.75 lie far below double precision; this is the path that shows them.
 *
 * p->fractal_type must be FR_FRACTAL_BURNING_SHIP and p->precision FR_PRECISION_F64.  FR_ERR_UNSUPPORTED also where the ship
 * needs the whole orbit -- orbit_trap_enabled, stripe_enabled with interior_style 2, interior_style 3 -- and for
 * FR_FLAG_DEEP_BLA or FR_FLAG_DEEPX_BLA (the ship's own flag is FR_FLAG_DEEP_SHIP_BLA, below).  The other fields follow
 * fr_params_validate's rules; bailout must be <= 2^16.
 * fr_render_deep keeps rejecting FR_FRACTAL_BURNING_SHIP.
 *
 * Reference orbit: fr_render_deep's fixed point and escape test, with
 *   Re = floor(Zr Zr / 2^F) - floor(Zi Zi / 2^F) + Cr,   Im = floor(2 |Zr| |Zi| / 2^F) + Ci
 * (|Zr|^2 = Zr^2, so Re is unchanged).  Z_0 .. Z_N are stored as doubles, SIGNED.
 *
 * The fold: for an orbit coordinate X and a delta a, |X + a| - |X| without forming |X + a| from a cancelling sum --
 *   fold(X, a):  w = X + a;  d = (X + X) + a;     X >= 0 ?  (w >= 0 ? a : -d)  :  (w > 0 ? d : -a)
 * The sign of w is exact: an IEEE sum is zero only when it is exactly zero.
 *
 * Per sample (x, y) and sub-sample s = 0 .. aa*aa-1 with sx = s / aa (OUTER), sy = s % aa -- shaders/burning_ship.comp:393,
 * :322-325, :337-344, the map fr_render's fp64 Burning Ship path applies, less the centre:
 *   uvx = x / W;  uvy = y / H;   aa > 1:  pixel_size = 1 / W;  sample_offset = pixel_size / aa;
 *       centre = sample_offset * (aa - 1) * 0.5;  uvx = uvx + (sx * sample_offset - centre) / W;
 *       uvy = uvy + (sy * sample_offset - centre) / H
 *   dc = ((uvx - 0.5) * zoom * aspect, (uvy - 0.5) * zoom),  aspect = (double)W / (double)H of the WHOLE frame
 * (not Mandelbrot's map).  dz = 0, m = 0; then for i = 0 .. max_iter-1, with Z_m = (X, Y), dz = (a, b),
 * U = (|X|, |Y|), f = (fold(X, a), fold(Y, b)):
 *   t = (U + U) + f;  dz' = (t.x f.x - t.y f.y, t.x f.y + t.y f.x) + dc;  m += 1;  z = Z_m + dz';  r2 = |z|^2
 *   r2 > bailout^2: escaped at i;  else if r2 < |dz'|^2 or m == N: dz = z, m = 0 (rebase);  else dz = dz'
 * each operation one fp64 rounding as written (no contraction).  Z_0 = 0 keeps the rebase valid: at m = 0 the step is
 * (|a| + i |b|)^2 + dc.  The planes are those of fr_render's fp64 Burning Ship path for the same (i, r2): nu (double) =
 * i + 1 - log2(log2(r2) / log2(bailout)) of sample s = 0 (max_iterations for interior), iter = its i, rgba = palette,
 * interior samples black (burning_ship.comp:259-283 without effects), aa average, FR_FLAG_POST_CHAIN with the Julia /
 * Burning Ship floors.  A shard's planes equal the matching rows of the whole frame, byte for byte.
 *
 * The context keeps the most recent ship orbit on the device in a slot of its own, keyed as fr_render_deep's: a ship render
 * never evicts the Mandelbrot orbit, nor the reverse.
 *
 * Out of scope: fr_node and .franim.  Extended exponents below 1e-290 are fr_render_deepx_ship (below, FR_HAS_DEEPX_SHIP), zoom
 * sequences fr_deep_ship_sequence_create (FR_HAS_DEEP_SHIP_SEQUENCE). */
#define FR_HAS_DEEP_SHIP 1
#define FR_HAS_DEEP_SHIP_BLA 1    /* FR_FLAG_DEEP_SHIP_BLA and fr_ctx_last_deep_ship_steps (below fr_render_deep_ship_async) */

/* fr_deep_reference_orbit for the ship's recurrence: same arguments, validation and cost */
int fr_deep_ship_reference_orbit(const fr_deep_view* v, double zoom, int32_t max_iter, float bailout, double* out_xy,
                                 int32_t* out_len);

/* fr_render_deep's contract (planes, memory kinds, FR_LAYOUT_FRAME, shards, options, fr_ctx_last_kernel_ms / _grid) */
int fr_render_deep_ship(fr_ctx* ctx, const fr_params* p, const fr_deep_view* view, uint32_t width, uint32_t height,
                        const fr_shard* shard, const fr_output* out);

/* fr_render_deep_async's contract: a render of a new view computes its orbit on the host first and is never launch-only */
int fr_render_deep_ship_async(fr_ctx* ctx, const fr_params* p, const fr_deep_view* view, uint32_t width, uint32_t height,
                              const fr_shard* shard, const fr_output* out, void* hip_stream);

/* Bilinear approximation for the ship, opt-in per call with FR_FLAG_DEEP_SHIP_BLA in p->flags.  Only fr_render_deep_ship and
 * fr_render_deep_ship_async read the flag; without it every byte they write is as above.  Take an orbit point Z_m = (X, Y)
 * and a delta dz = (a, b) with |a| < |X| and |b| < |Y|: no fold flips a sign, fold(X, a) = sgn(X) a, fold(Y, b) = sgn(Y) b,
 * and the ship's step less its square term is the REAL linear map dz' = A dz + dc with
 *   A = [[2X, -2Y], [2|Y| sgn X, 2|X| sgn Y]].
 * The columns of A are orthogonal and both have length 2 |Z_m|: A is 2 |Z_m| times a rotation or reflection, and so is every
 * product of such matrices.  The validity argument of FR_FLAG_DEEP_BLA therefore carries over with |A| read as a column
 * length; the only new conditions are the two fold conditions, which cap the single step's radius.
 *
 * Notation: matrices are (m11, m12, m21, m22), row by row; sgn(v) = (v >= 0 ? 1 : -1); every operation is one fp64 rounding
 * (no contraction); sqrt is correctly rounded (as for FR_FLAG_DEEP_BLA).
 *   - Constants: eps = 2^-53.  With a = (double)W / (double)H of the WHOLE frame (never of a shard's rows):
 *       hx = 0.5 + 0.5 / (W*W);  hy = 0.5 + 0.5 / (W*H);  ex = hx * a;  dcmax = (1.0000001 * zoom) * sqrt(ex*ex + hy*hy)
 *     (W*W and W*H as products of doubles).  Not FR_FLAG_DEEP_BLA's dcmax: with aa > 1 the ship shader's sub-sample offsets
 *     reach (aa-1)/(2 aa W^2) outside [0, 1) in uvx and (aa-1)/(2 aa W H) in uvy, more than the 1e-7 margin on small frames.
 *   - Single step at m >= 1 (never stored), Z_m = (X, Y), sx = sgn(X), sy = sgn(Y):
 *       A = (X + X, -(Y + Y), (|Y| + |Y|) * sx, (|X| + |X|) * sy),  B = (1, 0, 0, 1),
 *       r = eps * sqrt(X*X + Y*Y);  r = (r < |X| ? r : |X|);  r = (r < |Y| ? r : |Y|)
 *     The last two are the fold conditions.  An orbit on the real axis (centre_y "0") has Y = 0 throughout: r = 0, and it
 *     takes no BLA step.
 *   - Table: the levels, the entry coverage and the entry count (N - 1) - popcount(N - 1) of FR_FLAG_DEEP_BLA.  Entry j of
 *     level k merges x (level k-1 at m) and y (level k-1 at m + 2^(k-1)):
 *       A = A_y A_x, the real 2x2 product, each element p*q + s*t (a11 = y.a11*x.a11 + y.a12*x.a21, ...);
 *       B = A_y B_x + B_y, each element (p*q + s*t) + y.b (b11 = (y.a11*x.b11 + y.a12*x.b21) + y.b11, ...);
 *       |A_x| = sqrt(x.a11*x.a11 + x.a21*x.a21), the first column: A_x is a scaled orthogonal matrix, so its operator norm;
 *       |B_x| = sqrt((x.b11*x.b11 + x.b12*x.b12) + (x.b21*x.b21 + x.b22*x.b22)), the Frobenius norm;
 *       t = (r_y - |B_x| * dcmax) / |A_x|,  r = (t > 0 ? t : 0) (NaN: 0),  r = (r < r_x ? r : r_x),
 *       and r = 0 if any of the eight elements is not finite.
 *   - Stepping: FR_FLAG_DEEP_BLA's, u replacing the loop index.  At m >= 1 take the largest k >= 1 with
 *     (m-1) mod 2^k == 0, m + 2^k <= N, u + 2^k <= max_iterations and dz.x*dz.x + dz.y*dz.y < r*r; then
 *       dz' = ((a11 dz.x + a12 dz.y) + (b11 dc.x + b12 dc.y), (a21 dz.x + a22 dz.y) + (b21 dc.x + b22 dc.y)),
 *       m += 2^k, u += 2^k, z = Z_m + dz', r2 = |z|^2;
 *     r2 > bailout^2: escaped at u - 1; else the rebase rule of the plain step.  If no k qualifies, or m == 0, the ship's
 *     plain step above, operation for operation: it escapes at u and then u += 1.  The planes follow from (escape index,
 *     r2) exactly as without the flag.  No level's r exceeds eps |Z_m|.
 * Escapes between the first and the last update of a BLA step are not looked for.
 *
 * What it skips (the numpy restatement, 256 x 192, aa 1): on a view at 1e-30 whose reference escapes (N = 197) 42.8 % of the
 * updates, 1.70x fewer loop trips, iter equal to the unflagged path's on every pixel; on a view at 1e-100 (N = 590) 75.3 %,
 * 3.94x fewer trips, iter different on 23 of 49152 pixels.  Shallow views (|dc| far above every radius) take no BLA step.
 * Measured on one MI355X at 4096^2 (profiles/deep_ship_bla_time.txt, flagged and unflagged interleaved in one session):
 * 4.67 ms against 5.48 ms on the first view (1.17x) and 6.87 ms against 17.24 ms on the second (2.51x); a flagged loop trip
 * costs about 1.5 plain ones (the level probe, the 64-byte gather, 4 waves per SIMD for 5).
 *
 * Cost: 72 bytes per entry (r 8, A and B 64), on the device, per context, in buffers of the ship path's own, grown like the
 * orbit buffer and keyed by the ship's orbit and the bits of dcmax: a zoom change at a fixed centre rebuilds the table (K
 * small launches on the render's stream, no host work), a new view computes its orbit first.  A rebuild, and the upload of
 * a new ship orbit, are ordered behind the context's previous render with the flag, whatever stream it went to.  The
 * Mandelbrot tables, their counts and fr_ctx_last_deep_steps are untouched by ship renders, and the reverse. */

/* fr_ctx_last_deep_steps' contract for the context's most recent fr_render_deep_ship / fr_render_deep_ship_async call made with
 * FR_FLAG_DEEP_SHIP_BLA: out[0] plain steps, out[1] BLA steps, out[2] updates skipped.  FR_ERR_UNSUPPORTED if there is no such
 * call. */
int fr_ctx_last_deep_ship_steps(fr_ctx* ctx, uint64_t out[3]);

/* ---- deep views below 1e-290: extended-exponent deltas ----------------------------------------------------------------
 * fr_render_deep stops where a double can no longer hold the zoom, a sample's dc and dz, or an orbit point that passes
 * close to 0.  These entry points take the ZOOM as a decimal string too and carry every delta as two double mantissas
 * with one shared int32 binary exponent while it is small; nothing about fr_render_deep changes.
 *
 * The view: centre strings as fr_deep_view; zoom = the view height as a decimal string of the same grammar, read as
 * zm 2^ze, zm a double in [1, 2) holding the decimal value correctly rounded to 53 significant bits (ties to even), ze an
 * int32 (fr_deepx_zoom returns the pair).  1e-1000 <= zoom <= 1e3, compared on the rounded pair.  p->zoom, p->center_x and
 * p->center_y are ignored.  FR_ERR_UNSUPPORTED as for fr_render_deep, and for FR_FLAG_DEEP_BLA (the fp64 table; the
 * extended views' own flag is FR_FLAG_DEEPX_BLA, below), with or without FR_FLAG_DEEPX_BLA;
 * FR_ERR_INVALID_ARG for a malformed or out-of-range zoom, and otherwise as there.
 *
 * Reference orbit: Z_0 .. Z_N exactly as for fr_render_deep (same recurrence, same escape test, F = frac_bits or
 * fr_deepx_frac_bits(zoom)); what differs is the storage.  Point n is (mx, my) 2^e: two doubles and one int32, in two
 * arrays (mantissa pairs, exponents).  A point whose larger component is at least 2^-1022 has e = 0 and (mx, my) = the
 * doubles of fr_deep_reference_orbit; a smaller one has e = floor(log2(larger component)) + 1, so that its larger mantissa
 * lies in [0.5, 1), each mantissa rounded once to nearest from the fixed-point value; (0, 0) has e = FR_DEEPX_ZERO_EXP.  The
 * device also keeps P_n = (ldexp(mx, e), ldexp(my, e)) as plain doubles (rounded to nearest; for e = 0 the same doubles):
 * the plain mode below loads 16 bytes per point as fr_render_deep does, the extended mode 20.
 *
 * Extended numbers: X = (x, y, e) stands for (x, y) 2^e, x and y doubles.  Every mantissa operation below is one IEEE
 * fp64 operation, rounded to nearest (no contraction; gradual underflow of a mantissa as IEEE has it), every exponent
 * operation is exact int32 arithmetic, ldexp(x, n) = x 2^n rounded to nearest (exact unless the result is subnormal).
 *   norm(x, y, e):  k = frexp exponent of max(|x|, |y|) (that maximum in [2^(k-1), 2^k); 0 for 0);
 *                   (ldexp(x, -k), ldexp(y, -k), e + k), and e = FR_DEEPX_ZERO_EXP when x = y = 0.
 *   A (+) B:        e = max(A.e, B.e);  (ldexp(A.x, A.e - e) + ldexp(B.x, B.e - e), same in y, e)   -- not normalised
 * Per sample: fx = ((x + sx/aa) - 0.5 W) / H, fy = ((y + sy/aa) - 0.5 H) / H as fr_render_deep forms them;
 *   dc = norm(fx * zm, fy * zm, ze): one rounding per component, then an exact exponent (for a zoom that is a normal double
 *   this is the dc of fr_render_deep, bit for bit);  dcp (the plain mode's dc) = (ldexp(dc.x, dc.e), ldexp(dc.y, dc.e)) with
 *   a component whose value is below 2^-1022 taken as 0;  dz = (0, 0, FR_DEEPX_ZERO_EXP), m = 0, mode = extended.
 * Then for i = 0 .. max_iter-1 one step in the sample's mode.
 *   EXTENDED (dz an extended number, normalised; Z_m, Z_{m+1} in the extended storage):
 *     t = (Z_m.x, Z_m.y, Z_m.e + 1) (+) dz;
 *     p = (t.x dz.x - t.y dz.y, t.x dz.y + t.y dz.x, t.e + dz.e);   n = p (+) dc;   m += 1;   z = Z_m (+) n;
 *     r2 = z.x z.x + z.y z.y;   escaped at i if ldexp(r2, 2 z.e) > bailout^2 (that double is the sample's r2);
 *     else rebase if r2 < ldexp(n.x n.x + n.y n.y, 2 (n.e - z.e)) or m == N   (z.e >= n.e always);
 *     dz = norm(rebase ? z : n), m = 0 on a rebase.
 *     If now dz.e > -400 -- max(|dz.x|, |dz.y|) 2^dz.e >= 2^-400 -- the sample turns PLAIN with
 *     dz = (ldexp(dz.x, dz.e), ldexp(dz.y, dz.e)).
 *   PLAIN (dz two doubles): the step of fr_render_deep, operation for operation, on P_m, P_{m+1} and dcp.  If afterwards
 *     max(|dz.x|, |dz.y|) < 2^-400 the sample turns EXTENDED with dz = norm(dz.x, dz.y, 0).
 * The threshold 2^-400: the plain step multiplies two deltas (at m = 0, t = dz), so its products stay above 2^-802, far
 * inside the normal range, and nothing a double would flush enters a plain step; a component of dc below 2^-1022 is below
 * 2^-220 of those products, far under half an ulp of the dz' it is added to, so taking it as 0 loses nothing; an orbit
 * point below 2^-1022 read as P_m is likewise below half an ulp of the dz of at least 2^-401 it meets.  An extended step on
 * operands that a double holds performs the same roundings as the plain step (the exponents only carry the scale), so a
 * view whose dc is at least 2^-400 -- every zoom down to about 1e-117 -- leaves the extended mode on its first step and
 * gets the bytes of fr_render_deep.  Planes, shards, layouts, memory kinds, options, fr_ctx_last_kernel_ms / _grid and
 * the asynchronous form's rules are those of fr_render_deep; the context keeps the most recent extended orbit on the device
 * next to (and independent of) fr_render_deep's, keyed by (centre strings, F, max_iterations, bailout).
 *
 * Out of scope: fr_node and .franim for deep views, and depths beyond 1e-1000 (the 4096-bit cap of F).  A zoom into one
 * centre, frame after frame, is fr_deep_sequence (below, FR_HAS_DEEP_SEQUENCE); fr_zoom_path stays a double. */
#define FR_HAS_DEEPX 1
#define FR_HAS_DEEPX_BLA 1        /* FR_FLAG_DEEPX_BLA and fr_ctx_last_deepx_steps (below fr_render_deepx_async) */
#define FR_DEEPX_ZERO_EXP (-(1 << 28))   /* the exponent of a zero in the extended storage */

typedef struct fr_deepx_view {
    const char* center_x;          /* as fr_deep_view */
    const char* center_y;
    const char* zoom;              /* the view height as a decimal string, same grammar as the centre, > 0 */
    int32_t     frac_bits;         /* 0 = automatic (fr_deepx_frac_bits(zoom)) */
    int32_t     reserved;          /* must be 0 */
} fr_deepx_view;                   /* 32 bytes on LP64 */

/* "-0.5", "0", "3", 0, 0 */
int fr_deepx_view_default(fr_deepx_view* v);

/* The zoom string as *mant 2^*exp2, *mant in [1, 2) (above).  FR_ERR_INVALID_ARG for a malformed string or a value
 * outside [1e-1000, 1e3]. */
int fr_deepx_zoom(const char* zoom, double* mant, int32_t* exp2);

/* The automatic fraction bits: fr_deep_frac_bits((double)zoom) for a zoom that is a double >= 1e-290, else the same rule on
 * -log10(zoom) = -(log10(zm) + ze * log10(2)): 3456 at 1e-1000.  < 0: the error of fr_deepx_zoom. */
int fr_deepx_frac_bits(const char* zoom);

/* The reference orbit in the extended storage, on the host: out_mant_xy receives 2 (max_iter + 1) doubles at most,
 * out_exp2 max_iter + 1 exponents; *out_len = N + 1.  Cost as fr_deep_reference_orbit. */
int fr_deepx_reference_orbit(const fr_deepx_view* v, int32_t max_iter, float bailout, double* out_mant_xy, int32_t* out_exp2,
                             int32_t* out_len);

/* fr_render_deep's contract (planes, memory kinds, FR_LAYOUT_FRAME, shards, options, the orbit cache) for an extended view */
int fr_render_deepx(fr_ctx* ctx, const fr_params* p, const fr_deepx_view* view, uint32_t width, uint32_t height,
                    const fr_shard* shard, const fr_output* out);

/* fr_render_deep_async's contract: a render of a new view computes its orbit on the host first and is never launch-only */
int fr_render_deepx_async(fr_ctx* ctx, const fr_params* p, const fr_deepx_view* view, uint32_t width, uint32_t height,
                          const fr_shard* shard, const fr_output* out, void* hip_stream);

/* Bilinear approximation for extended views, opt-in per call with FR_FLAG_DEEPX_BLA in p->flags.  Only fr_render_deepx and
 * fr_render_deepx_async read the flag; without it every byte they write is as above.  It is FR_FLAG_DEEP_BLA's scheme with
 * the table and the BLA step carried in the extended arithmetic of this section (A grows like 1 / zoom, far beyond a
 * double), taken by samples in either mode.  (A, B, r) come from a table built on the device from the cached extended orbit.
 *
 * Notation: extended complex (x, y, e), norm and (+) as above.  An extended real (v, e) stands for v 2^e; normalised it has
 * v in [0.5, 1) (k = frexp exponent of v; (ldexp(v, -k), e + k)), and zero has e = FR_DEEPX_ZERO_EXP.  P (x) Q is the complex
 * mantissa product written out as in the plain step, (P.x Q.x - P.y Q.y, P.x Q.y + P.y Q.x), each operation one rounding,
 * with the exponent P.e + Q.e, not normalised unless said.  |w| of a normalised extended complex is
 * (sqrt(w.x*w.x + w.y*w.y), w.e), then normalised; sqrt is correctly rounded as for FR_FLAG_DEEP_BLA.
 *   - Constants: eps = 2^-53;  dcmax = the extended real ((1.0000001 * (0.5 * zm)) * sqrt((W/H)*(W/H) + 1), ze), normalised,
 *     W/H of the WHOLE frame (never of a shard's rows).
 *   - Single step at m >= 1 (never stored): A = norm(Z_m.x, Z_m.y, Z_m.e + 1) from the extended storage, B = norm(1, 0, 0),
 *     r = eps * |norm(Z_m)|, the multiplication by 2^-53 going to the exponent (r = 0 stays the zero).
 *   - Table: levels, entry indexing and the existence rule are exactly those of FR_FLAG_DEEP_BLA.  Merging x then y:
 *       A = norm(A_y (x) A_x),   B = norm((A_y (x) B_x) (+) B_y),
 *       t = (r_y (-) |B_x| dcmax) (/) |A_x|:  |B_x| dcmax = (|B_x|.v dcmax.v, |B_x|.e + dcmax.e);  (-) aligns both to the larger
 *         exponent e with ldexp and subtracts once;  (/) is one division of the mantissas with the exponent e - |A_x|.e;
 *       r = norm(t) if t's mantissa is > 0 and finite, else the zero (NaN: zero);  then r = r_x unless r < r_x, compared on
 *       the normalised (exponent, mantissa);
 *       if the exponent of A or of B lies outside [-2^27, 2^27] the entry is void: r, A and B are all stored as zero (this
 *       replaces the fp64 table's "not finite" rule; zeroing A and B too keeps every int32 exponent sum of the levels above
 *       in range, and r of every level above a void entry is 0 by the two rules before);
 *       last, the STORED r keeps the top 24 bits of its mantissa, the rest cleared (toward zero: a float holds it exactly),
 *       so that r is 8 bytes, a float and an int32; the merges of the next level and the probes read that stored value.  The
 *       single step's r is not stored and not cut.  A radius is a bound: cutting it can only refuse a step.
 *   - Stepping: u replaces the loop index as for FR_FLAG_DEEP_BLA, and the level choice is the one there: the largest
 *     k >= 1 with (m-1) mod 2^k == 0, m + 2^k <= N and u + 2^k <= max_iterations whose probe passes.  The probe is on dz as a
 *     normalised extended number -- a sample in the PLAIN mode uses norm(dz.x, dz.y, 0) --:
 *       dz.x*dz.x + dz.y*dz.y < ldexp(r.v*r.v, 2 (r.e - dz.e))      (r.v*r.v is exact: 24 bits squared).
 *     A BLA step is always taken in extended arithmetic, on that dz and the extended dc (never dcp):
 *       n = (A (x) dz) (+) (B (x) dc);   m += 2^k;   u += 2^k;   z = Z_m (+) n  (Z_m from the extended storage);
 *     then the escape test, the rebase rule, norm and the mode rule of the EXTENDED step, unchanged: escaped at u - 1 if
 *     ldexp(r2, 2 z.e) > bailout^2; dz = norm(rebase ? z : n); a result with dz.e > -400 turns the sample PLAIN.
 *     If no level qualifies, or m == 0, the sample takes the step of its mode above, operation for operation: it escapes at
 *     u and then u += 1.
 * Cost: (N - 1) - popcount(N - 1) entries of 48 bytes (r 8, the mantissas of A and B 32, their exponents 8), cached per
 * context next to the extended orbit, keyed by that orbit and the bits of dcmax (mantissa and exponent), grown like the orbit
 * buffer.  A zoom change at a fixed centre rebuilds it (K small launches on the render's stream, ordered behind the context's
 * previous render with the flag, whatever stream that went to); a cached view is launch-only.  The table belongs to this
 * path alone: it is not shared with, and does not invalidate, FR_FLAG_DEEP_BLA's. */

/* fr_ctx_last_deep_steps' contract for the context's most recent fr_render_deepx(_async) call made with FR_FLAG_DEEPX_BLA:
 * out[0] single steps (plain and extended), out[1] BLA steps, out[2] updates skipped.  FR_ERR_UNSUPPORTED if there is no
 * such call.  fr_ctx_last_deep_steps does not report these calls. */
int fr_ctx_last_deepx_steps(fr_ctx* ctx, uint64_t out[3]);

/* ---- distance estimates for extended views ------------------------------------------------------------------------------------
 * fr_render_deep_de (above, FR_HAS_DEEP_DE) for the views of fr_render_deepx: the same two planes more, the distance estimate
 * of sample (0,0) in pixel spacings and the scaled derivative D = dz/dc * s, down to zoom 1e-1000.  The view is fr_deepx_view,
 * the distance block fr_deep_de with fr_deep_de_default unchanged; range, precision and flags are fr_render_deepx's:
 * Mandelbrot, FR_PRECISION_F64, plain or with FR_FLAG_DEEPX_BLA.  Every other entry point is untouched.
 *
 * Below 1e-290 s = zoom / H underflows and D, which starts at s and reaches about 1 / de, crosses more than a double's range
 * on its way.  So D is an extended complex number (D.x, D.y, D.e) for the whole orbit, whatever mode the sample's delta is in,
 * normalised with norm after every update; the zero has FR_DEEPX_ZERO_EXP.  Notation as above: norm, and
 * (a, ea) (+) (b, eb) = ldexp(a, ea - e) + ldexp(b, eb - e) at e = max(ea, eb), per component.  Every operation is one fp64
 * rounding or an exact scaling, no contraction.
 *   - s = (sm, es) = the extended real (zm / (double)H, ze) normalised, H the height of the WHOLE frame, zm 2^ze the view's
 *     zoom (fr_deepx_zoom); the division is rounded once.  D = (0, 0, FR_DEEPX_ZERO_EXP) at the start.
 *   - EXTENDED single step: D' is formed from the sample's point before the update,
 *       eb = max(Z_m.e, dz.e);   b = ldexp(Z_m, Z_m.e - eb) + ldexp(dz, dz.e - eb), per component;
 *       P = (b.x D.x - b.y D.y,  b.x D.y + b.y D.x) at the exponent eP = eb + 1 + D.e  (the + 1 is the 2 of w = 2 z);
 *       e = max(eP, es);   D' = norm(ldexp(P.x, eP - e) + ldexp(sm, es - e),  ldexp(P.y, eP - e),  e)
 *     -- s is real: nothing is added to the imaginary part, whose zero keeps its sign as in fr_render_deep_de.
 *   - PLAIN single step: b = Z_m + dz on the plain doubles, w = b + b (the sums of fr_render_deep_de's step),
 *       P = (w.x D.x - w.y D.y,  w.x D.y + w.y D.x) at eP = D.e;   D' as above.
 *   - BLA step (FR_FLAG_DEEPX_BLA) with the entry (A, B) the sample takes, in either mode:
 *       P = A (x) D at eP = A.e + D.e;   Q = (B.x sm, B.y sm) at eQ = B.e + es;   D' = norm(P (+) Q)
 *     -- the derivative of the linear map the step applies.
 *   - A rebase and a change of mode leave D alone.
 *   - Escape with r2 (the plain double both modes produce):  zl = sqrt(r2);  dl = sqrt(D.x D.x + D.y D.y) on the MANTISSAS;
 *     de = ldexp((zl * log(zl)) / dl, -D.e), a NaN quotient becoming 0 first;  deriv = (ldexp(D.x, D.e), ldexp(D.y, D.e)),
 *     which saturates to +-inf or 0 outside a double's range -- de does not, being formed from the mantissas.
 *   - Interior samples: de = 0, deriv = (0, 0).
 * Scaling by a power of two is exact, so on a view both entry points accept -- the zoom a double's decimal string -- iter,
 * r2, de and deriv without BLA are bit for bit fr_render_deep_de's while no intermediate of either leaves a double's range.
 * D never feeds back: iter, nu, rgba without shading and the three step counts are fr_render_deepx's byte for byte.
 *
 * Shading and planes: as fr_render_deep_de.  Shared state: the extended orbit slot, the extended BLA table with its key and
 * fr_ctx_last_deepx_steps are fr_render_deepx's own -- a call here after fr_render_deepx of the same view computes no orbit
 * and builds no table, and the reverse.
 * Validation: everything fr_render_deepx checks; every BLA flag but FR_FLAG_DEEPX_BLA is FR_ERR_UNSUPPORTED (the two of the
 * Burning Ship included, which fr_render_deepx does not read); `de` NULL, shade outside {0, 1}, or shade == 1 with edge_px not
 * finite or <= 0 is FR_ERR_INVALID_ARG; of the five planes at least one must be given.
 * Cost: five live VGPRs; per single step a complex product, an alignment and a norm on top of the step (README: measured).
 * Neither kernel uses scratch or spills a VGPR.  Like every deep kernel they sit at the cap of 106 SGPRs and park scalar kernel
 * arguments in VGPR lanes: 84 and 87 of them (76 and 78 in fr_render_deepx's kernels; the distance block adds nine scalars),
 * written once in the prologue and read back per sample around the orbit loop, never inside it (checked on the ISA by
 * tests/test_deepx_de_host.py).
 * Julia sets are fr_render_deepx_julia_de (below, FR_HAS_DEEPX_JULIA_DE), the Burning Ship is fr_render_deepx_ship_de
 * (FR_HAS_DEEPX_SHIP_DE).
 * Out of scope: fr_deep_sequence, fr_node and .franim, slope or normal lighting. */
#define FR_HAS_DEEPX_DE 1

/* What fr_render_deepx_de checks of its arguments, the view's strings parsed included (no context needed). */
int fr_deepx_de_validate(const fr_params* p, const fr_deepx_view* view, const fr_deep_de* de, uint32_t width, uint32_t height);

/* fr_render_deepx with the distance planes; options, timing and the orbit cache as there. */
int fr_render_deepx_de(fr_ctx* ctx, const fr_params* p, const fr_deepx_view* view, const fr_deep_de* de, uint32_t width,
                       uint32_t height, const fr_shard* shard, const fr_output* out);

/* Asynchronous form: fr_render_deepx_async's contract, de->de and de->deriv device planes like the others. */
int fr_render_deepx_de_async(fr_ctx* ctx, const fr_params* p, const fr_deepx_view* view, const fr_deep_de* de, uint32_t width,
                             uint32_t height, const fr_shard* shard, const fr_output* out, void* hip_stream);

/* ---- deep zoom sequences: one centre, one orbit, frame after frame ---------------------------------------------------------
 * A zoom into one centre as an object: the zoom walked in log space over the whole range of fr_render_deepx, every frame
 * and keyframe rendered around ONE reference orbit, and -- in mode 1 -- only one keyframe per octave rendered exactly, the
 * frames in between resampled on the device from the two neighbouring keyframes.  Nothing about fr_render_deepx changes.
 *
 * Zoom of frame f.  (zm0, ze0), (zm1, ze1) = the fr_deepx_zoom pairs of zoom_first and zoom_last;
 *   D = (double)(ze1 - ze0) + (log2(zm1) - log2(zm0)), each operation one fp64 rounding, log2 and exp2 the host's libm.
 *   Frame 0 has the first pair exactly (L = 0), frame frames-1 the last pair exactly (L = D).  Any other frame:
 *   L = (D * f) / (frames - 1), q = floor(L), r = L - q, m = zm0 * exp2(r); if m >= 2 then m = m / 2, q = q + 1; the pair is
 *   (m, ze0 + q).  Two equal mantissas make D an exact integer, and every frame with integral L lies exactly on
 *   zoom_first 2^L: its decimal string exists and fr_render_deepx renders the same view.
 *   s = -L, k = floor(s) (fr_deep_sequence_frame.keyframe).  The frame is on the keyframe grid iff s == k; then u = 1, else
 *   u = exp2(-(s - k)), in (0.5, 1): the frame's height over keyframe k's.  Keyframe j is the view at (zm0, ze0 - j), for a
 *   zoom-out sequence too, where j goes negative.
 * F and the orbit.  frac_bits = 0: F = fr_deepx_frac_bits' rule applied to HALF the smaller of the two zooms (the pair
 *   (zm, ze - 1) of the smaller), in both modes; else F = frac_bits as for fr_deepx_view.  Every frame and keyframe of a
 *   sequence is an extended view with this one F, p's max_iterations and bailout: they all hit the context's extended-orbit
 *   cache under one key, and the orbit is computed once (until another fr_render_deepx view on the context displaces it).
 * Validation.  p: fr_render_deepx's rules, FR_FLAG_DEEPX_BLA included -- every exact render honours the flag.  The zoom
 *   strings: fr_deepx_zoom's rules.  Centre strings and frac_bits as for fr_deepx_view.  frames < 2, a mode outside {0, 1}
 *   or reserved != 0: FR_ERR_INVALID_ARG.  Mode 1: every keyframe the plan needs (k of every frame, k + 1 of every frame
 *   off the grid) must lie in [1e-1000, 1e3], compared on the pair as there: FR_ERR_INVALID_ARG.  fr_deep_sequence_plan
 *   performs the descriptor's checks with no device (and no p); a frame outside [0, frames) is FR_ERR_INVALID_ARG.
 * Mode 0.  Frame f is fr_render_deepx's render at the planned pair: all three planes, FR_MEM_HOST / FR_MEM_DEVICE,
 *   FR_LAYOUT_PACKED whole frames.  A frame whose pair is that of a decimal string gets the bytes of fr_render_deepx with
 *   that string and frac_bits = F.
 * Mode 1.  A frame on the grid is its keyframe, rendered exactly: the bytes of mode 0, all three planes.  Any other frame
 *   (fr_deep_sequence_frame.resampled = 1) is resampled from keyframes k and k + 1, rgba only: asking for nu or iter is
 *   FR_ERR_UNSUPPORTED.  The sequence owns two device rgba planes that hold the two most recently needed keyframes, rendered
 *   with p's flags (with FR_FLAG_POST_CHAIN the resampled colour is post-chained colour), so a monotone walk over the
 *   frames renders each keyframe once.  (A last frame whose mantissa differs from zm0 while D still came out integral is
 *   rendered at its own pair and not kept as a keyframe.)  fr_ctx_last_kernel_ms after a sequence call is the device time of
 *   everything that call enqueued: the keyframes it had to render and the resampling.
 * Resampling, per pixel (x, y): coordinates fp64, colour fp32, every operation one rounding, no contraction.
 *   dx = x - 0.5 W, dy = y - 0.5 H, u2 = u + u;  qx = 0.5 W + dx*u2, qy = 0.5 H + dy*u2.
 *   If 0 <= qx <= W-1 and 0 <= qy <= H-1 read keyframe k + 1 at (qx, qy), else keyframe k at (0.5 W + dx*u, 0.5 H + dy*u).
 *   At the read point (sx, sy): x0 = floor(sx) clamped to [0, W-1], x1 = min(x0 + 1, W-1), wx = (float)(sx - x0),
 *   cx = 1.0f - wx; the same for y.  Per colour channel, v00 = (x0, y0), v01 = (x1, y0), v10 = (x0, y1), v11 = (x1, y1):
 *   top = v00*cx + v01*wx, bot = v10*cx + v11*wx, out = top*cy + bot*wy.  Alpha is 1.
 * Calls are synchronous, frames may be asked for in any order, and a sequence is used from one thread at a time, like its
 * context, which must outlive it.  W * H < 2^31.
 *
 * Burning Ship sequences are fr_deep_ship_sequence_create (below, FR_HAS_DEEP_SHIP_SEQUENCE).
 * Out of scope: a max_iterations that varies per frame (it would change the BLA table's N and the
 * colour scale between keyframes); shards, fr_node and .franim files; asynchronous forms; a moving centre. */
#define FR_HAS_DEEP_SEQUENCE 1

typedef struct fr_deep_sequence fr_deep_sequence;

typedef struct fr_deep_sequence_desc {
    const char* center_x;      /* as fr_deep_view */
    const char* center_y;
    const char* zoom_first;    /* view height of frame 0, fr_deepx_view's grammar and range */
    const char* zoom_last;     /* view height of frame frames-1 */
    int32_t     frames;        /* >= 2 */
    int32_t     frac_bits;     /* 0 = automatic (above), else as fr_deepx_view */
    int32_t     mode;          /* 0 = every frame rendered exactly; 1 = octave keyframes + resampling */
    int32_t     reserved;      /* must be 0 */
} fr_deep_sequence_desc;       /* 48 bytes on LP64 */

typedef struct fr_deep_sequence_frame {   /* what frame f is: host arithmetic only */
    double  zoom_mant;         /* in [1, 2) */
    int32_t zoom_exp2;
    int32_t frac_bits;         /* the sequence's F */
    int32_t keyframe;          /* k (above); may be negative */
    int32_t resampled;         /* 1: mode 1 and the frame is not a keyframe itself */
    double  u;                 /* 1.0 on a keyframe, else in (0.5, 1) */
} fr_deep_sequence_frame;      /* 32 bytes */

/* Frame `frame` of the sequence `desc` describes; no device is touched. */
int fr_deep_sequence_plan(const fr_deep_sequence_desc* desc, int32_t frame, fr_deep_sequence_frame* out);

/* A sequence of width x height frames on ctx.  p, the strings and desc are copied.  Mode 1 allocates its two keyframe
 * planes (32 width height bytes) here. */
int fr_deep_sequence_create(fr_ctx* ctx, const fr_params* p, const fr_deep_sequence_desc* desc, uint32_t width, uint32_t height,
                            fr_deep_sequence** out);
void fr_deep_sequence_destroy(fr_deep_sequence* seq);

/* Frame `frame` into out's planes (rules above); returns when they are written. */
int fr_deep_sequence_render(fr_deep_sequence* seq, int32_t frame, const fr_output* out);

/* The frame with FR_FLAG_POST_CHAIN forced, then fr_render_frame_png's tail: fp16 round, 8-bit export, flip, PNG.  (A
 * keyframe plane remembers the flag it was rendered with: a mode-1 sequence created without the flag that alternates between
 * this call and fr_deep_sequence_render renders its keyframes again at every change.) */
int fr_deep_sequence_render_png(fr_deep_sequence* seq, int32_t frame, const char* path);

/* out[0] exact renders enqueued (mode-0 frames and keyframes), out[1] frames produced by resampling, out[2] reference
 * orbits computed during this sequence's calls. */
int fr_deep_sequence_stats(const fr_deep_sequence* seq, uint64_t out[3]);

/* ---- Burning Ship views below 1e-290: the ship's step with extended-exponent deltas ------------------------------------------
 * fr_render_deep_ship for a view that a double cannot hold, as fr_render_deepx is for fr_render_deep.  Everything of the
 * fr_render_deepx section is reused unchanged: extended numbers, norm, (+), the -400 mode rule, FR_DEEPX_ZERO_EXP; the view
 * fr_deepx_view, fr_deepx_zoom, fr_deepx_frac_bits; the storage of an orbit point, (mx, my) 2^e plus the plain doubles P_n.
 *
 * Validation: fr_render_deep_ship's rules with the zoom taken from the view's string, 1e-1000 <= zoom <= 1e3; p->zoom and the
 * double centre are ignored.  FR_FLAG_DEEP_BLA, FR_FLAG_DEEPX_BLA and FR_FLAG_DEEP_SHIP_BLA are FR_ERR_UNSUPPORTED here, alone
 * or with this path's own flag: their tables belong to the other deep paths.  BLA for extended ship views is
 * FR_FLAG_DEEPX_SHIP_BLA (below, FR_HAS_DEEPX_SHIP_BLA).
 *
 * Orbit: the recurrence of fr_deep_ship_reference_orbit (points SIGNED) in the storage of fr_deepx_reference_orbit.  The
 * exponent of a point is shared by its two coordinates and belongs to the larger one: a coordinate more than 2^1074 below its
 * partner is stored as 0.
 *
 * dc: the ship's viewport map of fr_render_deep_ship -- uvx, uvy with the sx-outer sub-sample offsets -- then
 *   dc = norm(((uvx - 0.5) * zm) * aspect, (uvy - 0.5) * zm, ze),  aspect = (double)W / (double)H of the WHOLE frame;
 * dcp follows from dc as for fr_render_deepx.  dz = (0, 0, FR_DEEPX_ZERO_EXP), m = 0, mode = extended.
 *
 * EXTENDED step, Z_m = (X, Y, eZ) from the extended storage, dz = (a, b, ed) normalised.  The fold is taken IN THE DELTA'S
 * FRAME, the orbit coordinate brought to the delta's exponent:
 *   fold_x(X, eZ, a, ed):  Xs = ldexp(X, eZ - ed);  X2s = ldexp(X, eZ + 1 - ed);  w = Xs + a;  d = X2s + a;
 *                          X >= 0 ? (w >= 0 ? a : -d) : (w > 0 ? d : -a)             -- a mantissa at exponent ed
 *   f = (fold_x(X, eZ, a, ed), fold_x(Y, eZ, b, ed), ed)
 *   t = (|X|, |Y|, eZ + 1) (+) f;   p = (t.x f.x - t.y f.y, t.x f.y + t.y f.x, t.e + ed);   n = p (+) dc;   m += 1;
 *   z = Z_m (+) n
 * and then the escape test, the rebase rule, norm and the mode rule of fr_render_deepx's EXTENDED step, unchanged.  For an
 * orbit coordinate far above the delta the ldexp may give +-inf: w then has the sign of X, the fold returns +-a and the
 * infinite d is discarded by the select.  For one far below the delta it gives 0 or a subnormal: that coordinate is below
 * half an ulp of a.  (Aligning the fold to max(eZ + 1, ed) instead would be wrong: the orbit's exponent belongs to the larger
 * coordinate, and a centre on the real axis has Y = 0 beside X near 2 -- its flipped d = 2Y + b would underflow to nothing.)
 *
 * PLAIN step: fr_render_deep_ship's step, operation for operation, on P_m, P_{m+1} and dcp; the mode switches are those of
 * fr_render_deepx.
 *
 * On operands that a double holds the extended step performs the plain step's roundings (the exponents only carry the
 * scale), so a view whose dc is at least 2^-400 -- every zoom down to about 1e-117 -- leaves the extended mode on its first
 * step and gets the bytes of fr_render_deep_ship.
 *
 * Planes, colour stage, shards, layouts, memory kinds, options and fr_ctx_last_kernel_ms / _grid are those of
 * fr_render_deep_ship.  The context keeps the most recent extended ship orbit on the device in a slot of its own, keyed as
 * fr_render_deepx's: none of the four deep paths evicts another's orbit.
 *
 * Sequences (FR_HAS_DEEP_SHIP_SEQUENCE): fr_deep_ship_sequence_create makes a fr_deep_sequence whose exact renders are
 * fr_render_deepx_ship's; the descriptor, the walk, F, mode 1's keyframe planes and the resampling are fr_deep_sequence's,
 * and so are _plan, _render, _render_png, _stats and _destroy.  (At aa 1 the ship's map is ((x - 0.5 W) / H) zoom too, so the
 * resampling geometry holds.)  p follows fr_render_deepx_ship's rules: p->fractal_type must be FR_FRACTAL_BURNING_SHIP, and
 * fr_deep_sequence_create keeps rejecting it.
 *
 * Out of scope: fr_node and .franim; depths beyond 1e-1000; per-coordinate exponents in the orbit storage. */
#define FR_HAS_DEEPX_SHIP 1
#define FR_HAS_DEEP_SHIP_SEQUENCE 1
#define FR_HAS_DEEPX_SHIP_BLA 1   /* FR_FLAG_DEEPX_SHIP_BLA and fr_ctx_last_deepx_ship_steps (below fr_deep_ship_sequence_create) */

/* fr_deepx_reference_orbit for the ship's recurrence: same arguments, validation and cost */
int fr_deepx_ship_reference_orbit(const fr_deepx_view* v, int32_t max_iter, float bailout, double* out_mant_xy, int32_t* out_exp2,
                                  int32_t* out_len);

/* fr_render_deep_ship's contract (planes, memory kinds, FR_LAYOUT_FRAME, shards, options, the orbit cache) for an extended view */
int fr_render_deepx_ship(fr_ctx* ctx, const fr_params* p, const fr_deepx_view* view, uint32_t width, uint32_t height,
                         const fr_shard* shard, const fr_output* out);

/* fr_render_deep_async's contract: a render of a new view computes its orbit on the host first and is never launch-only */
int fr_render_deepx_ship_async(fr_ctx* ctx, const fr_params* p, const fr_deepx_view* view, uint32_t width, uint32_t height,
                               const fr_shard* shard, const fr_output* out, void* hip_stream);

/* fr_deep_sequence_create for a Burning Ship sequence (above); the object is used and destroyed as any fr_deep_sequence */
int fr_deep_ship_sequence_create(fr_ctx* ctx, const fr_params* p, const fr_deep_sequence_desc* desc, uint32_t width,
                                 uint32_t height, fr_deep_sequence** out);

/* Bilinear approximation for extended ship views, opt-in per call with FR_FLAG_DEEPX_SHIP_BLA in p->flags.  Only
 * fr_render_deepx_ship, fr_render_deepx_ship_async and fr_deep_ship_sequence_create (every exact render of the sequence) read
 * the flag; without it every byte they write is as above.  It is FR_FLAG_DEEP_SHIP_BLA's scheme -- the ship's real 2x2 maps
 * and fold-capped radii -- with the table and the BLA step carried in FR_FLAG_DEEPX_BLA's extended arithmetic, taken by samples
 * in either mode.  Everything of the fr_render_deepx / fr_render_deepx_ship sections is reused: extended numbers, norm, (+), the
 * -400 mode rule, FR_DEEPX_ZERO_EXP, normalised extended reals (v, e) and |w|.
 *
 * Extended 2x2 matrix: (m11, m12, m21, m22, e), four mantissas, row by row, and one shared int32 exponent.
 *   norm4(m11, m12, m21, m22, e):  k = frexp exponent of the largest |mij|;  (ldexp(mij, -k) ..., e + k), and
 *                                  e = FR_DEEPX_ZERO_EXP for the all-zero matrix.
 *   - Constants: eps = 2^-53.  dcmax is FR_FLAG_DEEP_SHIP_BLA's formula on the zoom pair: with a = (double)W / (double)H of the
 *     WHOLE frame (never of a shard's rows),
 *       hx = 0.5 + 0.5 / (W*W);  hy = 0.5 + 0.5 / (W*H);  ex = hx * a;
 *       dcmax = the extended real ((1.0000001 * zm) * sqrt(ex*ex + hy*hy), ze), normalised.
 *   - Single step at m >= 1 (never stored), Z_m = (X, Y, eZ) from the extended storage, sx = sgn(X), sy = sgn(Y):
 *       A = norm4(X, -Y, |Y| * sx, |X| * sy, eZ + 1)   (the doubling goes to the exponent, as for FR_FLAG_DEEPX_BLA),
 *       B = norm4(1, 0, 0, 1, 0),
 *       r = eps * |norm(Z_m)| as for FR_FLAG_DEEPX_BLA;  then the two fold conditions on extended reals,
 *       r = (r < |X| ? r : |X|);  r = (r < |Y| ? r : |Y|),   |X| = (|X|, eZ) and |Y| = (|Y|, eZ) normalised,
 *     compared on (exponent, mantissa) with zero below everything.  A coordinate stored as 0 gives r = 0, no BLA step from
 *     that point: the real axis, and a coordinate more than 2^1074 below its partner.
 *   - Table: levels, entry indexing, the existence rule and the entry count (N - 1) - popcount(N - 1) of FR_FLAG_DEEP_BLA.
 *     Merging x then y:
 *       A = norm4(A_y A_x): each element p*q + s*t on mantissas as FR_FLAG_DEEP_SHIP_BLA writes them, exponent A_y.e + A_x.e;
 *       B = norm4((A_y B_x) (+) B_y): the product (p*q + s*t per element) at exponent A_y.e + B_x.e; (+) aligns both
 *         four-tuples to the larger exponent with ldexp and adds once per element;
 *       |A_x| = (sqrt(a11*a11 + a21*a21), A_x.e), normalised: the first column (A_x is a scaled orthogonal matrix);
 *       |B_x| = (sqrt((b11*b11 + b12*b12) + (b21*b21 + b22*b22)), B_x.e), normalised;
 *       t, r, the r < r_x rule, the void rule (an exponent of A or B outside [-2^27, 2^27] zeroes r, A and B) and the 24-bit
 *       cut of the STORED radius (a float and an int32) are FR_FLAG_DEEPX_BLA's.
 *   - Stepping: FR_FLAG_DEEPX_BLA's level choice and probe; samples in either mode take steps, a PLAIN sample probing
 *     norm(dz.x, dz.y, 0).  A BLA step is always extended, on that dz and the extended dc:
 *       n = (A dz) (+) (B dc),  A dz = (a11 dz.x + a12 dz.y, a21 dz.x + a22 dz.y, A.e + dz.e),  B dc likewise at B.e + dc.e;
 *       m += 2^k;   u += 2^k;   z = Z_m (+) n;
 *     then the escape test (escaped at u - 1), the rebase rule, norm and the mode rule of the EXTENDED step, unchanged.  If no
 *     level qualifies, or m == 0, the sample takes the step of its mode from fr_render_deepx_ship, operation for operation.
 * Escapes between the first and the last update of a BLA step are not looked for.
 *
 * What it skips (the numpy restatement, 128 x 96, aa 1): on a structured view at 1e-400 (N = 2766) 94.7 % of the updates, 18.0x
 * fewer loop trips, iter equal to the unflagged path's on 12279 of 12288 pixels; at 1e-310 (N = 2173) 93.2 %, 13.9x, 12241 of
 * 12288; on a view inside a period-546 nucleus 99.5 %, every iter equal.  A centre on the real axis takes no BLA step.
 * Measured on one MI355X at 4096^2 (profiles/deepx_ship_bla_time.txt, flagged and unflagged interleaved in one session): 9.94 ms
 * against 126.1 ms on the first view (12.7x), 10.6 ms against 97.1 ms on the second (9.1x); a flagged loop trip costs about 1.4
 * unflagged ones (the pre-filter and the level probe, the 72-byte gather, 3 waves per SIMD for 4).  Where no step can qualify
 * the probe is all the flag adds: the tip (-2, 0) at 1e-1000 takes 153.6 ms flagged against 84.4 ms.  The flag is opt-in.
 *
 * Cost: 80 bytes per entry (r 8, the eight mantissas 64, the two exponents 8), on the device, per context, in buffers of this
 * path's own, keyed by the extended ship orbit and the bits of dcmax (mantissa and exponent), grown like the orbit buffer.  A
 * zoom change at a fixed centre rebuilds it (K small launches on the render's stream); a cached view is launch-only.
 * Rebuilds, and the upload of a new extended ship orbit, are ordered behind the context's previous render with the flag,
 * whatever stream it went to.  The tables and counts of the other three BLA paths are untouched, and the reverse. */

/* fr_ctx_last_deepx_steps' contract for the context's most recent fr_render_deepx_ship(_async) call or ship-sequence render
 * made with FR_FLAG_DEEPX_SHIP_BLA: out[0] single steps (plain and extended), out[1] BLA steps, out[2] updates skipped.
 * FR_ERR_UNSUPPORTED if there is no such call.  The other three counts do not report these calls. */
int fr_ctx_last_deepx_ship_steps(fr_ctx* ctx, uint64_t out[3]);

/* ---- Julia set views deeper than double precision: perturbation around two reference orbits -----------------------------------
 * fr_render with FR_FRACTAL_JULIA holds its centre as a double: below a zoom of about 1e-13 neighbouring pixels collapse onto
 * one z_0.  fr_render_deep_julia takes the centre as decimal strings (fr_deep_view, p->zoom in [1e-290, 1e3]),
 * fr_render_deepx_julia the zoom as a string too (fr_deepx_view, 1e-1000 .. 1e3).  c = (p->julia_c_real, p->julia_c_imag),
 * both doubles.  p->center_x, p->center_y and, in the extended form, p->zoom are ignored.
 *
 * A Julia view does not fit the loops above as they stand: its reference orbit starts at the view's centre, not at 0; there is
 * no dc term (c is the same for every sample, the sample's offset is its first delta); and the rebase "dz = z, m = 0" is only
 * valid on an orbit whose first point is 0.  Hence TWO orbits, both on the host in fr_render_deep's fixed point (the same F
 * rules, floor shifts and escape test "|Z_n|^2 > bailout^2, compared exactly, tested before the update"), with the
 * recurrence of Mandelbrot's orbit; c enters the fixed point as the exact value of its doubles, rounded to nearest-even only
 * where F is too small to hold it:
 *   P (primary):   P_0 = the centre, P_{n+1} = P_n^2 + c, stored P_0 .. P_{N_P}
 *   Q (critical):  Q_0 = 0,          Q_{n+1} = Q_n^2 + c, stored Q_0 .. Q_{N_Q}: fr_deep_reference_orbit's orbit at C = c, so
 *                  Q_1 = c and N_Q >= 1
 * A centre with |P_0|^2 > bailout^2 (exact compare) is FR_ERR_INVALID_ARG; hence N_P >= 1.  A sample starts on P and moves to
 * Q at its first rebase, for good; that rebase is exact because Q_0 = 0, which is the whole no-glitch argument of
 * fr_render_deep, unchanged.
 *
 * Per sample, fp64 deltas (fr_render_deep_julia): d0 = fr_render_deep_ship's dc of the pixel and sub-sample -- Julia's viewport
 * map less the centre (shaders/julia.comp:221-225, :253-264; sx OUTER, aspect of the WHOLE frame; the shader text is the
 * ship's).  dz = d0, on P, m = 0; then for i = 0 .. max_iter-1, Z the sample's current orbit and N its last index:
 *   t = (Z_m + Z_m) + dz;  dz' = (t.x dz.x - t.y dz.y, t.x dz.y + t.y dz.x);  m += 1;  z = Z_m + dz';  r2 = |z|^2
 *   r2 > bailout^2: escaped at i;  else if r2 < |dz'|^2 or m == N: dz = z, m = 0, the orbit becomes Q (rebase);  else dz = dz'
 * each operation one fp64 rounding as written (no contraction), and no dc term.
 *
 * Extended deltas (fr_render_deepx_julia): fr_render_deepx's arithmetic, orbit storage (both orbits) and -400 mode rule,
 * operation for operation, with these differences.  The first delta is dz = norm(d0's mantissas, ze) -- fr_render_deepx_ship's
 * dc -- and the mode rule applies to it at once: a sample with dz.e > -400 starts PLAIN with (ldexp(dz.x, dz.e),
 * ldexp(dz.y, dz.e)).  There is no (+) dc: n = p.  Rebasing follows the two-orbit rule.  FLUSH: without a dc term a delta in a
 * superattracting basin (c = -1, c = 0, ...) squares itself towards nothing, and its int32 exponent would run away; so after
 * every norm of dz a result with e < -2^27 becomes the zero (0, 0, FR_DEEPX_ZERO_EXP), and every exponent sum of a step stays
 * above -2^29.  Such a delta is below 2^(-2^27) of the orbit it follows and cannot change any z.  On operands that a double
 * holds the extended step does the plain step's roundings, so a view whose d0 is at least 2^-400 gets the bytes of
 * fr_render_deep_julia.
 *
 * Planes: those of fr_render's fp64 Julia path for the same (i, r2): nu (double) = i + 1 - log2(log2(r2) / log2(bailout)) of
 * sample s = 0 (the as-written library-log form at bailout <= 1; max_iterations for interior), iter = its i,
 * t = color_offset + nu / max_iter * color_scale, interior black, the aa average in the shader's order, FR_FLAG_POST_CHAIN
 * with the Julia floors.  Julia has no trap, stripe or interior styles: those fields are ignored, as fr_render ignores them.
 *
 * Validation (fr_deep_julia_validate, fr_deepx_julia_validate: no device needed): FR_ERR_UNSUPPORTED if p->fractal_type is not
 * FR_FRACTAL_JULIA, p->precision not FR_PRECISION_F64, or with any of the four BLA flags of the other formulas or with the
 * other Julia entry point's flag (FR_FLAG_DEEPX_JULIA_BLA in fr_render_deep_julia, FR_FLAG_DEEP_JULIA_BLA in
 * fr_render_deepx_julia); FR_ERR_INVALID_ARG for c not finite or a component of |c| >= 2^32, bailout > 2^16, the centre rule
 * above, and otherwise as fr_render_deep_ship / fr_render_deepx_ship.  The other deep entry points keep rejecting
 * FR_FRACTAL_JULIA, and answer FR_ERR_UNSUPPORTED for the two Julia BLA flags (fr_render_deep, fr_render_deepx,
 * fr_render_deep_ship, fr_render_deepx_ship and the two sequence creators).
 *
 * Argument shape, shards, FR_LAYOUT_FRAME, memory kinds, options, fr_ctx_last_kernel_ms / _grid and the asynchronous rules are
 * fr_render_deep_ship's and fr_render_deepx_ship's; a render of a new view computes its orbits on the host first and is
 * never launch-only.  The context keeps the most recent pair of orbits of each of the two paths in slots of their own, keyed
 * by (centre strings, F, max_iterations, bailout, the bits of c): none of the six deep paths evicts another's orbit.
 *
 * Measured on one MI355X at 4096^2 (profiles/deep_julia_time.txt, the cases interleaved in one session, device time): RABBIT30
 * (1e-30, max_iter 1100) 17.58 ms and DENDRITE100 (1e-100, 1200) 12.31 ms through fr_render_deep_julia, 946 and 970 G
 * lane-updates/s, next to fr_render_deep's 16.54 ms (830 G/s) on its 1e-100 view; the dendrite at 1e-400 (3000) 95.6 ms through
 * fr_render_deepx_julia, 496 G/s, next to fr_render_deepx's 111.9 ms (487 G/s) on its 1e-400 view.
 *
 * Out of scope: Julia zoom sequences; fr_node and .franim; c as a decimal string. */
#define FR_HAS_DEEP_JULIA 1
#define FR_HAS_DEEPX_JULIA 1
#define FR_HAS_DEEP_JULIA_BLA 1   /* FR_FLAG_DEEP_JULIA_BLA and fr_ctx_last_deep_julia_steps (below the render entry points) */
#define FR_HAS_DEEPX_JULIA_BLA 1  /* FR_FLAG_DEEPX_JULIA_BLA and fr_ctx_last_deepx_julia_steps */

/* Both orbits as doubles, on the host: out_p_xy and out_q_xy receive 2 (max_iter + 1) doubles each at most;
 * *out_p_len = N_P + 1, *out_q_len = N_Q + 1.  Validation and cost as two fr_deep_reference_orbit calls. */
int fr_deep_julia_reference_orbits(const fr_deep_view* v, double c_re, double c_im, double zoom, int32_t max_iter, float bailout,
                                   double* out_p_xy, int32_t* out_p_len, double* out_q_xy, int32_t* out_q_len);

/* Both orbits in the extended storage of fr_deepx_reference_orbit */
int fr_deepx_julia_reference_orbits(const fr_deepx_view* v, double c_re, double c_im, int32_t max_iter, float bailout,
                                    double* out_p_mant_xy, int32_t* out_p_exp2, int32_t* out_p_len, double* out_q_mant_xy,
                                    int32_t* out_q_exp2, int32_t* out_q_len);

int fr_deep_julia_validate(const fr_params* p, const fr_deep_view* view, uint32_t width, uint32_t height);
int fr_deepx_julia_validate(const fr_params* p, const fr_deepx_view* view, uint32_t width, uint32_t height);

int fr_render_deep_julia(fr_ctx* ctx, const fr_params* p, const fr_deep_view* view, uint32_t width, uint32_t height,
                         const fr_shard* shard, const fr_output* out);
int fr_render_deep_julia_async(fr_ctx* ctx, const fr_params* p, const fr_deep_view* view, uint32_t width, uint32_t height,
                               const fr_shard* shard, const fr_output* out, void* hip_stream);
int fr_render_deepx_julia(fr_ctx* ctx, const fr_params* p, const fr_deepx_view* view, uint32_t width, uint32_t height,
                          const fr_shard* shard, const fr_output* out);
int fr_render_deepx_julia_async(fr_ctx* ctx, const fr_params* p, const fr_deepx_view* view, uint32_t width, uint32_t height,
                                const fr_shard* shard, const fr_output* out, void* hip_stream);

/* Bilinear approximation for Julia views, opt-in per call: FR_FLAG_DEEP_JULIA_BLA is read by fr_render_deep_julia(_async) only,
 * FR_FLAG_DEEPX_JULIA_BLA by fr_render_deepx_julia(_async) only; without its flag every byte an entry point writes is as above.
 * It is FR_FLAG_DEEP_BLA's scheme with B = 0: a Julia step has no dc term, so a step over 2^k updates is ONE complex product
 * dz' = A dz, the table holds no B, and no dcmax enters a radius -- the tables do not depend on the frame.
 *
 * Notation and rounding are FR_FLAG_DEEP_BLA's: one fp64 rounding per operation, no contraction, |w| = sqrt(w.x*w.x + w.y*w.y)
 * with sqrt correctly rounded.  eps = 2^-53.
 *   - Single step at m >= 1 on an orbit Z (never stored): A = Z_m + Z_m, r = eps * |Z_m|.
 *   - Tables: TWO, one over Q_1 .. Q_{N_Q - 1} and one over P_1 .. P_{N_P - 1}, each with FR_FLAG_DEEP_BLA's levels
 *     (K = floor(log2(N - 1)); N <= 2: no table for that orbit), entry coverage, existence rule and entry count
 *     E(N) = (N - 1) - popcount(N - 1).  Either table may be absent while the other exists.  They live in one set of buffers,
 *     Q's entries first: entries [0, E(N_Q)) are Q's table level after level, [E(N_Q), E(N_Q) + E(N_P)) are P's.  An fp64 entry
 *     is 24 bytes (r 8, A 16), an extended one 28 (the radius 8, A's mantissas 16, A.e 4).
 *   - Merge (fp64), x then y:  A = A_y*A_x,  t = r_y / |A_x|,  r = (t > 0 ? t : 0) (NaN: 0),  r = (r < r_x ? r : r_x),  and
 *     r = 0 if A is not finite.  This is FR_FLAG_DEEP_BLA's merge with B = 0.
 *   - Extended tables: FR_FLAG_DEEPX_BLA's arithmetic with the B terms removed.  Single step: A = norm(Z_m.x, Z_m.y, Z_m.e + 1),
 *     r = eps * |norm(Z_m)|.  Merge: A = norm(A_y (x) A_x) with the exponent A_y.e + A_x.e;  t = r_y (/) |A_x| (one division of
 *     the mantissas, exponent r_y.e - |A_x|.e), r = norm(t) if t's mantissa is > 0 and finite, else the zero;  then r = r_x
 *     unless r < r_x on (exponent, mantissa).  An entry whose A.e leaves [-2^27, 2^27] is void (r and A stored as zero), and the
 *     STORED radius is cut to 24 bits, as there.
 *   - Stepping: FR_FLAG_DEEP_BLA's on the sample's CURRENT orbit Z with its N and that orbit's table.  At m >= 1 take the
 *     largest k >= 1 with (m-1) mod 2^k == 0, m + 2^k <= N, u + 2^k <= max_iterations and |dz|^2 < r*r; then
 *       dz' = (A.x dz.x - A.y dz.y, A.x dz.y + A.y dz.x),  m += 2^k,  u += 2^k,  z = Z_m + dz',  r2 = |z|^2;
 *     r2 > bailout^2: escaped at u - 1; otherwise the two-orbit rebase rule of the plain Julia step (r2 < |dz'|^2 or m == N:
 *     dz = z, m = 0, and the orbit -- with it the table -- becomes Q's for good).  A sample starts on P with dz = d0, m = 0 and
 *     takes the plain step there: at m = 0 no BLA is tried, on either orbit.  If no k qualifies the plain step runs unchanged.
 *   - Extended stepping: a sample in either mode probes on its dz as a normalised extended number (FR_FLAG_DEEPX_BLA's probe); the
 *     BLA step is dz' = norm(A.mant (x) dz.mant, A.e + dz.e), then the FLUSH (e < -2^27 gives the zero), then the -400 mode
 *     rule, escape and rebase as above.  Every exponent sum stays above -2^29, as without the flag.
 * Where it differs from the plain step: as FR_FLAG_DEEP_BLA -- a single step drops dz^2 only where it is below one rounding of
 * the kept term, merged steps differ by rounding order, and escapes inside a BLA step are not looked for.
 *
 * Cost: E(N_Q) + E(N_P) entries on the device, per context and path, grown like the orbit buffers; the two paths' tables are
 * slots of their own and neither evicts another path's orbit or table.  The tables are keyed by the orbit slot alone: a new c, a
 * new centre, F, max_iterations or bailout recomputes the orbits and then the tables (K_Q + K_P small launches on the render's
 * stream, ordered behind the slot's previous render with the flag, whatever stream that went to); a zoom change at the same
 * key rebuilds nothing and is launch-only.
 *
 * Measured on one MI355X at 4096^2 (profiles/deep_julia_bla_time.txt, flagged and unflagged interleaved in one session, device
 * time): the dendrite at 1e-400 96.36 -> 5.49 ms (17.6x, 95.8 % of the updates skipped), DENDRITE100 12.40 -> 4.30 ms (2.88x),
 * RABBIT30 17.89 -> 14.46 ms (1.24x: its interior samples leave the linear phase early), a view at 1e-60 centred on a preimage
 * of 0, whose samples step on both tables, 5.52 -> 2.36 ms in fp64 deltas and 7.93 -> 2.94 ms in extended ones; every pixel of
 * these frames has the unflagged iter.  Where nothing qualifies the flag costs: c = 0 (every radius over a zero is 0) runs at
 * 0.53x (fp64) and 0.69x (extended) of the unflagged kernels. */

/* fr_ctx_last_deep_steps' contract for the context's most recent fr_render_deep_julia(_async) call made with
 * FR_FLAG_DEEP_JULIA_BLA, and for the most recent fr_render_deepx_julia(_async) call made with FR_FLAG_DEEPX_JULIA_BLA:
 * out[0] single steps, out[1] BLA steps, out[2] updates skipped, over every sub-sample of the in-frame pixels, both orbits
 * counted together.  FR_ERR_UNSUPPORTED if there is no such call. */
int fr_ctx_last_deep_julia_steps(fr_ctx* ctx, uint64_t out[3]);
int fr_ctx_last_deepx_julia_steps(fr_ctx* ctx, uint64_t out[3]);

/* The tables as the device holds them, copied to the host after a device synchronise: the first n entries, Q's table first, then
 * P's (a caller splits them with E(N_Q), then E(N_P), the lengths from fr_deep_julia_reference_orbits /
 * fr_deepx_julia_reference_orbits; inside a table level k starts E(N) - E(((N - 1) >> (k - 1)) + 1) entries in).  r: n doubles, or
 * n 8-byte radii (the mantissa as a float, the int32 exponent); a: 2 n doubles (A.x, A.y; extended: the mantissas); a_exp: n
 * int32.  NULL skips a part.  Returns the number of entries the context holds (0: no table, or the orbits have changed since). */
int64_t fr_deep_julia_bla_table(fr_ctx* ctx, double* r, double* a, int64_t n);
int64_t fr_deepx_julia_bla_table(fr_ctx* ctx, void* r, double* a, int32_t* a_exp, int64_t n);

/* ---- distance estimates for deep Julia views ------------------------------------------------------------------------------------
 * fr_render_deep_de and fr_render_deepx_de (above) for the views of fr_render_deep_julia and fr_render_deepx_julia: the same two
 * planes more, the exterior distance estimate of sample (0,0) in pixel spacings and the scaled derivative.  Dust and dendrite Julia
 * sets have no interior; at depth their filaments are far thinner than a pixel (48x36 frames of the tests: 63 % of the escaped
 * pixels of DUST30 and 49 % of RABBIT30 lie less than one pixel spacing from the set) and the smooth count of a frame is noise.
 * The distance block is fr_deep_de with fr_deep_de_default, unchanged.  Range, view, c, orbits (P and Q), tables, rebasing and
 * flags are exactly the plain Julia entry points': FR_FLAG_DEEP_JULIA_BLA is read by fr_render_deep_julia_de,
 * FR_FLAG_DEEPX_JULIA_BLA by fr_render_deepx_julia_de.  Every other entry point is untouched.
 *
 * D is dz_n/dz_0 * s: the derivative of the sample's point with respect to ITS OWN starting point (Julia's parameter is the
 * start, c is fixed), times one pixel spacing s, so that |D| at escape is about 1 / de with de in pixel spacings.  The map is
 * analytic and has no dc term: an update is one complex product, D' = 2 z D, and nothing is ever added.  Every operation is one
 * fp64 rounding or an exact scaling, no contraction.
 *
 * fp64 (fr_render_deep_julia_de), next to fr_render_deep_julia's step:
 *   - s = zoom / H, H the height of the WHOLE frame.  D = (s, +0.0) at the start (fr_render_deep_de starts at (0, 0): there the
 *     parameter is c, here it is z_0, and dz_0/dz_0 = 1).
 *   - Plain step, formed in every trip from the point before the update on the sample's CURRENT orbit (P at first):
 *       z = Z_m + dz;   w = z + z;   D' = (w.x D.x - w.y D.y,  w.x D.y + w.y D.x)
 *     -- nothing is added: adding 0.0 would change the sign of a zero.
 *   - BLA step with the entry A the sample takes: D' = (A.x D.x - A.y D.y,  A.x D.y + A.y D.x).
 *   - A rebase, the move from P to Q included, leaves D alone: the point does not move.
 *   - Escape with r2: fr_render_deep_de's, zl = sqrt(r2); dl = sqrt(D.x D.x + D.y D.y); de = (zl * log(zl)) / dl; a NaN de becomes
 *     0; an overflowing |D| gives 0 by the division; a ZERO D gives +inf (see the underflow note).
 *   - Interior samples (iter == max_iterations): de = 0, deriv = (0, 0).
 *
 * Extended (fr_render_deepx_julia_de): D is fr_render_deepx_de's extended complex number (D.x, D.y, D.e), normalised after every
 * update whatever mode the sample's delta is in; notation as there.
 *   - s = (sm, es) = norm1(zm / (double)H, ze).  D = (sm, +0.0, es) at the start.
 *   - EXTENDED single step:  eb = max(Z_m.e, dz.e);   b = ldexp(Z_m, Z_m.e - eb) + ldexp(dz, dz.e - eb), per component;
 *       P = (b.x D.x - b.y D.y,  b.x D.y + b.y D.x) at eP = eb + 1 + D.e;   D' = norm(P.x, P.y, eP)
 *   - PLAIN single step:  w = (Z_m + dz) + (Z_m + dz) on the plain doubles;   P = w (x) D at eP = D.e;   D' = norm(P)
 *   - BLA step with the entry A:  P = A (x) D at eP = A.e + D.e;   D' = norm(P)
 *   - FLUSH of D: after every norm a D with e < -2^27 becomes the zero (0, 0, FR_DEEPX_ZERO_EXP) and stays zero (a product with
 *     the zero is the zero).  In a superattracting basin (c = 0, c = -1) |2 z| squares itself towards nothing and an int32
 *     exponent would wrap after about 30 updates.  The other way: |D| <= s (2 bailout + 1)^n with bailout <= 2^16, so D.e stays
 *     below 18 * 2^24 < 2^29 for every max_iterations the validator accepts.  With both bounds every exponent sum of a step stays
 *     inside (-2^29, 2^29).
 *   - A change of mode and a rebase leave D alone.
 *   - Escape: fr_render_deepx_de's -- de = ldexp(q, -D.e), q = (zl * log(zl)) / dl formed from the mantissas (a NaN quotient
 *     becoming 0 first);  deriv = (ldexp(D.x, D.e), ldexp(D.y, D.e)), which saturates outside a double's range.  A zero D
 *     gives de = +inf and deriv = (0, 0).
 *   - Interior samples: de = 0, deriv = (0, 0).
 *
 * D never feeds back: iter, nu, rgba without shading and the three step counts (fr_ctx_last_deep_julia_steps,
 * fr_ctx_last_deepx_julia_steps, which report these calls too) are the plain Julia entry point's, byte for byte.
 * Scaling by a power of two is exact, so on a view both entry points accept whose d0 is at least 2^-400, de and deriv of the two
 * unflagged entry points are bit-identical while no intermediate leaves a double's range.
 *
 * Underflow, documented and not worked around: the fp64 D starts near zoom / H and can leave a double's range only downwards,
 * where an orbit passes close to 0 at great depth (a centre on a depth-12 preimage of 0 at 1e-290: D is exactly 0 on every
 * pixel of a 48x36 frame, and de = +inf).  The fp64 deltas of fr_render_deep_julia underflow on the same view and every iter
 * already differs from the exact one: the limit of the fp64 derivative is the limit the fp64 path already has.  Such views
 * belong to fr_render_deepx_julia_de.
 *
 * Accuracy: below de of about 1e-3 pixel spacings the relative error of any fp64 iteration grows like 2^-53 / de -- the orbit
 * hugs the set for many updates after its delta has reached the size of z.  Above it the tests bound the error against the
 * derivative iterated directly at F + 64 bits (README: measured).
 *
 * Shading (shade == 1): fr_render_deep_de's, on every escaped sub-sample before the aa average and the post chain.
 * Planes: de->de and de->deriv follow out->memory and out->layout as out->nu does; of the five planes rgba, nu, iter, de, deriv at
 * least one must be given.  Shards and FR_LAYOUT_FRAME as fr_render_deep_de.
 * Shared state: the orbit slots, the tables with their keys and the step counts are the plain Julia paths' own -- a call here
 * after fr_render_deep_julia / fr_render_deepx_julia of the same view computes no orbit and builds no table, and the reverse.
 * Validation: everything fr_deep_julia_validate / fr_deepx_julia_validate checks; then `de` NULL, shade outside {0, 1}, or
 * shade == 1 with edge_px not finite or <= 0 is FR_ERR_INVALID_ARG.
 * Cost: four live VGPRs (five extended) and per plain update 10 fp64 operations on top of the step's 16.  The four kernels use
 * no scratch and spill no VGPR; the fp64 pair keeps the occupancy of the kernels it extends (5 and 4 waves per SIMD), the
 * extended pair runs a wave per SIMD below them (4 and 3).  Measured on one MI355X at 4096^2 (profiles/deep_julia_de_time.txt,
 * interleaved with the plain entry points in one session, device time), without / with the BLA flag: 1.26 / 1.14 of
 * fr_render_deep_julia on RABBIT30 and on DENDRITE100, 1.33 / 1.38 of fr_render_deepx_julia on the dendrite at 1e-400; in the
 * same session fr_render_deep_de costs 1.30 / 1.18 of fr_render_deep and fr_render_deepx_de 1.36 / 1.39 of fr_render_deepx.
 * The Burning Ship, with a real 2x2 Jacobian and a fixed norm, is fr_render_deep_ship_de / fr_render_deepx_ship_de (below).
 * Out of scope: sequences, fr_node and .franim, c as a decimal string, slope or normal lighting -- deriv is what a caller needs
 * for it. */
#define FR_HAS_DEEP_JULIA_DE 1
#define FR_HAS_DEEPX_JULIA_DE 1

/* What the two entry points check of their arguments, the view's strings parsed included (no context needed). */
int fr_deep_julia_de_validate(const fr_params* p, const fr_deep_view* view, const fr_deep_de* de, uint32_t width, uint32_t height);
int fr_deepx_julia_de_validate(const fr_params* p, const fr_deepx_view* view, const fr_deep_de* de, uint32_t width,
                               uint32_t height);

/* fr_render_deep_julia / fr_render_deepx_julia with the distance planes; options, timing and the orbit cache as there.  The
 * asynchronous forms: fr_render_deep_julia_async's contract, de->de and de->deriv device planes like the others. */
int fr_render_deep_julia_de(fr_ctx* ctx, const fr_params* p, const fr_deep_view* view, const fr_deep_de* de, uint32_t width,
                            uint32_t height, const fr_shard* shard, const fr_output* out);
int fr_render_deep_julia_de_async(fr_ctx* ctx, const fr_params* p, const fr_deep_view* view, const fr_deep_de* de, uint32_t width,
                                  uint32_t height, const fr_shard* shard, const fr_output* out, void* hip_stream);
int fr_render_deepx_julia_de(fr_ctx* ctx, const fr_params* p, const fr_deepx_view* view, const fr_deep_de* de, uint32_t width,
                             uint32_t height, const fr_shard* shard, const fr_output* out);
int fr_render_deepx_julia_de_async(fr_ctx* ctx, const fr_params* p, const fr_deepx_view* view, const fr_deep_de* de, uint32_t width,
                                   uint32_t height, const fr_shard* shard, const fr_output* out, void* hip_stream);

/* ---- distance estimates for deep Burning Ship views ----------------------------------------------------------------------
 * fr_render_deep_ship_de (zoom 1e-290 .. 1e3, plain or FR_FLAG_DEEP_SHIP_BLA) and fr_render_deepx_ship_de (zoom 1e-1000 .. 1e3,
 * plain or FR_FLAG_DEEPX_SHIP_BLA): fr_render_deep_ship / fr_render_deepx_ship with fr_render_deep_de's two planes and shading.
 * The ship's map is not conformal, so the derivative of z with respect to c is a real 2x2 matrix
 *   J = [[dx/dcx, dx/dcy], [dy/dcx, dy/dcy]] * s,   s = zoom / H of the whole frame (never of a shard's rows),
 * the zero matrix at the start, and the estimate takes the gradient of |z|: de = |z| log|z| / |J^T z / |z||.  For a conformal
 * J = [[Dx, -Dy], [Dy, Dx]] that norm is |D| and the estimate is fr_render_deep_de's.
 * fr_deep_de is reused unchanged with one difference: deriv is rows*W*4 doubles, (J11, J12, J21, J22) of sample (0,0) at its
 * escaping update, zeros for interior pixels.  de, shade and edge_px are as in fr_render_deep_de.
 *
 * The arithmetic, fp64 range; every operation is one rounding as written, no contraction.  sgn v = v >= 0 ? 1 : -1.
 *   plain step, every trip, at the sample's point before the update, (x, y) = Z_m + dz (the sum of fr_render_deep_de's step):
 *     wx = x + x, wy = y + y;   L = [[wx, -wy], [|wy| sgn x, |wx| sgn y]]
 *     J11' = (L11 J11 + L12 J21) + s     J12' = L11 J12 + L12 J22
 *     J21' = L21 J11 + L22 J21           J22' = (L21 J12 + L22 J22) + s
 *   the derivative of (|x| + i |y|)^2 + c on the piece the sample's own orbit is on.
 *   BLA step with the entry (A, B) the sample takes, from the one load the step makes: Jij' = (ai1 J1j + ai2 J2j) + bij s.
 *   a rebase leaves J alone.
 *   escape at z = (zx, zy) with r2:  zl = sqrt(r2), ux = zx / zl, uy = zy / zl,
 *     g = (J11 ux + J21 uy, J12 ux + J22 uy),  de = (zl log zl) / sqrt(g.x g.x + g.y g.y), NaN -> 0.
 *   interior samples: de = 0, deriv = 0.
 * J never feeds back into the orbit: iter, nu, rgba without shading and the three step counts are the plain ship entry
 * point's, byte for byte.
 *
 * Extended range: J is four double mantissas and one shared int32 exponent J.e, normalised with norm4 (the ship's BLA section)
 * after every update, in either mode of the lane's delta; the zero has FR_DEEPX_ZERO_EXP.  s = norm1(zm / H, ze) = (sm, es).
 *   extended step: b = (Z_m, eZ) (+) (dz, ed) at eb = max(eZ, ed); L = [[b.x, -b.y], [|b.y| sgn w.x, |b.x| sgn w.y]] from b's
 *     mantissas, the doubling in the exponent: J' = norm4((L J, eb + 1 + J.e) (+) (sm I, es)), L J without s as above, (+)
 *     aligning both to the larger exponent with ldexp and adding; off the diagonal nothing is added.  The signs are those of
 *     w = (ldexp(Z_m.x, eZ - ed) + dz.x, ldexp(Z_m.y, eZ - ed) + dz.y), fold_x's sum in the delta's frame: aligned to eb a
 *     coordinate far below the other is 0 and has no sign left (the tip of the needle, where Y = 0 exactly and y = dz.y).
 *   plain-mode step: L from the plain doubles as in the fp64 range, J' = norm4((L J, J.e) (+) (sm I, es)).
 *   BLA step: J' = norm4((A J, A.e + J.e) (+) (B sm, B.e + es)).
 *   no flush: every step adds s.
 *   escape: z as plain doubles (|z| > bailout there: ldexp of the extended sum's mantissas), g and deep_de_of from J's
 *     mantissas, de = ldexp(that, -J.e), finite at any depth; deriv = ldexp(Jij, J.e), which saturates outside a double's range
 *     as in fr_render_deepx_de.
 * On views both ranges take (1e-30, 1e-100) de and deriv are equal bit for bit.
 *
 * Accuracy: as for the other distance estimates the fp64 iteration loses 2^-53 / de below de of about 1e-3 pixel spacings;
 * above it the tests bound the error against J iterated directly at F + 64 bits (README: measured).
 * Planes, shards, FR_LAYOUT_FRAME, FR_MEM_HOST: de->de and de->deriv follow out->memory and out->layout as out->nu does, deriv
 * sized for four doubles per pixel; of the five planes at least one must be given.
 * Shared state: the orbit slot, the BLA table with its key and fr_ctx_last_deep_ship_steps / fr_ctx_last_deepx_ship_steps are
 * those of the plain ship entry point of the same range -- a call here after it on the same view computes no orbit and builds no
 * table, and the reverse.
 * Validation: everything fr_deep_ship_validate / fr_deepx_ship_validate checks (the other BLA flags are FR_ERR_UNSUPPORTED);
 * then `de` NULL, shade outside {0, 1}, or shade == 1 with edge_px not finite or <= 0 is FR_ERR_INVALID_ARG.
 * Cost: eight live VGPRs (nine extended) and per plain update 22 fp64 operations on top of the step's.  The four kernels use no
 * scratch and spill no VGPR: 109 VGPRs and 4 waves per SIMD (fr_render_deep_ship_de), 153 and 3 (with FR_FLAG_DEEP_SHIP_BLA), 125
 * and 4 (fr_render_deepx_ship_de), 160 and 3 (with FR_FLAG_DEEPX_SHIP_BLA), against 89 / 5, 120 / 4, 101 / 4 and 130 / 3 in the
 * kernels they extend: the fp64 pair runs a wave per SIMD below them, the extended pair keeps their occupancy (README: measured).
 * Out of scope: sequences, fr_node and .franim, slope or normal lighting -- deriv is what a caller needs for it. */
#define FR_HAS_DEEP_SHIP_DE 1
#define FR_HAS_DEEPX_SHIP_DE 1

/* What the two entry points check of their arguments, the view's strings parsed included (no context needed). */
int fr_deep_ship_de_validate(const fr_params* p, const fr_deep_view* view, const fr_deep_de* de, uint32_t width, uint32_t height);
int fr_deepx_ship_de_validate(const fr_params* p, const fr_deepx_view* view, const fr_deep_de* de, uint32_t width,
                              uint32_t height);

/* fr_render_deep_ship / fr_render_deepx_ship with the distance planes; options, timing and the orbit cache as there.  The
 * asynchronous forms: fr_render_deep_ship_async's contract, de->de and de->deriv device planes like the others. */
int fr_render_deep_ship_de(fr_ctx* ctx, const fr_params* p, const fr_deep_view* view, const fr_deep_de* de, uint32_t width,
                           uint32_t height, const fr_shard* shard, const fr_output* out);
int fr_render_deep_ship_de_async(fr_ctx* ctx, const fr_params* p, const fr_deep_view* view, const fr_deep_de* de, uint32_t width,
                                 uint32_t height, const fr_shard* shard, const fr_output* out, void* hip_stream);
int fr_render_deepx_ship_de(fr_ctx* ctx, const fr_params* p, const fr_deepx_view* view, const fr_deep_de* de, uint32_t width,
                            uint32_t height, const fr_shard* shard, const fr_output* out);
int fr_render_deepx_ship_de_async(fr_ctx* ctx, const fr_params* p, const fr_deepx_view* view, const fr_deep_de* de, uint32_t width,
                                  uint32_t height, const fr_shard* shard, const fr_output* out, void* hip_stream);

/* ---- Phoenix views deeper than double precision --------------------------------------------------------------------------
 * fr_render_phoenix (above) below the 1e-13 wall of its double centre: perturbation around one reference orbit with rebasing,
 * for z' = z^2 + c + r z_prev + p z.  The view is a fr_deep_view (p->center_x / p->center_y ignored), p->zoom in [1e-290, 1e3];
 * deltas are fp64.  The recurrence is second order, and so is everything below: the reference orbit is read at two indices, a
 * sample carries two deltas, and a rebase restores a pair of values.
 *
 * Validation (fr_deep_phoenix_validate), in this order: a NULL argument is FR_ERR_INVALID_ARG; p->fractal_type must be
 * FR_FRACTAL_PHOENIX and p->precision FR_PRECISION_F64, otherwise FR_ERR_UNSUPPORTED; the frame size and the fields Phoenix
 * reads, as fr_render_phoenix checks them (phoenix_p and phoenix_r finite, use_julia_set 0 or 1, reserved 0); |p|, |r| < 2^32,
 * the range of the orbit's fixed point, as for a centre; use_julia_set must be 0 -- a Julia-mode Phoenix frame starts every
 * pixel from z = 0 with the same c and is one colour (see fr_render_phoenix), so a deep view of it is FR_ERR_UNSUPPORTED; the
 * zoom in [1e-290, 1e3]; every BLA flag of another path (FR_FLAG_DEEP_BLA .. FR_FLAG_DEEPX_JULIA_BLA) is FR_ERR_UNSUPPORTED,
 * and so is FR_FLAG_DEEPX_PHOENIX_BLA, alone or next to the path's own FR_FLAG_DEEP_PHOENIX_BLA (below), which is accepted; then the view as fr_render_deep checks it (reserved, frac_bits, the centre strings).  bailout, color_offset,
 * interior_style, the orbit trap, stripe_enabled and use_perturbation are ignored as fr_render_phoenix ignores them: the
 * bailout is the shader's fixed 2.  fr_render_deep and the other deep entry points keep rejecting FR_FRACTAL_PHOENIX.
 *
 * Reference orbit: fr_render_deep's fixed point (F fraction bits, the centre strings parsed as there).  P = floor(p 2^F) and
 * R = floor(r 2^F) of the floats' exact values; Z_{-1} = Z_0 = 0; with Q = Z_{n-1}
 *   Re = floor(Zr Zr / 2^F) - floor(Zi Zi / 2^F) + Cr + floor(R Qr / 2^F) + floor(P Zr / 2^F)
 *   Im = floor(2 Zr Zi / 2^F) + Ci + floor(R Qi / 2^F) + floor(P Zi / 2^F)
 * floor being the arithmetic shift of the signed product.  It stops at the first N with |Z_N|^2 > 4, compared exactly, or at
 * N = max_iterations; Z_0 .. Z_N are stored as doubles, rounded to nearest.  With p = r = 0 it is fr_deep_reference_orbit's
 * orbit at bailout 2, bit for bit.
 *
 * Per sample (x, y) and sub-sample s = 0 .. aa*aa-1 with sx = s / aa (OUTER), sy = s % aa: dc is the Phoenix shader's viewport
 * map (phoenix.comp:103-110) less the centre, which is fr_render_deep_ship's map above, operation for operation.  The state is
 * dz, dq (the delta of the previous point) and m, all 0 at the start; Z_{-1} = Z_0 = 0.  For i = 0 .. max_iter-1, with
 * p and r widened to double:
 *   t   = (((Z_m.x + Z_m.x) + dz.x) + p,  (Z_m.y + Z_m.y) + dz.y)
 *   dz' = (((t.x dz.x - t.y dz.y) + r dq.x) + dc.x,  ((t.x dz.y + t.y dz.x) + r dq.y) + dc.y)
 *   dq' = dz;  m += 1;  z = Z_m + dz';  q = Z_{m-1} + dq';  r2 = z.x z.x + z.y z.y
 *   r2 > 4:                                                       escaped at i, lastZ = z
 *   else if r2 + (r r)(q.x q.x + q.y q.y) < (dz'.x dz'.x + dz'.y dz'.y) + (r r)(dq'.x dq'.x + dq'.y dq'.y)  or  m == N:
 *                                                                 rebase: dz = z, dq = q, m = 0
 *   else:                                                         dz = dz', dq = dq'
 * each operation one fp64 rounding as written (no contraction).  Since Z_{-1} = Z_0 = 0, the two deltas after a rebase are the
 * two whole values and the step at m = 0 is the recurrence itself.
 *
 * The rebase rule weighs the previous point by |r|, which is how strongly it feeds the next update.  At r = 0 it is exactly
 * fr_render_deep's rule.  For r of order 1 it rebases only when the whole PAIR (z, q) is smaller than the pair of deltas, so a
 * rebase never puts an O(1) term r q next to pixel-dependent terms many orders below it.  This is an empirical rule, not a
 * theorem: it was checked against the exact fixed-point iteration of every pixel on the views of tests/deep_phoenix_ref.py
 * (zooms 3 down to 1e-100, r from 0 to -0.5), where the escape index agrees everywhere.
 *
 * Planes: iter and nu (double) are sample (0,0)'s i and smooth count, max_iterations for interior samples; rgba is the fp64
 * Phoenix path's colour stage unchanged -- the smooth count of (i, lastZ), then the colour of (smooth / max_iter, smooth,
 * lastZ) narrowed to float, flow stripes when stripe_density > 0.01, the aa x aa average -- and FR_FLAG_POST_CHAIN the post
 * chain with Phoenix's floors.  lastZ of a sample that never escaped is Z_m + dz of its final state, the z of its last update.  Shards, FR_MEM_HOST / FR_MEM_DEVICE, FR_LAYOUT_FRAME, "timing", fr_ctx_last_kernel_ms and
 * fr_ctx_last_grid as for fr_render_deep_ship.
 *
 * The context keeps the most recent Phoenix orbit on the device in a slot of its own, keyed by the centre strings, F,
 * max_iterations and the bits of p and r: no other deep path evicts it, and it evicts none of theirs.
 *
 * Out of scope: distance estimates, sequences, fr_node, .franim and Julia mode; below 1e-290: fr_render_deepx_phoenix.
 * Iteration skipping is FR_FLAG_DEEP_PHOENIX_BLA (below fr_render_deep_phoenix_async, FR_HAS_DEEP_PHOENIX_BLA). */
#define FR_HAS_DEEP_PHOENIX 1
#define FR_HAS_DEEP_PHOENIX_BLA 1 /* FR_FLAG_DEEP_PHOENIX_BLA and fr_ctx_last_deep_phoenix_steps (below fr_render_deep_phoenix_async) */

/* What fr_render_deep_phoenix checks of its arguments, the centre strings parsed included (no context needed). */
int fr_deep_phoenix_validate(const fr_params* p, const fr_phoenix_params* ph, const fr_deep_view* view, uint32_t width,
                             uint32_t height);

/* Z_0 .. Z_N of the view's centre (host only): out_xy holds (max_iter + 1) pairs, *out_len receives N + 1.  Reads ph's p and r
 * (finite, below 2^32); zoom, in [1e-290, 1e3], chooses the automatic fraction bits as in fr_deep_reference_orbit. */
int fr_deep_phoenix_reference_orbit(const fr_deep_view* view, const fr_phoenix_params* ph, double zoom, int32_t max_iter,
                                    double* out_xy, int32_t* out_len);

/* fr_render_deep_ship's contract (planes, memory kinds, FR_LAYOUT_FRAME, shards, options, fr_ctx_last_kernel_ms / _grid) */
int fr_render_deep_phoenix(fr_ctx* ctx, const fr_params* p, const fr_phoenix_params* ph, const fr_deep_view* view, uint32_t width,
                           uint32_t height, const fr_shard* shard, const fr_output* out);

/* fr_render_deep_async's contract: a render of a new view computes its orbit on the host first and is never launch-only */
int fr_render_deep_phoenix_async(fr_ctx* ctx, const fr_params* p, const fr_phoenix_params* ph, const fr_deep_view* view,
                                 uint32_t width, uint32_t height, const fr_shard* shard, const fr_output* out, void* hip_stream);

/* Bilinear approximation for Phoenix, opt-in per call with FR_FLAG_DEEP_PHOENIX_BLA in p->flags.  Only fr_render_deep_phoenix,
 * fr_render_deep_phoenix_async and fr_deep_phoenix_validate read the flag; without it every byte they write is as above.
 * fr_deepx_phoenix_validate answers FR_ERR_UNSUPPORTED for it: the extended path's table is FR_FLAG_DEEPX_PHOENIX_BLA's, in
 * another arithmetic (below fr_render_deepx_phoenix_async).  The recurrence is second order,
 * so the step less its dz^2 term, dz' = (2 Z_m + p) dz + r dq + dc, dq' = dz, is a linear map of the PAIR (dz, dq): an entry of
 * the table is a complex 2x2 matrix M, a complex 2-vector B and a radius that bounds the pair.  The dropped term is below one
 * rounding of (2 Z_m + p) dz while |dz| < 2^-54 |2 Z_m + p|.
 *
 * Notation: every operation is one fp64 rounding as written (no contraction); sqrt is correctly rounded; a complex product a*b
 * is (a.x b.x - a.y b.y, a.x b.y + a.y b.x); sums of complex numbers are componentwise; |c|^2 = c.x c.x + c.y c.y; p and r are
 * the floats widened to double; Z_m is the cached Phoenix orbit, N its last index; M = (M11, M12, M21, M22), B = (B1, B2).
 *   - Constants: eps = 2^-53; dcmax is FR_FLAG_DEEP_SHIP_BLA's, operation for operation (Phoenix uses the ship's viewport map),
 *     from the WHOLE frame's W, H and zoom, never from a shard's rows.
 *   - Single step at 1 <= m <= N-1 (never stored):
 *       a = ((Z_m.x + Z_m.x) + p, Z_m.y + Z_m.y);  M = (a, (r, 0), (1, 0), (0, 0));  B = ((1, 0), (0, 0));
 *       rad = (0.5 * eps) * sqrt(a.x a.x + a.y a.y)
 *   - Table: the levels K = floor(log2(N-1)), the entry coverage (entry j of level k starts at m = 1 + j 2^k and exists iff
 *     m + 2^k <= N) and the entry count (N - 1) - popcount(N - 1) of FR_FLAG_DEEP_BLA; no table for N <= 2.  An entry merges x
 *     (level k-1 at m) and y (level k-1 at m + 2^(k-1)):
 *       Mij = (y.Mi1 * x.M1j) + (y.Mi2 * x.M2j);   Bi = ((y.Mi1 * x.B1) + (y.Mi2 * x.B2)) + y.Bi;
 *       |M_x| = sqrt((|M11|^2 + |M12|^2) + (|M21|^2 + |M22|^2)) of x, the Frobenius norm, an upper bound of the operator norm;
 *       |B_x| = sqrt(|B1|^2 + |B2|^2) of x;
 *       t = (rad_y - |B_x| * dcmax) / |M_x|,  rad = (t > 0 ? t : 0) (NaN: 0),  rad = (rad < rad_x ? rad : rad_x),
 *       and rad = 0 if any of the 12 doubles of M, B is not finite.
 *     The radius bounds the pair: if |dz|^2 + |dq|^2 < rad_x^2 then x is valid, and the pair behind x has norm at most
 *     |M_x| |(dz, dq)| + |B_x| dcmax, which the rule keeps below rad_y.
 *   - Stepping: u is the update index and replaces the loop index.  At a trip with m >= 1 take the largest k >= 1 with
 *     (m-1) mod 2^k == 0, m + 2^k <= N, u + 2^k <= max_iterations and
 *     (dz.x dz.x + dz.y dz.y) + (dq.x dq.x + dq.y dq.y) < rad*rad; then
 *       dz' = ((M11*dz) + (M12*dq)) + (B1*dc),  dq' = ((M21*dz) + (M22*dq)) + (B2*dc),
 *       m += 2^k, u += 2^k, z = Z_m + dz', q = Z_{m-1} + dq', r2 = z.x z.x + z.y z.y;
 *     r2 > 4: escaped at u - 1 with lastZ = z; else the plain step's pair rebase rule on (r2, q, dz', dq'), or m == N: rebase;
 *     else dz = dz', dq = dq'.  If no k qualifies, or m == 0, the plain step above, operation for operation: it escapes at u
 *     and then u += 1.  The planes follow from (escape index, lastZ) exactly as without the flag.  Radii are monotone in k, and
 *     no level's exceeds (0.5 eps) |2 Z_m + p|.
 * Escapes between the first and the last update of a BLA step are not looked for.
 *
 * What it skips (the numpy restatement tests/deep_phoenix_bla_ref.py, 48 x 36, aa 1, the views of tests/deep_phoenix_ref.py):
 * 37.2 % of the updates at 1e-30 with N = 244 (PA30), 43.1 % with N = 391 (PB30); 79.5 % at 1e-100 with N = 758 (PA), 76.5 % with
 * N = 1330 (PB); iter equal to the unflagged path's, and to the exact fixed-point iteration's at 24 x 18, on every pixel of the
 * four.  Shallow views (|dc| far above every radius) take no BLA step.  Measured on one MI355X at 4096^2, aa 1
 * (profiles/deep_phoenix_bla_time.txt, flagged and unflagged interleaved in one session): 7.87 ms against 23.38 ms on PA (2.97x),
 * 15.50 ms against 40.51 ms on PB (2.61x), 8.30 ms against 8.33 ms on PA30 (1.00x: 1.56x fewer loop trips, each costing 1.56
 * plain ones -- the level probe, the 96-byte gather, 4 waves per SIMD for 5), and 2.77 ms against 1.81 ms on the shallow view
 * (0.65x), where the flag can only cost time; iter equal to the unflagged render's on every pixel of all four.
 *
 * Cost: 104 bytes per entry (rad 8, M 64, B 32), on the device, per context, in buffers of the Phoenix path's own, grown like
 * the orbit buffer and keyed by the Phoenix orbit (whose key holds p and r) and the bits of dcmax: a zoom change at a fixed
 * centre rebuilds the table (K small launches on the render's stream, no host work), a new view computes its orbit first.  A
 * rebuild, and the upload of a new Phoenix orbit, are ordered behind the context's previous render with the flag, whatever
 * stream it went to.  The other paths' orbits, tables and counts are untouched by Phoenix renders, and the reverse. */

/* fr_ctx_last_deep_ship_steps' contract for the context's most recent fr_render_deep_phoenix / fr_render_deep_phoenix_async call
 * made with FR_FLAG_DEEP_PHOENIX_BLA: out[0] plain steps, out[1] BLA steps, out[2] updates skipped.  FR_ERR_UNSUPPORTED if there
 * is no such call. */
int fr_ctx_last_deep_phoenix_steps(fr_ctx* ctx, uint64_t out[3]);

/* ---- Phoenix views below 1e-290: extended-exponent deltas ------------------------------------------------------------------
 * fr_render_deep_phoenix stops at 1e-290, where a double can no longer hold the zoom, dc or its two deltas.  These entry points
 * take fr_render_deep_phoenix's arguments with a fr_deepx_view -- centre AND zoom as decimal strings, 1e-1000 <= zoom <= 1e3 as for
 * fr_render_deepx -- and carry dz and dq each as two double mantissas and one int32 exponent while they are small.  p->zoom,
 * p->center_x and p->center_y are not read.  Nothing about fr_render_deep_phoenix changes (it still refuses a zoom below 1e-290).
 *
 * Validation (fr_deepx_phoenix_validate): fr_deep_phoenix_validate's rules in its order -- NULL arguments; FR_FRACTAL_PHOENIX and
 * FR_PRECISION_F64, otherwise FR_ERR_UNSUPPORTED; the frame size and the fields Phoenix reads; |p|, |r| < 2^32; use_julia_set is
 * FR_ERR_UNSUPPORTED for the reason given there; every BLA flag of another path, FR_FLAG_DEEP_PHOENIX_BLA included, is
 * FR_ERR_UNSUPPORTED, alone or next to the path's own FR_FLAG_DEEPX_PHOENIX_BLA (below), which is accepted -- then the view as
 * fr_deepx_validate
 * checks its own: reserved, frac_bits, the centre strings, the zoom string and its range (FR_ERR_INVALID_ARG).
 *
 * Reference orbit (fr_deepx_phoenix_reference_orbit): fr_deep_phoenix_reference_orbit's recurrence at F = frac_bits or
 * fr_deepx_frac_bits(zoom), in the extended storage of fr_deepx_reference_orbit (signed mantissas, int32 exponents,
 * FR_DEEPX_ZERO_EXP for the zero).  Where both entry points accept a view the points are equal bit for bit.
 *
 * Per sample: dc = norm(fx zm, fy zm, ze) with fr_render_deep_phoenix's map on the zoom's mantissa, dcp = dc as plain doubles
 * (a component below 2^-1022 is 0); dz = dq = the zero, m = 0, mode EXTENDED.  Notation (norm, (+), ldexp, extended numbers) as for
 * fr_render_deepx.  For i = 0 .. max_iter-1 one step in the sample's mode, p and r widened to double.
 *   EXTENDED: Z_m = (X, Y, eZ), Z_{m+1} = (Xn, Yn, eZn), dz = (a, b, ed) normalised, dq = (c, d, eq), |c|, |d| <= 2.  pe = 0, or
 *   FR_DEEPX_ZERO_EXP when p == 0; er = eq, or FR_DEEPX_ZERO_EXP when r == 0 (an exact zero never raises a common exponent).
 *     eu = max(eZ + 1, ed);   u = (ldexp(X, eZ + 1 - eu) + ldexp(a, ed - eu),  ldexp(Y, eZ + 1 - eu) + ldexp(b, ed - eu))
 *     et = max(eu, pe);       t = (ldexp(u.x, eu - et) + ldexp(p, pe - et),  ldexp(u.y, eu - et))
 *     P = (t.x a - t.y b,  t.x b + t.y a) at eP = et + ed
 *     e1 = max(eP, er);       s = (ldexp(P.x, eP - e1) + ldexp(r c, er - e1),  ldexp(P.y, eP - e1) + ldexp(r d, er - e1))
 *     en = max(e1, ec);       n = (ldexp(s.x, e1 - en) + ldexp(dc.x, ec - en),  ldexp(s.y, e1 - en) + ldexp(dc.y, ec - en))
 *     m += 1
 *     ez = max(eZn, en);      z = (ldexp(Xn, eZn - ez) + ldexp(n.x, en - ez),  ldexp(Yn, eZn - ez) + ldexp(n.y, en - ez))
 *     eq' = max(eZ, ed);      q = (ldexp(X, eZ - eq') + ldexp(a, ed - eq'),  ldexp(Y, eZ - eq') + ldexp(b, ed - eq'))
 *     r2 = z.x z.x + z.y z.y;   escaped at i if ldexp(r2, 2 ez) > 4, lastZ = (ldexp(z.x, ez), ldexp(z.y, ez))
 *     else rebase if
 *       r2 + ldexp((r r)(q.x q.x + q.y q.y), 2 (eq' - ez)) < ldexp(n.x n.x + n.y n.y, 2 (en - ez)) + ldexp((r r)(a a + b b), 2 (ed - ez))
 *       or m == N:      dz = norm(z, ez), dq = (q, eq') with FR_DEEPX_ZERO_EXP for q = 0, m = 0
 *     else:             dz = norm(n, en), dq = (a, b, ed): a copy, no rounding, no second normalisation
 *     If now dz.e > -400 the sample turns PLAIN with dz = ldexp(dz, dz.e), dq = ldexp(dq, dq.e), which may flush.
 *   PLAIN: the step and the rule of fr_render_deep_phoenix, operation for operation, on the plain doubles of the orbit and dcp.
 *     If afterwards max(|dz.x|, |dz.y|) < 2^-400 the sample turns EXTENDED with dz = norm(dz, 0), dq = norm(dq, 0).
 * The mode is decided by the new dz alone.  In the plain mode |dz| >= 2^-400, so t dz is at least 2^-800 unless t is down at its
 * own rounding error, and an r dq or a dc that a double cannot hold is more than 2^200 below the sum it enters.  On operands a double
 * holds every ldexp is exact and the extended step performs the plain step's roundings, so on every view fr_render_deep_phoenix
 * accepts (the zoom string naming its double) iter, nu and rgba are its bytes.  lastZ of a sample that never escaped is
 * Z_m (+) dz of its final state as a double.  Planes, shards, memory kinds, options and the asynchronous form as there.
 *
 * The pair rebase rule stays empirical: below 1e-290 it was checked against the exact iteration of every pixel on the views of
 * tests/deepx_phoenix_ref.py (1e-310 and 1e-400 with r = -0.5 and -0.375; 1e-1000 with p = r = 0).  No view with r != 0 was
 * checked below 1e-400.  Near Z_m = -p/2 the sum 2 Z_m + p cancels and the stored orbit point limits it to about 2^-53 |p|
 * absolute accuracy, exactly as in fr_render_deep_phoenix.
 *
 * The context keeps the most recent extended Phoenix orbit in a slot of its own, keyed by the centre strings, F,
 * max_iterations and the bits of p and r: it evicts no other slot and none evicts it.
 *
 * Out of scope: distance estimates, sequences, fr_node, .franim and Julia mode.  Iteration skipping is
 * FR_FLAG_DEEPX_PHOENIX_BLA (below fr_render_deepx_phoenix_async, FR_HAS_DEEPX_PHOENIX_BLA). */
#define FR_HAS_DEEPX_PHOENIX 1
#define FR_HAS_DEEPX_PHOENIX_BLA 1 /* FR_FLAG_DEEPX_PHOENIX_BLA and fr_ctx_last_deepx_phoenix_steps (below fr_render_deepx_phoenix_async) */

/* What fr_render_deepx_phoenix checks of its arguments, the view's strings parsed included (no context needed). */
int fr_deepx_phoenix_validate(const fr_params* p, const fr_phoenix_params* ph, const fr_deepx_view* view, uint32_t width,
                              uint32_t height);

/* Z_0 .. Z_N of the view's centre in the extended storage (host only): out_mant_xy holds 2 (max_iter + 1) doubles, out_exp2
 * max_iter + 1 exponents, *out_len receives N + 1.  Reads ph's p and r (finite, below 2^32). */
int fr_deepx_phoenix_reference_orbit(const fr_deepx_view* view, const fr_phoenix_params* ph, int32_t max_iter, double* out_mant_xy,
                                     int32_t* out_exp2, int32_t* out_len);

/* fr_render_deep_phoenix's contract for an extended view */
int fr_render_deepx_phoenix(fr_ctx* ctx, const fr_params* p, const fr_phoenix_params* ph, const fr_deepx_view* view, uint32_t width,
                            uint32_t height, const fr_shard* shard, const fr_output* out);

/* fr_render_deep_async's contract: a render of a new view computes its orbit on the host first and is never launch-only */
int fr_render_deepx_phoenix_async(fr_ctx* ctx, const fr_params* p, const fr_phoenix_params* ph, const fr_deepx_view* view,
                                  uint32_t width, uint32_t height, const fr_shard* shard, const fr_output* out, void* hip_stream);

/* Bilinear approximation for Phoenix views below 1e-290, opt-in per call with FR_FLAG_DEEPX_PHOENIX_BLA in p->flags.  Only
 * fr_render_deepx_phoenix, its _async form and fr_deepx_phoenix_validate read the flag; without it every byte they write is as
 * above, from the same orbit slot and the same kernel.  Every other deep validator answers FR_ERR_UNSUPPORTED for it.  It is
 * FR_FLAG_DEEP_PHOENIX_BLA's scheme -- complex 2x2 maps M and 2-vectors B of the PAIR (dz, dq), a radius on the pair -- with the
 * table and the BLA step carried in FR_FLAG_DEEPX_BLA's extended arithmetic, taken by samples in either mode.
 *
 * Notation: FR_FLAG_DEEP_PHOENIX_BLA's (complex products a*b, componentwise sums, |c|^2, M = (M11, M12, M21, M22), B = (B1, B2),
 * one fp64 rounding per operation as written, sqrt correctly rounded) and FR_FLAG_DEEPX_BLA's: ldexp, FR_DEEPX_ZERO_EXP, the -400
 * mode rule, normalised extended reals (v, e) with v in [0.5, 1), and for mantissas sharing an exponent e
 *   norm(c_1, .., c_n, e) = (ldexp(c_i, -k), e + k), k the frexp exponent of the largest |component| of all the c_i;
 *                           e = FR_DEEPX_ZERO_EXP when all are zero.
 * (P, eP) (+) (Q, eQ) = (ldexp(P, eP - e) + ldexp(Q, eQ - e), e) per component at e = max(eP, eQ), one addition per component.
 * M is its four complex mantissas (8 doubles) with one int32 exponent M.e, B its two (4 doubles) with B.e, both normalised.
 *   - Constants: eps = 2^-53.  dcmax is FR_FLAG_DEEPX_SHIP_BLA's extended real (dcv, dce), operation for operation (Phoenix uses
 *     the ship's viewport map), from the WHOLE frame's W, H and zoom pair, never from a shard's rows.
 *   - Single step at 1 <= m <= N-1 (never stored), from the extended storage Z_m = (X, Y, eZ); pe = 0, or FR_DEEPX_ZERO_EXP
 *     when p == 0, as in the extended step:
 *       ea = max(eZ + 1, pe);   a = (ldexp(X, eZ + 1 - ea) + ldexp(p, pe - ea),  ldexp(Y, eZ + 1 - ea))    (the doubling goes
 *                               to the exponent)
 *       em = max(ea, 0);        M = norm(ldexp(a, ea - em), (ldexp(r, -em), 0), (ldexp(1, -em), 0), (0, 0), em)
 *       B = norm((1, 0), (0, 0), 0) = ((0.5, 0), (0, 0)) with B.e = 1
 *       n = norm(a, ea);  rad = (sqrt(n.x n.x + n.y n.y), n.e) normalised, then rad.e -= 54 unless rad is zero: (0.5 eps) |a|
 *       with the factor in the exponent.  Neither a nor rad is formed from the slot's plain doubles: an orbit point below 2^-1074
 *       is 0 there, and 2^-54 |a| underflows a double for |a| < 2^-968.
 *   - Table: levels, entry coverage, the existence rule and the entry count (N - 1) - popcount(N - 1) of FR_FLAG_DEEP_BLA; no
 *     table for N <= 2.  Merging x then y, products on mantissas in FR_FLAG_DEEP_PHOENIX_BLA's element order:
 *       M = norm(Mij = (y.Mi1 * x.M1j) + (y.Mi2 * x.M2j), y.M.e + x.M.e)
 *       Qi = (y.Mi1 * x.B1) + (y.Mi2 * x.B2) at e1 = y.M.e + x.B.e;   eB = max(e1, y.B.e);
 *       B = norm(Bi = ldexp(Qi, e1 - eB) + ldexp(y.Bi, y.B.e - eB) per component, eB)
 *       |M_x| = (sqrt((|M11|^2 + |M12|^2) + (|M21|^2 + |M22|^2)) of x's mantissas, x.M.e) normalised (the Frobenius norm);
 *       |B_x| = (sqrt(|B1|^2 + |B2|^2) of x's mantissas, x.B.e) normalised;
 *       t = (rad_y (-) |B_x| dcmax) (/) |M_x|, the > 0 and finite rule, rad = rad_x unless rad < rad_x, the void rule (an M.e
 *       or B.e outside [-2^27, 2^27] zeroes the whole entry) and the 24-bit cut of the STORED radius, all exactly as
 *       FR_FLAG_DEEPX_BLA writes them for (A, B) -- with ONE addition, which that flag's formulas never meet: M may be the zero
 *       matrix.  At r = 0 the single step is M = (a, 0, 1, 0), and an a more than 2^1074 below the 1 of M21 (an orbit that
 *       returns below 2^-1075) has no mantissa left under the shared exponent, so the merge behind it is all zero: the map
 *       dz' = B1 dc, dq' = B2 dc, off by less than 2^-1074 |dz|.  The zero matrix (M.e = FR_DEEPX_ZERO_EXP) is NOT void, and
 *       where |M_x| is zero and rad_y (-) |B_x| dcmax > 0 (t would be +inf) rad = rad_x.  Without this a period-201 nucleus at
 *       1e-1000 takes 40 176 loop trips for a 24 x 18 frame instead of 3 456.
 *     An entry is 112 bytes: radius 8 (a float and an int32), mantissas 96, exponents 8.
 *   - Stepping: u replaces the loop index.  At m >= 1, in either mode, the sample's pair as two normalised extended numbers
 *     dz = (a, b, ed), dq = (c, d, eq) -- a PLAIN sample forms norm(dz, 0) and norm(dq, 0) -- is probed on
 *       ev = max(ed, eq);   v2 = (A A + B B) + (C C + D D),  A = ldexp(a, ed - ev), B = ldexp(b, ed - ev), C = ldexp(c, eq - ev),
 *       D = ldexp(d, eq - ev);   the probe passes if v2 < ldexp(rad.v rad.v, 2 (rad.e - ev)).
 *     Take the largest k >= 1 with (m-1) mod 2^k == 0, m + 2^k <= N, u + 2^k <= max_iterations and a passing probe.  The step
 *     is always extended, on the extended dc = (dc, ec).  A term is a product of mantissas at the sum of the exponents; a term
 *     that is exactly zero has FR_DEEPX_ZERO_EXP and raises no common exponent (M12 = M22 = 0 at r = 0, next to a dq that may
 *     lie 2^1300 above dz):
 *       dz' = ((M11*dz, M.e + ed) (+) (M12*dq, M.e + eq)) (+) (B1*dc, B.e + ec)    at en
 *       dq' = ((M21*dz, M.e + ed) (+) (M22*dq, M.e + eq)) (+) (B2*dc, B.e + ec)    at enq
 *       m += 2^k, u += 2^k;   z = Z_m (+) dz' at ez,   q = Z_{m-1} (+) dq' at eq', both orbit points from the extended storage;
 *     then the EXTENDED step's tail with (n, en) = dz' and dq' in the place of its (a, b, ed): escaped at u - 1 if
 *     ldexp(r2, 2 ez) > 4; else the pair rebase rule with its four terms at z's exponent, or m == N: dz = norm(z, ez),
 *     dq = norm(q, eq'), m = 0; else dz = norm(dz', en), dq = norm(dq', enq).  dq' is computed, not copied, so this is where it
 *     is normalised: a BLA step stores both deltas normalised (the zero with FR_DEEPX_ZERO_EXP), and at m >= 1 an extended
 *     sample's dq is always normalised -- a copy of a normalised dz, or this.  Then the mode rule on the new dz alone.
 *     If no level qualifies, or m == 0, the sample's own step of fr_render_deepx_phoenix in its mode, operation for operation:
 *     it escapes at u, then u += 1.  Escapes inside a BLA step are not looked for.  Radii are monotone in k, and none exceeds
 *     2^-54 (4 + |p|).
 *
 * What it skips (the numpy restatement tests/deepx_phoenix_bla_ref.py, 24 x 18, aa 1, the views of tests/deepx_phoenix_ref.py):
 * 79.5 % of the updates on PX310 (N = 2258; 4.9x fewer loop trips), 83.0 % on PX400A (2826; 5.8x), 86.6 % on PX400B (4656;
 * 7.4x), 75.4 % on PXRET (2408; 4.0x), 96.0 % on TIP1000 (2400; 23x), 99.9 % on NUC201X (the period-201 nucleus at 1e-1000,
 * 2412; 302x).  iter equals the unflagged restatement's and the exact fixed-point iteration's on every pixel of PX310, PX400A,
 * PX400B, PXRET and TIP1000 (0 of 432 differ on each; on TIP1000, whose escapes hang on margins of 1e-1000, the unflagged
 * restatement agrees with exact everywhere too); NUC201X is interior on every pixel.
 * Measured on one MI355X at 4096^2, aa 1 (profiles/deepx_phoenix_bla_time.txt, flagged and unflagged interleaved in one session,
 * the unflagged render being the parent's kernel unchanged): PX310 34.19 ms against 142.41 ms (4.17x; 4.55x fewer loop trips),
 * PX400A 32.78 ms against 184.02 ms (5.61x; 6.03x), PX400B 46.77 ms against 301.70 ms (6.45x; 7.17x), TIP1000 3.28 ms against
 * 107.80 ms (32.9x; 48.9x), NUC201X 1.50 ms against 164.74 ms (110x; 302x), and PA (1e-100) passed as an extended view 11.22 ms
 * against 30.44 ms (2.71x; 4.74x); iter equal to the unflagged render's on every pixel of all six.  A flagged trip costs 1.07 to
 * 1.11 unflagged ones on the 1e-310 / 1e-400 views, 1.5 to 2.7 where most trips are BLA steps, 1.74 on PA, whose lanes are
 * plain; the table build is 0.16 to 0.72 ms.  On the shallow view (zoom 3, passed as an extended view; a session of its own) the
 * flag can only cost: 3.56 ms against 2.43 ms (0.68x), no lane passes the pre-filter, the cost is the 3 waves per SIMD for 4
 * and the longer loop body.
 *
 * Cost: 112 bytes per entry on the device, per context, in buffers of the extended Phoenix slot's own, keyed by that slot's
 * orbit generation (the orbit key holds p and r) and the bits of dcmax (mantissa and exponent): a zoom change at a fixed centre
 * and fixed fraction bits rebuilds the table (K small launches on the render's stream) and not the orbit; a second flagged render
 * builds nothing; unflagged renders, and every other path's slots, tables and counters, are untouched. */

/* fr_ctx_last_deepx_ship_steps' contract for the context's most recent fr_render_deepx_phoenix / fr_render_deepx_phoenix_async call
 * made with FR_FLAG_DEEPX_PHOENIX_BLA: out[0] single steps (plain and extended), out[1] BLA steps, out[2] updates skipped.
 * FR_ERR_UNSUPPORTED if there is no such call.  The seven other counters do not report these calls, and the reverse. */
int fr_ctx_last_deepx_phoenix_steps(fr_ctx* ctx, uint64_t out[3]);

/* ---- frames over the GPUs of a node (BASELINE.json north_star: "tiled across the 8 GPUs of one node as disjoint row
 * bands with a final RCCL gather over xGMI") -----------------------------------------------------------------------------
 * New design, no reference counterpart: the reference renders on the one GPU it picked (src/vk_engine.cpp:608).  What it
 * replaces is the same RenderFrameCallback / dispatch surface as fr_render (src/animation_renderer.h:41-48,
 * src/compute_effect_manager.h:435-468), for a caller that owns several devices and, like the reference's caller
 * (AnimationRenderer::start_render, src/animation_renderer.cpp:75-127), renders a sequence of frames: ONE process, one
 * host worker thread per device, up to 4 render contexts ("lanes") per device, a ring of frame slots.
 *
 * fr_node_create: devices[0..n-1] are HIP device ordinals (n <= 16).  They may repeat: n parts on ONE device are n
 *   concurrent renders on that device -- and how the band arithmetic and the in-place stores are tested on one card.
 *   The caller's current device is left as it was, by this and every other fr_node_* call.
 * A frame: its rows are cut into strips (fr_shard: strips of R rows dealt round-robin, part k on devices[k]; "layout" = 1
 *   makes them n contiguous bands), every part renders its rows concurrently, and the frame is assembled in `out`, whose
 *   planes live on devices[root] (FR_MEM_DEVICE) or in host memory (FR_MEM_HOST: staged through a frame buffer on
 *   devices[root], copied back when the frame is waited for).  No collective on the compute path; the one exchange is the
 *   gather, by
 *     FR_GATHER_PEER  the kernels of every part store straight into the root's planes (FR_LAYOUT_FRAME), mapped into the
 *                     other devices' address spaces with hipDeviceEnablePeerAccess: the gather is fused into the stores,
 *                     nothing is staged and nothing waits for a transfer phase (last sentence);
 *     FR_GATHER_RCCL  every part renders into a buffer on its own device and ships its strips to the root with grouped
 *                     ncclSend / ncclRecv (RCCL, point to point over xGMI's full mesh) on a communication stream of its own,
 *                     ordered behind its render by an event, received in place.  For the plain colourings the parts render
 *                     and ship only the smooth-count plane (8 B/pixel instead of 16) and the root recolours the assembled
 *                     frame (fr_colorize_async), bit-identically ("payload").  Needs distinct devices (one communicator
 *                     rank per device); librccl is loaded, through libfractalrenderer_amd_rccl.so, by the first frame that
 *                     uses it.  Fail-safe: every part enqueues its render and reports before ANY part posts a send or a
 *                     receive, so the two sides always match; a failure after that point, or a gather that does not finish
 *                     in 30 s, aborts every communicator (ncclCommAbort) instead of leaving a stream waiting, the frame
 *                     reports the error, and the node carries on with FR_GATHER_PEER where the devices can map each other.
 *   Planes are byte-identical to fr_render's, whatever n, root, layout, gather, slots and lanes.
 * fr_node_render: one frame, synchronously (= fr_node_submit + fr_node_wait_frame).
 * fr_node_submit: validates, takes a frame slot, hands the frame to the workers and returns its ticket (1, 2, ...) without
 *   waiting for anything: up to "slots" frames are IN FLIGHT at once, frame t's parts running on lane t % "lanes" of every
 *   device, so that frame t + 1's ramp-up fills frame t's drain (a 1/8 share of a frame rendered alone costs 1.8x its size).
 *   A submit that finds its slot (ticket % slots) still holding an earlier frame first completes that frame; its verdict is
 *   kept for its ticket (the last 64 are).  `root` is per frame: a caller rotates it (frame f to root f % n) so that every
 *   link carries gather traffic; FR_ROOT_ROTATE does that for FR_MEM_HOST planes.  `out`'s planes must stay valid until the
 *   frame has been waited for.  fr_node_render_async is fr_node_submit without the ticket.
 * fr_node_wait_frame(ticket): waits for that frame alone (its parts' device work; FR_MEM_HOST: + the copy back), in any
 *   order, and returns its verdict.  fr_node_wait: waits for every frame in flight, oldest first, and returns the first
 *   failure nobody has been told about yet.
 * One caller thread at a time drives a node (as one fr_ctx); distinct nodes are independent.
 * fr_node_set_option (refused while frames are in flight): "gather" (fr_gather; 0 = automatic: in-place stores wherever
 *   the devices can map each other -- the gather every one-card test compares bitwise --, RCCL where they cannot; an
 *   explicit 2 whose plugin or communicators cannot be had falls back to 1 if possible: fr_node_last_gather tells),
 *   "layout" (0 = interleaved strips, balanced within a frame; 1 = contiguous bands), "rows_per_strip" (0 = automatic:
 *   32, a whole number of sub-tile rows), "payload" (0 = automatic: the smooth-count plane where fr_colorize_supported,
 *   1 = always the planes asked for), "slots" (1..8 frames in flight, 0 = automatic: 2), "lanes" (1..4 render contexts
 *   per part, created on first use, 0 = automatic: 2), and every fr_ctx_set_option name, applied to all contexts. */
typedef struct fr_node fr_node;
typedef struct fr_anim fr_anim;   /* (.franim animations, below) */
typedef enum fr_gather { FR_GATHER_AUTO = 0, FR_GATHER_PEER = 1, FR_GATHER_RCCL = 2 } fr_gather;
#define FR_ROOT_ROTATE (-1)           /* fr_node_submit / fr_node_render: root = (ticket - 1) % n; FR_MEM_HOST planes */

int  fr_node_create(const int* devices, int n, fr_node** out);
void fr_node_destroy(fr_node* node);
int  fr_node_device_count(const fr_node* node);
int  fr_node_set_option(fr_node* node, const char* name, int64_t value);
int  fr_node_render(fr_node* node, const fr_params* p, uint32_t width, uint32_t height, int root, const fr_output* out);
int  fr_node_submit(fr_node* node, const fr_params* p, uint32_t width, uint32_t height, int root, const fr_output* out,
                    uint64_t* ticket);
int  fr_node_wait_frame(fr_node* node, uint64_t ticket);
int  fr_node_render_async(fr_node* node, const fr_params* p, uint32_t width, uint32_t height, int root, const fr_output* out);
int  fr_node_wait(fr_node* node);
/* frames submitted and not waited for (or completed by a later submit) yet */
int  fr_node_in_flight(const fr_node* node);
/* the gather the most recently submitted frame uses (fr_gather, never AUTO), or < 0 before the first one */
int  fr_node_last_gather(const fr_node* node);
/* device time of part `part`'s kernels of the most recently submitted frame (fr_ctx_last_kernel_ms of its context: needs the
 * option "timing" = 1 on the node) */
float fr_node_last_kernel_ms(fr_node* node, int part);

/* AnimationRenderer::start_render (src/animation_renderer.cpp:26-152) over the GPUs of a node: for frame = first, first +
 * step, ...: time = frame / float(target_fps) (:80), state = interpolate(time) (:83; fr_anim_state_at with `base`, whose
 * fractal_type / precision / flags are not animated), the frame rendered over the node's parts with the shader's post chain
 * (fr_node_submit, roots rotating, up to "slots" frames in flight), and the RenderFrameCallback's tail
 * (src/vk_engine.cpp:1266-1381: readback, second ACES + gamma, u8, flip, PNG) done where the frame was assembled -- the
 * 8-bit export on the root's device, 3 bytes per pixel back, "<folder>/frame_%06d.png" (:86-88) written by a thread of
 * its own while the devices render the next frames.  Files are byte-identical to fr_render_frame_png's.  Fewer than 2
 * keyframes: FR_ERR_INVALID_ARG ("Need at least 2 keyframes to render", :35-42).  on_frame_complete (:123-125) is called on
 * the CALLER's thread for every frame whose file is complete, in order; returning non-zero requests cancellation
 * (cancel_requested, :76): no further frame is started, the call returns FR_OK with *frames_written short of the plan. */
typedef int (*fr_frame_callback)(int32_t frame, int32_t total_frames, void* user);
typedef struct fr_anim_render_options {
    int32_t width, height;                /* 0: the animation's export_width / export_height                        */
    int32_t first_frame, frame_count;     /* frame_count 0: to the end (total = int(duration * target_fps), :48)     */
    int32_t frame_step;                   /* every n-th frame (a sub-sampled sweep); 0 / 1: every frame              */
    int32_t max_iterations_override;      /* 0: the keyframes'                                                       */
    int32_t fractal_type_override;        /* 0: base's; else fr_fractal_type + 1 (the engine's current_fractal_type) */
    fr_frame_callback on_frame_complete;  /* may be NULL                                                             */
    void* user;
    int32_t raw_fd;                       /* > 0: no PNG files -- every frame goes to this file descriptor as packed RGB24,
                                           * top row first, in frame order (fr_write_raw_rgb24: the stdin of `ffmpeg -f rawvideo
                                           * -pix_fmt rgb24 -s WxH -framerate F -i -`); the bytes are the PNG files' pixels.
                                           * output_folder may then be NULL.  0: PNG files (the reference's behaviour)    */
    int32_t reserved;                     /* 0 */
} fr_anim_render_options;
int  fr_node_render_animation(fr_node* node, const fr_anim* anim, const fr_params* base, const fr_anim_render_options* options,
                              const char* output_folder, int32_t* frames_written);

/* ---- recolour from the smooth-count plane (multi-GPU exchange payload) ------------------------
 * New design, no reference counterpart (the reference is single-GPU): for the plain colourings the
 * shaders' colour is a function of the smooth count alone (shaders/mandelbrot.comp:179-190,
 * shaders/julia.comp:243-248, shaders/burning_ship.comp:296-299), so the ranks of a row-band sharded
 * frame can ship the 8-byte (fp64) / 4-byte (fp32) nu plane over xGMI instead of the 16-byte colour
 * and the destination recolours it, bit-identically to what the render kernels write.
 *
 * fr_colorize_supported: 1 when that holds for `params` (Mandelbrot / JuliaSet / BurningShip, no
 * trap / stripe / interior-style variant, antialiasing_samples <= 1, bailout large enough that
 * nu == max_iterations identifies exactly the interior samples, and for FR_PRECISION_F32 max_iterations
 * <= 2^22 so that a float nu just below max_iterations does not round up to it), else 0.
 * fr_colorize_async: nu (n_pixels doubles for FR_PRECISION_F64, floats for F32) -> rgba (n_pixels x
 * RGBA f32), both device pointers, enqueued on hip_stream (NULL: the context's stream), no host sync;
 * FR_FLAG_POST_CHAIN applies the post chain as fr_render does.  FR_ERR_UNSUPPORTED when not supported. */
int fr_colorize_supported(const fr_params* params);
int fr_colorize_async(fr_ctx* ctx, const fr_params* params, uint64_t n_pixels, const void* nu, float* rgba,
                      void* hip_stream);

/* ---- 8-bit export (reference a9) ------------------------------------------------------ */

/* The CPU loop of VulkanEngine::render_animation_frame, src/vk_engine.cpp:1344-1371, on the
 * GPU: per channel ACES tonemap -> pow(1/2.2) -> (uint8)(v*255) with a vertical flip
 * (:1359), RGBA f32 in -> packed RGB8 out (rows*W*3).  through_half != 0 first rounds each
 * channel to fp16 as the reference's rgba16f storage image does (shaders/mandelbrot.comp:5). */
int fr_export_rgb8(fr_ctx* ctx, const float* rgba, uint32_t width, uint32_t height,
                   uint8_t* rgb8, int32_t memory, int32_t through_half);

/* 16-bit export of VulkanEngine::export_print_quality, src/vk_engine.cpp:2054-2073: per channel
 * clamp(v, 0, 1) -> (uint16)(v*65535) with a vertical flip and NO second tonemap (unlike the 8-bit path),
 * RGBA f32 in -> packed RGB16 (host-endian uint16, rows*W*3) out. */
int fr_export_rgb16(fr_ctx* ctx, const float* rgba, uint32_t width, uint32_t height,
                    uint16_t* rgb16, int32_t memory, int32_t through_half);

/* Stream ordering of the two exports above (and of fr_colorize_async with a NULL stream): they run on the
 * context's own stream, ordered behind the most recent render of THIS context whatever stream that was
 * enqueued on; a plane produced by anything else (another context, torch) must be complete, or the caller
 * uses the _async forms below on the producing stream.  The _async forms: device memory only, enqueued on
 * `hip_stream` (NULL = the context's stream), no host synchronisation. */
int fr_export_rgb8_async(fr_ctx* ctx, const float* rgba, uint32_t width, uint32_t height, uint8_t* rgb8,
                         int32_t through_half, void* hip_stream);
int fr_export_rgb16_async(fr_ctx* ctx, const float* rgba, uint32_t width, uint32_t height, uint16_t* rgb16,
                          int32_t through_half, void* hip_stream);

/* ---- frame output (reference f3) ---------------------------------------------------------- */

typedef struct fr_png_text { const char* key; const char* text; } fr_png_text;   /* one tEXt chunk */

/* PNG writer (colour type RGB, no interlace, filter None, zlib deflate).  bit_depth 8: the file
 * stbi_write_png produces pixel-wise (src/vk_engine.cpp:1374-1381); bit_depth 16: host-endian uint16
 * samples written big-endian, compression level 9 (src/vk_engine.cpp:2114-2208).  print_metadata != 0
 * adds what the print export adds: gAMA 1/2.2, sRGB perceptual, pHYs 300 dpi, tIME; `texts` become
 * uncompressed tEXt chunks.  The deflate is band-parallel (FR_PNG_THREADS, default: all cores); for 8-bit files the
 * environment variable FR_PNG_LEVEL = 1..9 picks the zlib level (default 6: an animation export is bound by it). */
int fr_write_png(const char* path, uint32_t width, uint32_t height, int32_t bit_depth, const void* rgb,
                 const fr_png_text* texts, int32_t ntexts, int32_t print_metadata);

/* One packed RGB24 frame to a file descriptor (the stdin pipe of an encoder such as
 * `ffmpeg -f rawvideo -pix_fmt rgb24 -s WxH -i -`, src/video_encoder.cpp:195-224), retrying short writes.  A reader that
 * has gone away is FR_ERR_IO: SIGPIPE is blocked in the calling thread for the duration of the call. */
int fr_write_raw_rgb24(int fd, const uint8_t* rgb8, uint32_t width, uint32_t height);

/* "<folder>/frame_%06d.png", src/animation_renderer.cpp:86-88 */
int fr_frame_path(const char* folder, int32_t frame, char* out, size_t cap);

/* The body of the RenderFrameCallback, bool(const FractalState&, width, height, path)
 * (src/animation_renderer.h:41-48 -> VulkanEngine::render_animation_frame, src/vk_engine.cpp:1181-1418),
 * end to end on the GPU: render with the shader's post chain (what the rgba16f storage image holds),
 * round to fp16, second ACES + gamma, u8, vertical flip (:1344-1371), copy 3 B/pixel back, write the PNG. */
int fr_render_frame_png(fr_ctx* ctx, const fr_params* p, uint32_t width, uint32_t height, const char* path);

/* ---- .franim animations --------------------------------------------------------------- */

typedef struct fr_anim fr_anim;

/* InterpolationType, src/animation_system.h:8-14 */
typedef enum fr_interp {
    FR_INTERP_LINEAR = 0, FR_INTERP_EASE_IN_OUT = 1, FR_INTERP_EASE_IN = 2,
    FR_INTERP_EASE_OUT = 3, FR_INTERP_EXPONENTIAL = 4
} fr_interp;

/* Animation metadata, src/animation_system.h:24-35 */
typedef struct fr_anim_info {
    float   duration;
    int32_t loop;
    int32_t target_fps;
    int32_t export_width;
    int32_t export_height;
    int32_t keyframe_count;
} fr_anim_info;

/* One Keyframe (src/animation_system.h:16-22) restricted to the fields
 * AnimationSystem::load_from_file reads (src/animation_system.cpp:291-301). */
typedef struct fr_keyframe {
    float   time;
    int32_t interp_type;
    fr_params state;
} fr_keyframe;

/* AnimationSystem::load_from_file, src/animation_system.cpp:275-313: parses the .franim
 * JSON.  Required keys exactly as the reference reads them: top level name, description,
 * duration, loop, target_fps, export_width, export_height, keyframes[]; per keyframe time,
 * interp_type, center_x, center_y, zoom, max_iterations, palette_mode, color_offset,
 * color_scale.  The extra keys the reference's writer emits (:246-255) are accepted and
 * loaded when present.  Keyframes keep file order (the reference does not sort on load). */
int  fr_anim_load(const char* path, fr_anim** out);
int  fr_anim_parse(const char* json, size_t len, fr_anim** out);
void fr_anim_free(fr_anim* a);

/* AnimationSystem::save_to_file, src/animation_system.cpp:221-273 (same 19 keyframe keys). */
int  fr_anim_save(const fr_anim* a, const char* path);

int  fr_anim_get_info(const fr_anim* a, fr_anim_info* info);
int  fr_anim_get_keyframe(const fr_anim* a, int32_t index, fr_keyframe* out);
/* name / description strings (owned by the animation) */
const char* fr_anim_name(const fr_anim* a);
const char* fr_anim_description(const fr_anim* a);

/* Empty animation (AnimationSystem ctor, src/animation_system.cpp:7-10: duration 10) and
 * AnimationSystem::add_keyframe (:12-23: append, stable-sort by time, extend duration to
 * time+1 when time > duration). */
int  fr_anim_create(fr_anim** out);
int  fr_anim_add_keyframe(fr_anim* a, float time, const fr_params* state, int32_t interp_type);

/* AnimationSystem::interpolate(time), src/animation_system.cpp:82-181 (+ find_keyframe_pair
 * :183-197, easing :199-212).  `base` is the live FractalState returned when there are no
 * keyframes (:83); fields the reference leaves at FractalState defaults because `result` is
 * default-constructed (:125) come out as fr_params_default() values.  fractal_type/precision/
 * flags are not animated: they are copied from `base`. */
int  fr_anim_state_at(const fr_anim* a, float time, const fr_params* base, fr_params* out);

/* AnimationRenderer::start_render frame arithmetic, src/animation_renderer.cpp:48,80:
 * total_frames = int(duration * target_fps); time(frame) = frame / float(target_fps). */
int32_t fr_anim_frame_count(const fr_anim* a);
float   fr_anim_frame_time(const fr_anim* a, int32_t frame);

/* ---- deep-zoom reference orbit (reference a8) ------------------------------------------- */

/* DeepZoomManager::compute_reference_orbit fp64 loop, src/deep_zoom_system.cpp:378-424:
 * single point, host side in the reference too.  out_xy has room for max_iter (re,im)
 * pairs; *out_len receives the trimmed length. */
int fr_reference_orbit(double cx, double cy, int32_t max_iter, double* out_xy, int32_t* out_len);

/* ---- deep-zoom zoom paths ---------------------------------------------------------------------
 * DeepZoomManager's zoom-path animation, src/deep_zoom_system.cpp:454-556 (host side in the reference too): a list of
 * ZoomKeyframes (src/deep_zoom_system.h:84-89; centre and zoom are "ArbitraryFloat"s that hold a double) walked by
 * update_animation(delta_time): centre linear, zoom in log space, the view snapped onto a keyframe when its duration
 * has passed.  *orbit_dirty is set where the reference recomputes its reference orbit (:505); here the next
 * fr_render of a Deep_Zoom frame does that anyway. */
typedef struct fr_zoom_keyframe {
    double center_x, center_y, zoom;
    float  duration;               /* seconds from the previous keyframe to this one */
} fr_zoom_keyframe;
typedef struct fr_zoom_path fr_zoom_path;

int  fr_zoom_path_create(fr_zoom_path** out);
void fr_zoom_path_free(fr_zoom_path* z);
/* playZoomPath, :454-460 (n == 0: nothing to play) */
int  fr_zoom_path_play(fr_zoom_path* z, const fr_zoom_keyframe* path, int32_t n);
/* zoomTo, :462-485: from `current`'s view (a start keyframe of duration 0) to the target in `duration` seconds */
int  fr_zoom_path_zoom_to(fr_zoom_path* z, const fr_params* current, double target_x, double target_y, double target_zoom,
                          float duration);
/* update_animation, :487-531: advances by delta_time and writes centre / zoom into *state; *animating and *progress
 * mirror DeepZoomState::zoom_animating / zoom_progress (src/deep_zoom_system.h:115-116).  Output pointers may be NULL. */
int  fr_zoom_path_update(fr_zoom_path* z, float delta_time, fr_params* state, int32_t* animating, float* progress,
                         int32_t* orbit_dirty);
/* DeepZoomPresets, :575-601: 0 Seahorse (1e-6, 5 s), 1 Elephant (1e-8, 7 s), 2 Mini Mandelbrot (1e-10, 10 s) */
int  fr_zoom_preset(int32_t which, fr_zoom_keyframe* out);

/* ---- misc ---------------------------------------------------------------------------------- */

const char* fr_last_error(void);
const char* fr_status_string(int status);
void        fr_version(int* major, int* minor);

#ifdef __cplusplus
}
#endif
#endif /* FRACTALRENDERER_AMD_H */
