/*
 * srt_pathtrace.h — C-ABI of the MI355X path-trace library (libsrt_pathtrace.so).
 *
 * (ABI 7.)  This is the drop-in boundary for ONE hot path of JoshuaLim007/Software-Raytracer:
 * the per-pixel trace / shade / accumulate loop.  The reference has no plugin or
 * FFI interface; the seam this ABI replaces is the tile worker
 *
 *     void renderArea(unsigned index, unsigned minX, unsigned maxX,
 *                     unsigned minY, unsigned maxY, const Transform* camera)
 *                                                  (Raytracer/Raytracer.cpp:223-257)
 *
 * together with the globals that worker reads (Raytracer.cpp:30-35,46-48,55-61) and
 * the two buffers it writes (colorBuffer :60, renderSurface->pixels :50,64).
 * Every entry point below names the reference state it stands for.
 *
 * Conventions
 *   - plain C, POD structs, caller-owned host memory; no pointer is retained after a
 *     call returns (srt_set_scene copies).
 *   - every function returns an srt_status (0 = ok); srt_last_error() gives text.
 *     Nothing throws or aborts across the boundary.
 *   - a handle is single-owner and not re-entrant; independent handles (one per GPU)
 *     may be used from independent threads.
 *   - srt_render is asynchronous on the handle's HIP stream; srt_wait / srt_poll
 *     stand for the reference's threadGroupStatus[] scan (Raytracer.cpp:373-384).
 *   - there is NO CPU fallback: without a HIP device srt_create fails with
 *     SRT_ERR_NO_DEVICE.
 *
 * Framebuffer contract (Raytracer.cpp:64, Common.hpp:189-208):
 *   uint32 per pixel = A<<24 | R<<16 | G<<8 | B  (A is always 0), rows bottom-up:
 *   scene pixel (x, y) lives in memory row H-1-y.  "Memory rows" below always mean
 *   rows of that flipped image; the float4 accumulator is indexed x + y*W with the
 *   scene row y (Raytracer.cpp:67), exactly as colorBuffer is.
 */
#ifndef SRT_PATHTRACE_H
#define SRT_PATHTRACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_ABI_VERSION 7

typedef enum srt_status {
    SRT_OK = 0,
    SRT_ERR_INVALID_ARG = 1,
    SRT_ERR_NO_DEVICE = 2,   /* no HIP device / HIP runtime unusable: there is no CPU fallback */
    SRT_ERR_HIP = 3,         /* a HIP call failed; text in srt_last_error */
    SRT_ERR_STATE = 4,       /* call order violated (e.g. render before set_scene / set_camera) */
    SRT_ERR_OOM = 5
} srt_status;

/* Object kinds the reference loader knows (Raytracer/Scene.hpp:43-55). */
typedef enum srt_object_type {
    SRT_OBJ_NONE = 0,    /* inert Object: occupies a list slot, never hit (Object.hpp:21-23) */
    SRT_OBJ_SPHERE = 1,  /* Sphere (Object.hpp:86-168): uses position + radius          */
    SRT_OBJ_BOX = 2,     /* Box    (Object.hpp:170-234): axis-aligned, half_size = Box::size */
    SRT_OBJ_MESH = 3     /* EXTENSION (not in the reference, which has no triangle primitive):
                            an indexed triangle mesh, see srt_mesh / srt_set_meshes          */
} srt_object_type;

/* Material (Raytracer/Common.hpp:293-319), 11 floats. Colours are the r,g,b of the
 * reference's Color (its a is always 0 on this path). */
typedef struct srt_material {
    float smoothness;
    float specular_amount;
    float base_color[3];
    float emissive_color[3];
    float specular_color[3];
} srt_material;

/* One element of ObjectsToRender (Raytracer.cpp:61), flattened. List order is kept:
 * the closest-hit scan keeps the lower index on equal distances (Raytracer.cpp:132). */
typedef struct srt_object {
    int32_t type;        /* srt_object_type */
    float position[3];   /* transform.position */
    float radius;        /* Sphere::radius (transform.scale is NOT used by the intersector) */
    float half_size[3];  /* Box::size, half extents */
    srt_material material;
    int32_t mesh;        /* SRT_OBJ_MESH: index into the array given to srt_set_meshes; else ignored */
} srt_object;

/* EXTENSION — triangle meshes (BASELINE.json configs 4-5).  The reference defines no triangle
 * arithmetic, so this project does: world vertex = vertex + object position
 * (binary32 add); Moller-Trumbore in binary32 without FMA in a fixed operation order; a hit is
 * valid for 0.01 <= t <= 10000 (the Box bounds, Object.hpp:226); the normal is the unit geometric
 * normal turned against the ray.  Among equal distances the earlier object in ObjectsToRender
 * wins, then the lower triangle index.  Vertices: 3 floats each; indices: 3 uint32 per triangle.
 * Limits (SRT_ERR_INVALID_ARG beyond them, with a message that names the limit): 2^24 - 1 = 16,777,215
 * triangles in one mesh (srt_set_meshes) and over all SRT_OBJ_MESH objects of a scene (srt_set_scene: a
 * mesh counts once per object that uses it, triangles that are ignored included), 2^26 - 1 BVH nodes
 * (more than that many triangles can make), world coordinates of magnitude <= 1e9 (judged on the box
 * around all triangles), a `mesh` index within the meshes set, and a BVH of <= 61 levels of 8-wide nodes
 * (7 * depth + 80 entries of the 512-entry traversal buffer).  The builder makes at most
 * 40 + log2(triangles / 4) levels: no scene of up to 2^23 triangles can reach the depth limit, and a larger
 * one only if its tree does not collapse by a single level, so no test provokes that error; the check of
 * the builders (tests/native/builders_check.cpp) asserts the bound for every mesh it builds.  After a
 * refused scene the context holds either the previous scene or none, never half of one.  Triangles with
 * an index out of range or a non-finite vertex are ignored (they cannot produce a valid hit). */
typedef struct srt_mesh {
    const float* vertices;
    size_t vertex_count;
    const uint32_t* indices;
    size_t triangle_count;
} srt_mesh;

/* Environment globals (Raytracer.cpp:55-59). sun_direction is the already normalised
 * vector (the reference normalises once at start-up, :264). */
typedef struct srt_environment {
    float sun_direction[3];
    float sky_color[3];
    float horizon_color[3];
    float ground_color[3];
    float sun_color[3];
} srt_environment;

/* Camera = the reference's Transform (Common.hpp:281-292) + the FOV global (:31).
 * FOV is an integer number of degrees, vertical, exactly as in Raytracer.cpp:112. */
typedef struct srt_camera {
    float position[3];
    float right[3];
    float up[3];
    float forward[3];
    int32_t fov_degrees;
} srt_camera;

#define SRT_RENDER_RESET 1u       /* first sample of this call overwrites (setFrame, :69-71) */
#define SRT_RENDER_COUNT_RAYS 2u  /* fill srt_stats.rays (costs one atomic per wave)       */
#define SRT_RENDER_PREVIEW 4u     /* SIMPLEDRAW == true: the one-ray preview shader (:147-160)
                                     instead of the path-traced branch (:162-185)           */
#define SRT_RENDER_COUNT_WORK 8u  /* count what the launch's loops execute (srt_get_work_counts); same image, a little slower */
#define SRT_RENDER_NO_TIMING 16u  /* do not bracket this render's kernels with timing events: srt_stats.kernel_ms reads 0 for
                                     it.  Two stream markers less per launch (about 1 % of a 2 ms launch) for a caller that
                                     queues render after render and times them itself, or not at all */

/* One render call = sample_count successive "frames" of the reference's loop over a
 * band of memory rows, all on the device, accumulator kept in registers in between
 * (or, for launches with many samples per pixel, the sample colours kept in device memory and folded
 * in order by a second kernel — INTEGRATION.md §6; the result bits are the same).
 *   sample f (1-based, = ACCUMULATIONFRAMES) keys the RNG and sets the running-mean
 *   weight w = (float)(1.0 / f)               (Raytracer.cpp:66-67).
 *   Clean sequence: first_sample = 1 with SRT_RENDER_RESET, later calls continue with
 *   first_sample = previous + count and no reset. */
typedef struct srt_render_params {
    int32_t row_begin;      /* first memory row (inclusive), 0 = top line of the blitted image */
    int32_t row_end;        /* one past the last memory row */
    uint32_t first_sample;  /* >= 1 */
    uint32_t sample_count;  /* >= 1 */
    int32_t max_bounces;    /* MAXBOUNCES (Raytracer.cpp:32), >= 0 */
    uint32_t seed;          /* RNG seed; the reference names only srand(0) (:263) */
    uint32_t flags;         /* SRT_RENDER_* */
    /* progressive-resolution blocks of renderArea (:233-248): one ray per steps x steps block,
     * its colour replicated into every pixel of the block.  0 or 1 = one ray per pixel.  The
     * reference anchors blocks at the start of each worker's column stripe (:235, :338-340):
     * stripe_width = that stripe width (`div`), 0 = a single stripe (anchors at x = 0). */
    int32_t steps;
    int32_t stripe_width;
    int32_t selected_object; /* list index of selectedObject (:53) for the preview highlight; -1 = none */
} srt_render_params;

typedef struct srt_stats {
    uint64_t rays;          /* GetClosestObject calls (primary counted once per sample; steps > 1: per block, as renderArea traces) */
    uint64_t path_samples;  /* W_band * H_band * sample_count of the last render */
    float kernel_ms;        /* HIP-event time of the last render's kernel(s) on its stream; 0 for a render with SRT_RENDER_NO_TIMING */
    uint32_t sample_chunks; /* 1: one kernel traced and folded every sample; n > 1: the samples of a tile were split
                               over n workgroups (grid layers) that stored the colours, and a second, streaming kernel folded
                               them in order (16 B written + 16 B read per traced sample on top of the 20 B/pixel) */
    /* The launch shape srt_render chose (ABI 6).  It is a function of the request, the grid, the device's CU count and — from the
     * second launch of a band on — the loop counts the band's first launch recorded; never of a clock: the same calls give the
     * same shape in every run. */
    uint32_t tile_rows;     /* rows of a wavefront's pixel tile: 8, or 4 / 2 / 1 for launches of few workgroups */
    uint32_t chunk_samples; /* samples per full-size sample chunk (the last layers may hold half as many); 0: not chunked */
    uint32_t shape_source;  /* 0: the static rule (request and grid only); 1: the band's recorded block work as well */
} srt_stats;

/* What the kernels of ONE render executed (SRT_RENDER_COUNT_WORK), counted by the launch itself in wave-uniform loop counters.
 * "tests" are lane-level and EXECUTED: a wavefront runs every trip of these loops for all 64 lanes whatever they carry, so a
 * trip counts 64 tests; cluster_items counts the useful ones of the exact rounds.  Not part of the reference's interface; it is
 * what bench.py prices its roofline line from. */
typedef struct srt_work_counts {
    uint32_t valid;                /* 0: this launch could not count (scene image too large for LDS); all fields 0 */
    uint32_t reserved;
    uint64_t waves;                /* wavefronts that ran a tile (each stages the scene and traces 64 primary rays) */
    uint64_t pool_steps;           /* wave-level steps of the path pool: one bounce for up to 64 paths */
    uint64_t closest_hit_calls;    /* GetClosestObject at wave level: pool steps + the tiles' primary rays */
    uint64_t uniform_sphere_tests; /* Sphere::Raytrace, spheres every ray is tested against            (Object.hpp:104-141) */
    uint64_t cluster_bound_tests;  /* conservative cluster-bound tests (no counterpart in the reference: the culling filter) */
    uint64_t cluster_sphere_tests; /* Sphere::Raytrace, clustered spheres, in the exact rounds (a round: 64 lanes x 4, 2 or 1 tests) */
    uint64_t cluster_items;        /* (ray, cluster) pairs that passed the bounds: the rounds' useful lanes */
    uint64_t box_tests;            /* Box::Raytrace                                                    (Object.hpp:173-233) */
    uint64_t bvh_child_tests;      /* EXTENSION: quantized child boxes of BVH nodes */
    uint64_t triangle_tests;       /* EXTENSION: Moller-Trumbore */
    uint64_t bvh_node_rounds;      /* EXTENSION: wave-level node rounds of the traversal */
    uint64_t mesh_phases;          /* EXTENSION: wave-level traversal phases */
} srt_work_counts;

typedef struct srt_context srt_context;

/* ---- lifetime ------------------------------------------------------------------ */
int srt_abi_version(void);
/* Number of HIP devices visible; *count = 0 and SRT_ERR_NO_DEVICE when none. */
int srt_device_count(int* count);
/* width/height replace SCREEN_WIDTH / SCREEN_HEIGHT (Raytracer.cpp:26-27) at run time. */
int srt_create(int device, int width, int height, srt_context** out);
int srt_destroy(srt_context* ctx);
/* Text of the last failure on ctx (ctx may be NULL: last srt_create failure of this thread). */
const char* srt_last_error(const srt_context* ctx);

/* ---- state the worker reads ---------------------------------------------------- */
/* Replaces ObjectsToRender (Raytracer.cpp:61,293). Copies; count may be 0 and at most 32767
 * (SRT_ERR_INVALID_ARG beyond).  Scenes of up to ~2000 primitives are staged in LDS; larger ones are
 * read from HBM by a slower instantiation of the same kernel (same results). */
int srt_set_scene(srt_context* ctx, const srt_object* objects, size_t count);
/* EXTENSION: mesh geometry referenced by SRT_OBJ_MESH objects.  Call BEFORE srt_set_scene; copies. */
int srt_set_meshes(srt_context* ctx, const srt_mesh* meshes, size_t count);
/* Replaces SunDirection/SkyColor/HorizonColor/GroundColor/SunColor (:55-59). */
int srt_set_environment(srt_context* ctx, const srt_environment* env);
/* Fills env with the reference's start-up values, computed the way :55-59,264 do. */
int srt_environment_default(srt_environment* env);
/* Replaces the `camera` Transform handed to renderArea (:227,295-297) and FOV (:31). */
int srt_set_camera(srt_context* ctx, const srt_camera* camera);

/* ---- optional device-side plumbing --------------------------------------------- */
/* Launch on this hipStream_t instead of the handle's own stream (NULL = own stream). */
int srt_set_stream(srt_context* ctx, void* hip_stream);
/* Render into caller-provided DEVICE buffers (e.g. a torch tensor's data_ptr) instead of
 * the handle's own: framebuffer = W*H uint32, accumulator = W*H float4. NULL = own.  Takes effect for the
 * calls that follow and does not wait: renders already enqueued keep the buffers they were given (the caller
 * keeps those alive until they finish) — so frame k + 1 can render into a second framebuffer while frame k
 * is copied to the host. */
int srt_bind_output(srt_context* ctx, void* d_framebuffer, void* d_accumulator);
int srt_device_framebuffer(srt_context* ctx, void** d_ptr);
int srt_device_accumulator(srt_context* ctx, void** d_ptr);

/* ---- the hot path -------------------------------------------------------------- */
/* Replaces one release of the workers (threadGroupStatus[i] = false, :592-595) for
 * sample_count frames. Asynchronous. */
int srt_render(srt_context* ctx, const srt_render_params* params);
int srt_wait(srt_context* ctx);             /* block until the last render finished */
int srt_poll(srt_context* ctx, int* done);  /* *done = 1 when finished              */
int srt_get_stats(srt_context* ctx, srt_stats* out);  /* waits for the last render */
/* The loop counts of the last render, which must have had SRT_RENDER_COUNT_WORK set (else SRT_ERR_STATE).  Waits. */
int srt_get_work_counts(srt_context* ctx, srt_work_counts* out);

/* Picking (Raytracer.cpp:525-541): GetClosestObject(camera.position, GetRayDirection(camera, x, y))
 * with y in SCENE rows (the reference flips the mouse y first, :532).  *object_index = list
 * index of the hit object or -1.  Synchronous. */
int srt_pick(srt_context* ctx, int x, int y, int* object_index);

/* ---- first-hit buffers (G-buffer / AOVs; ABI 7) ----------------------------------------
 * For every pixel (x, y) of a band: the camera ray GetRayDirection(camera, x, y) from camera.position against the current
 * scene — the same ray, ray generation and closest-hit tie rule as srt_pick and as the primary ray of srt_render — i.e.
 * GetClosestObject's RayHitObject (Raytracer.cpp:123-140, Common.hpp:320-325) and the hit object's material.BaseColor
 * (Raytracer.cpp:163-165).  The reference has no sub-pixel jitter (:106-122): this first hit is the same for every sample.
 * One ray per pixel, always (no progressive blocks).  Outputs, one bit each:
 *
 *   bit                      element  hit                                                  miss
 *   SRT_GBUF_OBJECT          int32    list index of the hit object (what srt_pick returns)  -1
 *   SRT_GBUF_NORMAL_DEPTH    float4   rayHit.normal xyz, w = rayHit.distance                (0, 0, 0, +inf)
 *   SRT_GBUF_POSITION        float4   rayHit.point xyz, w = 1                               (0, 0, 0, 0)
 *   SRT_GBUF_ALBEDO          float4   material.base_color rgb of the hit object, w = 0      (0, 0, 0, 0)
 *                                     (as the reference's Color holds it: negative components clamped to 0, Common.hpp:253-262)
 *
 * Layout: W*H elements indexed x + y*W with the SCENE row y, exactly like the float4 accumulator.  A band is given in MEMORY
 * rows like srt_render_params.row_begin / row_end and writes scene rows [H - row_end, H - row_begin), nothing else.  On hits,
 * normal, distance and point are the bits GetClosestObject computes, the sign of zero included; meshes (the extension) use
 * the triangle definition of srt_mesh.  A NaN camera direction gives a miss everywhere, as in srt_pick. */
#define SRT_GBUF_OBJECT 1u
#define SRT_GBUF_NORMAL_DEPTH 2u
#define SRT_GBUF_POSITION 4u
#define SRT_GBUF_ALBEDO 8u
#define SRT_GBUF_ALL 15u

typedef struct srt_gbuffer_params {
    int32_t row_begin;  /* first memory row (inclusive) */
    int32_t row_end;    /* one past the last memory row */
    uint32_t outputs;   /* SRT_GBUF_* bits, at least one */
    uint32_t flags;     /* reserved, must be 0 */
} srt_gbuffer_params;

/* Asynchronous on the launch stream (the handle's own or the one given to srt_set_stream), behind earlier renders; scene and
 * camera are captured at enqueue.  srt_wait / srt_poll cover it.  SRT_ERR_STATE before srt_set_scene and srt_set_camera;
 * SRT_ERR_INVALID_ARG for an empty or out-of-range band, outputs == 0, unknown output bits or non-zero flags.  Touches neither
 * framebuffer nor accumulator, and leaves what srt_get_stats / srt_get_work_counts report (the last srt_render) and the
 * launch shape of later renders as they are.  Handle-owned G-buffer memory is allocated on first use, per output. */
int srt_render_gbuffer(srt_context* ctx, const srt_gbuffer_params* params);
/* Write ONE output (a single SRT_GBUF_* bit) into a caller DEVICE buffer of W*H elements (e.g. a torch tensor's data_ptr)
 * instead of the handle's own; NULL = own.  Same rules as srt_bind_output: does not wait, enqueued work keeps its buffer. */
int srt_bind_gbuffer(srt_context* ctx, uint32_t output, void* d_ptr);
/* Wait, then copy the whole W*H buffer of ONE output (bound or own) to host memory, as srt_read_accumulator does.
 * SRT_ERR_STATE when that output has neither been bound nor written yet. */
int srt_read_gbuffer(srt_context* ctx, uint32_t output, void* dst);

/* ---- denoiser (edge-avoiding à-trous wavelet filter guided by the first-hit buffers; ABI 7, backward compatible) -------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.
 *
 * Inputs, W*H in the accumulator's layout (x + y*W, scene rows): the colour c_p is the accumulator's rgb (bound or own) as it
 * stands when the filter runs; the guides o_p (SRT_GBUF_OBJECT), n_p, d_p (SRT_GBUF_NORMAL_DEPTH), x_p (SRT_GBUF_POSITION) and
 * a_p (SRT_GBUF_ALBEDO) are the G-buffer slots, bound or own.  srt_denoise does NOT render the G-buffer: call
 * srt_render_gbuffer first (or bind guides of your own).
 *   1. miss pixels (o_p == -1): output = input, all four channels bit for bit; never used as taps.
 *   2. SRT_DENOISE_ALBEDO: per channel m_p = a_p >= 1e-3 ? a_p : 1; the filter runs on c_p / m_p and the result is multiplied
 *      by m_p after the last level.  Without the flag m_p = 1.
 *   3. levels i = 0 .. L-1, step s = 2^i, taps q = p + s*(dx, dy), dx, dy in -2..2, h = [1, 4, 6, 4, 1] / 16; taps outside the
 *      frame are skipped (not clamped); out_p = sum w(p,q) c_q / sum w(p,q) with
 *        w(p,q) = h(dx) h(dy) [o_q == o_p] * max(0, n_p.n_q)^sigma_normal            (sigma_normal = 0: term off)
 *                 * exp(-|n_p.(x_q - x_p)| / (sigma_plane * d_p))                   (sigma_plane = 0: term off)
 *                 * exp(-|c_p - c_q|^2 / (sigma_color * 2^-i)^2)                    (sigma_color = 0: term off; rgb of this
 *                                                                                      level's working colour)
 *      A tap of another object is skipped before any of its values is used (non-finite values there change nothing); the
 *      centre tap always weighs 36/256.  So a pixel of object A depends on input pixels of object A only.
 *      Every sigma >= 0 is accepted, +inf and subnormals included, and an exact tie keeps its weight 1 at all of them
 *      (max(0, 1)^inf = 1, exp(-0 / tiny) = 1): the kernel's reciprocal scales 1 / (sigma_color 2^-i)^2 and
 *      1 / (sigma_plane d_p), and the exponent sigma_normal, stop at FLT_MAX instead of reaching inf.  So a tiny sigma gives
 *      an exact tie the weight 1 and a difference whose square (colour) or size (plane) times FLT_MAX is large the weight
 *      0; only differences below about 1e-19 (colour) or 1e-37 (plane) then weigh more than the definition says.  A
 *      sigma_plane above FLT_MAX (+inf) counts as FLT_MAX, so that the scale of a first hit at d_p = 0 is FLT_MAX like that
 *      of any other vanishing sigma_plane * d_p (an exact tie weighs 1, every other tap 0) instead of 1 / (inf * 0).  A
 *      negative d_p (a first hit behind the camera) turns the plane term into exp(+...), which can overflow.
 *   4. output alpha = input alpha of p.
 *   5. fixed tap order (dy outer, dx inner), no atomics: repeated calls give the same bits. */
#define SRT_DENOISE_ALBEDO 1u       /* demodulate by the ALBEDO guide before filtering, remodulate after */
#define SRT_DENOISE_FRAMEBUFFER 2u  /* also write tone_map(result) into the framebuffer (all memory rows) */

typedef struct srt_denoise_params {
    int32_t iterations;   /* à-trous levels L, 1..8 (footprint +-2*(2^L - 1) px) */
    float sigma_color;    /* sigma_c, >= 0 */
    float sigma_normal;   /* sigma_n, >= 0 */
    float sigma_plane;    /* sigma_x, >= 0 */
    uint32_t flags;       /* SRT_DENOISE_* */
} srt_denoise_params;

/* The library's defaults (pure host, no device needed). */
int srt_denoise_params_default(srt_denoise_params* out);
/* The whole frame, asynchronous on the launch stream behind earlier renders and G-buffer passes; srt_wait / srt_poll cover it.
 * SRT_ERR_INVALID_ARG for iterations outside 1..8, a negative or NaN sigma or unknown flags; SRT_ERR_STATE when a guide it needs
 * (OBJECT, NORMAL_DEPTH, POSITION, plus ALBEDO with SRT_DENOISE_ALBEDO) has never been bound or rendered.  Writes neither the
 * accumulator nor the G-buffer, the framebuffer only with SRT_DENOISE_FRAMEBUFFER (through the render's tone map and packing),
 * and leaves srt_get_stats / srt_get_work_counts and the launch shape of later renders as they are.  The output buffer and
 * one ping-pong buffer (16 B per pixel each) are allocated on first use. */
int srt_denoise(srt_context* ctx, const srt_denoise_params* params);
/* Write the result into a caller DEVICE buffer of W*H float4 instead of the handle's own; NULL = own.  Does not wait. */
int srt_bind_denoised(srt_context* ctx, void* d_float4);
/* Wait, then copy the W*H float4 result (scene rows) to host memory.  SRT_ERR_STATE before the first srt_denoise. */
int srt_read_denoised(srt_context* ctx, float* dst_rgba);

/* ---- temporal reprojection (keeps the accumulated estimate across camera moves; ABI 7, backward compatible) -----------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.
 *
 * Inputs, W*H in the accumulator's layout (x + y*W, scene rows): p is a current pixel, its guides o_p (SRT_GBUF_OBJECT),
 * n_p, d_p (SRT_GBUF_NORMAL_DEPTH) and x_p (SRT_GBUF_POSITION) are the G-buffer slots, bound or own, and c_p is the
 * accumulator's rgb (bound or own) as it stands when the call runs; it must hold n = samples samples of the current camera.
 * Primed values are the history the previous call stored: its camera C' (fov included), result colour h', history length
 * L', object o', normal n' and point x'.
 *   1. miss pixels (o_p == -1): the accumulator is untouched, bit for bit; L_p = 0; never used as taps.
 *   2. projection: B' = [right'*rd' | up'*ld' | forward'*clip] (columns; rd', ld', clip as srt_render folds them from C' and
 *      W / H), inverted once per call on the host in double and passed as float.  (a, b, g) = B'^-1 (x_p - C'.position); if
 *      g <= 0 p has no history, else u = (a/g + 1) * W/2, v = (b/g + 1) * H/2: the exact inverse of the primary ray (no
 *      jitter, no half-pixel offset), so pixel (x, y) of an unchanged camera lands on (x, y).
 *   3. taps: the 2x2 bilinear footprint of (u, v), x0 = floor(u), fx = u - x0 (the same for v).  A tap q counts when it lies
 *      inside the frame, o'_q == o_p, |n_p.(x'_q - x_p)| <= plane_tolerance * d_p and (unless normal_threshold <= -1)
 *      n_p.n'_q >= normal_threshold.  Taps that fail, or whose bilinear weight is 0, are skipped before their colour is
 *      loaded.  w_q = bilinear_q * [q counts], W = sum w_q.
 *   4. blend: if W == 0 or the history is invalid, c_p is kept bit for bit and L_p = n.  Otherwise H_p = sum w_q h'_q / W,
 *      Lh_p = sum w_q L'_q / W, L_p = min(Lh_p + n, max_samples), a_p = n / L_p and the result is (1 - a_p) H_p + a_p c_p
 *      per channel.  With max_samples = inf and a still camera that is the running mean of all frames.
 *   5. output: the result replaces the accumulator's rgb in place (its alpha is never written), so srt_denoise,
 *      srt_read_accumulator and bound tensors see it.  The accumulator then holds an estimate of L_p samples that no render
 *      can continue: the next srt_render must use SRT_RENDER_RESET.  SRT_TEMPORAL_FRAMEBUFFER also writes tone_map(result)
 *      into the framebuffer (all memory rows, the render's packing; miss pixels: tone_map of the accumulator).
 *   6. history: result colour, L, object, normal and point per pixel (48 B) plus the camera, in two handle-owned slots
 *      allocated on first use (96 B per pixel).  A call reads one slot and writes the other: one launch, no pixel reads what
 *      another writes.  The history is invalid on the first call, with SRT_TEMPORAL_RESET, and after srt_set_scene,
 *      srt_set_meshes or srt_set_environment; srt_set_camera does NOT invalidate it.
 *   7. whole frame only, asynchronous on the launch stream behind earlier work (srt_wait / srt_poll cover it).  Leaves
 *      srt_get_stats, srt_get_work_counts, the G-buffer and the launch shape of later renders as they are.  No atomics: the
 *      same sequence of calls gives the same bits. */
#define SRT_TEMPORAL_RESET 1u        /* drop the history: every hit pixel keeps its input, history length = samples */
#define SRT_TEMPORAL_FRAMEBUFFER 2u  /* also write tone_map(result) into the framebuffer (all memory rows) */

typedef struct srt_temporal_params {
    uint32_t samples;        /* n: samples per pixel the accumulator holds for THIS frame, >= 1 */
    float max_samples;       /* L_max: cap on the history length, >= samples (inf: no cap) */
    float plane_tolerance;   /* sigma_t > 0: a tap is kept when |n_p.(x_q - x_p)| <= sigma_t * d_p */
    float normal_threshold;  /* a tap is kept when n_p.n_q >= this; -1 (or less) turns the term off */
    uint32_t flags;          /* SRT_TEMPORAL_* */
} srt_temporal_params;

/* The library's defaults, samples = 1 (pure host, no device needed). */
int srt_temporal_params_default(srt_temporal_params* out);
/* SRT_ERR_INVALID_ARG for samples == 0, max_samples < samples or NaN, plane_tolerance <= 0 or NaN, a NaN normal_threshold or
 * unknown flags.  SRT_ERR_STATE before srt_set_camera, when OBJECT, NORMAL_DEPTH or POSITION has never been bound or
 * rendered, or when one of those three is the handle's own and was last rendered with a camera other than the current one
 * (bound guides cannot be checked: the caller answers for their matching the current camera). */
int srt_temporal_accumulate(srt_context* ctx, const srt_temporal_params* params);
/* Wait, then copy the W*H history lengths L_p of the last call (float, scene rows).  SRT_ERR_STATE before the first call. */
int srt_read_history_length(srt_context* ctx, float* dst);

/* ---- moving objects and motion vectors (the temporal history across scene edits; ABI 7, backward compatible) -----------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7, srt_temporal_params keeps its 20 bytes
 * and there is no new SRT_TEMPORAL_* bit.  A sequence of calls that uses none of them runs what it ran before, bit for bit.
 *
 * Every object is placed by its `position` alone (spheres; boxes, whose rotation the intersector ignores; meshes, as
 * vertex + position), so an object edit that keeps the history is a per-object translation.
 *
 * srt_update_scene replaces the scene exactly as srt_set_scene does — the same validation, scene image, mesh BVH (rebuilt in
 * full: an update costs what a set costs, unless srt_update_mode below allows a refit), and the same resets of dispatch order, recorded work and cost estimate — so
 * srt_render, srt_render_gbuffer, srt_pick and srt_estimate_row_costs give the bits a fresh srt_set_scene of the same list
 * gives.  The one difference: it does NOT invalidate the temporal history.  SRT_ERR_STATE when no scene is set,
 * SRT_ERR_INVALID_ARG when count differs from the current scene's; both are found before anything is touched, so scene and
 * history stay as they were.  Otherwise it fails as srt_set_scene fails: after a refused list the context holds the previous
 * scene or none, and when it holds none the history is dropped too.
 *
 * The context keeps the current object list and a snapshot of the list as it stood at the last srt_temporal_accumulate.
 * Updates between two temporal calls compose: the displacement is taken against the snapshot, not against the previous update.
 * When srt_temporal_accumulate runs with a valid history it makes, for every object i,
 *     delta_i = position_now - position_then   (three binary32 subtractions)
 *     keep_i  = 1 when type, radius, half_size, material and mesh have the same bytes in both lists, else 0.
 * If every delta_i is zero (either sign) and every keep_i is 1 the call is the one defined above, the same kernel included.
 * Otherwise the table (count float4 rows (delta.xyz, keep)) is uploaded on the launch stream and the definition changes to
 *   2'. x~_p = x_p - delta[o_p] (binary32); (a, b, g) = B'^-1 (x~_p - C'.position).
 *   3'. the plane test is |n_p.(x'_q - x~_p)| <= plane_tolerance * d_p.  Object, normal and bilinear rules are unchanged.
 *   4'. a pixel whose object has keep = 0 has no history: c_p is kept bit for bit, L_p = n.  (A reshaped or recoloured object
 *       restarts its own pixels.  The light it sends to its neighbours is not restarted: their history lags behind the edit
 *       by up to max_samples frames, as it does behind any moved object's shadow and bounce light.)
 *   6'. the stored history point is x_p, not x~_p.
 * An object index beyond the table (possible with bound guides only) counts as delta = 0, keep = 1.
 *
 * srt_motion_output switches a second output of srt_temporal_accumulate on or off (per context, off by default): W*H float4
 * (u - x, v - y, Wsum, 0) in the accumulator's layout, scene rows.  u, v are step 2's (2''s) previous-frame coordinates of
 * pixel (x, y), written whenever the pixel has a history (the history is valid and keep = 1), g > 0 and (u, v) lies in the
 * window (-1, W) x (-1, H); otherwise (0, 0).  Wsum is W of step 3, the sum of the counted taps' weights (0 when none
 * counted).  Miss pixels get (0, 0, 0, 0).  The buffer is the handle's own, allocated by the first call that writes it, or
 * the caller's: srt_bind_motion follows srt_bind_denoised (NULL = own, does not wait), srt_read_motion follows
 * srt_read_denoised (waits, copies W*H float4 of the current buffer, bound or own; SRT_ERR_STATE unless that buffer is the one
 * the last call with the output on wrote).  With the output
 * off nothing is allocated and nothing is written, a bound buffer included. */
int srt_update_scene(srt_context* ctx, const srt_object* objects, size_t count);
int srt_motion_output(srt_context* ctx, int enabled);
int srt_bind_motion(srt_context* ctx, void* d_float4);
int srt_read_motion(srt_context* ctx, float* dst);

/* ---- refitting the mesh BVH when an update only moves objects (ABI 7, backward compatible) -------------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.  With the mode left at its default,
 * SRT_UPDATE_REBUILD, srt_update_scene does what it did before, bit for bit, and launches and uploads nothing else.
 *
 * srt_update_mode sets, per context, what srt_update_scene may do to the mesh image (SRT_ERR_INVALID_ARG for another value).
 * The mode is read when srt_set_scene / srt_update_scene run: a mesh image built under SRT_UPDATE_REFIT is followed to the
 * device by its refit data (the meshes' vertices, the triangles' vertex indices, scratch for the exact boxes); a scene set
 * while the mode was SRT_UPDATE_REBUILD has none, so its first update under SRT_UPDATE_REFIT rebuilds (reason 4) and uploads it.
 *
 * Under SRT_UPDATE_REFIT srt_update_scene runs the same validation first (SRT_ERR_STATE, the count check), then picks a path
 * for the mesh image:
 *   kept (3)    old and new list differ at most in `position` of objects that are not SRT_OBJ_MESH (or the scene has no
 *               triangles).  The mesh image, its device buffers and the triangle-id table are not touched.
 *   refit (2)   the lists differ only in `position`, at least one mesh object moved, the refit data is on the device, every
 *               mesh object's position is finite in both lists and the build dropped no triangle of a moved object's mesh for a
 *               non-finite vertex (so the set of valid triangles is the same).  The root box is derived on the host from the
 *               per-object boxes and the positions, and the limit of 1e9 on world coordinates is checked there, before anything
 *               is enqueued: SRT_ERR_INVALID_ARG with srt_set_scene's message, and the previous scene stands.  Then two kernels
 *               rewrite the image in place on the launch stream, behind every render already enqueued: every triangle record
 *               (vertex + position, the edges; the .w words kept) and, level by level from the deepest, every node's origin,
 *               exponents and child bytes from the exact boxes below it.  All triangles and all levels are rewritten, not
 *               only the moved objects'.  Nothing is read back and nothing waits for the kernels.
 *   rebuilt (1) in every other case (also after srt_set_meshes): exactly the code of SRT_UPDATE_REBUILD.
 * In all three paths the analytic scene image is rebuilt on the host and uploaded, dispatch order, recorded work and the cost
 * estimate are reset, and the temporal history and the displacement table are handled as srt_update_scene documents above.
 *
 * Guarantee: after a refit, srt_render, srt_render_gbuffer, srt_render_subsamples and srt_pick give the bits that a fresh
 * srt_set_scene of the same list gives: the triangle records are identical, the child boxes enclose the exact boxes, and the
 * closest-hit key (distance, list order, global triangle id) does not depend on traversal order.  Not promised, and free to
 * differ from a fresh set: srt_estimate_row_costs, srt_get_work_counts, the launch shape of later renders, times.  A tree
 * refitted after a large move is a worse tree; srt_set_scene, or an update under SRT_UPDATE_REBUILD, rebuilds it.  The root's
 * bounding sphere after a refit is the root box's, looser than the per-vertex one of a build.
 *
 * srt_get_update_info describes the last successful srt_update_scene of the context (path 0 before the first).
 *
 * Diagnostics: srt_mesh_image_size gives the bytes of the node array (80 per node) and of the triangle array (48 per triangle)
 * as the kernels read them, 0 and 0 for a scene without triangles; srt_read_mesh_image waits, then copies both (a NULL
 * destination is allowed for an array of 0 bytes).  SRT_ERR_STATE before srt_set_scene. */
#define SRT_UPDATE_REBUILD 0 /* default: srt_update_scene rebuilds the mesh image */
#define SRT_UPDATE_REFIT 1
typedef struct srt_update_info {
    int32_t path;      /* 0: no srt_update_scene yet; 1: rebuilt; 2: refitted; 3: mesh image kept */
    int32_t reason;    /* path 1 only: 1 the mode is REBUILD; 2 a field other than position differs; 3 the valid-triangle set
                          cannot be shown unchanged; 4 the scene was set without refit data (or srt_set_meshes came since) */
    int32_t levels;    /* path 2: launches of the level kernel (= depth of the wide tree) */
    uint32_t triangles; /* path 2: triangle records rewritten */
    uint32_t nodes;     /* path 2: nodes requantized */
    uint32_t moved_mesh_objects; /* mesh objects whose position differs between the two lists */
} srt_update_info;
int srt_update_mode(srt_context* ctx, int mode);
int srt_get_update_info(srt_context* ctx, srt_update_info* out);
int srt_mesh_image_size(srt_context* ctx, size_t* node_bytes, size_t* triangle_bytes);
int srt_read_mesh_image(srt_context* ctx, void* nodes, void* triangles);

/* ---- guided upsampling of progressive-resolution blocks (ABI 7, backward compatible) -------------------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.
 *
 * srt_render with steps > 1 traces one ray per steps x steps block, through the block's ANCHOR pixel, and copies its colour
 * into the block.  There is no sub-pixel jitter, so the full-resolution first-hit buffers hold at the anchor exactly the
 * first hit the block's colour belongs to.  srt_upsample rebuilds every other pixel from the anchors around it, weighed
 * bilinearly and by how well the anchor's first hit agrees with the pixel's own (a joint-bilateral upsample).
 *
 * Inputs, W*H in the accumulator's layout (x + y*W, scene rows): the colour c is the accumulator's rgb (bound or own) as it
 * stands when the pass runs; the guides o (SRT_GBUF_OBJECT), n, d (SRT_GBUF_NORMAL_DEPTH) and x (SRT_GBUF_POSITION) are the
 * G-buffer slots, bound or own.  srt_upsample does NOT render the G-buffer: call srt_render_gbuffer first (or bind guides).
 *   1. anchors: rows — the scene rows that are multiples of steps; columns — with S = stripe_width > 0 ? stripe_width : W,
 *      the columns k*S + j*steps that lie inside stripe k (below (k + 1)*S) and inside the frame.  These are exactly the
 *      pixels srt_render traces for the same steps / stripe_width.  For a pixel p = (px, py): x0 = the largest anchor column
 *      <= px, x1 = the smallest anchor column > px (there may be none; it may be the next stripe's first column and closer
 *      than steps), fx = (px - x0) / (x1 - x0) in binary32, fx = 0 without x1; y0, y1, fy alike on rows.
 *   2. taps: the up to four anchors q = (x0 | x1, y0 | y1) with bilinear weights b_q = (1 - fx | fx) (1 - fy | fy), in the
 *      fixed order y outer, x inner.  A tap counts when it exists, b_q != 0 and o_q == o_p; one that does not is skipped
 *      before any of its other values is loaded, so non-finite colours or guides of another object cannot reach p.
 *      A miss pixel (o_p == -1) takes miss anchors with w_q = b_q: the sky is interpolated too.  A hit pixel weighs
 *        w_q = b_q * max(0, n_p.n_q)^sigma_normal                    (sigma_normal = 0: term off)
 *                  * exp(-|n_p.(x_q - x_p)| / (sigma_plane * d_p))   (sigma_plane = 0: term off)
 *      with the denoiser's arithmetic and clamping rules (srt_denoise, step 3): every sigma >= 0 is accepted, the exponent
 *      and the reciprocal scale 1 / (sigma_plane d_p) stop at FLT_MAX, an exact tie keeps its weight 1.
 *   3. result: sum w_q c_q / sum w_q per channel.  When no tap counts, or the weights sum to 0, the pixel keeps c_p bit for
 *      bit: an object thinner than a block that no anchor of the four sees keeps the block colour (there is no wider
 *      search).  An anchor pixel's one tap is itself, with weight exactly 1 (the two terms are not evaluated): it keeps its
 *      bits, and steps = 1 is the identity on every pixel.  Output alpha = input alpha of p.
 *   4. only ANCHOR pixels of c are read as taps: whether the other pixels of a block hold the block's colour (srt_render
 *      with SRT_RENDER_RESET), a running mean of their own (later one-sample renders) or anything else does not matter.
 *   5. output: W*H float4 into the handle's own "upsampled" buffer (allocated on first use) or a bound one.
 *      SRT_UPSAMPLE_FRAMEBUFFER also writes tone_map(result) into the framebuffer (all memory rows, the render's packing).
 *      SRT_UPSAMPLE_IN_PLACE instead writes the rgb of the NON-anchor pixels that step 3 recomputes into the accumulator;
 *      anchor pixels, all alphas and the upsampled buffer are not written.  The pass then reads only anchors and writes
 *      only non-anchors — no pixel reads what another writes, and a second call gives the same bits — and srt_denoise and
 *      srt_temporal_accumulate can follow on the accumulator.  The accumulator then holds an estimate that no render can
 *      continue: the next srt_render must use SRT_RENDER_RESET.
 *   6. whole frame only, one launch, asynchronous on the launch stream behind earlier work (srt_wait / srt_poll cover it).
 *      Leaves srt_get_stats, srt_get_work_counts, the G-buffer, the temporal history and the launch shape of later renders
 *      as they are.  No atomics: repeated calls give the same bits. */
#define SRT_UPSAMPLE_IN_PLACE 1u     /* write the non-anchor pixels' rgb into the accumulator instead of the upsampled buffer */
#define SRT_UPSAMPLE_FRAMEBUFFER 2u  /* also write tone_map(result) into the framebuffer (all memory rows) */

typedef struct srt_upsample_params {
    int32_t steps;         /* block size of the render being reconstructed, 1..32768 (1: the identity) */
    int32_t stripe_width;  /* that render's stripe_width, >= 0 (0: a single stripe) */
    float sigma_normal;    /* sigma_n, >= 0 */
    float sigma_plane;     /* sigma_x, >= 0 */
    uint32_t flags;        /* SRT_UPSAMPLE_* */
} srt_upsample_params;

/* The library's defaults: steps = 2, stripe_width = 0, the denoiser's sigma_normal and sigma_plane (pure host, no device needed). */
int srt_upsample_params_default(srt_upsample_params* out);
/* SRT_ERR_INVALID_ARG for steps outside 1..32768, a negative stripe_width, a negative or NaN sigma or unknown flags;
 * SRT_ERR_STATE when OBJECT, NORMAL_DEPTH or POSITION has never been bound or rendered. */
int srt_upsample(srt_context* ctx, const srt_upsample_params* params);
/* Write the result into a caller DEVICE buffer of W*H float4 instead of the handle's own; NULL = own.  Does not wait. */
int srt_bind_upsampled(srt_context* ctx, void* d_float4);
/* Wait, then copy the W*H float4 result (scene rows) to host memory.  SRT_ERR_STATE before the first srt_upsample without
 * SRT_UPSAMPLE_IN_PLACE. */
int srt_read_upsampled(srt_context* ctx, float* dst_rgba);

/* ---- geometry-supersampled anti-aliasing (ABI 7, backward compatible) ------------------------------------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.
 *
 * The camera ray of a pixel is the same for every sample (no sub-pixel jitter, Raytracer.cpp:106-122): a frame converges in
 * colour, never in coverage.  Two passes mend the silhouettes without touching srt_render (subpixel reconstruction
 * anti-aliasing, Chajdas, McGuire and Luebke 2011): srt_render_subsamples traces the GEOMETRY at k x k sub-pixel positions,
 * shading stays one estimate per pixel, and srt_antialias rebuilds each pixel as the coverage-weighted mix of its own colour
 * and the colours of the neighbouring pixels whose object its sub-samples see.
 *
 * srt_render_subsamples.  k is 1..4, K = k*k.  Sub-sample s = j*k + i (i, j in 0..k-1) of pixel (x, y) is BY DEFINITION the
 * ray GetRayDirection gives for the integer pixel
 *     (X, Y) = (2k*x + 2i - (k-1), 2k*y + 2j - (k-1))
 * of a virtual frame of (2k*W) x (2k*H) pixels, same camera, fov and origin: nX = ((float)X / (float)(2kW)) * 2 - 1 and the
 * same folded basis ((float)(2kW) / (float)(2kH) == (float)W / (float)H exactly while 2kW, 2kH < 2^24; larger frames are
 * refused).  X and Y are negative for some sub-samples of border pixels; the formula holds for them.  The sub-samples thus
 * lie on a centred k x k grid at offsets (2i - (k-1)) / (2k) pixels from the pixel's own ray; for odd k the centre one IS the
 * pixel's own ray, bit for bit, and k = 1 gives the SRT_GBUF_OBJECT output.  Output: the list index of the hit object or -1,
 * from the same closest hit, scene image and tie rule as srt_render_gbuffer and srt_pick (meshes included), K*W*H int32,
 * plane-major: sub[s][y][x] = index s*W*H + x + y*W with the SCENE row y.  Band, stream and asynchrony are those of
 * srt_render_gbuffer: the band is given in memory rows, only scene rows [H - row_end, H - row_begin) of each plane are
 * written, scene and camera are captured at enqueue, srt_wait / srt_poll cover the call; stats, work counts, the launch shape,
 * the G-buffer, the accumulator and the framebuffer are left alone.  The handle's own buffer is allocated on first use and
 * re-allocated when k grows. */
typedef struct srt_subsample_params {
    int32_t row_begin;  /* first memory row (inclusive) */
    int32_t row_end;    /* one past the last memory row */
    int32_t k;          /* 1..4: k x k sub-samples per pixel */
    uint32_t flags;     /* reserved, must be 0 */
} srt_subsample_params;

/* SRT_ERR_STATE before srt_set_scene and srt_set_camera; SRT_ERR_INVALID_ARG for an empty or out-of-range band, k outside
 * 1..4, non-zero flags, or a frame with 2k*W or 2k*H >= 2^24. */
int srt_render_subsamples(srt_context* ctx, const srt_subsample_params* params);
/* Write the sub-samples into a caller DEVICE buffer of K*W*H int32 instead of the handle's own; NULL = own.  As
 * srt_bind_gbuffer: does not wait, enqueued work keeps its buffer.  What a bound buffer holds is the caller's responsibility. */
int srt_bind_subsamples(srt_context* ctx, void* d_int32);
/* Wait, then copy the K*W*H int32 of the k last rendered into the current buffer (bound or own) to host memory.
 * SRT_ERR_STATE before the first srt_render_subsamples. */
int srt_read_subsamples(srt_context* ctx, int32_t* dst);

/* srt_antialias.  Inputs, W*H in the accumulator's layout (x + y*W, scene rows): the colour c from the chosen source (the
 * accumulator, or the current "denoised" buffer); the pixel guide o = SRT_GBUF_OBJECT, bound or own; the sub-sample buffer
 * sub, bound or own.  srt_antialias renders neither guide.
 *   1. offsets: for sub-sample s = j*k + i of p = (x, y): dx = (float)(2i - (k-1)) / (float)(2k) in binary32, dy alike from j.
 *   2. own sub-samples: sub[s][p] == o_p gives the sub-sample the colour C_s = c_p.
 *   3. foreign sub-samples (sub[s][p] != o_p; a miss counts as the object -1 like any other, so the sky is mixed in at
 *      silhouettes): the taps are the pixels q = p + (ax, ay), ax, ay in {-1, 0, 1}, inside the frame, with the tent weight
 *      w_q = max(0, 1 - |ax - dx|) * max(0, 1 - |ay - dy|) — the 2 x 2 bilinear footprint of the sub-sample's position.  A tap
 *      counts when w_q != 0 and o_q == sub[s][p]; one that does not is skipped before its colour is loaded.
 *      C_s = sum w_q c_q / sum w_q per channel, taps in the fixed order ay outer, ax inner.  When no tap counts — the object
 *      is thinner than a pixel there and no neighbour's own ray sees it — C_s = c_p.
 *   4. result: (sum_s C_s) / K per channel, s ascending, in binary32.  If EVERY C_s is c_p by rule 2 or by the fallback of
 *      rule 3, the output is the input pixel, all four channels bit for bit: every interior pixel is the identity, and so is
 *      k = 1.  Output alpha = input alpha, always.
 *   5. a pixel's output depends on c_p and on the colours of neighbouring pixels whose object one of its sub-samples sees, on
 *      nothing else: non-finite colours on another object cannot reach it.
 *   6. whole frame only, one launch, no atomics: repeated calls give the same bits.  Output: W*H float4 into the handle's own
 *      "antialiased" buffer (allocated on first use) or a bound one — never into the source, whose neighbours the pass reads.
 *      SRT_AA_FRAMEBUFFER also writes tone_map(result) into the framebuffer (all memory rows, the render's packing).
 *      Asynchronous on the launch stream behind earlier work (srt_wait / srt_poll cover it).
 *   7. leaves the accumulator, the denoised buffer, the G-buffer, the sub-sample buffer, the temporal history,
 *      srt_get_stats, srt_get_work_counts and the launch shape of later renders as they are. */
#define SRT_AA_FRAMEBUFFER 2u        /* also write tone_map(result) into the framebuffer (all memory rows) */
#define SRT_AA_SOURCE_ACCUMULATOR 0  /* c = the accumulator, bound or own */
#define SRT_AA_SOURCE_DENOISED 1     /* c = the current "denoised" buffer, bound or own; SRT_ERR_STATE before the first srt_denoise */

typedef struct srt_antialias_params {
    int32_t k;       /* the k of the sub-sample buffer, 1..4 (1: the identity) */
    int32_t source;  /* SRT_AA_SOURCE_* */
    uint32_t flags;  /* SRT_AA_* */
} srt_antialias_params;

/* The library's defaults: k = 2, the accumulator, flags 0 (pure host, no device needed). */
int srt_antialias_params_default(srt_antialias_params* out);
/* SRT_ERR_INVALID_ARG for k outside 1..4, an unknown source or unknown flags.  SRT_ERR_STATE when OBJECT has never been bound
 * or rendered, when the sub-sample buffer has never been bound or rendered, and when that buffer is the handle's own and its
 * last render used another k, has not covered the whole frame since the last scene or camera change, or used a camera other
 * than the current one (a bound buffer is the caller's responsibility). */
int srt_antialias(srt_context* ctx, const srt_antialias_params* params);
/* Write the result into a caller DEVICE buffer of W*H float4 instead of the handle's own; NULL = own.  Does not wait. */
int srt_bind_antialiased(srt_context* ctx, void* d_float4);
/* Wait, then copy the W*H float4 result (scene rows) to host memory.  SRT_ERR_STATE before the first srt_antialias. */
int srt_read_antialiased(srt_context* ctx, float* dst_rgba);

/* ---- variance estimate and variance-guided denoiser (ABI 7, backward compatible) -------------------------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.  srt_render, srt_denoise and
 * srt_temporal_accumulate run what they ran before, bit for bit.
 *
 * srt_denoise has one global sigma_color: it cannot know which pixels are still noisy.  The remedy is the spatial stage of SVGF
 * (Schied et al. 2017, §4.2–4.4): a per-pixel variance scales the colour edge-stop and is filtered along with the colour.  The
 * variance comes from two independently seeded half renders A and B of the same frame (the dual-buffer estimate of Rousselle
 * et al. 2012).  srt_bind_output lets a render accumulate into any device float4 buffer, so both halves come from srt_render:
 *     srt_render(RESET, seed s, n samples)                                  -> half A, in the accumulator
 *     srt_device_half(ctx, &half); srt_bind_output(ctx, NULL, half);
 *     srt_render(RESET, another seed, n samples); srt_bind_output(ctx, NULL, NULL)   -> half B, in the half buffer
 *     srt_render_gbuffer; srt_variance(SRT_VARIANCE_MERGE | ...); srt_denoise_variance
 * All buffers are W*H in the accumulator's layout (x + y*W, scene rows).
 *
 * The second half buffer.  srt_device_half allocates the handle's own W*H float4 buffer on first use and returns it.
 * srt_bind_half makes the passes read the caller's DEVICE buffer instead; NULL = the handle's own.  It does not wait, like the
 * other bind calls.
 *
 * srt_variance.  Inputs: half A = the accumulator (bound or own) as it stands; half B = the half buffer (bound, or own once
 * srt_device_half has fetched it); o = SRT_GBUF_OBJECT and, with SRT_VARIANCE_ALBEDO, a = SRT_GBUF_ALBEDO, bound or own.  The
 * call renders no guide.  lum(c) = (0.2126f*r + 0.7152f*g) + 0.0722f*b in binary32, in this order, without FMA.
 *   1. miss pixels (o_p == -1): v_p = 0.
 *   2. m_p as srt_denoise rule 2 under SRT_VARIANCE_ALBEDO (per channel a_p >= 1e-3 ? a_p : 1), else 1.
 *   3. lA = lum(A_p / m_p), lB = lum(B_p / m_p)  (per channel; no division without the flag).
 *   4. d = 0.5f*lA - 0.5f*lB and v_p = d*d: the variance of the mean of the two halves.  Equal halves give +0, and swapping the
 *      halves gives the same bits.
 *   5. SRT_VARIANCE_MERGE also writes the mean 0.5f*A_p + 0.5f*B_p per rgb channel into the accumulator, in place, for every
 *      pixel, misses included.  The alpha is never written; each pixel reads and writes only itself.  The accumulator then
 *      holds an estimate that no render can continue: the next srt_render must use SRT_RENDER_RESET, as after
 *      srt_temporal_accumulate.  Without the flag the accumulator is not written.
 *   6. output: W*H float into the handle's own "variance" buffer (allocated on first use) or a bound one.  The context remembers
 *      whether the last srt_variance into its own buffer used SRT_VARIANCE_ALBEDO.
 *   7. whole frame, one launch, no atomics; asynchronous on the launch stream behind earlier work (srt_wait / srt_poll cover
 *      it).  Leaves srt_get_stats, srt_get_work_counts, the launch shape of later renders, the G-buffer, the temporal history
 *      and the denoised buffer as they are. */
#define SRT_VARIANCE_ALBEDO 1u  /* the variance of the demodulated luminance: what srt_denoise_variance with SRT_DENOISE_ALBEDO filters */
#define SRT_VARIANCE_MERGE 2u   /* also write the mean of the halves into the accumulator's rgb */

typedef struct srt_variance_params {
    uint32_t flags;  /* SRT_VARIANCE_* */
} srt_variance_params;

/* The library's defaults: SRT_VARIANCE_ALBEDO | SRT_VARIANCE_MERGE (pure host, no device needed). */
int srt_variance_params_default(srt_variance_params* out);
int srt_device_half(srt_context* ctx, void** d_ptr);
int srt_bind_half(srt_context* ctx, void* d_float4);
/* SRT_ERR_INVALID_ARG for unknown flags; SRT_ERR_STATE when OBJECT (or ALBEDO with SRT_VARIANCE_ALBEDO) has never been bound or
 * rendered, and when the half buffer has neither been bound nor fetched with srt_device_half. */
int srt_variance(srt_context* ctx, const srt_variance_params* params);
/* Write the variance into a caller DEVICE buffer of W*H float instead of the handle's own; NULL = own.  Does not wait. */
int srt_bind_variance(srt_context* ctx, void* d_float);
/* Wait, then copy the W*H float variance (scene rows) to host memory.  SRT_ERR_STATE before the first srt_variance. */
int srt_read_variance(srt_context* ctx, float* dst);

/* srt_denoise_variance is srt_denoise with two changes.  Inputs: srt_denoise's (the accumulator and the four guides) and the
 * variance v, the current "variance" buffer, bound or own.  The working variance of level 0 is v; like the working colour it
 * is defined on hit pixels only.
 *   A. a luminance term in place of the colour term:
 *        w_l(p,q) = exp(-|lum(c_p) - lum(c_q)| / (sigma_luminance * sqrt(g_p) + 1e-10f))     (sigma_luminance = 0: term off)
 *      on this level's working colour, where g_p is the 3 x 3 prefiltered working variance of this level: taps p + (dx, dy),
 *      dx, dy in -1..1, at spacing 1 at every level, kernel [1,2,1] x [1,2,1] / 16; only taps inside the frame with o_q == o_p
 *      count and the centre always counts; g_p = sum k v_q / sum k over the counted taps, in the order dy outer, dx inner.
 *      The products k v_q are binary32 products: one at or below 2^-150, half the smallest subnormal, is 0, so a variance of
 *      a few times 1.4e-45 counts as a variance of 0.
 *      As for srt_denoise's terms the reciprocal scale stops at FLT_MAX and an exact tie keeps its weight 1.  Every
 *      sigma_luminance >= 0 is accepted; one above FLT_MAX (+inf) counts as FLT_MAX, so that a zero variance closes the stop at
 *      every sigma (FLT_MAX * 0 = 0) and any other variance opens it (a scale of 0: weight 1 for every finite difference).
 *   B. the variance is filtered with the colour: v_out_p = sum w(p,q)^2 v_q / (sum w(p,q))^2 over the same taps and weights,
 *      ping-ponged per level next to the colour.  The last level's variance is not kept.
 * Everything else is srt_denoise rules 1-5 to the letter: the taps, h, the step 2^i, the skipping of taps outside the frame,
 * the object test before any other value of a tap is used, the normal and plane terms and their clamping, demodulation, the
 * pass-through of miss pixels, the alpha and the tap order; the kernel calls the same device functions.  So with
 * sigma_luminance = 0 the colour result equals srt_denoise's with sigma_color = 0 and otherwise equal parameters bit for bit,
 * and a pixel of object A depends on colours and variances of object A only.
 * Output: the colour goes to the current "denoised" buffer (bound or own), so srt_read_denoised, srt_bind_denoised and
 * srt_antialias with SRT_AA_SOURCE_DENOISED work on it unchanged.  The variance buffer itself is never written.  Flags are
 * SRT_DENOISE_ALBEDO and SRT_DENOISE_FRAMEBUFFER.  Asynchronous as srt_denoise; it leaves alone what srt_denoise leaves alone. */
typedef struct srt_denoise_variance_params {
    int32_t iterations;     /* à-trous levels L, 1..8 */
    float sigma_luminance;  /* sigma_l, >= 0 */
    float sigma_normal;     /* sigma_n, >= 0 */
    float sigma_plane;      /* sigma_x, >= 0 */
    uint32_t flags;         /* SRT_DENOISE_ALBEDO | SRT_DENOISE_FRAMEBUFFER */
} srt_denoise_variance_params;

/* The library's defaults: srt_denoise's for iterations, sigma_normal, sigma_plane and flags, sigma_luminance = 4 (SVGF's). */
int srt_denoise_variance_params_default(srt_denoise_variance_params* out);
/* SRT_ERR_INVALID_ARG for iterations outside 1..8, a negative or NaN sigma or unknown flags; SRT_ERR_STATE when a guide it needs
 * (OBJECT, NORMAL_DEPTH, POSITION, plus ALBEDO with SRT_DENOISE_ALBEDO) has never been bound or rendered, when no variance buffer
 * has been bound or written, and when the variance buffer is the handle's own and the srt_variance that wrote it disagrees
 * with this call on the ALBEDO flag (a bound buffer is the caller's responsibility). */
int srt_denoise_variance(srt_context* ctx, const srt_denoise_variance_params* params);

/* ---- variance from the temporal history (SVGF's luminance moments; ABI 7, backward compatible) ---------------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7, srt_temporal_params keeps its 20 bytes
 * and there is no new SRT_TEMPORAL_* bit.  A sequence of calls that uses none of them runs what it ran before, bit for bit, and
 * with the output off srt_temporal_accumulate launches the kernels it launched before.
 *
 * srt_variance needs the frame rendered twice.  A frame that goes through srt_temporal_accumulate can have its variance from
 * the history instead, at one render per frame: the temporal call keeps, next to the colour, the running first and second
 * moments of the frames' luminance (Schied et al. 2017, §4.2), and srt_temporal_variance turns them into the variance buffer
 * that srt_denoise_variance reads.
 *
 * Moments.  srt_moments_output switches a further output of srt_temporal_accumulate on or off (per context, off by default);
 * flags is 0 or SRT_VARIANCE_ALBEDO.  With it on the call keeps a second history of one float4 record (M1, M2, Lm, 0) per
 * pixel in two handle-owned slots allocated on first use (32 B per pixel); they flip with the colour slots: a call reads one
 * and writes the other.  In the terms of srt_temporal_accumulate's rules, n = samples:
 *   1. miss pixels store (0, 0, 0, 0).
 *   2. mu_p = lum(c_p / m_p): c_p is the accumulator's rgb as the call finds it, before blending; lum and m_p are those of
 *      srt_variance rules 2-3 (m_p = 1, and no division, without SRT_VARIANCE_ALBEDO).  With the flag the ALBEDO guide is
 *      required, under the rule of the other three guides (SRT_ERR_STATE when it is missing or an own one of another camera).
 *   3. the taps are exactly the taps the colour blend counts (rule 3, 3'), with the same weights w_q, in the same order:
 *      s1 = sum w_q M1'_q, s2 = sum w_q M2'_q, sm = sum w_q Lm'_q.  A tap that does not count is skipped before its record is
 *      loaded.
 *   4. if the moments history is valid and W > 0: Lm = min(sm / W + n, max_samples), a = n / Lm,
 *      M1 = (1 - a) * (s1 / W) + a * mu, M2 = (1 - a) * (s2 / W) + a * (mu * mu); binary32, without FMA, in this order.
 *      Otherwise M1 = mu, M2 = mu * mu, Lm = n.  A pixel whose object has keep = 0 restarts, because it has W = 0.
 *   5. the moments history is valid only when the immediately preceding srt_temporal_accumulate wrote it with the same flags
 *      AND the colour history is valid for this call.  So srt_moments_output with another `enabled` or other flags drops it,
 *      and so do SRT_TEMPORAL_RESET and everything that invalidates the colour history.  Lm is the moments' own length: a
 *      sequence that switches the output on midway starts at Lm = n whatever L_p says.
 *   6. turning the output on changes no bit of the accumulator, the history length, the motion output or the framebuffer.
 * srt_read_moments waits and copies the W*H records (scene rows) of the last srt_temporal_accumulate; SRT_ERR_STATE when that
 * call ran with the output off, or there has been none.
 *
 * srt_temporal_variance.  Inputs: the records the last srt_temporal_accumulate wrote, its n (the context remembers it), and
 * o = SRT_GBUF_OBJECT, bound or own, which must be the guide that call read.  The call renders no guide.
 *   1. miss pixels (o_p == -1): v_p = 0.
 *   2. if Lm_p >= min_frames * n (a binary32 product) the temporal estimate applies: s = fmaxf(0, M2_p - M1_p * M1_p).
 *   3. otherwise the pixel is young and the spatial estimate applies: taps q = p + (dx, dy), |dx|, |dy| <= radius, inside the
 *      frame, with o_q == o_p (the centre always counts), in the order dy outer, dx inner; A1 = sum M1_q / cnt,
 *      A2 = sum M2_q / cnt, s = fmaxf(0, A2 - A1 * A1).  A tap of another object is rejected on its object index before its
 *      record is used, so a pixel of object A depends on records of object A only.
 *   4. v_p = s * (n / Lm_p): the variance of the estimate the accumulator holds, the quantity srt_variance also defines.
 *      min_frames = 0 means always temporal, +inf always spatial.
 *   5. output: the current "variance" buffer, bound or own: the buffer and the state srt_variance writes, so that
 *      srt_denoise_variance, srt_read_variance and srt_bind_variance work on it unchanged.  An own buffer is marked with the
 *      records' SRT_VARIANCE_ALBEDO flag, and srt_denoise_variance's flag check applies.
 *   6. whole frame, one launch, no atomics: repeated calls give the same bits.  Asynchronous on the launch stream behind
 *      earlier work (srt_wait / srt_poll cover it).  It leaves alone what srt_variance leaves alone, the accumulator and the
 *      moments themselves included. */
int srt_moments_output(srt_context* ctx, int enabled, uint32_t flags);
int srt_read_moments(srt_context* ctx, float* dst);

typedef struct srt_temporal_variance_params {
    float min_frames;  /* a record of at least min_frames * n samples is used alone; >= 0, +inf allowed */
    int32_t radius;    /* the young pixels' window is (2 * radius + 1)^2, 1..3 */
    uint32_t flags;    /* 0 */
} srt_temporal_variance_params;

/* The library's defaults: min_frames = 4 and radius = 3 (SVGF's four frames and 7 x 7 window), flags = 0 (pure host, no
 * device needed). */
int srt_temporal_variance_params_default(srt_temporal_variance_params* out);
/* SRT_ERR_INVALID_ARG for unknown flags (both calls), a negative or NaN min_frames or a radius outside 1..3; SRT_ERR_STATE
 * when the last srt_temporal_accumulate wrote no moments or there has been none, and when OBJECT has never been bound or
 * rendered.  All are found before anything is touched. */
int srt_temporal_variance(srt_context* ctx, const srt_temporal_variance_params* params);

/* ---- ray queries: closest hits of caller-supplied rays (ABI 7, backward compatible) ---------------------------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of
 * them runs what it ran before.
 *
 * Every other call traces rays that start at the camera.  srt_trace_rays answers, for N rays (o, d) of the caller's, what
 * GetClosestObject(o, d) (Raytracer.cpp:123-140) returns against the current scene: the same closest-hit code, scene image,
 * instantiation (scene in LDS or in memory, with or without the mesh BVH) and tie rule — the earlier entry of the object list
 * keeps an exact distance tie — as srt_render_gbuffer and srt_pick.  No camera is needed.
 *
 * Rays.  A batch is N rays, 1 <= N <= 2^30, in two arrays of N float4:
 *   origin[i]    = (o.xyz, w ignored): the (point, 1) elements of SRT_GBUF_POSITION can be bound as they stand;
 *   direction[i] = (d.xyz, w = t_max); t_max is read by the OCCLUDED output only.
 * srt_write_rays copies host arrays (4 * count floats each) into handle-owned device buffers, which grow on demand, waits like
 * srt_write_accumulator, and makes them the current rays (a binding made by srt_bind_rays ends).  srt_bind_rays makes caller
 * DEVICE arrays (e.g. torch tensors' data_ptr) the current rays; it does not wait and copies nothing: the caller keeps the
 * arrays alive and unchanged until the traces that read them have finished.  NULL, NULL, 0 returns to the handle's own buffers
 * (the current rays are then the last ones written, none before the first srt_write_rays).  SRT_ERR_INVALID_ARG for a NULL
 * array or a count outside 1..2^30; the previous rays stay.
 *
 * Outputs, N elements each, indexed by ray, one bit each.  The four SRT_GBUF_* bits have the element types and the hit / miss
 * values of the srt_render_gbuffer table above, and
 *   SRT_RAYS_OCCLUDED        int32    1 when the ray has a closest hit and rayHit.distance < t_max, else 0
 *                                     (a binary32 <: t_max = NaN gives 0, t_max = +inf gives 1 on every hit; a miss gives 0).
 * OCCLUDED is defined on the CLOSEST hit: it is not an any-hit test of the segment, and an intersection that
 * GetClosestObject does not report does not occlude.
 * The buffers are the handle's own (allocated on first use, grown when a batch needs more) or the caller's: srt_bind_ray_output
 * binds ONE output (a single bit) to a DEVICE buffer of at least N elements, NULL = own, under srt_bind_gbuffer's rules (does
 * not wait, enqueued work keeps its buffer).  They are separate from the G-buffer slots: a trace never touches the G-buffer.
 * srt_read_ray_output waits, then copies the N elements that the last srt_trace_rays wrote for ONE output, from the buffer
 * that trace wrote; SRT_ERR_STATE when the last trace did not write that output (or there has been none).
 *
 * Directions are used as given.  With SRT_RAYS_NORMALIZE the kernel first replaces d by float3::Normalized(d)
 * (Common.hpp:159-162): sqrtf((x*x + y*y) + z*z), then three IEEE divisions.  Input domain:
 *   - unit-length directions (|d.d - 1| <= 1e-6 in binary32, which SRT_RAYS_NORMALIZE provides for every finite non-zero d
 *     whose squared length neither overflows nor underflows) with finite origins: the bits of GetClosestObject, for analytic
 *     objects and for meshes (the triangle definition of srt_mesh), the sign of zero included.  Zero and -0.0 components,
 *     origins inside or exactly on an object and coincident objects are part of this domain.
 *   - a direction with a NaN component: a miss, as in srt_pick.
 *   - other finite non-zero directions (not unit length): handled as srt_render handles the ray of a degenerate lerp.  Spheres
 *     and boxes are tested without the cluster culling, and the result is still exactly GetClosestObject's.  In a scene with
 *     triangles only unit-length directions are pinned: the BVH's culling distances assume them.
 *   - an all-zero direction, infinite components, or origins beyond 1e29 are outside what srt_render itself produces; the
 *     result is some valid output element, not necessarily the reference's.
 *
 * srt_trace_rays is asynchronous on the launch stream behind earlier work; srt_wait / srt_poll cover it.  The scene is captured
 * at enqueue: a trace enqueued after srt_update_scene (rebuilt, refitted or kept) sees the new scene, one enqueued before it the
 * old.  The rays and the output buffers are those current at enqueue.  Errors, all found before anything is touched:
 * SRT_ERR_STATE before srt_set_scene and when no rays have been written or bound; SRT_ERR_INVALID_ARG for outputs == 0,
 * unknown output bits or unknown flags.  The call leaves alone: framebuffer, accumulator, G-buffer, every pass buffer, the
 * temporal history, what srt_get_stats / srt_get_work_counts report and the launch shape of later renders.  No atomics reach
 * the outputs: repeated calls give the same bits. */
#define SRT_RAYS_OCCLUDED 16u
#define SRT_RAYS_NORMALIZE 1u /* srt_trace_params.flags: normalize every direction first */

typedef struct srt_trace_params {
    uint32_t outputs; /* SRT_GBUF_* bits and SRT_RAYS_OCCLUDED, at least one */
    uint32_t flags;   /* 0 or SRT_RAYS_NORMALIZE */
} srt_trace_params;

/* All five outputs, flags = 0 (pure host, no device needed). */
int srt_trace_params_default(srt_trace_params* out);
int srt_write_rays(srt_context* ctx, const float* origins, const float* directions, size_t count);
int srt_bind_rays(srt_context* ctx, const void* d_origins, const void* d_directions, size_t count);
int srt_bind_ray_output(srt_context* ctx, uint32_t output, void* d_ptr);
int srt_trace_rays(srt_context* ctx, const srt_trace_params* params);
int srt_read_ray_output(srt_context* ctx, uint32_t output, void* dst);

/* ---- any-hit queries: is a segment occluded? (ABI 7, backward compatible) ----------------------------------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of
 * them runs what it ran before; srt_trace_params.flags and the output bits of srt_trace_rays are as they were.
 *
 * A shadow, ambient-occlusion or visibility ray knows how far it has to look (t_max), needs one bit, and may stop at the first
 * occluder.  srt_trace_occlusion answers, for every current ray, "does some object report a valid hit with distance < t_max?"
 * — the same predicate as "the closest hit's distance is < t_max", so no new definition is needed — with a kernel of its own
 * that culls by the segment, leaves each primitive scan at the first occluder and never builds a hit record.
 *
 * Rays.  The current rays of srt_write_rays / srt_bind_rays: origin.w is ignored, direction.w is t_max.  The input domain is
 * that of srt_trace_rays: unit-length directions with finite origins are pinned, a direction with a NaN component gives what
 * GetClosestObject gives it (a miss against spheres and triangles; Box::iBox drops a NaN slab distance in its max / min, so a
 * box can still report its hit), other finite non-zero directions are pinned in analytic scenes only.  SRT_OCCLUSION_NORMALIZE is SRT_RAYS_NORMALIZE.
 *
 * Output.  One int32 per ray, written to the SRT_RAYS_OCCLUDED slot: the handle's own buffer or the one bound through
 * srt_bind_ray_output(SRT_RAYS_OCCLUDED).  The call counts as "the last trace", having written that one output:
 * srt_read_ray_output(SRT_RAYS_OCCLUDED) reads it, and the four SRT_GBUF_* outputs give SRT_ERR_STATE until the next
 * srt_trace_rays writes them again.
 *
 * Guarantee.  out[i] equals, bit for bit, what srt_trace_rays writes for SRT_RAYS_OCCLUDED on the same rays and scene, for
 * every ray of that call's pinned domain: t_max = NaN gives 0, +inf gives 1 on every hit, and t_max = 0, a negative t_max or
 * a t_max exactly at or one ulp either side of the closest distance compare as the binary32 < does.  (Box and triangle hits
 * have distances >= 0.01; Sphere::Raytrace reports a negative distance from inside a sphere, so a segment with t_max <= 0
 * can be occluded by a sphere around its origin and by nothing else.)  The closest occluder is not found and no order of
 * testing is promised.
 *
 * Scene and asynchrony.  The scene is captured at enqueue (set, updated, refitted or kept), the rays and the output buffer
 * are those current at enqueue.  Asynchronous on the launch stream behind earlier work; srt_wait / srt_poll cover it.  Errors
 * are those of srt_trace_rays, all found before anything is touched: SRT_ERR_STATE before srt_set_scene and when no rays have
 * been written or bound; SRT_ERR_INVALID_ARG for unknown flags or reserved != 0.  The call leaves alone everything
 * srt_trace_rays leaves alone, and the other four ray outputs' buffers.
 *
 * Work counts.  With SRT_OCCLUSION_COUNT_WORK the launch counts the lane-level tests it EXECUTED for rays of the batch (lanes
 * past the batch count nothing).  The counts are deterministic — the same calls give the same numbers — are summed per wave
 * and added with one vector atomic per wave at the end into a handle-owned record, never into the outputs; without the flag
 * there are no atomics at all.  srt_get_occlusion_work waits and copies the record of the last srt_trace_occlusion;
 * SRT_ERR_STATE unless that trace had SRT_OCCLUSION_COUNT_WORK (or when there has been none). */
#define SRT_OCCLUSION_NORMALIZE 1u  /* as SRT_RAYS_NORMALIZE */
#define SRT_OCCLUSION_COUNT_WORK 2u /* fill srt_occlusion_work for this trace */

typedef struct srt_occlusion_params {
    uint32_t flags;    /* SRT_OCCLUSION_* bits */
    uint32_t reserved; /* must be 0 */
} srt_occlusion_params;

typedef struct srt_occlusion_work { /* lane-level tests EXECUTED for rays of the batch */
    uint32_t valid, reserved;       /* 1, 0 */
    uint64_t rays, occluded;        /* rays of the batch; those with output 1 */
    uint64_t analytic_tests;        /* Sphere::Raytrace + Box::Raytrace evaluations */
    uint64_t node_visits;           /* (ray, BVH node) pairs whose child boxes were tested */
    uint64_t triangle_tests;        /* Moller-Trumbore evaluations */
} srt_occlusion_work;

/* flags = 0, reserved = 0 (pure host, no device needed). */
int srt_occlusion_params_default(srt_occlusion_params* out);
int srt_trace_occlusion(srt_context* ctx, const srt_occlusion_params* params);
int srt_get_occlusion_work(srt_context* ctx, srt_occlusion_work* out);

/* ---- per-pixel visibility: ambient occlusion and sun shadows (ABI 7, backward compatible) -------------------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of
 * them runs what it ran before.
 *
 * srt_render_visibility is a fused device-side pass over the first-hit buffers: per pixel it builds ambient-occlusion and sun
 * segments at the first hit and asks the any-hit query of srt_trace_occlusion about each, without a ray ever leaving the device.
 * Outputs, W*H floats each, indexed x + y*W with the SCENE row y like the G-buffer:
 *   SRT_VIS_AO    the fraction of the pixel's n hemisphere segments that reach ao_radius unoccluded; 1 on a miss
 *   SRT_VIS_SUN   n . s when the ray towards the sun is unoccluded, else 0 (s = -sun_direction); 0 on a miss
 *
 * Rules.
 * 1. Inputs.  Three G-buffer slots, bound (srt_bind_gbuffer) or own (srt_render_gbuffer): o from SRT_GBUF_OBJECT, n from
 *    SRT_GBUF_NORMAL_DEPTH.xyz, x from SRT_GBUF_POSITION.xyz.  The pass renders no guide and needs no camera.  The scene is the
 *    one captured at enqueue (set, updated, refitted or kept), exactly as for srt_trace_occlusion; that the guides belong to
 *    that scene is the caller's business — the pass cannot check it.
 * 2. Origin.  All arithmetic is binary32 without FMA.  O = (x.x + n.x * .00001f, x.y + n.y * .00001f, x.z + n.z * .00001f), the
 *    bounce origin of Raytracer.cpp:177.
 * 3. AO.  For f = first_sample .. first_sample + n - 1: key = srt_rng_key(seed, px + py*W, f) with scene coordinates;
 *    r_k = srt_rng_draw(key, k) for k = 1, 2, 3 (draw 0, the specular lottery that srt_render's sample f spends before its first
 *    bounce, is left out, so this is the hemisphere direction that sample draws); sr = ((float)r_k / 32767 - 0.5f) * 2 per
 *    component; d = float3::Normalized(sr), turned by * -1 when (d.x*n.x + d.y*n.y) + d.z*n.z < 0
 *    (GetRandomNormalOrientedHemisphere, :90-105).  The segment (O, d, t_max = ao_radius) is OPEN when the any-hit query reports
 *    no occluder; ao = (float)open_count / (float)n, an IEEE division of an integer count: no order of evaluation matters.
 * 4. Sun.  s = -sun_direction of the environment captured at enqueue; c = (n.x*s.x + n.y*s.y) + n.z*s.z.  If !(c > 0), sun = 0
 *    and no segment is traced; otherwise sun = 0 when the segment (O, s, t_max = +inf) is occluded, else c.  A sun_direction
 *    that is not unit length is pinned in analytic scenes only (srt_trace_occlusion's domain rule).
 * 5. Miss pixels (o == -1): ao = 1, sun = 0; nothing is traced and none of their other guide values is loaded.
 * 6. Pinned domain.  Guides written by srt_render_gbuffer are pinned bit for bit, and so are bound guides with unit normals and
 *    finite points.  Anything else gives some float per pixel and does not fault.
 * 7. Band.  As srt_gbuffer_params: a band is given in MEMORY rows and only scene rows [H - row_end, H - row_begin) of each
 *    requested output are written.
 * 8. Buffers.  The handle's own (allocated on first use) or the caller's: srt_bind_visibility binds ONE output (a single bit)
 *    to a DEVICE buffer of W*H floats, NULL = own, under srt_bind_gbuffer's rules (does not wait, enqueued work keeps its
 *    buffer).  srt_read_visibility waits, then copies the W*H floats of ONE output from the buffer the last
 *    srt_render_visibility wrote it to; SRT_ERR_STATE unless that call wrote that output (or when there has been none).
 * 9. Side effects.  Asynchronous on the launch stream behind earlier work; srt_wait / srt_poll cover it.  The call leaves alone
 *    everything srt_trace_occlusion leaves alone, and the ray buffers and ray outputs as well.
 * 10. Errors, all found before anything is touched, in this order: SRT_ERR_STATE before srt_set_scene; SRT_ERR_INVALID_ARG for
 *    an empty or out-of-range band, outputs == 0, unknown output or flag bits and, with SRT_VIS_AO, ao_samples outside 1..4096,
 *    first_sample == 0, first_sample + ao_samples - 1 > 2^32 - 1, or an ao_radius that is NaN or <= 0; SRT_ERR_STATE when
 *    OBJECT, NORMAL_DEPTH or POSITION has never been bound or rendered.  ao_samples, first_sample, seed and ao_radius are
 *    not read without SRT_VIS_AO.
 * 11. Work counts.  With SRT_VIS_COUNT_WORK the launch counts, deterministically: the segments it traced (n per hit pixel with
 *    SRT_VIS_AO, one per pixel with c > 0 with SRT_VIS_SUN), those with no occluder, the wave-level any-hit calls — a wave packs
 *    the h * n AO segments of its 8 x 8 tile (h hit pixels) into ceil(h * n / 64) calls and spends one more on the tile's sun
 *    segments when some pixel has c > 0 — and the lane-level tests of srt_occlusion_work.  The counts are summed per wave and
 *    added with one vector atomic per wave into a handle-owned record; without the flag there are no atomics at all.
 *    srt_get_visibility_work waits and copies the record of the last srt_render_visibility; SRT_ERR_STATE unless that call had
 *    SRT_VIS_COUNT_WORK (or when there has been none). */
#define SRT_VIS_AO 1u         /* float per pixel */
#define SRT_VIS_SUN 2u        /* float per pixel */
#define SRT_VIS_COUNT_WORK 1u /* flags: fill srt_visibility_work for this call */

typedef struct srt_visibility_params {
    int32_t row_begin;     /* first memory row (inclusive), as srt_gbuffer_params */
    int32_t row_end;       /* one past the last memory row */
    uint32_t outputs;      /* SRT_VIS_AO | SRT_VIS_SUN, at least one */
    uint32_t flags;        /* 0 or SRT_VIS_COUNT_WORK */
    uint32_t ao_samples;   /* n: 1..4096 (read with SRT_VIS_AO only) */
    uint32_t first_sample; /* f0 >= 1, f0 + n - 1 <= 2^32 - 1 */
    uint32_t seed;
    float ao_radius;       /* t_max of the AO segments: > 0, +inf allowed; NaN, 0 and negative values are refused */
} srt_visibility_params;

typedef struct srt_visibility_work {
    uint32_t valid, reserved;  /* 1, 0 */
    uint64_t segments, open;   /* segments traced; those with no occluder */
    uint64_t wave_trips;       /* wave-level any-hit calls */
    uint64_t analytic_tests;   /* as srt_occlusion_work */
    uint64_t node_visits;
    uint64_t triangle_tests;
} srt_visibility_work;

/* outputs = AO | SUN, flags = 0, ao_samples = 16, first_sample = 1, seed = 0, ao_radius = +inf; row_begin = row_end = 0: the
 * band is the caller's to fill (pure host, no device needed). */
int srt_visibility_params_default(srt_visibility_params* out);
int srt_render_visibility(srt_context* ctx, const srt_visibility_params* params);
int srt_bind_visibility(srt_context* ctx, uint32_t output, void* d_float);
int srt_read_visibility(srt_context* ctx, uint32_t output, float* dst);
int srt_get_visibility_work(srt_context* ctx, srt_visibility_work* out);

/* ---- radiance queries: path-traced radiance of caller-supplied rays (ABI 7, backward compatible) ------------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of
 * them runs what it ran before.
 *
 * srt_trace_rays says what a ray hits, srt_trace_occlusion whether a segment is blocked, srt_render_visibility how open the
 * hemisphere at a first hit is.  srt_trace_radiance says how much light arrives along a ray: srt_render's shading loop
 * (RaytraceScene's path branch, Raytracer.cpp:162-185) and its running mean, without the camera, the pixel grid and the
 * framebuffer — for irradiance and reflection probes, light-map texels, the secondary rays of a hybrid renderer.
 *
 * Rules.
 * 1. Rays.  The current rays of srt_write_rays / srt_bind_rays.  origin.w and direction.w are ignored: there is no t_max.
 *    The input domain is that of srt_trace_rays: finite origins with unit-length directions are pinned bit for bit
 *    (SRT_RADIANCE_NORMALIZE provides unit length: float3::Normalized first, as SRT_RAYS_NORMALIZE); in analytic scenes other
 *    finite non-zero directions are pinned as well; anything else gives some float4 per ray and does not fault.
 * 2. Sample.  For f = first_sample .. first_sample + sample_count - 1 and ray i: key = srt_rng_key(seed, id_base + i, f) (the id
 *    wraps modulo 2^32), draws counted from 0, and colour_f = RaytraceScene(o_i, d_i), the path branch of Raytracer.cpp:141-146,
 *    162-185, 212, in binary32 without contraction — the arithmetic of srt_render's kernel.  Draw order: draw 0 is the specular
 *    lottery at the first hit (:165); then, per bounce, three draws for the hemisphere direction (x, y, z; :90-105) and, when the
 *    bounce ray hits, one lottery at that hit (:182).  The dissipation is 0.8 from the second bounce on (:169-171), a bounce ray
 *    starts at point + normal * .00001f (:177), a ray that leaves the scene adds GetEnvironmentColor times the throughput and ends
 *    the path (:178-181), a primary miss gives GetEnvironmentColor(d_i) (:143-145), and max_bounces = 0 gives the first hit's
 *    emissive colour.  The colour has four lanes: the fourth is +0, or NaN exactly when the lerp parameter of an environment
 *    lookup of the path is NaN (a non-finite direction), as in srt_render.
 * 3. Mean.  out_i = SetScreenPixel's running mean (:63-71) over f in ascending order: with weight = (float)(1.0 / f),
 *    out = clamp0(out * (1 - weight)) + colour_f * weight per lane.  With SRT_RADIANCE_RESET sample first_sample overwrites the
 *    element (setFrame, :69-71); without it the mean continues from what the element holds, so a call with samples 1..3 and RESET
 *    followed by one with samples 4..9 without gives the bits of one call with samples 1..9.  The fold order per ray is fixed:
 *    repeated calls give the same bits however the kernel packs its work.
 * 4. Equivalence.  For the rays (camera.position, GetRayDirection(camera, x, y)) in the order i = x + y*W (scene rows), with
 *    id_base = 0 and equal seed, samples and bounces, out_i equals in all four lanes (NaN as NaN) the accumulator element srt_render
 *    writes for that pixel — the scene in LDS or in memory, with or without meshes.
 * 5. Splitting.  Tracing rays [a, b) as a batch of their own with id_base raised by a gives the bits of the whole batch.
 * 6. Output.  N float4, the handle's own buffer (allocated on first use, grown when a batch needs more) or the caller's:
 *    srt_bind_radiance binds a DEVICE buffer of at least N float4, NULL = own, under srt_bind_ray_output's rules (does not wait,
 *    enqueued work keeps its buffer).  srt_read_radiance waits, then copies the N float4 the last srt_trace_radiance wrote, from
 *    the buffer it wrote; SRT_ERR_STATE before the first trace.
 * 7. Asynchrony.  Asynchronous on the launch stream behind earlier work; srt_wait / srt_poll cover it.  The scene and the
 *    environment are those captured at enqueue (set, updated, refitted or kept); the rays and the output buffer are those current
 *    at enqueue.
 * 8. What it leaves alone.  Everything srt_trace_rays leaves alone, and the ray outputs and their "last trace" record as well:
 *    srt_read_ray_output behaves as before the call.
 * 9. Errors, all found before anything is touched: SRT_ERR_STATE before srt_set_scene; SRT_ERR_INVALID_ARG for unknown flags,
 *    first_sample == 0, sample_count outside 1..4096, first_sample + sample_count - 1 > 2^32 - 1 or a negative max_bounces;
 *    SRT_ERR_STATE when no rays have been written or bound.
 * 10. Work counts.  With SRT_RADIANCE_COUNT_WORK the launch counts, deterministically: its rays, its samples (N * n), the
 *    lane-level GetClosestObject calls by srt_stats.rays' rule (the primary call counts once PER SAMPLE, although the kernel
 *    traces it once per ray), and the wave-level closest-hit invocations it executed, primaries included — a wave traces the
 *    primary rays of 64 consecutive rays in one invocation and packs their samples' bounce rays, 64 to an invocation, whichever
 *    ray they belong to.  The counts are summed per wave and added with one vector atomic per wave into a handle-owned record;
 *    without the flag there are no atomics at all.  srt_get_radiance_work waits and copies the record of the last
 *    srt_trace_radiance; SRT_ERR_STATE unless that trace had SRT_RADIANCE_COUNT_WORK (or when there has been none). */
#define SRT_RADIANCE_RESET 1u      /* sample first_sample overwrites the output element; without it the running mean continues */
#define SRT_RADIANCE_NORMALIZE 2u  /* as SRT_RAYS_NORMALIZE */
#define SRT_RADIANCE_COUNT_WORK 4u /* fill srt_radiance_work for this call */
#define SRT_RADIANCE_SUN_SAMPLING 0x10u /* 16: sun sampling at diffuse bounces, rules S1 - S9 at the end of this file (8 is unassigned and refused) */

typedef struct srt_radiance_params { /* 24 bytes */
    uint32_t first_sample;           /* f0 >= 1 */
    uint32_t sample_count;           /* n, 1..4096, f0 + n - 1 <= 2^32 - 1 */
    int32_t max_bounces;             /* MAXBOUNCES, >= 0 */
    uint32_t seed;
    uint32_t id_base;                /* ray i draws from the stream of "pixel" id_base + i (mod 2^32) */
    uint32_t flags;                  /* SRT_RADIANCE_* */
} srt_radiance_params;

typedef struct srt_radiance_work {
    uint32_t valid, reserved; /* 1, 0 */
    uint64_t rays, samples;   /* N; N * n */
    uint64_t closest_calls;   /* lane-level GetClosestObject calls by srt_stats.rays' rule: the primary counts once PER SAMPLE */
    uint64_t wave_calls;      /* wave-level closest-hit invocations the launch executed, primaries included */
} srt_radiance_work;

/* first_sample 1, sample_count 16, max_bounces 8, seed 0, id_base 0, flags SRT_RADIANCE_RESET (pure host, no device needed). */
int srt_radiance_params_default(srt_radiance_params* out);
int srt_trace_radiance(srt_context* ctx, const srt_radiance_params* params);
int srt_bind_radiance(srt_context* ctx, void* d_float4);
int srt_read_radiance(srt_context* ctx, float* dst_rgba);
int srt_get_radiance_work(srt_context* ctx, srt_radiance_work* out);

/* ---- adaptive sampling: per-pixel sample counts and a variance budget (ABI 7, backward compatible) -----------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of
 * them runs what it ran before, bit for bit.
 *
 * srt_render gives every pixel of a band the same number of samples.  srt_variance and srt_temporal_variance say which pixels
 * are still noisy; srt_sample_budget turns that variance into a per-pixel number of further samples and srt_render_adaptive
 * traces exactly those, continuing every pixel's running mean where it stands.
 *
 * Two per-pixel buffers, both W*H uint32 indexed x + y*W with the scene row y, like the accumulator; both the handle's own
 * (allocated on first use) or the caller's DEVICE buffer (srt_bind_*; NULL = own; does not wait, enqueued work keeps the buffer
 * it was given):
 *   sample counts  n_p: how many samples the accumulator element of pixel p holds;
 *   sample budget  b_p: how many more samples the next adaptive render may add to it.
 * srt_set_sample_counts fills the current counts buffer with one value, asynchronously on the launch stream: how a caller says
 * "I have just run srt_render with n samples".  srt_write_* wait like srt_write_accumulator, then copy W*H uint32 from the host;
 * srt_read_* wait, then copy to the host, and give SRT_ERR_STATE while the buffer has never been written, filled or bound.
 *
 * srt_render_adaptive.  Rules.
 * 1. Effective budget.  For every pixel p = (x, y) of the band (scene coordinates, id = x + y*W):
 *    e_p = min(b_p, max_samples, 2147483646 - n_p), and e_p = 0 when n_p >= 2147483646.  srt_render accepts frames up to
 *    2^31 - 2; this call never goes past them.
 * 2. Samples.  For f = n_p + 1 .. n_p + e_p: colour_f = RaytraceScene of the pixel's camera ray (GetRayDirection, no jitter), the
 *    path branch, drawn from srt_rng_key(seed, id, f) in srt_render's draw order, folded in ascending f with weight
 *    (float)(1.0 / f) into the accumulator element (SetScreenPixel's running mean).  When n_p = 0 sample 1 overwrites the
 *    element (setFrame); otherwise the mean continues from what the element holds.  There is no preview and there are no
 *    progressive blocks.
 * 3. Equivalence.  After any sequence of adaptive calls with one seed and bounce count that started from n_p = 0, pixel p's
 *    accumulator element equals the element srt_render writes with first_sample = 1, sample_count = n_p, SRT_RENDER_RESET, the
 *    same seed and bounces: in all four lanes (NaN as NaN), and the framebuffer pixel (tone_map, memory row H - 1 - y) is equal
 *    too — the scene in LDS or in memory, with or without meshes.  It also holds from a start of srt_render(1..n) followed by
 *    srt_set_sample_counts(n).
 * 4. Untouched pixels.  A pixel with e_p = 0 is not written: not its accumulator element, its framebuffer pixel or its count;
 *    no ray is traced for it.  A tile of 8 x 8 pixels that all have e_p = 0 costs the loads of its budgets and counts.
 * 5. Counts.  Without SRT_ADAPTIVE_KEEP_COUNTS, n_p += e_p.  With the flag the counts buffer is only read: for callers that keep
 *    several estimates of the same frame with equal counts (the two halves of srt_variance advanced in turn through
 *    srt_bind_output, the first call with the flag).  The budget buffer is never written.
 * 6. Determinism.  No atomic reaches accumulator, framebuffer or counts and the fold order per pixel is fixed: repeated calls
 *    from the same state give the same bits, whatever order the tiles run in.
 * 7. Asynchrony and captured state.  Asynchronous on the launch stream behind earlier work; srt_wait / srt_poll cover it.
 *    Scene, environment and camera are captured at enqueue; accumulator and framebuffer are those current at enqueue
 *    (srt_bind_output), the counts and budget buffers likewise.
 * 8. What it leaves alone.  srt_get_stats, srt_get_work_counts, the launch shape and dispatch order of later renders, the
 *    G-buffer, every pass buffer, the temporal history, the ray and radiance outputs.
 * 9. Errors, all found before anything is touched: SRT_ERR_STATE before srt_set_scene and srt_set_camera; SRT_ERR_INVALID_ARG
 *    for an empty or out-of-range band, unknown flags, reserved != 0, max_samples outside 1..4096 or a negative max_bounces;
 *    SRT_ERR_STATE when counts or budget have never been written, filled or bound.
 * 10. Work counts.  With SRT_ADAPTIVE_COUNT_WORK the launch counts, deterministically: its pixels (those with e_p > 0), its
 *    samples (the sum of e_p), the lane-level GetClosestObject calls by srt_stats.rays' rule (the primary counts once PER
 *    SAMPLE, although the kernel traces it once per pixel) and the wave-level closest-hit invocations it executed, primaries
 *    included: a wave traces a tile's primaries in one invocation and packs the bounce rays of its pixels' samples, 64 to an
 *    invocation.  Summed per wave and added with one vector atomic per wave into a handle-owned record; srt_get_adaptive_work
 *    waits and copies it, SRT_ERR_STATE unless the last srt_render_adaptive counted.
 *
 * srt_sample_budget.  Inputs: v = the current variance buffer, n = the counts, c = the accumulator's rgb, o = SRT_GBUF_OBJECT
 * and, with SRT_BUDGET_ALBEDO, a = SRT_GBUF_ALBEDO; all bound or own, the pass renders no guide.  Binary32 without FMA, in
 * this order:
 *   1. o_p = -1 or n_p = 0: b_p = 0.  A primary miss is exactly converged after one sample; a pixel without samples has no
 *      variance: seed the frame with a uniform render.
 *   2. g_p = the 3 x 3 prefiltered variance of srt_denoise_variance rule A at level 0 (the same device function): a two-half
 *      variance is far too noisy to use raw.
 *   3. m_p and l_p = lum(c_p / m_p) as srt_variance rules 2-3 (no division without the flag); t = threshold * (l_p + floor);
 *      T = t * t.
 *   4. if !(g_p > T): b_p = 0.  Otherwise r = g_p / T (IEEE division), e = (float)n_p * r - (float)n_p, and b_p = max_budget
 *      when !(e < (float)max_budget), else max(1, (uint32)ceilf(e)).  The variance of a mean falls as 1/n: n_p * r is the count at
 *      which g_p would reach T.
 *   5. output: the current budget buffer.  The sum of all b_p goes to a handle-owned uint64 (one integer vector atomic per
 *      wave, zeroed before the launch); srt_get_budget_total waits and returns it: what the next adaptive render will cost.
 *      SRT_ERR_STATE before the first srt_sample_budget.
 *   6. whole frame, one launch; asynchronous; it leaves alone what srt_variance leaves alone, and the variance, the counts and
 *      the accumulator as well.
 *   7. SRT_ERR_INVALID_ARG for a NaN or non-positive threshold (+inf is allowed), a NaN or negative floor, max_budget outside
 *      1..4096 or unknown flags; SRT_ERR_STATE for a missing guide, variance or counts buffer, and when the variance buffer is
 *      the handle's own and the pass that wrote it disagrees with this call on the ALBEDO flag.
 * n_p and b_p are in the unit of the counts buffer.  In the two-half workflow v is the variance of the mean of the halves, n
 * the per-half count and b the per-half extra:
 *     srt_render(RESET, seed sA, n) -> half A; srt_bind_output(ctx, NULL, half); srt_render(RESET, seed sB, n) -> half B
 *     srt_set_sample_counts(n); srt_render_gbuffer (once)
 *     per round: srt_bind_output(ctx, NULL, NULL); srt_variance(no MERGE); srt_sample_budget;
 *                srt_render_adaptive(seed sA, KEEP_COUNTS); srt_bind_output(ctx, NULL, half); srt_render_adaptive(seed sB)
 *     after the last round: srt_bind_output(ctx, NULL, NULL); srt_variance(MERGE)
 * A and B are seeded differently throughout. */
#define SRT_ADAPTIVE_KEEP_COUNTS 1u /* do not write the counts back */
#define SRT_ADAPTIVE_COUNT_WORK 2u  /* fill srt_adaptive_work for this call */
#define SRT_ADAPTIVE_SUN_SAMPLING 0x10u /* 16: sun sampling at diffuse bounces, rules AS1 - AS8 at the end of this file (4 and 8 are unassigned and refused) */
#define SRT_BUDGET_ALBEDO 1u        /* the luminance of the demodulated colour: must agree with the variance buffer */

typedef struct srt_adaptive_params { /* 28 bytes */
    int32_t row_begin, row_end;      /* memory rows, as srt_render_params */
    int32_t max_bounces;             /* MAXBOUNCES, >= 0 */
    uint32_t seed;
    uint32_t max_samples;            /* 1..4096: cap on what one call adds to a pixel */
    uint32_t flags;                  /* SRT_ADAPTIVE_* */
    uint32_t reserved;               /* 0 */
} srt_adaptive_params;

typedef struct srt_adaptive_work {
    uint32_t valid, reserved;  /* 1, 0 */
    uint64_t pixels, samples;  /* pixels with e_p > 0; the sum of e_p */
    uint64_t closest_calls;    /* lane-level GetClosestObject calls by srt_stats.rays' rule: the primary counts once PER SAMPLE */
    uint64_t wave_calls;       /* wave-level closest-hit invocations the launch executed, primaries included */
} srt_adaptive_work;

typedef struct srt_budget_params { /* 16 bytes */
    float threshold;               /* tau > 0 (+inf allowed): target relative standard error */
    float floor;                   /* >= 0: added to the luminance so that dark pixels do not ask for everything */
    uint32_t max_budget;           /* 1..4096 */
    uint32_t flags;                /* 0 or SRT_BUDGET_ALBEDO */
} srt_budget_params;

int srt_set_sample_counts(srt_context* ctx, uint32_t value);
int srt_write_sample_counts(srt_context* ctx, const uint32_t* src);
int srt_read_sample_counts(srt_context* ctx, uint32_t* dst);
int srt_bind_sample_counts(srt_context* ctx, void* d_u32);
int srt_write_sample_budget(srt_context* ctx, const uint32_t* src);
int srt_read_sample_budget(srt_context* ctx, uint32_t* dst);
int srt_bind_sample_budget(srt_context* ctx, void* d_u32);
/* max_bounces 8, seed 0, max_samples 4096, flags 0; the band is left to the caller (0, 0).  Pure host, no device needed. */
int srt_adaptive_params_default(srt_adaptive_params* out);
int srt_render_adaptive(srt_context* ctx, const srt_adaptive_params* params);
int srt_get_adaptive_work(srt_context* ctx, srt_adaptive_work* out);
/* threshold 0.05, floor 0.01, max_budget 64, flags SRT_BUDGET_ALBEDO: picks, not swept.  Pure host, no device needed. */
int srt_budget_params_default(srt_budget_params* out);
int srt_sample_budget(srt_context* ctx, const srt_budget_params* params);
int srt_get_budget_total(srt_context* ctx, uint64_t* total);

/* ---- reflection guides: first-hit buffers traced through mirror chains (ABI 7, backward compatible) ---------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of
 * them runs what it ran before, bit for bit.
 *
 * The first-hit buffers steer every post-process, and they cannot see reflected geometry: a mirror is filtered as one object.
 * For a material with smoothness = specular_amount = 1 the path tracer has no randomness at the bounce (the specular lottery
 * always succeeds and Lerp(random, reflected, 1) is the reflected ray), so the chain of mirror hits behind a pixel is the same in
 * every sample and all of the pixel's noise is made at the first NON-mirror surface at the end of it.  That surface's object,
 * normal, point and albedo are the right guides, and srt_render_reflection_gbuffer computes them once per camera.
 *
 * 1. Definition.  Binary32 without contraction.  For every pixel (x, y) of the band:
 *    Start.     Ray 0 is the camera ray of srt_render_gbuffer, srt_pick and srt_render's primary: camera.position and
 *               GetRayDirection(camera, x, y).  h_j = GetClosestObject of ray j: the closest_hit, scene image, instantiation and
 *               tie rule of srt_render_gbuffer, meshes included.
 *    Continue.  While ray j hits, j < max_bounces, and the hit object's material has smoothness >= min_smoothness &&
 *               specular_amount >= min_specular (a NaN comparison fails), with d the direction of ray j, n and p the normal and
 *               point of h_j:
 *                 k  = 2 * ((d.x*n.x + d.y*n.y) + d.z*n.z)
 *                 r  = (d.x - n.x*k, d.y - n.y*k, d.z - n.z*k)                 float3::Reflect, Common.hpp:163-165
 *                 d' = float3::Normalized(r)                                   sqrtf((x*x + y*y) + z*z), three IEEE divisions, :176
 *                 o' = (p.x + n.x*.00001f, p.y + n.y*.00001f, p.z + n.z*.00001f)   :177
 *    Stop.      J is the index of the last ray traced.  The chain either ends on an object (h_J is the terminal hit) or leaves
 *               the scene (ray J misses).
 *    Defaults.  min_smoothness = min_specular = 1, max_bounces = 8.  At those thresholds ray j + 1 is the bounce ray srt_render
 *               traces from h_j in every sample; the only possible difference is the sign of a zero component, which
 *               Lerp(a, b, 1) = a*0 + b may change.
 *    Wider.     Lower thresholds follow the mirror direction of glossy surfaces as an approximation; +inf thresholds or
 *               max_bounces = 0 follow nothing.
 * 2. Outputs, W*H elements each, indexed x + y*W with the scene row y, one bit each.  The first four have the element types of
 *    the SRT_GBUF_* table, so a buffer of one can be bound with srt_bind_gbuffer:
 *                                         chain ends on an object                      chain leaves the scene
 *      SRT_REFL_OBJECT         int32      list index of the terminal object            -1
 *      SRT_REFL_NORMAL_DEPTH   float4     terminal normal xyz, w = D                   (0, 0, 0, +inf)
 *      SRT_REFL_POSITION       float4     terminal point, w = 1                        (0, 0, 0, 0)
 *      SRT_REFL_ALBEDO         float4     throughput x terminal base colour, w = 0     (0, 0, 0, 0)
 *      SRT_REFL_BOUNCES        int32      J                                            J
 *    D is the path length ((t_0 + t_1) + ...) + t_J, summed in ascending order from the distances GetClosestObject reports: what
 *    the plane edge-stops should scale by.
 *    ALBEDO: colours are the ones the scene image holds (clamped at 0 like Color's constructor).  Per channel
 *      T = base_0;  for j = 1 .. J: { if (j >= 2) T = T * 0.8f;  if (j < J) T = T * specular_j; }
 *      albedo = J == 0 ? base_0 : T * base_J
 *    which follows hitColor of Raytracer.cpp:163-184 along the chain — the dissipation from the second bounce on and the mirror's
 *    Lerp(base, specular, 1) — with the base colour at the terminal, as SRT_GBUF_ALBEDO has it.
 *    Identity: for J = 0 every one of the four guide outputs equals the SRT_GBUF_* output bit for bit.
 * 3. Band, stream and asynchrony are srt_render_gbuffer's: the band is given in memory rows, only scene rows
 *    [H - row_end, H - row_begin) are written; scene, meshes and camera are captured at enqueue; srt_wait / srt_poll cover it.
 * 4. What it leaves alone: the framebuffer, the accumulator, the G-buffer slots, every pass buffer, srt_get_stats,
 *    srt_get_work_counts and the launch shape of later renders.
 * 5. Determinism.  No atomics reach the outputs; each pixel is written once and its value does not depend on how the kernel packs
 *    its work.
 * 6. Buffers.  The handle's own (allocated on first use) or the caller's: srt_bind_reflection binds ONE output (a single bit) to a
 *    DEVICE buffer of W*H elements (NULL = own; does not wait, enqueued launches keep the buffer they were given).
 *    srt_read_reflection waits, then copies the whole W*H buffer of ONE output to host memory under srt_read_gbuffer's rule:
 *    SRT_ERR_STATE when that output has neither been bound nor written yet.  srt_device_reflection gives the address of the
 *    handle's OWN buffer of one output, allocated (and zeroed) on first use, as srt_device_half: this is how the four guide outputs
 *    are handed to srt_bind_gbuffer, after which srt_denoise, srt_denoise_variance, srt_variance and srt_sample_budget are steered
 *    by the reflected geometry.  srt_temporal_accumulate reprojects with first hits, and through the chains
 *    only with the mirror history on (the block below), which reads four of these outputs next to the first hits.
 * 7. Errors, all found before anything is touched, in this order: SRT_ERR_STATE before srt_set_scene and srt_set_camera;
 *    SRT_ERR_INVALID_ARG for an empty or out-of-range band, outputs == 0 or unknown output bits, unknown flags, reserved != 0,
 *    max_bounces outside 0..64, a NaN threshold.
 * 8. Work counts.  With SRT_REFL_COUNT_WORK the launch counts, deterministically on a given device: the pixels of the band, the
 *    reflections (the sum of J over them), the wave-level closest-hit invocations and the waves that ran at least one.  Per-wave
 *    sums, one vector atomic per wave into a handle-owned record zeroed before the launch; without the flag there are no
 *    atomics at all.  The kernel keeps its lanes filled from a stream of pixel slots, so
 *      wave_calls <= (64 * tiles + reflections) / 64 + waves * (max_bounces + 1)
 *    with tiles = the 8 x 8 tiles that meet the band.  srt_get_reflection_work waits and copies the record of the last
 *    srt_render_reflection_gbuffer; SRT_ERR_STATE unless that call had SRT_REFL_COUNT_WORK (or when there has been none). */
#define SRT_REFL_OBJECT 1u
#define SRT_REFL_NORMAL_DEPTH 2u
#define SRT_REFL_POSITION 4u
#define SRT_REFL_ALBEDO 8u
#define SRT_REFL_BOUNCES 16u
#define SRT_REFL_GUIDES 15u    /* the four outputs that have SRT_GBUF_* element types */
#define SRT_REFL_ALL 31u
#define SRT_REFL_COUNT_WORK 1u /* flags: fill srt_reflection_work for this call */

typedef struct srt_reflection_params {  /* 32 bytes */
    int32_t row_begin, row_end;         /* memory rows, as srt_gbuffer_params */
    uint32_t outputs;                   /* SRT_REFL_* bits, at least one */
    uint32_t flags;                     /* 0 or SRT_REFL_COUNT_WORK */
    int32_t max_bounces;                /* 0..64 */
    float min_smoothness, min_specular; /* not NaN; +inf allowed */
    uint32_t reserved;                  /* 0 */
} srt_reflection_params;

typedef struct srt_reflection_work { /* 40 bytes */
    uint32_t valid, reserved;        /* 1, 0 */
    uint64_t pixels, reflections;    /* pixels of the band; the sum of J over them */
    uint64_t wave_calls, waves;      /* wave-level closest-hit invocations; waves that ran at least one */
} srt_reflection_work;

/* outputs SRT_REFL_ALL, flags 0, max_bounces 8, min_smoothness 1, min_specular 1; the band is left to the caller (0, 0).  Pure
 * host, no device needed. */
int srt_reflection_params_default(srt_reflection_params* out);
int srt_render_reflection_gbuffer(srt_context* ctx, const srt_reflection_params* params);
int srt_bind_reflection(srt_context* ctx, uint32_t output, void* d_ptr);
int srt_read_reflection(srt_context* ctx, uint32_t output, void* dst);
int srt_device_reflection(srt_context* ctx, uint32_t output, void** d_ptr);
int srt_get_reflection_work(srt_context* ctx, srt_reflection_work* out);

/* ---- mirror history: temporal reprojection through mirror chains, by the reflection guides (ABI 7, backward compatible) -------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7, srt_temporal_params keeps its 20 bytes
 * and there is no new SRT_TEMPORAL_* bit.  A sequence of calls that uses none of them runs what it ran before, bit for bit.
 *
 * srt_temporal_accumulate reprojects first hits, so a mirror's pixels carry their history along the mirror's surface while the
 * image in the mirror moves differently: reflections lag and smear.  The mirror history is a per-context mode, off by default.
 * With it on a pixel whose camera ray goes through J >= 1 mirrors (srt_render_reflection_gbuffer's chain) is reprojected by the
 * virtual image of the surface at the END of its chain, accepts a history tap only if that tap looked through the same mirror
 * over a chain of the same length at nearly the same terminal point, and otherwise restarts.  It never smears.
 * With the mode off every call runs the kernels it ran before.  With the mode on and no pixel with J >= 1 the results are bit for
 * bit those of the mode off.
 *
 * Definition.  Binary32 without contraction.  Steps 1-7 of the temporal block and 2'-6' of the moving-objects block stand; with
 * the mode on they change as follows.
 * Inputs.  The G-buffer slots OBJECT, NORMAL_DEPTH, POSITION must hold FIRST hits, as before: per pixel m_p, t0_p (the w of
 *      NORMAL_DEPTH) and x0_p.  Four reflection outputs are needed besides, bound or own: SRT_REFL_OBJECT, NORMAL_DEPTH, POSITION
 *      and BOUNCES give J_p and, for J_p >= 1, the terminal o_p, n_p, D_p (the w) and x_p.  SRT_ERR_STATE when one of the four has
 *      neither been bound nor written, or is the handle's own and was last rendered with a camera other than the current one
 *      (bound ones cannot be checked, as the G-buffer's).
 *  M1. tags: tag_p = 0 for J_p = 0, tag_p = J_p * 32768 + m_p for J_p >= 1 (object indices are < 32768, J <= 64).  The stored
 *      history keeps tag_p as int bits in the w of its normal row, a word that is 0 without the mode.
 *  M2. pixels with J_p = 0 (first-hit misses included) are handled exactly as before, from the G-buffer slots alone, with one
 *      more test: a tap q counts only when tag'_q == 0.  In a frame without mirrors every tag is 0 and nothing changes.
 *  M3. pixels with J_p >= 1 and o_p == -1 (the chain leaves the scene: reflected sky, the same value in every sample) have no
 *      history: c_p is kept bit for bit, L_p = n.  They are stored with object -1, so they are never taps; colour row (c_p, n).
 *  M4. pixels with J_p >= 1 and o_p >= 0.  C is the current camera's position,
 *      rho = (float)((double)radius_pixels * 2 * tan(fov_degrees * pi / 360) / H), the angle of radius_pixels pixels, computed
 *      once per call on the host, and r_p = rho * D_p.  Two candidates are tried in order:
 *        candidate 1:  y = C + (x0_p - C) * (D_p / t0_p) per component — the virtual point, the mirror image of the terminal
 *                      point for a flat mirror;
 *        candidate 2:  y = x0_p — the mirror's own surface (a strongly curved mirror keeps the image near its surface).
 *      For each: step 2 applied to y, the window test, the 2x2 footprint of step 3.  A tap counts when it lies inside the frame,
 *      its bilinear weight is > 0, o'_q == o_p, tag'_q == tag_p, ((dx*dx + dy*dy) + dz*dz) <= r_p * r_p with d = x'_q - x_p (the
 *      ball replaces the plane test; written so that a NaN fails) and step 3's normal test holds against the terminal normal n_p.
 *      The first candidate whose counted weights sum to W > 0 is blended by step 4; the second is not evaluated then.  With no
 *      such candidate c_p is kept and L_p = n.  The stored history is (result, L), (x_p, o_p), (n_p, tag_p).
 *  M5. moving objects: when the call uses a displacement table (some delta non-zero or some keep = 0), a pixel with J_p >= 1 has
 *      no history for this call — the chain's inner objects are not recorded, so their motion cannot be undone.  Its history is
 *      still stored per M3 / M4.  Pixels with J_p = 0 follow 2'-6' unchanged.
 *  M6. motion output: (u - x, v - y, W, 0) of the candidate that was blended; when neither counted a tap, candidate 1's (u, v)
 *      under the rule of the moving-objects block and W = 0; (0, 0, 0, 0) for a pixel of M3 or M5.  The moments history rides the
 *      taps the colour blend counted, as before.
 *  M7. whole frame, one launch, no atomics: the same sequence of calls gives the same bits.
 * Not covered: refraction; glossy surfaces below the reflection pass's thresholds; chains whose inner objects move; a search
 * beyond the two candidates.
 *
 * srt_mirror_history sets the mode and the radius.  SRT_ERR_INVALID_ARG for enabled outside 0..1, a radius that is NaN or <= 0,
 * non-zero flags or reserved; the previous setting then stands.  Changing `enabled` drops the colour history and the moments
 * history — the next srt_temporal_accumulate behaves as with SRT_TEMPORAL_RESET — because a history written under one mode
 * carries or lacks the tags the other relies on.  Changing only the radius keeps the history.  It touches no device memory and
 * launches nothing. */
typedef struct srt_mirror_history_params { /* 16 bytes */
    int32_t enabled;                       /* 0 or 1 */
    float radius_pixels;                   /* > 0, +inf allowed (the distance test always passes), NaN refused */
    uint32_t flags;                        /* 0 */
    uint32_t reserved;                     /* 0 */
} srt_mirror_history_params;

/* enabled 1, radius_pixels 2.  Pure host, no device needed. */
int srt_mirror_history_params_default(srt_mirror_history_params* out);
int srt_mirror_history(srt_context* ctx, const srt_mirror_history_params* params);

/* ---- buffers the worker writes ------------------------------------------------- */
/* Copies memory rows [row_begin,row_end) into dst (dst points at row_begin's first
 * pixel), pitch_bytes per row (>= 4*W) — the renderSurface->pixels layout (:64). Waits. */
int srt_read_framebuffer(srt_context* ctx, void* dst, size_t pitch_bytes, int row_begin, int row_end);
/* The same copy without the wait: enqueued on `copy_stream` (a hipStream_t of the caller's; NULL = the handle's launch stream)
 * behind every render enqueued on the handle so far, then the call returns.  dst must stay valid — and should be pinned host memory,
 * or the copy is not asynchronous — until the caller has synchronised copy_stream.  With two device framebuffers bound in turn
 * (srt_bind_output, which does not wait) frame k travels to the host while frame k + 1 renders: the blit of Raytracer.cpp:549-556
 * off the critical path (bench.py `readback`: 0.155 ms per 1080p frame hidden, +1.5 % per step instead of +6.9 %). */
int srt_read_framebuffer_async(srt_context* ctx, void* dst, size_t pitch_bytes, int row_begin, int row_end, void* copy_stream);
/* colorBuffer (:60): W*H float4 (r,g,b,a), index x + y*W, scene rows. Wait + copy. */
int srt_read_accumulator(srt_context* ctx, float* dst_rgba);
int srt_write_accumulator(srt_context* ctx, const float* src_rgba);

/* ---- light probes: SH-projected path-traced radiance at probe points (ABI 7, backward compatible) ------------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of
 * them runs what it ran before, bit for bit.
 *
 * srt_trace_radiance says how much light arrives along a ray.  A light probe wants that for K directions around each of P
 * points and keeps nine spherical-harmonics coefficients per point.  srt_trace_light_probes forms the P*K rays on the device
 * from P positions and K shared directions, path-traces them with srt_trace_radiance's sample semantics and projects each
 * probe's K radiances onto the real SH basis of bands 0..2 in a fixed summation order: 16 * (P + K) bytes go up, 144 * P bytes
 * come back, and nothing of size P*K exists in memory unless the caller asks for the RADIANCE output.
 *
 * Rules.
 * 1. Inputs.  P probe positions (srt_write_light_probes copies them from the host and waits like srt_write_rays;
 *    srt_bind_light_probes binds a DEVICE array, does not wait and does not copy; NULL, 0 returns to the own array): float4, xyz
 *    used, w ignored, 1 <= P <= 2^30.  K directions shared by all probes (srt_write_light_probe_directions,
 *    srt_bind_light_probe_directions, the same way): float4, xyz = direction, w = quadrature weight (solid angle),
 *    1 <= K <= 4096.  P*K <= 2^30, srt_trace_radiance's batch limit.  Finite positions with unit directions and finite weights are
 *    pinned bit for bit; other inputs give some value and do not fault.
 * 2. Ray (p, k).  Origin = position_p; direction = d_k, or float3::Normalized(d_k) with SRT_LIGHT_PROBE_NORMALIZE, as
 *    SRT_RADIANCE_NORMALIZE (the weight passes through unscaled); ray id = id_base + p*K + k (mod 2^32).  Its radiance L_{p,k}
 *    is by definition element p*K + k of what srt_trace_radiance writes for the explicit batch of those rays with the same
 *    first_sample, sample_count, max_bounces, seed, id_base and RESET: rules 2, 3 and 5 of that block, all four lanes, the
 *    alpha-NaN rule included.
 * 3. Basis.  Evaluated on the direction as traced (x, y, z), in binary32 without contraction, in exactly this order:
 *      b0 = 0.282095f                     b1 = 0.488603f*y                 b2 = 0.488603f*z
 *      b3 = 0.488603f*x                   b4 = 1.092548f*(x*y)             b5 = 1.092548f*(y*z)
 *      b6 = 0.315392f*((3.0f*(z*z)) - 1.0f)   b7 = 1.092548f*(x*z)         b8 = 0.546274f*((x*x) - (y*y))
 * 4. Term.  t_c = w_k * b_c, and the lane value v = (L.r*t_c, L.g*t_c, L.b*t_c, t_c).  The fourth lane is the projection of the
 *    constant 1: a caller can renormalise an imperfect direction set with it.
 * 5. Sum order.  Directions are taken in blocks j of 64, k = 64j + l; positions l with k >= K contribute +0.0f in all four
 *    lanes.  Within a block a pairwise tree of six levels, v'[m] = v[2m] + v[2m+1]; across blocks S = B_0, then S = S + B_j for
 *    j = 1, 2, ... ascending.  out[p*9 + c] = S, a float4: nine float4 per probe.  No atomics reach any output: repeated calls
 *    give the same bits.
 * 6. Outputs, a bit mask as the G-buffer's: SRT_LIGHT_PROBE_COEFFICIENTS, P*9 float4, and SRT_LIGHT_PROBE_RADIANCE, the P*K
 *    float4 running means L_{p,k} (element p*K + k), optional.  Each is the handle's own buffer (allocated on first use, grown
 *    when a call needs more) or the caller's: srt_bind_light_probe_output binds a DEVICE buffer, NULL = own, under
 *    srt_bind_ray_output's rules.  Without RADIANCE nothing of size P*K is allocated.  srt_read_light_probe_output waits, then
 *    copies what the last srt_trace_light_probes wrote of that output, from the buffer it wrote; SRT_ERR_STATE when the last trace
 *    did not write it.
 * 7. RESET.  Without SRT_LIGHT_PROBE_RESET the means continue from the RADIANCE buffer, as srt_trace_radiance's rule 3.  That
 *    needs the RADIANCE output and a previous srt_trace_light_probes of the same P and K into the buffer now bound (or the own
 *    one); otherwise the call returns SRT_ERR_STATE.
 * 8. Asynchrony.  As rule 7 of the radiance block; positions, directions and output buffers are those current at enqueue.
 * 9. What it leaves alone.  Everything srt_trace_radiance leaves alone, and the ray batch of srt_write_rays / srt_bind_rays, the
 *    radiance output and its "last trace" record, and the accumulator as well.
 * 10. Errors, all found before anything is touched: SRT_ERR_STATE before srt_set_scene; SRT_ERR_INVALID_ARG for unknown flags or
 *    outputs, outputs == 0, first_sample == 0, sample_count outside 1..4096, first_sample + sample_count - 1 > 2^32 - 1, a
 *    negative max_bounces or a non-zero reserved; SRT_ERR_STATE with no positions or no directions; SRT_ERR_INVALID_ARG for K
 *    outside 1..4096 or P*K > 2^30; SRT_ERR_STATE by rule 7.  SRT_ERR_OOM when a buffer cannot be had.
 * 11. Work counts.  With SRT_LIGHT_PROBE_COUNT_WORK the launch counts, deterministically: its probes, its rays (P*K), its
 *    samples (P*K*n), the lane-level GetClosestObject calls by srt_stats.rays' rule and the wave-level closest-hit invocations, as
 *    srt_radiance_work, and the waves of the launch.  One vector atomic per wave at the end; without the flag there are no atomics
 *    at all.  srt_get_light_probe_work waits and copies the record of the last srt_trace_light_probes; SRT_ERR_STATE unless that
 *    trace had the flag. */
#define SRT_LIGHT_PROBE_RESET 1u      /* sample first_sample overwrites the means; without it they continue from the RADIANCE buffer */
#define SRT_LIGHT_PROBE_NORMALIZE 2u  /* as SRT_RADIANCE_NORMALIZE */
#define SRT_LIGHT_PROBE_COUNT_WORK 4u /* fill srt_light_probe_work for this call */
#define SRT_LIGHT_PROBE_SUN_SAMPLING 0x10u /* 16: srt_trace_light_probes and srt_trace_light_probes_listed, rules S1 - S9 (8 is refused) */
#define SRT_LIGHT_PROBE_COEFFICIENTS 1u /* output: P*9 float4 */
#define SRT_LIGHT_PROBE_RADIANCE 2u     /* output: P*K float4 */
#define SRT_LIGHT_PROBE_MAX_DIRECTIONS 4096u

typedef struct srt_light_probe_params { /* 32 bytes */
    uint32_t first_sample;              /* f0 >= 1 */
    uint32_t sample_count;              /* n, 1..4096, f0 + n - 1 <= 2^32 - 1 */
    int32_t max_bounces;                /* MAXBOUNCES, >= 0 */
    uint32_t seed;
    uint32_t id_base;                   /* ray (p, k) draws from the stream of "pixel" id_base + p*K + k (mod 2^32) */
    uint32_t flags;                     /* SRT_LIGHT_PROBE_RESET | _NORMALIZE | _COUNT_WORK */
    uint32_t outputs;                   /* SRT_LIGHT_PROBE_COEFFICIENTS | _RADIANCE, not 0 */
    uint32_t reserved;                  /* 0 */
} srt_light_probe_params;

typedef struct srt_light_probe_work { /* 56 bytes */
    uint32_t valid, reserved;         /* 1, 0 */
    uint64_t probes, rays, samples;   /* P; P*K; P*K*n */
    uint64_t closest_calls;           /* lane-level GetClosestObject calls by srt_stats.rays' rule: the primary counts once PER SAMPLE */
    uint64_t wave_calls;              /* wave-level closest-hit invocations the launch executed, primaries included */
    uint64_t waves;                   /* waves of the launch */
} srt_light_probe_work;

int srt_write_light_probes(srt_context* ctx, const float* positions, size_t count);
int srt_bind_light_probes(srt_context* ctx, const void* d_positions, size_t count);
int srt_write_light_probe_directions(srt_context* ctx, const float* directions, size_t count);
int srt_bind_light_probe_directions(srt_context* ctx, const void* d_directions, size_t count);
/* first_sample 1, sample_count 16, max_bounces 8, seed 0, id_base 0, flags SRT_LIGHT_PROBE_RESET, outputs
 * SRT_LIGHT_PROBE_COEFFICIENTS, reserved 0 (pure host, no device needed). */
int srt_light_probe_params_default(srt_light_probe_params* out);
int srt_trace_light_probes(srt_context* ctx, const srt_light_probe_params* params);
int srt_bind_light_probe_output(srt_context* ctx, uint32_t output, void* d_ptr);
int srt_read_light_probe_output(srt_context* ctx, uint32_t output, void* dst);
int srt_get_light_probe_work(srt_context* ctx, srt_light_probe_work* out);
/* Pure host, no device: fills `count` float4 (count >= 1) with a spherical Fibonacci set.  For i = 0 .. count - 1, in double:
 * z = 1 - (2i + 1) / count, r = sqrt(1 - z*z), a = i * pi * (3 - sqrt(5)), (x, y) = (r cos a, r sin a); each component is rounded
 * once to binary32, and every weight is (float)(4 pi / count). */
int srt_light_probe_sphere(size_t count, float* dst);
/* Pure host, no device: the irradiance at a unit normal n from nine float4 coefficients, rgb[l] for l = 0, 1, 2 (the fourth lanes are
 * not read).  In binary32 without contraction: with b_c(n) as in rule 3 and A_0 = 3.14159274f (pi), A_1..3 = 2.09439516f (2 pi / 3),
 * A_4..8 = 0.785398185f (pi / 4), term_c = (A_c * coefficient_c[l]) * b_c(n); E = term_0, then E = E + term_c for c = 1 .. 8
 * ascending; rgb[l] = E. */
int srt_light_probe_irradiance(const float* coefficients, const float* normal, float* rgb);

/* ---- multi-GPU row stripes in ONE process -----------------------------
 * The reference splits a frame over 16 worker threads that write disjoint columns of one
 * surface (Raytracer.cpp:330-342); across GPUs the split is disjoint bands of MEMORY rows,
 * one context per GPU, and this call is the gather: it copies memory rows
 * [row_begin,row_end) of `src`'s framebuffer into the same rows of `dst`'s framebuffer,
 * device to device (a peer copy over xGMI when the two contexts live on different GPUs),
 * enqueued on src's stream behind its render; dst's stream is made to wait for it, so a
 * following srt_read_framebuffer(dst) sees the band.  Both contexts must have the same
 * width and height.  (Across PROCESSES the same gather is one RCCL collective:
 * software-raytracer_amd/stripes.py, bench.py --gpus N.) */
int srt_gather_band(srt_context* dst, srt_context* src, int row_begin, int row_end);
/* Which way `src`'s last srt_gather_band went, as text: the same device, a peer copy with peer access enabled (hipDeviceCanAccessPeer
 * is asked once per pair of devices), or a copy the runtime had to stage.  The cross-device ways have never run on this project's
 * one-GPU boxes; this is how the first multi-GPU run reports what it did.  The pointer stays valid until src is destroyed. */
const char* srt_gather_path(const srt_context* src);
/* Relative cost of every MEMORY row of the frame for the current scene and camera (row_costs[height], arbitrary
 * units), from a device-side probe: the path-trace kernel's own path pool, run over a quarter of the pixels for the
 * frame's first 32 samples, COUNTING what its loops do (pool steps, exactly tested sphere groups, BVH rounds, per-tile
 * work) instead of writing the frame; the counts are weighed into a cost.  Nothing of the frame is read or written.
 * Costs the work of 8 sample-frames on this device (32 samples on a quarter of the pixels: 1.6 % of a 512-spp launch of the
 * frame, a quarter of a 32-spp one) and a host round trip.  Counts, not times: deterministic — every process of a multi-GPU job computes the
 * same numbers, so the ranks can agree on cost-balanced row bands without talking to each other.  The reference's
 * static split into 16 equal column stripes (Raytracer.cpp:330-342) leaves its workers idle behind the slowest one;
 * equal ROW bands are worse (sky rows cost a tenth of floor rows).  Synchronous. */
int srt_estimate_row_costs(srt_context* ctx, int max_bounces, uint32_t seed, float* row_costs);

/* ---- probe-grid shading: per-pixel irradiance from a grid of light probes (ABI 7, backward compatible) ---------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of
 * them runs what it ran before, bit for bit.
 *
 * srt_trace_light_probes leaves nine SH coefficients per probe on the device.  srt_shade_probe_grid is the pass that uses them:
 * for probes on a regular grid it gives every pixel of a band the irradiance at its first hit — the eight probes around the point,
 * weighted trilinearly, optionally by how far each lies in front of the surface, and optionally only those the surface can see
 * (one any-hit query of srt_trace_occlusion per corner, on the device).  The output is W*H float4 (r, g, b, a), a = the sum of the
 * weights that survived: a == 0 says that no probe was usable.  The coefficient layout is exactly SRT_LIGHT_PROBE_COEFFICIENTS
 * (probe p's nine float4 at 9p .. 9p + 8), so a device buffer bound with srt_bind_light_probe_output can be bound here too and
 * nothing crosses the bus.
 *
 * Rules.  All arithmetic is binary32 without contraction.  Per pixel of the band, with o from SRT_GBUF_OBJECT, n from
 * SRT_GBUF_NORMAL_DEPTH.xyz and x from SRT_GBUF_POSITION.xyz (bound or own, as srt_render_visibility's rule 1), and albedo from
 * SRT_GBUF_ALBEDO only with SRT_PROBE_GRID_ALBEDO:
 * 1. Miss pixel (o == -1): out = (0, 0, 0, 0), and no other guide value is loaded.
 * 2. Cell, per axis a with n_a = counts[a]: m = (float)(n_a - 1); u = (x_a - origin_a) / spacing_a;
 *    u = !(u > 0) ? 0 : (u > m ? m : u), so a NaN gives 0; i = (int)u, lowered to n_a - 2 when i > n_a - 2 and n_a >= 2;
 *    f = u - (float)i.  An axis with n_a == 1 has i = 0 and f = 0.
 * 3. Corners c = 0 .. 7 with bits (cx, cy, cz) = (c & 1, (c >> 1) & 1, (c >> 2) & 1).  Per axis w_a = c_a ? f : (1.0f - f); the
 *    trilinear weight t = (w_x * w_y) * w_z.  A corner whose bit is set on an axis with n_a == 1 does not exist; it has w_a = f = 0
 *    and so weight 0.  A corner with !(t > 0) is skipped.
 * 4. Probe position p_a = origin_a + (float)(i_a + c_a) * spacing_a.  srt_probe_grid_positions computes the same expression, so
 *    the positions agree bit for bit.
 * 5. Segment to the probe.  O = (x.x + n.x * .00001f, x.y + n.y * .00001f, x.z + n.z * .00001f) as visibility rule 2; v = p - O;
 *    q = (v.x*v.x + v.y*v.y) + v.z*v.z; L = sqrtf(q).  If !(L > 0) the corner is skipped.  d = (v.x / L, v.y / L, v.z / L).
 * 6. Normal weight.  With SRT_PROBE_GRID_NORMAL_WEIGHT: h = (((d.x*n.x + d.y*n.y) + d.z*n.z) + 1.0f) * 0.5f and
 *    t = t * ((h*h) + 0.2f).
 * 7. Visibility.  With SRT_PROBE_GRID_VISIBILITY the segment (O, d, t_max = L) goes through the any-hit query, exactly as
 *    srt_trace_occlusion answers it for the scene captured at enqueue.  An occluded corner is skipped.  Corners skipped by rules
 *    3 and 5 are never traced.
 * 8. Corner irradiance.  With k = probe index (i_x + c_x) + n_x * ((i_y + c_y) + n_y * (i_z + c_z)), b_j(n) the basis of the
 *    light-probe block's rule 3 on the normal, A_0 = band_weight[0], A_1..3 = band_weight[1], A_4..8 = band_weight[2]:
 *    term_j = (A_j * coefficient[9k + j][l]) * b_j(n); e_c[l] = term_0, then e_c[l] = e_c[l] + term_j for j = 1 .. 8 ascending
 *    (srt_light_probe_irradiance's rule), for l = 0, 1, 2.  The fourth lanes of the coefficients are not read.
 * 9. Sum.  E[l] = +0.0f and T = +0.0f; then for c = 0 .. 7 ascending E[l] = E[l] + (t_c * e_c[l]) and T = T + t_c, where a skipped
 *    corner contributes +0.0f to each.  If T > 0: out = (E[0] / T, E[1] / T, E[2] / T, T), with r, g, b multiplied by albedo.rgb
 *    after the division with SRT_PROBE_GRID_ALBEDO.  Otherwise out = (0, 0, 0, 0): the caller sees a == 0 and can fall back, for
 *    instance to a second call without SRT_PROBE_GRID_VISIBILITY.
 * 10. Band weights.  The default (3.14159274f, 2.09439516f, 0.785398185f) are srt_light_probe_irradiance's constants: the
 *    cosine-weighted integral.  (1.0f, 0.5f, 0.0f) is the MEAN over the hemisphere around n, which is what this renderer's diffuse
 *    bounce averages, up to the non-uniformity of GetRandomDirection.
 * 11. Band.  As srt_gbuffer_params: a band is given in MEMORY rows and only scene rows [H - row_end, H - row_begin) of the output
 *    are written, indexed x + y*W with the SCENE row y.  Nothing outside the band is written.
 * 12. Grid and coefficients.  srt_set_probe_grid copies the grid; it refuses, with SRT_ERR_INVALID_ARG, counts < 1, a product
 *    nx*ny*nz > 2^30, a spacing that is NaN, infinite or <= 0 and a non-finite origin, and then leaves the previous grid.
 *    srt_write_probe_grid_coefficients copies probes * 9 float4 from the host into the handle's own array and waits, like
 *    srt_write_light_probes; srt_bind_probe_grid_coefficients binds a DEVICE array of probes * 9 float4, does not copy and does
 *    not wait; NULL, 0 returns to the own array.  1 <= probes <= 2^30.
 * 13. Output.  The handle's own buffer (allocated on first use) or the caller's: srt_bind_probe_grid_output binds a DEVICE buffer
 *    of W*H float4, NULL = own, under srt_bind_gbuffer's rules (does not wait, enqueued work keeps its buffer).
 *    srt_read_probe_grid_output waits, then copies the W*H float4 of the current buffer; SRT_ERR_STATE before the first
 *    srt_shade_probe_grid.
 * 14. Side effects.  Asynchronous on the launch stream behind earlier work; srt_wait / srt_poll cover it; grid, coefficients,
 *    guides and output are those current at enqueue.  The call leaves alone everything srt_render_visibility leaves alone, and
 *    the visibility outputs and the light-probe inputs, outputs and records as well.
 * 15. Pinned domain.  Guides written by srt_render_gbuffer, or bound guides with unit normals and finite points, with finite
 *    coefficients, are pinned bit for bit.  Other inputs give some value and do not fault: every probe index is clamped to the
 *    grid by construction, so no coefficient load can leave the array.
 * 16. Errors, all found before anything is touched, in this order: SRT_ERR_STATE before srt_set_scene; SRT_ERR_INVALID_ARG for an
 *    empty or out-of-range band, unknown flags, a non-zero reserved word or a NaN band_weight; SRT_ERR_STATE when there is no
 *    grid, when there are no coefficients, when OBJECT, NORMAL_DEPTH, POSITION or (with SRT_PROBE_GRID_ALBEDO) ALBEDO has never
 *    been bound or rendered, or when the current coefficient count is not nx*ny*nz.
 * 17. Work counts.  With SRT_PROBE_GRID_COUNT_WORK the launch counts, deterministically: the hit pixels; the corners that reach
 *    rule 7 (weight > 0 and L > 0, with or without the query); the segments traced and those with no occluder (both 0 without
 *    SRT_PROBE_GRID_VISIBILITY); the wave-level trips — a wave numbers the corners of its 8 x 8 tile's h hit pixels, in lane order,
 *    j = 8 * rank + c and serves 64 of them per trip, so a tile takes ceil(h / 8) trips; the lane-level tests of
 *    srt_occlusion_work; and the waves of the launch.  One vector atomic per wave at the end; without the flag there are no
 *    atomics at all.  srt_get_probe_grid_work waits and copies the record of the last srt_shade_probe_grid; SRT_ERR_STATE unless
 *    that call had the flag (or when there has been none). */
#define SRT_PROBE_GRID_VISIBILITY 1u    /* rule 7 */
#define SRT_PROBE_GRID_NORMAL_WEIGHT 2u /* rule 6 */
#define SRT_PROBE_GRID_ALBEDO 4u        /* rule 9: rgb times SRT_GBUF_ALBEDO.rgb */
#define SRT_PROBE_GRID_COUNT_WORK 8u    /* fill srt_probe_grid_work for this call */

typedef struct srt_probe_grid { /* 36 bytes */
    float origin[3];            /* position of probe (0,0,0) */
    float spacing[3];           /* > 0, finite */
    int32_t counts[3];          /* nx, ny, nz >= 1; nx*ny*nz <= 2^30; probe (ix,iy,iz) has index ix + nx*(iy + ny*iz) */
} srt_probe_grid;

typedef struct srt_probe_grid_params { /* 32 bytes */
    int32_t row_begin;                 /* first memory row (inclusive), as srt_gbuffer_params / srt_visibility_params */
    int32_t row_end;                   /* one past the last memory row */
    uint32_t flags;                    /* SRT_PROBE_GRID_VISIBILITY | _NORMAL_WEIGHT | _ALBEDO | _COUNT_WORK */
    float band_weight[3];              /* A for SH bands 0, 1, 2 (rule 10) */
    uint32_t reserved[2];              /* 0 */
} srt_probe_grid_params;

typedef struct srt_probe_grid_work { /* 80 bytes */
    uint32_t valid, reserved;        /* 1, 0 */
    uint64_t pixels;                 /* hit pixels of the band */
    uint64_t corners;                /* corners with weight > 0 and L > 0: those that reach the query */
    uint64_t segments, open;         /* segments traced; those with no occluder */
    uint64_t wave_trips;             /* sum over tiles of ceil(h / 8) */
    uint64_t analytic_tests;         /* as srt_occlusion_work */
    uint64_t node_visits;
    uint64_t triangle_tests;
    uint64_t waves;                  /* waves of the launch */
} srt_probe_grid_work;

/* Pure host, no device: fills nx*ny*nz float4 with the probe positions of rule 4 in index order, w = 0.  SRT_ERR_INVALID_ARG for
 * a grid srt_set_probe_grid would refuse. */
int srt_probe_grid_positions(const srt_probe_grid* grid, float* dst);
/* flags = 0, band_weight = (3.14159274f, 2.09439516f, 0.785398185f), reserved = 0; row_begin = row_end = 0: the band is the
 * caller's to fill (pure host, no device needed). */
int srt_probe_grid_params_default(srt_probe_grid_params* out);
int srt_set_probe_grid(srt_context* ctx, const srt_probe_grid* grid);
int srt_write_probe_grid_coefficients(srt_context* ctx, const float* coefficients, size_t probes);
int srt_bind_probe_grid_coefficients(srt_context* ctx, const void* d_ptr, size_t probes);
int srt_shade_probe_grid(srt_context* ctx, const srt_probe_grid_params* params);
int srt_bind_probe_grid_output(srt_context* ctx, void* d_float4);
int srt_read_probe_grid_output(srt_context* ctx, float* dst);
int srt_get_probe_grid_work(srt_context* ctx, srt_probe_grid_work* out);

/* ---- diagnostics ----------------------------------------------------------------- */
/* Self-test of the kernel's shortened arithmetic (csrc/srt_kernel.hip.h: float3::Normalized, the box slab slopes and the
 * accumulation weight 1 / frame without the rescaling and fix-up steps of the library sqrt / divide where those are
 * identities): `vectors` pseudo-random vectors — all magnitudes, zero and denormal components, infinities, NaNs — through
 * the short and the library path on the device, and 1 / frame for every frame up to 2^24 (vectors >= 2^24 covers them
 * all); the random direction's normalization without its window test on triples of draws (the 64 extreme combinations, then random
 * ones); the sphere test's short square root against sqrtf for the bit pattern of every vector index below 2^31 that lies in
 * its window (vectors >= 2^31 covers every float there); *mismatches = how many differ in any bit (must be 0).  Not part of the
 * reference's interface. */
int srt_selftest_arith(int device, uint32_t seed, uint64_t vectors, uint64_t* mismatches);

/* ---- probe cascades: shade from nested probe grids, blended at borders (ABI 7, backward compatible) ------------------------------
 * These calls were added without changing anything else, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of them
 * runs what it ran before, bit for bit.  A grid that follows the viewer is either fine and small — every point outside it is
 * clamped to its outer probe layer — or coarse and blurred.  A cascade is up to four grids around the same centre, level 0 the
 * finest; srt_shade_probe_cascade gives every pixel the irradiance of the finest level that holds its first hit, blended into the
 * next coarser level across a border band, in one pass on the device.  Each level has coefficients, and optionally depth moments
 * and state records, of its own; the handle's single grid (srt_set_probe_grid) and its arrays are neither read nor changed by the
 * shading.  The per-level pipeline (scroll, classify, list, trace, blend) runs through the single-grid calls, one level at a time;
 * srt_capture_probe_cascade_level then keeps that level's results.  All arithmetic is binary32 without contraction.
 * C1. Per-level evaluation.  For a level l, (I_l, T_l) is what the single-grid pass gives for the pixel on that level's grid,
 *    coefficients, moments and records: probe-grid rules 1 - 9, with rule 6 under SRT_PROBE_CASCADE_NORMAL_WEIGHT, rules 3s / 4s
 *    under _STATES and rule 7b under _DEPTH (with the call's bias and min_variance and the cascade's R); there is no any-hit query
 *    in this pass (rule 7 never applies).  The eight corners are added ascending (rule 9).  I_l = E / T and T_l = T when T > 0,
 *    otherwise the level is UNUSABLE.  Albedo is not applied here.
 * C2. Level weight beta_l(x), x = SRT_GBUF_POSITION.xyz.  Per axis a with n_a >= 2: u = (x_a - origin_a) / spacing_a (rule 2's
 *    expression before its clamp) and m = (float)(n_a - 1).  If !(u >= 0 && u <= m) on any such axis, beta_l = 0: a NaN or a point
 *    outside gives 0.  Otherwise e starts at +inf and on the axes x, y, z in order: g = m - u; ea = u < g ? u : g;
 *    e = ea < e ? ea : e.  beta_l = e >= blend_cells ? 1.0f : e / blend_cells.  Axes with n_a == 1 are ignored (a level of one
 *    probe has beta = 1 everywhere).  The FIRST LEVEL f is the lowest l with beta_l > 0, or levels - 1 when there is none: the
 *    coarsest level then serves the point through rule 2's clamp, as the single grid does.  If f == levels - 1 or beta_f >= 1 the
 *    pixel has ONE evaluation, level f.  Otherwise it has TWO: f with weight beta = beta_f and f + 1 with weight 1.0f - beta;
 *    level f + 1 is evaluated by C1 whatever its own beta is.  srt_probe_cascade_weights (pure host) is this rule for one point:
 *    it returns f, the number of evaluations and beta_f (0.0f when no level holds the point); SRT_ERR_INVALID_ARG for a cascade
 *    srt_set_probe_cascade would refuse.
 * C3. Combination.  One evaluation: out = (I_f, T_f), or zeros if unusable.  Two, both usable:
 *    out[l] = (beta * I_f[l]) + ((1.0f - beta) * I_f+1[l]) for l = 0, 1, 2 and a = (beta * T_f) + ((1.0f - beta) * T_f+1).  Two,
 *    one usable: that level's (I, T) unchanged.  None usable: (0, 0, 0, 0).  With SRT_PROBE_CASCADE_ALBEDO, r, g, b are multiplied
 *    by SRT_GBUF_ALBEDO.rgb last.  A miss pixel (OBJECT == -1) gets zeros and loads no other guide, as rule 1.  The band is rule
 *    11's: MEMORY rows in, scene rows written, nothing outside the band.
 * C4. Safety.  Every coefficient, moment and record index is built from cell indices clamped to [0, n_a - 1] per axis and from
 *    f, f + 1 <= levels - 1: no load can leave an array whatever the guides hold.  The pinned domain is rule 15's.
 * C5. Work counts.  With SRT_PROBE_CASCADE_COUNT_WORK the launch counts, deterministically: the hit pixels; the level evaluations
 *    (1 or 2 per hit pixel); the pixels with 2; per k the hit pixels whose first level is k; the corners live after rules
 *    3 / 3s / 5; with _DEPTH the corners whose weight stays > 0 after rule 7b (`open`, else 0); the wave-level trips — a wave
 *    numbers its 8 x 8 tile's evaluations in lane order of the hit pixels, a pixel's level f before its level f + 1, and serves
 *    eight evaluations (64 corner items) per trip, so a tile with Q evaluations takes ceil(Q / 8) trips; and the waves of the
 *    launch.  One vector atomic per wave at the end; without the flag there are no atomics at all.  srt_get_probe_cascade_work
 *    waits and copies the record of the last srt_shade_probe_cascade; SRT_ERR_STATE unless that call had the flag (or when there
 *    has been none).  The record is the cascade's own: srt_get_probe_grid_work answers what it answered before.
 * C6. The cascade and its arrays.  srt_set_probe_cascade copies the cascade; it refuses, with SRT_ERR_INVALID_ARG, levels outside
 *    1 .. 4, a resolution not in {0, 4, 8, 16}, a blend_cells that is NaN, infinite or <= 0, a non-zero reserved word and a level
 *    grid srt_set_probe_grid would refuse, and then leaves the previous cascade and all its arrays.  A level whose probe count
 *    nx*ny*nz changed (or that is new, or gone) loses its arrays' "present" marks, own and bound, and a changed resolution takes
 *    every level's moments; a level whose origin or spacing alone changed keeps them: the scroll case.  Per level and array
 *    (`which` is exactly one bit): srt_write_probe_cascade_level copies `probes` elements from the host into the handle's own
 *    array and waits, like srt_write_probe_grid_coefficients; srt_bind_probe_cascade_level binds a DEVICE array, does not copy and
 *    does not wait; NULL, 0 returns to the own array.  Elements: SRT_PROBE_CASCADE_COEFFICIENTS 9 float4, _MOMENTS R*R float4 of
 *    the cascade's resolution (SRT_ERR_INVALID_ARG when that is 0), _RECORDS one float4, in the single-grid layouts.  Both:
 *    SRT_ERR_STATE without a cascade; SRT_ERR_INVALID_ARG for level >= levels, a `which` that is not one bit, probes outside
 *    1 .. 2^30 or probes*R*R > 2^30.  srt_capture_probe_cascade_level copies, device to device on the launch stream and without
 *    waiting, what the single-grid calls would read right now — the current probe-grid coefficients, depth moments and state
 *    records, as selected by which_mask — into the level's OWN arrays, which become current (a binding of that array ends).
 *    SRT_ERR_STATE without a cascade; SRT_ERR_INVALID_ARG for level >= levels or an empty or unknown mask; SRT_ERR_STATE when there
 *    is no current grid, when its counts differ from the level's, when a selected source is absent or not of the level's P, or,
 *    for moments, when the current R differs from the cascade's; the level is then as it was.
 * C7. The call.  srt_shade_probe_cascade writes the probe-grid output slot (srt_bind_probe_grid_output,
 *    srt_read_probe_grid_output serve it, as for the depth and states calls).  Asynchronous on the launch stream; cascade, arrays,
 *    guides and output are those current at enqueue.  It leaves alone everything srt_shade_probe_grid_states leaves alone, and
 *    the single grid, its bindings and its "last call" record as well.  Errors, all found before anything is touched, in this
 *    order: SRT_ERR_STATE before srt_set_scene; SRT_ERR_INVALID_ARG for an empty or out-of-range band, unknown flags, a non-zero
 *    reserved word or a NaN band_weight, and with _DEPTH for a NaN or negative bias or min_variance; SRT_ERR_STATE for no cascade;
 *    SRT_ERR_STATE for a missing OBJECT, NORMAL_DEPTH or POSITION guide, or ALBEDO with the flag; SRT_ERR_STATE, per level
 *    ascending, for missing coefficients or a count other than that level's P, with _DEPTH for resolution == 0 or missing or
 *    mis-sized moments, with _STATES for missing or mis-sized records.
 * C8. srt_probe_cascade_grids (pure host).  Level l has the given counts and spacing_a = ldexpf(base_spacing_a, l).  Its origin is
 *    snapped to whole cells of its own spacing, so every later move is a whole-cell srt_scroll_probes shift:
 *    k = floorf(centre_a / spacing_a), clamped to +-1048576, a NaN gives 0; origin_a = (k - (float)((n_a - 1) / 2)) * spacing_a
 *    with integer division.  blend_cells = 1.0f, resolution = 0.  SRT_ERR_INVALID_ARG for levels outside 1 .. 4 or a level
 *    srt_set_probe_grid would refuse; *out is then untouched.
 * Not here: the cascade in srt_probe_tail / srt_render_adaptive_tail, the exact any-hit test per level, more than two levels per
 * pixel, a per-level blend_cells. */
#define SRT_PROBE_CASCADE_MAX_LEVELS 4
/* srt_probe_cascade_params.flags */
#define SRT_PROBE_CASCADE_NORMAL_WEIGHT 1u /* probe-grid rule 6, every level */
#define SRT_PROBE_CASCADE_DEPTH 2u         /* rule 7b from each level's moments */
#define SRT_PROBE_CASCADE_STATES 4u        /* rules 3s, 4s from each level's records */
#define SRT_PROBE_CASCADE_ALBEDO 8u        /* rule C3: rgb times SRT_GBUF_ALBEDO.rgb */
#define SRT_PROBE_CASCADE_COUNT_WORK 16u   /* fill srt_probe_cascade_work for this call */
/* which (level arrays) */
#define SRT_PROBE_CASCADE_COEFFICIENTS 1u  /* [P][9] float4 */
#define SRT_PROBE_CASCADE_MOMENTS 2u       /* [P][R*R] float4 */
#define SRT_PROBE_CASCADE_RECORDS 4u       /* [P] float4 */

typedef struct srt_probe_cascade {                     /* 160 bytes */
    uint32_t levels;                                   /* 1 .. 4; level 0 is the finest */
    uint32_t resolution;                               /* R of every level's moments: 0 (none), 4, 8 or 16 */
    float blend_cells;                                 /* width of the border band in cells of the level, finite, > 0 */
    uint32_t reserved;                                 /* 0 */
    srt_probe_grid grid[SRT_PROBE_CASCADE_MAX_LEVELS]; /* entries >= levels are ignored */
} srt_probe_cascade;

typedef struct srt_probe_cascade_params { /* 40 bytes */
    int32_t row_begin;                    /* first memory row (inclusive), as srt_probe_grid_params */
    int32_t row_end;                      /* one past the last memory row */
    uint32_t flags;                       /* SRT_PROBE_CASCADE_NORMAL_WEIGHT | _DEPTH | _STATES | _ALBEDO | _COUNT_WORK */
    float band_weight[3];                 /* A for SH bands 0, 1, 2 (probe-grid rule 10) */
    float bias, min_variance;             /* rule 7b; read only with SRT_PROBE_CASCADE_DEPTH */
    uint32_t reserved[2];                 /* 0 */
} srt_probe_cascade_params;

typedef struct srt_probe_cascade_work {                   /* 112 bytes */
    uint32_t valid, reserved;                             /* 1, 0 */
    uint64_t pixels;                                      /* hit pixels of the band */
    uint64_t evaluations;                                 /* level evaluations: 1 or 2 per hit pixel */
    uint64_t blended;                                     /* hit pixels with 2 */
    uint64_t first_level[SRT_PROBE_CASCADE_MAX_LEVELS];   /* hit pixels whose first level is k */
    uint64_t corners, open;                               /* live corners; with _DEPTH those whose weight stays > 0 */
    uint64_t wave_trips;                                  /* sum over tiles of ceil(Q / 8) */
    uint64_t waves;                                       /* waves of the launch */
    uint64_t spare[2];                                    /* 0 */
} srt_probe_cascade_work;

/* flags 0, band_weight = (3.14159274f, 2.09439516f, 0.785398185f), bias and min_variance as srt_probe_grid_depth_params_default
 * (0.0f, 1e-4f), reserved 0; row_begin = row_end = 0: the band is the caller's to fill (pure host). */
int srt_probe_cascade_params_default(srt_probe_cascade_params* out);
/* pure host: rule C8 */
int srt_probe_cascade_grids(const float centre[3], const float base_spacing[3], const int32_t counts[3], uint32_t levels, srt_probe_cascade* out);
/* pure host: rule C2 for one point */
int srt_probe_cascade_weights(const srt_probe_cascade* cascade, const float point[3], int32_t* first_level, int32_t* evaluations, float* beta);
int srt_set_probe_cascade(srt_context* ctx, const srt_probe_cascade* cascade);
int srt_write_probe_cascade_level(srt_context* ctx, uint32_t level, uint32_t which, const float* src, size_t probes);
int srt_bind_probe_cascade_level(srt_context* ctx, uint32_t level, uint32_t which, const void* d_ptr, size_t probes);
int srt_capture_probe_cascade_level(srt_context* ctx, uint32_t level, uint32_t which_mask);
int srt_shade_probe_cascade(srt_context* ctx, const srt_probe_cascade_params* params);
int srt_get_probe_cascade_work(srt_context* ctx, srt_probe_cascade_work* out);

/* ---- scrolling probe grids: move a grid and keep its histories (ABI 7, backward compatible) --------------------------------------
 * These calls were added without changing anything else, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of them
 * runs what it ran before, bit for bit.  A grid that covers only the surroundings of the viewer has to move with the viewer;
 * srt_set_probe_grid followed by srt_reset_probe_history throws every blended sample away.  srt_scroll_probes moves the grid's
 * per-probe arrays by a whole number of cells instead: a probe that stands where the old grid had one keeps that probe's history,
 * the others start over.  Every buffer stays on the device and no call waits.
 * SC1. Mapping.  The current grid (srt_set_probe_grid) has nx, ny, nz probes, P = nx*ny*nz, probe (ix, iy, iz) at index
 *    ix + nx*(iy + ny*iz).  For a destination probe i = (ix, iy, iz) the source is j = i + shift per axis, in 64-bit integer
 *    arithmetic; shift may be any int32.  Probe i is RETAINED when 0 <= j_a < n_a on all three axes, otherwise EXPOSED.  An axis
 *    with |shift_a| >= n_a exposes every probe.  (The grid moves by +shift cells: new probe i stands where old probe i + shift
 *    stood.)
 * SC2. Histories.  `which` selects the histories of the blend: the [P][9] float4 coefficients (SRT_PROBE_SCROLL_COEFFICIENTS) and
 *    the [P][R*R] float4 moments (SRT_PROBE_SCROLL_MOMENTS), each in its current buffer: the handle's own unless
 *    srt_bind_probe_history bound the caller's.  After the call that buffer holds, at a retained i, the bits that were at j before
 *    the call (a NaN stays that NaN, all four lanes) and at an exposed i all-zero bits; srt_blend_probes' rule U2 then restarts
 *    exactly the exposed probes and goes on blending the retained ones.  The move is never done in place: the kernel reads the
 *    current buffer and writes a distinct one, a handle-owned spare of the same size, allocated on first use (SRT_ERR_OOM if it
 *    cannot be had).  An own history then swaps with the spare; a bound history is copied back from it on the launch stream.  A
 *    zero shift leaves every history bit alone and launches nothing for the histories.
 * SC3. States.  With SRT_PROBE_SCROLL_STATES the P records current for srt_shade_probe_grid_states (srt_write_probe_grid_states,
 *    srt_bind_probe_grid_states) are read; that slot is a const pointer and is never written.  The handle's own previous-records
 *    array, the one srt_write_probe_previous_states fills, then holds record j at a retained i and zero bits at an exposed i, and
 *    becomes the current previous-records source with count P, as after that call (a binding of srt_bind_probe_previous_states
 *    ends).  With shift 0 this is a plain device copy "current -> previous", which a per-frame loop wants anyway.
 *    srt_read_probe_previous_states waits and copies the records that are the current previous-records source (this array, the
 *    one srt_write_probe_previous_states filled, or the bound one), 4 floats per probe; SRT_ERR_STATE when there is none.
 * SC4. Grid.  With SRT_PROBE_SCROLL_SET_GRID the handle's grid keeps spacing and counts and origin_a becomes
 *    origin_a + ((float)shift_a * spacing_a): binary32, no contraction, the product first.  Without the flag the grid is untouched
 *    and the caller calls srt_set_probe_grid.  New probe i and old probe j are at BIT-EQUAL positions only when these products and
 *    sums are exact, for instance with a dyadic origin and spacing; otherwise the two positions differ by rounding, and the history
 *    is kept all the same.  A caller who scrolls often should compute origins from a fixed base and a cumulative integer shift and
 *    set them with srt_set_probe_grid, not by repeated _SET_GRID: the roundings of repeated steps add up.  A moved origin that is
 *    not finite is SRT_ERR_INVALID_ARG (after the check for a grid).
 * SC5. Stale inputs.  After a call with a non-zero shift, the records that say which buffers the last
 *    srt_trace_light_probes[_listed] wrote COEFFICIENTS to and the last srt_trace_probe_depth[_listed] wrote MOMENTS to count as
 *    "did not write" (for srt_blend_probes and for the two srt_read_*_output calls alike): srt_blend_probes answers SRT_ERR_STATE
 *    until a new trace.  A trace indexed by the old grid must not be blended into the new one.  The list bound for tracing, the
 *    light-probe positions, the current records and a continuing RADIANCE buffer are the caller's to refresh.  A frame:
 *    srt_scroll_probes (with _STATES and _SET_GRID) -> srt_classify_probes -> bind its positions and records -> srt_list_probes ->
 *    the listed traces -> srt_blend_probes with _LISTED | _PREVIOUS_STATES.
 * SC6. Determinism and work.  One wave per destination probe, the decision is wave-uniform; no atomic reaches an output, and
 *    repeated calls on the same input give the same bits.  With SRT_PROBE_SCROLL_COUNT_WORK the call records the probes (P), the
 *    retained, the exposed and the waves of the launch, counted once per call, not once per selected array (a call with the flag
 *    always launches, with a zero shift too); one vector atomic per wave at the end, without the flag no atomics at all.
 *    srt_get_probe_scroll_work waits and copies the record; SRT_ERR_STATE unless the last srt_scroll_probes had the flag.
 * SC7. srt_probe_grid_follow (pure host).  Per axis, in binary32 without contraction: c = origin_a + (((float)(n_a - 1)) * 0.5f)
 *    * spacing_a, u = (point_a - c) / spacing_a, shift_a = (int32)u truncated towards zero after clamping u to +-1048576; a NaN
 *    gives 0.  Truncation means the grid moves only once the point is a whole cell off centre.  SRT_ERR_INVALID_ARG for a grid
 *    srt_set_probe_grid would refuse.
 * SC8. Errors, all found before anything is touched, in this order: SRT_ERR_STATE before srt_set_scene; SRT_ERR_INVALID_ARG for
 *    which == 0, unknown bits in which or flags, or a non-zero reserved word; SRT_ERR_STATE for no grid, or for a selected history
 *    that was never reset or whose size is not the grid's P; with _STATES, SRT_ERR_STATE for no current records or a count other
 *    than P; SRT_ERR_OOM.  Asynchrony: as for the blend; the call is enqueued on the launch stream and covered by srt_wait /
 *    srt_poll. */
#define SRT_PROBE_SCROLL_COEFFICIENTS 1u /* srt_probe_scroll_params.which: = SRT_PROBE_HISTORY_COEFFICIENTS */
#define SRT_PROBE_SCROLL_MOMENTS 2u      /* = SRT_PROBE_HISTORY_MOMENTS */
#define SRT_PROBE_SCROLL_STATES 4u       /* current records -> previous records, scrolled (rule SC3) */
#define SRT_PROBE_SCROLL_COUNT_WORK 1u   /* srt_probe_scroll_params.flags: fill srt_probe_scroll_work for this call */
#define SRT_PROBE_SCROLL_SET_GRID 2u     /* also move the handle's grid origin (rule SC4) */

typedef struct srt_probe_scroll_params { /* 32 bytes */
    int32_t shift[3];                    /* cells the grid moves along +x, +y, +z */
    uint32_t which;                      /* SRT_PROBE_SCROLL_COEFFICIENTS | _MOMENTS | _STATES, not 0 */
    uint32_t flags;                      /* SRT_PROBE_SCROLL_COUNT_WORK | _SET_GRID */
    uint32_t reserved[3];                /* 0 */
} srt_probe_scroll_params;

typedef struct srt_probe_scroll_work { /* 40 bytes */
    uint32_t valid, reserved;          /* 1, 0 */
    uint64_t probes;                   /* P */
    uint64_t retained;                 /* ... of which keep a history (rule SC1) */
    uint64_t exposed;                  /* ... of which start over */
    uint64_t waves;                    /* waves of the launch */
} srt_probe_scroll_work;

/* shift 0, which SRT_PROBE_SCROLL_COEFFICIENTS, flags 0, reserved 0 (pure host). */
int srt_probe_scroll_params_default(srt_probe_scroll_params* out);
int srt_scroll_probes(srt_context* ctx, const srt_probe_scroll_params* params);
int srt_get_probe_scroll_work(srt_context* ctx, srt_probe_scroll_work* out);
int srt_read_probe_previous_states(srt_context* ctx, float* dst);
/* pure host: the shift that re-centres `grid` on `point` (rule SC7) */
int srt_probe_grid_follow(const srt_probe_grid* grid, const float point[3], int32_t shift[3]);

/* ---- probe tail: radiance paths that end in the probe grid (ABI 7, backward compatible) -----------------------------------------
 * These calls were added without changing anything else, so SRT_ABI_VERSION stays 7.  srt_probe_tail sets a per-context mode, off
 * by default.  With it on, a path of srt_trace_radiance, srt_trace_light_probes or srt_trace_light_probes_listed that ends BECAUSE
 * THE BOUNCE LIMIT WAS REACHED ON A SURFACE adds the grid's hemisphere-mean radiance at that surface, times the path's throughput:
 * one or two bounces and a lookup instead of eight bounces, and no light lost to truncation.  Everything else stays as it is, RNG
 * streams included.  With the mode off every call launches the kernels it launched before.  srt_render, srt_render_adaptive and
 * every other pass ignore the mode.
 *
 * srt_probe_tail touches no device memory and launches nothing.  SRT_ERR_INVALID_ARG, and the previous setting stands, for: enabled
 * outside 0..1; unknown flags; a NaN band weight; a bias that is NaN, infinite or < 0; a min_variance that is NaN, infinite or
 * <= 0; a non-zero reserved word.
 *
 * The grid, coefficients, depth maps and states are those of srt_set_probe_grid and the three srt_write_ / srt_bind_probe_grid_*
 * pairs, CURRENT AT THE ENQUEUE OF THE TRACE: exactly what srt_shade_probe_grid_states would read.  Each affected trace call
 * checks them after its own errors and before anything is touched, and returns SRT_ERR_STATE when there is no grid or there are
 * no coefficients; when a count is not nx*ny*nz; when the depth maps are missing under DEPTH or the states under STATES; when the
 * coefficient array the tail would read overlaps, as a byte range, the buffer the call is about to write (RADIANCE, or the
 * light-probe COEFFICIENTS output): a feedback loop reads the history or the previous frame's buffer, never the one being written.
 *
 * T1. Where.  A sample's path (radiance block rule 2) ends at a primary miss, at a bounce ray that leaves the scene, or at
 *     bounce >= max_bounces after a surface hit.  Only the third case changes, and only for max_bounces >= 1: with
 *     max_bounces == 0 the call is unchanged (and checks none of the above).
 * T2. State after Raytracer.cpp:182-184 for that last hit: L; T, already multiplied by the surface's colour of the lottery; spec,
 *     the lottery just drawn; x and n, the hit's point and normal; Smoothness of the hit material.  No draw is consumed.
 * T3. g = 1.0f - (Smoothness * spec): the share of the next bounce's direction that would have been the random one (:175).
 *     If !(g > 0), nothing is added (work: mirror_ends).
 * T4. (M, a) is the float4 that srt_shade_probe_grid_states (or _depth, or srt_shade_probe_grid without VISIBILITY, according to
 *     the flags) writes for a pixel whose guides hold a hit, POSITION x and NORMAL n, without ALBEDO, with the mode's band
 *     weights, bias and min_variance: probe-grid rules 2 - 6, 7b, 3s / 4s, 8 and 9 in the same operation order; corners are
 *     summed in ascending c, starting from +0; a skipped corner contributes +0; rule 5's origin is x + n * .00001f.
 *     If !(a > 0), nothing is added (work: dark).  Then M_l = !(M_l > 0) ? 0 : M_l per lane: SH ringing and NaN stay out.
 * T5. k_l = (T_l * 0.8f) * g and L_l = L_l + (k_l * M_l) for l = 0, 1, 2: the 0.8 is the dissipation the next bounce would have
 *     applied (:169-171).  The colour's alpha lane and tag are untouched.
 * T6. Everything after that is as before: the scratch row, the ordered fold, the running mean of rule 3.
 * Binary32 without contraction throughout.  With all coefficients zero the outputs are, bit for bit, those of the mode off.
 * srt_trace_light_probes' RADIANCE still equals srt_trace_radiance on the explicit rays under the same mode, its COEFFICIENTS are
 * still the fixed-order projection of that RADIANCE, and the listed call still writes at the listed probes what the unlisted one
 * writes there.  Pinned domain: finite coefficients, moments and offsets, over the pinned domain of the trace call; anything else
 * gives some value and does not fault (every index is clamped as in the shading pass).
 *
 * srt_get_probe_tail_work waits and copies the record of the last affected trace; SRT_ERR_STATE unless that trace ran with the
 * mode on and COUNT_WORK set (all zeros when max_bounces == 0 kept the mode from applying).  srt_radiance_work and
 * srt_light_probe_work are filled exactly as before: a lookup traces no ray.  wave_lookups counts the steps of a wave's sample
 * pool in which at least one of its lanes ended at the bounce limit on a surface (the wave then goes through the lookup's
 * eight-corner loop once, all its terminal lanes together); it depends on the launch's grid only through which wave runs which
 * block, so repeated runs on one device give the same number. */
#define SRT_PROBE_TAIL_NORMAL_WEIGHT 1u  /* probe-grid rule 6 */
#define SRT_PROBE_TAIL_DEPTH 2u          /* rule 7b, from the maps of srt_write/bind_probe_grid_depth */
#define SRT_PROBE_TAIL_STATES 4u         /* rules 3s, 4s, from the records of srt_write/bind_probe_grid_states */
#define SRT_PROBE_TAIL_COUNT_WORK 8u

typedef struct srt_probe_tail_params { /* 32 bytes */
    int32_t enabled;                   /* 0 or 1 */
    uint32_t flags;                    /* SRT_PROBE_TAIL_* */
    float band_weight[3];              /* A for SH bands 0, 1, 2 */
    float bias, min_variance;          /* rule 7b; as srt_probe_grid_depth_params */
    uint32_t reserved;                 /* 0 */
} srt_probe_tail_params;

typedef struct srt_probe_tail_work {   /* 56 bytes */
    uint32_t valid, reserved;          /* 1, 0 */
    uint64_t tails;        /* paths that ended at the bounce limit on a surface with g > 0: lookups made */
    uint64_t corners;      /* corners that reached rule 7 (weight > 0, L > 0, not buried) */
    uint64_t open;         /* corners that entered the sum (== corners without DEPTH) */
    uint64_t dark;         /* lookups whose weights summed to 0: nothing added */
    uint64_t mirror_ends;  /* paths that ended at the limit with !(g > 0): no lookup */
    uint64_t wave_lookups; /* wave-level passes through the lookup code (see above) */
} srt_probe_tail_work;

/* enabled 1, flags 0, band_weight (1.0f, 0.5f, 0.0f) — the hemisphere MEAN of probe-grid rule 10, which is what this renderer's
 * diffuse bounce averages — bias 0, min_variance 1e-4f, reserved 0.  Pure host. */
int srt_probe_tail_params_default(srt_probe_tail_params* out);
int srt_probe_tail(srt_context* ctx, const srt_probe_tail_params* params);
int srt_get_probe_tail_work(srt_context* ctx, srt_probe_tail_work* out);

/* ---- adaptive renders that end in the probe grid (ABI 7, backward compatible) ---------------------------------------------------
 * This call was added without changing anything else, so SRT_ABI_VERSION stays 7.  srt_render_adaptive_tail is srt_render_adaptive
 * (rules 1 - 10 of its block) with rules T1 - T6 of the probe-tail block applied to every sample's path: a picture — band,
 * framebuffer, per-pixel counts and budget — whose paths take one or two bounces and a lookup in the probe grid.  It uses the
 * context's srt_probe_tail setting (flags, band weights, bias, min_variance) and reads the grid, coefficients, depth maps and
 * states CURRENT AT THE ENQUEUE, as the affected traces do.  The struct and its two flags are srt_render_adaptive's.
 *
 * R1. Order of checks.  First srt_render_adaptive's own errors, in its order (rule 9).  Then SRT_ERR_STATE when the context's tail
 *     setting is off (there has been no accepted srt_probe_tail with enabled = 1, or a later one switched it off).  Then, only for
 *     max_bounces >= 1, the refusals of an affected trace (probe-tail block: no grid, no coefficients, a count that is not
 *     nx*ny*nz, DEPTH without maps, STATES without records), where "the buffer about to be written" is BOTH the current
 *     accumulator and the current framebuffer (srt_bind_output): SRT_ERR_STATE when the coefficient array shares a byte with
 *     either.  Nothing is touched on any refusal.
 * R2. max_bounces == 0.  After R1's first two steps the call launches exactly what srt_render_adaptive launches and checks no
 *     grid input (T1).
 * R3. Equivalence.  After any sequence of srt_render_adaptive_tail calls that started from n_p = 0, with one seed, one bounce
 *     count, one tail setting and unchanged grid inputs, pixel p's accumulator element equals element p of srt_trace_radiance's
 *     output under the same mode on the frame's camera rays — origin the camera position, direction GetRayDirection, ray index
 *     x + y*W, id_base = 0, first_sample = 1, sample_count = n_p, SRT_RADIANCE_RESET, the same seed and bounces — in all four
 *     lanes (NaN as NaN); the framebuffer pixel is tone_map of that element at memory row H - 1 - y (adaptive rule 3).  The scene
 *     in LDS or in memory, with or without meshes.  It does NOT hold from a start of srt_render(1..n) followed by
 *     srt_set_sample_counts(n): srt_render's paths end without the lookup, so the two calls estimate different quantities and
 *     their samples do not belong in one mean.  Start a tail frame from srt_set_sample_counts(0).
 * R4. Zero coefficients.  With all coefficients zero the accumulator, the framebuffer, the counts and srt_adaptive_work are those
 *     of srt_render_adaptive, bit for bit.
 * R5. Adaptive rules 4 (untouched pixels), 5 (counts, KEEP_COUNTS), 6 (determinism), 7 and 8 hold unchanged.
 * R6. Work records.  srt_get_adaptive_work treats this call as an adaptive render, under the same SRT_ADAPTIVE_COUNT_WORK rule.
 *     srt_get_probe_tail_work treats it as the last affected trace (SRT_PROBE_TAIL_COUNT_WORK of the setting); the record is all
 *     zeros under R2.  wave_lookups is deterministic here: a tile's pool drains before its wave takes another tile, so the count
 *     does not depend on which wave drew the tile.
 * R7. srt_render_adaptive, srt_render and every other pass behave exactly as before and still ignore the mode. */
int srt_render_adaptive_tail(srt_context* ctx, const srt_adaptive_params* params);

/* ---- per-frame probe updates: active-probe lists, listed traces and a hysteresis blend (ABI 7, backward compatible) ---------------
 * These calls were added without changing anything else, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of them
 * runs what it ran before, bit for bit.  They keep a classified probe grid alive from frame to frame: srt_list_probes compacts the
 * probes worth tracing, the two listed traces trace only those, and srt_blend_probes folds a few new samples per frame into a
 * persistent history (DDGI's exponential blend).  Every buffer stays on the device, and no call waits for a count: the number of
 * listed probes is read by the kernels from the list's header; the host never learns it.  All arithmetic is binary32 without
 * contraction.
 *
 * The list.  SRT_PROBE_LIST is 4 + P uint32: word 0 the count n, word 1 P, words 2 and 3 zero, words 4 .. 4+n-1 the indices p
 * with (state & skip_mask) == 0 in ascending order, words 4+n .. 4+P-1 0xFFFFFFFF.  srt_list_probes reads the P records that are
 * current for srt_shade_probe_grid_states (srt_write_probe_grid_states, srt_bind_probe_grid_states; 1 <= P <= 2^30; with a grid
 * set, P must be nx*ny*nz) and writes the list into the handle's own buffer or the DEVICE buffer of srt_bind_probe_list_output
 * (NULL = own), under srt_bind_probe_states_output's rules; srt_read_probe_list_output waits and copies the 4 + P words the last
 * srt_list_probes wrote, from the buffer it wrote, SRT_ERR_STATE when there has been none.  skip_mask: any subset of
 * SRT_PROBE_MOVED | _BURIED | _INSIDE | _IDLE; the default is SRT_PROBE_BURIED | SRT_PROBE_IDLE.  The compaction is deterministic:
 * one workgroup walks the records in chunks with a running base (wave ballots, LDS for the wave counts); no atomic reaches the
 * output, and repeated calls give the same bits.  With SRT_PROBE_LIST_COUNT_WORK the launch counts its probes (P), the listed
 * ones (n) and its waves; srt_get_probe_list_work waits and copies that record, SRT_ERR_STATE unless the last call had the flag.
 * Errors, all found before anything is touched, in this order: SRT_ERR_STATE before srt_set_scene; SRT_ERR_INVALID_ARG for
 * unknown flags, a skip_mask outside the four bits or a non-zero reserved; SRT_ERR_STATE for no states or a count other than the
 * grid's; SRT_ERR_OOM when a buffer cannot be had.
 *
 * The listed traces.  srt_bind_probe_list(ctx, d_list, capacity) binds a DEVICE buffer in SRT_PROBE_LIST's layout for tracing; it
 * does not copy and does not wait (what srt_bind_probe_list_output filled can be bound); NULL, 0 unbinds.  srt_write_probe_list
 * copies `capacity` words from the host into the handle's own array and waits.  capacity = 4 + P', 1 <= P' <= 2^30, otherwise
 * SRT_ERR_INVALID_ARG.  srt_trace_light_probes_listed and srt_trace_probe_depth_listed take their parents' parameter structs,
 * output slots, "last trace" records and work records, and make the parents' checks first; then SRT_ERR_STATE for no list or a
 * capacity other than 4 + P for the current positions' P.
 * L. Let q run over 0 .. n-1 and p = list[4 + q].  The listed call writes, for each listed p, exactly the bits the unlisted call
 *    writes there: coefficients [p][0..8], RADIANCE elements p*K + k, moments [p][0..R*R), distances p*K + k; the stream id of ray
 *    (p, k) stays id_base + p*K + k.  Elements of probes not listed are neither read nor written.  The continuation rule (no
 *    SRT_LIGHT_PROBE_RESET) holds per slot and is checked on the host as for the parent.  The launch is sized for P (grid, sample
 *    scratch, partial buffer); the kernel reads n (clamped to P) from the header.  A word list[4 + q] >= P skips that unit, so a
 *    bad list cannot cause an out-of-range store.  The order of the indices is irrelevant to the bits of a slot.  The indices
 *    must be DISTINCT (srt_list_probes' are): with an index listed twice two waves would update the same RADIANCE elements of a
 *    continuing trace, or the same history slot of a listed blend, in no defined order; nothing checks it.  Work counts:
 *    `probes` counts the listed probes, and the other counters follow.
 *
 * The blend.  The histories: coefficients [P][9] float4 (SRT_PROBE_HISTORY_COEFFICIENTS) and, optionally, moments [P][R*R] float4
 * (SRT_PROBE_HISTORY_MOMENTS), each the handle's own buffer or the DEVICE buffer of srt_bind_probe_history (one bit; NULL = own;
 * no copy, no wait).  srt_reset_probe_history(ctx, which, probes, resolution) gives the histories of the set `which` their size
 * (P, and R for the moments: 4, 8 or 16, P*R*R <= 2^30; ignored without the moments) and zero-fills them, enqueued on the stream;
 * srt_read_probe_history waits and copies one; SRT_ERR_STATE before the first reset.  The new data N are the buffers the last
 * srt_trace_light_probes[_listed] wrote COEFFICIENTS to and (SRT_PROBE_BLEND_MOMENTS) the last srt_trace_probe_depth[_listed]
 * wrote MOMENTS to; if that call did not write the output, or wrote it for another P (or R) than the history's, SRT_ERR_STATE.
 * The history H is updated in place; afterwards it is what srt_bind_probe_grid_coefficients / srt_bind_probe_grid_depth take.
 * U1. Which probes.  With SRT_PROBE_BLEND_LISTED, p = list[4 + q] for q < n of the list bound for tracing (capacity 4 + P; a word
 *    >= P is skipped); without it, p = 0 .. P-1.  Every other probe's history keeps its bits.
 * U2. Restart.  A probe restarts when the bits of H[p][0].w are 0 (the buffer was reset or never filled; a traced probe has the
 *    sum of 0.282095 * w_k > 0 there), or when SRT_PROBE_BLEND_PREVIOUS_STATES is set and, between the current record (the slot of
 *    srt_write_probe_grid_states / srt_bind_probe_grid_states) and the previous one (srt_write_probe_previous_states /
 *    srt_bind_probe_previous_states, the same rules), any offset lane differs bitwise or (state ^ previous) & (BURIED | IDLE) is
 *    not 0.  A restarting probe gets H = N, bits copied, for the coefficients and (with _MOMENTS) the moments.
 * U3. Change.  Y(v) = (0.2126f*v.x + 0.7152f*v.y) + 0.0722f*v.z (Rec. 709; no other header of the project fixes luminance
 *    weights).  yh = Y(H[p][0]), yn = Y(N[p][0]); d = fabsf(yn - yh); m = fabsf(yh) > fabsf(yn) ? fabsf(yh) : fabsf(yn);
 *    changed = d > change_threshold * m; h = changed ? fast_hysteresis : hysteresis.
 * U4. Blend.  For every coefficient and lane, H = N + ((H - N) * h).
 * U5. Moments.  With _MOMENTS the same expression with depth_hysteresis, all four lanes of every texel.
 * U6. Determinism.  No atomics reach an output; one wave per probe, the decision is wave-uniform.
 * U7. Work counts.  With SRT_PROBE_BLEND_COUNT_WORK: the probes blended, those that restarted, those that did not restart and
 *    changed, and the waves of the launch.  One vector atomic per wave at the end; without the flag no atomics at all.
 *    srt_get_probe_blend_work waits and copies the record; SRT_ERR_STATE unless the last srt_blend_probes had the flag.
 * U8. Parameters.  hysteresis, fast_hysteresis, depth_hysteresis: each in [0, 1); change_threshold: finite, >= 0.  The defaults
 *    (0.9, 0.5, 0.9, 0.25) are picks, DDGI's customary values, not measurements.
 * U9. Errors, all found before anything is touched, in this order: SRT_ERR_STATE before srt_set_scene; SRT_ERR_INVALID_ARG for
 *    unknown flags, a parameter outside its range (a NaN included) or a non-zero reserved; SRT_ERR_STATE for a history that was
 *    never reset, new data that are missing or of another size, (with _LISTED) no list or another capacity, (with
 *    _PREVIOUS_STATES) missing records or another count.  Asynchrony: as rule 8 of the light-probe block. */
#define SRT_PROBE_LIST_COUNT_WORK 1u           /* srt_probe_list_params.flags: fill srt_probe_list_work for this call */
#define SRT_PROBE_LIST_HEADER 4u               /* words in front of the indices */
#define SRT_PROBE_HISTORY_COEFFICIENTS 1u      /* history: [P][9] float4 */
#define SRT_PROBE_HISTORY_MOMENTS 2u           /* history: [P][R*R] float4 */
#define SRT_PROBE_BLEND_MOMENTS 1u             /* srt_probe_blend_params.flags: rule U5 */
#define SRT_PROBE_BLEND_LISTED 2u              /* only the probes of the bound list (rule U1) */
#define SRT_PROBE_BLEND_PREVIOUS_STATES 4u     /* restart where a record changed (rule U2) */
#define SRT_PROBE_BLEND_COUNT_WORK 8u          /* fill srt_probe_blend_work for this call */

typedef struct srt_probe_list_params { /* 16 bytes */
    uint32_t skip_mask;                /* state bits that exclude a probe */
    uint32_t flags;                    /* SRT_PROBE_LIST_COUNT_WORK */
    uint32_t reserved[2];              /* 0 */
} srt_probe_list_params;

typedef struct srt_probe_list_work { /* 32 bytes */
    uint32_t valid, reserved;        /* 1, 0 */
    uint64_t probes;                 /* P */
    uint64_t listed;                 /* n */
    uint64_t waves;                  /* waves of the launch */
} srt_probe_list_work;

typedef struct srt_probe_blend_params { /* 24 bytes */
    float hysteresis;                   /* share of the history kept where the light did not change; [0, 1) */
    float fast_hysteresis;              /* ... where it did (rule U3); [0, 1) */
    float depth_hysteresis;             /* ... of the moments; [0, 1) */
    float change_threshold;             /* relative luminance change of the DC term that counts as a change; >= 0 */
    uint32_t flags;                     /* SRT_PROBE_BLEND_MOMENTS | _LISTED | _PREVIOUS_STATES | _COUNT_WORK */
    uint32_t reserved;                  /* 0 */
} srt_probe_blend_params;

typedef struct srt_probe_blend_work { /* 40 bytes */
    uint32_t valid, reserved;         /* 1, 0 */
    uint64_t probes;                  /* probes blended */
    uint64_t restarted;               /* ... of which restarted (rule U2) */
    uint64_t changed;                 /* ... of which did not restart and changed (rule U3) */
    uint64_t waves;                   /* waves of the launch */
} srt_probe_blend_work;

struct srt_light_probe_params; /* (defined in the light-probe block below) */
struct srt_probe_depth_params; /* (defined in the probe-depth block below) */
/* skip_mask SRT_PROBE_BURIED | SRT_PROBE_IDLE, flags 0, reserved 0 (pure host). */
int srt_probe_list_params_default(srt_probe_list_params* out);
int srt_list_probes(srt_context* ctx, const srt_probe_list_params* params);
int srt_bind_probe_list_output(srt_context* ctx, void* d_list);
int srt_read_probe_list_output(srt_context* ctx, uint32_t* dst);
int srt_get_probe_list_work(srt_context* ctx, srt_probe_list_work* out);
int srt_bind_probe_list(srt_context* ctx, const void* d_list, size_t capacity);
int srt_write_probe_list(srt_context* ctx, const uint32_t* list, size_t capacity);
int srt_trace_light_probes_listed(srt_context* ctx, const struct srt_light_probe_params* params);
int srt_trace_probe_depth_listed(srt_context* ctx, const struct srt_probe_depth_params* params);
/* hysteresis 0.9f, fast_hysteresis 0.5f, depth_hysteresis 0.9f, change_threshold 0.25f, flags 0, reserved 0 (pure host; picks). */
int srt_probe_blend_params_default(srt_probe_blend_params* out);
int srt_reset_probe_history(srt_context* ctx, uint32_t which, size_t probes, uint32_t resolution);
int srt_bind_probe_history(srt_context* ctx, uint32_t which, void* d_ptr);
int srt_read_probe_history(srt_context* ctx, uint32_t which, float* dst);
int srt_write_probe_previous_states(srt_context* ctx, const float* records, size_t probes);
int srt_bind_probe_previous_states(srt_context* ctx, const void* d_ptr, size_t probes);
int srt_blend_probes(srt_context* ctx, const srt_probe_blend_params* params);
int srt_get_probe_blend_work(srt_context* ctx, srt_probe_blend_work* out);

/* ---- probe classification and relocation: states and offsets for a probe grid (ABI 7, backward compatible) ----------------------
 * These calls were added without changing anything else, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of them
 * runs what it ran before, bit for bit.  (The rules are numbered S1 .. S9; the blocks that use them follow further down.)
 *
 * A grid laid blindly over a scene puts probes inside objects, where they see nothing of use and where the filtered visibility
 * test cannot tell (a depth map traced from inside a sphere or a box does not give the probe away).  srt_classify_probes finds
 * those probes, and with SRT_PROBE_CLASSIFY_RELOCATE moves probes that are inside or too near a surface to a free place nearby.
 * Spheres and axis-aligned boxes have an exact signed distance, so the pass traces no ray.  LIMIT: mesh objects contribute no
 * distance; a probe inside a mesh is not found, and a scene with a mesh object never gets an IDLE probe.
 *
 * Inputs: the grid of srt_set_probe_grid, P = nx*ny*nz probes, probe g at the position of the probe-grid block's rule 4; with
 * SRT_PROBE_CLASSIFY_RELOCATE the K shared directions of the light-probe block (srt_write_light_probe_directions,
 * srt_bind_light_probe_directions), of which only xyz is read, each replaced by float3::Normalized(d) with
 * SRT_PROBE_CLASSIFY_NORMALIZE (as SRT_RAYS_NORMALIZE); and the scene's object list as srt_set_scene / srt_update_scene keep it at
 * enqueue.  The pass keeps a primitive table of its own, rebuilt from the list at the first srt_classify_probes after the scene
 * changed (that call then waits for earlier work); srt_set_scene and srt_update_scene do what they did.
 *
 * Rules.  All arithmetic is binary32 without contraction.
 * S1. Scene distance S(x).  S = +inf; then for every sphere and box of the list S = sd < S ? sd : S, so a NaN is ignored and the
 *    order is irrelevant.  Sphere: e = x - c; D = sqrtf((e.x*e.x + e.y*e.y) + e.z*e.z); sd = D - fabsf(radius).  Box, per axis a:
 *    q_a = fabsf(x_a - c_a) - h_a; m_a = q_a > 0 ? q_a : 0; then with max(a, b) = a > b ? a : b and min0(a) = a < 0 ? a : 0:
 *    sd = sqrtf((m.x*m.x + m.y*m.y) + m.z*m.z) + min0(max(max(q.x, q.y), q.z)).  Inert and mesh objects contribute nothing.
 * S2. Scales.  smin = the smallest spacing component; margin = clearance * smin; reach = sqrtf((sx*sx + sy*sy) + sz*sz);
 *    dt = max_offset / (float)steps.
 * S3. Probe at rest.  s0 = S(g).  Without SRT_PROBE_CLASSIFY_RELOCATE: state = s0 < 0 ? BURIED|INSIDE : CLEAR (0), offset 0.
 *    With it and !(s0 < margin): CLEAR, offset 0.  A CLEAR probe with s0 > 1.0625f * reach additionally gets IDLE, but only when
 *    the scene has no mesh object: 1.0625f covers the rounding of S and shading rule 5's 1e-5 normal offset, so no first-hit
 *    point on an analytic surface can lie in one of the probe's eight cells.
 * S4. Search, with SRT_PROBE_CLASSIFY_RELOCATE and s0 < margin.  For m = 1 .. steps ascending: t = (float)m * dt; for every k the
 *    offset is o_a = (d_k.a * t) * spacing_a and the candidate x_a = g_a + o_a; a candidate is accepted if S(x) >= margin.  At
 *    the first m with an accepted candidate the one with the largest S(x) as a binary32 value wins, on equal values the lowest
 *    k: state = MOVED, plus INSIDE if s0 < 0, offset o.  If no m has one: s0 < 0 ? BURIED|INSIDE : CLEAR, offset 0.
 * S5. Outputs, a bit mask.  SRT_PROBE_STATE_RECORDS: P float4 (o.x, o.y, o.z, the state's uint32 bits in w).
 *    SRT_PROBE_STATE_POSITIONS, optional: P float4 (g_a + o_a, w = 0), srt_write_light_probes' layout, so the buffer can be bound
 *    with srt_bind_light_probes and nothing crosses the bus.  Each is the handle's own buffer (allocated on first use, grown when
 *    a call needs more) or the caller's: srt_bind_probe_states_output binds a DEVICE buffer, NULL = own, under
 *    srt_bind_probe_depth_output's rules.  srt_read_probe_states_output waits, then copies what the last srt_classify_probes
 *    wrote of that output, from the buffer it wrote; SRT_ERR_STATE when the last call did not write it.
 * S6. Determinism.  No atomics reach an output; repeated calls give the same bits.
 * S7. Work counts.  With SRT_PROBE_CLASSIFY_COUNT_WORK the launch counts, deterministically: its probes (P), those with INSIDE,
 *    MOVED, BURIED and IDLE, the candidate positions evaluated (K per step a searching probe ran) and the waves of the launch.
 *    One vector atomic per wave at the end; without the flag there are no atomics at all.  srt_get_probe_classify_work waits and
 *    copies the record of the last srt_classify_probes; SRT_ERR_STATE unless that call had the flag.
 * S8. Parameters.  clearance: finite, 0 < clearance <= 0.5; max_offset: finite, 0 < max_offset <= 0.5, a fraction of the spacing,
 *    so with directions no longer than 1 a probe never leaves its cell neighbourhood; steps: 1 .. 64.
 * S9. Errors, all found before anything is touched, in this order: SRT_ERR_STATE before srt_set_scene; SRT_ERR_INVALID_ARG for
 *    unknown flags or outputs, outputs == 0, a clearance or max_offset outside its range (a NaN included), steps outside 1 .. 64
 *    or a non-zero reserved; SRT_ERR_STATE with no grid, or (with SRT_PROBE_CLASSIFY_RELOCATE) no directions; SRT_ERR_OOM when
 *    a buffer cannot be had.  Asynchrony: as rule 8 of the light-probe block. */
#define SRT_PROBE_STATE_RECORDS 1u      /* output: P float4 (offset, state bits) */
#define SRT_PROBE_STATE_POSITIONS 2u    /* output: P float4 (position, 0), optional */
#define SRT_PROBE_CLASSIFY_RELOCATE 1u  /* flags: rule S4 */
#define SRT_PROBE_CLASSIFY_NORMALIZE 2u /* flags: as SRT_RAYS_NORMALIZE */
#define SRT_PROBE_CLASSIFY_COUNT_WORK 4u /* flags: fill srt_probe_classify_work for this call */
#define SRT_PROBE_CLEAR 0u              /* state bits in a record's w lane */
#define SRT_PROBE_MOVED 1u              /* stands at grid position + offset */
#define SRT_PROBE_BURIED 2u             /* inside an object and not moved out: shading skips it */
#define SRT_PROBE_INSIDE 4u             /* the grid position lies inside an object */
#define SRT_PROBE_IDLE 8u               /* clear, and no analytic surface comes near any of its eight cells */

typedef struct srt_probe_classify_params { /* 24 bytes */
    float clearance;                       /* margin = clearance * smallest spacing; (0, 0.5] */
    float max_offset;                      /* longest offset as a fraction of the spacing; (0, 0.5] */
    uint32_t steps;                        /* 1..64 offset lengths tried, ascending */
    uint32_t flags;                        /* SRT_PROBE_CLASSIFY_RELOCATE | _NORMALIZE | _COUNT_WORK */
    uint32_t outputs;                      /* SRT_PROBE_STATE_RECORDS | _POSITIONS, not 0 */
    uint32_t reserved;                     /* 0 */
} srt_probe_classify_params;

typedef struct srt_probe_classify_work { /* 64 bytes */
    uint32_t valid, reserved;            /* 1, 0 */
    uint64_t probes;                     /* P */
    uint64_t inside, moved, buried, idle; /* probes whose state has that bit */
    uint64_t candidates;                 /* candidate positions evaluated: K per step run */
    uint64_t waves;                      /* waves of the launch */
} srt_probe_classify_work;

/* clearance 0.2f, max_offset 0.45f, steps 8, flags 0, outputs SRT_PROBE_STATE_RECORDS, reserved 0 (pure host). */
int srt_probe_classify_params_default(srt_probe_classify_params* out);
int srt_classify_probes(srt_context* ctx, const srt_probe_classify_params* params);
int srt_bind_probe_states_output(srt_context* ctx, uint32_t output, void* d_ptr);
int srt_read_probe_states_output(srt_context* ctx, uint32_t output, void* dst);
int srt_get_probe_classify_work(srt_context* ctx, srt_probe_classify_work* out);

/* ---- probe-grid shading that obeys the probe states (ABI 7, backward compatible) -------------------------------------------------
 * srt_shade_probe_grid_states(ctx, params, depth) is srt_shade_probe_grid (depth == NULL) or srt_shade_probe_grid_depth (otherwise)
 * rule for rule — the same grid, coefficients, depth maps, guides, band and band weights, the same output slot and the same "last
 * call" record (srt_get_probe_grid_work) — except for two rules:
 * 3s. After rule 3, rec = states[k] for the clamped probe index k of rule 8 (one 16-byte load).  A corner whose record has
 *    SRT_PROBE_BURIED is skipped before rule 5 and enters no counter.  IDLE, MOVED and INSIDE are not looked at.
 * 4s. p_a = (origin_a + (float)(i_a + c_a) * spacing_a) + rec.o_a.  Rules 5, 6, 7b, 8 and 9 use that p.  The trilinear weights
 *    stay the grid's.  The coefficients and moments are expected to have been traced at the relocated positions.
 * The states are P = nx*ny*nz float4 in SRT_PROBE_STATE_RECORDS' layout.  srt_write_probe_grid_states copies them from the host
 * into the handle's own array and waits; srt_bind_probe_grid_states binds a DEVICE array, does not copy and does not wait (what
 * srt_bind_probe_states_output filled can be bound here); NULL, 0 returns to the own array.  1 <= probes <= 2^30, otherwise
 * SRT_ERR_INVALID_ARG and the previous states stay.
 * Flags: SRT_PROBE_GRID_VISIBILITY is SRT_ERR_INVALID_ARG, found where an unknown flag is: the exact test towards relocated
 * probes needs a tracing kernel and is out of scope.  Without depth the work record's segments and open are 0, as they are for
 * srt_shade_probe_grid without the query.  Extra errors, after all of the parent call's: SRT_ERR_STATE for no states, or for a
 * state count other than nx*ny*nz.
 * Pinned domain.  Finite offsets are pinned bit for bit.  Other values give some value and no fault: indices stay clamped. */
int srt_write_probe_grid_states(srt_context* ctx, const float* records, size_t probes);
int srt_bind_probe_grid_states(srt_context* ctx, const void* d_ptr, size_t probes);
struct srt_probe_grid_depth_params; /* (defined in the filtered-shading block below) */
int srt_shade_probe_grid_states(srt_context* ctx, const srt_probe_grid_params* params, const struct srt_probe_grid_depth_params* depth);

/* ---- probe depth moments: a filtered estimate of what a probe sees (ABI 7, backward compatible) ---------------------------------
 * These calls were added without changing anything above, so SRT_ABI_VERSION stays 7.  A sequence of calls that uses none of
 * them runs what it ran before, bit for bit.
 *
 * SRT_PROBE_GRID_VISIBILITY answers "does this probe see this point" with one exact any-hit query per corner per pixel per frame:
 * a hard bit whose cost grows with the scene.  srt_trace_probe_depth instead gives every probe an octahedral map of R x R texels
 * that holds, per texel direction, the weighted mean and mean square of the distance to the nearest surface over the K shared
 * directions, once per probe update.  srt_shade_probe_grid_depth (the next block) turns the two moments into a smooth weight.
 * The probes and directions are the current ones of the light-probe block (srt_write_light_probes, srt_bind_light_probes,
 * srt_write_light_probe_directions, srt_bind_light_probe_directions): there are no new input calls.
 *
 * Rules.  All arithmetic is binary32 without contraction.
 * 1. Texel directions.  srt_probe_depth_texels gives texel (i, j), 0 <= i, j < R, the index j*R + i.  In double:
 *    u = (2i + 1) / R - 1, v = (2j + 1) / R - 1, z = 1 - |u| - |v|; if z < 0: (x, y) = ((1 - |v|) * sgn u, (1 - |u|) * sgn v),
 *    otherwise (x, y) = (u, v), where sgn of a number >= 0 is +1 and -1 otherwise; (x, y, z) is normalised in double, each
 *    component is rounded once to binary32, and w = 0.  The device reads this table; it does not recompute it.
 * 2. Distance.  Ray (p, k) has origin position_p and direction d_k, or float3::Normalized(d_k) with SRT_PROBE_DEPTH_NORMALIZE
 *    (as SRT_RAYS_NORMALIZE).  Let t be what srt_trace_rays writes into SRT_GBUF_NORMAL_DEPTH.w for that ray: the hit distance,
 *    or +inf on a miss.  r = !(t > 0) ? 0 : (t > max_distance ? max_distance : t).  A probe inside a sphere gets the negative
 *    distance Sphere::Raytrace reports, so r = 0; a NaN direction misses, so r = max_distance.  DISTANCES[p*K + k] = r.
 * 3. Accumulation.  For probe p and texel tau with direction e, M1 = M2 = Wt = Ft = +0.0f; then for k = 0 .. K - 1 ascending:
 *    c = (e.x*d.x + e.y*d.y) + e.z*d.z with d as traced.  If c > 0: w = c, then s times w = w*w, then w = w * d_k.w (the
 *    direction's weight, unscaled); M1 = M1 + w*r; M2 = M2 + w*(r*r); Wt = Wt + w; and if r >= max_distance, Ft = Ft + w.
 *    A direction with !(c > 0) contributes nothing.
 * 4. Texel.  If Wt > 0: MOMENTS[p*R*R + tau] = (M1 / Wt, M2 / Wt, Wt, Ft / Wt).  Otherwise (max_distance,
 *    max_distance*max_distance, 0, 1).
 * 5. Determinism.  No atomics reach an output; the order of rule 3 is the only order; repeated calls give the same bits.
 * 6. Outputs, a bit mask: SRT_PROBE_DEPTH_MOMENTS, P*R*R float4, and SRT_PROBE_DEPTH_DISTANCES, P*K float, optional.  Each is
 *    the handle's own buffer (allocated on first use, grown when a call needs more) or the caller's: srt_bind_probe_depth_output
 *    binds a DEVICE buffer, NULL = own, under srt_bind_light_probe_output's rules.  Without DISTANCES nothing of size P*K is
 *    allocated.  srt_read_probe_depth_output waits, then copies what the last srt_trace_probe_depth wrote of that output, from
 *    the buffer it wrote; SRT_ERR_STATE when the last trace did not write it.  Asynchrony: as rule 8 of the light-probe block;
 *    positions, directions and output buffers are those current at enqueue.  The call leaves alone everything
 *    srt_trace_light_probes leaves alone, and the light-probe outputs and records as well.
 * 7. Errors, all found before anything is touched, in this order: SRT_ERR_STATE before srt_set_scene; SRT_ERR_INVALID_ARG for
 *    unknown flags or outputs, outputs == 0, a resolution not in {4, 8, 16}, sharpness > 6, a max_distance that is NaN, infinite
 *    or <= 0, or a non-zero reserved; SRT_ERR_STATE with no positions or no directions; SRT_ERR_INVALID_ARG for P*K > 2^30 or
 *    P*R*R > 2^30; SRT_ERR_OOM when a buffer cannot be had.
 * 8. Work counts.  With SRT_PROBE_DEPTH_COUNT_WORK the launch counts, deterministically: its probes (P), its rays (P*K), the rays
 *    with r >= max_distance, the wave-level closest-hit invocations and the waves of the launch.  One vector atomic per wave at
 *    the end; without the flag there are no atomics at all.  srt_get_probe_depth_work waits and copies the record of the last
 *    srt_trace_probe_depth; SRT_ERR_STATE unless that trace had the flag. */
#define SRT_PROBE_DEPTH_MOMENTS 1u    /* output: P*R*R float4 */
#define SRT_PROBE_DEPTH_DISTANCES 2u  /* output: P*K float, optional */
#define SRT_PROBE_DEPTH_NORMALIZE 1u  /* flags: as SRT_RAYS_NORMALIZE */
#define SRT_PROBE_DEPTH_COUNT_WORK 2u /* flags: fill srt_probe_depth_work for this call */

typedef struct srt_probe_depth_params { /* 24 bytes */
    uint32_t resolution;                /* R: 4, 8 or 16 texels per side of a probe's octahedral map */
    uint32_t sharpness;                 /* s, 0..6: a direction weighs cos^(2^s) */
    float max_distance;                 /* > 0, finite */
    uint32_t flags;                     /* SRT_PROBE_DEPTH_NORMALIZE | _COUNT_WORK */
    uint32_t outputs;                   /* SRT_PROBE_DEPTH_MOMENTS | _DISTANCES, not 0 */
    uint32_t reserved;                  /* 0 */
} srt_probe_depth_params;

typedef struct srt_probe_depth_work { /* 48 bytes */
    uint32_t valid, reserved;         /* 1, 0 */
    uint64_t probes, rays;            /* P; P*K */
    uint64_t far_rays;                /* rays with r >= max_distance */
    uint64_t wave_calls;              /* wave-level closest-hit invocations: P * ceil(K / 64) */
    uint64_t waves;                   /* waves of the launch */
} srt_probe_depth_work;

/* resolution 16, sharpness 5, max_distance 10000.0f, flags 0, outputs SRT_PROBE_DEPTH_MOMENTS, reserved 0 (pure host). */
int srt_probe_depth_params_default(srt_probe_depth_params* out);
/* Pure host, no device: fills resolution * resolution float4 with rule 1's texel directions.  SRT_ERR_INVALID_ARG for a resolution
 * not in {4, 8, 16} or a NULL dst. */
int srt_probe_depth_texels(uint32_t resolution, float* dst);
int srt_trace_probe_depth(srt_context* ctx, const srt_probe_depth_params* params);
int srt_bind_probe_depth_output(srt_context* ctx, uint32_t output, void* d_ptr);
int srt_read_probe_depth_output(srt_context* ctx, uint32_t output, void* dst);
int srt_get_probe_depth_work(srt_context* ctx, srt_probe_depth_work* out);

/* ---- probe-grid shading with the filtered visibility test (ABI 7, backward compatible) ------------------------------------------
 * srt_shade_probe_grid_depth is srt_shade_probe_grid rule for rule — the same grid, coefficients, guides, band and band weights,
 * the same output slot (srt_bind_probe_grid_output, srt_read_probe_grid_output) and the same "last call" record
 * (srt_get_probe_grid_work serves both calls) — with the probe-grid block's rule 7 replaced by rule 7b below, applied after rule 6.
 * Accepted flags: SRT_PROBE_GRID_NORMAL_WEIGHT, _ALBEDO and _COUNT_WORK.  SRT_PROBE_GRID_VISIBILITY is SRT_ERR_INVALID_ARG here,
 * found where an unknown flag is: the exact and the filtered test exclude each other.  srt_shade_probe_grid itself is unchanged.
 *
 * The depth maps are P = nx*ny*nz probes of R*R float4 in SRT_PROBE_DEPTH_MOMENTS' layout (probe k's texel tau at k*R*R + tau;
 * the x and y lanes are read).  srt_write_probe_grid_depth copies them from the host into the handle's own array and waits;
 * srt_bind_probe_grid_depth binds a DEVICE array, does not copy and does not wait (what srt_bind_probe_depth_output filled can
 * be bound here); NULL, 0 returns to the own array.  Both want R in {4, 8, 16}, 1 <= probes and probes*R*R <= 2^30, and return
 * SRT_ERR_INVALID_ARG otherwise, leaving the previous maps.
 *
 * 7b. Filtered visibility, for a corner that reached rule 7 (weight > 0 and L > 0), with d and L of rule 5 and the clamped probe
 *    index k of rule 8:
 *    Texel lookup.  q = (-d.x, -d.y, -d.z); s = (|q.x| + |q.y|) + |q.z|; u = q.x / s, v = q.y / s.  If q.z < 0:
 *    u' = (1 - |v|) * sgn u and v' = (1 - |u|) * sgn v, then (u, v) = (u', v'); sgn of a number >= 0 is +1, otherwise -1.
 *    Per axis, with g standing for u or v: a = ((g*0.5f) + 0.5f) * (float)R; a = !(a > 0) ? 0 : (a > (float)(R-1) ? (float)(R-1) : a);
 *    the index is (int)a.  tau = j*R + i with i taken from u and j from v.
 *    Moments.  (m1, m2) = the x and y lanes of depth[k*R*R + tau]: no load can leave the array.
 *    Weight.  Only if L > m1 + bias: var = |m2 - m1*m1|; var = var > min_variance ? var : min_variance; D = L - m1;
 *    ch = var / (var + D*D); t = t * ((ch*ch)*ch).
 *    Skip.  A corner with !(t > 0) is skipped.
 *    Work counts.  `segments` holds the corners that reach 7b, `open` those that survive it; the three test counters are 0.
 *    Extra errors, after all of rule 16's: SRT_ERR_STATE for no depth maps, or for a depth probe count other than nx*ny*nz; then
 *    SRT_ERR_INVALID_ARG for a bias that is NaN, infinite or < 0, a min_variance that is NaN, infinite or <= 0, or a non-zero
 *    reserved word.
 *    Pinned domain.  Finite moments are pinned bit for bit.  Other values give some value and no fault. */
typedef struct srt_probe_grid_depth_params { /* 16 bytes */
    float bias;                              /* >= 0, finite */
    float min_variance;                      /* > 0, finite */
    uint32_t reserved[2];                    /* 0 */
} srt_probe_grid_depth_params;

/* bias 0.0f, min_variance 1e-4f, reserved 0 (pure host). */
int srt_probe_grid_depth_params_default(srt_probe_grid_depth_params* out);
int srt_write_probe_grid_depth(srt_context* ctx, const float* moments, size_t probes, uint32_t resolution);
int srt_bind_probe_grid_depth(srt_context* ctx, const void* d_ptr, size_t probes, uint32_t resolution);
int srt_shade_probe_grid_depth(srt_context* ctx, const srt_probe_grid_params* params, const srt_probe_grid_depth_params* depth);

/* ---- sun sampling at diffuse bounces (ABI 7, backward compatible) ---------------------------------------------------------------
 * One flag bit, value 16, on two existing parameter structs: SRT_RADIANCE_SUN_SAMPLING (srt_trace_radiance) and
 * SRT_LIGHT_PROBE_SUN_SAMPLING (srt_trace_light_probes, srt_trace_light_probes_listed), defined next to the flags they join
 * (written 0x10u: the decimal constants of the two passes as they shipped are a closed set that their ABI tests keep pinned).  No entry point, no exported symbol; without
 * the flag every call launches the kernel it launched before.  Every path otherwise finds the sun by accident: GetEnvironmentColor
 * adds SunColor where dot(d, -SunDirection) > 0.99, and a diffuse bounce draws its direction blindly.  With the flag every diffuse
 * vertex sends one shadow segment to a point of that cap, and its own bounce sees the environment without the sun: next-event
 * estimation for the sun, converging to what the calls converge to without the flag.
 *
 * Binary32 without contraction throughout.  G = 0x9E3779B9; c is the float 0x3F7D70A4, GetEnvironmentColor's threshold as a float
 * compare; k = 1.0f - c; W0 = (float)(3.14159265358979323846 / 6.0 * (double)k).
 *
 * S1. Where the flag applies.  The path of radiance rule 2 is unchanged: the main stream's draws and their order, every bounce
 *     direction, every GetClosestObject call, the alpha lane, the fold.  Only the colour L changes.  With max_bounces == 0, or at a
 *     primary miss, nothing changes.
 * S2. Which vertex is diffuse.  A vertex is diffuse when tt = Smoothness * specularProb (Raytracer.cpp:175) == 0.0f.  Every other
 *     vertex is treated as without the flag, the sun inside its environment term.
 * S3. The sun stream of the vertex of loop iteration b.  With i, i+1, i+2 the indices of that iteration's three hemisphere draws
 *     in the stream of key = srt_rng_key(seed, id, f):  ks = srt_mix32((key + (i + 3) * G) ^ 0x53554E21u); the sun's draws are
 *     srt_rng_draw(ks, j).  The main stream is not advanced.
 * S4. Sampling the cap.  For J = 0 .. 7: a = (rand_unit(draw 2J) - 0.5f) * 2, b = (rand_unit(draw 2J + 1) - 0.5f) * 2,
 *     q = a*a + b*b (rand_unit(r) = (float)r / 32767.0f); take the first J with q <= 1, and a = b = q = 0 if there is none
 *     (probability 0.215^8).  Then z = 1 - q*k, h = sqrtf(k * (1 + z)), w' = (t1*(a*h) + t2*(b*h)) + s*z per component, in that
 *     order, w = float3::Normalized(w'): Lambert's equal-area map of the disc onto the cap, without trigonometry.
 * S5. The frame, made on the host once per enqueue from the environment captured there: s = sun_direction * -1,
 *     e = |s.x| < 0.5f ? (1,0,0) : (0,1,0), t1 = Normalized(cross(e, s)), t2 = cross(s, t1), the cross products written out
 *     component by component.  The flag is refused with SRT_ERR_STATE, after the call's own argument errors and before anything is
 *     touched, when a component of s is not finite or (s.x*s.x + s.y*s.y) + s.z*s.z lies outside [0.9999, 1.0001], and when the
 *     context's probe-tail mode is on (the combination is not built).
 * S6. The segment.  At a diffuse vertex with point p, normal n and the throughput T its bounce's result meets (after this
 *     iteration's x 0.8): sd = (w.x*s.x + w.y*s.y) + w.z*s.z, cn = (w.x*n.x + w.y*n.y) + w.z*n.z.  If sd >= c && cn > 0 the segment
 *     (p + n * .00001f, w, t_max = +inf) is traced by srt_trace_occlusion's predicate; if it is open, m = max(|w.x|, |w.y|, |w.z|),
 *     weight = W0 / ((m*m)*m) (one IEEE division) and L_l = L_l + ((Sun_l * weight) * T_l) for l = 0, 1, 2, Sun the clamped sun
 *     colour.  The add comes BEFORE the add of the same iteration's bounce result.  (The blind bounce is a normalised point of
 *     the cube [-1, 1]^3 folded into the normal's hemisphere — GetRandomDirection's rejection test never rejects — with density
 *     1 / (12 m^3) per steradian, not 1 / (2 pi): the cap of solid angle 2 pi k is met with probability (pi k / 6) / m^3.)
 * S7. The blind bounce of a diffuse vertex.  When its ray leaves the scene it adds E0(ray) * T, E0 being GetEnvironmentColor with
 *     SunColor = (0, 0, 0): its last line adds + 0.0f.  The alpha tag is as before.
 * S8. Invariants.  With SunColor = (0, 0, 0) the outputs are bit for bit those without the flag.  In a scene without a diffuse
 *     vertex (SpecularAmount >= 1 and Smoothness > 0 everywhere) the outputs and the work record are those without the flag.
 *     Radiance rules 3 - 6 hold under the flag (mean, camera-ray equivalence with the flag on both sides, splitting, continuation);
 *     srt_trace_light_probes' RADIANCE equals srt_trace_radiance on the explicit rays under the flag, its COEFFICIENTS are the
 *     fixed-order projection of that RADIANCE, and the listed call writes at the listed probes what the unlisted call writes.
 * S9. Work.  Under the flag wave_calls of srt_radiance_work (and of srt_light_probe_work) additionally counts one for every
 *     wave-level any-hit invocation; closest_calls is unchanged.  The number of sun segments is not reported.
 * srt_render does not take the flag, and srt_trace_radiance and the light-probe traces refuse it under the probe-tail mode;
 * srt_render_adaptive and srt_render_adaptive_tail take it as SRT_ADAPTIVE_SUN_SAMPLING, the latter together with the probe tail:
 * the next block. */

/* ---- sun sampling in adaptive renders (ABI 7, backward compatible) ---------------------------------------------------------------
 * One flag bit, value 16, on srt_adaptive_params.flags: SRT_ADAPTIVE_SUN_SAMPLING, defined next to the two adaptive flags (written
 * 0x10u for the reason given above), accepted by srt_render_adaptive and srt_render_adaptive_tail.  No entry point, no exported
 * symbol, no struct, so SRT_ABI_VERSION stays 7; without the flag both calls launch the kernel they launched before.  Bits 4 and
 * 8 stay unassigned and refused with SRT_ERR_INVALID_ARG.  It is sun sampling (rules S1 - S9 above) for pictures: per-pixel counts,
 * budgets, a framebuffer — and, in srt_render_adaptive_tail, the one-bounce frame that ends in the probe grid.
 *
 * AS1. srt_render_adaptive with the flag.  Adaptive rules 1 - 10 hold unchanged.  Every sample's path follows S1 - S9 with id = the
 *      pixel index x + y*W and f = the sample's frame.  Only the colour changes: the draws, the directions, the GetClosestObject
 *      calls and the fold are untouched.  The call ignores the context's probe-tail mode, as before: the tail-mode refusal of S5
 *      does not apply to it.
 * AS2. Equivalence.  After the call, pixel p's accumulator element equals element p of srt_trace_radiance with
 *      SRT_RADIANCE_SUN_SAMPLING on the frame's camera rays — ray index x + y*W, id_base 0, the same seed and bounces,
 *      first_sample = n_p + 1, sample_count = e_p — continuing from the element the pixel held by radiance's continuation rule, or
 *      with SRT_RADIANCE_RESET when n_p = 0; in all four lanes, NaN as NaN.  The framebuffer pixel is its tone map at the memory
 *      row of adaptive rule 3.
 * AS3. Mixing is allowed.  Samples with the flag and samples without it estimate the same quantity and may share one mean: a pixel
 *      that took frames 1..n without the flag (srt_render or srt_render_adaptive) and n+1..n+e with it holds the running mean in
 *      frame order, each frame computed under its own call's flag.  (R3 forbids such mixing for the tail: a path that ends in the
 *      probe grid estimates a different quantity from one that does not.  The sun flag only changes how the same quantity is
 *      estimated.)
 * AS4. srt_render_adaptive_tail with the flag: the combination, built for pictures only.  R1 - R7 hold.  Every sample's path
 *      follows S1 - S4 and S6 - S9, and T1 - T6.  A vertex from which a bounce is taken gets its sun segment, as without the tail.
 *      The vertex at which the path reaches the bounce limit takes no bounce, so it gets no segment; it gets the lookup of T1 - T6,
 *      unchanged.  The bounce that led to that vertex — like every bounce — met the environment under its own vertex's no_sun
 *      (S7) had it left the scene.  The expectation is that of the same call without the flag.  srt_trace_radiance and the
 *      light-probe traces keep refusing the flag under the mode, so R3's equivalence has no radiance counterpart under AS4.
 * AS5. Order of checks.  srt_render_adaptive: first the call's own errors in their order (rule 9), evaluated with the bit masked
 *      off; then S5's direction test: SRT_ERR_STATE when a component of s is not finite or its squared length lies outside
 *      [0.9999, 1.0001].  srt_render_adaptive_tail: all of R1 first, the direction test last.  The direction test runs whenever the
 *      bit is set, also with max_bounces == 0, as in srt_trace_radiance.  Nothing is touched on a refusal.
 * AS6. max_bounces == 0.  An accepted call launches exactly what it launches without the flag: srt_render_adaptive's kernel, also
 *      for the tail call (R2).
 * AS7. Invariants.  With SunColor = (0, 0, 0) the accumulator, the framebuffer and the counts are bit for bit those without the
 *      flag.  In a scene without a diffuse vertex those buffers and srt_adaptive_work are those without the flag.  Adaptive rules
 *      4 - 8 hold under the flag (untouched pixels, counts and KEEP_COUNTS, determinism, the rest).  R4 holds with the flag on both
 *      sides: zero coefficients give srt_render_adaptive's buffers.
 * AS8. Work.  Under the flag srt_adaptive_work.wave_calls additionally counts one for every wave-level any-hit invocation;
 *      pixels, samples and closest_calls are unchanged.  The count is deterministic: a tile's pool drains before its wave draws
 *      the next ticket.  srt_probe_tail_work is unchanged by the flag.
 * Not built: the flag in srt_render, the combination in srt_trace_radiance and the light-probe traces, a sun segment at the path's
 * last vertex, emissive objects, glossy vertices. */

#ifdef __cplusplus
}
#endif
#endif /* SRT_PATHTRACE_H */
