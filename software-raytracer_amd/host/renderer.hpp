// renderer.hpp — host C++ that owns camera, settings and the progressive-sample state and
// drives the C-ABI (include/srt_pathtrace.h).  It stands where the reference's main loop
// stands relative to its workers (Raytracer/Raytracer.cpp:329-342, 373-384, 572-595).
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "scene.hpp"
#include "srt_pathtrace.h"

namespace srt_host {

struct Vec3 {  // the members of Common.hpp's float3 that Transform uses
    float x = 0, y = 0, z = 0;
    Vec3() = default;
    Vec3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
    Vec3 operator+(const Vec3& o) const { return {x + o.x, y + o.y, z + o.z}; }
    Vec3 operator-(const Vec3& o) const { return {x - o.x, y - o.y, z - o.z}; }
    Vec3 operator*(float s) const { return {x * s, y * s, z * s}; }  // float3 * float3(s)
    static float Dot(const Vec3& l, const Vec3& r) { return (l.x * r.x + l.y * r.y + l.z * r.z); }
    static Vec3 Cross(const Vec3& l, const Vec3& r) {  // Common.hpp:94-96
        return {l.y * r.z - r.y * l.z, r.x * l.z - l.x * r.z, l.x * r.y - r.x * l.y};
    }
};

// Transform (Common.hpp:281-292)
struct Transform {
    Vec3 right{1, 0, 0};
    Vec3 up{0, 1, 0};
    Vec3 forward{0, 0, 1};
    Vec3 position{0, 0, 0};
    Vec3 scale{1, 1, 1};
    // Rodrigues rotation of the three basis vectors (Common.hpp:287-291)
    void RotateAboutAxis(float angle, Vec3 axis) {
        forward = forward * cosf(angle) + Vec3::Cross(axis, forward) * sinf(angle) + axis * Vec3::Dot(axis, forward) * (1 - cosf(angle));
        up = up * cosf(angle) + Vec3::Cross(axis, up) * sinf(angle) + axis * Vec3::Dot(axis, up) * (1 - cosf(angle));
        right = right * cosf(angle) + Vec3::Cross(axis, right) * sinf(angle) + axis * Vec3::Dot(axis, right) * (1 - cosf(angle));
    }
};

class RendererError : public std::runtime_error {
   public:
    RendererError(int code, const std::string& m) : std::runtime_error(m), code_(code) {}
    int code() const { return code_; }

   private:
    int code_;
};

// One GPU, one image (or one row band of it).
class PathTraceRenderer {
   public:
    // the reference's mutable globals (Raytracer.cpp:30-35,47-48,53) as members, same defaults
    float SCREEN_SCALE = .5f;
    int FOV = 55;
    int MAXBOUNCES = 2;
    int TARGETFRAMES = 4096;
    int ACCUMULATIONFRAMES = 1;
    bool SIMPLEDRAW = true;
    float progressiveResolutionScaler = 1;  // :47, set to 1 at :271
    bool setFrame = false;                  // :48
    int selectedObject = -1;                // :53 as an index into ObjectsToRender, -1 = NULL
    static constexpr int THREADS = 16;      // :28 — only used for the block anchoring of :235,330
    uint32_t seed = 0;  // the reference only ever names srand(0) (:263)
    // not in the reference: RenderFrame follows a frame of steps x steps blocks (steps > 1) with the first-hit guides and
    // srt_upsample into the framebuffer, so that the frame shown is reconstructed from the blocks' anchors instead of made of
    // squares.  The accumulator stays what the reference accumulates.  Whole frame only.
    bool guidedUpsample = false;
    // not in the reference: 1..4 makes RenderFrame and RenderTemporalFrame end in the anti-aliasing resolve (srt_antialias with
    // this k and SRT_AA_FRAMEBUFFER); 0 = off.  The accumulator stays what the reference accumulates.  Whole frame only.
    int antialias = 0;
    // not in the reference: RenderTemporalFrame also keeps the luminance moments of the history (srt_moments_output with
    // SRT_VARIANCE_ALBEDO) and, when it denoises, runs srt_temporal_variance + srt_denoise_variance at the library's defaults
    // where it otherwise runs srt_denoise: the per-pixel variance of a temporal frame at one render per frame.
    bool temporalVariance = false;
    // not in the reference: SetScene and UpdateScene run under SRT_UPDATE_REFIT (srt_update_mode), so an UpdateScene that only
    // moves objects refits the mesh BVH on the device instead of rebuilding it on the host.  Same pictures; read when a scene
    // is set or updated, so a scene set before it was switched on rebuilds once more.
    bool refitUpdates = false;
    Transform camera;   // :295-297

    PathTraceRenderer(int device, int width, int height);
    ~PathTraceRenderer();
    PathTraceRenderer(const PathTraceRenderer&) = delete;
    PathTraceRenderer& operator=(const PathTraceRenderer&) = delete;

    int width() const { return width_; }
    int height() const { return height_; }
    srt_context* handle() { return ctx_; }

    // ObjectsToRender = scene.GetObjects(); doSetFrame = true   (:293, :421-423)
    void SetScene(const Scene& scene);
    // An object edit that keeps the temporal history (srt_update_scene): the same list with other positions (or other fields,
    // whose objects then restart their own pixels).  doSetFrame = true for the plain accumulate loop, as any edit; the next
    // RenderTemporalFrame does NOT reset but reprojects every object by its displacement.  Falls back to SetScene when no
    // scene was set, the number of objects changed or the geometry of a mesh changed (srt_update_scene keeps the meshes of
    // the last srt_set_meshes).
    void UpdateScene(const Scene& scene);
    // what the last UpdateScene that reached srt_update_scene did to the mesh image (srt_get_update_info)
    srt_update_info UpdateInfo();
    void SetEnvironment(const srt_environment& env);
    // restrict rendering to memory rows [begin,end) (multi-GPU row stripes)
    void SetRowBand(int begin, int end);
    void RowBand(int* begin, int* end) const { *begin = row_begin_, *end = row_end_; }
    // doSetFrame = true: any camera / object / setting edit (:391,453,461,469,476,497,522).  Also drops the temporal
    // history: the next RenderTemporalFrame starts afresh (SRT_TEMPORAL_RESET).  A temporal camera move changes `camera`
    // without calling this.
    void Invalidate() { doSetFrame_ = true, temporal_reset_ = true; }

    // One iteration of the reference's frame loop as far as rendering is concerned: the
    // accumulate state machine (:572-590) followed by releasing the workers for ONE frame
    // (:592-595) with the globals as they then stand — including SIMPLEDRAW (preview shader),
    // the steps x steps progressive blocks (steps = ceil(1/(SCREEN_SCALE*scaler)), :233) anchored
    // at the 16 worker stripes (:330-340), and the reference's quirk that the first full
    // resolution frame after an edit has setFrame == true AND ACCUMULATIONFRAMES == 2.
    // The very first call renders with the start-up globals, as the workers do before the
    // loop's first pass.  Returns false when nothing was launched (ACC == TARGETFRAMES, :572).
    // With guidedUpsample a frame of blocks is followed by RenderGBuffer (the three guides) and Upsample with the library's
    // defaults, the frame's own steps and stripe_width and SRT_UPSAMPLE_FRAMEBUFFER — never in place; SRT_ERR_STATE when the
    // renderer has a row band.  Without it the calls are exactly the above.
    // With antialias = k > 0 the frame ends in Antialias(k): the OBJECT guide and the k x k sub-samples are rendered when the
    // scene, the camera or k has changed since they were last rendered — once per change, not per frame — and srt_antialias
    // resolves the accumulator into the framebuffer.  A frame the upsampler has just reconstructed (guidedUpsample, steps > 1)
    // is shown as the upsampler left it: its result is not a source of srt_antialias.  SRT_ERR_STATE with a row band.
    bool RenderFrame();
    // Picking (:525-541): x, y in window coordinates (y down, as the mouse reports it)
    int Pick(int mouse_x, int mouse_y);

    // Clean sequence used by benchmarks and fixtures: `count` further samples in ONE
    // launch; the first call after Invalidate() starts at sample 1 with reset.  steps > 1: one ray per steps x steps block
    // (a single stripe: anchors at x = 0), as srt_render_params.steps.
    void RenderSamples(uint32_t count, bool count_rays = false, int steps = 1);

    void Wait();
    bool Done();
    srt_stats Stats();
    // blit: copy the band into an SDL-surface-like buffer (renderSurface->pixels, :64)
    void ReadFramebuffer(void* pixels, size_t pitch_bytes);
    std::vector<float> ReadAccumulator();
    // First-hit buffers (srt_render_gbuffer) of the band with the current camera: `outputs` = SRT_GBUF_* bits.  Asynchronous;
    // ReadGBuffer waits and copies the whole W x H buffer of ONE output (int32 or float4 per pixel, scene rows).
    void RenderGBuffer(uint32_t outputs) { RenderGBufferRows(outputs, row_begin_, row_end_); }
    void RenderGBufferRows(uint32_t outputs, int row_begin, int row_end);  // any memory-row band (MultiGpuRenderer: the whole frame)
    void ReadGBuffer(uint32_t output, void* dst);
    // Ray queries (srt_write_rays + srt_trace_rays): the closest hit of `count` caller-supplied rays against the current scene.
    // origins / directions: count x 4 floats each, (o.xyz, ignored) and (d.xyz, t_max); outputs: SRT_GBUF_* bits and
    // SRT_RAYS_OCCLUDED; flags: 0 or SRT_RAYS_NORMALIZE.  No camera is involved.  Asynchronous once the rays are copied;
    // readRayOutput waits and copies the `count` elements of ONE output of the last traceRays (int32 or float4 per ray).
    void traceRays(const float* origins, const float* directions, size_t count, uint32_t outputs, uint32_t flags = 0);
    void readRayOutput(uint32_t output, void* dst);
    // Any-hit queries (srt_write_rays + srt_trace_occlusion): for each of `count` caller-supplied rays, is there a valid hit with
    // distance < t_max (directions' w)?  flags: SRT_OCCLUSION_* bits.  Asynchronous once the rays are copied; the result is the
    // SRT_RAYS_OCCLUDED output of readRayOutput (count int32), with the bits srt_trace_rays gives it.  occlusionWork waits and
    // returns the work counts of a trace that had SRT_OCCLUSION_COUNT_WORK.
    void traceOcclusion(const float* origins, const float* directions, size_t count, uint32_t flags = 0);
    srt_occlusion_work occlusionWork();
    // Radiance queries (srt_write_rays + srt_trace_radiance): the running mean of params.sample_count path-traced samples along
    // each of `count` caller-supplied rays — what Render leaves in the accumulator for a pixel, without a camera.  Asynchronous
    // once the rays are copied; readRadiance waits and copies the `count` float4 of the last traceRadiance; radianceWork waits and
    // returns the work counts of a trace that had SRT_RADIANCE_COUNT_WORK.  params.flags | SRT_RADIANCE_SUN_SAMPLING (and
    // SRT_LIGHT_PROBE_SUN_SAMPLING for traceLightProbes / traceLightProbesListed below): one shadow segment towards the sun at every
    // diffuse bounce, the sun taken out of that bounce (rules S1 - S9 of srt_pathtrace.h) — the same mean, far less noise in
    // sunlit scenes; throws (SRT_ERR_STATE) while the probe tail is on or when sun_direction is not a unit vector.
    void traceRadiance(const float* origins, const float* directions, size_t count, const srt_radiance_params& params);
    void readRadiance(float* dst_rgba);
    srt_radiance_work radianceWork();
    // Light probes (srt_write_light_probes + srt_write_light_probe_directions + srt_trace_light_probes): `probes` positions and
    // `directions` shared directions (float4 each; direction.w is the quadrature weight), path-traced as traceRadiance's rays and
    // projected onto nine SH coefficients per probe.  Asynchronous once the arrays are copied; readLightProbeOutput waits and copies
    // one output (SRT_LIGHT_PROBE_COEFFICIENTS: probes * 9 float4; SRT_LIGHT_PROBE_RADIANCE: probes * directions float4) of the
    // last traceLightProbes; lightProbeWork waits and returns the work counts of a trace that had SRT_LIGHT_PROBE_COUNT_WORK.
    void traceLightProbes(const float* positions, size_t probes, const float* directions, size_t direction_count, const srt_light_probe_params& params);
    void readLightProbeOutput(uint32_t output, float* dst);
    srt_light_probe_work lightProbeWork();
    // Probe-grid shading (srt_set_probe_grid + srt_write_probe_grid_coefficients + srt_shade_probe_grid): per-pixel irradiance at the
    // first hit from light probes on a regular grid.  setProbeGrid sets the grid.  shadeProbeGrid copies `probes` * 9 float4
    // coefficients (what readLightProbeOutput(SRT_LIGHT_PROBE_COEFFICIENTS) gives for srt_probe_grid_positions' probes; NULL: the
    // handle's current ones), renders the guides the pass reads (OBJECT, NORMAL_DEPTH, POSITION, and ALBEDO with
    // SRT_PROBE_GRID_ALBEDO) for the band with the current scene and camera, as renderVisibility, and enqueues the pass; a params
    // band of [0, 0) (srt_probe_grid_params_default's) means the renderer's own band.  Asynchronous once the coefficients are
    // copied.  readProbeGridOutput waits and copies the W x H float4 (scene rows); probeGridWork waits and returns the work counts
    // of a call that had SRT_PROBE_GRID_COUNT_WORK.
    void setProbeGrid(const srt_probe_grid& grid);
    void shadeProbeGrid(const float* coefficients, size_t probes, const srt_probe_grid_params& params);
    void readProbeGridOutput(float* dst_rgba);
    srt_probe_grid_work probeGridWork();
    // Probe depth moments (srt_trace_probe_depth) and the filtered probe-grid shading (srt_shade_probe_grid_depth).  traceProbeDepth
    // copies `probes` positions and `direction_count` directions as traceLightProbes does (they are the same current arrays) and
    // enqueues the pass; readProbeDepthOutput waits and copies one output of the last trace (SRT_PROBE_DEPTH_MOMENTS: probes * R*R
    // float4; SRT_PROBE_DEPTH_DISTANCES: probes * directions float); probeDepthWork waits and returns the work counts of a trace
    // that had SRT_PROBE_DEPTH_COUNT_WORK.  shadeProbeGridDepth is shadeProbeGrid with the filtered test: it also copies `probes`
    // * resolution^2 float4 moments (NULL: the handle's current ones); readProbeGridOutput and probeGridWork serve both calls.
    void traceProbeDepth(const float* positions, size_t probes, const float* directions, size_t direction_count, const srt_probe_depth_params& params);
    void readProbeDepthOutput(uint32_t output, void* dst);
    srt_probe_depth_work probeDepthWork();
    void shadeProbeGridDepth(const float* coefficients, const float* moments, size_t probes, uint32_t resolution, const srt_probe_grid_params& params,
                             const srt_probe_grid_depth_params& depth);
    // Probe classification and relocation (srt_classify_probes) on the grid of setProbeGrid, and the shading that obeys the records
    // (srt_shade_probe_grid_states).  classifyProbes copies `direction_count` directions (NULL: the handle's current ones; only a
    // relocating call reads them) and enqueues the pass; readProbeStatesOutput waits and copies one output of the last call
    // (SRT_PROBE_STATE_RECORDS or SRT_PROBE_STATE_POSITIONS: nx*ny*nz float4); probeClassifyWork waits and returns the counts of a
    // call that had SRT_PROBE_CLASSIFY_COUNT_WORK.  shadeProbeGridStates is shadeProbeGrid (depth == NULL) or shadeProbeGridDepth
    // with the records: it also copies `probes` float4 states (NULL: the handle's current ones).
    void classifyProbes(const float* directions, size_t direction_count, const srt_probe_classify_params& params);
    void readProbeStatesOutput(uint32_t output, void* dst);
    srt_probe_classify_work probeClassifyWork();
    void shadeProbeGridStates(const float* coefficients, const float* moments, const float* states, size_t probes, uint32_t resolution,
                              const srt_probe_grid_params& params, const srt_probe_grid_depth_params* depth);
    // Per-frame probe updates (srt_list_probes, the listed traces, srt_blend_probes).  listProbes copies `probes` state records (NULL:
    // the handle's current ones), lists the probes without a params.skip_mask bit, reads the 4 + probes words back and makes them
    // the list the listed traces read (through the host: waits); readProbeListOutput copies them again; probeListWork returns the
    // counts of a call that had SRT_PROBE_LIST_COUNT_WORK.  traceLightProbesListed / traceProbeDepthListed are traceLightProbes /
    // traceProbeDepth for the listed probes only (positions / directions NULL: the handle's current ones); the read and work calls
    // of the parents serve them.  resetProbeHistory sizes and zero-fills the handle's own histories (SRT_PROBE_HISTORY_* bits);
    // blendProbes folds the last traces' COEFFICIENTS (and MOMENTS) into them, copying `probes` previous records first unless
    // NULL; readProbeHistory waits and copies one history; probeBlendWork returns the counts of a counting blend.
    void listProbes(const float* states, size_t probes, const srt_probe_list_params& params);
    void readProbeListOutput(uint32_t* dst);
    srt_probe_list_work probeListWork();
    void traceLightProbesListed(const float* positions, size_t probes, const float* directions, size_t direction_count, const srt_light_probe_params& params);
    void traceProbeDepthListed(const float* positions, size_t probes, const float* directions, size_t direction_count, const srt_probe_depth_params& params);
    void resetProbeHistory(uint32_t which, size_t probes, uint32_t resolution);
    void blendProbes(const float* previous_states, size_t probes, const srt_probe_blend_params& params);
    void readProbeHistory(uint32_t which, float* dst);
    srt_probe_blend_work probeBlendWork();
    // Scrolling (srt_scroll_probes) of the grid of setProbeGrid.  scrollProbes moves the arrays of `which` (SRT_PROBE_SCROLL_* bits)
    // by `shift` cells with `flags` (SRT_PROBE_SCROLL_COUNT_WORK | _SET_GRID; with _SET_GRID the renderer's copy of the grid
    // follows by the header's rule SC4).  followProbeGrid is srt_probe_grid_follow on that grid, then scrollProbes with the two
    // histories that have been reset, _STATES and _SET_GRID; it returns the shift.  probeScrollWork returns the
    // counts of a counting scroll.
    void scrollProbes(const int32_t shift[3], uint32_t which, uint32_t flags);
    std::array<int32_t, 3> followProbeGrid(const float point[3]);
    srt_probe_scroll_work probeScrollWork();
    const srt_probe_grid& probeGrid() const { return probe_grid_; }  // setProbeGrid's, as the scrolls have moved it
    // Probe cascades (srt_set_probe_cascade, srt_capture_probe_cascade_level, srt_shade_probe_cascade): up to four nested grids,
    // level 0 the finest.  setProbeCascade sets the cascade.  A level is filled through the single-grid calls above (setProbeGrid
    // on the level's grid, classifyProbes, the traces, the blend, with their results written or bound as the current probe-grid
    // coefficients, depth moments and states), then captureProbeCascadeLevel copies what is current, as `which`
    // (SRT_PROBE_CASCADE_COEFFICIENTS | _MOMENTS | _RECORDS) selects, into the level on the device.  shadeProbeCascade renders the
    // guides as shadeProbeGrid does and enqueues the pass; a band of [0, 0) means the renderer's own; readProbeGridOutput reads the
    // result; probeCascadeWork returns the counts of a call that had SRT_PROBE_CASCADE_COUNT_WORK.
    void setProbeCascade(const srt_probe_cascade& cascade);
    void captureProbeCascadeLevel(uint32_t level, uint32_t which);
    void shadeProbeCascade(const srt_probe_cascade_params& params);
    srt_probe_cascade_work probeCascadeWork();
    // Adaptive sampling (srt_sample_budget, srt_render_adaptive), on the handle's buffers as they stand.  sampleBudget turns the
    // variance buffer, the sample counts, the accumulator and the guides into the per-pixel budget and returns its sum (waits).
    // renderAdaptive enqueues the adaptive render with the renderer's scene and camera; a band of [0, 0) means the renderer's
    // own.  setSampleCounts / readSampleCounts are srt_set_sample_counts / srt_read_sample_counts.
    // renderAdaptiveFrame is the two-half workflow of the header (whole frame only): spp / 2 uniform samples per half (seed and
    // seed ^ 0x9E3779B9, as denoiseVariance), the guides once, then `rounds` rounds of srt_variance without MERGE,
    // sampleBudget(budget) and renderAdaptive on half A (KEEP_COUNTS) and half B, and srt_variance with MERGE at the end: the
    // accumulator holds the mean of the halves.  Returns the samples of the frame, the sum over the pixels of twice the per-half
    // count; `counts`, when given, receives W x H per-pixel samples (both halves, scene rows).
    uint64_t sampleBudget(const srt_budget_params& params);
    void renderAdaptive(const srt_adaptive_params& params);
    void setSampleCounts(uint32_t value);
    void readSampleCounts(uint32_t* dst);
    uint64_t renderAdaptiveFrame(uint32_t spp, int rounds, const srt_budget_params& budget, uint32_t max_samples, std::vector<uint32_t>* counts = nullptr);
    // Per-pixel visibility (srt_render_visibility): ambient occlusion and sun visibility at the first hit.  renderVisibility first
    // renders the three guides the pass reads (OBJECT, NORMAL_DEPTH, POSITION) for the band with the current scene and camera —
    // the renderer cannot know whether the ones in the handle are stale, as with the denoiser's — and then enqueues the pass;
    // a params band of [0, 0) (srt_visibility_params_default's) means the renderer's own band.  Asynchronous.  readVisibility
    // waits and copies the W x H floats of ONE output (SRT_VIS_AO or SRT_VIS_SUN, scene rows); visibilityWork waits and returns
    // the work counts of a call that had SRT_VIS_COUNT_WORK.
    void renderVisibility(const srt_visibility_params& params);
    void readVisibility(uint32_t output, float* dst);
    srt_visibility_work visibilityWork();
    // Reflection guides (srt_render_reflection_gbuffer): the first-hit buffers traced through chains of mirror-like surfaces.
    // renderReflectionGBuffer pushes the camera and enqueues the pass; a params band of [0, 0) (srt_reflection_params_default's)
    // means the renderer's own band.  readReflection waits and copies the W x H buffer of ONE output (SRT_REFL_* bit; int32 or
    // float4 per pixel, scene rows); reflectionWork waits and returns the counts of a call that had SRT_REFL_COUNT_WORK.
    // reflectionGuides(true) binds the handle's own four reflection guide buffers into the four G-buffer slots (srt_bind_gbuffer)
    // and from then on RenderGBuffer / RenderGBufferRows render THEM, with reflectionBounces and the library's thresholds:
    // Denoise, denoiseVariance, renderAdaptiveFrame's variance and budget passes — everything that takes its guides from
    // RenderGBuffer — is steered by the reflected geometry, and the guides are re-rendered exactly when the first hits would
    // be.  reflectionGuides(false) binds NULL: the handle's own first-hit buffers again.  The passes that reproject or
    // resample by first hits keep first-hit guides: RenderTemporalFrame, Antialias, renderVisibility and RenderFrame's
    // guidedUpsample switch the binding off around their own guide render and pass and restore it afterwards.
    void reflectionGuides(bool on);
    bool reflectionGuides() const { return reflection_guides_; }
    int reflectionBounces = 8;
    void renderReflectionGBuffer(const srt_reflection_params& params);
    void readReflection(uint32_t output, void* dst);
    srt_reflection_work reflectionWork();
    // Denoiser (srt_denoise) over the whole frame: the accumulator guided by the first-hit buffers as they stand (call
    // RenderGBuffer first).  Asynchronous; ReadDenoised waits and copies the W x H float4 result (scene rows).
    void Denoise(const srt_denoise_params& params);
    void ReadDenoised(float* dst_rgba);
    // Temporal reprojection (srt_temporal_accumulate) over the whole frame with the guides as they stand; ReadHistoryLength
    // waits and copies the W x H history lengths (scene rows).
    void Temporal(const srt_temporal_params& params);
    void ReadHistoryLength(float* dst);
    // Motion vectors (srt_motion_output): with `on` every later Temporal / RenderTemporalFrame also writes W x H float4
    // (u - x, v - y, Wsum, 0); ReadMotion waits and copies them (scene rows).
    void MotionOutput(bool on);
    void ReadMotion(float* dst);
    // Guided upsampler (srt_upsample) over the whole frame: the accumulator's block anchors and the guides as they stand (call
    // RenderGBuffer first).  Asynchronous; ReadUpsampled waits and copies the W x H float4 result (scene rows).
    void Upsample(const srt_upsample_params& params);
    void ReadUpsampled(float* dst_rgba);
    // Anti-aliasing over the whole frame: render the OBJECT guide and the k x k sub-samples (srt_render_subsamples) if the
    // scene, the camera or k has changed since this renderer last rendered them, then srt_antialias with `source`
    // (SRT_AA_SOURCE_*) and `flags` (SRT_AA_*).  Asynchronous; ReadAntialiased waits and copies the W x H float4 result.
    void Antialias(int k, int source = SRT_AA_SOURCE_ACCUMULATOR, uint32_t flags = 0);
    void ReadAntialiased(float* dst_rgba);
    // One frame of a moving camera that keeps its samples (whole frame only): push the camera, render `spp` samples with
    // SRT_RENDER_RESET and seed + k (k = the number of temporal frames this renderer has rendered before, so that the noise
    // does not stay fixed to the screen), the first-hit guides (first hits even while reflectionGuides is on: the reprojection
    // follows the surface seen directly), srt_temporal_accumulate with the library's defaults
    // (samples = spp, max_samples raised to spp if below; SRT_TEMPORAL_RESET on the first temporal frame and after
    // Invalidate(), SetScene, SetEnvironment or SetRowBand), then with `denoise` srt_denoise with its defaults (with
    // temporalVariance: DenoiseTemporalVariance, and the moments are kept whether or not the frame is denoised), then with
    // antialias > 0 Antialias on the denoised buffer (with `denoise`) or the accumulator.  The last step
    // writes the framebuffer.  Later RenderFrame / RenderSamples calls start a fresh accumulation.
    // With mirrorHistory on (below) the frame also renders the four reflection outputs the mode reads (object, normal + path
    // length, point, bounces; reflectionBounces, the library's thresholds; the handle's own buffers) next to the first hits, and
    // the first-hit binding covers the temporal call only: while reflectionGuides is on as well, the frame's denoiser filters with
    // the reflection guides (rendered here, albedo included).  Without mirrorHistory the function does what is said above.
    void RenderTemporalFrame(uint32_t spp, bool denoise);
    // Mirror history (srt_mirror_history): with `on` the temporal pass reprojects pixels that look through mirrors by the virtual
    // image of what they show.  mirrorRadius is the radius of its distance test in pixels, taken when
    // mirrorHistory(bool) is called and again by every RenderTemporalFrame while the mode is on.  Switching drops the history.
    void mirrorHistory(bool on);
    bool mirrorHistory() const { return mirror_history_; }
    float mirrorRadius = 2.0f;
    // Probe tail (srt_probe_tail): with params.enabled the radiance and light-probe traces end a path that reaches the bounce limit
    // on a surface in the probe grid as it stands at the trace.  probeTailWork waits and returns the counts of
    // the last such trace that had SRT_PROBE_TAIL_COUNT_WORK.
    void probeTail(const srt_probe_tail_params& params);
    // What the tail (and the shading calls) read, without shading: each array that is given is written (coefficients probes x 9
    // float4, moments probes x resolution^2 float4, states probes float4); the grid is setProbeGrid's.
    void writeProbeGridInputs(const float* coefficients, const float* moments, const float* states, size_t probes, uint32_t resolution);
    srt_probe_tail_work probeTailWork();
    // Pictures under the probe tail (srt_render_adaptive_tail).  renderAdaptiveTail is renderAdaptive with every
    // path ended in the probe grid under the probeTail setting (which must be on); a band of [0, 0) means the renderer's own.
    // renderProbeTailFrame renders one whole frame that way: the sample counts set to 0, a uniform budget of `spp` (handed over in
    // chunks of at most 4096, the call's cap), renderAdaptiveTail with `bounces` and `seed` per chunk; the frame is left in the
    // accumulator and the framebuffer (ReadFramebuffer).  Whole frame only.  Later RenderFrame / RenderSamples calls start a
    // fresh accumulation.
    void renderAdaptiveTail(const srt_adaptive_params& params);
    void renderProbeTailFrame(uint32_t spp, int bounces, uint32_t seed);
    // Sun sampling in pictures (SRT_ADAPTIVE_SUN_SAMPLING).  Off by default.  The setting is read only by
    // renderAdaptiveFrame and renderProbeTailFrame, which build their parameter structs themselves: with it on, every
    // srt_render_adaptive / srt_render_adaptive_tail they issue — both halves, every round, every chunk — carries the flag
    // (renderAdaptiveFrame's two uniform srt_render halves cannot take it).  renderAdaptive and renderAdaptiveTail pass the
    // caller's flags through as they are.
    void sunSampling(bool on) { sun_sampling_ = on; }
    bool sunSampling() const { return sun_sampling_; }
    // One variance-guided denoised frame (whole frame only): push the camera, render spp / 2 samples with SRT_RENDER_RESET and
    // the frame's seed into the accumulator, spp / 2 with seed ^ 0x9E3779B9 into the handle's half buffer through
    // srt_bind_output (the binding is restored), the four guides, srt_variance with SRT_VARIANCE_MERGE, then
    // srt_denoise_variance with the library's defaults and `flags` (SRT_DENOISE_FRAMEBUFFER) added.  SRT_ERR_INVALID_ARG for an
    // odd spp or one below 2.  ReadDenoised gives the result, ReadVariance the W x H float variance estimate.  Later
    // RenderFrame / RenderSamples calls start a fresh accumulation.
    void denoiseVariance(uint32_t spp, uint32_t flags = 0);
    void ReadVariance(float* dst);
    // The variance-guided filter of a temporal frame rendered with temporalVariance (whole frame, the four guides as they
    // stand): srt_temporal_variance and srt_denoise_variance with the library's defaults and `flags` (SRT_DENOISE_FRAMEBUFFER)
    // added.  RenderTemporalFrame(spp, true) ends in it.  ReadMoments waits and copies the W x H float4 records
    // (M1, M2, Lm, 0) of the last temporal frame (scene rows).
    void DenoiseTemporalVariance(uint32_t flags = 0);
    void ReadMoments(float* dst);

    void PushCamera() { push_camera(); }  // srt_set_camera with the members as they stand (used by MultiGpuRenderer)

   private:
    void check(int rc, const char* what);
    void push_camera();
    srt_camera current_camera() const;
    bool reflection_guides_ = false;
    bool mirror_history_ = false;
    bool sun_sampling_ = false;
    void bind_guides(bool reflection);  // the four G-buffer slots: the own reflection guide buffers, or NULL
    // first hits for the lifetime of the object, whatever reflectionGuides says
    struct FirstHitScope {
        PathTraceRenderer& r;
        const bool was;
        explicit FirstHitScope(PathTraceRenderer& r_) : r(r_), was(r_.reflection_guides_) {
            if (was) r.bind_guides(false), r.reflection_guides_ = false;
        }
        ~FirstHitScope() {
            if (was) rebind(r);
        }
        static void rebind(PathTraceRenderer& r) noexcept;
    };
    // the sub-samples and the OBJECT guide Antialias last rendered: their k (0: none, or the scene has changed since) and camera
    int aa_k_ = 0;
    srt_camera aa_cam_{};
    srt_context* ctx_ = nullptr;
    int width_, height_;
    int row_begin_, row_end_;
    bool doSetFrame_ = false;
    bool scene_set_ = false;        // SetScene has succeeded
    size_t scene_count_ = 0;        // ... with this many objects (UpdateScene takes lists of that length)
    std::vector<std::vector<float>> mesh_vertices_;     // ... and this mesh geometry (UpdateScene takes no other)
    std::vector<std::vector<uint32_t>> mesh_indices_;
    bool SameMeshes(const std::vector<srt_mesh>& meshes) const;
    srt_probe_grid probe_grid_{};       // setProbeGrid's, moved by scrollProbes with SRT_PROBE_SCROLL_SET_GRID
    bool probe_grid_set_ = false;
    uint32_t probe_history_which_ = 0;  // the histories resetProbeHistory has sized
    std::vector<uint32_t> probe_list_;  // listProbes: the list on its way from the list output to the list for tracing
    bool temporal_reset_ = true;    // the next RenderTemporalFrame drops the history
    uint32_t temporal_frames_ = 0;  // RenderTemporalFrame calls so far (the seed offset)
    bool first_frame_ = true;
    bool clean_reset_ = true;  // RenderSamples: next call starts at sample 1 with reset
    uint32_t next_clean_sample_ = 1;
};

// One frame over N GPUs of one node, in ONE process: the reference's split of a frame over 16 worker threads
// (disjoint column stripes of one surface, Raytracer.cpp:330-342) becomes disjoint bands of MEMORY rows, one
// PathTraceRenderer (= one srt_context, one stream) per device.  Pixels share nothing — the random stream is keyed
// by the absolute pixel — so the bands render with no exchange, and ONE gather joins them: every band is copied,
// device to device, into the first device's framebuffer (srt_gather_band: peer copies over xGMI, each peer on its
// own link to the root).  Rank-order concatenation of memory-row bands IS the final image.  The same device may be
// listed several times (N contexts on N streams of one GPU): that is how the class is tested on a one-GPU box.
class MultiGpuRenderer {
   public:
    MultiGpuRenderer(const std::vector<int>& devices, int width, int height);
    ~MultiGpuRenderer();
    MultiGpuRenderer(const MultiGpuRenderer&) = delete;
    MultiGpuRenderer& operator=(const MultiGpuRenderer&) = delete;

    size_t size() const { return parts_.size(); }
    PathTraceRenderer& part(size_t i) { return *parts_[i]; }
    // memory-row band of part i.  Equal bands (the first height % N parts take one more row) until the first
    // RenderSamples; from then on, by default, bands of equal ESTIMATED cost (below).
    void Band(size_t i, int* begin, int* end) const;
    // Bands of equal ESTIMATED cost for the current scene, camera and bounce count (srt_estimate_row_costs on part 0: a
    // device-side probe that runs the kernel's path pool over a quarter of the pixels for the frame's first 32 samples and counts
    // its loop trips — the work of about 8 sample-frames on ONE device, synchronous, deterministic), boundaries on multiples of 2
    // rows (8 and 16 were tried: too coarse for the 48..64-row floor bands of an 8-way 1080p split).  Equal bands
    // leave the GPUs that own sky idle: on Scene1 the slowest of 8 equal bands takes 2.2x the average.
    //
    // Who decides the bands (round 4; the round-3 class re-split before EVERY restarted accumulation, whatever it cost):
    //   * automatic (default): RenderSamples(count) makes the balanced split when the accumulation (re)starts — after SetScene,
    //     Configure, Invalidate: every band starts from sample 1 then anyway — AND the request is worth the probe:
    //     count >= AutoBalanceMinSamples() x devices (default 32 per device: the probe's 8 sample-frames on one device are then
    //     at most a quarter of what the devices are about to do).  A smaller request — a preview frame, a camera move with a few
    //     samples per frame — keeps the bands it has (equal ones at first).  A split made for the same scene, camera, field of
    //     view and bounce count is reused: a new seed or an Invalidate() alone never probes again.
    //   * BalanceBands(): the balanced split now, kept until scene, camera, field of view or bounces change.
    //   * UseEqualBands(true): north_star's literal equal bands, never re-split.
    //   * UseManualBands(true): the bands the caller gave the parts through part(i).SetRowBand() are left alone (the caller
    //     answers for their covering the frame); without it the automatic split REPLACES such bands.
    void BalanceBands();
    void UseEqualBands(bool equal);
    void UseManualBands(bool manual) { manual_bands_ = manual; }
    void SetAutoBalanceMinSamples(uint32_t per_device) { auto_min_samples_ = per_device; }
    uint32_t AutoBalanceMinSamples() const { return auto_min_samples_; }

    void SetScene(const Scene& scene);  // replicated: every device gets its own copy (a few KB; meshes: a few MB)
    void SetEnvironment(const srt_environment& env);
    // camera and settings of every part (the reference's globals; see PathTraceRenderer)
    void Configure(const Transform& camera, int fov, int max_bounces, uint32_t seed);
    void Invalidate();
    // `count` further samples on every band (all launches are enqueued before anything is waited for), then the
    // gather into part 0; after Wait() part 0 holds the whole frame
    void RenderSamples(uint32_t count, bool count_rays = false);
    void Wait();
    void ReadFramebuffer(void* pixels, size_t pitch_bytes);  // the whole frame, from part 0
    // first-hit buffers of the WHOLE frame, made on part 0 (one ray per pixel: a fraction of a sample-frame, no gather)
    void RenderGBuffer(uint32_t outputs);
    void ReadGBuffer(uint32_t output, void* dst) { parts_[0]->ReadGBuffer(output, dst); }
    // per part: kernel time of its last launch and its ray count (imbalance of static bands, SURVEY §8e caveat)
    std::vector<srt_stats> Stats();

   private:
    std::vector<PathTraceRenderer*> parts_;
    std::vector<int> bounds_;  // band i = memory rows [bounds_[i], bounds_[i + 1])
    int width_, height_;
    bool equal_bands_ = false;    // UseEqualBands(true)
    bool manual_bands_ = false;   // UseManualBands(true)
    bool split_pending_ = true;   // the accumulation restarts with the next RenderSamples: the moment rows may change owners
    uint32_t auto_min_samples_ = 32;
    // what the current balanced split was made for (valid while balanced_): a split for the same inputs is reused
    bool balanced_ = false;
    unsigned long long scene_generation_ = 0, split_scene_generation_ = 0;
    Transform split_camera_{};
    int split_fov_ = 0, split_bounces_ = 0;
    bool SplitIsCurrent() const;
    void EqualBands();
};

}  // namespace srt_host
