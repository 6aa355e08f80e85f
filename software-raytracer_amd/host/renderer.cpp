// renderer.cpp — see renderer.hpp.
#include "renderer.hpp"

#include <algorithm>
#include <cstring>
#include <optional>

namespace srt_host {

void PathTraceRenderer::check(int rc, const char* what) {
    if (rc != SRT_OK) {
        const char* msg = srt_last_error(ctx_);
        throw RendererError(rc, std::string(what) + ": " + (msg ? msg : "?"));
    }
}

PathTraceRenderer::PathTraceRenderer(int device, int width, int height)
    : width_(width), height_(height), row_begin_(0), row_end_(height) {
    int rc = srt_create(device, width, height, &ctx_);
    if (rc != SRT_OK) {
        const char* msg = srt_last_error(nullptr);
        throw RendererError(rc, std::string("srt_create: ") + (msg ? msg : "?"));
    }
}

PathTraceRenderer::~PathTraceRenderer() { srt_destroy(ctx_); }

void PathTraceRenderer::SetScene(const Scene& scene) {
    std::vector<srt_object> flat = scene.Flatten();
    std::vector<srt_mesh> meshes = scene.MeshViews();  // EXTENSION: geometry of "Mesh" renderers
    check(srt_set_meshes(ctx_, meshes.data(), meshes.size()), "srt_set_meshes");
    check(srt_update_mode(ctx_, refitUpdates ? SRT_UPDATE_REFIT : SRT_UPDATE_REBUILD), "srt_update_mode");
    scene_set_ = false;
    aa_k_ = 0;
    check(srt_set_scene(ctx_, flat.data(), flat.size()), "srt_set_scene");
    scene_set_ = true;
    scene_count_ = flat.size();
    mesh_vertices_.clear();
    mesh_indices_.clear();
    for (const srt_mesh& m : meshes) {
        mesh_vertices_.emplace_back(m.vertices, m.vertices + 3 * m.vertex_count);
        mesh_indices_.emplace_back(m.indices, m.indices + 3 * m.triangle_count);
    }
    Invalidate();
}

bool PathTraceRenderer::SameMeshes(const std::vector<srt_mesh>& meshes) const {
    if (meshes.size() != mesh_vertices_.size()) return false;
    for (size_t i = 0; i < meshes.size(); ++i) {
        const srt_mesh& m = meshes[i];
        if (3 * m.vertex_count != mesh_vertices_[i].size() || 3 * m.triangle_count != mesh_indices_[i].size()) return false;
        if (!std::equal(mesh_vertices_[i].begin(), mesh_vertices_[i].end(), m.vertices, [](float a, float b) { return std::memcmp(&a, &b, 4) == 0; }))
            return false;
        if (!std::equal(mesh_indices_[i].begin(), mesh_indices_[i].end(), m.indices)) return false;
    }
    return true;
}

void PathTraceRenderer::UpdateScene(const Scene& scene) {
    std::vector<srt_object> flat = scene.Flatten();
    if (!scene_set_ || flat.size() != scene_count_ || !SameMeshes(scene.MeshViews())) {
        SetScene(scene);
        return;
    }
    aa_k_ = 0;
    check(srt_update_mode(ctx_, refitUpdates ? SRT_UPDATE_REFIT : SRT_UPDATE_REBUILD), "srt_update_mode");
    const int rc = srt_update_scene(ctx_, flat.data(), flat.size());
    if (rc != SRT_OK) {
        // a refused list may have left the context without a scene: start afresh (the next edit goes through SetScene)
        scene_set_ = false;
        Invalidate();
    }
    check(rc, "srt_update_scene");
    doSetFrame_ = true;
}

srt_update_info PathTraceRenderer::UpdateInfo() {
    srt_update_info info{};
    check(srt_get_update_info(ctx_, &info), "srt_get_update_info");
    return info;
}

void PathTraceRenderer::SetEnvironment(const srt_environment& env) {
    check(srt_set_environment(ctx_, &env), "srt_set_environment");
    Invalidate();
}

void PathTraceRenderer::SetRowBand(int begin, int end) {
    if (begin < 0 || end > height_ || begin >= end) throw RendererError(SRT_ERR_INVALID_ARG, "SetRowBand: bad band");
    row_begin_ = begin;
    row_end_ = end;
    Invalidate();
}

srt_camera PathTraceRenderer::current_camera() const {
    srt_camera c{};
    const Vec3* src[4] = {&camera.position, &camera.right, &camera.up, &camera.forward};
    float* dst[4] = {c.position, c.right, c.up, c.forward};
    for (int i = 0; i < 4; ++i) {
        dst[i][0] = src[i]->x;
        dst[i][1] = src[i]->y;
        dst[i][2] = src[i]->z;
    }
    c.fov_degrees = FOV;
    return c;
}

void PathTraceRenderer::push_camera() {
    const srt_camera c = current_camera();
    check(srt_set_camera(ctx_, &c), "srt_set_camera");
}

bool PathTraceRenderer::RenderFrame() {
    if (guidedUpsample && (row_begin_ != 0 || row_end_ != height_))
        throw RendererError(SRT_ERR_STATE, "RenderFrame: guidedUpsample with a row band; the upsampler covers the whole frame");
    if (antialias > 0 && (row_begin_ != 0 || row_end_ != height_))
        throw RendererError(SRT_ERR_STATE, "RenderFrame: antialias with a row band; the resolve covers the whole frame");
    if (first_frame_) {
        first_frame_ = false;  // workers start with the initial globals (:30-35,47-48,271)
    } else {
        if (ACCUMULATIONFRAMES == TARGETFRAMES) return false;  // :572-574
        if (doSetFrame_) {                                     // :576-582
            setFrame = true;
            ACCUMULATIONFRAMES = 1;
            progressiveResolutionScaler = 1.0f / 4.0f;
            doSetFrame_ = false;
        } else {                                               // :583-590
            setFrame = false;
            if (progressiveResolutionScaler != 1) setFrame = true;
            progressiveResolutionScaler = 1;
            ACCUMULATIONFRAMES += SIMPLEDRAW ? 0 : 1;
        }
    }
    push_camera();
    srt_render_params p{};
    p.row_begin = row_begin_;
    p.row_end = row_end_;
    p.first_sample = (uint32_t)ACCUMULATIONFRAMES;
    p.sample_count = 1;
    p.max_bounces = MAXBOUNCES < 0 ? 0 : MAXBOUNCES;  // :475
    p.seed = seed;
    p.flags = (setFrame ? SRT_RENDER_RESET : 0u) | (SIMPLEDRAW ? SRT_RENDER_PREVIEW : 0u);
    p.steps = (int)ceil(1 / ((float)SCREEN_SCALE * progressiveResolutionScaler));  // :233
    p.stripe_width = (int)ceil(width_ / (THREADS)) + 1;                             // :330 (integer divide first)
    p.selected_object = selectedObject;
    check(srt_render(ctx_, &p), "srt_render");
    clean_reset_ = true;
    if (guidedUpsample && p.steps > 1) {
        FirstHitScope first_hits(*this);  // the block anchors are samples of the surfaces seen directly
        RenderGBuffer(SRT_GBUF_OBJECT | SRT_GBUF_NORMAL_DEPTH | SRT_GBUF_POSITION);
        srt_upsample_params u{};
        check(srt_upsample_params_default(&u), "srt_upsample_params_default");
        u.steps = p.steps;
        u.stripe_width = p.stripe_width;
        u.flags = SRT_UPSAMPLE_FRAMEBUFFER;  // (not in place: the accumulator stays what the reference accumulates)
        Upsample(u);
    } else if (antialias > 0) {
        Antialias(antialias, SRT_AA_SOURCE_ACCUMULATOR, SRT_AA_FRAMEBUFFER);
    }
    return true;
}

int PathTraceRenderer::Pick(int mouse_x, int mouse_y) {
    push_camera();
    int idx = -1;
    check(srt_pick(ctx_, mouse_x, height_ - mouse_y, &idx), "srt_pick");  // :532 y = SCREEN_HEIGHT - y
    return idx;
}

void PathTraceRenderer::RenderSamples(uint32_t count, bool count_rays, int steps) {
    if (count == 0) return;
    bool reset = doSetFrame_ || clean_reset_;
    if (reset) next_clean_sample_ = 1;
    doSetFrame_ = false;
    clean_reset_ = false;
    push_camera();
    srt_render_params p{};
    p.row_begin = row_begin_;
    p.row_end = row_end_;
    p.first_sample = next_clean_sample_;
    p.sample_count = count;
    p.max_bounces = MAXBOUNCES < 0 ? 0 : MAXBOUNCES;
    p.seed = seed;
    p.flags = (reset ? SRT_RENDER_RESET : 0) | (count_rays ? SRT_RENDER_COUNT_RAYS : 0);
    p.steps = steps;
    p.selected_object = -1;
    check(srt_render(ctx_, &p), "srt_render");
    next_clean_sample_ += count;
    ACCUMULATIONFRAMES = (int)(next_clean_sample_ - 1);
    first_frame_ = false;
    setFrame = false;
    progressiveResolutionScaler = 1;
}

void PathTraceRenderer::Wait() { check(srt_wait(ctx_), "srt_wait"); }

bool PathTraceRenderer::Done() {
    int d = 0;
    check(srt_poll(ctx_, &d), "srt_poll");
    return d != 0;
}

srt_stats PathTraceRenderer::Stats() {
    srt_stats s{};
    check(srt_get_stats(ctx_, &s), "srt_get_stats");
    return s;
}

void PathTraceRenderer::ReadFramebuffer(void* pixels, size_t pitch_bytes) {
    check(srt_read_framebuffer(ctx_, pixels, pitch_bytes, row_begin_, row_end_), "srt_read_framebuffer");
}

void PathTraceRenderer::bind_guides(bool reflection) {
    for (uint32_t bit = SRT_GBUF_OBJECT; bit <= SRT_GBUF_ALBEDO; bit <<= 1) {
        void* p = nullptr;
        if (reflection) check(srt_device_reflection(ctx_, bit, &p), "srt_device_reflection");  // (SRT_REFL_* guide bits are the SRT_GBUF_* bits)
        check(srt_bind_gbuffer(ctx_, bit, p), "srt_bind_gbuffer");
    }
}

void PathTraceRenderer::reflectionGuides(bool on) {
    bind_guides(on);
    reflection_guides_ = on;
}

void PathTraceRenderer::mirrorHistory(bool on) {
    srt_mirror_history_params m{};
    check(srt_mirror_history_params_default(&m), "srt_mirror_history_params_default");
    m.enabled = on ? 1 : 0;
    m.radius_pixels = mirrorRadius;
    check(srt_mirror_history(ctx_, &m), "srt_mirror_history");
    mirror_history_ = on;
}

void PathTraceRenderer::probeTail(const srt_probe_tail_params& params) { check(srt_probe_tail(ctx_, &params), "srt_probe_tail"); }

void PathTraceRenderer::writeProbeGridInputs(const float* coefficients, const float* moments, const float* states, size_t probes, uint32_t resolution) {
    if (coefficients) check(srt_write_probe_grid_coefficients(ctx_, coefficients, probes), "srt_write_probe_grid_coefficients");
    if (moments) check(srt_write_probe_grid_depth(ctx_, moments, probes, resolution), "srt_write_probe_grid_depth");
    if (states) check(srt_write_probe_grid_states(ctx_, states, probes), "srt_write_probe_grid_states");
}

srt_probe_tail_work PathTraceRenderer::probeTailWork() {
    srt_probe_tail_work w{};
    check(srt_get_probe_tail_work(ctx_, &w), "srt_get_probe_tail_work");
    return w;
}

void PathTraceRenderer::FirstHitScope::rebind(PathTraceRenderer& r) noexcept {
    try {
        r.bind_guides(true);
        r.reflection_guides_ = true;
    } catch (...) {  // (a destructor: the binding stays off, as reflectionGuides() then reports)
    }
}

void PathTraceRenderer::renderReflectionGBuffer(const srt_reflection_params& params) {
    srt_reflection_params r = params;
    if (r.row_begin == 0 && r.row_end == 0) r.row_begin = row_begin_, r.row_end = row_end_;
    push_camera();
    check(srt_render_reflection_gbuffer(ctx_, &r), "srt_render_reflection_gbuffer");
}

void PathTraceRenderer::readReflection(uint32_t output, void* dst) { check(srt_read_reflection(ctx_, output, dst), "srt_read_reflection"); }

srt_reflection_work PathTraceRenderer::reflectionWork() {
    srt_reflection_work w{};
    check(srt_get_reflection_work(ctx_, &w), "srt_get_reflection_work");
    return w;
}

void PathTraceRenderer::RenderGBufferRows(uint32_t outputs, int row_begin, int row_end) {
    if (reflection_guides_) {  // the same bits, traced through the mirrors, into the buffers the G-buffer slots are bound to
        srt_reflection_params r{};
        check(srt_reflection_params_default(&r), "srt_reflection_params_default");
        r.row_begin = row_begin, r.row_end = row_end, r.outputs = outputs, r.max_bounces = reflectionBounces;
        renderReflectionGBuffer(r);
        return;
    }
    push_camera();
    srt_gbuffer_params g{};
    g.row_begin = row_begin;
    g.row_end = row_end;
    g.outputs = outputs;
    check(srt_render_gbuffer(ctx_, &g), "srt_render_gbuffer");
}

void PathTraceRenderer::ReadGBuffer(uint32_t output, void* dst) { check(srt_read_gbuffer(ctx_, output, dst), "srt_read_gbuffer"); }

void PathTraceRenderer::traceRays(const float* origins, const float* directions, size_t count, uint32_t outputs, uint32_t flags) {
    check(srt_write_rays(ctx_, origins, directions, count), "srt_write_rays");
    srt_trace_params t{};
    t.outputs = outputs;
    t.flags = flags;
    check(srt_trace_rays(ctx_, &t), "srt_trace_rays");
}

void PathTraceRenderer::traceOcclusion(const float* origins, const float* directions, size_t count, uint32_t flags) {
    check(srt_write_rays(ctx_, origins, directions, count), "srt_write_rays");
    srt_occlusion_params t{};
    t.flags = flags;
    check(srt_trace_occlusion(ctx_, &t), "srt_trace_occlusion");
}

srt_occlusion_work PathTraceRenderer::occlusionWork() {
    srt_occlusion_work w{};
    check(srt_get_occlusion_work(ctx_, &w), "srt_get_occlusion_work");
    return w;
}

void PathTraceRenderer::traceRadiance(const float* origins, const float* directions, size_t count, const srt_radiance_params& params) {
    check(srt_write_rays(ctx_, origins, directions, count), "srt_write_rays");
    check(srt_trace_radiance(ctx_, &params), "srt_trace_radiance");
}

void PathTraceRenderer::readRadiance(float* dst_rgba) { check(srt_read_radiance(ctx_, dst_rgba), "srt_read_radiance"); }

srt_radiance_work PathTraceRenderer::radianceWork() {
    srt_radiance_work w{};
    check(srt_get_radiance_work(ctx_, &w), "srt_get_radiance_work");
    return w;
}

void PathTraceRenderer::traceLightProbes(const float* positions, size_t probes, const float* directions, size_t direction_count,
                                         const srt_light_probe_params& params) {
    check(srt_write_light_probes(ctx_, positions, probes), "srt_write_light_probes");
    check(srt_write_light_probe_directions(ctx_, directions, direction_count), "srt_write_light_probe_directions");
    check(srt_trace_light_probes(ctx_, &params), "srt_trace_light_probes");
}

void PathTraceRenderer::readLightProbeOutput(uint32_t output, float* dst) {
    check(srt_read_light_probe_output(ctx_, output, dst), "srt_read_light_probe_output");
}

srt_light_probe_work PathTraceRenderer::lightProbeWork() {
    srt_light_probe_work w{};
    check(srt_get_light_probe_work(ctx_, &w), "srt_get_light_probe_work");
    return w;
}

void PathTraceRenderer::setProbeGrid(const srt_probe_grid& grid) {
    check(srt_set_probe_grid(ctx_, &grid), "srt_set_probe_grid");
    probe_grid_ = grid, probe_grid_set_ = true;
}

void PathTraceRenderer::shadeProbeGrid(const float* coefficients, size_t probes, const srt_probe_grid_params& params) {
    srt_probe_grid_params s = params;
    if (s.row_begin == 0 && s.row_end == 0) s.row_begin = row_begin_, s.row_end = row_end_;
    if (coefficients) check(srt_write_probe_grid_coefficients(ctx_, coefficients, probes), "srt_write_probe_grid_coefficients");
    FirstHitScope first_hits(*this);  // irradiance AT the first hit
    RenderGBufferRows(SRT_GBUF_OBJECT | SRT_GBUF_NORMAL_DEPTH | SRT_GBUF_POSITION | ((s.flags & SRT_PROBE_GRID_ALBEDO) ? SRT_GBUF_ALBEDO : 0u), s.row_begin,
                      s.row_end);  // (pushes the camera)
    check(srt_shade_probe_grid(ctx_, &s), "srt_shade_probe_grid");
}

void PathTraceRenderer::readProbeGridOutput(float* dst_rgba) { check(srt_read_probe_grid_output(ctx_, dst_rgba), "srt_read_probe_grid_output"); }

srt_probe_grid_work PathTraceRenderer::probeGridWork() {
    srt_probe_grid_work w{};
    check(srt_get_probe_grid_work(ctx_, &w), "srt_get_probe_grid_work");
    return w;
}

void PathTraceRenderer::traceProbeDepth(const float* positions, size_t probes, const float* directions, size_t direction_count,
                                        const srt_probe_depth_params& params) {
    check(srt_write_light_probes(ctx_, positions, probes), "srt_write_light_probes");
    check(srt_write_light_probe_directions(ctx_, directions, direction_count), "srt_write_light_probe_directions");
    check(srt_trace_probe_depth(ctx_, &params), "srt_trace_probe_depth");
}

void PathTraceRenderer::readProbeDepthOutput(uint32_t output, void* dst) {
    check(srt_read_probe_depth_output(ctx_, output, dst), "srt_read_probe_depth_output");
}

srt_probe_depth_work PathTraceRenderer::probeDepthWork() {
    srt_probe_depth_work w{};
    check(srt_get_probe_depth_work(ctx_, &w), "srt_get_probe_depth_work");
    return w;
}

void PathTraceRenderer::shadeProbeGridDepth(const float* coefficients, const float* moments, size_t probes, uint32_t resolution,
                                            const srt_probe_grid_params& params, const srt_probe_grid_depth_params& depth) {
    srt_probe_grid_params s = params;
    if (s.row_begin == 0 && s.row_end == 0) s.row_begin = row_begin_, s.row_end = row_end_;
    if (coefficients) check(srt_write_probe_grid_coefficients(ctx_, coefficients, probes), "srt_write_probe_grid_coefficients");
    if (moments) check(srt_write_probe_grid_depth(ctx_, moments, probes, resolution), "srt_write_probe_grid_depth");
    FirstHitScope first_hits(*this);  // irradiance AT the first hit
    RenderGBufferRows(SRT_GBUF_OBJECT | SRT_GBUF_NORMAL_DEPTH | SRT_GBUF_POSITION | ((s.flags & SRT_PROBE_GRID_ALBEDO) ? SRT_GBUF_ALBEDO : 0u), s.row_begin,
                      s.row_end);  // (pushes the camera)
    check(srt_shade_probe_grid_depth(ctx_, &s, &depth), "srt_shade_probe_grid_depth");
}

void PathTraceRenderer::classifyProbes(const float* directions, size_t direction_count, const srt_probe_classify_params& params) {
    if (directions) check(srt_write_light_probe_directions(ctx_, directions, direction_count), "srt_write_light_probe_directions");
    check(srt_classify_probes(ctx_, &params), "srt_classify_probes");
}

void PathTraceRenderer::readProbeStatesOutput(uint32_t output, void* dst) {
    check(srt_read_probe_states_output(ctx_, output, dst), "srt_read_probe_states_output");
}

srt_probe_classify_work PathTraceRenderer::probeClassifyWork() {
    srt_probe_classify_work w{};
    check(srt_get_probe_classify_work(ctx_, &w), "srt_get_probe_classify_work");
    return w;
}

void PathTraceRenderer::shadeProbeGridStates(const float* coefficients, const float* moments, const float* states, size_t probes, uint32_t resolution,
                                             const srt_probe_grid_params& params, const srt_probe_grid_depth_params* depth) {
    srt_probe_grid_params s = params;
    if (s.row_begin == 0 && s.row_end == 0) s.row_begin = row_begin_, s.row_end = row_end_;
    if (coefficients) check(srt_write_probe_grid_coefficients(ctx_, coefficients, probes), "srt_write_probe_grid_coefficients");
    if (moments) check(srt_write_probe_grid_depth(ctx_, moments, probes, resolution), "srt_write_probe_grid_depth");
    if (states) check(srt_write_probe_grid_states(ctx_, states, probes), "srt_write_probe_grid_states");
    FirstHitScope first_hits(*this);  // irradiance AT the first hit
    RenderGBufferRows(SRT_GBUF_OBJECT | SRT_GBUF_NORMAL_DEPTH | SRT_GBUF_POSITION | ((s.flags & SRT_PROBE_GRID_ALBEDO) ? SRT_GBUF_ALBEDO : 0u), s.row_begin,
                      s.row_end);  // (pushes the camera)
    check(srt_shade_probe_grid_states(ctx_, &s, depth), "srt_shade_probe_grid_states");
}

void PathTraceRenderer::listProbes(const float* states, size_t probes, const srt_probe_list_params& params) {
    if (states) check(srt_write_probe_grid_states(ctx_, states, probes), "srt_write_probe_grid_states");
    check(srt_list_probes(ctx_, &params), "srt_list_probes");
    probe_list_.resize(SRT_PROBE_LIST_HEADER + probes);
    check(srt_read_probe_list_output(ctx_, probe_list_.data()), "srt_read_probe_list_output");
    check(srt_write_probe_list(ctx_, probe_list_.data(), probe_list_.size()), "srt_write_probe_list");
}

void PathTraceRenderer::readProbeListOutput(uint32_t* dst) { check(srt_read_probe_list_output(ctx_, dst), "srt_read_probe_list_output"); }

srt_probe_list_work PathTraceRenderer::probeListWork() {
    srt_probe_list_work w{};
    check(srt_get_probe_list_work(ctx_, &w), "srt_get_probe_list_work");
    return w;
}

void PathTraceRenderer::traceLightProbesListed(const float* positions, size_t probes, const float* directions, size_t direction_count,
                                               const srt_light_probe_params& params) {
    if (positions) check(srt_write_light_probes(ctx_, positions, probes), "srt_write_light_probes");
    if (directions) check(srt_write_light_probe_directions(ctx_, directions, direction_count), "srt_write_light_probe_directions");
    check(srt_trace_light_probes_listed(ctx_, &params), "srt_trace_light_probes_listed");
}

void PathTraceRenderer::traceProbeDepthListed(const float* positions, size_t probes, const float* directions, size_t direction_count,
                                              const srt_probe_depth_params& params) {
    if (positions) check(srt_write_light_probes(ctx_, positions, probes), "srt_write_light_probes");
    if (directions) check(srt_write_light_probe_directions(ctx_, directions, direction_count), "srt_write_light_probe_directions");
    check(srt_trace_probe_depth_listed(ctx_, &params), "srt_trace_probe_depth_listed");
}

void PathTraceRenderer::resetProbeHistory(uint32_t which, size_t probes, uint32_t resolution) {
    check(srt_reset_probe_history(ctx_, which, probes, resolution), "srt_reset_probe_history");
    probe_history_which_ |= which;
}

void PathTraceRenderer::blendProbes(const float* previous_states, size_t probes, const srt_probe_blend_params& params) {
    if (previous_states) check(srt_write_probe_previous_states(ctx_, previous_states, probes), "srt_write_probe_previous_states");
    check(srt_blend_probes(ctx_, &params), "srt_blend_probes");
}

void PathTraceRenderer::readProbeHistory(uint32_t which, float* dst) { check(srt_read_probe_history(ctx_, which, dst), "srt_read_probe_history"); }

srt_probe_blend_work PathTraceRenderer::probeBlendWork() {
    srt_probe_blend_work w{};
    check(srt_get_probe_blend_work(ctx_, &w), "srt_get_probe_blend_work");
    return w;
}

void PathTraceRenderer::scrollProbes(const int32_t shift[3], uint32_t which, uint32_t flags) {
    srt_probe_scroll_params p{};
    check(srt_probe_scroll_params_default(&p), "srt_probe_scroll_params_default");
    for (int a = 0; a < 3; ++a) p.shift[a] = shift[a];
    p.which = which, p.flags = flags;
    check(srt_scroll_probes(ctx_, &p), "srt_scroll_probes");
    if ((flags & SRT_PROBE_SCROLL_SET_GRID) && probe_grid_set_)
        for (int a = 0; a < 3; ++a) {  // rule SC4, as the handle moved its own copy
            volatile float step = (float)shift[a] * probe_grid_.spacing[a];
            probe_grid_.origin[a] = probe_grid_.origin[a] + step;
        }
}

std::array<int32_t, 3> PathTraceRenderer::followProbeGrid(const float point[3]) {
    if (!probe_grid_set_) throw RendererError(SRT_ERR_STATE, "followProbeGrid: no grid (setProbeGrid)");
    std::array<int32_t, 3> shift{};
    check(srt_probe_grid_follow(&probe_grid_, point, shift.data()), "srt_probe_grid_follow");
    scrollProbes(shift.data(), probe_history_which_ | SRT_PROBE_SCROLL_STATES, SRT_PROBE_SCROLL_SET_GRID);
    return shift;
}

srt_probe_scroll_work PathTraceRenderer::probeScrollWork() {
    srt_probe_scroll_work w{};
    check(srt_get_probe_scroll_work(ctx_, &w), "srt_get_probe_scroll_work");
    return w;
}

void PathTraceRenderer::setProbeCascade(const srt_probe_cascade& cascade) { check(srt_set_probe_cascade(ctx_, &cascade), "srt_set_probe_cascade"); }

void PathTraceRenderer::captureProbeCascadeLevel(uint32_t level, uint32_t which) {
    check(srt_capture_probe_cascade_level(ctx_, level, which), "srt_capture_probe_cascade_level");
}

void PathTraceRenderer::shadeProbeCascade(const srt_probe_cascade_params& params) {
    srt_probe_cascade_params s = params;
    if (s.row_begin == 0 && s.row_end == 0) s.row_begin = row_begin_, s.row_end = row_end_;
    FirstHitScope first_hits(*this);  // irradiance AT the first hit
    RenderGBufferRows(SRT_GBUF_OBJECT | SRT_GBUF_NORMAL_DEPTH | SRT_GBUF_POSITION | ((s.flags & SRT_PROBE_CASCADE_ALBEDO) ? SRT_GBUF_ALBEDO : 0u), s.row_begin,
                      s.row_end);  // (pushes the camera)
    check(srt_shade_probe_cascade(ctx_, &s), "srt_shade_probe_cascade");
}

srt_probe_cascade_work PathTraceRenderer::probeCascadeWork() {
    srt_probe_cascade_work w{};
    check(srt_get_probe_cascade_work(ctx_, &w), "srt_get_probe_cascade_work");
    return w;
}

uint64_t PathTraceRenderer::sampleBudget(const srt_budget_params& params) {
    check(srt_sample_budget(ctx_, &params), "srt_sample_budget");
    uint64_t total = 0;
    check(srt_get_budget_total(ctx_, &total), "srt_get_budget_total");
    return total;
}

void PathTraceRenderer::renderAdaptive(const srt_adaptive_params& params) {
    srt_adaptive_params a = params;
    if (a.row_begin == 0 && a.row_end == 0) a.row_begin = row_begin_, a.row_end = row_end_;
    push_camera();
    check(srt_render_adaptive(ctx_, &a), "srt_render_adaptive");
}

void PathTraceRenderer::renderAdaptiveTail(const srt_adaptive_params& params) {
    srt_adaptive_params a = params;
    if (a.row_begin == 0 && a.row_end == 0) a.row_begin = row_begin_, a.row_end = row_end_;
    push_camera();
    check(srt_render_adaptive_tail(ctx_, &a), "srt_render_adaptive_tail");
}

void PathTraceRenderer::renderProbeTailFrame(uint32_t spp, int bounces, uint32_t seed) {
    if (spp < 1) throw RendererError(SRT_ERR_INVALID_ARG, "renderProbeTailFrame: spp must be >= 1");
    if (row_begin_ != 0 || row_end_ != height_)
        throw RendererError(SRT_ERR_STATE, "renderProbeTailFrame: the renderer has a row band; the frame covers the whole image");
    setSampleCounts(0);
    srt_adaptive_params a{};
    check(srt_adaptive_params_default(&a), "srt_adaptive_params_default");
    a.row_begin = 0, a.row_end = height_, a.max_bounces = bounces, a.seed = seed;
    if (sun_sampling_) a.flags |= SRT_ADAPTIVE_SUN_SAMPLING;
    std::vector<uint32_t> budget((size_t)width_ * height_);
    for (uint32_t done = 0; done < spp;) {  // (the counts carry the frame from chunk to chunk)
        const uint32_t chunk = spp - done < a.max_samples ? spp - done : a.max_samples;
        if (done == 0 || chunk != budget[0]) {
            std::fill(budget.begin(), budget.end(), chunk);
            check(srt_write_sample_budget(ctx_, budget.data()), "srt_write_sample_budget");
        }
        renderAdaptiveTail(a);
        done += chunk;
    }
    // the accumulator holds a tail frame, which no srt_render can continue
    doSetFrame_ = true;
    clean_reset_ = true;
    first_frame_ = false;
}

void PathTraceRenderer::setSampleCounts(uint32_t value) { check(srt_set_sample_counts(ctx_, value), "srt_set_sample_counts"); }

void PathTraceRenderer::readSampleCounts(uint32_t* dst) { check(srt_read_sample_counts(ctx_, dst), "srt_read_sample_counts"); }

uint64_t PathTraceRenderer::renderAdaptiveFrame(uint32_t spp, int rounds, const srt_budget_params& budget, uint32_t max_samples, std::vector<uint32_t>* counts) {
    if (spp < 2 || (spp & 1u))
        throw RendererError(SRT_ERR_INVALID_ARG, "renderAdaptiveFrame: spp must be even and >= 2 (two half renders of spp / 2 samples each)");
    if (rounds < 0) throw RendererError(SRT_ERR_INVALID_ARG, "renderAdaptiveFrame: rounds must be >= 0");
    if (row_begin_ != 0 || row_end_ != height_)
        throw RendererError(SRT_ERR_STATE, "renderAdaptiveFrame: the renderer has a row band; the variance passes cover the whole frame");
    push_camera();
    srt_render_params p{};
    p.row_begin = 0;
    p.row_end = height_;
    p.first_sample = 1;
    p.sample_count = spp / 2;
    p.max_bounces = MAXBOUNCES < 0 ? 0 : MAXBOUNCES;
    p.seed = seed;
    p.flags = SRT_RENDER_RESET;
    p.steps = 1;
    p.selected_object = -1;
    const uint32_t seed_b = seed ^ 0x9E3779B9u;
    check(srt_render(ctx_, &p), "srt_render");  // half A, into the accumulator
    void *fb = nullptr, *acc = nullptr, *half = nullptr;
    check(srt_device_framebuffer(ctx_, &fb), "srt_device_framebuffer");
    check(srt_device_accumulator(ctx_, &acc), "srt_device_accumulator");
    check(srt_device_half(ctx_, &half), "srt_device_half");
    check(srt_bind_output(ctx_, fb, half), "srt_bind_output");
    p.seed = seed_b;
    int rc = srt_render(ctx_, &p);  // half B, into the half buffer; then the binding as it was
    check(srt_bind_output(ctx_, fb, acc), "srt_bind_output");
    check(rc, "srt_render");
    setSampleCounts(spp / 2);
    const bool demod = (budget.flags & SRT_BUDGET_ALBEDO) != 0;
    RenderGBuffer(SRT_GBUF_OBJECT | (demod ? SRT_GBUF_ALBEDO : 0u));
    srt_variance_params v{};
    v.flags = demod ? SRT_VARIANCE_ALBEDO : 0u;
    srt_adaptive_params a{};
    check(srt_adaptive_params_default(&a), "srt_adaptive_params_default");
    a.row_begin = 0, a.row_end = height_, a.max_bounces = p.max_bounces, a.max_samples = max_samples;
    const uint32_t sun = sun_sampling_ ? SRT_ADAPTIVE_SUN_SAMPLING : 0u;  // (mixing with the uniform halves is rule AS3)
    for (int k = 0; k < rounds; ++k) {
        check(srt_variance(ctx_, &v), "srt_variance");
        (void)sampleBudget(budget);
        a.seed = seed, a.flags = SRT_ADAPTIVE_KEEP_COUNTS | sun;
        check(srt_render_adaptive(ctx_, &a), "srt_render_adaptive");  // half A: the counts stay for half B
        check(srt_bind_output(ctx_, fb, half), "srt_bind_output");
        a.seed = seed_b, a.flags = sun;
        rc = srt_render_adaptive(ctx_, &a);
        check(srt_bind_output(ctx_, fb, acc), "srt_bind_output");
        check(rc, "srt_render_adaptive");
    }
    v.flags |= SRT_VARIANCE_MERGE;
    check(srt_variance(ctx_, &v), "srt_variance");
    std::vector<uint32_t> n((size_t)width_ * height_);
    readSampleCounts(n.data());
    uint64_t total = 0;
    for (uint32_t& c : n) c *= 2u, total += c;
    if (counts) counts->swap(n);
    // the accumulator now holds the mean of the halves, which no render can continue
    doSetFrame_ = true;
    clean_reset_ = true;
    first_frame_ = false;
    return total;
}

void PathTraceRenderer::renderVisibility(const srt_visibility_params& params) {
    srt_visibility_params v = params;
    if (v.row_begin == 0 && v.row_end == 0) v.row_begin = row_begin_, v.row_end = row_end_;
    FirstHitScope first_hits(*this);  // visibility AT the first hit
    RenderGBufferRows(SRT_GBUF_OBJECT | SRT_GBUF_NORMAL_DEPTH | SRT_GBUF_POSITION, v.row_begin, v.row_end);  // (pushes the camera)
    check(srt_render_visibility(ctx_, &v), "srt_render_visibility");
}

void PathTraceRenderer::readVisibility(uint32_t output, float* dst) { check(srt_read_visibility(ctx_, output, dst), "srt_read_visibility"); }

srt_visibility_work PathTraceRenderer::visibilityWork() {
    srt_visibility_work w{};
    check(srt_get_visibility_work(ctx_, &w), "srt_get_visibility_work");
    return w;
}

void PathTraceRenderer::readRayOutput(uint32_t output, void* dst) { check(srt_read_ray_output(ctx_, output, dst), "srt_read_ray_output"); }

void PathTraceRenderer::Denoise(const srt_denoise_params& params) { check(srt_denoise(ctx_, &params), "srt_denoise"); }

void PathTraceRenderer::ReadDenoised(float* dst_rgba) { check(srt_read_denoised(ctx_, dst_rgba), "srt_read_denoised"); }

void PathTraceRenderer::Temporal(const srt_temporal_params& params) { check(srt_temporal_accumulate(ctx_, &params), "srt_temporal_accumulate"); }

void PathTraceRenderer::ReadHistoryLength(float* dst) { check(srt_read_history_length(ctx_, dst), "srt_read_history_length"); }

void PathTraceRenderer::MotionOutput(bool on) { check(srt_motion_output(ctx_, on ? 1 : 0), "srt_motion_output"); }

void PathTraceRenderer::ReadMotion(float* dst) { check(srt_read_motion(ctx_, dst), "srt_read_motion"); }

void PathTraceRenderer::Upsample(const srt_upsample_params& params) { check(srt_upsample(ctx_, &params), "srt_upsample"); }

void PathTraceRenderer::ReadUpsampled(float* dst_rgba) { check(srt_read_upsampled(ctx_, dst_rgba), "srt_read_upsampled"); }

void PathTraceRenderer::Antialias(int k, int source, uint32_t flags) {
    if (row_begin_ != 0 || row_end_ != height_)
        throw RendererError(SRT_ERR_STATE, "Antialias: the renderer has a row band; the resolve covers the whole frame");
    const srt_camera c = current_camera();
    FirstHitScope first_hits(*this);  // the sub-samples are first hits, and so is the pixel guide they are compared with
    if (aa_k_ != k || std::memcmp(&aa_cam_, &c, sizeof c) != 0) {
        aa_k_ = 0;
        RenderGBufferRows(SRT_GBUF_OBJECT, 0, height_);  // (pushes the camera)
        srt_subsample_params s{};
        s.row_begin = 0, s.row_end = height_, s.k = k;
        check(srt_render_subsamples(ctx_, &s), "srt_render_subsamples");
        aa_k_ = k, aa_cam_ = c;
    }
    srt_antialias_params a{};
    a.k = k, a.source = source, a.flags = flags;
    check(srt_antialias(ctx_, &a), "srt_antialias");
}

void PathTraceRenderer::ReadAntialiased(float* dst_rgba) { check(srt_read_antialiased(ctx_, dst_rgba), "srt_read_antialiased"); }

void PathTraceRenderer::RenderTemporalFrame(uint32_t spp, bool denoise) {
    if (spp == 0) throw RendererError(SRT_ERR_INVALID_ARG, "RenderTemporalFrame: spp must be >= 1");
    if (row_begin_ != 0 || row_end_ != height_)
        throw RendererError(SRT_ERR_STATE, "RenderTemporalFrame: the renderer has a row band; temporal frames cover the whole frame");
    // the temporal pass keeps first-hit guides in the G-buffer slots, also while reflectionGuides is on: it reprojects the surface
    // seen directly.  Without mirrorHistory the image in a mirror is carried along with the mirror and the
    // frame's denoiser filters with the first hits too; with it the pass reads the reflection outputs next to the first hits
    // (§4.26) and the scope ends behind the temporal call, so that the denoiser filters with whatever reflectionGuides says.
    const bool denoise_by_reflection = mirror_history_ && reflection_guides_;
    std::optional<FirstHitScope> first_hits;
    first_hits.emplace(*this);
    push_camera();
    srt_render_params p{};
    p.row_begin = 0;
    p.row_end = height_;
    p.first_sample = 1;
    p.sample_count = spp;
    p.max_bounces = MAXBOUNCES < 0 ? 0 : MAXBOUNCES;
    p.seed = seed + temporal_frames_;
    p.flags = SRT_RENDER_RESET;
    p.steps = 1;
    p.selected_object = -1;
    check(srt_render(ctx_, &p), "srt_render");
    RenderGBuffer(SRT_GBUF_OBJECT | SRT_GBUF_NORMAL_DEPTH | SRT_GBUF_POSITION | (denoise || temporalVariance ? SRT_GBUF_ALBEDO : 0u));
    if (mirror_history_) {
        mirrorHistory(true);  // (mirrorRadius as it stands now; a change of the radius alone keeps the history)
        srt_reflection_params r{};
        check(srt_reflection_params_default(&r), "srt_reflection_params_default");
        r.row_begin = 0, r.row_end = height_, r.max_bounces = reflectionBounces;
        r.outputs = SRT_REFL_OBJECT | SRT_REFL_NORMAL_DEPTH | SRT_REFL_POSITION | SRT_REFL_BOUNCES | (denoise_by_reflection && denoise ? SRT_REFL_ALBEDO : 0u);
        renderReflectionGBuffer(r);
    }
    // the moments of the demodulated luminance: what srt_denoise_variance's defaults filter
    check(srt_moments_output(ctx_, temporalVariance ? 1 : 0, temporalVariance ? SRT_VARIANCE_ALBEDO : 0u), "srt_moments_output");
    srt_temporal_params t{};
    check(srt_temporal_params_default(&t), "srt_temporal_params_default");
    t.samples = spp;
    if (t.max_samples < (float)spp) t.max_samples = (float)spp;
    t.flags = (temporal_reset_ ? SRT_TEMPORAL_RESET : 0u) | (denoise ? 0u : SRT_TEMPORAL_FRAMEBUFFER);
    Temporal(t);
    if (mirror_history_) first_hits.reset();
    if (denoise && temporalVariance) {
        DenoiseTemporalVariance(SRT_DENOISE_FRAMEBUFFER);
    } else if (denoise) {
        srt_denoise_params d{};
        check(srt_denoise_params_default(&d), "srt_denoise_params_default");
        d.flags |= SRT_DENOISE_FRAMEBUFFER;
        Denoise(d);
    }
    if (antialias > 0) Antialias(antialias, denoise ? SRT_AA_SOURCE_DENOISED : SRT_AA_SOURCE_ACCUMULATOR, SRT_AA_FRAMEBUFFER);
    temporal_reset_ = false;
    ++temporal_frames_;
    // the accumulator now holds a blended estimate no render can continue
    doSetFrame_ = true;
    clean_reset_ = true;
    first_frame_ = false;
}

void PathTraceRenderer::denoiseVariance(uint32_t spp, uint32_t flags) {
    if (spp < 2 || (spp & 1u))
        throw RendererError(SRT_ERR_INVALID_ARG, "denoiseVariance: spp must be even and >= 2 (two half renders of spp / 2 samples each)");
    if (row_begin_ != 0 || row_end_ != height_)
        throw RendererError(SRT_ERR_STATE, "denoiseVariance: the renderer has a row band; the variance passes cover the whole frame");
    push_camera();
    srt_render_params p{};
    p.row_begin = 0;
    p.row_end = height_;
    p.first_sample = 1;
    p.sample_count = spp / 2;
    p.max_bounces = MAXBOUNCES < 0 ? 0 : MAXBOUNCES;
    p.seed = seed;
    p.flags = SRT_RENDER_RESET;
    p.steps = 1;
    p.selected_object = -1;
    check(srt_render(ctx_, &p), "srt_render");  // half A, into the accumulator
    // half B: the same frame with another seed, accumulated into the half buffer; then the binding as it was
    void *fb = nullptr, *acc = nullptr, *half = nullptr;
    check(srt_device_framebuffer(ctx_, &fb), "srt_device_framebuffer");
    check(srt_device_accumulator(ctx_, &acc), "srt_device_accumulator");
    check(srt_device_half(ctx_, &half), "srt_device_half");
    check(srt_bind_output(ctx_, fb, half), "srt_bind_output");
    p.seed = seed ^ 0x9E3779B9u;
    const int rc = srt_render(ctx_, &p);
    check(srt_bind_output(ctx_, fb, acc), "srt_bind_output");
    check(rc, "srt_render");
    RenderGBuffer(SRT_GBUF_ALL);
    srt_variance_params v{};
    check(srt_variance_params_default(&v), "srt_variance_params_default");
    v.flags |= SRT_VARIANCE_MERGE;
    srt_denoise_variance_params d{};
    check(srt_denoise_variance_params_default(&d), "srt_denoise_variance_params_default");
    d.flags |= flags;
    // the estimate and the filter agree on demodulation
    v.flags = (d.flags & SRT_DENOISE_ALBEDO) ? (v.flags | SRT_VARIANCE_ALBEDO) : (v.flags & ~SRT_VARIANCE_ALBEDO);
    check(srt_variance(ctx_, &v), "srt_variance");
    check(srt_denoise_variance(ctx_, &d), "srt_denoise_variance");
    // the accumulator now holds the mean of the halves, which no render can continue
    doSetFrame_ = true;
    clean_reset_ = true;
    first_frame_ = false;
}

void PathTraceRenderer::ReadVariance(float* dst) { check(srt_read_variance(ctx_, dst), "srt_read_variance"); }

void PathTraceRenderer::DenoiseTemporalVariance(uint32_t flags) {
    srt_temporal_variance_params v{};
    check(srt_temporal_variance_params_default(&v), "srt_temporal_variance_params_default");
    srt_denoise_variance_params d{};
    check(srt_denoise_variance_params_default(&d), "srt_denoise_variance_params_default");
    d.flags |= flags;
    check(srt_temporal_variance(ctx_, &v), "srt_temporal_variance");
    check(srt_denoise_variance(ctx_, &d), "srt_denoise_variance");
}

void PathTraceRenderer::ReadMoments(float* dst) { check(srt_read_moments(ctx_, dst), "srt_read_moments"); }

std::vector<float> PathTraceRenderer::ReadAccumulator() {
    std::vector<float> out((size_t)width_ * height_ * 4);
    check(srt_read_accumulator(ctx_, out.data()), "srt_read_accumulator");
    return out;
}

// ---- MultiGpuRenderer -------------------------------------------------------------------
MultiGpuRenderer::MultiGpuRenderer(const std::vector<int>& devices, int width, int height) : width_(width), height_(height) {
    if (devices.empty() || (int)devices.size() > height) throw RendererError(SRT_ERR_INVALID_ARG, "MultiGpuRenderer: need 1 <= devices <= height");
    bounds_.assign(devices.size() + 1, 0);
    try {
        for (int d : devices) parts_.push_back(new PathTraceRenderer(d, width, height));
        EqualBands();
        split_pending_ = true;  // (the first RenderSamples makes the default split)
    } catch (...) {
        for (PathTraceRenderer* p : parts_) delete p;
        throw;
    }
}

MultiGpuRenderer::~MultiGpuRenderer() {
    for (PathTraceRenderer* p : parts_) delete p;
}

void MultiGpuRenderer::Band(size_t i, int* begin, int* end) const {
    if (manual_bands_) {  // the caller's own bands (part(i).SetRowBand)
        parts_[i]->RowBand(begin, end);
        return;
    }
    *begin = bounds_[i];
    *end = bounds_[i + 1];
}

void MultiGpuRenderer::EqualBands() {
    const int n = (int)parts_.size(), q = height_ / n, r = height_ % n;
    for (int k = 0; k <= n; ++k) bounds_[(size_t)k] = k * q + (k < r ? k : r);
    for (int k = 0; k < n; ++k) parts_[(size_t)k]->SetRowBand(bounds_[(size_t)k], bounds_[(size_t)k + 1]);
    split_pending_ = false;
    balanced_ = false;
}

static bool same_vec(const Vec3& a, const Vec3& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// the balanced split in force was made for this scene, camera, field of view and bounce count (the probe's inputs that matter;
// its seed moves the estimate by noise only)
bool MultiGpuRenderer::SplitIsCurrent() const {
    if (!balanced_ || parts_.empty()) return false;
    const PathTraceRenderer& p0 = *parts_[0];
    return split_scene_generation_ == scene_generation_ && split_fov_ == p0.FOV && split_bounces_ == p0.MAXBOUNCES &&
           same_vec(split_camera_.position, p0.camera.position) && same_vec(split_camera_.right, p0.camera.right) &&
           same_vec(split_camera_.up, p0.camera.up) && same_vec(split_camera_.forward, p0.camera.forward);
}

void MultiGpuRenderer::UseEqualBands(bool equal) {
    equal_bands_ = equal;
    Invalidate();  // rows change owners: every band starts over
}

void MultiGpuRenderer::BalanceBands() {
    const int n = (int)parts_.size();
    if (n < 2) return;
    std::vector<float> cost((size_t)height_);
    PathTraceRenderer& p0 = *parts_[0];
    p0.Wait();
    p0.PushCamera();
    int rc = srt_estimate_row_costs(p0.handle(), p0.MAXBOUNCES < 0 ? 0 : p0.MAXBOUNCES, p0.seed, cost.data());
    if (rc != SRT_OK) {
        const char* msg = srt_last_error(p0.handle());
        throw RendererError(rc, std::string("srt_estimate_row_costs: ") + (msg ? msg : "?"));
    }
    std::vector<double> prefix((size_t)height_ + 1, 0.0);
    for (int i = 0; i < height_; ++i) prefix[(size_t)i + 1] = prefix[(size_t)i] + (cost[(size_t)i] > 0 ? cost[(size_t)i] : 0.0);
    const double total = prefix[(size_t)height_];
    bounds_[0] = 0;
    for (int k = 1; k < n; ++k) {  // first row whose prefix cost reaches k/n of the total, rounded to 2 rows, every band >= 1 row
        const int lo = bounds_[(size_t)k - 1] + 1, hi = height_ - (n - k);
        int i = lo;
        while (i < hi && prefix[(size_t)i] < total * k / n) ++i;
        const int j = ((i + 1) / 2) * 2;
        if (j >= lo && j <= hi) i = j;
        bounds_[(size_t)k] = i < lo ? lo : (i > hi ? hi : i);
    }
    bounds_[(size_t)n] = height_;
    for (int k = 0; k < n; ++k) parts_[(size_t)k]->SetRowBand(bounds_[(size_t)k], bounds_[(size_t)k + 1]);
    split_pending_ = false;
    balanced_ = true;
    split_scene_generation_ = scene_generation_;
    split_camera_ = p0.camera, split_fov_ = p0.FOV, split_bounces_ = p0.MAXBOUNCES;
}

void MultiGpuRenderer::SetScene(const Scene& scene) {
    for (PathTraceRenderer* p : parts_) p->SetScene(scene);
    ++scene_generation_;
    split_pending_ = true;
}

void MultiGpuRenderer::SetEnvironment(const srt_environment& env) {
    for (PathTraceRenderer* p : parts_) p->SetEnvironment(env);
}

void MultiGpuRenderer::Configure(const Transform& camera, int fov, int max_bounces, uint32_t seed) {
    for (PathTraceRenderer* p : parts_) {
        p->camera = camera;
        p->FOV = fov;
        p->MAXBOUNCES = max_bounces;
        p->seed = seed;
        p->Invalidate();
    }
    split_pending_ = true;
}

void MultiGpuRenderer::Invalidate() {
    for (PathTraceRenderer* p : parts_) p->Invalidate();
    split_pending_ = true;
}

void MultiGpuRenderer::RenderSamples(uint32_t count, bool count_rays) {
    if (split_pending_ && !manual_bands_) {  // the accumulation starts over: the moment rows may change owners
        // The balance probe is the work of about 8 sample-frames on ONE device, synchronous: worth it only for a request that is a
        // multiple of that per device, and not again for inputs the split in force was made for (renderer.hpp).
        if (equal_bands_) {
            EqualBands();
        } else if (SplitIsCurrent()) {
            // (same scene, camera, field of view and bounces: a new seed or an Invalidate() alone does not move the costs)
        } else if ((unsigned long long)count >= (unsigned long long)auto_min_samples_ * parts_.size()) {
            BalanceBands();
        } else if (balanced_) {
            EqualBands();  // a split made for other inputs is worth no more than equal bands, and the request is too small to probe for
        }
    }
    split_pending_ = false;
    for (PathTraceRenderer* p : parts_) p->RenderSamples(count, count_rays);  // asynchronous: one stream per part
    for (size_t i = 1; i < parts_.size(); ++i) {                              // the one gather
        int b, e;
        Band(i, &b, &e);
        int rc = srt_gather_band(parts_[0]->handle(), parts_[i]->handle(), b, e);
        if (rc != SRT_OK) {
            const char* msg = srt_last_error(parts_[0]->handle());
            throw RendererError(rc, std::string("srt_gather_band: ") + (msg ? msg : "?"));
        }
    }
}

void MultiGpuRenderer::Wait() {
    for (size_t i = parts_.size(); i-- > 0;) parts_[i]->Wait();  // part 0 last: its stream waits for every band
}

void MultiGpuRenderer::RenderGBuffer(uint32_t outputs) { parts_[0]->RenderGBufferRows(outputs, 0, height_); }

void MultiGpuRenderer::ReadFramebuffer(void* pixels, size_t pitch_bytes) {
    Wait();
    int rc = srt_read_framebuffer(parts_[0]->handle(), pixels, pitch_bytes, 0, height_);
    if (rc != SRT_OK) {
        const char* msg = srt_last_error(parts_[0]->handle());
        throw RendererError(rc, std::string("srt_read_framebuffer: ") + (msg ? msg : "?"));
    }
}

std::vector<srt_stats> MultiGpuRenderer::Stats() {
    std::vector<srt_stats> out;
    for (PathTraceRenderer* p : parts_) out.push_back(p->Stats());
    return out;
}

}  // namespace srt_host
