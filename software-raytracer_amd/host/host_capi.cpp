// host_capi.cpp — extern "C" view of the C++ host layer, for ctypes (tests, bench.py).
// Scene functions need no GPU; renderer functions go through the C-ABI library.
#include <cstring>
#include <new>
#include <string>

#include "renderer.hpp"
#include "scene.hpp"

using namespace srt_host;

static thread_local std::string g_err;

extern "C" {

struct srt_host_scene {
    Scene scene;
    std::vector<srt_object> flat;
    std::string dump;
    explicit srt_host_scene(const char* path) : scene(path) {}
};

// Scene(file).Load()   (Raytracer/Scene.hpp:18-20,27-80)
srt_host_scene* srt_host_scene_load(const char* path) {
    srt_host_scene* s = new (std::nothrow) srt_host_scene(path ? path : "");
    if (!s) return nullptr;
    s->scene.Load();
    s->flat = s->scene.Flatten();
    return s;
}
srt_host_scene* srt_host_scene_new(const char* path) {
    return new (std::nothrow) srt_host_scene(path ? path : "");
}
void srt_host_scene_free(srt_host_scene* s) { delete s; }
size_t srt_host_scene_count(const srt_host_scene* s) { return s->scene.GetObjects().size(); }
// ObjectsToRender as the C-ABI array; valid until the scene is freed or modified
const srt_object* srt_host_scene_objects(srt_host_scene* s) {
    s->flat = s->scene.Flatten();
    return s->flat.data();
}
// EXTENSION: geometry of the scene's Mesh objects (index = srt_object.mesh); valid until the scene changes
size_t srt_host_scene_mesh_count(srt_host_scene* s) { return s->scene.MeshViews().size(); }
int srt_host_scene_mesh(srt_host_scene* s, size_t i, srt_mesh* out) {
    std::vector<srt_mesh> v = s->scene.MeshViews();
    if (i >= v.size()) return 1;
    *out = v[i];
    return 0;
}
const char* srt_host_scene_error(const srt_host_scene* s) { return s->scene.lastError().c_str(); }
const char* srt_host_scene_name(const srt_host_scene* s) { return s->scene.sceneName.c_str(); }
const char* srt_host_scene_object_name(const srt_host_scene* s, size_t i) {
    return i < s->scene.GetObjects().size() ? s->scene.GetObjects()[i].name.c_str() : "";
}
// Scene::AddObject (Scene.hpp:105-107)
// transform.position of object `index` (the inspector's position edit); 0 when there is no such object
int srt_host_scene_set_position(srt_host_scene* s, size_t index, float x, float y, float z) {
    if (index >= s->scene.Objects().size()) return 0;
    float* p = s->scene.Objects()[index].position;
    p[0] = x, p[1] = y, p[2] = z;
    return 1;
}
void srt_host_scene_add(srt_host_scene* s, const srt_object* o, const char* name) {
    SceneObject so;
    so.type = (RendererType)o->type;
    so.name = name ? name : "";
    for (int i = 0; i < 3; ++i) {
        so.position[i] = o->position[i];
        so.size[i] = o->half_size[i];
    }
    so.radius = o->radius;
    so.material.Smoothness = o->material.smoothness;
    so.material.SpecularAmount = o->material.specular_amount;
    so.material.BaseColor = Color3(o->material.base_color[0], o->material.base_color[1], o->material.base_color[2]);
    so.material.EmissiveColor = Color3(o->material.emissive_color[0], o->material.emissive_color[1], o->material.emissive_color[2]);
    so.material.SpecularColor = Color3(o->material.specular_color[0], o->material.specular_color[1], o->material.specular_color[2]);
    s->scene.AddObject(so);
}
int srt_host_scene_remove(srt_host_scene* s, size_t index) { return s->scene.RemoveObject(index) ? 1 : 0; }
// Scene::SaveAs (Scene.hpp:101-104)
void srt_host_scene_save_as(srt_host_scene* s, const char* path) { s->scene.SaveAs(path); }
// the bytes Save() would write (dump(4)); valid until the next call
const char* srt_host_scene_dump(srt_host_scene* s) {
    s->dump = s->scene.Dump();
    return s->dump.c_str();
}
// Json::format_double, exposed for writer tests
// Json::parse + dump(indent) of an arbitrary document (differential tests against the reference's
// nlohmann/json).  Returns the length written (truncated to cap - 1), or (size_t)-1 on a parse error.
size_t srt_host_json_roundtrip(const char* text, int indent, char* out, size_t cap) {
    try {
        std::string t = Json::parse(text ? text : "").dump(indent);
        if (cap) {
            std::strncpy(out, t.c_str(), cap - 1);
            out[cap - 1] = 0;
        }
        return t.size();
    } catch (const std::exception& e) {
        g_err = e.what();
        return (size_t)-1;
    }
}

size_t srt_host_format_double(double v, char* out, size_t cap) {
    std::string t = Json::format_double(v);
    if (cap) {
        std::strncpy(out, t.c_str(), cap - 1);
        out[cap - 1] = 0;
    }
    return t.size();
}

// Transform::RotateAboutAxis (Common.hpp:287-291): basis = 9 floats right,up,forward
void srt_host_rotate_about_axis(float* right_up_forward, float angle, const float* axis) {
    Transform t;
    t.right = Vec3(right_up_forward[0], right_up_forward[1], right_up_forward[2]);
    t.up = Vec3(right_up_forward[3], right_up_forward[4], right_up_forward[5]);
    t.forward = Vec3(right_up_forward[6], right_up_forward[7], right_up_forward[8]);
    t.RotateAboutAxis(angle, Vec3(axis[0], axis[1], axis[2]));
    const Vec3* v[3] = {&t.right, &t.up, &t.forward};
    for (int i = 0; i < 3; ++i) {
        right_up_forward[3 * i] = v[i]->x;
        right_up_forward[3 * i + 1] = v[i]->y;
        right_up_forward[3 * i + 2] = v[i]->z;
    }
}

// ---- PathTraceRenderer -------------------------------------------------------------
struct srt_host_renderer {
    PathTraceRenderer* r = nullptr;
    std::string error;
};

const char* srt_host_last_error() { return g_err.c_str(); }

srt_host_renderer* srt_host_renderer_create(int device, int width, int height) {
    try {
        srt_host_renderer* h = new srt_host_renderer();
        h->r = new PathTraceRenderer(device, width, height);
        return h;
    } catch (const std::exception& e) {
        g_err = e.what();
        return nullptr;
    }
}
void srt_host_renderer_destroy(srt_host_renderer* h) {
    if (h) {
        delete h->r;
        delete h;
    }
}
#define SRT_HOST_TRY(h, body)                \
    try {                                    \
        body;                                \
        return 0;                            \
    } catch (const RendererError& e) {       \
        g_err = e.what();                    \
        return e.code();                     \
    } catch (const std::exception& e) {      \
        g_err = e.what();                    \
        return SRT_ERR_STATE;                \
    }
int srt_host_renderer_set_scene(srt_host_renderer* h, srt_host_scene* s) { SRT_HOST_TRY(h, h->r->SetScene(s->scene)) }
int srt_host_renderer_set_band(srt_host_renderer* h, int rb, int re) { SRT_HOST_TRY(h, h->r->SetRowBand(rb, re)) }
int srt_host_renderer_settings(srt_host_renderer* h, int fov, int max_bounces, int target_frames, uint32_t seed) {
    h->r->FOV = fov;
    h->r->MAXBOUNCES = max_bounces;
    h->r->TARGETFRAMES = target_frames;
    h->r->seed = seed;
    h->r->Invalidate();
    return 0;
}
// SIMPLEDRAW (:35), SCREEN_SCALE (:30), selectedObject (:53)
int srt_host_renderer_mode(srt_host_renderer* h, int simpledraw, float screen_scale, int selected_object) {
    h->r->SIMPLEDRAW = simpledraw != 0;
    h->r->SCREEN_SCALE = screen_scale;
    h->r->selectedObject = selected_object;
    h->r->Invalidate();
    return 0;
}
int srt_host_renderer_pick(srt_host_renderer* h, int mouse_x, int mouse_y, int* index) { SRT_HOST_TRY(h, *index = h->r->Pick(mouse_x, mouse_y)) }
int srt_host_renderer_set_camera(srt_host_renderer* h, const float* pos, const float* right_up_forward) {
    Transform& t = h->r->camera;
    t.position = Vec3(pos[0], pos[1], pos[2]);
    t.right = Vec3(right_up_forward[0], right_up_forward[1], right_up_forward[2]);
    t.up = Vec3(right_up_forward[3], right_up_forward[4], right_up_forward[5]);
    t.forward = Vec3(right_up_forward[6], right_up_forward[7], right_up_forward[8]);
    h->r->Invalidate();
    return 0;
}
void srt_host_renderer_invalidate(srt_host_renderer* h) { h->r->Invalidate(); }
// returns 1 if a frame was launched, 0 if ACCUMULATIONFRAMES == TARGETFRAMES, <0 on error
int srt_host_renderer_render_frame(srt_host_renderer* h) {
    try {
        return h->r->RenderFrame() ? 1 : 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}
int srt_host_renderer_render_samples(srt_host_renderer* h, uint32_t count, int count_rays) {
    SRT_HOST_TRY(h, h->r->RenderSamples(count, count_rays != 0))
}
int srt_host_renderer_accumulation_frames(srt_host_renderer* h) { return h->r->ACCUMULATIONFRAMES; }
int srt_host_renderer_wait(srt_host_renderer* h) { SRT_HOST_TRY(h, h->r->Wait()) }
int srt_host_renderer_read_framebuffer(srt_host_renderer* h, void* dst, size_t pitch) { SRT_HOST_TRY(h, h->r->ReadFramebuffer(dst, pitch)) }
int srt_host_renderer_read_accumulator(srt_host_renderer* h, float* dst) {
    SRT_HOST_TRY(h, {
        std::vector<float> a = h->r->ReadAccumulator();
        std::memcpy(dst, a.data(), a.size() * sizeof(float));
    })
}
// first-hit buffers of the renderer's band with its current camera (srt_render_gbuffer / srt_read_gbuffer)
int srt_host_renderer_render_gbuffer(srt_host_renderer* h, uint32_t outputs) { SRT_HOST_TRY(h, h->r->RenderGBuffer(outputs)) }
int srt_host_renderer_read_gbuffer(srt_host_renderer* h, uint32_t output, void* dst) { SRT_HOST_TRY(h, h->r->ReadGBuffer(output, dst)) }
// ray queries against the renderer's scene (srt_write_rays + srt_trace_rays / srt_read_ray_output)
int srt_host_renderer_trace_rays(srt_host_renderer* h, const float* origins, const float* directions, size_t count, uint32_t outputs, uint32_t flags) {
    SRT_HOST_TRY(h, h->r->traceRays(origins, directions, count, outputs, flags))
}
// any-hit queries against the renderer's scene (srt_write_rays + srt_trace_occlusion; the result is read_ray_output's SRT_RAYS_OCCLUDED)
int srt_host_renderer_trace_occlusion(srt_host_renderer* h, const float* origins, const float* directions, size_t count, uint32_t flags) {
    SRT_HOST_TRY(h, h->r->traceOcclusion(origins, directions, count, flags))
}
int srt_host_renderer_occlusion_work(srt_host_renderer* h, srt_occlusion_work* out) { SRT_HOST_TRY(h, *out = h->r->occlusionWork()) }
// radiance queries against the renderer's scene (srt_write_rays + srt_trace_radiance)
int srt_host_renderer_trace_radiance(srt_host_renderer* h, const float* origins, const float* directions, size_t count, const srt_radiance_params* p) {
    SRT_HOST_TRY(h, h->r->traceRadiance(origins, directions, count, *p))
}
int srt_host_renderer_read_radiance(srt_host_renderer* h, float* dst) { SRT_HOST_TRY(h, h->r->readRadiance(dst)) }
int srt_host_renderer_radiance_work(srt_host_renderer* h, srt_radiance_work* out) { SRT_HOST_TRY(h, *out = h->r->radianceWork()) }
// light probes against the renderer's scene (srt_write_light_probes + srt_write_light_probe_directions + srt_trace_light_probes)
int srt_host_renderer_trace_light_probes(srt_host_renderer* h, const float* positions, size_t probes, const float* directions, size_t direction_count,
                                         const srt_light_probe_params* p) {
    SRT_HOST_TRY(h, h->r->traceLightProbes(positions, probes, directions, direction_count, *p))
}
int srt_host_renderer_read_light_probe_output(srt_host_renderer* h, uint32_t output, float* dst) { SRT_HOST_TRY(h, h->r->readLightProbeOutput(output, dst)) }
int srt_host_renderer_light_probe_work(srt_host_renderer* h, srt_light_probe_work* out) { SRT_HOST_TRY(h, *out = h->r->lightProbeWork()) }
// probe-grid shading with the renderer's scene and camera (PathTraceRenderer::setProbeGrid / shadeProbeGrid: the coefficients are
// copied unless NULL, the guides rendered, a band of [0, 0) means the renderer's own)
int srt_host_renderer_set_probe_grid(srt_host_renderer* h, const srt_probe_grid* g) { SRT_HOST_TRY(h, h->r->setProbeGrid(*g)) }
int srt_host_renderer_shade_probe_grid(srt_host_renderer* h, const float* coefficients, size_t probes, const srt_probe_grid_params* p) {
    SRT_HOST_TRY(h, h->r->shadeProbeGrid(coefficients, probes, *p))
}
int srt_host_renderer_read_probe_grid_output(srt_host_renderer* h, float* dst) { SRT_HOST_TRY(h, h->r->readProbeGridOutput(dst)) }
int srt_host_renderer_probe_grid_work(srt_host_renderer* h, srt_probe_grid_work* out) { SRT_HOST_TRY(h, *out = h->r->probeGridWork()) }
// probe depth moments against the renderer's scene, and the probe-grid shading that reads them (PathTraceRenderer::traceProbeDepth /
// shadeProbeGridDepth: coefficients and moments are copied unless NULL; the output and the work record are the probe-grid pass's)
int srt_host_renderer_trace_probe_depth(srt_host_renderer* h, const float* positions, size_t probes, const float* directions, size_t direction_count,
                                        const srt_probe_depth_params* p) {
    SRT_HOST_TRY(h, h->r->traceProbeDepth(positions, probes, directions, direction_count, *p))
}
int srt_host_renderer_read_probe_depth_output(srt_host_renderer* h, uint32_t output, void* dst) { SRT_HOST_TRY(h, h->r->readProbeDepthOutput(output, dst)) }
int srt_host_renderer_probe_depth_work(srt_host_renderer* h, srt_probe_depth_work* out) { SRT_HOST_TRY(h, *out = h->r->probeDepthWork()) }
int srt_host_renderer_shade_probe_grid_depth(srt_host_renderer* h, const float* coefficients, const float* moments, size_t probes, uint32_t resolution,
                                             const srt_probe_grid_params* p, const srt_probe_grid_depth_params* d) {
    SRT_HOST_TRY(h, h->r->shadeProbeGridDepth(coefficients, moments, probes, resolution, *p, *d))
}
// probe classification on the renderer's grid and scene, and the probe-grid shading that obeys the records
// (PathTraceRenderer::classifyProbes / shadeProbeGridStates: directions, coefficients, moments and states are copied unless NULL;
// depth may be NULL: no filtered test)
int srt_host_renderer_classify_probes(srt_host_renderer* h, const float* directions, size_t direction_count, const srt_probe_classify_params* p) {
    SRT_HOST_TRY(h, h->r->classifyProbes(directions, direction_count, *p))
}
int srt_host_renderer_read_probe_states_output(srt_host_renderer* h, uint32_t output, void* dst) { SRT_HOST_TRY(h, h->r->readProbeStatesOutput(output, dst)) }
int srt_host_renderer_probe_classify_work(srt_host_renderer* h, srt_probe_classify_work* out) { SRT_HOST_TRY(h, *out = h->r->probeClassifyWork()) }
int srt_host_renderer_shade_probe_grid_states(srt_host_renderer* h, const float* coefficients, const float* moments, const float* states, size_t probes,
                                              uint32_t resolution, const srt_probe_grid_params* p, const srt_probe_grid_depth_params* d) {
    SRT_HOST_TRY(h, h->r->shadeProbeGridStates(coefficients, moments, states, probes, resolution, *p, d))
}
// per-frame probe updates on the renderer's handle (PathTraceRenderer::listProbes ... probeBlendWork: states, positions, directions
// and previous records are copied unless NULL)
int srt_host_renderer_list_probes(srt_host_renderer* h, const float* states, size_t probes, const srt_probe_list_params* p) {
    SRT_HOST_TRY(h, h->r->listProbes(states, probes, *p))
}
int srt_host_renderer_read_probe_list_output(srt_host_renderer* h, uint32_t* dst) { SRT_HOST_TRY(h, h->r->readProbeListOutput(dst)) }
int srt_host_renderer_probe_list_work(srt_host_renderer* h, srt_probe_list_work* out) { SRT_HOST_TRY(h, *out = h->r->probeListWork()) }
int srt_host_renderer_trace_light_probes_listed(srt_host_renderer* h, const float* positions, size_t probes, const float* directions, size_t direction_count,
                                                const srt_light_probe_params* p) {
    SRT_HOST_TRY(h, h->r->traceLightProbesListed(positions, probes, directions, direction_count, *p))
}
int srt_host_renderer_trace_probe_depth_listed(srt_host_renderer* h, const float* positions, size_t probes, const float* directions, size_t direction_count,
                                               const srt_probe_depth_params* p) {
    SRT_HOST_TRY(h, h->r->traceProbeDepthListed(positions, probes, directions, direction_count, *p))
}
int srt_host_renderer_reset_probe_history(srt_host_renderer* h, uint32_t which, size_t probes, uint32_t resolution) {
    SRT_HOST_TRY(h, h->r->resetProbeHistory(which, probes, resolution))
}
int srt_host_renderer_blend_probes(srt_host_renderer* h, const float* previous_states, size_t probes, const srt_probe_blend_params* p) {
    SRT_HOST_TRY(h, h->r->blendProbes(previous_states, probes, *p))
}
int srt_host_renderer_read_probe_history(srt_host_renderer* h, uint32_t which, float* dst) { SRT_HOST_TRY(h, h->r->readProbeHistory(which, dst)) }
int srt_host_renderer_probe_blend_work(srt_host_renderer* h, srt_probe_blend_work* out) { SRT_HOST_TRY(h, *out = h->r->probeBlendWork()) }
// scrolling the renderer's grid (PathTraceRenderer::scrollProbes / followProbeGrid / probeScrollWork)
int srt_host_renderer_scroll_probes(srt_host_renderer* h, const int32_t* shift, uint32_t which, uint32_t flags) {
    SRT_HOST_TRY(h, h->r->scrollProbes(shift, which, flags))
}
int srt_host_renderer_follow_probe_grid(srt_host_renderer* h, const float* point, int32_t* shift) { SRT_HOST_TRY(h, {
        const auto s = h->r->followProbeGrid(point);
        std::memcpy(shift, s.data(), sizeof s);
    })
}
int srt_host_renderer_probe_scroll_work(srt_host_renderer* h, srt_probe_scroll_work* out) { SRT_HOST_TRY(h, *out = h->r->probeScrollWork()) }
// probe cascades on the renderer's handle (PathTraceRenderer::setProbeCascade / captureProbeCascadeLevel / shadeProbeCascade /
// probeCascadeWork: the guides are rendered, a band of [0, 0) means the renderer's own; the output is the probe-grid pass's)
int srt_host_renderer_set_probe_cascade(srt_host_renderer* h, const srt_probe_cascade* c) { SRT_HOST_TRY(h, h->r->setProbeCascade(*c)) }
int srt_host_renderer_capture_probe_cascade_level(srt_host_renderer* h, uint32_t level, uint32_t which) {
    SRT_HOST_TRY(h, h->r->captureProbeCascadeLevel(level, which))
}
int srt_host_renderer_shade_probe_cascade(srt_host_renderer* h, const srt_probe_cascade_params* p) { SRT_HOST_TRY(h, h->r->shadeProbeCascade(*p)) }
int srt_host_renderer_probe_cascade_work(srt_host_renderer* h, srt_probe_cascade_work* out) { SRT_HOST_TRY(h, *out = h->r->probeCascadeWork()) }
// adaptive sampling on the handle's buffers as they stand (srt_sample_budget + srt_get_budget_total, srt_render_adaptive; a band
// of [0, 0) means the renderer's own), and the two-half workflow (PathTraceRenderer::renderAdaptiveFrame; counts may be NULL)
int srt_host_renderer_sample_budget(srt_host_renderer* h, const srt_budget_params* p, uint64_t* total) { SRT_HOST_TRY(h, *total = h->r->sampleBudget(*p)) }
int srt_host_renderer_render_adaptive(srt_host_renderer* h, const srt_adaptive_params* p) { SRT_HOST_TRY(h, h->r->renderAdaptive(*p)) }
int srt_host_renderer_set_sample_counts(srt_host_renderer* h, uint32_t value) { SRT_HOST_TRY(h, h->r->setSampleCounts(value)) }
int srt_host_renderer_read_sample_counts(srt_host_renderer* h, uint32_t* dst) { SRT_HOST_TRY(h, h->r->readSampleCounts(dst)) }
int srt_host_renderer_adaptive_frame(srt_host_renderer* h, uint32_t spp, int rounds, const srt_budget_params* budget, uint32_t max_samples, uint32_t* counts,
                                     uint64_t* total) {
    SRT_HOST_TRY(h, {
        std::vector<uint32_t> n;
        *total = h->r->renderAdaptiveFrame(spp, rounds, *budget, max_samples, counts ? &n : nullptr);
        if (counts) std::memcpy(counts, n.data(), n.size() * sizeof(uint32_t));
    })
}
// per-pixel visibility: the guides of the band, then srt_render_visibility (a band of [0, 0) means the renderer's own)
int srt_host_renderer_render_visibility(srt_host_renderer* h, const srt_visibility_params* p) { SRT_HOST_TRY(h, h->r->renderVisibility(*p)) }
int srt_host_renderer_read_visibility(srt_host_renderer* h, uint32_t output, float* dst) { SRT_HOST_TRY(h, h->r->readVisibility(output, dst)) }
int srt_host_renderer_visibility_work(srt_host_renderer* h, srt_visibility_work* out) { SRT_HOST_TRY(h, *out = h->r->visibilityWork()) }
// reflection guides: the pass itself (a band of [0, 0) means the renderer's own), its outputs and work record, and the switch that
// makes RenderGBuffer — so every pass that takes its guides from it — render them (PathTraceRenderer::reflectionGuides; bounces < 0
// keeps reflectionBounces as it is)
int srt_host_renderer_render_reflection(srt_host_renderer* h, const srt_reflection_params* p) { SRT_HOST_TRY(h, h->r->renderReflectionGBuffer(*p)) }
int srt_host_renderer_read_reflection(srt_host_renderer* h, uint32_t output, void* dst) { SRT_HOST_TRY(h, h->r->readReflection(output, dst)) }
int srt_host_renderer_reflection_work(srt_host_renderer* h, srt_reflection_work* out) { SRT_HOST_TRY(h, *out = h->r->reflectionWork()) }
int srt_host_renderer_reflection_guides(srt_host_renderer* h, int on, int bounces) {
    SRT_HOST_TRY(h, {
        if (bounces >= 0) h->r->reflectionBounces = bounces;
        h->r->reflectionGuides(on != 0);
    })
}
// the mirror history of RenderTemporalFrame (PathTraceRenderer::mirrorHistory; radius_pixels <= 0 keeps mirrorRadius as it is)
int srt_host_renderer_mirror_history(srt_host_renderer* h, int on, float radius_pixels) {
    SRT_HOST_TRY(h, {
        if (radius_pixels > 0.0f) h->r->mirrorRadius = radius_pixels;
        h->r->mirrorHistory(on != 0);
    })
}
// the probe tail of the radiance and light-probe traces (PathTraceRenderer::probeTail) and its work record
int srt_host_renderer_probe_tail(srt_host_renderer* h, const srt_probe_tail_params* p) { SRT_HOST_TRY(h, h->r->probeTail(*p)) }
int srt_host_renderer_probe_tail_work(srt_host_renderer* h, srt_probe_tail_work* out) { SRT_HOST_TRY(h, *out = h->r->probeTailWork()) }
// pictures under the probe tail: srt_render_adaptive_tail (a band of [0, 0) means the renderer's own) and one whole frame of it
int srt_host_renderer_render_adaptive_tail(srt_host_renderer* h, const srt_adaptive_params* p) { SRT_HOST_TRY(h, h->r->renderAdaptiveTail(*p)) }
int srt_host_renderer_render_probe_tail_frame(srt_host_renderer* h, uint32_t spp, int bounces, uint32_t seed) {
    SRT_HOST_TRY(h, h->r->renderProbeTailFrame(spp, bounces, seed))
}
// sun sampling in renderAdaptiveFrame and renderProbeTailFrame (PathTraceRenderer::sunSampling)
int srt_host_renderer_sun_sampling(srt_host_renderer* h, int on) { SRT_HOST_TRY(h, h->r->sunSampling(on != 0)) }
int srt_host_renderer_read_ray_output(srt_host_renderer* h, uint32_t output, void* dst) { SRT_HOST_TRY(h, h->r->readRayOutput(output, dst)) }
// denoiser over the whole frame with the guides as they stand (srt_denoise / srt_read_denoised)
int srt_host_renderer_denoise(srt_host_renderer* h, const srt_denoise_params* p) { SRT_HOST_TRY(h, h->r->Denoise(*p)) }
int srt_host_renderer_read_denoised(srt_host_renderer* h, float* dst) { SRT_HOST_TRY(h, h->r->ReadDenoised(dst)) }
// temporal reprojection (srt_temporal_accumulate / srt_read_history_length) and the temporal frame of a moving camera
int srt_host_renderer_temporal(srt_host_renderer* h, const srt_temporal_params* p) { SRT_HOST_TRY(h, h->r->Temporal(*p)) }
int srt_host_renderer_read_history_length(srt_host_renderer* h, float* dst) { SRT_HOST_TRY(h, h->r->ReadHistoryLength(dst)) }
int srt_host_renderer_render_temporal_frame(srt_host_renderer* h, uint32_t spp, int denoise) {
    SRT_HOST_TRY(h, h->r->RenderTemporalFrame(spp, denoise != 0))
}
// a camera move that keeps the temporal history: srt_host_renderer_set_camera without the Invalidate()
int srt_host_renderer_move_camera(srt_host_renderer* h, const float* pos, const float* right_up_forward) {
    Transform& t = h->r->camera;
    t.position = Vec3(pos[0], pos[1], pos[2]);
    t.right = Vec3(right_up_forward[0], right_up_forward[1], right_up_forward[2]);
    t.up = Vec3(right_up_forward[3], right_up_forward[4], right_up_forward[5]);
    t.forward = Vec3(right_up_forward[6], right_up_forward[7], right_up_forward[8]);
    return 0;
}
// an object edit that keeps the temporal history (srt_update_scene), and the motion-vector output (srt_motion_output / srt_read_motion)
int srt_host_renderer_update_scene(srt_host_renderer* h, srt_host_scene* s) { SRT_HOST_TRY(h, h->r->UpdateScene(s->scene)) }
// the refitUpdates setting of SetScene / UpdateScene (srt_update_mode) and what the last update did (srt_get_update_info)
int srt_host_renderer_refit_updates(srt_host_renderer* h, int on) {
    h->r->refitUpdates = on != 0;
    return 0;
}
int srt_host_renderer_update_info(srt_host_renderer* h, srt_update_info* out) { SRT_HOST_TRY(h, *out = h->r->UpdateInfo()) }
int srt_host_renderer_motion_output(srt_host_renderer* h, int on) { SRT_HOST_TRY(h, h->r->MotionOutput(on != 0)) }
int srt_host_renderer_read_motion(srt_host_renderer* h, float* dst) { SRT_HOST_TRY(h, h->r->ReadMotion(dst)) }
// guided upsampler over the whole frame with the guides as they stand (srt_upsample / srt_read_upsampled), and the
// guidedUpsample setting of RenderFrame
int srt_host_renderer_upsample(srt_host_renderer* h, const srt_upsample_params* p) { SRT_HOST_TRY(h, h->r->Upsample(*p)) }
int srt_host_renderer_read_upsampled(srt_host_renderer* h, float* dst) { SRT_HOST_TRY(h, h->r->ReadUpsampled(dst)) }
int srt_host_renderer_guided_upsample(srt_host_renderer* h, int on) {
    h->r->guidedUpsample = on != 0;
    return 0;
}
// anti-aliasing over the whole frame (PathTraceRenderer::Antialias renders the OBJECT guide and the sub-samples when they are
// stale), its result, and the antialias setting of RenderFrame / RenderTemporalFrame (0 = off)
int srt_host_renderer_antialias(srt_host_renderer* h, const srt_antialias_params* p) { SRT_HOST_TRY(h, h->r->Antialias(p->k, p->source, p->flags)) }
int srt_host_renderer_read_antialiased(srt_host_renderer* h, float* dst) { SRT_HOST_TRY(h, h->r->ReadAntialiased(dst)) }
int srt_host_renderer_set_antialias(srt_host_renderer* h, int k) {
    if (k < 0 || k > 4) return SRT_ERR_INVALID_ARG;
    h->r->antialias = k;
    return 0;
}
// one variance-guided denoised frame of spp samples in two halves (PathTraceRenderer::denoiseVariance), and its variance estimate
int srt_host_renderer_denoise_variance(srt_host_renderer* h, uint32_t spp, uint32_t flags) { SRT_HOST_TRY(h, h->r->denoiseVariance(spp, flags)) }
int srt_host_renderer_read_variance(srt_host_renderer* h, float* dst) { SRT_HOST_TRY(h, h->r->ReadVariance(dst)) }
// the temporalVariance setting of RenderTemporalFrame, and the moments of the last temporal frame (srt_read_moments)
int srt_host_renderer_temporal_variance(srt_host_renderer* h, int on) {
    h->r->temporalVariance = on != 0;
    return 0;
}
int srt_host_renderer_read_moments(srt_host_renderer* h, float* dst) { SRT_HOST_TRY(h, h->r->ReadMoments(dst)) }
int srt_host_renderer_stats(srt_host_renderer* h, srt_stats* out) { SRT_HOST_TRY(h, *out = h->r->Stats()) }
void* srt_host_renderer_handle(srt_host_renderer* h) { return h->r->handle(); }

// ---- MultiGpuRenderer -----------------------------------------------------------------
struct srt_host_multi {
    MultiGpuRenderer* r = nullptr;
};
srt_host_multi* srt_host_multi_create(const int* devices, int n, int width, int height) {
    try {
        srt_host_multi* h = new srt_host_multi();
        h->r = new MultiGpuRenderer(std::vector<int>(devices, devices + n), width, height);
        return h;
    } catch (const std::exception& e) {
        g_err = e.what();
        return nullptr;
    }
}
void srt_host_multi_destroy(srt_host_multi* h) {
    if (h) {
        delete h->r;
        delete h;
    }
}
int srt_host_multi_set_scene(srt_host_multi* h, srt_host_scene* s) { SRT_HOST_TRY(h, h->r->SetScene(s->scene)) }
int srt_host_multi_configure(srt_host_multi* h, const float* pos, const float* right_up_forward, int fov, int max_bounces, uint32_t seed) {
    Transform t;
    t.position = Vec3(pos[0], pos[1], pos[2]);
    t.right = Vec3(right_up_forward[0], right_up_forward[1], right_up_forward[2]);
    t.up = Vec3(right_up_forward[3], right_up_forward[4], right_up_forward[5]);
    t.forward = Vec3(right_up_forward[6], right_up_forward[7], right_up_forward[8]);
    SRT_HOST_TRY(h, h->r->Configure(t, fov, max_bounces, seed))
}
int srt_host_multi_render_samples(srt_host_multi* h, uint32_t count, int count_rays) { SRT_HOST_TRY(h, h->r->RenderSamples(count, count_rays != 0)) }
int srt_host_multi_read_framebuffer(srt_host_multi* h, void* dst, size_t pitch) { SRT_HOST_TRY(h, h->r->ReadFramebuffer(dst, pitch)) }
int srt_host_multi_band(srt_host_multi* h, int i, int* begin, int* end) { SRT_HOST_TRY(h, h->r->Band((size_t)i, begin, end)) }
int srt_host_multi_balance(srt_host_multi* h) { SRT_HOST_TRY(h, h->r->BalanceBands()) }
int srt_host_multi_use_equal_bands(srt_host_multi* h, int equal) { SRT_HOST_TRY(h, h->r->UseEqualBands(equal != 0)) }
int srt_host_multi_use_manual_bands(srt_host_multi* h, int manual) { SRT_HOST_TRY(h, h->r->UseManualBands(manual != 0)) }
int srt_host_multi_set_auto_balance_min_samples(srt_host_multi* h, uint32_t per_device) { SRT_HOST_TRY(h, h->r->SetAutoBalanceMinSamples(per_device)) }
int srt_host_multi_set_row_band(srt_host_multi* h, int i, int begin, int end) { SRT_HOST_TRY(h, h->r->part((size_t)i).SetRowBand(begin, end)) }
int srt_host_multi_stats(srt_host_multi* h, srt_stats* out, int n) {
    SRT_HOST_TRY(h, {
        std::vector<srt_stats> st = h->r->Stats();
        for (int i = 0; i < n && i < (int)st.size(); ++i) out[i] = st[(size_t)i];
    })
}

}  // extern "C"
