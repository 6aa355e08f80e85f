// srt_capi.hip — implementation of include/srt_pathtrace.h on HIP (gfx950).
//
// Host duties only: flatten ObjectsToRender into the device scene image, fold the
// frame-constant camera terms of GetRayDirection (Raytracer.cpp:111-115: tanf, aspect),
// launch srt::pathtrace_kernel on the handle's stream, move buffers.  No CPU fallback:
// without a usable HIP device srt_create fails.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <exception>
#include <new>
#include <type_traits>
#include <vector>

#include "srt_kernel.hip.h"
#include "srt_gbuffer.hip.h"
#include "srt_denoise.hip.h"
#include "srt_temporal.hip.h"
#include "srt_upsample.hip.h"
#include "srt_antialias.hip.h"
#include "srt_variance.hip.h"
#include "srt_moments.hip.h"
#include "srt_refit.hip.h"
#include "srt_rays.hip.h"
#include "srt_outputs_host.h"
#include "srt_rays_host.h"
#include "srt_occlusion.hip.h"
#include "srt_occlusion_host.h"
#include "srt_visibility.hip.h"
#include "srt_visibility_host.h"
#include "srt_reflection.hip.h"
#include "srt_reflection_host.h"
#include "srt_mirror_history.hip.h"
#include "srt_mirror_history_host.h"
#include "srt_radiance.hip.h"
#include "srt_radiance_host.h"
#include "srt_light_probes.hip.h"
#include "srt_light_probes_host.h"
#include "srt_probe_grid.hip.h"
#include "srt_probe_grid_host.h"
#include "srt_probe_depth.hip.h"
#include "srt_probe_depth_host.h"
#include "srt_probe_states.hip.h"
#include "srt_probe_states_host.h"
#include "srt_probe_update.hip.h"
#include "srt_probe_update_host.h"
#include "srt_probe_scroll.hip.h"
#include "srt_probe_scroll_host.h"
#include "srt_probe_cascade.hip.h"
#include "srt_probe_cascade_host.h"
#include "srt_probe_tail.hip.h"
#include "srt_probe_tail_host.h"
#include "srt_sun_sampling.hip.h"
#include "srt_sun_sampling_host.h"
#include "srt_adaptive.hip.h"
#include "srt_adaptive_host.h"
#include "srt_adaptive_tail_host.h"
#include "srt_adaptive_sun_host.h"
#include "srt_launch_shape.h"
#include "srt_scene_image.h"
#include "srt_mesh_bvh.h"
#include "srt_pathtrace.h"

namespace {

thread_local char g_create_error[512] = "";

// Tuning switches.  The shipped library has none: every value below is a constant.  A development build
// (make -C software-raytracer_amd/csrc dev -> libsrt_pathtrace_dev.so, -DSRT_DEV) reads them from the
// environment for in-process A/B timing (tests/ab_bench.py); all settings produce identical bits.
#ifndef SRT_FILL_MIN
#define SRT_FILL_MIN 0.85  // mesh launches: simulated fill of the chip's workgroup slots below which a launch of >= 256 spp is cut into four sample chunks
#endif
#ifndef SRT_ORDER_MIN_WG
#define SRT_ORDER_MIN_WG 256  // fewest blocks of tiles for which a launch records costs and is dispatched in cost order (round 3: 512 -> 256,
                              // the 48..64-row bands of a cost-balanced 8-rank 1080p frame: -4..-5 %)
#endif
struct DevSwitches {
    int kernel = 0;        // SRT_KERNEL: tuning variant
    bool no_cluster = false;  // SRT_NO_CLUSTER
    int tile_h = 0;        // SRT_TILE_H: 8/4/2/1 forces the tile height
    int defer = -1;        // SRT_DEFER: 0 never chunk samples, n > 0 force n samples per chunk
    bool lpt = true;       // SRT_LPT=0: natural dispatch order
    int lpt_buckets = 128; // SRT_LPT_BUCKETS
    int chunk_beta = 30;   // SRT_CHUNK_BETA (percent): sample chunks from recorded block costs, see srt_render
    bool host_order = true;  // SRT_HOST_ORDER=0: no host-derived initial dispatch order
    int kernel_flags = 0;    // SRT_KFLAGS: extra KernelParams.flags bits of timing experiments
    bool chain = true;       // SRT_CHAIN=0: every chunk of a sample-chunked launch goes through the sample buffer (round 3's form)
};
#ifdef SRT_DEV
const DevSwitches& dev_switches() {
    static const DevSwitches sw = [] {
        DevSwitches d;
        auto geti = [](const char* name, int dflt) {
            const char* v = getenv(name);
            return v ? atoi(v) : dflt;
        };
        d.kernel = geti("SRT_KERNEL", 0);
        d.no_cluster = getenv("SRT_NO_CLUSTER") != nullptr;
        d.tile_h = geti("SRT_TILE_H", 0);
        d.defer = geti("SRT_DEFER", -1);
        d.lpt = geti("SRT_LPT", 1) != 0;
        int b = geti("SRT_LPT_BUCKETS", 128);
        d.lpt_buckets = b < 2 ? 2 : (b > 4096 ? 4096 : b);
        d.chunk_beta = geti("SRT_CHUNK_BETA", 30);
        d.host_order = geti("SRT_HOST_ORDER", 1) != 0;
        d.kernel_flags = geti("SRT_KFLAGS", 0);
        d.chain = geti("SRT_CHAIN", 1) != 0;
        return d;
    }();
    return sw;
}
#else
constexpr DevSwitches k_dev_switches{};
constexpr const DevSwitches& dev_switches() { return k_dev_switches; }
#endif

constexpr size_t REC_WORDS = 1 + 4 * srt::TALLY_N;  // per block in the cost record: wave time, then TALLY_N counts for each of the four waves
// srt_launch_shape.h is host-only C++ (unit-tested on the CPU) and repeats the kernel's tile geometry:
static_assert(srt::OUT_TILE == srt::TILE_W && srt::OUT_TILE == srt::TILE_H && srt::OUT_WG_UNITS == srt::WG_TILES_X * srt::WG_TILES_Y, "srt_outputs_host.h and srt_kernel.hip.h disagree");
static_assert(srt::SHAPE_TILE_H == srt::TILE_H && srt::SHAPE_WG_W == srt::WG_W && srt::SHAPE_WG_H == srt::WG_H && srt::SHAPE_WG_TILES_Y == srt::WG_TILES_Y &&
              srt::SHAPE_WAVES_PER_WG == srt::WG_TILES_X * srt::WG_TILES_Y && srt::SHAPE_TALLY_N == srt::TALLY_N && srt::SHAPE_ROWS_WG_SCRATCH_BYTES == (size_t)srt::WG_SCRATCH_BYTES_ROWS,
              "srt_launch_shape.h and srt_kernel.hip.h disagree");

struct HostCamera {
    srt_camera cam;
    bool set = false;
};

// Owners of one HIP resource each: the destructor frees it, with the context's device current (srt_destroy sets it).
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};

// Device (or pinned host) memory.  ensure(bytes) allocates when the buffer is empty or smaller than bytes, without keeping the old
// contents; after a failure the buffer is empty.
template <class T, bool PINNED = false>
class Buffer : NoCopy {
  public:
    ~Buffer() { reset(); }
    operator T*() const { return p_; }
    size_t bytes() const { return bytes_; }
    void reset() {
        if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr, bytes_ = 0;
    }
    hipError_t ensure(size_t bytes) {
        if (p_ && bytes <= bytes_) return hipSuccess;
        reset();
        const hipError_t e = PINNED ? hipHostMalloc((void**)&p_, bytes, hipHostMallocDefault) : hipMalloc((void**)&p_, bytes);
        if (e == hipSuccess) bytes_ = bytes;
        else p_ = nullptr;
        return e;
    }
    void swap(Buffer& o) {
        T* const p = p_;
        const size_t b = bytes_;
        p_ = o.p_, bytes_ = o.bytes_, o.p_ = p, o.bytes_ = b;
    }

  private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};
template <class T> using DeviceBuffer = Buffer<T>;
template <class T> using PinnedBuffer = Buffer<T, true>;

// The work record of a counting launch: N counters the kernel adds to (the pass's *_WORK_N, in its enum's order), never an output
// buffer.  The count is part of the type, so zero_work and read_work cannot be given another pass's.
template <int N>
struct WorkBuffer : DeviceBuffer<unsigned long long> {};

// An event or stream, created into h.
template <class H, hipError_t (*DESTROY)(H)>
struct Handle : NoCopy {
    H h = nullptr;
    ~Handle() { if (h) (void)DESTROY(h); }
    operator H() const { return h; }
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

}  // namespace

// Members are destroyed in reverse order: the buffers and events first, the own stream last.
struct srt_context {
    int device = 0;
    int width = 0, height = 0;
    Stream own_stream;
    hipStream_t stream = nullptr;  // launch stream (own or caller's)
    Event ev_begin, ev_end;
    bool launched = false;

    // device buffers
    // two images of the same scene: [0] clustered (default), [1] plain brute force (A/B aid)
    DeviceBuffer<float4> d_scene[2];
    srt::SceneLayout layout[2];
    bool scene_set = false;
    std::vector<float4> h_scene[2];  // staging for the async upload

    DeviceBuffer<uint32_t> d_fb_own;
    DeviceBuffer<float4> d_acc_own;
    uint32_t* d_fb = nullptr;
    float4* d_acc = nullptr;
    DeviceBuffer<unsigned long long> d_rays;
    DeviceBuffer<unsigned long long> d_work;  // SRT_RENDER_COUNT_WORK: the launch's loop counts (srt::TALLY_ALL words)
    DeviceBuffer<int> d_pick;
    int last_pick[4] = {0, 0, 0, 0};  // list index, distance bits, primitive id, normal.z bits (debug)

    // EXTENSION: triangle meshes
    std::vector<srt::HostMesh> meshes;
    srt::MeshImage mesh_image;
    DeviceBuffer<float4> d_bvh_nodes;
    DeviceBuffer<float4> d_bvh_tris;
    DeviceBuffer<int32_t> d_bvh_gidpos;

    // refitting the mesh image (srt_update_mode, srt_refit.hip.h): the mode, what the last successful srt_update_scene did, and the
    // refit data — every mesh's vertices, the triangles' vertex indices, the exact boxes of triangles and nodes, the objects'
    // positions — which is on the device only for a mesh image built while the mode was SRT_UPDATE_REFIT (refit_ready) and is
    // out of date once srt_set_meshes has replaced the geometry (meshes_stale, until the next build).  The staging vectors are
    // rewritten only behind the stream synchronisation every scene change starts with.
    int update_mode = SRT_UPDATE_REBUILD;
    srt_update_info update_info{};
    bool refit_ready = false;
    bool meshes_stale = false;
    DeviceBuffer<float4> d_refit_verts;
    DeviceBuffer<uint32_t> d_refit_tri_verts;
    DeviceBuffer<float4> d_refit_tri_box;
    DeviceBuffer<float4> d_refit_node_box;
    DeviceBuffer<float4> d_refit_pos;
    std::vector<float4> h_refit_verts;
    std::vector<float4> h_refit_pos;

    // sample-chunked launches (narrow row bands at high sample counts): sample colours + per-tile masks
    DeviceBuffer<float4> d_samples;
    DeviceBuffer<unsigned long long> d_tile_masks;
    DeviceBuffer<uint32_t> d_tile_chain;  // sample-chunked launches: chunks of a tile folded in order so far (KernelParams.tile_chain)

    // cost-ordered dispatch: a launch may record the ray count of every block of tiles; once that copy has
    // arrived (polled, never waited for) later launches of the same grid start the expensive blocks first
    DeviceBuffer<uint32_t> d_wg_cost;
    DeviceBuffer<uint32_t> d_wg_est;  // estimated block costs (block_cost_kernel), input of order_sort_kernel
    DeviceBuffer<uint32_t> d_wg_order;
    PinnedBuffer<uint32_t> h_wg_cost;
    PinnedBuffer<uint32_t> h_wg_order;
    unsigned order_gx = 0, order_gy = 0;  // grid the order in d_wg_order was made for (0 = none)
    unsigned rec_gx = 0, rec_gy = 0;      // grid of the recording in flight
    bool recording = false;               // a cost copy is in flight (ev_cost)
    bool rec_has_work = false;            // ... and behind the times it holds the waves' loop counts (the recording launch was a TALLY instantiation)
    double rec_step_w = 0.0;              // what a pool step of the recorded launch weighs (probe_step_weight: depends on the scene's layout)
    int work_layout[4] = {0, 0, 0, 0};    // of the last launch: uniform spheres, clusters, spheres per cluster, boxes (srt_get_work_counts)
    bool order_stale = true;              // scene / camera changed since the costs were recorded
    // the launch-shape record (round 4): every block's WORK as the recording launch counted it — loop trips under the balance
    // probe's weights, not times — so the sample-chunk rule is a deterministic function of scene, camera, band and call history
    srt::WorkRecord work;                 // the launch-shape record of the current band (srt_launch_shape.h)
    int band_y0 = -1, band_rows = -1;     // the row band the order, the recording and the cost figures above belong to
    bool estimate_stale = true;           // the scene changed since the order was last estimated on the device
    bool order_disabled = false;          // buffers for the feedback could not be allocated
    Event ev_cost, ev_order, ev_gather, ev_read;
    unsigned long long peer_asked = 0;    // srt_gather_band: destination devices this context has asked hipDeviceCanAccessPeer about (once per pair)
    unsigned long long peer_direct = 0;   // ... and those it may reach directly (peer access enabled)
    char gather_path[160] = "no gather yet";  // which way this context's last srt_gather_band went (srt_gather_path)

    srt_environment env;
    HostCamera camera;
    srt_stats stats{};
    bool stats_pending = false;
    uint64_t pending_samples = 0;
    uint32_t pending_chunks = 1;
    bool count_rays = false;
    bool count_work = false, count_work_valid = false;
    bool pending_timed = true;  // the last render was bracketed by ev_begin / ev_end (not SRT_RENDER_NO_TIMING)
    uint32_t pending_tile_rows = 8, pending_chunk_samples = 0, pending_shape_source = 0;
    srt_work_counts work_counts{};
    int lds_limit_bytes = 64 * 1024;
    int cu_count = 256;
    bool scene_in_lds[2] = {true, true};  // per scene image: does it fit into LDS next to the scratch?
    bool pick_in_lds[2] = {true, true};
    int variant = -1;  // >= 0 overrides SRT_KERNEL (set through srt_debug_set_variant)
#ifdef SRT_DEV
    // srt_debug_set_chain / srt_debug_set_shape: per-handle development settings (the environment switches are read once per process)
    int chain_mode = srt::DEV_CHAIN_NATURAL;
    uint32_t chain_arg = 0;
    int shape_defer = -2;     // < -1: SRT_DEFER
    int shape_no_taper = -1;  // < 0: SRT_KFLAGS & 0x400
    // the last sample-chunked launch, for srt_debug_read_chain
    int chain_layers = 0, chain_chunk = 0, chain_chunk_full = 0, chain_wg_x = 0;
    size_t chain_tiles = 0;
    bool chain_used = false;  // it had a chain buffer (KernelParams.tile_chain)
    int chain_used_mode = srt::DEV_CHAIN_NATURAL;
    uint32_t chain_used_arg = 0;
#endif

    // Every output a caller can bind or read back is an own buffer (allocated on first use) and an srt::OutputSlot
    // (srt_outputs_host.h): the caller's bound buffer (srt_bind_*; NULL = own) and the record of what has been written.  DESIGN.md
    // §4.21 lists them with the rule each srt_read_* applies.  The ray and probe passes below keep, in their state, the shared
    // records of the same header: a CallRecord (has the pass run, did its last call count work), a LastOutputs (which outputs that
    // call wrote, and where) and InputArrays (which input array is current); a counting launch adds to a WorkBuffer<*_WORK_N>,
    // zeroed on the stream in front of it and never an output buffer.

    // first-hit buffers (srt_render_gbuffer), one per SRT_GBUF_* bit
    DeviceBuffer<void> d_gbuf_own[4];
    srt::OutputSlot gbuf[4];

    // denoiser (srt_denoise, srt_denoise_variance): the result, and the ping-pong buffer of the preparation pass and the levels
    // before the last
    DeviceBuffer<float4> d_dn_own;
    DeviceBuffer<float4> d_dn_tmp;
    srt::OutputSlot dn;

    // the camera each own first-hit slot was last rendered with (srt_temporal_accumulate refuses own guides of another camera)
    srt_camera gbuf_own_cam[4] = {};
    bool gbuf_own_cam_set[4] = {false, false, false, false};

    // temporal reprojection (srt_temporal_accumulate): two history slots of three W*H float4 arrays each (allocated on first
    // use), the slot the last call wrote and the camera it was written with, whether that history may be reprojected (false
    // after a scene, mesh or environment change), and whether any call has been enqueued yet (srt_read_history_length)
    DeviceBuffer<float4> d_tp[2][3];
    int tp_cur = 0;
    srt_camera tp_cam{};
    bool tp_valid = false;
    bool tp_written = false;

    // object motion (srt_update_scene): the object list the scene was last made from, and the list as it stood at the last
    // srt_temporal_accumulate (the one the history's points belong to).  The table of per-object displacements between the two
    // is staged in h_tp_table and uploaded on the launch stream; ev_tp_table marks the end of that upload (the staging is not
    // rewritten before).
    std::vector<srt_object> objects;
    std::vector<srt_object> tp_objects;
    PinnedBuffer<float4> h_tp_table;
    DeviceBuffer<float4> d_tp_table;
    Event ev_tp_table;
    bool tp_table_in_flight = false;
    // the motion-vector output (srt_motion_output; srt_read_motion reads no buffer but the one the last call with the output on wrote)
    bool mv_on = false;
    DeviceBuffer<float4> d_mv_own;
    srt::OutputSlot mv;

    // guided upsampler (srt_upsample; an in-place call writes no result buffer)
    DeviceBuffer<float4> d_up_own;
    srt::OutputSlot up;

    // anti-aliasing (srt_render_subsamples, srt_antialias).  The sub-sample planes: the own buffer is re-allocated when k grows,
    // and the slot's count is the k of the last render, into whichever buffer.  What the OWN buffer holds: its k, the camera and the
    // scene (a count of scene changes) it was rendered with, and the memory rows rendered with exactly those so far — srt_antialias
    // refuses an own buffer that is not a whole frame of the current scene and camera.
    DeviceBuffer<int32_t> d_ss_own;
    srt::OutputSlot ss;
    int ss_own_k = 0;
    srt_camera ss_own_cam{};
    uint64_t ss_own_scene = 0;
    std::vector<bool> ss_own_rows;
    uint64_t scene_changes = 0;  // srt_set_scene / srt_update_scene / srt_set_meshes calls so far
    // the resolve's result (srt_antialias)
    DeviceBuffer<float4> d_aa_own;
    srt::OutputSlot aa;

    // variance estimate and variance-guided denoiser (srt_variance, srt_temporal_variance, srt_denoise_variance).  The second half
    // render is an input: its own buffer is allocated by the first srt_device_half and nothing records a write.  The variance:
    // besides the slot, whether a call has written the OWN buffer and whether that one used SRT_VARIANCE_ALBEDO
    // (srt_denoise_variance refuses an own buffer of the other kind).
    DeviceBuffer<float4> d_half_own;
    srt::OutputSlot half;
    DeviceBuffer<float> d_var_own;
    srt::OutputSlot var;
    bool var_own_written = false;
    bool var_own_albedo = false;

    // luminance moments of the temporal history (srt_moments_output, srt_temporal_variance): whether the output is on and
    // with which flags; two slots of W*H float4 records (allocated on first use) that flip with d_tp, so d_mom[tp_cur] is what
    // the last srt_temporal_accumulate wrote; whether that call wrote it at all (srt_read_moments, srt_temporal_variance), with
    // which flags and which n; and whether the next call may blend with it (dropped when the output is switched or its flags
    // change, and by a call that ran with the output off).
    bool mom_on = false;
    uint32_t mom_flags = 0;
    DeviceBuffer<float4> d_mom[2];
    bool mom_written = false;
    uint32_t mom_written_flags = 0;
    float mom_samples = 0.0f;
    bool mom_history = false;

    // ray queries (srt_trace_rays): the handle's own ray arrays (srt_write_rays; they grow on demand) and output buffers, one
    // per output bit (grown when a batch needs more) with its slot (the bound buffer only), and the host-side state
    // (srt_rays_host.h): which arrays are the current rays (d_ray_origin is the own array of rays.origins) and what the last
    // trace wrote (rays.last)
    DeviceBuffer<float4> d_ray_origin;
    DeviceBuffer<float4> d_ray_direction;
    DeviceBuffer<void> d_rayout_own[srt::RAYS_SLOTS];
    srt::OutputSlot rayout[srt::RAYS_SLOTS];
    srt::RaysState rays;
    // any-hit queries (srt_trace_occlusion): the call record (whether the last one counted its work), and the record its kernel
    // adds to
    srt::CallRecord occlusion;
    WorkBuffer<srt::OCC_WORK_N> d_occlusion_work;
    // per-pixel visibility (srt_render_visibility), one own buffer of W*H floats per SRT_VIS_* bit with its slot (the bound
    // buffer only); what the last call wrote and whether it counted (srt_visibility_host.h); the record a counting launch adds to
    DeviceBuffer<void> d_vis_own[srt::VIS_SLOTS];
    srt::OutputSlot vis[srt::VIS_SLOTS];
    srt::VisibilityState visibility;
    WorkBuffer<srt::VIS_WORK_N> d_visibility_work;
    // reflection guides (srt_render_reflection_gbuffer): one own buffer of W*H elements per SRT_REFL_* bit with its slot, the call
    // record (whether the last call counted), and the record a counting launch adds to
    DeviceBuffer<void> d_refl_own[srt::REFL_SLOTS];
    srt::ReflectionSlots refl;
    srt::CallRecord reflection;
    WorkBuffer<srt::REFL_WORK_N> d_reflection_work;
    // the camera each own reflection slot was last rendered with, as gbuf_own_cam (srt_temporal_accumulate with the mirror history
    // on refuses own reflection outputs of another camera), and the mirror history's setting (srt_mirror_history_host.h)
    srt_camera refl_own_cam[srt::REFL_SLOTS] = {};
    bool refl_own_cam_set[srt::REFL_SLOTS] = {false, false, false, false, false};
    srt::MirrorHistoryState mirror;
    // radiance queries (srt_trace_radiance): the own output buffer of N float4 (grown when a batch needs more) with its slot (the
    // bound buffer only); what the last trace wrote and whether it counted (srt_radiance_host.h); the sample scratch of the
    // launch's grid (grown when a launch has more workgroups); the record a counting launch adds to
    DeviceBuffer<float4> d_radiance_own;
    srt::OutputSlot radiance_out;
    srt::RadianceState radiance;
    DeviceBuffer<float4> d_radiance_rows;
    WorkBuffer<srt::RAD_WORK_N> d_radiance_work;
    // light probes (srt_trace_light_probes): the own position and direction arrays (srt_write_light_probes,
    // srt_write_light_probe_directions; they grow on demand); one own output buffer per SRT_LIGHT_PROBE_* output bit (grown when
    // a call needs more) with its slot (the bound buffer only); which arrays are current, what the last trace wrote and whether
    // it counted (srt_light_probes_host.h); the block sums of a projection over more than one block of 64 directions; the record
    // a counting launch adds to.  The sample scratch is the radiance pass's, d_radiance_rows.
    DeviceBuffer<float4> d_probe_position;
    DeviceBuffer<float4> d_probe_direction;
    DeviceBuffer<float4> d_probe_out_own[srt::LIGHT_PROBE_SLOTS];
    srt::OutputSlot probe_out[srt::LIGHT_PROBE_SLOTS];
    srt::LightProbeState probes;
    DeviceBuffer<float4> d_probe_partial;
    WorkBuffer<srt::LP_WORK_N> d_probe_work;
    // probe-grid shading (srt_shade_probe_grid): the grid, which coefficient array is current and whether the last call counted
    // (srt_probe_grid_host.h); the own coefficient array (srt_write_probe_grid_coefficients; it grows on demand); the own output
    // buffer of W*H float4 with its slot; the record a counting launch adds to
    srt::ProbeGridState probe_grid;
    DeviceBuffer<float4> d_probe_grid_coefficients;
    DeviceBuffer<float4> d_probe_grid_own;
    srt::OutputSlot probe_grid_out;
    WorkBuffer<srt::PG_WORK_N> d_probe_grid_work;
    // probe depth moments (srt_trace_probe_depth): the three texel tables (uploaded once, on first use); one own output buffer per
    // SRT_PROBE_DEPTH_* output bit (grown when a call needs more) with its slot (the bound buffer only); what the last trace wrote
    // and whether it counted (srt_probe_depth_host.h); the record a counting launch adds to.  The filtered
    // shading (srt_shade_probe_grid_depth): which moment array is current, and the own one (srt_write_probe_grid_depth).
    DeviceBuffer<float4> d_probe_depth_texels;
    bool probe_depth_texels_ready = false;
    DeviceBuffer<void> d_probe_depth_own[srt::PROBE_DEPTH_SLOTS];
    srt::OutputSlot probe_depth_out[srt::PROBE_DEPTH_SLOTS];
    srt::ProbeDepthState probe_depth;
    WorkBuffer<srt::PD_WORK_N> d_probe_depth_work;
    srt::ProbeGridDepthState probe_grid_depth;
    DeviceBuffer<float4> d_probe_grid_depth;
    // probe classification and relocation (srt_classify_probes): the primitive table the kernel reads, built from the object list at
    // the first classification after the scene changed (scene_changes says when); one own output buffer per SRT_PROBE_STATE_* output
    // bit with its slot (the bound buffer only); what the last classification wrote, whether it counted and which state array
    // srt_shade_probe_grid_states reads (srt_probe_states_host.h); the own state array (srt_write_probe_grid_states); the record a
    // counting launch adds to.
    srt::ProbeTable probe_table;
    DeviceBuffer<float4> d_probe_table;
    bool probe_table_ready = false;
    unsigned long long probe_table_scene = 0;
    DeviceBuffer<void> d_probe_states_own[srt::PROBE_STATE_SLOTS];
    srt::OutputSlot probe_states_out[srt::PROBE_STATE_SLOTS];
    srt::ProbeStatesState probe_states;
    DeviceBuffer<float4> d_probe_grid_states;
    WorkBuffer<srt::PS_WORK_N> d_probe_classify_work;
    // per-frame probe updates (srt_list_probes, the listed traces, srt_blend_probes): the rules' state (srt_probe_update_host.h:
    // what the last listing wrote, which list is bound for tracing, the previous records, which P and R the histories stand for);
    // the own list output, the own list input (srt_write_probe_list), the own previous records, the two own histories; the records
    // the counting launches of the listing and of the blend add to.
    srt::ProbeUpdateState probe_update;
    DeviceBuffer<uint32_t> d_probe_list_out;
    DeviceBuffer<uint32_t> d_probe_list;
    DeviceBuffer<float4> d_probe_previous_states;
    DeviceBuffer<float4> d_probe_history[srt::PROBE_HISTORY_SLOTS];
    WorkBuffer<srt::PL_WORK_N> d_probe_list_work;
    WorkBuffer<srt::PB_WORK_N> d_probe_blend_work;
    // scrolling (srt_scroll_probes): the call record (whether the last call counted); one spare per history, the buffer a
    // scroll writes (an own history swaps with it, a bound one is copied back from it); the record a counting launch adds to.
    // The scrolled records go to d_probe_previous_states.
    srt::CallRecord probe_scroll;
    DeviceBuffer<float4> d_probe_history_spare[srt::PROBE_HISTORY_SLOTS];
    WorkBuffer<srt::PSC_WORK_N> d_probe_scroll_work;
    // the probe cascade (srt_shade_probe_cascade): the cascade, which array of each level is current and whether the last call
    // counted (srt_probe_cascade_host.h); the own arrays per level (coefficients, moments, records; they grow on demand); the record
    // a counting launch adds to.  The output is the probe-grid slot's.
    srt::ProbeCascadeState probe_cascade;
    DeviceBuffer<float4> d_probe_cascade[srt::PROBE_CASCADE_MAX_LEVELS][srt::PROBE_CASCADE_ARRAYS];
    WorkBuffer<srt::PC_WORK_N> d_probe_cascade_work;
    // the probe tail (srt_probe_tail): the mode's setting and whether the last affected trace ran under it and counted
    // (srt_probe_tail_host.h); the record a counting launch adds to
    srt::ProbeTailState probe_tail;
    WorkBuffer<srt::PT_WORK_N> d_probe_tail_work;
    // adaptive sampling (srt_render_adaptive, srt_sample_budget): the per-pixel sample counts and sample budget, W*H uint32 each,
    // own buffer and slot; whether the last adaptive render counted and whether a budget pass has run (srt_adaptive_host.h); the
    // tile ticket of a launch (zeroed on the stream in front of it); the record a counting launch adds to;
    // the budget pass's total (one word).  The sample scratch is the radiance pass's, d_radiance_rows: one stream runs both.
    DeviceBuffer<uint32_t> d_counts_own;
    srt::OutputSlot counts;
    DeviceBuffer<uint32_t> d_budget_own;
    srt::OutputSlot budget;
    srt::AdaptiveState adaptive;
    DeviceBuffer<uint32_t> d_adaptive_ticket;
    WorkBuffer<srt::ADP_WORK_N> d_adaptive_work;
    WorkBuffer<1> d_budget_total;

    char error[512] = "";
};

namespace {

int fail(srt_context* ctx, int code, const char* fmt, ...) {
    char* dst = ctx ? ctx->error : g_create_error;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
    return code;
}

#define SRT_HIP(ctx, call)                                                                       \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(ctx, e_ == hipErrorOutOfMemory ? SRT_ERR_OOM : SRT_ERR_HIP, "%s: %s", #call, \
                        hipGetErrorString(e_));                                                  \
    } while (0)

float clamp0h(float v) { return v < 0 ? 0.0f : v; }

// the context's device made current and everything enqueued on its stream finished
int finish_stream(srt_context* ctx) {
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    SRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SRT_OK;
}

// the buffer an output lives in: the caller's bound one, else the handle's own (NULL before its first use)
template <class T>
T* current(const srt::OutputSlot& s, const DeviceBuffer<T>& own) {
    return (T*)const_cast<void*>(s.current((T*)own));
}

// dst = the buffer a call writes `nbytes` of an output to: the bound one, else the own one, allocated or grown first when it is too
// small (a grown buffer takes the record of a last write into it along).  A macro, so that the text of a failed allocation names
// the buffer.  _AFTER: `before_grow` (an int, SRT_OK to go on) runs in front of a re-allocation.
#define SRT_WRITE_TARGET_AFTER(ctx, slot, own, nbytes, dst, before_grow) \
    do {                                                                 \
        if ((slot).target((own).bytes(), nbytes).grow) {                 \
            if (const int rc_ = (before_grow)) return rc_;               \
            (slot).own_released(own);                                    \
            SRT_HIP(ctx, own.ensure(nbytes));                            \
        }                                                                \
        dst = current(slot, own);                                        \
    } while (0)
#define SRT_WRITE_TARGET(ctx, slot, own, nbytes, dst) SRT_WRITE_TARGET_AFTER(ctx, slot, own, nbytes, dst, SRT_OK)

// ... in front of the re-allocation of the own buffer, at `own`, of output `i` of a ray, radiance or probe call: earlier calls
// may still be writing it, so the stream is finished, and the last call's copy of the output goes with it
template <int N>
int output_released(srt_context* ctx, srt::LastOutputs<N>& last, int i, const void* own) {
    if (const int rc = finish_stream(ctx)) return rc;
    last.released(i, own);
    return SRT_OK;
}

// Every srt_write_* of a probe input, its range checked by the caller: `count` elements of `elem_bytes` into the own array, which
// becomes the current one (a state that keeps more than the count does so after this returns SRT_OK)
template <class T>
int write_probe_input(srt_context* ctx, srt::InputArray& in, DeviceBuffer<T>& own, const void* src, size_t count, size_t elem_bytes) {
    if (const int rc = finish_stream(ctx)) return rc;  // (launches in flight read the own array; it may be re-allocated below)
    const size_t bytes = count * elem_bytes;
    if (own.bytes() < bytes) {
        in.own_count = 0;  // (a failed allocation leaves no own array)
        SRT_HIP(ctx, own.ensure(bytes));
    }
    SRT_HIP(ctx, hipMemcpy(own, src, bytes, hipMemcpyHostToDevice));
    srt::input_written(in, count);
    return SRT_OK;
}

// The tail of every srt_read_*: `src` is what the output's read rule gave (NULL: refused with `why`, which may print `output`).
int read_slot(srt_context* ctx, const void* src, void* dst, size_t bytes, const char* why, uint32_t output = 0) {
    if (!src) return fail(ctx, SRT_ERR_STATE, why, output);
    if (const int rc = finish_stream(ctx)) return rc;
    SRT_HIP(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return SRT_OK;
}

// srt_bind_*_output of a pass with several outputs: `slot` is the pass's slot of `output`, -1 when it is not a single output bit
// (refused with `not_a_bit`, which prints `output`).  No synchronisation: enqueued launches keep the buffer they were given.
int bind_output(srt_context* ctx, srt::OutputSlot* slots, int slot, void* d_ptr, const char* not_a_bit, uint32_t output) {
    if (slot < 0) return fail(ctx, SRT_ERR_INVALID_ARG, not_a_bit, output);
    return slots[slot].bind(d_ptr), SRT_OK;
}

// The matching srt_read_*_output: `bytes` of what the last call wrote as `output`, or `not_written`.
template <int N>
int read_output(srt_context* ctx, const srt::LastOutputs<N>& last, uint32_t output, int slot, void* dst, size_t bytes, const char* not_a_bit,
                const char* not_written) {
    if (slot < 0) return fail(ctx, SRT_ERR_INVALID_ARG, not_a_bit, output);
    return read_slot(ctx, last.read(output, slot), dst, bytes, not_written, output);
}

// The work record of a counting launch: zeroed on the stream in front of the launch, and read back once the stream has finished.
template <int N>
int zero_work(srt_context* ctx, WorkBuffer<N>& d) {
    if (!d) SRT_HIP(ctx, d.ensure(N * sizeof(unsigned long long)));
    SRT_HIP(ctx, hipMemsetAsync(d, 0, N * sizeof(unsigned long long), ctx->stream));
    return SRT_OK;
}
template <int N>
int read_work(srt_context* ctx, const WorkBuffer<N>& d, unsigned long long* w) {
    if (const int rc = finish_stream(ctx)) return rc;
    SRT_HIP(ctx, hipMemcpy(w, d, N * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return SRT_OK;
}

// Every srt_get_*_work whose public struct is {uint32 valid, reserved; uint64 counters[N]} in the order of the pass's *_WORK_*
// enum (SRT_WORK_LAYOUT in front of each use asserts it): only the record of a last call that counted, else `why`.
template <class Work, int N>
int get_work(srt_context* ctx, const srt::CallRecord& call, const WorkBuffer<N>& d, Work* out, const char* why) {
    static_assert(sizeof(Work) == 8 + 8 * N && sizeof(unsigned long long) == sizeof(uint64_t), "the work struct is not two words and N counters");
    if (call.work() != srt::RAYS_OK) return fail(ctx, SRT_ERR_STATE, "%s", why);
    unsigned long long w[N];
    if (const int rc = read_work(ctx, d, w)) return rc;
    out->valid = 1, out->reserved = 0;
    memcpy((char*)out + 8, w, sizeof w);
    return SRT_OK;
}
#define SRT_WORK_LAYOUT(Work, N, first, FIRST, last, LAST)                                                                               \
    static_assert(sizeof(Work) == 8 + 8 * (N) && offsetof(Work, first) == 8 + 8 * (FIRST) && offsetof(Work, last) == 8 + 8 * (LAST) && \
                      (LAST) == (N)-1,                                                                                                   \
                  #Work " does not list the counters of its enum in the enum's order")

// the array a call reads an input from: the caller's bound one, else the handle's own
template <class T>
const T* current(const srt::InputArray& in, const DeviceBuffer<T>& own) {
    return in.bound ? (const T*)in.bound : (const T*)own;
}

// the list the listed traces and a listed blend read
const uint32_t* current_probe_list(const srt_context* ctx) { return current(ctx->probe_update.list, ctx->d_probe_list); }

size_t frame_pixels(const srt_context* ctx) { return (size_t)ctx->width * (size_t)ctx->height; }

// the full frame in workgroups of 2 x 2 waves, one wave per 8 x 8 tile
dim3 frame_tile_grid(const srt_context* ctx) {
    return dim3((unsigned)((ctx->width + srt::WG_W - 1) / srt::WG_W), (unsigned)((ctx->height + srt::WG_H - 1) / srt::WG_H));
}

}  // namespace

extern "C" {

int srt_abi_version(void) { return SRT_ABI_VERSION; }

int srt_device_count(int* count) {
    if (!count) return SRT_ERR_INVALID_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        *count = 0;
        fail(nullptr, SRT_ERR_NO_DEVICE, "no HIP device (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return SRT_ERR_NO_DEVICE;
    }
    *count = n;
    return SRT_OK;
}

const char* srt_last_error(const srt_context* ctx) { return ctx ? ctx->error : g_create_error; }

int srt_environment_default(srt_environment* env) {
    if (!env) return SRT_ERR_INVALID_ARG;
    // SunDirection = float3(1,-1,-1).Normalized()   (Raytracer.cpp:55,264)
    float len = sqrtf(1.0f * 1.0f + -1.0f * -1.0f + -1.0f * -1.0f);
    env->sun_direction[0] = 1.0f / len;
    env->sun_direction[1] = -1.0f / len;
    env->sun_direction[2] = -1.0f / len;
    // SkyColor = Color(.2,.35,1.0f)*10.0f; HorizonColor = Color(1.0,0.9f,0.5f)*5.0f  (:56-57)
    env->sky_color[0] = clamp0h((float).2 * 10.0f);
    env->sky_color[1] = clamp0h((float).35 * 10.0f);
    env->sky_color[2] = clamp0h(1.0f * 10.0f);
    env->horizon_color[0] = clamp0h((float)1.0 * 5.0f);
    env->horizon_color[1] = clamp0h(0.9f * 5.0f);
    env->horizon_color[2] = clamp0h(0.5f * 5.0f);
    env->ground_color[0] = .08f;  // :58
    env->ground_color[1] = .06f;
    env->ground_color[2] = .03f;
    env->sun_color[0] = env->sun_color[1] = env->sun_color[2] = 500.0f;  // :59
    return SRT_OK;
}

int srt_create(int device, int width, int height, srt_context** out) {
    if (!out) return fail(nullptr, SRT_ERR_INVALID_ARG, "srt_create: out is NULL");
    *out = nullptr;
    if (width <= 0 || height <= 0 || (long long)width * height > 0x7fffffffLL)
        return fail(nullptr, SRT_ERR_INVALID_ARG, "srt_create: bad size %dx%d", width, height);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, SRT_ERR_NO_DEVICE, "srt_create: no HIP device (%s); this library has no CPU fallback",
                    e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(nullptr, SRT_ERR_INVALID_ARG, "srt_create: device %d of %d", device, n);
    srt_context* ctx = new (std::nothrow) srt_context();
    if (!ctx) return fail(nullptr, SRT_ERR_OOM, "srt_create: host allocation failed");
    ctx->device = device;
    ctx->width = width;
    ctx->height = height;
    srt_environment_default(&ctx->env);
    auto bail = [&](hipError_t err, const char* what) {
        int code = fail(nullptr, err == hipErrorOutOfMemory ? SRT_ERR_OOM : SRT_ERR_HIP, "srt_create: %s: %s", what,
                        hipGetErrorString(err));
        srt_destroy(ctx);
        return code;
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return bail(e, "hipSetDevice");
    if ((e = hipStreamCreateWithFlags(&ctx->own_stream.h, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    ctx->stream = ctx->own_stream;
    if ((e = hipEventCreate(&ctx->ev_begin.h)) != hipSuccess) return bail(e, "hipEventCreate");
    if ((e = hipEventCreate(&ctx->ev_end.h)) != hipSuccess) return bail(e, "hipEventCreate");
    const size_t px = (size_t)width * height;
    if ((e = ctx->d_fb_own.ensure(px * sizeof(uint32_t))) != hipSuccess) return bail(e, "hipMalloc framebuffer");
    if ((e = ctx->d_acc_own.ensure(px * sizeof(float4))) != hipSuccess) return bail(e, "hipMalloc accumulator");
    if ((e = ctx->d_rays.ensure(sizeof(unsigned long long))) != hipSuccess) return bail(e, "hipMalloc counter");
    if ((e = ctx->d_pick.ensure(4 * sizeof(int))) != hipSuccess) return bail(e, "hipMalloc pick");
    if ((e = ctx->d_work.ensure(srt::TALLY_ALL * sizeof(unsigned long long))) != hipSuccess) return bail(e, "hipMalloc work counters");
    if ((e = hipMemsetAsync(ctx->d_fb_own, 0, px * sizeof(uint32_t), ctx->stream)) != hipSuccess) return bail(e, "hipMemset");
    if ((e = hipMemsetAsync(ctx->d_acc_own, 0, px * sizeof(float4), ctx->stream)) != hipSuccess) return bail(e, "hipMemset");
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return bail(e, "hipStreamSynchronize");
    ctx->d_fb = ctx->d_fb_own;
    ctx->d_acc = ctx->d_acc_own;
    int lds = 0;
    if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && lds > 0)
        ctx->lds_limit_bytes = lds;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) ctx->cu_count = cus;
    *out = ctx;
    return SRT_OK;
}

int srt_destroy(srt_context* ctx) {
    if (!ctx) return SRT_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    delete ctx;  // (the members free their resources)
    return SRT_OK;
}

// what a scene change does to the mesh image (srt_update_info.path)
enum { MESH_REBUILD = 1, MESH_REFIT = 2, MESH_KEEP = 3 };

// the mesh image's root as the host derives it for a refit (srt::refit_root)
struct RefitRoot {
    float center[3], half[3], bs_radius;
};

// The refit data of the mesh image just built, uploaded behind it (only while the mode is SRT_UPDATE_REFIT).
static int upload_refit_data(srt_context* ctx, size_t count) {
    const srt::MeshImage& I = ctx->mesh_image;
    ctx->h_refit_verts = srt::refit_vertices(ctx->meshes);
    SRT_HIP(ctx, ctx->d_refit_verts.ensure(std::max<size_t>(ctx->h_refit_verts.size(), 1) * sizeof(float4)));
    SRT_HIP(ctx, ctx->d_refit_tri_verts.ensure(I.tri_verts.size() * sizeof(uint32_t)));
    SRT_HIP(ctx, ctx->d_refit_tri_box.ensure((size_t)I.n_tris * 2 * sizeof(float4)));
    SRT_HIP(ctx, ctx->d_refit_node_box.ensure((size_t)I.n_nodes * 2 * sizeof(float4)));
    SRT_HIP(ctx, ctx->d_refit_pos.ensure(std::max<size_t>(count, 1) * sizeof(float4)));
    if (!ctx->h_refit_verts.empty())
        SRT_HIP(ctx, hipMemcpyAsync(ctx->d_refit_verts, ctx->h_refit_verts.data(), ctx->h_refit_verts.size() * sizeof(float4),
                                    hipMemcpyHostToDevice, ctx->stream));
    SRT_HIP(ctx, hipMemcpyAsync(ctx->d_refit_tri_verts, I.tri_verts.data(), I.tri_verts.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                ctx->stream));
    ctx->refit_ready = true;
    return SRT_OK;
}

// The refit itself: the positions, then the triangle kernel and one level kernel per level of the tree, deepest first, all on the
// launch stream.  Nothing is read back; the root box comes from the host (root).
static int enqueue_refit(srt_context* ctx, const srt_object* objects, size_t count, const RefitRoot& root) {
    srt::MeshImage& I = ctx->mesh_image;
    ctx->h_refit_pos.resize(count);
    for (size_t i = 0; i < count; ++i) ctx->h_refit_pos[i] = make_float4(objects[i].position[0], objects[i].position[1], objects[i].position[2], 0.0f);
    SRT_HIP(ctx, hipMemcpyAsync(ctx->d_refit_pos, ctx->h_refit_pos.data(), count * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    srt::RefitLaunch R{};
    R.tris = ctx->d_bvh_tris, R.nodes = ctx->d_bvh_nodes;
    R.tri_verts = ctx->d_refit_tri_verts, R.verts = ctx->d_refit_verts, R.positions = ctx->d_refit_pos;
    R.tri_box = ctx->d_refit_tri_box, R.node_box = ctx->d_refit_node_box;
    R.n_tris = (uint32_t)I.n_tris, R.n_nodes = (uint32_t)I.n_nodes;
    hipLaunchKernelGGL(srt::refit_triangles_kernel, dim3((R.n_tris + srt::REFIT_THREADS - 1) / srt::REFIT_THREADS), dim3(srt::REFIT_THREADS), 0,
                       ctx->stream, R);
    SRT_HIP(ctx, hipGetLastError());
    for (size_t l = I.level_first.size(); l-- > 0;) {
        R.level_first = (uint32_t)I.level_first[l];
        R.level_nodes = (uint32_t)(l + 1 < I.level_first.size() ? I.level_first[l + 1] : I.n_nodes) - R.level_first;
        hipLaunchKernelGGL(srt::refit_level_kernel, dim3((8 * R.level_nodes + srt::REFIT_THREADS - 1) / srt::REFIT_THREADS),
                           dim3(srt::REFIT_THREADS), 0, ctx->stream, R);
        SRT_HIP(ctx, hipGetLastError());
    }
    for (int ax = 0; ax < 3; ++ax) I.center[ax] = root.center[ax], I.half[ax] = root.half[ax];
    I.bs_radius = root.bs_radius;
    return SRT_OK;
}

// EXTENSION: flatten mesh objects into a world-space triangle list + BVH (HBM resident).  The size limits
// of the device encoding (24-bit triangle ids, 26-bit node ids) are checked BEFORE the build and the uploads.
static int rebuild_mesh_image(srt_context* ctx, const char* fn, const srt_object* objects, size_t count) {
    ctx->refit_ready = false;
    {
        unsigned long long total_tris = 0;
        for (size_t i = 0; i < count; ++i)
            if (objects[i].type == SRT_OBJ_MESH) total_tris += ctx->meshes[(size_t)objects[i].mesh].indices.size() / 3;
        if (total_tris >= (1ull << 24))
            return fail(ctx, SRT_ERR_INVALID_ARG, "%s: %llu mesh triangles exceed the limit of 2^24 - 1 per scene", fn, total_tris);
    }
    srt::build_mesh_image(objects, count, ctx->meshes, ctx->layout[0].nsT + ctx->layout[0].nb, ctx->mesh_image);
    // (allocated to size for every scene, not grown)
    ctx->d_bvh_nodes.reset();
    ctx->d_bvh_tris.reset();
    ctx->d_bvh_gidpos.reset();
    ctx->d_refit_verts.reset(), ctx->d_refit_tri_verts.reset(), ctx->d_refit_tri_box.reset(), ctx->d_refit_node_box.reset(), ctx->d_refit_pos.reset();
    ctx->meshes_stale = false;
    if (ctx->mesh_image.n_tris > 0) {
        // strict depth-first traversal (the kernel's last resort) keeps at most 7 entries per level
        if (7 * ctx->mesh_image.max_depth + 80 > srt::MESH_Q)
            return fail(ctx, SRT_ERR_INVALID_ARG, "%s: BVH too deep (%d levels)", fn, ctx->mesh_image.max_depth);
        if (ctx->mesh_image.n_nodes >= (1 << 26) || ctx->mesh_image.n_tris >= (1 << 24))  // (item encoding of the traversal queues)
            return fail(ctx, SRT_ERR_INVALID_ARG, "%s: mesh too large (%d triangles)", fn, ctx->mesh_image.n_tris);
        for (int ax = 0; ax < 3; ++ax)  // keeps cell * slope finite in the kernel's plane distances
            if (!(fabsf(ctx->mesh_image.center[ax]) + ctx->mesh_image.half[ax] <= 1e9f))
                return fail(ctx, SRT_ERR_INVALID_ARG, "%s: mesh coordinates beyond 1e9 are not supported", fn);
        SRT_HIP(ctx, ctx->d_bvh_nodes.ensure(ctx->mesh_image.nodes.size() * sizeof(float4)));
        SRT_HIP(ctx, ctx->d_bvh_tris.ensure(ctx->mesh_image.tris.size() * sizeof(float4)));
        SRT_HIP(ctx, hipMemcpyAsync(ctx->d_bvh_nodes, ctx->mesh_image.nodes.data(), ctx->mesh_image.nodes.size() * sizeof(float4),
                                    hipMemcpyHostToDevice, ctx->stream));
        SRT_HIP(ctx, hipMemcpyAsync(ctx->d_bvh_tris, ctx->mesh_image.tris.data(), ctx->mesh_image.tris.size() * sizeof(float4),
                                    hipMemcpyHostToDevice, ctx->stream));
        SRT_HIP(ctx, ctx->d_bvh_gidpos.ensure(ctx->mesh_image.gidpos.size() * sizeof(int32_t)));
        SRT_HIP(ctx, hipMemcpyAsync(ctx->d_bvh_gidpos, ctx->mesh_image.gidpos.data(), ctx->mesh_image.gidpos.size() * sizeof(int32_t),
                                    hipMemcpyHostToDevice, ctx->stream));
    }
    if (ctx->update_mode == SRT_UPDATE_REFIT && ctx->mesh_image.n_tris > 0) return upload_refit_data(ctx, count);
    return SRT_OK;
}

static int set_scene_impl(srt_context* ctx, const char* fn, const srt_object* objects, size_t count, int mesh_path, const RefitRoot* root) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (count && !objects) return fail(ctx, SRT_ERR_INVALID_ARG, "%s: objects is NULL", fn);
    if (count > 0x3fffffff) return fail(ctx, SRT_ERR_INVALID_ARG, "%s: too many objects", fn);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    for (size_t i = 0; i < count; ++i) {
        int t = objects[i].type;
        if (t != SRT_OBJ_SPHERE && t != SRT_OBJ_BOX && t != SRT_OBJ_NONE && t != SRT_OBJ_MESH)
            return fail(ctx, SRT_ERR_INVALID_ARG, "%s: object %zu has unknown type %d", fn, i, t);
        if (t == SRT_OBJ_MESH && (objects[i].mesh < 0 || (size_t)objects[i].mesh >= ctx->meshes.size()))
            return fail(ctx, SRT_ERR_INVALID_ARG, "%s: object %zu refers to mesh %d but %zu meshes are set (call srt_set_meshes first)", fn,
                        i, objects[i].mesh, ctx->meshes.size());
    }
    // the previous upload may still be in flight from h_scene
    SRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // from here on the context holds no scene until this call completes: a failure below must not leave
    // a half-replaced one (new image, freed BVH) for srt_render to launch on
    ctx->scene_set = false;
    ctx->objects.clear();
    const bool no_cluster = dev_switches().no_cluster;
    bool has_mesh = false;
    for (size_t i = 0; i < count; ++i) has_mesh = has_mesh || objects[i].type == SRT_OBJ_MESH;
    for (int v = 0; v < 2; ++v) {
        // with meshes both images are the same one, so that primitive ids agree with the BVH
        srt::SceneLayout L = srt::build_scene_image(objects, count, (v == 0 || has_mesh) && !no_cluster, ctx->h_scene[v]);
        srt::environment_rows(ctx->env, ctx->h_scene[v].data() + srt::SRT_CONST_ENV_ROW);
        // hit_key packs the list index in 15 bits and the primitive id in 16
        if (count >= 32768 || L.nsT + L.nb + L.nm >= 65536)
            return fail(ctx, SRT_ERR_INVALID_ARG, "%s: %zu objects (%d sphere slots + %d boxes + %d meshes) exceed the 32767-object limit", fn,
                        count, L.nsT, L.nb, L.nm);
        // an image that does not fit into LDS next to the per-wave scratch stays in HBM (slower kernel
        // instantiation, same bits); the pick kernel runs one wave, so it is judged separately.  The LDS instantiations also
        // take the square root of the sphere test in its short form (sqrt_window, srt_kernel.hip.h), which needs every r*r in
        // [2^-72, FLT_MAX]: a scene with a sphere outside that window runs the instantiations that keep the library sqrtf.
        const size_t image_bytes = (size_t)L.total_vec4 * sizeof(float4);
        const size_t mesh_scratch = has_mesh ? (size_t)(srt::WG_MESH_SCRATCH_BYTES) : 0;
        ctx->scene_in_lds[v] = L.radii_in_sqrt_window && image_bytes + (size_t)srt::WG_SCRATCH_BYTES + mesh_scratch <= (size_t)ctx->lds_limit_bytes;
        ctx->pick_in_lds[v] = L.radii_in_sqrt_window && image_bytes + srt::WAVE_SCRATCH_BYTES + srt::MESH_WAVE_BYTES <= (size_t)ctx->lds_limit_bytes;
        SRT_HIP(ctx, ctx->d_scene[v].ensure(ctx->h_scene[v].size() * sizeof(float4)));
        SRT_HIP(ctx, hipMemcpyAsync(ctx->d_scene[v], ctx->h_scene[v].data(), ctx->h_scene[v].size() * sizeof(float4),
                                    hipMemcpyHostToDevice, ctx->stream));
        ctx->layout[v] = L;
    }
    // an update that only moved objects (srt_update_scene under SRT_UPDATE_REFIT) keeps the mesh image or refits it in place
    if (mesh_path == MESH_REFIT) {
        if (const int rc = enqueue_refit(ctx, objects, count, *root)) return rc;
    } else if (mesh_path == MESH_REBUILD) {
        if (const int rc = rebuild_mesh_image(ctx, fn, objects, count)) return rc;
    }
    ctx->objects.assign(objects, objects + count);
    ctx->scene_set = true;
    ctx->order_stale = true;
    ctx->estimate_stale = true;
    ctx->work.clear();  // the recorded block work describes another scene
    // ... and so does a cost copy that may still be in flight, and the dispatch order made from the old scene's costs: both are
    // dropped (the stream was synchronised above, so nothing still writes h_wg_cost), the next launch estimates afresh
    ctx->recording = false;
    ctx->order_gx = ctx->order_gy = 0;
    return SRT_OK;
}

// Host-side allocation failures (std::bad_alloc from the image / BVH builders) must not cross the C boundary.
static int set_scene_guarded(srt_context* ctx, const char* fn, const srt_object* objects, size_t count, int mesh_path = MESH_REBUILD,
                             const RefitRoot* root = nullptr) {
    if (ctx) ++ctx->scene_changes;  // the handle's own sub-samples belong to the old scene
    try {
        return set_scene_impl(ctx, fn, objects, count, mesh_path, root);
    } catch (const std::bad_alloc&) {
        if (ctx) ctx->scene_set = false;
        return fail(ctx, SRT_ERR_OOM, "%s: host allocation failed", fn);
    } catch (const std::exception& e) {
        if (ctx) ctx->scene_set = false;
        return fail(ctx, SRT_ERR_INVALID_ARG, "%s: %s", fn, e.what());
    }
}

// What srt_update_scene does to the mesh image (info.path, info.reason; for a refit also the root the host derives).  Pure host
// work on the old and the new list; the one failure, a refit beyond the coordinate limit, is found here, before anything is
// touched or enqueued.
static int choose_update_path(srt_context* ctx, const srt_object* objects, size_t count, srt_update_info& info, RefitRoot& root) {
    info = srt_update_info{};
    info.path = MESH_REBUILD;
    if (count && !objects) return SRT_OK;  // (refused by the common validation)
    const srt::MeshImage& I = ctx->mesh_image;
    bool same_but_position = true, finite = true, dropped = false;
    for (size_t i = 0; i < count; ++i) {
        const srt_object &a = ctx->objects[i], &b = objects[i];
        constexpr size_t after = offsetof(srt_object, position) + sizeof(a.position);
        if (a.type != b.type || memcmp((const char*)&a + after, (const char*)&b + after, sizeof(srt_object) - after) != 0) same_but_position = false;
        if (a.type != SRT_OBJ_MESH || b.type != SRT_OBJ_MESH) continue;
        for (int ax = 0; ax < 3; ++ax) finite = finite && std::isfinite(a.position[ax]) && std::isfinite(b.position[ax]);
        if (memcmp(a.position, b.position, sizeof(a.position)) != 0) {
            ++info.moved_mesh_objects;
            if (b.mesh >= 0 && (size_t)b.mesh < I.mesh_dropped.size() && I.mesh_dropped[(size_t)b.mesh]) dropped = true;
        }
    }
    if (ctx->update_mode != SRT_UPDATE_REFIT) return info.reason = 1, SRT_OK;
    if (!same_but_position) return info.reason = 2, SRT_OK;
    if (ctx->meshes_stale) return info.reason = 4, SRT_OK;  // (srt_set_meshes since the build: the image is of other geometry)
    if (info.moved_mesh_objects == 0 || I.n_tris == 0) return info.path = MESH_KEEP, SRT_OK;
    if (!ctx->refit_ready) return info.reason = 4, SRT_OK;
    if (!finite || dropped) return info.reason = 3, SRT_OK;
    float lo[3], hi[3];
    if (!srt::refit_root(I, objects, lo, hi, root.center, root.half, root.bs_radius)) return info.reason = 3, SRT_OK;
    for (int ax = 0; ax < 3; ++ax)  // (the limit srt_set_scene applies)
        if (!(fabsf(root.center[ax]) + root.half[ax] <= 1e9f))
            return fail(ctx, SRT_ERR_INVALID_ARG, "srt_update_scene: mesh coordinates beyond 1e9 are not supported");
    info.path = MESH_REFIT;
    info.levels = (int32_t)I.level_first.size();
    info.triangles = (uint32_t)I.n_tris;
    info.nodes = (uint32_t)I.n_nodes;
    return SRT_OK;
}

int srt_set_scene(srt_context* ctx, const srt_object* objects, size_t count) {
    if (ctx) ctx->tp_valid = false;  // the temporal history's object indices and points belong to the old scene
    return set_scene_guarded(ctx, "srt_set_scene", objects, count);
}

// srt_set_scene for a list of the same length that keeps the temporal history: srt_temporal_accumulate compares the new list
// with the one its history was stored for and reprojects every object by its displacement.
int srt_update_scene(srt_context* ctx, const srt_object* objects, size_t count) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (!ctx->scene_set) return fail(ctx, SRT_ERR_STATE, "srt_update_scene: srt_set_scene has not been called");
    if (count != ctx->objects.size())
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_update_scene: %zu objects, the scene has %zu (a list of another length goes through srt_set_scene)",
                    count, ctx->objects.size());
    srt_update_info info{};
    RefitRoot root{};
    if (const int rc = choose_update_path(ctx, objects, count, info, root)) return rc;  // (nothing touched: the previous scene stands)
    const int rc = set_scene_guarded(ctx, "srt_update_scene", objects, count, info.path, &root);
    if (!ctx->scene_set) ctx->tp_valid = false;  // the refused list left no scene: nothing for the history to belong to
    if (rc == SRT_OK) ctx->update_info = info;
    return rc;
}

int srt_update_mode(srt_context* ctx, int mode) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (mode != SRT_UPDATE_REBUILD && mode != SRT_UPDATE_REFIT) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_update_mode: unknown mode %d", mode);
    ctx->update_mode = mode;
    return SRT_OK;
}

int srt_get_update_info(srt_context* ctx, srt_update_info* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    *out = ctx->update_info;
    return SRT_OK;
}

int srt_mesh_image_size(srt_context* ctx, size_t* node_bytes, size_t* triangle_bytes) {
    if (!ctx || !node_bytes || !triangle_bytes) return SRT_ERR_INVALID_ARG;
    if (!ctx->scene_set) return fail(ctx, SRT_ERR_STATE, "srt_mesh_image_size: srt_set_scene has not been called");
    const bool any = ctx->mesh_image.n_tris > 0;
    *node_bytes = any ? (size_t)ctx->mesh_image.n_nodes * srt::NODE_VEC4 * sizeof(float4) : 0;
    *triangle_bytes = any ? (size_t)ctx->mesh_image.n_tris * 3 * sizeof(float4) : 0;
    return SRT_OK;
}

int srt_read_mesh_image(srt_context* ctx, void* nodes, void* triangles) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    size_t nb = 0, tb = 0;
    if (const int rc = srt_mesh_image_size(ctx, &nb, &tb)) return rc;
    if ((nb && !nodes) || (tb && !triangles)) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_read_mesh_image: NULL destination");
    if (const int rc = finish_stream(ctx)) return rc;
    if (nb) SRT_HIP(ctx, hipMemcpy(nodes, ctx->d_bvh_nodes, nb, hipMemcpyDeviceToHost));
    if (tb) SRT_HIP(ctx, hipMemcpy(triangles, ctx->d_bvh_tris, tb, hipMemcpyDeviceToHost));
    return SRT_OK;
}

static int set_meshes_impl(srt_context* ctx, const srt_mesh* meshes, size_t count) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (count && !meshes) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_set_meshes: meshes is NULL");
    std::vector<srt::HostMesh> copy(count);
    for (size_t i = 0; i < count; ++i) {
        const srt_mesh& m = meshes[i];
        if ((m.vertex_count && !m.vertices) || (m.triangle_count && !m.indices))
            return fail(ctx, SRT_ERR_INVALID_ARG, "srt_set_meshes: mesh %zu has NULL arrays", i);
        if (m.triangle_count >= ((size_t)1 << 24))  // the same limit srt_set_scene applies to the scene's total
            return fail(ctx, SRT_ERR_INVALID_ARG, "srt_set_meshes: mesh %zu has %zu triangles, the limit is 2^24 - 1", i, m.triangle_count);
        copy[i].vertices.assign(m.vertices, m.vertices + 3 * m.vertex_count);
        copy[i].indices.assign(m.indices, m.indices + 3 * m.triangle_count);
    }
    ctx->meshes.swap(copy);
    return SRT_OK;
}

int srt_set_meshes(srt_context* ctx, const srt_mesh* meshes, size_t count) {
    if (ctx) ctx->tp_valid = false, ++ctx->scene_changes, ctx->meshes_stale = true;
    try {
        return set_meshes_impl(ctx, meshes, count);
    } catch (const std::bad_alloc&) {
        return fail(ctx, SRT_ERR_OOM, "srt_set_meshes: host allocation failed");
    } catch (const std::exception& e) {
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_set_meshes: %s", e.what());
    }
}

int srt_set_environment(srt_context* ctx, const srt_environment* env) {
    if (!ctx || !env) return SRT_ERR_INVALID_ARG;
    ctx->env = *env;
    ctx->tp_valid = false;  // the lighting changed: the temporal history's colours are another image's
    // the environment lives in the scene image's constants block (srt_scene_image.h): patch the uploaded images in place
    if (ctx->scene_set) {
        SRT_HIP(ctx, hipSetDevice(ctx->device));
        SRT_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (h_scene may still be the source of an upload in flight)
        for (int v = 0; v < 2; ++v) {
            float4* rows = ctx->h_scene[v].data() + srt::SRT_CONST_ENV_ROW;
            srt::environment_rows(ctx->env, rows);
            SRT_HIP(ctx, hipMemcpyAsync(ctx->d_scene[v] + srt::SRT_CONST_ENV_ROW, rows, 4 * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
        }
    }
    return SRT_OK;
}

int srt_set_camera(srt_context* ctx, const srt_camera* camera) {
    if (!ctx || !camera) return SRT_ERR_INVALID_ARG;
    ctx->camera.cam = *camera;
    ctx->camera.set = true;
    // block costs change with the view: the order learned for the previous view stays in use (for a moving camera it is
    // a better guess than a fresh probe estimate) until the next launch has recorded new costs
    ctx->order_stale = true;
    return SRT_OK;
}

int srt_set_stream(srt_context* ctx, void* hip_stream) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (const int rc = finish_stream(ctx)) return rc;
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return SRT_OK;
}

int srt_bind_output(srt_context* ctx, void* d_framebuffer, void* d_accumulator) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    // (no synchronisation, round 4: a launch takes its buffer addresses when it is enqueued, so renders in flight keep writing
    // the buffers they were given and only later calls see the new ones — which is what lets a caller render frame k + 1 into a
    // second framebuffer while frame k is still being copied to the host, bench.py's overlapped read-back)
    ctx->d_fb = d_framebuffer ? (uint32_t*)d_framebuffer : ctx->d_fb_own;
    ctx->d_acc = d_accumulator ? (float4*)d_accumulator : ctx->d_acc_own;
    return SRT_OK;
}

int srt_device_framebuffer(srt_context* ctx, void** d_ptr) {
    if (!ctx || !d_ptr) return SRT_ERR_INVALID_ARG;
    *d_ptr = ctx->d_fb;
    return SRT_OK;
}

int srt_device_accumulator(srt_context* ctx, void** d_ptr) {
    if (!ctx || !d_ptr) return SRT_ERR_INVALID_ARG;
    *d_ptr = ctx->d_acc;
    return SRT_OK;
}

}  // extern "C"

// frame-constant part of GetRayDirection (Raytracer.cpp:107-115): the ray basis right * rd, up * ld, forward * clipDistance
// (srt_render, srt_render_gbuffer and the reprojection of srt_temporal_accumulate fold it the same way)
static void fold_camera(const srt_camera& c, int W, int H, float* right_rd, float* up_ld, float* fwd_clip) {
    const float clipDistance = .01f;
    float aspecRatio = (float)W / (float)H;
    float hFov = (float)(c.fov_degrees * 3.14159265358979323846 / 180.0f);
    float rd = (clipDistance * tanf(hFov / 2.0f)) * aspecRatio;
    float ld = (clipDistance * tanf(hFov / 2.0f));
    for (int i = 0; i < 3; ++i) {
        right_rd[i] = c.right[i] * rd;
        up_ld[i] = c.up[i] * ld;
        fwd_clip[i] = c.forward[i] * clipDistance;
    }
}

struct KernelSetup {
    size_t lds_bytes;  // of a pathtrace_kernel workgroup
    int use;           // tuning variant (srt_debug_set_variant, SRT_KERNEL)
    int img;           // scene image: 0 clustered, 1 plain brute force
};

static KernelSetup fill_kernel_params(srt_context* ctx, const srt_render_params* p, srt::KernelParams& K) {
    const int W = ctx->width, H = ctx->height;
    memset(&K, 0, sizeof K);
    const srt_camera& c = ctx->camera.cam;
    fold_camera(c, W, H, K.right_rd, K.up_ld, K.fwd_clip);
    for (int i = 0; i < 3; ++i) K.cam_pos[i] = c.position[i];
    K.width = W;
    K.height = H;
    K.y0 = H - p->row_end;  // memory rows [rb,re) = scene rows [H-re, H-rb)
    K.rows = p->row_end - p->row_begin;
    K.first_sample = p->first_sample;
    K.sample_count = p->sample_count;
    K.max_bounces = p->max_bounces;
    K.seed = p->seed;
    K.flags = p->flags & (SRT_RENDER_RESET | SRT_RENDER_COUNT_RAYS | SRT_RENDER_PREVIEW);
#ifdef SRT_DEV
    K.flags |= (uint32_t)dev_switches().kernel_flags;  // SRT_KFLAGS: timing experiments, see the kernel
#endif
    K.steps = p->steps > 1 ? p->steps : 1;
    K.stripe_width = p->stripe_width > 0 ? p->stripe_width : 0;
    K.selected = p->selected_object;
    const int use = ctx->variant >= 0 ? ctx->variant : dev_switches().kernel;
    const int img = (use == 2) ? 1 : 0;  // variant 2: plain brute-force image
    K.mesh_defer = use >= 100 && use < 200 ? use - 100 : 12;  // variants 100 + n: mesh phases wait for n rays
    K.mesh_wait = use >= 200 && use < 300 ? use - 200 : 3;   // variants 200 + w: ... for at most w steps
    if (use >= 300 && use < 500) K.mesh_defer = (use - 300) / 10, K.mesh_wait = (use - 300) % 10;  // variants 300 + 10 n + w: both
#ifdef SRT_DEV
    if (use >= 1000 && use < 2000) K.flags |= (uint32_t)(use - 1000) << 8;  // variants 1000 + f: kernel experiment flags f << 8
#endif
    const srt::SceneLayout& SL = ctx->layout[img];
    K.nu4 = SL.nu4;
    K.nu = SL.nu;
    K.nc = SL.nc;
    K.K = SL.K;
    K.nsT = SL.nsT;
    K.nb = SL.nb;
    if (SL.boxes_finite) K.flags |= srt::KF_BOXES_FINITE;
    K.off_bounds = SL.off_bounds;
    K.off_box = SL.off_box;
    K.off_mat = SL.off_mat;
    K.off_bounds2 = SL.off_bounds2;
    for (int i = 0; i < 3; ++i) K.bound_G[i] = SL.G[i];
    K.bound_cmaxp = SL.cmaxp, K.bound_Rgmax2 = SL.Rgmax2, K.bound_aG = SL.aG;
    K.scene_vec4 = SL.total_vec4;
    K.scene = ctx->d_scene[img];
    K.bvh_nodes = ctx->d_bvh_nodes;
    K.bvh_tris = ctx->d_bvh_tris;
    K.bvh_gidpos = ctx->d_bvh_gidpos;
    K.n_tris = ctx->mesh_image.n_tris;
    for (int i = 0; i < 3; ++i) K.mesh_center[i] = ctx->mesh_image.center[i], K.mesh_half[i] = ctx->mesh_image.half[i];
    K.mesh_r1 = (ctx->mesh_image.half[0] + ctx->mesh_image.half[1] + ctx->mesh_image.half[2]) +
                (fabsf(ctx->mesh_image.center[0]) + fabsf(ctx->mesh_image.center[1]) + fabsf(ctx->mesh_image.center[2]));
    K.mesh_bs_radius = ctx->mesh_image.bs_radius;
    K.accumulator = ctx->d_acc;
    K.framebuffer = ctx->d_fb;
    K.ray_counter = ctx->d_rays;

    const size_t lds_bytes = (ctx->scene_in_lds[img] ? (size_t)(SL.total_vec4 > 0 ? SL.total_vec4 : 1) * sizeof(float4) : 0) +
                             srt::WG_SCRATCH_BYTES + (ctx->mesh_image.n_tris > 0 ? srt::WG_MESH_SCRATCH_BYTES : 0);
    return KernelSetup{lds_bytes, use, img};
}

// The scene side of the kernel parameters for memory rows [row_begin, row_end): what the first-hit, ray and visibility passes
// take from the render's — scene image, mesh image, the scene_in_lds judgement and the LDS bytes, the camera as it stands (the ray
// passes do not read it) — with no flag but KF_BOXES_FINITE and none of the render's buffers.
static KernelSetup scene_kernel_params(srt_context* ctx, int row_begin, int row_end, srt::KernelParams& K) {
    srt_render_params p{};
    p.row_begin = row_begin, p.row_end = row_end, p.first_sample = 1, p.sample_count = 1;
    const KernelSetup ks = fill_kernel_params(ctx, &p, K);
    K.flags &= srt::KF_BOXES_FINITE;
    K.accumulator = nullptr, K.framebuffer = nullptr, K.ray_counter = nullptr;
    return ks;
}

// Workgroups of `kernel` the chip keeps resident: LDS and registers decide how many per CU, at most four (one where the
// runtime cannot say).
static long long resident_workgroups(srt_context* ctx, const void* kernel, size_t lds_bytes) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, srt::WG_THREADS, lds_bytes) != hipSuccess || per_cu < 1)
        per_cu = 1, (void)hipGetLastError();
    return (long long)ctx->cu_count * (per_cu > 4 ? 4 : per_cu);
}

// Persistent workgroups: each stages the scene once and its waves stride over 8 x 8 tiles or blocks of 64 rays; about as many
// as are resident, never more than there is work for (srt::persistent_grid).
template <class IO>
static int launch_persistent(srt_context* ctx, void (*kernel)(srt::KernelParams, IO), unsigned wgs, const KernelSetup& ks, const srt::KernelParams& K, const IO& io) {
    hipLaunchKernelGGL(kernel, dim3(wgs), dim3(srt::WG_THREADS), ks.lds_bytes, ctx->stream, K, io);
    SRT_HIP(ctx, hipGetLastError());
    return SRT_OK;
}
// ... of a TAIL instantiation (srt_probe_tail.hip.h): the tail's inputs are a kernel argument of their own
template <class IO>
static int launch_persistent_tail(srt_context* ctx, void (*kernel)(srt::KernelParams, IO, srt::ProbeTailIO), unsigned wgs, const KernelSetup& ks,
                                  const srt::KernelParams& K, const IO& io, const srt::ProbeTailIO& tio) {
    hipLaunchKernelGGL(kernel, dim3(wgs), dim3(srt::WG_THREADS), ks.lds_bytes, ctx->stream, K, io, tio);
    SRT_HIP(ctx, hipGetLastError());
    return SRT_OK;
}
// ... of a SUN instantiation (srt_sun_sampling.hip.h): the frame is a kernel argument of its own
template <class IO>
static int launch_persistent_sun(srt_context* ctx, void (*kernel)(srt::KernelParams, IO, srt::SunIO), unsigned wgs, const KernelSetup& ks,
                                 const srt::KernelParams& K, const IO& io, const srt::SunIO& sio) {
    hipLaunchKernelGGL(kernel, dim3(wgs), dim3(srt::WG_THREADS), ks.lds_bytes, ctx->stream, K, io, sio);
    SRT_HIP(ctx, hipGetLastError());
    return SRT_OK;
}
// ... of an instantiation with both (srt_render_adaptive_tail with SRT_ADAPTIVE_SUN_SAMPLING): two arguments of their own
template <class IO>
static int launch_persistent_tail_sun(srt_context* ctx, void (*kernel)(srt::KernelParams, IO, srt::ProbeTailIO, srt::SunIO), unsigned wgs, const KernelSetup& ks,
                                      const srt::KernelParams& K, const IO& io, const srt::ProbeTailIO& tio, const srt::SunIO& sio) {
    hipLaunchKernelGGL(kernel, dim3(wgs), dim3(srt::WG_THREADS), ks.lds_bytes, ctx->stream, K, io, tio, sio);
    SRT_HIP(ctx, hipGetLastError());
    return SRT_OK;
}
// ... over the tiles of K's band
template <class IO>
static int launch_tiles(srt_context* ctx, void (*kernel)(srt::KernelParams, IO), const KernelSetup& ks, const srt::KernelParams& K, const IO& io) {
    const long long resident = resident_workgroups(ctx, (const void*)kernel, ks.lds_bytes);
    return launch_persistent(ctx, kernel, srt::persistent_grid(srt::band_tiles(K.width, K.rows), srt::OUT_WG_UNITS, resident), ks, K, io);
}
// ... over n rays
template <class IO>
static int launch_rays(srt_context* ctx, void (*kernel)(srt::KernelParams, IO), size_t n, const KernelSetup& ks, const srt::KernelParams& K, const IO& io) {
    return launch_persistent(ctx, kernel, srt::rays_grid(n, srt::OUT_WG_UNITS, resident_workgroups(ctx, (const void*)kernel, ks.lds_bytes)), ks, K, io);
}

// SRT_KERNEL(kernel, b0, b1, ...): the instantiation kernel<b0, b1, ...> of a kernel template whose parameters are all bools, for
// run-time values — the scene image in LDS or in memory, with or without meshes, with or without the work record, and so on.
// Every combination is instantiated.  pick_flags turns one bool after the other into std::true_type / std::false_type.
template <class F>
static auto pick_flags(F f) {
    return f();
}
template <class F, class... Bools>
static auto pick_flags(F f, bool b, Bools... rest) {
    return b ? pick_flags([f](auto... t) { return f(std::true_type{}, t...); }, rest...)
             : pick_flags([f](auto... t) { return f(std::false_type{}, t...); }, rest...);
}
#define SRT_KERNEL(kernel, ...) pick_flags([](auto... flag) { return &kernel<decltype(flag)::value...>; }, __VA_ARGS__)

// What a block costs, from its counts: the weights are wave instructions per trip of the loop counted (a pool step costs its fixed
// part plus the uniform-sphere groups, cluster bounds and boxes every step runs through), fitted on measured band times of
// configs 3 and 5, Scene3, Scene_indirect and config 4's scene (tools/band_fit.py, profiles/r03/band_fit*.txt).  Valid for a probe
// of PROBE_SAMPLES = 32 samples (shorter pools take more steps per sample) and, as relative weights, for a launch's own counts.
struct ProbeWeights {
    // a pool step: its fixed part + what every step runs through per group of four uniform spheres / cluster bound / box / mesh root test
    double step = 700.0, step_ugroup = 70.0, step_cluster = 12.0, step_box = 45.0, step_mesh = 60.0;
    // Round 4: refitted JOINTLY on the 2- / 4- / 8-way splits of configs 3 and 5 AND of Scene3 at 1080p / 512 spp — the held-out
    // scene round 3's weights failed on (mean / slowest 0.80 at N = 8: they had been fitted in a closed loop on configs 3 and 5 only,
    // where the group weight of 760 and the per-tile 5830 stood in for each other; per block a group of exact tests costs a
    // seventh of a step, profiles/r04/shape_fit.txt, and Scene3's rows differ in exactly that).  Scene2, Scene_indirect and config
    // 4's scene at 4K stay held out (profiles/emulated_ranks.json; tools/band_fit.py, profiles/r04/band_fit.txt).
    // Refitted once more at the end of round 4 on the final kernels (a pool step had become ~ 9 % cheaper, the exact rounds cheaper than
    // that; same three workloads, same tool; before: group 134, node_round 27, leaf_trip 200, mesh_phase 64, node_test 62, wave 80,
    // untraced_wave 74): mean / slowest at N = 8 0.941 / 0.934 / 0.933 on the fitted workloads, 0.962 / 0.991 / 0.927 on the held-out ones.
    double group = 220.0;          // four clustered spheres through the exact test for 64 items (with the scatter, shuffles and merge of its round)
    double node_round = 23.0, leaf_trip = 346.0, mesh_phase = 58.0, node_test = 63.0;  // BVH traversal: rounds, triangle trips, phases, child boxes per lane and round
    double wave = 114.0;           // per tile: staging, primary rays, ring — what every sample chunk of a real launch repeats
    double untraced_wave = 94.0;   // a tile with sample-independent pixels folds their colour sample by sample
};
static double probe_step_weight(const srt::KernelParams& K, const ProbeWeights& w) {
    return w.step + w.step_ugroup * ((K.nu + 3) / 4) + w.step_cluster * K.nc + w.step_box * K.nb + (K.n_tris > 0 ? w.step_mesh : 0.0);
}
static double probe_block_cost(const uint32_t* c, const srt::KernelParams& K, const ProbeWeights& w) {
    return probe_step_weight(K, w) * c[srt::TALLY_STEPS] + w.group * c[srt::TALLY_GROUPS] + w.node_round * c[srt::TALLY_NODE_ROUNDS] + w.leaf_trip * c[srt::TALLY_LEAF_TRIPS] +
           w.mesh_phase * c[srt::TALLY_MESH_PHASES] + w.wave * c[srt::TALLY_WAVES] + w.untraced_wave * c[srt::TALLY_UNTRACED_WAVES] + w.node_test * c[srt::TALLY_NODE_TESTS];
}

// A recording launch's cost copy has completed: make the dispatch order of the following launches from the blocks' wave TIMES
// (any order gives the same image) and the launch-shape record from the blocks' WORK (counts: the same in every run).
static int consume_record(srt_context* ctx) {
    ctx->recording = false;
    const size_t n = (size_t)ctx->rec_gx * ctx->rec_gy;
    const uint32_t* const cost = ctx->h_wg_cost;
    if (ctx->order_gx) (void)hipEventSynchronize(ctx->ev_order);  // (long done) the previous upload read h_wg_order
    // linear buckets between the cheapest and the dearest block, expensive first; the counting sort
    // keeps the spatial order inside a bucket
    const int NB = dev_switches().lpt_buckets;
    // a launch whose blocks all cost about the same (5th..95th percentile within 1.5x) keeps the
    // natural order: nothing to gain, and neighbouring blocks stay together
    bool uniform = false;
    {
        std::vector<uint32_t> tmp(cost, cost + n);
        std::nth_element(tmp.begin(), tmp.begin() + n / 20, tmp.end());
        const double p05 = (double)tmp[n / 20];
        std::nth_element(tmp.begin(), tmp.begin() + (n - 1 - n / 20), tmp.end());
        const double p95 = (double)tmp[n - 1 - n / 20];
        uniform = p95 <= 1.5 * p05;
    }
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    for (size_t i = 0; i < n; ++i) lo = cost[i] < lo ? cost[i] : lo, hi = cost[i] > hi ? cost[i] : hi;
    // the launch-shape record: behind the times, the loop counts of every wave (present when the recording launch kept them)
    ctx->work.clear();
    if (ctx->rec_has_work) srt::weigh_record(cost + n, n, ctx->rec_gx, ctx->rec_gy, ctx->rec_step_w, ctx->mesh_image.n_tris > 0, ctx->work);
#ifdef SRT_DEV
    if (getenv("SRT_DEBUG_CHUNKS")) {  // the time-based figures of round 3 next to the counted ones, for calibration
        double tsum = 0.0;
        for (size_t i = 0; i < n; ++i) tsum += (double)cost[i];
        float ms = 0.0f;
        double tfill = 0.0;
        if (ctx->pending_timed && hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end) == hipSuccess && ms > 0.0f)
            tfill = tsum * 1e-5 / ((double)ms * ctx->cu_count * (ctx->mesh_image.n_tris > 0 ? 16.0 : 20.0));
        else
            (void)hipGetLastError();
        const double slots = (double)ctx->cu_count * (ctx->mesh_image.n_tris > 0 ? 3.0 : 4.0);
        fprintf(stderr, "record: %zu blocks grid %u x %u | TIME dearest %u sum %.0f ratio %.3f fill %.3f (%.3f ms) | WORK dearest %.0f sum %.0f ratio %.3f", n, ctx->rec_gx, ctx->rec_gy,
                hi, tsum, tsum > 0 ? hi * slots / tsum : 0.0, tfill, ms, ctx->work.max, ctx->work.sum, ctx->work.sum > 0 ? ctx->work.max * slots / ctx->work.sum : 0.0);
        const int wslots = ctx->cu_count * (ctx->mesh_image.n_tris > 0 ? 4 : 5);
        for (int c : {1, 2, 3, 4, 6, 8}) fprintf(stderr, " fill(%d)=%.3f", c, srt::simulate_fill(ctx->work.blocks, c, wslots));
        fprintf(stderr, "\n");
    }
    if (const char* dump = getenv("SRT_DUMP_RECORD")) {  // development aid (tools/shape_fit.py): the raw record, appended as one binary blob
        if (FILE* f = fopen(dump, "ab")) {
            float ms = 0.0f;
            if (!ctx->pending_timed || hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end) != hipSuccess) ms = 0.0f, (void)hipGetLastError();
            uint32_t ms_bits, sw_bits;
            const float sw = (float)ctx->rec_step_w;
            memcpy(&ms_bits, &ms, 4), memcpy(&sw_bits, &sw, 4);
            const uint32_t head[10] = {0x53525452u, ctx->rec_gx, ctx->rec_gy, (uint32_t)ctx->band_y0, (uint32_t)ctx->band_rows, ms_bits, sw_bits,
                                       (uint32_t)ctx->cu_count, ctx->mesh_image.n_tris > 0 ? 1u : 0u, ctx->rec_has_work ? 1u : 0u};
            fwrite(head, 4, 10, f);
            fwrite(cost, 4, n * REC_WORDS, f);
            fclose(f);
        }
    }
#endif
    const double scale = hi > lo ? (double)(NB - 1) / (double)(hi - lo) : 0.0;
    auto bucket = [&](uint32_t c) { return (NB - 1) - (int)((double)(c - lo) * scale); };
    std::vector<size_t> start((size_t)NB + 1, 0);
    for (size_t i = 0; i < n; ++i) ++start[(size_t)bucket(cost[i]) + 1];
    for (int k = 0; k < NB; ++k) start[(size_t)k + 1] += start[(size_t)k];
    for (size_t i = 0; i < n; ++i) ctx->h_wg_order[start[(size_t)bucket(cost[i])]++] = (uint32_t)i;
    if (uniform)
        for (size_t i = 0; i < n; ++i) ctx->h_wg_order[i] = (uint32_t)i;
    SRT_HIP(ctx, hipMemcpyAsync(ctx->d_wg_order, ctx->h_wg_order, n * 4, hipMemcpyHostToDevice, ctx->stream));
    SRT_HIP(ctx, hipEventRecord(ctx->ev_order, ctx->stream));
    ctx->order_gx = ctx->rec_gx, ctx->order_gy = ctx->rec_gy;
    return SRT_OK;
}

static int check_render_params(srt_context* ctx, const srt_render_params* p) {
    if (!ctx || !p) return SRT_ERR_INVALID_ARG;
    if (!ctx->scene_set) return fail(ctx, SRT_ERR_STATE, "srt_render: srt_set_scene has not been called");
    if (!ctx->camera.set) return fail(ctx, SRT_ERR_STATE, "srt_render: srt_set_camera has not been called");
    if (p->row_begin < 0 || p->row_end > ctx->height || p->row_begin >= p->row_end)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_render: bad row band [%d,%d) for height %d", p->row_begin, p->row_end, ctx->height);
    if (p->first_sample < 1 || p->sample_count < 1 || p->max_bounces < 0)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_render: first_sample/sample_count must be >= 1 and max_bounces >= 0");
    if (p->steps < 0 || p->stripe_width < 0)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_render: steps and stripe_width must be >= 0");
    if (p->sample_count > (1u << 20))
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_render: sample_count is limited to 2^20 per call (render in several calls)");
    if ((uint64_t)p->first_sample + p->sample_count > 0x7fffffffull)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_render: sample index overflows int (ACCUMULATIONFRAMES is an int)");
    return SRT_OK;
}

// The learned dispatch order, a cost copy in flight and the work record of the chunk rule describe ONE row band.  Another
// band of the same height has the same grid but other blocks behind every index: it starts from a fresh estimate, like a new
// scene.  (Found the hard way: a 270-row band of config 5 launched after its neighbour inherited "no sample chunks" and
// ran 46 ms instead of 12.)
// A record in flight is WAITED for (round 3 polled it): the launch after a recording launch always sees the record, whatever the
// host's timing — so which launch of a sequence changes to the recorded shape and order does not vary from run to run.  The
// wait ends when the recording launch does; it happens once per scene / camera / band change (a launch records only then),
// and costs the one enqueue that could have overlapped that launch's tail.
static int enter_band(srt_context* ctx, const srt::KernelParams& K) {
    if (K.y0 != ctx->band_y0 || K.rows != ctx->band_rows) {
        if (ctx->recording) (void)hipEventSynchronize(ctx->ev_cost);  // (nothing may still write h_wg_cost when the next record starts)
        ctx->band_y0 = K.y0, ctx->band_rows = K.rows;
        ctx->order_stale = ctx->estimate_stale = true;
        ctx->work.clear();
        ctx->recording = false;
        ctx->order_gx = ctx->order_gy = 0;
    }
    if (!ctx->recording) return SRT_OK;
    SRT_HIP(ctx, hipEventSynchronize(ctx->ev_cost));
    return consume_record(ctx);
}

// What srt_render's steps decide about its launch.
struct RenderLaunch {
    srt::LaunchShape shape;
    bool bgrid = false;   // progressive blocks: one lane per block
    bool defer = false;   // sample chunks (shape.chunks >= 2)
    bool rows = false;    // one chunk whose sample colours go through rows of the sample buffer (srt::fold_from_rows)
    dim3 grid;
    bool record = false;  // the launch records its blocks' costs
};

// Tile height: with few rows and many samples per pixel (a narrow stripe of a multi-GPU frame) 8-row
// tiles give too few workgroups to fill 256 CUs x 4 resident workgroups and leave nothing to balance
// the tail with; halve the tile (twice the workgroups, same lanes at work in each wave's path pool)
// until there are about four rounds of workgroups.  Results do not depend on the tiling.
// Progressive blocks (steps > 1): when every pixel of a block ends up with a value that one lane can produce — the
// launch starts the frame (all pixels of a block then hold the same running mean) or adds ONE sample (each pixel folds
// the block's colour into its own mean) — the launch's lanes are blocks, not pixels: 1 / steps^2 of the lanes, one
// ray per block, steps^2 pixel stores per lane (Raytracer.cpp:235-248).  Anything else (several samples onto an
// accumulated frame) keeps one lane per pixel with the block's ray traced once per wave tile.
static int plan_launch(srt_context* ctx, const srt_render_params* p, srt::KernelParams& K, const KernelSetup& ks, RenderLaunch& L) {
    const int W = ctx->width;
    L.bgrid = K.steps > 1 && ((K.flags & SRT_RENDER_RESET) || p->sample_count == 1);
    long long grid_w = W, grid_h = K.rows;
    if (L.bgrid) {
        const long long sw = K.stripe_width > 0 ? K.stripe_width : W;
        grid_w = ((W + sw - 1) / sw) * ((sw + K.steps - 1) / K.steps);
        grid_h = (K.y0 + K.rows - 1) / K.steps - K.y0 / K.steps + 1;  // block rows that meet the band (scene rows)
        K.flags |= srt::KF_BLOCK_GRID;
    }
    K.bgrid_w = (int32_t)grid_w, K.bgrid_h = (int32_t)grid_h;
    // Tile height, sample chunks and the taper of the last chunks: srt_launch_shape.h — a pure function of the request, the grid, the
    // CU count and the band's work record (counts, not times; round 3 read the blocks' wave times and the launch's event time, and
    // config 5's rank-4 band flipped between one piece and nine layers).  Same inputs and call history, same shape; unit-tested on
    // the CPU (tests/native/shape_check.cpp).  The one thing outside it: whether the sample buffer can be had.
    srt::ShapeRequest req;
    req.grid_w = grid_w, req.grid_h = grid_h, req.rows = K.rows, req.sample_count = p->sample_count, req.steps = K.steps;
    req.block_grid = L.bgrid, req.mesh = K.n_tris > 0, req.cu_count = ctx->cu_count;
    srt::ShapeOverrides ov;
    ov.tile_h = dev_switches().tile_h, ov.defer = dev_switches().defer, ov.chunk_beta = dev_switches().chunk_beta;
    ov.no_taper = (dev_switches().kernel_flags & 0x400) != 0, ov.fill_min = SRT_FILL_MIN;
#ifdef SRT_DEV
    if (ctx->shape_defer >= -1) ov.defer = ctx->shape_defer;
    if (ctx->shape_no_taper >= 0) ov.no_taper = ctx->shape_no_taper != 0;
#endif
    srt::LaunchShape& shape = L.shape;
    shape = srt::plan_launch_shape(req, &ctx->work, ov);
#ifdef SRT_DEV
    if (getenv("SRT_DEBUG_CHUNKS") && shape.source)
        fprintf(stderr, "chunks: dearest %.0f sum %.0f blocks %lld ratio %.3f fill %.3f -> %d layer(s) of %d\n", ctx->work.max, ctx->work.sum, shape.wg8, shape.ratio, shape.fill, shape.chunks, shape.chunk);
#endif
    const size_t tiles = (size_t)shape.wg8 * srt::WG_TILES_X * srt::WG_TILES_Y;
    if (shape.chunks >= 2) {
        // Costs 1 KiB of HBM per tile and sample; falls back to small tiles when that is not available
        const size_t need = tiles * (size_t)p->sample_count * 64 * sizeof(float4);
        bool ok = need <= ((size_t)96 << 30);  // (a third of the 288 GB; 24 GB until round 3 — the sky half of config 5 at 4K x 1024 spp needs 67)
        if (ok && need > ctx->d_samples.bytes()) {  // growing: take at most a quarter of what is free
            size_t free_b = 0, total_b = 0;
            ok = hipMemGetInfo(&free_b, &total_b) == hipSuccess && need <= (free_b + ctx->d_samples.bytes()) / 4;
        }
        if (ok && (ctx->d_samples.ensure(need) != hipSuccess || ctx->d_tile_masks.ensure(tiles * sizeof(unsigned long long)) != hipSuccess ||
                   ctx->d_tile_chain.ensure(tiles * sizeof(uint32_t)) != hipSuccess))
            ok = false, (void)hipGetLastError();
        if (!ok) srt::shape_without_sample_buffer(shape);  // no room for the sample buffer: small tiles instead
    }
    srt::finish_launch_shape(shape, p->sample_count, ov);
    L.defer = shape.chunks >= 2;
    // One chunk of full tiles: the colours go through rows of the sample buffer and the ring leaves LDS (srt_launch_shape.h,
    // fold_from_rows).  Without the buffer the launch keeps the ring: same bits.
    L.rows = srt::fold_from_rows(shape, req, (p->flags & SRT_RENDER_PREVIEW) != 0, ctx->scene_in_lds[ks.img]);
    if (L.rows && ctx->d_samples.ensure((size_t)srt::rows_bytes(shape, p->sample_count)) != hipSuccess) {
        (void)hipGetLastError();
        L.rows = false;
    }
    K.tile_h = shape.tile_h;
    K.chunk = L.defer ? shape.chunk : 0;
    K.chunk_full = shape.chunk_full;
    K.sample_rows = ctx->d_samples;
    K.tile_masks = ctx->d_tile_masks;
    // chained chunks: a chunk that finds its tile's running mean at its own first sample folds its samples itself (srt_kernel.hip.h,
    // KernelParams.tile_chain); the counts start at zero
    K.tile_chain = L.defer && dev_switches().chain ? (uint32_t*)ctx->d_tile_chain : nullptr;
    K.chunk_layers = shape.chunks;
#ifdef SRT_DEV
    if (ctx->chain_mode == srt::DEV_CHAIN_OFF) K.tile_chain = nullptr;
    K.chain_mode = ctx->chain_mode, K.chain_arg = ctx->chain_arg;
    if (L.defer) {
        ctx->chain_layers = shape.chunks, ctx->chain_chunk = shape.chunk, ctx->chain_chunk_full = shape.chunk_full, ctx->chain_wg_x = (int)shape.wg_x;
        ctx->chain_tiles = tiles;
        ctx->chain_used = K.tile_chain != nullptr;
        ctx->chain_used_mode = ctx->chain_mode, ctx->chain_used_arg = ctx->chain_arg;
    }
#endif
    if (K.tile_chain) SRT_HIP(ctx, hipMemsetAsync(K.tile_chain, 0, tiles * sizeof(uint32_t), ctx->stream));
    L.grid = dim3((unsigned)shape.wg_x, (unsigned)((grid_h + shape.tile_h * srt::WG_TILES_Y - 1) / (shape.tile_h * srt::WG_TILES_Y)), (unsigned)shape.chunks);
    return SRT_OK;
}

// Cost-ordered dispatch.  The hardware starts workgroups in linear order; with the natural order the
// last ones to start are whatever lies at the top of the band, and the chip idles while a few expensive
// blocks finish.  Starting blocks in order of decreasing cost (coarse buckets, so that neighbours stay
// together) removes most of that tail: Scene1 3.39 -> 3.25 ms, config 4 19.7 -> 17.5 ms.  Costs are
// the blocks' wave-cycles in the band's recording launch (the first after a scene, camera or band change), copied back
// asynchronously; the next srt_render of the handle waits for that copy (see enter_band).  Any order gives the same image.
static int plan_cost_order(srt_context* ctx, const srt_render_params* p, srt::KernelParams& K, const KernelSetup& ks, RenderLaunch& L) {
    const size_t nwg = (size_t)L.grid.x * L.grid.y;
    const bool eligible = dev_switches().lpt && !ctx->order_disabled && nwg >= SRT_ORDER_MIN_WG && p->sample_count >= 4 &&
                          !(p->flags & SRT_RENDER_PREVIEW) && !L.bgrid;
    if (!eligible) return SRT_OK;
    if (REC_WORDS * nwg * 4 > ctx->h_wg_cost.bytes()) {
        SRT_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (h_wg_cost may still be the target of a cost copy)
        ctx->order_gx = ctx->order_gy = 0;
        ctx->recording = false;
        // an optimisation must not be able to fail a render: if anything here cannot be had (pinned host
        // memory, for one), the handle simply keeps the natural order from now on
        // (cost buffers: the blocks' wave times, then the loop counts of every wave of every block)
        const bool ok = ctx->d_wg_cost.ensure(REC_WORDS * nwg * 4) == hipSuccess && ctx->d_wg_order.ensure(nwg * 4) == hipSuccess &&
                        ctx->d_wg_est.ensure(2 * nwg * 4) == hipSuccess &&  // raw + smoothed
                        ctx->h_wg_cost.ensure(REC_WORDS * nwg * 4) == hipSuccess && ctx->h_wg_order.ensure(nwg * 4) == hipSuccess &&
                        (ctx->ev_cost || hipEventCreateWithFlags(&ctx->ev_cost.h, hipEventDisableTiming) == hipSuccess) &&
                        (ctx->ev_order || hipEventCreateWithFlags(&ctx->ev_order.h, hipEventDisableTiming) == hipSuccess);
        if (!ok) {
            (void)hipGetLastError();
            ctx->order_disabled = true;
            return SRT_OK;
        }
    }
    // No recorded costs for this frame yet (first launch, or the scene has changed): estimate the blocks'
    // costs on the device — 16 one-sample probe paths per block, block_cost_kernel — and sort them there (order_sort_kernel);
    // both run on the launch stream ahead of the frame, nothing comes back to the host.  Measured with warm clocks:
    // first launch of a frame vs the learned order: config 4 +13 % -> see DESIGN.md, Scene1 +3 %.
    const dim3 grid = L.grid;
    if (dev_switches().host_order && (ctx->estimate_stale || ctx->order_gx != grid.x || ctx->order_gy != grid.y)) {
        const size_t image_bytes = (size_t)(K.scene_vec4 > 0 ? K.scene_vec4 : 1) * sizeof(float4);
        const size_t est_lds = (ctx->pick_in_lds[ks.img] ? image_bytes : 0) + srt::WAVE_SCRATCH_BYTES + srt::MESH_WAVE_BYTES;
        void (*const estimate)(srt::KernelParams, uint32_t*, int, int) = SRT_KERNEL(srt::block_cost_kernel, ctx->pick_in_lds[ks.img]);
        hipLaunchKernelGGL(estimate, dim3((unsigned)((nwg + 3) / 4)), dim3(64), est_lds, ctx->stream, K, ctx->d_wg_est, (int)grid.x, (int)nwg);
        hipLaunchKernelGGL(srt::smooth_cost_kernel, dim3((unsigned)((nwg + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_wg_est, ctx->d_wg_est + nwg, (int)nwg, (int)grid.x);
        hipLaunchKernelGGL(srt::order_sort_kernel, dim3(1), dim3(srt::ORDER_SORT_THREADS), 0, ctx->stream, ctx->d_wg_est + nwg, ctx->d_wg_order, (int)nwg);
        if (hipGetLastError() == hipSuccess) {
            ctx->order_gx = grid.x, ctx->order_gy = grid.y;
            ctx->estimate_stale = false;
        } else {
            ctx->order_gx = ctx->order_gy = 0;  // an optimisation must not fail the render: natural order
        }
    }
    if (ctx->order_gx == grid.x && ctx->order_gy == grid.y) K.wg_order = ctx->d_wg_order;
    if (ctx->order_stale || ctx->order_gx != grid.x || ctx->order_gy != grid.y) {  // (no record is in flight here: it was waited for in enter_band)
        SRT_HIP(ctx, hipMemsetAsync(ctx->d_wg_cost, 0, REC_WORDS * nwg * 4, ctx->stream));
        K.wg_cost = ctx->d_wg_cost;
        K.wg_blocks = (uint32_t)nwg;
        L.record = true;
    }
    return SRT_OK;
}

// The nine pathtrace_kernel instantiations of one <MIN_WAVES, MESH> pair: scene image in LDS or HBM, full tiles / small tiles
// (multi-sample hand-out) / sample chunks, with or without the loop counts.  All are bit-identical.  Each is named once, by the
// comment that tests/test_gpu_paths.py reads.
template <int MIN_WAVES, bool MESH>
static void launch_pathtrace(bool tally, bool in_lds, bool multi, bool defer, dim3 grid, size_t lds_bytes, hipStream_t stream, const srt::KernelParams& K) {
    using srt::pathtrace_kernel;
    void (*const kernel)(srt::KernelParams) =
        tally && defer    ? pathtrace_kernel<MIN_WAVES, MESH, true, false, true, false, true>   // t_lds_defer
        : tally && multi  ? pathtrace_kernel<MIN_WAVES, MESH, true, true, false, false, true>   // t_lds_multi
        : tally           ? pathtrace_kernel<MIN_WAVES, MESH, true, false, false, false, true>  // t_lds
        : in_lds && defer ? pathtrace_kernel<MIN_WAVES, MESH, true, false, true>                // k_lds_defer
        : in_lds && multi ? pathtrace_kernel<MIN_WAVES, MESH, true, true, false>                // k_lds_multi
        : in_lds          ? pathtrace_kernel<MIN_WAVES, MESH, true, false, false>               // k_lds
        : defer           ? pathtrace_kernel<MIN_WAVES, MESH, false, false, true>               // k_hbm_defer
        : multi           ? pathtrace_kernel<MIN_WAVES, MESH, false, true, false>               // k_hbm_multi
                          : pathtrace_kernel<MIN_WAVES, MESH, false, false, false>;             // k_hbm
    hipLaunchKernelGGL(kernel, grid, dim3(srt::WG_THREADS), lds_bytes, stream, K);
}

// The ROWS instantiations of the analytic scenes — a launch in one chunk of full tiles whose sample colours go through rows of the sample
// buffer (RenderLaunch.rows; the scene image is in LDS) — in place of k_lds / t_lds: the recording and the counting launch keep the
// timed launch's shape.  Their workgroups have no ring in LDS (`lds_bytes` is theirs), and where six of them fit into a CU's LDS
// (srt::rows_six_waves) the timed launch runs at six waves per SIMD: 80 VGPRs, no scratch.  A larger image keeps the five-wave
// kernel (a bound of six would cost it three registers for nothing), and so does the counting instantiation, which would spill at
// six.  Bit-identical to the others: the pool is per wave, and register allocation changes no bit under -ffp-contract=off.
static void launch_pathtrace_rows(bool tally, bool six, dim3 grid, size_t lds_bytes, hipStream_t stream, const srt::KernelParams& K) {
    using srt::pathtrace_kernel;
    void (*const kernel)(srt::KernelParams) =
        tally ? pathtrace_kernel<5, false, true, false, false, false, true, true>     // t_lds_rows
        : six ? pathtrace_kernel<6, false, true, false, false, false, false, true>    // k_lds_rows6
              : pathtrace_kernel<5, false, true, false, false, false, false, true>;   // k_lds_rows
    hipLaunchKernelGGL(kernel, grid, dim3(srt::WG_THREADS), lds_bytes, stream, K);
}

// The TALLY instantiations keep the wave-uniform loop counts (srt_kernel.hip.h, Tally): the recording launch of a band (its
// blocks' work is the launch-shape record) and launches with SRT_RENDER_COUNT_WORK.  Scene images that live in HBM have none
// (a correctness fallback): such launches keep the static shape rule and report no work counts.
// (A recording launch keeps the counts only where the sample-chunk rule could ever read them — launches of the sample counts the
// rule applies to.  A 32-sample analytic frame, config 2, records its blocks' times with the plain instantiation: the counting
// one is 0..2 % slower, bench.py's kernel_ms_counting_launch, and that would be the frame's FIRST launch.)
static int launch_render(srt_context* ctx, const srt_render_params* p, srt::KernelParams& K, const KernelSetup& ks, const RenderLaunch& L) {
    const bool in_lds = ctx->scene_in_lds[ks.img];
    const bool want_work = (p->flags & SRT_RENDER_COUNT_WORK) != 0;
    const bool rule_applies = (p->sample_count >= 64 || K.n_tris > 0) && p->sample_count >= 32 && K.steps <= 1;
    const bool tally = ((L.record && rule_applies) || want_work) && in_lds;
    ctx->count_work = want_work;
    ctx->count_work_valid = want_work && tally;
    if (tally && want_work) {
        SRT_HIP(ctx, hipMemsetAsync(ctx->d_work, 0, srt::TALLY_ALL * sizeof(unsigned long long), ctx->stream));
        K.work_counter = ctx->d_work;
    }
    const bool timing = !(p->flags & SRT_RENDER_NO_TIMING);
    if (timing) SRT_HIP(ctx, hipEventRecord(ctx->ev_begin, ctx->stream));
    // variants 1 / 3 / 5 are a development aid for in-process A/B timing
    const bool multi = L.shape.tile_h < srt::TILE_H || (K.steps > 1 && !(K.flags & SRT_RENDER_PREVIEW)) || L.bgrid;
    if (K.n_tris > 0)  // EXTENSION: scenes with triangle meshes use the BVH-enabled instantiations
        launch_pathtrace<4, true>(tally, in_lds, multi, L.defer, L.grid, ks.lds_bytes, ctx->stream, K);
#ifdef SRT_DEV  // occupancy variants for A/B timing; never in the shipped library
    else if (ks.use == 1 && in_lds && !multi && !L.defer && !tally)
        hipLaunchKernelGGL((srt::pathtrace_kernel<4, false>), L.grid, dim3(srt::WG_THREADS), ks.lds_bytes, ctx->stream, K);
    else if (ks.use == 3 && in_lds && !multi && !L.defer && !tally)
        hipLaunchKernelGGL((srt::pathtrace_kernel<3, false>), L.grid, dim3(srt::WG_THREADS), ks.lds_bytes, ctx->stream, K);
#endif
    else if (L.rows) {  // (one chunk of full tiles of an analytic scene in LDS, never `multi` or L.defer)
        const size_t rows_lds = ks.lds_bytes - (size_t)(srt::WG_SCRATCH_BYTES - srt::WG_SCRATCH_BYTES_ROWS);
        bool six = srt::rows_six_waves(rows_lds);
#ifdef SRT_DEV  // variant 5 keeps the five-wave rows kernel, for A/B timing against the six-wave one inside one library
        if (ks.use == 5) six = false;
#endif
        launch_pathtrace_rows(tally, six, L.grid, rows_lds, ctx->stream, K);
    }
    else
        // (five waves per SIMD, 96 VGPRs.  Since srt_powf's coefficients come from the LDS constants block — the 64-bit literals had
        // been living in hoisted register pairs — the kernels need 85..95 registers, the multi-sample hand-out of small tiles /
        // progressive blocks included (it stayed at four waves before: 111), and the mesh kernels 119..125: four waves, no spill)
        launch_pathtrace<5, false>(tally, in_lds, multi, L.defer, L.grid, ks.lds_bytes, ctx->stream, K);
    if (L.defer) {
        SRT_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(srt::fold_kernel, dim3((unsigned)L.shape.wg8), dim3(256), 0, ctx->stream, K, (int)L.shape.wg_x);
    }
    SRT_HIP(ctx, hipGetLastError());
    if (timing) SRT_HIP(ctx, hipEventRecord(ctx->ev_end, ctx->stream));
    ctx->pending_timed = timing;
    if (L.record) {
        const size_t nwg = (size_t)L.grid.x * L.grid.y;
        SRT_HIP(ctx, hipMemcpyAsync(ctx->h_wg_cost, ctx->d_wg_cost, REC_WORDS * nwg * 4, hipMemcpyDeviceToHost, ctx->stream));
        SRT_HIP(ctx, hipEventRecord(ctx->ev_cost, ctx->stream));
        ctx->recording = true;
        ctx->rec_gx = L.grid.x, ctx->rec_gy = L.grid.y;
        ctx->rec_has_work = tally;  // (a counting launch that also records does keep them)
        ctx->rec_step_w = probe_step_weight(K, ProbeWeights());
        ctx->order_stale = false;
    }
    return SRT_OK;
}

// what srt_get_stats reports for the launch
static void note_pending(srt_context* ctx, const srt_render_params* p, const srt::KernelParams& K, const RenderLaunch& L) {
    ctx->launched = true;
    ctx->stats_pending = true;
    ctx->pending_samples = (uint64_t)ctx->width * (uint64_t)K.rows * p->sample_count;
    ctx->pending_chunks = (uint32_t)L.shape.chunks;
    ctx->pending_tile_rows = (uint32_t)L.shape.tile_h;
    ctx->pending_chunk_samples = L.defer ? (uint32_t)L.shape.chunk : 0u;
    ctx->pending_shape_source = L.shape.source;
    ctx->work_layout[0] = K.nu, ctx->work_layout[1] = K.nc, ctx->work_layout[2] = K.K, ctx->work_layout[3] = K.nb;
}

extern "C" {

int srt_render(srt_context* ctx, const srt_render_params* p) {
    if (const int rc = check_render_params(ctx, p)) return rc;
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    srt::KernelParams K;
    const KernelSetup ks = fill_kernel_params(ctx, p, K);
    ctx->count_rays = (p->flags & SRT_RENDER_COUNT_RAYS) != 0;
    if (ctx->count_rays) SRT_HIP(ctx, hipMemsetAsync(ctx->d_rays, 0, sizeof(unsigned long long), ctx->stream));
    RenderLaunch L;
    if (const int rc = enter_band(ctx, K)) return rc;
    if (const int rc = plan_launch(ctx, p, K, ks, L)) return rc;
    if (const int rc = plan_cost_order(ctx, p, K, ks, L)) return rc;
    if (const int rc = launch_render(ctx, p, K, ks, L)) return rc;
    note_pending(ctx, p, K, L);
    return SRT_OK;
}

#ifdef SRT_DEV
// Development aids (libsrt_pathtrace_dev.so only, not part of the public header): the last pick's raw
// record, and a kernel tuning variant for A/B timing inside one process.  All variants produce identical bits.
int srt_debug_last_pick(srt_context* ctx, int* out4) {
    if (!ctx || !out4) return SRT_ERR_INVALID_ARG;
    memcpy(out4, ctx->last_pick, sizeof ctx->last_pick);
    return SRT_OK;
}

int srt_debug_set_variant(srt_context* ctx, int variant) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    ctx->variant = variant;
    return SRT_OK;
}

// The chained chunks of sample-chunked launches (KernelParams.tile_chain), per handle: mode 0 as shipped, 1 no chain buffer (as
// SRT_CHAIN=0), 2 chunk z may chain only if z < arg, 3 tile t's chain is cut at a layer in [0, layers] drawn from (arg, t)
// (srt::dev_chain_cut).  A cut can only shorten a chain.
int srt_debug_set_chain(srt_context* ctx, int mode, unsigned arg) {
    if (!ctx || mode < srt::DEV_CHAIN_NATURAL || mode > srt::DEV_CHAIN_TILES) return SRT_ERR_INVALID_ARG;
    ctx->chain_mode = mode, ctx->chain_arg = arg;
    return SRT_OK;
}

// Per-handle SRT_DEFER and SRT_KFLAGS & 0x400: defer -1 the rule, 0 never chunk samples, n > 0 n samples per chunk; no_taper 0 / 1.
// defer < -1 and no_taper < 0 go back to the environment.
int srt_debug_set_shape(srt_context* ctx, int defer, int no_taper) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    ctx->shape_defer = defer, ctx->shape_no_taper = no_taper;
    return SRT_OK;
}

// The last sample-chunked launch, once it has finished: every tile's count of chunks folded in order (where fold_kernel took the
// tile up; 0 for every tile without a chain buffer) and the cut srt_debug_set_chain applied to it (0 without a chain buffer).
// info[6]: layers, chunk, chunk_full, tiles, blocks of tiles across, chain buffer or not.  out_at / out_cut may be NULL; otherwise they
// hold n >= tiles entries (tile t = 4 x block + wave, the block's waves 2 x 2 across and down).
int srt_debug_read_chain(srt_context* ctx, uint32_t* out_at, uint32_t* out_cut, size_t n, int* info) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    const size_t tiles = ctx->chain_tiles;
    if ((out_at || out_cut) && n < tiles) return SRT_ERR_INVALID_ARG;
    if (const int rc = finish_stream(ctx)) return rc;
    if (info) {
        info[0] = ctx->chain_layers, info[1] = ctx->chain_chunk, info[2] = ctx->chain_chunk_full;
        info[3] = (int)tiles, info[4] = ctx->chain_wg_x, info[5] = ctx->chain_used ? 1 : 0;
    }
    if (out_at && tiles) {
        if (ctx->chain_used) SRT_HIP(ctx, hipMemcpy(out_at, ctx->d_tile_chain, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost));
        else memset(out_at, 0, tiles * sizeof(uint32_t));
    }
    if (out_cut)
        for (size_t t = 0; t < tiles; ++t)
            out_cut[t] = ctx->chain_used ? srt::dev_chain_cut(ctx->chain_used_mode, ctx->chain_used_arg, (uint32_t)ctx->chain_layers, (uint32_t)t) : 0u;
    return SRT_OK;
}
#endif  // SRT_DEV

#ifdef SRT_STATS
int srt_debug_read_stats(unsigned long long* out8) {
    (void)hipDeviceSynchronize();
#if SRT_STATS == 7 || SRT_STATS == 8  // per-wave rows, summed here
    std::vector<unsigned long long> rows(8 * (size_t)srt::SEG_ROWS);
    hipError_t e = hipMemcpyFromSymbol(rows.data(), HIP_SYMBOL(srt::g_seg), rows.size() * sizeof(unsigned long long));
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    for (size_t r = 0; r < (size_t)srt::SEG_ROWS; ++r)
        for (int i = 0; i < 8; ++i) out8[i] += rows[8 * r + (size_t)i];
    std::fill(rows.begin(), rows.end(), 0ull);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(srt::g_seg), rows.data(), rows.size() * sizeof(unsigned long long));
    return e == hipSuccess ? 0 : 3;
#else
    hipError_t e = hipMemcpyFromSymbol(out8, HIP_SYMBOL(srt::g_stats), 8 * sizeof(unsigned long long));
    unsigned long long z[8] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(srt::g_stats), z, sizeof z);
    return e == hipSuccess ? 0 : 3;
#endif
}
#endif

#if defined(SRT_STATS) && SRT_STATS == 6
int srt_debug_read_wave_log(unsigned long long* out, size_t waves) {
    (void)hipDeviceSynchronize();
    if (waves > (size_t)srt::WAVE_LOG_MAX) waves = srt::WAVE_LOG_MAX;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(srt::g_wave_log), waves * 6 * sizeof(unsigned long long)) == hipSuccess ? 0 : 3;
}
#endif

int srt_pick(srt_context* ctx, int x, int y, int* object_index) {
    if (!ctx || !object_index) return SRT_ERR_INVALID_ARG;
    if (!ctx->scene_set) return fail(ctx, SRT_ERR_STATE, "srt_pick: srt_set_scene has not been called");
    if (!ctx->camera.set) return fail(ctx, SRT_ERR_STATE, "srt_pick: srt_set_camera has not been called");
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    srt_render_params p{};
    p.row_begin = 0;
    p.row_end = ctx->height;
    p.first_sample = 1;
    p.sample_count = 1;
    srt::KernelParams K;
    const int img = fill_kernel_params(ctx, &p, K).img;
    int* d_out = ctx->d_pick;
    // one wave: image (if it fits) + one wave's scratch + one wave's mesh queues
    const size_t image_bytes = (size_t)(K.scene_vec4 > 0 ? K.scene_vec4 : 1) * sizeof(float4);
    const bool in_lds = ctx->pick_in_lds[img];
    hipLaunchKernelGGL(SRT_KERNEL(srt::pick_kernel, in_lds), dim3(1), dim3(64),
                       (in_lds ? image_bytes : 0) + srt::WAVE_SCRATCH_BYTES + srt::MESH_WAVE_BYTES, ctx->stream, K, x, y, d_out);
    SRT_HIP(ctx, hipGetLastError());
    int idx[4] = {-1, 0, 0, 0};
    SRT_HIP(ctx, hipMemcpyAsync(idx, d_out, sizeof idx, hipMemcpyDeviceToHost, ctx->stream));
    SRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *object_index = idx[0];
    memcpy(ctx->last_pick, idx, sizeof idx);
    return SRT_OK;
}

// ---- first-hit buffers --------------------------------------------------------------------------------------------
// slot of a single SRT_GBUF_* bit, -1 for anything else
static int gbuf_slot(uint32_t output) {
    switch (output) {
        case SRT_GBUF_OBJECT: return 0;
        case SRT_GBUF_NORMAL_DEPTH: return 1;
        case SRT_GBUF_POSITION: return 2;
        case SRT_GBUF_ALBEDO: return 3;
        default: return -1;
    }
}
static size_t gbuf_elem_bytes(int slot) { return slot == 0 ? sizeof(int32_t) : sizeof(float4); }

static bool same_camera(const srt_camera& a, const srt_camera& b) {
    for (int i = 0; i < 3; ++i)
        if (a.position[i] != b.position[i] || a.right[i] != b.right[i] || a.up[i] != b.up[i] || a.forward[i] != b.forward[i]) return false;
    return a.fov_degrees == b.fov_degrees;
}

// The first-hit guides [0, n) of a pass (srt_denoise, srt_temporal_accumulate), bound or own; SRT_ERR_STATE for the first that is
// missing or, given a camera, is an own one rendered with another camera (bound ones cannot be checked).
static int find_guides(srt_context* ctx, const char* fn, int n, const srt_camera* cam, const void** guide) {
    static const char* const names[4] = {"OBJECT", "NORMAL_DEPTH", "POSITION", "ALBEDO"};
    for (int i = 0; i < n; ++i) {
        guide[i] = current(ctx->gbuf[i], ctx->d_gbuf_own[i]);
        if (!guide[i]) return fail(ctx, SRT_ERR_STATE, "%s: the %s guide has neither been bound nor rendered (srt_render_gbuffer)", fn, names[i]);
        if (cam && !ctx->gbuf[i].bound && (!ctx->gbuf_own_cam_set[i] || !same_camera(ctx->gbuf_own_cam[i], *cam)))
            return fail(ctx, SRT_ERR_STATE, "%s: the %s guide was rendered with another camera (srt_render_gbuffer after srt_set_camera)", fn, names[i]);
    }
    return SRT_OK;
}

int srt_render_gbuffer(srt_context* ctx, const srt_gbuffer_params* g) {
    if (!ctx || !g) return SRT_ERR_INVALID_ARG;
    if (!ctx->scene_set) return fail(ctx, SRT_ERR_STATE, "srt_render_gbuffer: srt_set_scene has not been called");
    if (!ctx->camera.set) return fail(ctx, SRT_ERR_STATE, "srt_render_gbuffer: srt_set_camera has not been called");
    const int H = ctx->height;
    if (g->row_begin < 0 || g->row_end > H || g->row_begin >= g->row_end)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_render_gbuffer: bad row band [%d,%d) for height %d", g->row_begin, g->row_end, H);
    if (g->outputs == 0 || (g->outputs & ~SRT_GBUF_ALL))
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_render_gbuffer: outputs 0x%x: want a non-empty set of SRT_GBUF_* bits", g->outputs);
    if (g->flags != 0) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_render_gbuffer: flags must be 0");
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t px = frame_pixels(ctx);
    void* dst[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 4; ++i) {
        if (!(g->outputs & (1u << i))) continue;
        SRT_WRITE_TARGET(ctx, ctx->gbuf[i], ctx->d_gbuf_own[i], px * gbuf_elem_bytes(i), dst[i]);
        if (!ctx->gbuf[i].bound) ctx->gbuf_own_cam[i] = ctx->camera.cam, ctx->gbuf_own_cam_set[i] = true;
    }
    srt::KernelParams K;
    const KernelSetup ks = scene_kernel_params(ctx, g->row_begin, g->row_end, K);
    const srt::GBufferOut out{(int32_t*)dst[0], (float4*)dst[1], (float4*)dst[2], (float4*)dst[3]};
    return launch_tiles(ctx, SRT_KERNEL(srt::gbuffer_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0), ks, K, out);
}

int srt_bind_gbuffer(srt_context* ctx, uint32_t output, void* d_ptr) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return bind_output(ctx, ctx->gbuf, gbuf_slot(output), d_ptr, "srt_bind_gbuffer: output 0x%x is not a single SRT_GBUF_* bit", output);
}

int srt_read_gbuffer(srt_context* ctx, uint32_t output, void* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    const int i = gbuf_slot(output);
    if (i < 0) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_read_gbuffer: output 0x%x is not a single SRT_GBUF_* bit", output);
    return read_slot(ctx, current(ctx->gbuf[i], ctx->d_gbuf_own[i]), dst, frame_pixels(ctx) * gbuf_elem_bytes(i),
                     "srt_read_gbuffer: output 0x%x has neither been bound nor rendered", output);
}

// ---- ray queries ---------------------------------------------------------------------------------------------------
static_assert(SRT_GBUF_OBJECT == srt::RAYS_OUT_OBJECT && SRT_GBUF_NORMAL_DEPTH == srt::RAYS_OUT_NORMAL_DEPTH && SRT_GBUF_POSITION == srt::RAYS_OUT_POSITION &&
              SRT_GBUF_ALBEDO == srt::RAYS_OUT_ALBEDO && SRT_RAYS_OCCLUDED == srt::RAYS_OUT_OCCLUDED && SRT_RAYS_NORMALIZE == srt::RAYS_FLAG_NORMALIZE &&
              (int)SRT_OK == (int)srt::RAYS_OK && (int)SRT_ERR_INVALID_ARG == (int)srt::RAYS_INVALID_ARG && (int)SRT_ERR_STATE == (int)srt::RAYS_STATE,
              "srt_rays_host.h and srt_pathtrace.h disagree");

int srt_trace_params_default(srt_trace_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    out->outputs = SRT_GBUF_ALL | SRT_RAYS_OCCLUDED;
    out->flags = 0;
    return SRT_OK;
}

int srt_write_rays(srt_context* ctx, const float* origins, const float* directions, size_t count) {
    if (!ctx || !origins || !directions) return SRT_ERR_INVALID_ARG;
    if (!srt::rays_count_ok(count)) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_write_rays: %zu rays: want 1 .. 2^30", count);
    if (const int rc = finish_stream(ctx)) return rc;  // (traces in flight read the own arrays; they may be re-allocated below)
    const size_t bytes = count * sizeof(float4);
    if (ctx->d_ray_origin.bytes() < bytes || ctx->d_ray_direction.bytes() < bytes) {
        ctx->rays.origins.own_count = 0;  // (a failed allocation leaves no own rays)
        SRT_HIP(ctx, ctx->d_ray_origin.ensure(bytes));
        SRT_HIP(ctx, ctx->d_ray_direction.ensure(bytes));
    }
    SRT_HIP(ctx, hipMemcpy(ctx->d_ray_origin, origins, bytes, hipMemcpyHostToDevice));
    SRT_HIP(ctx, hipMemcpy(ctx->d_ray_direction, directions, bytes, hipMemcpyHostToDevice));
    srt::rays_written(ctx->rays, count);
    return SRT_OK;
}

int srt_bind_rays(srt_context* ctx, const void* d_origins, const void* d_directions, size_t count) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    // (no synchronisation: enqueued traces keep the arrays they were given, as srt_bind_gbuffer)
    if (srt::rays_bind(ctx->rays, d_origins, d_directions, count) != srt::RAYS_OK)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_bind_rays: want two device arrays and 1 .. 2^30 rays, or NULL, NULL, 0 (got %zu rays)", count);
    return SRT_OK;
}

int srt_bind_ray_output(srt_context* ctx, uint32_t output, void* d_ptr) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return bind_output(ctx, ctx->rayout, srt::rays_slot(output), d_ptr, "srt_bind_ray_output: output 0x%x is not a single SRT_GBUF_* / SRT_RAYS_OCCLUDED bit", output);
}

int srt_trace_rays(srt_context* ctx, const srt_trace_params* t) {
    if (!ctx || !t) return SRT_ERR_INVALID_ARG;
    const char* why = "";
    if (const srt::RaysStatus rs = srt::rays_check_trace(ctx->rays, ctx->scene_set, t->outputs, t->flags, &why))
        return fail(ctx, (int)rs, "srt_trace_rays: %s (outputs 0x%x, flags 0x%x)", why, t->outputs, t->flags);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = ctx->rays.count();
    void* dst[srt::RAYS_SLOTS] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < srt::RAYS_SLOTS; ++i)
        if (t->outputs & (1u << i))
            SRT_WRITE_TARGET_AFTER(ctx, ctx->rayout[i], ctx->d_rayout_own[i], n * srt::rays_elem_bytes(i), dst[i], output_released(ctx, ctx->rays.last, i, ctx->d_rayout_own[i]));
    srt::KernelParams K;
    const KernelSetup ks = scene_kernel_params(ctx, 0, ctx->height, K);
    srt::RaysIO io{};
    io.origin = current(ctx->rays.origins, ctx->d_ray_origin);
    io.direction = ctx->rays.bound() ? (const float4*)ctx->rays.bound_direction : (const float4*)ctx->d_ray_direction;
    io.count = (uint32_t)n;
    io.normalize = (t->flags & SRT_RAYS_NORMALIZE) ? 1u : 0u;
    io.object = (int32_t*)dst[0], io.normal_depth = (float4*)dst[1], io.position = (float4*)dst[2], io.albedo = (float4*)dst[3], io.occluded = (int32_t*)dst[4];
    if (const int rc = launch_rays(ctx, SRT_KERNEL(srt::rays_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0), n, ks, K, io)) return rc;
    srt::rays_traced(ctx->rays, t->outputs, dst);
    return SRT_OK;
}

int srt_read_ray_output(srt_context* ctx, uint32_t output, void* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    const int i = srt::rays_slot(output);
    return read_output(ctx, ctx->rays.last, output, i, dst, ctx->rays.last_count * srt::rays_elem_bytes(i),
                       "srt_read_ray_output: output 0x%x is not a single SRT_GBUF_* / SRT_RAYS_OCCLUDED bit",
                       "srt_read_ray_output: output 0x%x was not written by the last srt_trace_rays");
}

// ---- any-hit queries -----------------------------------------------------------------------------------------------
static_assert(SRT_OCCLUSION_NORMALIZE == srt::OCCLUSION_FLAG_NORMALIZE && SRT_OCCLUSION_COUNT_WORK == srt::OCCLUSION_FLAG_COUNT_WORK &&
              sizeof(srt_occlusion_params) == 8 && sizeof(srt_occlusion_work) == 48,
              "srt_occlusion_host.h and srt_pathtrace.h disagree");

int srt_occlusion_params_default(srt_occlusion_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    out->flags = 0;
    out->reserved = 0;
    return SRT_OK;
}

int srt_trace_occlusion(srt_context* ctx, const srt_occlusion_params* t) {
    if (!ctx || !t) return SRT_ERR_INVALID_ARG;
    const char* why = "";
    if (const srt::RaysStatus rs = srt::occlusion_check_trace(ctx->rays, ctx->scene_set, t->flags, t->reserved, &why))
        return fail(ctx, (int)rs, "srt_trace_occlusion: %s (flags 0x%x, reserved 0x%x)", why, t->flags, t->reserved);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = ctx->rays.count();
    const int slot = srt::OCCLUSION_SLOT;
    const bool count = (t->flags & SRT_OCCLUSION_COUNT_WORK) != 0;
    void* dst = nullptr;
    SRT_WRITE_TARGET_AFTER(ctx, ctx->rayout[slot], ctx->d_rayout_own[slot], n * sizeof(int32_t), dst, output_released(ctx, ctx->rays.last, slot, ctx->d_rayout_own[slot]));
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_occlusion_work)) return rc;
    }
    srt::KernelParams K;
    const KernelSetup ks = scene_kernel_params(ctx, 0, ctx->height, K);
    srt::OcclusionIO io{};
    io.origin = current(ctx->rays.origins, ctx->d_ray_origin);
    io.direction = ctx->rays.bound() ? (const float4*)ctx->rays.bound_direction : (const float4*)ctx->d_ray_direction;
    io.count = (uint32_t)n;
    io.normalize = (t->flags & SRT_OCCLUSION_NORMALIZE) ? 1u : 0u;
    io.occluded = (int32_t*)dst;
    io.work = count ? (unsigned long long*)ctx->d_occlusion_work : nullptr;
    if (const int rc = launch_rays(ctx, SRT_KERNEL(srt::occlusion_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0, count), n, ks, K, io)) return rc;
    srt::occlusion_traced(ctx->rays, ctx->occlusion, dst, t->flags);
    return SRT_OK;
}

SRT_WORK_LAYOUT(srt_occlusion_work, srt::OCC_WORK_N, rays, srt::OCC_WORK_RAYS, triangle_tests, srt::OCC_WORK_TRIANGLES);
int srt_get_occlusion_work(srt_context* ctx, srt_occlusion_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->occlusion, ctx->d_occlusion_work, out,
                    "srt_get_occlusion_work: the last srt_trace_occlusion did not ask for SRT_OCCLUSION_COUNT_WORK (or there has been none)");
}

// ---- per-pixel visibility ------------------------------------------------------------------------------------------
static_assert(SRT_VIS_AO == srt::VIS_OUT_AO && SRT_VIS_SUN == srt::VIS_OUT_SUN && SRT_VIS_COUNT_WORK == srt::VIS_FLAG_COUNT_WORK &&
              sizeof(srt_visibility_params) == 32 && sizeof(srt::VisibilityCall) == 32 && sizeof(srt_visibility_work) == 56,
              "srt_visibility_host.h and srt_pathtrace.h disagree");

int srt_visibility_params_default(srt_visibility_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    out->row_begin = 0, out->row_end = 0;
    out->outputs = SRT_VIS_AO | SRT_VIS_SUN;
    out->flags = 0;
    out->ao_samples = 16, out->first_sample = 1, out->seed = 0;
    out->ao_radius = INFINITY;
    return SRT_OK;
}

int srt_render_visibility(srt_context* ctx, const srt_visibility_params* v) {
    if (!ctx || !v) return SRT_ERR_INVALID_ARG;
    const srt::VisibilityCall call{v->row_begin, v->row_end, v->outputs, v->flags, v->ao_samples, v->first_sample, v->seed, v->ao_radius};
    bool present[srt::VIS_GUIDES];
    for (int i = 0; i < srt::VIS_GUIDES; ++i) present[i] = current(ctx->gbuf[i], ctx->d_gbuf_own[i]) != nullptr;
    const char* why = "";
    if (const srt::RaysStatus rs = srt::visibility_check(call, ctx->scene_set, ctx->height, present, &why))
        return fail(ctx, (int)rs, "srt_render_visibility: %s (rows [%d,%d) of %d, outputs 0x%x, flags 0x%x, ao_samples %u, first_sample %u, ao_radius %g)", why,
                    v->row_begin, v->row_end, ctx->height, v->outputs, v->flags, v->ao_samples, v->first_sample, (double)v->ao_radius);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const bool count = (v->flags & SRT_VIS_COUNT_WORK) != 0;
    const size_t px = frame_pixels(ctx);
    void* dst[srt::VIS_SLOTS] = {nullptr, nullptr};
    for (int i = 0; i < srt::VIS_SLOTS; ++i)
        if (v->outputs & (1u << i))
            SRT_WRITE_TARGET(ctx, ctx->vis[i], ctx->d_vis_own[i], px * sizeof(float), dst[i]);
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_visibility_work)) return rc;
    }
    srt::KernelParams K;
    const KernelSetup ks = scene_kernel_params(ctx, v->row_begin, v->row_end, K);
    const bool ao = (v->outputs & SRT_VIS_AO) != 0;
    srt::VisibilityIO io{};
    io.object = (const int32_t*)current(ctx->gbuf[0], ctx->d_gbuf_own[0]);
    io.normal_depth = (const float4*)current(ctx->gbuf[1], ctx->d_gbuf_own[1]);
    io.position = (const float4*)current(ctx->gbuf[2], ctx->d_gbuf_own[2]);
    io.ao = (float*)dst[0], io.sun = (float*)dst[1];
    io.n = ao ? v->ao_samples : 1u, io.first_sample = ao ? v->first_sample : 1u, io.seed = ao ? v->seed : 0u;
    io.radius = ao ? v->ao_radius : INFINITY;
    io.work = count ? (unsigned long long*)ctx->d_visibility_work : nullptr;
    if (const int rc = launch_tiles(ctx, SRT_KERNEL(srt::visibility_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0, count), ks, K, io)) return rc;
    srt::visibility_rendered(ctx->visibility, v->outputs, dst, v->flags);
    return SRT_OK;
}

int srt_bind_visibility(srt_context* ctx, uint32_t output, void* d_float) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return bind_output(ctx, ctx->vis, srt::visibility_slot(output), d_float, "srt_bind_visibility: output 0x%x is not a single SRT_VIS_* bit", output);
}

int srt_read_visibility(srt_context* ctx, uint32_t output, float* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    return read_output(ctx, ctx->visibility.last, output, srt::visibility_slot(output), dst, frame_pixels(ctx) * sizeof(float),
                       "srt_read_visibility: output 0x%x is not a single SRT_VIS_* bit",
                       "srt_read_visibility: the last srt_render_visibility did not write output 0x%x (or there has been none)");
}

SRT_WORK_LAYOUT(srt_visibility_work, srt::VIS_WORK_N, segments, srt::VIS_WORK_SEGMENTS, triangle_tests, srt::VIS_WORK_TRIANGLES);
int srt_get_visibility_work(srt_context* ctx, srt_visibility_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->visibility.call, ctx->d_visibility_work, out,
                    "srt_get_visibility_work: the last srt_render_visibility did not ask for SRT_VIS_COUNT_WORK (or there has been none)");
}

// ---- reflection guides ---------------------------------------------------------------------------------------------
static_assert(SRT_REFL_OBJECT == srt::REFL_OUT_OBJECT && SRT_REFL_NORMAL_DEPTH == srt::REFL_OUT_NORMAL_DEPTH && SRT_REFL_POSITION == srt::REFL_OUT_POSITION &&
              SRT_REFL_ALBEDO == srt::REFL_OUT_ALBEDO && SRT_REFL_BOUNCES == srt::REFL_OUT_BOUNCES && SRT_REFL_GUIDES == srt::REFL_OUT_GUIDES &&
              SRT_REFL_ALL == srt::REFL_OUT_ALL && SRT_REFL_COUNT_WORK == srt::REFL_FLAG_COUNT_WORK && SRT_REFL_GUIDES == SRT_GBUF_ALL &&
              sizeof(srt_reflection_params) == 32 && sizeof(srt::ReflectionCall) == 32 && sizeof(srt_reflection_work) == 40,
              "srt_reflection_host.h and srt_pathtrace.h disagree");

int srt_reflection_params_default(srt_reflection_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    const srt::ReflectionCall c = srt::reflection_defaults();
    out->row_begin = c.row_begin, out->row_end = c.row_end;
    out->outputs = c.outputs, out->flags = c.flags;
    out->max_bounces = c.max_bounces;
    out->min_smoothness = c.min_smoothness, out->min_specular = c.min_specular;
    out->reserved = c.reserved;
    return SRT_OK;
}

int srt_render_reflection_gbuffer(srt_context* ctx, const srt_reflection_params* r) {
    if (!ctx || !r) return SRT_ERR_INVALID_ARG;
    const srt::ReflectionCall call{r->row_begin, r->row_end, r->outputs, r->flags, r->max_bounces, r->min_smoothness, r->min_specular, r->reserved};
    const char* why = "";
    if (const srt::RaysStatus rs = srt::reflection_check(call, ctx->scene_set, ctx->camera.set, ctx->height, &why))
        return fail(ctx, (int)rs, "srt_render_reflection_gbuffer: %s (rows [%d,%d) of %d, outputs 0x%x, flags 0x%x, max_bounces %d, min_smoothness %g, min_specular %g, reserved %u)",
                    why, r->row_begin, r->row_end, ctx->height, r->outputs, r->flags, r->max_bounces, (double)r->min_smoothness, (double)r->min_specular, r->reserved);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const bool count = (r->flags & SRT_REFL_COUNT_WORK) != 0;
    const size_t px = frame_pixels(ctx);
    void* dst[srt::REFL_SLOTS] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < srt::REFL_SLOTS; ++i)
        if (r->outputs & (1u << i))
            SRT_WRITE_TARGET(ctx, ctx->refl.out[i], ctx->d_refl_own[i], px * srt::reflection_elem_bytes(i), dst[i]);
    for (int i = 0; i < srt::REFL_SLOTS; ++i)
        if ((r->outputs & (1u << i)) && !ctx->refl.out[i].bound) ctx->refl_own_cam[i] = ctx->camera.cam, ctx->refl_own_cam_set[i] = true;
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_reflection_work)) return rc;
    }
    srt::KernelParams K;
    const KernelSetup ks = scene_kernel_params(ctx, r->row_begin, r->row_end, K);
    srt::ReflectionIO io{};
    io.object = (int32_t*)dst[0], io.normal_depth = (float4*)dst[1], io.position = (float4*)dst[2], io.albedo = (float4*)dst[3];
    io.bounces = (int32_t*)dst[4];
    io.max_bounces = r->max_bounces, io.min_smoothness = r->min_smoothness, io.min_specular = r->min_specular;
    io.work = count ? (unsigned long long*)ctx->d_reflection_work : nullptr;
    if (const int rc = launch_tiles(ctx, SRT_KERNEL(srt::reflection_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0, count), ks, K, io)) return rc;
    srt::reflection_rendered(ctx->reflection, ctx->refl, r->outputs, dst, r->flags);
    return SRT_OK;
}

int srt_bind_reflection(srt_context* ctx, uint32_t output, void* d_ptr) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return bind_output(ctx, ctx->refl.out, srt::reflection_slot(output), d_ptr, "srt_bind_reflection: output 0x%x is not a single SRT_REFL_* bit", output);
}

int srt_read_reflection(srt_context* ctx, uint32_t output, void* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    const void* own[srt::REFL_SLOTS];
    for (int i = 0; i < srt::REFL_SLOTS; ++i) own[i] = (void*)ctx->d_refl_own[i];
    const void* src = nullptr;
    const srt::RaysStatus rs = srt::reflection_check_read(ctx->refl, output, own, &src);
    if (rs == srt::RAYS_INVALID_ARG) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_read_reflection: output 0x%x is not a single SRT_REFL_* bit", output);
    const int i = srt::reflection_slot(output);
    return read_slot(ctx, rs == srt::RAYS_OK ? src : nullptr, dst, frame_pixels(ctx) * srt::reflection_elem_bytes(i),
                     "srt_read_reflection: output 0x%x has neither been bound nor rendered", output);
}

int srt_device_reflection(srt_context* ctx, uint32_t output, void** d_ptr) {
    if (!ctx || !d_ptr) return SRT_ERR_INVALID_ARG;
    const int i = srt::reflection_slot(output);
    if (i < 0) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_device_reflection: output 0x%x is not a single SRT_REFL_* bit", output);
    if (!(void*)ctx->d_refl_own[i]) {
        SRT_HIP(ctx, hipSetDevice(ctx->device));
        const size_t bytes = frame_pixels(ctx) * srt::reflection_elem_bytes(i);
        SRT_HIP(ctx, ctx->d_refl_own[i].ensure(bytes));
        SRT_HIP(ctx, hipMemsetAsync(ctx->d_refl_own[i], 0, bytes, ctx->stream));  // as srt_device_half's buffer starts
    }
    *d_ptr = (void*)ctx->d_refl_own[i];
    return SRT_OK;
}

SRT_WORK_LAYOUT(srt_reflection_work, srt::REFL_WORK_N, pixels, srt::REFL_WORK_PIXELS, waves, srt::REFL_WORK_WAVES);
int srt_get_reflection_work(srt_context* ctx, srt_reflection_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->reflection, ctx->d_reflection_work, out,
                    "srt_get_reflection_work: the last srt_render_reflection_gbuffer did not ask for SRT_REFL_COUNT_WORK (or there has been none)");
}

// ---- radiance queries ----------------------------------------------------------------------------------------------
static_assert(SRT_RADIANCE_RESET == srt::RADIANCE_FLAG_RESET && SRT_RADIANCE_NORMALIZE == srt::RADIANCE_FLAG_NORMALIZE &&
              SRT_RADIANCE_COUNT_WORK == srt::RADIANCE_FLAG_COUNT_WORK && SRT_RADIANCE_RESET == SRT_RENDER_RESET &&
              sizeof(srt_radiance_params) == 24 && sizeof(srt::RadianceCall) == 24 && sizeof(srt_radiance_work) == 40 &&
              srt::RADIANCE_CHUNK == srt::RAD_CHUNK,
              "srt_radiance_host.h, srt_sample_pool.hip.h and srt_pathtrace.h disagree");

int srt_radiance_params_default(srt_radiance_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt::RadianceCall c;
    srt::radiance_call_default(c);
    out->first_sample = c.first_sample, out->sample_count = c.sample_count, out->max_bounces = c.max_bounces;
    out->seed = c.seed, out->id_base = c.id_base, out->flags = c.flags;
    return SRT_OK;
}

// srt_probe_tail is on and changes this trace: what the mode requires of the grid's inputs, and a coefficient array that is not
// the buffer the call is about to write, `written` (NULL: an own buffer not allocated yet)
static int check_probe_tail(srt_context* ctx, const char* who, const void* written, size_t written_bytes) {
    const char* why = "";
    if (const srt::RaysStatus rs = srt::probe_tail_check_trace(ctx->probe_tail, ctx->probe_grid, ctx->probe_grid_depth, ctx->probe_states,
                                                                current(ctx->probe_grid.coefficients, ctx->d_probe_grid_coefficients), written, written_bytes, &why))
        return fail(ctx, (int)rs, "%s: %s", who, why);
    return SRT_OK;
}

// the record of an affected trace under the mode with SRT_PROBE_TAIL_COUNT_WORK, zeroed on the stream in front of it
static int zero_probe_tail_work(srt_context* ctx) {
    if (!ctx->probe_tail.enabled || !(ctx->probe_tail.call.flags & SRT_PROBE_TAIL_COUNT_WORK)) return SRT_OK;
    return zero_work(ctx, ctx->d_probe_tail_work);
}

// the tail's kernel argument: the grid and the arrays current now, as shade_probe_grid takes them
static srt::ProbeTailIO probe_tail_io(srt_context* ctx) {
    const srt::ProbeTailCall& c = ctx->probe_tail.call;
    const srt::ProbeGrid& g = ctx->probe_grid.grid;
    srt::ProbeTailIO io{};
    io.coefficients = current(ctx->probe_grid.coefficients, ctx->d_probe_grid_coefficients);
    if (c.flags & SRT_PROBE_TAIL_DEPTH) {
        io.depth = current(ctx->probe_grid_depth.moments, ctx->d_probe_grid_depth);
        io.resolution = ctx->probe_grid_depth.resolution();
    }
    if (c.flags & SRT_PROBE_TAIL_STATES) io.states = current(ctx->probe_states.states, ctx->d_probe_grid_states);
    for (int a = 0; a < 3; ++a) io.origin[a] = g.origin[a], io.spacing[a] = g.spacing[a], io.counts[a] = g.counts[a], io.band_weight[a] = c.band_weight[a];
    io.flags = c.flags & (SRT_PROBE_TAIL_NORMAL_WEIGHT | SRT_PROBE_TAIL_DEPTH | SRT_PROBE_TAIL_STATES);
    io.bias = c.bias, io.min_variance = c.min_variance;
    io.work = (c.flags & SRT_PROBE_TAIL_COUNT_WORK) ? (unsigned long long*)ctx->d_probe_tail_work : nullptr;
    return io;
}

// ---- sun sampling (rules S1 - S9; srt_sun_sampling_host.h) -----------------------------------------------------------
static_assert(SRT_RADIANCE_SUN_SAMPLING == srt::SUN_SAMPLING_FLAG && SRT_LIGHT_PROBE_SUN_SAMPLING == srt::SUN_SAMPLING_FLAG &&
                  !(srt::RADIANCE_FLAG_ALL & srt::SUN_SAMPLING_FLAG) && !(srt::LIGHT_PROBE_FLAG_ALL & srt::SUN_SAMPLING_FLAG) &&
                  sizeof(srt::SunFrame) == sizeof(srt::SunIO) && sizeof(srt::SunIO) == 36,
              "srt_sun_sampling_host.h, srt_sun_sampling.hip.h and srt_pathtrace.h disagree");

// the flag's refusals (S5), after the call's own errors and before anything is touched
static int check_sun_sampling(srt_context* ctx, const char* who) {
    const char* why = "";
    if (const srt::RaysStatus rs = srt::sun_sampling_check(ctx->env.sun_direction, ctx->probe_tail.enabled, &why))
        return fail(ctx, (int)rs, "%s: %s (sun_direction %g %g %g)", who, why, ctx->env.sun_direction[0], ctx->env.sun_direction[1], ctx->env.sun_direction[2]);
    return SRT_OK;
}

// the frame of the environment as it stands at the enqueue: a kernel argument, so an enqueued launch keeps it
static srt::SunIO sun_io(srt_context* ctx) {
    srt::SunFrame f;
    srt::sun_frame(ctx->env.sun_direction, f);
    srt::SunIO io;
    for (int a = 0; a < 3; ++a) io.s[a] = f.s[a], io.t1[a] = f.t1[a], io.t2[a] = f.t2[a];
    return io;
}

// The sample scratch of the three sample-pool launches (srt_trace_radiance, srt_trace_light_probes, srt_render_adaptive; one
// stream runs them all): every wave of a grid of `wgs` workgroups has its own region.  Grown once the stream has finished with
// the smaller one.
static int ensure_sample_rows(srt_context* ctx, unsigned wgs) {
    const size_t scratch = srt::radiance_scratch_bytes(wgs, srt::OUT_WG_UNITS);
    if (ctx->d_radiance_rows.bytes() < scratch) {
        if (const int rc = finish_stream(ctx)) return rc;
        SRT_HIP(ctx, ctx->d_radiance_rows.ensure(scratch));
    }
    return SRT_OK;
}

int srt_trace_radiance(srt_context* ctx, const srt_radiance_params* t) {
    if (!ctx || !t) return SRT_ERR_INVALID_ARG;
    const srt::RadianceCall call{t->first_sample, t->sample_count, t->max_bounces, t->seed, t->id_base, t->flags};
    const char* why = "";
    if (const srt::RaysStatus rs = srt::sun_radiance_check_trace(ctx->rays, ctx->scene_set, call, &why))
        return fail(ctx, (int)rs, "srt_trace_radiance: %s (first_sample %u, sample_count %u, max_bounces %d, flags 0x%x)", why, t->first_sample,
                    t->sample_count, t->max_bounces, t->flags);
    if (srt::sun_sampling_asked(t->flags)) {
        if (const int rc = check_sun_sampling(ctx, "srt_trace_radiance")) return rc;
    }
    const bool sun = srt::sun_sampling_applies(t->flags, t->max_bounces);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = ctx->rays.count();
    const bool count = (t->flags & SRT_RADIANCE_COUNT_WORK) != 0;
    const bool tail = srt::probe_tail_applies(ctx->probe_tail, t->max_bounces);
    if (tail) {  // the output where it stands now (an own buffer that is about to be allocated cannot be the bound coefficient array)
        if (const int rc = check_probe_tail(ctx, "srt_trace_radiance", current(ctx->radiance_out, ctx->d_radiance_own), n * sizeof(float4))) return rc;
    }
    float4* dst = nullptr;
    SRT_WRITE_TARGET_AFTER(ctx, ctx->radiance_out, ctx->d_radiance_own, n * sizeof(float4), dst, output_released(ctx, ctx->radiance.last, 0, ctx->d_radiance_own));
    srt::KernelParams K;
    const KernelSetup ks = scene_kernel_params(ctx, 0, ctx->height, K);
    // (the fields accumulate_sample and the bounce loop read)
    K.first_sample = t->first_sample, K.sample_count = t->sample_count, K.max_bounces = t->max_bounces, K.seed = t->seed;
    if (t->flags & SRT_RADIANCE_RESET) K.flags |= SRT_RENDER_RESET;
    const auto kernel = SRT_KERNEL(srt::radiance_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0, count);
    const auto tail_kernel = SRT_KERNEL(srt::radiance_tail_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0);
    const auto sun_kernel = SRT_KERNEL(srt::radiance_sun_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0);
    // the grid first: the sample scratch is sized by it
    const unsigned wgs = srt::radiance_grid(
        n, srt::OUT_WG_UNITS, resident_workgroups(ctx, sun ? (const void*)sun_kernel : tail ? (const void*)tail_kernel : (const void*)kernel, ks.lds_bytes));
    if (const int rc = ensure_sample_rows(ctx, wgs)) return rc;
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_radiance_work)) return rc;
    }
    if (const int rc = zero_probe_tail_work(ctx)) return rc;
    srt::RadianceIO io{};
    io.origin = current(ctx->rays.origins, ctx->d_ray_origin);
    io.direction = ctx->rays.bound() ? (const float4*)ctx->rays.bound_direction : (const float4*)ctx->d_ray_direction;
    io.count = (uint32_t)n;
    io.normalize = (t->flags & SRT_RADIANCE_NORMALIZE) ? 1u : 0u;
    io.id_base = t->id_base;
    io.out = dst;
    io.rows = ctx->d_radiance_rows;
    io.work = count ? (unsigned long long*)ctx->d_radiance_work : nullptr;
    if (const int rc = sun    ? launch_persistent_sun(ctx, sun_kernel, wgs, ks, K, io, sun_io(ctx))
                       : tail ? launch_persistent_tail(ctx, tail_kernel, wgs, ks, K, io, probe_tail_io(ctx))
                              : launch_persistent(ctx, kernel, wgs, ks, K, io))
        return rc;
    srt::radiance_traced(ctx->radiance, n, dst, t->flags);
    srt::probe_tail_traced(ctx->probe_tail);
    return SRT_OK;
}

int srt_bind_radiance(srt_context* ctx, void* d_float4) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return ctx->radiance_out.bind(d_float4), SRT_OK;  // (no synchronisation: enqueued traces keep the buffer they were given, as srt_bind_ray_output)
}

int srt_read_radiance(srt_context* ctx, float* dst_rgba) {
    if (!ctx || !dst_rgba) return SRT_ERR_INVALID_ARG;
    return read_slot(ctx, ctx->radiance.last.read(1u, 0), dst_rgba, ctx->radiance.last_count * sizeof(float4),
                     "srt_read_radiance: there has been no srt_trace_radiance (or its buffer has been re-allocated)");
}

SRT_WORK_LAYOUT(srt_radiance_work, srt::RAD_WORK_N, rays, srt::RAD_WORK_RAYS, wave_calls, srt::RAD_WORK_WAVE_CALLS);
int srt_get_radiance_work(srt_context* ctx, srt_radiance_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->radiance.call, ctx->d_radiance_work, out,
                    "srt_get_radiance_work: the last srt_trace_radiance did not ask for SRT_RADIANCE_COUNT_WORK (or there has been none)");
}

// ---- light probes --------------------------------------------------------------------------------------------------
static_assert(SRT_LIGHT_PROBE_RESET == srt::LIGHT_PROBE_FLAG_RESET && SRT_LIGHT_PROBE_NORMALIZE == srt::LIGHT_PROBE_FLAG_NORMALIZE &&
              SRT_LIGHT_PROBE_COUNT_WORK == srt::LIGHT_PROBE_FLAG_COUNT_WORK && SRT_LIGHT_PROBE_RESET == SRT_RENDER_RESET &&
              SRT_LIGHT_PROBE_COEFFICIENTS == srt::LIGHT_PROBE_OUT_COEFFICIENTS && SRT_LIGHT_PROBE_RADIANCE == srt::LIGHT_PROBE_OUT_RADIANCE &&
              SRT_LIGHT_PROBE_MAX_DIRECTIONS == srt::LIGHT_PROBE_MAX_DIRECTIONS && sizeof(srt_light_probe_params) == 32 &&
              sizeof(srt::LightProbeCall) == 32 && sizeof(srt_light_probe_work) == 56 && (int)srt::LIGHT_PROBE_COEFFS == (int)srt::LP_COEFFS &&
              srt::LP_WORK_N == 6,
              "srt_light_probes_host.h, srt_light_probes.hip.h and srt_pathtrace.h disagree");

// srt_write_light_probes / srt_write_light_probe_directions / srt_write_probe_previous_states: 1 .. limit float4
static int write_light_probe_input(srt_context* ctx, srt::InputArray& in, DeviceBuffer<float4>& own, const float* src, size_t count, size_t limit,
                                   const char* who) {
    if (count < 1 || count > limit) return fail(ctx, SRT_ERR_INVALID_ARG, "%s: %zu elements: want 1 .. %zu", who, count, limit);
    return write_probe_input(ctx, in, own, src, count, sizeof(float4));
}

int srt_write_light_probes(srt_context* ctx, const float* positions, size_t count) {
    if (!ctx || !positions) return SRT_ERR_INVALID_ARG;
    return write_light_probe_input(ctx, ctx->probes.positions, ctx->d_probe_position, positions, count, srt::LIGHT_PROBE_MAX_RAYS, "srt_write_light_probes");
}

int srt_bind_light_probes(srt_context* ctx, const void* d_positions, size_t count) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    // (no synchronisation: enqueued traces keep the array they were given, as srt_bind_rays)
    if (srt::input_bind(ctx->probes.positions, d_positions, count, srt::LIGHT_PROBE_MAX_RAYS) != srt::RAYS_OK)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_bind_light_probes: want a device array and 1 .. 2^30 positions, or NULL, 0 (got %zu)", count);
    return SRT_OK;
}

int srt_write_light_probe_directions(srt_context* ctx, const float* directions, size_t count) {
    if (!ctx || !directions) return SRT_ERR_INVALID_ARG;
    return write_light_probe_input(ctx, ctx->probes.directions, ctx->d_probe_direction, directions, count, srt::LIGHT_PROBE_MAX_DIRECTIONS,
                                   "srt_write_light_probe_directions");
}

int srt_bind_light_probe_directions(srt_context* ctx, const void* d_directions, size_t count) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (srt::input_bind(ctx->probes.directions, d_directions, count, srt::LIGHT_PROBE_MAX_DIRECTIONS) != srt::RAYS_OK)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_bind_light_probe_directions: want a device array and 1 .. 4096 directions, or NULL, 0 (got %zu)", count);
    return SRT_OK;
}

int srt_light_probe_params_default(srt_light_probe_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt::LightProbeCall c;
    srt::light_probe_call_default(c);
    out->first_sample = c.first_sample, out->sample_count = c.sample_count, out->max_bounces = c.max_bounces;
    out->seed = c.seed, out->id_base = c.id_base, out->flags = c.flags, out->outputs = c.outputs, out->reserved = c.reserved;
    return SRT_OK;
}

// srt_trace_light_probes (listed == false) and srt_trace_light_probes_listed: one body.  The listed call is sized for P as the
// unlisted one is (the grid, the sample scratch, the partial buffer): the count of the list stays on the device.
static int trace_light_probes(srt_context* ctx, const srt_light_probe_params* t, bool listed, const char* who) {
    if (!ctx || !t) return SRT_ERR_INVALID_ARG;
    const srt::LightProbeCall call{t->first_sample, t->sample_count, t->max_bounces, t->seed, t->id_base, t->flags, t->outputs, t->reserved};
    const char* why = "";
    if (const srt::RaysStatus rs = srt::sun_light_probe_check_trace(ctx->probes, ctx->scene_set, call, current(ctx->probe_out[1], ctx->d_probe_out_own[1]), &why))
        return fail(ctx, (int)rs, "%s: %s (first_sample %u, sample_count %u, max_bounces %d, flags 0x%x, outputs 0x%x, reserved %u)", who, why, t->first_sample,
                    t->sample_count, t->max_bounces, t->flags, t->outputs, t->reserved);
    const size_t np = ctx->probes.positions.count(), nk = ctx->probes.directions.count();
    if (listed) {
        if (const srt::RaysStatus rs = srt::probe_list_check_trace(ctx->probe_update, np, &why)) return fail(ctx, (int)rs, "%s: %s", who, why);
    }
    if (srt::sun_sampling_asked(t->flags)) {
        if (const int rc = check_sun_sampling(ctx, who)) return rc;
    }
    const bool sun = srt::sun_sampling_applies(t->flags, t->max_bounces);
    const bool tail = srt::probe_tail_applies(ctx->probe_tail, t->max_bounces);
    if (tail) {  // the outputs this call writes, where they stand now: COEFFICIENTS, and RADIANCE as srt_trace_radiance's
        for (int i = 0; i < srt::LIGHT_PROBE_SLOTS; ++i)
            if (t->outputs & (1u << i))
                if (const int rc = check_probe_tail(ctx, who, current(ctx->probe_out[i], ctx->d_probe_out_own[i]), srt::light_probe_elems(i, np, nk) * sizeof(float4)))
                    return rc;
    }
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t J = srt::light_probe_blocks(nk);
    const bool count = (t->flags & SRT_LIGHT_PROBE_COUNT_WORK) != 0;
    const bool coefficients = (t->outputs & SRT_LIGHT_PROBE_COEFFICIENTS) != 0;
    float4* dst[srt::LIGHT_PROBE_SLOTS] = {nullptr, nullptr};
    for (int i = 0; i < srt::LIGHT_PROBE_SLOTS; ++i)
        if (t->outputs & (1u << i))
            SRT_WRITE_TARGET_AFTER(ctx, ctx->probe_out[i], ctx->d_probe_out_own[i], srt::light_probe_elems(i, np, nk) * sizeof(float4), dst[i],
                                   output_released(ctx, ctx->probes.last, i, ctx->d_probe_out_own[i]));
    const size_t partial = coefficients ? srt::light_probe_partial_bytes(np, nk) : 0;
    if (ctx->d_probe_partial.bytes() < partial) {
        if (const int rc = finish_stream(ctx)) return rc;
        SRT_HIP(ctx, ctx->d_probe_partial.ensure(partial));
    }
    srt::KernelParams K;
    const KernelSetup ks = scene_kernel_params(ctx, 0, ctx->height, K);
    // (the fields accumulate_sample and the bounce loop read)
    K.first_sample = t->first_sample, K.sample_count = t->sample_count, K.max_bounces = t->max_bounces, K.seed = t->seed;
    if (t->flags & SRT_LIGHT_PROBE_RESET) K.flags |= SRT_RENDER_RESET;
    const auto kernel = SRT_KERNEL(srt::light_probe_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0, count, listed);
    const auto tail_kernel = SRT_KERNEL(srt::light_probe_tail_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0, listed);
    const auto sun_kernel = SRT_KERNEL(srt::light_probe_sun_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0, listed);
    // the grid first: the sample scratch is sized by it
    const unsigned wgs = srt::light_probe_grid(
        np, nk, srt::OUT_WG_UNITS, resident_workgroups(ctx, sun ? (const void*)sun_kernel : tail ? (const void*)tail_kernel : (const void*)kernel, ks.lds_bytes));
    if (const int rc = ensure_sample_rows(ctx, wgs)) return rc;
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_probe_work)) return rc;
    }
    if (const int rc = zero_probe_tail_work(ctx)) return rc;
    srt::LightProbeIO io{};
    io.position = current(ctx->probes.positions, ctx->d_probe_position);
    io.direction = current(ctx->probes.directions, ctx->d_probe_direction);
    io.probes = (uint32_t)np, io.directions = (uint32_t)nk, io.blocks = (uint32_t)J;
    io.normalize = (t->flags & SRT_LIGHT_PROBE_NORMALIZE) ? 1u : 0u;
    io.id_base = t->id_base;
    io.coefficients = J == 1 ? dst[0] : nullptr;
    io.partial = J > 1 && coefficients ? (float4*)ctx->d_probe_partial : nullptr;
    io.radiance = dst[1];
    io.rows = ctx->d_radiance_rows;
    io.work = count ? (unsigned long long*)ctx->d_probe_work : nullptr;
    io.list = listed ? current_probe_list(ctx) : nullptr;
    if (const int rc = sun    ? launch_persistent_sun(ctx, sun_kernel, wgs, ks, K, io, sun_io(ctx))
                       : tail ? launch_persistent_tail(ctx, tail_kernel, wgs, ks, K, io, probe_tail_io(ctx))
                              : launch_persistent(ctx, kernel, wgs, ks, K, io))
        return rc;
    if (J > 1 && coefficients) {  // the block sums of every probe, added in ascending block order
        const size_t elems = np * (size_t)srt::LP_COEFFS;
        if (listed)
            hipLaunchKernelGGL(srt::light_probe_sum_listed_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, ctx->stream,
                               (const float4*)ctx->d_probe_partial, dst[0], io.list, (uint32_t)np, (uint32_t)J);
        else
            hipLaunchKernelGGL(srt::light_probe_sum_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, ctx->stream, (const float4*)ctx->d_probe_partial,
                               dst[0], elems, (uint32_t)J);
        SRT_HIP(ctx, hipGetLastError());
    }
    void* const wrote[srt::LIGHT_PROBE_SLOTS] = {dst[0], dst[1]};
    srt::light_probe_traced(ctx->probes, np, nk, t->outputs, wrote, t->flags);
    srt::probe_tail_traced(ctx->probe_tail);
    return SRT_OK;
}

int srt_trace_light_probes(srt_context* ctx, const srt_light_probe_params* t) { return trace_light_probes(ctx, t, false, "srt_trace_light_probes"); }
int srt_trace_light_probes_listed(srt_context* ctx, const srt_light_probe_params* t) { return trace_light_probes(ctx, t, true, "srt_trace_light_probes_listed"); }

int srt_bind_light_probe_output(srt_context* ctx, uint32_t output, void* d_ptr) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return bind_output(ctx, ctx->probe_out, srt::light_probe_slot(output), d_ptr,
                       "srt_bind_light_probe_output: output 0x%x is not a single SRT_LIGHT_PROBE_COEFFICIENTS / _RADIANCE bit", output);
}

int srt_read_light_probe_output(srt_context* ctx, uint32_t output, void* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    const int i = srt::light_probe_slot(output);
    return read_output(ctx, ctx->probes.last, output, i, dst, srt::light_probe_elems(i, ctx->probes.last_probes, ctx->probes.last_directions) * sizeof(float4),
                       "srt_read_light_probe_output: output 0x%x is not a single SRT_LIGHT_PROBE_COEFFICIENTS / _RADIANCE bit",
                       "srt_read_light_probe_output: output 0x%x was not written by the last srt_trace_light_probes");
}

SRT_WORK_LAYOUT(srt_light_probe_work, srt::LP_WORK_N, probes, srt::LP_WORK_PROBES, waves, srt::LP_WORK_WAVES);
int srt_get_light_probe_work(srt_context* ctx, srt_light_probe_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->probes.call, ctx->d_probe_work, out,
                    "srt_get_light_probe_work: the last srt_trace_light_probes did not ask for SRT_LIGHT_PROBE_COUNT_WORK (or there has been none)");
}

int srt_light_probe_sphere(size_t count, float* dst) {
    if (count < 1 || !dst) return SRT_ERR_INVALID_ARG;
    srt::light_probe_sphere(count, dst);
    return SRT_OK;
}

int srt_light_probe_irradiance(const float* coefficients, const float* normal, float* rgb) {
    if (!coefficients || !normal || !rgb) return SRT_ERR_INVALID_ARG;
    srt::light_probe_irradiance(coefficients, normal, rgb);
    return SRT_OK;
}

// ---- probe-grid shading --------------------------------------------------------------------------------------------
static_assert(SRT_PROBE_GRID_VISIBILITY == srt::PROBE_GRID_FLAG_VISIBILITY && SRT_PROBE_GRID_NORMAL_WEIGHT == srt::PROBE_GRID_FLAG_NORMAL_WEIGHT &&
              SRT_PROBE_GRID_ALBEDO == srt::PROBE_GRID_FLAG_ALBEDO && SRT_PROBE_GRID_COUNT_WORK == srt::PROBE_GRID_FLAG_COUNT_WORK &&
              sizeof(srt_probe_grid) == 36 && sizeof(srt::ProbeGrid) == 36 && sizeof(srt_probe_grid_params) == 32 && sizeof(srt::ProbeGridCall) == 32 &&
              sizeof(srt_probe_grid_work) == 80 && (int)srt::PG_COEFFS == (int)srt::LIGHT_PROBE_COEFFS,
              "srt_probe_grid_host.h, srt_probe_grid.hip.h and srt_pathtrace.h disagree");

static srt::ProbeGrid probe_grid_of(const srt_probe_grid* g) {
    srt::ProbeGrid r;
    for (int a = 0; a < 3; ++a) r.origin[a] = g->origin[a], r.spacing[a] = g->spacing[a], r.counts[a] = g->counts[a];
    return r;
}

int srt_probe_grid_positions(const srt_probe_grid* grid, float* dst) {
    if (!grid || !dst) return SRT_ERR_INVALID_ARG;
    const srt::ProbeGrid g = probe_grid_of(grid);
    if (srt::probe_grid_check(g, nullptr) != srt::RAYS_OK) return SRT_ERR_INVALID_ARG;
    srt::probe_grid_positions(g, dst);
    return SRT_OK;
}

int srt_probe_grid_params_default(srt_probe_grid_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt::ProbeGridCall c;
    srt::probe_grid_call_default(c);
    memcpy(out, &c, sizeof c);
    return SRT_OK;
}

int srt_set_probe_grid(srt_context* ctx, const srt_probe_grid* grid) {
    if (!ctx || !grid) return SRT_ERR_INVALID_ARG;
    const srt::ProbeGrid g = probe_grid_of(grid);
    const char* why = "";
    if (srt::probe_grid_check(g, &why) != srt::RAYS_OK)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_set_probe_grid: %s (origin %g %g %g, spacing %g %g %g, counts %d %d %d)", why, (double)g.origin[0],
                    (double)g.origin[1], (double)g.origin[2], (double)g.spacing[0], (double)g.spacing[1], (double)g.spacing[2], g.counts[0], g.counts[1], g.counts[2]);
    ctx->probe_grid.grid = g, ctx->probe_grid.grid_set = true;  // (an enqueued launch keeps the grid it was given: a kernel argument)
    return SRT_OK;
}

int srt_write_probe_grid_coefficients(srt_context* ctx, const float* coefficients, size_t probes) {
    if (!ctx || !coefficients) return SRT_ERR_INVALID_ARG;
    if (probes < 1 || probes > srt::PROBE_GRID_MAX_PROBES)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_write_probe_grid_coefficients: %zu probes: want 1 .. 2^30", probes);
    return write_probe_input(ctx, ctx->probe_grid.coefficients, ctx->d_probe_grid_coefficients, coefficients, probes, srt::PG_COEFFS * sizeof(float4));
}

int srt_bind_probe_grid_coefficients(srt_context* ctx, const void* d_ptr, size_t probes) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (srt::input_bind(ctx->probe_grid.coefficients, d_ptr, probes, srt::PROBE_GRID_MAX_PROBES) != srt::RAYS_OK)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_bind_probe_grid_coefficients: want a device array and 1 .. 2^30 probes, or NULL, 0 (got %zu)", probes);
    return SRT_OK;
}

// srt_shade_probe_grid, srt_shade_probe_grid_depth (`d` given) and srt_shade_probe_grid_states (`d` given or NULL): one body.  The
// entry points have checked ctx, s and, where the call requires it, d.
enum ProbeGridShading { PG_SHADE_QUERY, PG_SHADE_DEPTH, PG_SHADE_STATES };
static int shade_probe_grid(srt_context* ctx, const char* who, const srt_probe_grid_params* s, const srt_probe_grid_depth_params* d, ProbeGridShading which) {
    srt::ProbeGridCall call;
    memcpy(&call, s, sizeof call);
    srt::ProbeGridDepthCall dcall{};
    if (d) memcpy(&dcall, d, sizeof dcall);
    bool present[srt::PROBE_GRID_GUIDES];
    for (int i = 0; i < srt::PROBE_GRID_GUIDES; ++i) present[i] = current(ctx->gbuf[i], ctx->d_gbuf_own[i]) != nullptr;
    const char* why = "";
    const srt::RaysStatus rs =
        which == PG_SHADE_QUERY   ? srt::probe_grid_check_shade(ctx->probe_grid, call, ctx->scene_set, ctx->height, present, &why)
        : which == PG_SHADE_DEPTH ? srt::probe_grid_depth_check_shade(ctx->probe_grid, ctx->probe_grid_depth, call, dcall, ctx->scene_set, ctx->height, present, &why)
                                  : srt::probe_grid_states_check_shade(ctx->probe_grid, ctx->probe_grid_depth, ctx->probe_states, call, d ? &dcall : nullptr,
                                                                       ctx->scene_set, ctx->height, present, &why);
    if (rs) {
        char depth[96] = "";
        if (d) snprintf(depth, sizeof depth, "; bias %g, min_variance %g, reserved %u %u", (double)d->bias, (double)d->min_variance, d->reserved[0], d->reserved[1]);
        return fail(ctx, (int)rs, "%s: %s (rows [%d,%d) of %d, flags 0x%x, band_weight %g %g %g, reserved %u %u%s)", who, why, s->row_begin, s->row_end, ctx->height,
                    s->flags, (double)s->band_weight[0], (double)s->band_weight[1], (double)s->band_weight[2], s->reserved[0], s->reserved[1], depth);
    }
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const bool count = (s->flags & SRT_PROBE_GRID_COUNT_WORK) != 0;
    float4* dst = nullptr;
    SRT_WRITE_TARGET(ctx, ctx->probe_grid_out, ctx->d_probe_grid_own, frame_pixels(ctx) * sizeof(float4), dst);
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_probe_grid_work)) return rc;
    }
    srt::KernelParams K;
    KernelSetup ks = scene_kernel_params(ctx, s->row_begin, s->row_end, K);
    void (*kernel)(srt::KernelParams, srt::ProbeGridIO);
    if (which == PG_SHADE_QUERY) {
        kernel = SRT_KERNEL(srt::probe_grid_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0, count);
    } else {
        ks.lds_bytes = 0;  // (the kernel traces nothing: no scene image, and its own LDS is static)
        kernel = which == PG_SHADE_DEPTH ? SRT_KERNEL(srt::probe_grid_depth_kernel, count) : SRT_KERNEL(srt::probe_grid_states_kernel, d != nullptr, count);
    }
    const srt::ProbeGrid& g = ctx->probe_grid.grid;
    srt::ProbeGridIO io{};
    io.object = (const int32_t*)current(ctx->gbuf[0], ctx->d_gbuf_own[0]);
    io.normal_depth = (const float4*)current(ctx->gbuf[1], ctx->d_gbuf_own[1]);
    io.position = (const float4*)current(ctx->gbuf[2], ctx->d_gbuf_own[2]);
    io.albedo = (s->flags & SRT_PROBE_GRID_ALBEDO) ? (const float4*)current(ctx->gbuf[3], ctx->d_gbuf_own[3]) : nullptr;
    io.coefficients = current(ctx->probe_grid.coefficients, ctx->d_probe_grid_coefficients);
    io.out = dst;
    for (int a = 0; a < 3; ++a) io.origin[a] = g.origin[a], io.spacing[a] = g.spacing[a], io.counts[a] = g.counts[a], io.band_weight[a] = s->band_weight[a];
    io.visibility = (s->flags & SRT_PROBE_GRID_VISIBILITY) ? 1u : 0u;  // (the rules of the other two calls refuse the flag)
    io.normal_weight = (s->flags & SRT_PROBE_GRID_NORMAL_WEIGHT) ? 1u : 0u;
    io.work = count ? (unsigned long long*)ctx->d_probe_grid_work : nullptr;
    if (which == PG_SHADE_STATES) io.states = current(ctx->probe_states.states, ctx->d_probe_grid_states);
    if (d) {
        io.depth = current(ctx->probe_grid_depth.moments, ctx->d_probe_grid_depth);
        io.resolution = ctx->probe_grid_depth.resolution();
        io.bias = d->bias, io.min_variance = d->min_variance;
    }
    if (const int rc = launch_tiles(ctx, kernel, ks, K, io)) return rc;
    ctx->probe_grid_out.wrote(dst);
    srt::probe_grid_shaded(ctx->probe_grid, s->flags);
    return SRT_OK;
}

int srt_shade_probe_grid(srt_context* ctx, const srt_probe_grid_params* s) {
    if (!ctx || !s) return SRT_ERR_INVALID_ARG;
    return shade_probe_grid(ctx, "srt_shade_probe_grid", s, nullptr, PG_SHADE_QUERY);
}

int srt_bind_probe_grid_output(srt_context* ctx, void* d_float4) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return ctx->probe_grid_out.bind(d_float4), SRT_OK;  // (no synchronisation: an enqueued call keeps the buffer it was given, as srt_bind_gbuffer)
}

int srt_read_probe_grid_output(srt_context* ctx, float* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    return read_slot(ctx, ctx->probe_grid_out.read_any(ctx->d_probe_grid_own), dst, frame_pixels(ctx) * sizeof(float4),
                     "srt_read_probe_grid_output: there has been no srt_shade_probe_grid");
}

SRT_WORK_LAYOUT(srt_probe_grid_work, srt::PG_WORK_N, pixels, srt::PG_WORK_PIXELS, waves, srt::PG_WORK_WAVES);
int srt_get_probe_grid_work(srt_context* ctx, srt_probe_grid_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->probe_grid.call, ctx->d_probe_grid_work, out,
                    "srt_get_probe_grid_work: the last srt_shade_probe_grid did not ask for SRT_PROBE_GRID_COUNT_WORK (or there has been none)");
}

// ---- probe depth moments -------------------------------------------------------------------------------------------
static_assert(SRT_PROBE_DEPTH_MOMENTS == srt::PROBE_DEPTH_OUT_MOMENTS && SRT_PROBE_DEPTH_DISTANCES == srt::PROBE_DEPTH_OUT_DISTANCES &&
              SRT_PROBE_DEPTH_NORMALIZE == srt::PROBE_DEPTH_FLAG_NORMALIZE && SRT_PROBE_DEPTH_COUNT_WORK == srt::PROBE_DEPTH_FLAG_COUNT_WORK &&
              sizeof(srt_probe_depth_params) == 24 && sizeof(srt::ProbeDepthCall) == 24 && sizeof(srt_probe_depth_work) == 48 && srt::PD_WORK_N == 5 &&
              sizeof(srt_probe_grid_depth_params) == 16 && sizeof(srt::ProbeGridDepthCall) == 16,
              "srt_probe_depth_host.h, srt_probe_depth.hip.h and srt_pathtrace.h disagree");

int srt_probe_depth_params_default(srt_probe_depth_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt::ProbeDepthCall c;
    srt::probe_depth_call_default(c);
    memcpy(out, &c, sizeof c);
    return SRT_OK;
}

int srt_probe_depth_texels(uint32_t resolution, float* dst) {
    if (!dst || !srt::probe_depth_resolution_ok(resolution)) return SRT_ERR_INVALID_ARG;
    srt::probe_depth_texels(resolution, dst);
    return SRT_OK;
}

// srt_trace_probe_depth (listed == false) and srt_trace_probe_depth_listed: one body
static int trace_probe_depth(srt_context* ctx, const srt_probe_depth_params* t, bool listed, const char* who) {
    if (!ctx || !t) return SRT_ERR_INVALID_ARG;
    srt::ProbeDepthCall call;
    memcpy(&call, t, sizeof call);
    const char* why = "";
    if (const srt::RaysStatus rs = srt::probe_depth_check_trace(ctx->probes, ctx->scene_set, call, &why))
        return fail(ctx, (int)rs, "%s: %s (resolution %u, sharpness %u, max_distance %g, flags 0x%x, outputs 0x%x, reserved %u)", who, why, t->resolution, t->sharpness,
                    (double)t->max_distance, t->flags, t->outputs, t->reserved);
    const size_t np = ctx->probes.positions.count(), nk = ctx->probes.directions.count();
    if (listed) {
        if (const srt::RaysStatus rs = srt::probe_list_check_trace(ctx->probe_update, np, &why)) return fail(ctx, (int)rs, "%s: %s", who, why);
    }
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const bool count = (t->flags & SRT_PROBE_DEPTH_COUNT_WORK) != 0;
    if (!ctx->probe_depth_texels_ready) {  // the three tables, once: no launch has read the buffer yet
        float table[srt::PROBE_DEPTH_TABLE * 4];
        for (uint32_t r = 4; r <= 16; r *= 2) srt::probe_depth_texels(r, table + 4 * srt::probe_depth_table_offset(r));
        SRT_HIP(ctx, ctx->d_probe_depth_texels.ensure(sizeof table));
        SRT_HIP(ctx, hipMemcpy(ctx->d_probe_depth_texels, table, sizeof table, hipMemcpyHostToDevice));
        ctx->probe_depth_texels_ready = true;
    }
    void* dst[srt::PROBE_DEPTH_SLOTS] = {nullptr, nullptr};
    for (int i = 0; i < srt::PROBE_DEPTH_SLOTS; ++i)
        if (t->outputs & (1u << i))
            SRT_WRITE_TARGET_AFTER(ctx, ctx->probe_depth_out[i], ctx->d_probe_depth_own[i], srt::probe_depth_bytes(i, np, nk, t->resolution), dst[i],
                                   output_released(ctx, ctx->probe_depth.last, i, ctx->d_probe_depth_own[i]));
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_probe_depth_work)) return rc;
    }
    srt::KernelParams K;
    const KernelSetup ks = scene_kernel_params(ctx, 0, ctx->height, K);
    const auto kernel = SRT_KERNEL(srt::probe_depth_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0, count, listed);
    const unsigned wgs = srt::probe_depth_grid(np, srt::OUT_WG_UNITS, resident_workgroups(ctx, (const void*)kernel, ks.lds_bytes));
    srt::ProbeDepthIO io{};
    io.position = current(ctx->probes.positions, ctx->d_probe_position);
    io.direction = current(ctx->probes.directions, ctx->d_probe_direction);
    io.texel = (const float4*)ctx->d_probe_depth_texels + srt::probe_depth_table_offset(t->resolution);
    io.probes = (uint32_t)np, io.directions = (uint32_t)nk, io.resolution = t->resolution, io.sharpness = t->sharpness;
    io.max_distance = t->max_distance;
    io.normalize = (t->flags & SRT_PROBE_DEPTH_NORMALIZE) ? 1u : 0u;
    io.moments = (float4*)dst[0];
    io.distances = (float*)dst[1];
    io.work = count ? (unsigned long long*)ctx->d_probe_depth_work : nullptr;
    io.list = listed ? current_probe_list(ctx) : nullptr;
    if (const int rc = launch_persistent(ctx, kernel, wgs, ks, K, io)) return rc;
    srt::probe_depth_traced(ctx->probe_depth, np, nk, call, dst);
    return SRT_OK;
}

int srt_trace_probe_depth(srt_context* ctx, const srt_probe_depth_params* t) { return trace_probe_depth(ctx, t, false, "srt_trace_probe_depth"); }
int srt_trace_probe_depth_listed(srt_context* ctx, const srt_probe_depth_params* t) { return trace_probe_depth(ctx, t, true, "srt_trace_probe_depth_listed"); }

int srt_bind_probe_depth_output(srt_context* ctx, uint32_t output, void* d_ptr) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return bind_output(ctx, ctx->probe_depth_out, srt::probe_depth_slot(output), d_ptr,
                       "srt_bind_probe_depth_output: output 0x%x is not a single SRT_PROBE_DEPTH_MOMENTS / _DISTANCES bit", output);
}

int srt_read_probe_depth_output(srt_context* ctx, uint32_t output, void* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    const srt::ProbeDepthState& s = ctx->probe_depth;
    const int i = srt::probe_depth_slot(output);
    return read_output(ctx, s.last, output, i, dst, srt::probe_depth_bytes(i, s.last_probes, s.last_directions, s.last_resolution),
                       "srt_read_probe_depth_output: output 0x%x is not a single SRT_PROBE_DEPTH_MOMENTS / _DISTANCES bit",
                       "srt_read_probe_depth_output: output 0x%x was not written by the last srt_trace_probe_depth");
}

SRT_WORK_LAYOUT(srt_probe_depth_work, srt::PD_WORK_N, probes, srt::PD_WORK_PROBES, waves, srt::PD_WORK_WAVES);
int srt_get_probe_depth_work(srt_context* ctx, srt_probe_depth_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->probe_depth.call, ctx->d_probe_depth_work, out,
                    "srt_get_probe_depth_work: the last srt_trace_probe_depth did not ask for SRT_PROBE_DEPTH_COUNT_WORK (or there has been none)");
}

// ---- probe-grid shading with the filtered visibility test ------------------------------------------------------------
int srt_probe_grid_depth_params_default(srt_probe_grid_depth_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt::ProbeGridDepthCall c;
    srt::probe_grid_depth_call_default(c);
    memcpy(out, &c, sizeof c);
    return SRT_OK;
}

int srt_write_probe_grid_depth(srt_context* ctx, const float* moments, size_t probes, uint32_t resolution) {
    if (!ctx || !moments) return SRT_ERR_INVALID_ARG;
    if (srt::probe_grid_depth_check_input(probes, resolution) != srt::RAYS_OK)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_write_probe_grid_depth: %zu probes of resolution %u: want resolution 4, 8 or 16 and 1 <= probes * resolution^2 <= 2^30",
                    probes, resolution);
    if (const int rc = write_probe_input(ctx, ctx->probe_grid_depth.moments, ctx->d_probe_grid_depth, moments, probes, (size_t)resolution * resolution * sizeof(float4)))
        return rc;
    srt::probe_grid_depth_written(ctx->probe_grid_depth, probes, resolution);  // (the resolution with the count)
    return SRT_OK;
}

int srt_bind_probe_grid_depth(srt_context* ctx, const void* d_ptr, size_t probes, uint32_t resolution) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (srt::probe_grid_depth_bind(ctx->probe_grid_depth, d_ptr, probes, resolution) != srt::RAYS_OK)
        return fail(ctx, SRT_ERR_INVALID_ARG,
                    "srt_bind_probe_grid_depth: want a device array, resolution 4, 8 or 16 and 1 <= probes * resolution^2 <= 2^30, or NULL, 0 (got %zu, %u)", probes,
                    resolution);
    return SRT_OK;
}

int srt_shade_probe_grid_depth(srt_context* ctx, const srt_probe_grid_params* s, const srt_probe_grid_depth_params* d) {
    if (!ctx || !s || !d) return SRT_ERR_INVALID_ARG;
    return shade_probe_grid(ctx, "srt_shade_probe_grid_depth", s, d, PG_SHADE_DEPTH);
}

// ---- probe classification and relocation ----------------------------------------------------------------------------
static_assert(SRT_PROBE_STATE_RECORDS == srt::PROBE_STATE_OUT_RECORDS && SRT_PROBE_STATE_POSITIONS == srt::PROBE_STATE_OUT_POSITIONS &&
              SRT_PROBE_CLASSIFY_RELOCATE == srt::PROBE_CLASSIFY_FLAG_RELOCATE && SRT_PROBE_CLASSIFY_NORMALIZE == srt::PROBE_CLASSIFY_FLAG_NORMALIZE &&
              SRT_PROBE_CLASSIFY_COUNT_WORK == srt::PROBE_CLASSIFY_FLAG_COUNT_WORK && SRT_PROBE_MOVED == srt::PROBE_MOVED && SRT_PROBE_BURIED == srt::PROBE_BURIED &&
              SRT_PROBE_INSIDE == srt::PROBE_INSIDE && SRT_PROBE_IDLE == srt::PROBE_IDLE && (uint32_t)srt::PS_MOVED == srt::PROBE_MOVED &&
              (uint32_t)srt::PS_BURIED == srt::PROBE_BURIED && (uint32_t)srt::PS_INSIDE == srt::PROBE_INSIDE && (uint32_t)srt::PS_IDLE == srt::PROBE_IDLE &&
              SRT_OBJ_SPHERE == srt::PROBE_TABLE_OBJ_SPHERE && SRT_OBJ_BOX == srt::PROBE_TABLE_OBJ_BOX && SRT_OBJ_MESH == srt::PROBE_TABLE_OBJ_MESH &&
              sizeof(srt_probe_classify_params) == 24 && sizeof(srt::ProbeClassifyCall) == 24 && sizeof(srt_probe_classify_work) == 64 && srt::PS_WORK_N == 7,
              "srt_probe_states_host.h, srt_probe_states.hip.h and srt_pathtrace.h disagree");

int srt_probe_classify_params_default(srt_probe_classify_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt::ProbeClassifyCall c;
    srt::probe_classify_call_default(c);
    memcpy(out, &c, sizeof c);
    return SRT_OK;
}

// The primitive table of the scene as it stands, on the device: rebuilt when the scene has changed since the last build.  Earlier
// classifications may still read the old one, so the stream is finished first.
static int probe_table_current(srt_context* ctx) {
    if (ctx->probe_table_ready && ctx->probe_table_scene == ctx->scene_changes) return SRT_OK;
    if (const int rc = finish_stream(ctx)) return rc;
    ctx->probe_table_ready = false;
    try {
        srt::probe_table_build(ctx->objects.data(), ctx->objects.size(), ctx->probe_table);
    } catch (const std::bad_alloc&) {
        return fail(ctx, SRT_ERR_OOM, "srt_classify_probes: host allocation failed");
    }
    const size_t bytes = (ctx->probe_table.vec4() > 0 ? ctx->probe_table.vec4() : 1) * sizeof(float4);
    SRT_HIP(ctx, ctx->d_probe_table.ensure(bytes));
    if (ctx->probe_table.vec4() > 0)
        SRT_HIP(ctx, hipMemcpy(ctx->d_probe_table, ctx->probe_table.rows.data(), ctx->probe_table.vec4() * sizeof(float4), hipMemcpyHostToDevice));
    ctx->probe_table_ready = true, ctx->probe_table_scene = ctx->scene_changes;
    return SRT_OK;
}

int srt_classify_probes(srt_context* ctx, const srt_probe_classify_params* t) {
    if (!ctx || !t) return SRT_ERR_INVALID_ARG;
    srt::ProbeClassifyCall call;
    memcpy(&call, t, sizeof call);
    const char* why = "";
    if (const srt::RaysStatus rs = srt::probe_classify_check(ctx->probe_grid, ctx->probes.directions.count(), ctx->scene_set, call, &why))
        return fail(ctx, (int)rs, "srt_classify_probes: %s (clearance %g, max_offset %g, steps %u, flags 0x%x, outputs 0x%x, reserved %u)", why, (double)t->clearance,
                    (double)t->max_offset, t->steps, t->flags, t->outputs, t->reserved);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const srt::ProbeGrid& g = ctx->probe_grid.grid;
    const size_t np = srt::probe_grid_probes(g);
    const bool count = (t->flags & SRT_PROBE_CLASSIFY_COUNT_WORK) != 0, relocate = (t->flags & SRT_PROBE_CLASSIFY_RELOCATE) != 0;
    if (const int rc = probe_table_current(ctx)) return rc;
    void* dst[srt::PROBE_STATE_SLOTS] = {nullptr, nullptr};
    for (int i = 0; i < srt::PROBE_STATE_SLOTS; ++i)
        if (t->outputs & (1u << i))
            SRT_WRITE_TARGET_AFTER(ctx, ctx->probe_states_out[i], ctx->d_probe_states_own[i], srt::probe_state_bytes(np), dst[i],
                                   output_released(ctx, ctx->probe_states.last, i, ctx->d_probe_states_own[i]));
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_probe_classify_work)) return rc;
    }
    const srt::ProbeTable& T = ctx->probe_table;
    const bool in_lds = T.vec4() <= (size_t)srt::PS_TABLE_LDS_VEC4;
    const size_t lds_bytes = in_lds ? T.vec4() * sizeof(float4) : 0;
    void (*const kernel)(srt::ProbeClassifyIO) = SRT_KERNEL(srt::probe_classify_kernel, in_lds, count);
    const unsigned wgs = srt::probe_classify_grid(np, srt::OUT_WG_UNITS, resident_workgroups(ctx, (const void*)kernel, lds_bytes));
    srt::ProbeClassifyIO io{};
    io.table = (const float4*)ctx->d_probe_table;
    io.spheres = T.spheres, io.boxes = T.boxes;
    if (relocate) {
        io.direction = current(ctx->probes.directions, ctx->d_probe_direction);
        io.directions = (uint32_t)ctx->probes.directions.count();
    }
    io.probes = (uint32_t)np;
    for (int a = 0; a < 3; ++a) io.origin[a] = g.origin[a], io.spacing[a] = g.spacing[a], io.counts[a] = g.counts[a];
    io.clearance = t->clearance, io.max_offset = t->max_offset, io.steps = t->steps;
    io.relocate = relocate ? 1u : 0u, io.normalize = (t->flags & SRT_PROBE_CLASSIFY_NORMALIZE) ? 1u : 0u, io.has_mesh = T.has_mesh ? 1u : 0u;
    io.records = (float4*)dst[0];
    io.positions = (float4*)dst[1];
    io.work = count ? (unsigned long long*)ctx->d_probe_classify_work : nullptr;
    hipLaunchKernelGGL(kernel, dim3(wgs), dim3(srt::WG_THREADS), lds_bytes, ctx->stream, io);
    SRT_HIP(ctx, hipGetLastError());
    srt::probe_states_classified(ctx->probe_states, np, call, dst);
    return SRT_OK;
}

int srt_bind_probe_states_output(srt_context* ctx, uint32_t output, void* d_ptr) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return bind_output(ctx, ctx->probe_states_out, srt::probe_state_slot(output), d_ptr,
                       "srt_bind_probe_states_output: output 0x%x is not a single SRT_PROBE_STATE_RECORDS / _POSITIONS bit", output);
}

int srt_read_probe_states_output(srt_context* ctx, uint32_t output, void* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    return read_output(ctx, ctx->probe_states.last, output, srt::probe_state_slot(output), dst, srt::probe_state_bytes(ctx->probe_states.last_probes),
                       "srt_read_probe_states_output: output 0x%x is not a single SRT_PROBE_STATE_RECORDS / _POSITIONS bit",
                       "srt_read_probe_states_output: output 0x%x was not written by the last srt_classify_probes");
}

SRT_WORK_LAYOUT(srt_probe_classify_work, srt::PS_WORK_N, probes, srt::PS_WORK_PROBES, waves, srt::PS_WORK_WAVES);
int srt_get_probe_classify_work(srt_context* ctx, srt_probe_classify_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->probe_states.call, ctx->d_probe_classify_work, out,
                    "srt_get_probe_classify_work: the last srt_classify_probes did not ask for SRT_PROBE_CLASSIFY_COUNT_WORK (or there has been none)");
}

// ---- probe-grid shading that obeys the probe states ---------------------------------------------------------------------
int srt_write_probe_grid_states(srt_context* ctx, const float* records, size_t probes) {
    if (!ctx || !records) return SRT_ERR_INVALID_ARG;
    if (probes < 1 || probes > srt::PROBE_GRID_MAX_PROBES) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_write_probe_grid_states: %zu probes: want 1 .. 2^30", probes);
    return write_probe_input(ctx, ctx->probe_states.states, ctx->d_probe_grid_states, records, probes, sizeof(float4));
}

int srt_bind_probe_grid_states(srt_context* ctx, const void* d_ptr, size_t probes) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (srt::input_bind(ctx->probe_states.states, d_ptr, probes, srt::PROBE_GRID_MAX_PROBES) != srt::RAYS_OK)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_bind_probe_grid_states: want a device array and 1 .. 2^30 probes, or NULL, 0 (got %zu)", probes);
    return SRT_OK;
}

int srt_shade_probe_grid_states(srt_context* ctx, const srt_probe_grid_params* s, const srt_probe_grid_depth_params* d) {
    if (!ctx || !s) return SRT_ERR_INVALID_ARG;
    return shade_probe_grid(ctx, "srt_shade_probe_grid_states", s, d, PG_SHADE_STATES);
}

// ---- per-frame probe updates: the list, the histories and the blend (the two listed traces are with their parents) --------
static_assert(SRT_PROBE_LIST_COUNT_WORK == srt::PROBE_LIST_FLAG_COUNT_WORK && SRT_PROBE_LIST_HEADER == srt::PROBE_LIST_HEADER && srt::PL_HEADER == srt::PROBE_LIST_HEADER &&
              SRT_PROBE_HISTORY_COEFFICIENTS == srt::PROBE_HISTORY_COEFFICIENTS && SRT_PROBE_HISTORY_MOMENTS == srt::PROBE_HISTORY_MOMENTS &&
              SRT_PROBE_BLEND_MOMENTS == srt::PROBE_BLEND_FLAG_MOMENTS && SRT_PROBE_BLEND_LISTED == srt::PROBE_BLEND_FLAG_LISTED &&
              SRT_PROBE_BLEND_PREVIOUS_STATES == srt::PROBE_BLEND_FLAG_PREVIOUS_STATES && SRT_PROBE_BLEND_COUNT_WORK == srt::PROBE_BLEND_FLAG_COUNT_WORK &&
              sizeof(srt_probe_list_params) == 16 && sizeof(srt::ProbeListCall) == 16 && sizeof(srt_probe_list_work) == 32 && srt::PL_WORK_N == 3 &&
              sizeof(srt_probe_blend_params) == 24 && sizeof(srt::ProbeBlendCall) == 24 && sizeof(srt_probe_blend_work) == 40 && srt::PB_WORK_N == 4 &&
              (int)srt::PB_COEFFS == (int)srt::LIGHT_PROBE_COEFFS && (int)srt::LP_COEFFS == (int)srt::PB_COEFFS,
              "srt_probe_update_host.h, srt_probe_update.hip.h and srt_pathtrace.h disagree");

int srt_probe_list_params_default(srt_probe_list_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt::ProbeListCall c;
    srt::probe_list_call_default(c);
    memcpy(out, &c, sizeof c);
    return SRT_OK;
}

int srt_list_probes(srt_context* ctx, const srt_probe_list_params* t) {
    if (!ctx || !t) return SRT_ERR_INVALID_ARG;
    srt::ProbeListCall call;
    memcpy(&call, t, sizeof call);
    const char* why = "";
    if (const srt::RaysStatus rs = srt::probe_list_check(ctx->probe_grid, ctx->probe_states, ctx->scene_set, call, &why))
        return fail(ctx, (int)rs, "srt_list_probes: %s (skip_mask 0x%x, flags 0x%x, reserved %u %u)", why, t->skip_mask, t->flags, t->reserved[0], t->reserved[1]);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t np = ctx->probe_states.states.count();
    const bool count = (t->flags & SRT_PROBE_LIST_COUNT_WORK) != 0;
    uint32_t* dst = (uint32_t*)const_cast<void*>(ctx->probe_update.list_out_bound);
    if (!dst) {
        if (ctx->d_probe_list_out.bytes() < srt::probe_list_bytes(np)) {  // earlier listings may still be writing it, listed traces reading it
            if (const int rc = output_released(ctx, ctx->probe_update.list_last, 0, ctx->d_probe_list_out)) return rc;
            SRT_HIP(ctx, ctx->d_probe_list_out.ensure(srt::probe_list_bytes(np)));
        }
        dst = ctx->d_probe_list_out;
    }
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_probe_list_work)) return rc;
    }
    srt::ProbeListIO io{};
    io.states = current(ctx->probe_states.states, ctx->d_probe_grid_states);
    io.list = dst;
    io.probes = (uint32_t)np, io.skip_mask = t->skip_mask;
    io.work = count ? (unsigned long long*)ctx->d_probe_list_work : nullptr;
    hipLaunchKernelGGL(SRT_KERNEL(srt::probe_list_kernel, count), dim3(1), dim3(srt::WG_THREADS), 0, ctx->stream, io);
    SRT_HIP(ctx, hipGetLastError());
    srt::probe_list_listed(ctx->probe_update, np, t->flags, dst);
    return SRT_OK;
}

int srt_bind_probe_list_output(srt_context* ctx, void* d_list) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return ctx->probe_update.list_out_bound = d_list, SRT_OK;  // (no synchronisation: enqueued calls keep the buffer they were given, as srt_bind_probe_states_output)
}

int srt_read_probe_list_output(srt_context* ctx, uint32_t* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    return read_slot(ctx, ctx->probe_update.list_last.read(1u, 0), dst, srt::probe_list_bytes(ctx->probe_update.list_probes),
                     "srt_read_probe_list_output: there has been no srt_list_probes");
}

SRT_WORK_LAYOUT(srt_probe_list_work, srt::PL_WORK_N, probes, srt::PL_WORK_PROBES, waves, srt::PL_WORK_WAVES);
int srt_get_probe_list_work(srt_context* ctx, srt_probe_list_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->probe_update.list_call, ctx->d_probe_list_work, out,
                    "srt_get_probe_list_work: the last srt_list_probes did not ask for SRT_PROBE_LIST_COUNT_WORK (or there has been none)");
}

int srt_bind_probe_list(srt_context* ctx, const void* d_list, size_t capacity) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (srt::probe_list_bind(ctx->probe_update, d_list, capacity) != srt::RAYS_OK)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_bind_probe_list: want a device array and a capacity of 4 + (1 .. 2^30) words, or NULL, 0 (got %zu)", capacity);
    return SRT_OK;
}

int srt_write_probe_list(srt_context* ctx, const uint32_t* list, size_t capacity) {
    if (!ctx || !list) return SRT_ERR_INVALID_ARG;
    if (!srt::probe_list_capacity_ok(capacity)) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_write_probe_list: %zu words: want 4 + (1 .. 2^30)", capacity);
    return write_probe_input(ctx, ctx->probe_update.list, ctx->d_probe_list, list, capacity, sizeof(uint32_t));
}

int srt_probe_blend_params_default(srt_probe_blend_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt::ProbeBlendCall c;
    srt::probe_blend_call_default(c);
    memcpy(out, &c, sizeof c);
    return SRT_OK;
}

// the history of slot i: the bound buffer, else the own one
static float4* current_probe_history(const srt_context* ctx, int i) {
    const void* b = ctx->probe_update.history[i].bound;
    return b ? (float4*)const_cast<void*>(b) : (float4*)ctx->d_probe_history[i];
}

int srt_reset_probe_history(srt_context* ctx, uint32_t which, size_t probes, uint32_t resolution) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    const char* why = "";
    if (const srt::RaysStatus rs = srt::probe_history_check_reset(which, probes, resolution, &why))
        return fail(ctx, (int)rs, "srt_reset_probe_history: %s (which 0x%x, probes %zu, resolution %u)", why, which, probes, resolution);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < srt::PROBE_HISTORY_SLOTS; ++i) {
        if (!(which & (1u << i))) continue;
        const size_t bytes = srt::probe_history_bytes(i, probes, resolution);
        if (!ctx->probe_update.history[i].bound && ctx->d_probe_history[i].bytes() < bytes) {  // earlier blends and shading calls may still use it
            if (const int rc = finish_stream(ctx)) return rc;
            srt::probe_history_lost(ctx->probe_update, i);
            SRT_HIP(ctx, ctx->d_probe_history[i].ensure(bytes));
        }
        SRT_HIP(ctx, hipMemsetAsync(current_probe_history(ctx, i), 0, bytes, ctx->stream));
        srt::probe_history_was_reset(ctx->probe_update, i, probes, resolution);
    }
    return SRT_OK;
}

int srt_bind_probe_history(srt_context* ctx, uint32_t which, void* d_ptr) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    const int i = srt::probe_history_slot(which);
    if (i < 0) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_bind_probe_history: which 0x%x is not a single SRT_PROBE_HISTORY_COEFFICIENTS / _MOMENTS bit", which);
    return ctx->probe_update.history[i].bound = d_ptr, SRT_OK;  // (no synchronisation: enqueued calls keep the buffer they were given)
}

int srt_read_probe_history(srt_context* ctx, uint32_t which, float* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    int i = -1;
    size_t bytes = 0;
    const srt::RaysStatus rs = srt::probe_history_check_read(ctx->probe_update, which, &i, &bytes);
    if (rs == srt::RAYS_INVALID_ARG)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_read_probe_history: which 0x%x is not a single SRT_PROBE_HISTORY_COEFFICIENTS / _MOMENTS bit", which);
    const float4* src = rs == srt::RAYS_OK ? current_probe_history(ctx, i) : nullptr;
    if (src && !ctx->probe_update.history[i].bound && ctx->d_probe_history[i].bytes() < bytes) src = nullptr;  // (unbound after the reset: the own buffer is not that history)
    return read_slot(ctx, src, dst, bytes, "srt_read_probe_history: history 0x%x has not been reset (srt_reset_probe_history)", which);
}

int srt_write_probe_previous_states(srt_context* ctx, const float* records, size_t probes) {
    if (!ctx || !records) return SRT_ERR_INVALID_ARG;
    return write_light_probe_input(ctx, ctx->probe_update.previous, ctx->d_probe_previous_states, records, probes, srt::PROBE_GRID_MAX_PROBES, "srt_write_probe_previous_states");
}

int srt_bind_probe_previous_states(srt_context* ctx, const void* d_ptr, size_t probes) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (srt::input_bind(ctx->probe_update.previous, d_ptr, probes, srt::PROBE_GRID_MAX_PROBES) != srt::RAYS_OK)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_bind_probe_previous_states: want a device array and 1 .. 2^30 probes, or NULL, 0 (got %zu)", probes);
    return SRT_OK;
}

int srt_blend_probes(srt_context* ctx, const srt_probe_blend_params* t) {
    if (!ctx || !t) return SRT_ERR_INVALID_ARG;
    srt::ProbeBlendCall call;
    memcpy(&call, t, sizeof call);
    const char* why = "";
    if (const srt::RaysStatus rs = srt::probe_blend_check(ctx->probe_update, ctx->probes, ctx->probe_depth, ctx->probe_states, ctx->scene_set, call, &why))
        return fail(ctx, (int)rs, "srt_blend_probes: %s (hysteresis %g, fast_hysteresis %g, depth_hysteresis %g, change_threshold %g, flags 0x%x, reserved %u)", why,
                    (double)t->hysteresis, (double)t->fast_hysteresis, (double)t->depth_hysteresis, (double)t->change_threshold, t->flags, t->reserved);
    const bool moments = (t->flags & SRT_PROBE_BLEND_MOMENTS) != 0, listed = (t->flags & SRT_PROBE_BLEND_LISTED) != 0;
    const bool prev = (t->flags & SRT_PROBE_BLEND_PREVIOUS_STATES) != 0, count = (t->flags & SRT_PROBE_BLEND_COUNT_WORK) != 0;
    const size_t np = ctx->probe_update.history[0].probes;
    const uint32_t R = moments ? ctx->probe_update.history[1].resolution : 0u;
    // (a history unbound after its reset may have no own buffer of that size: the one case the rules cannot see)
    for (int i = 0; i < (moments ? 2 : 1); ++i)
        if (!ctx->probe_update.history[i].bound && ctx->d_probe_history[i].bytes() < srt::probe_history_bytes(i, np, R))
            return fail(ctx, SRT_ERR_STATE, "srt_blend_probes: history 0x%x was unbound after its reset (srt_reset_probe_history)", 1u << i);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_probe_blend_work)) return rc;
    }
    srt::ProbeBlendIO io{};
    io.history = current_probe_history(ctx, 0);
    io.fresh = (const float4*)ctx->probes.last.dst[0];
    if (moments) io.depth_history = current_probe_history(ctx, 1), io.depth_fresh = (const float4*)ctx->probe_depth.last.dst[0];
    io.list = listed ? current_probe_list(ctx) : nullptr;
    if (prev) {
        io.states = current(ctx->probe_states.states, ctx->d_probe_grid_states);
        io.previous = current(ctx->probe_update.previous, ctx->d_probe_previous_states);
    }
    io.probes = (uint32_t)np, io.texels = R * R;
    io.hysteresis = t->hysteresis, io.fast_hysteresis = t->fast_hysteresis, io.depth_hysteresis = t->depth_hysteresis, io.change_threshold = t->change_threshold;
    io.work = count ? (unsigned long long*)ctx->d_probe_blend_work : nullptr;
    void (*const kernel)(srt::ProbeBlendIO) = SRT_KERNEL(srt::probe_blend_kernel, listed, prev, count);
    const unsigned wgs = srt::probe_blend_grid(np, srt::OUT_WG_UNITS, resident_workgroups(ctx, (const void*)kernel, 0));
    hipLaunchKernelGGL(kernel, dim3(wgs), dim3(srt::WG_THREADS), 0, ctx->stream, io);
    SRT_HIP(ctx, hipGetLastError());
    srt::probe_blend_blended(ctx->probe_update, t->flags);
    return SRT_OK;
}

SRT_WORK_LAYOUT(srt_probe_blend_work, srt::PB_WORK_N, probes, srt::PB_WORK_PROBES, waves, srt::PB_WORK_WAVES);
int srt_get_probe_blend_work(srt_context* ctx, srt_probe_blend_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->probe_update.blend_call, ctx->d_probe_blend_work, out,
                    "srt_get_probe_blend_work: the last srt_blend_probes did not ask for SRT_PROBE_BLEND_COUNT_WORK (or there has been none)");
}

// ---- scrolling probe grids -------------------------------------------------------------------------------------------
static_assert(SRT_PROBE_SCROLL_COEFFICIENTS == srt::PROBE_SCROLL_COEFFICIENTS && SRT_PROBE_SCROLL_MOMENTS == srt::PROBE_SCROLL_MOMENTS &&
              SRT_PROBE_SCROLL_STATES == srt::PROBE_SCROLL_STATES && SRT_PROBE_SCROLL_COEFFICIENTS == SRT_PROBE_HISTORY_COEFFICIENTS &&
              SRT_PROBE_SCROLL_MOMENTS == SRT_PROBE_HISTORY_MOMENTS && SRT_PROBE_SCROLL_COUNT_WORK == srt::PROBE_SCROLL_FLAG_COUNT_WORK &&
              SRT_PROBE_SCROLL_SET_GRID == srt::PROBE_SCROLL_FLAG_SET_GRID && sizeof(srt_probe_scroll_params) == 32 && sizeof(srt::ProbeScrollCall) == 32 &&
              sizeof(srt_probe_scroll_work) == 40 && srt::PSC_WORK_N == 4 && (int)srt::PSC_ARRAYS == (int)srt::PROBE_SCROLL_ARRAYS &&
              srt::PROBE_SCROLL_ARRAYS == srt::PROBE_HISTORY_SLOTS + 1,
              "srt_probe_scroll_host.h, srt_probe_scroll.hip.h and srt_pathtrace.h disagree");

int srt_probe_scroll_params_default(srt_probe_scroll_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt::ProbeScrollCall c;
    srt::probe_scroll_call_default(c);
    memcpy(out, &c, sizeof c);
    return SRT_OK;
}

int srt_probe_grid_follow(const srt_probe_grid* grid, const float point[3], int32_t shift[3]) {
    if (!grid || !point || !shift) return SRT_ERR_INVALID_ARG;
    const srt::ProbeGrid g = probe_grid_of(grid);
    if (srt::probe_grid_check(g, nullptr) != srt::RAYS_OK) return SRT_ERR_INVALID_ARG;
    srt::probe_grid_follow(g, point, shift);
    return SRT_OK;
}

int srt_scroll_probes(srt_context* ctx, const srt_probe_scroll_params* t) {
    if (!ctx || !t) return SRT_ERR_INVALID_ARG;
    srt::ProbeScrollCall call;
    memcpy(&call, t, sizeof call);
    const char* why = "";
    if (const srt::RaysStatus rs = srt::probe_scroll_check(ctx->probe_grid, ctx->probe_update, ctx->probe_states, ctx->scene_set, call, &why))
        return fail(ctx, (int)rs, "srt_scroll_probes: %s (shift %d %d %d, which 0x%x, flags 0x%x, reserved %u %u %u)", why, t->shift[0], t->shift[1], t->shift[2],
                    t->which, t->flags, t->reserved[0], t->reserved[1], t->reserved[2]);
    const srt::ProbeGrid& g = ctx->probe_grid.grid;
    const size_t np = srt::probe_grid_probes(g);
    const bool moving = !srt::probe_scroll_shift_is_zero(call.shift);
    const bool states = (t->which & SRT_PROBE_SCROLL_STATES) != 0, count = (t->flags & SRT_PROBE_SCROLL_COUNT_WORK) != 0;
    size_t bytes[srt::PROBE_HISTORY_SLOTS] = {0, 0};  // of the histories this call moves (a zero shift moves none)
    for (int i = 0; i < srt::PROBE_HISTORY_SLOTS; ++i) {
        if (!moving || !(t->which & (1u << i))) continue;
        bytes[i] = srt::probe_history_bytes(i, np, ctx->probe_update.history[i].resolution);
        // (a history unbound after its reset may have no own buffer of that size: the one case the rules cannot see)
        if (!ctx->probe_update.history[i].bound && ctx->d_probe_history[i].bytes() < bytes[i])
            return fail(ctx, SRT_ERR_STATE, "srt_scroll_probes: history 0x%x was unbound after its reset (srt_reset_probe_history)", 1u << i);
    }
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    // every buffer first: a failed allocation leaves the histories, the previous records and the grid as they were
    for (int i = 0; i < srt::PROBE_HISTORY_SLOTS; ++i)
        if (ctx->d_probe_history_spare[i].bytes() < bytes[i]) {  // an earlier scroll's copy back may still read it
            if (const int rc = finish_stream(ctx)) return rc;
            SRT_HIP(ctx, ctx->d_probe_history_spare[i].ensure(bytes[i]));
        }
    if (states && ctx->d_probe_previous_states.bytes() < np * sizeof(float4)) {  // earlier blends may still read it
        if (const int rc = finish_stream(ctx)) return rc;
        ctx->probe_update.previous.own_count = 0;  // (a failed allocation leaves no own array)
        SRT_HIP(ctx, ctx->d_probe_previous_states.ensure(np * sizeof(float4)));
    }
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_probe_scroll_work)) return rc;
    }
    srt::ProbeScrollIO io{};
    for (int i = 0; i < srt::PROBE_HISTORY_SLOTS; ++i) {
        if (bytes[i] == 0) continue;
        io.src[i] = (const uint4*)current_probe_history(ctx, i), io.dst[i] = (uint4*)(float4*)ctx->d_probe_history_spare[i];
        io.elems[i] = (uint32_t)(bytes[i] / np / sizeof(float4));
    }
    if (states) {
        io.src[2] = (const uint4*)current(ctx->probe_states.states, ctx->d_probe_grid_states), io.dst[2] = (uint4*)(float4*)ctx->d_probe_previous_states;
        io.elems[2] = 1u;
    }
    io.probes = (uint32_t)np;
    for (int a = 0; a < 3; ++a) io.counts[a] = g.counts[a], io.shift[a] = t->shift[a];
    io.work = count ? (unsigned long long*)ctx->d_probe_scroll_work : nullptr;
    if (io.dst[0] || io.dst[1] || io.dst[2] || count) {
        void (*const kernel)(srt::ProbeScrollIO) = SRT_KERNEL(srt::probe_scroll_kernel, count);
        const unsigned wgs = srt::probe_scroll_grid(np, srt::OUT_WG_UNITS, resident_workgroups(ctx, (const void*)kernel, 0));
        hipLaunchKernelGGL(kernel, dim3(wgs), dim3(srt::WG_THREADS), 0, ctx->stream, io);
        SRT_HIP(ctx, hipGetLastError());
    }
    for (int i = 0; i < srt::PROBE_HISTORY_SLOTS; ++i) {
        if (bytes[i] == 0) continue;
        if (ctx->probe_update.history[i].bound)
            SRT_HIP(ctx, hipMemcpyAsync(current_probe_history(ctx, i), ctx->d_probe_history_spare[i], bytes[i], hipMemcpyDeviceToDevice, ctx->stream));
        else
            ctx->d_probe_history[i].swap(ctx->d_probe_history_spare[i]);  // (enqueued launches keep the pointers they were given)
    }
    if (states) srt::input_written(ctx->probe_update.previous, np);
    if (t->flags & SRT_PROBE_SCROLL_SET_GRID) srt::probe_scroll_origin(g, call.shift, ctx->probe_grid.grid.origin);
    if (moving) srt::probe_scroll_stale(ctx->probes, ctx->probe_depth);
    srt::probe_scroll_scrolled(ctx->probe_scroll, t->flags);
    return SRT_OK;
}

int srt_read_probe_previous_states(srt_context* ctx, float* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    const size_t np = ctx->probe_update.previous.count();
    return read_slot(ctx, np ? current(ctx->probe_update.previous, ctx->d_probe_previous_states) : nullptr, dst, np * sizeof(float4),
                     "srt_read_probe_previous_states: no previous states have been written, bound or scrolled");
}

SRT_WORK_LAYOUT(srt_probe_scroll_work, srt::PSC_WORK_N, probes, srt::PSC_WORK_PROBES, waves, srt::PSC_WORK_WAVES);
int srt_get_probe_scroll_work(srt_context* ctx, srt_probe_scroll_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->probe_scroll, ctx->d_probe_scroll_work, out,
                    "srt_get_probe_scroll_work: the last srt_scroll_probes did not ask for SRT_PROBE_SCROLL_COUNT_WORK (or there has been none)");
}

// ---- probe cascade -------------------------------------------------------------------------------------------------
static_assert(SRT_PROBE_CASCADE_MAX_LEVELS == srt::PROBE_CASCADE_MAX_LEVELS && SRT_PROBE_CASCADE_MAX_LEVELS == srt::PC_LEVELS &&
              SRT_PROBE_CASCADE_NORMAL_WEIGHT == srt::PROBE_CASCADE_FLAG_NORMAL_WEIGHT && SRT_PROBE_CASCADE_DEPTH == srt::PROBE_CASCADE_FLAG_DEPTH &&
              SRT_PROBE_CASCADE_STATES == srt::PROBE_CASCADE_FLAG_STATES && SRT_PROBE_CASCADE_ALBEDO == srt::PROBE_CASCADE_FLAG_ALBEDO &&
              SRT_PROBE_CASCADE_COUNT_WORK == srt::PROBE_CASCADE_FLAG_COUNT_WORK && SRT_PROBE_CASCADE_COEFFICIENTS == srt::PROBE_CASCADE_COEFFICIENTS &&
              SRT_PROBE_CASCADE_MOMENTS == srt::PROBE_CASCADE_MOMENTS && SRT_PROBE_CASCADE_RECORDS == srt::PROBE_CASCADE_RECORDS &&
              sizeof(srt_probe_cascade) == 160 && sizeof(srt::ProbeCascade) == 160 && sizeof(srt_probe_cascade_params) == 40 && sizeof(srt::ProbeCascadeCall) == 40 &&
              sizeof(srt_probe_cascade_work) == 112 && srt::PC_WORK_N == 11 && sizeof(srt::ProbeCascadeLevel) == 64,
              "srt_probe_cascade_host.h, srt_probe_cascade.hip.h and srt_pathtrace.h disagree");

int srt_probe_cascade_params_default(srt_probe_cascade_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt::ProbeCascadeCall c;
    srt::probe_cascade_call_default(c);
    memcpy(out, &c, sizeof c);
    return SRT_OK;
}

int srt_probe_cascade_grids(const float centre[3], const float base_spacing[3], const int32_t counts[3], uint32_t levels, srt_probe_cascade* out) {
    if (!centre || !base_spacing || !counts || !out) return SRT_ERR_INVALID_ARG;
    srt::ProbeCascade c;
    if (srt::probe_cascade_grids(centre, base_spacing, counts, levels, c) != srt::RAYS_OK) return SRT_ERR_INVALID_ARG;
    memcpy(out, &c, sizeof c);
    return SRT_OK;
}

int srt_probe_cascade_weights(const srt_probe_cascade* cascade, const float point[3], int32_t* first_level, int32_t* evaluations, float* beta) {
    if (!cascade || !point || !first_level || !evaluations || !beta) return SRT_ERR_INVALID_ARG;
    srt::ProbeCascade c;
    memcpy(&c, cascade, sizeof c);
    if (srt::probe_cascade_check(c, nullptr) != srt::RAYS_OK) return SRT_ERR_INVALID_ARG;
    srt::probe_cascade_weights(c, point, first_level, evaluations, beta);
    return SRT_OK;
}

int srt_set_probe_cascade(srt_context* ctx, const srt_probe_cascade* cascade) {
    if (!ctx || !cascade) return SRT_ERR_INVALID_ARG;
    srt::ProbeCascade c;
    memcpy(&c, cascade, sizeof c);
    const char* why = "";
    if (srt::probe_cascade_set(ctx->probe_cascade, c, &why) != srt::RAYS_OK)  // (an enqueued launch keeps the cascade it was given: a kernel argument)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_set_probe_cascade: %s (levels %u, resolution %u, blend_cells %g, reserved %u)", why, c.levels, c.resolution,
                    (double)c.blend_cells, c.reserved);
    return SRT_OK;
}

int srt_write_probe_cascade_level(srt_context* ctx, uint32_t level, uint32_t which, const float* src, size_t probes) {
    if (!ctx || !src) return SRT_ERR_INVALID_ARG;
    int slot = -1;
    const char* why = "";
    if (const srt::RaysStatus rs = srt::probe_cascade_check_level_array(ctx->probe_cascade, level, which, probes, &slot, &why))
        return fail(ctx, (int)rs, "srt_write_probe_cascade_level: %s (level %u, which 0x%x, %zu probes)", why, level, which, probes);
    return write_probe_input(ctx, ctx->probe_cascade.arrays[level][slot], ctx->d_probe_cascade[level][slot], src, probes,
                             srt::probe_cascade_probe_bytes(slot, ctx->probe_cascade.cascade.resolution));
}

int srt_bind_probe_cascade_level(srt_context* ctx, uint32_t level, uint32_t which, const void* d_ptr, size_t probes) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    int slot = -1;
    const char* why = "";
    const bool unbind = !d_ptr && probes == 0;
    if (const srt::RaysStatus rs = srt::probe_cascade_check_level_array(ctx->probe_cascade, level, which, unbind ? 1 : probes, &slot, &why))
        return fail(ctx, (int)rs, "srt_bind_probe_cascade_level: %s (level %u, which 0x%x, %zu probes)", why, level, which, probes);
    if (srt::input_bind(ctx->probe_cascade.arrays[level][slot], d_ptr, probes, srt::PROBE_GRID_MAX_PROBES) != srt::RAYS_OK)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_bind_probe_cascade_level: want a device array and 1 .. 2^30 probes, or NULL, 0 (got %zu)", probes);
    return SRT_OK;
}

int srt_capture_probe_cascade_level(srt_context* ctx, uint32_t level, uint32_t which_mask) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    const char* why = "";
    if (const srt::RaysStatus rs = srt::probe_cascade_check_capture(ctx->probe_cascade, level, which_mask, ctx->probe_grid, ctx->probe_grid_depth, ctx->probe_states, &why))
        return fail(ctx, (int)rs, "srt_capture_probe_cascade_level: %s (level %u, which 0x%x)", why, level, which_mask);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t np = srt::probe_grid_probes(ctx->probe_cascade.cascade.grid[level]);
    const float4* const src[srt::PROBE_CASCADE_ARRAYS] = {current(ctx->probe_grid.coefficients, ctx->d_probe_grid_coefficients),
                                                          current(ctx->probe_grid_depth.moments, ctx->d_probe_grid_depth),
                                                          current(ctx->probe_states.states, ctx->d_probe_grid_states)};
    for (int i = 0; i < srt::PROBE_CASCADE_ARRAYS; ++i) {
        if (!(which_mask & (1u << i))) continue;
        const size_t bytes = np * srt::probe_cascade_probe_bytes(i, ctx->probe_cascade.cascade.resolution);
        DeviceBuffer<float4>& own = ctx->d_probe_cascade[level][i];
        srt::InputArray& in = ctx->probe_cascade.arrays[level][i];
        if (own.bytes() < bytes) {
            if (const int rc = finish_stream(ctx)) return rc;  // (launches in flight read the own array; it is re-allocated below)
            in.own_count = 0;                                  // (a failed allocation leaves no own array)
            SRT_HIP(ctx, own.ensure(bytes));
        }
        SRT_HIP(ctx, hipMemcpyAsync(own, src[i], bytes, hipMemcpyDeviceToDevice, ctx->stream));
        srt::input_written(in, np);  // (a binding of that array ends)
    }
    return SRT_OK;
}

int srt_shade_probe_cascade(srt_context* ctx, const srt_probe_cascade_params* s) {
    if (!ctx || !s) return SRT_ERR_INVALID_ARG;
    srt::ProbeCascadeCall call;
    memcpy(&call, s, sizeof call);
    bool present[srt::PROBE_GRID_GUIDES];
    for (int i = 0; i < srt::PROBE_GRID_GUIDES; ++i) present[i] = current(ctx->gbuf[i], ctx->d_gbuf_own[i]) != nullptr;
    const char* why = "";
    if (const srt::RaysStatus rs = srt::probe_cascade_check_shade(ctx->probe_cascade, call, ctx->scene_set, ctx->height, present, &why))
        return fail(ctx, (int)rs, "srt_shade_probe_cascade: %s (rows [%d,%d) of %d, flags 0x%x, band_weight %g %g %g, bias %g, min_variance %g, reserved %u %u)", why,
                    s->row_begin, s->row_end, ctx->height, s->flags, (double)s->band_weight[0], (double)s->band_weight[1], (double)s->band_weight[2], (double)s->bias,
                    (double)s->min_variance, s->reserved[0], s->reserved[1]);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const bool count = (s->flags & SRT_PROBE_CASCADE_COUNT_WORK) != 0, depth = (s->flags & SRT_PROBE_CASCADE_DEPTH) != 0,
               states = (s->flags & SRT_PROBE_CASCADE_STATES) != 0;
    float4* dst = nullptr;
    SRT_WRITE_TARGET(ctx, ctx->probe_grid_out, ctx->d_probe_grid_own, frame_pixels(ctx) * sizeof(float4), dst);
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_probe_cascade_work)) return rc;
    }
    srt::KernelParams K;
    KernelSetup ks = scene_kernel_params(ctx, s->row_begin, s->row_end, K);
    ks.lds_bytes = 0;  // (the kernel traces nothing: no scene image, and its own LDS is static)
    void (*kernel)(srt::KernelParams, srt::ProbeCascadeIO) = SRT_KERNEL(srt::probe_cascade_kernel, depth, states, count);
    const srt::ProbeCascade& c = ctx->probe_cascade.cascade;
    srt::ProbeCascadeIO io{};
    io.object = (const int32_t*)current(ctx->gbuf[0], ctx->d_gbuf_own[0]);
    io.normal_depth = (const float4*)current(ctx->gbuf[1], ctx->d_gbuf_own[1]);
    io.position = (const float4*)current(ctx->gbuf[2], ctx->d_gbuf_own[2]);
    io.albedo = (s->flags & SRT_PROBE_CASCADE_ALBEDO) ? (const float4*)current(ctx->gbuf[3], ctx->d_gbuf_own[3]) : nullptr;
    io.out = dst;
    for (uint32_t l = 0; l < c.levels; ++l) {
        srt::ProbeCascadeLevel& lv = io.level[l];
        for (int a = 0; a < 3; ++a) lv.origin[a] = c.grid[l].origin[a], lv.spacing[a] = c.grid[l].spacing[a], lv.counts[a] = c.grid[l].counts[a];
        lv.coefficients = current(ctx->probe_cascade.arrays[l][0], ctx->d_probe_cascade[l][0]);
        lv.depth = depth ? current(ctx->probe_cascade.arrays[l][1], ctx->d_probe_cascade[l][1]) : nullptr;
        lv.states = states ? current(ctx->probe_cascade.arrays[l][2], ctx->d_probe_cascade[l][2]) : nullptr;
    }
    io.levels = c.levels, io.resolution = c.resolution, io.blend_cells = c.blend_cells;
    for (int b = 0; b < 3; ++b) io.band_weight[b] = s->band_weight[b];
    io.normal_weight = (s->flags & SRT_PROBE_CASCADE_NORMAL_WEIGHT) ? 1u : 0u;
    io.bias = s->bias, io.min_variance = s->min_variance;
    io.work = count ? (unsigned long long*)ctx->d_probe_cascade_work : nullptr;
    if (const int rc = launch_tiles(ctx, kernel, ks, K, io)) return rc;
    ctx->probe_grid_out.wrote(dst);
    srt::probe_cascade_shaded(ctx->probe_cascade, s->flags);
    return SRT_OK;
}

int srt_get_probe_cascade_work(srt_context* ctx, srt_probe_cascade_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    // (field by field, not get_work: the struct ends in spare[2], which the enum does not have)
    if (ctx->probe_cascade.call.work() != srt::RAYS_OK)
        return fail(ctx, SRT_ERR_STATE, "srt_get_probe_cascade_work: the last srt_shade_probe_cascade did not ask for SRT_PROBE_CASCADE_COUNT_WORK (or there has been none)");
    unsigned long long w[srt::PC_WORK_N];
    if (const int rc = read_work(ctx, ctx->d_probe_cascade_work, w)) return rc;
    out->valid = 1, out->reserved = 0, out->spare[0] = 0, out->spare[1] = 0;
    out->pixels = w[srt::PC_WORK_PIXELS], out->evaluations = w[srt::PC_WORK_EVALUATIONS], out->blended = w[srt::PC_WORK_BLENDED];
    for (int k = 0; k < SRT_PROBE_CASCADE_MAX_LEVELS; ++k) out->first_level[k] = w[srt::PC_WORK_FIRST0 + k];
    out->corners = w[srt::PC_WORK_CORNERS], out->open = w[srt::PC_WORK_OPEN], out->wave_trips = w[srt::PC_WORK_TRIPS], out->waves = w[srt::PC_WORK_WAVES];
    return SRT_OK;
}

// ---- adaptive sampling ---------------------------------------------------------------------------------------------
static_assert(SRT_ADAPTIVE_KEEP_COUNTS == srt::ADAPTIVE_FLAG_KEEP_COUNTS && SRT_ADAPTIVE_COUNT_WORK == srt::ADAPTIVE_FLAG_COUNT_WORK &&
              SRT_ADAPTIVE_SUN_SAMPLING == srt::ADAPTIVE_FLAG_SUN_SAMPLING && !(srt::ADAPTIVE_FLAG_ALL & srt::ADAPTIVE_FLAG_SUN_SAMPLING) &&
              SRT_BUDGET_ALBEDO == srt::BUDGET_FLAG_ALBEDO && sizeof(srt_adaptive_params) == 28 && sizeof(srt::AdaptiveCall) == 28 &&
              sizeof(srt_budget_params) == 16 && sizeof(srt::BudgetCall) == 16 && sizeof(srt_adaptive_work) == 40 &&
              srt::ADP_FRAME_LIMIT == srt::ADAPTIVE_FRAME_LIMIT && (int)srt::ADP_WORK_N == (int)srt::RAD_WORK_N,
              "srt_adaptive_host.h, srt_adaptive.hip.h and srt_pathtrace.h disagree");

// The counts or the budget as a write target: the bound buffer, else the own one, allocated on first use.
static int sample_buffer_target(srt_context* ctx, srt::OutputSlot& slot, DeviceBuffer<uint32_t>& own, uint32_t*& dst) {
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    SRT_WRITE_TARGET(ctx, slot, own, frame_pixels(ctx) * sizeof(uint32_t), dst);
    return SRT_OK;
}

static int write_sample_buffer(srt_context* ctx, srt::OutputSlot& slot, DeviceBuffer<uint32_t>& own, const uint32_t* src) {
    if (const int rc = finish_stream(ctx)) return rc;
    uint32_t* dst = nullptr;
    if (const int rc = sample_buffer_target(ctx, slot, own, dst)) return rc;
    SRT_HIP(ctx, hipMemcpy(dst, src, frame_pixels(ctx) * sizeof(uint32_t), hipMemcpyHostToDevice));
    slot.wrote(dst);
    return SRT_OK;
}

int srt_set_sample_counts(srt_context* ctx, uint32_t value) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    uint32_t* dst = nullptr;
    if (const int rc = sample_buffer_target(ctx, ctx->counts, ctx->d_counts_own, dst)) return rc;
    SRT_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)dst, (int)value, frame_pixels(ctx), ctx->stream));
    ctx->counts.wrote(dst);
    return SRT_OK;
}

int srt_write_sample_counts(srt_context* ctx, const uint32_t* src) {
    if (!ctx || !src) return SRT_ERR_INVALID_ARG;
    return write_sample_buffer(ctx, ctx->counts, ctx->d_counts_own, src);
}

int srt_read_sample_counts(srt_context* ctx, uint32_t* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    return read_slot(ctx, current(ctx->counts, ctx->d_counts_own), dst, frame_pixels(ctx) * sizeof(uint32_t),
                     "srt_read_sample_counts: the sample counts have never been written, filled or bound");
}

int srt_bind_sample_counts(srt_context* ctx, void* d_u32) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return ctx->counts.bind(d_u32), SRT_OK;  // (no synchronisation: an enqueued call keeps the buffer it was given)
}

int srt_write_sample_budget(srt_context* ctx, const uint32_t* src) {
    if (!ctx || !src) return SRT_ERR_INVALID_ARG;
    return write_sample_buffer(ctx, ctx->budget, ctx->d_budget_own, src);
}

int srt_read_sample_budget(srt_context* ctx, uint32_t* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    return read_slot(ctx, current(ctx->budget, ctx->d_budget_own), dst, frame_pixels(ctx) * sizeof(uint32_t),
                     "srt_read_sample_budget: the sample budget has never been written or bound");
}

int srt_bind_sample_budget(srt_context* ctx, void* d_u32) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return ctx->budget.bind(d_u32), SRT_OK;  // (no synchronisation: an enqueued call keeps the buffer it was given)
}

int srt_adaptive_params_default(srt_adaptive_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt::AdaptiveCall c;
    srt::adaptive_call_default(c);
    out->row_begin = c.row_begin, out->row_end = c.row_end, out->max_bounces = c.max_bounces, out->seed = c.seed;
    out->max_samples = c.max_samples, out->flags = c.flags, out->reserved = c.reserved;
    return SRT_OK;
}

// The launch of srt_render_adaptive and srt_render_adaptive_tail once the call is accepted: `choice` (srt_adaptive_sun_host.h)
// picks one of the four adaptive kernels; a TAIL kernel gets the tail's inputs as they stand now, a SUN kernel the frame of the
// environment as it stands now.  ADAPTIVE_KERNEL_PLAIN is srt_render_adaptive's launch without the flag.
static int launch_adaptive(srt_context* ctx, const srt_adaptive_params* a, uint32_t* counts, const uint32_t* budget, srt::AdaptiveKernelChoice choice) {
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const bool count = (a->flags & SRT_ADAPTIVE_COUNT_WORK) != 0;
    srt::KernelParams K;
    const KernelSetup ks = scene_kernel_params(ctx, a->row_begin, a->row_end, K);
    // (the fields the bounce loop and store_pixel read; the frames are per pixel)
    K.max_bounces = a->max_bounces, K.seed = a->seed;
    K.accumulator = ctx->d_acc, K.framebuffer = ctx->d_fb;
    const auto kernel = SRT_KERNEL(srt::adaptive_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0, count);
    const auto tail_kernel = SRT_KERNEL(srt::adaptive_tail_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0);
    const auto sun_kernel = SRT_KERNEL(srt::adaptive_sun_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0);
    const auto tail_sun_kernel = SRT_KERNEL(srt::adaptive_tail_sun_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0);
    // the grid first, by the kernel that runs: the sample scratch is sized by it
    const void* const runs = choice == srt::ADAPTIVE_KERNEL_TAIL_SUN ? (const void*)tail_sun_kernel
                             : choice == srt::ADAPTIVE_KERNEL_SUN    ? (const void*)sun_kernel
                             : choice == srt::ADAPTIVE_KERNEL_TAIL   ? (const void*)tail_kernel
                                                                     : (const void*)kernel;
    const unsigned wgs = srt::adaptive_grid(K.width, K.rows, srt::OUT_WG_UNITS, resident_workgroups(ctx, runs, ks.lds_bytes));
    if (const int rc = ensure_sample_rows(ctx, wgs)) return rc;
    if (!ctx->d_adaptive_ticket) SRT_HIP(ctx, ctx->d_adaptive_ticket.ensure(sizeof(uint32_t)));
    SRT_HIP(ctx, hipMemsetAsync(ctx->d_adaptive_ticket, 0, sizeof(uint32_t), ctx->stream));
    if (count) {
        if (const int rc = zero_work(ctx, ctx->d_adaptive_work)) return rc;
    }
    srt::AdaptiveIO io{};
    io.budget = budget;
    io.counts = counts;
    io.max_samples = a->max_samples;
    io.keep_counts = (a->flags & SRT_ADAPTIVE_KEEP_COUNTS) ? 1u : 0u;
    io.ticket = ctx->d_adaptive_ticket;
    io.rows = ctx->d_radiance_rows;
    io.work = count ? (unsigned long long*)ctx->d_adaptive_work : nullptr;
    if (const int rc = choice == srt::ADAPTIVE_KERNEL_TAIL_SUN ? launch_persistent_tail_sun(ctx, tail_sun_kernel, wgs, ks, K, io, probe_tail_io(ctx), sun_io(ctx))
                       : choice == srt::ADAPTIVE_KERNEL_SUN    ? launch_persistent_sun(ctx, sun_kernel, wgs, ks, K, io, sun_io(ctx))
                       : choice == srt::ADAPTIVE_KERNEL_TAIL   ? launch_persistent_tail(ctx, tail_kernel, wgs, ks, K, io, probe_tail_io(ctx))
                                                               : launch_persistent(ctx, kernel, wgs, ks, K, io))
        return rc;
    if (!io.keep_counts) ctx->counts.wrote(counts);
    return SRT_OK;
}

int srt_render_adaptive(srt_context* ctx, const srt_adaptive_params* a) {
    if (!ctx || !a) return SRT_ERR_INVALID_ARG;
    const srt::AdaptiveCall call{a->row_begin, a->row_end, a->max_bounces, a->seed, a->max_samples, a->flags, a->reserved};
    uint32_t* const counts = current(ctx->counts, ctx->d_counts_own);
    const uint32_t* const budget = current(ctx->budget, ctx->d_budget_own);
    const char* why = "";
    // (AS5: the own errors with the bit taken out, then the sun's direction)
    if (const srt::RaysStatus rs = srt::sun_adaptive_check(call, ctx->scene_set, ctx->camera.set, ctx->height, counts != nullptr, budget != nullptr,
                                                           ctx->env.sun_direction, &why))
        return fail(ctx, (int)rs, "srt_render_adaptive: %s (rows [%d,%d) of %d, max_bounces %d, max_samples %u, flags 0x%x, reserved %u)", why, a->row_begin,
                    a->row_end, ctx->height, a->max_bounces, a->max_samples, a->flags, a->reserved);
    if (const int rc = launch_adaptive(ctx, a, counts, budget, srt::adaptive_kernel_choice(false, ctx->probe_tail, call))) return rc;
    srt::adaptive_rendered(ctx->adaptive, a->flags);
    return SRT_OK;
}

// srt_render_adaptive under srt_probe_tail: rules R1 - R7 of srt_pathtrace.h; the order of the checks, which kernel runs and what
// the call leaves behind are srt_adaptive_tail_host.h's
int srt_render_adaptive_tail(srt_context* ctx, const srt_adaptive_params* a) {
    if (!ctx || !a) return SRT_ERR_INVALID_ARG;
    const srt::AdaptiveCall call{a->row_begin, a->row_end, a->max_bounces, a->seed, a->max_samples, a->flags, a->reserved};
    uint32_t* const counts = current(ctx->counts, ctx->d_counts_own);
    const uint32_t* const budget = current(ctx->budget, ctx->d_budget_own);
    const char* why = "";
    // (AS5: all of R1 with the bit taken out, then the sun's direction)
    if (const srt::RaysStatus rs = srt::sun_adaptive_tail_check(call, ctx->scene_set, ctx->camera.set, ctx->height, counts != nullptr, budget != nullptr, ctx->probe_tail,
                                                                ctx->probe_grid, ctx->probe_grid_depth, ctx->probe_states,
                                                                current(ctx->probe_grid.coefficients, ctx->d_probe_grid_coefficients),
                                                                srt::adaptive_tail_targets(ctx->d_acc, ctx->d_fb, ctx->width, ctx->height), ctx->env.sun_direction, &why))
        return fail(ctx, (int)rs, "srt_render_adaptive_tail: %s (rows [%d,%d) of %d, max_bounces %d, max_samples %u, flags 0x%x, reserved %u)", why, a->row_begin,
                    a->row_end, ctx->height, a->max_bounces, a->max_samples, a->flags, a->reserved);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    if (const int rc = zero_probe_tail_work(ctx)) return rc;
    if (const int rc = launch_adaptive(ctx, a, counts, budget, srt::adaptive_kernel_choice(true, ctx->probe_tail, call))) return rc;
    srt::adaptive_tail_rendered(ctx->adaptive, ctx->probe_tail, a->flags);
    return SRT_OK;
}

SRT_WORK_LAYOUT(srt_adaptive_work, srt::ADP_WORK_N, pixels, srt::ADP_WORK_PIXELS, wave_calls, srt::ADP_WORK_WAVE_CALLS);
int srt_get_adaptive_work(srt_context* ctx, srt_adaptive_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->adaptive.call, ctx->d_adaptive_work, out,
                    "srt_get_adaptive_work: the last srt_render_adaptive did not ask for SRT_ADAPTIVE_COUNT_WORK (or there has been none)");
}

int srt_budget_params_default(srt_budget_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt::BudgetCall c;
    srt::budget_call_default(c);
    out->threshold = c.threshold, out->floor = c.floor, out->max_budget = c.max_budget, out->flags = c.flags;
    return SRT_OK;
}

int srt_sample_budget(srt_context* ctx, const srt_budget_params* b) {
    if (!ctx || !b) return SRT_ERR_INVALID_ARG;
    const srt::BudgetCall call{b->threshold, b->floor, b->max_budget, b->flags};
    const bool demod = (b->flags & SRT_BUDGET_ALBEDO) != 0;
    const int32_t* const object = (const int32_t*)current(ctx->gbuf[0], ctx->d_gbuf_own[0]);
    const float4* const albedo = (const float4*)current(ctx->gbuf[3], ctx->d_gbuf_own[3]);
    const float* const var = ctx->var.bound ? (const float*)ctx->var.bound : ctx->var_own_written ? (float*)ctx->d_var_own : nullptr;
    const uint32_t* const counts = current(ctx->counts, ctx->d_counts_own);
    const char* why = "";
    if (const srt::RaysStatus rs = srt::budget_check(call, object != nullptr, albedo != nullptr, var != nullptr, !ctx->var.bound, ctx->var_own_albedo,
                                                     counts != nullptr, &why))
        return fail(ctx, (int)rs, "srt_sample_budget: %s (threshold %g, floor %g, max_budget %u, flags 0x%x)", why, (double)b->threshold, (double)b->floor,
                    b->max_budget, b->flags);
    srt::BudgetLaunch L{};
    if (const int rc = sample_buffer_target(ctx, ctx->budget, ctx->d_budget_own, L.budget)) return rc;
    if (const int rc = zero_work(ctx, ctx->d_budget_total)) return rc;
    L.variance = var, L.counts = counts, L.acc = ctx->d_acc, L.object = object, L.albedo = demod ? albedo : nullptr;
    L.total = ctx->d_budget_total;
    L.width = ctx->width, L.height = ctx->height;
    L.threshold = b->threshold, L.floor = b->floor, L.max_budget = b->max_budget;
    hipLaunchKernelGGL(srt::budget_kernel, frame_tile_grid(ctx), dim3(srt::WG_THREADS), 0, ctx->stream, L);
    SRT_HIP(ctx, hipGetLastError());
    ctx->budget.wrote(L.budget);
    ctx->adaptive.budgeted = true;
    return SRT_OK;
}

int srt_get_budget_total(srt_context* ctx, uint64_t* total) {
    if (!ctx || !total) return SRT_ERR_INVALID_ARG;
    if (srt::budget_check_total(ctx->adaptive) != srt::RAYS_OK) return fail(ctx, SRT_ERR_STATE, "srt_get_budget_total: there has been no srt_sample_budget");
    unsigned long long w = 0ull;
    if (const int rc = read_work(ctx, ctx->d_budget_total, &w)) return rc;
    *total = w;
    return SRT_OK;
}

// ---- denoiser ------------------------------------------------------------------------------------------------------
int srt_denoise_params_default(srt_denoise_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    // chosen by tools/denoise_time.py --sweep on Scene1 and Scene_indirect
    out->iterations = 4;
    out->sigma_color = 0.0f;
    out->sigma_normal = 32.0f;
    out->sigma_plane = 0.02f;
    out->flags = SRT_DENOISE_ALBEDO;
    return SRT_OK;
}

// The à-trous levels of srt_denoise (variance NULL: the colour stop of sigma_color) and srt_denoise_variance (the luminance stop of
// sigma_luminance over `variance`), after their checks: `guide` is what find_guides gave (ALBEDO with SRT_DENOISE_ALBEDO).
static int atrous_filter(srt_context* ctx, const void* const* guide, int iterations, uint32_t flags, float sigma_normal, float sigma_plane,
                         float sigma_color, float sigma_luminance, const float* variance) {
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    float4* out = nullptr;
    const size_t px = frame_pixels(ctx);
    SRT_WRITE_TARGET(ctx, ctx->dn, ctx->d_dn_own, px * sizeof(float4), out);
    SRT_HIP(ctx, ctx->d_dn_tmp.ensure(px * sizeof(float4)));
    srt::AtrousLevel L{};
    L.acc = ctx->d_acc;
    L.object = (const int32_t*)guide[0];
    L.normal_depth = (const float4*)guide[1];
    L.position = (const float4*)guide[2];
    L.albedo = (flags & SRT_DENOISE_ALBEDO) ? (const float4*)guide[3] : nullptr;
    L.variance = variance;
    L.width = ctx->width, L.height = ctx->height;
    // an infinite exponent becomes FLT_MAX: the same 0 for n_p.n_q < 1 and inf above 1, and 1 (FLT_MAX * log2 1 = 0, where
    // inf * 0 would be NaN) for an exact n_p.n_q == 1, as on one face of a box
    L.sigma_normal = fminf(sigma_normal, FLT_MAX);
    // ... and so does an infinite sigma_plane: FLT_MAX * d_p is 0 for a first hit at d_p = 0, where inf * 0 would be NaN and
    // turn every weight of the pixel, exact ties included, into NaN; for every other d_p the weights keep their bits
    L.sigma_plane = fminf(sigma_plane, FLT_MAX);
    // ... and sigma_luminance: FLT_MAX * sqrt(0) = 0 closes the stop on a zero variance, where inf * 0 would be NaN
    L.sigma_luminance = fminf(sigma_luminance, FLT_MAX);
    // [stop][last]: srt_denoise has the colour stop; srt_denoise_variance the luminance stop, or none with sigma_luminance = 0
    using Kernel = void (*)(srt::AtrousLevel);
    static const Kernel kernels[3][2] = {{srt::atrous_kernel<false, srt::STOP_COLOR>, srt::atrous_kernel<true, srt::STOP_COLOR>},
                                         {srt::atrous_kernel<false, srt::STOP_LUMINANCE>, srt::atrous_kernel<true, srt::STOP_LUMINANCE>},
                                         {srt::atrous_kernel<false, srt::STOP_NONE>, srt::atrous_kernel<true, srt::STOP_NONE>}};
    const Kernel* const level = kernels[!variance ? srt::STOP_COLOR : sigma_luminance > 0.0f ? srt::STOP_LUMINANCE : srt::STOP_NONE];
    const dim3 grid = frame_tile_grid(ctx), block(srt::WG_THREADS);
    // the preparation pass and the levels alternate between the ping-pong buffer and the result buffer so that the last
    // level lands in the result
    const int n = iterations;
    L.dst = (n & 1) ? ctx->d_dn_tmp : out;
    hipLaunchKernelGGL(srt::atrous_prep_kernel, grid, block, 0, ctx->stream, L);
    SRT_HIP(ctx, hipGetLastError());
    for (int i = 0; i < n; ++i) {
        const bool last = i == n - 1;
        L.src = L.dst;
        L.dst = ((n - 1 - i) & 1) ? ctx->d_dn_tmp : out;
        L.step = 1 << i;
        // any sigma_color > 0 keeps the term on at every level; a reciprocal past FLT_MAX (sigma_color * 2^-i below about
        // 5.4e-20, or rounded to 0) stops there, so an exact tie c_p == c_q keeps its weight 1 (0 * inf would be NaN)
        const float sc = sigma_color * ldexpf(1.0f, -i);
        L.color_scale = sigma_color > 0.0f ? fminf(1.0f / (sc * sc), FLT_MAX) : 0.0f;
        L.framebuffer = last && (flags & SRT_DENOISE_FRAMEBUFFER) ? ctx->d_fb : nullptr;
        hipLaunchKernelGGL(level[last], grid, block, 0, ctx->stream, L);
        SRT_HIP(ctx, hipGetLastError());
    }
    ctx->dn.wrote(out);
    return SRT_OK;
}

int srt_denoise(srt_context* ctx, const srt_denoise_params* d) {
    if (!ctx || !d) return SRT_ERR_INVALID_ARG;
    if (d->iterations < 1 || d->iterations > 8)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_denoise: iterations %d outside 1..8", d->iterations);
    // (written so that a NaN fails too)
    if (!(d->sigma_color >= 0.0f) || !(d->sigma_normal >= 0.0f) || !(d->sigma_plane >= 0.0f))
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_denoise: sigmas must be >= 0 (color %g, normal %g, plane %g)", d->sigma_color,
                    d->sigma_normal, d->sigma_plane);
    if (d->flags & ~(SRT_DENOISE_ALBEDO | SRT_DENOISE_FRAMEBUFFER))
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_denoise: unknown flags 0x%x", d->flags);
    const bool demod = (d->flags & SRT_DENOISE_ALBEDO) != 0;
    const void* guide[4] = {};
    if (const int rc = find_guides(ctx, "srt_denoise", demod ? 4 : 3, nullptr, guide)) return rc;
    return atrous_filter(ctx, guide, d->iterations, d->flags, d->sigma_normal, d->sigma_plane, d->sigma_color, 0.0f, nullptr);
}

int srt_bind_denoised(srt_context* ctx, void* d_float4) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return ctx->dn.bind(d_float4), SRT_OK;  // (no synchronisation: enqueued levels keep the buffer they were given)
}

int srt_read_denoised(srt_context* ctx, float* dst_rgba) {
    if (!ctx || !dst_rgba) return SRT_ERR_INVALID_ARG;
    return read_slot(ctx, ctx->dn.read_any(ctx->d_dn_own), dst_rgba, frame_pixels(ctx) * sizeof(float4), "srt_read_denoised: nothing has been denoised into this buffer yet");
}

// ---- mirror history ------------------------------------------------------------------------------------------------
static_assert(sizeof(srt_mirror_history_params) == 16 && sizeof(srt::MirrorHistoryCall) == 16 && srt::MIRROR_MAX_BOUNCES == srt::REFL_MAX_BOUNCES,
              "srt_mirror_history_host.h and srt_pathtrace.h disagree");

int srt_mirror_history_params_default(srt_mirror_history_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    const srt::MirrorHistoryCall c = srt::mirror_history_defaults();
    out->enabled = c.enabled, out->radius_pixels = c.radius_pixels, out->flags = c.flags, out->reserved = c.reserved;
    return SRT_OK;
}

int srt_mirror_history(srt_context* ctx, const srt_mirror_history_params* m) {
    if (!ctx || !m) return SRT_ERR_INVALID_ARG;
    const srt::MirrorHistoryCall call{m->enabled, m->radius_pixels, m->flags, m->reserved};
    const char* why = "";
    if (const srt::RaysStatus rs = srt::mirror_history_check(call, &why))
        return fail(ctx, (int)rs, "srt_mirror_history: %s (enabled %d, radius_pixels %g, flags 0x%x, reserved %u)", why, m->enabled,
                    (double)m->radius_pixels, m->flags, m->reserved);
    // a history of the other mode carries or lacks the tags this one relies on: the next call starts afresh
    if (srt::mirror_history_set(ctx->mirror, call)) ctx->tp_valid = false, ctx->mom_history = false;
    return SRT_OK;
}

// ---- probe tail ----------------------------------------------------------------------------------------------------
static_assert(sizeof(srt_probe_tail_params) == 32 && sizeof(srt::ProbeTailCall) == 32 && sizeof(srt_probe_tail_work) == 56 && srt::PT_WORK_N == 6 &&
                  SRT_PROBE_TAIL_NORMAL_WEIGHT == srt::PROBE_TAIL_FLAG_NORMAL_WEIGHT && SRT_PROBE_TAIL_DEPTH == srt::PROBE_TAIL_FLAG_DEPTH &&
                  SRT_PROBE_TAIL_STATES == srt::PROBE_TAIL_FLAG_STATES && SRT_PROBE_TAIL_COUNT_WORK == srt::PROBE_TAIL_FLAG_COUNT_WORK &&
                  SRT_PROBE_TAIL_NORMAL_WEIGHT == srt::PT_NORMAL_WEIGHT && SRT_PROBE_TAIL_DEPTH == srt::PT_DEPTH && SRT_PROBE_TAIL_STATES == srt::PT_STATES,
              "srt_probe_tail_host.h, srt_probe_tail.hip.h and srt_pathtrace.h disagree");

int srt_probe_tail_params_default(srt_probe_tail_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    const srt::ProbeTailCall c = srt::probe_tail_defaults();
    memcpy(out, &c, sizeof c);
    return SRT_OK;
}

int srt_probe_tail(srt_context* ctx, const srt_probe_tail_params* t) {
    if (!ctx || !t) return SRT_ERR_INVALID_ARG;
    srt::ProbeTailCall call;
    memcpy(&call, t, sizeof call);
    const char* why = "";
    if (const srt::RaysStatus rs = srt::probe_tail_check(call, &why))
        return fail(ctx, (int)rs, "srt_probe_tail: %s (enabled %d, flags 0x%x, band_weight %g %g %g, bias %g, min_variance %g, reserved %u)", why, t->enabled, t->flags,
                    (double)t->band_weight[0], (double)t->band_weight[1], (double)t->band_weight[2], (double)t->bias, (double)t->min_variance, t->reserved);
    srt::probe_tail_set(ctx->probe_tail, call);  // (an enqueued launch keeps the setting it was given: a kernel argument)
    return SRT_OK;
}

SRT_WORK_LAYOUT(srt_probe_tail_work, srt::PT_WORK_N, tails, srt::PT_WORK_TAILS, wave_lookups, srt::PT_WORK_WAVE_LOOKUPS);
int srt_get_probe_tail_work(srt_context* ctx, srt_probe_tail_work* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    return get_work(ctx, ctx->probe_tail.last, ctx->d_probe_tail_work, out,
                    "srt_get_probe_tail_work: the last radiance or light-probe trace did not run under srt_probe_tail with SRT_PROBE_TAIL_COUNT_WORK (or there has been none)");
}

// The reflection outputs srt_temporal_accumulate reads with the mirror history on (OBJECT, NORMAL_DEPTH, POSITION, BOUNCES), by
// slot, bound or own, under find_guides' rule: SRT_ERR_STATE for the first that is missing or is an own one of another camera.
static int find_reflection_guides(srt_context* ctx, const char* fn, const srt_camera* cam, const void** guide) {
    static const char* const names[srt::REFL_SLOTS] = {"OBJECT", "NORMAL_DEPTH", "POSITION", "ALBEDO", "BOUNCES"};
    for (int i = 0; i < srt::REFL_SLOTS; ++i) {
        if (i == 3) continue;  // (ALBEDO is not read)
        const srt::OutputSlot& slot = ctx->refl.out[i];
        guide[i] = slot.bound || slot.written ? slot.current((void*)ctx->d_refl_own[i]) : nullptr;
        if (!guide[i])
            return fail(ctx, SRT_ERR_STATE, "%s: the reflection output %s has neither been bound nor written (srt_render_reflection_gbuffer)", fn, names[i]);
        if (!slot.bound && (!ctx->refl_own_cam_set[i] || !same_camera(ctx->refl_own_cam[i], *cam)))
            return fail(ctx, SRT_ERR_STATE, "%s: the reflection output %s was rendered with another camera (srt_render_reflection_gbuffer after srt_set_camera)", fn, names[i]);
    }
    return SRT_OK;
}

// ---- temporal reprojection ------------------------------------------------------------------------------------------
int srt_temporal_params_default(srt_temporal_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    // chosen by tools/temporal_time.py sweep on Scene1 and Scene_indirect
    out->samples = 1;
    out->max_samples = 32.0f;
    out->plane_tolerance = 0.02f;
    out->normal_threshold = 0.9f;
    out->flags = 0;
    return SRT_OK;
}

// B^-1 of the camera's ray basis B = [right * rd | up * ld | forward * clip] (columns, the floats srt_render uses), inverted in
// double and rounded to float, row-major.  False when B is singular or not finite.
static bool invert_ray_basis(const srt_camera& c, int W, int H, float inv[9]) {
    float r[3], u[3], f[3];
    fold_camera(c, W, H, r, u, f);
    const double m[3][3] = {{r[0], u[0], f[0]}, {r[1], u[1], f[1]}, {r[2], u[2], f[2]}};
    const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2],
                 c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
    const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
    if (!(det != 0.0) || !std::isfinite(det)) return false;
    const double adj[3][3] = {{c00, m[0][2] * m[2][1] - m[0][1] * m[2][2], m[0][1] * m[1][2] - m[0][2] * m[1][1]},
                              {c01, m[0][0] * m[2][2] - m[0][2] * m[2][0], m[0][2] * m[1][0] - m[0][0] * m[1][2]},
                              {c02, m[0][1] * m[2][0] - m[0][0] * m[2][1], m[0][0] * m[1][1] - m[0][1] * m[1][0]}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            inv[3 * i + j] = (float)(adj[i][j] / det);
            if (!std::isfinite(inv[3 * i + j])) return false;
        }
    return true;
}

// The per-object motion table of this call: row i = (position now - position at the previous call, keep), keep = 1 when every
// other field of the object has the same bytes in both lists.  moved = false (and nothing uploaded) when no object moved or
// changed: the call then runs the kernel without a table.
static int build_motion_table(srt_context* ctx, bool& moved) {
    const size_t n = ctx->objects.size();
    moved = false;
    for (size_t i = 0; i < n && !moved; ++i) {
        srt_object then = ctx->tp_objects[i];
        const srt_object& now = ctx->objects[i];
        for (int k = 0; k < 3; ++k) {
            moved = moved || now.position[k] - then.position[k] != 0.0f;
            then.position[k] = now.position[k];
        }
        moved = moved || memcmp(&then, &now, sizeof(srt_object)) != 0;
    }
    if (!moved) return SRT_OK;
    if (ctx->tp_table_in_flight) SRT_HIP(ctx, hipEventSynchronize(ctx->ev_tp_table));
    ctx->tp_table_in_flight = false;
    SRT_HIP(ctx, ctx->h_tp_table.ensure(n * sizeof(float4)));
    SRT_HIP(ctx, ctx->d_tp_table.ensure(n * sizeof(float4)));
    if (!ctx->ev_tp_table.h) SRT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_tp_table.h, hipEventDisableTiming));
    float4* rows = ctx->h_tp_table;
    for (size_t i = 0; i < n; ++i) {
        srt_object then = ctx->tp_objects[i];
        const srt_object& now = ctx->objects[i];
        float d[3];
        for (int k = 0; k < 3; ++k) {
            d[k] = now.position[k] - then.position[k];
            then.position[k] = now.position[k];
        }
        rows[i] = make_float4(d[0], d[1], d[2], memcmp(&then, &now, sizeof(srt_object)) == 0 ? 1.0f : 0.0f);
    }
    SRT_HIP(ctx, hipMemcpyAsync(ctx->d_tp_table, rows, n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    SRT_HIP(ctx, hipEventRecord(ctx->ev_tp_table, ctx->stream));
    ctx->tp_table_in_flight = true;
    return SRT_OK;
}

int srt_temporal_accumulate(srt_context* ctx, const srt_temporal_params* t) {
    if (!ctx || !t) return SRT_ERR_INVALID_ARG;
    if (t->samples == 0) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_temporal_accumulate: samples must be >= 1");
    // (written so that a NaN fails too)
    if (!(t->max_samples >= (float)t->samples))
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_temporal_accumulate: max_samples %g < samples %u", t->max_samples, t->samples);
    if (!(t->plane_tolerance > 0.0f))
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_temporal_accumulate: plane_tolerance must be > 0 (%g)", t->plane_tolerance);
    if (t->normal_threshold != t->normal_threshold) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_temporal_accumulate: normal_threshold is NaN");
    if (t->flags & ~(SRT_TEMPORAL_RESET | SRT_TEMPORAL_FRAMEBUFFER))
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_temporal_accumulate: unknown flags 0x%x", t->flags);
    if (!ctx->camera.set) return fail(ctx, SRT_ERR_STATE, "srt_temporal_accumulate: srt_set_camera has not been called");
    // the handle's own guides must show the camera the history will be stored with
    const void* guide[3] = {};
    if (const int rc = find_guides(ctx, "srt_temporal_accumulate", 3, &ctx->camera.cam, guide)) return rc;
    // the moments of the demodulated luminance need the ALBEDO guide, under the same rule
    const float4* mom_albedo = nullptr;
    if (ctx->mom_on && (ctx->mom_flags & SRT_VARIANCE_ALBEDO)) {
        const void* g4[4] = {};
        if (const int rc = find_guides(ctx, "srt_temporal_accumulate (srt_moments_output with SRT_VARIANCE_ALBEDO)", 4, &ctx->camera.cam, g4)) return rc;
        mom_albedo = (const float4*)g4[3];
    }
    // the mirror history reads four reflection outputs next to the first hits, under the same rule
    const void* refl_guide[srt::REFL_SLOTS] = {};
    if (ctx->mirror.enabled) {
        if (const int rc = find_reflection_guides(ctx, "srt_temporal_accumulate (srt_mirror_history)", &ctx->camera.cam, refl_guide)) return rc;
    }
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t px = (size_t)ctx->width * (size_t)ctx->height;
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 3; ++k) SRT_HIP(ctx, ctx->d_tp[i][k].ensure(px * sizeof(float4)));
    if (ctx->mom_on && (!(float4*)ctx->d_mom[0] || !(float4*)ctx->d_mom[1])) {
        ctx->mom_written = ctx->mom_history = false;
        for (int i = 0; i < 2; ++i) SRT_HIP(ctx, ctx->d_mom[i].ensure(px * sizeof(float4)));
    }
    const int a = ctx->tp_cur, b = 1 - a;  // read slot a (when valid), write slot b
    srt::TemporalLaunch T{};
    T.acc = ctx->d_acc;
    T.object = (const int32_t*)guide[0];
    T.normal_depth = (const float4*)guide[1];
    T.position = (const float4*)guide[2];
    T.prev = srt::TemporalSlot{ctx->d_tp[a][0], ctx->d_tp[a][1], ctx->d_tp[a][2]};
    T.next = srt::TemporalSlot{ctx->d_tp[b][0], ctx->d_tp[b][1], ctx->d_tp[b][2]};
    T.framebuffer = (t->flags & SRT_TEMPORAL_FRAMEBUFFER) ? ctx->d_fb : nullptr;
    T.width = ctx->width, T.height = ctx->height;
    T.valid = ctx->tp_written && ctx->tp_valid && !(t->flags & SRT_TEMPORAL_RESET) &&
              invert_ray_basis(ctx->tp_cam, ctx->width, ctx->height, T.inv);
    for (int i = 0; i < 3; ++i) T.cam_pos[i] = ctx->tp_cam.position[i];
    T.samples = (float)t->samples;
    T.max_samples = t->max_samples;
    T.plane_tolerance = t->plane_tolerance;
    T.normal_threshold = t->normal_threshold;
    // object motion: only a valid history of a list of the same length can have moved
    bool motion = false;
    if (T.valid && !ctx->objects.empty() && ctx->objects.size() == ctx->tp_objects.size()) {
        if (const int rc = build_motion_table(ctx, motion)) return rc;
    }
    if (motion) T.table = ctx->d_tp_table, T.table_count = (int)ctx->objects.size();
    if (ctx->mv_on) {
        SRT_WRITE_TARGET(ctx, ctx->mv, ctx->d_mv_own, px * sizeof(float4), T.motion);
    }
    if (ctx->mom_on) {
        T.mom_prev = ctx->d_mom[a];
        T.mom_next = ctx->d_mom[b];
        T.albedo = mom_albedo;
        T.mom_valid = T.valid && ctx->mom_history && ctx->mom_written && ctx->mom_written_flags == ctx->mom_flags;
    }
    const dim3 grid = frame_tile_grid(ctx), block(srt::WG_THREADS);
    if (ctx->mirror.enabled) {
        srt::MirrorLaunch M{};
        M.T = T;
        M.r_object = (const int32_t*)refl_guide[0];
        M.r_normal_depth = (const float4*)refl_guide[1];
        M.r_position = (const float4*)refl_guide[2];
        M.r_bounces = (const int32_t*)refl_guide[4];
        for (int i = 0; i < 3; ++i) M.cam[i] = ctx->camera.cam.position[i];
        M.rho = srt::mirror_rho(ctx->mirror.radius_pixels, ctx->camera.cam.fov_degrees, ctx->height);
        const int pick = (motion ? 4 : 0) | (ctx->mv_on ? 2 : 0) | (ctx->mom_on ? 1 : 0);
        void (*const kernels[8])(srt::MirrorLaunch) = {
            srt::temporal_mirror_kernel<false, false, false>, srt::temporal_mirror_kernel<false, false, true>,
            srt::temporal_mirror_kernel<false, true, false>,  srt::temporal_mirror_kernel<false, true, true>,
            srt::temporal_mirror_kernel<true, false, false>,  srt::temporal_mirror_kernel<true, false, true>,
            srt::temporal_mirror_kernel<true, true, false>,   srt::temporal_mirror_kernel<true, true, true>};
        hipLaunchKernelGGL(kernels[pick], grid, block, 0, ctx->stream, M);
    }
    else if (ctx->mom_on) {
        void (*const kernel)(srt::TemporalLaunch) = SRT_KERNEL(srt::temporal_moments_kernel, motion, ctx->mv_on);
        hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, T);
    }
    else if (!motion && !ctx->mv_on) hipLaunchKernelGGL(srt::temporal_kernel, grid, block, 0, ctx->stream, T);
    else if (!motion) hipLaunchKernelGGL((srt::temporal_motion_kernel<false, true>), grid, block, 0, ctx->stream, T);
    else if (!ctx->mv_on) hipLaunchKernelGGL((srt::temporal_motion_kernel<true, false>), grid, block, 0, ctx->stream, T);
    else hipLaunchKernelGGL((srt::temporal_motion_kernel<true, true>), grid, block, 0, ctx->stream, T);
    SRT_HIP(ctx, hipGetLastError());
    // the records of slot b: this call's, or (output off) none
    ctx->mom_written = ctx->mom_on;
    ctx->mom_history = ctx->mom_on;
    if (ctx->mom_on) ctx->mom_written_flags = ctx->mom_flags, ctx->mom_samples = T.samples;
    ctx->tp_cur = b;
    ctx->tp_cam = ctx->camera.cam;
    ctx->tp_objects = ctx->objects;  // the list this history's points belong to
    ctx->tp_valid = true;
    ctx->tp_written = true;
    if (ctx->mv_on) ctx->mv.wrote(T.motion);
    return SRT_OK;
}

int srt_motion_output(srt_context* ctx, int enabled) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    ctx->mv_on = enabled != 0;
    return SRT_OK;
}

int srt_bind_motion(srt_context* ctx, void* d_float4) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return ctx->mv.bind(d_float4), SRT_OK;  // (no synchronisation: an enqueued call keeps the buffer it was given)
}

int srt_read_motion(srt_context* ctx, float* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    return read_slot(ctx, ctx->mv.read_last_only(ctx->d_mv_own), dst, frame_pixels(ctx) * sizeof(float4), "srt_read_motion: no srt_temporal_accumulate has written this buffer yet");
}

int srt_moments_output(srt_context* ctx, int enabled, uint32_t flags) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (flags & ~SRT_VARIANCE_ALBEDO) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_moments_output: unknown flags 0x%x", flags);
    const bool on = enabled != 0;
    if (on != ctx->mom_on || flags != ctx->mom_flags) ctx->mom_history = false;  // the next call starts the moments afresh
    ctx->mom_on = on;
    ctx->mom_flags = flags;
    return SRT_OK;
}

int srt_read_moments(srt_context* ctx, float* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    return read_slot(ctx, ctx->mom_written ? (const float4*)ctx->d_mom[ctx->tp_cur] : nullptr, dst, frame_pixels(ctx) * sizeof(float4),
                     "srt_read_moments: the last srt_temporal_accumulate wrote no moments (srt_moments_output)");
}

int srt_temporal_variance_params_default(srt_temporal_variance_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    out->min_frames = 4.0f;  // SVGF's (Schied et al. 2017, §4.2)
    out->radius = 3;         // its 7 x 7 window
    out->flags = 0;
    return SRT_OK;
}

int srt_temporal_variance(srt_context* ctx, const srt_temporal_variance_params* v) {
    if (!ctx || !v) return SRT_ERR_INVALID_ARG;
    if (v->flags != 0) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_temporal_variance: unknown flags 0x%x", v->flags);
    // (written so that a NaN fails too)
    if (!(v->min_frames >= 0.0f)) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_temporal_variance: min_frames must be >= 0 (%g)", v->min_frames);
    if (v->radius < 1 || v->radius > srt::MT_MAX_RADIUS)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_temporal_variance: radius %d outside 1..%d", v->radius, srt::MT_MAX_RADIUS);
    if (!ctx->mom_written)
        return fail(ctx, SRT_ERR_STATE, "srt_temporal_variance: the last srt_temporal_accumulate wrote no moments (srt_moments_output)");
    const void* guide[1] = {};
    if (const int rc = find_guides(ctx, "srt_temporal_variance", 1, nullptr, guide)) return rc;
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    srt::MomentsLaunch M{};
    const size_t px = frame_pixels(ctx);
    SRT_WRITE_TARGET(ctx, ctx->var, ctx->d_var_own, px * sizeof(float), M.variance);
    M.moments = ctx->d_mom[ctx->tp_cur];
    M.object = (const int32_t*)guide[0];
    M.width = ctx->width, M.height = ctx->height;
    M.samples = ctx->mom_samples;
    M.old_length = v->min_frames * ctx->mom_samples;
    void (*const kernel)(srt::MomentsLaunch) = v->radius == 1   ? srt::temporal_variance_kernel<1>
                                               : v->radius == 2 ? srt::temporal_variance_kernel<2>
                                                                : srt::temporal_variance_kernel<3>;
    hipLaunchKernelGGL(kernel, frame_tile_grid(ctx), dim3(srt::WG_THREADS), 0, ctx->stream, M);
    SRT_HIP(ctx, hipGetLastError());
    ctx->var.wrote(M.variance);
    if (!ctx->var.bound) ctx->var_own_written = true, ctx->var_own_albedo = (ctx->mom_written_flags & SRT_VARIANCE_ALBEDO) != 0;
    return SRT_OK;
}

int srt_read_history_length(srt_context* ctx, float* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    if (!ctx->tp_written) return fail(ctx, SRT_ERR_STATE, "srt_read_history_length: srt_temporal_accumulate has not been called");
    if (const int rc = finish_stream(ctx)) return rc;
    // L is the w of the history colour
    const size_t px = (size_t)ctx->width * ctx->height;
    std::vector<float4> tmp(px);
    SRT_HIP(ctx, hipMemcpy(tmp.data(), ctx->d_tp[ctx->tp_cur][0], px * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < px; ++i) dst[i] = tmp[i].w;
    return SRT_OK;
}

// ---- guided upsampler ------------------------------------------------------------------------------------------------
int srt_upsample_params_default(srt_upsample_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    // the denoiser's normal and plane sigmas (tools/upsample_time.py sweep is the tool that revisits them)
    srt_denoise_params d{};
    (void)srt_denoise_params_default(&d);
    out->steps = 2;
    out->stripe_width = 0;
    out->sigma_normal = d.sigma_normal;
    out->sigma_plane = d.sigma_plane;
    out->flags = 0;
    return SRT_OK;
}

int srt_upsample(srt_context* ctx, const srt_upsample_params* u) {
    if (!ctx || !u) return SRT_ERR_INVALID_ARG;
    if (u->steps < 1 || u->steps > 32768) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_upsample: steps %d outside 1..32768", u->steps);
    if (u->stripe_width < 0) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_upsample: stripe_width must be >= 0 (%d)", u->stripe_width);
    // (written so that a NaN fails too)
    if (!(u->sigma_normal >= 0.0f) || !(u->sigma_plane >= 0.0f))
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_upsample: sigmas must be >= 0 (normal %g, plane %g)", u->sigma_normal, u->sigma_plane);
    if (u->flags & ~(SRT_UPSAMPLE_IN_PLACE | SRT_UPSAMPLE_FRAMEBUFFER))
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_upsample: unknown flags 0x%x", u->flags);
    const void* guide[3] = {};
    if (const int rc = find_guides(ctx, "srt_upsample", 3, nullptr, guide)) return rc;
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const bool in_place = (u->flags & SRT_UPSAMPLE_IN_PLACE) != 0;
    srt::UpsampleLaunch U{};
    if (!in_place) {
        SRT_WRITE_TARGET(ctx, ctx->up, ctx->d_up_own, (size_t)ctx->width * (size_t)ctx->height * sizeof(float4), U.dst);
    }
    U.acc = ctx->d_acc;
    U.acc_rgb = in_place ? (float*)ctx->d_acc : nullptr;
    U.object = (const int32_t*)guide[0];
    U.normal_depth = (const float4*)guide[1];
    U.position = (const float4*)guide[2];
    U.framebuffer = (u->flags & SRT_UPSAMPLE_FRAMEBUFFER) ? ctx->d_fb : nullptr;
    U.width = ctx->width, U.height = ctx->height;
    U.steps = u->steps;
    U.stripe = u->stripe_width > 0 && u->stripe_width < ctx->width ? u->stripe_width : ctx->width;  // (a stripe as wide as the frame is a single one)
    U.sigma_normal = fminf(u->sigma_normal, FLT_MAX);  // as srt_denoise: FLT_MAX * log2 1 = 0 where inf * 0 would be NaN
    U.sigma_plane = fminf(u->sigma_plane, FLT_MAX);  // as srt_denoise: FLT_MAX * 0 = 0 where inf * 0 (a first hit at d_p = 0) would be NaN
    hipLaunchKernelGGL(srt::upsample_kernel, frame_tile_grid(ctx), dim3(srt::WG_THREADS), 0, ctx->stream, U);
    SRT_HIP(ctx, hipGetLastError());
    if (!in_place) ctx->up.wrote(U.dst);
    return SRT_OK;
}

int srt_bind_upsampled(srt_context* ctx, void* d_float4) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return ctx->up.bind(d_float4), SRT_OK;  // (no synchronisation: an enqueued call keeps the buffer it was given)
}

int srt_read_upsampled(srt_context* ctx, float* dst_rgba) {
    if (!ctx || !dst_rgba) return SRT_ERR_INVALID_ARG;
    return read_slot(ctx, ctx->up.read_any(ctx->d_up_own), dst_rgba, frame_pixels(ctx) * sizeof(float4), "srt_read_upsampled: nothing has been upsampled into this buffer yet");
}

// ---- anti-aliasing: sub-sample first hits and the resolve ------------------------------------------------------------------
int srt_render_subsamples(srt_context* ctx, const srt_subsample_params* g) {
    if (!ctx || !g) return SRT_ERR_INVALID_ARG;
    if (!ctx->scene_set) return fail(ctx, SRT_ERR_STATE, "srt_render_subsamples: srt_set_scene has not been called");
    if (!ctx->camera.set) return fail(ctx, SRT_ERR_STATE, "srt_render_subsamples: srt_set_camera has not been called");
    const int W = ctx->width, H = ctx->height;
    if (g->row_begin < 0 || g->row_end > H || g->row_begin >= g->row_end)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_render_subsamples: bad row band [%d,%d) for height %d", g->row_begin, g->row_end, H);
    if (g->k < 1 || g->k > 4) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_render_subsamples: k %d outside 1..4", g->k);
    if (g->flags != 0) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_render_subsamples: flags must be 0");
    // the virtual frame's pixel coordinates and sizes must be exact in binary32 (and its aspect ratio the frame's own)
    if (2ll * g->k * W >= (1ll << 24) || 2ll * g->k * H >= (1ll << 24))
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_render_subsamples: 2k x the frame (%d x %d, k %d) must stay below 2^24", W, H, g->k);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    srt::SubsampleOut out{nullptr, g->k};
    const size_t px = frame_pixels(ctx);
    SRT_WRITE_TARGET(ctx, ctx->ss, ctx->d_ss_own, (size_t)g->k * g->k * px * sizeof(int32_t), out.sub);
    if (!ctx->ss.bound) {
        if (ctx->ss_own_k != g->k || ctx->ss_own_scene != ctx->scene_changes || !same_camera(ctx->ss_own_cam, ctx->camera.cam) ||
            ctx->ss_own_rows.size() != (size_t)H) {
            ctx->ss_own_k = g->k, ctx->ss_own_scene = ctx->scene_changes, ctx->ss_own_cam = ctx->camera.cam;
            ctx->ss_own_rows.assign((size_t)H, false);
        }
        std::fill(ctx->ss_own_rows.begin() + g->row_begin, ctx->ss_own_rows.begin() + g->row_end, true);
    }
    srt::KernelParams K;
    const KernelSetup ks = scene_kernel_params(ctx, g->row_begin, g->row_end, K);
    if (const int rc = launch_tiles(ctx, SRT_KERNEL(srt::subsample_kernel, ctx->scene_in_lds[ks.img], K.n_tris > 0), ks, K, out)) return rc;
    ctx->ss.wrote(out.sub, (size_t)g->k);
    return SRT_OK;
}

int srt_bind_subsamples(srt_context* ctx, void* d_int32) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return ctx->ss.bind(d_int32), SRT_OK;  // (no synchronisation: enqueued launches keep the buffer they were given, as srt_bind_gbuffer)
}

int srt_read_subsamples(srt_context* ctx, int32_t* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    // (the k of a bound buffer is the last render's, into whichever buffer; the own buffer's is its own)
    const size_t k = ctx->ss.bound ? ctx->ss.last_count : (size_t)ctx->ss_own_k;
    return read_slot(ctx, k ? current(ctx->ss, ctx->d_ss_own) : nullptr, dst, k * k * frame_pixels(ctx) * sizeof(int32_t),
                     "srt_read_subsamples: no sub-samples have been rendered into this buffer yet");
}

int srt_antialias_params_default(srt_antialias_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    out->k = 2;
    out->source = SRT_AA_SOURCE_ACCUMULATOR;
    out->flags = 0;
    return SRT_OK;
}

int srt_antialias(srt_context* ctx, const srt_antialias_params* a) {
    if (!ctx || !a) return SRT_ERR_INVALID_ARG;
    if (a->k < 1 || a->k > 4) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_antialias: k %d outside 1..4", a->k);
    if (a->source != SRT_AA_SOURCE_ACCUMULATOR && a->source != SRT_AA_SOURCE_DENOISED)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_antialias: unknown source %d", a->source);
    if (a->flags & ~SRT_AA_FRAMEBUFFER) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_antialias: unknown flags 0x%x", a->flags);
    const void* guide[1] = {};
    if (const int rc = find_guides(ctx, "srt_antialias", 1, nullptr, guide)) return rc;
    const int32_t* const sub = current(ctx->ss, ctx->d_ss_own);
    if (!sub) return fail(ctx, SRT_ERR_STATE, "srt_antialias: the sub-sample buffer has neither been bound nor rendered (srt_render_subsamples)");
    if (!ctx->ss.bound) {  // the handle's own: a whole frame of this k, scene and camera, or nothing
        if (ctx->ss_own_k != a->k) return fail(ctx, SRT_ERR_STATE, "srt_antialias: the sub-samples were rendered with k %d, not %d", ctx->ss_own_k, a->k);
        if (ctx->ss_own_scene != ctx->scene_changes || !ctx->camera.set || !same_camera(ctx->ss_own_cam, ctx->camera.cam))
            return fail(ctx, SRT_ERR_STATE, "srt_antialias: the sub-samples were rendered with another scene or camera (srt_render_subsamples after the change)");
        if (std::find(ctx->ss_own_rows.begin(), ctx->ss_own_rows.end(), false) != ctx->ss_own_rows.end())
            return fail(ctx, SRT_ERR_STATE, "srt_antialias: the sub-samples do not cover the whole frame since the last scene or camera change");
    }
    const float4* src = ctx->d_acc;
    if (a->source == SRT_AA_SOURCE_DENOISED) {
        src = (const float4*)ctx->dn.read_any(ctx->d_dn_own);
        if (!src) return fail(ctx, SRT_ERR_STATE, "srt_antialias: SRT_AA_SOURCE_DENOISED before the first srt_denoise");
    }
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    srt::AntialiasLaunch A{};
    SRT_WRITE_TARGET(ctx, ctx->aa, ctx->d_aa_own, (size_t)ctx->width * (size_t)ctx->height * sizeof(float4), A.dst);
    A.src = src;
    A.object = (const int32_t*)guide[0];
    A.sub = sub;
    A.framebuffer = (a->flags & SRT_AA_FRAMEBUFFER) ? ctx->d_fb : nullptr;
    A.width = ctx->width, A.height = ctx->height;
    void (*const kernel)(srt::AntialiasLaunch) = a->k == 1 ? srt::antialias_kernel<1> : a->k == 2 ? srt::antialias_kernel<2>
                                                 : a->k == 3 ? srt::antialias_kernel<3> : srt::antialias_kernel<4>;
    hipLaunchKernelGGL(kernel, frame_tile_grid(ctx), dim3(srt::WG_THREADS), 0, ctx->stream, A);
    SRT_HIP(ctx, hipGetLastError());
    ctx->aa.wrote(A.dst);
    return SRT_OK;
}

int srt_bind_antialiased(srt_context* ctx, void* d_float4) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return ctx->aa.bind(d_float4), SRT_OK;  // (no synchronisation: an enqueued call keeps the buffer it was given)
}

int srt_read_antialiased(srt_context* ctx, float* dst_rgba) {
    if (!ctx || !dst_rgba) return SRT_ERR_INVALID_ARG;
    return read_slot(ctx, ctx->aa.read_any(ctx->d_aa_own), dst_rgba, frame_pixels(ctx) * sizeof(float4), "srt_read_antialiased: nothing has been anti-aliased into this buffer yet");
}

// ---- variance estimate and variance-guided denoiser -----------------------------------------------------------------------
int srt_variance_params_default(srt_variance_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    // what srt_denoise_variance's defaults expect: the demodulated variance, and the mean of the halves to filter
    out->flags = SRT_VARIANCE_ALBEDO | SRT_VARIANCE_MERGE;
    return SRT_OK;
}

int srt_device_half(srt_context* ctx, void** d_ptr) {
    if (!ctx || !d_ptr) return SRT_ERR_INVALID_ARG;
    if (!(float4*)ctx->d_half_own) {
        SRT_HIP(ctx, hipSetDevice(ctx->device));
        const size_t bytes = (size_t)ctx->width * (size_t)ctx->height * sizeof(float4);
        SRT_HIP(ctx, ctx->d_half_own.ensure(bytes));
        SRT_HIP(ctx, hipMemsetAsync(ctx->d_half_own, 0, bytes, ctx->stream));  // as the accumulator starts
    }
    *d_ptr = (float4*)ctx->d_half_own;
    return SRT_OK;
}

int srt_bind_half(srt_context* ctx, void* d_float4) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return ctx->half.bind(d_float4), SRT_OK;  // (no synchronisation: an enqueued call keeps the buffer it was given)
}

int srt_variance(srt_context* ctx, const srt_variance_params* v) {
    if (!ctx || !v) return SRT_ERR_INVALID_ARG;
    if (v->flags & ~(SRT_VARIANCE_ALBEDO | SRT_VARIANCE_MERGE)) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_variance: unknown flags 0x%x", v->flags);
    const bool demod = (v->flags & SRT_VARIANCE_ALBEDO) != 0;
    // OBJECT, and ALBEDO when demodulating (find_guides takes the slots in order: the two between are not needed here)
    const void* guide[4] = {};
    if (const int rc = find_guides(ctx, "srt_variance", 1, nullptr, guide)) return rc;
    if (demod) {
        guide[3] = current(ctx->gbuf[3], ctx->d_gbuf_own[3]);
        if (!guide[3]) return fail(ctx, SRT_ERR_STATE, "srt_variance: the ALBEDO guide has neither been bound nor rendered (srt_render_gbuffer)");
    }
    const float4* half = current(ctx->half, ctx->d_half_own);
    if (!half) return fail(ctx, SRT_ERR_STATE, "srt_variance: the half buffer has neither been bound (srt_bind_half) nor fetched (srt_device_half)");
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t px = frame_pixels(ctx);
    srt::VarianceLaunch V{};
    SRT_WRITE_TARGET(ctx, ctx->var, ctx->d_var_own, px * sizeof(float), V.variance);
    V.acc = ctx->d_acc;
    V.half = half;
    V.object = (const int32_t*)guide[0];
    V.albedo = demod ? (const float4*)guide[3] : nullptr;
    V.pixels = px;
    V.merge = (v->flags & SRT_VARIANCE_MERGE) ? 1 : 0;
    const unsigned blocks = (unsigned)((px + srt::VARIANCE_THREADS - 1) / srt::VARIANCE_THREADS);
    hipLaunchKernelGGL(srt::variance_kernel, dim3(blocks), dim3(srt::VARIANCE_THREADS), 0, ctx->stream, V);
    SRT_HIP(ctx, hipGetLastError());
    ctx->var.wrote(V.variance);
    if (!ctx->var.bound) ctx->var_own_written = true, ctx->var_own_albedo = demod;
    return SRT_OK;
}

int srt_bind_variance(srt_context* ctx, void* d_float) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    return ctx->var.bind(d_float), SRT_OK;  // (no synchronisation: an enqueued call keeps the buffer it was given)
}

int srt_read_variance(srt_context* ctx, float* dst) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    return read_slot(ctx, ctx->var.read_any(ctx->d_var_own), dst, frame_pixels(ctx) * sizeof(float), "srt_read_variance: no variance has been written into this buffer yet");
}

int srt_denoise_variance_params_default(srt_denoise_variance_params* out) {
    if (!out) return SRT_ERR_INVALID_ARG;
    srt_denoise_params d{};
    (void)srt_denoise_params_default(&d);
    out->iterations = d.iterations;
    out->sigma_luminance = 4.0f;  // SVGF's (Schied et al. 2017, §4.4)
    out->sigma_normal = d.sigma_normal;
    out->sigma_plane = d.sigma_plane;
    out->flags = d.flags;
    return SRT_OK;
}

int srt_denoise_variance(srt_context* ctx, const srt_denoise_variance_params* d) {
    if (!ctx || !d) return SRT_ERR_INVALID_ARG;
    if (d->iterations < 1 || d->iterations > 8)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_denoise_variance: iterations %d outside 1..8", d->iterations);
    // (written so that a NaN fails too)
    if (!(d->sigma_luminance >= 0.0f) || !(d->sigma_normal >= 0.0f) || !(d->sigma_plane >= 0.0f))
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_denoise_variance: sigmas must be >= 0 (luminance %g, normal %g, plane %g)",
                    d->sigma_luminance, d->sigma_normal, d->sigma_plane);
    if (d->flags & ~(SRT_DENOISE_ALBEDO | SRT_DENOISE_FRAMEBUFFER))
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_denoise_variance: unknown flags 0x%x", d->flags);
    const bool demod = (d->flags & SRT_DENOISE_ALBEDO) != 0;
    const void* guide[4] = {};
    if (const int rc = find_guides(ctx, "srt_denoise_variance", demod ? 4 : 3, nullptr, guide)) return rc;
    const float* const var = ctx->var.bound ? (const float*)ctx->var.bound : ctx->var_own_written ? (float*)ctx->d_var_own : nullptr;
    if (!var) return fail(ctx, SRT_ERR_STATE, "srt_denoise_variance: no variance buffer has been bound (srt_bind_variance) or written (srt_variance)");
    if (!ctx->var.bound && ctx->var_own_albedo != demod)
        return fail(ctx, SRT_ERR_STATE, "srt_denoise_variance: the variance was estimated %s SRT_VARIANCE_ALBEDO, this call is %s SRT_DENOISE_ALBEDO",
                    ctx->var_own_albedo ? "with" : "without", demod ? "with" : "without");
    return atrous_filter(ctx, guide, d->iterations, d->flags, d->sigma_normal, d->sigma_plane, 0.0f, d->sigma_luminance, var);
}

int srt_wait(srt_context* ctx) {
    if (!ctx) return SRT_ERR_INVALID_ARG;
    if (const int rc = finish_stream(ctx)) return rc;
    return SRT_OK;
}

int srt_poll(srt_context* ctx, int* done) {
    if (!ctx || !done) return SRT_ERR_INVALID_ARG;
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipStreamQuery(ctx->stream);
    if (e == hipSuccess) {
        *done = 1;
        return SRT_OK;
    }
    if (e == hipErrorNotReady) {
        (void)hipGetLastError();  // not an error: keep it from surfacing in a later hipGetLastError()
        *done = 0;
        return SRT_OK;
    }
    return fail(ctx, SRT_ERR_HIP, "hipStreamQuery: %s", hipGetErrorString(e));
}

int srt_get_stats(srt_context* ctx, srt_stats* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    if (!ctx->launched) return fail(ctx, SRT_ERR_STATE, "srt_get_stats: nothing rendered yet");
    if (const int rc = finish_stream(ctx)) return rc;
    if (ctx->stats_pending) {
        float ms = 0.0f;
        if (ctx->pending_timed) SRT_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
        ctx->stats.kernel_ms = ms;
        ctx->stats.path_samples = ctx->pending_samples;
        ctx->stats.sample_chunks = ctx->pending_chunks;
        ctx->stats.tile_rows = ctx->pending_tile_rows;
        ctx->stats.chunk_samples = ctx->pending_chunk_samples;
        ctx->stats.shape_source = ctx->pending_shape_source;
        ctx->stats.rays = 0;
        memset(&ctx->work_counts, 0, sizeof ctx->work_counts);
        if (ctx->count_work && ctx->count_work_valid) {
            unsigned long long t[srt::TALLY_ALL];
            SRT_HIP(ctx, hipMemcpy(t, ctx->d_work, sizeof t, hipMemcpyDeviceToHost));
            srt_work_counts& wc = ctx->work_counts;
            const uint64_t nu = (uint64_t)ctx->work_layout[0], nc = (uint64_t)ctx->work_layout[1], nb = (uint64_t)ctx->work_layout[3];
            wc.valid = 1;
            wc.waves = t[srt::TALLY_WAVES];
            wc.pool_steps = t[srt::TALLY_STEPS];
            wc.closest_hit_calls = t[srt::TALLY_CALLS];
            // a wave runs every trip of these loops for all of its 64 lanes, whatever they carry: executed tests = trips x 64
            wc.uniform_sphere_tests = t[srt::TALLY_CALLS] * nu * 64u;
            wc.box_tests = t[srt::TALLY_CALLS] * nb * 64u;
            wc.cluster_bound_tests = t[srt::TALLY_BOUND_CALLS] * nc * 64u;
            wc.cluster_sphere_tests = t[srt::TALLY_SPHERE_TESTS] * 64u;
            wc.cluster_items = t[srt::TALLY_ITEMS];
            wc.bvh_child_tests = t[srt::TALLY_NODE_TESTS] * 64u;
            wc.triangle_tests = t[srt::TALLY_LEAF_TRIPS] * 64u;
            wc.bvh_node_rounds = t[srt::TALLY_NODE_ROUNDS];
            wc.mesh_phases = t[srt::TALLY_MESH_PHASES];
        }
        if (ctx->count_rays) {
            unsigned long long r = 0;
            SRT_HIP(ctx, hipMemcpy(&r, ctx->d_rays, sizeof r, hipMemcpyDeviceToHost));
            ctx->stats.rays = r;
        }
        ctx->stats_pending = false;
    }
    *out = ctx->stats;
    return SRT_OK;
}

int srt_get_work_counts(srt_context* ctx, srt_work_counts* out) {
    if (!ctx || !out) return SRT_ERR_INVALID_ARG;
    srt_stats st;
    const int rc = srt_get_stats(ctx, &st);  // waits, and reads the counters of the last render back
    if (rc != SRT_OK) return rc;
    if (!ctx->count_work) return fail(ctx, SRT_ERR_STATE, "srt_get_work_counts: the last srt_render did not ask for SRT_RENDER_COUNT_WORK");
    *out = ctx->work_counts;
    return SRT_OK;
}

int srt_read_framebuffer(srt_context* ctx, void* dst, size_t pitch_bytes, int row_begin, int row_end) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    const size_t rowb = (size_t)ctx->width * 4;
    if (row_begin < 0 || row_end > ctx->height || row_begin >= row_end || pitch_bytes < rowb)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_read_framebuffer: bad rows [%d,%d) or pitch %zu", row_begin, row_end, pitch_bytes);
    if (const int rc = finish_stream(ctx)) return rc;
    SRT_HIP(ctx, hipMemcpy2D(dst, pitch_bytes, (const char*)ctx->d_fb + (size_t)row_begin * rowb, rowb, rowb,
                             (size_t)(row_end - row_begin), hipMemcpyDeviceToHost));
    return SRT_OK;
}

int srt_read_framebuffer_async(srt_context* ctx, void* dst, size_t pitch_bytes, int row_begin, int row_end, void* copy_stream) {
    if (!ctx || !dst) return SRT_ERR_INVALID_ARG;
    const size_t rowb = (size_t)ctx->width * 4;
    if (row_begin < 0 || row_end > ctx->height || row_begin >= row_end || pitch_bytes < rowb)
        return fail(ctx, SRT_ERR_INVALID_ARG, "srt_read_framebuffer_async: bad rows [%d,%d) or pitch %zu", row_begin, row_end, pitch_bytes);
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t cs = copy_stream ? (hipStream_t)copy_stream : ctx->stream;
    if (cs != ctx->stream) {  // the copy starts when the renders enqueued so far have finished, not before
        if (!ctx->ev_read) SRT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_read.h, hipEventDisableTiming));
        SRT_HIP(ctx, hipEventRecord(ctx->ev_read, ctx->stream));
        SRT_HIP(ctx, hipStreamWaitEvent(cs, ctx->ev_read, 0));
    }
    SRT_HIP(ctx, hipMemcpy2DAsync(dst, pitch_bytes, (const char*)ctx->d_fb + (size_t)row_begin * rowb, rowb, rowb, (size_t)(row_end - row_begin),
                                  hipMemcpyDeviceToHost, cs));
    return SRT_OK;
}

int srt_read_accumulator(srt_context* ctx, float* dst_rgba) {
    if (!ctx || !dst_rgba) return SRT_ERR_INVALID_ARG;
    if (const int rc = finish_stream(ctx)) return rc;
    SRT_HIP(ctx, hipMemcpy(dst_rgba, ctx->d_acc, (size_t)ctx->width * ctx->height * sizeof(float4), hipMemcpyDeviceToHost));
    return SRT_OK;
}

// The balance probe: the PROBE instantiation of pathtrace_kernel runs the real path pool over the WHOLE frame for the frame's
// first PROBE_SAMPLES = 32 samples on ONE of every workgroup's four waves (a quarter of the pixels) — nothing of the frame is read
// or written — and every wave adds what its loops did (srt::TALLY_*: pool steps, groups of exactly tested spheres, BVH rounds,
// triangle trips, phases, child-box tests, tiles with and without untraced pixels) to its 16 x 16 block's counters.  Counts, not
// times: the same on every GPU and in every run.  Cost: the work of 32 x 1/4 = 8 sample-frames on one device — 1.6 % of a 512-spp
// launch of the frame, 0.8 % of a 1024-spp one, a quarter of a 32-spp one — plus a host round trip (the call is synchronous).
constexpr int PROBE_SAMPLES = 32;
static_assert(PROBE_SAMPLES == 32, "ProbeWeights were fitted on probes of 32 samples (shorter pools take 12..37 % more steps per sample, unevenly over a frame): refit them (tools/band_fit.py) when this changes");
static int run_pool_probe(srt_context* ctx, int max_bounces, uint32_t seed, std::vector<uint32_t>& counts, int& bx, int& by) {
    SRT_HIP(ctx, hipSetDevice(ctx->device));
    srt_render_params p{};
    p.row_begin = 0, p.row_end = ctx->height, p.first_sample = 1, p.sample_count = PROBE_SAMPLES, p.max_bounces = max_bounces, p.seed = seed;
    p.flags = SRT_RENDER_RESET;
    srt::KernelParams K;
    const KernelSetup ks = fill_kernel_params(ctx, &p, K);
    K.flags = (K.flags & srt::KF_BOXES_FINITE) | SRT_RENDER_RESET;
    K.tile_h = srt::TILE_H;
    K.accumulator = nullptr, K.framebuffer = nullptr, K.ray_counter = nullptr;  // the probe touches none of them
    const dim3 grid = frame_tile_grid(ctx), block(srt::WG_THREADS);
    bx = (int)grid.x, by = (int)grid.y;
    const size_t words = (size_t)bx * by * srt::TALLY_N;
    DeviceBuffer<uint32_t> d;
    SRT_HIP(ctx, d.ensure(words * sizeof(uint32_t)));
    hipError_t e = hipMemsetAsync(d, 0, words * sizeof(uint32_t), ctx->stream);
    K.wg_cost = d;
    if (e == hipSuccess) {
        const bool in_lds = ctx->scene_in_lds[ks.img];
        if (K.n_tris > 0 && in_lds) hipLaunchKernelGGL((srt::pathtrace_kernel<4, true, true, false, false, true>), grid, block, ks.lds_bytes, ctx->stream, K);
        else if (K.n_tris > 0) hipLaunchKernelGGL((srt::pathtrace_kernel<4, true, false, false, false, true>), grid, block, ks.lds_bytes, ctx->stream, K);
        else if (in_lds) hipLaunchKernelGGL((srt::pathtrace_kernel<4, false, true, false, false, true>), grid, block, ks.lds_bytes, ctx->stream, K);
        else hipLaunchKernelGGL((srt::pathtrace_kernel<4, false, false, false, false, true>), grid, block, ks.lds_bytes, ctx->stream, K);
        e = hipGetLastError();
    }
    counts.resize(words);
    if (e == hipSuccess) e = hipMemcpyAsync(counts.data(), d, words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, SRT_ERR_HIP, "balance probe: %s", hipGetErrorString(e));
    return SRT_OK;
}

int srt_estimate_row_costs(srt_context* ctx, int max_bounces, uint32_t seed, float* row_costs) {
    if (!ctx || !row_costs) return SRT_ERR_INVALID_ARG;
    if (!ctx->scene_set) return fail(ctx, SRT_ERR_STATE, "srt_estimate_row_costs: srt_set_scene has not been called");
    if (!ctx->camera.set) return fail(ctx, SRT_ERR_STATE, "srt_estimate_row_costs: srt_set_camera has not been called");
    if (max_bounces < 0) return fail(ctx, SRT_ERR_INVALID_ARG, "srt_estimate_row_costs: max_bounces must be >= 0");
    const int H = ctx->height;
    std::vector<uint32_t> counts;
    int bx = 0, by = 0;
    const int rc = run_pool_probe(ctx, max_bounces, seed, counts, bx, by);
    if (rc != SRT_OK) return rc;
    srt_render_params p{};
    p.row_begin = 0, p.row_end = H, p.first_sample = 1, p.sample_count = 1, p.max_bounces = max_bounces;
    srt::KernelParams K;
    fill_kernel_params(ctx, &p, K);
    const ProbeWeights w;
    // a block covers WG_H scene rows; its cost is spread evenly over them; memory row m = scene row H - 1 - m
    for (int m = 0; m < H; ++m) row_costs[m] = 0.0f;
    for (int j = 0; j < by; ++j) {
        double sum = 0;
        for (int i = 0; i < bx; ++i) sum += probe_block_cost(&counts[((size_t)j * bx + i) * srt::TALLY_N], K, w);
        const int y0 = j * srt::WG_H, y1 = y0 + srt::WG_H < H ? y0 + srt::WG_H : H;
        for (int y = y0; y < y1; ++y) row_costs[H - 1 - y] = (float)(sum / (double)(y1 - y0));
    }
    return SRT_OK;
}

#ifdef SRT_DEV
// development aid (tools/band_fit.py): the balance probe's raw counts — out[TALLY_N * (bx * by)], block (i, j) covers scene rows
// [16 j, 16 j + 16) — and the scene constants a step's cost depends on: consts = {uniform sphere groups, clusters, boxes, triangles}
int srt_debug_probe_counts(srt_context* ctx, int max_bounces, uint32_t seed, uint32_t* out, int* blocks_x, int* blocks_y, int* consts4) {
    if (!ctx || !out || !blocks_x || !blocks_y || !consts4) return SRT_ERR_INVALID_ARG;
    std::vector<uint32_t> counts;
    const int rc = run_pool_probe(ctx, max_bounces, seed, counts, *blocks_x, *blocks_y);
    if (rc != SRT_OK) return rc;
    memcpy(out, counts.data(), counts.size() * sizeof(uint32_t));
    const srt::SceneLayout& SL = ctx->layout[0];
    consts4[0] = (SL.nu + 3) / 4, consts4[1] = SL.nc, consts4[2] = SL.nb, consts4[3] = ctx->mesh_image.n_tris;
    return SRT_OK;
}
#endif

int srt_selftest_arith(int device, uint32_t seed, uint64_t vectors, uint64_t* mismatches) {
    if (!mismatches || vectors == 0 || vectors > (1ull << 36)) return SRT_ERR_INVALID_ARG;
    int prev = 0;
    if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) {
        (void)hipGetLastError();
        return SRT_ERR_NO_DEVICE;
    }
    DeviceBuffer<unsigned long long> d;
    hipError_t e = d.ensure(sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemset(d, 0, sizeof(unsigned long long));
    for (uint64_t done = 0; e == hipSuccess && done < vectors; done += 1ull << 28) {  // grids of at most 2^20 blocks
        const uint64_t part = vectors - done < (1ull << 28) ? vectors - done : (1ull << 28);
        hipLaunchKernelGGL(srt::selftest_normalize_kernel, dim3((unsigned)((part + 255) / 256)), dim3(256), 0, 0, seed + (uint32_t)(done >> 28) * 0x85EBCA6Bu, (unsigned long long)done, part, d);
        e = hipGetLastError();
    }
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost);
    d.reset();  // (on its device)
    (void)hipSetDevice(prev);
    if (e != hipSuccess) return SRT_ERR_HIP;
    *mismatches = h;
    return SRT_OK;
}

int srt_gather_band(srt_context* dst, srt_context* src, int row_begin, int row_end) {
    if (!dst || !src) return SRT_ERR_INVALID_ARG;
    if (dst->width != src->width || dst->height != src->height)
        return fail(dst, SRT_ERR_INVALID_ARG, "srt_gather_band: %dx%d into %dx%d", src->width, src->height, dst->width, dst->height);
    if (row_begin < 0 || row_end > src->height || row_begin >= row_end)
        return fail(dst, SRT_ERR_INVALID_ARG, "srt_gather_band: bad rows [%d,%d)", row_begin, row_end);
    if (dst == src) return SRT_OK;
    const size_t rowb = (size_t)src->width * 4, off = (size_t)row_begin * rowb, bytes = (size_t)(row_end - row_begin) * rowb;
    // every HIP call below runs with the SOURCE's device current; whatever happens, the caller gets the destination's
    // device back (a failure must not leave the thread on another GPU)
    hipError_t e = hipSetDevice(src->device);
    const char* what = "hipSetDevice";
    if (e == hipSuccess && src->device != dst->device) {
        // direct xGMI path where the topology offers it: asked once per pair of devices and source context
        // (hipDeviceCanAccessPeer), enabled once; without peer access the runtime stages the copy through the host.
        // NOTE: this branch needs two GPUs and has never executed on this project's one-GPU boxes — it is
        // unverified code; srt_gather_path() says which way a gather went, so the first multi-GPU run tells.
        const unsigned long long bit = dst->device < 64 ? 1ull << dst->device : 0ull;
        if (bit && !(src->peer_asked & bit)) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, src->device, dst->device) != hipSuccess) can = 0, (void)hipGetLastError();
            if (can) {
                const hipError_t pe = hipDeviceEnablePeerAccess(dst->device, 0);
                if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) can = 0;
                if (pe != hipSuccess) (void)hipGetLastError();
            }
            src->peer_asked |= bit;
            if (can) src->peer_direct |= bit;
        }
        const bool direct = bit && (src->peer_direct & bit);
        snprintf(src->gather_path, sizeof src->gather_path, direct ? "device %d -> device %d: hipMemcpyPeerAsync with peer access enabled (direct link)"
                                                                   : "device %d -> device %d: hipMemcpyPeerAsync WITHOUT peer access (staged by the runtime)", src->device, dst->device);
        what = "hipMemcpyPeerAsync";
        e = hipMemcpyPeerAsync((char*)dst->d_fb + off, dst->device, (const char*)src->d_fb + off, src->device, bytes, src->stream);
    } else if (e == hipSuccess) {
        snprintf(src->gather_path, sizeof src->gather_path, "device %d -> device %d: same device, hipMemcpyAsync device to device", src->device, dst->device);
        what = "hipMemcpyAsync";
        e = hipMemcpyAsync((char*)dst->d_fb + off, (const char*)src->d_fb + off, bytes, hipMemcpyDeviceToDevice, src->stream);
    }
    if (e == hipSuccess && !src->ev_gather) what = "hipEventCreate", e = hipEventCreateWithFlags(&src->ev_gather.h, hipEventDisableTiming);
    if (e == hipSuccess) what = "hipEventRecord", e = hipEventRecord(src->ev_gather, src->stream);
    const hipError_t back = hipSetDevice(dst->device);
    if (e == hipSuccess) what = "hipSetDevice", e = back;
    if (e == hipSuccess) what = "hipStreamWaitEvent", e = hipStreamWaitEvent(dst->stream, src->ev_gather, 0);
    if (e != hipSuccess) return fail(dst, e == hipErrorOutOfMemory ? SRT_ERR_OOM : SRT_ERR_HIP, "srt_gather_band: %s: %s", what, hipGetErrorString(e));
    return SRT_OK;
}

const char* srt_gather_path(const srt_context* src) { return src ? src->gather_path : "(null context)"; }

int srt_write_accumulator(srt_context* ctx, const float* src_rgba) {
    if (!ctx || !src_rgba) return SRT_ERR_INVALID_ARG;
    if (const int rc = finish_stream(ctx)) return rc;
    SRT_HIP(ctx, hipMemcpy(ctx->d_acc, src_rgba, (size_t)ctx->width * ctx->height * sizeof(float4), hipMemcpyHostToDevice));
    return SRT_OK;
}

}  // extern "C"
