"""ctypes bindings of include/srt_pathtrace.h (libsrt_pathtrace.so).  Plumbing only.

Every call goes through the C-ABI — the same entry points a C, C++ or FFI caller would
bind.  No fallback: a missing library raises ImportError-like SrtError at load time,
a missing GPU makes srt_create fail with SRT_ERR_NO_DEVICE.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_PKG, "libsrt_pathtrace.so")

OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_STATE, ERR_OOM = range(6)
OBJ_NONE, OBJ_SPHERE, OBJ_BOX, OBJ_MESH = 0, 1, 2, 3
RENDER_RESET, RENDER_COUNT_RAYS, RENDER_PREVIEW, RENDER_COUNT_WORK, RENDER_NO_TIMING = 1, 2, 4, 8, 16
GBUF_OBJECT, GBUF_NORMAL_DEPTH, GBUF_POSITION, GBUF_ALBEDO, GBUF_ALL = 1, 2, 4, 8, 15
# first-hit buffer names (PathTracer.gbuffer / bind_gbuffer) -> (output bit, numpy dtype, per-pixel channels)
GBUFFERS = {"object": (GBUF_OBJECT, np.int32, 1), "normal_depth": (GBUF_NORMAL_DEPTH, np.float32, 4),
            "position": (GBUF_POSITION, np.float32, 4), "albedo": (GBUF_ALBEDO, np.float32, 4)}
# ray queries (srt_trace_rays): the four G-buffer bits plus OCCLUDED, and the one flag
RAYS_OCCLUDED, RAYS_ALL = 16, 31
RAYS_NORMALIZE = 1
# any-hit queries (srt_trace_occlusion): the flags of srt_occlusion_params
OCCLUSION_NORMALIZE, OCCLUSION_COUNT_WORK = 1, 2
# per-pixel visibility (srt_render_visibility): the output bits, their names, the one flag and the sample limit
VIS_AO, VIS_SUN, VIS_ALL = 1, 2, 3
VIS_COUNT_WORK = 1
VIS_MAX_SAMPLES = 4096
VISIBILITY = {"ao": VIS_AO, "sun": VIS_SUN}
# reflection guides (srt_render_reflection_gbuffer): the output bits, the one flag, the bounce limit, and the output names
# (PathTracer.read_reflection / bind_reflection) -> (output bit, numpy dtype, per-pixel channels); the first four are GBUFFERS'
REFL_OBJECT, REFL_NORMAL_DEPTH, REFL_POSITION, REFL_ALBEDO, REFL_BOUNCES, REFL_GUIDES, REFL_ALL = 1, 2, 4, 8, 16, 15, 31
REFL_COUNT_WORK = 1
REFL_MAX_BOUNCES = 64
REFLECTION = dict(GBUFFERS, bounces=(REFL_BOUNCES, np.int32, 1))
# reflection outputs srt_temporal_accumulate reads with the mirror history on
MIRROR_HISTORY_GUIDES = REFL_OBJECT | REFL_NORMAL_DEPTH | REFL_POSITION | REFL_BOUNCES
# radiance queries (srt_trace_radiance): the flags of srt_radiance_params and the sample limit
RADIANCE_RESET, RADIANCE_NORMALIZE, RADIANCE_COUNT_WORK = 1, 2, 4
RADIANCE_SUN_SAMPLING = 16  # SRT_RADIANCE_SUN_SAMPLING: sun sampling at diffuse bounces (rules S1 - S9); 8 is unassigned
RADIANCE_MAX_SAMPLES = 4096
# light probes (srt_trace_light_probes): the flags and outputs of srt_light_probe_params, the direction limit, float4 per probe
LIGHT_PROBE_RESET, LIGHT_PROBE_NORMALIZE, LIGHT_PROBE_COUNT_WORK = 1, 2, 4
LIGHT_PROBE_SUN_SAMPLING = 16  # SRT_LIGHT_PROBE_SUN_SAMPLING: the listed call takes it too
LIGHT_PROBE_COEFFICIENTS, LIGHT_PROBE_RADIANCE = 1, 2
LIGHT_PROBE_MAX_DIRECTIONS = 4096
LIGHT_PROBE_COEFFS = 9
# probe-grid shading (srt_shade_probe_grid): the flags of srt_probe_grid_params and the two documented band weights
PROBE_GRID_VISIBILITY, PROBE_GRID_NORMAL_WEIGHT, PROBE_GRID_ALBEDO, PROBE_GRID_COUNT_WORK = 1, 2, 4, 8
PROBE_GRID_BAND_WEIGHT_IRRADIANCE = (3.14159274, 2.09439516, 0.785398185)  # srt_light_probe_irradiance's: the cosine-weighted integral
PROBE_GRID_BAND_WEIGHT_HEMISPHERE = (1.0, 0.5, 0.0)  # the mean over the hemisphere around the normal
# probe depth moments (srt_trace_probe_depth): the outputs and flags of srt_probe_depth_params, the accepted resolutions
PROBE_DEPTH_MOMENTS, PROBE_DEPTH_DISTANCES = 1, 2
PROBE_DEPTH_NORMALIZE, PROBE_DEPTH_COUNT_WORK = 1, 2
PROBE_DEPTH_RESOLUTIONS = (4, 8, 16)
# probe classification and relocation (srt_classify_probes): the outputs and flags of srt_probe_classify_params, the state bits
PROBE_STATE_RECORDS, PROBE_STATE_POSITIONS = 1, 2
PROBE_CLASSIFY_RELOCATE, PROBE_CLASSIFY_NORMALIZE, PROBE_CLASSIFY_COUNT_WORK = 1, 2, 4
PROBE_CLEAR, PROBE_MOVED, PROBE_BURIED, PROBE_INSIDE, PROBE_IDLE = 0, 1, 2, 4, 8
# per-frame probe updates (srt_list_probes, the listed traces, srt_blend_probes): the list's flag and header, the histories, the
# flags of srt_probe_blend_params
PROBE_LIST_COUNT_WORK, PROBE_LIST_HEADER, PROBE_LIST_NONE = 1, 4, 0xFFFFFFFF
PROBE_HISTORY_COEFFICIENTS, PROBE_HISTORY_MOMENTS = 1, 2
PROBE_BLEND_MOMENTS, PROBE_BLEND_LISTED, PROBE_BLEND_PREVIOUS_STATES, PROBE_BLEND_COUNT_WORK = 1, 2, 4, 8
# scrolling probe grids (srt_scroll_probes): the arrays of srt_probe_scroll_params.which, its flags
PROBE_SCROLL_COEFFICIENTS, PROBE_SCROLL_MOMENTS, PROBE_SCROLL_STATES = 1, 2, 4
PROBE_SCROLL_COUNT_WORK, PROBE_SCROLL_SET_GRID = 1, 2
# probe cascades (srt_shade_probe_cascade): the most levels, the flags of srt_probe_cascade_params, the arrays of a level
PROBE_CASCADE_MAX_LEVELS = 4
PROBE_CASCADE_NORMAL_WEIGHT, PROBE_CASCADE_DEPTH, PROBE_CASCADE_STATES, PROBE_CASCADE_ALBEDO, PROBE_CASCADE_COUNT_WORK = 1, 2, 4, 8, 16
PROBE_CASCADE_COEFFICIENTS, PROBE_CASCADE_MOMENTS, PROBE_CASCADE_RECORDS = 1, 2, 4
# adaptive sampling (srt_render_adaptive, srt_sample_budget): the flags, the limits of max_samples / max_budget, the last frame
ADAPTIVE_KEEP_COUNTS, ADAPTIVE_COUNT_WORK = 1, 2
ADAPTIVE_SUN_SAMPLING = 16  # SRT_ADAPTIVE_SUN_SAMPLING: sun sampling in render_adaptive[_tail] (rules AS1 - AS8); 4 and 8 are unassigned
ADAPTIVE_MAX_SAMPLES = 4096
ADAPTIVE_FRAME_LIMIT = 2147483646
BUDGET_ALBEDO = 1
BUDGET_MAX = 4096
# ray output names (PathTracer.ray_output / bind_ray_output) -> (output bit, numpy dtype, per-ray channels)
RAY_OUTPUTS = dict(GBUFFERS, occluded=(RAYS_OCCLUDED, np.int32, 1))
DENOISE_ALBEDO, DENOISE_FRAMEBUFFER = 1, 2
# guides srt_denoise reads: OBJECT, NORMAL_DEPTH and POSITION always, ALBEDO when demodulating
DENOISE_GUIDES = GBUF_OBJECT | GBUF_NORMAL_DEPTH | GBUF_POSITION
TEMPORAL_RESET, TEMPORAL_FRAMEBUFFER = 1, 2
# guides srt_temporal_accumulate reads
TEMPORAL_GUIDES = GBUF_OBJECT | GBUF_NORMAL_DEPTH | GBUF_POSITION
UPSAMPLE_IN_PLACE, UPSAMPLE_FRAMEBUFFER = 1, 2
# guides srt_upsample reads
UPSAMPLE_GUIDES = GBUF_OBJECT | GBUF_NORMAL_DEPTH | GBUF_POSITION
AA_FRAMEBUFFER = 2
AA_SOURCE_ACCUMULATOR, AA_SOURCE_DENOISED = 0, 1
VARIANCE_ALBEDO, VARIANCE_MERGE = 1, 2
UPDATE_REBUILD, UPDATE_REFIT = 0, 1
# srt_update_info.path by name
UPDATE_PATHS = {0: "none", 1: "rebuilt", 2: "refitted", 3: "kept"}
ABI_VERSION = 7

# every symbol include/srt_pathtrace.h declares (tests check the library exports them all)
EXPORTS = [
    "srt_abi_version", "srt_device_count", "srt_create", "srt_destroy", "srt_last_error",
    "srt_set_scene", "srt_set_meshes", "srt_set_environment", "srt_environment_default", "srt_set_camera",
    "srt_set_stream", "srt_bind_output", "srt_device_framebuffer", "srt_device_accumulator",
    "srt_render", "srt_wait", "srt_poll", "srt_get_stats", "srt_get_work_counts", "srt_pick", "srt_read_framebuffer",
    "srt_read_framebuffer_async", "srt_read_accumulator", "srt_write_accumulator", "srt_gather_band", "srt_gather_path", "srt_estimate_row_costs",
    "srt_selftest_arith", "srt_render_gbuffer", "srt_bind_gbuffer", "srt_read_gbuffer",
    "srt_denoise_params_default", "srt_denoise", "srt_bind_denoised", "srt_read_denoised",
    "srt_temporal_params_default", "srt_temporal_accumulate", "srt_read_history_length",
    "srt_update_scene", "srt_motion_output", "srt_bind_motion", "srt_read_motion",
    "srt_upsample_params_default", "srt_upsample", "srt_bind_upsampled", "srt_read_upsampled",
    "srt_render_subsamples", "srt_bind_subsamples", "srt_read_subsamples",
    "srt_antialias_params_default", "srt_antialias", "srt_bind_antialiased", "srt_read_antialiased",
    "srt_variance_params_default", "srt_device_half", "srt_bind_half", "srt_variance", "srt_bind_variance", "srt_read_variance",
    "srt_denoise_variance_params_default", "srt_denoise_variance",
    "srt_moments_output", "srt_read_moments", "srt_temporal_variance_params_default", "srt_temporal_variance",
    "srt_update_mode", "srt_get_update_info", "srt_mesh_image_size", "srt_read_mesh_image",
    "srt_trace_params_default", "srt_write_rays", "srt_bind_rays", "srt_bind_ray_output", "srt_trace_rays", "srt_read_ray_output",
    "srt_occlusion_params_default", "srt_trace_occlusion", "srt_get_occlusion_work",
    "srt_visibility_params_default", "srt_render_visibility", "srt_bind_visibility", "srt_read_visibility", "srt_get_visibility_work",
    "srt_reflection_params_default", "srt_render_reflection_gbuffer", "srt_bind_reflection", "srt_read_reflection",
    "srt_device_reflection", "srt_get_reflection_work",
    "srt_mirror_history_params_default", "srt_mirror_history",
    "srt_radiance_params_default", "srt_trace_radiance", "srt_bind_radiance", "srt_read_radiance", "srt_get_radiance_work",
    "srt_set_sample_counts", "srt_write_sample_counts", "srt_read_sample_counts", "srt_bind_sample_counts",
    "srt_write_sample_budget", "srt_read_sample_budget", "srt_bind_sample_budget",
    "srt_adaptive_params_default", "srt_render_adaptive", "srt_get_adaptive_work",
    "srt_budget_params_default", "srt_sample_budget", "srt_get_budget_total",
    "srt_write_light_probes", "srt_bind_light_probes", "srt_write_light_probe_directions", "srt_bind_light_probe_directions",
    "srt_light_probe_params_default", "srt_trace_light_probes", "srt_bind_light_probe_output", "srt_read_light_probe_output",
    "srt_get_light_probe_work", "srt_light_probe_sphere", "srt_light_probe_irradiance",
    "srt_probe_grid_positions", "srt_probe_grid_params_default", "srt_set_probe_grid", "srt_write_probe_grid_coefficients",
    "srt_bind_probe_grid_coefficients", "srt_shade_probe_grid", "srt_bind_probe_grid_output", "srt_read_probe_grid_output",
    "srt_get_probe_grid_work",
    "srt_probe_depth_params_default", "srt_probe_depth_texels", "srt_trace_probe_depth", "srt_bind_probe_depth_output",
    "srt_read_probe_depth_output", "srt_get_probe_depth_work",
    "srt_probe_grid_depth_params_default", "srt_write_probe_grid_depth", "srt_bind_probe_grid_depth", "srt_shade_probe_grid_depth",
    "srt_probe_classify_params_default", "srt_classify_probes", "srt_bind_probe_states_output", "srt_read_probe_states_output",
    "srt_get_probe_classify_work", "srt_write_probe_grid_states", "srt_bind_probe_grid_states", "srt_shade_probe_grid_states",
    "srt_probe_list_params_default", "srt_list_probes", "srt_bind_probe_list_output", "srt_read_probe_list_output", "srt_get_probe_list_work",
    "srt_bind_probe_list", "srt_write_probe_list", "srt_trace_light_probes_listed", "srt_trace_probe_depth_listed",
    "srt_probe_blend_params_default", "srt_reset_probe_history", "srt_bind_probe_history", "srt_read_probe_history",
    "srt_write_probe_previous_states", "srt_bind_probe_previous_states", "srt_blend_probes", "srt_get_probe_blend_work",
    "srt_probe_scroll_params_default", "srt_scroll_probes", "srt_get_probe_scroll_work", "srt_probe_grid_follow",
    "srt_read_probe_previous_states",
    "srt_probe_cascade_params_default", "srt_probe_cascade_grids", "srt_probe_cascade_weights", "srt_set_probe_cascade",
    "srt_write_probe_cascade_level", "srt_bind_probe_cascade_level", "srt_capture_probe_cascade_level", "srt_shade_probe_cascade",
    "srt_get_probe_cascade_work",
    "srt_probe_tail_params_default", "srt_probe_tail", "srt_get_probe_tail_work",
    "srt_render_adaptive_tail",
]


class SrtError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("srt error %d: %s" % (code, text))
        self.code = code


class Material(C.Structure):
    _fields_ = [
        ("smoothness", C.c_float),
        ("specular_amount", C.c_float),
        ("base_color", C.c_float * 3),
        ("emissive_color", C.c_float * 3),
        ("specular_color", C.c_float * 3),
    ]


class Object(C.Structure):
    _fields_ = [
        ("type", C.c_int32),
        ("position", C.c_float * 3),
        ("radius", C.c_float),
        ("half_size", C.c_float * 3),
        ("material", Material),
        ("mesh", C.c_int32),
    ]


class Mesh(C.Structure):
    _fields_ = [
        ("vertices", C.POINTER(C.c_float)),
        ("vertex_count", C.c_size_t),
        ("indices", C.POINTER(C.c_uint32)),
        ("triangle_count", C.c_size_t),
    ]


class Environment(C.Structure):
    _fields_ = [
        ("sun_direction", C.c_float * 3),
        ("sky_color", C.c_float * 3),
        ("horizon_color", C.c_float * 3),
        ("ground_color", C.c_float * 3),
        ("sun_color", C.c_float * 3),
    ]


class Camera(C.Structure):
    _fields_ = [
        ("position", C.c_float * 3),
        ("right", C.c_float * 3),
        ("up", C.c_float * 3),
        ("forward", C.c_float * 3),
        ("fov_degrees", C.c_int32),
    ]


class RenderParams(C.Structure):
    _fields_ = [
        ("row_begin", C.c_int32),
        ("row_end", C.c_int32),
        ("first_sample", C.c_uint32),
        ("sample_count", C.c_uint32),
        ("max_bounces", C.c_int32),
        ("seed", C.c_uint32),
        ("flags", C.c_uint32),
        ("steps", C.c_int32),
        ("stripe_width", C.c_int32),
        ("selected_object", C.c_int32),
    ]


class GBufferParams(C.Structure):
    _fields_ = [("row_begin", C.c_int32), ("row_end", C.c_int32), ("outputs", C.c_uint32), ("flags", C.c_uint32)]


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float),
                ("flags", C.c_uint32)]


class TemporalParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("max_samples", C.c_float), ("plane_tolerance", C.c_float),
                ("normal_threshold", C.c_float), ("flags", C.c_uint32)]


class UpsampleParams(C.Structure):
    _fields_ = [("steps", C.c_int32), ("stripe_width", C.c_int32), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float),
                ("flags", C.c_uint32)]


class SubsampleParams(C.Structure):
    _fields_ = [("row_begin", C.c_int32), ("row_end", C.c_int32), ("k", C.c_int32), ("flags", C.c_uint32)]


class AntialiasParams(C.Structure):
    _fields_ = [("k", C.c_int32), ("source", C.c_int32), ("flags", C.c_uint32)]


class VarianceParams(C.Structure):
    _fields_ = [("flags", C.c_uint32)]


class DenoiseVarianceParams(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float),
                ("flags", C.c_uint32)]


class TemporalVarianceParams(C.Structure):
    _fields_ = [("min_frames", C.c_float), ("radius", C.c_int32), ("flags", C.c_uint32)]


class TraceParams(C.Structure):
    _fields_ = [("outputs", C.c_uint32), ("flags", C.c_uint32)]


class WorkRecord(C.Structure):
    """The base of the records a pass leaves of its last call (srt_*_work, srt_work_counts, srt_update_info)."""

    def as_dict(self):
        """Every field but `reserved` and `spare` as an int, an array field as a list of ints."""
        values = ((n, getattr(self, n)) for n, _ in self._fields_ if n not in ("reserved", "spare"))
        return {n: [int(x) for x in v] if isinstance(v, C.Array) else int(v) for n, v in values}


class OcclusionParams(C.Structure):
    """srt_occlusion_params: OCCLUSION_* flags; reserved must be 0."""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32)]


class OcclusionWork(WorkRecord):
    """srt_occlusion_work: lane-level tests executed by the last counting srt_trace_occlusion for rays of its batch."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("rays", C.c_uint64), ("occluded", C.c_uint64),
                ("analytic_tests", C.c_uint64), ("node_visits", C.c_uint64), ("triangle_tests", C.c_uint64)]


class VisibilityParams(C.Structure):
    """srt_visibility_params: a band in memory rows, VIS_* outputs, 0 or VIS_COUNT_WORK, and the AO sample range, seed and radius."""
    _fields_ = [("row_begin", C.c_int32), ("row_end", C.c_int32), ("outputs", C.c_uint32), ("flags", C.c_uint32),
                ("ao_samples", C.c_uint32), ("first_sample", C.c_uint32), ("seed", C.c_uint32), ("ao_radius", C.c_float)]


class VisibilityWork(WorkRecord):
    """srt_visibility_work: what the last counting srt_render_visibility traced."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("segments", C.c_uint64), ("open", C.c_uint64), ("wave_trips", C.c_uint64),
                ("analytic_tests", C.c_uint64), ("node_visits", C.c_uint64), ("triangle_tests", C.c_uint64)]


class ReflectionParams(C.Structure):
    """srt_reflection_params: a band in memory rows, REFL_* outputs, 0 or REFL_COUNT_WORK, the bounce limit and the two thresholds;
    reserved must be 0."""
    _fields_ = [("row_begin", C.c_int32), ("row_end", C.c_int32), ("outputs", C.c_uint32), ("flags", C.c_uint32),
                ("max_bounces", C.c_int32), ("min_smoothness", C.c_float), ("min_specular", C.c_float), ("reserved", C.c_uint32)]


class ReflectionWork(WorkRecord):
    """srt_reflection_work: what the last counting srt_render_reflection_gbuffer traced."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("pixels", C.c_uint64), ("reflections", C.c_uint64),
                ("wave_calls", C.c_uint64), ("waves", C.c_uint64)]


class MirrorHistoryParams(C.Structure):
    """srt_mirror_history_params: the mode (0 or 1) and the radius of its distance test in pixels; flags and reserved must be 0."""
    _fields_ = [("enabled", C.c_int32), ("radius_pixels", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


PROBE_TAIL_NORMAL_WEIGHT, PROBE_TAIL_DEPTH, PROBE_TAIL_STATES, PROBE_TAIL_COUNT_WORK = 1, 2, 4, 8


class ProbeTailParams(C.Structure):
    """srt_probe_tail_params: the mode (0 or 1), PROBE_TAIL_* flags, the band weights of the lookup and rule 7b's parameters."""
    _fields_ = [("enabled", C.c_int32), ("flags", C.c_uint32), ("band_weight", C.c_float * 3), ("bias", C.c_float),
                ("min_variance", C.c_float), ("reserved", C.c_uint32)]


class ProbeTailWork(WorkRecord):
    """srt_probe_tail_work: the lookups of the last trace that ran under srt_probe_tail with PROBE_TAIL_COUNT_WORK."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("tails", C.c_uint64), ("corners", C.c_uint64), ("open", C.c_uint64),
                ("dark", C.c_uint64), ("mirror_ends", C.c_uint64), ("wave_lookups", C.c_uint64)]


class RadianceParams(C.Structure):
    """srt_radiance_params: the sample range, bounces, seed, the id of ray 0's random stream and RADIANCE_* flags."""
    _fields_ = [("first_sample", C.c_uint32), ("sample_count", C.c_uint32), ("max_bounces", C.c_int32), ("seed", C.c_uint32),
                ("id_base", C.c_uint32), ("flags", C.c_uint32)]


class RadianceWork(WorkRecord):
    """srt_radiance_work: what the last counting srt_trace_radiance traced."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("rays", C.c_uint64), ("samples", C.c_uint64),
                ("closest_calls", C.c_uint64), ("wave_calls", C.c_uint64)]


class AdaptiveParams(C.Structure):
    """srt_adaptive_params: the band, bounces, seed, the cap on what one call adds to a pixel and ADAPTIVE_* flags."""
    _fields_ = [("row_begin", C.c_int32), ("row_end", C.c_int32), ("max_bounces", C.c_int32), ("seed", C.c_uint32),
                ("max_samples", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class AdaptiveWork(WorkRecord):
    """srt_adaptive_work: what the last counting srt_render_adaptive traced."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("pixels", C.c_uint64), ("samples", C.c_uint64),
                ("closest_calls", C.c_uint64), ("wave_calls", C.c_uint64)]


class BudgetParams(C.Structure):
    """srt_budget_params: the target relative standard error, the luminance floor, the largest budget and BUDGET_* flags."""
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("max_budget", C.c_uint32), ("flags", C.c_uint32)]


class LightProbeParams(C.Structure):
    """srt_light_probe_params: the sample range, bounces, seed, the id of ray (0, 0)'s random stream, LIGHT_PROBE_* flags and outputs."""
    _fields_ = [("first_sample", C.c_uint32), ("sample_count", C.c_uint32), ("max_bounces", C.c_int32), ("seed", C.c_uint32),
                ("id_base", C.c_uint32), ("flags", C.c_uint32), ("outputs", C.c_uint32), ("reserved", C.c_uint32)]


class LightProbeWork(WorkRecord):
    """srt_light_probe_work: what the last counting srt_trace_light_probes traced."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("probes", C.c_uint64), ("rays", C.c_uint64), ("samples", C.c_uint64),
                ("closest_calls", C.c_uint64), ("wave_calls", C.c_uint64), ("waves", C.c_uint64)]


class ProbeGrid(C.Structure):
    """srt_probe_grid: the position of probe (0, 0, 0), the spacing and the probe counts per axis."""
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("counts", C.c_int32 * 3)]


class ProbeGridParams(C.Structure):
    """srt_probe_grid_params: the band of memory rows, PROBE_GRID_* flags and the weights of SH bands 0, 1, 2."""
    _fields_ = [("row_begin", C.c_int32), ("row_end", C.c_int32), ("flags", C.c_uint32), ("band_weight", C.c_float * 3),
                ("reserved", C.c_uint32 * 2)]


class ProbeGridWork(WorkRecord):
    """srt_probe_grid_work: what the last counting srt_shade_probe_grid did."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("pixels", C.c_uint64), ("corners", C.c_uint64), ("segments", C.c_uint64),
                ("open", C.c_uint64), ("wave_trips", C.c_uint64), ("analytic_tests", C.c_uint64), ("node_visits", C.c_uint64),
                ("triangle_tests", C.c_uint64), ("waves", C.c_uint64)]


class ProbeDepthParams(C.Structure):
    """srt_probe_depth_params: the map resolution, the sharpness of the direction weight, the distance clamp, PROBE_DEPTH_* flags and outputs."""
    _fields_ = [("resolution", C.c_uint32), ("sharpness", C.c_uint32), ("max_distance", C.c_float), ("flags", C.c_uint32),
                ("outputs", C.c_uint32), ("reserved", C.c_uint32)]


class ProbeDepthWork(WorkRecord):
    """srt_probe_depth_work: what the last counting srt_trace_probe_depth traced."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("probes", C.c_uint64), ("rays", C.c_uint64), ("far_rays", C.c_uint64),
                ("wave_calls", C.c_uint64), ("waves", C.c_uint64)]


class ProbeGridDepthParams(C.Structure):
    """srt_probe_grid_depth_params: the bias and the variance floor of the filtered visibility test."""
    _fields_ = [("bias", C.c_float), ("min_variance", C.c_float), ("reserved", C.c_uint32 * 2)]


class ProbeClassifyParams(C.Structure):
    """srt_probe_classify_params: the clearance and the longest offset as fractions of the spacing, the offset steps,
    PROBE_CLASSIFY_* flags and PROBE_STATE_* outputs."""
    _fields_ = [("clearance", C.c_float), ("max_offset", C.c_float), ("steps", C.c_uint32), ("flags", C.c_uint32), ("outputs", C.c_uint32),
                ("reserved", C.c_uint32)]


class ProbeClassifyWork(WorkRecord):
    """srt_probe_classify_work: what the last counting srt_classify_probes found."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("probes", C.c_uint64), ("inside", C.c_uint64), ("moved", C.c_uint64),
                ("buried", C.c_uint64), ("idle", C.c_uint64), ("candidates", C.c_uint64), ("waves", C.c_uint64)]


class ProbeListParams(C.Structure):
    """srt_probe_list_params: the state bits that exclude a probe from the list, PROBE_LIST_COUNT_WORK."""
    _fields_ = [("skip_mask", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class ProbeListWork(WorkRecord):
    """srt_probe_list_work: what the last counting srt_list_probes found."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("probes", C.c_uint64), ("listed", C.c_uint64), ("waves", C.c_uint64)]


class ProbeBlendParams(C.Structure):
    """srt_probe_blend_params: the three hystereses, the change threshold, PROBE_BLEND_* flags."""
    _fields_ = [("hysteresis", C.c_float), ("fast_hysteresis", C.c_float), ("depth_hysteresis", C.c_float), ("change_threshold", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class ProbeBlendWork(WorkRecord):
    """srt_probe_blend_work: what the last counting srt_blend_probes did."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("probes", C.c_uint64), ("restarted", C.c_uint64), ("changed", C.c_uint64),
                ("waves", C.c_uint64)]


class ProbeScrollParams(C.Structure):
    """srt_probe_scroll_params: the shift in cells, the arrays to move (PROBE_SCROLL_COEFFICIENTS | _MOMENTS | _STATES), the flags."""
    _fields_ = [("shift", C.c_int32 * 3), ("which", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class ProbeScrollWork(WorkRecord):
    """srt_probe_scroll_work: what the last counting srt_scroll_probes did."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("probes", C.c_uint64), ("retained", C.c_uint64), ("exposed", C.c_uint64),
                ("waves", C.c_uint64)]


class ProbeCascade(C.Structure):
    """srt_probe_cascade: the level count (level 0 the finest), the resolution of every level's moments (0: none), the width of the
    border band in cells, and the levels' grids."""
    _fields_ = [("levels", C.c_uint32), ("resolution", C.c_uint32), ("blend_cells", C.c_float), ("reserved", C.c_uint32),
                ("grid", ProbeGrid * PROBE_CASCADE_MAX_LEVELS)]


class ProbeCascadeParams(C.Structure):
    """srt_probe_cascade_params: the band of memory rows, PROBE_CASCADE_* flags, the weights of SH bands 0, 1, 2 and rule 7b's bias
    and variance floor."""
    _fields_ = [("row_begin", C.c_int32), ("row_end", C.c_int32), ("flags", C.c_uint32), ("band_weight", C.c_float * 3), ("bias", C.c_float),
                ("min_variance", C.c_float), ("reserved", C.c_uint32 * 2)]


class ProbeCascadeWork(WorkRecord):
    """srt_probe_cascade_work: what the last counting srt_shade_probe_cascade did."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32), ("pixels", C.c_uint64), ("evaluations", C.c_uint64), ("blended", C.c_uint64),
                ("first_level", C.c_uint64 * PROBE_CASCADE_MAX_LEVELS), ("corners", C.c_uint64), ("open", C.c_uint64), ("wave_trips", C.c_uint64),
                ("waves", C.c_uint64), ("spare", C.c_uint64 * 2)]


class UpdateInfo(WorkRecord):
    """srt_update_info: what the last successful srt_update_scene did to the mesh image."""
    _fields_ = [("path", C.c_int32), ("reason", C.c_int32), ("levels", C.c_int32), ("triangles", C.c_uint32), ("nodes", C.c_uint32),
                ("moved_mesh_objects", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("path_samples", C.c_uint64), ("kernel_ms", C.c_float), ("sample_chunks", C.c_uint32),
                ("tile_rows", C.c_uint32), ("chunk_samples", C.c_uint32), ("shape_source", C.c_uint32)]


class WorkCounts(WorkRecord):
    """srt_work_counts: what one render's kernels executed (SRT_RENDER_COUNT_WORK)."""
    _fields_ = [("valid", C.c_uint32), ("reserved", C.c_uint32)] + [(n, C.c_uint64) for n in (
        "waves", "pool_steps", "closest_hit_calls", "uniform_sphere_tests", "cluster_bound_tests", "cluster_sphere_tests",
        "cluster_items", "box_tests", "bvh_child_tests", "triangle_tests", "bvh_node_rounds", "mesh_phases")]


def lib_path():
    return _LIB


def build_native(force=False):
    """hipcc --offload-arch=gfx950 build of the C-ABI library (cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_PKG, "csrc"), "-s"]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return _LIB


_lib = None


def use_dev_library(stats=None, rebuild=False):
    """Development tools only (tests/ab_bench.py, tests/mesh_stats.py, tools/): build and select
    libsrt_pathtrace_dev.so (-DSRT_DEV: environment switches, srt_debug_* entry points, optional STATS
    counters).  Must be called before the first load_library(); the product and the tests never call it."""
    global _LIB
    assert _lib is None, "use_dev_library() must come before load_library()"
    dev = os.path.join(_PKG, "libsrt_pathtrace_dev%s.so" % ("_stats%d" % stats if stats is not None else ""))
    args = ["make", "-C", os.path.join(_PKG, "csrc"), "-s", "dev"]
    if stats is not None:
        args.append("STATS=%d" % stats)
    if rebuild:
        args.append("-B")
    subprocess.check_call(args)
    _LIB = dev
    return dev


def load_library():
    """dlopen libsrt_pathtrace.so and declare prototypes. Raises SrtError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise SrtError(ERR_STATE, "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                  "or `make -C software-raytracer_amd/csrc` (there is no fallback path)" % _LIB)
    _lib = open_library(_LIB)
    return _lib


_ctx = C.c_void_p
# the parameter types of every export, one line each, as include/srt_pathtrace.h declares them (tests/test_capi_exports.py compares)
_PROTOTYPES = {
    "srt_abi_version": [],
    "srt_device_count": [C.POINTER(C.c_int)],
    "srt_create": [C.c_int, C.c_int, C.c_int, C.POINTER(_ctx)],
    "srt_destroy": [_ctx],
    "srt_last_error": [_ctx],
    "srt_set_scene": [_ctx, C.POINTER(Object), C.c_size_t],
    "srt_set_meshes": [_ctx, C.POINTER(Mesh), C.c_size_t],
    "srt_set_environment": [_ctx, C.POINTER(Environment)],
    "srt_environment_default": [C.POINTER(Environment)],
    "srt_set_camera": [_ctx, C.POINTER(Camera)],
    "srt_set_stream": [_ctx, C.c_void_p],
    "srt_bind_output": [_ctx, C.c_void_p, C.c_void_p],
    "srt_device_framebuffer": [_ctx, C.POINTER(C.c_void_p)],
    "srt_device_accumulator": [_ctx, C.POINTER(C.c_void_p)],
    "srt_render": [_ctx, C.POINTER(RenderParams)],
    "srt_wait": [_ctx],
    "srt_poll": [_ctx, C.POINTER(C.c_int)],
    "srt_get_stats": [_ctx, C.POINTER(Stats)],
    "srt_get_work_counts": [_ctx, C.POINTER(WorkCounts)],
    "srt_pick": [_ctx, C.c_int, C.c_int, C.POINTER(C.c_int)],
    "srt_read_framebuffer": [_ctx, C.c_void_p, C.c_size_t, C.c_int, C.c_int],
    "srt_read_framebuffer_async": [_ctx, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p],
    "srt_read_accumulator": [_ctx, C.POINTER(C.c_float)],
    "srt_write_accumulator": [_ctx, C.POINTER(C.c_float)],
    "srt_gather_band": [_ctx, _ctx, C.c_int, C.c_int],
    "srt_gather_path": [_ctx],
    "srt_estimate_row_costs": [_ctx, C.c_int, C.c_uint32, C.POINTER(C.c_float)],
    "srt_selftest_arith": [C.c_int, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)],
    "srt_render_gbuffer": [_ctx, C.POINTER(GBufferParams)],
    "srt_bind_gbuffer": [_ctx, C.c_uint32, C.c_void_p],
    "srt_read_gbuffer": [_ctx, C.c_uint32, C.c_void_p],
    "srt_denoise_params_default": [C.POINTER(DenoiseParams)],
    "srt_denoise": [_ctx, C.POINTER(DenoiseParams)],
    "srt_bind_denoised": [_ctx, C.c_void_p],
    "srt_read_denoised": [_ctx, C.POINTER(C.c_float)],
    "srt_temporal_params_default": [C.POINTER(TemporalParams)],
    "srt_temporal_accumulate": [_ctx, C.POINTER(TemporalParams)],
    "srt_read_history_length": [_ctx, C.POINTER(C.c_float)],
    "srt_update_scene": [_ctx, C.POINTER(Object), C.c_size_t],
    "srt_motion_output": [_ctx, C.c_int],
    "srt_bind_motion": [_ctx, C.c_void_p],
    "srt_read_motion": [_ctx, C.POINTER(C.c_float)],
    "srt_upsample_params_default": [C.POINTER(UpsampleParams)],
    "srt_upsample": [_ctx, C.POINTER(UpsampleParams)],
    "srt_bind_upsampled": [_ctx, C.c_void_p],
    "srt_read_upsampled": [_ctx, C.POINTER(C.c_float)],
    "srt_render_subsamples": [_ctx, C.POINTER(SubsampleParams)],
    "srt_bind_subsamples": [_ctx, C.c_void_p],
    "srt_read_subsamples": [_ctx, C.POINTER(C.c_int32)],
    "srt_antialias_params_default": [C.POINTER(AntialiasParams)],
    "srt_antialias": [_ctx, C.POINTER(AntialiasParams)],
    "srt_bind_antialiased": [_ctx, C.c_void_p],
    "srt_read_antialiased": [_ctx, C.POINTER(C.c_float)],
    "srt_variance_params_default": [C.POINTER(VarianceParams)],
    "srt_device_half": [_ctx, C.POINTER(C.c_void_p)],
    "srt_bind_half": [_ctx, C.c_void_p],
    "srt_variance": [_ctx, C.POINTER(VarianceParams)],
    "srt_bind_variance": [_ctx, C.c_void_p],
    "srt_read_variance": [_ctx, C.POINTER(C.c_float)],
    "srt_denoise_variance_params_default": [C.POINTER(DenoiseVarianceParams)],
    "srt_denoise_variance": [_ctx, C.POINTER(DenoiseVarianceParams)],
    "srt_moments_output": [_ctx, C.c_int, C.c_uint32],
    "srt_read_moments": [_ctx, C.POINTER(C.c_float)],
    "srt_temporal_variance_params_default": [C.POINTER(TemporalVarianceParams)],
    "srt_temporal_variance": [_ctx, C.POINTER(TemporalVarianceParams)],
    "srt_update_mode": [_ctx, C.c_int],
    "srt_get_update_info": [_ctx, C.POINTER(UpdateInfo)],
    "srt_mesh_image_size": [_ctx, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)],
    "srt_read_mesh_image": [_ctx, C.c_void_p, C.c_void_p],
    "srt_trace_params_default": [C.POINTER(TraceParams)],
    "srt_write_rays": [_ctx, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_size_t],
    "srt_bind_rays": [_ctx, C.c_void_p, C.c_void_p, C.c_size_t],
    "srt_bind_ray_output": [_ctx, C.c_uint32, C.c_void_p],
    "srt_trace_rays": [_ctx, C.POINTER(TraceParams)],
    "srt_read_ray_output": [_ctx, C.c_uint32, C.c_void_p],
    "srt_occlusion_params_default": [C.POINTER(OcclusionParams)],
    "srt_trace_occlusion": [_ctx, C.POINTER(OcclusionParams)],
    "srt_get_occlusion_work": [_ctx, C.POINTER(OcclusionWork)],
    "srt_visibility_params_default": [C.POINTER(VisibilityParams)],
    "srt_render_visibility": [_ctx, C.POINTER(VisibilityParams)],
    "srt_bind_visibility": [_ctx, C.c_uint32, C.c_void_p],
    "srt_read_visibility": [_ctx, C.c_uint32, C.POINTER(C.c_float)],
    "srt_get_visibility_work": [_ctx, C.POINTER(VisibilityWork)],
    "srt_reflection_params_default": [C.POINTER(ReflectionParams)],
    "srt_render_reflection_gbuffer": [_ctx, C.POINTER(ReflectionParams)],
    "srt_bind_reflection": [_ctx, C.c_uint32, C.c_void_p],
    "srt_read_reflection": [_ctx, C.c_uint32, C.c_void_p],
    "srt_device_reflection": [_ctx, C.c_uint32, C.POINTER(C.c_void_p)],
    "srt_get_reflection_work": [_ctx, C.POINTER(ReflectionWork)],
    "srt_mirror_history_params_default": [C.POINTER(MirrorHistoryParams)],
    "srt_mirror_history": [_ctx, C.POINTER(MirrorHistoryParams)],
    "srt_probe_tail_params_default": [C.POINTER(ProbeTailParams)],
    "srt_probe_tail": [_ctx, C.POINTER(ProbeTailParams)],
    "srt_get_probe_tail_work": [_ctx, C.POINTER(ProbeTailWork)],
    "srt_radiance_params_default": [C.POINTER(RadianceParams)],
    "srt_trace_radiance": [_ctx, C.POINTER(RadianceParams)],
    "srt_bind_radiance": [_ctx, C.c_void_p],
    "srt_read_radiance": [_ctx, C.POINTER(C.c_float)],
    "srt_get_radiance_work": [_ctx, C.POINTER(RadianceWork)],
    "srt_write_light_probes": [_ctx, C.POINTER(C.c_float), C.c_size_t],
    "srt_bind_light_probes": [_ctx, C.c_void_p, C.c_size_t],
    "srt_write_light_probe_directions": [_ctx, C.POINTER(C.c_float), C.c_size_t],
    "srt_bind_light_probe_directions": [_ctx, C.c_void_p, C.c_size_t],
    "srt_light_probe_params_default": [C.POINTER(LightProbeParams)],
    "srt_trace_light_probes": [_ctx, C.POINTER(LightProbeParams)],
    "srt_bind_light_probe_output": [_ctx, C.c_uint32, C.c_void_p],
    "srt_read_light_probe_output": [_ctx, C.c_uint32, C.c_void_p],
    "srt_get_light_probe_work": [_ctx, C.POINTER(LightProbeWork)],
    "srt_light_probe_sphere": [C.c_size_t, C.POINTER(C.c_float)],
    "srt_light_probe_irradiance": [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)],
    "srt_probe_grid_positions": [C.POINTER(ProbeGrid), C.POINTER(C.c_float)],
    "srt_probe_grid_params_default": [C.POINTER(ProbeGridParams)],
    "srt_set_probe_grid": [_ctx, C.POINTER(ProbeGrid)],
    "srt_write_probe_grid_coefficients": [_ctx, C.POINTER(C.c_float), C.c_size_t],
    "srt_bind_probe_grid_coefficients": [_ctx, C.c_void_p, C.c_size_t],
    "srt_shade_probe_grid": [_ctx, C.POINTER(ProbeGridParams)],
    "srt_bind_probe_grid_output": [_ctx, C.c_void_p],
    "srt_read_probe_grid_output": [_ctx, C.POINTER(C.c_float)],
    "srt_get_probe_grid_work": [_ctx, C.POINTER(ProbeGridWork)],
    "srt_probe_depth_params_default": [C.POINTER(ProbeDepthParams)],
    "srt_probe_depth_texels": [C.c_uint32, C.POINTER(C.c_float)],
    "srt_trace_probe_depth": [_ctx, C.POINTER(ProbeDepthParams)],
    "srt_bind_probe_depth_output": [_ctx, C.c_uint32, C.c_void_p],
    "srt_read_probe_depth_output": [_ctx, C.c_uint32, C.c_void_p],
    "srt_get_probe_depth_work": [_ctx, C.POINTER(ProbeDepthWork)],
    "srt_probe_grid_depth_params_default": [C.POINTER(ProbeGridDepthParams)],
    "srt_write_probe_grid_depth": [_ctx, C.POINTER(C.c_float), C.c_size_t, C.c_uint32],
    "srt_bind_probe_grid_depth": [_ctx, C.c_void_p, C.c_size_t, C.c_uint32],
    "srt_shade_probe_grid_depth": [_ctx, C.POINTER(ProbeGridParams), C.POINTER(ProbeGridDepthParams)],
    "srt_probe_classify_params_default": [C.POINTER(ProbeClassifyParams)],
    "srt_classify_probes": [_ctx, C.POINTER(ProbeClassifyParams)],
    "srt_bind_probe_states_output": [_ctx, C.c_uint32, C.c_void_p],
    "srt_read_probe_states_output": [_ctx, C.c_uint32, C.c_void_p],
    "srt_get_probe_classify_work": [_ctx, C.POINTER(ProbeClassifyWork)],
    "srt_write_probe_grid_states": [_ctx, C.POINTER(C.c_float), C.c_size_t],
    "srt_bind_probe_grid_states": [_ctx, C.c_void_p, C.c_size_t],
    "srt_shade_probe_grid_states": [_ctx, C.POINTER(ProbeGridParams), C.POINTER(ProbeGridDepthParams)],
    "srt_probe_list_params_default": [C.POINTER(ProbeListParams)],
    "srt_list_probes": [_ctx, C.POINTER(ProbeListParams)],
    "srt_bind_probe_list_output": [_ctx, C.c_void_p],
    "srt_read_probe_list_output": [_ctx, C.POINTER(C.c_uint32)],
    "srt_get_probe_list_work": [_ctx, C.POINTER(ProbeListWork)],
    "srt_bind_probe_list": [_ctx, C.c_void_p, C.c_size_t],
    "srt_write_probe_list": [_ctx, C.POINTER(C.c_uint32), C.c_size_t],
    "srt_trace_light_probes_listed": [_ctx, C.POINTER(LightProbeParams)],
    "srt_trace_probe_depth_listed": [_ctx, C.POINTER(ProbeDepthParams)],
    "srt_probe_blend_params_default": [C.POINTER(ProbeBlendParams)],
    "srt_reset_probe_history": [_ctx, C.c_uint32, C.c_size_t, C.c_uint32],
    "srt_bind_probe_history": [_ctx, C.c_uint32, C.c_void_p],
    "srt_read_probe_history": [_ctx, C.c_uint32, C.POINTER(C.c_float)],
    "srt_write_probe_previous_states": [_ctx, C.POINTER(C.c_float), C.c_size_t],
    "srt_bind_probe_previous_states": [_ctx, C.c_void_p, C.c_size_t],
    "srt_blend_probes": [_ctx, C.POINTER(ProbeBlendParams)],
    "srt_get_probe_blend_work": [_ctx, C.POINTER(ProbeBlendWork)],
    "srt_probe_scroll_params_default": [C.POINTER(ProbeScrollParams)],
    "srt_scroll_probes": [_ctx, C.POINTER(ProbeScrollParams)],
    "srt_get_probe_scroll_work": [_ctx, C.POINTER(ProbeScrollWork)],
    "srt_read_probe_previous_states": [_ctx, C.POINTER(C.c_float)],
    "srt_probe_grid_follow": [C.POINTER(ProbeGrid), C.POINTER(C.c_float), C.POINTER(C.c_int32)],
    "srt_probe_cascade_params_default": [C.POINTER(ProbeCascadeParams)],
    "srt_probe_cascade_grids": [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(ProbeCascade)],
    "srt_probe_cascade_weights": [C.POINTER(ProbeCascade), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float)],
    "srt_set_probe_cascade": [_ctx, C.POINTER(ProbeCascade)],
    "srt_write_probe_cascade_level": [_ctx, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.c_size_t],
    "srt_bind_probe_cascade_level": [_ctx, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t],
    "srt_capture_probe_cascade_level": [_ctx, C.c_uint32, C.c_uint32],
    "srt_shade_probe_cascade": [_ctx, C.POINTER(ProbeCascadeParams)],
    "srt_get_probe_cascade_work": [_ctx, C.POINTER(ProbeCascadeWork)],
    "srt_set_sample_counts": [_ctx, C.c_uint32],
    "srt_write_sample_counts": [_ctx, C.POINTER(C.c_uint32)],
    "srt_read_sample_counts": [_ctx, C.POINTER(C.c_uint32)],
    "srt_bind_sample_counts": [_ctx, C.c_void_p],
    "srt_write_sample_budget": [_ctx, C.POINTER(C.c_uint32)],
    "srt_read_sample_budget": [_ctx, C.POINTER(C.c_uint32)],
    "srt_bind_sample_budget": [_ctx, C.c_void_p],
    "srt_adaptive_params_default": [C.POINTER(AdaptiveParams)],
    "srt_render_adaptive": [_ctx, C.POINTER(AdaptiveParams)],
    "srt_get_adaptive_work": [_ctx, C.POINTER(AdaptiveWork)],
    "srt_render_adaptive_tail": [_ctx, C.POINTER(AdaptiveParams)],
    "srt_budget_params_default": [C.POINTER(BudgetParams)],
    "srt_sample_budget": [_ctx, C.POINTER(BudgetParams)],
    "srt_get_budget_total": [_ctx, C.POINTER(C.c_uint64)],
}
# every export returns an srt_status int but these
_RESTYPES = {"srt_last_error": C.c_char_p, "srt_gather_path": C.c_char_p}
# exports a build of an earlier commit may lack (tests/ab_passes.py and tests/ab_libs.py open such builds next to this one)
_OPTIONAL_EXPORTS = ("srt_probe_tail_params_default", "srt_probe_tail", "srt_get_probe_tail_work", "srt_render_adaptive_tail")


def open_library(path):
    """dlopen one build of the C-ABI library and declare its prototypes (load_library() for the product's; development
    tools open several builds side by side for interleaved A/B timing, tests/ab_libs.py)."""
    L = C.CDLL(path)
    for name, argtypes in _PROTOTYPES.items():
        if name in _OPTIONAL_EXPORTS and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, _RESTYPES.get(name, C.c_int)
    return L


# the names the calls below accept for the bits of an output, a history or a set of arrays (the image outputs, with their dtypes and
# channels, are GBUFFERS, REFLECTION, RAY_OUTPUTS and VISIBILITY above)
LIGHT_PROBE_OUTPUTS = {"coefficients": LIGHT_PROBE_COEFFICIENTS, "radiance": LIGHT_PROBE_RADIANCE}
PROBE_DEPTH_OUTPUTS = {"moments": PROBE_DEPTH_MOMENTS, "distances": PROBE_DEPTH_DISTANCES}
PROBE_STATE_OUTPUTS = {"records": PROBE_STATE_RECORDS, "positions": PROBE_STATE_POSITIONS}
PROBE_HISTORIES = {"coefficients": PROBE_HISTORY_COEFFICIENTS, "moments": PROBE_HISTORY_MOMENTS,
                   "both": PROBE_HISTORY_COEFFICIENTS | PROBE_HISTORY_MOMENTS}
PROBE_SCROLL_ARRAYS = {"coefficients": PROBE_SCROLL_COEFFICIENTS, "moments": PROBE_SCROLL_MOMENTS, "states": PROBE_SCROLL_STATES,
                       "both": PROBE_SCROLL_COEFFICIENTS | PROBE_SCROLL_MOMENTS,
                       "all": PROBE_SCROLL_COEFFICIENTS | PROBE_SCROLL_MOMENTS | PROBE_SCROLL_STATES}
PROBE_CASCADE_ARRAYS = {"coefficients": PROBE_CASCADE_COEFFICIENTS, "moments": PROBE_CASCADE_MOMENTS, "records": PROBE_CASCADE_RECORDS,
                        "all": PROBE_CASCADE_COEFFICIENTS | PROBE_CASCADE_MOMENTS | PROBE_CASCADE_RECORDS}


def _spec(table, name, what=None):
    """The entry of one name in a name table.  An unknown name is a ValueError that lists the table's names when `what` says what
    the table holds, else the table's own KeyError."""
    if what is not None and name not in table:
        raise ValueError("unknown %s %r (one of %s)" % (what, name, ", ".join(table)))
    return table[name]


def _mask(table, names, what=None):
    """A bit mask from an int (the mask itself), a name of `table` or a sequence of names; unknown names as _spec() refuses them."""
    if isinstance(names, (int, np.integer)):
        return int(names)
    mask = 0
    for name in ([names] if isinstance(names, str) else names):
        entry = _spec(table, name, what)
        mask |= entry[0] if isinstance(entry, tuple) else entry
    return mask


def _bit(table, which):
    """One selector: a name of `table`, or the bits themselves (anything int() takes)."""
    return int(table[which] if which in table else which)


def gbuffer_outputs(outputs):
    """An SRT_GBUF_* mask from an int or from names of GBUFFERS ("object", "normal_depth", "position", "albedo")."""
    return _mask(GBUFFERS, outputs, "G-buffer output")


def reflection_outputs(outputs):
    """An SRT_REFL_* mask from an int or from names of REFLECTION (GBUFFERS' four and "bounces")."""
    return _mask(REFLECTION, outputs, "reflection output")


def ray_outputs(outputs):
    """An output mask of srt_trace_rays from an int or from names of RAY_OUTPUTS ("object", "normal_depth", "position",
    "albedo", "occluded")."""
    return _mask(RAY_OUTPUTS, outputs, "ray output")


def _set(p, **fields):
    """Set the fields of struct `p` that were given (None: the field keeps its value), coerced by the field's ctype: float() for a
    c_float, int() for the integer types, an array field element by element from a sequence.  Returns p."""
    ctypes_of = dict(p._fields_)
    for name, value in fields.items():
        if value is None:
            continue
        t = ctypes_of[name]
        if issubclass(t, C.Array):
            coerce = float if t._type_ is C.c_float else int
            array = getattr(p, name)
            for i in range(t._length_):
                array[i] = coerce(value[i])
        else:
            setattr(p, name, float(value) if t is C.c_float else int(value))
    return p


def _default_params(struct, symbol, lib=None):
    """One parameter struct filled with the library's defaults (pure host: no GPU needed)."""
    p = struct()
    rc = getattr(lib if lib is not None else load_library(), symbol)(C.byref(p))
    if rc:
        raise SrtError(rc, symbol)
    return p


def _defaults_function(name, struct, symbol):
    def defaults(lib=None):
        p = _default_params(struct, symbol, lib)
        return {n: getattr(p, n) for n, _ in struct._fields_}

    defaults.__name__ = defaults.__qualname__ = name
    defaults.__doc__ = "%s as a dict (pure host: no GPU needed)." % symbol
    return defaults


# trace_defaults(lib=None), denoise_defaults(lib=None), ...: the library's defaults of a parameter struct as a dict; and
# TRACE_DEFAULTS, DENOISE_DEFAULTS, ...: the same, read when first asked for, so that importing this module does not need the built
# library (and never kept: `lib` exists so that two builds can be driven side by side)
_DEFAULTS = (
    ("trace_defaults", TraceParams, "srt_trace_params_default"),
    ("denoise_defaults", DenoiseParams, "srt_denoise_params_default"),
    ("temporal_defaults", TemporalParams, "srt_temporal_params_default"),
    ("upsample_defaults", UpsampleParams, "srt_upsample_params_default"),
    ("antialias_defaults", AntialiasParams, "srt_antialias_params_default"),
    ("variance_defaults", VarianceParams, "srt_variance_params_default"),
    ("denoise_variance_defaults", DenoiseVarianceParams, "srt_denoise_variance_params_default"),
    ("temporal_variance_defaults", TemporalVarianceParams, "srt_temporal_variance_params_default"),
)
_LAZY_DEFAULTS = {}
for _name, _struct, _symbol in _DEFAULTS:
    globals()[_name] = _LAZY_DEFAULTS[_name.upper()] = _defaults_function(_name, _struct, _symbol)


def __getattr__(name):
    if name in _LAZY_DEFAULTS:
        return _LAZY_DEFAULTS[name]()
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def denoise_params(iterations=None, sigma_color=None, sigma_normal=None, sigma_plane=None, albedo=True, framebuffer=False, lib=None):
    """A DenoiseParams: the library defaults, with every argument that is not None put in their place."""
    flags = (DENOISE_ALBEDO if albedo else 0) | (DENOISE_FRAMEBUFFER if framebuffer else 0)
    return _set(_default_params(DenoiseParams, "srt_denoise_params_default", lib), iterations=iterations, sigma_color=sigma_color,
                sigma_normal=sigma_normal, sigma_plane=sigma_plane, flags=flags)


def temporal_params(samples=1, max_samples=None, plane_tolerance=None, normal_threshold=None, reset=False, framebuffer=False,
                    lib=None):
    """A TemporalParams: the library defaults, with every argument that is not None put in their place."""
    flags = (TEMPORAL_RESET if reset else 0) | (TEMPORAL_FRAMEBUFFER if framebuffer else 0)
    return _set(_default_params(TemporalParams, "srt_temporal_params_default", lib), samples=int(samples), max_samples=max_samples,
                plane_tolerance=plane_tolerance, normal_threshold=normal_threshold, flags=flags)


def upsample_params(steps=None, stripe_width=None, sigma_normal=None, sigma_plane=None, in_place=False, framebuffer=False, lib=None):
    """An UpsampleParams: the library defaults, with every argument that is not None put in their place."""
    flags = (UPSAMPLE_IN_PLACE if in_place else 0) | (UPSAMPLE_FRAMEBUFFER if framebuffer else 0)
    return _set(_default_params(UpsampleParams, "srt_upsample_params_default", lib), steps=steps, stripe_width=stripe_width,
                sigma_normal=sigma_normal, sigma_plane=sigma_plane, flags=flags)


def antialias_params(k=None, denoised=False, framebuffer=False, lib=None):
    """An AntialiasParams: the library's default k unless one is given, the source and the flag by name."""
    return _set(_default_params(AntialiasParams, "srt_antialias_params_default", lib), k=k,
                source=AA_SOURCE_DENOISED if denoised else AA_SOURCE_ACCUMULATOR, flags=AA_FRAMEBUFFER if framebuffer else 0)


def variance_params(albedo=None, merge=None, lib=None):
    """A VarianceParams: the library's default flags, each overridden by name when given."""
    p = _default_params(VarianceParams, "srt_variance_params_default", lib)
    for bit, on in ((VARIANCE_ALBEDO, albedo), (VARIANCE_MERGE, merge)):
        if on is not None:
            p.flags = (p.flags | bit) if on else (p.flags & ~bit)
    return p


def denoise_variance_params(iterations=None, sigma_luminance=None, sigma_normal=None, sigma_plane=None, albedo=True,
                            framebuffer=False, lib=None):
    """A DenoiseVarianceParams: the library's defaults with the given fields replaced and the flags by name."""
    flags = (DENOISE_ALBEDO if albedo else 0) | (DENOISE_FRAMEBUFFER if framebuffer else 0)
    return _set(_default_params(DenoiseVarianceParams, "srt_denoise_variance_params_default", lib), iterations=iterations,
                sigma_luminance=sigma_luminance, sigma_normal=sigma_normal, sigma_plane=sigma_plane, flags=flags)


def temporal_variance_params(min_frames=None, radius=None, lib=None):
    """A TemporalVarianceParams: the library's defaults with the given fields replaced."""
    return _set(_default_params(TemporalVarianceParams, "srt_temporal_variance_params_default", lib), min_frames=min_frames, radius=radius)


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def default_environment():
    e = Environment()
    rc = load_library().srt_environment_default(C.byref(e))
    if rc:
        raise SrtError(rc, "srt_environment_default")
    return e


def light_probe_sphere(count, lib=None):
    """srt_light_probe_sphere: `count` spherical Fibonacci directions as a (count, 4) float32 array: a unit direction and the
    weight 4 pi / count.  Pure host."""
    L = lib or load_library()
    n = int(count)
    if n < 1:
        raise SrtError(ERR_INVALID_ARG, "srt_light_probe_sphere: want count >= 1, got %d" % n)
    out = np.empty((n, 4), dtype=np.float32)
    rc = L.srt_light_probe_sphere(n, out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        raise SrtError(rc, "srt_light_probe_sphere(%d)" % n)
    return out


def probe_depth_texels(resolution, lib=None):
    """srt_probe_depth_texels: the unit directions of the R x R texels of a probe's octahedral depth map as an (R*R, 4) float32
    array, texel (i, j) at index j*R + i, w = 0.  Pure host."""
    L = lib or load_library()
    r = int(resolution)
    if r not in PROBE_DEPTH_RESOLUTIONS:
        raise SrtError(ERR_INVALID_ARG, "srt_probe_depth_texels: want a resolution of 4, 8 or 16, got %d" % r)
    out = np.empty((r * r, 4), dtype=np.float32)
    rc = L.srt_probe_depth_texels(r, out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc:
        raise SrtError(rc, "srt_probe_depth_texels(%d)" % r)
    return out


def probe_grid(origin, spacing, counts):
    """An srt_probe_grid from three triples (a ProbeGrid passes through)."""
    if isinstance(origin, ProbeGrid) and spacing is None and counts is None:
        return origin
    g = ProbeGrid()
    for a in range(3):
        g.origin[a], g.spacing[a], g.counts[a] = float(origin[a]), float(spacing[a]), int(counts[a])
    return g


def probe_grid_follow(grid, point, lib=None):
    """srt_probe_grid_follow: the shift (sx, sy, sz), in cells, that re-centres `grid` (a ProbeGrid, or a triple of triples) on
    `point`: per axis (point - centre) / spacing truncated towards zero.  Pure host."""
    L = lib or load_library()
    g = grid if isinstance(grid, ProbeGrid) else probe_grid(*grid)
    pt = (C.c_float * 3)(*[float(v) for v in point])
    shift = (C.c_int32 * 3)()
    rc = L.srt_probe_grid_follow(C.byref(g), pt, shift)
    if rc != OK:
        raise SrtError(rc, "srt_probe_grid_follow: not a grid srt_set_probe_grid accepts")
    return tuple(int(v) for v in shift)


def probe_cascade(grids, resolution=0, blend_cells=1.0):
    """An srt_probe_cascade from 1 .. 4 grids (ProbeGrid, or triples of triples), finest first (a ProbeCascade passes through)."""
    if isinstance(grids, ProbeCascade):
        return grids
    c = ProbeCascade()
    c.levels, c.resolution, c.blend_cells, c.reserved = len(grids), int(resolution), float(blend_cells), 0
    for l, g in enumerate(grids[:PROBE_CASCADE_MAX_LEVELS]):
        g = g if isinstance(g, ProbeGrid) else probe_grid(*g)
        for a in range(3):
            c.grid[l].origin[a], c.grid[l].spacing[a], c.grid[l].counts[a] = g.origin[a], g.spacing[a], g.counts[a]
    return c


def probe_cascade_grids(centre, base_spacing, counts, levels, lib=None):
    """srt_probe_cascade_grids: a ProbeCascade of `levels` grids of `counts` probes around `centre`, level l with spacing
    base_spacing * 2^l and its origin snapped to whole cells of its own spacing; blend_cells 1, resolution 0.  Pure host."""
    L = lib or load_library()
    out = ProbeCascade()
    rc = L.srt_probe_cascade_grids((C.c_float * 3)(*[float(v) for v in centre]), (C.c_float * 3)(*[float(v) for v in base_spacing]),
                                   (C.c_int32 * 3)(*[int(v) for v in counts]), int(levels), C.byref(out))
    if rc != OK:
        raise SrtError(rc, "srt_probe_cascade_grids: levels outside 1 .. 4, or not grids srt_set_probe_grid accepts")
    return out


def probe_cascade_weights(cascade, point, lib=None):
    """srt_probe_cascade_weights: (first_level, evaluations, beta) of rule C2 for one point: the finest level that holds it (the
    coarsest when none does), whether it is blended into the next (2) or not (1), and that level's weight.  Pure host."""
    L = lib or load_library()
    c = probe_cascade(cascade)
    f, k, b = C.c_int32(), C.c_int32(), C.c_float()
    rc = L.srt_probe_cascade_weights(C.byref(c), (C.c_float * 3)(*[float(v) for v in point]), C.byref(f), C.byref(k), C.byref(b))
    if rc != OK:
        raise SrtError(rc, "srt_probe_cascade_weights: not a cascade srt_set_probe_cascade accepts")
    return int(f.value), int(k.value), np.float32(b.value)


def probe_grid_positions(origin, spacing=None, counts=None, lib=None):
    """srt_probe_grid_positions: the positions of the grid's probes as an (nx*ny*nz, 4) float32 array in index order
    ix + nx*(iy + ny*iz), w = 0 — what trace_light_probes() takes.  `origin`: a ProbeGrid, or three triples.  Pure host."""
    L = lib or load_library()
    g = probe_grid(origin, spacing, counts)
    n = [int(c) for c in g.counts]
    if min(n) < 1 or n[0] * n[1] * n[2] > 1 << 30:
        raise SrtError(ERR_INVALID_ARG, "srt_probe_grid_positions: counts %s" % (n,))
    out = np.empty((n[0] * n[1] * n[2], 4), dtype=np.float32)
    rc = L.srt_probe_grid_positions(C.byref(g), out.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != OK:
        raise SrtError(rc, "srt_probe_grid_positions")
    return out


def light_probe_irradiance(coefficients, normal, lib=None):
    """srt_light_probe_irradiance: the irradiance (r, g, b) at the unit `normal` from a probe's coefficients, an array (9, 4)
    float32 as light_probe_coefficients() returns per probe.  Pure host."""
    L = lib or load_library()
    c = np.ascontiguousarray(coefficients, dtype=np.float32)
    n = np.ascontiguousarray(normal, dtype=np.float32).reshape(-1)
    if c.shape != (LIGHT_PROBE_COEFFS, 4) or n.shape[0] < 3:
        raise ValueError("light_probe_irradiance: coefficients %s and normal %s, want (9, 4) and (3,)" % (c.shape, n.shape))
    out = np.empty(3, dtype=np.float32)
    f = C.POINTER(C.c_float)
    rc = L.srt_light_probe_irradiance(c.ctypes.data_as(f), n.ctypes.data_as(f), out.ctypes.data_as(f))
    if rc:
        raise SrtError(rc, "srt_light_probe_irradiance")
    return out


def default_camera(fov=55):
    """Raytracer.cpp:295-297 (origin, identity basis) and FOV :31."""
    c = Camera()
    c.position = _f3((0, 0, 0))
    c.right = _f3((1, 0, 0))
    c.up = _f3((0, 1, 0))
    c.forward = _f3((0, 0, 1))
    c.fov_degrees = fov
    return c


class PathTracer:
    """Thin RAII wrapper of an srt_context handle."""

    def __init__(self, width, height, device=0, lib=None):
        self.L = lib if lib is not None else load_library()
        self.width, self.height = int(width), int(height)
        self.device = int(device)
        self._h = C.c_void_p()
        rc = self.L.srt_create(int(device), self.width, self.height, C.byref(self._h))
        if rc:
            raise SrtError(rc, (self.L.srt_last_error(None) or b"").decode())
        # What this object remembers of its calls: sizes the readers shape their arrays by, switches that change what a later
        # call enqueues, and the tensors bound by address, which stay referenced for as long as they are bound.
        self._ray_count = None  # rays of the current batch (written or bound)
        self._ray_own_count = None  # rays in the handle's own buffers, current again after bind_rays(None, None)
        self._ray_bound = None  # (origins, directions) tensors of bind_rays
        self._ray_out_bound = {}  # output name -> tensor of bind_ray_output
        self._ray_traced = None  # rays of the last trace_rays / trace_occlusion: ray_output()'s length
        self._radiance_bound = None  # tensor of bind_radiance
        self._radiance_traced = None  # rays of the last trace_radiance: radiance()'s length
        self._reflection_guides = False  # use_reflection_guides(): gbuffer=True renders the reflection guides
        self._mirror_history = False  # mirror_history(): temporal(gbuffer=True) also renders the reflection outputs it reads
        self._moments_albedo = False  # moments_output(albedo=True): temporal(gbuffer=True) also renders the ALBEDO guide
        self._subsample_k = 0  # k of the last render_subsamples / bind_subsamples: subsamples()'s shape
        self._probe_count = None  # current probe positions (written or bound)
        self._probe_bound = None  # positions tensor, while bound
        self._probe_dir_count = None  # current shared directions (written or bound)
        self._probe_dir_bound = None  # directions tensor, while bound
        self._probe_out_bound = {}  # LIGHT_PROBE_* bit -> tensor of bind_light_probe_output
        self._probes_traced = (None, None)  # (probes, directions) of the last trace_light_probes: its readers' shapes
        self._probe_grid_probes = None  # probes of the grid of set_probe_grid
        self._probe_grid_bound = None  # coefficients tensor a shade_probe_grid* call bound
        self._probe_grid_out_bound = None  # tensor of bind_probe_grid_output
        self._probe_depth_bound = {}  # PROBE_DEPTH_* bit -> tensor of bind_probe_depth_output
        self._probe_depth_traced = None  # (probes, directions, resolution) of the last trace_probe_depth
        self._probe_grid_depth_bound = None  # moments tensor of bind_probe_grid_depth
        self._probe_states_bound = {}  # PROBE_STATE_* bit -> tensor of bind_probe_states_output
        self._probe_states_classified = None  # probes of the last classify_probes: probe_states_output()'s length
        self._probe_grid_states_bound = None  # records tensor of bind_probe_grid_states
        self._probe_list_out_bound = None  # tensor of bind_probe_list_output
        self._probe_list_bound = None  # tensor of bind_probe_list
        self._probe_history_sizes = {}  # PROBE_HISTORY_* bit -> (probes, resolution) of reset_probe_history
        self._probe_history_bound = {}  # PROBE_HISTORY_* bit -> tensor of bind_probe_history
        self._probe_previous_bound = None  # records tensor of bind_probe_previous_states
        self._probe_cascade = None  # the ProbeCascade of set_probe_cascade
        self._probe_cascade_bound = {}  # (level, PROBE_CASCADE_* bit) -> tensor of bind_probe_cascade_level

    def _ck(self, rc):
        if rc:
            raise SrtError(rc, (self.L.srt_last_error(self._h) or b"").decode())

    def _default(self, struct, fn):
        """A parameter struct filled by one srt_*_params_default of this tracer's library."""
        p = struct()
        self._ck(fn(C.byref(p)))
        return p

    def _band(self, rows):
        """A band of memory rows as (begin, end); None: the whole frame."""
        return (int(rows[0]), int(rows[1])) if rows is not None else (0, self.height)

    def _get_record(self, struct, fn):
        """One srt_get_*: a new `struct` filled by fn(handle, pointer to it)."""
        record = struct()
        self._ck(fn(self._h, C.byref(record)))
        return record

    def _get_work(self, struct, fn):
        """The record a counting call left, as a dict (WorkRecord.as_dict).  Waits."""
        return self._get_record(struct, fn).as_dict()

    def close(self):
        if self._h:
            self.L.srt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- state ---------------------------------------------------------------------
    def set_scene(self, objects, count=None):
        n = len(objects) if count is None else count
        ptr = C.cast(objects, C.POINTER(Object)) if n else None
        self._ck(self.L.srt_set_scene(self._h, ptr, n))

    def update_scene(self, objects, count=None):
        """srt_update_scene: set_scene for a list of the same length that keeps the temporal history; the next temporal()
        reprojects every object by how far its position moved since the previous one."""
        n = len(objects) if count is None else count
        ptr = C.cast(objects, C.POINTER(Object)) if n else None
        self._ck(self.L.srt_update_scene(self._h, ptr, n))

    def update_mode(self, refit=True):
        """srt_update_mode: let update_scene() refit the mesh BVH on the device when the lists differ only in positions
        (refit=False: rebuild it every time, the default)."""
        self._ck(self.L.srt_update_mode(self._h, UPDATE_REFIT if refit else UPDATE_REBUILD))

    def update_info(self):
        """srt_get_update_info: what the last update_scene() did, as a dict (path 1 rebuilt, 2 refitted, 3 kept; UPDATE_PATHS)."""
        return self._get_work(UpdateInfo, self.L.srt_get_update_info)

    def mesh_image(self):
        """srt_read_mesh_image: the mesh image as the kernels read it: (nodes (N, 5, 4) float32, triangles (T, 3, 4) float32)."""
        nb, tb = C.c_size_t(0), C.c_size_t(0)
        self._ck(self.L.srt_mesh_image_size(self._h, C.byref(nb), C.byref(tb)))
        nodes = np.empty((nb.value // 80, 5, 4), dtype=np.float32)
        tris = np.empty((tb.value // 48, 3, 4), dtype=np.float32)
        self._ck(self.L.srt_read_mesh_image(self._h, nodes.ctypes.data_as(C.c_void_p), tris.ctypes.data_as(C.c_void_p)))
        return nodes, tris

    def set_meshes(self, meshes, count=None):
        """EXTENSION: geometry for SRT_OBJ_MESH objects; call before set_scene."""
        n = len(meshes) if count is None else count
        self._ck(self.L.srt_set_meshes(self._h, C.cast(meshes, C.POINTER(Mesh)) if n else None, n))

    def set_environment(self, env):
        self._ck(self.L.srt_set_environment(self._h, C.byref(env)))

    def set_camera(self, cam):
        self._ck(self.L.srt_set_camera(self._h, C.byref(cam)))

    def set_stream(self, stream_ptr):
        self._ck(self.L.srt_set_stream(self._h, C.c_void_p(stream_ptr)))

    def bind_output(self, d_framebuffer=None, d_accumulator=None):
        self._ck(self.L.srt_bind_output(self._h, C.c_void_p(d_framebuffer or 0), C.c_void_p(d_accumulator or 0)))

    # ---- hot path --------------------------------------------------------------------
    def render(self, *, spp=1, bounces=4, seed=0, first_sample=1, reset=True, rows=None, count_rays=False,
               preview=False, steps=1, stripe_width=0, selected=-1, count_work=False, timing=True):
        rb, re = rows if rows is not None else (0, self.height)
        flags = ((RENDER_RESET if reset else 0) | (RENDER_COUNT_RAYS if count_rays else 0) | (RENDER_PREVIEW if preview else 0) |
                 (RENDER_COUNT_WORK if count_work else 0) | (0 if timing else RENDER_NO_TIMING))
        p = RenderParams(rb, re, first_sample, spp, bounces, seed, flags, steps, stripe_width, selected)
        self._ck(self.L.srt_render(self._h, C.byref(p)))

    def render_gbuffer(self, rows=None, outputs=GBUF_ALL, flags=0):
        """srt_render_gbuffer: the first-hit buffers of memory rows `rows` (default: the whole frame).  `outputs`: an SRT_GBUF_*
        mask or names of GBUFFERS.  Asynchronous, like render()."""
        rb, re = self._band(rows)
        p = GBufferParams(int(rb), int(re), gbuffer_outputs(outputs), int(flags))
        self._ck(self.L.srt_render_gbuffer(self._h, C.byref(p)))

    def _read_image(self, fn, shape, dtype, *args):
        """One srt_read_*: a new array of `shape` filled by fn(handle, *args, pointer to the array's data)."""
        out = np.empty(shape, dtype=dtype)
        self._ck(fn(self._h, *args, out.ctypes.data_as(fn.argtypes[-1])))
        return out

    def _image_spec(self, table, name, what):
        """(bit, dtype, shape) of one per-pixel output of GBUFFERS or REFLECTION."""
        bit, dtype, ch = _spec(table, name, what)
        return bit, dtype, ((self.height, self.width) if ch == 1 else (self.height, self.width, ch))

    def gbuffer(self, name):
        """srt_read_gbuffer: the whole buffer of one output as a numpy array, rows = scene rows (the orientation of
        accumulator()): "object" (H, W) int32, the others (H, W, 4) float32."""
        bit, dtype, shape = self._image_spec(GBUFFERS, name, "G-buffer output")
        return self._read_image(self.L.srt_read_gbuffer, shape, dtype, bit)

    def bind_gbuffer(self, name, tensor):
        """srt_bind_gbuffer: write output `name` into a torch tensor on this tracer's device (None: the handle's own buffer).
        Device, dtype, shape and contiguity are checked here, before any native call; the caller keeps the tensor alive
        until the work that writes it has finished."""
        bit, dtype, shape = self._image_spec(GBUFFERS, name, "G-buffer output")
        ptr = self._tensor_ptr("bind_gbuffer(%r)" % name, tensor, dtype, shape)  # (checked before the library is touched)
        self._ck(self.L.srt_bind_gbuffer(self._h, bit, ptr))

    # ---- ray queries -------------------------------------------------------------------
    def _ray_array(self, what, a):
        """A ray array as (kind, object, count): a host array of N x 4 float32 (numpy, or anything numpy converts) or a torch
        tensor on this tracer's device, float32, contiguous, of shape (N, 4)."""
        try:
            import torch
        except ImportError:  # numpy input needs no torch
            torch = None
        if torch is not None and isinstance(a, torch.Tensor):
            if a.device.type != "cuda":
                a = a.detach().numpy()
            else:
                if a.device.index != self.device:
                    raise ValueError("%s: tensor on %s, the tracer renders on cuda:%d" % (what, a.device, self.device))
                if a.dtype != torch.float32:
                    raise TypeError("%s: dtype %s, want torch.float32" % (what, a.dtype))
                if a.dim() != 2 or a.shape[1] != 4 or a.shape[0] < 1:
                    raise ValueError("%s: shape %s, want (N, 4)" % (what, tuple(a.shape)))
                if not a.is_contiguous():
                    raise ValueError("%s: tensor is not contiguous" % what)
                return "device", a, int(a.shape[0])
        h = np.ascontiguousarray(a, dtype=np.float32)
        if h.ndim != 2 or h.shape[1] != 4 or h.shape[0] < 1:
            raise ValueError("%s: shape %s, want (N, 4)" % (what, h.shape))
        return "host", h, int(h.shape[0])

    def write_rays(self, origins, directions):
        """srt_write_rays: copy N rays from host arrays (N, 4) float32 — origin (x, y, z, ignored), direction (x, y, z, t_max) —
        into the handle's own buffers and make them the current rays.  Waits for enqueued work."""
        ko, o, n = self._ray_array("write_rays(origins)", origins)
        kd, d, m = self._ray_array("write_rays(directions)", directions)
        if ko != "host" or kd != "host":
            raise TypeError("write_rays: host arrays wanted (device tensors go through bind_rays)")
        if n != m:
            raise ValueError("write_rays: %d origins, %d directions" % (n, m))
        f = C.POINTER(C.c_float)
        self._ck(self.L.srt_write_rays(self._h, o.ctypes.data_as(f), d.ctypes.data_as(f), n))
        self._ray_count = self._ray_own_count = n
        self._ray_bound = None

    def bind_rays(self, origins, directions, count=None):
        """srt_bind_rays: make two device arrays the current rays: torch tensors (N, 4) float32 on this tracer's device, or raw
        device pointers (ints) with `count`.  None, None returns to the handle's own buffers.  Does not wait or copy: the
        caller keeps the arrays alive until the traces that read them have finished."""
        if origins is None and directions is None:
            self._ck(self.L.srt_bind_rays(self._h, None, None, 0))
            self._ray_count = self._ray_own_count
            self._ray_bound = None
            return
        if isinstance(origins, (int, np.integer)) and isinstance(directions, (int, np.integer)):
            if count is None:
                raise ValueError("bind_rays: raw device pointers need count")
            po, pd, n = int(origins), int(directions), int(count)
            keep = None
        else:
            ko, o, n = self._ray_array("bind_rays(origins)", origins)
            kd, d, m = self._ray_array("bind_rays(directions)", directions)
            if ko != "device" or kd != "device":
                raise TypeError("bind_rays: device tensors wanted (host arrays go through write_rays)")
            if n != m:
                raise ValueError("bind_rays: %d origins, %d directions" % (n, m))
            if count is not None:
                if not 1 <= int(count) <= n:
                    raise ValueError("bind_rays: count %d of %d rays" % (int(count), n))
                n = int(count)
            po, pd = o.data_ptr(), d.data_ptr()
            keep = (o, d)
        self._ck(self.L.srt_bind_rays(self._h, C.c_void_p(po), C.c_void_p(pd), n))
        self._ray_count = n
        self._ray_bound = keep  # (bound tensors stay referenced for as long as they are bound)

    def _rays_given(self, what, origins, directions):
        """The `origins` / `directions` of a trace: host arrays are written (write_rays), device tensors bound (bind_rays); both
        None: the current rays stay."""
        if (origins is None) != (directions is None):
            raise ValueError("%s: origins and directions go together" % what)
        if origins is not None:
            if self._ray_array("%s(origins)" % what, origins)[0] == "host":
                self.write_rays(origins, directions)
            else:
                self.bind_rays(origins, directions)

    def trace_rays(self, outputs=RAYS_ALL, normalize=False, flags=0):
        """srt_trace_rays: the closest hit of every current ray against the current scene.  `outputs`: a mask or names of
        RAY_OUTPUTS; normalize=True normalizes every direction first (SRT_RAYS_NORMALIZE).  Asynchronous, like render()."""
        p = TraceParams(ray_outputs(outputs), int(flags) | (RAYS_NORMALIZE if normalize else 0))
        n = self._ray_count
        for name, t in self._ray_out_bound.items():
            if n is not None and (p.outputs & RAY_OUTPUTS[name][0]) and t.shape[0] < n:
                raise ValueError("trace_rays: the tensor bound to %r holds %d elements, the batch has %d rays" % (name, t.shape[0], n))
        self._ck(self.L.srt_trace_rays(self._h, C.byref(p)))
        self._ray_traced = n

    def trace_occlusion(self, origins=None, directions=None, normalize=False, count_work=False, flags=0):
        """srt_trace_occlusion: for every ray, is there a valid hit with distance < t_max (direction w)?  The any-hit counterpart
        of trace_rays("occluded"), with the same bits.  `origins` / `directions`: numpy arrays (N, 4) float32 (written with
        write_rays) or torch tensors on this tracer's device (bound with bind_rays, by data_ptr, no copy); both None: the current
        rays.  normalize: SRT_OCCLUSION_NORMALIZE; count_work: SRT_OCCLUSION_COUNT_WORK (occlusion_work() then reads the
        record).  Asynchronous, like render(); ray_output("occluded") reads the result."""
        self._rays_given("trace_occlusion", origins, directions)
        p = OcclusionParams(int(flags) | (OCCLUSION_NORMALIZE if normalize else 0) | (OCCLUSION_COUNT_WORK if count_work else 0), 0)
        n = self._ray_count
        t = self._ray_out_bound.get("occluded")
        if n is not None and t is not None and t.shape[0] < n:
            raise ValueError("trace_occlusion: the tensor bound to 'occluded' holds %d elements, the batch has %d rays" % (t.shape[0], n))
        self._ck(self.L.srt_trace_occlusion(self._h, C.byref(p)))
        self._ray_traced = n

    def occlusion_work(self):
        """srt_get_occlusion_work: the work counts of the last trace_occlusion(count_work=True) as a dict.  Waits."""
        return self._get_work(OcclusionWork, self.L.srt_get_occlusion_work)

    # ---- per-pixel visibility ------------------------------------------------------------
    def render_visibility(self, ao_samples=None, radius=None, sun=True, ao=True, first_sample=1, seed=0, rows=None, count_work=False):
        """srt_render_visibility: ambient occlusion ("ao": the fraction of `ao_samples` hemisphere segments of length `radius` that
        are unoccluded; defaults 16 and +inf) and sun visibility ("sun": n . -sun_direction where the sun is seen, else 0) per
        pixel, from the OBJECT, NORMAL_DEPTH and POSITION guides as they stand (render_gbuffer() first, or bind them).  `rows`:
        a band of memory rows (default: the whole frame).  count_work: SRT_VIS_COUNT_WORK (visibility_work() then reads the
        record).  Asynchronous, like render(); visibility("ao" | "sun") reads a result."""
        p = self._default(VisibilityParams, self.L.srt_visibility_params_default)
        p.row_begin, p.row_end = self._band(rows)
        _set(p, outputs=(VIS_AO if ao else 0) | (VIS_SUN if sun else 0), flags=VIS_COUNT_WORK if count_work else 0, ao_samples=ao_samples,
             ao_radius=radius, first_sample=first_sample, seed=seed)
        self._ck(self.L.srt_render_visibility(self._h, C.byref(p)))

    def visibility(self, name):
        """srt_read_visibility: output "ao" or "sun" of the last render_visibility() as an (H, W) float32 array, rows = scene rows."""
        return self._read_image(self.L.srt_read_visibility, (self.height, self.width), np.float32, _spec(VISIBILITY, name))

    def bind_visibility(self, name, tensor):
        """srt_bind_visibility: write output "ao" or "sun" into a torch tensor (H, W) float32 on this tracer's device (None: the
        handle's own buffer), checked like bind_gbuffer's."""
        ptr = self._tensor_ptr("bind_visibility(%r)" % name, tensor, np.float32, (self.height, self.width))
        self._ck(self.L.srt_bind_visibility(self._h, _spec(VISIBILITY, name), ptr))

    def visibility_work(self):
        """srt_get_visibility_work: the work counts of the last render_visibility(count_work=True) as a dict.  Waits."""
        return self._get_work(VisibilityWork, self.L.srt_get_visibility_work)

    # ---- radiance queries ----------------------------------------------------------------
    # ---- reflection guides ----------------------------------------------------------------
    def render_reflection_gbuffer(self, rows=None, outputs=REFL_ALL, max_bounces=None, min_smoothness=None, min_specular=None,
                                  count_work=False, flags=0, reserved=0):
        """srt_render_reflection_gbuffer: the first-hit buffers of memory rows `rows` (default: the whole frame) traced through
        chains of mirror-like surfaces — the object, normal + path length, point and albedo of the first surface that is not
        one, and the number of reflections.  `outputs`: an SRT_REFL_* mask or names of REFLECTION.  Arguments left at None take
        the library's defaults (8 reflections, smoothness and specular amount of at least 1).  count_work: SRT_REFL_COUNT_WORK
        (reflection_work() then reads the record).  Asynchronous, like render_gbuffer()."""
        p = self._default(ReflectionParams, self.L.srt_reflection_params_default)
        p.row_begin, p.row_end = self._band(rows)
        _set(p, outputs=reflection_outputs(outputs), flags=int(flags) | (REFL_COUNT_WORK if count_work else 0), max_bounces=max_bounces,
             min_smoothness=min_smoothness, min_specular=min_specular, reserved=reserved)
        self._ck(self.L.srt_render_reflection_gbuffer(self._h, C.byref(p)))

    def read_reflection(self, name):
        """srt_read_reflection: the whole buffer of one output as a numpy array, rows = scene rows: "object" and "bounces"
        (H, W) int32, the others (H, W, 4) float32.  Waits."""
        bit, dtype, shape = self._image_spec(REFLECTION, name, "reflection output")
        return self._read_image(self.L.srt_read_reflection, shape, dtype, bit)

    def bind_reflection(self, name, tensor):
        """srt_bind_reflection: write output `name` into a torch tensor on this tracer's device (None: the handle's own
        buffer), checked like bind_gbuffer's."""
        bit, dtype, shape = self._image_spec(REFLECTION, name, "reflection output")
        ptr = self._tensor_ptr("bind_reflection(%r)" % name, tensor, dtype, shape)
        self._ck(self.L.srt_bind_reflection(self._h, bit, ptr))

    def reflection_ptr(self, name):
        """srt_device_reflection: the device address of the handle's own buffer of output `name` (allocated on first use)."""
        p = C.c_void_p()
        self._ck(self.L.srt_device_reflection(self._h, _spec(REFLECTION, name, "reflection output")[0], C.byref(p)))
        return p.value

    def reflection_work(self):
        """srt_get_reflection_work: the work counts of the last render_reflection_gbuffer(count_work=True) as a dict.  Waits."""
        return self._get_work(ReflectionWork, self.L.srt_get_reflection_work)

    def use_reflection_guides(self, on=True):
        """Steer the guided passes by the reflection guides: with `on` the handle's own four reflection guide buffers are bound
        into the four G-buffer slots (srt_bind_gbuffer), with off NULL is (the handle's own first-hit buffers again).  While on,
        the gbuffer=True of denoise(), denoise_variance() and variance() renders the guides with render_reflection_gbuffer()
        (library defaults) instead of render_gbuffer(); the passes that reproject or
        resample by first hits — temporal(), upsample(), antialias() — refuse to render guides into those buffers: call them
        with the guides off, or with gbuffer=False on buffers of your own."""
        for name, (bit, _, _) in GBUFFERS.items():
            ptr = C.c_void_p(self.reflection_ptr(name)) if on else None
            self._ck(self.L.srt_bind_gbuffer(self._h, bit, ptr))
        self._reflection_guides = bool(on)

    def mirror_history(self, on=True, radius_pixels=None):
        """srt_mirror_history: with `on`, temporal() reprojects the pixels that look through mirrors by the virtual image of what
        they show, and accepts only history seen through the same mirror near the same terminal point (radius_pixels: the radius
        of that test in pixels; None: the library's default).  While on, temporal(gbuffer=True) renders the first hits AND the
        four reflection outputs the mode reads (object, normal_depth, position, bounces).  Switching drops the history."""
        p = _set(self._default(MirrorHistoryParams, self.L.srt_mirror_history_params_default), enabled=1 if on else 0, radius_pixels=radius_pixels)
        self._ck(self.L.srt_mirror_history(self._h, C.byref(p)))
        self._mirror_history = bool(on)

    def probe_tail(self, enabled=True, normal_weight=False, depth=False, states=False, band_weight=None, count_work=False, bias=None,
                   min_variance=None):
        """srt_probe_tail: with `enabled`, a path of trace_radiance() or of the light-probe traces that ends at the bounce limit on a
        surface adds the probe grid's hemisphere-mean radiance there (the grid, coefficients, depth maps and states current at the
        trace).  normal_weight / depth / states switch probe-grid rules 6 / 7b / 3s and 4s on; band_weight, bias and min_variance
        default to the library's (the hemisphere mean).  Touches no device memory."""
        p = self._default(ProbeTailParams, self.L.srt_probe_tail_params_default)
        flags = ((PROBE_TAIL_NORMAL_WEIGHT if normal_weight else 0) | (PROBE_TAIL_DEPTH if depth else 0) | (PROBE_TAIL_STATES if states else 0)
                 | (PROBE_TAIL_COUNT_WORK if count_work else 0))
        if band_weight is not None:
            p.band_weight[:] = [float(v) for v in band_weight]  # (exactly three: a slice assignment refuses any other length)
        _set(p, enabled=1 if enabled else 0, flags=flags, bias=bias, min_variance=min_variance)
        self._ck(self.L.srt_probe_tail(self._h, C.byref(p)))

    def probe_tail_work(self):
        """srt_get_probe_tail_work as a dict: the record of the last trace that ran under probe_tail(count_work=True)."""
        return self._get_work(ProbeTailWork, self.L.srt_get_probe_tail_work)

    def _render_guides(self, outputs, what, first_hit_only=False):
        """The guides a pass with gbuffer=True renders first: first hits, or the reflection guides while they are in use."""
        if not self._reflection_guides:
            return self.render_gbuffer(outputs=outputs)
        if first_hit_only:
            raise ValueError("%s works on first hits: use_reflection_guides(False) first, or pass guides of your own" % what)
        self.render_reflection_gbuffer(outputs=outputs)

    def trace_radiance(self, origins=None, directions=None, samples=None, bounces=None, seed=0, first_sample=1, reset=True, id_base=0,
                       normalize=False, count_work=False, flags=0, sun_sampling=False):
        """srt_trace_radiance: the running mean of `samples` path-traced samples (default 16) of `bounces` bounces (default 8) along
        every ray: what render() leaves in the accumulator for a pixel, for rays of the caller's.  `origins` / `directions`: numpy
        arrays (N, 4) float32 (written with write_rays) or torch tensors on this tracer's device (bound with bind_rays); both None:
        the current rays.  Ray i draws from the stream of pixel id_base + i; reset=False continues the mean the output holds;
        normalize: SRT_RADIANCE_NORMALIZE; count_work: SRT_RADIANCE_COUNT_WORK (radiance_work() then reads the record).
        sun_sampling: SRT_RADIANCE_SUN_SAMPLING — one shadow segment towards the sun at every diffuse bounce, the sun taken out of
        that bounce (rules S1 - S9): the same mean with far less noise in sunlit scenes; refused (SRT_ERR_STATE) while probe_tail is on
        or when the environment's sun_direction is not a unit vector.  Asynchronous, like render(); radiance() reads the result."""
        self._rays_given("trace_radiance", origins, directions)
        p = self._default(RadianceParams, self.L.srt_radiance_params_default)
        _set(p, sample_count=samples, max_bounces=bounces, first_sample=first_sample, seed=int(seed) & 0xFFFFFFFF, id_base=int(id_base) & 0xFFFFFFFF,
             flags=int(flags) | (RADIANCE_RESET if reset else 0) | (RADIANCE_NORMALIZE if normalize else 0) | (RADIANCE_COUNT_WORK if count_work else 0) |
             (RADIANCE_SUN_SAMPLING if sun_sampling else 0))
        n = self._ray_count
        t = self._radiance_bound
        if n is not None and t is not None and t.shape[0] < n:
            raise ValueError("trace_radiance: the bound tensor holds %d elements, the batch has %d rays" % (t.shape[0], n))
        self._ck(self.L.srt_trace_radiance(self._h, C.byref(p)))
        self._radiance_traced = n

    def bind_radiance(self, tensor):
        """srt_bind_radiance: write the radiance into a torch tensor (M, 4) float32 on this tracer's device, contiguous, M at least
        the batch size (checked by trace_radiance); None: the handle's own buffer.  The caller keeps the tensor alive until the
        traces have finished."""
        self._bind_sized("bind_radiance", self.L.srt_bind_radiance, (), tensor, np.float32, (4,))
        self._radiance_bound = tensor

    def radiance(self, count=None):
        """srt_read_radiance: the result of the last trace_radiance() as an (N, 4) float32 array.  `count`: N, for rays bound by
        raw pointer on another PathTracer object (default: this one's).  Waits."""
        n = count if count is not None else self._radiance_traced
        if n is None:
            raise SrtError(ERR_STATE, "radiance(): no trace_radiance() yet")
        return self._read_image(self.L.srt_read_radiance, (n, 4), np.float32)

    def radiance_work(self):
        """srt_get_radiance_work: the work counts of the last trace_radiance(count_work=True) as a dict.  Waits."""
        return self._get_work(RadianceWork, self.L.srt_get_radiance_work)

    # ---- adaptive sampling -----------------------------------------------------------------
    def _u32_frame(self, what, arr):
        a = np.ascontiguousarray(arr, dtype=np.uint32)
        if a.shape != (self.height, self.width):
            raise ValueError("%s: shape %s, want %s" % (what, a.shape, (self.height, self.width)))
        return a

    def _u32_tensor_ptr(self, what, tensor):
        """_tensor_ptr for a per-pixel uint32 buffer: an (H, W) torch.int32 tensor (the same 32 bits)."""
        return self._tensor_ptr(what, tensor, np.int32, (self.height, self.width))

    def set_sample_counts(self, value):
        """srt_set_sample_counts: every pixel's sample count = value ("I have just rendered `value` samples").  Asynchronous."""
        self._ck(self.L.srt_set_sample_counts(self._h, int(value)))

    def write_sample_counts(self, arr):
        """srt_write_sample_counts: the counts from an (H, W) array of uint32, rows = scene rows.  Waits."""
        a = self._u32_frame("write_sample_counts", arr)
        self._ck(self.L.srt_write_sample_counts(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32))))

    def sample_counts(self):
        """srt_read_sample_counts: (H, W) uint32, rows = scene rows (the orientation of accumulator()).  Waits."""
        return self._read_image(self.L.srt_read_sample_counts, (self.height, self.width), np.uint32)

    def bind_sample_counts(self, tensor):
        """srt_bind_sample_counts: keep the counts in a torch tensor on this tracer's device, (H, W) int32 (read as uint32) and
        contiguous (None: the handle's own buffer).  Checked here, before any native call, as bind_denoised checks."""
        self._ck(self.L.srt_bind_sample_counts(self._h, self._u32_tensor_ptr("bind_sample_counts", tensor)))

    def write_sample_budget(self, arr):
        """srt_write_sample_budget: the budget from an (H, W) array of uint32, rows = scene rows.  Waits."""
        a = self._u32_frame("write_sample_budget", arr)
        self._ck(self.L.srt_write_sample_budget(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32))))

    def sample_budget_map(self):
        """srt_read_sample_budget: (H, W) uint32, rows = scene rows.  Waits."""
        return self._read_image(self.L.srt_read_sample_budget, (self.height, self.width), np.uint32)

    def bind_sample_budget(self, tensor):
        """srt_bind_sample_budget: keep the budget in a torch tensor on this tracer's device, (H, W) int32 (read as uint32) and
        contiguous (None: the handle's own buffer).  Checked here, before any native call."""
        self._ck(self.L.srt_bind_sample_budget(self._h, self._u32_tensor_ptr("bind_sample_budget", tensor)))

    def sample_budget(self, threshold=None, floor=None, max_budget=None, albedo=None, flags=None):
        """srt_sample_budget over the whole frame: the variance buffer, the counts, the accumulator and the OBJECT (and ALBEDO)
        guides as they stand -> the budget buffer.  Arguments left at None take srt_budget_params_default.  Asynchronous;
        budget_total() reads the sum, sample_budget_map() the map."""
        p = _set(self._default(BudgetParams, self.L.srt_budget_params_default), threshold=threshold, floor=floor, max_budget=max_budget)
        if albedo is not None:
            p.flags = (p.flags & ~BUDGET_ALBEDO) | (BUDGET_ALBEDO if albedo else 0)
        _set(p, flags=flags)
        self._ck(self.L.srt_sample_budget(self._h, C.byref(p)))

    def budget_total(self):
        """srt_get_budget_total: the sum of the budget the last sample_budget() wrote.  Waits."""
        t = C.c_uint64(0)
        self._ck(self.L.srt_get_budget_total(self._h, C.byref(t)))
        return int(t.value)

    def render_adaptive(self, bounces=None, seed=0, max_samples=None, rows=None, keep_counts=False, count_work=False, flags=0, reserved=0, tail=False,
                        sun_sampling=False):
        """srt_render_adaptive: every pixel of memory rows `rows` (default: the whole frame) takes min(budget, max_samples) more
        samples, continuing its running mean from its count; the counts advance unless keep_counts.  Arguments left at None take
        srt_adaptive_params_default.  Asynchronous, like render().  (`tail` is render_adaptive_tail()'s switch.)
        sun_sampling: SRT_ADAPTIVE_SUN_SAMPLING — trace_radiance's sun sampling for every sample of the call (rules AS1 - AS8);
        samples with and without it may share a pixel's mean."""
        p = self._default(AdaptiveParams, self.L.srt_adaptive_params_default)
        p.row_begin, p.row_end = self._band(rows)
        _set(p, max_bounces=bounces, max_samples=max_samples, seed=int(seed) & 0xFFFFFFFF, reserved=reserved,
             flags=int(flags) | (ADAPTIVE_KEEP_COUNTS if keep_counts else 0) | (ADAPTIVE_COUNT_WORK if count_work else 0) |
             (ADAPTIVE_SUN_SAMPLING if sun_sampling else 0))
        self._ck((self.L.srt_render_adaptive_tail if tail else self.L.srt_render_adaptive)(self._h, C.byref(p)))

    def render_adaptive_tail(self, bounces=None, seed=0, max_samples=None, rows=None, keep_counts=False, count_work=False, flags=0, reserved=0,
                             sun_sampling=False):
        """srt_render_adaptive_tail: render_adaptive() whose paths end in the probe grid under the probe_tail() setting (which must
        be on), reading the grid, coefficients, depth maps and states as they stand now.  A tail frame starts from
        set_sample_counts(0); adaptive_work() and probe_tail_work() report it.  sun_sampling: every vertex a bounce is taken
        from gets its sun segment, the vertex at the bounce limit its lookup (rule AS4)."""
        self.render_adaptive(bounces, seed, max_samples, rows, keep_counts, count_work, flags, reserved, tail=True, sun_sampling=sun_sampling)

    def adaptive_work(self):
        """srt_get_adaptive_work: the work counts of the last render_adaptive(count_work=True) as a dict.  Waits."""
        return self._get_work(AdaptiveWork, self.L.srt_get_adaptive_work)

    # ---- light probes ----------------------------------------------------------------------
    def _input(self, what, a, write, bind, per_probe=1, want=None, limit=None, extra=()):
        """Make `a` a current input array of float4: a host array (N, 4) float32 is written (copied) with `write`, a torch tensor
        (N, 4) on this tracer's device is bound with `bind` by its data_ptr(), no copy, and None unbinds: the handle's own array
        is current again.  The native call gets N / per_probe as its count (`want` says per_probe in the refusal of an N that
        is no multiple of it; `limit`: the largest N), then `extra`.  Returns (count, tensor): the caller keeps the tensor
        referenced for as long as it is bound (None: nothing is bound)."""
        if a is None:
            self._ck(bind(self._h, None, 0, *extra))
            return 0, None
        kind, arr, n = self._ray_array(what, a)
        if limit is not None and n > limit:
            raise ValueError("%s: %d elements, want 1 .. %d" % (what, n, limit))
        if per_probe < 1 or n % per_probe:
            raise ValueError("%s: %d float4, want %s per probe" % (what, n, want))
        if kind == "host":
            self._ck(write(self._h, arr.ctypes.data_as(C.POINTER(C.c_float)), n // per_probe, *extra))
            return n // per_probe, None
        self._ck(bind(self._h, C.c_void_p(arr.data_ptr()), n // per_probe, *extra))
        return n // per_probe, arr

    def _probe_inputs(self, what, positions, directions):
        """The `positions` / `directions` of a probe trace: each a host array (written) or a device tensor (bound), `directions`
        also an int K for light_probe_sphere(K); None: the current ones stay."""
        L = self.L
        if positions is not None:
            self._probe_count, self._probe_bound = self._input("%s(positions)" % what, positions, L.srt_write_light_probes,
                                                               L.srt_bind_light_probes, limit=1 << 30)
        if directions is not None:
            if isinstance(directions, (int, np.integer)):
                directions = light_probe_sphere(int(directions), lib=L)
            self._probe_dir_count, self._probe_dir_bound = self._input("%s(directions)" % what, directions, L.srt_write_light_probe_directions,
                                                                       L.srt_bind_light_probe_directions, limit=LIGHT_PROBE_MAX_DIRECTIONS)

    def _bind_sized(self, what, fn, args, tensor, dtype, row, bound=None, key=None):
        """Bind an output whose length the traces set: a torch tensor (M,) + `row` of numpy dtype `dtype` on this tracer's device,
        contiguous, M >= 1 (the trace that writes it checks M against its batch); None: the handle's own buffer.  All checks come
        first, then fn(handle, *args, pointer), then `bound[key]` keeps the tensor referenced for as long as it is bound."""
        ptr = None
        if tensor is not None:
            import torch

            if not isinstance(tensor, torch.Tensor):
                raise TypeError("%s: expected a torch.Tensor, got %s" % (what, type(tensor).__name__))
            m = int(tensor.shape[0]) if tensor.dim() >= 1 else 0
            if m < 1:
                raise ValueError("%s: shape %s, want at least one element" % (what, tuple(tensor.shape)))
            ptr = self._tensor_ptr(what, tensor, dtype, (m,) + row)
        self._ck(fn(self._h, *args, ptr))
        if bound is not None and tensor is None:
            bound.pop(key, None)
        elif bound is not None:
            bound[key] = tensor

    def trace_light_probes(self, positions=None, directions=None, samples=None, bounces=None, seed=0, first_sample=1, reset=True, id_base=0,
                           normalize=False, count_work=False, coefficients=True, radiance=False, flags=0, listed=False, sun_sampling=False):
        """srt_trace_light_probes: for each of P probe positions, the running mean of `samples` path-traced samples (default 16) of
        `bounces` bounces (default 8) along each of K shared directions, projected onto the nine SH coefficients of bands 0..2.
        `positions`: numpy (P, 4) float32 (written) or a torch tensor on this tracer's device (bound); None: the current ones.
        `directions`: the same, (K, 4) with the quadrature weight in w; an int K: light_probe_sphere(K); None: the current ones.
        Ray (p, k) draws from the stream of pixel id_base + p*K + k.  coefficients / radiance: the outputs (light_probe_coefficients(),
        light_probe_radiance()); reset=False continues the means the RADIANCE buffer holds; normalize: SRT_LIGHT_PROBE_NORMALIZE;
        count_work: SRT_LIGHT_PROBE_COUNT_WORK (light_probe_work() then reads the record).  listed: srt_trace_light_probes_listed —
        only the probes of the list bound for tracing (bind_probe_list()); every other probe's outputs keep their bits.
        sun_sampling: SRT_LIGHT_PROBE_SUN_SAMPLING, as trace_radiance's (the listed call takes it too).
        Asynchronous, like render()."""
        L = self.L
        self._probe_inputs("trace_light_probes", positions, directions)
        p = self._default(LightProbeParams, L.srt_light_probe_params_default)
        _set(p, sample_count=samples, max_bounces=bounces, first_sample=first_sample, seed=int(seed) & 0xFFFFFFFF, id_base=int(id_base) & 0xFFFFFFFF,
             flags=int(flags) | (LIGHT_PROBE_RESET if reset else 0) | (LIGHT_PROBE_NORMALIZE if normalize else 0) |
             (LIGHT_PROBE_COUNT_WORK if count_work else 0) | (LIGHT_PROBE_SUN_SAMPLING if sun_sampling else 0),
             outputs=(LIGHT_PROBE_COEFFICIENTS if coefficients else 0) | (LIGHT_PROBE_RADIANCE if radiance else 0))
        np_, nk = self._probe_count, self._probe_dir_count
        if np_ is not None and nk is not None:
            for bit, need in ((LIGHT_PROBE_COEFFICIENTS, np_ * LIGHT_PROBE_COEFFS), (LIGHT_PROBE_RADIANCE, np_ * nk)):
                t = self._probe_out_bound.get(bit)
                if (p.outputs & bit) and t is not None and t.shape[0] < need:
                    raise ValueError("trace_light_probes: the bound tensor holds %d elements, the call writes %d" % (t.shape[0], need))
        self._ck((L.srt_trace_light_probes_listed if listed else L.srt_trace_light_probes)(self._h, C.byref(p)))
        self._probes_traced = (np_, nk)

    def bind_light_probe_output(self, output, tensor):
        """srt_bind_light_probe_output: write output "coefficients" (P*9 float4) or "radiance" (P*K float4) into a torch tensor (M, 4)
        float32 on this tracer's device, contiguous, M at least that many (checked by trace_light_probes); None: the handle's own
        buffer.  The caller keeps the tensor alive until the traces have finished."""
        bit = _bit(LIGHT_PROBE_OUTPUTS, output)
        self._bind_sized("bind_light_probe_output", self.L.srt_bind_light_probe_output, (bit,), tensor, np.float32, (4,), self._probe_out_bound, bit)

    def _light_probe_counts(self, what, probes, directions):
        p = probes if probes is not None else self._probes_traced[0]
        k = directions if directions is not None else self._probes_traced[1]
        if p is None or k is None:
            raise SrtError(ERR_STATE, "%s: no trace_light_probes() yet" % what)
        return int(p), int(k)

    def light_probe_coefficients(self, probes=None):
        """srt_read_light_probe_output(COEFFICIENTS): the (P, 9, 4) float32 coefficients of the last trace_light_probes().  Waits."""
        p, _ = self._light_probe_counts("light_probe_coefficients()", probes, 1)
        return self._read_image(self.L.srt_read_light_probe_output, (p, LIGHT_PROBE_COEFFS, 4), np.float32, LIGHT_PROBE_COEFFICIENTS)

    def light_probe_radiance(self, probes=None, directions=None):
        """srt_read_light_probe_output(RADIANCE): the (P, K, 4) float32 running means of the last trace_light_probes(radiance=True).
        Waits."""
        p, k = self._light_probe_counts("light_probe_radiance()", probes, directions)
        return self._read_image(self.L.srt_read_light_probe_output, (p, k, 4), np.float32, LIGHT_PROBE_RADIANCE)

    def light_probe_work(self):
        """srt_get_light_probe_work: the work counts of the last trace_light_probes(count_work=True) as a dict.  Waits."""
        return self._get_work(LightProbeWork, self.L.srt_get_light_probe_work)

    # ---- probe-grid shading -----------------------------------------------------------------
    def set_probe_grid(self, origin, spacing=None, counts=None):
        """srt_set_probe_grid: the grid later shade_probe_grid() calls interpolate on.  `origin`: a ProbeGrid, or three triples."""
        g = probe_grid(origin, spacing, counts)
        self._ck(self.L.srt_set_probe_grid(self._h, C.byref(g)))
        self._probe_grid_probes = int(g.counts[0]) * int(g.counts[1]) * int(g.counts[2])

    def shade_probe_grid(self, coefficients=None, visibility=False, normal_weight=False, albedo=False, band_weight=None, rows=None,
                         count_work=False, output=None, flags=0, reserved=(0, 0)):
        """srt_shade_probe_grid: per pixel of memory rows `rows` (default: the whole frame) the irradiance at the first hit from the
        grid's probes — trilinear weights, times a normal weight (normal_weight), only probes the surface sees (visibility), times
        the albedo guide (albedo) — from the OBJECT, NORMAL_DEPTH and POSITION guides as they stand (render_gbuffer() first, or bind
        them).  `coefficients`: numpy (P, 9, 4) or (P*9, 4) float32 (written) or a torch tensor (P*9, 4) on this tracer's device
        (bound, no copy: what bind_light_probe_output("coefficients", t) filled); None: the current ones.  `band_weight`: the weights
        of SH bands 0, 1, 2 (default PROBE_GRID_BAND_WEIGHT_IRRADIANCE).  `output`: a torch tensor (H, W, 4) float32 to write
        (bind_probe_grid_output).  count_work: SRT_PROBE_GRID_COUNT_WORK (probe_grid_work() then reads the record).  Asynchronous,
        like render(); probe_grid_output() reads the result."""
        self._probe_grid_coefficients("shade_probe_grid(coefficients)", coefficients)
        if output is not None:
            self.bind_probe_grid_output(output)
        p = self._probe_grid_params(rows, int(flags) | (PROBE_GRID_VISIBILITY if visibility else 0), normal_weight, albedo, count_work, band_weight,
                                    reserved)
        self._ck(self.L.srt_shade_probe_grid(self._h, C.byref(p)))

    def _probe_grid_coefficients(self, what, coefficients):
        """The `coefficients` of a shade_probe_grid* call: numpy (P, 9, 4) or (P*9, 4) is written, a device tensor (P*9, 4) bound
        (_input); None: the current ones stay."""
        if coefficients is None:
            return
        if isinstance(coefficients, np.ndarray) and coefficients.ndim == 3:
            coefficients = coefficients.reshape(-1, 4)
        _, self._probe_grid_bound = self._input(what, coefficients, self.L.srt_write_probe_grid_coefficients,
                                                self.L.srt_bind_probe_grid_coefficients, LIGHT_PROBE_COEFFS, "nine")

    def _probe_grid_params(self, rows, flags, normal_weight, albedo, count_work, band_weight, reserved):
        """The srt_probe_grid_params of a shade_probe_grid* call: the library's defaults, the band, `flags` and the three switches,
        and band_weight when given."""
        p = self._default(ProbeGridParams, self.L.srt_probe_grid_params_default)
        p.row_begin, p.row_end = self._band(rows)
        flags |= (PROBE_GRID_NORMAL_WEIGHT if normal_weight else 0) | (PROBE_GRID_ALBEDO if albedo else 0) | (PROBE_GRID_COUNT_WORK if count_work else 0)
        return _set(p, flags=flags, band_weight=band_weight, reserved=reserved)

    def _probe_grid_depth_params(self, bias, min_variance, reserved):
        """The srt_probe_grid_depth_params of the filtered visibility test: the library's defaults with what was given."""
        return _set(self._default(ProbeGridDepthParams, self.L.srt_probe_grid_depth_params_default), bias=bias, min_variance=min_variance,
                    reserved=reserved)

    def bind_probe_grid_output(self, tensor):
        """srt_bind_probe_grid_output: write the result into a torch tensor on this tracer's device, (H, W, 4) float32 and contiguous
        (None: the handle's own buffer).  Checked here, before any native call, as bind_gbuffer checks."""
        self._ck(self.L.srt_bind_probe_grid_output(self._h, self._float4_tensor_ptr("bind_probe_grid_output", tensor)))
        self._probe_grid_out_bound = tensor

    def probe_grid_output(self):
        """srt_read_probe_grid_output: (H, W, 4) float32, rows = scene rows: the irradiance and the surviving weight.  Waits."""
        return self._read_image(self.L.srt_read_probe_grid_output, (self.height, self.width, 4), np.float32)

    def probe_grid_work(self):
        """srt_get_probe_grid_work: the work counts of the last shade_probe_grid(count_work=True) as a dict.  Waits."""
        return self._get_work(ProbeGridWork, self.L.srt_get_probe_grid_work)

    # ---- probe depth moments and the filtered probe-grid shading -------------------------------
    def trace_probe_depth(self, positions=None, directions=None, resolution=None, sharpness=None, max_distance=None, normalize=False,
                          count_work=False, moments=True, distances=False, flags=0, reserved=0, listed=False):
        """srt_trace_probe_depth: for each of P probe positions an octahedral map of `resolution` x `resolution` texels (default 16)
        holding the weighted mean and mean square of the distance to the nearest surface over the K shared directions, each
        direction weighing cos^(2^sharpness) (default 5) times its quadrature weight, distances clamped to `max_distance` (default
        10000).  `positions` / `directions`: as trace_light_probes() takes them (they are the same current arrays); None: the
        current ones.  moments / distances: the outputs (probe_depth_output()); normalize: SRT_PROBE_DEPTH_NORMALIZE; count_work:
        SRT_PROBE_DEPTH_COUNT_WORK (probe_depth_work() then reads the record).  listed: srt_trace_probe_depth_listed — only the probes
        of the list bound for tracing (bind_probe_list()).  Asynchronous, like render()."""
        L = self.L
        self._probe_inputs("trace_probe_depth", positions, directions)
        p = self._default(ProbeDepthParams, L.srt_probe_depth_params_default)
        _set(p, resolution=resolution, sharpness=sharpness, max_distance=max_distance, reserved=reserved,
             flags=int(flags) | (PROBE_DEPTH_NORMALIZE if normalize else 0) | (PROBE_DEPTH_COUNT_WORK if count_work else 0),
             outputs=(PROBE_DEPTH_MOMENTS if moments else 0) | (PROBE_DEPTH_DISTANCES if distances else 0))
        np_, nk = self._probe_count, self._probe_dir_count
        if np_ is not None and nk is not None:
            for bit, need in ((PROBE_DEPTH_MOMENTS, np_ * int(p.resolution) ** 2 * 4), (PROBE_DEPTH_DISTANCES, np_ * nk)):
                t = self._probe_depth_bound.get(bit)
                if (p.outputs & bit) and t is not None and t.numel() < need:
                    raise ValueError("trace_probe_depth: the bound tensor holds %d floats, the call writes %d" % (t.numel(), need))
        self._ck((L.srt_trace_probe_depth_listed if listed else L.srt_trace_probe_depth)(self._h, C.byref(p)))
        self._probe_depth_traced = (np_, nk, int(p.resolution))

    def bind_probe_depth_output(self, output, tensor):
        """srt_bind_probe_depth_output: write output "moments" (P*R*R float4: a tensor (M, 4)) or "distances" (P*K float: a tensor
        (M,)) into a float32 torch tensor on this tracer's device, contiguous, at least that large (checked by trace_probe_depth);
        None: the handle's own buffer.  The caller keeps the tensor alive until the traces have finished."""
        bit = _bit(PROBE_DEPTH_OUTPUTS, output)
        self._bind_sized("bind_probe_depth_output", self.L.srt_bind_probe_depth_output, (bit,), tensor, np.float32,
                         (4,) if bit == PROBE_DEPTH_MOMENTS else (), self._probe_depth_bound, bit)

    def probe_depth_output(self, output="moments"):
        """srt_read_probe_depth_output: "moments": (P, R*R, 4) float32 (mean, mean square, weight, share at max_distance);
        "distances": (P, K) float32 of the last trace_probe_depth().  Waits."""
        bit = _bit(PROBE_DEPTH_OUTPUTS, output)
        t = self._probe_depth_traced
        if t is None or t[0] is None or t[1] is None:
            raise SrtError(ERR_STATE, "probe_depth_output(): no trace_probe_depth() yet")
        shape = (t[0], t[2] * t[2], 4) if bit == PROBE_DEPTH_MOMENTS else (t[0], t[1])
        return self._read_image(self.L.srt_read_probe_depth_output, shape, np.float32, bit)

    def probe_depth_work(self):
        """srt_get_probe_depth_work: the work counts of the last trace_probe_depth(count_work=True) as a dict.  Waits."""
        return self._get_work(ProbeDepthWork, self.L.srt_get_probe_depth_work)

    def bind_probe_grid_depth(self, moments, resolution=None):
        """srt_write_probe_grid_depth / srt_bind_probe_grid_depth: the depth maps shade_probe_grid_depth() reads, in
        probe_depth_output("moments")'s layout.  numpy (P, R*R, 4) or (P*R*R, 4) float32: written; a torch tensor (P*R*R, 4) on
        this tracer's device: bound, no copy (what bind_probe_depth_output("moments", t) filled); None: back to the own array.
        `resolution`: R (default: from a three-dimensional array's shape, else 16)."""
        a = moments
        if isinstance(a, np.ndarray) and a.ndim == 3:
            if resolution is None:
                resolution = int(round(a.shape[1] ** 0.5))
            a = a.reshape(-1, 4)
        r = 0 if a is None else 16 if resolution is None else int(resolution)
        _, self._probe_grid_depth_bound = self._input("bind_probe_grid_depth(moments)", a, self.L.srt_write_probe_grid_depth,
                                                      self.L.srt_bind_probe_grid_depth, r * r if r > 0 else 0, "%d" % (r * r), extra=(r,))

    def shade_probe_grid_depth(self, coefficients=None, moments=None, resolution=None, bias=None, min_variance=None, normal_weight=False,
                               albedo=False, band_weight=None, rows=None, count_work=False, output=None, flags=0, reserved=(0, 0),
                               depth_reserved=(0, 0)):
        """srt_shade_probe_grid_depth: shade_probe_grid() with the filtered visibility test in place of the exact one: every corner
        probe is weighted by Chebyshev's bound on "the probe sees at least as far as this point" from its depth map.  `moments` /
        `resolution`: as bind_probe_grid_depth() (None: the current maps); `bias` (default 0) and `min_variance` (default 1e-4): the
        test's parameters; everything else as shade_probe_grid().  probe_grid_output() and probe_grid_work() read the result."""
        self._probe_grid_coefficients("shade_probe_grid_depth(coefficients)", coefficients)
        if moments is not None:
            self.bind_probe_grid_depth(moments, resolution)
        if output is not None:
            self.bind_probe_grid_output(output)
        p = self._probe_grid_params(rows, int(flags), normal_weight, albedo, count_work, band_weight, reserved)
        d = self._probe_grid_depth_params(bias, min_variance, depth_reserved)
        self._ck(self.L.srt_shade_probe_grid_depth(self._h, C.byref(p), C.byref(d)))

    # ---- probe classification and relocation, and the probe-grid shading that obeys the records ----
    def classify_probes(self, directions=None, relocate=False, clearance=None, max_offset=None, steps=None, normalize=False, count_work=False,
                        records=True, positions=False, flags=0, reserved=0):
        """srt_classify_probes: the state of every probe of the grid (set_probe_grid() first) from the exact signed distance to the
        scene's spheres and boxes (meshes contribute nothing): PROBE_INSIDE when the grid position lies inside an object,
        PROBE_BURIED when it stays there, PROBE_IDLE when no analytic surface comes near its cells.  relocate: probes nearer than
        `clearance` (default 0.2) times the smallest spacing to a surface are moved along one of the K shared `directions` (as
        trace_light_probes() takes them; None: the current ones) by at most `max_offset` (default 0.45) of the spacing, tried in
        `steps` (default 8) lengths: PROBE_MOVED.  records / positions: the outputs (probe_states_output()); count_work:
        probe_states_work() then reads the record.  Asynchronous, like render()."""
        L = self.L
        self._probe_inputs("classify_probes", None, directions)
        p = self._default(ProbeClassifyParams, L.srt_probe_classify_params_default)
        _set(p, clearance=clearance, max_offset=max_offset, steps=steps, reserved=reserved,
             flags=int(flags) | (PROBE_CLASSIFY_RELOCATE if relocate else 0) | (PROBE_CLASSIFY_NORMALIZE if normalize else 0) |
             (PROBE_CLASSIFY_COUNT_WORK if count_work else 0),
             outputs=(PROBE_STATE_RECORDS if records else 0) | (PROBE_STATE_POSITIONS if positions else 0))
        n = self._probe_grid_probes
        if n is not None:
            for bit, t in self._probe_states_bound.items():
                if (p.outputs & bit) and t.numel() < 4 * n:
                    raise ValueError("classify_probes: the bound tensor holds %d floats, the call writes %d" % (t.numel(), 4 * n))
        self._ck(L.srt_classify_probes(self._h, C.byref(p)))
        self._probe_states_classified = n

    def bind_probe_states_output(self, output, tensor):
        """srt_bind_probe_states_output: write output "records" or "positions" (P float4 each) into a float32 torch tensor (M, 4),
        M >= P, on this tracer's device, contiguous (checked by classify_probes); None: the handle's own buffer.  The caller keeps
        the tensor alive until the calls have finished."""
        bit = _bit(PROBE_STATE_OUTPUTS, output)
        self._bind_sized("bind_probe_states_output", self.L.srt_bind_probe_states_output, (bit,), tensor, np.float32, (4,), self._probe_states_bound, bit)

    def probe_states_output(self, output="records"):
        """srt_read_probe_states_output: "records": (P, 4) float32, the offset in xyz and the state's uint32 bits in w
        (records[:, 3].view(np.uint32)); "positions": (P, 4) float32, the probes where they stand, w = 0.  Waits."""
        bit = _bit(PROBE_STATE_OUTPUTS, output)
        n = self._probe_states_classified
        if n is None:
            raise SrtError(ERR_STATE, "probe_states_output(): no classify_probes() yet")
        return self._read_image(self.L.srt_read_probe_states_output, (n, 4), np.float32, bit)

    def probe_states_work(self):
        """srt_get_probe_classify_work: the work counts of the last classify_probes(count_work=True) as a dict.  Waits."""
        return self._get_work(ProbeClassifyWork, self.L.srt_get_probe_classify_work)

    def bind_probe_grid_states(self, records):
        """srt_write_probe_grid_states / srt_bind_probe_grid_states: the records shade_probe_grid_states() obeys, in
        probe_states_output("records")'s layout.  numpy (P, 4) float32: written; a torch tensor (P, 4) on this tracer's device: bound,
        no copy (what bind_probe_states_output("records", t) filled); None: back to the own array."""
        _, self._probe_grid_states_bound = self._input("bind_probe_grid_states(records)", records, self.L.srt_write_probe_grid_states,
                                                       self.L.srt_bind_probe_grid_states)

    def shade_probe_grid_states(self, coefficients=None, states=None, depth=False, moments=None, resolution=None, bias=None, min_variance=None,
                                normal_weight=False, albedo=False, band_weight=None, rows=None, count_work=False, output=None, flags=0,
                                reserved=(0, 0), depth_reserved=(0, 0)):
        """srt_shade_probe_grid_states: shade_probe_grid() (depth=False) or shade_probe_grid_depth() (depth=True, or `moments`
        given) that obeys the probe records: a PROBE_BURIED probe is skipped, every other probe stands at its grid position plus
        the record's offset.  `states`: as bind_probe_grid_states() (None: the current records); everything else as the parent
        calls.  The exact visibility test is not available.  probe_grid_output() and probe_grid_work() read the result."""
        self._probe_grid_coefficients("shade_probe_grid_states(coefficients)", coefficients)
        if states is not None:
            self.bind_probe_grid_states(states)
        if moments is not None:
            self.bind_probe_grid_depth(moments, resolution)
            depth = True
        if output is not None:
            self.bind_probe_grid_output(output)
        p = self._probe_grid_params(rows, int(flags), normal_weight, albedo, count_work, band_weight, reserved)
        d = C.byref(self._probe_grid_depth_params(bias, min_variance, depth_reserved)) if depth else None
        self._ck(self.L.srt_shade_probe_grid_states(self._h, C.byref(p), d))

    # ---- per-frame probe updates: the list of active probes, the histories and the hysteresis blend ----
    def list_probes(self, skip_mask=None, count_work=False, output=None, flags=0, reserved=(0, 0)):
        """srt_list_probes: the indices of the probes whose current record (bind_probe_grid_states()) has none of the `skip_mask`
        bits (default PROBE_BURIED | PROBE_IDLE), ascending, in SRT_PROBE_LIST's layout: 4 + P uint32 (n, P, 0, 0, the n indices,
        then 0xFFFFFFFF).  output: a torch int32 / uint32 tensor of at least 4 + P words on this tracer's device to write into
        (bound for later calls too); probe_list_output() reads the list, probe_list_work() the counts.  Asynchronous."""
        if output is not None:
            self.bind_probe_list_output(output)
        p = _set(self._default(ProbeListParams, self.L.srt_probe_list_params_default), skip_mask=skip_mask,
                 flags=int(flags) | (PROBE_LIST_COUNT_WORK if count_work else 0), reserved=reserved)
        self._ck(self.L.srt_list_probes(self._h, C.byref(p)))

    def _word_tensor(self, what, tensor):
        """The device pointer and word count of a contiguous 32-bit integer torch tensor on this tracer's device."""
        import torch

        if not isinstance(tensor, torch.Tensor):
            raise TypeError("%s: expected a torch.Tensor, got %s" % (what, type(tensor).__name__))
        if tensor.device.type != "cuda" or tensor.device.index != self.device:
            raise ValueError("%s: tensor on %s, the tracer renders on cuda:%d" % (what, tensor.device, self.device))
        if tensor.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
            raise TypeError("%s: dtype %s, want a 32-bit integer type" % (what, tensor.dtype))
        if tensor.dim() != 1 or not tensor.is_contiguous():
            raise ValueError("%s: want a contiguous one-dimensional tensor, got shape %s" % (what, tuple(tensor.shape)))
        return C.c_void_p(tensor.data_ptr()), int(tensor.shape[0])

    def bind_probe_list_output(self, tensor):
        """srt_bind_probe_list_output: list_probes() writes into a 32-bit integer torch tensor of at least 4 + P words on this
        tracer's device (the caller sees to the size and keeps it alive); None: the handle's own buffer."""
        ptr = None if tensor is None else self._word_tensor("bind_probe_list_output", tensor)[0]
        self._ck(self.L.srt_bind_probe_list_output(self._h, ptr))
        self._probe_list_out_bound = tensor

    def probe_list_output(self, probes):
        """srt_read_probe_list_output: the 4 + `probes` uint32 words of the last list_probes().  Waits."""
        return self._read_image(self.L.srt_read_probe_list_output, (PROBE_LIST_HEADER + int(probes),), np.uint32)

    def probe_list_work(self):
        """srt_get_probe_list_work: the work counts of the last list_probes(count_work=True) as a dict.  Waits."""
        return self._get_work(ProbeListWork, self.L.srt_get_probe_list_work)

    def bind_probe_list(self, words):
        """srt_write_probe_list / srt_bind_probe_list: the list the listed traces and a listed blend read, 4 + P words in
        SRT_PROBE_LIST's layout.  A numpy array: written; a 32-bit integer torch tensor on this tracer's device: bound, no copy
        (what bind_probe_list_output(t) filled); None: unbound."""
        L = self.L
        if words is None:
            self._ck(L.srt_bind_probe_list(self._h, None, 0))
            self._probe_list_bound = None
            return
        try:
            import torch
        except ImportError:
            torch = None
        if torch is not None and isinstance(words, torch.Tensor) and words.device.type == "cuda":
            ptr, n = self._word_tensor("bind_probe_list", words)
            self._ck(L.srt_bind_probe_list(self._h, ptr, n))
            self._probe_list_bound = words  # (a bound tensor stays referenced for as long as it is bound)
            return
        a = np.ascontiguousarray(words.numpy() if torch is not None and isinstance(words, torch.Tensor) else words).astype(np.uint32, copy=False).reshape(-1)
        self._ck(L.srt_write_probe_list(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)), a.shape[0]))
        self._probe_list_bound = None

    def reset_probe_history(self, probes, resolution=0, which=None):
        """srt_reset_probe_history: give the histories of `which` ("coefficients", "moments", "both"; default: both when a
        resolution is given) their size — `probes` probes, `resolution` texels a side for the moments — and zero-fill them, so
        that every probe restarts at the next blend_probes().  Enqueued on the stream."""
        bits = _bit(PROBE_HISTORIES, which) if which is not None else (PROBE_HISTORY_COEFFICIENTS | (PROBE_HISTORY_MOMENTS if resolution else 0))
        self._ck(self.L.srt_reset_probe_history(self._h, bits, int(probes), int(resolution)))
        for bit in (PROBE_HISTORY_COEFFICIENTS, PROBE_HISTORY_MOMENTS):
            if bits & bit:
                self._probe_history_sizes[bit] = (int(probes), int(resolution))

    def bind_probe_history(self, which, tensor):
        """srt_bind_probe_history: keep history "coefficients" (P*9 float4) or "moments" (P*R*R float4) in a float32 torch tensor
        (M, 4) on this tracer's device, contiguous, at least that large (the caller sees to it and keeps it alive); None: the
        handle's own buffer.  reset_probe_history() gives it its size."""
        bit = _bit(PROBE_HISTORIES, which)
        self._bind_sized("bind_probe_history", self.L.srt_bind_probe_history, (bit,), tensor, np.float32, (4,), self._probe_history_bound, bit)

    def probe_history(self, which="coefficients"):
        """srt_read_probe_history: "coefficients": (P, 9, 4) float32; "moments": (P, R*R, 4) float32.  Waits."""
        bit = _bit(PROBE_HISTORIES, which)
        size = self._probe_history_sizes.get(bit)
        if size is None:
            raise SrtError(ERR_STATE, "probe_history(): no reset_probe_history() for that history yet")
        shape = (size[0], LIGHT_PROBE_COEFFS, 4) if bit == PROBE_HISTORY_COEFFICIENTS else (size[0], size[1] * size[1], 4)
        return self._read_image(self.L.srt_read_probe_history, shape, np.float32, bit)

    def bind_probe_previous_states(self, records):
        """srt_write_probe_previous_states / srt_bind_probe_previous_states: the records blend_probes(previous_states=True)
        compares the current ones with; as bind_probe_grid_states() takes them."""
        _, self._probe_previous_bound = self._input("bind_probe_previous_states(records)", records, self.L.srt_write_probe_previous_states,
                                                    self.L.srt_bind_probe_previous_states)

    def blend_probes(self, hysteresis=None, fast_hysteresis=None, depth_hysteresis=None, change_threshold=None, moments=False, listed=False,
                     previous_states=False, count_work=False, flags=0, reserved=0):
        """srt_blend_probes: fold what the last trace_light_probes() wrote to COEFFICIENTS (and, moments=True, the last
        trace_probe_depth() to MOMENTS) into the histories, in place: H = N + (H - N) * h, with h = `hysteresis` (default 0.9), or
        `fast_hysteresis` (0.5) where the DC luminance changed by more than `change_threshold` (0.25) of the larger value, and
        `depth_hysteresis` (0.9) for the moments.  A probe whose history is empty restarts (H = N), and with previous_states=True
        one whose record differs from bind_probe_previous_states()'s in its offset or its BURIED / IDLE bits.  listed: only the
        probes of bind_probe_list().  probe_history() reads the result; probe_blend_work() the counts.  Asynchronous."""
        p = self._default(ProbeBlendParams, self.L.srt_probe_blend_params_default)
        _set(p, hysteresis=hysteresis, fast_hysteresis=fast_hysteresis, depth_hysteresis=depth_hysteresis, change_threshold=change_threshold,
             reserved=reserved, flags=int(flags) | (PROBE_BLEND_MOMENTS if moments else 0) | (PROBE_BLEND_LISTED if listed else 0) |
             (PROBE_BLEND_PREVIOUS_STATES if previous_states else 0) | (PROBE_BLEND_COUNT_WORK if count_work else 0))
        self._ck(self.L.srt_blend_probes(self._h, C.byref(p)))

    def probe_blend_work(self):
        """srt_get_probe_blend_work: the work counts of the last blend_probes(count_work=True) as a dict.  Waits."""
        return self._get_work(ProbeBlendWork, self.L.srt_get_probe_blend_work)

    def scroll_probes(self, shift, which="coefficients", set_grid=False, count_work=False, flags=0, reserved=(0, 0, 0)):
        """srt_scroll_probes: move the grid of set_probe_grid() by `shift` = (sx, sy, sz) cells and keep what stays inside: new probe
        i takes the history of old probe i + shift, a probe without such a source gets zero bits and restarts at the next
        blend_probes().  `which`: "coefficients", "moments", "states" (the current records, scrolled, become the previous records
        of blend_probes(previous_states=True)), "both", "all", a sequence of these, or PROBE_SCROLL_* bits.  set_grid: also move the
        handle's grid origin by shift * spacing; otherwise call set_probe_grid().  A non-zero shift makes the last traces stale:
        blend_probes() refuses until trace_light_probes() (and trace_probe_depth()) ran again.  count_work: probe_scroll_work()
        then reads the record.  Asynchronous."""
        p = self._default(ProbeScrollParams, self.L.srt_probe_scroll_params_default)
        _set(p, shift=shift, reserved=reserved, which=_mask(PROBE_SCROLL_ARRAYS, which),
             flags=int(flags) | (PROBE_SCROLL_SET_GRID if set_grid else 0) | (PROBE_SCROLL_COUNT_WORK if count_work else 0))
        self._ck(self.L.srt_scroll_probes(self._h, C.byref(p)))
        if p.which & PROBE_SCROLL_STATES:
            self._probe_previous_bound = None  # (the handle's own previous records are current again)

    def probe_grid_follow(self, grid, point, which="all", count_work=False):
        """srt_probe_grid_follow, then scroll_probes(shift, which, set_grid=True): re-centre the grid on `point`.  `grid`: the
        ProbeGrid (or triple of triples) last given to set_probe_grid(), or as moved by earlier calls.  Returns the shift."""
        shift = probe_grid_follow(grid, point, lib=self.L)
        self.scroll_probes(shift, which=which, set_grid=True, count_work=count_work)
        return shift

    def probe_scroll_work(self):
        """srt_get_probe_scroll_work: the work counts of the last scroll_probes(count_work=True) as a dict.  Waits."""
        return self._get_work(ProbeScrollWork, self.L.srt_get_probe_scroll_work)

    get_probe_scroll_work = probe_scroll_work

    def probe_previous_states(self, probes):
        """srt_read_probe_previous_states: the (probes, 4) float32 records blend_probes(previous_states=True) compares with — what
        bind_probe_previous_states() or scroll_probes(which="states") left.  Waits."""
        return self._read_image(self.L.srt_read_probe_previous_states, (int(probes), 4), np.float32)

    # ---- probe cascades: nested grids, the finest level that holds a pixel blended into the next at its border ----
    def set_probe_cascade(self, grids, resolution=0, blend_cells=1.0):
        """srt_set_probe_cascade: the cascade shade_probe_cascade() reads: a ProbeCascade (probe_cascade_grids()), or 1 .. 4 grids,
        finest first, with the resolution R of every level's moments (0: none) and the band width in cells.  A level whose probe
        count changed loses its arrays; one that only moved keeps them."""
        c = probe_cascade(grids, resolution, blend_cells)
        self._ck(self.L.srt_set_probe_cascade(self._h, C.byref(c)))
        self._probe_cascade = c

    def write_probe_cascade_level(self, level, which, array):
        """srt_write_probe_cascade_level: copy a level's "coefficients" (P, 9, 4), "moments" (P, R*R, 4) or "records" (P, 4), numpy
        float32, into the handle's own array of that level.  Waits."""
        bit = _mask(PROBE_CASCADE_ARRAYS, which)
        a = np.ascontiguousarray(array, dtype=np.float32)
        probes = int(a.shape[0]) if a.ndim >= 1 else 0
        self._ck(self.L.srt_write_probe_cascade_level(self._h, int(level), bit, a.ctypes.data_as(C.POINTER(C.c_float)), probes))
        self._probe_cascade_bound.pop((int(level), bit), None)

    def bind_probe_cascade_level(self, level, which, tensor, probes=None):
        """srt_bind_probe_cascade_level: read a level's "coefficients", "moments" or "records" from a float32 torch tensor on this
        tracer's device, contiguous, (P, 9, 4) / (P, R*R, 4) / (P, 4) (or flat with `probes` given); no copy, the caller keeps it
        alive.  None: back to the own array."""
        bit = _mask(PROBE_CASCADE_ARRAYS, which)
        if tensor is None:
            self._ck(self.L.srt_bind_probe_cascade_level(self._h, int(level), bit, None, 0))
            self._probe_cascade_bound.pop((int(level), bit), None)
            return
        # (the tensor's own shape is the wanted one: any shape goes, with `probes` or its first dimension as the count)
        ptr = self._tensor_ptr("bind_probe_cascade_level", tensor, np.float32, getattr(tensor, "shape", ()))
        n = int(probes) if probes is not None else (int(tensor.shape[0]) if tensor.dim() >= 1 else 0)
        self._ck(self.L.srt_bind_probe_cascade_level(self._h, int(level), bit, ptr, n))
        self._probe_cascade_bound[(int(level), bit)] = tensor

    def capture_probe_cascade_level(self, level, which="all"):
        """srt_capture_probe_cascade_level: copy, on the device, what the single-grid calls would read now (the current probe-grid
        coefficients, depth moments, state records, as `which` selects) into the level's own arrays.  Asynchronous."""
        bits = _mask(PROBE_CASCADE_ARRAYS, which)
        self._ck(self.L.srt_capture_probe_cascade_level(self._h, int(level), bits))
        for b in (PROBE_CASCADE_COEFFICIENTS, PROBE_CASCADE_MOMENTS, PROBE_CASCADE_RECORDS):
            if bits & b:
                self._probe_cascade_bound.pop((int(level), b), None)

    def shade_probe_cascade(self, depth=False, states=False, normal_weight=False, albedo=False, band_weight=None, bias=None, min_variance=None,
                            rows=None, count_work=False, output=None, flags=0, reserved=(0, 0)):
        """srt_shade_probe_cascade: per pixel the irradiance of the finest level of set_probe_cascade() that holds its first hit,
        blended into the next coarser level across the border band.  depth / states: rule 7b from each level's moments, rules
        3s / 4s from each level's records; the other arguments as shade_probe_grid_states().  probe_grid_output() reads the result,
        probe_cascade_work() the counts.  Asynchronous."""
        if output is not None:
            self.bind_probe_grid_output(output)
        p = self._default(ProbeCascadeParams, self.L.srt_probe_cascade_params_default)
        p.row_begin, p.row_end = self._band(rows)
        flags = (int(flags) | (PROBE_CASCADE_NORMAL_WEIGHT if normal_weight else 0) | (PROBE_CASCADE_DEPTH if depth else 0) |
                 (PROBE_CASCADE_STATES if states else 0) | (PROBE_CASCADE_ALBEDO if albedo else 0) | (PROBE_CASCADE_COUNT_WORK if count_work else 0))
        _set(p, flags=flags, band_weight=band_weight, bias=bias, min_variance=min_variance, reserved=reserved)
        self._ck(self.L.srt_shade_probe_cascade(self._h, C.byref(p)))

    def probe_cascade_work(self):
        """srt_get_probe_cascade_work: the work counts of the last shade_probe_cascade(count_work=True) as a dict.  Waits."""
        return self._get_work(ProbeCascadeWork, self.L.srt_get_probe_cascade_work)

    def ray_output(self, name, count=None):
        """srt_read_ray_output: one output of the last trace_rays() as a numpy array: "object" and "occluded" (N,) int32, the
        others (N, 4) float32.  `count`: N, for rays bound by raw pointer on another PathTracer object (default: this one's)."""
        bit, dtype, ch = _spec(RAY_OUTPUTS, name, "ray output")
        n = count if count is not None else self._ray_traced
        if n is None:
            raise SrtError(ERR_STATE, "ray_output(%r): no trace_rays() yet" % name)
        return self._read_image(self.L.srt_read_ray_output, (n,) if ch == 1 else (n, ch), dtype, bit)

    def bind_ray_output(self, name, tensor):
        """srt_bind_ray_output: write output `name` into a torch tensor on this tracer's device (None: the handle's own buffer):
        (M,) int32 for "object" / "occluded", (M, 4) float32 for the others, contiguous, M at least the batch size (checked by
        trace_rays).  Checked here, before any native call; the caller keeps the tensor alive until the traces have finished."""
        bit, dtype, ch = _spec(RAY_OUTPUTS, name, "ray output")
        self._bind_sized("bind_ray_output(%r)" % name, self.L.srt_bind_ray_output, (bit,), tensor, dtype, () if ch == 1 else (ch,),
                         self._ray_out_bound, name)

    def _tensor_ptr(self, what, tensor, dtype, shape):
        """The device pointer of a tensor an output is bound to: on this tracer's device, of numpy dtype `dtype` (int32 or
        float32), of `shape` and contiguous; None passes through (the handle's own buffer)."""
        if tensor is None:
            return None
        import torch

        want = torch.int32 if dtype == np.int32 else torch.float32
        if not isinstance(tensor, torch.Tensor):
            raise TypeError("%s: expected a torch.Tensor, got %s" % (what, type(tensor).__name__))
        if tensor.device.type != "cuda" or tensor.device.index != self.device:
            raise ValueError("%s: tensor on %s, the tracer renders on cuda:%d" % (what, tensor.device, self.device))
        if tensor.dtype != want:
            raise TypeError("%s: dtype %s, want %s" % (what, tensor.dtype, want))
        if tuple(tensor.shape) != tuple(shape):
            raise ValueError("%s: shape %s, want %s" % (what, tuple(tensor.shape), tuple(shape)))
        if not tensor.is_contiguous():
            raise ValueError("%s: tensor is not contiguous" % what)
        return C.c_void_p(tensor.data_ptr())

    def _float4_tensor_ptr(self, what, tensor):
        """_tensor_ptr for a float4 output: (H, W, 4) float32."""
        return self._tensor_ptr(what, tensor, np.float32, (self.height, self.width, 4))

    def denoise(self, iterations=None, sigma_color=None, sigma_normal=None, sigma_plane=None, albedo=True, framebuffer=False,
                gbuffer=True):
        """srt_denoise over the whole frame: the accumulator as it stands, guided by the first-hit buffers.  Arguments left at
        None take DENOISE_DEFAULTS.  gbuffer=True first enqueues render_gbuffer() for the guides the filter reads (with the
        current scene and camera); gbuffer=False uses the guides as they are (rendered earlier or bound).  Asynchronous."""
        p = denoise_params(iterations, sigma_color, sigma_normal, sigma_plane, albedo, framebuffer, lib=self.L)
        if gbuffer:
            self._render_guides(DENOISE_GUIDES | (GBUF_ALBEDO if albedo else 0), "denoise")
        self._ck(self.L.srt_denoise(self._h, C.byref(p)))

    def denoised(self):
        """srt_read_denoised: the result, (H, W, 4) float32, rows = scene rows (the orientation of accumulator())."""
        return self._read_image(self.L.srt_read_denoised, (self.height, self.width, 4), np.float32)

    def bind_denoised(self, tensor):
        """srt_bind_denoised: write the result into a torch tensor on this tracer's device, (H, W, 4) float32 and contiguous
        (None: the handle's own buffer).  Checked here, before any native call, as bind_gbuffer checks."""
        self._ck(self.L.srt_bind_denoised(self._h, self._float4_tensor_ptr("bind_denoised", tensor)))

    def temporal(self, samples=1, max_samples=None, plane_tolerance=None, normal_threshold=None, reset=False, framebuffer=False,
                 gbuffer=True):
        """srt_temporal_accumulate: blend the accumulator (which must hold `samples` samples of the current camera) with the
        history of the previous call, reprojected, in place.  Arguments left at None take TEMPORAL_DEFAULTS.  gbuffer=True
        first enqueues render_gbuffer() for the guides it reads (current scene and camera) and, while mirror_history() is on,
        render_reflection_gbuffer() for the four reflection outputs that mode reads; gbuffer=False uses the guides as they
        are.  Asynchronous.  The next render() must reset."""
        p = temporal_params(samples, max_samples, plane_tolerance, normal_threshold, reset, framebuffer, lib=self.L)
        if gbuffer:
            self._render_guides(TEMPORAL_GUIDES | (GBUF_ALBEDO if self._moments_albedo else 0), "temporal", True)
            if self._mirror_history:
                self.render_reflection_gbuffer(outputs=MIRROR_HISTORY_GUIDES)
        self._ck(self.L.srt_temporal_accumulate(self._h, C.byref(p)))

    def history_length(self):
        """srt_read_history_length: L of the last temporal() call, (H, W) float32, rows = scene rows."""
        return self._read_image(self.L.srt_read_history_length, (self.height, self.width), np.float32)

    def motion_output(self, on=True):
        """srt_motion_output: every later temporal() also writes the motion buffer (u - x, v - y, Wsum, 0)."""
        self._ck(self.L.srt_motion_output(self._h, 1 if on else 0))

    def motion(self):
        """srt_read_motion: the motion buffer of the last temporal() call that wrote it, (H, W, 4) float32, scene rows."""
        return self._read_image(self.L.srt_read_motion, (self.height, self.width, 4), np.float32)

    def bind_motion(self, tensor):
        """srt_bind_motion: write the motion buffer into a torch tensor on this tracer's device, (H, W, 4) float32 and
        contiguous (None: the handle's own buffer).  Checked here, before any native call, as bind_denoised checks."""
        self._ck(self.L.srt_bind_motion(self._h, self._float4_tensor_ptr("bind_motion", tensor)))

    def upsample(self, steps=None, stripe_width=None, sigma_normal=None, sigma_plane=None, in_place=False, framebuffer=False,
                 gbuffer=True):
        """srt_upsample over the whole frame: every pixel rebuilt from the anchors of the steps x steps blocks a render(steps=...,
        stripe_width=...) traced, guided by the first-hit buffers.  Arguments left at None take UPSAMPLE_DEFAULTS.
        in_place=True writes the non-anchor pixels into the accumulator (the next render() must reset) instead of the
        upsampled buffer.  gbuffer=True first enqueues render_gbuffer() for the guides it reads (current scene and camera);
        gbuffer=False uses the guides as they are.  Asynchronous."""
        p = upsample_params(steps, stripe_width, sigma_normal, sigma_plane, in_place, framebuffer, lib=self.L)
        if gbuffer:
            self._render_guides(UPSAMPLE_GUIDES, "upsample", True)
        self._ck(self.L.srt_upsample(self._h, C.byref(p)))

    def upsampled(self):
        """srt_read_upsampled: the result, (H, W, 4) float32, rows = scene rows (the orientation of accumulator())."""
        return self._read_image(self.L.srt_read_upsampled, (self.height, self.width, 4), np.float32)

    def bind_upsampled(self, tensor):
        """srt_bind_upsampled: write the result into a torch tensor on this tracer's device, (H, W, 4) float32 and contiguous
        (None: the handle's own buffer).  Checked here, before any native call, as bind_denoised checks."""
        self._ck(self.L.srt_bind_upsampled(self._h, self._float4_tensor_ptr("bind_upsampled", tensor)))

    def render_subsamples(self, k=None, rows=None, flags=0):
        """srt_render_subsamples: the hit object of the k x k sub-pixel rays of every pixel of memory rows `rows` (default: the
        whole frame); k None takes ANTIALIAS_DEFAULTS.  Asynchronous, like render_gbuffer()."""
        rb, re = self._band(rows)
        p = SubsampleParams(int(rb), int(re), int(antialias_defaults(self.L)["k"] if k is None else k), int(flags))
        self._ck(self.L.srt_render_subsamples(self._h, C.byref(p)))
        self._subsample_k = p.k

    def subsamples(self, k=None):
        """srt_read_subsamples: (k*k, H, W) int32, rows = scene rows; k is that of the last render_subsamples of this tracer
        unless given (a buffer filled by other means)."""
        k = int(self._subsample_k if k is None else k)
        return self._read_image(self.L.srt_read_subsamples, (max(k, 1) ** 2, self.height, self.width), np.int32)

    def bind_subsamples(self, tensor, k=None):
        """srt_bind_subsamples: keep the sub-samples in a torch tensor on this tracer's device, (k*k, H, W) int32 and
        contiguous (None: the handle's own buffer); k None takes the tensor's first dimension.  Checked before any native
        call, as bind_gbuffer checks."""
        if tensor is None:
            self._ck(self.L.srt_bind_subsamples(self._h, None))
            return
        if k is None:
            k = {1: 1, 4: 2, 9: 3, 16: 4}.get(tensor.shape[0] if getattr(tensor, "ndim", 0) == 3 else None)
        if k not in (1, 2, 3, 4):
            raise ValueError("bind_subsamples: want (k*k, H, W) for k in 1..4")
        ptr = self._tensor_ptr("bind_subsamples", tensor, np.int32, (k * k, self.height, self.width))
        self._ck(self.L.srt_bind_subsamples(self._h, ptr))
        self._subsample_k = k

    def antialias(self, k=None, denoised=False, framebuffer=False, guides=True):
        """srt_antialias over the whole frame: every pixel rebuilt from its own colour and those of the neighbours whose object
        its k x k sub-samples see.  The colour is the accumulator or, with denoised=True, the denoised buffer.  guides=True
        first enqueues render_gbuffer("object") and render_subsamples(k) for the current scene and camera; guides=False
        uses both as they are.  Asynchronous."""
        p = antialias_params(k, denoised, framebuffer, lib=self.L)
        if guides:
            self._render_guides(GBUF_OBJECT, "antialias", True)
            self.render_subsamples(p.k)
        self._ck(self.L.srt_antialias(self._h, C.byref(p)))

    def antialiased(self):
        """srt_read_antialiased: the result, (H, W, 4) float32, rows = scene rows (the orientation of accumulator())."""
        return self._read_image(self.L.srt_read_antialiased, (self.height, self.width, 4), np.float32)

    def bind_antialiased(self, tensor):
        """srt_bind_antialiased: write the result into a torch tensor on this tracer's device, (H, W, 4) float32 and contiguous
        (None: the handle's own buffer).  Checked here, before any native call, as bind_denoised checks."""
        ptr = self._float4_tensor_ptr("bind_antialiased", tensor)
        self._ck(self.L.srt_bind_antialiased(self._h, ptr))

    def half_ptr(self):
        """srt_device_half: the device address of the handle's own second-half buffer (allocated on first use), W*H float4.
        Render into it with bind_output(None, half_ptr()), render(...), bind_output()."""
        p = C.c_void_p()
        self._ck(self.L.srt_device_half(self._h, C.byref(p)))
        return p.value

    def bind_half(self, tensor):
        """srt_bind_half: take half B from a torch tensor on this tracer's device, (H, W, 4) float32 and contiguous (None: the
        handle's own buffer).  Checked here, before any native call, as bind_denoised checks."""
        self._ck(self.L.srt_bind_half(self._h, self._float4_tensor_ptr("bind_half", tensor)))

    def variance(self, albedo=None, merge=None, gbuffer=True):
        """srt_variance over the whole frame: the squared half-difference of the luminances of the accumulator and the half
        buffer; merge=True also leaves the mean of the halves in the accumulator.  Arguments left at None take
        VARIANCE_DEFAULTS.  gbuffer=True first enqueues render_gbuffer() for the guides the pass reads; gbuffer=False uses the
        guides as they are.  Asynchronous."""
        p = variance_params(albedo, merge, lib=self.L)
        if gbuffer:
            self._render_guides(GBUF_OBJECT | (GBUF_ALBEDO if p.flags & VARIANCE_ALBEDO else 0), "variance")
        self._ck(self.L.srt_variance(self._h, C.byref(p)))

    def variance_map(self):
        """srt_read_variance: the variance, (H, W) float32, rows = scene rows (the orientation of accumulator())."""
        return self._read_image(self.L.srt_read_variance, (self.height, self.width), np.float32)

    def bind_variance(self, tensor):
        """srt_bind_variance: keep the variance in a torch tensor on this tracer's device, (H, W) float32 and contiguous (None:
        the handle's own buffer).  Checked here, before any native call, as bind_denoised checks."""
        self._ck(self.L.srt_bind_variance(self._h, self._tensor_ptr("bind_variance", tensor, np.float32, (self.height, self.width))))

    def denoise_variance(self, iterations=None, sigma_luminance=None, sigma_normal=None, sigma_plane=None, albedo=True,
                         framebuffer=False, gbuffer=True):
        """srt_denoise_variance over the whole frame: denoise() with the variance-scaled luminance edge-stop, on the accumulator
        and the variance buffer as they stand; the result is what denoised() reads.  Arguments left at None take
        DENOISE_VARIANCE_DEFAULTS.  gbuffer as in denoise().  Asynchronous."""
        p = denoise_variance_params(iterations, sigma_luminance, sigma_normal, sigma_plane, albedo, framebuffer, lib=self.L)
        if gbuffer:
            self._render_guides(DENOISE_GUIDES | (GBUF_ALBEDO if albedo else 0), "denoise_variance")
        self._ck(self.L.srt_denoise_variance(self._h, C.byref(p)))

    def moments_output(self, on=True, albedo=False):
        """srt_moments_output: every later temporal() also keeps the luminance moments (M1, M2, Lm, 0) of the history;
        albedo=True takes the luminance of the demodulated colour (SRT_VARIANCE_ALBEDO; temporal(gbuffer=True) then renders the
        ALBEDO guide too).  Switching it, or changing albedo, starts the moments afresh."""
        self._ck(self.L.srt_moments_output(self._h, 1 if on else 0, VARIANCE_ALBEDO if albedo else 0))
        self._moments_albedo = bool(on and albedo)

    def moments(self):
        """srt_read_moments: the records of the last temporal() call, (H, W, 4) float32 (M1, M2, Lm, 0), scene rows."""
        return self._read_image(self.L.srt_read_moments, (self.height, self.width, 4), np.float32)

    def temporal_variance(self, min_frames=None, radius=None):
        """srt_temporal_variance over the whole frame: the variance buffer (variance_map(), denoise_variance()) from the
        moments of the last temporal() call and the OBJECT guide as it stands; pixels whose moments are younger than
        min_frames frames take a spatial estimate over (2 * radius + 1)^2 pixels.  Arguments left at None take
        TEMPORAL_VARIANCE_DEFAULTS.  Asynchronous."""
        p = temporal_variance_params(min_frames, radius, lib=self.L)
        self._ck(self.L.srt_temporal_variance(self._h, C.byref(p)))

    def wait(self):
        self._ck(self.L.srt_wait(self._h))

    def poll(self):
        d = C.c_int(0)
        self._ck(self.L.srt_poll(self._h, C.byref(d)))
        return bool(d.value)

    def pick(self, x, y):
        """Raytracer.cpp:525-541; y in scene rows. Returns the list index or -1."""
        idx = C.c_int(-2)
        self._ck(self.L.srt_pick(self._h, int(x), int(y), C.byref(idx)))
        return idx.value

    def stats(self):
        s = Stats()
        self._ck(self.L.srt_get_stats(self._h, C.byref(s)))
        return s

    def work_counts(self):
        """srt_get_work_counts: the loop counts of the last render (it must have had count_work=True)."""
        return self._get_record(WorkCounts, self.L.srt_get_work_counts)

    # ---- buffers ---------------------------------------------------------------------
    def framebuffer(self, rows=None):
        rb, re = rows if rows is not None else (0, self.height)
        out = np.empty((re - rb, self.width), dtype=np.uint32)
        self._ck(self.L.srt_read_framebuffer(self._h, out.ctypes.data_as(C.c_void_p), self.width * 4, rb, re))
        return out

    def read_framebuffer_async(self, dst_ptr, rows=None, copy_stream=0):
        """srt_read_framebuffer_async: memory rows `rows` into host memory at dst_ptr (pinned, tightly packed), enqueued on
        hipStream_t `copy_stream` (0: the launch stream) behind the renders enqueued so far; returns at once."""
        rb, re = self._band(rows)
        self._ck(self.L.srt_read_framebuffer_async(self._h, C.c_void_p(dst_ptr), self.width * 4, rb, re, C.c_void_p(copy_stream or 0)))

    def accumulator(self):
        return self._read_image(self.L.srt_read_accumulator, (self.height, self.width, 4), np.float32)

    def write_accumulator(self, arr):
        a = np.ascontiguousarray(arr, dtype=np.float32)
        assert a.shape == (self.height, self.width, 4)
        self._ck(self.L.srt_write_accumulator(self._h, a.ctypes.data_as(C.POINTER(C.c_float))))

    def estimate_row_costs(self, bounces, seed=0):
        """srt_estimate_row_costs: relative cost per memory row (list of floats) from the device-side probe."""
        out = (C.c_float * self.height)()
        self._ck(self.L.srt_estimate_row_costs(self._h, int(bounces), int(seed), out))
        return list(out)

    def gather_band_from(self, src, rows):
        """srt_gather_band: memory rows `rows` of PathTracer `src`'s framebuffer into this one's (device to device)."""
        self._ck(self.L.srt_gather_band(self._h, src._h, int(rows[0]), int(rows[1])))

    def gather_path(self):
        """srt_gather_path: which way this tracer's last band went in gather_band_from (text)."""
        return (self.L.srt_gather_path(self._h) or b"").decode()

    def device_framebuffer_ptr(self):
        p = C.c_void_p()
        self._ck(self.L.srt_device_framebuffer(self._h, C.byref(p)))
        return p.value
