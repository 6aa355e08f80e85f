// srt_render — command-line front end of the host layer: load a scene in the reference's
// JSON format, path-trace it on one MI355X, write the framebuffer as a binary PPM (P6)
// top-down (the framebuffer's memory rows are already in blit order, Raytracer.cpp:64).
//
// The file reads top-down as main() runs: the options (one struct, one table row each), parse(), validate() with every
// cross-option rule in the order its messages win, the file helpers, then one function per mode.  DESIGN.md §4.37.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "renderer.hpp"

using namespace srt_host;

// --probe-grid G --probe-directions K --irradiance-out FILE: a real-time preview of the diffuse indirect light.  The first-hit buffers of
// the W x H frame, light probes (srt_trace_light_probes: K spherical Fibonacci directions, samples 1..--radiance N, --bounces, --seed,
// id_base 0) at the grid's positions (srt_probe_grid_positions), then srt_shade_probe_grid over the whole frame with the shading flags
// and the default or the hemisphere band weights.  FILE receives W*H float4, scene rows.
// --probe-depth R: the filtered visibility test instead of none or the exact one: srt_trace_probe_depth at the same positions and
// directions (resolution R, --probe-depth-sharpness, --probe-depth-max), then srt_shade_probe_grid_depth (--probe-depth-bias);
// --probe-depth-out receives the probes' R*R float4 moments.
struct ProbeDepthOptions {
    int resolution = 0;  // 0: no --probe-depth
    int sharpness = 5;
    float max_distance = 10000.0f, bias = 0.0f;
    std::string out;
    bool given = false, option = false;  // --probe-depth itself, any of its options
};
// --probe-classify: srt_classify_probes on the grid first (--probe-relocate: with relocation along the same directions;
// --probe-clearance, --probe-max-offset, --probe-steps), the probes and depth maps traced at the positions it gives, and
// srt_shade_probe_grid_states in place of the shading call; --states-out receives the probes' records (float4 each).
struct ProbeClassifyOptions {
    bool on = false, relocate = false;
    float clearance = 0.2f, max_offset = 0.45f;
    int steps = 8;
    std::string out;
    bool option = false;  // any of its options
};
// --move-object IDX:DX,DY,DZ: before every frame but the first, DX, DY, DZ are added to the position of object IDX
struct ObjectMove {
    size_t index;
    float step[3];
};

// --probe-update FRAMES (with --probe-classify): the per-frame route in place of the one trace: the classification once, the list
// of active probes once (srt_list_probes), then FRAMES times a listed trace of --probe-samples N samples with seed = the frame
// number (and, with --probe-depth, a listed depth trace) and srt_blend_probes with --probe-hysteresis H for both hystereses; the
// frame is shaded from the histories.  With --move-object the objects move before every frame but the first: srt_update_scene, the
// classification and the list again, the traces at the new positions, and the blend with SRT_PROBE_BLEND_PREVIOUS_STATES against the
// records of the frame before, so that a probe that moved, or went into or came out of an object, restarts.
struct ProbeUpdateOptions {
    int frames = 0;  // 0: no --probe-update
    int samples = 1;
    float hysteresis = 0.9f;
    bool given = false, option = false;  // --probe-update itself, any of its options
};

// --probe-tail [--probe-tail-depth] [--probe-tail-states] [--probe-tail-normal-weight]: srt_probe_tail for the traces of a flow.
// With --rays --radiance N the grid and its coefficients come from --probe-tail-grid G and --probe-tail-coefficients FILE.f32 (P x 9
// float4: what --probes-out writes for the grid's positions); depth maps and records exist in the --probe-grid flow only.
// With --probe-grid: --probe-feedback F (1..4096; --probe-tail alone means 2) runs F rounds of (trace the probes at --probe-bounces B
// bounces, default --bounces, seed = the round, then srt_blend_probes with the library's defaults into the coefficient history);
// round 1 has no history and runs with the mode off, every later round runs with the tail reading the history (copied through the
// host into the grid's coefficient array: the trace writes its own output, never the array it reads), with the flow's depth maps
// (--probe-depth R) under --probe-tail-depth and its records (--probe-classify) under --probe-tail-states.  The frame is shaded
// from the history.  --probe-tail-frame also renders the picture: after the rounds, PathTraceRenderer::renderProbeTailFrame(--spp,
// --bounces, --seed) with the tail reading the history (and the maps and records the two flags ask for), written to --out.
// --probe-scroll SX,SY,SZ [--probe-scroll-after ROUND, default 1]: after the blend of round ROUND the grid moves by SX, SY, SZ cells
// (PathTraceRenderer::scrollProbes on the coefficient history with SRT_PROBE_SCROLL_SET_GRID | _COUNT_WORK); the positions, and the
// flow's records and depth maps, are made again for the moved grid, and the rounds go on: the probes that stayed inside keep
// blending, the others restart.  The frame is shaded on the moved grid.
struct ProbeTailOptions {
    bool on = false, depth = false, states = false, normal_weight = false;
    bool frame = false;     // --probe-tail-frame
    int frame_spp = 0;      // --spp (validate)
    std::string frame_out;  // --out (validate)
    int feedback = 0;  // 0: no --probe-feedback (validate: --probe-tail with --probe-grid alone means 2)
    int bounces = -1;  // < 0: --bounces
    bool scroll_on = false;  // --probe-scroll
    int32_t scroll[3] = {0, 0, 0};
    int scroll_after = 1;    // --probe-scroll-after
    std::string grid, coefficients;
    bool feedback_given = false, bounces_given = false;
    bool scroll_given = false, scroll_ok = true;  // --probe-scroll or --probe-scroll-after; --probe-scroll's text was three integers
    uint32_t flags() const {
        return (depth ? SRT_PROBE_TAIL_DEPTH : 0u) | (states ? SRT_PROBE_TAIL_STATES : 0u) | (normal_weight ? SRT_PROBE_TAIL_NORMAL_WEIGHT : 0u);
    }
};

// Every option with its default (the frame's: Raytracer.cpp:26-27,31-32).  A *_given flag says that the option stood on the command
// line where its value cannot.  parse() fills everything but the last block, which validate() derives.
struct Options {
    std::string scene_path, out = "frame.ppm", resave;
    int W = 1280, H = 720, spp = 32, bounces = 2, fov = 55, device = 0;
    unsigned seed = 0;
    std::vector<int> devices;
    bool equal_bands = false;
    // the frame's stages and the passes after it
    std::string gbuffer, denoise, upsample, denoise_variance;
    int steps = 1, aa = 0;
    bool aa_given = false;
    std::string vis_out;
    int ao = 0;
    bool ao_given = false, sun_visibility = false;
    float ao_radius = INFINITY;
    bool reflection_guides = false, reflection_bounces_given = false;
    int reflection_bounces = 8;
    std::string reflection_out;
    // --temporal
    int temporal = 0;
    float move[3] = {0, 0, 0}, turn_deg = 0;
    std::vector<ObjectMove> object_moves;
    bool refit = false, temporal_variance = false, mirror_history = false, mirror_radius_given = false;
    float mirror_radius = 2.0f;
    // --adaptive
    int adaptive = 0, adaptive_max = 0;
    float adaptive_threshold = 0;
    bool adaptive_given = false, adaptive_threshold_given = false, adaptive_max_given = false;
    std::string counts_out;
    // --rays, --probes
    std::string rays_in, rays_out;
    bool rays_normalize = false, rays_any_hit = false;
    int radiance = 0;
    bool radiance_given = false;
    std::string probes_in, probes_out, probe_directions, probe_radiance_out;
    // --probe-grid
    std::string probe_grid_arg, irradiance_out;
    bool probe_visibility = false, probe_normal_weight = false, probe_albedo = false, probe_hemisphere = false;
    ProbeDepthOptions probe_depth;
    ProbeClassifyOptions probe_classify;
    ProbeUpdateOptions probe_update;
    ProbeTailOptions probe_tail;
    int probe_cascade_levels = 0;  // 0: no --probe-cascade
    float probe_cascade_blend = 1.0f;
    bool probe_cascade_given = false;
    // what validate() derives: --probe-grid's and --probe-tail-grid's grids and --probe-directions as a count
    srt_probe_grid probe_grid{}, tail_grid{};
    int probe_grid_directions = 0;

    int probe_samples() const { return radiance_given ? radiance : 16; }  // --radiance N in the probe flows
};

static void usage() {
    std::fprintf(stderr,
                 "usage: srt_render --scene FILE [--width 1280] [--height 720] [--spp 32] [--bounces 2]\n"
                 "                  [--fov 55] [--seed 0] [--device 0 | --devices 0,1,2,...] [--out frame.ppm] [--resave FILE]\n"
                 "                  [--gbuffer PREFIX] [--denoise PATH] [--temporal FRAMES [--move R,U,F] [--turn DEG]\n"
                 "                  [--move-object IDX:DX,DY,DZ]... [--refit]] [--steps N] [--upsample PATH] [--aa K]\n"
                 "                  [--denoise-variance PATH] [--temporal-variance] [--mirror-history [--mirror-radius R]]\n"
                 "                  [--ao N [--ao-radius R]] [--sun-visibility] [--vis-out FILE]\n"
                 "                  [--reflection-guides] [--reflection-bounces N] [--reflection-out PREFIX]\n"
                 "       srt_render --scene FILE --rays IN.f32 --rays-out OUT.bin [--rays-normalize] [--any-hit] [--device 0]\n"
                 "       srt_render --scene FILE --rays IN.f32 --rays-out OUT.bin --radiance N [--bounces B] [--seed S] [--rays-normalize]\n"
                 "       srt_render --scene FILE --probes IN.f32 --probe-directions K|FILE.f32 --probes-out OUT.bin [--radiance N]\n"
                 "                  [--probe-radiance-out FILE] [--bounces B] [--seed S]\n"
                 "       srt_render --scene FILE --probe-grid OX,OY,OZ,SX,SY,SZ,NX,NY,NZ --probe-directions K [--radiance N] --irradiance-out FILE\n"
                 "                  [--probe-visibility] [--probe-normal-weight] [--probe-albedo] [--probe-hemisphere] [--width W] [--height H] ...\n"
                 "                  [--probe-depth R [--probe-depth-sharpness S] [--probe-depth-max D] [--probe-depth-bias B] [--probe-depth-out FILE]]\n"
                 "                  [--probe-classify [--probe-relocate] [--probe-clearance C] [--probe-max-offset F] [--probe-steps M] [--states-out FILE]]\n"
                 "                  [--probe-update FRAMES [--probe-hysteresis H] [--probe-samples N]]\n"
                 "                  [--probe-cascade L [--probe-cascade-blend B]]\n"
                 "                  [--probe-tail [--probe-feedback F [--probe-scroll SX,SY,SZ [--probe-scroll-after ROUND]]] [--probe-bounces B] [--probe-tail-frame [--spp N] [--out frame.ppm]]]\n"
                 "       srt_render --scene FILE --adaptive ROUNDS [--adaptive-threshold T] [--adaptive-max M] [--counts-out FILE] [--spp N] ...\n"
                 "  --devices: one frame over several GPUs of this node in one process (equal row bands, one gather;\n"
                 "             a device may be listed more than once); bands of equal estimated cost (default; --balance is accepted\n"
                 "             and means the same), --equal-bands: bands of equal height\n"
                 "  --gbuffer: also write the first-hit buffers as PREFIX_object.npy (int32 HxW), PREFIX_normal_depth.npy,\n"
                 "             PREFIX_position.npy and PREFIX_albedo.npy (float32 HxWx4), rows top-down like the PPM\n"
                 "             (with --devices: made for the whole frame on the first device)\n"
                 "  --denoise: also render the first-hit buffers, denoise the accumulator with the library's defaults\n"
                 "             (srt_denoise) and write the tone-mapped result to PATH as a PPM (single device only)\n"
                 "  --denoise-variance: render the frame again as two independently seeded halves of --spp / 2 samples each, estimate\n"
                 "             the per-pixel variance from them (srt_variance) and write the tone-mapped result of the variance-guided\n"
                 "             filter with the library's defaults (srt_denoise_variance) to PATH as a PPM; needs an even --spp >= 2;\n"
                 "             not with --denoise, --temporal, --steps, --upsample or --devices\n"
                 "  --steps:   trace one ray per N x N block of pixels and copy its colour into the block (the progressive-resolution\n"
                 "             blocks of the reference's interactive frames); single device, not with --temporal\n"
                 "  --upsample: also render the first-hit buffers, rebuild the full-resolution frame from the blocks' anchor\n"
                 "             pixels with the library's defaults (srt_upsample) and write the tone-mapped result to PATH as a PPM;\n"
                 "             with --denoise the upsampler works in place and the denoiser runs on its result (single device only)\n"
                 "  --aa:      anti-alias the silhouettes: trace the first hit at K x K sub-pixel positions (K in 1..4,\n"
                 "             srt_render_subsamples) and write every PPM (--out, --upsample, --denoise, with or without --temporal) as\n"
                 "             the resolve of its stage (srt_antialias); with --upsample the upsampler works in place (single device only)\n"
                 "  --temporal: render FRAMES frames of --spp samples each while the camera moves, keeping samples across\n"
                 "             frames (srt_temporal_accumulate), and write the last one to --out (--denoise PATH: also its\n"
                 "             denoised form); before every frame but the first the camera moves by R, U, F along its right,\n"
                 "             up and forward axes (--move) and turns by DEG degrees about world up (--turn); single device only\n"
                 "  --move-object: with --temporal, before every frame but the first add DX, DY, DZ to the position of object IDX\n"
                 "             (list order) and keep the history across the edit (srt_update_scene); may be given several times\n"
                 "  --refit:   with --move-object, refit the mesh BVH on the device after every edit instead of rebuilding it on the\n"
                 "             host (srt_update_mode); the same frames; what every update did is printed\n"
                 "  --temporal-variance: with --temporal, also keep the luminance moments of the history (srt_moments_output) and\n"
                 "             filter the --denoise frame by the per-pixel variance they give (srt_temporal_variance,\n"
                 "             srt_denoise_variance, the library's defaults) instead of srt_denoise; not with --steps, --upsample or\n"
                 "             --devices\n"
                 "  --mirror-history: with --temporal, reproject the pixels that look through mirrors by the virtual image of what they\n"
                 "             show and keep only history seen through the same mirror near the same point (srt_mirror_history);\n"
                 "             --mirror-radius R: the radius of that test in pixels (> 0; default: the library's, 2)\n"
                 "  --rays:    instead of rendering a frame, answer closest-hit queries (srt_trace_rays) for the rays in IN.f32: N records\n"
                 "             of 8 float32, origin x y z w (w ignored) and direction x y z t_max; --rays-out receives the five outputs\n"
                 "             one after the other: object (N int32), normal_depth, position, albedo (N x 4 float32 each), occluded\n"
                 "             (N int32); --rays-normalize normalizes every direction first; single device, no other output\n"
                 "  --any-hit: with --rays, ask srt_trace_occlusion (is there a hit with distance < t_max?) instead; --rays-out then receives\n"
                 "             the occluded array (N int32) alone, with the bits the closest-hit query gives it\n"
                 "  --radiance N: with --rays, ask srt_trace_radiance instead: the running mean of N (1..4096) path-traced samples of\n"
                 "             --bounces bounces along every ray (samples 1..N, --seed, ray i draws from the stream of pixel i); --rays-out\n"
                 "             then receives the N float4 alone; not with --any-hit\n"
                 "  --probes:  instead of rendering a frame, trace light probes (srt_trace_light_probes) at the positions in IN.f32: P records\n"
                 "             of 4 float32 (x y z w, w ignored); --probe-directions K: K (1..4096) spherical Fibonacci directions, or\n"
                 "             FILE.f32: K records of 4 float32 (x y z weight); --radiance N: samples per ray (1..4096, default 16) of\n"
                 "             --bounces bounces; --probes-out receives P x 9 float4 SH coefficients, --probe-radiance-out the P x K float4\n"
                 "             running means; single device, not with --rays, no frame options\n"
                 "  --probe-grid: instead of rendering a frame, shade it from a grid of light probes (srt_shade_probe_grid): probe (0,0,0) at\n"
                 "             OX,OY,OZ, spacings SX,SY,SZ > 0, NX x NY x NZ probes; the first-hit buffers of the frame are rendered, the probes traced\n"
                 "             (--probe-directions K: 1..4096 spherical Fibonacci directions; --radiance N: samples per ray, 1..4096, default 16;\n"
                 "             --bounces, --seed) and --irradiance-out receives W x H float4 (r g b, a = surviving weight), scene rows;\n"
                 "             --probe-visibility: only probes the surface sees; --probe-normal-weight: favour probes in front of the surface;\n"
                 "             --probe-albedo: times the albedo guide; --probe-hemisphere: band weights 1, 0.5, 0 (the mean over the hemisphere)\n"
                 "             instead of the cosine-weighted integral; single device, not with --rays, --probes, --temporal or --devices\n"
                 "  --probe-depth R: with --probe-grid, the filtered visibility test (srt_trace_probe_depth + srt_shade_probe_grid_depth): an\n"
                 "             octahedral depth map of R x R texels (4, 8 or 16) per probe from the same directions; --probe-depth-sharpness S\n"
                 "             (0..6, default 5); --probe-depth-max D: distance clamp (> 0, default 10000); --probe-depth-bias B (>= 0, default 0);\n"
                 "             --probe-depth-out receives the probes' R*R float4 moments; not with --probe-visibility\n"
                 "  --probe-classify: with --probe-grid, srt_classify_probes first: probes inside a sphere or a box are skipped by the shading\n"
                 "             (srt_shade_probe_grid_states); --probe-relocate: probes inside or nearer than --probe-clearance C (0..0.5 of the\n"
                 "             spacing, default 0.2) to a surface are moved by at most --probe-max-offset F (0..0.5, default 0.45) in\n"
                 "             --probe-steps M (1..64, default 8) lengths, and probes and depth maps are traced where they stand;\n"
                 "             --states-out receives the probes' records (offset, state bits); not with --probe-visibility\n"
                 "  --probe-update FRAMES: with --probe-classify, the per-frame route: the active probes are listed once (srt_list_probes), then\n"
                 "             FRAMES (1..4096) times a listed trace of --probe-samples N (1..4096, default 1) samples with seed = the frame number\n"
                 "             is blended into a history (srt_blend_probes, --probe-hysteresis H in [0, 1), default 0.9), and the frame is shaded\n"
                 "             from the history; with --probe-depth the depth maps are traced listed and blended too; with --move-object the\n"
                 "             objects move before every frame but the first, the grid is classified and listed again, and probes whose record\n"
                 "             changed restart (SRT_PROBE_BLEND_PREVIOUS_STATES)\n"
                 "  --adaptive ROUNDS: adaptive sampling in place of the uniform frame: an even --spp is the uniform seed, split into two\n"
                 "             independently seeded halves; then ROUNDS (1..64) rounds of srt_variance, srt_sample_budget and srt_render_adaptive\n"
                 "             on both halves, and the mean of the halves goes to --out; the frame's total samples are printed on stderr;\n"
                 "             single device, no other frame option\n"
                 "  --adaptive-threshold T: the budget's target relative standard error (> 0; default: the library's, 0.05)\n"
                 "  --adaptive-max M: the most samples a round adds to a pixel of a half (1..4096; default: the library's, 64)\n"
                 "  --counts-out FILE: with --adaptive, the per-pixel samples of the frame (W x H uint32, scene rows, both halves)\n"
                 "  --ao N:    after the frame, per-pixel ambient occlusion (srt_render_visibility): the fraction of N (1..4096) hemisphere\n"
                 "             segments of length --ao-radius (default: unbounded) at the first hit that are unoccluded; samples 1..N, --seed\n"
                 "  --sun-visibility: after the frame, per-pixel sun visibility: n . -sunDirection where the sun is seen, else 0\n"
                 "  --vis-out: receives the raw float32 planes (W x H each, scene rows), AO then SUN, whichever were asked for;\n"
                 "             needs --ao or --sun-visibility; single device, not with --temporal\n"
                 "  --reflection-guides: --denoise and --denoise-variance are guided by the first-hit buffers traced through chains of\n"
                 "             mirror-like surfaces (srt_render_reflection_gbuffer, the library's thresholds) instead of the first hits: a\n"
                 "             mirror is filtered by what is seen in it; needs one of the two; not with --devices or --temporal\n"
                 "  --reflection-bounces N: the most reflections a chain follows (0..64; default: the library's, 8); needs --reflection-guides\n"
                 "             or --reflection-out\n"
                 "  --reflection-out PREFIX: also write the reflection guides as PREFIX_object.npy, PREFIX_normal_depth.npy, PREFIX_position.npy,\n"
                 "             PREFIX_albedo.npy (as --gbuffer's) and PREFIX_bounces.npy (int32 HxW: reflections followed); not with --devices\n"
                 "             or --temporal\n"
                 "  --probe-tail: srt_probe_tail: radiance and light-probe paths that reach the bounce limit on a surface add the probe grid's\n"
                 "             radiance there.  With --rays --radiance N: the grid is --probe-tail-grid G (as --probe-grid's) and its coefficients\n"
                 "             --probe-tail-coefficients FILE.f32 (P x 9 float4, what --probes-out writes); --probe-tail-normal-weight: rule 6.\n"
                 "             With --probe-grid: --probe-feedback F (1..4096; --probe-tail alone: 2) rounds of (trace the probes at\n"
                 "             --probe-bounces B bounces, default --bounces, with the tail reading the coefficient history, then\n"
                 "             srt_blend_probes); round 1 runs with the mode off; the frame is shaded from the history;\n"
                 "             --probe-tail-depth needs --probe-depth R, --probe-tail-states needs --probe-classify; not with --probe-update\n"
                 "  --probe-cascade L: with --probe-grid ...: shade from L = 1..4 nested grids around the camera position (srt_shade_probe_cascade):\n"
                 "             level l has the grid's counts and its spacing times 2^l (srt_probe_cascade_grids; the grid's origin is not read);\n"
                 "             each level is traced as --probe-grid traces its grid (--probe-depth, --probe-classify apply to every level) and\n"
                 "             a pixel takes the finest level that holds its first hit, blended into the next across a border band of\n"
                 "             --probe-cascade-blend B cells (default 1).  Not with --probe-visibility, --probe-update or --probe-tail\n"
                 "  --probe-scroll SX,SY,SZ: with --probe-grid ... --probe-feedback F: after the blend of round --probe-scroll-after ROUND (1..F,\n"
                 "             default 1) the grid moves by SX, SY, SZ whole cells (srt_scroll_probes: the coefficient history of the probes\n"
                 "             that stay inside the grid is kept, the others restart; the origin follows), and the rounds go on; the frame is\n"
                 "             shaded on the moved grid\n"
                 "  --probe-tail-frame: with --probe-grid ... --probe-tail: after the feedback rounds also render the picture — --spp samples per\n"
                 "             pixel from n = 0 at --bounces bounces with --seed, every path ended in the history (srt_render_adaptive_tail), with\n"
                 "             the maps and records of --probe-tail-depth / --probe-tail-states — and write it to --out as a PPM; not with\n"
                 "             --devices, --temporal, --adaptive or --steps\n");
}

// How a row of the option table turns the text after the option into its destination: a flag takes no text; the others are named
// after the conversion they have always gone through (it decides what a malformed number becomes).
enum class Kind { Flag, Clear, Atoi, Strtoul, Strtof, Atof, Str, Custom };

struct OptionRow {
    const char* name;
    Kind kind;
    void* dest;                                      // bool, int, unsigned, float or std::string, by kind; null for Custom
    bool* given = nullptr;                           // raised when the option stands on the command line
    int (*custom)(Options&, const char*) = nullptr;  // Kind::Custom: 0, or the exit status after its own message
};

static int parse_devices(Options& o, const char* p) {  // --devices 0,1,2,...
    while (*p) {
        o.devices.push_back(std::atoi(p));
        while (*p && *p != ',') ++p;
        if (*p == ',') ++p;
    }
    return 0;
}

static int parse_move(Options& o, const char* p) {  // --move R,U,F
    for (int k = 0; k < 3; ++k) {
        char* end = nullptr;
        o.move[k] = std::strtof(p, &end);
        if (end == p || (k < 2 && *end != ',') || (k == 2 && *end)) {
            std::fprintf(stderr, "--move wants R,U,F\n");
            return 2;
        }
        p = end + 1;
    }
    return 0;
}

static int parse_move_object(Options& o, const char* p) {  // --move-object IDX:DX,DY,DZ
    char* end = nullptr;
    ObjectMove m{};
    m.index = (size_t)std::strtoul(p, &end, 10);
    bool ok = end != p && *end == ':';
    for (int k = 0; ok && k < 3; ++k) {
        p = end + 1;
        m.step[k] = std::strtof(p, &end);
        ok = end != p && (k < 2 ? *end == ',' : !*end);
    }
    if (!ok) {
        std::fprintf(stderr, "--move-object wants IDX:DX,DY,DZ\n");
        return 2;
    }
    o.object_moves.push_back(m);
    return 0;
}

static int parse_probe_scroll(Options& o, const char* v) {  // --probe-scroll SX,SY,SZ: a malformed one is validate()'s to refuse
    ProbeTailOptions& t = o.probe_tail;
    int n = 0;
    t.scroll_on = true;
    t.scroll_ok = std::sscanf(v, "%d,%d,%d%n", &t.scroll[0], &t.scroll[1], &t.scroll[2], &n) == 3 && v[n] == 0;
    return 0;
}

// One row per option: the name, the kind, the destination and the flag it raises.  (--balance clears what --equal-bands sets.)
static std::vector<OptionRow> option_table(Options& o) {
    ProbeDepthOptions& depth = o.probe_depth;
    ProbeClassifyOptions& classify = o.probe_classify;
    ProbeUpdateOptions& update = o.probe_update;
    ProbeTailOptions& tail = o.probe_tail;
    return {
        {"--scene", Kind::Str, &o.scene_path},
        {"--width", Kind::Atoi, &o.W},
        {"--height", Kind::Atoi, &o.H},
        {"--spp", Kind::Atoi, &o.spp},
        {"--bounces", Kind::Atoi, &o.bounces},
        {"--fov", Kind::Atoi, &o.fov},
        {"--seed", Kind::Strtoul, &o.seed},
        {"--device", Kind::Atoi, &o.device},
        {"--balance", Kind::Clear, &o.equal_bands},
        {"--equal-bands", Kind::Flag, &o.equal_bands},
        {"--devices", Kind::Custom, nullptr, nullptr, parse_devices},
        {"--out", Kind::Str, &o.out},
        {"--resave", Kind::Str, &o.resave},
        {"--gbuffer", Kind::Str, &o.gbuffer},
        {"--denoise", Kind::Str, &o.denoise},
        {"--denoise-variance", Kind::Str, &o.denoise_variance},
        {"--steps", Kind::Atoi, &o.steps},
        {"--upsample", Kind::Str, &o.upsample},
        {"--aa", Kind::Atoi, &o.aa, &o.aa_given},
        {"--temporal-variance", Kind::Flag, &o.temporal_variance},
        {"--refit", Kind::Flag, &o.refit},
        {"--rays", Kind::Str, &o.rays_in},
        {"--rays-out", Kind::Str, &o.rays_out},
        {"--rays-normalize", Kind::Flag, &o.rays_normalize},
        {"--any-hit", Kind::Flag, &o.rays_any_hit},
        {"--radiance", Kind::Atoi, &o.radiance, &o.radiance_given},
        {"--probes", Kind::Str, &o.probes_in},
        {"--probes-out", Kind::Str, &o.probes_out},
        {"--probe-directions", Kind::Str, &o.probe_directions},
        {"--probe-radiance-out", Kind::Str, &o.probe_radiance_out},
        {"--probe-grid", Kind::Str, &o.probe_grid_arg},
        {"--irradiance-out", Kind::Str, &o.irradiance_out},
        {"--probe-visibility", Kind::Flag, &o.probe_visibility},
        {"--probe-normal-weight", Kind::Flag, &o.probe_normal_weight},
        {"--probe-albedo", Kind::Flag, &o.probe_albedo},
        {"--probe-hemisphere", Kind::Flag, &o.probe_hemisphere},
        {"--probe-depth", Kind::Atoi, &depth.resolution, &depth.given},
        {"--probe-depth-sharpness", Kind::Atoi, &depth.sharpness, &depth.option},
        {"--probe-depth-max", Kind::Strtof, &depth.max_distance, &depth.option},
        {"--probe-depth-bias", Kind::Strtof, &depth.bias, &depth.option},
        {"--probe-depth-out", Kind::Str, &depth.out, &depth.option},
        {"--probe-classify", Kind::Flag, &classify.on},
        {"--probe-relocate", Kind::Flag, &classify.relocate, &classify.option},
        {"--probe-clearance", Kind::Strtof, &classify.clearance, &classify.option},
        {"--probe-max-offset", Kind::Strtof, &classify.max_offset, &classify.option},
        {"--probe-steps", Kind::Atoi, &classify.steps, &classify.option},
        {"--states-out", Kind::Str, &classify.out, &classify.option},
        {"--probe-update", Kind::Atoi, &update.frames, &update.given},
        {"--probe-hysteresis", Kind::Strtof, &update.hysteresis, &update.option},
        {"--probe-samples", Kind::Atoi, &update.samples, &update.option},
        {"--probe-tail", Kind::Flag, &tail.on},
        {"--probe-tail-frame", Kind::Flag, &tail.frame},
        {"--probe-tail-depth", Kind::Flag, &tail.depth},
        {"--probe-tail-states", Kind::Flag, &tail.states},
        {"--probe-tail-normal-weight", Kind::Flag, &tail.normal_weight},
        {"--probe-tail-grid", Kind::Str, &tail.grid},
        {"--probe-tail-coefficients", Kind::Str, &tail.coefficients},
        {"--probe-feedback", Kind::Atoi, &tail.feedback, &tail.feedback_given},
        {"--probe-bounces", Kind::Atoi, &tail.bounces, &tail.bounces_given},
        {"--probe-scroll", Kind::Custom, nullptr, &tail.scroll_given, parse_probe_scroll},
        {"--probe-scroll-after", Kind::Atoi, &tail.scroll_after, &tail.scroll_given},
        {"--probe-cascade", Kind::Atoi, &o.probe_cascade_levels, &o.probe_cascade_given},
        {"--probe-cascade-blend", Kind::Strtof, &o.probe_cascade_blend, &o.probe_cascade_given},
        {"--adaptive", Kind::Atoi, &o.adaptive, &o.adaptive_given},
        {"--adaptive-threshold", Kind::Strtof, &o.adaptive_threshold, &o.adaptive_threshold_given},
        {"--adaptive-max", Kind::Atoi, &o.adaptive_max, &o.adaptive_max_given},
        {"--counts-out", Kind::Str, &o.counts_out},
        {"--ao", Kind::Atoi, &o.ao, &o.ao_given},
        {"--ao-radius", Kind::Strtof, &o.ao_radius},
        {"--sun-visibility", Kind::Flag, &o.sun_visibility},
        {"--vis-out", Kind::Str, &o.vis_out},
        {"--reflection-guides", Kind::Flag, &o.reflection_guides},
        {"--reflection-bounces", Kind::Atoi, &o.reflection_bounces, &o.reflection_bounces_given},
        {"--reflection-out", Kind::Str, &o.reflection_out},
        {"--mirror-history", Kind::Flag, &o.mirror_history},
        {"--mirror-radius", Kind::Atof, &o.mirror_radius, &o.mirror_radius_given},
        {"--temporal", Kind::Atoi, &o.temporal},
        {"--turn", Kind::Strtof, &o.turn_deg},
        {"--move", Kind::Custom, nullptr, nullptr, parse_move},
        {"--move-object", Kind::Custom, nullptr, nullptr, parse_move_object},
    };
}

// The command line into the options, in argv order: 0, or 2 after the message of the first argument that does not parse.
static int parse(int argc, char** argv, Options& o) {
    const std::vector<OptionRow> table = option_table(o);
    for (int i = 1; i < argc; ++i) {
        const OptionRow* row = nullptr;
        for (size_t k = 0; k < table.size() && !row; ++k)
            if (!std::strcmp(argv[i], table[k].name)) row = &table[k];
        if (!row) {
            usage();
            return 2;
        }
        const char* v = nullptr;
        if (row->kind != Kind::Flag && row->kind != Kind::Clear) {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "%s needs a value\n", row->name);
                return 2;
            }
            v = argv[++i];
        }
        if (row->given) *row->given = true;
        switch (row->kind) {
            case Kind::Flag: *(bool*)row->dest = true; break;
            case Kind::Clear: *(bool*)row->dest = false; break;
            case Kind::Atoi: *(int*)row->dest = std::atoi(v); break;
            case Kind::Strtoul: *(unsigned*)row->dest = (unsigned)std::strtoul(v, nullptr, 10); break;
            case Kind::Strtof: *(float*)row->dest = std::strtof(v, nullptr); break;
            case Kind::Atof: *(float*)row->dest = (float)std::atof(v); break;
            case Kind::Str: *(std::string*)row->dest = v; break;
            case Kind::Custom:
                if (int e = row->custom(o, v)) return e;
                break;
        }
    }
    return 0;
}

// --probe-grid OX,OY,OZ,SX,SY,SZ,NX,NY,NZ: false (with nothing written to g) unless the text is nine numbers, the last three integers
static bool parse_probe_grid(const char* p, srt_probe_grid* g) {
    char* end = nullptr;
    for (int k = 0; k < 9; ++k) {
        if (k < 6) (k < 3 ? g->origin[k] : g->spacing[k - 3]) = std::strtof(p, &end);
        else {
            const long n = std::strtol(p, &end, 10);
            if (n < 1 || n > (1L << 30)) return false;
            g->counts[k - 6] = (int32_t)n;
        }
        if (end == p || (k < 8 ? *end != ',' : *end != 0)) return false;
        p = end + 1;
    }
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(g->origin[a]) || !std::isfinite(g->spacing[a]) || !(g->spacing[a] > 0)) return false;
    return (long long)g->counts[0] * g->counts[1] <= (1LL << 30) && (long long)g->counts[0] * g->counts[1] * g->counts[2] <= (1LL << 30);
}

static int refuse(const std::string& text) {
    std::fputs(text.c_str(), stderr);
    return 2;
}

// Every rule that needs the command line alone, in the order in which the messages win when several are broken: 0 or 2.  The modes
// that render no frame each refuse a list of frame options of their own; the lists are built from the named sets below so that
// what one mode refuses and another lets through (and then ignores) can be read off.  What the rules derive — the parsed grids,
// the direction count, --probe-tail's defaults and --probe-tail-frame's --spp and --out — is stored as they pass.
static int validate(Options& o) {
    ProbeDepthOptions& depth = o.probe_depth;
    ProbeClassifyOptions& classify = o.probe_classify;
    ProbeUpdateOptions& update = o.probe_update;
    ProbeTailOptions& tail = o.probe_tail;
    const bool multi_device = !o.devices.empty();  // everything but the plain frame is single device
    const bool rays = !o.rays_in.empty(), probes = !o.probes_in.empty();
    const bool grid_flow = !o.probe_grid_arg.empty();  // has a probe-grid flow
    // the frame options: the stages that change or filter the frame, --gbuffer, and the passes and modes added since
    const bool frame_stages = o.steps > 1 || o.aa_given || !o.denoise.empty() || !o.upsample.empty() || !o.denoise_variance.empty();
    const bool frame_outputs = frame_stages || !o.gbuffer.empty();
    const bool frame_extras = o.adaptive_given || o.ao_given || o.sun_visibility || !o.vis_out.empty() || o.reflection_guides || !o.reflection_out.empty();

    if (!o.object_moves.empty() && !o.temporal && !update.given) return refuse("--move-object needs --temporal or --probe-update\n");
    if (o.refit && o.object_moves.empty()) return refuse("--refit needs --move-object\n");
    if (o.scene_path.empty() || o.W <= 0 || o.H <= 0 || o.spp <= 0 || o.temporal < 0 || o.steps < 1) {
        usage();
        return 2;
    }
    if (o.rays_in.empty() != o.rays_out.empty() || ((o.rays_normalize || o.rays_any_hit) && !rays))
        return refuse("--rays, --rays-out, --rays-normalize and --any-hit go together: --rays IN.f32 --rays-out OUT.bin [--rays-normalize] [--any-hit]\n");
    if (depth.given || depth.option) {
        if (!grid_flow || !depth.given)
            return refuse("--probe-depth R and its options go with --probe-grid: --probe-grid G --probe-depth R [--probe-depth-sharpness S] [--probe-depth-max D] "
                          "[--probe-depth-bias B] [--probe-depth-out FILE]\n");
        if (o.probe_visibility) return refuse("--probe-depth and --probe-visibility exclude each other: the filtered or the exact test\n");
        if ((depth.resolution != 4 && depth.resolution != 8 && depth.resolution != 16) || depth.sharpness < 0 || depth.sharpness > 6 ||
            !(depth.max_distance > 0.0f) || !std::isfinite(depth.max_distance) || !(depth.bias >= 0.0f) || !std::isfinite(depth.bias))
            return refuse("--probe-depth takes 4, 8 or 16, --probe-depth-sharpness 0..6, --probe-depth-max a finite distance > 0 and --probe-depth-bias a finite "
                          "value >= 0\n");
    }
    if (classify.on || classify.option) {
        if (!grid_flow || !classify.on)
            return refuse("--probe-classify and its options go with --probe-grid: --probe-grid G --probe-classify [--probe-relocate] [--probe-clearance C] "
                          "[--probe-max-offset F] [--probe-steps M] [--states-out FILE]\n");
        if (o.probe_visibility)
            return refuse("--probe-classify and --probe-visibility exclude each other: the exact test towards relocated probes is not available\n");
        if (!(classify.clearance > 0.0f) || !(classify.clearance <= 0.5f) || !(classify.max_offset > 0.0f) || !(classify.max_offset <= 0.5f) ||
            classify.steps < 1 || classify.steps > 64)
            return refuse("--probe-classify: --probe-clearance and --probe-max-offset take a value in (0, 0.5], --probe-steps 1..64\n");
    }
    if (update.given || update.option) {
        if (!update.given || !classify.on || !grid_flow)
            return refuse("--probe-update and its options go with --probe-grid G --probe-classify: --probe-update FRAMES [--probe-hysteresis H] [--probe-samples N]\n");
        if (update.frames < 1 || update.frames > 4096 || update.samples < 1 || update.samples > 4096 || !(update.hysteresis >= 0.0f) || !(update.hysteresis < 1.0f))
            return refuse("--probe-update takes 1..4096 frames, --probe-samples 1..4096, --probe-hysteresis a value in [0, 1)\n");
    }
    if (tail.frame) {
        if (!tail.on || !grid_flow || multi_device || o.temporal || o.adaptive_given || o.steps > 1)
            return refuse("--probe-tail-frame goes with --probe-grid ... --probe-tail; not with --devices, --temporal, --adaptive or --steps\n");
        if (o.spp < 1) return refuse("--probe-tail-frame: --spp must be >= 1\n");
        tail.frame_spp = o.spp, tail.frame_out = o.out;
    }
    if (o.probe_cascade_given && (!grid_flow || o.probe_cascade_levels < 1 || o.probe_cascade_levels > SRT_PROBE_CASCADE_MAX_LEVELS ||
                                  !(o.probe_cascade_blend > 0.0f) || !std::isfinite(o.probe_cascade_blend) || o.probe_visibility || update.given || tail.on ||
                                  !o.object_moves.empty() || !depth.out.empty() || !classify.out.empty()))
        return refuse("--probe-cascade L (1..4) [--probe-cascade-blend B, finite and > 0] goes with --probe-grid, not with --probe-visibility, --probe-update, "
                      "--probe-tail, --move-object, --probe-depth-out or --states-out\n");
    if (tail.scroll_given && (!grid_flow || !tail.feedback_given || !tail.scroll_on || !tail.scroll_ok || tail.scroll_after < 1 || tail.scroll_after > tail.feedback))
        return refuse("--probe-scroll SX,SY,SZ (three integers) goes with --probe-grid ... --probe-feedback F, and --probe-scroll-after takes a round in 1..F\n");
    if (tail.on || tail.depth || tail.states || tail.normal_weight || tail.feedback_given || tail.bounces_given || !tail.grid.empty() || !tail.coefficients.empty()) {
        if (grid_flow) {  // the --probe-grid flow: feedback rounds
            if (!tail.grid.empty() || !tail.coefficients.empty() || update.given)
                return refuse("--probe-tail with --probe-grid reads the flow's own grid and history: no --probe-tail-grid / --probe-tail-coefficients, not with --probe-update\n");
            if (!tail.feedback_given) tail.feedback = 2;
            if (tail.feedback < 1 || tail.feedback > 4096 || (tail.bounces_given && tail.bounces < 0))
                return refuse("--probe-feedback takes 1..4096 rounds and --probe-bounces a count >= 0\n");
            if ((tail.depth && !depth.given) || (tail.states && !classify.on))
                return refuse("--probe-tail-depth needs --probe-depth R and --probe-tail-states needs --probe-classify\n");
            tail.on = true;
        } else if (!tail.on || !rays || !o.radiance_given || tail.depth || tail.states || tail.feedback_given || tail.bounces_given || tail.grid.empty() ||
                   tail.coefficients.empty() || !parse_probe_grid(tail.grid.c_str(), &o.tail_grid)) {  // --rays --radiance N
            return refuse("--probe-tail goes with --probe-grid, or with --rays --radiance N --probe-tail-grid G --probe-tail-coefficients FILE.f32 "
                          "[--probe-tail-normal-weight] (depth maps, records and --probe-feedback exist in the --probe-grid flow only)\n");
        }
    }
    if (grid_flow || !o.irradiance_out.empty() || o.probe_visibility || o.probe_normal_weight || o.probe_albedo || o.probe_hemisphere) {
        if (!grid_flow) return refuse("--irradiance-out, --probe-visibility, --probe-normal-weight, --probe-albedo and --probe-hemisphere need --probe-grid\n");
        if (!parse_probe_grid(o.probe_grid_arg.c_str(), &o.probe_grid))
            return refuse("--probe-grid wants OX,OY,OZ,SX,SY,SZ,NX,NY,NZ: a finite origin, finite spacings > 0, integer counts >= 1, at most 2^30 probes\n");
        if (o.irradiance_out.empty()) return refuse("--probe-grid needs --irradiance-out FILE\n");
        if (rays || probes || !o.probes_out.empty() || !o.probe_radiance_out.empty() || o.temporal || multi_device)
            return refuse(std::string("--probe-grid shades a frame from light probes: single device, not with ") +
                          (rays ? "--rays" : o.temporal ? "--temporal" : multi_device ? "--devices" : "--probes") + "\n");
        o.probe_grid_directions = o.probe_directions.find_first_not_of("0123456789") == std::string::npos ? std::atoi(o.probe_directions.c_str()) : 0;
        if (o.probe_directions.empty() || o.probe_grid_directions < 1 || o.probe_grid_directions > (int)SRT_LIGHT_PROBE_MAX_DIRECTIONS)
            return refuse("--probe-grid needs --probe-directions K with K in 1..4096\n");
        if ((o.radiance_given && (o.radiance < 1 || o.radiance > 4096)) || o.bounces < 0)
            return refuse("--probe-grid: --radiance N takes 1..4096 samples and --bounces must be >= 0\n");
        if (frame_outputs || frame_extras) return refuse("--probe-grid shades a frame from light probes instead of rendering it: no other frame options\n");
    }
    if (o.radiance_given && !probes && !grid_flow && (!rays || o.rays_any_hit || o.radiance < 1 || o.radiance > 4096 || o.bounces < 0))
        return refuse("--radiance N (1..4096) needs --rays and --rays-out, a --bounces >= 0, and does not go with --any-hit\n");
    if (probes || !o.probes_out.empty() || (!o.probe_directions.empty() && !grid_flow) || !o.probe_radiance_out.empty()) {
        if (!probes || o.probes_out.empty() || o.probe_directions.empty())
            return refuse("--probes, --probe-directions, --probes-out and --probe-radiance-out go together: --probes IN.f32 --probe-directions K|FILE.f32 "
                          "--probes-out OUT.bin [--radiance N] [--probe-radiance-out FILE]\n");
        if ((o.radiance_given && (o.radiance < 1 || o.radiance > 4096)) || o.bounces < 0)
            return refuse("--probes: --radiance N takes 1..4096 samples and --bounces must be >= 0\n");
        if (rays || multi_device || o.temporal || frame_outputs || frame_extras)
            return refuse("--probes traces light probes instead of rendering a frame: single device, not with --rays, no frame options\n");
    }
    // (--rays lets the extras through: the visibility and reflection rules below refuse theirs, --adaptive refuses --rays)
    if (rays && (multi_device || o.temporal || frame_outputs)) return refuse("--rays answers ray queries instead of rendering a frame: single device, no frame options\n");
    if ((o.ao_given || o.sun_visibility) == o.vis_out.empty() || (o.ao_given && (o.ao < 1 || o.ao > 4096)) || (!o.ao_given && o.ao_radius != INFINITY) ||
        !(o.ao_radius > 0) || (!o.vis_out.empty() && (multi_device || o.temporal || rays)))
        return refuse("--ao N (1..4096) [--ao-radius R > 0] and --sun-visibility need --vis-out FILE and the other way round; single device, "
                      "not with --temporal or --rays\n");
    if (o.reflection_guides || o.reflection_bounces_given || !o.reflection_out.empty()) {
        if ((o.reflection_guides && o.denoise.empty() && o.denoise_variance.empty()) || (o.reflection_bounces_given && !o.reflection_guides && o.reflection_out.empty()) ||
            o.reflection_bounces < 0 || o.reflection_bounces > 64 || multi_device || o.temporal || rays || o.adaptive_given)
            return refuse("--reflection-guides needs --denoise or --denoise-variance; --reflection-bounces N (0..64) needs --reflection-guides or "
                          "--reflection-out; single device, not with --devices, --temporal, --rays or --adaptive\n");
    }
    if ((o.mirror_history && !o.temporal) || (o.mirror_radius_given && (!o.mirror_history || !(o.mirror_radius > 0.0f))))
        return refuse("--mirror-history needs --temporal; --mirror-radius R (> 0) needs --mirror-history\n");
    if (o.temporal_variance && (!o.temporal || multi_device || o.steps > 1 || !o.upsample.empty()))
        return refuse("--temporal-variance needs --temporal and works on one device only, not with --steps or --upsample\n");
    if (!o.denoise.empty() && multi_device) return refuse("--denoise works on one device only: the accumulator bands of --devices live on different GPUs\n");
    if ((o.steps > 1 || !o.upsample.empty()) && (multi_device || o.temporal)) return refuse("--steps and --upsample work on one device only and not with --temporal\n");
    if (!o.denoise_variance.empty()) {
        if (!o.denoise.empty()) return refuse("--denoise-variance and --denoise exclude each other: both write the denoised buffer\n");
        if (o.spp < 2 || (o.spp & 1)) return refuse("--denoise-variance needs an even --spp >= 2: it renders two halves of --spp / 2 samples\n");
        if (multi_device || o.temporal || o.steps > 1 || !o.upsample.empty())
            return refuse("--denoise-variance works on one device only and not with --temporal, --steps or --upsample\n");
    }
    if (!o.adaptive_given && (o.adaptive_threshold_given || o.adaptive_max_given || !o.counts_out.empty()))
        return refuse("--adaptive-threshold, --adaptive-max and --counts-out need --adaptive ROUNDS\n");
    if (o.adaptive_given) {
        if (o.adaptive < 1 || o.adaptive > 64 || o.spp < 2 || (o.spp & 1) || o.bounces < 0 || (o.adaptive_threshold_given && !(o.adaptive_threshold > 0)) ||
            (o.adaptive_max_given && (o.adaptive_max < 1 || o.adaptive_max > 4096)))
            return refuse("--adaptive ROUNDS (1..64) needs an even --spp >= 2 and a --bounces >= 0; --adaptive-threshold T > 0; --adaptive-max M in 1..4096\n");
        // (--gbuffer is written after an adaptive frame, so the stages alone; the reflection rule above has refused its options)
        if (multi_device || o.temporal || frame_stages || rays || !o.vis_out.empty())
            return refuse("--adaptive renders the frame itself: single device, not with --devices, --temporal, --steps, --aa, --upsample, --denoise, "
                          "--denoise-variance, --rays, --ao or --sun-visibility\n");
    }
    if (o.aa_given && (o.aa < 1 || o.aa > 4 || multi_device)) return refuse("--aa takes K in 1..4 and works on one device only\n");
    if (o.temporal && multi_device) return refuse("--temporal works on one device only: the history of --devices would be split over different GPUs\n");
    return 0;
}

// The bytes of a file, checked: false after a message when the file cannot be opened or not all of it reaches the disk.
static bool write_file(const std::string& path, const void* data, size_t bytes) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) {
        std::perror(path.c_str());
        return false;
    }
    bool ok = std::fwrite(data, 1, bytes, f) == bytes;
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) std::fprintf(stderr, "%s: write failed\n", path.c_str());
    return ok;
}

static bool write_floats(const std::string& path, const std::vector<float>& v) { return write_file(path, v.data(), v.size() * sizeof(float)); }

// (unchecked, as it has always been: a full disk gives a short PPM and exit status 0)
static int write_ppm_file(const std::vector<uint32_t>& fb, int W, int H, const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) {
        std::perror(path.c_str());
        return 1;
    }
    std::fprintf(f, "P6\n%d %d\n255\n", W, H);
    for (uint32_t px : fb) {
        unsigned char rgb[3] = {(unsigned char)(px >> 16), (unsigned char)(px >> 8), (unsigned char)px};
        std::fwrite(rgb, 1, 3, f);
    }
    std::fclose(f);
    return 0;
}

// The framebuffer as it stands, read back and written as a PPM.
static int write_framebuffer(PathTraceRenderer& r, const Options& o, const std::string& path) {
    std::vector<uint32_t> fb((size_t)o.W * o.H);
    r.ReadFramebuffer(fb.data(), (size_t)o.W * 4);
    return write_ppm_file(fb, o.W, o.H, path);
}

// Every float32 of a file whose length is N >= 1 records of `record` floats: 0, or, with v empty, 1 after perror when the file
// cannot be opened and 2 after a message when it does not hold whole records.
static int read_float_records(const std::string& path, size_t record, std::vector<float>& v) {
    v.clear();
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) {
        std::perror(path.c_str());
        return 1;
    }
    float buf[2048];
    for (size_t got; (got = std::fread(buf, sizeof(float), 2048, f)) > 0;) v.insert(v.end(), buf, buf + got);
    std::fclose(f);
    if (v.empty() || v.size() % record) {
        std::fprintf(stderr, "%s: %zu floats: want N >= 1 records of %zu float32\n", path.c_str(), v.size(), record);
        v.clear();
        return 2;
    }
    return 0;
}

// One H x W (x channels) plane as a NumPy .npy file (format 1.0: magic, version, little-endian header length, a Python-literal header
// padded with spaces to a multiple of 64 bytes and ended by a newline, then the raw C-order data), rows top-down (memory rows, as the
// PPM): memory row m = scene row H - 1 - m of `scene_rows`.  (Little-endian hosts: the descriptors say '<'.)
static bool write_npy(const std::string& path, const char* descr, int H, int W, int channels, const std::vector<char>& scene_rows) {
    char shape[64];
    if (channels == 1) std::snprintf(shape, sizeof shape, "(%d, %d)", H, W);
    else std::snprintf(shape, sizeof shape, "(%d, %d, %d)", H, W, channels);
    std::string bytes = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': " + shape + ", }";
    const size_t pre = 10;  // magic (6) + version (2) + header length (2)
    while ((pre + bytes.size() + 1) % 64) bytes += ' ';
    bytes += '\n';
    const char head[10] = {(char)0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0, (char)(bytes.size() & 255), (char)(bytes.size() >> 8)};
    bytes.insert(0, head, sizeof head);
    const size_t row_bytes = scene_rows.size() / (size_t)H;
    for (int m = 0; m < H; ++m) bytes.append(scene_rows.data() + (size_t)(H - 1 - m) * row_bytes, row_bytes);
    return write_file(path, bytes.data(), bytes.size());
}

// The planes that --gbuffer PREFIX (the first four: the first-hit buffers) and --reflection-out PREFIX (all five: the outputs of the
// reflection guides, whose first four bits are the G-buffer's) write as PREFIX_name.npy; `read` copies the plane of a bit.
struct Plane {
    uint32_t bit;
    const char* name;
    const char* descr;
    int channels;
};
static const Plane kPlanes[5] = {{SRT_GBUF_OBJECT, "object", "<i4", 1}, {SRT_GBUF_NORMAL_DEPTH, "normal_depth", "<f4", 4}, {SRT_GBUF_POSITION, "position", "<f4", 4},
                                 {SRT_GBUF_ALBEDO, "albedo", "<f4", 4}, {SRT_REFL_BOUNCES, "bounces", "<i4", 1}};
static_assert(SRT_REFL_OBJECT == SRT_GBUF_OBJECT && SRT_REFL_NORMAL_DEPTH == SRT_GBUF_NORMAL_DEPTH && SRT_REFL_POSITION == SRT_GBUF_POSITION &&
                  SRT_REFL_ALBEDO == SRT_GBUF_ALBEDO, "one plane table serves both");

template <class Read>
static int write_planes(const std::string& prefix, const Options& o, size_t count, Read read) {
    for (size_t i = 0; i < count; ++i) {
        const Plane& p = kPlanes[i];
        std::vector<char> buf((size_t)o.W * 4 * (size_t)p.channels * (size_t)o.H);
        read(p.bit, buf.data());
        if (!write_npy(prefix + "_" + p.name + ".npy", p.descr, o.H, o.W, p.channels, buf)) return 1;
    }
    return 0;
}

// --gbuffer PREFIX, when given (with --devices: made for the whole frame on the first device)
template <class R>
static int write_gbuffers(R& r, const Options& o) {
    if (o.gbuffer.empty()) return 0;
    r.RenderGBuffer(SRT_GBUF_ALL);
    return write_planes(o.gbuffer, o, 4, [&](uint32_t bit, void* dst) { r.ReadGBuffer(bit, dst); });
}

// --reflection-out PREFIX: srt_render_reflection_gbuffer with the library's thresholds and --reflection-bounces reflections at most
static int write_reflection(PathTraceRenderer& r, const Options& o) {
    srt_reflection_params rp{};
    srt_reflection_params_default(&rp);
    rp.row_begin = 0, rp.row_end = o.H, rp.max_bounces = o.reflection_bounces;
    r.renderReflectionGBuffer(rp);
    return write_planes(o.reflection_out, o, 5, [&](uint32_t bit, void* dst) { r.readReflection(bit, dst); });
}

// --rays IN.f32 --rays-out OUT.bin: closest-hit queries for the rays of a file (N records of 8 float32: origin xyzw, direction
// xyz + t_max) against the scene; the five outputs of srt_trace_rays follow each other in OUT.bin in the order of their bits.
// With --any-hit the rays go through srt_trace_occlusion instead and OUT.bin receives the occluded array (N int32) alone.
// With --radiance N they go through srt_trace_radiance — samples 1..N, --bounces, --seed, id_base 0 — and OUT.bin receives the N
// float4 running means alone; with --probe-tail (--probe-tail-grid's grid, the P x 9 float4 coefficients of
// --probe-tail-coefficients and SRT_PROBE_TAIL_* flags) that trace runs under srt_probe_tail.
static int trace_ray_file(const Options& o, const Scene& scene) {
    const ProbeTailOptions& tail = o.probe_tail;
    std::vector<float> coefficients, rec;
    if (tail.on) {
        read_float_records(tail.coefficients, 4, coefficients);
        const size_t np = (size_t)o.tail_grid.counts[0] * (size_t)o.tail_grid.counts[1] * (size_t)o.tail_grid.counts[2];
        if (coefficients.size() != np * 36) {
            std::fprintf(stderr, "--probe-tail-coefficients: want %zu probes x 9 float4 for the grid of --probe-tail-grid\n", np);
            return 2;
        }
    }
    if (int e = read_float_records(o.rays_in, 8, rec)) return e;
    const size_t n = rec.size() / 8;
    std::vector<float> org(4 * n), d(4 * n);
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(&org[4 * i], &rec[8 * i], 4 * sizeof(float));
        std::memcpy(&d[4 * i], &rec[8 * i + 4], 4 * sizeof(float));
    }
    const bool normalize = o.rays_normalize, any_hit = o.rays_any_hit;
    PathTraceRenderer r(o.device, 8, 8);  // (the frame size plays no part in a ray query)
    r.SetScene(scene);
    if (o.radiance_given) {
        srt_radiance_params rp{};
        srt_radiance_params_default(&rp);
        rp.sample_count = (uint32_t)o.radiance, rp.max_bounces = o.bounces, rp.seed = o.seed;
        if (normalize) rp.flags |= SRT_RADIANCE_NORMALIZE;
        if (tail.on) {
            r.setProbeGrid(o.tail_grid);
            r.writeProbeGridInputs(coefficients.data(), nullptr, nullptr, coefficients.size() / 36, 0);
            srt_probe_tail_params tp{};
            srt_probe_tail_params_default(&tp);
            tp.flags = tail.flags();
            r.probeTail(tp);
        }
        r.traceRadiance(org.data(), d.data(), n, rp);
        std::vector<float> rad(4 * n);
        r.readRadiance(rad.data());
        if (!write_floats(o.rays_out, rad)) return 1;
        std::fprintf(stderr, "%zu rays, %d samples of radiance each%s: %s\n", n, o.radiance, normalize ? " (directions normalized)" : "", o.rays_out.c_str());
        return 0;
    }
    if (any_hit) r.traceOcclusion(org.data(), d.data(), n, normalize ? SRT_OCCLUSION_NORMALIZE : 0u);
    else r.traceRays(org.data(), d.data(), n, SRT_GBUF_ALL | SRT_RAYS_OCCLUDED, normalize ? SRT_RAYS_NORMALIZE : 0u);
    std::vector<char> data;
    for (uint32_t bit = any_hit ? SRT_RAYS_OCCLUDED : 1u; bit <= SRT_RAYS_OCCLUDED; bit <<= 1) {
        const size_t at = data.size();
        data.resize(at + n * ((bit == SRT_GBUF_OBJECT || bit == SRT_RAYS_OCCLUDED) ? sizeof(int32_t) : 4 * sizeof(float)));
        r.readRayOutput(bit, data.data() + at);
    }
    if (!write_file(o.rays_out, data.data(), data.size())) return 1;
    std::fprintf(stderr, "%zu rays traced%s%s: %s\n", n, any_hit ? " (any hit)" : "", normalize ? " (directions normalized)" : "", o.rays_out.c_str());
    return 0;
}

// --probes IN.f32 --probe-directions K|FILE.f32 --probes-out OUT.bin: light probes (srt_trace_light_probes) at the positions of a
// file (P records of 4 float32: xyz, w ignored) over K spherical Fibonacci directions (srt_light_probe_sphere) or the directions
// of a file (K records of 4 float32: xyz, weight) — samples 1..--radiance N, --bounces, --seed, id_base 0.  OUT.bin receives the P*9
// float4 coefficients; --probe-radiance-out, when given, the P*K float4 running means.
static int trace_probe_file(const Options& o, const Scene& scene) {
    const std::string& dirs = o.probe_directions;
    std::vector<float> pos, dir;
    if (read_float_records(o.probes_in, 4, pos)) return 2;
    if (dirs.find_first_not_of("0123456789") == std::string::npos) {
        const long k = std::atol(dirs.c_str());
        if (k < 1 || k > (long)SRT_LIGHT_PROBE_MAX_DIRECTIONS) {
            std::fprintf(stderr, "--probe-directions %s: want a count 1..4096 or a file\n", dirs.c_str());
            return 2;
        }
        dir.resize(4 * (size_t)k);
        srt_light_probe_sphere((size_t)k, dir.data());
    } else if (read_float_records(dirs, 4, dir) || dir.size() / 4 > SRT_LIGHT_PROBE_MAX_DIRECTIONS) {
        std::fprintf(stderr, "--probe-directions %s: want 1..4096 records of 4 float32\n", dirs.c_str());
        return 2;
    }
    const size_t np = pos.size() / 4, nk = dir.size() / 4;
    PathTraceRenderer r(o.device, 8, 8);  // (the frame size plays no part in a probe trace)
    r.SetScene(scene);
    srt_light_probe_params lp{};
    srt_light_probe_params_default(&lp);
    lp.sample_count = (uint32_t)o.probe_samples(), lp.max_bounces = o.bounces, lp.seed = o.seed;
    if (!o.probe_radiance_out.empty()) lp.outputs |= SRT_LIGHT_PROBE_RADIANCE;
    r.traceLightProbes(pos.data(), np, dir.data(), nk, lp);
    std::vector<float> coeff(np * 9 * 4);
    r.readLightProbeOutput(SRT_LIGHT_PROBE_COEFFICIENTS, coeff.data());
    if (!write_floats(o.probes_out, coeff)) return 1;
    if (!o.probe_radiance_out.empty()) {
        std::vector<float> rad(np * nk * 4);
        r.readLightProbeOutput(SRT_LIGHT_PROBE_RADIANCE, rad.data());
        if (!write_floats(o.probe_radiance_out, rad)) return 1;
    }
    std::fprintf(stderr, "%zu probes x %zu directions, %d samples each: %s\n", np, nk, o.probe_samples(), o.probes_out.c_str());
    return 0;
}

// What the two --probe-grid flows share: the renderer with the frame's settings and the scene, the K directions, the probes'
// arrays (positions, coefficients, R*R moments, records), and the parameter blocks of the light-probe, classify and depth calls
// as the options fill them.
struct ProbeFlow {
    PathTraceRenderer r;
    const size_t np, nk;
    const uint32_t resolution;  // --probe-depth R, or 0
    std::vector<float> pos, dir, coeff, moments, states;
    srt_light_probe_params lp{};
    srt_probe_classify_params cp{};
    srt_probe_depth_params dp{};

    ProbeFlow(const Options& o, const Scene& scene, std::vector<float> positions)
        : r(o.device, o.W, o.H), np(positions.size() / 4), nk((size_t)o.probe_grid_directions), resolution((uint32_t)o.probe_depth.resolution),
          pos(std::move(positions)), dir(4 * nk), coeff(np * 9 * 4), moments(np * (size_t)resolution * resolution * 4), states(o.probe_classify.on ? 4 * np : 0) {
        srt_light_probe_sphere(nk, dir.data());
        r.FOV = o.fov;
        r.MAXBOUNCES = o.bounces;
        r.seed = o.seed;
        r.SetScene(scene);
        srt_light_probe_params_default(&lp);
        lp.sample_count = (uint32_t)o.probe_samples(), lp.max_bounces = o.bounces, lp.seed = o.seed;
        const ProbeClassifyOptions& classify = o.probe_classify;
        srt_probe_classify_params_default(&cp);
        cp.clearance = classify.clearance, cp.max_offset = classify.max_offset, cp.steps = (uint32_t)classify.steps;
        cp.flags = classify.relocate ? SRT_PROBE_CLASSIFY_RELOCATE : 0u;
        cp.outputs = SRT_PROBE_STATE_RECORDS | SRT_PROBE_STATE_POSITIONS;
        srt_probe_depth_params_default(&dp);
        if (resolution) dp.resolution = resolution, dp.sharpness = (uint32_t)o.probe_depth.sharpness, dp.max_distance = o.probe_depth.max_distance;
    }
    void classify() {  // the records, and the positions the probes are traced at
        r.classifyProbes(dir.data(), nk, cp);
        r.readProbeStatesOutput(SRT_PROBE_STATE_RECORDS, states.data());
        r.readProbeStatesOutput(SRT_PROBE_STATE_POSITIONS, pos.data());
    }
    void trace_depth() {  // the depth maps at the positions, and their moments
        r.traceProbeDepth(pos.data(), np, dir.data(), nk, dp);
        r.readProbeDepthOutput(SRT_PROBE_DEPTH_MOMENTS, moments.data());
    }
    void write_grid_inputs(bool with_moments, bool with_states) {  // the coefficients, and what the flags ask for, into the grid's arrays
        r.writeProbeGridInputs(coeff.data(), with_moments ? moments.data() : nullptr, with_states ? states.data() : nullptr, np, resolution);
    }
};

static void hemisphere_band_weights(float* w) { w[0] = 1.0f, w[1] = 0.5f, w[2] = 0.0f; }  // --probe-hemisphere

// --probe-update FRAMES: the listed traces and blends of the frames; the histories end in f.coeff and f.moments.
static int update_probe_frames(ProbeFlow& f, const Options& o, Scene& scene) {
    PathTraceRenderer& r = f.r;
    const ProbeUpdateOptions& update = o.probe_update;
    srt_probe_list_params ls{};
    srt_probe_list_params_default(&ls);
    r.listProbes(f.states.data(), f.np, ls);
    r.resetProbeHistory(SRT_PROBE_HISTORY_COEFFICIENTS | (f.resolution ? SRT_PROBE_HISTORY_MOMENTS : 0u), f.np, f.resolution);
    srt_probe_blend_params bp{};
    srt_probe_blend_params_default(&bp);
    bp.hysteresis = bp.depth_hysteresis = update.hysteresis;
    if (bp.fast_hysteresis > update.hysteresis) bp.fast_hysteresis = update.hysteresis;
    bp.flags = SRT_PROBE_BLEND_LISTED | (f.resolution ? SRT_PROBE_BLEND_MOMENTS : 0u);
    f.lp.sample_count = (uint32_t)update.samples;
    std::vector<float> previous;
    for (int k = 1; k <= update.frames; ++k) {
        const bool moved = k > 1 && !o.object_moves.empty();
        if (moved) {  // the objects move; the classification and the list follow, the records of the frame before are kept
            for (const auto& m : o.object_moves) {
                float* p = scene.Objects()[m.index].position;
                for (int a = 0; a < 3; ++a) p[a] = p[a] + m.step[a];
            }
            r.UpdateScene(scene);
            previous = f.states;
            f.classify();
            r.listProbes(f.states.data(), f.np, ls);
        }
        f.lp.seed = (uint32_t)k;
        r.traceLightProbesListed(k == 1 || moved ? f.pos.data() : nullptr, f.np, k == 1 ? f.dir.data() : nullptr, f.nk, f.lp);
        if (f.resolution) r.traceProbeDepthListed(nullptr, f.np, nullptr, f.nk, f.dp);
        srt_probe_blend_params b = bp;
        if (moved) b.flags |= SRT_PROBE_BLEND_PREVIOUS_STATES | SRT_PROBE_BLEND_COUNT_WORK;
        r.blendProbes(moved ? previous.data() : nullptr, f.np, b);
        if (moved) {
            const srt_probe_blend_work w = r.probeBlendWork();
            std::fprintf(stderr, "probe update frame %d: %llu probes blended, %llu restarted, %llu changed\n", k, (unsigned long long)w.probes,
                         (unsigned long long)w.restarted, (unsigned long long)w.changed);
        }
    }
    const std::string& states_out = o.probe_classify.out;
    if (!states_out.empty() && o.object_moves.size() && !write_floats(states_out, f.states)) return 1;  // (the records of the last frame)
    r.readProbeHistory(SRT_PROBE_HISTORY_COEFFICIENTS, f.coeff.data());
    if (f.resolution) r.readProbeHistory(SRT_PROBE_HISTORY_MOMENTS, f.moments.data());
    return 0;
}

// --probe-tail with --probe-grid: the feedback rounds, --probe-scroll's move of `grid` and --probe-tail-frame's picture; the
// coefficient history ends in f.coeff.
static int feedback_probe_rounds(ProbeFlow& f, const Options& o, srt_probe_grid& grid) {
    PathTraceRenderer& r = f.r;
    const ProbeTailOptions& tail = o.probe_tail;
    r.setProbeGrid(grid);
    if (f.resolution) f.trace_depth();  // the maps the tail reads under --probe-tail-depth, and the shading after the last round
    r.resetProbeHistory(SRT_PROBE_HISTORY_COEFFICIENTS, f.np, 0);
    srt_probe_blend_params bp{};
    srt_probe_blend_params_default(&bp);
    srt_probe_tail_params tp{};
    srt_probe_tail_params_default(&tp);
    tp.flags = tail.flags() | SRT_PROBE_TAIL_COUNT_WORK;
    if (tail.bounces >= 0) f.lp.max_bounces = tail.bounces;
    for (int k = 1; k <= tail.feedback; ++k) {
        tp.enabled = k > 1 ? 1 : 0;  // round 1 has no history
        if (k > 1) {
            r.readProbeHistory(SRT_PROBE_HISTORY_COEFFICIENTS, f.coeff.data());
            f.write_grid_inputs(tail.depth, tail.states);
        }
        r.probeTail(tp);
        f.lp.seed = (uint32_t)k;
        r.traceLightProbes(f.pos.data(), f.np, f.dir.data(), f.nk, f.lp);
        r.blendProbes(nullptr, f.np, bp);
        if (k > 1) {
            const srt_probe_tail_work w = r.probeTailWork();
            std::fprintf(stderr, "probe feedback round %d: %llu lookups, %llu dark, %llu mirror ends\n", k, (unsigned long long)w.tails,
                         (unsigned long long)w.dark, (unsigned long long)w.mirror_ends);
        }
        if (tail.scroll_on && k == tail.scroll_after) {  // the grid moves; what is made per grid is made again
            r.scrollProbes(tail.scroll, SRT_PROBE_SCROLL_COEFFICIENTS, SRT_PROBE_SCROLL_SET_GRID | SRT_PROBE_SCROLL_COUNT_WORK);
            grid = r.probeGrid();
            srt_probe_grid_positions(&grid, f.pos.data());
            if (o.probe_classify.on) f.classify();
            if (f.resolution) f.trace_depth();
            const srt_probe_scroll_work w = r.probeScrollWork();
            std::fprintf(stderr, "probe scroll after round %d by %d,%d,%d: %llu probes, %llu retained, %llu exposed\n", k, tail.scroll[0], tail.scroll[1],
                         tail.scroll[2], (unsigned long long)w.probes, (unsigned long long)w.retained, (unsigned long long)w.exposed);
        }
    }
    r.readProbeHistory(SRT_PROBE_HISTORY_COEFFICIENTS, f.coeff.data());
    if (tail.frame) {  // the picture: every path of the frame ends in the history the rounds have left
        f.write_grid_inputs(tail.depth, tail.states);
        tp.enabled = 1;
        r.probeTail(tp);
        r.renderProbeTailFrame((uint32_t)tail.frame_spp, o.bounces, o.seed);
        std::vector<uint32_t> fb((size_t)o.W * o.H);
        r.ReadFramebuffer(fb.data(), (size_t)o.W * 4);
        const srt_probe_tail_work w = r.probeTailWork();
        std::fprintf(stderr, "probe tail frame: %d samples per pixel at %d bounces, %llu lookups, %llu dark, %llu mirror ends: %s\n", tail.frame_spp, o.bounces,
                     (unsigned long long)w.tails, (unsigned long long)w.dark, (unsigned long long)w.mirror_ends, tail.frame_out.c_str());
        if (write_ppm_file(fb, o.W, o.H, tail.frame_out)) return 1;
    }
    tp.enabled = 0;
    r.probeTail(tp);
    return 0;
}

// --probe-grid G --probe-directions K --irradiance-out FILE (the structs at the top say what each group of options adds): the
// classification, then the coefficients by one trace, by --probe-update's frames or by --probe-tail's rounds, then the shading call
// that the depth maps and records ask for.
static int shade_probe_grid_file(const Options& o, Scene& scene) {
    srt_probe_grid grid = o.probe_grid;  // (--probe-scroll moves it)
    const ProbeDepthOptions& depth = o.probe_depth;
    const ProbeClassifyOptions& classify = o.probe_classify;
    const bool moves = !o.object_moves.empty();
    std::vector<float> pos(4 * (size_t)grid.counts[0] * (size_t)grid.counts[1] * (size_t)grid.counts[2]);
    if (srt_probe_grid_positions(&grid, pos.data()) != SRT_OK) {
        std::fprintf(stderr, "--probe-grid: want finite origins, finite spacings > 0, counts >= 1 and at most 2^30 probes\n");
        return 2;
    }
    ProbeFlow f(o, scene, std::move(pos));
    PathTraceRenderer& r = f.r;
    if (classify.on) {  // the states first: the probes are traced where the classification puts them
        r.setProbeGrid(grid);
        f.classify();
        if (!classify.out.empty() && !moves && !write_floats(classify.out, f.states)) return 1;
    }
    const bool one_trace = !o.probe_update.frames && !o.probe_tail.feedback;
    if (o.probe_update.frames) {  // (classify.on: validate() has seen to it)
        if (update_probe_frames(f, o, scene)) return 1;
    } else if (o.probe_tail.feedback) {
        if (feedback_probe_rounds(f, o, grid)) return 1;
    } else {
        r.traceLightProbes(f.pos.data(), f.np, f.dir.data(), f.nk, f.lp);
        r.readLightProbeOutput(SRT_LIGHT_PROBE_COEFFICIENTS, f.coeff.data());
    }
    srt_probe_grid_params sp{};
    srt_probe_grid_params_default(&sp);
    const uint32_t flags = (o.probe_visibility ? SRT_PROBE_GRID_VISIBILITY : 0u) | (o.probe_normal_weight ? SRT_PROBE_GRID_NORMAL_WEIGHT : 0u) |
                           (o.probe_albedo ? SRT_PROBE_GRID_ALBEDO : 0u);
    sp.row_begin = 0, sp.row_end = o.H, sp.flags = flags;
    if (o.probe_hemisphere) hemisphere_band_weights(sp.band_weight);
    r.setProbeGrid(grid);
    if (f.resolution) {
        if (one_trace) f.trace_depth();  // (the frames have blended their maps, the rounds traced theirs up front)
        if (!depth.out.empty() && !write_floats(depth.out, f.moments)) return 1;
        srt_probe_grid_depth_params gd{};
        srt_probe_grid_depth_params_default(&gd);
        gd.bias = depth.bias;
        if (classify.on) r.shadeProbeGridStates(f.coeff.data(), f.moments.data(), f.states.data(), f.np, f.resolution, sp, &gd);
        else r.shadeProbeGridDepth(f.coeff.data(), f.moments.data(), f.np, f.resolution, sp, gd);
    } else if (classify.on) {
        r.shadeProbeGridStates(f.coeff.data(), nullptr, f.states.data(), f.np, 0, sp, nullptr);
    } else {
        r.shadeProbeGrid(f.coeff.data(), f.np, sp);
    }
    std::vector<float> img((size_t)o.W * o.H * 4);
    r.readProbeGridOutput(img.data());
    if (!write_floats(o.irradiance_out, img)) return 1;
    std::fprintf(stderr, "%dx%d: %zu probes x %d directions, %d samples each, flags 0x%x%s: %s\n", o.W, o.H, f.np, o.probe_grid_directions, o.probe_samples(), flags,
                 o.probe_hemisphere ? " (hemisphere band weights)" : "", o.irradiance_out.c_str());
    return 0;
}

// --probe-grid G --probe-directions K --probe-cascade L [--probe-cascade-blend B] --irradiance-out FILE: the frame shaded from L
// nested grids (srt_shade_probe_cascade).  The levels come from srt_probe_cascade_grids around the camera position, with G's
// spacing as the finest spacing and G's counts (G's origin is not read); per level the route of --probe-grid runs on the level's
// grid through the single-grid calls — the classification (--probe-classify), the probes traced at the positions it gives, the
// depth maps (--probe-depth R) — and PathTraceRenderer::captureProbeCascadeLevel keeps its results; then the cascade shading runs
// in place of the single-grid call.  FILE receives W*H float4, scene rows.
static int shade_probe_cascade_file(const Options& o, const Scene& scene) {
    const srt_probe_grid& finest = o.probe_grid;
    const int levels = o.probe_cascade_levels;
    const bool classify = o.probe_classify.on;
    ProbeFlow f(o, scene, std::vector<float>(4 * (size_t)finest.counts[0] * (size_t)finest.counts[1] * (size_t)finest.counts[2]));
    PathTraceRenderer& r = f.r;
    const float centre[3] = {r.camera.position.x, r.camera.position.y, r.camera.position.z};
    srt_probe_cascade cascade{};
    if (srt_probe_cascade_grids(centre, finest.spacing, finest.counts, (uint32_t)levels, &cascade) != SRT_OK) {
        std::fprintf(stderr, "--probe-cascade: the levels' spacings must stay finite and the probes of a level at most 2^30\n");
        return 2;
    }
    cascade.resolution = f.resolution, cascade.blend_cells = o.probe_cascade_blend;
    r.setProbeCascade(cascade);
    for (int l = 0; l < levels; ++l) {
        const srt_probe_grid& g = cascade.grid[l];
        r.setProbeGrid(g);
        srt_probe_grid_positions(&g, f.pos.data());
        if (classify) f.classify();  // the states first: the probes are traced where the classification puts them
        r.traceLightProbes(f.pos.data(), f.np, f.dir.data(), f.nk, f.lp);
        r.readLightProbeOutput(SRT_LIGHT_PROBE_COEFFICIENTS, f.coeff.data());
        if (f.resolution) f.trace_depth();
        f.write_grid_inputs(f.resolution != 0, classify);
        r.captureProbeCascadeLevel((uint32_t)l, SRT_PROBE_CASCADE_COEFFICIENTS | (f.resolution ? SRT_PROBE_CASCADE_MOMENTS : 0u) | (classify ? SRT_PROBE_CASCADE_RECORDS : 0u));
        std::fprintf(stderr, "probe cascade level %d: origin %g %g %g, spacing %g %g %g\n", l, (double)g.origin[0], (double)g.origin[1], (double)g.origin[2],
                     (double)g.spacing[0], (double)g.spacing[1], (double)g.spacing[2]);
    }
    srt_probe_cascade_params sp{};
    srt_probe_cascade_params_default(&sp);
    sp.row_begin = 0, sp.row_end = o.H;
    sp.flags = (o.probe_normal_weight ? SRT_PROBE_CASCADE_NORMAL_WEIGHT : 0u) | (o.probe_albedo ? SRT_PROBE_CASCADE_ALBEDO : 0u) |
               (f.resolution ? SRT_PROBE_CASCADE_DEPTH : 0u) | (classify ? SRT_PROBE_CASCADE_STATES : 0u) | SRT_PROBE_CASCADE_COUNT_WORK;
    sp.bias = o.probe_depth.bias;
    if (o.probe_hemisphere) hemisphere_band_weights(sp.band_weight);
    r.shadeProbeCascade(sp);
    std::vector<float> img((size_t)o.W * o.H * 4);
    r.readProbeGridOutput(img.data());
    if (!write_floats(o.irradiance_out, img)) return 1;
    const srt_probe_cascade_work w = r.probeCascadeWork();
    std::fprintf(stderr, "%dx%d: %d levels of %zu probes x %d directions, %d samples each, flags 0x%x%s: %llu hit pixels, %llu blended, first level %llu %llu %llu %llu: %s\n",
                 o.W, o.H, levels, f.np, o.probe_grid_directions, o.probe_samples(), sp.flags, o.probe_hemisphere ? " (hemisphere band weights)" : "",
                 (unsigned long long)w.pixels, (unsigned long long)w.blended, (unsigned long long)w.first_level[0], (unsigned long long)w.first_level[1],
                 (unsigned long long)w.first_level[2], (unsigned long long)w.first_level[3], o.irradiance_out.c_str());
    return 0;
}

static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3; }

// --devices: one frame over several GPUs in one process
static int render_multi_device(const Options& o, const Scene& scene) {
    MultiGpuRenderer m(o.devices, o.W, o.H);
    m.SetScene(scene);
    m.Configure(Transform(), o.fov, o.bounces, o.seed);
    if (o.equal_bands) m.UseEqualBands(true);
    auto t0 = std::chrono::steady_clock::now();
    m.RenderSamples((uint32_t)o.spp, true);
    std::vector<uint32_t> fb((size_t)o.W * o.H);
    m.ReadFramebuffer(fb.data(), (size_t)o.W * 4);
    const double wall_ms = ms_since(t0);
    std::vector<srt_stats> st = m.Stats();
    double slowest = 0;
    for (size_t i = 0; i < st.size(); ++i) {
        int b, e;
        m.Band(i, &b, &e);
        std::fprintf(stderr, "  part %zu (device %d, memory rows %d-%d): kernel %.3f ms, %.2f rays/sample\n", i, o.devices[i], b, e, st[i].kernel_ms,
                     (double)st[i].rays / (double)st[i].path_samples);
        slowest = st[i].kernel_ms > slowest ? st[i].kernel_ms : slowest;
    }
    std::fprintf(stderr, "%dx%d spp=%d bounces=%d over %zu parts: slowest kernel %.3f ms, render + gather + read-back wall %.3f ms\n", o.W, o.H, o.spp, o.bounces,
                 st.size(), slowest, wall_ms);
    if (write_ppm_file(fb, o.W, o.H, o.out)) return 1;
    return write_gbuffers(m, o);
}

// The single-device renderer of the three frame modes, with the frame's settings and the scene.
struct FrameRenderer : PathTraceRenderer {
    FrameRenderer(const Options& o, const Scene& scene) : PathTraceRenderer(o.device, o.W, o.H) {
        FOV = o.fov;
        MAXBOUNCES = o.bounces;
        seed = o.seed;
        refitUpdates = o.refit;
        SetScene(scene);
    }
};

// --aa: the stage's result resolved into the framebuffer before it is read (the sub-samples are traced once per camera)
static void resolve(PathTraceRenderer& r, const Options& o, int source) {
    if (o.aa) r.Antialias(o.aa, source, SRT_AA_FRAMEBUFFER);
}

// --temporal FRAMES: a moving camera that keeps its samples: every frame renders --spp samples, reprojects the history and writes
// the framebuffer; each frame's camera is printed exactly (%.9g round-trips a float) so that callers can replay it
static int render_temporal(const Options& o, Scene& scene) {
    FrameRenderer r(o, scene);
    r.antialias = o.aa;  // every temporal frame ends in the resolve
    r.temporalVariance = o.temporal_variance;  // every temporal frame keeps the moments
    if (o.mirror_history) {  // every temporal frame reprojects through the mirrors
        if (o.mirror_radius_given) r.mirrorRadius = o.mirror_radius;
        r.mirrorHistory(true);
    }
    const Vec3 world_up(0, 1, 0);
    const float turn = (float)(o.turn_deg * 3.14159265358979323846 / 180.0);
    auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < o.temporal; ++k) {
        if (k > 0) {
            Transform& c = r.camera;
            c.position = c.position + c.right * o.move[0] + c.up * o.move[1] + c.forward * o.move[2];
            if (turn != 0) c.RotateAboutAxis(turn, world_up);
            // object edits: each moved object's position is printed exactly, like the camera
            for (const auto& m : o.object_moves) {
                float* pos = scene.Objects()[m.index].position;
                for (int a = 0; a < 3; ++a) pos[a] = pos[a] + m.step[a];
            }
            if (!o.object_moves.empty()) r.UpdateScene(scene);
            if (o.refit) {
                const srt_update_info u = r.UpdateInfo();
                std::fprintf(stderr, "temporal frame %d update path %d reason %d levels %d triangles %u nodes %u\n", k, u.path, u.reason, u.levels, u.triangles, u.nodes);
            }
        }
        for (const auto& m : o.object_moves) {
            const float* pos = scene.GetObjects()[m.index].position;
            std::fprintf(stderr, "temporal frame %d object %zu position %.9g %.9g %.9g\n", k, m.index, pos[0], pos[1], pos[2]);
        }
        const Transform& c = r.camera;
        std::fprintf(stderr, "temporal frame %d camera %.9g %.9g %.9g  %.9g %.9g %.9g  %.9g %.9g %.9g  %.9g %.9g %.9g\n", k, c.position.x, c.position.y, c.position.z,
                     c.right.x, c.right.y, c.right.z, c.up.x, c.up.y, c.up.z, c.forward.x, c.forward.y, c.forward.z);
        r.RenderTemporalFrame((uint32_t)o.spp, false);
    }
    r.Wait();
    std::fprintf(stderr, "%dx%d spp=%d bounces=%d: %d temporal frames, wall %.3f ms\n", o.W, o.H, o.spp, o.bounces, o.temporal, ms_since(t0));
    if (write_framebuffer(r, o, o.out) || write_gbuffers(r, o)) return 1;
    if (!o.denoise.empty()) {
        // the last frame's accumulator (the reprojected result) through the denoiser, as RenderTemporalFrame(spp, true) does
        srt_denoise_params dp{};
        srt_denoise_params_default(&dp);
        dp.flags |= SRT_DENOISE_FRAMEBUFFER;
        r.RenderGBuffer(SRT_GBUF_ALL);
        // --temporal-variance: the variance of the history's moments and the variance-guided filter in its place
        if (o.temporal_variance) r.DenoiseTemporalVariance(SRT_DENOISE_FRAMEBUFFER);
        else r.Denoise(dp);
        resolve(r, o, SRT_AA_SOURCE_DENOISED);
        if (write_framebuffer(r, o, o.denoise)) return 1;
    }
    return 0;
}

// --adaptive ROUNDS: the uniform seed in two halves, the rounds, the merge (PathTraceRenderer::renderAdaptiveFrame); --out is the
// merged accumulator through SetScreenPixel's tone map (memory row H - 1 - y), which no kernel has written for the mean
static int render_adaptive(const Options& o, const Scene& scene) {
    FrameRenderer r(o, scene);
    const int W = o.W, H = o.H;
    srt_budget_params bp{};
    srt_budget_params_default(&bp);
    if (o.adaptive_threshold_given) bp.threshold = o.adaptive_threshold;
    if (o.adaptive_max_given) bp.max_budget = (uint32_t)o.adaptive_max;
    std::vector<uint32_t> counts;
    auto t0 = std::chrono::steady_clock::now();
    const uint64_t total = r.renderAdaptiveFrame((uint32_t)o.spp, o.adaptive, bp, bp.max_budget, &counts);
    const double wall_ms = ms_since(t0);
    std::fprintf(stderr, "%dx%d spp=%d bounces=%d adaptive rounds=%d threshold=%g max=%u: total samples %llu (%.2f per pixel), wall %.3f ms\n", W, H, o.spp, o.bounces,
                 o.adaptive, (double)bp.threshold, bp.max_budget, (unsigned long long)total, (double)total / ((double)W * H), wall_ms);
    const std::vector<float> acc = r.ReadAccumulator();
    std::vector<uint32_t> fb((size_t)W * H);
    auto channel = [](float v) {
        const float s = v / (1.0f + v) * 255;
        return (uint32_t)(s != s || s < 0 ? 0 : s > 255 ? 255 : (int)s);
    };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float* c = &acc[4 * ((size_t)y * W + x)];
            fb[(size_t)(H - 1 - y) * W + x] = 0xFF000000u | channel(c[0]) << 16 | channel(c[1]) << 8 | channel(c[2]);
        }
    if (write_ppm_file(fb, W, H, o.out) || write_gbuffers(r, o)) return 1;
    if (!o.counts_out.empty() && !write_file(o.counts_out, counts.data(), counts.size() * sizeof(uint32_t))) return 1;
    return 0;
}

// The plain frame, then the passes that were asked for, each writing its own file.
static int render_frame(const Options& o, const Scene& scene) {
    FrameRenderer r(o, scene);
    auto t0 = std::chrono::steady_clock::now();
    r.RenderSamples((uint32_t)o.spp, true, o.steps);
    r.Wait();
    const double wall_ms = ms_since(t0);
    srt_stats st = r.Stats();
    std::fprintf(stderr, "%dx%d spp=%d bounces=%d: kernel %.3f ms (wall %.3f ms), %.3e path-samples/s, %.2f rays/sample\n", o.W, o.H, o.spp, o.bounces, st.kernel_ms,
                 wall_ms, (double)st.path_samples / (st.kernel_ms * 1e-3), (double)st.rays / (double)st.path_samples);
    resolve(r, o, SRT_AA_SOURCE_ACCUMULATOR);
    if (write_framebuffer(r, o, o.out) || write_gbuffers(r, o)) return 1;
    if (!o.vis_out.empty()) {
        // the guides of the whole frame, then the visibility pass; the planes asked for follow each other in the file, AO first
        srt_visibility_params vp{};
        srt_visibility_params_default(&vp);
        vp.outputs = (o.ao_given ? SRT_VIS_AO : 0u) | (o.sun_visibility ? SRT_VIS_SUN : 0u);
        if (o.ao_given) vp.ao_samples = (uint32_t)o.ao, vp.ao_radius = o.ao_radius;
        vp.seed = o.seed;
        r.renderVisibility(vp);
        std::vector<float> planes;
        for (uint32_t bit = SRT_VIS_AO; bit <= SRT_VIS_SUN; bit <<= 1) {
            if (!(vp.outputs & bit)) continue;
            planes.resize(planes.size() + (size_t)o.W * o.H);
            r.readVisibility(bit, planes.data() + planes.size() - (size_t)o.W * o.H);
        }
        if (!write_floats(o.vis_out, planes)) return 1;
    }
    if (!o.upsample.empty()) {
        // the guides of the whole frame, then the blocks' anchors interpolated with the library's defaults; the kernel
        // tone-maps its result into the framebuffer (--out is already written).  With --denoise the result replaces the
        // accumulator's non-anchor pixels, which is what the denoiser below then filters — and with --aa too, whose resolve
        // reads the accumulator.
        srt_upsample_params up{};
        srt_upsample_params_default(&up);
        up.steps = o.steps;
        up.flags = SRT_UPSAMPLE_FRAMEBUFFER | (o.denoise.empty() && !o.aa ? 0u : SRT_UPSAMPLE_IN_PLACE);
        r.RenderGBuffer(SRT_GBUF_OBJECT | SRT_GBUF_NORMAL_DEPTH | SRT_GBUF_POSITION);
        r.Upsample(up);
        resolve(r, o, SRT_AA_SOURCE_ACCUMULATOR);
        if (write_framebuffer(r, o, o.upsample)) return 1;
    }
    if (!o.reflection_out.empty() && write_reflection(r, o)) return 1;
    // --reflection-guides: from here on RenderGBuffer renders the reflection guides into the G-buffer slots (--gbuffer, the
    // visibility pass and the upsampler above have had their first hits; --aa's resolve keeps first hits by itself)
    if (o.reflection_guides) r.reflectionBounces = o.reflection_bounces, r.reflectionGuides(true);
    if (!o.denoise.empty()) {
        // the guides of the whole frame, then the filter with the library's defaults; the kernel tone-maps its result into
        // the framebuffer (--out is already written), read back top-down like --out
        srt_denoise_params dp{};
        srt_denoise_params_default(&dp);
        dp.flags |= SRT_DENOISE_FRAMEBUFFER;
        r.RenderGBuffer(SRT_GBUF_ALL);
        r.Denoise(dp);
        resolve(r, o, SRT_AA_SOURCE_DENOISED);
        if (write_framebuffer(r, o, o.denoise)) return 1;
    }
    if (!o.denoise_variance.empty()) {
        // the frame again as two halves, their variance and mean, the guides and the variance-guided filter with the
        // library's defaults (PathTraceRenderer::denoiseVariance); the kernel tone-maps its result into the framebuffer
        // (--out is already written)
        r.denoiseVariance((uint32_t)o.spp, SRT_DENOISE_FRAMEBUFFER);
        resolve(r, o, SRT_AA_SOURCE_DENOISED);
        if (write_framebuffer(r, o, o.denoise_variance)) return 1;
    }
    return 0;
}

// The mode the options ask for (validate() has seen to it that they ask for one).
static int run_mode(const Options& o, Scene& scene) {
    if (!o.probe_grid_arg.empty()) return o.probe_cascade_levels ? shade_probe_cascade_file(o, scene) : shade_probe_grid_file(o, scene);
    if (!o.probes_in.empty()) return trace_probe_file(o, scene);
    if (!o.rays_in.empty()) return trace_ray_file(o, scene);
    if (!o.devices.empty()) return render_multi_device(o, scene);
    if (o.temporal) return render_temporal(o, scene);
    return o.adaptive_given ? render_adaptive(o, scene) : render_frame(o, scene);
}

int main(int argc, char** argv) {
    Options o;
    if (int e = parse(argc, argv, o)) return e;
    if (int e = validate(o)) return e;
    Scene scene(o.scene_path);
    scene.Load();
    if (!scene.lastError().empty()) std::fprintf(stderr, "scene: %s\n", scene.lastError().c_str());  // Scene.hpp:76
    std::fprintf(stderr, "scene %s: %zu objects\n", o.scene_path.c_str(), scene.GetObjects().size());
    if (!o.resave.empty()) scene.SaveAs(o.resave);
    for (const auto& m : o.object_moves)
        if (m.index >= scene.GetObjects().size()) {
            std::fprintf(stderr, "--move-object: the scene has no object %zu\n", m.index);
            return 2;
        }
    try {  // whatever the library or the host layer refuses from here on
        return run_mode(o, scene);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
