// srt_render — command-line front end of the host layer: load a scene in the reference's
// JSON format, path-trace it on one MI355X, write the framebuffer as a binary PPM (P6)
// top-down (the framebuffer's memory rows are already in blit order, Raytracer.cpp:64).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "renderer.hpp"

using namespace srt_host;

// One array as a NumPy .npy file (format 1.0: magic, version, little-endian header length, a Python-literal header padded
// with spaces to a multiple of 64 bytes and ended by a newline, then the raw C-order data).  `rows` rows of `row_bytes`.
static bool write_npy(const std::string& path, const char* descr, int h, int w, int channels, const std::vector<const char*>& rows, size_t row_bytes) {
    char shape[64];
    if (channels == 1) std::snprintf(shape, sizeof shape, "(%d, %d)", h, w);
    else std::snprintf(shape, sizeof shape, "(%d, %d, %d)", h, w, channels);
    std::string header = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': " + shape + ", }";
    const size_t pre = 10;  // magic (6) + version (2) + header length (2)
    while ((pre + header.size() + 1) % 64) header += ' ';
    header += '\n';
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) {
        std::perror(path.c_str());
        return false;
    }
    const unsigned char magic[8] = {0x93, 'N', 'U', 'M', 'P', 'Y', 1, 0};
    const unsigned char len[2] = {(unsigned char)(header.size() & 255), (unsigned char)(header.size() >> 8)};
    bool ok = std::fwrite(magic, 1, 8, f) == 8 && std::fwrite(len, 1, 2, f) == 2 && std::fwrite(header.data(), 1, header.size(), f) == header.size();
    for (const char* r : rows) ok = ok && std::fwrite(r, 1, row_bytes, f) == row_bytes;
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) std::fprintf(stderr, "%s: write failed\n", path.c_str());
    return ok;
}

// --gbuffer PREFIX: the four first-hit buffers, rows top-down (memory rows, as the PPM): memory row m = scene row H - 1 - m.
// (Little-endian hosts: the .npy descriptors say '<'.)
template <class R>
static int write_gbuffers(R& r, const std::string& prefix, int W, int H) {
    struct Out {
        uint32_t bit;
        const char* name;
        const char* descr;
        int channels;
    };
    const Out outs[4] = {{SRT_GBUF_OBJECT, "object", "<i4", 1}, {SRT_GBUF_NORMAL_DEPTH, "normal_depth", "<f4", 4},
                         {SRT_GBUF_POSITION, "position", "<f4", 4}, {SRT_GBUF_ALBEDO, "albedo", "<f4", 4}};
    r.RenderGBuffer(SRT_GBUF_ALL);
    for (const Out& o : outs) {
        const size_t row_bytes = (size_t)W * 4 * (size_t)o.channels;
        std::vector<char> buf(row_bytes * (size_t)H);
        r.ReadGBuffer(o.bit, buf.data());
        std::vector<const char*> rows((size_t)H);
        for (int m = 0; m < H; ++m) rows[(size_t)m] = buf.data() + (size_t)(H - 1 - m) * row_bytes;
        if (!write_npy(prefix + "_" + o.name + ".npy", o.descr, H, W, o.channels, rows, row_bytes)) return 1;
    }
    return 0;
}

// --reflection-out PREFIX: the five outputs of the reflection guides (srt_render_reflection_gbuffer with the library's thresholds
// and `bounces` reflections at most), named and laid out like --gbuffer's, plus PREFIX_bounces.npy (int32 HxW).
static int write_reflection(PathTraceRenderer& r, const std::string& prefix, int W, int H, int bounces) {
    struct Out {
        uint32_t bit;
        const char* name;
        const char* descr;
        int channels;
    };
    const Out outs[5] = {{SRT_REFL_OBJECT, "object", "<i4", 1},    {SRT_REFL_NORMAL_DEPTH, "normal_depth", "<f4", 4}, {SRT_REFL_POSITION, "position", "<f4", 4},
                         {SRT_REFL_ALBEDO, "albedo", "<f4", 4}, {SRT_REFL_BOUNCES, "bounces", "<i4", 1}};
    srt_reflection_params rp{};
    srt_reflection_params_default(&rp);
    rp.row_begin = 0, rp.row_end = H, rp.max_bounces = bounces;
    r.renderReflectionGBuffer(rp);
    for (const Out& o : outs) {
        const size_t row_bytes = (size_t)W * 4 * (size_t)o.channels;
        std::vector<char> buf(row_bytes * (size_t)H);
        r.readReflection(o.bit, buf.data());
        std::vector<const char*> rows((size_t)H);
        for (int m = 0; m < H; ++m) rows[(size_t)m] = buf.data() + (size_t)(H - 1 - m) * row_bytes;
        if (!write_npy(prefix + "_" + o.name + ".npy", o.descr, H, W, o.channels, rows, row_bytes)) return 1;
    }
    return 0;
}

// --rays IN.f32 --rays-out OUT.bin: closest-hit queries for the rays of a file (N records of 8 float32: origin xyzw, direction
// xyz + t_max) against the scene; the five outputs of srt_trace_rays follow each other in OUT.bin in the order of their bits.
// With --any-hit the rays go through srt_trace_occlusion instead and OUT.bin receives the occluded array (N int32) alone.
// With --radiance N (radiance_samples > 0) they go through srt_trace_radiance — samples 1..N, `bounces`, `seed`, id_base 0 — and
// OUT.bin receives the N float4 running means alone.
// With `tail` (--probe-tail: a grid, P x 9 float4 coefficients and SRT_PROBE_TAIL_* flags) the radiance trace runs under srt_probe_tail.
struct RayTail {
    const srt_probe_grid* grid = nullptr;
    std::vector<float> coefficients;
    uint32_t flags = 0;
};

static int trace_ray_file(const Scene& scene, int device, const std::string& in, const std::string& out, bool normalize, bool any_hit,
                          int radiance_samples, int bounces, unsigned seed, const RayTail& tail = RayTail()) {
    FILE* f = std::fopen(in.c_str(), "rb");
    if (!f) {
        std::perror(in.c_str());
        return 1;
    }
    std::vector<float> rec;
    float buf[2048];
    for (size_t got; (got = std::fread(buf, sizeof(float), 2048, f)) > 0;) rec.insert(rec.end(), buf, buf + got);
    std::fclose(f);
    if (rec.empty() || rec.size() % 8) {
        std::fprintf(stderr, "%s: %zu floats: want N >= 1 records of 8 float32\n", in.c_str(), rec.size());
        return 2;
    }
    const size_t n = rec.size() / 8;
    std::vector<float> o(4 * n), d(4 * n);
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(&o[4 * i], &rec[8 * i], 4 * sizeof(float));
        std::memcpy(&d[4 * i], &rec[8 * i + 4], 4 * sizeof(float));
    }
    try {
        PathTraceRenderer r(device, 8, 8);  // (the frame size plays no part in a ray query)
        r.SetScene(scene);
        if (radiance_samples > 0) {
            srt_radiance_params rp{};
            srt_radiance_params_default(&rp);
            rp.sample_count = (uint32_t)radiance_samples, rp.max_bounces = bounces, rp.seed = seed;
            if (normalize) rp.flags |= SRT_RADIANCE_NORMALIZE;
            if (tail.grid) {
                r.setProbeGrid(*tail.grid);
                r.writeProbeGridInputs(tail.coefficients.data(), nullptr, nullptr, tail.coefficients.size() / 36, 0);
                srt_probe_tail_params tp{};
                srt_probe_tail_params_default(&tp);
                tp.flags = tail.flags;
                r.probeTail(tp);
            }
            r.traceRadiance(o.data(), d.data(), n, rp);
            std::vector<float> rad(4 * n);
            r.readRadiance(rad.data());
            FILE* g = std::fopen(out.c_str(), "wb");
            if (!g) {
                std::perror(out.c_str());
                return 1;
            }
            bool ok = std::fwrite(rad.data(), sizeof(float), rad.size(), g) == rad.size();
            ok = (std::fclose(g) == 0) && ok;
            if (!ok) {
                std::fprintf(stderr, "%s: write failed\n", out.c_str());
                return 1;
            }
            std::fprintf(stderr, "%zu rays, %d samples of radiance each%s: %s\n", n, radiance_samples, normalize ? " (directions normalized)" : "", out.c_str());
            return 0;
        }
        if (any_hit) r.traceOcclusion(o.data(), d.data(), n, normalize ? SRT_OCCLUSION_NORMALIZE : 0u);
        else r.traceRays(o.data(), d.data(), n, SRT_GBUF_ALL | SRT_RAYS_OCCLUDED, normalize ? SRT_RAYS_NORMALIZE : 0u);
        FILE* g = std::fopen(out.c_str(), "wb");
        if (!g) {
            std::perror(out.c_str());
            return 1;
        }
        bool ok = true;
        std::vector<char> data;
        for (uint32_t bit = any_hit ? SRT_RAYS_OCCLUDED : 1u; bit <= SRT_RAYS_OCCLUDED; bit <<= 1) {
            data.resize(n * ((bit == SRT_GBUF_OBJECT || bit == SRT_RAYS_OCCLUDED) ? sizeof(int32_t) : 4 * sizeof(float)));
            r.readRayOutput(bit, data.data());
            ok = ok && std::fwrite(data.data(), 1, data.size(), g) == data.size();
        }
        ok = (std::fclose(g) == 0) && ok;
        if (!ok) {
            std::fprintf(stderr, "%s: write failed\n", out.c_str());
            return 1;
        }
        std::fprintf(stderr, "%zu rays traced%s%s: %s\n", n, any_hit ? " (any hit)" : "", normalize ? " (directions normalized)" : "", out.c_str());
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

// Every float32 of a file, or an empty vector (with a message) when it cannot be read or does not hold N >= 1 records of 4.
static std::vector<float> read_float4_file(const std::string& path) {
    std::vector<float> v;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) {
        std::perror(path.c_str());
        return v;
    }
    float buf[2048];
    for (size_t got; (got = std::fread(buf, sizeof(float), 2048, f)) > 0;) v.insert(v.end(), buf, buf + got);
    std::fclose(f);
    if (v.empty() || v.size() % 4) {
        std::fprintf(stderr, "%s: %zu floats: want N >= 1 records of 4 float32\n", path.c_str(), v.size());
        v.clear();
    }
    return v;
}

static bool write_floats(const std::string& path, const std::vector<float>& v) {
    FILE* g = std::fopen(path.c_str(), "wb");
    if (!g) {
        std::perror(path.c_str());
        return false;
    }
    bool ok = std::fwrite(v.data(), sizeof(float), v.size(), g) == v.size();
    ok = (std::fclose(g) == 0) && ok;
    if (!ok) std::fprintf(stderr, "%s: write failed\n", path.c_str());
    return ok;
}

// --probes IN.f32 --probe-directions K|FILE.f32 --probes-out OUT.bin: light probes (srt_trace_light_probes) at the positions of a
// file (P records of 4 float32: xyz, w ignored) over K spherical Fibonacci directions (srt_light_probe_sphere) or the directions
// of a file (K records of 4 float32: xyz, weight) — samples 1..`samples`, `bounces`, `seed`, id_base 0.  OUT.bin receives the P*9
// float4 coefficients; radiance_out, when given, the P*K float4 running means.
static int trace_probe_file(const Scene& scene, int device, const std::string& in, const std::string& dirs, const std::string& out,
                            const std::string& radiance_out, int samples, int bounces, unsigned seed) {
    const std::vector<float> pos = read_float4_file(in);
    if (pos.empty()) return 2;
    std::vector<float> dir;
    if (dirs.find_first_not_of("0123456789") == std::string::npos) {
        const long k = std::atol(dirs.c_str());
        if (k < 1 || k > (long)SRT_LIGHT_PROBE_MAX_DIRECTIONS) {
            std::fprintf(stderr, "--probe-directions %s: want a count 1..4096 or a file\n", dirs.c_str());
            return 2;
        }
        dir.resize(4 * (size_t)k);
        srt_light_probe_sphere((size_t)k, dir.data());
    } else {
        dir = read_float4_file(dirs);
        if (dir.empty() || dir.size() / 4 > SRT_LIGHT_PROBE_MAX_DIRECTIONS) {
            std::fprintf(stderr, "--probe-directions %s: want 1..4096 records of 4 float32\n", dirs.c_str());
            return 2;
        }
    }
    const size_t np = pos.size() / 4, nk = dir.size() / 4;
    try {
        PathTraceRenderer r(device, 8, 8);  // (the frame size plays no part in a probe trace)
        r.SetScene(scene);
        srt_light_probe_params lp{};
        srt_light_probe_params_default(&lp);
        lp.sample_count = (uint32_t)samples, lp.max_bounces = bounces, lp.seed = seed;
        if (!radiance_out.empty()) lp.outputs |= SRT_LIGHT_PROBE_RADIANCE;
        r.traceLightProbes(pos.data(), np, dir.data(), nk, lp);
        std::vector<float> coeff(np * 9 * 4);
        r.readLightProbeOutput(SRT_LIGHT_PROBE_COEFFICIENTS, coeff.data());
        if (!write_floats(out, coeff)) return 1;
        if (!radiance_out.empty()) {
            std::vector<float> rad(np * nk * 4);
            r.readLightProbeOutput(SRT_LIGHT_PROBE_RADIANCE, rad.data());
            if (!write_floats(radiance_out, rad)) return 1;
        }
        std::fprintf(stderr, "%zu probes x %zu directions, %d samples each: %s\n", np, nk, samples, out.c_str());
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
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

// --probe-grid G --probe-directions K --irradiance-out FILE: a real-time preview of the diffuse indirect light.  The first-hit buffers of
// the W x H frame, light probes (srt_trace_light_probes: K spherical Fibonacci directions, samples 1..`samples`, `bounces`, `seed`,
// id_base 0) at the grid's positions (srt_probe_grid_positions), then srt_shade_probe_grid over the whole frame with `flags` and the
// default or the hemisphere band weights.  FILE receives W*H float4, scene rows.
// --probe-depth R: the filtered visibility test instead of none or the exact one: srt_trace_probe_depth at the same positions and
// directions (resolution R, --probe-depth-sharpness, --probe-depth-max), then srt_shade_probe_grid_depth (--probe-depth-bias);
// --probe-depth-out receives the probes' R*R float4 moments.
struct ProbeDepthOptions {
    int resolution = 0;  // 0: no --probe-depth
    int sharpness = 5;
    float max_distance = 10000.0f, bias = 0.0f;
    std::string out;
};
// --probe-classify: srt_classify_probes on the grid first (--probe-relocate: with relocation along the same directions;
// --probe-clearance, --probe-max-offset, --probe-steps), the probes and depth maps traced at the positions it gives, and
// srt_shade_probe_grid_states in place of the shading call; --states-out receives the probes' records (float4 each).
struct ProbeClassifyOptions {
    bool on = false, relocate = false;
    float clearance = 0.2f, max_offset = 0.45f;
    int steps = 8;
    std::string out;
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
    int frame_spp = 0;      // --spp
    std::string frame_out;  // --out
    int feedback = 0;  // 0: no --probe-feedback
    int bounces = -1;  // < 0: --bounces
    bool scroll_on = false;  // --probe-scroll
    int32_t scroll[3] = {0, 0, 0};
    int scroll_after = 1;    // --probe-scroll-after
    std::string grid, coefficients;
    uint32_t flags() const {
        return (depth ? SRT_PROBE_TAIL_DEPTH : 0u) | (states ? SRT_PROBE_TAIL_STATES : 0u) | (normal_weight ? SRT_PROBE_TAIL_NORMAL_WEIGHT : 0u);
    }
};

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

static int shade_probe_grid_file(Scene& scene, int device, int W, int H, int fov, srt_probe_grid grid, int directions, int samples, int bounces,
                                 unsigned seed, uint32_t flags, bool hemisphere, const std::string& out, const ProbeDepthOptions& depth,
                                 const ProbeClassifyOptions& classify, const ProbeUpdateOptions& update, const std::vector<ObjectMove>& moves,
                                 const ProbeTailOptions& tail) {
    const size_t np = (size_t)grid.counts[0] * (size_t)grid.counts[1] * (size_t)grid.counts[2];
    std::vector<float> pos(4 * np), dir(4 * (size_t)directions);
    if (srt_probe_grid_positions(&grid, pos.data()) != SRT_OK) {
        std::fprintf(stderr, "--probe-grid: want finite origins, finite spacings > 0, counts >= 1 and at most 2^30 probes\n");
        return 2;
    }
    srt_light_probe_sphere((size_t)directions, dir.data());
    try {
        PathTraceRenderer r(device, W, H);
        r.FOV = fov;
        r.MAXBOUNCES = bounces;
        r.seed = seed;
        r.SetScene(scene);
        srt_light_probe_params lp{};
        srt_light_probe_params_default(&lp);
        lp.sample_count = (uint32_t)samples, lp.max_bounces = bounces, lp.seed = seed;
        std::vector<float> states;
        srt_probe_classify_params cp{};
        srt_probe_classify_params_default(&cp);
        cp.clearance = classify.clearance, cp.max_offset = classify.max_offset, cp.steps = (uint32_t)classify.steps;
        cp.flags = classify.relocate ? SRT_PROBE_CLASSIFY_RELOCATE : 0u;
        cp.outputs = SRT_PROBE_STATE_RECORDS | SRT_PROBE_STATE_POSITIONS;
        auto classify_now = [&]() {  // the records, and the positions the probes are traced at
            r.classifyProbes(dir.data(), (size_t)directions, cp);
            states.resize(4 * np);
            r.readProbeStatesOutput(SRT_PROBE_STATE_RECORDS, states.data());
            r.readProbeStatesOutput(SRT_PROBE_STATE_POSITIONS, pos.data());
        };
        if (classify.on) {  // the states first: the probes are traced where the classification puts them
            r.setProbeGrid(grid);
            classify_now();
            if (!classify.out.empty() && !moves.size() && !write_floats(classify.out, states)) return 1;
        }
        std::vector<float> coeff(np * 9 * 4), moments;
        bool have_moments = false;  // (the feedback rounds trace the maps up front)
        srt_probe_depth_params dp{};
        srt_probe_depth_params_default(&dp);
        if (depth.resolution) {
            dp.resolution = (uint32_t)depth.resolution, dp.sharpness = (uint32_t)depth.sharpness, dp.max_distance = depth.max_distance;
            moments.resize(np * (size_t)depth.resolution * depth.resolution * 4);
        }
        if (update.frames) {  // (classify.on: main() has seen to it)
            srt_probe_list_params ls{};
            srt_probe_list_params_default(&ls);
            r.listProbes(states.data(), np, ls);
            r.resetProbeHistory(SRT_PROBE_HISTORY_COEFFICIENTS | (depth.resolution ? SRT_PROBE_HISTORY_MOMENTS : 0u), np, (uint32_t)depth.resolution);
            srt_probe_blend_params bp{};
            srt_probe_blend_params_default(&bp);
            bp.hysteresis = bp.depth_hysteresis = update.hysteresis;
            if (bp.fast_hysteresis > update.hysteresis) bp.fast_hysteresis = update.hysteresis;
            bp.flags = SRT_PROBE_BLEND_LISTED | (depth.resolution ? SRT_PROBE_BLEND_MOMENTS : 0u);
            lp.sample_count = (uint32_t)update.samples;
            std::vector<float> previous;
            for (int f = 1; f <= update.frames; ++f) {
                const bool moved = f > 1 && !moves.empty();
                if (moved) {  // the objects move; the classification and the list follow, the records of the frame before are kept
                    for (const auto& m : moves) {
                        float* p = scene.Objects()[m.index].position;
                        for (int a = 0; a < 3; ++a) p[a] = p[a] + m.step[a];
                    }
                    r.UpdateScene(scene);
                    previous = states;
                    classify_now();
                    r.listProbes(states.data(), np, ls);
                }
                lp.seed = (uint32_t)f;
                r.traceLightProbesListed(f == 1 || moved ? pos.data() : nullptr, np, f == 1 ? dir.data() : nullptr, (size_t)directions, lp);
                if (depth.resolution) r.traceProbeDepthListed(nullptr, np, nullptr, (size_t)directions, dp);
                srt_probe_blend_params b = bp;
                if (moved) b.flags |= SRT_PROBE_BLEND_PREVIOUS_STATES | SRT_PROBE_BLEND_COUNT_WORK;
                r.blendProbes(moved ? previous.data() : nullptr, np, b);
                if (moved) {
                    const srt_probe_blend_work w = r.probeBlendWork();
                    std::fprintf(stderr, "probe update frame %d: %llu probes blended, %llu restarted, %llu changed\n", f, (unsigned long long)w.probes,
                                 (unsigned long long)w.restarted, (unsigned long long)w.changed);
                }
            }
            if (!classify.out.empty() && moves.size() && !write_floats(classify.out, states)) return 1;  // (the records of the last frame)
            r.readProbeHistory(SRT_PROBE_HISTORY_COEFFICIENTS, coeff.data());
            if (depth.resolution) r.readProbeHistory(SRT_PROBE_HISTORY_MOMENTS, moments.data());
        } else if (tail.feedback) {
            r.setProbeGrid(grid);
            if (depth.resolution) {  // the maps the tail reads under --probe-tail-depth, and the shading after the last round
                r.traceProbeDepth(pos.data(), np, dir.data(), (size_t)directions, dp);
                r.readProbeDepthOutput(SRT_PROBE_DEPTH_MOMENTS, moments.data());
                have_moments = true;
            }
            r.resetProbeHistory(SRT_PROBE_HISTORY_COEFFICIENTS, np, 0);
            srt_probe_blend_params bp{};
            srt_probe_blend_params_default(&bp);
            srt_probe_tail_params tp{};
            srt_probe_tail_params_default(&tp);
            tp.flags = tail.flags() | SRT_PROBE_TAIL_COUNT_WORK;
            if (tail.bounces >= 0) lp.max_bounces = tail.bounces;
            for (int f = 1; f <= tail.feedback; ++f) {
                tp.enabled = f > 1 ? 1 : 0;  // round 1 has no history
                if (f > 1) {
                    r.readProbeHistory(SRT_PROBE_HISTORY_COEFFICIENTS, coeff.data());
                    r.writeProbeGridInputs(coeff.data(), tail.depth ? moments.data() : nullptr, tail.states ? states.data() : nullptr, np, (uint32_t)depth.resolution);
                }
                r.probeTail(tp);
                lp.seed = (uint32_t)f;
                r.traceLightProbes(pos.data(), np, dir.data(), (size_t)directions, lp);
                r.blendProbes(nullptr, np, bp);
                if (f > 1) {
                    const srt_probe_tail_work w = r.probeTailWork();
                    std::fprintf(stderr, "probe feedback round %d: %llu lookups, %llu dark, %llu mirror ends\n", f, (unsigned long long)w.tails,
                                 (unsigned long long)w.dark, (unsigned long long)w.mirror_ends);
                }
                if (tail.scroll_on && f == tail.scroll_after) {  // the grid moves; what is made per grid is made again
                    r.scrollProbes(tail.scroll, SRT_PROBE_SCROLL_COEFFICIENTS, SRT_PROBE_SCROLL_SET_GRID | SRT_PROBE_SCROLL_COUNT_WORK);
                    grid = r.probeGrid();
                    srt_probe_grid_positions(&grid, pos.data());
                    if (classify.on) classify_now();
                    if (depth.resolution) {
                        r.traceProbeDepth(pos.data(), np, dir.data(), (size_t)directions, dp);
                        r.readProbeDepthOutput(SRT_PROBE_DEPTH_MOMENTS, moments.data());
                    }
                    const srt_probe_scroll_work w = r.probeScrollWork();
                    std::fprintf(stderr, "probe scroll after round %d by %d,%d,%d: %llu probes, %llu retained, %llu exposed\n", f, tail.scroll[0], tail.scroll[1],
                                 tail.scroll[2], (unsigned long long)w.probes, (unsigned long long)w.retained, (unsigned long long)w.exposed);
                }
            }
            r.readProbeHistory(SRT_PROBE_HISTORY_COEFFICIENTS, coeff.data());
            if (tail.frame) {  // the picture: every path of the frame ends in the history the rounds have left
                r.writeProbeGridInputs(coeff.data(), tail.depth ? moments.data() : nullptr, tail.states ? states.data() : nullptr, np, (uint32_t)depth.resolution);
                tp.enabled = 1;
                r.probeTail(tp);
                r.renderProbeTailFrame((uint32_t)tail.frame_spp, bounces, seed);
                std::vector<uint32_t> fb((size_t)W * H);
                r.ReadFramebuffer(fb.data(), (size_t)W * 4);
                const srt_probe_tail_work w = r.probeTailWork();
                std::fprintf(stderr, "probe tail frame: %d samples per pixel at %d bounces, %llu lookups, %llu dark, %llu mirror ends: %s\n", tail.frame_spp, bounces,
                             (unsigned long long)w.tails, (unsigned long long)w.dark, (unsigned long long)w.mirror_ends, tail.frame_out.c_str());
                if (write_ppm_file(fb, W, H, tail.frame_out)) return 1;
            }
            tp.enabled = 0;
            r.probeTail(tp);
        } else {
            r.traceLightProbes(pos.data(), np, dir.data(), (size_t)directions, lp);
            r.readLightProbeOutput(SRT_LIGHT_PROBE_COEFFICIENTS, coeff.data());
        }
        srt_probe_grid_params sp{};
        srt_probe_grid_params_default(&sp);
        sp.row_begin = 0, sp.row_end = H, sp.flags = flags;
        if (hemisphere) sp.band_weight[0] = 1.0f, sp.band_weight[1] = 0.5f, sp.band_weight[2] = 0.0f;
        r.setProbeGrid(grid);
        if (depth.resolution) {
            if (!update.frames && !have_moments) {
                r.traceProbeDepth(pos.data(), np, dir.data(), (size_t)directions, dp);
                r.readProbeDepthOutput(SRT_PROBE_DEPTH_MOMENTS, moments.data());
            }
            if (!depth.out.empty() && !write_floats(depth.out, moments)) return 1;
            srt_probe_grid_depth_params gd{};
            srt_probe_grid_depth_params_default(&gd);
            gd.bias = depth.bias;
            if (classify.on) r.shadeProbeGridStates(coeff.data(), moments.data(), states.data(), np, (uint32_t)depth.resolution, sp, &gd);
            else r.shadeProbeGridDepth(coeff.data(), moments.data(), np, (uint32_t)depth.resolution, sp, gd);
        } else if (classify.on) {
            r.shadeProbeGridStates(coeff.data(), nullptr, states.data(), np, 0, sp, nullptr);
        } else {
            r.shadeProbeGrid(coeff.data(), np, sp);
        }
        std::vector<float> img((size_t)W * H * 4);
        r.readProbeGridOutput(img.data());
        if (!write_floats(out, img)) return 1;
        std::fprintf(stderr, "%dx%d: %zu probes x %d directions, %d samples each, flags 0x%x%s: %s\n", W, H, np, directions, samples, flags,
                     hemisphere ? " (hemisphere band weights)" : "", out.c_str());
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

// --probe-grid G --probe-directions K --probe-cascade L [--probe-cascade-blend B] --irradiance-out FILE: the frame shaded from L
// nested grids (srt_shade_probe_cascade).  The levels come from srt_probe_cascade_grids around the camera position, with G's
// spacing as the finest spacing and G's counts (G's origin is not read); per level the route of --probe-grid runs on the level's
// grid through the single-grid calls — the classification (--probe-classify), the probes traced at the positions it gives, the
// depth maps (--probe-depth R) — and PathTraceRenderer::captureProbeCascadeLevel keeps its results; then the cascade shading runs
// in place of the single-grid call.  FILE receives W*H float4, scene rows.
static int shade_probe_cascade_file(Scene& scene, int device, int W, int H, int fov, const srt_probe_grid& finest, int levels, float blend, int directions,
                                    int samples, int bounces, unsigned seed, uint32_t grid_flags, bool hemisphere, const std::string& out,
                                    const ProbeDepthOptions& depth, const ProbeClassifyOptions& classify) {
    const size_t np = (size_t)finest.counts[0] * (size_t)finest.counts[1] * (size_t)finest.counts[2];
    std::vector<float> pos(4 * np), dir(4 * (size_t)directions);
    srt_light_probe_sphere((size_t)directions, dir.data());
    try {
        PathTraceRenderer r(device, W, H);
        r.FOV = fov;
        r.MAXBOUNCES = bounces;
        r.seed = seed;
        r.SetScene(scene);
        const float centre[3] = {r.camera.position.x, r.camera.position.y, r.camera.position.z};
        srt_probe_cascade cascade{};
        if (srt_probe_cascade_grids(centre, finest.spacing, finest.counts, (uint32_t)levels, &cascade) != SRT_OK) {
            std::fprintf(stderr, "--probe-cascade: the levels' spacings must stay finite and the probes of a level at most 2^30\n");
            return 2;
        }
        cascade.resolution = (uint32_t)depth.resolution, cascade.blend_cells = blend;
        r.setProbeCascade(cascade);
        srt_light_probe_params lp{};
        srt_light_probe_params_default(&lp);
        lp.sample_count = (uint32_t)samples, lp.max_bounces = bounces, lp.seed = seed;
        srt_probe_classify_params cp{};
        srt_probe_classify_params_default(&cp);
        cp.clearance = classify.clearance, cp.max_offset = classify.max_offset, cp.steps = (uint32_t)classify.steps;
        cp.flags = classify.relocate ? SRT_PROBE_CLASSIFY_RELOCATE : 0u;
        cp.outputs = SRT_PROBE_STATE_RECORDS | SRT_PROBE_STATE_POSITIONS;
        srt_probe_depth_params dp{};
        srt_probe_depth_params_default(&dp);
        if (depth.resolution) dp.resolution = (uint32_t)depth.resolution, dp.sharpness = (uint32_t)depth.sharpness, dp.max_distance = depth.max_distance;
        std::vector<float> coeff(np * 9 * 4), moments(np * (size_t)depth.resolution * depth.resolution * 4), states(classify.on ? 4 * np : 0);
        for (int l = 0; l < levels; ++l) {
            const srt_probe_grid& g = cascade.grid[l];
            r.setProbeGrid(g);
            srt_probe_grid_positions(&g, pos.data());
            if (classify.on) {  // the states first: the probes are traced where the classification puts them
                r.classifyProbes(dir.data(), (size_t)directions, cp);
                r.readProbeStatesOutput(SRT_PROBE_STATE_RECORDS, states.data());
                r.readProbeStatesOutput(SRT_PROBE_STATE_POSITIONS, pos.data());
            }
            r.traceLightProbes(pos.data(), np, dir.data(), (size_t)directions, lp);
            r.readLightProbeOutput(SRT_LIGHT_PROBE_COEFFICIENTS, coeff.data());
            if (depth.resolution) {
                r.traceProbeDepth(pos.data(), np, dir.data(), (size_t)directions, dp);
                r.readProbeDepthOutput(SRT_PROBE_DEPTH_MOMENTS, moments.data());
            }
            r.writeProbeGridInputs(coeff.data(), depth.resolution ? moments.data() : nullptr, classify.on ? states.data() : nullptr, np, (uint32_t)depth.resolution);
            r.captureProbeCascadeLevel((uint32_t)l, SRT_PROBE_CASCADE_COEFFICIENTS | (depth.resolution ? SRT_PROBE_CASCADE_MOMENTS : 0u) |
                                                        (classify.on ? SRT_PROBE_CASCADE_RECORDS : 0u));
            std::fprintf(stderr, "probe cascade level %d: origin %g %g %g, spacing %g %g %g\n", l, (double)g.origin[0], (double)g.origin[1], (double)g.origin[2],
                         (double)g.spacing[0], (double)g.spacing[1], (double)g.spacing[2]);
        }
        srt_probe_cascade_params sp{};
        srt_probe_cascade_params_default(&sp);
        sp.row_begin = 0, sp.row_end = H;
        sp.flags = ((grid_flags & SRT_PROBE_GRID_NORMAL_WEIGHT) ? SRT_PROBE_CASCADE_NORMAL_WEIGHT : 0u) | ((grid_flags & SRT_PROBE_GRID_ALBEDO) ? SRT_PROBE_CASCADE_ALBEDO : 0u) |
                   (depth.resolution ? SRT_PROBE_CASCADE_DEPTH : 0u) | (classify.on ? SRT_PROBE_CASCADE_STATES : 0u) | SRT_PROBE_CASCADE_COUNT_WORK;
        sp.bias = depth.bias;
        if (hemisphere) sp.band_weight[0] = 1.0f, sp.band_weight[1] = 0.5f, sp.band_weight[2] = 0.0f;
        r.shadeProbeCascade(sp);
        std::vector<float> img((size_t)W * H * 4);
        r.readProbeGridOutput(img.data());
        if (!write_floats(out, img)) return 1;
        const srt_probe_cascade_work w = r.probeCascadeWork();
        std::fprintf(stderr, "%dx%d: %d levels of %zu probes x %d directions, %d samples each, flags 0x%x%s: %llu hit pixels, %llu blended, first level %llu %llu %llu %llu: %s\n",
                     W, H, levels, np, directions, samples, sp.flags, hemisphere ? " (hemisphere band weights)" : "", (unsigned long long)w.pixels,
                     (unsigned long long)w.blended, (unsigned long long)w.first_level[0], (unsigned long long)w.first_level[1], (unsigned long long)w.first_level[2],
                     (unsigned long long)w.first_level[3], out.c_str());
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}

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

int main(int argc, char** argv) {
    std::string scene_path, out = "frame.ppm", resave, gbuffer, denoise, upsample, denoise_variance, rays_in, rays_out;
    bool rays_normalize = false, rays_any_hit = false;
    int radiance = 0;
    bool radiance_given = false;
    std::string probes_in, probes_out, probe_directions, probe_radiance_out;
    std::string probe_grid_arg, irradiance_out;
    bool probe_visibility = false, probe_normal_weight = false, probe_albedo = false, probe_hemisphere = false;
    ProbeDepthOptions probe_depth;
    bool probe_depth_given = false, probe_depth_option = false;
    ProbeClassifyOptions probe_classify;
    bool probe_classify_option = false;
    ProbeUpdateOptions probe_update;
    ProbeTailOptions probe_tail;
    int probe_cascade_levels = 0;  // 0: no --probe-cascade
    float probe_cascade_blend = 1.0f;
    bool probe_cascade_given = false;
    bool probe_feedback_given = false, probe_bounces_given = false, probe_scroll_given = false, probe_scroll_ok = true;
    bool probe_update_given = false, probe_update_option = false;
    int adaptive = 0, adaptive_max = 0;
    bool adaptive_given = false, adaptive_threshold_given = false, adaptive_max_given = false;
    float adaptive_threshold = 0;
    std::string counts_out;
    std::string vis_out;
    int ao = 0;
    bool ao_given = false, sun_visibility = false;
    float ao_radius = INFINITY;
    bool reflection_guides = false, reflection_bounces_given = false;
    int reflection_bounces = 8;
    std::string reflection_out;
    int temporal = 0, steps = 1, aa = 0;
    bool aa_given = false, temporal_variance = false, refit = false;
    bool mirror_history = false, mirror_radius_given = false;
    float mirror_radius = 2.0f;
    float move[3] = {0, 0, 0}, turn_deg = 0;
    std::vector<ObjectMove> object_moves;
    int W = 1280, H = 720, spp = 32, bounces = 2, fov = 55, device = 0;  // Raytracer.cpp:26-27,31-32
    unsigned seed = 0;
    std::vector<int> devices;
    bool equal_bands = false;
    for (int i = 1; i < argc; ++i) {
        auto need = [&](const char* n) -> const char* {
            if (i + 1 >= argc) {
                std::fprintf(stderr, "%s needs a value\n", n);
                std::exit(2);
            }
            return argv[++i];
        };
        if (!std::strcmp(argv[i], "--scene")) scene_path = need("--scene");
        else if (!std::strcmp(argv[i], "--width")) W = std::atoi(need("--width"));
        else if (!std::strcmp(argv[i], "--height")) H = std::atoi(need("--height"));
        else if (!std::strcmp(argv[i], "--spp")) spp = std::atoi(need("--spp"));
        else if (!std::strcmp(argv[i], "--bounces")) bounces = std::atoi(need("--bounces"));
        else if (!std::strcmp(argv[i], "--fov")) fov = std::atoi(need("--fov"));
        else if (!std::strcmp(argv[i], "--seed")) seed = (unsigned)std::strtoul(need("--seed"), nullptr, 10);
        else if (!std::strcmp(argv[i], "--device")) device = std::atoi(need("--device"));
        else if (!std::strcmp(argv[i], "--balance")) equal_bands = false;
        else if (!std::strcmp(argv[i], "--equal-bands")) equal_bands = true;
        else if (!std::strcmp(argv[i], "--devices")) {
            for (const char* p = need("--devices"); *p;) {
                devices.push_back(std::atoi(p));
                while (*p && *p != ',') ++p;
                if (*p == ',') ++p;
            }
        }
        else if (!std::strcmp(argv[i], "--out")) out = need("--out");
        else if (!std::strcmp(argv[i], "--resave")) resave = need("--resave");
        else if (!std::strcmp(argv[i], "--gbuffer")) gbuffer = need("--gbuffer");
        else if (!std::strcmp(argv[i], "--denoise")) denoise = need("--denoise");
        else if (!std::strcmp(argv[i], "--denoise-variance")) denoise_variance = need("--denoise-variance");
        else if (!std::strcmp(argv[i], "--steps")) steps = std::atoi(need("--steps"));
        else if (!std::strcmp(argv[i], "--upsample")) upsample = need("--upsample");
        else if (!std::strcmp(argv[i], "--aa")) aa = std::atoi(need("--aa")), aa_given = true;
        else if (!std::strcmp(argv[i], "--temporal-variance")) temporal_variance = true;
        else if (!std::strcmp(argv[i], "--refit")) refit = true;
        else if (!std::strcmp(argv[i], "--rays")) rays_in = need("--rays");
        else if (!std::strcmp(argv[i], "--rays-out")) rays_out = need("--rays-out");
        else if (!std::strcmp(argv[i], "--rays-normalize")) rays_normalize = true;
        else if (!std::strcmp(argv[i], "--any-hit")) rays_any_hit = true;
        else if (!std::strcmp(argv[i], "--radiance")) radiance = std::atoi(need("--radiance")), radiance_given = true;
        else if (!std::strcmp(argv[i], "--probes")) probes_in = need("--probes");
        else if (!std::strcmp(argv[i], "--probes-out")) probes_out = need("--probes-out");
        else if (!std::strcmp(argv[i], "--probe-directions")) probe_directions = need("--probe-directions");
        else if (!std::strcmp(argv[i], "--probe-radiance-out")) probe_radiance_out = need("--probe-radiance-out");
        else if (!std::strcmp(argv[i], "--probe-grid")) probe_grid_arg = need("--probe-grid");
        else if (!std::strcmp(argv[i], "--irradiance-out")) irradiance_out = need("--irradiance-out");
        else if (!std::strcmp(argv[i], "--probe-visibility")) probe_visibility = true;
        else if (!std::strcmp(argv[i], "--probe-normal-weight")) probe_normal_weight = true;
        else if (!std::strcmp(argv[i], "--probe-albedo")) probe_albedo = true;
        else if (!std::strcmp(argv[i], "--probe-hemisphere")) probe_hemisphere = true;
        else if (!std::strcmp(argv[i], "--probe-depth")) probe_depth.resolution = std::atoi(need("--probe-depth")), probe_depth_given = true;
        else if (!std::strcmp(argv[i], "--probe-depth-sharpness")) probe_depth.sharpness = std::atoi(need("--probe-depth-sharpness")), probe_depth_option = true;
        else if (!std::strcmp(argv[i], "--probe-depth-max")) probe_depth.max_distance = std::strtof(need("--probe-depth-max"), nullptr), probe_depth_option = true;
        else if (!std::strcmp(argv[i], "--probe-depth-bias")) probe_depth.bias = std::strtof(need("--probe-depth-bias"), nullptr), probe_depth_option = true;
        else if (!std::strcmp(argv[i], "--probe-depth-out")) probe_depth.out = need("--probe-depth-out"), probe_depth_option = true;
        else if (!std::strcmp(argv[i], "--probe-classify")) probe_classify.on = true;
        else if (!std::strcmp(argv[i], "--probe-relocate")) probe_classify.relocate = true, probe_classify_option = true;
        else if (!std::strcmp(argv[i], "--probe-clearance")) probe_classify.clearance = std::strtof(need("--probe-clearance"), nullptr), probe_classify_option = true;
        else if (!std::strcmp(argv[i], "--probe-max-offset")) probe_classify.max_offset = std::strtof(need("--probe-max-offset"), nullptr), probe_classify_option = true;
        else if (!std::strcmp(argv[i], "--probe-steps")) probe_classify.steps = std::atoi(need("--probe-steps")), probe_classify_option = true;
        else if (!std::strcmp(argv[i], "--states-out")) probe_classify.out = need("--states-out"), probe_classify_option = true;
        else if (!std::strcmp(argv[i], "--probe-update")) probe_update.frames = std::atoi(need("--probe-update")), probe_update_given = true;
        else if (!std::strcmp(argv[i], "--probe-hysteresis")) probe_update.hysteresis = std::strtof(need("--probe-hysteresis"), nullptr), probe_update_option = true;
        else if (!std::strcmp(argv[i], "--probe-tail")) probe_tail.on = true;
        else if (!std::strcmp(argv[i], "--probe-tail-frame")) probe_tail.frame = true;
        else if (!std::strcmp(argv[i], "--probe-tail-depth")) probe_tail.depth = true;
        else if (!std::strcmp(argv[i], "--probe-tail-states")) probe_tail.states = true;
        else if (!std::strcmp(argv[i], "--probe-tail-normal-weight")) probe_tail.normal_weight = true;
        else if (!std::strcmp(argv[i], "--probe-tail-grid")) probe_tail.grid = need("--probe-tail-grid");
        else if (!std::strcmp(argv[i], "--probe-tail-coefficients")) probe_tail.coefficients = need("--probe-tail-coefficients");
        else if (!std::strcmp(argv[i], "--probe-feedback")) probe_tail.feedback = std::atoi(need("--probe-feedback")), probe_feedback_given = true;
        else if (!std::strcmp(argv[i], "--probe-cascade")) probe_cascade_levels = std::atoi(need("--probe-cascade")), probe_cascade_given = true;
        else if (!std::strcmp(argv[i], "--probe-cascade-blend")) probe_cascade_blend = std::strtof(need("--probe-cascade-blend"), nullptr), probe_cascade_given = true;
        else if (!std::strcmp(argv[i], "--probe-scroll")) {
            int n = 0;
            probe_scroll_given = probe_tail.scroll_on = true;
            const char* v = need("--probe-scroll");
            probe_scroll_ok = std::sscanf(v, "%d,%d,%d%n", &probe_tail.scroll[0], &probe_tail.scroll[1], &probe_tail.scroll[2], &n) == 3 && v[n] == 0;
        } else if (!std::strcmp(argv[i], "--probe-scroll-after")) probe_tail.scroll_after = std::atoi(need("--probe-scroll-after")), probe_scroll_given = true;
        else if (!std::strcmp(argv[i], "--probe-bounces")) probe_tail.bounces = std::atoi(need("--probe-bounces")), probe_bounces_given = true;
        else if (!std::strcmp(argv[i], "--probe-samples")) probe_update.samples = std::atoi(need("--probe-samples")), probe_update_option = true;
        else if (!std::strcmp(argv[i], "--adaptive")) adaptive = std::atoi(need("--adaptive")), adaptive_given = true;
        else if (!std::strcmp(argv[i], "--adaptive-threshold")) adaptive_threshold = std::strtof(need("--adaptive-threshold"), nullptr), adaptive_threshold_given = true;
        else if (!std::strcmp(argv[i], "--adaptive-max")) adaptive_max = std::atoi(need("--adaptive-max")), adaptive_max_given = true;
        else if (!std::strcmp(argv[i], "--counts-out")) counts_out = need("--counts-out");
        else if (!std::strcmp(argv[i], "--ao")) ao = std::atoi(need("--ao")), ao_given = true;
        else if (!std::strcmp(argv[i], "--ao-radius")) ao_radius = std::strtof(need("--ao-radius"), nullptr);
        else if (!std::strcmp(argv[i], "--sun-visibility")) sun_visibility = true;
        else if (!std::strcmp(argv[i], "--vis-out")) vis_out = need("--vis-out");
        else if (!std::strcmp(argv[i], "--reflection-guides")) reflection_guides = true;
        else if (!std::strcmp(argv[i], "--mirror-history")) mirror_history = true;
        else if (!std::strcmp(argv[i], "--mirror-radius")) mirror_radius = (float)std::atof(need("--mirror-radius")), mirror_radius_given = true;
        else if (!std::strcmp(argv[i], "--reflection-bounces")) reflection_bounces = std::atoi(need("--reflection-bounces")), reflection_bounces_given = true;
        else if (!std::strcmp(argv[i], "--reflection-out")) reflection_out = need("--reflection-out");
        else if (!std::strcmp(argv[i], "--temporal")) temporal = std::atoi(need("--temporal"));
        else if (!std::strcmp(argv[i], "--turn")) turn_deg = std::strtof(need("--turn"), nullptr);
        else if (!std::strcmp(argv[i], "--move")) {
            const char* p = need("--move");
            for (int k = 0; k < 3; ++k) {
                char* end = nullptr;
                move[k] = std::strtof(p, &end);
                if (end == p || (k < 2 && *end != ',') || (k == 2 && *end)) {
                    std::fprintf(stderr, "--move wants R,U,F\n");
                    return 2;
                }
                p = end + 1;
            }
        }
        else if (!std::strcmp(argv[i], "--move-object")) {
            const char* p = need("--move-object");
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
            object_moves.push_back(m);
        }
        else {
            usage();
            return 2;
        }
    }
    if (!object_moves.empty() && !temporal && !probe_update_given) {
        std::fprintf(stderr, "--move-object needs --temporal or --probe-update\n");
        return 2;
    }
    if (refit && object_moves.empty()) {
        std::fprintf(stderr, "--refit needs --move-object\n");
        return 2;
    }
    if (scene_path.empty() || W <= 0 || H <= 0 || spp <= 0 || temporal < 0 || steps < 1) {
        usage();
        return 2;
    }
    if (rays_in.empty() != rays_out.empty() || ((rays_normalize || rays_any_hit) && rays_in.empty())) {
        std::fprintf(stderr, "--rays, --rays-out, --rays-normalize and --any-hit go together: --rays IN.f32 --rays-out OUT.bin [--rays-normalize] [--any-hit]\n");
        return 2;
    }
    srt_probe_grid probe_grid{};
    int probe_grid_directions = 0;
    if (probe_depth_given || probe_depth_option) {
        if (probe_grid_arg.empty() || !probe_depth_given) {
            std::fprintf(stderr, "--probe-depth R and its options go with --probe-grid: --probe-grid G --probe-depth R [--probe-depth-sharpness S] [--probe-depth-max D] "
                                 "[--probe-depth-bias B] [--probe-depth-out FILE]\n");
            return 2;
        }
        if (probe_visibility) {
            std::fprintf(stderr, "--probe-depth and --probe-visibility exclude each other: the filtered or the exact test\n");
            return 2;
        }
        if ((probe_depth.resolution != 4 && probe_depth.resolution != 8 && probe_depth.resolution != 16) || probe_depth.sharpness < 0 || probe_depth.sharpness > 6 ||
            !(probe_depth.max_distance > 0.0f) || !std::isfinite(probe_depth.max_distance) || !(probe_depth.bias >= 0.0f) || !std::isfinite(probe_depth.bias)) {
            std::fprintf(stderr, "--probe-depth takes 4, 8 or 16, --probe-depth-sharpness 0..6, --probe-depth-max a finite distance > 0 and --probe-depth-bias a finite "
                                 "value >= 0\n");
            return 2;
        }
    }
    if (probe_classify.on || probe_classify_option) {
        if (probe_grid_arg.empty() || !probe_classify.on) {
            std::fprintf(stderr, "--probe-classify and its options go with --probe-grid: --probe-grid G --probe-classify [--probe-relocate] [--probe-clearance C] "
                                 "[--probe-max-offset F] [--probe-steps M] [--states-out FILE]\n");
            return 2;
        }
        if (probe_visibility) {
            std::fprintf(stderr, "--probe-classify and --probe-visibility exclude each other: the exact test towards relocated probes is not available\n");
            return 2;
        }
        if (!(probe_classify.clearance > 0.0f) || !(probe_classify.clearance <= 0.5f) || !(probe_classify.max_offset > 0.0f) || !(probe_classify.max_offset <= 0.5f) ||
            probe_classify.steps < 1 || probe_classify.steps > 64) {
            std::fprintf(stderr, "--probe-classify: --probe-clearance and --probe-max-offset take a value in (0, 0.5], --probe-steps 1..64\n");
            return 2;
        }
    }
    if (probe_update_given || probe_update_option) {
        if (!probe_update_given || !probe_classify.on || probe_grid_arg.empty()) {
            std::fprintf(stderr, "--probe-update and its options go with --probe-grid G --probe-classify: --probe-update FRAMES [--probe-hysteresis H] [--probe-samples N]\n");
            return 2;
        }
        if (probe_update.frames < 1 || probe_update.frames > 4096 || probe_update.samples < 1 || probe_update.samples > 4096 || !(probe_update.hysteresis >= 0.0f) ||
            !(probe_update.hysteresis < 1.0f)) {
            std::fprintf(stderr, "--probe-update takes 1..4096 frames, --probe-samples 1..4096, --probe-hysteresis a value in [0, 1)\n");
            return 2;
        }
    }
    if (probe_tail.frame) {
        if (!probe_tail.on || probe_grid_arg.empty() || !devices.empty() || temporal || adaptive_given || steps > 1) {
            std::fprintf(stderr, "--probe-tail-frame goes with --probe-grid ... --probe-tail; not with --devices, --temporal, --adaptive or --steps\n");
            return 2;
        }
        if (spp < 1) {
            std::fprintf(stderr, "--probe-tail-frame: --spp must be >= 1\n");
            return 2;
        }
        probe_tail.frame_spp = spp, probe_tail.frame_out = out;
    }
    srt_probe_grid tail_grid{};
    if (probe_cascade_given && (probe_grid_arg.empty() || probe_cascade_levels < 1 || probe_cascade_levels > SRT_PROBE_CASCADE_MAX_LEVELS ||
                                !(probe_cascade_blend > 0.0f) || !std::isfinite(probe_cascade_blend) || probe_visibility || probe_update_given || probe_tail.on ||
                                !object_moves.empty() || !probe_depth.out.empty() || !probe_classify.out.empty())) {
        std::fprintf(stderr, "--probe-cascade L (1..4) [--probe-cascade-blend B, finite and > 0] goes with --probe-grid, not with --probe-visibility, --probe-update, "
                             "--probe-tail, --move-object, --probe-depth-out or --states-out\n");
        return 2;
    }
    if (probe_scroll_given && (probe_grid_arg.empty() || !probe_feedback_given || !probe_tail.scroll_on || !probe_scroll_ok || probe_tail.scroll_after < 1 ||
                               probe_tail.scroll_after > probe_tail.feedback)) {
        std::fprintf(stderr, "--probe-scroll SX,SY,SZ (three integers) goes with --probe-grid ... --probe-feedback F, and --probe-scroll-after takes a round in 1..F\n");
        return 2;
    }
    if (probe_tail.on || probe_tail.depth || probe_tail.states || probe_tail.normal_weight || probe_feedback_given || probe_bounces_given ||
        !probe_tail.grid.empty() || !probe_tail.coefficients.empty()) {
        if (!probe_grid_arg.empty()) {  // the --probe-grid flow: feedback rounds
            if (!probe_tail.grid.empty() || !probe_tail.coefficients.empty() || probe_update_given) {
                std::fprintf(stderr, "--probe-tail with --probe-grid reads the flow's own grid and history: no --probe-tail-grid / --probe-tail-coefficients, not with --probe-update\n");
                return 2;
            }
            if (!probe_feedback_given) probe_tail.feedback = 2;
            if (probe_tail.feedback < 1 || probe_tail.feedback > 4096 || (probe_bounces_given && probe_tail.bounces < 0)) {
                std::fprintf(stderr, "--probe-feedback takes 1..4096 rounds and --probe-bounces a count >= 0\n");
                return 2;
            }
            if ((probe_tail.depth && !probe_depth_given) || (probe_tail.states && !probe_classify.on)) {
                std::fprintf(stderr, "--probe-tail-depth needs --probe-depth R and --probe-tail-states needs --probe-classify\n");
                return 2;
            }
            probe_tail.on = true;
        } else {  // --rays --radiance N
            if (!probe_tail.on || rays_in.empty() || !radiance_given || probe_tail.depth || probe_tail.states || probe_feedback_given || probe_bounces_given ||
                probe_tail.grid.empty() || probe_tail.coefficients.empty() || !parse_probe_grid(probe_tail.grid.c_str(), &tail_grid)) {
                std::fprintf(stderr, "--probe-tail goes with --probe-grid, or with --rays --radiance N --probe-tail-grid G --probe-tail-coefficients FILE.f32 "
                                     "[--probe-tail-normal-weight] (depth maps, records and --probe-feedback exist in the --probe-grid flow only)\n");
                return 2;
            }
        }
    }
    if (!probe_grid_arg.empty() || !irradiance_out.empty() || probe_visibility || probe_normal_weight || probe_albedo || probe_hemisphere) {
        if (probe_grid_arg.empty()) {
            std::fprintf(stderr, "--irradiance-out, --probe-visibility, --probe-normal-weight, --probe-albedo and --probe-hemisphere need --probe-grid\n");
            return 2;
        }
        if (!parse_probe_grid(probe_grid_arg.c_str(), &probe_grid)) {
            std::fprintf(stderr, "--probe-grid wants OX,OY,OZ,SX,SY,SZ,NX,NY,NZ: a finite origin, finite spacings > 0, integer counts >= 1, at most 2^30 probes\n");
            return 2;
        }
        if (irradiance_out.empty()) {
            std::fprintf(stderr, "--probe-grid needs --irradiance-out FILE\n");
            return 2;
        }
        if (!rays_in.empty() || !probes_in.empty() || !probes_out.empty() || !probe_radiance_out.empty() || temporal || !devices.empty()) {
            std::fprintf(stderr, "--probe-grid shades a frame from light probes: single device, not with %s\n",
                         !rays_in.empty() ? "--rays" : temporal ? "--temporal" : !devices.empty() ? "--devices" : "--probes");
            return 2;
        }
        probe_grid_directions = probe_directions.find_first_not_of("0123456789") == std::string::npos ? std::atoi(probe_directions.c_str()) : 0;
        if (probe_directions.empty() || probe_grid_directions < 1 || probe_grid_directions > (int)SRT_LIGHT_PROBE_MAX_DIRECTIONS) {
            std::fprintf(stderr, "--probe-grid needs --probe-directions K with K in 1..4096\n");
            return 2;
        }
        if ((radiance_given && (radiance < 1 || radiance > 4096)) || bounces < 0) {
            std::fprintf(stderr, "--probe-grid: --radiance N takes 1..4096 samples and --bounces must be >= 0\n");
            return 2;
        }
        if (steps > 1 || aa_given || !gbuffer.empty() || !denoise.empty() || !upsample.empty() || !denoise_variance.empty() || adaptive_given || ao_given ||
            sun_visibility || !vis_out.empty() || reflection_guides || !reflection_out.empty()) {
            std::fprintf(stderr, "--probe-grid shades a frame from light probes instead of rendering it: no other frame options\n");
            return 2;
        }
    }
    if (radiance_given && probes_in.empty() && probe_grid_arg.empty() && (rays_in.empty() || rays_any_hit || radiance < 1 || radiance > 4096 || bounces < 0)) {
        std::fprintf(stderr, "--radiance N (1..4096) needs --rays and --rays-out, a --bounces >= 0, and does not go with --any-hit\n");
        return 2;
    }
    if (!probes_in.empty() || !probes_out.empty() || (!probe_directions.empty() && probe_grid_arg.empty()) || !probe_radiance_out.empty()) {
        if (probes_in.empty() || probes_out.empty() || probe_directions.empty()) {
            std::fprintf(stderr, "--probes, --probe-directions, --probes-out and --probe-radiance-out go together: --probes IN.f32 --probe-directions K|FILE.f32 "
                                 "--probes-out OUT.bin [--radiance N] [--probe-radiance-out FILE]\n");
            return 2;
        }
        if ((radiance_given && (radiance < 1 || radiance > 4096)) || bounces < 0) {
            std::fprintf(stderr, "--probes: --radiance N takes 1..4096 samples and --bounces must be >= 0\n");
            return 2;
        }
        if (!rays_in.empty() || !devices.empty() || temporal || steps > 1 || aa_given || !gbuffer.empty() || !denoise.empty() || !upsample.empty() ||
            !denoise_variance.empty() || adaptive_given || ao_given || sun_visibility || !vis_out.empty() || reflection_guides || !reflection_out.empty()) {
            std::fprintf(stderr, "--probes traces light probes instead of rendering a frame: single device, not with --rays, no frame options\n");
            return 2;
        }
    }
    if (!rays_in.empty() && (!devices.empty() || temporal || steps > 1 || aa_given || !gbuffer.empty() || !denoise.empty() || !upsample.empty() ||
                             !denoise_variance.empty())) {
        std::fprintf(stderr, "--rays answers ray queries instead of rendering a frame: single device, no frame options\n");
        return 2;
    }
    if ((ao_given || sun_visibility) == vis_out.empty() || (ao_given && (ao < 1 || ao > 4096)) || (!ao_given && ao_radius != INFINITY) || !(ao_radius > 0) ||
        (!vis_out.empty() && (!devices.empty() || temporal || !rays_in.empty()))) {
        std::fprintf(stderr, "--ao N (1..4096) [--ao-radius R > 0] and --sun-visibility need --vis-out FILE and the other way round; single device, "
                             "not with --temporal or --rays\n");
        return 2;
    }
    if (reflection_guides || reflection_bounces_given || !reflection_out.empty()) {
        if ((reflection_guides && denoise.empty() && denoise_variance.empty()) || (reflection_bounces_given && !reflection_guides && reflection_out.empty()) ||
            reflection_bounces < 0 || reflection_bounces > 64 || !devices.empty() || temporal || !rays_in.empty() || adaptive_given) {
            std::fprintf(stderr, "--reflection-guides needs --denoise or --denoise-variance; --reflection-bounces N (0..64) needs --reflection-guides or "
                                 "--reflection-out; single device, not with --devices, --temporal, --rays or --adaptive\n");
            return 2;
        }
    }
    if ((mirror_history && !temporal) || (mirror_radius_given && (!mirror_history || !(mirror_radius > 0.0f)))) {
        std::fprintf(stderr, "--mirror-history needs --temporal; --mirror-radius R (> 0) needs --mirror-history\n");
        return 2;
    }
    if (temporal_variance && (!temporal || !devices.empty() || steps > 1 || !upsample.empty())) {
        std::fprintf(stderr, "--temporal-variance needs --temporal and works on one device only, not with --steps or --upsample\n");
        return 2;
    }
    if (!denoise.empty() && !devices.empty()) {
        std::fprintf(stderr, "--denoise works on one device only: the accumulator bands of --devices live on different GPUs\n");
        return 2;
    }
    if ((steps > 1 || !upsample.empty()) && (!devices.empty() || temporal)) {
        std::fprintf(stderr, "--steps and --upsample work on one device only and not with --temporal\n");
        return 2;
    }
    if (!denoise_variance.empty()) {
        if (!denoise.empty()) {
            std::fprintf(stderr, "--denoise-variance and --denoise exclude each other: both write the denoised buffer\n");
            return 2;
        }
        if (spp < 2 || (spp & 1)) {
            std::fprintf(stderr, "--denoise-variance needs an even --spp >= 2: it renders two halves of --spp / 2 samples\n");
            return 2;
        }
        if (!devices.empty() || temporal || steps > 1 || !upsample.empty()) {
            std::fprintf(stderr, "--denoise-variance works on one device only and not with --temporal, --steps or --upsample\n");
            return 2;
        }
    }
    if (!adaptive_given && (adaptive_threshold_given || adaptive_max_given || !counts_out.empty())) {
        std::fprintf(stderr, "--adaptive-threshold, --adaptive-max and --counts-out need --adaptive ROUNDS\n");
        return 2;
    }
    if (adaptive_given) {
        if (adaptive < 1 || adaptive > 64 || spp < 2 || (spp & 1) || bounces < 0 || (adaptive_threshold_given && !(adaptive_threshold > 0)) ||
            (adaptive_max_given && (adaptive_max < 1 || adaptive_max > 4096))) {
            std::fprintf(stderr, "--adaptive ROUNDS (1..64) needs an even --spp >= 2 and a --bounces >= 0; --adaptive-threshold T > 0; --adaptive-max M in 1..4096\n");
            return 2;
        }
        if (!devices.empty() || temporal || steps > 1 || aa_given || !upsample.empty() || !denoise.empty() || !denoise_variance.empty() || !rays_in.empty() ||
            !vis_out.empty()) {
            std::fprintf(stderr, "--adaptive renders the frame itself: single device, not with --devices, --temporal, --steps, --aa, --upsample, --denoise, "
                                 "--denoise-variance, --rays, --ao or --sun-visibility\n");
            return 2;
        }
    }
    if (aa_given && (aa < 1 || aa > 4 || !devices.empty())) {
        std::fprintf(stderr, "--aa takes K in 1..4 and works on one device only\n");
        return 2;
    }
    if (temporal && !devices.empty()) {
        std::fprintf(stderr, "--temporal works on one device only: the history of --devices would be split over different GPUs\n");
        return 2;
    }
    Scene scene(scene_path);
    scene.Load();
    if (!scene.lastError().empty()) std::fprintf(stderr, "scene: %s\n", scene.lastError().c_str());  // Scene.hpp:76
    std::fprintf(stderr, "scene %s: %zu objects\n", scene_path.c_str(), scene.GetObjects().size());
    if (!resave.empty()) scene.SaveAs(resave);
    for (const auto& m : object_moves)
        if (m.index >= scene.GetObjects().size()) {
            std::fprintf(stderr, "--move-object: the scene has no object %zu\n", m.index);
            return 2;
        }
    if (!probe_grid_arg.empty() && probe_cascade_levels)
        return shade_probe_cascade_file(scene, device, W, H, fov, probe_grid, probe_cascade_levels, probe_cascade_blend, probe_grid_directions,
                                        radiance_given ? radiance : 16, bounces, seed,
                                        (probe_normal_weight ? SRT_PROBE_GRID_NORMAL_WEIGHT : 0u) | (probe_albedo ? SRT_PROBE_GRID_ALBEDO : 0u), probe_hemisphere,
                                        irradiance_out, probe_depth, probe_classify);
    if (!probe_grid_arg.empty())
        return shade_probe_grid_file(scene, device, W, H, fov, probe_grid, probe_grid_directions, radiance_given ? radiance : 16, bounces, seed,
                                     (probe_visibility ? SRT_PROBE_GRID_VISIBILITY : 0u) | (probe_normal_weight ? SRT_PROBE_GRID_NORMAL_WEIGHT : 0u) |
                                         (probe_albedo ? SRT_PROBE_GRID_ALBEDO : 0u),
                                     probe_hemisphere, irradiance_out, probe_depth, probe_classify, probe_update, object_moves, probe_tail);
    if (!probes_in.empty()) return trace_probe_file(scene, device, probes_in, probe_directions, probes_out, probe_radiance_out, radiance_given ? radiance : 16, bounces, seed);
    if (!rays_in.empty()) {
        RayTail ray_tail;
        if (probe_tail.on) {
            ray_tail.coefficients = read_float4_file(probe_tail.coefficients);
            const size_t np = (size_t)tail_grid.counts[0] * (size_t)tail_grid.counts[1] * (size_t)tail_grid.counts[2];
            if (ray_tail.coefficients.size() != np * 36) {
                std::fprintf(stderr, "--probe-tail-coefficients: want %zu probes x 9 float4 for the grid of --probe-tail-grid\n", np);
                return 2;
            }
            ray_tail.grid = &tail_grid, ray_tail.flags = probe_tail.flags();
        }
        return trace_ray_file(scene, device, rays_in, rays_out, rays_normalize, rays_any_hit, radiance_given ? radiance : 0, bounces, seed, ray_tail);
    }
    auto write_ppm = [&](const std::vector<uint32_t>& fb, const std::string& path) { return write_ppm_file(fb, W, H, path); };
    if (!devices.empty()) {
        try {
            MultiGpuRenderer m(devices, W, H);
            m.SetScene(scene);
            m.Configure(Transform(), fov, bounces, seed);
            if (equal_bands) m.UseEqualBands(true);
            auto t0 = std::chrono::steady_clock::now();
            m.RenderSamples((uint32_t)spp, true);
            std::vector<uint32_t> fb((size_t)W * H);
            m.ReadFramebuffer(fb.data(), (size_t)W * 4);
            double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            std::vector<srt_stats> st = m.Stats();
            double slowest = 0;
            for (size_t i = 0; i < st.size(); ++i) {
                int b, e;
                m.Band(i, &b, &e);
                std::fprintf(stderr, "  part %zu (device %d, memory rows %d-%d): kernel %.3f ms, %.2f rays/sample\n", i, devices[i], b, e, st[i].kernel_ms,
                             (double)st[i].rays / (double)st[i].path_samples);
                slowest = st[i].kernel_ms > slowest ? st[i].kernel_ms : slowest;
            }
            std::fprintf(stderr, "%dx%d spp=%d bounces=%d over %zu parts: slowest kernel %.3f ms, render + gather + read-back wall %.3f ms\n", W, H, spp, bounces,
                         st.size(), slowest, wall * 1e3);
            if (write_ppm(fb, out)) return 1;
            if (!gbuffer.empty() && write_gbuffers(m, gbuffer, W, H)) return 1;
            return 0;
        } catch (const std::exception& e) {
            std::fprintf(stderr, "error: %s\n", e.what());
            return 1;
        }
    }
    try {
        PathTraceRenderer r(device, W, H);
        r.FOV = fov;
        r.MAXBOUNCES = bounces;
        r.seed = seed;
        r.refitUpdates = refit;
        r.SetScene(scene);
        // --aa: the stage's result resolved into the framebuffer before it is read (the sub-samples are traced once per camera)
        auto resolve = [&](int source) {
            if (aa) r.Antialias(aa, source, SRT_AA_FRAMEBUFFER);
        };
        if (temporal) {
            r.antialias = aa;  // every temporal frame ends in the resolve
            r.temporalVariance = temporal_variance;  // every temporal frame keeps the moments
            if (mirror_history) {  // every temporal frame reprojects through the mirrors
                if (mirror_radius_given) r.mirrorRadius = mirror_radius;
                r.mirrorHistory(true);
            }
            // a moving camera that keeps its samples: every frame renders spp samples, reprojects the history and writes the
            // framebuffer; each frame's camera is printed exactly (%.9g round-trips a float) so that callers can replay it
            std::vector<uint32_t> fb((size_t)W * H);
            const Vec3 world_up(0, 1, 0);
            const float turn = (float)(turn_deg * 3.14159265358979323846 / 180.0);
            auto t0 = std::chrono::steady_clock::now();
            for (int k = 0; k < temporal; ++k) {
                if (k > 0) {
                    Transform& c = r.camera;
                    c.position = c.position + c.right * move[0] + c.up * move[1] + c.forward * move[2];
                    if (turn != 0) c.RotateAboutAxis(turn, world_up);
                    // object edits: each moved object's position is printed exactly, like the camera
                    for (const auto& m : object_moves) {
                        float* pos = scene.Objects()[m.index].position;
                        for (int a = 0; a < 3; ++a) pos[a] = pos[a] + m.step[a];
                    }
                    if (!object_moves.empty()) r.UpdateScene(scene);
                    if (refit) {
                        const srt_update_info u = r.UpdateInfo();
                        std::fprintf(stderr, "temporal frame %d update path %d reason %d levels %d triangles %u nodes %u\n", k, u.path, u.reason, u.levels,
                                     u.triangles, u.nodes);
                    }
                }
                for (const auto& m : object_moves) {
                    const float* pos = scene.GetObjects()[m.index].position;
                    std::fprintf(stderr, "temporal frame %d object %zu position %.9g %.9g %.9g\n", k, m.index, pos[0], pos[1], pos[2]);
                }
                const Transform& c = r.camera;
                std::fprintf(stderr, "temporal frame %d camera %.9g %.9g %.9g  %.9g %.9g %.9g  %.9g %.9g %.9g  %.9g %.9g %.9g\n", k, c.position.x,
                             c.position.y, c.position.z, c.right.x, c.right.y, c.right.z, c.up.x, c.up.y, c.up.z, c.forward.x, c.forward.y,
                             c.forward.z);
                r.RenderTemporalFrame((uint32_t)spp, false);
            }
            r.Wait();
            double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            std::fprintf(stderr, "%dx%d spp=%d bounces=%d: %d temporal frames, wall %.3f ms\n", W, H, spp, bounces, temporal, wall * 1e3);
            r.ReadFramebuffer(fb.data(), (size_t)W * 4);
            if (write_ppm(fb, out)) return 1;
            if (!gbuffer.empty() && write_gbuffers(r, gbuffer, W, H)) return 1;
            if (!denoise.empty()) {
                // the last frame's accumulator (the reprojected result) through the denoiser, as RenderTemporalFrame(spp, true) does
                srt_denoise_params dp{};
                srt_denoise_params_default(&dp);
                dp.flags |= SRT_DENOISE_FRAMEBUFFER;
                r.RenderGBuffer(SRT_GBUF_ALL);
                // --temporal-variance: the variance of the history's moments and the variance-guided filter in its place
                if (temporal_variance) r.DenoiseTemporalVariance(SRT_DENOISE_FRAMEBUFFER);
                else r.Denoise(dp);
                resolve(SRT_AA_SOURCE_DENOISED);
                r.ReadFramebuffer(fb.data(), (size_t)W * 4);
                if (write_ppm(fb, denoise)) return 1;
            }
            return 0;
        }
        if (adaptive_given) {
            // the uniform seed in two halves, the rounds, the merge (PathTraceRenderer::renderAdaptiveFrame); --out is the merged
            // accumulator through SetScreenPixel's tone map (memory row H - 1 - y), which no kernel has written for the mean
            srt_budget_params bp{};
            srt_budget_params_default(&bp);
            if (adaptive_threshold_given) bp.threshold = adaptive_threshold;
            if (adaptive_max_given) bp.max_budget = (uint32_t)adaptive_max;
            std::vector<uint32_t> counts;
            auto t0 = std::chrono::steady_clock::now();
            const uint64_t total = r.renderAdaptiveFrame((uint32_t)spp, adaptive, bp, bp.max_budget, &counts);
            double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            std::fprintf(stderr, "%dx%d spp=%d bounces=%d adaptive rounds=%d threshold=%g max=%u: total samples %llu (%.2f per pixel), wall %.3f ms\n", W, H, spp,
                         bounces, adaptive, (double)bp.threshold, bp.max_budget, (unsigned long long)total, (double)total / ((double)W * H), wall * 1e3);
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
            if (write_ppm(fb, out)) return 1;
            if (!gbuffer.empty() && write_gbuffers(r, gbuffer, W, H)) return 1;
            if (!counts_out.empty()) {
                FILE* g = std::fopen(counts_out.c_str(), "wb");
                if (!g) {
                    std::perror(counts_out.c_str());
                    return 1;
                }
                bool ok = std::fwrite(counts.data(), sizeof(uint32_t), counts.size(), g) == counts.size();
                ok = (std::fclose(g) == 0) && ok;
                if (!ok) {
                    std::fprintf(stderr, "%s: write failed\n", counts_out.c_str());
                    return 1;
                }
            }
            return 0;
        }
        auto t0 = std::chrono::steady_clock::now();
        r.RenderSamples((uint32_t)spp, true, steps);
        r.Wait();
        double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        srt_stats st = r.Stats();
        std::fprintf(stderr, "%dx%d spp=%d bounces=%d: kernel %.3f ms (wall %.3f ms), %.3e path-samples/s, %.2f rays/sample\n", W, H, spp,
                     bounces, st.kernel_ms, wall * 1e3, (double)st.path_samples / (st.kernel_ms * 1e-3),
                     (double)st.rays / (double)st.path_samples);
        std::vector<uint32_t> fb((size_t)W * H);
        resolve(SRT_AA_SOURCE_ACCUMULATOR);
        r.ReadFramebuffer(fb.data(), (size_t)W * 4);
        if (write_ppm(fb, out)) return 1;
        if (!gbuffer.empty() && write_gbuffers(r, gbuffer, W, H)) return 1;
        if (!vis_out.empty()) {
            // the guides of the whole frame, then the visibility pass; the planes asked for follow each other in the file, AO first
            srt_visibility_params vp{};
            srt_visibility_params_default(&vp);
            vp.outputs = (ao_given ? SRT_VIS_AO : 0u) | (sun_visibility ? SRT_VIS_SUN : 0u);
            if (ao_given) vp.ao_samples = (uint32_t)ao, vp.ao_radius = ao_radius;
            vp.seed = seed;
            r.renderVisibility(vp);
            FILE* g = std::fopen(vis_out.c_str(), "wb");
            if (!g) {
                std::perror(vis_out.c_str());
                return 1;
            }
            bool ok = true;
            std::vector<float> plane((size_t)W * H);
            for (uint32_t bit = SRT_VIS_AO; bit <= SRT_VIS_SUN; bit <<= 1) {
                if (!(vp.outputs & bit)) continue;
                r.readVisibility(bit, plane.data());
                ok = ok && std::fwrite(plane.data(), sizeof(float), plane.size(), g) == plane.size();
            }
            ok = (std::fclose(g) == 0) && ok;
            if (!ok) {
                std::fprintf(stderr, "%s: write failed\n", vis_out.c_str());
                return 1;
            }
        }
        if (!upsample.empty()) {
            // the guides of the whole frame, then the blocks' anchors interpolated with the library's defaults; the kernel
            // tone-maps its result into the framebuffer (--out is already written).  With --denoise the result replaces the
            // accumulator's non-anchor pixels, which is what the denoiser below then filters — and with --aa too, whose resolve
            // reads the accumulator.
            srt_upsample_params up{};
            srt_upsample_params_default(&up);
            up.steps = steps;
            up.flags = SRT_UPSAMPLE_FRAMEBUFFER | (denoise.empty() && !aa ? 0u : SRT_UPSAMPLE_IN_PLACE);
            r.RenderGBuffer(SRT_GBUF_OBJECT | SRT_GBUF_NORMAL_DEPTH | SRT_GBUF_POSITION);
            r.Upsample(up);
            resolve(SRT_AA_SOURCE_ACCUMULATOR);
            r.ReadFramebuffer(fb.data(), (size_t)W * 4);
            if (write_ppm(fb, upsample)) return 1;
        }
        if (!reflection_out.empty() && write_reflection(r, reflection_out, W, H, reflection_bounces)) return 1;
        // --reflection-guides: from here on RenderGBuffer renders the reflection guides into the G-buffer slots (--gbuffer, the
        // visibility pass and the upsampler above have had their first hits; --aa's resolve keeps first hits by itself)
        if (reflection_guides) r.reflectionBounces = reflection_bounces, r.reflectionGuides(true);
        if (!denoise.empty()) {
            // the guides of the whole frame, then the filter with the library's defaults; the kernel tone-maps its result into
            // the framebuffer (--out is already written), read back top-down like --out
            srt_denoise_params dp{};
            srt_denoise_params_default(&dp);
            dp.flags |= SRT_DENOISE_FRAMEBUFFER;
            r.RenderGBuffer(SRT_GBUF_ALL);
            r.Denoise(dp);
            resolve(SRT_AA_SOURCE_DENOISED);
            r.ReadFramebuffer(fb.data(), (size_t)W * 4);
            if (write_ppm(fb, denoise)) return 1;
        }
        if (!denoise_variance.empty()) {
            // the frame again as two halves, their variance and mean, the guides and the variance-guided filter with the
            // library's defaults (PathTraceRenderer::denoiseVariance); the kernel tone-maps its result into the framebuffer
            // (--out is already written)
            r.denoiseVariance((uint32_t)spp, SRT_DENOISE_FRAMEBUFFER);
            resolve(SRT_AA_SOURCE_DENOISED);
            r.ReadFramebuffer(fb.data(), (size_t)W * 4);
            if (write_ppm(fb, denoise_variance)) return 1;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
