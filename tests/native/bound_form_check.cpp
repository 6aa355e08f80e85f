// The cluster bound test of closest_hit (csrc/srt_kernel.hip.h) in the form about the ray's foot point, against the reference's
// candidate test of every member sphere: a culled cluster must not hold a candidate.  The scene images — bound rows, the reference
// point G and the scene-wide scalars — are built by the library's own build_scene_image (csrc/srt_scene_image.h, which has the
// proof this program backs with evidence); the three tests are evaluated in binary32 as the kernel and the reference do
// (fmaf where the kernel has an FMA, plain operations where the reference has them: build with -ffp-contract=off):
//   (a) the reference's candidate test of a member sphere (Object.hpp:115-127, closest_hit's part1), no FMA
//   (b) the cluster test about the origin, rows (C, Rg) at off_bounds: srt_occlusion.hip.h's, closest_hit's until now
//   (c) the cluster test about the foot point, rows (C', K) at off_bounds2
// Scenes: the ones given on the command line, and the random families of tests/test_gpu_fuzz.py (unit, far, tiny, mixed, offset;
// spheres only), each as it is and translated by 1e3 and by 1e5 in x and z.  Origins: on the largest sphere (the floor) out to its
// horizon, inside clusters, around the cluster field, at |o| = 1e4 and 1e8, and in front of spheres that lie BEHIND the ray (the
// reference's |L.d| mirror).  Directions: aimed to graze a member sphere or a cluster's bound within 1e-7 .. 1e-1 of its radius,
// random, axis-parallel, all with |d|^2 = 1 +- 1e-6 (beyond that the kernel does not use the bounds at all); and rays with a NaN or
// an infinity in o or d, which every cluster must pass.
//   bound_form_check [--pairs N] <scene.json>...     N (ray, cluster) pairs at least, default 1e8; the first scene is taken for
//                                                    the recorded figure: the share of clusters that (b) and (c) pass for its own
//                                                    rays (camera rays of the default camera, random bounces off the floor).
// Prints "ok <pairs> pairs, <culled> culled by (c), 0 violations" or the first violations and exit status 1.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "scene.hpp"
#include "srt_scene_image.h"

struct Rng {
    uint64_t s;
    uint64_t next() {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * 0x1p-53; }             // [0, 1)
    double sym() { return 2.0 * uni() - 1.0; }                            // [-1, 1)
    int below(int n) { return (int)(next() % (uint64_t)n); }
    void dir(double v[3]) {  // uniform on the sphere
        double n;
        do {
            v[0] = sym(), v[1] = sym(), v[2] = sym();
            n = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        } while (n > 1.0 || n < 1e-6);
        n = sqrt(n);
        v[0] /= n, v[1] /= n, v[2] /= n;
    }
};

struct Image {
    std::vector<float4> img;
    srt::SceneLayout L;
    const float4* v() const { return img.data() + srt::SRT_CONST_ROWS; }
    int floor_slot = -1;  // the largest uniform sphere
};

static Image build(const std::vector<srt_object>& objs) {
    Image I;
    I.L = srt::build_scene_image(objs.data(), objs.size(), true, I.img);
    float best = 0;
    for (int p = 0; p < I.L.nu; ++p)
        if (I.v()[p].w > best && std::isfinite(I.v()[p].w)) best = I.v()[p].w, I.floor_slot = p;
    return I;
}

// (a) closest_hit's part1, Object.hpp:115-127
static bool candidate(const float4 s, const float o[3], const float d[3]) {
    float Lx = s.x - o[0], Ly = s.y - o[1], Lz = s.z - o[2];
    float tc = fabsf((Lx * d[0] + Ly * d[1]) + Lz * d[2]);
    float qx = d[0] * tc + o[0], qy = d[1] * tc + o[1], qz = d[2] * tc + o[2];
    float ex = qx - s.x, ey = qy - s.y, ez = qz - s.z;
    float d2 = (ex * ex + ey * ey) + ez * ez;
    return !(d2 > s.w);
}

// (b) the test about the origin
static bool passes_old(const float4 b, const float o[3], const float d[3]) {
    const float o1 = (fabsf(o[0]) + fabsf(o[1])) + fabsf(o[2]);
    float Lx = b.x - o[0], Ly = b.y - o[1], Lz = b.z - o[2];
    float LL = fmaf(Lz, Lz, fmaf(Ly, Ly, Lx * Lx));
    float sd = fmaf(Lz, d[2], fmaf(Ly, d[1], Lx * d[0]));
    float Rinf = fmaf(8e-6f, o1, b.w);
    float lhs = fmaf(-sd, sd, LL);
    float rhs = fmaf(4e-6f, LL, Rinf * Rinf);
    return lhs <= rhs;
}

// (c) the test about the foot point: the per-ray part and the per-cluster part, as closest_hit writes them
struct RayPart {
    float w2x, w2y, w2z, T;
};
static RayPart ray_part(const srt::SceneLayout& L, const float o[3], const float d[3]) {
    const float ox = o[0] - L.G[0], oy = o[1] - L.G[1], oz = o[2] - L.G[2];
    const float od = fmaf(oz, d[2], fmaf(oy, d[1], ox * d[0]));
    const float wx = fmaf(-od, d[0], ox), wy = fmaf(-od, d[1], oy), wz = fmaf(-od, d[2], oz);
    const float WW = fmaf(wz, wz, fmaf(wy, wy, wx * wx));
    const float p1 = (fabsf(ox) + fabsf(oy)) + fabsf(oz);
    const float Mb = fmaf(2.1f, p1, L.cmaxp), ab = fmaf(8.2e-6f, p1, L.aG);
    const float Tb = fmaf(ab, L.Rgmax2 + ab, (1e-5f * Mb) * Mb) - WW;
    return RayPart{2.0f * wx, 2.0f * wy, 2.0f * wz, Tb};
}
static bool passes_new(const float4 b, const RayPart& r, const float d[3]) {
    const float g = fmaf(-b.z, r.w2z, fmaf(-b.y, r.w2y, fmaf(-b.x, r.w2x, b.w)));
    const float e = fmaf(b.z, d[2], fmaf(b.y, d[1], b.x * d[0]));
    const float lhs = fmaf(-e, e, g);
    return !(lhs > r.T);
}

static bool unit(const float d[3]) {
    const float dd = fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]));
    return fabsf(dd - 1.0f) <= 1e-6f;
}

struct Totals {
    unsigned long long pairs = 0, culled = 0, culled_old = 0, violations = 0, violations_old = 0, odd_rays = 0, skipped = 0;
};

// one ray against every cluster; returns false on a violation of (c)
static void check_ray(const Image& I, const float o[3], const float d[3], Totals& t, const char* what) {
    const srt::SceneLayout& L = I.L;
    const float4* v = I.v();
    const RayPart r = ray_part(L, o, d);
    for (int k = 0; k < L.nc; ++k) {
        const bool c = passes_new(v[L.off_bounds2 + k], r, d), b = passes_old(v[L.off_bounds + k], o, d);
        ++t.pairs;
        t.culled += !c, t.culled_old += !b;
        if (c && b) continue;
        bool any = false;
        for (int i = 0; i < L.K; ++i) any = any || candidate(v[L.nu4 + k * L.K + i], o, d);
        if (any && !b) ++t.violations_old;
        if (any && !c) {
            if (t.violations++ < 10)
                printf("VIOLATION (%s): cluster %d culled with a candidate inside; o = (%.9g, %.9g, %.9g), d = (%.9g, %.9g, %.9g)\n", what, k,
                       (double)o[0], (double)o[1], (double)o[2], (double)d[0], (double)d[1], (double)d[2]);
        }
    }
}

// a direction of |d|^2 = 1 +- 1e-6 from any vector; false where the kernel would not use the bounds
static bool make_dir(Rng& g, const double v[3], float d[3]) {
    const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(n > 0) || !std::isfinite(n)) return false;
    const double s = 1.0 + 4.9e-7 * (g.below(3) == 0 ? (g.below(2) ? 1.0 : -1.0) : g.sym());
    for (int a = 0; a < 3; ++a) d[a] = (float)(v[a] / n * s);
    return unit(d);
}

static void rays_of_scene(const Image& I, Rng& g, unsigned long long pairs_wanted, Totals& t) {
    const srt::SceneLayout& L = I.L;
    if (L.nc == 0) return;
    const float4* v = I.v();
    // the extent of the cluster field
    double ext = 0;
    for (int k = 0; k < L.nc; ++k) {
        const float4 b = v[L.off_bounds2 + k];
        ext = std::max(ext, sqrt((double)b.x * b.x + (double)b.y * b.y + (double)b.z * b.z) + (double)v[L.off_bounds + k].w);
    }
    const unsigned long long until = t.pairs + pairs_wanted;
    while (t.pairs < until) {
        // a target: a point that grazes a member sphere, or a cluster's bound
        const int k = g.below(L.nc);
        float4 s = v[L.nu4 + k * L.K + g.below(L.K)];
        if (!(s.w >= 0)) s = v[L.nu4 + k * L.K];  // (padding: the cluster's first sphere is real)
        double r = sqrt((double)s.w), c[3] = {s.x, s.y, s.z};
        if (g.below(4) == 0) {
            const float4 b = v[L.off_bounds + k];
            r = b.w, c[0] = b.x, c[1] = b.y, c[2] = b.z;
        }
        double u[3];
        g.dir(u);
        const double rel = (g.below(2) ? 1.0 : -1.0) * pow(10.0, -7.0 * g.uni() - 1.0) * (g.below(8) ? 1.0 : 0.0);
        double target[3], o[3], dv[3];
        for (int a = 0; a < 3; ++a) target[a] = c[a] + u[a] * r * (1.0 + rel);
        // the direction that grazes there is perpendicular to u
        double q[3], along[3];
        g.dir(q);
        along[0] = u[1] * q[2] - u[2] * q[1], along[1] = u[2] * q[0] - u[0] * q[2], along[2] = u[0] * q[1] - u[1] * q[0];
        const int okind = g.below(8), dkind = g.below(8);
        const char* what = "aimed";
        double dist = ext * pow(10.0, 2.0 * g.sym());  // how far the origin lies from the target along the ray
        if (dkind == 0) {  // axis-parallel
            const int ax = g.below(3);
            along[0] = along[1] = along[2] = 0, along[ax] = g.below(2) ? 1.0 : -1.0;
            // graze: put the target beside the centre, perpendicular to the axis
            u[ax] = 0;
            const double n = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
            if (n > 0)
                for (int a = 0; a < 3; ++a) target[a] = c[a] + u[a] / n * r * (1.0 + rel);
            what = "axis";
        }
        if (okind == 0 && I.floor_slot >= 0) {  // on the floor, out to its horizon as seen from the field
            const float4 f = v[I.floor_slot];
            const double R = sqrt((double)f.w);
            double up[3] = {(double)L.G[0] - f.x, (double)L.G[1] - f.y, (double)L.G[2] - f.z};
            const double h = sqrt(up[0] * up[0] + up[1] * up[1] + up[2] * up[2]);
            const double theta = g.uni() * g.uni() * acos(std::min(1.0, R / std::max(h + ext, R)));
            double side[3];
            g.dir(side);
            for (int a = 0; a < 3; ++a) o[a] = f.x * (a == 0) + f.y * (a == 1) + f.z * (a == 2) + R * (cos(theta) * up[a] / h + sin(theta) * side[a]);
            if (dkind != 0)
                for (int a = 0; a < 3; ++a) along[a] = target[a] - o[a];
            else
                for (int a = 0; a < 3; ++a) o[a] = target[a] - along[a] * dist;  // (an axis ray cannot start where it likes)
            what = dkind ? "floor" : "axis";
        } else if (okind == 1) {  // inside a cluster
            dist = r * g.uni();
            for (int a = 0; a < 3; ++a) o[a] = target[a] - along[a] * dist;
            what = "inside";
        } else if (okind == 2 || okind == 3) {  // far out
            dist = okind == 2 ? 1e4 : 1e8;
            for (int a = 0; a < 3; ++a) o[a] = target[a] - along[a] * dist;
            what = okind == 2 ? "1e4" : "1e8";
        } else if (okind == 4) {  // the spheres lie behind the ray
            for (int a = 0; a < 3; ++a) o[a] = target[a] + along[a] * dist;
            what = "behind";
        } else {
            for (int a = 0; a < 3; ++a) o[a] = target[a] - along[a] * dist;
        }
        if (dkind == 1) g.dir(along), what = "random";
        for (int a = 0; a < 3; ++a) dv[a] = along[a];
        float of[3] = {(float)o[0], (float)o[1], (float)o[2]}, df[3];
        if (!make_dir(g, dv, df)) {
            ++t.skipped;
            continue;
        }
        check_ray(I, of, df, t, what);
        if (g.below(64) == 0) {  // a NaN or an infinity somewhere: every cluster passes
            float oo[3] = {of[0], of[1], of[2]}, dd[3] = {df[0], df[1], df[2]};
            const float odd[3] = {NAN, INFINITY, -INFINITY};
            (g.below(2) ? oo : dd)[g.below(3)] = odd[g.below(3)];
            const RayPart rp = ray_part(L, oo, dd);
            ++t.odd_rays;
            for (int kk = 0; kk < L.nc; ++kk)
                if (!passes_new(v[L.off_bounds2 + kk], rp, dd)) {
                    if (t.violations++ < 10)
                        printf("VIOLATION (non-finite): cluster %d culled; o = (%g, %g, %g), d = (%g, %g, %g)\n", kk, (double)oo[0], (double)oo[1],
                               (double)oo[2], (double)dd[0], (double)dd[1], (double)dd[2]);
                }
        }
    }
}

static std::vector<srt_object> translated(const std::vector<srt_object>& objs, float by) {
    std::vector<srt_object> out = objs;
    for (srt_object& o : out) o.position[0] += by, o.position[2] += by;
    return out;
}

// the sphere part of tests/test_gpu_fuzz.py's random scenes
static std::vector<srt_object> family(Rng& g, int kind) {
    const double scale[5] = {1.0, 1.0e4, 1.0e-2, 1.0, 1.0};
    const double off[5][3] = {{0, 0, 6}, {3.0e4, -2.0e4, 5.0e4}, {0, 0, 0.06}, {0, 0, 6}, {2.5e4, -1.5e4, 4.0e4}};
    std::vector<srt_object> objs;
    const int n = 16 + g.below(74);
    for (int i = 0; i < n; ++i) {
        srt_object o{};
        o.type = SRT_OBJ_SPHERE, o.mesh = -1;
        double r = (0.02 + 0.58 * g.uni()) * scale[kind];
        if (kind == 3 && g.uni() < 0.1) r *= (g.below(3) == 0 ? 30.0 : g.below(2) ? 300.0 : -1.0);
        o.radius = (float)r;
        for (int a = 0; a < 3; ++a) o.position[a] = (float)(off[kind][a] + 4.0 * g.sym() * scale[kind]);
        objs.push_back(o);
    }
    return objs;
}

static std::vector<srt_object> load(const char* path) {
    srt_host::Scene s(path);
    s.Load();
    return s.Flatten();
}

// the recorded figure: the first scene's own rays
static void own_rays(const Image& I, Rng& g) {
    const srt::SceneLayout& L = I.L;
    if (L.nc == 0) return;
    Totals cam, bounce;
    const int W = 192, H = 108;
    const double t = tan(55.0 * 0.5 * M_PI / 180.0);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const double dv[3] = {((x + 0.5) / W * 2 - 1) * t * W / H, ((y + 0.5) / H * 2 - 1) * t, 1.0};
            const float o[3] = {0, 0, 0};
            float d[3];
            if (make_dir(g, dv, d)) check_ray(I, o, d, cam, "camera");
        }
    if (I.floor_slot >= 0) {
        const float4 f = I.v()[I.floor_slot];
        const double R = sqrt((double)f.w);
        for (int i = 0; i < 20000; ++i) {  // a point of the floor under the camera's view, a direction of its upper hemisphere
            const double px = 8.0 * g.sym(), pz = 2.0 + 28.0 * g.uni();
            const double dx = px - f.x, dz = pz - f.z, py = f.y + sqrt(std::max(0.0, R * R - dx * dx - dz * dz));
            double dv[3];
            g.dir(dv);
            if (dv[0] * dx + dv[1] * (py - f.y) + dv[2] * dz < 0) dv[0] = -dv[0], dv[1] = -dv[1], dv[2] = -dv[2];
            const float o[3] = {(float)px, (float)py, (float)pz};
            float d[3];
            if (make_dir(g, dv, d)) check_ray(I, o, d, bounce, "bounce");
        }
    }
    auto share = [](unsigned long long culled, unsigned long long pairs) { return pairs ? 100.0 * (double)(pairs - culled) / (double)pairs : 0.0; };
    printf("first scene, %d clusters: camera rays pass %.2f %% of the clusters about the origin, %.2f %% about the foot point; "
           "bounces off the floor %.2f %% and %.2f %%\n",
           L.nc, share(cam.culled_old, cam.pairs), share(cam.culled, cam.pairs), share(bounce.culled_old, bounce.pairs), share(bounce.culled, bounce.pairs));
    if (cam.violations || bounce.violations) exit(1);
}

int main(int argc, char** argv) {
    unsigned long long pairs = 100000000ull;
    std::vector<std::vector<srt_object>> bases;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--pairs") && i + 1 < argc) {
            pairs = strtoull(argv[++i], nullptr, 10);
            continue;
        }
        bases.push_back(load(argv[i]));
        if (bases.back().empty()) {
            printf("cannot load %s\n", argv[i]);
            return 2;
        }
    }
    Rng g{12345};
    if (!bases.empty()) own_rays(build(bases[0]), g);
    const int n_files = (int)bases.size(), n_random = 25;
    for (int i = 0; i < n_random; ++i) bases.push_back(family(g, i % 5));
    Totals t;
    const float shifts[3] = {0.0f, 1.0e3f, 1.0e5f};
    int scenes = 0;
    // (the files get half of the pairs, the random families the other half)
    for (size_t b = 0; b < bases.size(); ++b)
        for (int s = 0; s < 3; ++s) {
            const Image I = build(translated(bases[b], shifts[s]));
            if (I.L.nc == 0) continue;
            const bool file = (int)b < n_files;
            const unsigned long long share = pairs / 2 / 3 / (unsigned long long)(file ? (n_files ? n_files : 1) : n_random) + 1;
            rays_of_scene(I, g, n_files ? share : 2 * share, t);
            ++scenes;
        }
    printf("%d scene images, %llu non-finite rays, %llu directions outside the unit window skipped\n", scenes, t.odd_rays, t.skipped);
    printf("(b) about the origin: %llu culled, %llu violations; (c) about the foot point: %llu culled\n", t.culled_old, t.violations_old, t.culled);
    if (t.violations || t.pairs < pairs) {
        printf("FAILED: %llu violations in %llu pairs\n", t.violations, t.pairs);
        return 1;
    }
    printf("ok %llu pairs, %llu culled by (c), 0 violations\n", t.pairs, t.culled);
    return 0;
}
