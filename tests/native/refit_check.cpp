// The refit of the mesh image on the host (built with ASan + UBSan by test_refit_native.py): a loop over the functions the refit
// kernels run per thread (srt_mesh_bvh.h: refit_triangle, refit_child_box, quantize_child, pack_node; refit_node is the eight
// lanes of one node in sequence), on the image build_mesh_image made.
//   identity   a refit at unchanged positions reproduces `nodes` and `tris` of the build byte for byte;
//   records    after a move every triangle record has the bits a fresh build of the moved list gives it (matched by global
//              triangle id), and float4 1 of every node and every triangle .w are untouched;
//   enclosure  after a move the decoded box  origin + q * 2^(expo - 127)  of every child encloses the world vertices
//              (float vertex + position) of everything below it, and absent children stay inverted;
//   root       refit_root's box equals the min / max over all world vertices bit for bit, its centre and half extent are the
//              fresh build's bits, its sphere contains every vertex;
//   levels     level_first has max_depth entries, starts at 0, rises, and every inner child lies in the level after its parent's;
//   exponent   quant_exponent's closed form gives what the build's loop (kept below) gave, on boundaries and random extents.
// Meshes: strips of 1, 4, 5, 9 and 33 triangles, a 600-triangle sphere, an axis-aligned flat triangle, vertices at 6e-17 inside
// a box that starts at -1, positions at 1e6 (vertex + position rounds), two objects sharing one mesh of which one moves.
// Prints one line and returns non-zero on the first violation.
#include <cstdio>
#include <random>
#include "srt_mesh_bvh.h"

namespace {

uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

srt_object mesh_object(int mesh, float x, float y, float z) {
    srt_object o;
    memset(&o, 0, sizeof o);
    o.type = SRT_OBJ_MESH;
    o.position[0] = x, o.position[1] = y, o.position[2] = z;
    o.material.base_color[0] = o.material.base_color[1] = o.material.base_color[2] = 0.5f;
    o.mesh = mesh;
    return o;
}

void add_tri(srt::HostMesh& m, const float* a, const float* b, const float* c) {
    const uint32_t base = (uint32_t)(m.vertices.size() / 3);
    for (const float* v : {a, b, c})
        for (int ax = 0; ax < 3; ++ax) m.vertices.push_back(v[ax]);
    for (uint32_t q = 0; q < 3; ++q) m.indices.push_back(base + q);
}

// n triangles along x, wobbling in y and z, sharing vertices
srt::HostMesh strip(int n) {
    srt::HostMesh m;
    for (int k = 0; k < n + 2; ++k) {
        m.vertices.push_back(0.37f * (float)k);
        m.vertices.push_back((k & 1) ? 0.9f : -0.2f * (float)(k % 5));
        m.vertices.push_back(0.11f * (float)((k * 7) % 4));
    }
    for (int k = 0; k < n; ++k)
        for (int q = 0; q < 3; ++q) m.indices.push_back((uint32_t)(k + q));
    return m;
}

srt::HostMesh uv_sphere(float radius, int stacks, int slices) {
    srt::HostMesh m;
    for (int i = 0; i <= stacks; ++i)
        for (int j = 0; j < slices; ++j) {
            const double th = M_PI * i / stacks, ph = 2 * M_PI * j / slices;
            m.vertices.push_back((float)(radius * sin(th) * cos(ph)));
            m.vertices.push_back((float)(radius * cos(th)));
            m.vertices.push_back((float)(radius * sin(th) * sin(ph)));
        }
    for (int i = 0; i < stacks; ++i)
        for (int j = 0; j < slices; ++j) {
            const uint32_t a = (uint32_t)(i * slices + j), b = (uint32_t)(i * slices + (j + 1) % slices), c = a + (uint32_t)slices, d = b + (uint32_t)slices;
            if (i > 0) m.indices.insert(m.indices.end(), {a, b, c});
            if (i + 1 < stacks) m.indices.insert(m.indices.end(), {b, d, c});
        }
    return m;
}

struct Refit {
    srt::MeshImage img;  // nodes and tris rewritten in place
    std::vector<float4> verts, tri_box, node_box;
};

// what the two kernels do, in stream order
void host_refit(Refit& R, const std::vector<srt::HostMesh>& meshes, const srt_object* objs, size_t count) {
    R.verts = srt::refit_vertices(meshes);
    std::vector<float4> pos(count);
    for (size_t i = 0; i < count; ++i) pos[i] = make_float4(objs[i].position[0], objs[i].position[1], objs[i].position[2], 0.0f);
    R.tri_box.assign((size_t)R.img.n_tris * 2, make_float4(NAN, NAN, NAN, NAN));
    R.node_box.assign((size_t)R.img.n_nodes * 2, make_float4(NAN, NAN, NAN, NAN));
    for (uint32_t t = 0; t < (uint32_t)R.img.n_tris; ++t)
        srt::refit_triangle(R.img.tris.data(), R.img.tri_verts.data(), R.verts.data(), pos.data(), R.tri_box.data(), t);
    for (size_t l = R.img.level_first.size(); l-- > 0;) {
        const int first = R.img.level_first[l], end = l + 1 < R.img.level_first.size() ? R.img.level_first[l + 1] : R.img.n_nodes;
        for (int k = first; k < end; ++k)
            srt::refit_node(R.img.nodes.data(), R.tri_box.data(), R.node_box.data(), (uint32_t)R.img.n_nodes, (uint32_t)R.img.n_tris, (uint32_t)k);
    }
}

const char* g_err = nullptr;
int g_node = -1, g_child = -1;

// box of the world vertices below node nd; checks every child's decoded box on the way
bool walk(const srt::MeshImage& mi, const std::vector<double>& tlo, const std::vector<double>& thi, std::vector<int>& seen, int nd, int depth,
          const std::vector<int>& level_of, double* lo, double* hi) {
    const float4* row = &mi.nodes[srt::NODE_VEC4 * (size_t)nd];
    const uint32_t w0 = bits(row[0].w), first_inner = bits(row[1].x), first_tri = bits(row[1].y), lw = bits(row[1].z);
    const uint32_t innermask = w0 >> 24, leafmask = lw & 255u, counts = lw >> 8;
    const double origin[3] = {row[0].x, row[0].y, row[0].z};
    double cell[3];
    for (int ax = 0; ax < 3; ++ax) cell[ax] = ldexp(1.0, (int)((w0 >> (8 * ax)) & 255u) - 127);
    const float words[12] = {row[2].x, row[2].y, row[2].z, row[2].w, row[3].x, row[3].y, row[3].z, row[3].w, row[4].x, row[4].y, row[4].z, row[4].w};
    uint8_t q[6][8];
    for (int p = 0; p < 6; ++p)
        for (int c = 0; c < 8; ++c) q[p][c] = (uint8_t)(bits(words[2 * p + (c >> 2)]) >> (8 * (c & 3)));
    for (int ax = 0; ax < 3; ++ax) lo[ax] = INFINITY, hi[ax] = -INFINITY;
    g_node = nd;
    if (level_of[(size_t)nd] != depth) return g_err = "node is not in the level of its depth", false;
    int ni = 0;
    uint32_t tri = first_tri;
    for (int c = 0; c < 8; ++c) {
        g_child = c;
        double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        if (innermask >> c & 1u) {
            const int ref = (int)first_inner + ni++;
            if (ref <= nd || ref >= mi.n_nodes) return g_err = "bad node reference", false;
            if (!walk(mi, tlo, thi, seen, ref, depth + 1, level_of, clo, chi)) return false;
            g_node = nd, g_child = c;
        } else if (leafmask >> c & 1u) {
            const int cnt = 1 + (int)((counts >> (2 * c)) & 3u);
            for (int k = 0; k < cnt; ++k, ++tri) {
                if ((int)tri >= mi.n_tris) return g_err = "bad leaf", false;
                seen[(size_t)tri]++;
                for (int ax = 0; ax < 3; ++ax) clo[ax] = std::min(clo[ax], tlo[3 * (size_t)tri + ax]), chi[ax] = std::max(chi[ax], thi[3 * (size_t)tri + ax]);
            }
        } else {
            for (int ax = 0; ax < 3; ++ax)
                if (q[ax][c] <= q[3 + ax][c]) return g_err = "absent child's box is not inverted", false;
            continue;
        }
        for (int ax = 0; ax < 3; ++ax) {
            const double blo = origin[ax] + q[ax][c] * cell[ax], bhi = origin[ax] + q[3 + ax][c] * cell[ax];
            if (!(blo <= clo[ax] && chi[ax] <= bhi)) return g_err = "child box does not enclose what lies below it", false;
            lo[ax] = std::min(lo[ax], clo[ax]), hi[ax] = std::max(hi[ax], chi[ax]);
        }
    }
    return true;
}

bool fail(const char* what, int id, const char* msg) {
    printf("FAIL %s #%d: %s (node %d child %d)\n", what, id, msg, g_node, g_child);
    return false;
}

// build at `from`, refit to `from` (identity), refit to `to`, compare with a fresh build at `to`
bool check(const char* what, int id, const std::vector<srt::HostMesh>& meshes, const std::vector<srt_object>& from, const std::vector<srt_object>& to) {
    const size_t count = from.size();
    srt::MeshImage built;
    srt::build_mesh_image(from.data(), count, meshes, 0, built);
    if (built.n_tris == 0) return fail(what, id, "no triangles");
    // levels
    if ((int)built.level_first.size() != built.max_depth || built.level_first[0] != 0) return fail(what, id, "level_first does not have max_depth entries from 0");
    std::vector<int> level_of((size_t)built.n_nodes, 0);
    for (size_t l = 0; l < built.level_first.size(); ++l) {
        const int first = built.level_first[l], end = l + 1 < built.level_first.size() ? built.level_first[l + 1] : built.n_nodes;
        if (first >= end) return fail(what, id, "empty level");
        for (int k = first; k < end; ++k) level_of[(size_t)k] = (int)l + 1;
    }
    if (built.tri_verts.size() != 3 * (size_t)built.n_tris) return fail(what, id, "tri_verts size");
    // identity
    Refit R;
    R.img = built;
    host_refit(R, meshes, from.data(), count);
    if (memcmp(R.img.nodes.data(), built.nodes.data(), built.nodes.size() * sizeof(float4)) != 0) return fail(what, id, "identity refit changed node bytes");
    if (memcmp(R.img.tris.data(), built.tris.data(), built.tris.size() * sizeof(float4)) != 0) return fail(what, id, "identity refit changed triangle bytes");
    // move
    host_refit(R, meshes, to.data(), count);
    srt::MeshImage fresh;
    srt::build_mesh_image(to.data(), count, meshes, 0, fresh);
    if (fresh.n_tris != built.n_tris) return fail(what, id, "the move changed the valid-triangle set (test input)");
    for (int g = 0; g < built.n_tris; ++g)
        if (memcmp(&R.img.tris[3 * (size_t)built.gidpos[(size_t)g]], &fresh.tris[3 * (size_t)fresh.gidpos[(size_t)g]], 3 * sizeof(float4)) != 0)
            return fail(what, id, "a refitted triangle record differs from the fresh build's");
    for (int k = 0; k < built.n_nodes; ++k)
        if (memcmp(&R.img.nodes[srt::NODE_VEC4 * (size_t)k + 1], &built.nodes[srt::NODE_VEC4 * (size_t)k + 1], sizeof(float4)) != 0 ||
            (bits(R.img.nodes[srt::NODE_VEC4 * (size_t)k].w) >> 24) != (bits(built.nodes[srt::NODE_VEC4 * (size_t)k].w) >> 24))
            return fail(what, id, "the refit changed a node's topology words");
    // enclosure, against world vertices recomputed here
    std::vector<double> tlo(3 * (size_t)built.n_tris), thi(3 * (size_t)built.n_tris);
    float wlo[3] = {INFINITY, INFINITY, INFINITY}, whi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int t = 0; t < built.n_tris; ++t) {
        const uint32_t ord = bits(R.img.tris[3 * (size_t)t + 2].w);
        if (ord >= count) return fail(what, id, "list index out of range");
        for (int ax = 0; ax < 3; ++ax) {
            float lo = INFINITY, hi = -INFINITY;
            for (int q = 0; q < 3; ++q) {
                const float4 v = R.verts[built.tri_verts[3 * (size_t)t + q]];
                const float w = (ax == 0 ? v.x : ax == 1 ? v.y : v.z) + to[ord].position[ax];
                lo = std::min(lo, w), hi = std::max(hi, w);
            }
            tlo[3 * (size_t)t + ax] = lo, thi[3 * (size_t)t + ax] = hi;
            wlo[ax] = std::min(wlo[ax], lo), whi[ax] = std::max(whi[ax], hi);
        }
    }
    std::vector<int> seen((size_t)built.n_tris, 0);
    double lo[3], hi[3];
    g_err = nullptr;
    if (!walk(R.img, tlo, thi, seen, 0, 1, level_of, lo, hi)) return fail(what, id, g_err);
    for (int t = 0; t < built.n_tris; ++t)
        if (seen[(size_t)t] != 1) return fail(what, id, "a triangle is not in exactly one leaf");
    // root
    float rlo[3], rhi[3], center[3], half[3], radius;
    if (!srt::refit_root(built, to.data(), rlo, rhi, center, half, radius)) return fail(what, id, "refit_root found no triangle");
    for (int ax = 0; ax < 3; ++ax) {
        if (bits(rlo[ax]) != bits(wlo[ax]) || bits(rhi[ax]) != bits(whi[ax])) return fail(what, id, "the host-derived root box is not the min / max of the world vertices");
        if (bits(center[ax]) != bits(fresh.center[ax]) || bits(half[ax]) != bits(fresh.half[ax])) return fail(what, id, "centre / half differ from the fresh build's");
    }
    for (int t = 0; t < built.n_tris; ++t)
        for (int cx = 0; cx < 2; ++cx)
            for (int cy = 0; cy < 2; ++cy)
                for (int cz = 0; cz < 2; ++cz) {  // (the corners of a triangle's box are at least as far out as its vertices)
                    const double dx = (cx ? thi : tlo)[3 * (size_t)t] - center[0], dy = (cy ? thi : tlo)[3 * (size_t)t + 1] - center[1],
                                 dz = (cz ? thi : tlo)[3 * (size_t)t + 2] - center[2];
                    if (!(dx * dx + dy * dy + dz * dz <= (double)radius * (double)radius)) return fail(what, id, "the refitted bounding sphere misses a vertex");
                }
    return true;
}

// the loop build_mesh_image used before the closed form
uint32_t exponent_by_loop(float lo, float hi) {
    const srt::QuantDiff ext = srt::quant_diff(hi, lo);
    int e = -126;
    while (e < 127 && (ldexp(255.0, e) < ext.d || (ldexp(255.0, e) == ext.d && ext.err > 0))) ++e;
    return (uint32_t)(e + 127);
}

bool exponents() {
    std::mt19937 rng(99);
    std::uniform_real_distribution<float> mant(1.0f, 2.0f);
    std::uniform_int_distribution<int> ex(-149, 127);
    long n = 0;
    auto one = [&](float lo, float hi) {
        ++n;
        if (srt::quant_exponent(lo, hi) == exponent_by_loop(lo, hi)) return true;
        printf("FAIL exponent: lo %a hi %a closed %u loop %u\n", lo, hi, srt::quant_exponent(lo, hi), exponent_by_loop(lo, hi));
        return false;
    };
    for (int e = -149; e <= 120; ++e) {  // extents of exactly 255 * 2^e, 256 * 2^e, and an ulp either side, from 0 and from an offset
        for (float scale : {255.0f, 256.0f, 1.0f}) {
            const float x = ldexpf(scale, e);
            for (float v : {nextafterf(x, 0.0f), x, nextafterf(x, INFINITY)}) {
                if (!std::isfinite(v)) continue;  // (a node's box is finite)
                if (!one(0.0f, v) || !one(-v, 0.0f) || !one(-v, v) || !one(-1.0f, v) || !one(-v, 6e-17f)) return false;
            }
        }
    }
    if (!one(0.0f, 0.0f) || !one(-3e38f, 3e38f) || !one(5.0f, 5.0f) || !one(-1.0f, 6e-17f)) return false;
    for (int k = 0; k < 200000; ++k) {
        float a = ldexpf(mant(rng), ex(rng)) * ((k & 1) ? -1.0f : 1.0f), b = ldexpf(mant(rng), ex(rng)) * ((k & 2) ? -1.0f : 1.0f);
        if (!std::isfinite(a) || !std::isfinite(b)) continue;
        if (b < a) std::swap(a, b);
        if (!one(a, b)) return false;
    }
    return n > 0;
}

}  // namespace

int main() {
    if (!exponents()) return 1;
    int id = 0, cases = 0;
    auto run = [&](const char* what, const std::vector<srt::HostMesh>& meshes, std::vector<srt_object> from, std::vector<srt_object> to) {
        ++cases;
        return check(what, id++, meshes, from, to);
    };
    const float moves[][3] = {{0.1f, -0.05f, 0.3f}, {40.0f, -17.0f, 250.0f}, {-1e-3f, 0.0f, 0.0f}};
    // strips and the sphere, moved a little, a lot, and by less than the quantization cell
    std::vector<srt::HostMesh> shapes;
    for (int n : {1, 4, 5, 9, 33}) shapes.push_back(strip(n));
    shapes.push_back(uv_sphere(1.5f, 16, 20));  // 600 triangles
    {  // an axis-aligned flat triangle: extent 0 on z
        srt::HostMesh m;
        const float a[3] = {0, 0, 2}, b[3] = {1, 0, 2}, c[3] = {0, 1, 2};
        add_tri(m, a, b, c);
        shapes.push_back(m);
    }
    {  // vertices at 6e-17 inside a box that starts at -1: differences that are not exact in double
        srt::HostMesh m;
        const float a[3] = {-1, -1, -1}, b[3] = {6e-17f, -1, 6e-17f}, c[3] = {-1, 6e-17f, 0.5f}, d[3] = {6e-17f, 6e-17f, 6e-17f}, e[3] = {0.25f, 6e-17f, -1};
        add_tri(m, a, b, c), add_tri(m, b, c, d), add_tri(m, c, d, e), add_tri(m, a, d, e), add_tri(m, a, b, e), add_tri(m, b, d, e);
        shapes.push_back(m);
    }
    for (size_t s = 0; s < shapes.size(); ++s)
        for (const float* mv : moves) {
            const std::vector<srt::HostMesh> meshes = {shapes[s]};
            if (!run("shape", meshes, {mesh_object(0, 0, 0, 0)}, {mesh_object(0, mv[0], mv[1], mv[2])})) return 1;
            // positions at 1e6: vertex + position rounds, differently before and after
            if (!run("shape at 1e6", meshes, {mesh_object(0, 1e6f, -1e6f, 1e6f)}, {mesh_object(0, 1e6f + mv[0], -1e6f + mv[1], 1e6f + mv[2])})) return 1;
            if (!run("shape to 1e6", meshes, {mesh_object(0, mv[0], mv[1], mv[2])}, {mesh_object(0, 1e6f, 3e5f, -1e6f)})) return 1;
        }
    // several objects: two share a mesh and only the later one moves; then both onto the same position; a sphere in between
    {
        const std::vector<srt::HostMesh> meshes = {strip(9), uv_sphere(1.0f, 16, 20), strip(5)};
        srt_object ball;
        memset(&ball, 0, sizeof ball);
        ball.type = SRT_OBJ_SPHERE, ball.radius = 1.0f;
        const std::vector<srt_object> from = {mesh_object(1, -2, 0, 6), ball, mesh_object(0, 0, 1, 5), mesh_object(1, 2, 0, 6), mesh_object(2, 0, -2, 4)};
        std::vector<srt_object> to = from;
        to[3].position[0] = 2.5f, to[3].position[2] = 7.0f;
        if (!run("shared mesh", meshes, from, to)) return 1;
        to[3] = from[3];
        for (int ax = 0; ax < 3; ++ax) to[3].position[ax] = from[0].position[ax];
        if (!run("coincident", meshes, from, to)) return 1;
        to = from;
        for (srt_object& o : to) o.position[1] += 100.0f;
        if (!run("all moved", meshes, from, to)) return 1;
        if (!run("and back", meshes, to, from)) return 1;
    }
    printf("ok %d refit cases\n", cases);
    return 0;
}
