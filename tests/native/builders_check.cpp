// Host-side builders on random, degenerate and adversarial inputs (built with ASan + UBSan by test_builders_sanitized.py).
// build_scene_image: must not trip a sanitizer.  build_mesh_image: the image is decoded the way closest_hit decodes it and
// checked, in double, for what the kernel relies on —
//   structure    every triangle is referenced by exactly one leaf, children are in one mask at most, absent ones are inverted;
//   containment  the decoded box  origin + q * 2^(expo - 127)  of every child encloses every vertex below it, [center - half,
//                center + half] and the sphere (center, bs_radius) enclose every vertex of the mesh;
//   depth        max_depth is the depth of the node walk and fits the kernel's last-resort stack (7 * depth + 80 <= MESH_Q);
//   rows         gidpos is a permutation, row gidpos[g] carries gid g and the prim / ord / v0 / e1 / e2 bits recomputed from the
//                inputs, gids rise with (object list index, triangle index), exactly the valid triangles are present;
//   determinism  a second build gives the same bytes.
// Prints one line and returns non-zero on the first violation.
#include <cstdio>
#include <random>
#include "srt_scene_image.h"
#include "srt_mesh_bvh.h"

namespace {

constexpr int MESH_Q = 512;  // srt_kernel.hip.h (a device header): entries of the traversal buffer

struct Expect {
    float v[3][3];
    int32_t prim, ord;
};

struct Walk {
    const srt::MeshImage* mi;
    std::vector<int> seen;
    std::vector<double> tlo, thi;  // per triangle row: box of the float vertices and of the double sums v0 + e
    int depth = 0;
    const char* err = nullptr;
    int err_node = -1, err_child = -1, err_axis = -1;
};

uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// box (double lo[3], hi[3]) of everything below node `nd`; checks the node's children on the way
bool walk_node(Walk& W, int nd, int depth, double* lo, double* hi) {
    const srt::MeshImage& mi = *W.mi;
    W.depth = std::max(W.depth, depth);
    if (depth > 200) { W.err = "node chain deeper than 200"; W.err_node = nd; return false; }
    const float4* row = &mi.nodes[srt::NODE_VEC4 * (size_t)nd];
    const uint32_t w0 = bits(row[0].w), first_inner = bits(row[1].x), first_tri = bits(row[1].y), lw = bits(row[1].z);
    const uint32_t innermask = w0 >> 24, leafmask = lw & 255u, counts = lw >> 8;
    if (innermask & leafmask) { W.err = "child both inner and leaf"; W.err_node = nd; return false; }
    const double origin[3] = {row[0].x, row[0].y, row[0].z};
    double cell[3];
    for (int ax = 0; ax < 3; ++ax) cell[ax] = ldexp(1.0, (int)((w0 >> (8 * ax)) & 255u) - 127);
    uint8_t q[6][8];  // lo.x, lo.y, lo.z, hi.x, hi.y, hi.z
    {
        const float words[12] = {row[2].x, row[2].y, row[2].z, row[2].w, row[3].x, row[3].y, row[3].z, row[3].w, row[4].x, row[4].y, row[4].z, row[4].w};
        for (int p = 0; p < 6; ++p)
            for (int c = 0; c < 8; ++c) q[p][c] = (uint8_t)(bits(words[2 * p + (c >> 2)]) >> (8 * (c & 3)));
    }
    for (int ax = 0; ax < 3; ++ax) lo[ax] = INFINITY, hi[ax] = -INFINITY;
    int ni = 0;
    uint32_t tri = first_tri;
    for (int c = 0; c < 8; ++c) {
        double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        if (innermask >> c & 1u) {
            const int ref = (int)first_inner + ni++;
            if (ref <= nd || ref >= mi.n_nodes) { W.err = "bad node ref"; W.err_node = nd; W.err_child = c; return false; }
            if (!walk_node(W, ref, depth + 1, clo, chi)) return false;
        } else if (leafmask >> c & 1u) {
            const int cnt = 1 + (int)((counts >> (2 * c)) & 3u);
            for (int k = 0; k < cnt; ++k, ++tri) {
                if ((int)tri >= mi.n_tris) { W.err = "bad leaf"; W.err_node = nd; W.err_child = c; return false; }
                W.seen[(size_t)tri]++;
                for (int ax = 0; ax < 3; ++ax) clo[ax] = std::min(clo[ax], W.tlo[3 * (size_t)tri + ax]), chi[ax] = std::max(chi[ax], W.thi[3 * (size_t)tri + ax]);
            }
        } else {
            for (int ax = 0; ax < 3; ++ax)
                if (q[ax][c] <= q[3 + ax][c]) { W.err = "absent child's box is not inverted"; W.err_node = nd; W.err_child = c; W.err_axis = ax; return false; }
            continue;
        }
        for (int ax = 0; ax < 3; ++ax) {
            const double blo = origin[ax] + q[ax][c] * cell[ax], bhi = origin[ax] + q[3 + ax][c] * cell[ax];
            if (!(blo <= clo[ax] && chi[ax] <= bhi)) { W.err = "child box does not enclose its triangles"; W.err_node = nd; W.err_child = c; W.err_axis = ax; return false; }
            lo[ax] = std::min(lo[ax], clo[ax]), hi[ax] = std::max(hi[ax], chi[ax]);
        }
    }
    return true;
}

// one float ulp at magnitude m: what v0 + e (double) may differ by from the float vertex the boxes were built on
double ulp_at(double m) {
    const float f = (float)fabs(m);
    return (double)nextafterf(f, INFINITY) - (double)f;
}

bool verify(const char* what, int id, const srt_object* objs, size_t count, const std::vector<srt::HostMesh>& meshes, int prim_base, bool within_limits = true) {
    srt::MeshImage mi, again;
    srt::build_mesh_image(objs, count, meshes, prim_base, mi);
    srt::build_mesh_image(objs, count, meshes, prim_base, again);
#define FAIL(...) do { std::printf("%s %d: ", what, id); std::printf(__VA_ARGS__); std::printf("\n"); return false; } while (0)
    // ---- the triangles the inputs define: (object list index, triangle index) order; world = vertex + position in binary32
    std::vector<Expect> ex;
    int mesh_obj = 0;
    for (size_t i = 0; i < count; ++i) {
        if (objs[i].type != SRT_OBJ_MESH) continue;
        const int prim = prim_base + mesh_obj++;  // (an object with a bad mesh index keeps its primitive id)
        if (objs[i].mesh < 0 || (size_t)objs[i].mesh >= meshes.size()) continue;
        const srt::HostMesh& m = meshes[(size_t)objs[i].mesh];
        const size_t nv = m.vertices.size() / 3;
        for (size_t k = 0; k < m.indices.size() / 3; ++k) {
            Expect e;
            bool ok = true;
            for (int p = 0; p < 3 && ok; ++p) {
                const uint32_t ix = m.indices[3 * k + p];
                if (ix >= nv) { ok = false; break; }
                for (int ax = 0; ax < 3; ++ax) {
                    e.v[p][ax] = m.vertices[3 * (size_t)ix + ax] + objs[i].position[ax];
                    ok = ok && std::isfinite(e.v[p][ax]);
                }
            }
            e.prim = prim, e.ord = (int32_t)i;
            if (ok) ex.push_back(e);
        }
    }
    if (mi.n_mesh_objects != mesh_obj) FAIL("n_mesh_objects %d, expected %d", mi.n_mesh_objects, mesh_obj);
    if (mi.n_tris != (int)ex.size()) FAIL("n_tris %d, the inputs hold %zu valid triangles", mi.n_tris, ex.size());
    if (mi.tris.size() != 3 * ex.size() || mi.gidpos.size() != ex.size() || mi.nodes.size() != (size_t)srt::NODE_VEC4 * (size_t)mi.n_nodes) FAIL("array sizes");
    // ---- determinism
    if (again.n_tris != mi.n_tris || again.n_nodes != mi.n_nodes || again.max_depth != mi.max_depth || again.tris.size() != mi.tris.size() ||
        again.nodes.size() != mi.nodes.size() || (!mi.tris.empty() && memcmp(again.tris.data(), mi.tris.data(), mi.tris.size() * sizeof(float4)) != 0) ||
        (!mi.nodes.empty() && memcmp(again.nodes.data(), mi.nodes.data(), mi.nodes.size() * sizeof(float4)) != 0) || again.gidpos != mi.gidpos ||
        memcmp(again.center, mi.center, sizeof mi.center) != 0 || memcmp(again.half, mi.half, sizeof mi.half) != 0 || bits(again.bs_radius) != bits(mi.bs_radius))
        FAIL("a second build differs");
    if (ex.empty()) {
        if (mi.n_nodes != 0) FAIL("nodes without triangles");
        return true;
    }
    // ---- triangle rows
    Walk W;
    W.mi = &mi;
    W.seen.assign(ex.size(), 0);
    W.tlo.assign(3 * ex.size(), 0.0), W.thi.assign(3 * ex.size(), 0.0);
    std::vector<char> taken(ex.size(), 0);
    double r2max = 0;
    for (size_t g = 0; g < ex.size(); ++g) {
        const int32_t pos = mi.gidpos[g];
        if (pos < 0 || (size_t)pos >= ex.size() || taken[(size_t)pos]++) FAIL("gidpos is not a permutation (gid %zu -> %d)", g, pos);
        const float4 a = mi.tris[3 * (size_t)pos], b = mi.tris[3 * (size_t)pos + 1], c = mi.tris[3 * (size_t)pos + 2];
        const Expect& e = ex[g];
        if (bits(b.w) != (uint32_t)g) FAIL("row %d carries gid %u, not %zu", pos, bits(b.w), g);
        if (bits(a.w) != (uint32_t)e.prim || bits(c.w) != (uint32_t)e.ord) FAIL("gid %zu: prim %u ord %u, expected %d %d", g, bits(a.w), bits(c.w), e.prim, e.ord);
        if (g > 0 && ex[g - 1].ord > e.ord) FAIL("gids do not rise with the list index");
        const float v0[3] = {a.x, a.y, a.z}, e1[3] = {b.x, b.y, b.z}, e2[3] = {c.x, c.y, c.z};
        for (int ax = 0; ax < 3; ++ax) {
            if (bits(v0[ax]) != bits(e.v[0][ax]) || bits(e1[ax]) != bits(e.v[1][ax] - e.v[0][ax]) || bits(e2[ax]) != bits(e.v[2][ax] - e.v[0][ax]))
                FAIL("gid %zu: vertex / edge bits differ from the inputs (axis %d)", g, ax);
            // what lies below a box: the float vertices, and v0 + e summed in double (what the kernel's arithmetic starts from) —
            // the latter differs from the float vertex by the rounding of e = fl(v - v0), at most one ulp at the larger magnitude
            const double s1 = (double)v0[ax] + e1[ax], s2 = (double)v0[ax] + e2[ax];
            const double tol1 = ulp_at(std::max(fabs((double)v0[ax]), fabs(s1))), tol2 = ulp_at(std::max(fabs((double)v0[ax]), fabs(s2)));
            if (fabs(s1 - e.v[1][ax]) > tol1 || fabs(s2 - e.v[2][ax]) > tol2) FAIL("gid %zu: v0 + e is more than an ulp from the vertex", g);
            double lo = std::min((double)e.v[0][ax], std::min((double)e.v[1][ax], (double)e.v[2][ax]));
            double hi = std::max((double)e.v[0][ax], std::max((double)e.v[1][ax], (double)e.v[2][ax]));
            lo = std::min(lo, std::min(s1 + tol1, s2 + tol2));  // (the allowance: a sum may leave the box by its ulp, no further)
            hi = std::max(hi, std::max(s1 - tol1, s2 - tol2));
            W.tlo[3 * (size_t)pos + ax] = lo, W.thi[3 * (size_t)pos + ax] = hi;
        }
        for (int p = 0; p < 3; ++p) {
            double d2f = 0, d2s = 0;
            for (int ax = 0; ax < 3; ++ax) {
                const double s = (double)v0[ax] + (p == 1 ? (double)e1[ax] : p == 2 ? (double)e2[ax] : 0.0);
                d2f += ((double)e.v[p][ax] - mi.center[ax]) * ((double)e.v[p][ax] - mi.center[ax]);
                d2s += (s - mi.center[ax]) * (s - mi.center[ax]);
            }
            r2max = std::max(r2max, std::max(d2f, d2s));
        }
    }
    // ---- nodes: structure, containment, depth
    double lo[3], hi[3];
    if (!walk_node(W, 0, 1, lo, hi)) FAIL("%s (node %d child %d axis %d)", W.err, W.err_node, W.err_child, W.err_axis);
    for (size_t k = 0; k < ex.size(); ++k)
        if (W.seen[k] != 1) FAIL("triangle row %zu is in %d leaves", k, W.seen[k]);
    if (W.depth != mi.max_depth) FAIL("max_depth %d, the nodes are %d levels deep", mi.max_depth, W.depth);
    if (within_limits && 7 * mi.max_depth + 80 > MESH_Q) FAIL("depth %d does not fit the traversal buffer", mi.max_depth);
    // ---- root box and bounding sphere
    for (int ax = 0; ax < 3; ++ax)
        if (!((double)mi.center[ax] - mi.half[ax] <= lo[ax] && hi[ax] <= (double)mi.center[ax] + mi.half[ax]))
            FAIL("center +- half does not enclose the mesh (axis %d: [%.17g, %.17g] vs [%.17g, %.17g])", ax, (double)mi.center[ax] - mi.half[ax],
                 (double)mi.center[ax] + mi.half[ax], lo[ax], hi[ax]);
    if (!((double)mi.bs_radius >= sqrt(r2max))) FAIL("bs_radius %.9g is below the largest vertex distance %.17g", mi.bs_radius, sqrt(r2max));
#undef FAIL
    return true;
}

srt_object mesh_object(int mesh, float x = 0, float y = 0, float z = 0) {
    srt_object o;
    memset(&o, 0, sizeof o);
    o.type = SRT_OBJ_MESH;
    o.mesh = mesh;
    o.position[0] = x, o.position[1] = y, o.position[2] = z;
    return o;
}

void add_tri(srt::HostMesh& m, const float* a, const float* b, const float* c) {
    const uint32_t base = (uint32_t)(m.vertices.size() / 3);
    for (const float* p : {a, b, c})
        for (int ax = 0; ax < 3; ++ax) m.vertices.push_back(p[ax]);
    m.indices.push_back(base), m.indices.push_back(base + 1), m.indices.push_back(base + 2);
}

// n x n quads of side `step` lying exactly in the plane  coordinate[axis] = c  (shared vertices)
srt::HostMesh flat_grid(int n, int axis, float c, float step) {
    srt::HostMesh m;
    const int u = (axis + 1) % 3, v = (axis + 2) % 3;
    for (int j = 0; j <= n; ++j)
        for (int i = 0; i <= n; ++i) {
            float p[3];
            p[axis] = c, p[u] = (float)(i - n / 2) * step, p[v] = (float)(j - n / 2) * step;
            for (float f : p) m.vertices.push_back(f);
        }
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            const uint32_t a = (uint32_t)(j * (n + 1) + i), b = a + 1, d = a + (uint32_t)(n + 1), e = d + 1;
            for (uint32_t ix : {a, b, e, a, e, d}) m.indices.push_back(ix);
        }
    return m;
}

void add_uv_sphere(srt::HostMesh& m, float radius, int stacks, int slices, float cx, float cy, float cz) {
    const uint32_t base = (uint32_t)(m.vertices.size() / 3);
    auto put = [&](double x, double y, double z) { m.vertices.push_back((float)x + cx), m.vertices.push_back((float)y + cy), m.vertices.push_back((float)z + cz); };
    put(0, radius, 0);
    for (int i = 1; i < stacks; ++i)
        for (int j = 0; j < slices; ++j) {
            const double phi = M_PI * i / stacks, th = 2 * M_PI * j / slices;
            put(radius * sin(phi) * cos(th), radius * cos(phi), radius * sin(phi) * sin(th));
        }
    put(0, -radius, 0);
    auto ring = [&](int i, int j) { return base + 1u + (uint32_t)((i - 1) * slices + (j % slices)); };
    const uint32_t south = base + 1u + (uint32_t)((stacks - 1) * slices);
    for (int j = 0; j < slices; ++j)
        for (uint32_t ix : {base, ring(1, j + 1), ring(1, j)}) m.indices.push_back(ix);
    for (int i = 1; i < stacks - 1; ++i)
        for (int j = 0; j < slices; ++j)
            for (uint32_t ix : {ring(i, j), ring(i, j + 1), ring(i + 1, j + 1), ring(i, j), ring(i + 1, j + 1), ring(i + 1, j)}) m.indices.push_back(ix);
    for (int j = 0; j < slices; ++j)
        for (uint32_t ix : {south, ring(stacks - 1, j), ring(stacks - 1, j + 1)}) m.indices.push_back(ix);
}

bool one_mesh(const char* what, int id, const srt::HostMesh& m, float x = 0, float y = 0, float z = 0) {
    const srt_object o = mesh_object(0, x, y, z);
    return verify(what, id, &o, 1, std::vector<srt::HostMesh>{m}, 3);
}

bool adversarial_generators() {
    std::mt19937 rng(11);
    // flat grids lying exactly in each axis plane (zero extent on one axis: that axis' cell exponent sits at its floor)
    for (int axis = 0; axis < 3; ++axis)
        for (int n : {1, 3, 16, 100}) {
            if (!one_mesh("flat grid", 10 * n + axis, flat_grid(n, axis, 2.5f, 0.125f))) return false;
            if (!one_mesh("flat grid, offset", 10 * n + axis, flat_grid(n, axis, -0.375f, 0.25f), 1000.0f, -3.0f, 0.5f)) return false;
        }
    {  // a single triangle
        srt::HostMesh m;
        const float a[3] = {0, 0, 1}, b[3] = {1, 0, 1}, c[3] = {0, 1, 1};
        add_tri(m, a, b, c);
        if (!one_mesh("single triangle", 0, m)) return false;
    }
    // a 4000-unit two-triangle ground and a fine sphere in ONE mesh: the sphere's boxes sit on cells of the ground's grid
    for (int st : {4, 32, 100}) {
        srt::HostMesh m;
        const float a[3] = {-2000, -1, -2000}, b[3] = {2000, -1, -2000}, c[3] = {2000, -1, 2000}, d[3] = {-2000, -1, 2000};
        add_tri(m, a, c, b), add_tri(m, a, d, c);
        add_uv_sphere(m, 1.0f, st, st, 0.3f, 0.0f, 5.0f);
        if (!one_mesh("ground + sphere", st, m)) return false;
    }
    // diagonal slivers, 1e5 : 1, whose boxes all overlap
    for (int n : {1, 50, 2000, 20000}) {
        srt::HostMesh m;
        std::uniform_real_distribution<float> U(-1.f, 1.f);
        for (int k = 0; k < n; ++k) {
            const float s = U(rng) * 0.5f, L = 8.0f, w = L * 1e-5f;
            const float a[3] = {s, -s, 0.5f * s}, b[3] = {s + L, -s + L, 0.5f * s + L}, c[3] = {s + w, -s - w, 0.5f * s};
            add_tri(m, a, b, c);
        }
        if (!one_mesh("slivers", n, m, 0, 0, 3)) return false;
    }
    // one triangle repeated under shuffled indices (copies of one centroid cannot be told apart by any split)
    for (int rep : {1, 4, 5, 9, 70}) {
        srt::HostMesh g = flat_grid(rep == 70 ? 4 : 12, 2, 4.0f, 0.25f), m;
        m.vertices = g.vertices;
        std::vector<uint32_t> order;
        for (uint32_t k = 0; k < g.indices.size() / 3; ++k)
            for (int r = 0; r < rep; ++r) order.push_back(k);
        std::shuffle(order.begin(), order.end(), rng);
        for (uint32_t k : order)
            for (int p = 0; p < 3; ++p) m.indices.push_back(g.indices[3 * k + p]);
        if (!one_mesh("repeated triangles", rep, m)) return false;
        srt::HostMesh one;  // and a single triangle, `rep` times
        one.vertices = {0, 0, 2, 1, 0, 2, 0, 1, 2};
        for (int r = 0; r < rep; ++r)
            for (uint32_t ix : {0u, 1u, 2u}) one.indices.push_back(ix);
        if (!one_mesh("one triangle repeated", rep, one)) return false;
    }
    // world coordinates up to 9e8 (a float ulp there is 64): a grid of 1024-unit quads, a soup, the object position carrying the offset
    for (int n : {1, 8, 100}) {
        if (!one_mesh("9e8 grid", n, flat_grid(n, 1, 0.0f, 1024.0f), 8.9e8f, -8.9e8f, 8.9e8f)) return false;
        srt::HostMesh m;
        std::uniform_real_distribution<float> U(-1.f, 1.f);
        for (int k = 0; k < 2 * n * n; ++k) {
            float p[3][3];
            for (auto& q : p)
                for (float& f : q) f = 9e8f * U(rng);
            add_tri(m, p[0], p[1], p[2]);
        }
        if (!one_mesh("9e8 soup", n, m)) return false;
        srt::HostMesh s;
        for (int k = 0; k < 2 * n * n; ++k) {
            float b[3] = {8.99e8f + 4096.0f * U(rng), -8.99e8f + 4096.0f * U(rng), 8.99e8f * U(rng)}, p[3][3];
            for (auto& q : p)
                for (int ax = 0; ax < 3; ++ax) q[ax] = b[ax] + 512.0f * U(rng);
            add_tri(m, p[0], p[1], p[2]);
            add_tri(s, p[0], p[1], p[2]);
        }
        if (!one_mesh("9e8 corner soup", n, s) || !one_mesh("9e8 mixed soup", n, m)) return false;
    }
    // extents of exactly 255 * 2^e, one ulp below and one ulp above it (where the cell exponent steps), at several origins
    for (int e : {-20, -3, 0, 7, 20})
        for (int step = -1; step <= 1; ++step)
            for (float origin : {0.0f, -1.0f, 0.3f, 1000.0f}) {
                float ext = ldexpf(255.0f, e);
                ext = step < 0 ? nextafterf(ext, 0.0f) : step > 0 ? nextafterf(ext, INFINITY) : ext;
                srt::HostMesh m;
                for (int k = 0; k < 40; ++k) {  // small triangles strung along the extent, on all three axes at once
                    const float t0 = ext * (float)k / 40.0f, t1 = k == 39 ? ext : ext * (float)(k + 1) / 40.0f;
                    const float a[3] = {origin + t0, origin + t0, origin + t0}, b[3] = {origin + t1, origin + t0, origin + t1}, c[3] = {origin + t0, origin + t1, origin + t1};
                    add_tri(m, a, b, c);
                }
                if (!one_mesh("extent 255 * 2^e", 10 * e + step, m)) return false;
            }
    // a mesh object with a bad mesh index between valid ones keeps its primitive id and contributes nothing
    for (int bad : {-1, 2, 1000}) {
        std::vector<srt::HostMesh> meshes{flat_grid(3, 2, 4.0f, 0.5f), flat_grid(2, 0, -1.0f, 0.5f)};
        std::vector<srt_object> objs{mesh_object(0), mesh_object(bad), mesh_object(1, 0.5f), mesh_object(bad, 1, 2, 3), mesh_object(0, 0, 0, 1)};
        objs.insert(objs.begin() + 1, srt_object());
        memset(&objs[1], 0, sizeof(srt_object));  // SRT_OBJ_NONE
        if (!verify("bad mesh index", bad, objs.data(), objs.size(), meshes, 7)) return false;
        const srt_object only = mesh_object(bad);
        if (!verify("only a bad mesh index", bad, &only, 1, meshes, 0)) return false;
    }
    {  // a NaN in the second or third vertex only (min / max pass such a vertex by), infinities, indices out of range
        srt::HostMesh m = flat_grid(4, 2, 3.0f, 0.5f);
        srt::HostMesh n1 = m, n2 = m, inf = m, ix = m;
        n1.vertices[3 * n1.indices[1] + 0] = NAN;
        n2.vertices[3 * n2.indices[5] + 2] = NAN;
        inf.vertices[3 * inf.indices[2] + 1] = -INFINITY;
        ix.indices[4] = 1000;
        int id = 0;
        for (const srt::HostMesh& x : {n1, n2, inf, ix})
            if (!one_mesh("invalid triangles", id++, x)) return false;
    }
    return true;
}

}  // namespace

int main() {
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    size_t nodes = 0, vec4 = 0;
    for (int it = 0; it < 300; ++it) {
        int nobj = rng() % 200;
        std::vector<srt_object> objs(nobj);
        std::vector<srt::HostMesh> meshes(1 + rng() % 2);
        for (auto& m : meshes) {
            int nt = it % 7 == 0 ? 0 : (int)(rng() % (it % 11 == 0 ? 20000 : 300));
            int mode = rng() % 5;
            for (int k = 0; k < nt; ++k) {
                float b[3] = {U(rng) * 3, U(rng) * 3, U(rng) * 3};
                for (int q = 0; q < 3; ++q)
                    for (int a = 0; a < 3; ++a) {
                        float v = mode == 0 ? b[a] : b[a] + U(rng) * (mode == 1 ? 0.0f : 0.3f);
                        if (mode == 2 && k % 17 == 0) v *= 1e6f;
                        if (mode == 3) v = (float)(int)(v * 2);
                        m.vertices.push_back(v);
                    }
                uint32_t base = (uint32_t)(3 * k);
                m.indices.push_back(base); m.indices.push_back(base + 1); m.indices.push_back(mode == 4 && k % 5 == 0 ? base + 100000 : base + 2);
            }
        }
        for (auto& o : objs) {
            memset(&o, 0, sizeof o);
            int t = rng() % 10;
            o.type = t < 6 ? SRT_OBJ_SPHERE : t < 8 ? SRT_OBJ_BOX : t < 9 ? SRT_OBJ_MESH : SRT_OBJ_NONE;
            for (int a = 0; a < 3; ++a) o.position[a] = U(rng) * (it % 5 == 0 ? 1e5f : 8.f), o.half_size[a] = U(rng) + 1.f;
            o.radius = it % 13 == 0 && rng() % 20 == 0 ? INFINITY : U(rng) * (rng() % 30 == 0 ? 500.f : 0.5f);
            if (rng() % 50 == 0) o.position[0] = NAN;
            o.mesh = (int)(rng() % meshes.size());
        }
        std::vector<float4> img;
        srt::SceneLayout L = srt::build_scene_image(objs.data(), objs.size(), it % 3 != 0, img);
        vec4 += (size_t)L.total_vec4;
        srt::MeshImage mi;
        srt::build_mesh_image(objs.data(), objs.size(), meshes, L.nsT + L.nb, mi);
        nodes += (size_t)mi.n_nodes;
        // structural checks of the wide BVH: every triangle is referenced by exactly one leaf
        if (mi.n_tris > 0) {
            std::vector<int> seen((size_t)mi.n_tris, 0);
            std::vector<int> stack{0};
            while (!stack.empty()) {
                int nd = stack.back(); stack.pop_back();
                const float4 h0 = mi.nodes[srt::NODE_VEC4 * (size_t)nd], h1 = mi.nodes[srt::NODE_VEC4 * (size_t)nd + 1];
                uint32_t w0, first_inner, first_tri, lw;
                memcpy(&w0, &h0.w, 4); memcpy(&first_inner, &h1.x, 4); memcpy(&first_tri, &h1.y, 4); memcpy(&lw, &h1.z, 4);
                const uint32_t innermask = w0 >> 24, leafmask = lw & 255u, counts = lw >> 8;
                if (innermask & leafmask) { std::printf("child both inner and leaf\n"); return 1; }
                int ni = 0; uint32_t tri = first_tri;
                for (int c = 0; c < 8; ++c) {
                    if (innermask >> c & 1u) { int ref = (int)first_inner + ni++; if (ref <= nd || ref >= mi.n_nodes) { std::printf("bad node ref\n"); return 1; } stack.push_back(ref); }
                    else if (leafmask >> c & 1u) { int cnt = 1 + (int)((counts >> (2 * c)) & 3u); for (int k = 0; k < cnt; ++k) { if ((int)tri >= mi.n_tris) { std::printf("bad leaf\n"); return 1; } seen[(size_t)tri++]++; } }
                }
            }
            for (int k = 0; k < mi.n_tris; ++k) if (seen[(size_t)k] != 1) { std::printf("triangle %d seen %d times (it %d)\n", k, seen[(size_t)k], it); return 1; }
        }
        // ... and containment, rows, depth, determinism
        if (!verify("random scene", it, objs.data(), objs.size(), meshes, L.nsT + L.nb)) return 1;
    }
    int adversarial_depth = 0;
    {  // adversarial for a binned SAH: geometrically spaced centroids peel one triangle off per level.  The
       // builder must neither recurse once per triangle nor produce a tree deeper than its median-split bound.
        srt::HostMesh m;
        const int nt = 60000;
        double x = 1e-30;
        for (int k = 0; k < nt; ++k) {
            x *= 1.0012;
            const float f = (float)x;
            const float v[9] = {f, 0, 0, f * 1.0001f, f * 1e-3f, 0, f, 0, f * 1e-3f};
            for (float q : v) m.vertices.push_back(q);
            m.indices.push_back(3 * k), m.indices.push_back(3 * k + 1), m.indices.push_back(3 * k + 2);
        }
        srt_object o;
        memset(&o, 0, sizeof o);
        o.type = SRT_OBJ_MESH;
        srt::MeshImage mi;
        srt::build_mesh_image(&o, 1, std::vector<srt::HostMesh>{m}, 0, mi);
        if (mi.n_tris != nt || mi.max_depth > 40 + 17) { std::printf("adversarial mesh: %d tris depth %d\n", mi.n_tris, mi.max_depth); return 1; }
        // ... and it must BE deep, or the GPU test that traverses this mesh (test_gpu_mesh_edges.py) tests nothing: a balanced tree of
        // its 15000 leaves is 14 binary levels, so 30 levels of 8-wide nodes can only come from the peeled chain
        if (mi.max_depth < 30) { std::printf("adversarial mesh: only %d levels deep\n", mi.max_depth); return 1; }
        if (!verify("geometric centroids", nt, &o, 1, std::vector<srt::HostMesh>{m}, 0)) return 1;
        adversarial_depth = mi.max_depth;
    }
    if (!adversarial_generators()) return 1;
    std::printf("ok nodes %zu vec4 %zu (geometric-centroid mesh: %d levels)\n", nodes, vec4, adversarial_depth);
}
