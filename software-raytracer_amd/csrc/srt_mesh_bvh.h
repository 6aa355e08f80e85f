// srt_mesh_bvh.h — host-side flattening of SRT_OBJ_MESH objects into one world-space
// triangle list + an 8-wide BVH (EXTENSION: the reference has no triangle primitive).
//
// Device layout (HBM, read through L2; too large for LDS at 100k triangles):
//   tris : 3 float4 per triangle, in BVH leaf order
//            (v0.xyz, bits(primitive id p))      p indexes the LDS material table
//            (e1.xyz, bits(global triangle id))  id = position in (object list order, triangle
//            (e2.xyz, bits(list index))               index) — restores the tie rule
//   nodes: 5 float4 (80 B) per 8-WIDE inner node, child boxes quantized to 8 bits on the node's own box:
//            (origin.xyz, bits(ex | ey<<8 | ez<<16 | innermask<<24))   cell size per axis = 2^(e-127)
//            (bits(first inner child), bits(first leaf triangle), bits(leafmask | counts<<8), 0)
//            (lo.x[0..3], lo.x[4..7], lo.y[0..3], lo.y[4..7])   one byte per child
//            (lo.z[0..3], lo.z[4..7], hi.x[0..3], hi.x[4..7])
//            (hi.y[0..3], hi.y[4..7], hi.z[0..3], hi.z[4..7])
//          child box = origin + q*cell, lo rounded down / hi up, so it encloses the exact box.
//          Children are IMPLICIT: nodes are numbered breadth-first, so the inner children of a node are
//          consecutive — child c (bit c of innermask) is node  first_inner + popcount(innermask & ((1<<c)-1));
//          triangles are stored in the same breadth-first order, so the leaf children of a node are
//          consecutive too — child c (bit c of leafmask) holds  1 + ((counts >> 2c) & 3)  triangles starting at
//          first_leaf_triangle + the sum of the counts of the leaf children before it.  A child in neither
//          mask is absent (its box is inverted).  Node 0 is the root; a mesh of <= 4 triangles is a root
//          with one leaf child.
// Build: binary binned surface-area heuristic (16 bins per axis, median fallback), leaves of <= 4
// triangles, then collapsed to 8 children per node — deterministic.  Bounds are exact (float min/max of the float vertices); the
// kernel pads them per ray (see closest_hit) so that the box filter is conservative with
// respect to the rounding of the triangle test.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <stdexcept>
#include <vector>

#include "srt_pathtrace.h"

namespace srt {

struct HostMesh {
    std::vector<float> vertices;
    std::vector<uint32_t> indices;
};

constexpr int NODE_VEC4 = 5;  // float4 per node (80 B)

struct MeshImage {
    std::vector<float4> tris, nodes;
    std::vector<int32_t> gidpos;  // global triangle id -> position in `tris` (leaf order)
    int n_tris = 0, n_nodes = 0, n_mesh_objects = 0, max_depth = 0;
    float center[3] = {0, 0, 0}, half[3] = {0, 0, 0};  // root box
    float bs_radius = 0;  // radius of a sphere around `center` that contains every triangle (rounded up)
    // What a refit (srt_refit.hip.h) needs and the build knows.  Vertex indices point into the concatenation of all meshes'
    // vertex arrays, in mesh order (refit_vertex_bases).
    std::vector<int32_t> level_first;    // first node of every breadth-first level (max_depth entries)
    std::vector<uint32_t> tri_verts;     // 3 per triangle, leaf order
    struct ObjectBox {
        int32_t list_index;  // of the mesh object
        float lo[3], hi[3];  // box of its valid triangles' LOCAL vertices (inverted when it has none)
    };
    std::vector<ObjectBox> object_boxes;   // one per mesh object, list order
    std::vector<uint8_t> mesh_dropped;     // per mesh: a triangle of an object of this mesh was dropped as non-finite
};

inline float bits_of(int32_t v) {
    float f;
    memcpy(&f, &v, 4);
    return f;
}

// std::min / std::max as the build has always used them (the first argument wins a tie, so also between -0 and +0), for host and device
__host__ __device__ inline float box_min(float a, float b) { return b < a ? b : a; }
__host__ __device__ inline float box_max(float a, float b) { return a < b ? b : a; }

// The triangle record's arithmetic, shared by the build and the refit kernel: world vertex = vertex + position, the edges from
// the world vertices, and the exact box of the three world vertices (never v0 + e1, which is another float).
struct TriangleRecord {
    float v[3][3];  // world vertices
    float e1[3], e2[3], lo[3], hi[3];
};
__host__ __device__ inline void triangle_record(const float* a, const float* b, const float* c, const float* position, TriangleRecord& t) {
    for (int ax = 0; ax < 3; ++ax) {
        t.v[0][ax] = a[ax] + position[ax];
        t.v[1][ax] = b[ax] + position[ax];
        t.v[2][ax] = c[ax] + position[ax];
        t.e1[ax] = t.v[1][ax] - t.v[0][ax];
        t.e2[ax] = t.v[2][ax] - t.v[0][ax];
        t.lo[ax] = box_min(t.v[0][ax], box_min(t.v[1][ax], t.v[2][ax]));
        t.hi[ax] = box_max(t.v[0][ax], box_max(t.v[1][ax], t.v[2][ax]));
    }
}

// Quantization of child boxes on the 256^3 grid spanned by a node's own box, shared by the build and the refit kernel.
// origin = node.lo (float), cell = 2^e per axis (the smallest power of two, e >= -126, with 255 cells >= extent); lo is rounded
// down, hi up, so  origin + q*cell  (as real numbers) encloses the child.  A difference of two floats is only exact in double
// while their exponents are within 29 of each other (a vertex at 6e-17 in a box that starts at -1 is not), so the
// differences carry their rounding error along (Knuth's TwoSum) and a quotient that lands exactly on a cell boundary
// is pushed outwards by it.  (TwoSum relies on IEEE addition as written: no -ffast-math / reassociation / contraction on a
// translation unit that includes this header.)
struct QuantDiff {
    double d, err;  // a - b = d + err exactly
};
__host__ __device__ inline QuantDiff quant_diff(float a, float b) {
    const double x = (double)a, y = -(double)b, s = x + y, yy = s - x;
    return QuantDiff{s, (x - (s - yy)) + (y - yy)};
}
// the biased exponent byte of one axis of a node whose box is [lo, hi].  255 * 2^e = (255/256) * 2^(e + 8), so with
// extent = m * 2^x, m in [0.5, 1), the smallest e with 255 * 2^e >= extent is x - 8 (m <= 255/256) or x - 7.
__host__ __device__ inline uint32_t quant_exponent(float lo, float hi) {
    const QuantDiff ext = quant_diff(hi, lo);
    int e = -126;
    if (ext.d > 0) {
        int x;
        const double m = frexp(ext.d, &x);
        e = m <= 255.0 / 256.0 ? x - 8 : x - 7;
        if (e < -126) e = -126;
        if (e < 127 && ldexp(255.0, e) == ext.d && ext.err > 0) ++e;
        if (e > 127) e = 127;
    }
    return (uint32_t)(e + 127);
}
// one axis of one child: the bytes of its lo (rounded down) and hi (rounded up) on the node's grid
__host__ __device__ inline void quant_child_axis(float child_lo, float child_hi, float node_lo, uint32_t expo, uint32_t& qlo, uint32_t& qhi) {
    const double cell = ldexp(1.0, (int)expo - 127);
    const QuantDiff dl = quant_diff(child_lo, node_lo), dh = quant_diff(child_hi, node_lo);
    double ql = floor(dl.d / cell);  // (a division by a power of two: exact)
    double qh = ceil(dh.d / cell);
    if (ql * cell == dl.d && dl.err < 0) ql -= 1;
    if (qh * cell == dh.d && dh.err > 0) qh += 1;
    ql = ql < 0 ? 0 : (ql > 255 ? 255 : ql);
    qh = qh < 0 ? 0 : (qh > 255 ? 255 : qh);
    qlo = (uint32_t)ql;
    qhi = (uint32_t)qh;
}
// One child slot of a node whose box is [node_lo, node_hi]: its three lo bytes (x | y << 8 | z << 16) and its three hi bytes.
// An absent child keeps the inverted box (lo 255, hi 0).
__host__ __device__ inline void quantize_child(const float* node_lo, const float* node_hi, const float* child_lo, const float* child_hi,
                                               bool present, uint32_t& lo_bytes, uint32_t& hi_bytes) {
    lo_bytes = 0x00ffffffu, hi_bytes = 0;
    if (!present) return;
    lo_bytes = 0;
    for (int ax = 0; ax < 3; ++ax) {
        uint32_t ql, qh;
        quant_child_axis(child_lo[ax], child_hi[ax], node_lo[ax], quant_exponent(node_lo[ax], node_hi[ax]), ql, qh);
        lo_bytes |= ql << (8 * ax);
        hi_bytes |= qh << (8 * ax);
    }
}
// The words of a node's float4 0, 2, 3 and 4 from its box, the inner mask and the eight slots' bytes (float4 1 — first inner
// child, first leaf triangle, leaf mask and counts — is topology and is not made here).
struct NodeWords {
    uint32_t expo_mask;  // float4 0 .w
    uint32_t q[12];      // float4 2, 3, 4
};
__host__ __device__ inline NodeWords pack_node(const float* node_lo, const float* node_hi, uint32_t innermask, const uint32_t* lo_bytes,
                                               const uint32_t* hi_bytes) {
    NodeWords w;
    w.expo_mask = quant_exponent(node_lo[0], node_hi[0]) | (quant_exponent(node_lo[1], node_hi[1]) << 8) |
                  (quant_exponent(node_lo[2], node_hi[2]) << 16) | (innermask << 24);
    for (int row = 0; row < 6; ++row)  // rows: lo.x, lo.y, lo.z, hi.x, hi.y, hi.z; two words of four children each
        for (int g = 0; g < 2; ++g) {
            uint32_t word = 0;
            for (int c = 0; c < 4; ++c) {
                const uint32_t src = row < 3 ? lo_bytes[4 * g + c] : hi_bytes[4 * g + c];
                word |= ((src >> (8 * (row % 3))) & 255u) << (8 * c);
            }
            w.q[2 * row + g] = word;
        }
    return w;
}

// The concatenated vertex array's first index of every mesh (what MeshImage::tri_verts counts from).
inline std::vector<uint32_t> refit_vertex_bases(const std::vector<HostMesh>& meshes) {
    std::vector<uint32_t> base(meshes.size() + 1, 0);
    for (size_t m = 0; m < meshes.size(); ++m) base[m + 1] = base[m] + (uint32_t)(meshes[m].vertices.size() / 3);
    return base;
}

// prim_base = primitive id of the first mesh object (spheres and boxes come before)
inline void build_mesh_image(const srt_object* objects, size_t count, const std::vector<HostMesh>& meshes, int prim_base,
                             MeshImage& out) {
    struct Tri {
        float v0[3], e1[3], e2[3], lo[3], hi[3], c[3];
        int32_t prim, gid, ord;
        uint32_t vert[3];  // in the concatenated vertex array
    };
    std::vector<Tri> tris;
    int mesh_obj = 0;
    const std::vector<uint32_t> vertex_base = refit_vertex_bases(meshes);
    std::vector<MeshImage::ObjectBox> object_boxes;
    std::vector<uint8_t> mesh_dropped(meshes.size(), 0);
    for (size_t i = 0; i < count; ++i) {
        const srt_object& o = objects[i];
        if (o.type != SRT_OBJ_MESH) continue;
        const int prim = prim_base + mesh_obj++;
        MeshImage::ObjectBox ob;
        ob.list_index = (int32_t)i;
        for (int ax = 0; ax < 3; ++ax) ob.lo[ax] = INFINITY, ob.hi[ax] = -INFINITY;
        object_boxes.push_back(ob);
        if (o.mesh < 0 || (size_t)o.mesh >= meshes.size()) continue;
        const HostMesh& m = meshes[(size_t)o.mesh];
        const size_t nv = m.vertices.size() / 3, nt = m.indices.size() / 3;
        for (size_t k = 0; k < nt; ++k) {
            const uint32_t a = m.indices[3 * k], b = m.indices[3 * k + 1], c = m.indices[3 * k + 2];
            if (a >= nv || b >= nv || c >= nv) continue;
            Tri t;
            const uint32_t ix[3] = {a, b, c};
            TriangleRecord r;  // world = vertex + position
            triangle_record(&m.vertices[3 * (size_t)a], &m.vertices[3 * (size_t)b], &m.vertices[3 * (size_t)c], o.position, r);
            for (int ax = 0; ax < 3; ++ax) {
                t.v0[ax] = r.v[0][ax];
                t.e1[ax] = r.e1[ax];
                t.e2[ax] = r.e2[ax];
                t.lo[ax] = r.lo[ax];
                t.hi[ax] = r.hi[ax];
                t.c[ax] = (t.lo[ax] + t.hi[ax]) * 0.5f;
            }
            t.prim = prim;
            t.gid = (int32_t)tris.size();
            t.ord = (int32_t)i;
            for (int q = 0; q < 3; ++q) t.vert[q] = vertex_base[(size_t)o.mesh] + ix[q];
            bool finite = true;  // (every vertex: min / max pass a NaN in the second or third one by)
            for (int q = 0; q < 3; ++q)
                for (int ax = 0; ax < 3; ++ax) finite = finite && std::isfinite(r.v[q][ax]);
            if (!finite) {  // a non-finite triangle can never produce a valid hit
                mesh_dropped[(size_t)o.mesh] = 1;
                continue;
            }
            tris.push_back(t);
            MeshImage::ObjectBox& box = object_boxes.back();
            for (int q = 0; q < 3; ++q)
                for (int ax = 0; ax < 3; ++ax) {
                    box.lo[ax] = box_min(box.lo[ax], m.vertices[3 * (size_t)ix[q] + ax]);
                    box.hi[ax] = box_max(box.hi[ax], m.vertices[3 * (size_t)ix[q] + ax]);
                }
        }
    }
    out = MeshImage();
    out.n_mesh_objects = mesh_obj;
    out.n_tris = (int)tris.size();
    out.object_boxes.swap(object_boxes);
    out.mesh_dropped.swap(mesh_dropped);
    if (tris.empty()) return;

    struct Node {
        float lo[3], hi[3];
        int32_t a, b;  // inner: a = right child, b = -(split axis + 1); leaf: a = first triangle, b = count
    };
    std::vector<Node> nodes;
    nodes.reserve(tris.size() / 2 + 16);
    // Depth-first with an explicit stack (an adversarial mesh — geometrically spaced centroids — lets the
    // binned SAH peel one triangle off per level, so recursion depth would be O(triangles)): the left child
    // of node `me` is me + 1, the right child is numbered when the left subtree is complete.  Beyond
    // SAH_DEPTH levels only median splits are made, which bounds the depth by SAH_DEPTH + log2(n).
    constexpr int SAH_DEPTH = 40;
    struct Frame {
        int b, e, depth, parent;  // parent >= 0: this is that node's right child
    };
    std::vector<Frame> stack;
    stack.push_back(Frame{0, (int)tris.size(), 1, -1});
    int max_depth = 0;
    while (!stack.empty()) {
        const Frame f = stack.back();
        stack.pop_back();
        const int b = f.b, e = f.e, depth = f.depth;
        const int me = (int)nodes.size();
        if (f.parent >= 0) nodes[(size_t)f.parent].a = me;
        nodes.push_back(Node());
        Node nd;
        float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int ax = 0; ax < 3; ++ax) {
            nd.lo[ax] = INFINITY;
            nd.hi[ax] = -INFINITY;
        }
        for (int k = b; k < e; ++k)
            for (int ax = 0; ax < 3; ++ax) {
                nd.lo[ax] = std::min(nd.lo[ax], tris[k].lo[ax]);
                nd.hi[ax] = std::max(nd.hi[ax], tris[k].hi[ax]);
                clo[ax] = std::min(clo[ax], tris[k].c[ax]);
                chi[ax] = std::max(chi[ax], tris[k].c[ax]);
            }
        max_depth = std::max(max_depth, depth);
        if (e - b <= 4) {
            nd.a = b;
            nd.b = e - b;
            nodes[(size_t)me] = nd;
            continue;
        }
        // binned surface-area heuristic (16 bins per axis); falls back to the median of the
        // longest axis when no split is cheaper (leaves must not exceed 4 triangles)
        auto area = [](const float* lo, const float* hi) {
            double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
            return dx < 0 ? 0.0 : 2.0 * (dx * dy + dy * dz + dz * dx);
        };
        constexpr int NB = 16;
        int best_axis = -1, best_bin = -1;
        double best_cost = 1e300;
        for (int ax = 0; ax < 3 && depth <= SAH_DEPTH; ++ax) {
            const double ext = (double)chi[ax] - clo[ax];
            if (!(ext > 0)) continue;
            float blo[NB][3], bhi[NB][3];
            int bcnt[NB];
            for (int q = 0; q < NB; ++q) {
                bcnt[q] = 0;
                for (int a2 = 0; a2 < 3; ++a2) blo[q][a2] = INFINITY, bhi[q][a2] = -INFINITY;
            }
            for (int k = b; k < e; ++k) {
                int q = (int)(((double)tris[k].c[ax] - clo[ax]) / ext * NB);
                q = q < 0 ? 0 : (q >= NB ? NB - 1 : q);
                bcnt[q]++;
                for (int a2 = 0; a2 < 3; ++a2) {
                    blo[q][a2] = std::min(blo[q][a2], tris[k].lo[a2]);
                    bhi[q][a2] = std::max(bhi[q][a2], tris[k].hi[a2]);
                }
            }
            double rarea[NB];
            int rcnt[NB];
            {
                float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
                int c = 0;
                for (int q = NB - 1; q >= 1; --q) {
                    for (int a2 = 0; a2 < 3; ++a2) lo[a2] = std::min(lo[a2], blo[q][a2]), hi[a2] = std::max(hi[a2], bhi[q][a2]);
                    c += bcnt[q];
                    rarea[q] = area(lo, hi);
                    rcnt[q] = c;
                }
            }
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            int c = 0;
            for (int q = 0; q < NB - 1; ++q) {  // split between bin q and q + 1
                for (int a2 = 0; a2 < 3; ++a2) lo[a2] = std::min(lo[a2], blo[q][a2]), hi[a2] = std::max(hi[a2], bhi[q][a2]);
                c += bcnt[q];
                if (c == 0 || rcnt[q + 1] == 0) continue;
                const double cost = area(lo, hi) * c + rarea[q + 1] * rcnt[q + 1];
                if (cost < best_cost) best_cost = cost, best_axis = ax, best_bin = q;
            }
        }
        int mid = b;
        if (best_axis >= 0) {
            const int ax = best_axis;
            const double ext = (double)chi[ax] - clo[ax], lo0 = clo[ax];
            const int bin = best_bin;
            auto it = std::stable_partition(tris.begin() + b, tris.begin() + e, [=](const Tri& x) {
                int q = (int)(((double)x.c[ax] - lo0) / ext * NB);
                q = q < 0 ? 0 : (q >= NB ? NB - 1 : q);
                return q <= bin;
            });
            mid = (int)(it - tris.begin());
        }
        if (best_axis < 0 || mid == b || mid == e) {  // degenerate (or very deep): median of the longest axis
            int axis = 0;
            if (chi[1] - clo[1] > chi[axis] - clo[axis]) axis = 1;
            if (chi[2] - clo[2] > chi[axis] - clo[axis]) axis = 2;
            mid = (b + e) / 2;
            std::nth_element(tris.begin() + b, tris.begin() + mid, tris.begin() + e, [axis](const Tri& x, const Tri& y) {
                return x.c[axis] < y.c[axis] || (x.c[axis] == y.c[axis] && x.gid < y.gid);
            });
        }
        nd.a = -1;  // set when the right child is numbered
        nd.b = 0;
        nodes[(size_t)me] = nd;
        stack.push_back(Frame{mid, e, depth + 1, me});  // right: after the whole left subtree
        stack.push_back(Frame{b, mid, depth + 1, -1});  // left = me + 1
    }
    out.max_depth = max_depth;

    // second pass: collapse the binary tree into 8-wide nodes so that the expected number of wide nodes a random
    // ray visits — the sum of the wide nodes' surface areas — is smallest (the dynamic programme of Ylitie et al.,
    // "Efficient incoherent ray traversal on GPUs through compressed wide BVHs", 2017, with our fixed leaves):
    //   F[n][i] = cheapest way to hang the subtree of binary node n below a wide node using <= i of its child slots
    //           = 0                                              n a leaf (its triangles cost the same in every collapse)
    //           = min(area(n) + D[n][8],  D[n][i])               n inner: its own wide node, or dissolved (i >= 2)
    //   D[n][i] = min over k of F[left][k] + F[right][i - k]     the slots split between n's two children
    // Nodes are in depth-first preorder (children after their parent), so one backward sweep fills the tables.  The greedy
    // collapse used before (keep expanding the child with the largest area) left the 224 x 224 sphere of BASELINE configs
    // 4-5 with 8499 wide nodes of 4.5 children on average, 8 levels deep.
    struct Wide {
        int child[8];  // binary node indices
        int n;
    };
    std::vector<Wide> wide;
    auto area_of = [&](int k) {
        const double dx = (double)nodes[k].hi[0] - nodes[k].lo[0], dy = (double)nodes[k].hi[1] - nodes[k].lo[1],
                     dz = (double)nodes[k].hi[2] - nodes[k].lo[2];
        return 2.0 * (dx * dy + dy * dz + dz * dx);
    };
    struct Plan {
        double F[9];  // F[1..8]
        double D[9];  // D[2..8]
    };
    std::vector<Plan> plan(nodes.size());
    for (size_t kk = nodes.size(); kk-- > 0;) {
        Plan& pl = plan[kk];
        if (nodes[kk].b > 0) {
            for (int i = 0; i <= 8; ++i) pl.F[i] = 0.0, pl.D[i] = 0.0;
            continue;
        }
        const Plan &pa = plan[kk + 1], &pb = plan[(size_t)nodes[kk].a];
        pl.D[0] = pl.D[1] = 1e300;
        for (int i = 2; i <= 8; ++i) {
            double best = 1e300;
            for (int k = 1; k < i; ++k) best = std::min(best, pa.F[k] + pb.F[i - k]);
            pl.D[i] = best;
        }
        const double own = area_of((int)kk) + pl.D[8];
        pl.F[0] = 1e300;
        pl.F[1] = own;
        for (int i = 2; i <= 8; ++i) pl.F[i] = std::min(own, pl.D[i]);
    }
    // children of the wide node that stands for binary inner node k: k's subtree dissolved into <= 8 slots, in spatial
    // (left to right) order.  Explicit stack; a slot count of 1 or a cheaper own node keeps an inner node whole.
    auto children_of = [&](int k, Wide& w) {
        struct Item {
            int node, slots;
            bool dissolve;
        };
        Item st[32];
        int sp = 0;
        w.n = 0;
        st[sp++] = Item{k, 8, true};
        while (sp > 0) {
            const Item it = st[--sp];
            const Node& nd = nodes[(size_t)it.node];
            const Plan& pl = plan[(size_t)it.node];
            if (nd.b > 0 || (!it.dissolve && (it.slots == 1 || pl.F[1] < pl.D[it.slots]))) {
                w.child[w.n++] = it.node;
                continue;
            }
            const Plan &pa = plan[(size_t)it.node + 1], &pb = plan[(size_t)nd.a];
            int bk = 1;
            double best = 1e300;
            for (int q = 1; q < it.slots; ++q)
                if (pa.F[q] + pb.F[it.slots - q] < best) best = pa.F[q] + pb.F[it.slots - q], bk = q;
            st[sp++] = Item{nd.a, it.slots - bk, false};  // right: after the left one (LIFO)
            st[sp++] = Item{it.node + 1, bk, false};
        }
    };
    std::vector<int> wide_of(nodes.size(), -1);  // binary inner node -> wide node that expands it
    std::vector<std::pair<int, int>> todo;       // (binary node, depth), breadth-first so that siblings are neighbours
    if (nodes[0].b > 0) {                        // the whole mesh is one leaf
        Wide w;
        w.child[0] = 0;
        w.n = 1;
        wide.push_back(w);
        out.max_depth = 1;
        out.level_first.push_back(0);
    } else {
        wide_of[0] = 0;
        wide.push_back(Wide());
        todo.push_back({0, 1});
        out.max_depth = 1;
        for (size_t q = 0; q < todo.size(); ++q) {
            const int k = todo[q].first, depth = todo[q].second;
            Wide w;
            children_of(k, w);
            for (int c = 0; c < w.n; ++c)
                if (nodes[w.child[c]].b <= 0) {
                    wide_of[w.child[c]] = (int)wide.size();
                    wide.push_back(Wide());
                    todo.push_back({w.child[c], depth + 1});
                    out.max_depth = std::max(out.max_depth, depth + 1);
                }
            wide[(size_t)wide_of[k]] = w;
        }
        // (todo[q] is wide node q, and the depths never decrease along it)
        for (size_t q = 0; q < todo.size(); ++q)
            if (q == 0 || todo[q].second != todo[q - 1].second) out.level_first.push_back((int32_t)q);
    }
    // triangle storage order: breadth-first like the nodes — for every wide node, the triangles of its leaf
    // children in child order — so that a node needs one "first leaf triangle" instead of a reference per child
    std::vector<int32_t> newpos(tris.size(), -1);  // position in `tris` (build order) -> position in the output
    std::vector<int32_t> first_tri(wide.size(), 0), first_inner(wide.size(), 0);
    {
        int32_t next = 0;
        for (size_t k = 0; k < wide.size(); ++k) {
            first_tri[k] = next;
            first_inner[k] = 0;
            for (int c = 0; c < wide[k].n; ++c) {
                const Node& ch = nodes[wide[k].child[c]];
                if (ch.b > 0)
                    for (int t = 0; t < ch.b; ++t) newpos[(size_t)(ch.a + t)] = next++;
                else if (first_inner[k] == 0)
                    first_inner[k] = wide_of[wide[k].child[c]];
            }
        }
    }
    // quantize the child boxes on the grid of the node's own box (quantize_child, pack_node)
    out.n_nodes = (int)wide.size();
    out.nodes.assign(wide.size() * NODE_VEC4, make_float4(0, 0, 0, 0));
    for (size_t k = 0; k < wide.size(); ++k) {
        const Wide& w = wide[k];
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int c = 0; c < w.n; ++c)
            for (int ax = 0; ax < 3; ++ax) {
                lo[ax] = std::min(lo[ax], nodes[w.child[c]].lo[ax]);
                hi[ax] = std::max(hi[ax], nodes[w.child[c]].hi[ax]);
            }
        uint32_t lo_bytes[8], hi_bytes[8];
        uint32_t innermask = 0, leafmask = 0, counts = 0;
        int expect_inner = first_inner[k];
        for (int c = 0; c < 8; ++c) {
            if (c >= w.n) {  // absent child: inverted box, in neither mask
                quantize_child(lo, hi, lo, hi, false, lo_bytes[c], hi_bytes[c]);
                continue;
            }
            const Node& ch = nodes[w.child[c]];
            quantize_child(lo, hi, ch.lo, ch.hi, true, lo_bytes[c], hi_bytes[c]);
            if (ch.b > 0) {
                leafmask |= 1u << c;
                counts |= (uint32_t)(ch.b - 1) << (2 * c);
            } else {
                innermask |= 1u << c;
                if (wide_of[w.child[c]] != expect_inner++) throw std::logic_error("BVH: inner children are not consecutive");
            }
        }
        const NodeWords nw = pack_node(lo, hi, innermask, lo_bytes, hi_bytes);
        auto word = [&](int q) { return bits_of((int32_t)nw.q[q]); };
        float4* nd = &out.nodes[NODE_VEC4 * k];
        nd[0] = make_float4(lo[0], lo[1], lo[2], bits_of((int32_t)nw.expo_mask));
        nd[1] = make_float4(bits_of(first_inner[k]), bits_of(first_tri[k]), bits_of((int32_t)(leafmask | (counts << 8))), 0.0f);
        nd[2] = make_float4(word(0), word(1), word(2), word(3));    // lo.x[0..7], lo.y[0..7]
        nd[3] = make_float4(word(4), word(5), word(6), word(7));    // lo.z, hi.x
        nd[4] = make_float4(word(8), word(9), word(10), word(11));  // hi.y, hi.z
    }
    out.tris.resize(tris.size() * 3);
    out.gidpos.assign(tris.size(), 0);
    out.tri_verts.assign(tris.size() * 3, 0);
    for (size_t k = 0; k < tris.size(); ++k) {
        const size_t pos = (size_t)newpos[k];
        for (int q = 0; q < 3; ++q) out.tri_verts[3 * pos + q] = tris[k].vert[q];
        out.gidpos[(size_t)tris[k].gid] = (int32_t)pos;
        out.tris[3 * pos] = make_float4(tris[k].v0[0], tris[k].v0[1], tris[k].v0[2], bits_of(tris[k].prim));
        out.tris[3 * pos + 1] = make_float4(tris[k].e1[0], tris[k].e1[1], tris[k].e1[2], bits_of(tris[k].gid));
        out.tris[3 * pos + 2] = make_float4(tris[k].e2[0], tris[k].e2[1], tris[k].e2[2], bits_of(tris[k].ord));
    }
    for (int ax = 0; ax < 3; ++ax) out.center[ax] = 0.5f * (nodes[0].lo[ax] + nodes[0].hi[ax]);
    {  // bounding sphere around the root box's centre: max vertex distance in double, inflated and rounded up
        double r2 = 0;
        for (const Tri& t : tris)
            for (int q = 0; q < 3; ++q) {
                double d2 = 0;
                for (int ax = 0; ax < 3; ++ax) {
                    const double v = (double)t.v0[ax] + (q == 1 ? (double)t.e1[ax] : q == 2 ? (double)t.e2[ax] : 0.0);
                    d2 += (v - (double)out.center[ax]) * (v - (double)out.center[ax]);
                }
                r2 = std::max(r2, d2);
            }
        // (v0 + e1 in double differs from the float vertex by <= 1 ulp of the coordinate: covered by the 1e-5 inflation)
        const double r = sqrt(r2) * (1.0 + 1e-5) + 1e-30;
        out.bs_radius = (float)r;
        if ((double)out.bs_radius < r) out.bs_radius = nextafterf(out.bs_radius, INFINITY);
    }
    for (int ax = 0; ax < 3; ++ax) {
        // half extent rounded up so that [center - half, center + half] contains the root box
        float h = std::max(nodes[0].hi[ax] - out.center[ax], out.center[ax] - nodes[0].lo[ax]);
        out.half[ax] = nextafterf(h * 1.000001f, INFINITY);
    }
}

// ---- refit: the same topology, every object translated anew -----------------------------------------------------------------
// The two steps below are what srt_refit.hip.h runs per thread; they are plain functions so that a host loop can run them too
// (tests/native/refit_check.cpp).  Step 1 rewrites every triangle record and leaves the triangle's exact box in tri_box
// (2 float4: lo, hi); step 2 goes over the levels, deepest first, and for every node takes the exact boxes of its eight child
// slots (leaves from tri_box, inner children from node_box, 2 float4 per node, written one level earlier), joins them, stores
// the join in node_box and requantizes float4 0, 2, 3 and 4 of the node.  Float4 1 and every triangle .w are topology: never written.
__host__ __device__ inline uint32_t word_of(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
__host__ __device__ inline float float_of(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// positions: one float4 per object of the list (xyz = position); the list index is the record's third .w
__host__ __device__ inline void refit_triangle(float4* tris, const uint32_t* tri_verts, const float4* verts, const float4* positions,
                                               float4* tri_box, uint32_t t) {
    float4* rec = tris + 3 * (size_t)t;
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    const float4 a = verts[tri_verts[3 * (size_t)t]], b = verts[tri_verts[3 * (size_t)t + 1]], c = verts[tri_verts[3 * (size_t)t + 2]];
    const float4 p = positions[word_of(r2.w)];
    const float va[3] = {a.x, a.y, a.z}, vb[3] = {b.x, b.y, b.z}, vc[3] = {c.x, c.y, c.z}, pos[3] = {p.x, p.y, p.z};
    TriangleRecord r;
    triangle_record(va, vb, vc, pos, r);
    rec[0] = make_float4(r.v[0][0], r.v[0][1], r.v[0][2], r0.w);
    rec[1] = make_float4(r.e1[0], r.e1[1], r.e1[2], r1.w);
    rec[2] = make_float4(r.e2[0], r.e2[1], r.e2[2], r2.w);
    tri_box[2 * (size_t)t] = make_float4(r.lo[0], r.lo[1], r.lo[2], 0.0f);
    tri_box[2 * (size_t)t + 1] = make_float4(r.hi[0], r.hi[1], r.hi[2], 0.0f);
}

// the exact box of child slot c of node k (false, and the inverted box, for an absent child).  A reference beyond the arrays —
// which a consistent image never holds — counts as absent.
__host__ __device__ inline bool refit_child_box(const float4* nodes, const float4* tri_box, const float4* node_box, uint32_t n_nodes,
                                                uint32_t n_tris, uint32_t k, int c, float* lo, float* hi) {
    for (int ax = 0; ax < 3; ++ax) lo[ax] = INFINITY, hi[ax] = -INFINITY;
    const float4* nd = nodes + NODE_VEC4 * (size_t)k;
    const uint32_t innermask = word_of(nd[0].w) >> 24;
    const float4 topo = nd[1];
    const uint32_t leafmask = word_of(topo.z) & 255u, counts = word_of(topo.z) >> 8;
    const uint32_t below = (1u << c) - 1u;
    if ((innermask >> c) & 1u) {
        uint32_t child = word_of(topo.x), m = innermask & below;
        for (; m; m &= m - 1) ++child;
        if (child >= n_nodes) return false;
        const float4 l = node_box[2 * (size_t)child], h = node_box[2 * (size_t)child + 1];
        lo[0] = l.x, lo[1] = l.y, lo[2] = l.z, hi[0] = h.x, hi[1] = h.y, hi[2] = h.z;
        return true;
    }
    if (!((leafmask >> c) & 1u)) return false;
    uint32_t first = word_of(topo.y);
    for (int q = 0; q < c; ++q)
        if ((leafmask >> q) & 1u) first += 1u + ((counts >> (2 * q)) & 3u);
    const uint32_t n = 1u + ((counts >> (2 * c)) & 3u);
    if (first >= n_tris || n > n_tris - first) return false;
    for (uint32_t t = first; t < first + n; ++t) {
        const float4 l = tri_box[2 * (size_t)t], h = tri_box[2 * (size_t)t + 1];
        lo[0] = box_min(lo[0], l.x), lo[1] = box_min(lo[1], l.y), lo[2] = box_min(lo[2], l.z);
        hi[0] = box_max(hi[0], h.x), hi[1] = box_max(hi[1], h.y), hi[2] = box_max(hi[2], h.z);
    }
    return true;
}

// one node on the host: what the eight lanes of refit_level_kernel do together
inline void refit_node(float4* nodes, const float4* tri_box, float4* node_box, uint32_t n_nodes, uint32_t n_tris, uint32_t k) {
    float clo[8][3], chi[8][3], lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool present[8];
    for (int c = 0; c < 8; ++c) {
        present[c] = refit_child_box(nodes, tri_box, node_box, n_nodes, n_tris, k, c, clo[c], chi[c]);
        for (int ax = 0; ax < 3; ++ax) lo[ax] = box_min(lo[ax], clo[c][ax]), hi[ax] = box_max(hi[ax], chi[c][ax]);
    }
    uint32_t lo_bytes[8], hi_bytes[8];
    for (int c = 0; c < 8; ++c) quantize_child(lo, hi, clo[c], chi[c], present[c], lo_bytes[c], hi_bytes[c]);
    float4* nd = nodes + NODE_VEC4 * (size_t)k;
    const NodeWords w = pack_node(lo, hi, word_of(nd[0].w) >> 24, lo_bytes, hi_bytes);
    node_box[2 * (size_t)k] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    node_box[2 * (size_t)k + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    nd[0] = make_float4(lo[0], lo[1], lo[2], float_of(w.expo_mask));
    nd[2] = make_float4(float_of(w.q[0]), float_of(w.q[1]), float_of(w.q[2]), float_of(w.q[3]));
    nd[3] = make_float4(float_of(w.q[4]), float_of(w.q[5]), float_of(w.q[6]), float_of(w.q[7]));
    nd[4] = make_float4(float_of(w.q[8]), float_of(w.q[9]), float_of(w.q[10]), float_of(w.q[11]));
}

// The meshes' vertices as the refit reads them: one float4 per vertex, all meshes one after the other.
inline std::vector<float4> refit_vertices(const std::vector<HostMesh>& meshes) {
    std::vector<float4> v;
    for (const HostMesh& m : meshes)
        for (size_t k = 0; k + 2 < m.vertices.size(); k += 3) v.push_back(make_float4(m.vertices[k], m.vertices[k + 1], m.vertices[k + 2], 0.0f));
    return v;
}

// Root box, centre, half extent and bounding sphere of the image's triangles with every mesh object at objects[list index].position,
// from the host alone.  Rounded addition is monotone, so min over vertices of fl(v + p) is fl(min v + p): the union over the mesh
// objects of (local box + position) is the box the build's min / max over the world vertices gives (the same floats; where a
// -0 and a +0 tie, the sign of a zero bound is the only thing that can differ).  center and half are then the build's
// expressions.  bs_radius is the root box's half-diagonal about center in double, inflated and rounded up the way the build
// rounds: it encloses every vertex, and is looser than the build's largest vertex distance.  False when no triangle is valid.
inline bool refit_root(const MeshImage& img, const srt_object* objects, float* lo, float* hi, float* center, float* half, float& bs_radius) {
    for (int ax = 0; ax < 3; ++ax) lo[ax] = INFINITY, hi[ax] = -INFINITY;
    for (const MeshImage::ObjectBox& b : img.object_boxes) {
        if (!(b.lo[0] <= b.hi[0])) continue;  // no valid triangle
        const float* p = objects[b.list_index].position;
        for (int ax = 0; ax < 3; ++ax) lo[ax] = box_min(lo[ax], b.lo[ax] + p[ax]), hi[ax] = box_max(hi[ax], b.hi[ax] + p[ax]);
    }
    if (!(lo[0] <= hi[0])) return false;
    double d2 = 0;
    for (int ax = 0; ax < 3; ++ax) {
        center[ax] = 0.5f * (lo[ax] + hi[ax]);
        const float h = std::max(hi[ax] - center[ax], center[ax] - lo[ax]);
        half[ax] = nextafterf(h * 1.000001f, INFINITY);
        const double d = std::max((double)hi[ax] - (double)center[ax], (double)center[ax] - (double)lo[ax]);
        d2 += d * d;
    }
    const double r = sqrt(d2) * (1.0 + 1e-5) + 1e-30;
    bs_radius = (float)r;
    if ((double)bs_radius < r) bs_radius = nextafterf(bs_radius, INFINITY);
    return true;
}

}  // namespace srt
