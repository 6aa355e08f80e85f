// srt_refit.hip.h — gfx950 refit of the mesh image (srt_update_scene under SRT_UPDATE_REFIT): every object is placed by its
// position alone, so an update that only moves objects keeps the 8-wide tree's topology and changes nothing but the triangle
// records and the quantized child boxes.  Both are rewritten in place, in HBM, behind every render already on the stream.
//
//   refit_triangles_kernel  one thread per triangle, leaf order: three 16-byte vertex gathers, + position[list index], the three
//                           float4 of the record (its .w words kept) and the triangle's exact box (2 float4) to a side array.
//                           A stream: 48 B of record read and written, 48 B gathered, 32 B of box out.
//   refit_level_kernel      one launch per level of the tree, deepest first.  Eight lanes per node, one per child slot: a lane
//                           takes its child's exact box — a leaf's from the 1..4 triangle boxes, an inner child's from the node
//                           side array the previous launch wrote — the eight join by three xor-shuffles, every lane quantizes
//                           its own child on the joined box (srt_mesh_bvh.h: the build's own functions), the bytes go round by
//                           shuffles, and lanes 0..5 store float4 0, 2, 3, 4 of the node and the two of its exact box.
//                           Float4 1 (topology) is read, never written.
//
// Stream order is the only synchronisation: a level reads what the launch before it wrote, nothing within a launch depends on
// another workgroup.  No atomics, no LDS, no scratch; every group of eight lanes lies inside one wave and is either whole or idle
// (threads = 8 * nodes, a workgroup of 256 covers 32 nodes), so the shuffles never read an exited lane.  The arithmetic is the
// build's: binary32 adds and min / max for the boxes, binary64 TwoSum differences for the bytes (no contraction, no fast-math).
#pragma once

#include <hip/hip_runtime.h>

#include "srt_mesh_bvh.h"

namespace srt {

constexpr int REFIT_THREADS = 256;

struct RefitLaunch {
    float4* tris;               // the image's triangle records (rewritten)
    float4* nodes;              // the image's nodes (float4 0, 2, 3, 4 rewritten)
    const uint32_t* tri_verts;  // 3 per triangle: indices into verts
    const float4* verts;        // every mesh's local vertices
    const float4* positions;    // one per object of the list
    float4* tri_box;            // 2 per triangle: exact lo, hi
    float4* node_box;           // 2 per node: exact lo, hi
    uint32_t n_tris, n_nodes;
    uint32_t level_first, level_nodes;  // refit_level_kernel: the nodes of this launch
};

__global__ void __launch_bounds__(REFIT_THREADS) refit_triangles_kernel(const RefitLaunch R) {
    const uint32_t t = blockIdx.x * REFIT_THREADS + threadIdx.x;
    if (t >= R.n_tris) return;
    refit_triangle(R.tris, R.tri_verts, R.verts, R.positions, R.tri_box, t);
}

__global__ void __launch_bounds__(REFIT_THREADS) refit_level_kernel(const RefitLaunch R) {
    const uint32_t g = (blockIdx.x * REFIT_THREADS + threadIdx.x) >> 3;  // node of the level
    const int c = (int)(threadIdx.x & 7u);
    if (g >= R.level_nodes) return;  // (a whole group of eight at once)
    const uint32_t k = R.level_first + g;
    if (k >= R.n_nodes) return;
    float clo[3], chi[3];
    const bool present = refit_child_box(R.nodes, R.tri_box, R.node_box, R.n_nodes, R.n_tris, k, c, clo, chi);
    float lo[3], hi[3];
    for (int ax = 0; ax < 3; ++ax) {
        lo[ax] = clo[ax], hi[ax] = chi[ax];
        for (int m = 1; m < 8; m <<= 1) {
            lo[ax] = box_min(lo[ax], __shfl_xor(lo[ax], m, 8));
            hi[ax] = box_max(hi[ax], __shfl_xor(hi[ax], m, 8));
        }
    }
    uint32_t my_lo, my_hi;
    quantize_child(lo, hi, clo, chi, present, my_lo, my_hi);
    uint32_t lo_bytes[8], hi_bytes[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        lo_bytes[j] = (uint32_t)__shfl((int)my_lo, j, 8);
        hi_bytes[j] = (uint32_t)__shfl((int)my_hi, j, 8);
    }
    float4* nd = R.nodes + NODE_VEC4 * (size_t)k;
    const NodeWords w = pack_node(lo, hi, word_of(nd[0].w) >> 24, lo_bytes, hi_bytes);
    if (c == 0) nd[0] = make_float4(lo[0], lo[1], lo[2], float_of(w.expo_mask));
    if (c == 1) nd[2] = make_float4(float_of(w.q[0]), float_of(w.q[1]), float_of(w.q[2]), float_of(w.q[3]));
    if (c == 2) nd[3] = make_float4(float_of(w.q[4]), float_of(w.q[5]), float_of(w.q[6]), float_of(w.q[7]));
    if (c == 3) nd[4] = make_float4(float_of(w.q[8]), float_of(w.q[9]), float_of(w.q[10]), float_of(w.q[11]));
    if (c == 4) R.node_box[2 * (size_t)k] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    if (c == 5) R.node_box[2 * (size_t)k + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
}

}  // namespace srt
