// srt::rows_six_waves (csrc/srt_launch_shape.h) — which rows launches run the six-wave kernel: true where six workgroups' LDS,
// each rounded up to the allocation granule, fit into a CU's 160 KiB.  Checked at the edge (the largest fitting size, one byte
// and one granule above it), for requests that fill LDS, and for the LDS bytes of the shipped scenes, whose images are built here
// by the library's own build_scene_image.
//   six_wave_rule_check <scene.json>...          the checks; every scene given must pass the rule.  Prints "ok <checks> edge <bytes>".
//   six_wave_rule_check --grow <scene.json>      reads "x y z radius" lines; prints "<k> <lds bytes> <0|1>" for the scene plus
//                                                the first k of those spheres, k = 0 .. lines (what tests/test_gpu_six_waves.py
//                                                takes its sphere count from).
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "scene.hpp"
#include "srt_launch_shape.h"
#include "srt_scene_image.h"

static int checks = 0, failed = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        ++checks;                                                    \
        if (!(c)) {                                                  \
            ++failed;                                                \
            printf("FAILED line %d: %s\n", __LINE__, #c);            \
        }                                                            \
    } while (0)

// LDS bytes of a rows workgroup for these objects: the clustered scene image and the waves' scratch without the ring
static size_t rows_lds_bytes(const std::vector<srt_object>& objs) {
    std::vector<float4> img;
    const srt::SceneLayout L = srt::build_scene_image(objs.data(), objs.size(), true, img);
    return (size_t)(L.total_vec4 > 0 ? L.total_vec4 : 1) * sizeof(float4) + srt::SHAPE_ROWS_WG_SCRATCH_BYTES;
}

static std::vector<srt_object> load(const char* path) {
    srt_host::Scene s(path);
    s.Load();
    return s.Flatten();
}

int main(int argc, char** argv) {
    using namespace srt;
    if (argc == 3 && !strcmp(argv[1], "--grow")) {
        std::vector<srt_object> objs = load(argv[2]);
        if (objs.empty()) return 2;
        int k = 0;
        float x, y, z, r;
        do {
            const size_t b = rows_lds_bytes(objs);
            printf("%d %zu %d\n", k++, b, rows_six_waves(b) ? 1 : 0);
            if (scanf("%f %f %f %f", &x, &y, &z, &r) != 4) break;
            srt_object o{};
            o.type = SRT_OBJ_SPHERE, o.mesh = -1, o.radius = r;
            o.position[0] = x, o.position[1] = y, o.position[2] = z;
            objs.push_back(o);
        } while (true);
        return 0;
    }
    const size_t G = LDS_GRANULE_BYTES, CU = LDS_BYTES_PER_CU;
    CHECK(CU == 163840 && G == 1280 && CU % G == 0);
    // the edge: floor(CU / 6) rounded DOWN to the granule
    const size_t edge = CU / 6 / G * G;
    CHECK(edge == 26880);
    CHECK(rows_six_waves(edge) && 6 * edge <= CU);
    CHECK(rows_six_waves(edge - 1) && rows_six_waves(edge - G + 1));
    CHECK(!rows_six_waves(edge + 1));  // occupies one more granule: six of those are 168 960 bytes
    CHECK(!rows_six_waves(edge + G));
    CHECK(6 * (edge + G) > CU);
    // a size whose six copies fit BEFORE rounding, but not once each is rounded up to the granule
    CHECK(6 * (size_t)27300 <= CU && !rows_six_waves(27300));
    // at the edge the answer is the same for a granule of 512 bytes
    CHECK(6 * ((edge + 511) / 512 * 512) <= CU);
    // the scratch alone, and the smallest image
    CHECK(rows_six_waves(SHAPE_ROWS_WG_SCRATCH_BYTES) && rows_six_waves(SHAPE_ROWS_WG_SCRATCH_BYTES + 16));
    CHECK(SHAPE_ROWS_WG_SCRATCH_BYTES < edge);
    // images that fill LDS: the 64 KiB a workgroup may take by default, a whole CU's, and requests beyond it (no wrap)
    CHECK(!rows_six_waves(64 * 1024) && !rows_six_waves(64 * 1024 - 8192));
    CHECK(!rows_six_waves(CU) && !rows_six_waves(CU + 1) && !rows_six_waves(~(size_t)0) && !rows_six_waves(~(size_t)0 / 6 + 1));
    // five fit where six do not: the five-wave kernel keeps its occupancy just above the edge
    CHECK(5 * (edge + G) <= CU);
    // the shipped scenes
    for (int i = 1; i < argc; ++i) {
        const std::vector<srt_object> objs = load(argv[i]);
        CHECK(!objs.empty());
        const size_t b = rows_lds_bytes(objs);
        printf("%s: %zu objects, %zu bytes of LDS per rows workgroup, %zu granules\n", argv[i], objs.size(), b, (b + G - 1) / G);
        CHECK(b > SHAPE_ROWS_WG_SCRATCH_BYTES && rows_six_waves(b));
    }
    if (failed) return 1;
    printf("ok %d edge %zu\n", checks, edge);
    return 0;
}
