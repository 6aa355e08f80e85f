// srt::fold_from_rows (csrc/srt_launch_shape.h) — which launches send their sample colours through rows of the sample buffer —
// on both sides of the sample minimum and of the byte cap, for every excluded launch kind, and through plan_launch_shape /
// finish_launch_shape for the shapes real requests take.
//   rows_rule_check          the checks.  Prints "ok <checks> min <ROWS_MIN_SAMPLES>".
//   rows_rule_check --ask    reads requests "w rows spp cu_count mesh preview steps block_grid scene_in_lds lds_bytes" (w x rows: the
//                            launch's lanes; lds_bytes: what a rows workgroup asks for, six_wave_rule_check's figure) and prints for
//                            each "tile_h chunks wg8 rows six rows_bytes": the finished shape of a first launch, fold_from_rows,
//                            rows_six_waves(lds_bytes), and the rows' bytes (0 without rows).  The GPU tests take the kernel they
//                            expect from here (tests/test_gpu_rows_at_scale.py, tests/test_gpu_paths.py).
#include <stdio.h>
#include <string.h>

#include "srt_launch_shape.h"

static int checks = 0, failed = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        ++checks;                                                    \
        if (!(c)) {                                                  \
            ++failed;                                                \
            printf("FAILED line %d: %s\n", __LINE__, #c);            \
        }                                                            \
    } while (0)

// the finished shape of a request, as srt_render plans it (no work record)
static srt::LaunchShape shape_of(srt::ShapeRequest& q, int w, int rows, uint32_t spp, bool mesh = false) {
    q = srt::ShapeRequest();
    q.grid_w = w, q.grid_h = rows, q.rows = rows, q.sample_count = spp, q.mesh = mesh;
    srt::LaunchShape s = srt::plan_launch_shape(q, nullptr);
    srt::finish_launch_shape(s, spp);
    return s;
}

// --ask: the rule's answer for the requests on stdin, as srt_render plans a first launch (no work record, no overrides)
static int ask() {
    long long w, rows;
    unsigned spp;
    int cu, mesh, preview, steps, block_grid, in_lds;
    unsigned long long lds_bytes;
    int n;
    while ((n = scanf("%lld %lld %u %d %d %d %d %d %d %llu", &w, &rows, &spp, &cu, &mesh, &preview, &steps, &block_grid, &in_lds, &lds_bytes)) == 10) {
        if (w < 1 || rows < 1 || rows > 0x7FFFFFFF || spp < 1 || cu < 1 || steps < 1) return 2;
        srt::ShapeRequest q;
        q.grid_w = w, q.grid_h = rows, q.rows = (int)rows, q.sample_count = spp, q.cu_count = cu;
        q.mesh = mesh != 0, q.steps = steps, q.block_grid = block_grid != 0;
        srt::LaunchShape s = srt::plan_launch_shape(q, nullptr);
        srt::finish_launch_shape(s, spp);
        const bool r = srt::fold_from_rows(s, q, preview != 0, in_lds != 0);
        printf("%d %d %lld %d %d %llu\n", s.tile_h, s.chunks, s.wg8, r ? 1 : 0, srt::rows_six_waves((size_t)lds_bytes) ? 1 : 0,
               r ? srt::rows_bytes(s, spp) : 0ull);
    }
    return n == EOF ? 0 : 2;  // (a line that does not parse is an error, not the end)
}

int main(int argc, char** argv) {
    using namespace srt;
    if (argc == 2 && !strcmp(argv[1], "--ask")) return ask();
    if (argc != 1) return 2;
    const uint32_t MIN = ROWS_MIN_SAMPLES;
    CHECK(MIN >= 2 && MIN <= 16);  // (from 16 samples on small frames take small tiles: below that the minimum can be met on any frame)
    ShapeRequest q;
    // a small frame, as the GPU tests render it: 40 x 24 is 3 x 2 blocks of 16 x 16
    LaunchShape s = shape_of(q, 40, 24, MIN);
    CHECK(s.wg8 == 6 && s.tile_h == 8 && s.chunks == 1);
    CHECK(fold_from_rows(s, q, false, true));
    CHECK(rows_bytes(s, MIN) == 6ull * 4 * MIN * 1024);
    s = shape_of(q, 40, 24, MIN - 1);
    CHECK(!fold_from_rows(s, q, false, true));
    s = shape_of(q, 40, 24, 15);
    CHECK(fold_from_rows(s, q, false, true));
    // the excluded kinds, each on a request that takes the path without them
    s = shape_of(q, 40, 24, 8);
    CHECK(fold_from_rows(s, q, false, true) && !fold_from_rows(s, q, true, true));  // the preview shader
    {
        ShapeRequest b = q;
        b.block_grid = true;
        CHECK(!fold_from_rows(s, b, false, true));
        b = q, b.steps = 2;  // progressive blocks, one lane per pixel
        CHECK(!fold_from_rows(s, b, false, true));
        LaunchShape t = s;
        t.tile_h = 4;  // small tiles
        CHECK(!fold_from_rows(t, q, false, true));
        t = s, t.chunks = 2, t.chunk = 4;  // sample chunks
        CHECK(!fold_from_rows(t, q, false, true));
        t = s, t.wg8 = 0;
        CHECK(!fold_from_rows(t, q, false, true));
    }
    // 16 samples and more on a frame of few blocks: small tiles, the ring
    s = shape_of(q, 40, 24, 32);
    CHECK(s.tile_h < 8 && !fold_from_rows(s, q, false, true));
    // ... 64 and more: sample chunks
    s = shape_of(q, 40, 24, 64);
    CHECK(s.chunks >= 2 && !fold_from_rows(s, q, false, true));
    // whole 1080p frames: 32 samples (1.0 GiB of rows) take the path, the analytic 64 are chunked, mesh scenes and scene images in memory keep the ring
    s = shape_of(q, 1920, 1080, 32);
    CHECK(s.tile_h == 8 && s.chunks == 1 && s.wg8 == 120 * 68 && fold_from_rows(s, q, false, true));
    CHECK(rows_bytes(s, 32) == 120ull * 68 * 4 * 32 * 1024);
    s = shape_of(q, 1920, 1080, 64, true);
    CHECK(s.chunks == 1 && s.tile_h == 8 && !fold_from_rows(s, q, false, true));
    s = shape_of(q, 40, 24, 8, true);
    CHECK(s.chunks == 1 && s.tile_h == 8 && !fold_from_rows(s, q, false, true));
    s = shape_of(q, 1920, 1080, 32);  // a scene image in memory
    CHECK(!fold_from_rows(s, q, false, false));
    s = shape_of(q, 40, 24, 8);
    CHECK(!fold_from_rows(s, q, false, false));
    s = shape_of(q, 1920, 1080, 64);
    CHECK(s.chunks >= 2 && !fold_from_rows(s, q, false, true));
    s = shape_of(q, 1920, 1080, 1);
    CHECK(!fold_from_rows(s, q, false, true));
    // the byte cap, exactly: tiles x samples KiB against ROWS_MAX_BYTES
    {
        LaunchShape t;
        t.tile_h = 8, t.chunks = 1;
        ShapeRequest r;
        r.sample_count = 16;
        const unsigned long long tiles_at_cap = ROWS_MAX_BYTES / (16ull * 1024);
        CHECK(tiles_at_cap % 4 == 0);
        t.wg8 = (long long)(tiles_at_cap / 4);
        CHECK(rows_bytes(t, 16) == ROWS_MAX_BYTES && fold_from_rows(t, r, false, true));
        t.wg8 += 1;
        CHECK(rows_bytes(t, 16) > ROWS_MAX_BYTES && !fold_from_rows(t, r, false, true));
        r.sample_count = 17, t.wg8 -= 1;
        CHECK(!fold_from_rows(t, r, false, true));
        // the largest request srt_render accepts on the largest grid does not wrap around
        r.sample_count = 1u << 20, t.wg8 = 1ll << 40;
        CHECK(!fold_from_rows(t, r, false, true));
        r.sample_count = 0xFFFFFFFFu, t.wg8 = 0x7FFFFFFFFFFFFFFFll;
        CHECK(!fold_from_rows(t, r, false, true));
        r.sample_count = 1u << 20, t.wg8 = 1;  // (4 GiB for one block of tiles: the cap exactly)
        CHECK(fold_from_rows(t, r, false, true));
    }
    // a 4K frame (129600 tiles): 32 samples stay under the cap (3.96 GiB), 33 do not
    s = shape_of(q, 3840, 2160, 32);
    CHECK(s.wg8 == 240 * 135 && s.chunks == 1 && fold_from_rows(s, q, false, true));
    s = shape_of(q, 3840, 2160, 33);
    CHECK(s.chunks == 1 && !fold_from_rows(s, q, false, true));
    if (failed) return 1;
    printf("ok %d min %u\n", checks, MIN);
    return 0;
}
