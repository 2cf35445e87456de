// Stress driver of the sanitizer builds (`make sanitize`): HostPool, the seam's lock order across two caller threads and a fork, the banded add, the live rectangle of degenerate scenes, a
// frame's checkpoint written and read back whole and cut short, a frame's bookkeeping through whole life cycles (slices merged in every order; save, load and go on), and the run-time instantiations' code cache from several threads at once.  Built twice, with -fsanitize=thread and -fsanitize=address,undefined (Makefile).
// usage: stress_<san> [iterations]      exit code 0 = every check passed (the sanitizer itself aborts or reports on stderr otherwise)
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <initializer_list>
#include <vector>

#include "../../include/kyhip.h"

extern "C" {
int kyhostcheck_seam_stress(int iterations);
int kyhostcheck_add_rows(int width, int height, int stride_px, int n_threads, int rounds);
int kyhostcheck_chunks(int spp);
int kyhostcheck_screen_bound(void);
int kyhostcheck_filter(void);
int kyhostcheck_lens(void);
int kyhostcheck_jit_stress(int n_threads, int rounds);
int kyhostcheck_checkpoint(const ky_render_params* p, int noise, int blocks, int check_blocks, const int* counts_in, const int32_t* states, size_t check_bytes,
                           size_t* offsets, int* counts_out, void* state_out, size_t state_capacity);
int kyhostcheck_book(const ky_render_params* p, uint64_t scene_hash, uint64_t source_hash, const int* books, int n_books, const int* ops, int n_ops, int* records, unsigned char* slots_out,
                     size_t slot_capacity, size_t* slot_bytes);
const char* kyhip_jit_status(void);
}

// whole life cycles of a frame's bookkeeping (kyhostcheck_book, ky_hostcheck.cpp): 0, or the number of the comparison that went wrong
static int book_scripts(const ky_render_params& p) {
    enum { PASS, SAVE, LOAD, MERGE, MERGE_FROM, TRACK_NOISE, TRACK_BLOCKS, NOTHING };
    enum { STATUS, FRONT, HELD, N_RANGES, OWN_FIRST, OWN_END, BATCHES, N_PREV, PASSES, N_LIVE, STATE_BYTES, RECORD = 11 + 2 * KYHIP_SLICE_MAX_RANGES };
    struct Op { int op, book, arg, arg2; };
    std::vector<int> rec;
    size_t sizes[4];
    auto run = [&](const std::vector<int>& books, const std::vector<Op>& ops) {
        rec.assign(ops.size() * RECORD, -1);
        if (kyhostcheck_book(&p, 0x1234, 0, books.data(), (int)books.size() / 2, &ops[0].op, (int)ops.size(), rec.data(), nullptr, 0, sizes) != KY_OK) return false;
        for (size_t k = 0; k < ops.size(); ++k)
            if (rec[k * RECORD + STATUS] != KY_OK) return false;
        return true;
    };
    auto at = [&](size_t k, int field) { return rec[k * RECORD + field]; };
    {   // three slices and a collector that track noise, rendered in passes of 100, saved, and merged into the collector in every order
        const std::vector<int> books = {0, 48, 48, 308, 308, 500, 0, 0};
        std::vector<Op> ops;
        for (int b = 0; b < 4; ++b) ops.push_back({TRACK_NOISE, b, 0, 0});
        for (int b = 0; b < 4; ++b) {
            for (int k = 0; k < 4; ++k) ops.push_back({PASS, b, 100, 0});
            ops.push_back({SAVE, b, b, 0});
        }
        const int held[4] = {48, 260, 192, 0}, front[4] = {48, 308, 500, 0};
        const int order[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        for (const int* o : order) {
            std::vector<Op> script = ops;
            for (int k = 0; k < 3; ++k) script.push_back({MERGE, 3, o[k], 0});
            if (!run(books, script)) return 1;
            int batches = 0;
            for (int b = 0; b < 4; ++b) {
                const size_t k = 4 + 5 * (size_t)b + 4;   // the book's save
                if (at(k, HELD) != held[b] || at(k, FRONT) != front[b] || sizes[b] != (size_t)at(k, STATE_BYTES) || sizes[b] != sizes[0]) return 2;
                batches += at(k, BATCHES);
            }
            const size_t last = script.size() - 1;
            if (at(last, HELD) != 500 || at(last, N_RANGES) != 1 || at(last, STATE_BYTES + 1) != 0 || at(last, STATE_BYTES + 2) != 500 || at(last, BATCHES) != batches) return 3;
            if (o[0] + o[1] == 2 && (at(last - 1, N_RANGES) != 2 || at(last - 1, HELD) != 240)) return 4;   // [(0, 48), (308, 500)]
        }
    }
    // what one book saves at every fifth boundary a fresh one loads, and both go on alike: all four (noise, blocks), and the slice 48..308 with and without noise
    for (int config = 0; config < 6; ++config) {
        const bool noise = config & 1, blocks = config == 2 || config == 3, slice = config >= 4;
        const std::vector<int> books = slice ? std::vector<int>{48, 308, 48, 308} : std::vector<int>{0, 500, 0, 500};
        const int n_bounds = slice ? 17 : 51;   // (the chunks of 500 samples: 2 of 24, 17 of 16 up to 308, then 16 of 8 and 16 of 4)
        for (int k = 5; k <= n_bounds; k += 5) {
            std::vector<Op> ops;
            for (int b = 0; b < 2; ++b) {
                if (noise) ops.push_back({TRACK_NOISE, b, 0, 0});
                if (blocks) ops.push_back({TRACK_BLOCKS, b, 0, 0});
            }
            for (int i = 0; i < k; ++i) ops.push_back({PASS, 0, 1, 0});
            const size_t saved = ops.size();
            ops.push_back({SAVE, 0, 2, 0});
            ops.push_back({LOAD, 1, 2, 0});
            for (int i = k; i <= n_bounds; ++i) { ops.push_back({PASS, 0, 1, 0}); ops.push_back({PASS, 1, 1, 0}); }
            if (!run(books, ops)) return 5;
            if (at(saved, BATCHES) != (noise ? k : 0) || at(saved, PASSES) != (blocks ? k : 0) || at(saved, HELD) != at(saved, FRONT) - books[0]) return 6;
            for (size_t a = saved; a + 1 < ops.size(); a += 2)
                for (int f = FRONT; f < RECORD; ++f)
                    if (at(a, f) != at(a + 1, f)) return 7;
            if (at(ops.size() - 1, FRONT) != books[1]) return 8;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    const int it = argc > 1 ? std::atoi(argv[1]) : 2000;
    int rc = kyhostcheck_seam_stress(it);
    std::printf("seam_stress(%d) -> %d\n", it, rc);
    if (rc) return 1;
    rc = kyhostcheck_add_rows(253, 97, 260, 4, 5);
    std::printf("add_rows -> %d\n", rc);
    if (rc) return 2;
    for (int spp : {1, 2, 3, 4, 5, 16, 63, 64, 65, 447, 448, 449, 472, 1024, 4096, 16384, 100003})
        if (kyhostcheck_chunks(spp) < 1) { std::printf("chunks(%d) failed\n", spp); return 3; }
    std::printf("chunk schedules ok\n");
    rc = kyhostcheck_screen_bound();   // the live rectangle on degenerate scenes (a camera on / inside the bound, NaN, radius zero, no surfaces)
    std::printf("screen_bound -> %d\n", rc);
    if (rc) return 5;
    rc = kyhostcheck_filter();   // pixel filters: check, defaults, table, the header fold, the widened live rectangle
    std::printf("filter -> %d\n", rc);
    if (rc) return 9;
    rc = kyhostcheck_lens();   // the lens: launch constants, the header fold beside the filter's, refusals that name the lens
    std::printf("lens -> %d\n", rc);
    if (rc) return 10;
    {   // a checkpoint of a 40 x 24 frame (ragged tiles) for what it can track: accepted whole, refused one byte short of every part's end and by the other `blocks`
        ky_render_params p = {};
        p.integrator = KY_INTEGRATOR_PATH_TRACING_ITERATION; p.max_path_depth = 5; p.direct_sample = KY_DIRECT_BOTH_MIS; p.samples_per_pixel = 500; p.sampler = KY_SAMPLER_RANDOM;
        p.width = 40; p.height = 24; p.tile_w = 16; p.tile_h = 16; p.tile_first = 0; p.tile_step = 1;
        const int counts[4] = {224, 3, 224, 5};
        for (int k = 0; k < 4; ++k) {
            const int noise = k & 1, blocks = k >> 1;
            size_t at[6];
            int back[5];
            if (kyhostcheck_checkpoint(&p, noise, blocks, blocks, counts, nullptr, (size_t)-1, at, back, nullptr, 0) != KY_OK || back[1] != 224) { std::printf("checkpoint(%d) failed\n", k); return 6; }
            for (size_t end : at)
                if (kyhostcheck_checkpoint(&p, noise, blocks, blocks, counts, nullptr, end - 1, at, back, nullptr, 0) != KY_ERR_INVALID_VALUE) { std::printf("checkpoint(%d) cut at %zu accepted\n", k, end); return 6; }
            if (kyhostcheck_checkpoint(&p, noise, blocks, !blocks, counts, nullptr, (size_t)-1, at, back, nullptr, 0) != KY_ERR_INVALID_VALUE) return 6;
        }
        std::printf("checkpoints ok\n");
        rc = book_scripts(p);   // ... and its bookkeeping through whole life cycles: slices merged in every order; save, load and go on
        std::printf("book scripts -> %d\n", rc);
        if (rc) return 7;
    }
    if (std::getenv("KYHIP_HIPCC")) {   // the cache's threads: only with a stand-in compiler (the real one takes seconds per object)
        const int got = kyhostcheck_jit_stress(6, 4);
        std::printf("jit_stress -> %d objects of 24 requests; status: %s\n", got, kyhip_jit_status());
        if (got != 24) return 4;
    }
    return 0;
}
