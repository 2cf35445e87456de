// Stress driver of the sanitizer builds (`make sanitize`): HostPool, the seam's lock order across two caller threads and a fork, the banded add, the live rectangle of degenerate scenes, a
// frame's checkpoint written and read back whole and cut short, and the run-time instantiations' code cache from several threads at once.  Built twice, with -fsanitize=thread and -fsanitize=address,undefined (Makefile).
// usage: stress_<san> [iterations]      exit code 0 = every check passed (the sanitizer itself aborts or reports on stderr otherwise)
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <initializer_list>

#include "../../include/kyhip.h"

extern "C" {
int kyhostcheck_seam_stress(int iterations);
int kyhostcheck_add_rows(int width, int height, int stride_px, int n_threads, int rounds);
int kyhostcheck_chunks(int spp);
int kyhostcheck_screen_bound(void);
int kyhostcheck_jit_stress(int n_threads, int rounds);
int kyhostcheck_checkpoint(const ky_render_params* p, int noise, int blocks, int check_blocks, const int* counts_in, const int32_t* states, size_t check_bytes,
                           size_t* offsets, int* counts_out, void* state_out, size_t state_capacity);
const char* kyhip_jit_status(void);
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
    }
    if (std::getenv("KYHIP_HIPCC")) {   // the cache's threads: only with a stand-in compiler (the real one takes seconds per object)
        const int got = kyhostcheck_jit_stress(6, 4);
        std::printf("jit_stress -> %d objects of 24 requests; status: %s\n", got, kyhip_jit_status());
        if (got != 24) return 4;
    }
    return 0;
}
