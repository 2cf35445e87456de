/*
 * ky_hostcheck.cpp -- entry points of the SANITIZER builds only (`make sanitize`: g++ -fsanitize=address,undefined and -fsanitize=thread over ky_pack.cpp,
 * ky_jit.cpp and this file; never part of libkyhip.so).  They drive the host code that has no C-ABI entry of its own -- scene packing into a heap DScene,
 * the scene cache's keys, the chunk schedule, the banded add, HostPool and the seam's lock order under contention and across a fork -- so that
 * tests/test_sanitize.py can run it under the sanitizers from Python (ctypes) or from the stress binary (tools/sanitize/stress.cpp).  A frame's bookkeeping
 * (FrameBook, ky_frame_book.hpp), a checkpoint's layout, writer and check (ky_checkpoint.hpp; both ky_frame_book.cpp) and the stop rule's argument checks
 * (ky_host.hpp, ky_pack.cpp) are the product's own: kyhostcheck_frame and kyhostcheck_book drive the book through whole life cycles, kyhostcheck_checkpoint and
 * the kyhip_frame_* stand-ins at the end of this file call the rest, and nothing of it is restated here.
 */
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <thread>
#include <sys/wait.h>
#include <unistd.h>

#include "ky_frame_book.hpp"   // ky_checkpoint.hpp, ky_host.hpp, ky_blocks.hpp, ky_noise.hpp
#include "ky_denoise.hpp"

using namespace kyh;

extern "C" {

// pack_scene + scene_hash + scene_input on the caller's scene; returns pack_scene's status, the facts and both hashes
int kyhostcheck_pack(const ky_scene* scene, int* feat, uint64_t* packed_hash, uint64_t* input_hash, int* n_planar_occ, int* ts_light) {
    std::unique_ptr<DScene> d(new DScene);
    const int rc = pack_scene(scene, d.get());
    if (rc != KY_OK) return rc;
    if (feat) *feat = d->feat;
    if (packed_hash) *packed_hash = scene_hash(*d);
    std::vector<unsigned char> in;
    uint64_t h = 0;
    const bool keyed = scene_input(scene, in, h);
    if (input_hash) *input_hash = keyed ? h : 0;
    if (n_planar_occ) *n_planar_occ = d->occ.n_aar + d->occ.n_par;
    if (ts_light) *ts_light = d->ts_light;
    // every index the device follows must stay inside its table
    for (int i = 0; i < d->n_lights; ++i) {
        const DLight& L = d->light[i];
        for (int k = 0; k < L.n_carriers; ++k)
            if (L.carrier[k] < 0 || L.carrier[k] >= d->n_surfaces) return fail(KY_ERR_DEVICE, "carrier index out of range");
        const unsigned tab = (unsigned)L.shadow_table & ~1u;
        if (tab != __builtin_offsetof(DScene, occ_front) && tab != __builtin_offsetof(DScene, occ) && tab != __builtin_offsetof(DScene, trav)) return fail(KY_ERR_DEVICE, "shadow_table is not a table");
    }
    for (int j = 0; j < d->n_surfaces; ++j)
        if (d->orig[j] < 0 || d->orig[j] >= scene->surface_count || d->hit[j].material < 0 || d->hit[j].material >= d->n_materials) return fail(KY_ERR_DEVICE, "surface table out of range");
    return KY_OK;
}

// pack_material on the caller's material: DMat::exp_flags (integral / odd exponent, the two not-black bits, the Phong power's zero bound) and the two colours as
// packed (colours6: c0 then c1; plastic divides by the lobe probabilities there)
int kyhostcheck_material(const ky_material* m, int32_t* exp_flags, float* colours6) {
    if (!m || !exp_flags) return fail(KY_ERR_INVALID_VALUE, "bad arguments");
    DMat d;
    pack_material(*m, &d);
    *exp_flags = d.exp_flags;
    if (colours6) { cp3(colours6, d.c0); cp3(colours6 + 3, d.c1); }
    return KY_OK;
}

// the chunk schedule of `spp` samples covers [0, spp) exactly once, in order; returns the chunk count or -1
int kyhostcheck_chunks(int spp) {
    const ChunkPlan p = chunk_plan(spp);
    const int n = chunk_count(p);
    int next = 0;
    for (int c = 0; c < n; ++c) {
        int b, e;
        chunk_range(p, c, b, e);
        if (b != next || e <= b || e - b > KY_CHUNK) return -1;
        next = e;
    }
    return next == spp ? n : -1;
}

// A frame's host bookkeeping on the caller's parameters, without a device: the passes of at least min_samples that the book of a frame that owns everything takes
// (FrameBook::next_pass / commit_pass, what kyhip_frame_render asks and commits) cover every chunk once, in order, each ending at a value of pass_boundaries; a
// checkpoint written at every such point is accepted and gives the chunk count back, and one cut short, of another seed, or with a sample count no chunk ends at is
// refused.  Returns the number of passes, or a negative number.
int kyhostcheck_frame(const ky_render_params* p, int min_samples) {
    if (!valid_params(p) || min_samples < 1) return KY_ERR_INVALID_VALUE;
    const ChunkPlan plan = chunk_plan(p->samples_per_pixel);
    std::vector<int> bounds((size_t)chunk_count(plan));
    if (pass_boundaries(p->samples_per_pixel, bounds.data(), (int)bounds.size()) != (int)bounds.size()) return -10;
    FrameBook book;
    book.begin(p, 0x1234, 0, p->samples_per_pixel);
    const FrameHeader own = book.header;
    const size_t state_end = book.layout.total;
    std::vector<unsigned char> state(state_end, 0);
    ky_render_params q = *p;
    q.seed ^= 1u;
    int passes = 0;
    while (!book.owned_rendered()) {
        const int done = book.chunks_done, before = book.front();
        PassStep step;
        if (book.next_pass(min_samples, &step) != KY_OK || step.chunk_first != done || step.chunk_count <= 0 || done + step.chunk_count > (int)bounds.size()) return -11;
        book.commit_pass(step);
        if (book.chunks_done != done + step.chunk_count || book.front() != bounds[(size_t)book.chunks_done - 1] || book.held() != book.front()) return -11;
        if (!book.owned_rendered() && book.front() - before < min_samples) return -12;
        ++passes;
        int back = -1;
        FrameHeader h = own;
        h.samples_done = book.front();
        std::memcpy(state.data(), &h, sizeof h);
        if (frame_state_check(own, state.data(), state.size(), state_end, &back) != KY_OK || back != book.chunks_done) return -13;
        if (frame_state_check(own, state.data(), state.size() - 1, state_end, &back) == KY_OK || frame_state_check(own, state.data(), sizeof h - 1, state_end, &back) == KY_OK) return -14;
        if (frame_state_check(frame_header(&q, 0x1234, 0), state.data(), state.size(), state_end, &back) == KY_OK) return -15;
        if (frame_state_check(frame_header(p, 0x1235, 0), state.data(), state.size(), state_end, &back) == KY_OK) return -16;
    }
    if (chunks_at_sample(plan, 0) != 0 || chunks_at_sample(plan, p->samples_per_pixel + 1) != -1) return -17;
    for (int s = 1, c = 0; s <= p->samples_per_pixel; ++s) {   // every sample count: a chunk count exactly at the boundaries
        const bool is_bound = bounds[(size_t)c] == s;
        if (chunks_at_sample(plan, s) != (is_bound ? c + 1 : -1)) return -18;
        if (is_bound) ++c;
    }
    return passes;
}

// blocks_init_kernel's rule (ky_blocks.hip) for a block with `inside` pixels inside the film, and what blocks_refresh (ky_frame.cpp) counts when the states come home
static kyb::BlockState block_init_state(int inside) { return inside > 0 ? kyb::BlockState{-1, 0} : kyb::BlockState{0, 0}; }
static int blocks_come_home(FrameBook* book) {
    int n_live = 0;
    for (const kyb::BlockState& s : book->blocks.host) n_live += s.retired_at < 0;
    return book->blocks_home(n_live);
}
// one operation of kyhostcheck_book on `book`: what the kyhip_frame_* entry of that name does (ky_frame.cpp) without its device work -- ask the book, commit
static int book_op(FrameBook* books, int n_books, std::vector<unsigned char>* slots, int op, int at, int arg, int arg2) {
    FrameBook& book = books[at];
    auto slot_of = [&](std::vector<unsigned char>** out) {
        if (arg < 0 || arg >= 4) return fail(KY_ERR_INVALID_VALUE, "slot %d", arg);
        *out = &slots[arg];
        return (int)KY_OK;
    };
    std::vector<unsigned char>* slot = nullptr;
    switch (op) {
    case 0: {   // kyhip_frame_render
        PassStep step;
        KY_TRY(book.next_pass(arg, &step));
        book.commit_pass(step);
        return KY_OK;
    }
    case 1: {   // kyhip_frame_save: the host parts into a zeroed buffer
        KY_TRY(slot_of(&slot));
        std::vector<unsigned char> buf(book.layout.total, 0);
        KY_TRY(book.save_host(buf.data(), buf.size()));
        slot->swap(buf);
        return KY_OK;
    }
    case 2: {   // kyhip_frame_load of the slot's bytes but the last arg2
        KY_TRY(slot_of(&slot));
        const size_t bytes = slot->size() - ((size_t)arg2 < slot->size() ? (size_t)arg2 : slot->size());
        CheckpointCounts n;
        KY_TRY(book.load_check(slot->data(), bytes, &n));
        if (book.blocks.on && book.sh.n_blocks > 0) {
            std::memcpy(book.blocks.host.data(), slot->data() + book.layout.block_states, book.layout.block_states_bytes());
            KY_TRY(blocks_come_home(&book));
        }
        book.commit_load(n);
        return KY_OK;
    }
    case 3: {   // kyhip_frame_merge of the slot's bytes but the last arg2
        KY_TRY(slot_of(&slot));
        const size_t bytes = slot->size() - ((size_t)arg2 < slot->size() ? (size_t)arg2 : slot->size());
        MergeStep step;
        KY_TRY(book.merge_state(slot->data(), bytes, &step));
        book.commit_merge(step);
        return KY_OK;
    }
    case 4: {   // kyhip_frame_merge_from book arg
        if (arg < 0 || arg >= n_books) return fail(KY_ERR_INVALID_VALUE, "book %d", arg);
        MergeStep step;
        KY_TRY(book.merge_book(books[arg], &step));
        book.commit_merge(step);
        return KY_OK;
    }
    case 5:   // kyhip_frame_track_noise
        if (book.noise.on) return KY_OK;
        KY_TRY(book.can_track_noise());
        book.track_noise();
        return KY_OK;
    case 6:   // kyhip_frame_track_blocks
        if (book.blocks.on) return KY_OK;
        KY_TRY(book.can_track_blocks());
        book.size_blocks();
        for (size_t b = 0; b < book.blocks.host.size(); ++b) book.blocks.host[b] = block_init_state(book.blocks.inside[b]);
        KY_TRY(blocks_come_home(&book));
        book.track_blocks();
        return KY_OK;
    case 7: return KY_OK;   // nothing: the book as it stands is recorded
    default: return fail(KY_ERR_INVALID_VALUE, "operation %d", op);
    }
}

// Whole life cycles of up to five frames of one ky_render_params and one scene hash (source_hash, when not 0: the kernel source hash their headers carry instead of
// this build's, which another compiler made -- a caller that holds the books' states against libkyhip.so's passes that library's), without a device: books[i] = {own_first, own_end} opens book i (begin_check,
// FrameBook::begin), then ops[k] = {operation, book, arg, arg2} run in order on the books and on four state slots:
//   0 a pass of at least arg samples      1 save into slot arg            2 load from slot arg (without its last arg2 bytes)      3 merge slot arg's state (likewise)
//   4 merge from book arg                 5 track noise                   6 track blocks                                          7 nothing
// (kyhip_frame_keep has no operation: the rule of ky_blocks.hip's keep kernel is no function of ky_blocks.hpp, and it is not restated here.)
// Behind every operation records[k] (KY_BOOK_RECORD ints) = {status, front, held, coverage ranges, own_first, own_end, batches, n_prev, passes, n_live,
// state_bytes, then the coverage's pairs, zeros behind them} of the book it addressed.  At the end slot i's bytes lie at slots_out + i * slot_capacity when they
// fit, and slot_bytes[i] is their number.  Returns KY_OK when the script ran (a refused operation shows in its record and leaves the message), or the status of
// arguments or of a book that is none.
constexpr int KY_BOOK_RECORD = 11 + 2 * KY_SLICE_MAX_RANGES, KY_BOOK_MAX = 5;   // (five: three slices, a collector and a fresh collector that loads its state)
int kyhostcheck_book(const ky_render_params* p, uint64_t scene_hash, uint64_t source_hash, const int* books, int n_books, const int* ops, int n_ops, int* records, unsigned char* slots_out,
                     size_t slot_capacity, size_t* slot_bytes) {
    if (n_books < 1 || n_books > KY_BOOK_MAX || n_ops < 0 || !books || (n_ops > 0 && (!ops || !records))) return fail(KY_ERR_INVALID_VALUE, "bad arguments");
    FrameBook book[KY_BOOK_MAX];
    std::vector<unsigned char> slots[4];
    for (int i = 0; i < n_books; ++i) {
        kyhip_frame* none;
        KY_TRY(begin_check(nullptr, p, books[2 * i], books[2 * i + 1], &none));
        book[i].begin(p, scene_hash, books[2 * i], books[2 * i + 1]);
        if (source_hash) book[i].header.source_hash = source_hash;
    }
    for (int k = 0; k < n_ops; ++k) {
        const int* op = ops + 4 * (size_t)k;
        if (op[1] < 0 || op[1] >= n_books) return fail(KY_ERR_INVALID_VALUE, "operation %d: book %d", k, op[1]);
        const FrameBook& b = book[op[1]];
        int* r = records + (size_t)KY_BOOK_RECORD * (size_t)k;
        std::memset(r, 0, sizeof(int) * KY_BOOK_RECORD);
        r[0] = book_op(book, n_books, slots, op[0], op[1], op[2], op[3]);
        const int after[10] = {b.front(), b.held(), b.cov.n, b.own_first, b.own_end, b.noise.batches, b.noise.n_prev, b.blocks.passes, b.blocks.n_live, (int)b.layout.total};
        std::memcpy(r + 1, after, sizeof after);
        b.coverage(r + 11, KY_SLICE_MAX_RANGES, nullptr);
    }
    for (int i = 0; i < 4; ++i) {
        if (slot_bytes) slot_bytes[i] = slots[i].size();
        if (slots_out && !slots[i].empty() && slots[i].size() <= slot_capacity) std::memcpy(slots_out + (size_t)i * slot_capacity, slots[i].data(), slots[i].size());
    }
    return KY_OK;
}

// A whole checkpoint without a device (ky_checkpoint.hpp): the layout of a frame of p that tracks (noise, blocks) -> offsets[6] = where the accumulators, the noise
// trailer, the noise pixels, the block trailer and the block states begin, and the total; the host-side parts written into a zeroed buffer of that total from
// counts_in = {samples_done, batches, n_prev, passes} and `states` (n_blocks x {retired_at, batches}; NULL: every block live) -- copied to state_out when its
// capacity holds it --, then checkpoint_check on the first check_bytes bytes of it (at most the total) by a frame that tracks (noise, check_blocks) ->
// counts_out = {chunks_done, samples_done, batches, n_prev, passes}.  Returns the check's status, or KY_ERR_INVALID_VALUE for arguments that are none.
int kyhostcheck_checkpoint(const ky_render_params* p, int noise, int blocks, int check_blocks, const int* counts_in, const int32_t* states, size_t check_bytes,
                           size_t* offsets, int* counts_out, void* state_out, size_t state_capacity) {
    if (!valid_params(p) || !shard_in_range(p) || !counts_in || !offsets || !counts_out) return fail(KY_ERR_INVALID_VALUE, "bad arguments");
    const CheckpointLayout L = checkpoint_layout(p, noise != 0, blocks != 0);
    const size_t at[6] = {L.accum, L.noise, L.noise_pixels, L.blocks, L.block_states, L.total};
    std::memcpy(offsets, at, sizeof at);
    std::vector<kyb::BlockState> st((size_t)L.n_blocks, kyb::BlockState{-1, 0});
    for (int b = 0; b < L.n_blocks && states; ++b) st[(size_t)b] = kyb::BlockState{states[2 * b], states[2 * b + 1]};
    CheckpointCounts n;
    n.samples_done = counts_in[0]; n.batches = counts_in[1]; n.n_prev = counts_in[2]; n.passes = counts_in[3];
    const FrameHeader own = frame_header(p, 0x1234, 0);
    std::vector<unsigned char> buf(L.total, 0);
    checkpoint_write_host(own, L, n, st.data(), buf.data());
    if (state_out && state_capacity >= L.total) std::memcpy(state_out, buf.data(), L.total);
    CheckpointCounts back;
    KY_TRY(checkpoint_check(own, checkpoint_layout(p, noise != 0, check_blocks != 0), buf.data(), check_bytes < L.total ? check_bytes : L.total, &back));
    const int got[5] = {back.chunks_done, back.samples_done, back.batches, back.n_prev, back.passes};
    std::memcpy(counts_out, got, sizeof got);
    return KY_OK;
}

// make_shard / shard_in_range / valid_params on the caller's parameters: n_items, or a negative status
long long kyhostcheck_shard(const ky_render_params* p) {
    if (!valid_params(p)) return KY_ERR_INVALID_VALUE;
    if (!shard_in_range(p)) return KY_ERR_LIMIT;
    const ShardConst s = make_shard(p);
    return (long long)s.n_items;
}

// film += src over rows [y0, y1) by n_threads workers of the pool (what the seam's step 4 does); returns 0 when the sum is right
int kyhostcheck_add_rows(int width, int height, int stride_px, int n_threads, int rounds) {
    std::vector<float> film((size_t)height * stride_px * 3, 1.f), src((size_t)height * width * 3);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (float)(i % 7);
    for (int r = 0; r < rounds; ++r)
        host_pool().run(n_threads, [&](int t) {
            const int r0 = (int)((long long)height * t / n_threads), r1 = (int)((long long)height * (t + 1) / n_threads);
            host_add_rows(film.data(), (size_t)stride_px, src.data(), width, r0, r1);
        });
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < stride_px * 3; ++x) {
            const float want = x < width * 3 ? 1.f + rounds * (float)(((size_t)y * width * 3 + x) % 7) : 1.f;
            if (film[(size_t)y * stride_px * 3 + x] != want) return 1 + y;
        }
    return 0;
}

// Two caller threads x two "devices": each call takes the seam mutexes of its device list in ascending device order (lock_seams, what
// kyhip_render_multi does), runs a pool job inside, releases; the lists overlap in opposite orders.  In between the process forks once and the
// child runs a pool job of its own (a forked child inherits the pool object, not its threads).  Returns 0, or what went wrong.
int kyhostcheck_seam_stress(int iterations) {
    std::mutex seam[2];
    std::atomic<long long> total{0};
    std::atomic<int> bad{0};
    auto call = [&](std::vector<int> devices) {
        std::vector<std::pair<int, std::mutex*>> want;
        for (int d : devices) want.emplace_back(d, &seam[d]);
        auto locks = lock_seams(want);
        long long local[4] = {0, 0, 0, 0};
        host_pool().run(3, [&](int t) { local[t] += t + 1; });
        if (local[0] != 1 || local[1] != 2 || local[2] != 3) bad.fetch_add(1);
        total.fetch_add(local[0] + local[1] + local[2]);
    };
    auto worker = [&](bool flip) {
        for (int i = 0; i < iterations; ++i) call(flip ? std::vector<int>{1, 0} : std::vector<int>{0, 1, 0});
    };
    {
        std::thread a(worker, false), b(worker, true);
        a.join(); b.join();
    }
    const pid_t pid = fork();
    if (pid == 0) {   // the child: its pool must come up again by itself
        long long local[3] = {0, 0, 0};
        host_pool().run(3, [&](int t) { local[t] = t + 1; });
        _exit(local[0] == 1 && local[1] == 2 && local[2] == 3 ? 0 : 7);
    }
    int status = 0;
    if (pid < 0 || waitpid(pid, &status, 0) != pid || !WIFEXITED(status) || WEXITSTATUS(status) != 0) return 100;
    {
        std::thread a(worker, true), b(worker, false);
        a.join(); b.join();
    }
    if (bad.load()) return 200;
    return total.load() == 4LL * iterations * 6 ? 0 : 300;
}

// Several threads ask the code cache for the same and for different instantiations at once, blocking and not (KYHIP_HIPCC points the cache at a
// stand-in compiler: tests/test_sanitize.py); returns the number of requests that ended with an object
int kyhostcheck_jit_stress(int n_threads, int rounds) {
    std::atomic<int> got{0};
    std::vector<std::thread> th;
    for (int t = 0; t < n_threads; ++t)
        th.emplace_back([&, t] {
            for (int r = 0; r < rounds; ++r) {
                char args[96];
                snprintf(args, sizeof args, "false, 48, false, false, %d, 11, false", (t + r) % 3);
                bool pending = false;
                const kyjit::Code* c = kyjit::get_code(args, (t & 1) == 0, &pending);
                for (int spin = 0; !c && pending && spin < 2000; ++spin) { usleep(1000); c = kyjit::get_code(args, false, &pending); }
                if (c && !c->object.empty()) got.fetch_add(1);
            }
        });
    for (auto& x : th) x.join();
    return got.load();
}

// The noise estimate's arithmetic (ky_noise.hpp: what noise_update_kernel and noise_map_kernel do per pixel) on the caller's accumulators -- accum:
// n_pass x n_pix x 3 words as they stand after each pass, done: the samples done after each pass, flags: n_pix flag words (NULL: none set) -- writing after
// every pass the pixels' {y_prev, m2} (out_state: n_pass x n_pix x 2) and their map values (out_map: n_pass x n_pix); then, when `state` is given, the
// trailer check of a checkpoint of state_bytes bytes whose accumulators end at base_bytes, for a frame of trailer_n_pix pixels at samples_done.
// Returns the trailer check's status (KY_OK without one), or KY_ERR_INVALID_VALUE for arguments that are none.
int kyhostcheck_noise(const long long* accum, const int* done, int n_pass, int n_pix, int total_spp, const unsigned* flags, double* out_state, float* out_map,
                      const void* state, size_t state_bytes, size_t base_bytes, int trailer_n_pix, int samples_done) {
    using namespace kyn;
    if (n_pass < 0 || n_pix < 0 || (n_pass > 0 && n_pix > 0 && (!accum || !done || !out_state || !out_map))) return fail(KY_ERR_INVALID_VALUE, "bad arguments");
    std::vector<NoisePixel> px((size_t)n_pix, NoisePixel{0.0, 0.0});
    int n_prev = 0;
    for (int k = 0; k < n_pass; ++k) {
        if (done[k] <= n_prev) return fail(KY_ERR_INVALID_VALUE, "pass %d ends at %d samples, the one before at %d", k, done[k], n_prev);
        for (int i = 0; i < n_pix; ++i) {
            const long long* a = accum + ((size_t)k * n_pix + (size_t)i) * 3;
            noise_update(px[(size_t)i], noise_luminance(a[0], a[1], a[2], total_spp), n_prev, done[k]);
            out_state[((size_t)k * n_pix + (size_t)i) * 2] = px[(size_t)i].y_prev;
            out_state[((size_t)k * n_pix + (size_t)i) * 2 + 1] = px[(size_t)i].m2;
            out_map[(size_t)k * n_pix + (size_t)i] = noise_value(px[(size_t)i], k + 1, done[k], flags ? flags[i] : 0u);
        }
        n_prev = done[k];
    }
    if (!state) return KY_OK;
    NoiseTrailer t;
    return noise_trailer_check(state, state_bytes, base_bytes, trailer_n_pix, samples_done, &t);
}

// A merge's arithmetic (ky_noise.hpp: merge_pixel, what ky_merge.hip's kernel does per pixel) on the caller's arrays: words_a (n_pix x 3), flags_a (n_pix) and,
// when given, pairs_a (n_pix x {y_prev, m2}; pairs_b then too) receive the frame b, which holds n_b samples, a holding n_a.  Returns KY_OK, or
// KY_ERR_INVALID_VALUE for arguments that are none.
int kyhostcheck_merge(long long* words_a, const long long* words_b, unsigned* flags_a, const unsigned* flags_b, double* pairs_a, const double* pairs_b, int n_pix,
                      int total_spp, int n_a, int n_b) {
    using namespace kyn;
    if (n_pix < 0 || n_a < 0 || n_b < 0 || (n_pix > 0 && (!words_a || !words_b || !flags_a || !flags_b || (pairs_a && !pairs_b)))) return fail(KY_ERR_INVALID_VALUE, "bad arguments");
    for (int i = 0; i < n_pix; ++i) {
        NoisePixel a = {0.0, 0.0}, b = {0.0, 0.0};
        if (pairs_a) { a = NoisePixel{pairs_a[2 * (size_t)i], pairs_a[2 * (size_t)i + 1]}; b = NoisePixel{pairs_b[2 * (size_t)i], pairs_b[2 * (size_t)i + 1]}; }
        merge_pixel(words_a + 3 * (size_t)i, words_b + 3 * (size_t)i, flags_a[i], flags_b[i], pairs_a ? &a : nullptr, &b, total_spp, n_a, n_b);
        if (pairs_a) { pairs_a[2 * (size_t)i] = a.y_prev; pairs_a[2 * (size_t)i + 1] = a.m2; }
    }
    return KY_OK;
}

// Slices without a device (ky_checkpoint.hpp), by `mode`; ranges are {first, end} pairs of int, a coverage is built from its pairs one coverage_union at a time:
//   0  kyhip_slice_bounds(spp = na, n_slices = nb) -> out (nb + 1 values);
//   1  the coverage of a's na pairs U the coverage of b's nb pairs -> out (pairs), counts[0] = their number.  Returns the first status that is not KY_OK;
//   2  the host-side parts of the checkpoint of a frame of p that owns a[0] .. a[1], stands at a[2] and holds b's nb pairs (noise = extra[0]: it tracks noise, with
//      extra[1] batches) into buf, zeroed first, when its `bytes` hold them; counts = {the state's size, where its slice trailer begins, where its noise trailer does};
//   3  checkpoint_check of buf's first `bytes` bytes by a frame of p that owns a[0] .. a[1] (noise = extra[0]) -> counts = {chunks_done, samples held, batches,
//      n_prev, front, ranges}, out = the ranges;
//   4  merge_source_check of buf by a frame of p, then merge_accept by one that owns a[0] .. a[1], holds b's nb pairs and tracks noise (extra[0]) or blocks
//      (extra[1]) -> out = the union, counts = {its ranges, the samples the state holds, its batches}.
// Returns the status of what it ran, or KY_ERR_INVALID_VALUE for arguments that are none.
int kyhostcheck_slices(int mode, const ky_render_params* p, const int* a, int na, const int* b, int nb, int* out, int* counts, void* buf, size_t bytes, const int* extra) {
    if (mode == 0) return kyhip_slice_bounds(na, nb, out);
    auto build = [](const int* pairs, int n, Coverage* cov) {
        for (int i = 0; i < n; ++i) {
            Coverage one;
            one.n = 1; one.r[0] = pairs[2 * i]; one.r[1] = pairs[2 * i + 1];
            KY_TRY(coverage_union(*cov, one, cov));
        }
        return (int)KY_OK;
    };
    auto give = [&](const Coverage& cov) { for (int i = 0; i < 2 * cov.n; ++i) out[i] = cov.r[i]; };
    if (na < 0 || nb < 0 || (na > 0 && !a) || (nb > 0 && !b) || !out || !counts) return fail(KY_ERR_INVALID_VALUE, "bad arguments");
    if (mode == 1) {
        Coverage ca, cb, u;
        KY_TRY(build(a, na, &ca));
        KY_TRY(build(b, nb, &cb));
        KY_TRY(coverage_union(ca, cb, &u));
        give(u);
        counts[0] = u.n;
        return KY_OK;
    }
    if (!valid_params(p) || !shard_in_range(p) || !extra || !a || !buf) return fail(KY_ERR_INVALID_VALUE, "bad arguments");
    const FrameHeader own = frame_header(p, 0x1234, 0);
    if (mode == 2) {
        KY_TRY(slice_range_check(p->samples_per_pixel, a[0], a[1]));
        const CheckpointLayout L = checkpoint_layout(p, extra[0] != 0, false, a[0], a[1]);
        counts[0] = (int)L.total; counts[1] = (int)L.slice; counts[2] = (int)L.noise;
        if (bytes < L.total) return KY_OK;
        CheckpointCounts n;
        KY_TRY(build(b, nb, &n.cov));
        n.samples_done = n.n_prev = n.cov.held();
        n.front = a[2];
        n.batches = extra[1];
        std::memset(buf, 0, L.total);
        checkpoint_write_host(own, L, n, nullptr, buf);
        return KY_OK;
    }
    if (mode == 3) {
        KY_TRY(slice_range_check(p->samples_per_pixel, a[0], a[1]));
        CheckpointCounts n;
        KY_TRY(checkpoint_check(own, checkpoint_layout(p, extra[0] != 0, false, a[0], a[1]), buf, bytes, &n));
        const int got[6] = {n.chunks_done, n.samples_done, n.batches, n.n_prev, n.front, n.cov.n};
        std::memcpy(counts, got, sizeof got);
        give(n.cov);
        return KY_OK;
    }
    if (mode == 4) {
        MergeSource m;
        KY_TRY(merge_source_check(own, buf, bytes, &m));
        Coverage mine, u;
        KY_TRY(build(b, nb, &mine));
        KY_TRY(merge_accept(mine, a[0], a[1], p->samples_per_pixel, extra[0] != 0, extra[1] != 0, m.cov, m.noise_pixels != 0, &u));
        give(u);
        counts[0] = u.n; counts[1] = m.cov.held(); counts[2] = m.batches;
        return KY_OK;
    }
    return fail(KY_ERR_INVALID_VALUE, "mode %d", mode);
}

// The block arithmetic of a frame that retires pixel blocks (ky_blocks.hpp: what ky_blocks.hip's kernels do per block) for the shard of p.  Each part runs when its
// pointers are given:
//   out_block (n_pix), out_pixel (n_blocks x 64), out_inside (n_blocks): the pixel -> block map, its inverse, and each block's pixels inside the film;
//   state (n_blocks x {retired_at, batches}, in and out) with map and cls (n_pix, compact tile order; cls NULL: derived from the film's edges, nothing flagged):
//     blocks_init_kernel's rule when init != 0, then one application of the retire rule at `front` / `batches`;
//   trailer: block_trailer_check of a checkpoint of trailer_bytes bytes whose block trailer begins at trailer_offset, for a frame at samples_done whose noise estimate has noise_batches batches (0: it tracks none).
// Returns the trailer check's status (KY_OK without one), or KY_ERR_INVALID_VALUE for arguments that are none.
int kyhostcheck_blocks(const ky_render_params* p, int* out_block, int* out_pixel, int* out_inside, int32_t* state, int init, const float* map, const unsigned char* cls,
                       float threshold, float max_fraction_above, int min_batches, int front, int batches, const void* trailer, size_t trailer_bytes,
                       size_t trailer_offset, int samples_done, int noise_batches) {
    using namespace kyb;
    if (!valid_params(p) || !shard_in_range(p)) return fail(KY_ERR_INVALID_VALUE, "invalid render params");
    const ShardConst sh = make_shard(p);
    for (int i = 0; i < sh.n_pix && out_block; ++i) out_block[i] = block_of_pixel(sh, i);
    for (int b = 0; b < sh.n_blocks; ++b) {
        int inside = 0;
        for (int lane = 0; lane < KY_BLOCK_PIXELS; ++lane) {
            const int i = pixel_of_block(sh, b, lane);
            if (out_pixel) out_pixel[(size_t)b * KY_BLOCK_PIXELS + lane] = i;
            inside += pixel_inside(sh, i, p->width, p->height);
        }
        if (out_inside) out_inside[b] = inside;
        if (!state) continue;
        BlockState s = {state[2 * b], state[2 * b + 1]};
        if (init) s = block_init_state(inside);
        if (map && s.retired_at < 0) {
            int counted = 0, above = 0;
            for (int lane = 0; lane < KY_BLOCK_PIXELS; ++lane) {
                const int i = pixel_of_block(sh, b, lane);
                const int c = cls ? cls[i] : (pixel_inside(sh, i, p->width, p->height) ? kyn::KY_NOISE_INSIDE : kyn::KY_NOISE_PADDING);
                counted += c == kyn::KY_NOISE_INSIDE;
                above += c == kyn::KY_NOISE_INSIDE && map[i] > threshold;
            }
            if (block_retires(batches, min_batches, above, counted, max_fraction_above)) s = BlockState{front, batches};
        }
        state[2 * b] = s.retired_at; state[2 * b + 1] = s.batches;
    }
    if (!trailer) return KY_OK;
    return block_trailer_check(trailer, trailer_bytes, trailer_offset, sh.n_blocks, p->samples_per_pixel, samples_done, noise_batches);
}

// The denoise filter's arithmetic (ky_denoise.hpp: what denoise_level_kernel does per pixel) on the caller's film-order buffers -- cv {r, g, b, v}, ga {n, t},
// gb {P, class}: width x height x 4 floats each -- for p->levels levels with steps 1, 2, 4 ...; `pix` is the width of a pixel at unit distance.  Writes the last
// level's {r, g, b, v}, unclamped, to out (width x height x 4).  Returns denoise_params_check's status, or KY_ERR_INVALID_VALUE for arguments that are none.
// `key`: NULL (level_pixel, the filter of a frame without guide bounces), or width x height chain keys (level_pixel_t<true>: taps share the pixel's key).
static int denoise_on_host(const float* cv, const float* ga, const float* gb, const uint64_t* key, int width, int height, const ky_denoise_params* p, double pix, float* out) {
    using namespace kydn;
    if (!cv || !ga || !gb || !p || !out || width < 1 || height < 1) return fail(KY_ERR_INVALID_VALUE, "bad arguments");
    KY_TRY(denoise_params_check(p));
    const size_t n = (size_t)width * (size_t)height;
    std::vector<uint64_t> keys(key ? n : 0);
    if (key) std::memcpy(keys.data(), key, n * sizeof(uint64_t));
    std::vector<Px4> c[2] = {std::vector<Px4>(n), std::vector<Px4>(n)}, a(n), b(n);   // (16-byte aligned copies: the caller's arrays need not be)
    std::memcpy(c[0].data(), cv, n * sizeof(Px4));
    std::memcpy(a.data(), ga, n * sizeof(Px4));
    std::memcpy(b.data(), gb, n * sizeof(Px4));
    LevelConst k{};
    k.width = width; k.height = height;
    k.normal_squarings = p->normal_squarings;
    k.sigma_l2 = (double)p->sigma_luminance * (double)p->sigma_luminance;
    k.sigma_plane = (double)p->sigma_plane;
    k.pix = pix;
    for (int l = 0; l < p->levels; ++l)
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x)
                c[(l + 1) & 1][(size_t)y * width + x] = key ? level_pixel_t<true>(c[l & 1].data(), a.data(), b.data(), keys.data(), x, y, 1 << l, k)
                                                            : level_pixel(c[l & 1].data(), a.data(), b.data(), x, y, 1 << l, k);
    std::memcpy(out, c[p->levels & 1].data(), n * sizeof(Px4));
    return KY_OK;
}
int kyhostcheck_denoise(const float* cv, const float* ga, const float* gb, int width, int height, const ky_denoise_params* p, double pix, float* out) {
    return denoise_on_host(cv, ga, gb, nullptr, width, height, p, pix, out);
}
// ... with one chain key per pixel (width x height uint64_t, film order): the filter of a frame with guide bounces
int kyhostcheck_denoise_keyed(const float* cv, const float* ga, const float* gb, const uint64_t* key, int width, int height, const ky_denoise_params* p, double pix,
                              float* out) {
    if (!key) return fail(KY_ERR_INVALID_VALUE, "bad arguments");
    return denoise_on_host(cv, ga, gb, key, width, height, p, pix, out);
}

// ... of a frame with an albedo grid (DESIGN.md "Denoise", "Albedo"): `albedo` is width x height x 4 floats {r, g, b, w}; the class-0 pixels are demodulated
// (demodulate_pixel), the levels run -- keyed where `key` is not NULL --, and the class-0 pixels are remodulated (remodulate_pixel).  Writes {r, g, b, v} like the others.
int kyhostcheck_denoise_albedo(const float* cv, const float* ga, const float* gb, const uint64_t* key, const float* albedo, int width, int height, const ky_denoise_params* p,
                               double pix, float* out) {
    using namespace kydn;
    if (!cv || !gb || !albedo || !out || width < 1 || height < 1) return fail(KY_ERR_INVALID_VALUE, "bad arguments");
    const size_t n = (size_t)width * (size_t)height;
    std::vector<Px4> c(n), b(n), a(n);
    std::memcpy(c.data(), cv, n * sizeof(Px4));
    std::memcpy(b.data(), gb, n * sizeof(Px4));
    std::memcpy(a.data(), albedo, n * sizeof(Px4));
    for (size_t i = 0; i < n; ++i)
        if (is_surface(b[i])) c[i] = demodulate_pixel(c[i], a[i]);
    KY_TRY(denoise_on_host(&c[0].x, ga, gb, key, width, height, p, pix, &c[0].x));
    for (size_t i = 0; i < n; ++i)
        if (is_surface(b[i])) c[i] = remodulate_pixel(c[i], a[i]);
    std::memcpy(out, c.data(), n * sizeof(Px4));
    return KY_OK;
}

// The temporal step's arithmetic (ky_denoise.hpp, temporal_pixel_t: what denoise_temporal_kernel does per pixel) over whole film-order buffers: the frame's cv, ga,
// gb (width x height x 4 floats each; key: NULL, or width x height chain keys), the history's old side hcv, hga, hgb = {P, m} (all three NULL: a history that holds
// no picture), n_p the samples the frame holds, `pix` the current camera's pixel width, `then` the history's camera.  Writes the history's new {r, g, b, v} to
// out_cv and its new {P, m} to out_gb.  Returns temporal_params_check's status, or KY_ERR_INVALID_VALUE for arguments that are none.
int kyhostcheck_temporal(const float* cv, const float* ga, const float* gb, const uint64_t* key, const float* hcv, const float* hga, const float* hgb, int width, int height,
                         double n_p, const ky_temporal_params* t, double pix, const ky_camera* then, float* out_cv, float* out_gb) {
    using namespace kydn;
    const bool has = hcv && hga && hgb;
    if (!cv || !ga || !gb || !t || !then || !out_cv || !out_gb || width < 1 || height < 1 || (!has && (hcv || hga || hgb))) return fail(KY_ERR_INVALID_VALUE, "bad arguments");
    KY_TRY(temporal_params_check(t));
    const size_t n = (size_t)width * (size_t)height;
    std::vector<uint64_t> keys(key ? n : 0);
    if (key) std::memcpy(keys.data(), key, n * sizeof(uint64_t));
    std::vector<Px4> c(n), a(n), b(n), hc(has ? n : 0), ha(has ? n : 0), hb(has ? n : 0), oc(n), ob(n);   // (16-byte aligned copies: the caller's arrays need not be)
    std::memcpy(c.data(), cv, n * sizeof(Px4));
    std::memcpy(a.data(), ga, n * sizeof(Px4));
    std::memcpy(b.data(), gb, n * sizeof(Px4));
    if (has) {
        std::memcpy(hc.data(), hcv, n * sizeof(Px4));
        std::memcpy(ha.data(), hga, n * sizeof(Px4));
        std::memcpy(hb.data(), hgb, n * sizeof(Px4));
    }
    TemporalConst k{};
    k.width = width; k.height = height;
    k.normal_squarings = t->normal_squarings;
    k.has_history = has ? 1 : 0;
    k.n_p = n_p;
    k.max_history = (double)t->max_history; k.sigma_plane = (double)t->sigma_plane; k.min_weight = (double)t->min_weight;
    k.pix = pix;
    k.then = *then;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const TemporalPixel o = key ? temporal_pixel_t<true>(c.data(), a.data(), b.data(), keys.data(), hc.data(), ha.data(), hb.data(), x, y, k)
                                        : temporal_pixel_t<false>(c.data(), a.data(), b.data(), nullptr, hc.data(), ha.data(), hb.data(), x, y, k);
            oc[(size_t)y * width + x] = o.cv;
            ob[(size_t)y * width + x] = o.gb;
        }
    std::memcpy(out_cv, oc.data(), n * sizeof(Px4));
    std::memcpy(out_gb, ob.data(), n * sizeof(Px4));
    return KY_OK;
}

// What kyhip_frame_denoise_temporal refuses of a frame and a history (FrameBook::temporal_check), without a device: the book of a frame of p that tracks noise
// (noise != 0) with `batches` noise batches and blocks (blocks != 0), on `device` with `albedo_grid`, against a history of hist_width x hist_height on hist_device
// whose albedo mode is hist_albedo (-1: it holds no picture).  Returns the check's status.
int kyhostcheck_temporal_refusal(const ky_render_params* p, int noise, int blocks, int batches, int device, int albedo_grid, int hist_device, int hist_width,
                                 int hist_height, int hist_albedo) {
    kyhip_frame* none;
    KY_TRY(begin_check(nullptr, p, 0, p ? p->samples_per_pixel : 0, &none));
    FrameBook book;
    book.begin(p, 0x1234, 0, p->samples_per_pixel);
    if (noise) KY_TRY(book_op(&book, 1, nullptr, 5, 0, 0, 0));
    if (blocks) KY_TRY(book_op(&book, 1, nullptr, 6, 0, 0, 0));
    book.noise.batches = batches;
    return book.temporal_check(device, albedo_grid, hist_device, hist_width, hist_height, hist_albedo);
}

// The live rectangle (screen_bound, kyhip_scene_screen_bound) on degenerate inputs: a unit box of five matte rectangles (open towards -z) or one sphere, seen by a
// camera that looks along +z.  Whatever the proof cannot cover must give the whole frame: the camera on the bound's face, inside the bound, a NaN vertex, no surfaces.
// A sphere of radius zero is a bound that is a point: a rectangle of a few pixels.  Returns 0, or the number of the case that went wrong.
int kyhostcheck_screen_bound(void) {
    const float q = std::numeric_limits<float>::quiet_NaN();
    auto rect_shape = [](const float (&p)[4][3], float nx, float ny, float nz) {
        ky_shape s{};
        s.kind = KY_SHAPE_RECTANGLE;
        std::memcpy(s.p, p, sizeof s.p);
        s.normal[0] = nx; s.normal[1] = ny; s.normal[2] = nz;
        return s;
    };
    const float back[4][3] = {{-1, -1, 1}, {1, -1, 1}, {1, 1, 1}, {-1, 1, 1}}, floor_[4][3] = {{-1, -1, -1}, {1, -1, -1}, {1, -1, 1}, {-1, -1, 1}},
                ceil_[4][3] = {{-1, 1, -1}, {1, 1, -1}, {1, 1, 1}, {-1, 1, 1}}, left[4][3] = {{-1, -1, -1}, {-1, -1, 1}, {-1, 1, 1}, {-1, 1, -1}},
                right[4][3] = {{1, -1, -1}, {1, -1, 1}, {1, 1, 1}, {1, 1, -1}};
    std::vector<ky_shape> box = {rect_shape(back, 0, 0, -1), rect_shape(floor_, 0, 1, 0), rect_shape(ceil_, 0, -1, 0), rect_shape(left, 1, 0, 0), rect_shape(right, -1, 0, 0)};
    ky_material matte{};
    matte.kind = KY_MATERIAL_MATTE; matte.color0[0] = matte.color0[1] = matte.color0[2] = 0.5f;
    ky_light lamp{};
    lamp.kind = KY_LIGHT_POINT; lamp.color[0] = lamp.color[1] = lamp.color[2] = 1.f;
    std::vector<ky_surface> surf;
    for (int i = 0; i < 5; ++i) surf.push_back(ky_surface{i, 0, -1});
    ky_render_params p{};
    p.integrator = KY_INTEGRATOR_PATH_TRACING_ITERATION; p.max_path_depth = 5; p.direct_sample = KY_DIRECT_BOTH_MIS; p.samples_per_pixel = 4; p.sampler = KY_SAMPLER_RANDOM;
    p.width = 256; p.height = 64; p.tile_w = 32; p.tile_h = 32; p.tile_first = 0; p.tile_step = 1;
    auto scene_at = [&](const std::vector<ky_shape>& shapes, int n_surfaces, float cz) {
        ky_scene s{};
        s.shapes = shapes.data(); s.shape_count = (int)shapes.size();
        s.materials = &matte; s.material_count = 1;
        s.lights = &lamp; s.light_count = 1;
        s.surfaces = surf.data(); s.surface_count = n_surfaces;
        s.environment_light = -1;
        s.camera.position[2] = cz; s.camera.front[2] = 1.f; s.camera.right[0] = 2.f; s.camera.up[1] = 0.5f;   // a 4 : 1 frame, half a unit high at unit depth
        s.camera.resolution[0] = 256.f; s.camera.resolution[1] = 64.f;
        return s;
    };
    auto whole = [&](const ky_scene& s) {
        int r[4] = {-1, -1, -1, -1};
        long long c[2] = {-1, -1};
        return kyhip_scene_screen_bound(&s, &p, r, c) == KY_OK && r[0] == 0 && r[1] == 0 && r[2] == p.width && r[3] == p.height && c[0] == 0 && c[1] == 8 * 32;
    };
    {   // the box from far in front: columns around the middle, every row, and dead blocks on both sides
        const ky_scene s = scene_at(box, 5, -5.f);
        int r[4];
        long long c[2];
        if (kyhip_scene_screen_bound(&s, &p, r, c) != KY_OK || !(r[0] > 8 && r[2] < p.width - 8 && r[0] < 128 && r[2] > 128 && r[1] == 0 && r[3] == p.height && c[0] > 0 && c[0] < c[1])) return 1;
    }
    if (!whole(scene_at(box, 5, -1.f))) return 2;        // the camera on the bound's open face
    if (!whole(scene_at(box, 5, 0.f))) return 3;         // ... inside the bound
    if (!whole(scene_at(box, 0, -5.f))) return 4;        // no surfaces
    {
        std::vector<ky_shape> bad = box;
        bad[2].p[1][0] = q;                               // a NaN vertex
        if (!whole(scene_at(bad, 5, -5.f))) return 5;
        bad = box;
        bad[0].p[3][2] = std::numeric_limits<float>::infinity();
        if (!whole(scene_at(bad, 5, -5.f))) return 6;
    }
    {   // a sphere of radius zero at the origin: a point, a few pixels around the frame's centre
        ky_shape sp{};
        sp.kind = KY_SHAPE_SPHERE; sp.radius = 0.f;
        std::vector<ky_shape> one = {sp};
        const ky_scene s = scene_at(one, 1, -5.f);
        int r[4];
        if (kyhip_scene_screen_bound(&s, &p, r, nullptr) != KY_OK || !(r[0] >= 125 && r[0] <= 127 && r[2] >= 129 && r[2] <= 131 && r[1] >= 29 && r[3] <= 35)) return 7;
        one[0].radius = q;
        if (!whole(scene_at(one, 1, -5.f))) return 8;
    }
    {   // the switch, and a NULL scene through the internal entry
        const ky_scene s = scene_at(box, 5, -5.f);
        const int prev = kyhip_set_screen_cull(0);
        const bool off = whole(s);
        kyhip_set_screen_cull(prev);
        if (!off || kyhip_set_screen_cull(-1) != prev) return 9;
        int32_t live[4];
        screen_bound(nullptr, live);
        if (live[0] != 0 || live[2] != KY_LIVE_MAX) return 10;
    }
    return 0;
}

// Pixel filters (ky_pack.cpp), host side: check, defaults and table (monotone, ends exact, symmetric) for every kind at the ends of the radius
// range; the header fold (the box leaves a frame's scene hash alone, two radii give two hashes, a filter is refused once the frame holds samples); the widened live
// rectangle on kyhostcheck_screen_bound's two scenes.  Returns 0, or the number of the case that went wrong.
int kyhostcheck_filter(void) {
    const float q = std::numeric_limits<float>::quiet_NaN();
    constexpr int T = KYHIP_FILTER_TABLE + 1;
    {   // what the check refuses, one rule at a time, and what it accepts
        const ky_pixel_filter ok[] = {{KY_FILTER_BOX, 0.f, 0.f, 0}, {KY_FILTER_BOX, 99.f, q, 0}, {KY_FILTER_TENT, 0.5f, 0.f, 0}, {KY_FILTER_TENT, 4.f, q, 0},
                                      {KY_FILTER_GAUSSIAN, 1.5f, 0.5f, 0}, {KY_FILTER_BLACKMAN_HARRIS, 2.f, -1.f, 0}};
        for (const ky_pixel_filter& f : ok) if (kyhip_filter_check(&f) != KY_OK) return 1;
        const ky_pixel_filter bad[] = {{-1, 2.f, 0.f, 0}, {4, 2.f, 0.f, 0}, {KY_FILTER_TENT, 0.49f, 0.f, 0}, {KY_FILTER_TENT, 4.01f, 0.f, 0}, {KY_FILTER_TENT, q, 0.f, 0},
                                       {KY_FILTER_TENT, std::numeric_limits<float>::infinity(), 0.f, 0}, {KY_FILTER_GAUSSIAN, 1.5f, 0.f, 0}, {KY_FILTER_GAUSSIAN, 1.5f, -0.5f, 0},
                                       {KY_FILTER_GAUSSIAN, 1.5f, q, 0}, {KY_FILTER_TENT, 2.f, 0.f, 1}, {KY_FILTER_BOX, 0.f, 0.f, 7}};
        for (const ky_pixel_filter& f : bad) if (kyhip_filter_check(&f) != KY_ERR_INVALID_VALUE) return 2;
        if (kyhip_filter_check(nullptr) != KY_ERR_INVALID_VALUE) return 3;
    }
    {   // the defaults
        ky_pixel_filter f;
        if (kyhip_filter_defaults(KY_FILTER_TENT, &f) != KY_OK || f.kind != KY_FILTER_TENT || f.radius != 2.f || f.reserved != 0 || kyhip_filter_check(&f) != KY_OK) return 4;
        if (kyhip_filter_defaults(KY_FILTER_GAUSSIAN, &f) != KY_OK || f.radius != 1.5f || f.param != 0.5f || kyhip_filter_check(&f) != KY_OK) return 5;
        if (kyhip_filter_defaults(KY_FILTER_BLACKMAN_HARRIS, &f) != KY_OK || f.radius != 2.f || kyhip_filter_check(&f) != KY_OK) return 6;
        if (kyhip_filter_defaults(KY_FILTER_BOX, &f) != KY_OK || f.kind != KY_FILTER_BOX) return 7;
        if (kyhip_filter_defaults(9, &f) != KY_ERR_INVALID_VALUE || kyhip_filter_defaults(KY_FILTER_TENT, nullptr) != KY_ERR_INVALID_VALUE) return 8;
    }
    {   // the table
        const ky_pixel_filter fs[] = {{KY_FILTER_BOX, 0.f, 0.f, 0}, {KY_FILTER_TENT, 0.5f, 0.f, 0}, {KY_FILTER_TENT, 4.f, 0.f, 0}, {KY_FILTER_GAUSSIAN, 0.5f, 0.5f, 0},
                                      {KY_FILTER_GAUSSIAN, 1.5f, 0.5f, 0}, {KY_FILTER_GAUSSIAN, 4.f, 1.f, 0}, {KY_FILTER_GAUSSIAN, 4.f, 0.25f, 0},
                                      {KY_FILTER_BLACKMAN_HARRIS, 0.5f, 0.f, 0}, {KY_FILTER_BLACKMAN_HARRIS, 2.f, 0.f, 0}, {KY_FILTER_BLACKMAN_HARRIS, 4.f, 0.f, 0}};
        for (const ky_pixel_filter& f : fs) {
            std::vector<float> t(T, q);
            if (kyhip_filter_table(&f, t.data(), T) != KY_OK) return 9;
            const float R = f.kind == KY_FILTER_BOX ? 0.5f : f.radius;
            if (t[0] != -R || t[T - 1] != R || t[T / 2] != 0.f) return 10;
            for (int i = 0; i + 1 < T; ++i) if (!(t[i] <= t[i + 1])) return 11;
            for (int i = 0; i < T; ++i) if (t[i] != -t[T - 1 - i]) return 12;
            if (f.kind == KY_FILTER_TENT && std::fabs((double)t[T / 4] - (double)R * (std::sqrt(0.5) - 1)) > 1e-6) return 13;   // F^-1(1/4) = R (sqrt(1/2) - 1)
        }
        std::vector<float> t(T);
        if (kyhip_filter_table(&fs[1], t.data(), T - 1) != KY_ERR_INVALID_VALUE || kyhip_filter_table(&fs[1], nullptr, T) != KY_ERR_INVALID_VALUE) return 14;
        const ky_pixel_filter bad = {KY_FILTER_TENT, 5.f, 0.f, 0};
        if (kyhip_filter_table(&bad, t.data(), T) != KY_ERR_INVALID_VALUE) return 15;
    }
    {   // the header fold, and when a frame takes a filter
        ky_render_params p{};
        p.integrator = KY_INTEGRATOR_PATH_TRACING_ITERATION; p.max_path_depth = 5; p.direct_sample = KY_DIRECT_BOTH_MIS; p.samples_per_pixel = 64; p.sampler = KY_SAMPLER_RANDOM;
        p.width = 16; p.height = 16; p.tile_w = 16; p.tile_h = 16; p.tile_first = 0; p.tile_step = 1;
        const ky_pixel_filter box = {KY_FILTER_BOX, 3.f, 0.f, 0}, t1 = {KY_FILTER_TENT, 1.f, 0.f, 0}, t2 = {KY_FILTER_TENT, 2.f, 7.f, 0}, t2b = {KY_FILTER_TENT, 2.f, 0.f, 0},
                              g = {KY_FILTER_GAUSSIAN, 1.5f, 0.5f, 0}, g2 = {KY_FILTER_GAUSSIAN, 1.5f, 0.25f, 0};
        FrameBook a, b;
        a.begin(&p, 0x1234, 0, 64);
        b.begin(&p, 0x1234, 0, 0);   // (a collector: it may merge what a holds)
        if (a.set_filter(&box) != KY_OK || a.header.scene_hash != 0x1234 || std::memcmp(&a.header, &b.header, sizeof a.header) != 0) return 16;
        if (a.set_filter(&t1) != KY_OK || b.set_filter(&t2) != KY_OK) return 17;
        if (a.header.scene_hash == 0x1234 || b.header.scene_hash == 0x1234 || a.header.scene_hash == b.header.scene_hash) return 18;
        const uint64_t h2 = b.header.scene_hash;
        if (b.set_filter(&t2b) != KY_OK || b.header.scene_hash != h2) return 19;   // (a tent's param names nothing)
        if (b.set_filter(&g) != KY_OK || b.header.scene_hash == h2) return 20;
        const uint64_t hg = b.header.scene_hash;
        if (b.set_filter(&g2) != KY_OK || b.header.scene_hash == hg) return 21;
        if (b.set_filter(&box) != KY_OK || b.header.scene_hash != 0x1234 || b.filter.kind != KY_FILTER_BOX) return 22;
        MergeStep ms;
        if (b.merge_book(a, &ms) != KY_ERR_INVALID_VALUE || last_error().find("pixel filter") == std::string::npos) return 23;
        if (b.set_filter(&t1) != KY_OK || b.merge_book(a, &ms) != KY_OK) return 24;
        // a saved state of the tent frame: the box frame and the Gaussian frame refuse it, the tent frame loads it; then no filter is taken any more
        std::vector<unsigned char> state(a.layout.total, 0);
        if (a.save_host(state.data(), state.size()) != KY_OK) return 25;
        FrameBook c;
        c.begin(&p, 0x1234, 0, 64);
        CheckpointCounts n;
        if (c.load_check(state.data(), state.size(), &n) != KY_ERR_INVALID_VALUE || last_error().find("pixel filter") == std::string::npos) return 26;
        if (c.set_filter(&g) != KY_OK || c.load_check(state.data(), state.size(), &n) != KY_ERR_INVALID_VALUE || last_error().find("Gaussian") == std::string::npos) return 27;
        if (c.set_filter(&t1) != KY_OK || c.load_check(state.data(), state.size(), &n) != KY_OK) return 28;
        c.commit_load(n);
        if (c.set_filter(&t1) != KY_ERR_INVALID_VALUE || c.set_filter(&box) != KY_ERR_INVALID_VALUE) return 29;
        const ky_pixel_filter bad = {KY_FILTER_TENT, 0.25f, 0.f, 0};
        if (a.set_filter(&bad) != KY_ERR_INVALID_VALUE || a.set_filter(nullptr) != KY_ERR_INVALID_VALUE || a.filter.radius != 1.f) return 30;
    }
    {   // the widened rectangle: kyhostcheck_screen_bound's box from far in front, and its point
        ky_shape sp{};
        sp.kind = KY_SHAPE_SPHERE; sp.radius = 0.f;
        ky_material matte{};
        matte.kind = KY_MATERIAL_MATTE; matte.color0[0] = matte.color0[1] = matte.color0[2] = 0.5f;
        ky_light lamp{};
        lamp.kind = KY_LIGHT_POINT; lamp.color[0] = lamp.color[1] = lamp.color[2] = 1.f;
        auto rect_shape = [](const float (&pts)[4][3], float nx, float ny, float nz) {
            ky_shape r{};
            r.kind = KY_SHAPE_RECTANGLE;
            std::memcpy(r.p, pts, sizeof r.p);
            r.normal[0] = nx; r.normal[1] = ny; r.normal[2] = nz;
            return r;
        };
        const float back[4][3] = {{-1, -1, 1}, {1, -1, 1}, {1, 1, 1}, {-1, 1, 1}}, floor_[4][3] = {{-1, -1, -1}, {1, -1, -1}, {1, -1, 1}, {-1, -1, 1}},
                    ceil_[4][3] = {{-1, 1, -1}, {1, 1, -1}, {1, 1, 1}, {-1, 1, 1}}, left[4][3] = {{-1, -1, -1}, {-1, -1, 1}, {-1, 1, 1}, {-1, 1, -1}},
                    right[4][3] = {{1, -1, -1}, {1, -1, 1}, {1, 1, 1}, {1, 1, -1}};
        const std::vector<ky_shape> box5 = {rect_shape(back, 0, 0, -1), rect_shape(floor_, 0, 1, 0), rect_shape(ceil_, 0, -1, 0), rect_shape(left, 1, 0, 0), rect_shape(right, -1, 0, 0)};
        std::vector<ky_surface> surf;
        for (int i = 0; i < 5; ++i) surf.push_back(ky_surface{i, 0, -1});
        ky_render_params p{};
        p.integrator = KY_INTEGRATOR_PATH_TRACING_ITERATION; p.max_path_depth = 5; p.direct_sample = KY_DIRECT_BOTH_MIS; p.samples_per_pixel = 4; p.sampler = KY_SAMPLER_RANDOM;
        p.width = 256; p.height = 64; p.tile_w = 32; p.tile_h = 32; p.tile_first = 0; p.tile_step = 1;
        for (int which = 0; which < 2; ++which) {
            ky_scene s{};
            s.shapes = which ? &sp : box5.data(); s.shape_count = which ? 1 : 5;
            s.materials = &matte; s.material_count = 1;
            s.lights = &lamp; s.light_count = 1;
            s.surfaces = surf.data(); s.surface_count = which ? 1 : 5;
            s.environment_light = -1;
            s.camera.position[2] = -5.f; s.camera.front[2] = 1.f; s.camera.right[0] = 2.f; s.camera.up[1] = 0.5f;
            s.camera.resolution[0] = 256.f; s.camera.resolution[1] = 64.f;
            int r0[4], r[4];
            long long c0[2], c[2];
            if (kyhip_scene_screen_bound(&s, &p, r0, c0) != KY_OK || !(c0[0] > 0)) return 31 + which;
            const ky_pixel_filter box = {KY_FILTER_BOX, 0.f, 0.f, 0};
            if (kyhip_scene_screen_bound_filtered(&s, &p, &box, r, c) != KY_OK || std::memcmp(r, r0, sizeof r) != 0 || c[0] != c0[0] || c[1] != c0[1]) return 33 + which;
            if (kyhip_scene_screen_bound_filtered(&s, &p, nullptr, r, c) != KY_OK || std::memcmp(r, r0, sizeof r) != 0) return 35 + which;
            const float radii[] = {0.5f, 0.75f, 1.5f, 2.f, 4.f};
            const int grows[] = {0, 1, 1, 2, 4};
            for (int k = 0; k < 5; ++k) {
                const ky_pixel_filter f = {KY_FILTER_TENT, radii[k], 0.f, 0};
                if (kyhip_scene_screen_bound_filtered(&s, &p, &f, r, c) != KY_OK) return 37 + which;
                const int g = grows[k];
                if (r[0] != std::max(r0[0] - g, 0) || r[1] != std::max(r0[1] - g, 0) || r[2] != std::min(r0[2] + g, p.width) || r[3] != std::min(r0[3] + g, p.height)) return 39 + which;
                if (c[1] != c0[1] || c[0] > c0[0]) return 41 + which;   // a wider rectangle skips no more blocks
            }
            const ky_pixel_filter bad = {KY_FILTER_TENT, 9.f, 0.f, 0};
            if (kyhip_scene_screen_bound_filtered(&s, &p, &bad, r, c) != KY_ERR_INVALID_VALUE) return 43 + which;
        }
    }
    return 0;
}

// The thin lens (ky_pack.cpp, ky_frame_book.cpp), host side: the launch constants of a camera whose vectors are not unit length; the header
// fold (the pinhole leaves a frame's scene hash alone whatever its focus distance, two radii and two focus distances give different hashes, a lens and a filter
// fold independently and in either order of setting); when a frame takes a lens; what a frame with another lens refuses, and that the refusal names the lens.
// Returns 0, or the number of the case that went wrong.
int kyhostcheck_lens(void) {
    {   // the constants: radius / |right|, radius / |up|, w |front| / focus, h |front| / focus
        ky_camera cam{};
        cam.front[2] = 2.f; cam.right[0] = 4.f; cam.up[1] = 0.5f; cam.resolution[0] = 256.f; cam.resolution[1] = 64.f;
        const ky_lens l = {0.25f, 8.f, {0, 0}};
        const LensConst c = lens_const(&cam, &l);
        if (c.ar != 0.0625f || c.bu != 0.5f || c.wf != 64.f || c.hf != 16.f) return 1;
    }
    ky_render_params p{};
    p.integrator = KY_INTEGRATOR_PATH_TRACING_ITERATION; p.max_path_depth = 5; p.direct_sample = KY_DIRECT_BOTH_MIS; p.samples_per_pixel = 64; p.sampler = KY_SAMPLER_RANDOM;
    p.width = 16; p.height = 16; p.tile_w = 16; p.tile_h = 16; p.tile_first = 0; p.tile_step = 1;
    const ky_lens pin = {0.f, 3.f, {0, 0}}, l1 = {0.05f, 2.f, {0, 0}}, l2 = {0.06f, 2.f, {0, 0}}, l3 = {0.05f, 1.5f, {0, 0}}, bad = {0.05f, 0.f, {0, 0}};
    const ky_pixel_filter tent = {KY_FILTER_TENT, 2.f, 0.f, 0}, box = {KY_FILTER_BOX, 0.f, 0.f, 0};
    FrameBook a, b;
    a.begin(&p, 0x1234, 0, 64);
    b.begin(&p, 0x1234, 0, 0);   // (a collector)
    if (a.set_lens(&pin) != KY_OK || a.header.scene_hash != 0x1234 || a.lens.focus_distance != 0.f || std::memcmp(&a.header, &b.header, sizeof a.header) != 0) return 2;
    if (a.set_lens(&l1) != KY_OK || b.set_lens(&l2) != KY_OK) return 3;
    const uint64_t h1 = a.header.scene_hash, h2 = b.header.scene_hash;
    if (h1 == 0x1234 || h2 == 0x1234 || h1 == h2) return 4;
    if (b.set_lens(&l3) != KY_OK || b.header.scene_hash == h1 || b.header.scene_hash == h2) return 5;
    if (b.set_lens(&bad) != KY_ERR_INVALID_VALUE || b.set_lens(nullptr) != KY_ERR_INVALID_VALUE || b.lens.focus_distance != 1.5f) return 6;
    // the lens and the filter fold independently: set in either order they give one hash, which is neither's alone
    if (a.set_filter(&tent) != KY_OK) return 7;
    const uint64_t both = a.header.scene_hash;
    if (b.set_filter(&tent) != KY_OK || b.set_lens(&l1) != KY_OK || b.header.scene_hash != both || both == h1 || both == filter_fold(0x1234, &tent)) return 8;
    if (a.set_filter(&box) != KY_OK || a.header.scene_hash != h1) return 9;
    MergeStep ms;
    if (b.merge_book(a, &ms) != KY_ERR_INVALID_VALUE || last_error().find("filter") == std::string::npos) return 10;   // (same lens, another filter)
    if (b.set_filter(&box) != KY_OK || b.set_lens(&l2) != KY_OK || b.merge_book(a, &ms) != KY_ERR_INVALID_VALUE || last_error().find("lens radius 0.06, focus 2") == std::string::npos) return 11;
    if (b.set_lens(&l1) != KY_OK || b.merge_book(a, &ms) != KY_OK) return 12;
    // a saved state of the lens frame: the pinhole frame and a frame with another lens refuse it, the same lens loads it; then no lens is taken any more
    std::vector<unsigned char> state(a.layout.total, 0);
    if (a.save_host(state.data(), state.size()) != KY_OK) return 13;
    FrameBook c;
    c.begin(&p, 0x1234, 0, 64);
    CheckpointCounts n;
    if (c.load_check(state.data(), state.size(), &n) != KY_ERR_INVALID_VALUE || last_error().find("lens") == std::string::npos) return 14;
    if (c.set_lens(&l3) != KY_OK || c.load_check(state.data(), state.size(), &n) != KY_ERR_INVALID_VALUE || last_error().find("lens radius 0.05, focus 1.5") == std::string::npos) return 15;
    if (c.set_lens(&l1) != KY_OK || c.load_check(state.data(), state.size(), &n) != KY_OK) return 16;
    c.commit_load(n);
    if (c.set_lens(&l1) != KY_ERR_INVALID_VALUE || c.set_lens(&pin) != KY_ERR_INVALID_VALUE || last_error().find("lens") == std::string::npos) return 17;
    FrameBook d;   // a pinhole state into a lens frame: "without a lens"
    d.begin(&p, 0x1234, 0, 64);
    std::vector<unsigned char> plain(d.layout.total, 0);
    if (d.save_host(plain.data(), plain.size()) != KY_OK) return 18;
    FrameBook e;
    e.begin(&p, 0x1234, 0, 64);
    if (e.set_lens(&l1) != KY_OK || e.load_check(plain.data(), plain.size(), &n) != KY_ERR_INVALID_VALUE || last_error().find("without a lens") == std::string::npos) return 19;
    return 0;
}

// ---- the entry points that need a GPU: absent from this build. They exist as symbols because the host mirror (ky.hpp) and ctypes resolve every
// symbol when a library is loaded; each validates what the product validates before it touches a device where a CPU test looks at that, and then
// reports that there is no device -- exactly what libkyhip.so reports on a machine without a gfx950 GPU.
static int no_gpu() { return fail(KY_ERR_NO_DEVICE, "sanitizer build of the host-only code: no GPU entry points"); }
int kyhip_device_count(void) { return 0; }
int kyhip_render(int, const ky_scene*, const ky_render_params* p, float*, size_t) { return valid_params(p) ? no_gpu() : fail(KY_ERR_INVALID_VALUE, "invalid render params"); }
int kyhip_render_multi(const int*, int, const ky_scene*, const ky_render_params* p, float*, size_t) { return valid_params(p) ? no_gpu() : fail(KY_ERR_INVALID_VALUE, "invalid render params"); }
int kyhip_render_tiles_device(int, const ky_scene*, const ky_render_params* p, float*, void*, size_t, void*) { return valid_params(p) ? no_gpu() : fail(KY_ERR_INVALID_VALUE, "invalid render params"); }
int kyhip_film_add_tiles_device(int, const ky_render_params*, const float*, float*, size_t, void*) { return no_gpu(); }
int kyhip_film_add_gathered_device(int, const ky_render_params*, int, const float*, size_t, float*, size_t, void*) { return no_gpu(); }
float kyhip_kernel_ms(int) { return -1.f; }
const char* kyhip_last_kernel(int) { return ""; }
const char* kyhip_multi_status(int) { return ""; }
void* kyhip_film_alloc(size_t) { return nullptr; }   // no device: callers fall back to ordinary memory
void kyhip_film_free(void*) {}
int kyhip_kat_intersect(int, const ky_shape*, const float*, int, float*) { return no_gpu(); }
int kyhip_kat_camera(int, const ky_camera*, const float*, int, float*) { return no_gpu(); }
int kyhip_kat_bsdf(int, const ky_material*, const float*, int, float*) { return no_gpu(); }
int kyhip_kat_bsdf_continue(int, const ky_material*, const float*, int, int, float*) { return no_gpu(); }
int kyhip_kat_light(int, const ky_scene*, int, const float*, int, float*) { return no_gpu(); }
int kyhip_kat_scene_intersect(int, const ky_scene*, const float*, int, float*) { return no_gpu(); }
int kyhip_kat_occluded(int, const ky_scene*, const float*, int, float*) { return no_gpu(); }
int kyhip_kat_any_pair(int, const ky_scene*, const float*, int, float*) { return no_gpu(); }
int kyhip_kat_occluded_between(int, const ky_scene*, int, const float*, int, float*) { return no_gpu(); }
// (the stratified sampler's sample range is refused before any device work, like the real entry's: strat_samples_check is host code)
int kyhip_kat_li(int, const ky_scene*, const ky_render_params* p, int, int, int s0, int n, float*) {
    if (!valid_params(p)) return fail(KY_ERR_INVALID_VALUE, "invalid render params");
    KY_TRY(strat_samples_check(p, s0, n));
    return no_gpu();
}
// (the masked entries refuse an invalid mask before they look for a device, like the real ones: lighting_plan is host code)
int kyhip_render_lighting(int, const ky_scene*, const ky_render_params* p, int lighting, float*, size_t) { LightingPlan pl; const int rc = lighting_plan(p, lighting, &pl); return rc != KY_OK ? rc : no_gpu(); }
int kyhip_kat_li_lighting(int, const ky_scene*, const ky_render_params* p, int lighting, int, int, int, int, float*) { LightingPlan pl; const int rc = lighting_plan(p, lighting, &pl); return rc != KY_OK ? rc : no_gpu(); }
// (a frame refuses what the real entries refuse, by their own check, before it looks for a device; no frame ever exists here, so the other entries see NULL only)
int kyhip_frame_begin(int, const ky_scene* scene, const ky_render_params* p, kyhip_frame** out) {
    KY_TRY(begin_check(scene, p, 0, p ? p->samples_per_pixel : 0, out));
    return no_gpu();
}
int kyhip_frame_begin_slice(int, const ky_scene* scene, const ky_render_params* p, int first_sample, int end_sample, kyhip_frame** out) {
    KY_TRY(begin_check(scene, p, first_sample, end_sample, out));
    return no_gpu();
}
int kyhip_frame_coverage(const kyhip_frame*, int*, int, int*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_merge(kyhip_frame*, const void*, size_t) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_merge_from(kyhip_frame*, kyhip_frame*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_merge_ms(const kyhip_frame*, float*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_render(kyhip_frame*, int, int*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_samples(const kyhip_frame*, int*, int*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_resolve(kyhip_frame*, int, float*, size_t) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int64_t kyhip_frame_state_bytes(const kyhip_frame*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_save(kyhip_frame*, void*, size_t) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_load(kyhip_frame*, const void*, size_t) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
void kyhip_frame_end(kyhip_frame*) {}
// (the noise and block entries refuse their other arguments first, by the real ones' own checks in the real ones' order: ky_host.hpp)
static int no_frame(const void* out) { return fail(KY_ERR_INVALID_VALUE, out ? "frame is NULL" : "out is NULL"); }
int kyhip_frame_track_noise(kyhip_frame*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_noise(kyhip_frame*, float*, size_t) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_noise_stats(kyhip_frame*, float threshold, ky_noise_stats* out) {
    KY_TRY(threshold_check(threshold));
    return no_frame(out);
}
int kyhip_frame_render_until(kyhip_frame*, float threshold, float max_fraction_above, int min_batches, int min_samples_per_pass, int*, ky_noise_stats* out) {
    KY_TRY(stop_rule_check(threshold, max_fraction_above, min_batches));
    KY_TRY(pass_samples_check(min_samples_per_pass));
    return no_frame(out);
}
int kyhip_frame_noise_ms(const kyhip_frame*, float*, float*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_track_blocks(kyhip_frame*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_keep(kyhip_frame*, const unsigned char* mask, size_t) { return fail(KY_ERR_INVALID_VALUE, mask ? "frame is NULL" : "mask is NULL"); }
int kyhip_frame_retire_noisy(kyhip_frame*, float threshold, float max_fraction_above, int min_batches, ky_block_stats* out) {
    KY_TRY(stop_rule_check(threshold, max_fraction_above, min_batches));
    return no_frame(out);
}
int kyhip_frame_render_adaptive(kyhip_frame*, float threshold, float max_fraction_above, int min_batches, int min_samples_per_pass, int*, ky_block_stats* out) {
    KY_TRY(stop_rule_check(threshold, max_fraction_above, min_batches));
    KY_TRY(pass_samples_check(min_samples_per_pass));
    return no_frame(out);
}
int kyhip_frame_sample_map(kyhip_frame*, int32_t*, size_t) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_block_stats(kyhip_frame*, ky_block_stats* out) { return no_frame(out); }
int kyhip_frame_blocks_ms(const kyhip_frame*, float*, float*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
// (the denoise entries: the parameters first, as the real ones check them; kyhip_denoise_defaults is host code, ky_pack.cpp)
int kyhip_frame_denoise(kyhip_frame*, const ky_denoise_params* p, float*, size_t) {
    ky_denoise_params q;
    kyhip_denoise_defaults(&q);
    if (p) q = *p;
    KY_TRY(denoise_params_check(&q));
    return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
}
int kyhip_frame_guides(kyhip_frame*, float*, float*, size_t) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_denoise_ms(const kyhip_frame*, float*, float*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_set_guide_bounces(kyhip_frame*, int bounces) {
    if (bounces < 0 || bounces > KYHIP_GUIDE_MAX_BOUNCES) return fail(KY_ERR_INVALID_VALUE, "guide bounces %d: 0 .. %d", bounces, KYHIP_GUIDE_MAX_BOUNCES);
    return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
}
int kyhip_frame_guide_bounces(const kyhip_frame*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_guide_chains(kyhip_frame*, uint64_t*, size_t) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_set_albedo_grid(kyhip_frame*, int grid) {
    if (grid < 0 || grid > KYHIP_ALBEDO_MAX_GRID) return fail(KY_ERR_INVALID_VALUE, "albedo grid %d: 0 .. %d", grid, KYHIP_ALBEDO_MAX_GRID);
    return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
}
int kyhip_frame_albedo_grid(const kyhip_frame*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_albedo(kyhip_frame*, float*, size_t) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_frame_albedo_ms(const kyhip_frame*, float*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
// (the temporal entries: both parameter sets first, as the real one checks them; a history needs a device; kyhip_temporal_defaults is host code, ky_pack.cpp)
int kyhip_history_create(int, int width, int height, kyhip_history** out) {
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    *out = nullptr;
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 28)) return fail(KY_ERR_INVALID_VALUE, "a history of %d x %d pixels", width, height);
    return no_gpu();
}
int kyhip_history_destroy(kyhip_history*) { return fail(KY_ERR_INVALID_VALUE, "history is NULL"); }
int kyhip_history_reset(kyhip_history*) { return fail(KY_ERR_INVALID_VALUE, "history is NULL"); }
int kyhip_history_frames(const kyhip_history*) { return fail(KY_ERR_INVALID_VALUE, "history is NULL"); }
int kyhip_history_read(kyhip_history*, float*, float*, size_t) { return fail(KY_ERR_INVALID_VALUE, "history is NULL"); }
int kyhip_history_ms(const kyhip_history*, float*) { return fail(KY_ERR_INVALID_VALUE, "history is NULL"); }
int kyhip_frame_denoise_temporal(kyhip_frame*, kyhip_history*, const ky_denoise_params* p, const ky_temporal_params* t, float*, size_t) {
    ky_denoise_params q;
    kyhip_denoise_defaults(&q);
    if (p) q = *p;
    ky_temporal_params tt;
    kyhip_temporal_defaults(&tt);
    if (t) tt = *t;
    KY_TRY(denoise_params_check(&q));
    KY_TRY(temporal_params_check(&tt));
    return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
}
// (the filter entries refuse an invalid filter before they look for a device or a frame, like the real ones: filter_check is host code; a box filter is the unfiltered entry)
int kyhip_render_filtered(int device, const ky_scene* scene, const ky_render_params* p, const ky_pixel_filter* filter, float* film, size_t stride) {
    if (filter) KY_TRY(filter_check(filter));
    return kyhip_render(device, scene, p, film, stride);
}
int kyhip_frame_set_filter(kyhip_frame*, const ky_pixel_filter* filter) {
    KY_TRY(filter_check(filter));
    return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
}
int kyhip_frame_filter(const kyhip_frame*, ky_pixel_filter*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_kat_filter(int, const ky_pixel_filter* filter, const float*, int, float*) {
    KY_TRY(filter_check(filter));
    return no_gpu();
}
int kyhip_kat_li_filtered(int device, const ky_scene* scene, const ky_render_params* p, const ky_pixel_filter* filter, int x, int y, int s0, int n, float* out3) {
    if (filter) KY_TRY(filter_check(filter));
    return kyhip_kat_li(device, scene, p, x, y, s0, n, out3);
}
// (... and the lens entries an invalid lens, then an invalid filter: lens_check is host code; the pinhole is the filtered entry)
int kyhip_render_lens(int device, const ky_scene* scene, const ky_render_params* p, const ky_pixel_filter* filter, const ky_lens* lens, float* film, size_t stride) {
    if (lens) KY_TRY(lens_check(lens));
    return kyhip_render_filtered(device, scene, p, filter, film, stride);
}
int kyhip_frame_set_lens(kyhip_frame*, const ky_lens* lens) {
    KY_TRY(lens_check(lens));
    return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
}
int kyhip_frame_lens(const kyhip_frame*, ky_lens*) { return fail(KY_ERR_INVALID_VALUE, "frame is NULL"); }
int kyhip_kat_lens(int, const float*, int, float*) { return no_gpu(); }
int kyhip_kat_li_lens(int device, const ky_scene* scene, const ky_render_params* p, const ky_pixel_filter* filter, const ky_lens* lens, int x, int y, int s0, int n, float* out3) {
    if (lens) KY_TRY(lens_check(lens));
    return kyhip_kat_li_filtered(device, scene, p, filter, x, y, s0, n, out3);
}
// (... and the texture entries an invalid set first: texture_check is host code; no textures is the lens entry)
int kyhip_render_textured(int device, const ky_scene* scene, const ky_texture* textures, int n, const ky_render_params* p, const ky_pixel_filter* filter, const ky_lens* lens,
                          float* film, size_t stride) {
    KY_TRY(texture_check(scene, textures, n));
    if (n == 0) return kyhip_render_lens(device, scene, p, filter, lens, film, stride);
    return no_gpu();
}
int kyhip_frame_set_textures(kyhip_frame*, const ky_texture* textures, int n) {
    if (n < 0 || (n > 0 && !textures)) return fail(KY_ERR_INVALID_VALUE, "bad texture arguments");
    if (n > KYHIP_MAX_TEXTURES) return fail(KY_ERR_LIMIT, "textures: %d, at most %d", n, KYHIP_MAX_TEXTURES);
    return fail(KY_ERR_INVALID_VALUE, "frame is NULL");
}
int kyhip_kat_li_textured(int device, const ky_scene* scene, const ky_texture* textures, int n_textures, const ky_render_params* p, const ky_pixel_filter* filter,
                          const ky_lens* lens, int x, int y, int s0, int n, float* out3) {
    KY_TRY(texture_check(scene, textures, n_textures));
    if (n_textures == 0) return kyhip_kat_li_lens(device, scene, p, filter, lens, x, y, s0, n, out3);
    return no_gpu();
}
int kyhip_kat_texture(int, const ky_scene* scene, const ky_texture* textures, int n_textures, int, const float*, int, float*) {
    KY_TRY(texture_check(scene, textures, n_textures));
    return no_gpu();
}
int kyhip_kat_nee(int, const ky_scene*, int, int, const float*, int, float*) { return no_gpu(); }
int kyhip_kat_light_pick(int, const ky_scene*, int, const float*, int, float*) { return no_gpu(); }   // (kyhip_scene_light_pick is host code: ky_pack.cpp)
int kyhip_kat_single_light_rule(int, const ky_scene*, int, const float*, int, float*) { return no_gpu(); }
int kyhip_kat_li_trace(int, const ky_scene*, const ky_render_params*, int, int, int, float*, int, float*) { return no_gpu(); }
int kyhip_smallpt_render(int, const ky_smallpt_sphere* spheres, int n, const ky_smallpt_params* p, double* image) {
    const int rc = smallpt_check(spheres, n, p);
    if (rc != KY_OK) return rc;
    return image ? no_gpu() : fail(KY_ERR_INVALID_VALUE, "null image");
}
int kyhip_smallpt_kat_radiance(int, const ky_smallpt_sphere* spheres, int n, const ky_smallpt_params* p, int x, int y, int sx, int sy, int s0, int cnt, double* out3) {
    const int rc = smallpt_check(spheres, n, p);
    if (rc != KY_OK) return rc;
    if (!out3 || cnt <= 0 || s0 < 0 || x < 0 || y < 0 || x >= p->width || y >= p->height || (sx | sy) < 0 || sx > 1 || sy > 1) return fail(KY_ERR_INVALID_VALUE, "bad KAT arguments");
    if (p->variant == KY_SP_VARIANT_REWRITE && (sx | sy) != 0) return fail(KY_ERR_INVALID_VALUE, "variant 1 has no subpixels: sx = sy = 0");
    return no_gpu();
}
int kyhip_kat_sampler(int, uint32_t, const uint32_t*, int, int, int, uint32_t*) { return no_gpu(); }
int kyhip_kat_sampler_kind(int, int kind, uint32_t, int spp, const uint32_t* keys2, int n, int k, uint32_t* out) {
    KY_TRY(kat_sampler_kind_check(kind, spp, keys2, n, k, out));
    return no_gpu();
}
int kyhip_smallpt_kat_rng(int, uint32_t, const uint32_t*, int, int, uint64_t*) { return no_gpu(); }

}  // extern "C"
