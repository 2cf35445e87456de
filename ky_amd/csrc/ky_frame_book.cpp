/*
 * ky_frame_book.cpp -- the host side of a frame in passes, all of it: pass boundaries, what a checkpoint is (its header, layout, host-side parts and the check of a
 * buffer), slices, coverage and a merge's acceptance (ky_checkpoint.hpp), both trailer checks (ky_noise.hpp, ky_blocks.hpp), and the frame's book (ky_frame_book.hpp):
 * the state machine ky_frame.cpp's entries ask and commit to around their device work.  Plain C++17 with no HIP header and no HIP call: hipcc compiles it into the
 * library, `make sanitize` compiles the very same file with g++ -fsanitize=address,undefined and -fsanitize=thread, and kyhostcheck_book (ky_hostcheck.cpp) drives
 * whole life cycles through it without a GPU.
 */
#include <cstring>

#include "ky_frame_book.hpp"

namespace kyh {

// The sample counts at which a pass of an spp-sample frame can end: the ends of the chunks of chunk_plan(spp)
int pass_boundaries(int spp, int* bounds, int n) {
    if (spp < 1 || spp > (1 << 24)) return fail(KY_ERR_INVALID_VALUE, "pass boundaries of %d samples per pixel (1 .. 2^24)", spp);
    if (n > 0 && !bounds) return fail(KY_ERR_INVALID_VALUE, "bounds is NULL");
    const ChunkPlan plan = chunk_plan(spp);
    const int count = chunk_count(plan);
    for (int c = 0; c < count && c < n; ++c) bounds[c] = chunk_end(plan, c);
    return count;
}
FrameHeader frame_header(const ky_render_params* p, uint64_t hash, int samples_done) {
    FrameHeader h;
    std::memset(&h, 0, sizeof h);   // (padding too: headers are compared and saved as bytes)
    h.magic = KY_FRAME_MAGIC;
    h.source_hash = kyjit::source_hash();
    h.params = *p;
    h.scene_hash = hash;
    h.samples_done = samples_done;
    h.n_pix = make_shard(p).n_pix;
    return h;
}
static const char* magic_kind(uint64_t magic) {
    return magic == KY_FRAME_BLOCKS_MAGIC ? "retires pixel blocks" : magic == KY_FRAME_SLICE_MAGIC ? "owns a slice of its samples" : "does neither";
}
// what every reader of a state asks of its header: a frame state of own's identity, long enough; any_kind: whatever its magic, else own's
static int frame_header_check(const FrameHeader& own, const void* buf, size_t bytes, size_t state_end, bool any_kind, FrameHeader* out) {
    if (!buf || bytes < sizeof(FrameHeader)) return fail(KY_ERR_INVALID_VALUE, "frame state: %zu bytes hold no header", bytes);
    FrameHeader theirs;
    std::memcpy(&theirs, buf, sizeof theirs);
    if (theirs.magic != KY_FRAME_MAGIC && theirs.magic != KY_FRAME_BLOCKS_MAGIC && theirs.magic != KY_FRAME_SLICE_MAGIC)
        return fail(KY_ERR_INVALID_VALUE, "frame state: not a kyhip_frame_save buffer");
    if (!any_kind && theirs.magic != own.magic)
        return fail(KY_ERR_INVALID_VALUE, "frame state: saved by a frame that %s, this one %s (kyhip_frame_track_blocks, kyhip_frame_begin_slice)", magic_kind(theirs.magic),
                    magic_kind(own.magic));
    if (theirs.source_hash != own.source_hash) return fail(KY_ERR_INVALID_VALUE, "frame state: saved by a library with other kernel sources (%016llx, this one %016llx)",
                                                          (unsigned long long)theirs.source_hash, (unsigned long long)own.source_hash);
    FrameHeader same = theirs;
    same.samples_done = own.samples_done;
    same.magic = own.magic;
    if (std::memcmp(&same, &own, sizeof own) != 0) {
        same.scene_hash = own.scene_hash;   // (the header's scene hash carries the frame's pixel filter too: filter_fold, ky_pack.cpp)
        if (std::memcmp(&same, &own, sizeof own) == 0) return fail(KY_ERR_INVALID_VALUE, "frame state: saved from another frame (its scene, its pixel filter or its lens differs from this frame's; kyhip_frame_set_filter, kyhip_frame_set_lens)");
        return fail(KY_ERR_INVALID_VALUE, "frame state: saved from another frame (its render params, scene or film size differ from this frame's)");
    }
    if (bytes < state_end) return fail(KY_ERR_INVALID_VALUE, "frame state: %zu bytes, the frame's state has %zu", bytes, state_end);
    *out = theirs;
    return KY_OK;
}
// what a plain state at samples_done holds, [0, samples_done), and the chunks that are; refused where no chunk of the frame ends there
static int plain_coverage(int spp, int samples_done, Coverage* cov, int* chunks_done) {
    const int c = samples_done < 0 ? -1 : chunks_at_sample(chunk_plan(spp), samples_done);
    if (c < 0) return fail(KY_ERR_INVALID_VALUE, "frame state: no pass of a %d-sample frame ends at %d samples", spp, samples_done);
    Coverage held;
    if (samples_done > 0) { held.n = 1; held.r[0] = 0; held.r[1] = samples_done; }
    *cov = held;
    *chunks_done = c;
    return KY_OK;
}
int frame_state_check(const FrameHeader& own, const void* buf, size_t bytes, size_t state_end, int* chunks_done) {
    FrameHeader theirs;
    KY_TRY(frame_header_check(own, buf, bytes, state_end, false, &theirs));
    Coverage held;
    return plain_coverage(own.params.samples_per_pixel, theirs.samples_done, &held, chunks_done);
}

// ---- a checkpoint as a whole (ky_checkpoint.hpp) ----
CheckpointLayout checkpoint_layout(const ky_render_params* p, bool noise, bool blocks, int own_first, int own_end) {
    const ShardConst sh = make_shard(p);
    CheckpointLayout L;
    L.n_pix = sh.n_pix; L.n_blocks = sh.n_blocks; L.tracks_noise = noise; L.tracks_blocks = blocks;
    L.own_first = own_end < 0 ? 0 : own_first;
    L.own_end = own_end < 0 ? p->samples_per_pixel : own_end;
    L.sliced = !(L.own_first == 0 && L.own_end == p->samples_per_pixel);
    L.accum = sizeof(FrameHeader);
    L.noise = L.accum + workspace_bytes_for(sh);
    L.noise_pixels = L.noise + (noise ? sizeof(kyn::NoiseTrailer) : 0);
    L.blocks = L.noise_pixels + (noise ? (size_t)sh.n_pix * sizeof(kyn::NoisePixel) : 0);
    L.block_states = L.blocks + (blocks ? sizeof(kyb::BlockTrailer) : 0);
    L.slice = L.block_states + (blocks ? (size_t)sh.n_blocks * sizeof(kyb::BlockState) : 0);
    L.total = L.slice + (L.sliced ? sizeof(SliceTrailer) : 0);
    return L;
}
// the frame's header as its checkpoints carry it: the magic says whether the layout ends with blocks or with a slice trailer (never both: a slice tracks no blocks)
static FrameHeader checkpoint_header(FrameHeader own, const CheckpointLayout& L, int samples_done) {
    own.magic = L.sliced ? KY_FRAME_SLICE_MAGIC : L.tracks_blocks ? KY_FRAME_BLOCKS_MAGIC : KY_FRAME_MAGIC;
    own.samples_done = samples_done;
    return own;
}
void checkpoint_write_host(const FrameHeader& own, const CheckpointLayout& L, const CheckpointCounts& n, const kyb::BlockState* states, void* buf) {
    char* at = (char*)buf;
    const FrameHeader h = checkpoint_header(own, L, n.samples_done);
    std::memcpy(at, &h, sizeof h);
    if (L.tracks_noise) {
        const kyn::NoiseTrailer t = {kyn::KY_NOISE_MAGIC, n.batches, n.n_prev};
        std::memcpy(at + L.noise, &t, sizeof t);
    }
    if (L.tracks_blocks) {
        const kyb::BlockTrailer t = {kyb::KY_BLOCKS_MAGIC, L.n_blocks, n.passes};
        std::memcpy(at + L.blocks, &t, sizeof t);
        if (L.n_blocks > 0) std::memcpy(at + L.block_states, states, L.block_states_bytes());
    }
    if (L.sliced) {
        SliceTrailer t;
        std::memset(&t, 0, sizeof t);
        t.magic = KY_SLICE_MAGIC;
        t.own_first = L.own_first; t.own_end = L.own_end; t.front = n.front;
        t.n_ranges = n.cov.n;
        std::memcpy(t.ranges, n.cov.r, sizeof(int32_t) * 2 * (size_t)n.cov.n);
        std::memcpy(at + L.slice, &t, sizeof t);
    }
}
static Coverage trailer_coverage(const SliceTrailer& s) {
    Coverage cov;
    cov.n = s.n_ranges;
    std::memcpy(cov.r, s.ranges, sizeof s.ranges);
    return cov;
}
int checkpoint_check(const FrameHeader& own, const CheckpointLayout& L, const void* buf, size_t bytes, CheckpointCounts* out) {
    CheckpointCounts n;
    const int spp = own.params.samples_per_pixel;
    FrameHeader theirs;
    KY_TRY(frame_header_check(checkpoint_header(own, L, own.samples_done), buf, bytes, L.noise, false, &theirs));
    n.samples_done = n.front = theirs.samples_done;
    // (a slice's samples_done is the held count: checked against the trailers, not against a chunk end)
    if (!L.sliced) KY_TRY(plain_coverage(spp, n.samples_done, &n.cov, &n.chunks_done));
    if (L.tracks_noise) {   // (a frame that does not track accepts a longer buffer and ignores the trailer)
        kyn::NoiseTrailer t;
        KY_TRY(kyn::noise_trailer_check(buf, bytes, L.noise, L.n_pix, n.samples_done, &t));
        n.batches = t.batches; n.n_prev = t.n_prev;
    }
    if (L.sliced) {
        SliceTrailer s;
        KY_TRY(slice_trailer_check(buf, bytes, L.slice, spp, n.samples_done, L.own_first, L.own_end, &s));
        n.front = s.front;
        n.chunks_done = chunks_at_sample(chunk_plan(spp), s.front);
        n.cov = trailer_coverage(s);
    }
    if (L.tracks_blocks) {
        kyb::BlockTrailer t;
        KY_TRY(kyb::block_trailer_check(buf, bytes, L.blocks, L.n_blocks, spp, n.samples_done, n.batches, &t));
        n.passes = t.passes;
    }
    *out = n;
    return KY_OK;
}

// ---- slices (ky_checkpoint.hpp; DESIGN.md "Slices") ----
int slice_bounds(int spp, int n_slices, int* bounds) {
    const int count = pass_boundaries(spp, nullptr, 0);
    if (count < 0) return count;
    if (n_slices < 1 || !bounds) return fail(KY_ERR_INVALID_VALUE, "slice bounds: %d slices into %s", n_slices, bounds ? "bounds" : "a NULL bounds");
    if (count < n_slices) return fail(KY_ERR_INVALID_VALUE, "slice bounds: a %d-sample frame has %d chunks, fewer than %d slices", spp, count, n_slices);
    const ChunkPlan plan = chunk_plan(spp);
    bounds[0] = 0;
    int prev = -1;   // the chunk whose end the last bound is
    for (int k = 1; k < n_slices; ++k) {
        // the chunk end nearest to k * spp / n_slices, compared as integers times n_slices; the lower one on a tie ...
        const long long want = (long long)k * spp;
        int best = 0;
        long long best_d = -1;
        for (int c = 0; c < count; ++c) {
            long long d = (long long)chunk_end(plan, c) * n_slices - want;
            if (d < 0) d = -d;
            if (best_d < 0 || d < best_d) { best = c; best_d = d; }
        }
        // ... moved as little as it takes to leave a chunk to every slice before and behind it
        const int lo = prev + 1, hi = count - 1 - (n_slices - k);
        prev = best < lo ? lo : best > hi ? hi : best;
        bounds[k] = chunk_end(plan, prev);
    }
    bounds[n_slices] = spp;
    return KY_OK;
}
int slice_range_check(int spp, int first_sample, int end_sample) {
    const ChunkPlan plan = chunk_plan(spp);
    const bool ok = first_sample >= 0 && first_sample <= end_sample && end_sample <= spp && chunks_at_sample(plan, first_sample) >= 0 && chunks_at_sample(plan, end_sample) >= 0;
    return ok ? KY_OK : fail(KY_ERR_INVALID_VALUE, "a slice of samples %d..%d of %d: both are 0 or a pass boundary (kyhip_pass_boundaries), the first not beyond the end",
                             first_sample, end_sample, spp);
}
int coverage_union(const Coverage& a, const Coverage& b, Coverage* out) {
    int r[4 * KY_SLICE_MAX_RANGES + 2];
    int n = 0, i = 0, j = 0;
    while (i < a.n || j < b.n) {   // both ascending: the one that begins first is next
        const bool from_a = j >= b.n || (i < a.n && a.r[2 * i] <= b.r[2 * j]);
        const int first = from_a ? a.r[2 * i] : b.r[2 * j], end = from_a ? a.r[2 * i + 1] : b.r[2 * j + 1];
        if (from_a) ++i; else ++j;
        if (n > 0 && first < r[2 * n - 1])
            return fail(KY_ERR_INVALID_VALUE, "samples %d..%d are held twice: merged sample ranges must not intersect", first, end < r[2 * n - 1] ? end : r[2 * n - 1]);
        if (n > 0 && first == r[2 * n - 1]) r[2 * n - 1] = end;   // adjacent: joined
        else { r[2 * n] = first; r[2 * n + 1] = end; ++n; }
    }
    if (n > KY_SLICE_MAX_RANGES) return fail(KY_ERR_LIMIT, "%d sample ranges: a frame's coverage holds at most %d", n, KY_SLICE_MAX_RANGES);
    Coverage u;
    u.n = n;
    std::memcpy(u.r, r, sizeof(int) * 2 * (size_t)n);
    *out = u;
    return KY_OK;
}
int slice_trailer_check(const void* buf, size_t bytes, size_t offset, int total_spp, int samples_done, int own_first, int own_end, SliceTrailer* out) {
    if (!buf || bytes < offset || bytes - offset < sizeof(SliceTrailer))
        return fail(KY_ERR_INVALID_VALUE, "frame state: %zu bytes hold no slice trailer (the state of this frame has %zu)", bytes, offset + sizeof(SliceTrailer));
    SliceTrailer t;
    std::memcpy(&t, (const char*)buf + offset, sizeof t);
    if (t.magic != KY_SLICE_MAGIC) return fail(KY_ERR_INVALID_VALUE, "frame state: no slice trailer where this frame's state has one");
    const ChunkPlan plan = chunk_plan(total_spp);
    auto boundary = [&](int s) { return s >= 0 && s <= total_spp && chunks_at_sample(plan, s) >= 0; };
    if (!boundary(t.own_first) || !boundary(t.own_end) || t.own_first > t.own_end)
        return fail(KY_ERR_INVALID_VALUE, "frame state: a slice of samples %d..%d of %d: not a range between pass boundaries", t.own_first, t.own_end, total_spp);
    if (own_end >= 0 && (t.own_first != own_first || t.own_end != own_end))
        return fail(KY_ERR_INVALID_VALUE, "frame state: saved by the slice of samples %d..%d, this frame owns %d..%d", t.own_first, t.own_end, own_first, own_end);
    if (t.front < t.own_first || t.front > t.own_end || !boundary(t.front))
        return fail(KY_ERR_INVALID_VALUE, "frame state: the slice %d..%d stands at sample %d: outside it or on no pass boundary", t.own_first, t.own_end, t.front);
    if (t.n_ranges < 0 || t.n_ranges > KY_SLICE_MAX_RANGES) return fail(KY_ERR_INVALID_VALUE, "frame state: a coverage of %d sample ranges", t.n_ranges);
    int held = 0, last = -1, in_first = -1, in_end = -1, inside = 0;
    for (int i = 0; i < t.n_ranges; ++i) {
        const int first = t.ranges[2 * i], end = t.ranges[2 * i + 1];
        // (last: the end of the range before; equality would be two adjacent ranges that were not joined)
        if (!boundary(first) || !boundary(end) || first >= end || first <= last)
            return fail(KY_ERR_INVALID_VALUE, "frame state: sample range %d (%d..%d) of the coverage is not ascending, disjoint and between pass boundaries", i, first, end);
        last = end;
        held += end - first;
        const int a = first > t.own_first ? first : t.own_first, b = end < t.own_end ? end : t.own_end;   // its part inside the owned range
        if (a < b) { ++inside; in_first = a; in_end = b; }
    }
    const bool rendered_part_right = t.front == t.own_first ? inside == 0 : (inside == 1 && in_first == t.own_first && in_end == t.front);
    if (!rendered_part_right)
        return fail(KY_ERR_INVALID_VALUE, "frame state: the coverage inside the slice %d..%d is not the rendered part %d..%d", t.own_first, t.own_end, t.own_first, t.front);
    if (held != samples_done) return fail(KY_ERR_INVALID_VALUE, "frame state: the coverage holds %d samples, the header says %d", held, samples_done);
    if (out) *out = t;
    return KY_OK;
}
int merge_source_check(const FrameHeader& own, const void* buf, size_t bytes, MergeSource* out) {
    const ShardConst sh = make_shard(&own.params);
    MergeSource m;
    m.accum = sizeof(FrameHeader);
    const size_t noise = m.accum + workspace_bytes_for(sh);
    FrameHeader theirs;
    KY_TRY(frame_header_check(own, buf, bytes, noise, true, &theirs));
    if (theirs.magic == KY_FRAME_BLOCKS_MAGIC)
        return fail(KY_ERR_INVALID_VALUE, "frame state: saved by a frame that retires pixel blocks: its pixels stand at sample counts of their own and merge with nothing");
    const int spp = own.params.samples_per_pixel;
    // a noise trailer counts when it is valid as a whole: it is there, it is long enough and it stands at the header's samples
    size_t behind = noise;
    uint64_t magic = 0;
    if (bytes - noise >= sizeof magic) std::memcpy(&magic, (const char*)buf + noise, sizeof magic);
    if (magic == kyn::KY_NOISE_MAGIC) {
        kyn::NoiseTrailer t;
        KY_TRY(kyn::noise_trailer_check(buf, bytes, noise, sh.n_pix, theirs.samples_done, &t));
        m.noise_pixels = noise + sizeof t;
        m.batches = t.batches;
        behind = noise + kyn::noise_trailer_bytes(sh.n_pix);
    }
    if (theirs.magic == KY_FRAME_SLICE_MAGIC) {
        SliceTrailer s;
        KY_TRY(slice_trailer_check(buf, bytes, behind, spp, theirs.samples_done, 0, -1, &s));
        m.cov = trailer_coverage(s);
    } else {
        int chunks;
        KY_TRY(plain_coverage(spp, theirs.samples_done, &m.cov, &chunks));
    }
    *out = m;
    return KY_OK;
}
int merge_accept(const Coverage& mine, int own_first, int own_end, int total_spp, bool tracks_noise, bool tracks_blocks, const Coverage& theirs, bool has_noise, Coverage* merged) {
    if (tracks_blocks) return fail(KY_ERR_INVALID_VALUE, "merge: the receiving frame retires pixel blocks: its pixels stand at sample counts of their own");
    if (own_first == 0 && own_end == total_spp)
        return fail(KY_ERR_INVALID_VALUE, "merge: the receiving frame owns all %d samples and renders them itself (kyhip_frame_begin_slice: a slice, or a collector)", total_spp);
    for (int i = 0; i < theirs.n; ++i)
        if (theirs.r[2 * i] < own_end && own_first < theirs.r[2 * i + 1])
            return fail(KY_ERR_INVALID_VALUE, "merge: the state holds samples %d..%d, the receiving frame owns %d..%d and would count them twice", theirs.r[2 * i], theirs.r[2 * i + 1],
                        own_first, own_end);
    if (tracks_noise && !has_noise) return fail(KY_ERR_INVALID_VALUE, "merge: the receiving frame tracks noise, the state carries no valid noise trailer");
    return coverage_union(mine, theirs, merged);
}

// ---- the book (ky_frame_book.hpp) ----
int begin_check(const ky_scene* scene, const ky_render_params* p, int first_sample, int end_sample, kyhip_frame** out) {
    if (!valid_params(p)) return fail(KY_ERR_INVALID_VALUE, "invalid render params (integrator %d, direct_sample %d)", p ? p->integrator : -1, p ? p->direct_sample : -1);
    if (!shard_in_range(p)) return fail(KY_ERR_LIMIT, "frame too large for the device's 32-bit work-item and pixel indices (%d x %d, %d spp)", p->width, p->height, p->samples_per_pixel);
    if (film_range_check(p, scene) != KY_OK) return KY_ERR_LIMIT;
    if (!out) return fail(KY_ERR_INVALID_VALUE, "out is NULL");
    *out = nullptr;
    return slice_range_check(p->samples_per_pixel, first_sample, end_sample);
}
void FrameBook::begin(const ky_render_params* p, uint64_t scene_hash, int first_sample, int end_sample) {
    *this = FrameBook();
    params = *p;
    sh = make_shard(p);
    plan = chunk_plan(p->samples_per_pixel);
    own_first = first_sample; own_end = end_sample;
    own_c0 = chunks_at_sample(plan, first_sample); own_c1 = chunks_at_sample(plan, end_sample);
    chunks_done = own_c0;
    header = frame_header(p, scene_hash, 0);
    base_hash = scene_hash;
    retrack();
}
int FrameBook::set_filter(const ky_pixel_filter* f) {
    KY_TRY(filter_check(f));
    if (!untouched()) return fail(KY_ERR_INVALID_VALUE, "the frame holds samples already: its pixel filter is set before the first one is rendered, loaded or merged");
    filter = *f;
    if (filter.kind == KY_FILTER_BOX) filter = ky_pixel_filter{};   // (one box: its radius names nothing)
    header.scene_hash = texture_fold(lens_fold(filter_fold(base_hash, &filter), &lens), tex_digest);
    return KY_OK;
}
int FrameBook::set_lens(const ky_lens* l) {
    KY_TRY(lens_check(l));
    if (!untouched()) return fail(KY_ERR_INVALID_VALUE, "the frame holds samples already: its lens is set before the first one is rendered, loaded or merged");
    lens = *l;
    if (lens_is_pinhole(&lens)) lens = ky_lens{};   // (one pinhole: its focus distance names nothing)
    header.scene_hash = texture_fold(lens_fold(filter_fold(base_hash, &filter), &lens), tex_digest);
    return KY_OK;
}
int FrameBook::set_textures(uint64_t digest) {
    if (!untouched()) return fail(KY_ERR_INVALID_VALUE, "the frame holds samples already: its textures are set before the first sample is rendered, loaded or merged");
    tex_digest = digest;
    header.scene_hash = texture_fold(lens_fold(filter_fold(base_hash, &filter), &lens), tex_digest);
    return KY_OK;
}
// Where a saved state differs from this frame in nothing but the header's scene hash, the refusal names the filter when that can be told: KY_OK otherwise (the
// readers' own checks follow and refuse whatever else is wrong).
int FrameBook::filter_refusal(const void* buf, size_t bytes) const {
    if (!buf || bytes < sizeof(FrameHeader)) return KY_OK;
    FrameHeader theirs;
    std::memcpy(&theirs, buf, sizeof theirs);
    if (theirs.scene_hash == header.scene_hash) return KY_OK;
    FrameHeader same = theirs;
    same.scene_hash = header.scene_hash; same.samples_done = header.samples_done; same.magic = header.magic;
    if (std::memcmp(&same, &header, sizeof header) != 0) return KY_OK;
    if (tex_digest != 0)   // ... and the textures
        return fail(KY_ERR_INVALID_VALUE, "frame state: saved by a frame with other textures or none, another lens or pixel filter (or scene); this frame has a texture set (kyhip_frame_set_textures)");
    if (!lens_is_pinhole(&lens)) {   // ... and the lens
        if (theirs.scene_hash == filter_fold(base_hash, &filter))
            return fail(KY_ERR_INVALID_VALUE, "frame state: saved by a frame of this scene without a lens, this frame has a %s (kyhip_frame_set_lens)", lens_describe(&lens).c_str());
        return fail(KY_ERR_INVALID_VALUE, "frame state: saved by a frame with another lens or pixel filter (or scene), this frame has a %s and a %s (kyhip_frame_set_lens, kyhip_frame_set_filter)",
                    lens_describe(&lens).c_str(), filter_describe(&filter).c_str());
    }
    if (filter_is_box(&filter)) return KY_OK;   // (another scene, or a filter or lens this frame does not have: the header check says so)
    if (theirs.scene_hash == base_hash)
        return fail(KY_ERR_INVALID_VALUE, "frame state: saved by a frame of this scene with the box filter, this frame has a %s (kyhip_frame_set_filter)", filter_describe(&filter).c_str());
    return fail(KY_ERR_INVALID_VALUE, "frame state: saved by a frame with another pixel filter, a lens (or another scene), this frame has a %s and no lens (kyhip_frame_set_filter, kyhip_frame_set_lens)", filter_describe(&filter).c_str());
}
int FrameBook::load_check(const void* buf, size_t bytes, CheckpointCounts* out) const {
    KY_TRY(filter_refusal(buf, bytes));
    return checkpoint_check(header, layout, buf, bytes, out);
}
int FrameBook::tracks(bool want_blocks, bool want_noise) const {
    if (want_blocks && !blocks.on) return fail(KY_ERR_INVALID_VALUE, "the frame does not track blocks (kyhip_frame_track_blocks)");
    if (want_noise && !noise.on) return fail(KY_ERR_INVALID_VALUE, "the frame does not track noise (kyhip_frame_track_noise)");
    return KY_OK;
}
int FrameBook::coverage(int* ranges2, int n, int own[2]) const {
    if (n > 0 && !ranges2) return fail(KY_ERR_INVALID_VALUE, "ranges2 is NULL");
    for (int i = 0; i < 2 * cov.n && i < 2 * n; ++i) ranges2[i] = cov.r[i];
    if (own) { own[0] = own_first; own[1] = own_end; }
    return cov.n;
}

int FrameBook::next_pass(int min_samples, PassStep* out) const {
    if (min_samples < 1) return fail(KY_ERR_INVALID_VALUE, "min_samples %d: a pass renders at least one sample per pixel", min_samples);
    PassStep s;
    s.chunk_first = chunks_done;
    int c1 = pass_chunk_end(plan, chunks_done, min_samples);
    if (c1 > own_c1) c1 = own_c1;   // (a slice ends where its owned range does)
    if (!nothing_live() && c1 > chunks_done) {   // (every block retired: nothing is launched and the front stays)
        // what the frame holds behind the pass: its front moves, and the estimate's batch is the samples the pass adds to the held ones
        Coverage pass_range;
        pass_range.n = 1; pass_range.r[0] = front(); pass_range.r[1] = chunk_end(plan, c1 - 1);
        KY_TRY(coverage_union(cov, pass_range, &s.held_then));
        s.chunk_count = c1 - chunks_done;
        s.n_prev = noise.n_prev; s.n_now = s.held_then.held();
        s.launch = sh.n_pix > 0;
    }
    *out = s;
    return KY_OK;
}
// (behind the pass's synchronisation: a failed pass is not counted)
void FrameBook::commit_pass(const PassStep& s) {
    if (s.chunk_count == 0) return;
    if (noise.on) { noise.batches += 1; noise.n_prev = s.n_now; }
    if (blocks.on) blocks.passes += 1;
    cov = s.held_then;
    chunks_done = s.chunk_first + s.chunk_count;
}

int FrameBook::can_track_noise() const {
    if (!untouched()) return fail(KY_ERR_INVALID_VALUE, "noise is tracked from a frame's first pass: this one has rendered, loaded or merged something");
    return KY_OK;
}
void FrameBook::track_noise() {
    noise.on = true;
    retrack();
}
int FrameBook::can_track_blocks() const {
    if (layout.sliced)
        return fail(KY_ERR_INVALID_VALUE, "the frame owns samples %d..%d of %d: blocks retire on a frame that owns them all (per-block sample counts across slices are not kept)",
                    own_first, own_end, params.samples_per_pixel);
    if (!untouched()) return fail(KY_ERR_INVALID_VALUE, "blocks are tracked from a frame's first pass: this one has rendered or loaded something");
    return KY_OK;
}
void FrameBook::size_blocks() {
    blocks.host.assign((size_t)sh.n_blocks, kyb::BlockState{-1, 0});
    blocks.inside.assign((size_t)sh.n_blocks, 0);
    for (int i = 0; i < sh.n_pix; ++i)
        if (kyb::pixel_inside(sh, i, params.width, params.height)) blocks.inside[(size_t)kyb::block_of_pixel(sh, i)] += 1;
}
void FrameBook::track_blocks() {
    blocks.on = true;
    retrack();   // (the checkpoints' magic changes with the layout: plain frames refuse this one's states and it theirs)
}
int FrameBook::blocks_home(int n_live) {
    if (n_live < 0 || n_live > sh.n_blocks) return fail(KY_ERR_DEVICE, "internal: %d live blocks of %d", n_live, sh.n_blocks);
    blocks.n_live = n_live;
    return KY_OK;
}

int FrameBook::resolve(int normalise, const float* film_rgb, size_t stride_px, ResolveStep* out) const {
    if (normalise != 0 && normalise != 1) return fail(KY_ERR_INVALID_VALUE, "normalise %d: 0 (sum / total) or 1 (sum / done)", normalise);
    if (!film_rgb || stride_px < (size_t)params.width) return fail(KY_ERR_INVALID_VALUE, "bad film arguments");
    const int spp = params.samples_per_pixel;
    if (blocks.on && !normalise)
        for (size_t b = 0; b < blocks.host.size(); ++b)
            if (blocks.inside[b] > 0 && blocks.host[b].retired_at >= 0 && blocks.host[b].retired_at < spp)
                return fail(KY_ERR_INVALID_VALUE, "normalise 0 on a frame with blocks retired short of its %d samples (block %zu at %d): sum / total would darken them; normalise 1",
                            spp, b, blocks.host[b].retired_at);
    ResolveStep s;
    s.held = held();
    s.nothing = sh.n_pix == 0 || (normalise && s.held == 0);
    if (!s.nothing) {
        s.scale = normalise ? (double)spp / (double)s.held : 1.0;
        s.per_block = blocks.on && normalise;
    }
    *out = s;
    return KY_OK;
}
int FrameBook::denoise_check(bool needs_variance) const {
    KY_TRY(tracks(false, true));
    if (params.tile_first != 0 || params.tile_step != 1)
        return fail(KY_ERR_INVALID_VALUE, "the frame's shard (tile_first %d, tile_step %d) is not the whole film: a shard's neighbours live elsewhere", params.tile_first, params.tile_step);
    if (needs_variance && noise.batches < 2) return fail(KY_ERR_INVALID_VALUE, "%d noise batches: the filter needs a variance, two passes or more", noise.batches);
    return KY_OK;
}

int FrameBook::temporal_check(int device, int albedo_grid, int hist_device, int hist_width, int hist_height, int hist_albedo) const {
    KY_TRY(denoise_check(true));
    if (blocks.on) return fail(KY_ERR_INVALID_VALUE, "the frame tracks blocks: a history holds one sample count per pixel, not per block");
    if (hist_device != device) return fail(KY_ERR_INVALID_VALUE, "the history lives on device %d, the frame on device %d", hist_device, device);
    if (hist_width != params.width || hist_height != params.height)
        return fail(KY_ERR_INVALID_VALUE, "the history is %d x %d, the frame %d x %d", hist_width, hist_height, params.width, params.height);
    if (hist_albedo >= 0 && hist_albedo != (albedo_grid > 0 ? 1 : 0))
        return fail(KY_ERR_INVALID_VALUE, "the history holds %s colours, the frame's albedo grid is %d: reset the history or keep the mode",
                    hist_albedo ? "albedo-demodulated" : "plain", albedo_grid);
    return KY_OK;
}

int FrameBook::save_host(void* buf, size_t bytes) const {
    if (!buf || bytes < layout.total) return fail(KY_ERR_INVALID_VALUE, "frame state: a buffer of %zu bytes, the state has %zu", bytes, layout.total);
    CheckpointCounts n;
    n.samples_done = held();
    n.front = front(); n.cov = cov;
    n.batches = noise.batches; n.n_prev = noise.n_prev; n.passes = blocks.passes;
    checkpoint_write_host(header, layout, n, blocks.host.data(), buf);   // (the host's block states are current: every call that changes the device's brings them home)
    return KY_OK;
}
// (behind the copies of the state's device parts, and behind blocks_home for the block states among them)
void FrameBook::commit_load(const CheckpointCounts& n) {
    if (noise.on) { noise.batches = n.batches; noise.n_prev = n.n_prev; }
    if (blocks.on) blocks.passes = n.passes;
    chunks_done = n.chunks_done;
    cov = n.cov;
    loaded = true;
}

int FrameBook::merge_state(const void* state, size_t bytes, MergeStep* out) const {
    MergeSource m;
    KY_TRY(filter_refusal(state, bytes));
    KY_TRY(merge_source_check(header, state, bytes, &m));
    MergeStep s;
    KY_TRY(merge_accept(cov, own_first, own_end, params.samples_per_pixel, noise.on, blocks.on, m.cov, m.noise_pixels != 0, &s.merged));
    s.accum = m.accum; s.noise_pixels = m.noise_pixels;
    s.n_mine = held(); s.n_src = m.cov.held(); s.src_batches = m.batches;
    *out = s;
    return KY_OK;
}
int FrameBook::merge_book(const FrameBook& src, MergeStep* out) const {
    if (this == &src) return fail(KY_ERR_INVALID_VALUE, "merge: a frame holds its own samples already");
    if (std::memcmp(&header, &src.header, sizeof header) != 0) {
        if (tex_digest != src.tex_digest)
            return fail(KY_ERR_INVALID_VALUE, "merge: the frames differ in their textures (kyhip_frame_set_textures)");
        if (std::memcmp(&lens, &src.lens, sizeof lens) != 0)
            return fail(KY_ERR_INVALID_VALUE, "merge: the frames differ in their lens (this one: %s, the other: %s)", lens_describe(&lens).c_str(), lens_describe(&src.lens).c_str());
        if (std::memcmp(&filter, &src.filter, sizeof filter) != 0)
            return fail(KY_ERR_INVALID_VALUE, "merge: the frames differ in their pixel filter (this one: %s, the other: %s)", filter_describe(&filter).c_str(), filter_describe(&src.filter).c_str());
        return fail(KY_ERR_INVALID_VALUE, "merge: the frames differ in their render params, scene or film size");
    }
    if (src.blocks.on) return fail(KY_ERR_INVALID_VALUE, "merge: the other frame retires pixel blocks: its pixels stand at sample counts of their own and merge with nothing");
    MergeStep s;
    KY_TRY(merge_accept(cov, own_first, own_end, params.samples_per_pixel, noise.on, blocks.on, src.cov, src.noise.on, &s.merged));
    s.n_mine = held(); s.n_src = src.held(); s.src_batches = src.noise.batches;
    *out = s;
    return KY_OK;
}
// (behind the merge kernel's synchronisation: a failed merge is not counted)
void FrameBook::commit_merge(const MergeStep& s) {
    if (noise.on) { noise.batches += s.src_batches; noise.n_prev = s.merged.held(); }
    cov = s.merged;
}

void FrameBook::block_stats(ky_block_stats* out) const {
    std::memset(out, 0, sizeof *out);
    const int at = front();
    out->blocks = sh.n_blocks;
    out->live = blocks.n_live;
    out->passes = blocks.passes;
    out->samples_done = at;
    bool any = false;
    for (size_t i = 0; i < blocks.host.size(); ++i) {
        if (blocks.inside[i] == 0) continue;
        const int n = kyb::block_samples(blocks.host[i], at);
        out->pixels += blocks.inside[i];
        out->pixel_samples += (int64_t)blocks.inside[i] * n;
        if (!any || n < out->min_samples) out->min_samples = n;
        if (!any || n > out->max_samples) out->max_samples = n;
        any = true;
    }
}
int FrameBook::sample_map(int32_t* map, size_t stride_px) const {
    KY_TRY(tracks(true, false));
    if (!map || stride_px < (size_t)params.width) return fail(KY_ERR_INVALID_VALUE, "bad map arguments");
    const int at = front();
    for (int i = 0; i < sh.n_pix; ++i) {
        int x, y;
        if (!kyb::pixel_inside(sh, i, params.width, params.height, &x, &y)) continue;
        map[(size_t)y * stride_px + (size_t)x] = kyb::block_samples(blocks.host[(size_t)kyb::block_of_pixel(sh, i)], at);
    }
    return KY_OK;
}
bool FrameBook::until_stops(const ky_noise_stats& s, float max_fraction_above, int min_batches) const {
    const bool clean = s.batches >= min_batches && (double)s.above <= (double)max_fraction_above * (double)(s.pixels - s.flagged);
    // (a block-tracking frame without a live block renders no further: its front and its map stay what they are, and so would this verdict)
    return clean || owned_rendered() || nothing_live();
}
}  // namespace kyh

// the pieces of checkpoint_check: the noise trailer at `state_bytes` (CheckpointLayout::noise) ...
int kyn::noise_trailer_check(const void* buf, size_t bytes, size_t state_bytes, int n_pix, int samples_done, NoiseTrailer* out) {
    using kyh::fail;
    if (!buf || bytes < state_bytes || bytes - state_bytes < noise_trailer_bytes(n_pix))
        return fail(KY_ERR_INVALID_VALUE, "frame state: %zu bytes hold no noise trailer (the state of a frame that tracks noise has %zu)", bytes, state_bytes + noise_trailer_bytes(n_pix));
    NoiseTrailer t;
    std::memcpy(&t, (const char*)buf + state_bytes, sizeof t);
    if (t.magic != KY_NOISE_MAGIC) return fail(KY_ERR_INVALID_VALUE, "frame state: no noise trailer behind the accumulators (saved by a frame that does not track noise?)");
    if (t.batches < 0 || t.n_prev != samples_done)
        return fail(KY_ERR_INVALID_VALUE, "frame state: the noise estimate stands at %d samples in %d batches, the accumulators at %d", t.n_prev, t.batches, samples_done);
    if (out) *out = t;
    return KY_OK;
}
// ... and the block trailer at `offset` (CheckpointLayout::blocks)
int kyb::block_trailer_check(const void* buf, size_t bytes, size_t offset, int n_blocks, int total_spp, int samples_done, int noise_batches, BlockTrailer* out) {
    using kyh::fail;
    if (!buf || bytes < offset || bytes - offset < block_trailer_bytes(n_blocks))
        return fail(KY_ERR_INVALID_VALUE, "frame state: %zu bytes hold no block trailer (the state of this frame has %zu)", bytes, offset + block_trailer_bytes(n_blocks));
    BlockTrailer t;
    std::memcpy(&t, (const char*)buf + offset, sizeof t);
    if (t.magic != KY_BLOCKS_MAGIC) return fail(KY_ERR_INVALID_VALUE, "frame state: no block trailer where this frame's state has one");
    if (t.n_blocks != n_blocks) return fail(KY_ERR_INVALID_VALUE, "frame state: the block trailer counts %d blocks, the frame has %d", t.n_blocks, n_blocks);
    if (t.passes < 0) return fail(KY_ERR_INVALID_VALUE, "frame state: the block trailer counts %d passes", t.passes);
    const ChunkPlan plan = chunk_plan(total_spp);
    for (int b = 0; b < n_blocks; ++b) {
        BlockState s;
        std::memcpy(&s, (const char*)buf + offset + sizeof t + (size_t)b * sizeof s, sizeof s);
        // (a block's batch count is the frame's when it retired: at most the noise trailer's, and 0 where nothing was rendered yet and for a live block)
        if (s.batches < 0 || s.batches > noise_batches || (s.retired_at <= 0 && s.batches != 0))
            return fail(KY_ERR_INVALID_VALUE, "frame state: block %d (retired at %d) has %d batches, the noise estimate %d", b, s.retired_at, s.batches, noise_batches);
        if (s.retired_at == -1) continue;
        if (s.retired_at < 0 || s.retired_at > samples_done || chunks_at_sample(plan, s.retired_at) < 0)
            return fail(KY_ERR_INVALID_VALUE, "frame state: block %d retired at %d samples: no pass of a %d-sample frame that stands at %d ends there", b, s.retired_at,
                        total_spp, samples_done);
    }
    if (out) *out = t;
    return KY_OK;
}

extern "C" {
int kyhip_pass_boundaries(int spp, int* bounds, int n) { return kyh::pass_boundaries(spp, bounds, n); }
int kyhip_slice_bounds(int spp, int n_slices, int* bounds) { return kyh::slice_bounds(spp, n_slices, bounds); }
}
