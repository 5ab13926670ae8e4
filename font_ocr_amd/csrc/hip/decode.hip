// decode.hip — the `focr` line decoder on the device (include/focr_decode.h; decode_image / decode_line, src/main.rs:112-218).
//
// A batch of equal-size pages runs in three launches, whatever its line count:
//   1. line_prepass_kernel: one workgroup per (page, line) slot crops the line as the image crate does, inverts it
//      (r = 255 - luma) into a zero-padded strip and flags it non-blank (an empty crop counts as all-white);
//   2. line_compact_kernel: one workgroup turns the flags into the work list of non-blank slots, in (page, line) order;
//   3. line_decode_kernel: one wave per work-list line runs the reference's pen loop.  The pen and the step count are
//      uniform across the wave; each lane scores its glyphs (lane, lane + 64, ...) against the strip (LDS when it fits)
//      from the glyph's phase tile, then a wave argmin takes the lowest (score, glyph index).  With scores on
//      (focr_decoder_set_scores) the same launch also keeps the second lowest key and sums r^2 over the line's crop.
//      With a pen search radius (focr_decoder_set_pen_search) line_search_kernel takes its place: one workgroup per line,
//      the argmin over (glyph, pen offset), and the chosen offset of every step beside its glyph.
//      With the whole-line decode on (focr_decoder_set_whole_line) one of decode_whole.hip's kernels takes its place: a
//      dynamic programme over pens in 1/64 px, with margins or with a pen slack when those are on.
//      With a baseline search radius (focr_decoder_set_baseline_search) decode_baseline.hip's line_baseline_kernel takes its
//      place: the pen loop under every vertical candidate, and the candidate with the lowest summed footprint term.
//      With the whole-line decode on and a radius of its own (focr_decoder_set_whole_baseline)
//      decode_whole_baseline.hip's line_whole_baseline_kernel takes its place: the programme under every candidate.
//      With the font search on (focr_decoder_set_font_search, over the candidates of focr_decoder_set_font_candidates)
//      decode_fonts.hip's line_fonts_kernel takes its place, or beside the whole-line decode decode_whole_fonts.hip's
//      line_whole_fonts_kernel: the pen loop, or the programme, under every candidate font, and the cheapest line kept.
//      On a fractional line grid (focr_decoder_set_line_frac; the two baseline modes only) launch 1 is
//      line_prepass_frac_kernel: the slot grid in 1/64 px (decode.h).  Launch 3 of a baseline search is the same
//      line_baseline_kernel on either grid (it takes the grid as an argument, (0, 0) when it is off); the whole-line decode
//      under candidates launches line_whole_baseline_frac_kernel on the fractional grid.
// The reference scores sum over the canvas of (r - c)^2; that is sum r^2 + sum over the clipped glyph footprint of
// c * (c - 2r), and sum r^2 is the same for every candidate, so the footprint term alone decides the argmin, ties
// included.  It is exact integer arithmetic (v_dot4_u32_u8; the font builder bounds it below 2^31), so neither the
// order of the sums nor the device changes a choice.  The pen update is one f32 add of the host-computed increment.
//
// Which of these a run launches is decided once, by resolve_modes below: the settings become one RunMode (decode.h), with
// every refusal of a combination, and the run's steps (line_cap, reserve, launch, collect) read that and nothing else.
//
// The verify and --test images of a batch are decode_images.hip's; decode.h holds what the decoder's files share, and
// decode_line.h what this file shares with decode_whole.hip, decode_baseline.hip and decode_whole_baseline.hip.
#include <cmath>
#include <cstring>

#include "decode_line.h"

namespace focr_dec {

constexpr uint32_t PREPASS_THREADS = 256;
constexpr uint32_t COMPACT_THREADS = 1024;

// The prepass of one slot on a line grid (decode.h: the whole-pixel one, or the fractional one of focr_decoder_set_line_frac).
template <class Grid>
__device__ __forceinline__ void prepass_slot(const uint8_t *__restrict__ pages, const Geometry &g, const Grid &grid, uint8_t *__restrict__ strips,
                                             uint32_t *__restrict__ flags) {
    const uint32_t slot = blockIdx.x;
    uint32_t yc, h;
    int centre;
    grid.rows(g, slot % g.n_slots, 0, &yc, &h, &centre);
    const uint8_t *src = pages + (size_t)(slot / g.n_slots) * g.page_w * g.page_h + (size_t)yc * g.page_w + g.x;  // slot_crop
    uint8_t *dst = strips + (size_t)slot * g.stride * g.line_height;
    int ink = 0;
    const uint32_t n = g.stride * h;
    for (uint32_t k = threadIdx.x; k < n; k += PREPASS_THREADS) {
        const uint32_t row = k / g.stride;
        const int col = (int)(k % g.stride) - (int)PAD;
        uint8_t v = 0;
        if (col >= 0 && (uint32_t)col < g.w) {
            const uint8_t l = src[(size_t)row * g.page_w + col];
            v = 255 - l;
            ink |= l != 255;
        }
        dst[k] = v;
    }
    ink = __syncthreads_or(ink);
    if (threadIdx.x == 0) flags[slot] = ink ? 1u : 0u;
}

// 1. crop + invert + blank flag, one workgroup per slot
__global__ __launch_bounds__(PREPASS_THREADS) void line_prepass_kernel(const uint8_t *__restrict__ pages, Geometry g,
                                                                       uint8_t *__restrict__ strips, uint32_t *__restrict__ flags) {
    prepass_slot(pages, g, PixelGrid{}, strips, flags);
}

// 1f. ... on the fractional line grid: a kernel of its own, so that the plain prepass keeps its arguments and its
// instruction stream (tools/isa_hash.py)
__global__ __launch_bounds__(PREPASS_THREADS) void line_prepass_frac_kernel(const uint8_t *__restrict__ pages, Geometry g, LineFrac fr,
                                                                            uint8_t *__restrict__ strips, uint32_t *__restrict__ flags) {
    prepass_slot(pages, g, FracGrid{fr}, strips, flags);
}

// 2. order-preserving compaction of the non-blank slots, one workgroup
__global__ __launch_bounds__(COMPACT_THREADS) void line_compact_kernel(const uint32_t *__restrict__ flags, uint32_t total,
                                                                       uint32_t *__restrict__ work, uint32_t *__restrict__ count) {
    __shared__ uint32_t wave_sum[COMPACT_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t base = 0;
    for (uint32_t start = 0; start < total; start += COMPACT_THREADS) {
        const uint32_t s = start + threadIdx.x;
        const bool live = s < total && flags[s] != 0;
        const uint64_t m = __ballot(live);
        if (lane == 0) wave_sum[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < COMPACT_THREADS / 64; w++) {
            before += w < wave ? wave_sum[w] : 0;
            all += wave_sum[w];
        }
        if (live) work[base + before + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = s;
        base += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}

// The wave's sum of every lane's v, in every lane.
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

__device__ __forceinline__ int key_term(uint64_t key) { return (int)((uint32_t)(key >> 32) ^ 0x80000000u); }

// What line_decode_kernel<.., true> writes beside chars: per step (the layout of chars) the footprint terms of the
// chosen glyph and of the runner-up and the runner-up's index; per work-list line the sum of r^2 over its crop.
struct ScoreOut {
    int32_t *term, *runner_term;
    uint16_t *runner;
    uint64_t *base;
};

// 3. the pen loop, one wave per work-list line.  SCORES: also the runner-up of every step (the second lowest key;
// keys carry the glyph index, so they are distinct and a top-2 merge is exact) and the line's sum of r^2.
template <bool LDS, bool SCORES>
__global__ __launch_bounds__(64) void line_decode_kernel(const uint8_t *__restrict__ strips, Geometry g, const uint32_t *__restrict__ work,
                                                         const uint32_t *__restrict__ count, const DevGlyph *__restrict__ glyphs,
                                                         const int2 *__restrict__ offs, const uint32_t *__restrict__ bitmaps,
                                                         uint32_t n_glyphs, float origin_x, uint32_t *__restrict__ n_chars,
                                                         uint16_t *__restrict__ chars, ScoreOut so) {
    extern __shared__ uint32_t lds_strip[];
    const uint32_t k = blockIdx.x;
    if (k >= *count) return;
    const uint32_t slot = work[k];
    uint32_t yc, h;
    slot_rows(g, slot % g.n_slots, &yc, &h);
    const uint32_t *strip = (const uint32_t *)(strips + (size_t)slot * g.stride * g.line_height);
    const uint32_t sdw = g.stride / 4;
    if (LDS) {
        for (uint32_t q = threadIdx.x; q < sdw * h; q += 64) lds_strip[q] = strip[q];
        __syncthreads();
        strip = lds_strip;
    }
    const uint32_t lane = threadIdx.x;
    const int w = (int)g.w;
    const float fw = (float)g.w;
    uint16_t *out = chars + (size_t)k * g.cap;
    if (SCORES) {  // the rows below h hold nothing of this line, and a row's pad bytes are zero: whole rows of the crop
        uint64_t acc = 0;
        for (uint32_t q = lane; q < sdw * h; q += 64) acc += __builtin_amdgcn_udot4(strip[q], strip[q], 0u, false);
        acc = wave_sum_u64(acc);
        if (lane == 0) so.base[k] = acc;
    }
    float pos = 0.f;
    uint32_t n = 0;
    while (pos < fw && n < g.cap) {
        const int d = (int)((origin_x + pos) * 64.0f);  // FreeType's delta: trunc(t * 64)
        const int phase = d & 63, shift = d >> 6;
        uint64_t best = ~0ull, second = ~0ull;  // second: SCORES only
        for (uint32_t gi = lane; gi < n_glyphs; gi += 64) {
            const DevGlyph gl = glyphs[gi];
            const int2 o = offs[gi * 64 + phase];
            const int x0 = shift + o.x, y0 = o.y;
            const uint32_t *tile = bitmaps + gl.off_dw + (uint32_t)phase * gl.ndw * gl.box_h;
            const int r_lo = std::max(0, -y0), r_hi = std::min((int)gl.box_h, (int)h - y0);
            uint32_t cc = 0, cr = 0;
            for (int r = r_lo; r < r_hi; r++) {
                const uint32_t *srow = strip + (size_t)(y0 + r) * sdw;
                const uint32_t *trow = tile + (size_t)r * gl.ndw;
                for (uint32_t q = 0; q < gl.ndw; q++) {
                    const int base = x0 + 4 * (int)q;
                    if (base <= -4 || base >= w) continue;
                    uint32_t c = trow[q];
                    if (base < 0 || base + 4 > w) c &= edge_mask(base, w);
                    const uint32_t a = (uint32_t)(base + (int)PAD);
                    const uint32_t rv = __builtin_amdgcn_alignbyte(srow[(a >> 2) + 1], srow[a >> 2], a & 3);
                    cr = __builtin_amdgcn_udot4(c, rv, cr, false);
                    cc = __builtin_amdgcn_udot4(c, c, cc, false);
                }
            }
            const int score = (int)cc - 2 * (int)cr;
            const uint64_t key = ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | gi;  // (score, index), lowest first
            if (SCORES) second = std::min(second, std::max(best, key));
            best = std::min(best, key);
        }
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t lo = __shfl_xor((uint32_t)best, m, 64), hi = __shfl_xor((uint32_t)(best >> 32), m, 64);
            const uint64_t p1 = ((uint64_t)hi << 32) | lo;
            if (SCORES) {
                const uint32_t lo2 = __shfl_xor((uint32_t)second, m, 64), hi2 = __shfl_xor((uint32_t)(second >> 32), m, 64);
                second = std::min(std::max(best, p1), std::min(second, ((uint64_t)hi2 << 32) | lo2));
            }
            best = std::min(best, p1);
        }
        const uint32_t gbest = (uint32_t)best;
        if (lane == 0) out[n] = (uint16_t)gbest;
        if (SCORES && lane == 0) {  // no runner-up (one glyph): the key stays ~0, whose index reads 0xffff
            const size_t at = (size_t)k * g.cap + n;
            so.term[at] = key_term(best);
            so.runner_term[at] = key_term(second);
            so.runner[at] = (uint16_t)second;
        }
        n++;
        pos = __fadd_rn(pos, glyphs[gbest].inc);
    }
    if (lane == 0) n_chars[k] = n;
}

// ---- pen search (focr_decoder_set_pen_search; an extension, see include/focr_decode.h) ------------------------------

constexpr uint32_t SEARCH_THREADS = 256;    // one workgroup of four waves per work-list line
constexpr uint32_t SEARCH_WAVES = SEARCH_THREADS / 64;
constexpr uint32_t SEARCH_RED_BYTES = 2 * SEARCH_WAVES * 2 * 8;  // two parities of (best, other) per wave, behind the strip

// A search key: (score, rank of the offset, glyph index), lowest first (rank_offset, decode_line.h).
__device__ __forceinline__ uint32_t key_glyph(uint64_t key) { return (uint32_t)key & 0xffffu; }

// The minimum of two sets of keys, and the minimum of those of their keys whose glyph is not the minimum's.  Each set
// comes as (best, other): its lowest key, and its lowest key of another glyph than best's (~0: none).  The winner's
// other already leaves out the winner's glyph; of the loser's set, its best is the lowest of all and counts when its
// glyph differs, else its other does, which leaves out exactly that glyph.  So the merge is exact in any order.
__device__ __forceinline__ void merge_other_glyph(uint64_t &best, uint64_t &other, uint64_t b2, uint64_t o2) {
    const bool keep = best <= b2;
    const uint64_t win = keep ? best : b2, lose = keep ? b2 : best;
    const uint64_t o_win = keep ? other : o2, o_lose = keep ? o2 : other;
    other = std::min(o_win, key_glyph(lose) != key_glyph(win) ? lose : o_lose);  // an empty set's ~0 names no glyph
    best = win;
}

// 3s. the pen loop with a search over (glyph, pen offset), one workgroup per work-list line.  The candidates of a step,
// n_glyphs * (2 * radius + 1) of them, are flattened glyph-major over the 256 lanes (the offsets of one glyph share its
// box, so neighbouring lanes run the same trip counts); every lane keeps the (best, other-glyph) pair of its own, a wave
// merges by shuffles, and the four waves meet in LDS: one barrier per step, the pairs double-buffered by the step's
// parity (a wave that writes step n + 2 has passed the barrier of step n + 1, which every wave reaches only after it
// has read step n).  Pen, step count and choice are uniform across the workgroup.  radius >= 1.
template <bool LDS, bool SCORES>
__global__ __launch_bounds__(SEARCH_THREADS) void line_search_kernel(const uint8_t *__restrict__ strips, Geometry g, const uint32_t *__restrict__ work,
                                                                     const uint32_t *__restrict__ count, const DevGlyph *__restrict__ glyphs,
                                                                     const int2 *__restrict__ offs, const uint32_t *__restrict__ bitmaps,
                                                                     uint32_t n_glyphs, float origin_x, uint32_t radius, uint32_t *__restrict__ n_chars,
                                                                     uint16_t *__restrict__ chars, int8_t *__restrict__ pen_offs, ScoreOut so) {
    extern __shared__ uint32_t lds_search[];  // the reduction pairs, then (LDS) the strip
    uint64_t *red = (uint64_t *)lds_search;
    const uint32_t k = blockIdx.x;
    if (k >= *count) return;
    const uint32_t slot = work[k];
    uint32_t yc, h;
    slot_rows(g, slot % g.n_slots, &yc, &h);
    const uint32_t *strip = (const uint32_t *)(strips + (size_t)slot * g.stride * g.line_height);
    const uint32_t sdw = g.stride / 4;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (LDS) {
        uint32_t *lds_strip = lds_search + SEARCH_RED_BYTES / 4;
        for (uint32_t q = tid; q < sdw * h; q += SEARCH_THREADS) lds_strip[q] = strip[q];
        __syncthreads();
        strip = lds_strip;
    }
    const int w = (int)g.w;
    const float fw = (float)g.w;
    const size_t row = (size_t)k * g.cap;
    if (SCORES) {  // as in line_decode_kernel: whole rows of the crop
        uint64_t acc = 0;
        for (uint32_t q = tid; q < sdw * h; q += SEARCH_THREADS) acc += __builtin_amdgcn_udot4(strip[q], strip[q], 0u, false);
        acc = wave_sum_u64(acc);
        if (lane == 0) red[wave] = acc;
        __syncthreads();
        if (tid == 0) {
            uint64_t total = 0;
            for (uint32_t v = 0; v < SEARCH_WAVES; v++) total += red[v];
            so.base[k] = total;
        }
        __syncthreads();
    }
    const uint32_t n_off = 2 * radius + 1, n_cand = n_glyphs * n_off;
    float pos = 0.f;
    uint32_t n = 0;
    while (pos < fw && n < g.cap) {
        uint64_t best = ~0ull, other = ~0ull;  // other: SCORES only
        for (uint32_t c = tid; c < n_cand; c += SEARCH_THREADS) {
            const uint32_t gi = c / n_off, rank = c - gi * n_off;
            const float t = __fadd_rn(origin_x, __fadd_rn(pos, (float)rank_offset(rank) * 0.015625f));
            if (t < 0.f) continue;  // left of the line's first delta: no such rendering in the reference
            const int d = (int)__fmul_rn(t, 64.0f);  // FreeType's delta: trunc(t * 64)
            const int phase = d & 63, shift = d >> 6;
            const DevGlyph gl = glyphs[gi];
            const int2 o = offs[gi * 64 + phase];
            const int x0 = shift + o.x, y0 = o.y;
            const uint32_t *tile = bitmaps + gl.off_dw + (uint32_t)phase * gl.ndw * gl.box_h;
            const int r_lo = std::max(0, -y0), r_hi = std::min((int)gl.box_h, (int)h - y0);
            uint32_t cc = 0, cr = 0;
            for (int r = r_lo; r < r_hi; r++) {
                const uint32_t *srow = strip + (size_t)(y0 + r) * sdw;
                const uint32_t *trow = tile + (size_t)r * gl.ndw;
                for (uint32_t q = 0; q < gl.ndw; q++) {
                    const int base = x0 + 4 * (int)q;
                    if (base <= -4 || base >= w) continue;
                    uint32_t cv = trow[q];
                    if (base < 0 || base + 4 > w) cv &= edge_mask(base, w);
                    const uint32_t a = (uint32_t)(base + (int)PAD);
                    const uint32_t rv = __builtin_amdgcn_alignbyte(srow[(a >> 2) + 1], srow[a >> 2], a & 3);
                    cr = __builtin_amdgcn_udot4(cv, rv, cr, false);
                    cc = __builtin_amdgcn_udot4(cv, cv, cc, false);
                }
            }
            const int score = (int)cc - 2 * (int)cr;
            const uint64_t key = ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | (rank << 16) | gi;
            if (SCORES) merge_other_glyph(best, other, key, ~0ull);
            else best = std::min(best, key);
        }
        for (int m = 32; m >= 1; m >>= 1) {
            const uint64_t b2 = shfl_xor_u64(best, m);
            if (SCORES) merge_other_glyph(best, other, b2, shfl_xor_u64(other, m));
            else best = std::min(best, b2);
        }
        uint64_t *slot_red = red + (n & 1) * 2 * SEARCH_WAVES;
        if (lane == 0) {
            slot_red[2 * wave] = best;
            if (SCORES) slot_red[2 * wave + 1] = other;
        }
        __syncthreads();
        best = slot_red[0];
        if (SCORES) other = slot_red[1];
        for (uint32_t v = 1; v < SEARCH_WAVES; v++) {
            if (SCORES) merge_other_glyph(best, other, slot_red[2 * v], slot_red[2 * v + 1]);
            else best = std::min(best, slot_red[2 * v]);
        }
        if (best == ~0ull) break;  // every candidate dropped (a caller-built font with origin_x < 0): the line ends here; uniform
        const uint32_t gbest = key_glyph(best);
        const int j = rank_offset(((uint32_t)best >> 16) & 0xffu);
        if (tid == 0) {
            chars[row + n] = (uint16_t)gbest;
            pen_offs[row + n] = (int8_t)j;
            if (SCORES) {  // no other glyph (a one-glyph alphabet): the key stays ~0, and the host says so
                so.term[row + n] = key_term(best);
                so.runner_term[row + n] = key_term(other);
                so.runner[row + n] = (uint16_t)key_glyph(other);
            }
        }
        n++;
        pos = __fadd_rn(__fadd_rn(pos, (float)j * 0.015625f), glyphs[gbest].inc);  // the chosen candidate's pen, then its increment
    }
    if (tid == 0) n_chars[k] = n;
}

}  // namespace focr_dec

using namespace focr_dec;

extern "C" int focr_decoder_create(int device, focr_decoder_t **out) {
    focr_decoder *dec = nullptr;
    if (!out) return dfail(nullptr, "focr_decoder_create: null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return dfail(nullptr, "no HIP device available (the focr decoder has no CPU fallback)");
    if (device < 0 || device >= n) return dfail(nullptr, "focr_decoder_create: device index out of range");
    DEC_CHECK(hipSetDevice(device));
    dec = new focr_decoder;
    dec->device = device;
    bool ok = hipStreamCreateWithFlags(&dec->stream, hipStreamNonBlocking) == hipSuccess;
    for (Stage *s : {&dec->run, &dec->verify, &dec->test, &dec->vtext, &dec->stext, &dec->atext, &dec->ltext, &dec->rtext}) ok = ok && hipEventCreate(&s->begin) == hipSuccess && hipEventCreate(&s->end) == hipSuccess;
    if (!ok) {
        focr_decoder_destroy(dec);
        return dfail(nullptr, "focr_decoder_create: stream / event creation failed");
    }
    *out = dec;
    return 0;
}

extern "C" void focr_decoder_destroy(focr_decoder_t *dec) {
    if (!dec) return;
    (void)hipSetDevice(dec->device);
    if (dec->stream) (void)hipStreamSynchronize(dec->stream);
    for (const Stage &s : {dec->run, dec->verify, dec->test, dec->vtext, dec->stext, dec->atext, dec->ltext, dec->rtext})
        for (hipEvent_t e : {s.begin, s.end})
            if (e) (void)hipEventDestroy(e);
    if (dec->stream) (void)hipStreamDestroy(dec->stream);
    delete dec;  // every device array of the decoder dies here, behind the wait above
}

extern "C" const char *focr_decoder_last_error(const focr_decoder_t *dec) { return dec ? dec->err.c_str() : g_dec_err.c_str(); }

extern "C" int focr_decoder_set_font(focr_decoder_t *dec, const focr_decode_font_t *font) {
    if (dec) {  // the last run, the verify table, the y-phase fonts and the candidates belong to the previous font, whatever becomes of this one
        DEC_CHECK(hipSetDevice(dec->device));
        const bool scores = dec->last.mode.scores;  // ... but focr_decoder_get_scores has always gone on answering after a set_font: kept as it was
        dec->last = LastRun{};
        dec->last.mode.scores = scores;
        dec->vtables.ok = false;
        drop_baseline_fonts(dec);
        drop_font_candidates(dec);  // they share the previous font's alphabet
    }
    if (!dec || !font || !font->glyphs || !font->n_glyphs) return dfail(dec, "focr_decoder_set_font: bad arguments");
    // the font in locals: a refusal leaves the previous decode font as it was, its record, its tables and n_glyphs
    HostFont h;
    PackedGlyphs packed;
    GlyphTables tables;
    const std::string no = pack_font(*font, nullptr, &h, &packed);
    if (!no.empty()) return dfail(dec, "focr_decoder_set_font: " + no);
    if (tables.upload(packed, font->bitmaps) != hipSuccess) return dfail(dec, "focr_decoder_set_font: hipMalloc / hipMemcpy failed");
    dec->font = std::move(h);
    dec->tables = std::move(tables);
    dec->n_glyphs = (uint32_t)font->n_glyphs;
    dec->d_inc64.release();  // the previous font's; a whole-line run uploads its own
    return 0;
}

// ---- a run in its steps: resolve the settings, geometry and cap, reserve, the third launch, collect ------------------

namespace {

// A run starts: the results of the last one are gone, whatever becomes of this one.
void clear_results(focr_decoder *dec) {
    dec->last = LastRun{};
    dec->base_q.clear();
    dec->base_cost.clear();
    dec->line_font.clear();
    dec->font_cost.clear();
    dec->lines.clear();
    dec->chars.clear();
    dec->char_scores.clear();
    dec->line_base.clear();
    dec->offsets.clear();
    dec->pens.clear();
    dec->line_cost.clear();
    dec->margins.clear();
    dec->run.ms = 0.f;
    dec->run.launches = 0;
}

// What both baseline kinds need of the font, each refused in the kind's own words: the y-phase fonts of its y_bits, and an
// origin_y that is a whole number.
int baseline_font(focr_decoder *dec, uint32_t bits, const std::string &no_fonts, const std::string &bent_origin) {
    if (bits && !(dec->yfonts.ok && dec->yfonts.bits == bits)) return dfail(dec, no_fonts);
    return whole_origin(dec->font.origin_y) ? 0 : dfail(dec, bent_origin);
}

// The settings as one RunMode, or the refusal of their combination (include/focr_decode.h): every refusal that depends on
// the settings, the font and the y-phase fonts alone, before anything is launched, in the order a caller has come to see
// them.  What depends on the batch's geometry follows in the run (batch_geometry, whole_plan).
int resolve_modes(focr_decoder *dec, RunMode *out) {
    const Modes &m = dec->modes;
    const bool baseline = m.base.n != 0, candidates = m.wbase.n != 0;
    if (baseline) {
        const std::string pre = "focr_decoder_run: a baseline search (focr_decoder_set_baseline_search) does not go with ";
        if (m.scores) return dfail(dec, pre + "scores (focr_decoder_set_scores): a runner-up has no definition across candidates yet");
        if (m.pen_search) return dfail(dec, pre + "a pen search (focr_decoder_set_pen_search) yet");
        if (m.whole) return dfail(dec, pre + "the whole-line decode (focr_decoder_set_whole_line) yet");
        if (m.margins) return dfail(dec, pre + "margins (focr_decoder_set_whole_margins) yet");
        if (m.slack) return dfail(dec, pre + "a pen slack (focr_decoder_set_whole_slack) yet");
        if (baseline_font(dec, m.base.bits,
                          "focr_decoder_run: a baseline search with y_bits > 0 (focr_decoder_set_baseline_search) needs the y-phase fonts of that "
                          "y_bits (focr_decoder_set_baseline_fonts)",
                          "focr_decoder_run: a baseline search (focr_decoder_set_baseline_search) needs an origin_y that is a whole number >= 0"))
            return 1;
    }
    if (candidates) {  // a whole-line run under every baseline candidate
        const std::string pre = "focr_decoder_run: baseline candidates of a whole-line run (focr_decoder_set_whole_baseline) ";
        if (!m.whole)
            return dfail(dec, pre + "with the whole-line decode off (focr_decoder_set_whole_line; the pen loop's search is focr_decoder_set_baseline_search)");
        if (m.margins) return dfail(dec, pre + "do not go with margins (focr_decoder_set_whole_margins) yet");
        if (m.slack) return dfail(dec, pre + "do not go with a pen slack (focr_decoder_set_whole_slack) yet");
        if (baseline_font(dec, m.wbase.bits, pre + "with y_bits > 0 need the y-phase fonts of that y_bits (focr_decoder_set_baseline_fonts)",
                          pre + "need an origin_y that is a whole number >= 0"))
            return 1;
    }
    if (m.margins && !m.whole)
        return dfail(dec, "focr_decoder_run: margins on with the whole-line decode off (focr_decoder_set_whole_margins needs focr_decoder_set_whole_line)");
    if (m.slack && !m.whole)
        return dfail(dec, "focr_decoder_run: pen slack on with the whole-line decode off (focr_decoder_set_whole_slack needs focr_decoder_set_whole_line)");
    if (m.slack && m.margins)
        return dfail(dec, "focr_decoder_run: pen slack on with margins on (focr_decoder_set_whole_slack does not go with focr_decoder_set_whole_margins yet)");
    if ((float)m.pen_search * 0.015625f > dec->font.min_inc * 0.5f)
        return dfail(dec, "focr_decoder_run: the pen search radius is more than half the smallest pen increment (the pen could crawl)");
    if (m.frac.on() && !baseline && !candidates)
        return dfail(dec, "focr_decoder_run: a fractional line grid (focr_decoder_set_line_frac) needs a baseline search (focr_decoder_set_baseline_search) or "
                          "baseline candidates of a whole-line run (focr_decoder_set_whole_baseline) with a radius >= 1: no other mode renders at a "
                          "sub-pixel row yet");
    if (m.whole && m.scores) return dfail(dec, "focr_decoder_run: whole-line decode with scores on (a runner-up has no definition under the dynamic programme)");
    if (m.whole && m.pen_search) return dfail(dec, "focr_decoder_run: whole-line decode with a pen search radius (the dynamic programme does not search offsets)");
    if (m.font_search) {  // every line under every candidate font: the plain pen loop or the whole-line programme, and nothing else yet
        const std::string pre = "focr_decoder_run: a font search (focr_decoder_set_font_search) ";
        if (dec->cands.empty()) return dfail(dec, pre + "with no candidates uploaded (focr_decoder_set_font_candidates)");
        if (m.scores) return dfail(dec, pre + "does not go with scores (focr_decoder_set_scores) yet");
        if (m.pen_search) return dfail(dec, pre + "does not go with a pen search (focr_decoder_set_pen_search) yet");
        if (m.margins) return dfail(dec, pre + "does not go with margins (focr_decoder_set_whole_margins) yet");
        if (m.slack) return dfail(dec, pre + "does not go with a pen slack (focr_decoder_set_whole_slack) yet");
        if (baseline) return dfail(dec, pre + "does not go with a baseline search (focr_decoder_set_baseline_search) yet");
        if (candidates) return dfail(dec, pre + "does not go with baseline candidates of a whole-line run (focr_decoder_set_whole_baseline) yet");
    }
    RunMode r;
    r.frac = m.frac;
    if (m.font_search) r.kind = m.whole ? Kind::whole_fonts : Kind::fonts, r.grid = m.fonts_grid;
    else if (baseline) r.kind = Kind::baseline, r.radius = m.base.n, r.bits = m.base.bits, r.grid = m.base_grid;
    else if (candidates) r.kind = Kind::whole_baseline, r.radius = m.wbase.n, r.bits = m.wbase.bits, r.grid = m.whole_grid;
    else if (m.whole) r.kind = m.margins ? Kind::whole_margins : m.slack ? Kind::whole_slack : Kind::whole, r.radius = m.slack, r.grid = m.whole_grid;
    else r.kind = m.pen_search ? Kind::pen_search : Kind::pen_loop, r.radius = m.pen_search, r.scores = m.scores;
    *out = r;
    return 0;
}

// The strip's stride and the characters per line at most, into g.
int line_cap(focr_decoder *dec, const RunMode &mode, const WholePlan &plan, Geometry *g) {
    g->stride = ((g->w + PAD + 3) / 4 + 2) * 4;
    // characters per line at most: the pen moves at least min_inc per step, and f32 rounding is monotone, so the
    // sequence 0, min_inc, ... reaches w no earlier than any pen does.  With a pen search a step is two f32 adds,
    // pen' = (pen + j / 64) + inc with j / 64 >= -reach (exact) and inc >= min_inc; an f32 add is monotone in each
    // operand, so by induction the sequence q' = (q - reach) + min_inc from 0 stays at or below every pen and reaches w
    // no earlier.  It does advance: reach <= min_inc / 2 (resolve_modes), so a step gains min_inc / 2 up to rounding,
    // and one that stalls in f32 runs into the step limit below.  (Dropped candidates only remove choices.)
    const bool search = mode.kind == Kind::pen_search;
    const float reach = search ? (float)mode.radius * 0.015625f : 0.f;  // exact
    // a font search: every candidate's loop runs with its own increments, so the cap is the largest of the fonts' own
    uint32_t steps = 0;
    for (size_t k = 0; k <= (mode.kind == Kind::fonts ? dec->cands.size() : 0); k++) {
        const float min_inc = dec->font_at(k).min_inc;
        uint32_t own = 0;
        for (float p = 0.f; p < (float)g->w; p = search ? (p - reach) + min_inc : p + min_inc)
            if (++own > (1u << 20))
                return dfail(dec, "focr_decoder_run: " + (k ? "font candidate " + std::to_string(k) + ": " : std::string()) + "the pen advance is too small for the line width");
        steps = std::max(steps, own);
    }
    g->cap = mode.whole() ? plan.cap : std::max<uint32_t>(steps, 1);
    return 0;
}

int reserve(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan) {
    const size_t total = g.total, n_all = (size_t)g.cap * total;
    DEC_GROW(dec->d_strips, (size_t)g.stride * g.line_height * total);
    DEC_GROW(dec->d_flags, total);
    DEC_GROW(dec->d_work, total);
    DEC_GROW(dec->d_nchars, total);
    DEC_GROW(dec->d_count, 1);
    DEC_GROW(dec->d_chars, n_all);
    if (mode.scores) {
        DEC_GROW(dec->d_term, n_all);
        DEC_GROW(dec->d_runner_term, n_all);
        DEC_GROW(dec->d_runner, n_all);
        DEC_GROW(dec->d_base, total);
    }
    if (mode.offsets()) DEC_GROW(dec->d_pen, n_all);
    if (mode.fonts() && fonts_reserve(dec, mode, g, plan)) return 1;
    if (mode.whole()) return whole_reserve(dec, mode, g, plan);
    return mode.kind == Kind::baseline ? baseline_reserve(dec, g) : 0;
}

// The pen loop or its search as the third launch.
void pen_launch(focr_decoder *dec, const RunMode &mode, const Geometry &g, size_t strip_bytes) {
    const bool scores = mode.scores;
    const ScoreOut so{dec->d_term, dec->d_runner_term, dec->d_runner, dec->d_base};  // null arrays with scores off: never touched
    if (mode.kind == Kind::pen_search) {  // the strip shares LDS with the reduction pairs, so it stays in LDS up to that much less
        const bool lds = strip_bytes + SEARCH_RED_BYTES <= LDS_STRIP_MAX;
        const auto search = lds ? (scores ? line_search_kernel<true, true> : line_search_kernel<true, false>)
                                : (scores ? line_search_kernel<false, true> : line_search_kernel<false, false>);
        search<<<g.total, SEARCH_THREADS, SEARCH_RED_BYTES + (lds ? strip_bytes : 0), dec->stream>>>(
            dec->d_strips, g, dec->d_work, dec->d_count, dec->tables.glyphs, dec->tables.offs, dec->tables.bitmaps.as<const uint32_t>(), dec->n_glyphs,
            dec->font.origin_x, mode.radius, dec->d_nchars, dec->d_chars, dec->d_pen, so);
    } else {
        const auto decode = strip_bytes <= LDS_STRIP_MAX ? (scores ? line_decode_kernel<true, true> : line_decode_kernel<true, false>)
                                                         : (scores ? line_decode_kernel<false, true> : line_decode_kernel<false, false>);
        decode<<<g.total, 64, strip_bytes <= LDS_STRIP_MAX ? strip_bytes : 0, dec->stream>>>(dec->d_strips, g, dec->d_work, dec->d_count, dec->tables.glyphs,
                                                                                           dec->tables.offs, dec->tables.bitmaps.as<const uint32_t>(), dec->n_glyphs,
                                                                                           dec->font.origin_x, dec->d_nchars, dec->d_chars, so);
    }
}

// The run's three launches between its two events.
int launch(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan, const uint8_t *d_src) {
    const size_t strip_bytes = (size_t)g.stride * g.line_height;
    DEC_CHECK(hipEventRecord(dec->run.begin, dec->stream));
    if (mode.frac.on()) line_prepass_frac_kernel<<<g.total, PREPASS_THREADS, 0, dec->stream>>>(d_src, g, mode.frac, dec->d_strips, dec->d_flags);
    else line_prepass_kernel<<<g.total, PREPASS_THREADS, 0, dec->stream>>>(d_src, g, dec->d_strips, dec->d_flags);
    DEC_CHECK(hipGetLastError());
    line_compact_kernel<<<1, COMPACT_THREADS, 0, dec->stream>>>(dec->d_flags, g.total, dec->d_work, dec->d_count);
    DEC_CHECK(hipGetLastError());
    switch (mode.kind) {
    case Kind::pen_loop:
    case Kind::pen_search: pen_launch(dec, mode, g, strip_bytes); break;
    case Kind::whole:
    case Kind::whole_margins:
    case Kind::whole_slack: whole_launch(dec, mode, g, plan, strip_bytes); break;
    case Kind::whole_baseline: whole_baseline_launch(dec, mode, g, plan, strip_bytes); break;
    case Kind::baseline: baseline_launch(dec, mode, g, strip_bytes); break;
    case Kind::fonts: fonts_launch(dec, mode, g, plan, strip_bytes); break;
    case Kind::whole_fonts: whole_fonts_launch(dec, mode, g, plan, strip_bytes); break;
    }
    DEC_CHECK(hipGetLastError());
    DEC_CHECK(hipEventRecord(dec->run.end, dec->stream));
    return 0;
}

// The first n elements of a device array into v, queued on the decoder's stream.
template <typename T>
int read_back(focr_decoder *dec, std::vector<T> &v, const T *d, size_t n) {
    v.resize(n);
    DEC_CHECK(hipMemcpyAsync(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost, dec->stream));
    return 0;
}

// The n results of work-list line k, [k * cap, k * cap + n) of the device's array, behind those of the lines before it.
template <typename T>
void append_line(std::vector<T> &to, const std::vector<T> &all, size_t k, uint32_t cap, uint32_t n) {
    to.insert(to.end(), all.begin() + k * cap, all.begin() + k * cap + n);
}

// What the kernels wrote, read back and laid out line by line in the decoder's result vectors.
int collect(focr_decoder *dec, const RunMode &mode, const Geometry &g) {
    const size_t total = g.total, n_all = (size_t)g.cap * total;
    const bool baseline = mode.kind == Kind::baseline;
    std::vector<uint32_t> count, work, nch, wpens, lfont;
    std::vector<uint16_t> all, mrunner, runner;
    std::vector<int8_t> pen;
    std::vector<int64_t> wcost, mmargin, bcost, fcost;
    std::vector<int32_t> bq, mterm, term, runner_term;
    std::vector<uint64_t> base;
    if (read_back(dec, count, dec->d_count.p, 1) || read_back(dec, work, dec->d_work.p, total) || read_back(dec, nch, dec->d_nchars.p, total) ||
        read_back(dec, all, dec->d_chars.p, n_all))
        return 1;
    if (mode.offsets() && read_back(dec, pen, dec->d_pen.p, n_all)) return 1;
    if (mode.base_q() && read_back(dec, bq, dec->d_base_q.p, total)) return 1;
    if (baseline && read_back(dec, bcost, dec->d_base_cost.p, total)) return 1;  // under the whole-line decode the cost is that run's
    if (mode.fonts() && read_back(dec, lfont, dec->d_line_font.p, total)) return 1;
    if (mode.kind == Kind::fonts && read_back(dec, fcost, dec->d_font_cost.p, total)) return 1;  // under the whole-line decode the cost is that run's
    if (mode.whole() && (read_back(dec, wpens, dec->d_pens.p, n_all) || read_back(dec, wcost, dec->d_cost.p, total))) return 1;
    if (mode.margins() && (read_back(dec, mterm, dec->d_mterm.p, n_all) || read_back(dec, mrunner, dec->d_mrunner.p, n_all) || read_back(dec, mmargin, dec->d_margin.p, n_all)))
        return 1;
    if (mode.scores && (read_back(dec, term, dec->d_term.p, n_all) || read_back(dec, runner_term, dec->d_runner_term.p, n_all) ||
                        read_back(dec, runner, dec->d_runner.p, n_all) || read_back(dec, base, dec->d_base.p, total)))
        return 1;
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    DEC_CHECK(hipEventElapsedTime(&dec->run.ms, dec->run.begin, dec->run.end));
    dec->run.launches = 3;
    if (count[0] > total) return dfail(dec, "focr_decoder_run: inconsistent line count from the device");
    // q = c_i + offset, 0 <= c_i <= 2^B on the fractional grid and 0 off it
    const int q_hi = (int)FOCR_BASELINE_MAX + (mode.frac.on() ? 1 << mode.bits : 0);
    dec->lines.resize(count[0]);
    for (uint32_t k = 0; k < count[0]; k++) {
        const uint32_t slot = work[k], n = nch[k];
        if (slot >= total || n > g.cap) return dfail(dec, "focr_decoder_run: inconsistent result from the device");
        focr_decoded_line_t &l = dec->lines[k];
        l.page = slot / g.n_slots;
        l.y = (uint32_t)((mode.frac.top(g) + (uint64_t)(slot % g.n_slots) * mode.frac.step(g)) >> 6);  // yc_i; y_start + i * line_advance off the fractional grid
        l.first = dec->chars.size();
        l.n_chars = n;
        l.pad = 0;
        append_line(dec->chars, all, k, g.cap, n);
        if (mode.offsets()) append_line(dec->offsets, pen, k, g.cap, n);
        if (mode.base_q()) {
            if (bq[k] < -(int)FOCR_BASELINE_MAX || bq[k] > q_hi) return dfail(dec, "focr_decoder_run: inconsistent result from the device");
            dec->base_q.push_back((int8_t)bq[k]);
            dec->base_cost.push_back(baseline ? bcost[k] : wcost[k]);
        }
        if (mode.fonts()) {
            if (lfont[k] > dec->cands.size()) return dfail(dec, "focr_decoder_run: inconsistent result from the device");
            dec->line_font.push_back((uint8_t)lfont[k]);
            dec->font_cost.push_back(mode.kind == Kind::fonts ? fcost[k] : wcost[k]);
        }
        if (mode.whole()) {
            append_line(dec->pens, wpens, k, g.cap, n);
            dec->line_cost.push_back(wcost[k]);
        }
        for (size_t at = (size_t)k * g.cap; mode.margins() && at < (size_t)k * g.cap + n; at++)
            dec->margins.push_back(focr_char_margin_t{mterm[at], mrunner[at], 0, mmargin[at]});
        if (!mode.scores) continue;
        dec->line_base.push_back(base[k]);
        for (size_t at = (size_t)k * g.cap; at < (size_t)k * g.cap + n; at++) {  // the reference's score: sum r^2 plus the footprint term
            focr_char_score_t c{(int64_t)base[k] + term[at], (int64_t)base[k] + runner_term[at], runner[at], {0, 0, 0}};
            if (dec->n_glyphs == 1) c.runner_score = INT64_MAX, c.runner = 0xffff;
            dec->char_scores.push_back(c);
        }
    }
    if (!mode.offsets()) dec->offsets.assign(dec->chars.size(), 0);
    return 0;
}

}  // namespace

extern "C" int focr_decoder_run(focr_decoder_t *dec, const uint8_t *pages, int on_device, size_t n_pages, size_t page_w, size_t page_h,
                                uint32_t x_start, uint32_t y_start, uint32_t width, uint32_t line_height, uint32_t line_advance) {
    if (!dec) return dfail(nullptr, "focr_decoder_run: null decoder");
    clear_results(dec);
    if (!dec->n_glyphs) return dfail(dec, "focr_decoder_run: no font (focr_decoder_set_font)");
    if (n_pages && !pages) return dfail(dec, "focr_decoder_run: null pages");
    RunMode mode;
    if (resolve_modes(dec, &mode)) return 1;
    Geometry g{};
    if (batch_geometry(dec, "focr_decoder_run", n_pages, page_w, page_h, x_start, y_start, width, line_height, line_advance, &g, mode.frac)) return 1;
    DEC_CHECK(hipSetDevice(dec->device));
    const uint8_t *d_src = nullptr;
    if (stage_in(dec, dec->d_pages, pages, on_device, page_w * page_h * n_pages, &d_src)) return 1;
    WholePlan plan;
    if (mode.fonts() && fonts_plan(dec, &plan)) return 1;
    if (mode.whole() && whole_plan(dec, mode, g, &plan)) return 1;  // the font and width refusals of include/focr_decode.h, before anything is launched
    if (g.total == 0) {  // nothing to decode and nothing launched; a verify still draws the pages
        DEC_CHECK(hipStreamSynchronize(dec->stream));
    } else if (line_cap(dec, mode, plan, &g) || reserve(dec, mode, g, plan) || launch(dec, mode, g, plan, d_src) || collect(dec, mode, g)) {
        return 1;
    }
    dec->last = LastRun{true, mode, g, n_pages, x_start, d_src};  // what the getters answer from and focr_decoder_verify draws
    return 0;
}

// ---- the setters (each writes its field of Modes) and the getters (each answers from the last run) -------------------

extern "C" int focr_decoder_set_scores(focr_decoder_t *dec, int on) {
    if (!dec) return dfail(nullptr, "focr_decoder_set_scores: null decoder");
    dec->modes.scores = on != 0;
    return 0;
}

extern "C" int focr_decoder_set_pen_search(focr_decoder_t *dec, uint32_t n) {
    if (!dec) return dfail(nullptr, "focr_decoder_set_pen_search: null decoder");
    if (n > FOCR_PEN_SEARCH_MAX) return dfail(dec, "focr_decoder_set_pen_search: the radius is at most 64 (one pixel)");
    dec->modes.pen_search = n;
    return 0;
}

extern "C" int focr_decoder_set_whole_line(focr_decoder_t *dec, int on) {
    if (!dec) return dfail(nullptr, "focr_decoder_set_whole_line: null decoder");
    dec->modes.whole = on != 0;
    return 0;
}

extern "C" int focr_decoder_set_whole_slack(focr_decoder_t *dec, uint32_t n) {
    if (!dec) return dfail(nullptr, "focr_decoder_set_whole_slack: null decoder");
    if (n > FOCR_PEN_SEARCH_MAX) return dfail(dec, "focr_decoder_set_whole_slack: the slack radius is at most 64 (one pixel)");
    dec->modes.slack = n;
    return 0;
}

extern "C" int focr_decoder_set_whole_margins(focr_decoder_t *dec, int on) {
    if (!dec) return dfail(nullptr, "focr_decoder_set_whole_margins: null decoder");
    dec->modes.margins = on != 0;
    return 0;
}

extern "C" int focr_decoder_debug_set_whole_grid(focr_decoder_t *dec, uint32_t grid) {
    if (!dec) return dfail(nullptr, "focr_decoder_debug_set_whole_grid: null decoder");
    dec->modes.whole_grid = grid;
    return 0;
}

extern "C" int focr_decoder_get_offsets(const focr_decoder_t *dec, int8_t *offsets) {
    if (!dec) return dfail(nullptr, "focr_decoder_get_offsets: null decoder");
    if (offsets && !dec->offsets.empty()) memcpy(offsets, dec->offsets.data(), dec->offsets.size());
    return 0;
}

extern "C" int focr_decoder_get_pens(const focr_decoder_t *dec, uint32_t *pens, int64_t *line_cost) {
    if (!dec) return dfail(nullptr, "focr_decoder_get_pens: null decoder");
    if (!(dec->last.ok && dec->last.mode.whole()))
        return dfail(const_cast<focr_decoder *>(dec), "focr_decoder_get_pens: the last successful run was not a whole-line run (focr_decoder_set_whole_line)");
    if (pens && !dec->pens.empty()) memcpy(pens, dec->pens.data(), dec->pens.size() * sizeof(uint32_t));
    if (line_cost && !dec->line_cost.empty()) memcpy(line_cost, dec->line_cost.data(), dec->line_cost.size() * sizeof(int64_t));
    return 0;
}

extern "C" int focr_decoder_get_margins(const focr_decoder_t *dec, focr_char_margin_t *out) {
    if (!dec) return dfail(nullptr, "focr_decoder_get_margins: null decoder");
    if (!(dec->last.ok && dec->last.mode.margins()))
        return dfail(const_cast<focr_decoder *>(dec), "focr_decoder_get_margins: the last successful run was not a margins run (focr_decoder_set_whole_margins)");
    if (out && !dec->margins.empty()) memcpy(out, dec->margins.data(), dec->margins.size() * sizeof(focr_char_margin_t));
    return 0;
}

extern "C" int focr_decoder_get_scores(const focr_decoder_t *dec, focr_char_score_t *scores, uint64_t *line_base) {
    if (!dec) return dfail(nullptr, "focr_decoder_get_scores: null decoder");
    if (!dec->last.mode.scores)  // (not last.ok: see focr_decoder_set_font)
        return dfail(const_cast<focr_decoder *>(dec), "focr_decoder_get_scores: no successful run with scores on (focr_decoder_set_scores)");
    if (scores && !dec->char_scores.empty()) memcpy(scores, dec->char_scores.data(), dec->char_scores.size() * sizeof(focr_char_score_t));
    if (line_base && !dec->line_base.empty()) memcpy(line_base, dec->line_base.data(), dec->line_base.size() * sizeof(uint64_t));
    return 0;
}

extern "C" size_t focr_decoder_n_lines(const focr_decoder_t *dec) { return dec ? dec->lines.size() : 0; }
extern "C" size_t focr_decoder_n_chars(const focr_decoder_t *dec) { return dec ? dec->chars.size() : 0; }

extern "C" int focr_decoder_get(const focr_decoder_t *dec, focr_decoded_line_t *lines, uint16_t *chars) {
    if (!dec) return dfail(nullptr, "focr_decoder_get: null decoder");
    if (lines && !dec->lines.empty()) memcpy(lines, dec->lines.data(), dec->lines.size() * sizeof(focr_decoded_line_t));
    if (chars && !dec->chars.empty()) memcpy(chars, dec->chars.data(), dec->chars.size() * sizeof(uint16_t));
    return 0;
}

extern "C" float focr_decoder_last_ms(const focr_decoder_t *dec) { return dec ? dec->run.ms : 0.f; }
extern "C" uint32_t focr_decoder_last_launches(const focr_decoder_t *dec) { return dec ? dec->run.launches : 0; }
extern "C" float focr_decoder_last_verify_ms(const focr_decoder_t *dec) { return dec ? dec->verify.ms : 0.f; }
extern "C" uint32_t focr_decoder_last_verify_launches(const focr_decoder_t *dec) { return dec ? dec->verify.launches : 0; }
extern "C" float focr_decoder_last_test_ms(const focr_decoder_t *dec) { return dec ? dec->test.ms : 0.f; }
extern "C" uint32_t focr_decoder_last_test_launches(const focr_decoder_t *dec) { return dec ? dec->test.launches : 0; }
