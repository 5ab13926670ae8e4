// decode_whole_baseline.hip — the whole-line decode of the `focr` line decoder under every baseline candidate
// (focr_decoder_set_whole_baseline; an extension, see include/focr_decode.h): every line is decoded by the dynamic
// programme of decode_whole.hip once per vertical candidate q in -N ..= N, in steps of 2^-B px, and the candidate whose
// whole line costs least is the line.
//
// line_whole_baseline_kernel takes line_whole_kernel's place as the third launch of a whole-line run when the radius is
// not zero.  It is built from the phases of decode_whole.h; one workgroup of four waves takes a work-list line
// (grid-stride, so a smaller grid takes several):
//   - the strip is staged in LDS once and shared by every candidate (when it fits; else it is read from global memory);
//   - the candidates are taken in rank order (0, -1, +1, ...), one forward pass each; candidate q scores from y-phase
//     v = q & (2^B - 1) of the font (phase 0 is the decode font itself; the others are focr_decoder_set_baseline_fonts')
//     with every box moved down by d = q >> B rows, and footprint_term clips a box to the crop's rows on both sides;
//   - thread 0 keeps the lowest (cost, rank) with a strict <, so the first of equal costs stays;
//   - the workgroup's backpointer scratch has two halves: a candidate writes into the half that does not hold the best
//     so far, a new best swaps the roles, and the winner's end state and the glyph that reached it are kept beside its
//     cost, so the walk back runs once, from the winner's half, and no candidate is decoded twice.
// Everything is exact integer arithmetic.
#include "decode_whole.h"

namespace focr_dec {

// What line_whole_baseline_kernel needs beyond the plain programme: the y-phase tables v >= 1 (v-major, as
// focr_decoder_set_baseline_fonts left them), origin_y (a whole number >= 0), B, the radius, and per work-list line the
// chosen q.
struct WholeBase {
    const DevGlyph *yglyphs;
    const int2 *yoffs;
    const uint32_t *ybitmaps;
    int origin_y;
    uint32_t bits, radius;  // radius >= 1
    int32_t *line_q;
};

// 3wb. line_whole_kernel under every baseline candidate.  scratch holds two halves of wp.n_states backpointers per
// workgroup.  (line_whole_baseline_frac_kernel below restates this body on the fractional line grid: a fix here is a fix
// there.)
template <bool LDS>
__global__ __launch_bounds__(WHOLE_THREADS) void line_whole_baseline_kernel(const uint8_t *__restrict__ strips, Geometry g, const uint32_t *__restrict__ work,
                                                                            const uint32_t *__restrict__ count, const DevGlyph *__restrict__ glyphs,
                                                                            const int2 *__restrict__ offs, const uint32_t *__restrict__ bitmaps,
                                                                            const uint32_t *__restrict__ inc64, uint32_t n_glyphs, WholeParams wp,
                                                                            uint16_t *scratch, uint32_t *__restrict__ n_chars, uint16_t *chars,
                                                                            uint32_t *pens, int64_t *__restrict__ costs, WholeBase wb) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_whole[];
    const WholeLds L = whole_carve(lds_whole, false, wp.ring_mask + 1, 0);
    const uint32_t tid = threadIdx.x, mask = wp.ring_mask, n_live_states = 64u * g.w;
    const uint32_t n_cand = 2 * wb.radius + 1;
    TermIn T{nullptr, g.stride / 4, 0, (int)g.w, glyphs, offs, bitmaps, 0};
    uint16_t *halves = scratch + (size_t)blockIdx.x * 2 * wp.n_states;
    const uint32_t n_lines = *count;
    for (uint32_t k = blockIdx.x; k < n_lines; k += gridDim.x) {
        const size_t row = (size_t)k * g.cap;
        whole_stage<LDS>(L, strips, g, work[k], &T);
        if (tid == 0) *L.half = 0;  // the previous line's last reader is behind whole_reverse's barriers
        // thread 0's: the best candidate so far, its end state, the glyph that reached it, and the half its backpointers are in
        int64_t best_cost = INT64_MAX;
        int best_q = 0;
        uint32_t best_t = 0, best_gi = 0xffffu, best_half = 0;
        for (uint32_t rank = 0; rank < n_cand; rank++) {
            const int q = rank_offset(rank);
            if (wb.origin_y * (1 << wb.bits) + q < 0) continue;  // ty_q < 0: no such rendering (uniform; never rank 0)
            const uint32_t v = (uint32_t)q & ((1u << wb.bits) - 1);
            T.glyphs = v ? wb.yglyphs + (size_t)(v - 1) * n_glyphs : glyphs;
            T.offs = v ? wb.yoffs + (size_t)(v - 1) * n_glyphs * 64 : offs;
            T.bitmaps = v ? wb.ybitmaps : bitmaps;
            T.d = q >> wb.bits;  // floor
            whole_reset(L, mask);  // its barrier also publishes the half to write and, for rank 0, the strip
            const uint32_t half = *L.half;
            uint16_t *back = halves + (size_t)half * wp.n_states;
            whole_forward(
                L, T, wp, inc64, n_glyphs, n_live_states, 0u,
                [&](uint32_t b0, uint32_t j) {
                    const uint64_t key = L.ring[(b0 + j) & mask];
                    if (key == ~0ull) return;
                    back[b0 + j] = (uint16_t)key;
                    whole_list(L, j);
                },
                [&](uint32_t, uint32_t s) { return L.ring[s & mask] >> 16; });
            const uint64_t best = whole_end_state(L, wp, n_live_states);
            if (tid == 0) {
                int64_t cost;
                uint32_t t;
                const uint32_t gi = whole_walk_start(L, wp, best, n_live_states, &cost, &t);
                if (cost < best_cost) {  // ranks ascend: the first of equal costs stays
                    best_cost = cost, best_q = q, best_t = t, best_gi = gi, best_half = half;
                    *L.half = half ^ 1;  // the next candidate leaves this half alone
                }
            }
            __syncthreads();  // thread 0 has read the ring: the next candidate may reset it
        }
        if (tid == 0) {
            const uint16_t *won = halves + (size_t)best_half * wp.n_states;
            costs[k] = best_cost;
            wb.line_q[k] = best_q;
            whole_walk_from(L, best_t, best_gi, inc64, n_glyphs, g.cap, row, chars, pens, &n_chars[k], [&](uint32_t t) { return (uint32_t)won[t]; });
        }
        whole_reverse<false>(L, row, chars, pens, nullptr);
    }
}

// 3wbf. line_whole_baseline_kernel on the fractional line grid (focr_decoder_set_line_frac; decode.h): whole_stage reads the
// crop's rows from that grid and returns the line's own centre c, and the candidates are q = c + rank_offset(rank), for every
// line a workgroup takes.  The rest is line_whole_baseline_kernel's, restated: with one body behind both kernels both
// instantiations of line_whole_baseline_kernel changed their machine code (tools/isa_hash.py), which the mode-off timing pins.
template <bool LDS>
__global__ __launch_bounds__(WHOLE_THREADS) void line_whole_baseline_frac_kernel(const uint8_t *__restrict__ strips, Geometry g, LineFrac fr,
                                                                                 const uint32_t *__restrict__ work, const uint32_t *__restrict__ count,
                                                                                 const DevGlyph *__restrict__ glyphs, const int2 *__restrict__ offs,
                                                                                 const uint32_t *__restrict__ bitmaps, const uint32_t *__restrict__ inc64,
                                                                                 uint32_t n_glyphs, WholeParams wp, uint16_t *scratch, uint32_t *__restrict__ n_chars,
                                                                                 uint16_t *chars, uint32_t *pens, int64_t *__restrict__ costs, WholeBase wb) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_whole[];
    const WholeLds L = whole_carve(lds_whole, false, wp.ring_mask + 1, 0);
    const uint32_t tid = threadIdx.x, mask = wp.ring_mask, n_live_states = 64u * g.w;
    const uint32_t n_cand = 2 * wb.radius + 1;
    TermIn T{nullptr, g.stride / 4, 0, (int)g.w, glyphs, offs, bitmaps, 0};
    uint16_t *halves = scratch + (size_t)blockIdx.x * 2 * wp.n_states;
    const uint32_t n_lines = *count;
    for (uint32_t k = blockIdx.x; k < n_lines; k += gridDim.x) {
        const size_t row = (size_t)k * g.cap;
        const int c = whole_stage<LDS>(L, strips, g, work[k], &T, FracGrid{fr}, wb.bits);  // this line's
        if (tid == 0) *L.half = 0;
        int64_t best_cost = INT64_MAX;
        int best_q = 0;
        uint32_t best_t = 0, best_gi = 0xffffu, best_half = 0;
        for (uint32_t rank = 0; rank < n_cand; rank++) {
            const int q = c + rank_offset(rank);  // the absolute q: y + q * 2^-B is the line's top
            if (wb.origin_y * (1 << wb.bits) + q < 0) continue;  // ty_q < 0: no such rendering (uniform; never rank 0: c >= 0)
            const uint32_t v = (uint32_t)q & ((1u << wb.bits) - 1);
            T.glyphs = v ? wb.yglyphs + (size_t)(v - 1) * n_glyphs : glyphs;
            T.offs = v ? wb.yoffs + (size_t)(v - 1) * n_glyphs * 64 : offs;
            T.bitmaps = v ? wb.ybitmaps : bitmaps;
            T.d = q >> wb.bits;  // floor
            whole_reset(L, mask);
            const uint32_t half = *L.half;
            uint16_t *back = halves + (size_t)half * wp.n_states;
            whole_forward(
                L, T, wp, inc64, n_glyphs, n_live_states, 0u,
                [&](uint32_t b0, uint32_t j) {
                    const uint64_t key = L.ring[(b0 + j) & mask];
                    if (key == ~0ull) return;
                    back[b0 + j] = (uint16_t)key;
                    whole_list(L, j);
                },
                [&](uint32_t, uint32_t s) { return L.ring[s & mask] >> 16; });
            const uint64_t best = whole_end_state(L, wp, n_live_states);
            if (tid == 0) {
                int64_t cost;
                uint32_t t;
                const uint32_t gi = whole_walk_start(L, wp, best, n_live_states, &cost, &t);
                if (cost < best_cost) {  // ranks ascend: the first of equal costs stays
                    best_cost = cost, best_q = q, best_t = t, best_gi = gi, best_half = half;
                    *L.half = half ^ 1;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const uint16_t *won = halves + (size_t)best_half * wp.n_states;
            costs[k] = best_cost;
            wb.line_q[k] = best_q;
            whole_walk_from(L, best_t, best_gi, inc64, n_glyphs, g.cap, row, chars, pens, &n_chars[k], [&](uint32_t t) { return (uint32_t)won[t]; });
        }
        whole_reverse<false>(L, row, chars, pens, nullptr);
    }
}

// ---- the host's side (decode_line.h) ---------------------------------------------------------------------------------

// The LDS is the plain whole-line run's: the head, the live list and the ring, then the strip when it fits.
void whole_baseline_launch(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan, size_t strip_bytes) {
    const WholeParams wp{plan.origin_d, plan.batch, plan.ring - 1, plan.max_inc, plan.n_states};
    const size_t fixed = whole_fixed_bytes(false, plan.ring, 0);
    const bool lds = strip_bytes + fixed <= LDS_STRIP_MAX;
    const size_t lds_bytes = fixed + (lds ? strip_bytes : 0);
    const WholeBase wb{dec->yfonts.tables.glyphs, dec->yfonts.tables.offs, dec->yfonts.tables.bitmaps.as<const uint32_t>(), (int)dec->font.origin_y, mode.bits, mode.radius, dec->d_base_q};
    if (mode.frac.on())  // the kernel's form on the fractional grid: a kernel of its own beside the one it restates
        (lds ? line_whole_baseline_frac_kernel<true> : line_whole_baseline_frac_kernel<false>)<<<plan.grid, WHOLE_THREADS, lds_bytes, dec->stream>>>(
            dec->d_strips, g, mode.frac, dec->d_work, dec->d_count, dec->tables.glyphs, dec->tables.offs, dec->tables.bitmaps.as<const uint32_t>(), dec->d_inc64,
            dec->n_glyphs, wp, dec->d_back, dec->d_nchars, dec->d_chars, dec->d_pens, dec->d_cost, wb);
    else
        (lds ? line_whole_baseline_kernel<true> : line_whole_baseline_kernel<false>)<<<plan.grid, WHOLE_THREADS, lds_bytes, dec->stream>>>(
            dec->d_strips, g, dec->d_work, dec->d_count, dec->tables.glyphs, dec->tables.offs, dec->tables.bitmaps.as<const uint32_t>(), dec->d_inc64, dec->n_glyphs, wp,
            dec->d_back, dec->d_nchars, dec->d_chars, dec->d_pens, dec->d_cost, wb);
}

}  // namespace focr_dec

using namespace focr_dec;

extern "C" int focr_decoder_set_whole_baseline(focr_decoder_t *dec, uint32_t y_bits, uint32_t n) {
    if (!dec) return dfail(nullptr, "focr_decoder_set_whole_baseline: null decoder");
    if (y_bits > FOCR_BASELINE_Y_BITS_MAX) return dfail(dec, "focr_decoder_set_whole_baseline: y_bits is at most 3");
    if (n > FOCR_BASELINE_MAX) return dfail(dec, "focr_decoder_set_whole_baseline: the radius is at most 32 steps");
    dec->modes.wbase = BaseSearch{y_bits, n};
    return 0;
}
