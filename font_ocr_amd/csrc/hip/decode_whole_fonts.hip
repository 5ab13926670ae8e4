// decode_whole_fonts.hip — the whole-line decode of the `focr` line decoder under every candidate font
// (focr_decoder_set_font_search beside focr_decoder_set_whole_line; an extension, see include/focr_decode.h): every line is
// decoded by the dynamic programme of decode_whole.hip once per candidate font k in 0 ..= K, and the candidate whose whole
// line costs least is the line.
//
// line_whole_fonts_kernel takes line_whole_kernel's place as the third launch of a whole-line run when the search is on.
// It is built as decode_whole_baseline.hip's line_whole_baseline_kernel is, from the phases of decode_whole.h; one
// workgroup of four waves takes a work-list line (grid-stride, so a smaller grid takes several):
//   - the strip is staged in LDS once and shared by every candidate (when it fits; else it is read from global memory);
//   - the candidates are taken in index order, one forward pass each, with the candidate's own tables, inc64, origin,
//     batch and largest inc64 (FontDesc, decode_line.h; k is uniform, so the descriptor comes by scalar loads); the cost
//     ring and the scratch are sized for the largest of them, which every candidate's programme fits;
//   - thread 0 keeps the lowest (cost, k) with a strict <, so the first of equal costs stays;
//   - the workgroup's backpointer scratch has two halves: a candidate writes into the half that does not hold the best
//     so far, a new best swaps the roles, and the winner's end state and the glyph that reached it are kept beside its
//     cost, so the walk back runs once, from the winner's half and with the winner's inc64.
// Everything is exact integer arithmetic.
#include <cmath>

#include "decode_whole.h"

namespace focr_dec {

// What line_whole_fonts_kernel needs beyond the plain programme: the uploaded candidates' tables (k-major, as
// focr_decoder_set_font_candidates left them), every candidate's descriptor and inc64, and per work-list line the winner.
struct WholeFonts {
    const DevGlyph *fglyphs;
    const int2 *foffs;
    const uint32_t *fbitmaps;
    const FontDesc *desc;     // [n_fonts]
    const uint32_t *inc64;    // [n_fonts * n_glyphs], at desc[k].inc_base
    uint32_t n_fonts;         // K + 1 >= 2
    uint32_t *line_font;
};

// 3wf. line_whole_kernel under every candidate font.  scratch holds two halves of n_states backpointers per workgroup;
// ring_mask and n_states are the largest over the candidates.
template <bool LDS>
__global__ __launch_bounds__(WHOLE_THREADS) void line_whole_fonts_kernel(const uint8_t *__restrict__ strips, Geometry g, const uint32_t *__restrict__ work,
                                                                         const uint32_t *__restrict__ count, const DevGlyph *__restrict__ glyphs,
                                                                         const int2 *__restrict__ offs, const uint32_t *__restrict__ bitmaps,
                                                                         uint32_t n_glyphs, uint32_t ring_mask, uint32_t n_states, uint16_t *scratch,
                                                                         uint32_t *__restrict__ n_chars, uint16_t *chars, uint32_t *pens,
                                                                         int64_t *__restrict__ costs, WholeFonts wf) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_whole[];
    const WholeLds L = whole_carve(lds_whole, false, ring_mask + 1, 0);
    const uint32_t tid = threadIdx.x, mask = ring_mask, n_live_states = 64u * g.w;
    TermIn T{nullptr, g.stride / 4, 0, (int)g.w, glyphs, offs, bitmaps, 0};
    uint16_t *halves = scratch + (size_t)blockIdx.x * 2 * n_states;
    const uint32_t n_lines = *count;
    for (uint32_t k = blockIdx.x; k < n_lines; k += gridDim.x) {
        const size_t row = (size_t)k * g.cap;
        whole_stage<LDS>(L, strips, g, work[k], &T);
        if (tid == 0) *L.half = 0;  // the previous line's last reader is behind whole_reverse's barriers
        // thread 0's: the best candidate so far, its end state, the glyph that reached it, and the half its backpointers are in
        int64_t best_cost = INT64_MAX;
        uint32_t best_font = 0, best_t = 0, best_gi = 0xffffu, best_half = 0;
        for (uint32_t c = 0; c < wf.n_fonts; c++) {
            const FontDesc d = wf.desc[c];
            T.glyphs = c ? wf.fglyphs + d.glyph_base : glyphs;
            T.offs = c ? wf.foffs + (size_t)d.glyph_base * 64 : offs;
            T.bitmaps = c ? wf.fbitmaps : bitmaps;
            const WholeParams wp{d.origin_d, d.batch, mask, d.max_inc, n_states};
            const uint32_t *inc64 = wf.inc64 + d.inc_base;
            whole_reset(L, mask);  // its barrier also publishes the half to write and, for candidate 0, the strip
            const uint32_t half = *L.half;
            uint16_t *back = halves + (size_t)half * n_states;
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
                if (cost < best_cost) {  // candidates ascend: the first of equal costs stays
                    best_cost = cost, best_font = c, best_t = t, best_gi = gi, best_half = half;
                    *L.half = half ^ 1;  // the next candidate leaves this half alone
                }
            }
            __syncthreads();  // thread 0 has read the ring: the next candidate may reset it
        }
        if (tid == 0) {
            const uint16_t *won = halves + (size_t)best_half * n_states;
            costs[k] = best_cost;
            wf.line_font[k] = best_font;
            whole_walk_from(L, best_t, best_gi, wf.inc64 + wf.desc[best_font].inc_base, n_glyphs, g.cap, row, chars, pens, &n_chars[k],
                            [&](uint32_t t) { return (uint32_t)won[t]; });
        }
        whole_reverse<false>(L, row, chars, pens, nullptr);
    }
}

// ---- the host's side (decode_line.h) ---------------------------------------------------------------------------------

// whole_plan of a whole_fonts run: every candidate passes the whole-line checks with its own font (a refusal names the
// candidate's index), and the plan takes the largest cap, ring and inc64; the scratch and the grid are the baseline
// candidates'.  plan->fonts holds fonts_plan's descriptors; their whole-line part is filled here.
int whole_fonts_plan(focr_decoder *dec, const RunMode &mode, const Geometry &g, WholePlan *plan) {
    const uint32_t G = dec->n_glyphs;
    plan->fonts_inc64.clear();
    plan->cap = 1, plan->ring = 64, plan->max_inc = 0;
    for (size_t k = 0; k < plan->fonts.size(); k++) {
        WholeFontPlan fp;
        const std::string pre = k ? "focr_decoder_run: font candidate " + std::to_string(k) + ": " : std::string("focr_decoder_run: ");
        if (whole_font_plan(dec, pre, dec->font_at(k), dec->font_at(k).term_bound, 0, g.w, &fp)) return 1;
        FontDesc &d = plan->fonts[k];
        d.origin_d = fp.origin_d, d.batch = fp.batch, d.max_inc = fp.max_inc, d.inc_base = (uint32_t)(k * G);
        plan->fonts_inc64.insert(plan->fonts_inc64.end(), fp.inc64.begin(), fp.inc64.end());
        if (k == 0) plan->inc64 = fp.inc64, plan->origin_d = fp.origin_d, plan->batch = fp.batch;
        plan->cap = std::max(plan->cap, fp.cap), plan->ring = std::max(plan->ring, fp.ring), plan->max_inc = std::max(plan->max_inc, fp.max_inc);
    }
    whole_plan_grid(mode, g, false, WHOLE_SCRATCH_BASELINE, plan);
    return 0;
}

int whole_fonts_reserve(focr_decoder *dec, const WholePlan &plan) {
    DEC_GROW(dec->d_finc64, plan.fonts_inc64.size());
    DEC_CHECK(hipMemcpyAsync(dec->d_finc64, plan.fonts_inc64.data(), plan.fonts_inc64.size() * sizeof(uint32_t), hipMemcpyHostToDevice, dec->stream));
    return 0;
}

// The LDS is the plain whole-line run's with the largest ring: the head, the live list and the ring, then the strip when it fits.
void whole_fonts_launch(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan, size_t strip_bytes) {
    const size_t fixed = whole_fixed_bytes(false, plan.ring, 0);
    const bool lds = strip_bytes + fixed <= LDS_STRIP_MAX;
    const size_t lds_bytes = fixed + (lds ? strip_bytes : 0);
    const WholeFonts wf{dec->ftables.glyphs, dec->ftables.offs, dec->ftables.bitmaps.as<const uint32_t>(), dec->d_fdesc, dec->d_finc64, (uint32_t)plan.fonts.size(), dec->d_line_font};
    (lds ? line_whole_fonts_kernel<true> : line_whole_fonts_kernel<false>)<<<plan.grid, WHOLE_THREADS, lds_bytes, dec->stream>>>(
        dec->d_strips, g, dec->d_work, dec->d_count, dec->tables.glyphs, dec->tables.offs, dec->tables.bitmaps.as<const uint32_t>(), dec->n_glyphs, plan.ring - 1,
        plan.n_states, dec->d_back, dec->d_nchars, dec->d_chars, dec->d_pens, dec->d_cost, wf);
}

}  // namespace focr_dec
