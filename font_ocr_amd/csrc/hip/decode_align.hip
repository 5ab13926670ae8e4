// decode_align.hip — focr_decoder_align_text (include/focr_decode.h): a forced alignment of lines the caller supplies.  Where
// focr_decoder_score_text costs a line at the font's own advances, this fits every character's pen: a state (g, e) is character
// g at its nominal pen m_g (align_plan.h: the running sum of inc64 from `start`) moved by e / 64 px, -W <= e <= W, and a banded
// dynamic programme lets consecutive characters' offsets differ by at most N / 64 px.  (2W + 1) footprint terms per character
// where score_text has one.
//
// align_text_kernel, one workgroup of four waves per listed line:
//   - the line's crop is staged as score_text_kernel stages it (decode_score.h), in LDS behind the programme's two cost rows, or
//     by align_strip_kernel in global memory when the three do not fit LDS_STRIP_MAX together;
//   - step g is one pass over the band: thread t takes the states e = t - W, t + 256 - W, ...: consecutive lanes hold consecutive
//     e, so a wave reads one window of the strip (64 pens span one pixel) and the 64 phase tiles of one glyph, whose record is a
//     scalar load; a state's predecessor is the lowest (F(g - 1, e - d), rank(d)) over the window of the previous row in LDS,
//     read in rank order with a strict compare, so no key is packed and a cost has all of int64 (n terms of below 2^31 each); an
//     unreachable state (dead, or with no reachable predecessor) holds ALIGN_NONE and costs no term; its backpointer d goes to
//     the call's scratch in global memory, one int8 per character and state; one barrier per step, the rows swap;
//   - the end is the lowest (F(n - 1, e), rank(e)): per thread, per wave, then the four waves in LDS;
//   - thread 0 walks the backpointers once and writes the pens; the terms at those pens are computed once more by all threads
//     (the programme keeps no term), and written once.
// Fonts, y-phases, staging and refusals are score_text's (decode_score.h, text_plan.h, stage_text); the plan is align_plan.h's.
#include "decode_score.h"

namespace focr_dec {

// per wave: (cost, rank) of the end and the partial line_base; in front of the two cost rows
constexpr uint32_t ALIGN_RED_BYTES = SCORE_WAVES * 3 * 8;
constexpr int64_t ALIGN_NONE = INT64_MAX;  // an unreachable state: no sum of terms comes near it

__host__ __device__ inline size_t align_row_bytes(uint32_t band) { return (size_t)band * sizeof(int64_t); }

// The pen search's rank of an offset: 0, -1, +1, -2, ... are 0, 1, 2, 3, ... (rank_offset's inverse).
__device__ __forceinline__ uint32_t offset_rank(int e) { return e < 0 ? (uint32_t)(-2 * e - 1) : (uint32_t)(2 * e); }

// 1. (only when the strip does not fit in LDS beside the rows) every listed line's strip into global memory, one workgroup per line
__global__ __launch_bounds__(SCORE_THREADS) void align_strip_kernel(const uint8_t *__restrict__ pages, Geometry g, const TextRec *__restrict__ in,
                                                                    uint8_t *__restrict__ strips) {
    const TextRec l = in[blockIdx.x];
    uint32_t h;
    const uint8_t *src = score_crop(pages, g, l, &h);
    (void)score_stage((uint32_t *)(strips + (size_t)blockIdx.x * g.stride * g.line_height), src, g.page_w, g.w, h, g.stride / 4);
}

// T(g, e): glyph c (record gl) of the line's font at pen `pen` >= 0, the rows moved by d.
__device__ __forceinline__ int align_term(const uint32_t *strip, uint32_t sdw, int w, uint32_t h, const ScoreFont &f, const DevGlyph &gl, uint32_t c, int d,
                                          int pen) {
    const int delta = f.origin_d + pen;  // the whole-line programme's: 64 * origin_x + s, all integers
    const uint32_t phase = (uint32_t)delta & 63u;
    const int2 o = f.offs[c * 64 + phase];
    const uint32_t *tile = f.bitmaps + gl.off_dw + phase * gl.ndw * gl.box_h;
    return footprint_term_wide(strip, sdw, w, h, tile, f.end, gl.ndw, gl.box_h, (delta >> 6) + o.x, o.y + d);
}

// 2. the lines' alignments, one workgroup per listed line
template <bool LDS>
__global__ __launch_bounds__(SCORE_THREADS) void align_text_kernel(const uint8_t *__restrict__ pages, Geometry g, const TextRec *__restrict__ in,
                                                                   const AlignRec *__restrict__ arecs, const uint16_t *__restrict__ chars,
                                                                   const uint32_t *__restrict__ nominal, ScoreFonts fonts, uint32_t drift, uint32_t step,
                                                                   const uint8_t *__restrict__ strips, int8_t *__restrict__ back, uint32_t *__restrict__ pens,
                                                                   int32_t *__restrict__ terms, focr_text_align_t *__restrict__ out) {
    extern __shared__ __align__(8) uint32_t lds_align[];  // the waves' pairs and partial sums, the two cost rows, then (LDS) the strip
    uint64_t *red = (uint64_t *)lds_align;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const TextRec l = in[blockIdx.x];
    const uint32_t band = 2 * drift + 1, sdw = g.stride / 4;
    const int W = (int)drift;
    int64_t *prev = (int64_t *)(lds_align + ALIGN_RED_BYTES / 4), *cur = prev + band;
    uint32_t h;
    const uint8_t *src = score_crop(pages, g, l, &h);
    const uint32_t *strip;
    uint64_t acc = 0;
    if (LDS) {
        uint32_t *lds_strip = (uint32_t *)(cur + band);
        acc = score_stage(lds_strip, src, g.page_w, g.w, h, sdw);
        strip = lds_strip;
    } else {  // align_strip_kernel's: the rows below h hold nothing of this line, and a row's pad bytes are zero
        strip = (const uint32_t *)(strips + (size_t)blockIdx.x * g.stride * g.line_height);
        for (uint32_t i = tid; i < sdw * h; i += SCORE_THREADS) acc += __builtin_amdgcn_udot4(strip[i], strip[i], 0u, false);
    }
    acc = wave_sum(acc);
    if (lane == 0) red[2 * SCORE_WAVES + wave] = acc;
    __syncthreads();  // the strip is staged
    uint64_t base = 0;
    for (uint32_t u = 0; u < SCORE_WAVES; u++) base += red[2 * SCORE_WAVES + u];
    if (l.n == 0) {  // uniform
        if (tid == 0) out[blockIdx.x] = focr_text_align_t{base, 0, 0, 0};
        return;
    }
    int d;
    const ScoreFont f = score_font(fonts, l, &d);
    const uint16_t *cs = chars + l.first;
    const uint32_t *nom = nominal + l.out;
    int8_t *bk = back + arecs[blockIdx.x].back;
    const int w = (int)g.w;
    const uint32_t n_rank = 2 * std::min(step, 2 * drift) + 1;  // an offset step past the band's width reaches nothing
    for (uint32_t gi = 0; gi < l.n; gi++) {
        const uint32_t c = cs[gi];
        const int m = (int)nom[gi];
        const DevGlyph gl = f.glyphs[c];
        for (uint32_t i = tid; i < band; i += SCORE_THREADS) {
            const int pen = m + (int)i - W;
            int64_t best = ALIGN_NONE;
            int bd = 0;
            if (pen >= 0) {  // live
                if (gi == 0) best = 0;
                else
                    for (uint32_t rank = 0; rank < n_rank; rank++) {  // in rank order: a strict < keeps the lowest rank of equal costs
                        const int dd = rank_offset(rank), s = (int)i - dd;
                        if (s < 0 || s >= (int)band) continue;
                        const int64_t v = prev[s];
                        if (v < best) best = v, bd = dd;
                    }
                if (best != ALIGN_NONE) best += align_term(strip, sdw, w, h, f, gl, c, d, pen);
            }
            cur[i] = best;
            bk[(size_t)gi * band + i] = (int8_t)bd;
        }
        __syncthreads();  // the row is whole, and the previous one is free
        int64_t *t = prev;
        prev = cur, cur = t;
    }
    // the end: the lowest (F(n - 1, e), rank(e)); e = 0 is reachable in every row, so there is one
    int64_t end_cost = ALIGN_NONE;
    uint32_t end_rank = ~0u;
    for (uint32_t i = tid; i < band; i += SCORE_THREADS) {
        const int64_t v = prev[i];
        const uint32_t r = offset_rank((int)i - W);
        if (v < end_cost || (v == end_cost && v != ALIGN_NONE && r < end_rank)) end_cost = v, end_rank = r;
    }
    for (int s = 32; s >= 1; s >>= 1) {
        const int64_t v = (int64_t)shfl_xor_u64((uint64_t)end_cost, s);
        const uint32_t r = (uint32_t)__shfl_xor((int)end_rank, s, 64);
        if (v < end_cost || (v == end_cost && r < end_rank)) end_cost = v, end_rank = r;
    }
    if (lane == 0) red[2 * wave] = (uint64_t)end_cost, red[2 * wave + 1] = end_rank;
    __syncthreads();  // ... which also orders the last row's backpointers before the walk
    if (tid == 0) {
        end_cost = (int64_t)red[0], end_rank = (uint32_t)red[1];
        for (uint32_t u = 1; u < SCORE_WAVES; u++) {
            const int64_t v = (int64_t)red[2 * u];
            const uint32_t r = (uint32_t)red[2 * u + 1];
            if (v < end_cost || (v == end_cost && r < end_rank)) end_cost = v, end_rank = r;
        }
        const int last = rank_offset(end_rank);
        int e = last;
        for (uint32_t gi = l.n; gi-- > 0;) {  // the walk back
            pens[l.out + gi] = (uint32_t)((int)nom[gi] + e);
            if (gi) e -= bk[(size_t)gi * band + (uint32_t)(e + W)];
        }
        out[blockIdx.x] = focr_text_align_t{base, end_cost, e, last};
    }
    if (!terms) return;  // uniform
    __syncthreads();     // the pens are written (the workgroup's own global stores are visible behind its barrier)
    for (uint32_t gi = tid; gi < l.n; gi += SCORE_THREADS) {
        const uint32_t c = cs[gi];
        terms[l.out + gi] = align_term(strip, sdw, w, h, f, f.glyphs[c], c, d, (int)pens[l.out + gi]);
    }
}

}  // namespace focr_dec

using namespace focr_dec;

extern "C" int focr_decoder_align_text(focr_decoder_t *dec, const uint8_t *pages, int pages_on_device, size_t n_pages, size_t page_w, size_t page_h,
                                       uint32_t x_start, uint32_t width, uint32_t line_height, const focr_text_line_t *lines, size_t n_lines,
                                       const uint16_t *chars, size_t n_chars, const int8_t *line_q, uint32_t y_bits, uint32_t start, uint32_t drift,
                                       uint32_t step, uint32_t *pens_out, int32_t *terms, focr_text_align_t *out) {
    const std::string who = "focr_decoder_align_text: ";
    if (!dec) return dfail(nullptr, who + "null decoder");
    dec->atext.ms = 0.f;
    dec->atext.launches = 0;
    const TextInput in{lines, n_lines, chars, nullptr, nullptr, n_chars, n_pages};
    std::string no = text_guards(in, pages, n_lines && !out ? "out" : n_lines && !pens_out ? "pens_out" : nullptr);
    if (!no.empty()) return dfail(dec, who + no);
    if (!dec->n_glyphs) return dfail(dec, who + "no decode font (focr_decoder_set_font)");
    if (width == 0) return dfail(dec, who + "width 0");
    if (line_height == 0) return dfail(dec, who + "line_height 0");
    if (!(no = plan_align_radii(drift, step)).empty()) return dfail(dec, who + no);
    if (y_bits > FOCR_BASELINE_Y_BITS_MAX) return dfail(dec, who + "y_bits is at most 3");
    Geometry g{};
    if (batch_geometry(dec, "focr_decoder_align_text", n_pages, page_w, page_h, x_start, 0, width, 0, 1, &g)) return 1;
    if (n_lines > 0x7fffffffu || n_pages > 0x7fffffffu) return dfail(dec, who + "too many lines or pages in one call");
    if (line_q && y_bits && !(dec->yfonts.ok && dec->yfonts.bits == y_bits))
        return dfail(dec, who + "line_q with y_bits > 0 needs the y-phase fonts of that y_bits (focr_decoder_set_baseline_fonts)");
    TextAsk ask;
    ask.line_q = line_q;
    ask.y_bits = y_bits;
    ask.pen_origin = true;  // no pens come in; the whole origin_x the placement needs is plan_align's to ask for
    TextPlan text;
    AlignPlan plan;
    if (!(no = plan_text_lines(in, dec->font, dec->cands, ask, &text)).empty() || !(no = plan_text_chars(in, dec->n_glyphs)).empty() ||
        !(no = plan_align(in, text.recs, text.n_out, dec->font, dec->cands, start, drift, &plan)).empty())
        return dfail(dec, who + no);
    if (n_lines == 0) return 0;
    const uint64_t n_out = text.n_out;
    const uint32_t band = 2 * drift + 1;
    g.line_height = line_height;
    g.stride = ((g.w + PAD + 3) / 4 + 2) * 4;  // line_cap's
    const size_t strip_bytes = (size_t)g.stride * line_height, fixed = ALIGN_RED_BYTES + 2 * align_row_bytes(band);
    const bool lds = strip_bytes + fixed <= LDS_STRIP_MAX;  // the strip shares LDS with the waves' pairs and the two cost rows
    DEC_CHECK(hipSetDevice(dec->device));
    WholePlan fplan;
    ScoreFonts f;
    if (score_fonts(dec, &fplan, dec->d_adesc, line_q ? y_bits : 0, &f)) return 1;
    StagedText st;
    if (stage_text(dec, in, text.recs, pages, pages_on_device, n_pages * page_w * page_h, &st)) return 1;
    DEC_GROW(dec->d_arecs, n_lines);
    DEC_GROW(dec->d_anominal, std::max<size_t>(n_out, 1));
    DEC_GROW(dec->d_aback, std::max<size_t>(plan.back_bytes, 1));
    DEC_GROW(dec->d_apens, std::max<size_t>(n_out, 1));
    if (terms) DEC_GROW(dec->d_aterms, std::max<size_t>(n_out, 1));
    DEC_GROW(dec->d_aout, n_lines);
    if (!lds) DEC_GROW(dec->d_astrips, strip_bytes * n_lines);
    DEC_CHECK(hipMemcpyAsync(dec->d_arecs, plan.recs.data(), n_lines * sizeof(AlignRec), hipMemcpyHostToDevice, dec->stream));
    if (n_out) DEC_CHECK(hipMemcpyAsync(dec->d_anominal, plan.nominal.data(), n_out * sizeof(uint32_t), hipMemcpyHostToDevice, dec->stream));
    int32_t *d_terms = terms ? (int32_t *)dec->d_aterms : nullptr;
    DEC_CHECK(hipEventRecord(dec->atext.begin, dec->stream));
    if (lds) {
        align_text_kernel<true><<<(uint32_t)n_lines, SCORE_THREADS, fixed + strip_bytes, dec->stream>>>(
            st.pages, g, st.recs, dec->d_arecs, st.chars, dec->d_anominal, f, drift, step, nullptr, dec->d_aback, dec->d_apens, d_terms, dec->d_aout);
    } else {
        align_strip_kernel<<<(uint32_t)n_lines, SCORE_THREADS, 0, dec->stream>>>(st.pages, g, st.recs, dec->d_astrips);
        DEC_CHECK(hipGetLastError());
        align_text_kernel<false><<<(uint32_t)n_lines, SCORE_THREADS, fixed, dec->stream>>>(
            st.pages, g, st.recs, dec->d_arecs, st.chars, dec->d_anominal, f, drift, step, dec->d_astrips, dec->d_aback, dec->d_apens, d_terms, dec->d_aout);
    }
    DEC_CHECK(hipGetLastError());
    DEC_CHECK(hipEventRecord(dec->atext.end, dec->stream));
    DEC_CHECK(hipMemcpyAsync(out, dec->d_aout, n_lines * sizeof(focr_text_align_t), hipMemcpyDeviceToHost, dec->stream));
    if (n_out) DEC_CHECK(hipMemcpyAsync(pens_out, dec->d_apens, n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, dec->stream));
    if (terms && n_out) DEC_CHECK(hipMemcpyAsync(terms, dec->d_aterms, n_out * sizeof(int32_t), hipMemcpyDeviceToHost, dec->stream));
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    DEC_CHECK(hipEventElapsedTime(&dec->atext.ms, dec->atext.begin, dec->atext.end));
    dec->atext.launches = lds ? 1 : 2;
    return 0;
}

extern "C" float focr_decoder_last_align_text_ms(const focr_decoder_t *dec) { return dec ? dec->atext.ms : 0.f; }
extern "C" uint32_t focr_decoder_last_align_text_launches(const focr_decoder_t *dec) { return dec ? dec->atext.launches : 0; }
