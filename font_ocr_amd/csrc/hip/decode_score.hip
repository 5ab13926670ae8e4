// decode_score.hip — focr_decoder_score_text (include/focr_decode.h): the decoder's own cost of lines the caller supplies,
// each line in any font the decoder has uploaded: the decode font (0) or a candidate of the font search (1 ..= K).  Per line
// the sum of r^2 over its crop (line_base), every character's footprint term, and their sum: the number every mode of the
// decoder minimises, for a reading that was decoded, corrected, or typed in.  There is nothing to decode: one glyph per
// character, no alphabet per step and no dynamic programme.  With a shift radius N the whole line is scored 2N + 1 times,
// moved rigidly by j / 64 px, and the lowest (cost, rank of j) is the line.
//
// score_text_kernel, one workgroup of four waves per listed line:
//   - the line's crop is inverted into a PAD-padded strip (what line_prepass_kernel builds) in LDS, and line_base is summed
//     on the way; a strip that does not fit LDS_STRIP_MAX is built in global memory by score_strip_kernel first (a launch
//     of its own, in front) and read from there;
//   - wave w takes the shift candidates of rank w, w + 4, ...; within a candidate the lanes take the characters, 64 at a
//     time: the f32 pen walk is sequential (one readlane and one or two adds per character, as layout_line does it), the
//     terms are the work and come from footprint_term_wide (decode_pen.h), with the row move d it already takes;
//   - a wave keeps its lowest (cost, rank); the four waves meet in LDS, and every wave works out the same winner;
//   - the winner's terms are computed once more by all four waves, 64 characters a wave, and written once; with one
//     candidate (N = 0) that pass is the only one.
// Fonts are read as the font search reads them (a FontDesc per font 0 ..= K), y-phases as the baseline search does (the
// tables of focr_decoder_set_baseline_fonts, v-major).  Everything is exact integer arithmetic but the f32 pen.  The reading is
// checked by text_plan.h and staged by stage_text (decode.h), as focr_decoder_verify_text's is.  The strip staging, the fonts'
// record and the wave's sum are decode_score.h's, shared with focr_decoder_align_text (decode_align.hip).
#include "decode_score.h"

namespace focr_dec {

// per wave: (cost, rank) of the search, the winner's partial cost, the partial line_base; in front of the strip
constexpr uint32_t SCORE_RED_BYTES = SCORE_WAVES * 4 * 8;

struct ScoreText {  // the line's text and how it is placed
    const uint16_t *chars;
    const uint32_t *pens;  // null: the pen walk
    const int8_t *offs;    // null: no per-character offsets
    uint32_t n;
};

// 1. (only when the strip does not fit in LDS) every listed line's strip into global memory, one workgroup per line
__global__ __launch_bounds__(SCORE_THREADS) void score_strip_kernel(const uint8_t *__restrict__ pages, Geometry g, const TextRec *__restrict__ in,
                                                                    uint8_t *__restrict__ strips) {
    const TextRec l = in[blockIdx.x];
    uint32_t h;
    const uint8_t *src = score_crop(pages, g, l, &h);
    (void)score_stage((uint32_t *)(strips + (size_t)blockIdx.x * g.stride * g.line_height), src, g.page_w, g.w, h, g.stride / 4);
}

// The line's summed terms with the whole line moved by j / 64 px, over the 64-character batches wv, wv + nw, ... of the
// line (every wave walks the whole pen); with WRITE the terms go to `terms` (null: nowhere).  The wave's sum, in every lane.
template <bool WRITE>
__device__ __forceinline__ int64_t score_line(const uint32_t *strip, uint32_t sdw, int w, uint32_t h, const ScoreFont &f, const ScoreText &t, int d, int j,
                                              uint32_t wv, uint32_t nw, uint32_t lane, int32_t *__restrict__ terms) {
    int64_t cost = 0;
    float pen = 0.f;
    for (uint32_t base = 0, batch = 0; base < t.n; base += 64, batch++) {
        const uint32_t i = base + lane, m = std::min(64u, t.n - base);
        const bool live = i < t.n, mine = batch % nw == wv;  // mine: uniform
        if (t.pens && !mine) continue;
        const uint32_t c = live ? t.chars[i] : 0;
        int delta;
        if (t.pens) {  // the whole-line programme's: 64 * origin_x + s_g, all integers
            delta = f.origin_d + (live ? (int)t.pens[i] : 0) + j;
        } else {  // the pen loop's one add, or the pen search's two; the rigid shift joins the first character's offset
            const float inc = live ? f.glyphs[c].inc : 0.f;
            const float dj = (float)((live && t.offs ? (int)t.offs[i] : 0) + (i == 0 ? j : 0)) * 0.015625f;
            float pos = 0.f;
            for (uint32_t q = 0; q < m; q++) {
                pen = __fadd_rn(pen, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dj), q)));
                if (lane == q) pos = pen;
                pen = __fadd_rn(pen, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(inc), q)));
            }
            if (!mine) continue;
            delta = (int)__fmul_rn(__fadd_rn(f.origin_x, pos), 64.0f);  // FreeType's delta: trunc(t * 64), negative ones included
        }
        int term = 0;
        if (live) {
            const uint32_t phase = (uint32_t)delta & 63u;
            const int shift = delta >> 6;
            const DevGlyph gl = f.glyphs[c];
            const int2 o = f.offs[c * 64 + phase];
            const uint32_t *tile = f.bitmaps + gl.off_dw + phase * gl.ndw * gl.box_h;
            term = footprint_term_wide(strip, sdw, w, h, tile, f.end, gl.ndw, gl.box_h, shift + o.x, o.y + d);
            if (WRITE && terms) terms[i] = term;
        }
        cost += term;
    }
    return (int64_t)wave_sum((uint64_t)cost);
}

// 2. the lines' costs, one workgroup per listed line
template <bool LDS>
__global__ __launch_bounds__(SCORE_THREADS) void score_text_kernel(const uint8_t *__restrict__ pages, Geometry g, const TextRec *__restrict__ in,
                                                                   const uint16_t *__restrict__ chars, const uint32_t *__restrict__ pens,
                                                                   const int8_t *__restrict__ offs, ScoreFonts fonts, uint32_t radius,
                                                                   const uint8_t *__restrict__ strips, int32_t *__restrict__ terms,
                                                                   focr_text_score_t *__restrict__ out) {
    extern __shared__ __align__(8) uint32_t lds_score[];  // the waves' pairs and partial sums, then (LDS) the strip
    uint64_t *red = (uint64_t *)lds_score;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));  // uniform, and the compiler knows it
    const TextRec l = in[blockIdx.x];
    const uint32_t sdw = g.stride / 4;
    uint32_t h;
    const uint8_t *src = score_crop(pages, g, l, &h);
    const uint32_t *strip;
    uint64_t acc = 0;
    if (LDS) {
        uint32_t *lds_strip = lds_score + SCORE_RED_BYTES / 4;
        acc = score_stage(lds_strip, src, g.page_w, g.w, h, sdw);
        strip = lds_strip;
    } else {  // score_strip_kernel's: the rows below h hold nothing of this line, and a row's pad bytes are zero
        strip = (const uint32_t *)(strips + (size_t)blockIdx.x * g.stride * g.line_height);
        for (uint32_t i = tid; i < sdw * h; i += SCORE_THREADS) acc += __builtin_amdgcn_udot4(strip[i], strip[i], 0u, false);
    }
    acc = wave_sum(acc);
    if (lane == 0) red[3 * SCORE_WAVES + wave] = acc;
    __syncthreads();  // the strip is staged
    int d;
    const ScoreFont f = score_font(fonts, l, &d);
    const ScoreText t{chars + l.first, pens ? pens + l.first : nullptr, offs ? offs + l.first : nullptr, l.n};
    const int w = (int)g.w;
    uint32_t best_rank = 0;
    const uint32_t n_cand = 2 * radius + 1;
    if (n_cand > 1) {
        int64_t best_cost = INT64_MAX;
        best_rank = ~0u;  // a wave without a candidate: never the winner (wave 0 always has rank 0)
        for (uint32_t rank = wave; rank < n_cand; rank += SCORE_WAVES) {
            const int64_t cost = score_line<false>(strip, sdw, w, h, f, t, d, rank_offset(rank), 0, 1, lane, nullptr);
            if (cost < best_cost) best_cost = cost, best_rank = rank;  // a wave's ranks ascend: the first of equal costs stays
        }
        if (lane == 0) red[2 * wave] = (uint64_t)best_cost, red[2 * wave + 1] = best_rank;
        __syncthreads();
        best_cost = (int64_t)red[0], best_rank = (uint32_t)red[1];
        for (uint32_t u = 1; u < SCORE_WAVES; u++) {
            const int64_t c = (int64_t)red[2 * u];
            const uint32_t r = (uint32_t)red[2 * u + 1];
            if (c < best_cost || (c == best_cost && r < best_rank)) best_cost = c, best_rank = r;
        }
        best_rank = (uint32_t)__builtin_amdgcn_readfirstlane((int)best_rank);
    }
    const int j = rank_offset(best_rank);
    const int64_t part = score_line<true>(strip, sdw, w, h, f, t, d, j, wave, SCORE_WAVES, lane, terms ? terms + l.out : nullptr);
    if (lane == 0) red[2 * SCORE_WAVES + wave] = (uint64_t)part;
    __syncthreads();
    if (tid == 0) {
        uint64_t base = 0;
        int64_t cost = 0;
        for (uint32_t u = 0; u < SCORE_WAVES; u++) base += red[3 * SCORE_WAVES + u], cost += (int64_t)red[2 * SCORE_WAVES + u];
        out[blockIdx.x] = focr_text_score_t{base, cost, j, 0};
    }
}

}  // namespace focr_dec

using namespace focr_dec;

extern "C" int focr_decoder_score_text(focr_decoder_t *dec, const uint8_t *pages, int pages_on_device, size_t n_pages, size_t page_w, size_t page_h,
                                       uint32_t x_start, uint32_t width, uint32_t line_height, const focr_text_line_t *lines, size_t n_lines,
                                       const uint16_t *chars, const uint32_t *pens, const int8_t *offsets, size_t n_chars, const int8_t *line_q,
                                       uint32_t y_bits, uint32_t shift_radius, int32_t *terms, focr_text_score_t *out) {
    const std::string who = "focr_decoder_score_text: ";
    if (!dec) return dfail(nullptr, who + "null decoder");
    dec->stext.ms = 0.f;
    dec->stext.launches = 0;
    const TextInput in{lines, n_lines, chars, pens, offsets, n_chars, n_pages};
    std::string no = text_guards(in, pages, n_lines && !out ? "out" : nullptr);
    if (!no.empty()) return dfail(dec, who + no);
    if (!dec->n_glyphs) return dfail(dec, who + "no decode font (focr_decoder_set_font)");
    if (width == 0) return dfail(dec, who + "width 0");
    if (line_height == 0) return dfail(dec, who + "line_height 0");
    if (shift_radius > FOCR_PEN_SEARCH_MAX) return dfail(dec, who + "the shift radius is at most 64 (one pixel)");
    if (y_bits > FOCR_BASELINE_Y_BITS_MAX) return dfail(dec, who + "y_bits is at most 3");
    Geometry g{};
    if (batch_geometry(dec, "focr_decoder_score_text", n_pages, page_w, page_h, x_start, 0, width, 0, 1, &g)) return 1;
    if (n_lines > 0x7fffffffu || n_pages > 0x7fffffffu) return dfail(dec, who + "too many lines or pages in one call");
    if (line_q && y_bits && !(dec->yfonts.ok && dec->yfonts.bits == y_bits))
        return dfail(dec, who + "line_q with y_bits > 0 needs the y-phase fonts of that y_bits (focr_decoder_set_baseline_fonts)");
    TextAsk ask;
    ask.line_q = line_q;
    ask.y_bits = y_bits;
    ask.pen_origin = true;
    TextPlan text;
    if (!(no = plan_text_lines(in, dec->font, dec->cands, ask, &text)).empty() || !(no = plan_text_chars(in, dec->n_glyphs)).empty()) return dfail(dec, who + no);
    const uint64_t n_terms = text.n_out;
    if (n_lines == 0) return 0;
    g.line_height = line_height;
    g.stride = ((g.w + PAD + 3) / 4 + 2) * 4;  // line_cap's
    const size_t strip_bytes = (size_t)g.stride * line_height;
    const bool lds = strip_bytes + SCORE_RED_BYTES <= LDS_STRIP_MAX;  // the strip shares LDS with the waves' pairs and sums
    DEC_CHECK(hipSetDevice(dec->device));
    WholePlan plan;
    ScoreFonts f;
    if (score_fonts(dec, &plan, dec->d_sdesc, line_q ? y_bits : 0, &f)) return 1;
    StagedText st;
    if (stage_text(dec, in, text.recs, pages, pages_on_device, n_pages * page_w * page_h, &st)) return 1;
    if (terms) DEC_GROW(dec->d_sterms, std::max<size_t>(n_terms, 1));
    DEC_GROW(dec->d_sout, n_lines);
    if (!lds) DEC_GROW(dec->d_sstrips, strip_bytes * n_lines);
    int32_t *d_terms = terms ? (int32_t *)dec->d_sterms : nullptr;
    DEC_CHECK(hipEventRecord(dec->stext.begin, dec->stream));
    if (lds) {
        score_text_kernel<true><<<(uint32_t)n_lines, SCORE_THREADS, SCORE_RED_BYTES + strip_bytes, dec->stream>>>(
            st.pages, g, st.recs, st.chars, st.pens, st.offs, f, shift_radius, nullptr, d_terms, dec->d_sout);
    } else {
        score_strip_kernel<<<(uint32_t)n_lines, SCORE_THREADS, 0, dec->stream>>>(st.pages, g, st.recs, dec->d_sstrips);
        DEC_CHECK(hipGetLastError());
        score_text_kernel<false><<<(uint32_t)n_lines, SCORE_THREADS, SCORE_RED_BYTES, dec->stream>>>(
            st.pages, g, st.recs, st.chars, st.pens, st.offs, f, shift_radius, dec->d_sstrips, d_terms, dec->d_sout);
    }
    DEC_CHECK(hipGetLastError());
    DEC_CHECK(hipEventRecord(dec->stext.end, dec->stream));
    DEC_CHECK(hipMemcpyAsync(out, dec->d_sout, n_lines * sizeof(focr_text_score_t), hipMemcpyDeviceToHost, dec->stream));
    if (terms && n_terms) DEC_CHECK(hipMemcpyAsync(terms, dec->d_sterms, n_terms * sizeof(int32_t), hipMemcpyDeviceToHost, dec->stream));
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    DEC_CHECK(hipEventElapsedTime(&dec->stext.ms, dec->stext.begin, dec->stext.end));
    dec->stext.launches = lds ? 1 : 2;
    return 0;
}

extern "C" float focr_decoder_last_score_text_ms(const focr_decoder_t *dec) { return dec ? dec->stext.ms : 0.f; }
extern "C" uint32_t focr_decoder_last_score_text_launches(const focr_decoder_t *dec) { return dec ? dec->stext.launches : 0; }
