// decode_learn.hip — focr_decoder_learn_text (include/focr_decode.h): the sums from which glyph tables are averaged out of a
// reading the caller trusts.  Where focr_decoder_score_text costs every character of a line against the font's bitmap, this adds
// the page's inverted luma under the character's box to the cell (glyph, phase) the placement names: per cell a count, per
// bitmap byte of the cell a sum.  The mean (learn_font.h, on the host) is the least-squares template of the cell.
//
// learn_text_kernel, one workgroup of four waves per listed line; a line of another font than the one asked for ends at once:
//   - the line's crop is staged as score_text_kernel stages it (decode_score.h): the inverted PAD-padded strip in LDS, or by
//     learn_strip_kernel in global memory when it does not fit LDS_STRIP_MAX (a launch of its own, in front);
//   - the pen walk is score_line's (decode_score.hip), 64 characters a batch: every wave walks the whole pen (one readlane and
//     one or two f32 adds per character), lane q of every wave then holds character q's delta, and whether it contributes: in use,
//     and its box_w x box_h box wholly inside the crop;
//   - wave w takes the contributing characters w, w + 4, ... of the batch: the lanes take consecutive entries of the cell's
//     box_h x stride block of `sums` (256 contiguous bytes per step), each one no-return 32-bit integer atomic add of the strip
//     byte under it; a padding column and a zero byte add nothing and are not sent; lane 0 adds the cell's count.
// Integer sums do not depend on the order the adds arrive in: the result is the definition's, bit for bit, whatever the schedule.
// Fonts, staging and refusals are score_text's (decode_score.h, text_plan.h, stage_text); the sums, the counts, the `used` flags,
// the `use` mask, the box records and (when needed) the strips are buffers of this call's own.
#include "decode_score.h"

namespace focr_dec {

// 1. (only when the strip does not fit in LDS) the strip of every listed line of the font into global memory, one workgroup per line
__global__ __launch_bounds__(SCORE_THREADS) void learn_strip_kernel(const uint8_t *__restrict__ pages, Geometry g, const TextRec *__restrict__ in,
                                                                    uint32_t font, uint8_t *__restrict__ strips) {
    const TextRec l = in[blockIdx.x];
    if (l.font != font || l.n == 0) return;
    uint32_t h;
    const uint8_t *src = score_crop(pages, g, l, &h);
    (void)score_stage((uint32_t *)(strips + (size_t)blockIdx.x * g.stride * g.line_height), src, g.page_w, g.w, h, g.stride / 4);
}

// 2. the lines' samples, one workgroup per listed line
template <bool LDS>
__global__ __launch_bounds__(SCORE_THREADS) void learn_text_kernel(const uint8_t *__restrict__ pages, Geometry g, const TextRec *__restrict__ in,
                                                                   const uint16_t *__restrict__ chars, const uint32_t *__restrict__ pens,
                                                                   const int8_t *__restrict__ offs, const uint8_t *__restrict__ use, ScoreFonts fonts,
                                                                   uint32_t font, const LearnGlyph *__restrict__ boxes, const uint8_t *__restrict__ strips,
                                                                   uint32_t *__restrict__ sums, uint32_t *__restrict__ counts, uint8_t *__restrict__ used) {
    extern __shared__ __align__(8) uint32_t lds_learn[];  // (LDS) the strip
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));  // uniform, and the compiler knows it
    const TextRec l = in[blockIdx.x];
    if (l.font != font || l.n == 0) return;  // uniform: `used` is zeroed by the host
    const uint32_t sdw = g.stride / 4;
    uint32_t h;
    const uint8_t *src = score_crop(pages, g, l, &h);
    const uint8_t *strip;
    if (LDS) {
        (void)score_stage(lds_learn, src, g.page_w, g.w, h, sdw);
        strip = (const uint8_t *)lds_learn;
        __syncthreads();  // the strip is staged
    } else {  // learn_strip_kernel's: the rows below h hold nothing of this line and are not read
        strip = strips + (size_t)blockIdx.x * g.stride * g.line_height;
    }
    int d;
    const ScoreFont f = score_font(fonts, l, &d);  // no line_q: y-phase 0 and no row move
    const uint16_t *cs = chars + l.first;
    const uint32_t *ps = pens ? pens + l.first : nullptr;
    const int8_t *os = offs ? offs + l.first : nullptr;
    const uint8_t *us = use ? use + l.first : nullptr;
    float pen = 0.f;
    for (uint32_t base = 0, batch = 0; base < l.n; base += 64, batch++) {
        const uint32_t i = base + lane, m = std::min(64u, l.n - base);
        const bool live = i < l.n;
        const uint32_t c = live ? cs[i] : 0;
        int delta;
        if (ps) {  // the whole-line programme's: 64 * origin_x + s_g, all integers
            delta = f.origin_d + (live ? (int)ps[i] : 0);
        } else {  // the pen loop's one add, or the pen search's two
            const float inc = live ? f.glyphs[c].inc : 0.f;
            const float dj = (float)(live && os ? (int)os[i] : 0) * 0.015625f;
            float pos = 0.f;
            for (uint32_t q = 0; q < m; q++) {
                pen = __fadd_rn(pen, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dj), q)));
                if (lane == q) pos = pen;
                pen = __fadd_rn(pen, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(inc), q)));
            }
            delta = (int)__fmul_rn(__fadd_rn(f.origin_x, pos), 64.0f);  // FreeType's delta: trunc(t * 64), negative ones included
        }
        const uint32_t phase = (uint32_t)delta & 63u;
        const int2 o = f.offs[c * 64 + phase];
        const int x0 = (delta >> 6) + o.x, y0 = o.y;
        const uint32_t box_w = boxes[c].box_w, box_h = f.glyphs[c].box_h;  // below 2^15 each (glyph_term_bound): no sum below wraps
        // no partial boxes; an empty crop (h == 0 either way) holds none, not even a blank glyph's box without pixels
        const bool ok = live && h && (!us || us[i]) && x0 >= 0 && y0 >= 0 && x0 + (int)box_w <= (int)g.w && y0 + (int)box_h <= (int)h;
        if (used && live && batch % SCORE_WAVES == wave) used[l.out + i] = ok;
        const uint64_t mask = __ballot(ok);
        for (uint32_t q = wave; q < m; q += SCORE_WAVES) {  // a wave takes a character
            if (!((mask >> q) & 1)) continue;               // uniform
            const uint32_t cq = (uint32_t)__builtin_amdgcn_readlane((int)c, q), pq = (uint32_t)__builtin_amdgcn_readlane((int)phase, q);
            const uint32_t xq = (uint32_t)__builtin_amdgcn_readlane(x0, q), yq = (uint32_t)__builtin_amdgcn_readlane(y0, q);
            const DevGlyph gl = f.glyphs[cq];
            const LearnGlyph b = boxes[cq];
            const uint32_t stride = gl.ndw * 4, cell = stride * gl.box_h;
            uint32_t *dst = sums + b.at + (size_t)pq * cell;  // the font's own `bitmaps` layout, one uint32 per byte
            const uint8_t *from = strip + (size_t)yq * g.stride + PAD + xq;
            for (uint32_t e = lane; e < cell; e += 64) {
                const uint32_t row = e / stride, col = e % stride;
                if (col >= b.box_w) continue;  // a padding column stays 0
                const uint32_t r = from[(size_t)row * g.stride + col];
                if (r) (void)__hip_atomic_fetch_add(dst + e, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the result is not read: no return
            }
            if (lane == 0) (void)__hip_atomic_fetch_add(counts + cq * 64 + pq, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace focr_dec

using namespace focr_dec;

extern "C" int focr_decoder_learn_text(focr_decoder_t *dec, const uint8_t *pages, int pages_on_device, size_t n_pages, size_t page_w, size_t page_h,
                                       uint32_t x_start, uint32_t width, uint32_t line_height, const focr_text_line_t *lines, size_t n_lines,
                                       const uint16_t *chars, const uint32_t *pens, const int8_t *offsets, const uint8_t *use, size_t n_chars, uint32_t font,
                                       uint32_t *sums, uint32_t *counts, uint8_t *used) {
    const std::string who = "focr_decoder_learn_text: ";
    if (!dec) return dfail(nullptr, who + "null decoder");
    dec->ltext.ms = 0.f;
    dec->ltext.launches = 0;
    const TextInput in{lines, n_lines, chars, pens, offsets, n_chars, n_pages};
    std::string no = text_guards(in, pages, !sums ? "sums" : !counts ? "counts" : nullptr);
    if (!no.empty()) return dfail(dec, who + no);
    if (!dec->n_glyphs) return dfail(dec, who + "no decode font (focr_decoder_set_font)");
    if (width == 0) return dfail(dec, who + "width 0");
    if (line_height == 0) return dfail(dec, who + "line_height 0");
    Geometry g{};
    if (batch_geometry(dec, "focr_decoder_learn_text", n_pages, page_w, page_h, x_start, 0, width, 0, 1, &g)) return 1;
    if (n_lines > 0x7fffffffu || n_pages > 0x7fffffffu) return dfail(dec, who + "too many lines or pages in one call");
    TextAsk ask;
    ask.pen_origin = true;
    TextPlan text;
    if (!(no = plan_text_lines(in, dec->font, dec->cands, ask, &text)).empty() || !(no = plan_text_chars(in, dec->n_glyphs)).empty() ||
        !(no = plan_learn(font, dec->cands.size(), text.n_out)).empty())
        return dfail(dec, who + no);
    const HostFont &hf = dec->font_at(font);
    const size_t n_sums = hf.bitmaps_len, n_counts = (size_t)dec->n_glyphs * FOCR_DECODE_PHASES;
    const uint64_t n_out = text.n_out;
    if (n_lines == 0) {  // nothing to launch: the outputs are this call's alone
        memset(sums, 0, n_sums * sizeof(uint32_t));
        memset(counts, 0, n_counts * sizeof(uint32_t));
        return 0;
    }
    g.line_height = line_height;
    g.stride = ((g.w + PAD + 3) / 4 + 2) * 4;  // line_cap's
    const size_t strip_bytes = (size_t)g.stride * line_height;
    const bool lds = strip_bytes <= LDS_STRIP_MAX;
    DEC_CHECK(hipSetDevice(dec->device));
    WholePlan plan;
    ScoreFonts f;
    if (score_fonts(dec, &plan, dec->d_ldesc, 0, &f)) return 1;
    StagedText st;
    if (stage_text(dec, in, text.recs, pages, pages_on_device, n_pages * page_w * page_h, &st)) return 1;
    const std::vector<LearnGlyph> boxes = learn_boxes(hf);
    DEC_GROW(dec->d_lboxes, boxes.size());
    DEC_GROW(dec->d_lsums, std::max<size_t>(n_sums, 1));
    DEC_GROW(dec->d_lcounts, n_counts);
    if (used) DEC_GROW(dec->d_lused, std::max<size_t>(n_out, 1));
    if (use) DEC_GROW(dec->d_luse, std::max<size_t>(n_chars, 1));
    if (!lds) DEC_GROW(dec->d_lstrips, strip_bytes * n_lines);
    DEC_CHECK(hipMemcpyAsync(dec->d_lboxes, boxes.data(), boxes.size() * sizeof(LearnGlyph), hipMemcpyHostToDevice, dec->stream));
    if (use && n_chars) DEC_CHECK(hipMemcpyAsync(dec->d_luse, use, n_chars, hipMemcpyHostToDevice, dec->stream));
    const uint8_t *d_use = use ? (const uint8_t *)dec->d_luse : nullptr;
    uint8_t *d_used = used ? (uint8_t *)dec->d_lused : nullptr;
    DEC_CHECK(hipEventRecord(dec->ltext.begin, dec->stream));
    if (n_sums) DEC_CHECK(hipMemsetAsync(dec->d_lsums, 0, n_sums * sizeof(uint32_t), dec->stream));  // the outputs are zeroed first, inside the measured span
    DEC_CHECK(hipMemsetAsync(dec->d_lcounts, 0, n_counts * sizeof(uint32_t), dec->stream));
    if (used && n_out) DEC_CHECK(hipMemsetAsync(dec->d_lused, 0, n_out, dec->stream));
    if (lds) {
        learn_text_kernel<true><<<(uint32_t)n_lines, SCORE_THREADS, strip_bytes, dec->stream>>>(st.pages, g, st.recs, st.chars, st.pens, st.offs, d_use, f, font,
                                                                                                  dec->d_lboxes, nullptr, dec->d_lsums, dec->d_lcounts, d_used);
    } else {
        learn_strip_kernel<<<(uint32_t)n_lines, SCORE_THREADS, 0, dec->stream>>>(st.pages, g, st.recs, font, dec->d_lstrips);
        DEC_CHECK(hipGetLastError());
        learn_text_kernel<false><<<(uint32_t)n_lines, SCORE_THREADS, 0, dec->stream>>>(st.pages, g, st.recs, st.chars, st.pens, st.offs, d_use, f, font,
                                                                                        dec->d_lboxes, dec->d_lstrips, dec->d_lsums, dec->d_lcounts, d_used);
    }
    DEC_CHECK(hipGetLastError());
    DEC_CHECK(hipEventRecord(dec->ltext.end, dec->stream));
    if (n_sums) DEC_CHECK(hipMemcpyAsync(sums, dec->d_lsums, n_sums * sizeof(uint32_t), hipMemcpyDeviceToHost, dec->stream));
    DEC_CHECK(hipMemcpyAsync(counts, dec->d_lcounts, n_counts * sizeof(uint32_t), hipMemcpyDeviceToHost, dec->stream));
    if (used && n_out) DEC_CHECK(hipMemcpyAsync(used, dec->d_lused, n_out, hipMemcpyDeviceToHost, dec->stream));
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    DEC_CHECK(hipEventElapsedTime(&dec->ltext.ms, dec->ltext.begin, dec->ltext.end));
    dec->ltext.launches = lds ? 1 : 2;
    return 0;
}

extern "C" float focr_decoder_last_learn_text_ms(const focr_decoder_t *dec) { return dec ? dec->ltext.ms : 0.f; }
extern "C" uint32_t focr_decoder_last_learn_text_launches(const focr_decoder_t *dec) { return dec ? dec->ltext.launches : 0; }
