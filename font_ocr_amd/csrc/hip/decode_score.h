// decode_score.h — what the two entry points that cost a caller's lines share on the device: focr_decoder_score_text
// (decode_score.hip) and focr_decoder_align_text (decode_align.hip).  Both run one workgroup of four waves per listed line, stage
// the line's crop as the same PAD-padded inverted strip (in LDS, or in global memory when it does not fit), read the fonts
// 0 ..= K and the y-phases of font 0 through the same record, and take their terms from footprint_term_wide (decode_pen.h).
// Device helpers only (no relocatable device code: they are inlined into each kernel).
#pragma once

#include "decode_pen.h"

namespace focr_dec {

constexpr uint32_t SCORE_THREADS = 256;  // one workgroup of four waves per listed line
constexpr uint32_t SCORE_WAVES = SCORE_THREADS / 64;

// The fonts 0 ..= K and the y-phases v >= 1 of font 0 as a line reads them.
struct ScoreFonts {
    const DevGlyph *glyphs, *fglyphs, *yglyphs;
    const int2 *offs, *foffs, *yoffs;
    const uint32_t *bitmaps, *fbitmaps, *ybitmaps;
    const FontDesc *desc;  // [K + 1]: glyph_base, end_dw, origin_x and origin_d (64 * origin_x where it is whole)
    uint32_t n_glyphs, yn_dw;
    uint32_t bits;         // B of line_q
};

// The tables one line renders from, chosen once per workgroup.
struct ScoreFont {
    const DevGlyph *glyphs;
    const int2 *offs;
    const uint32_t *bitmaps, *end;
    float origin_x;
    int origin_d;
};

// The descriptors of the fonts 0 ..= K in plan->fonts (it outlives the copy: the caller's), origin_d filled, queued into `desc` on the
// decoder's stream, and the record a kernel reads them through; bits is B of line_q (0 without one).
inline int score_fonts(focr_decoder *dec, WholePlan *plan, focr::DevArray<FontDesc> &desc, uint32_t bits, ScoreFonts *out) {
    if (fonts_plan(dec, plan)) return 1;
    for (FontDesc &fd : plan->fonts) fd.origin_d = whole_origin(fd.origin_x) ? 64 * (int)fd.origin_x : 0;
    DEC_GROW(desc, plan->fonts.size());
    DEC_CHECK(hipMemcpyAsync(desc, plan->fonts.data(), plan->fonts.size() * sizeof(FontDesc), hipMemcpyHostToDevice, dec->stream));
    const GlyphTables &t = dec->tables, &c = dec->ftables, &y = dec->yfonts.tables;
    *out = ScoreFonts{t.glyphs, c.glyphs, y.glyphs, t.offs, c.offs, y.offs, t.bitmaps.as<const uint32_t>(), c.bitmaps.as<const uint32_t>(),
                      y.bitmaps.as<const uint32_t>(), desc, dec->n_glyphs, y.n_dw, bits};
    return 0;
}

// The wave's sum of every lane's v (mod 2^64, so a signed sum as well), in every lane.
__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_u64(v, m);
    return v;
}

// The inverted strip of a crop (w columns by h rows at src, PAD zero bytes in front of every row, sdw dwords a row), by a
// workgroup of SCORE_THREADS; this thread's share of the sum of r^2.
__device__ __forceinline__ uint64_t score_stage(uint32_t *dst, const uint8_t *__restrict__ src, uint32_t page_w, uint32_t w, uint32_t h, uint32_t sdw) {
    uint64_t acc = 0;
    for (uint32_t i = threadIdx.x; i < sdw * h; i += SCORE_THREADS) {
        const uint32_t row = i / sdw;
        const int col = 4 * (int)(i % sdw) - (int)PAD;
        uint32_t v = 0;
        for (int b = 0; b < 4; b++)
            if (col + b >= 0 && (uint32_t)(col + b) < w) v |= (uint32_t)(uint8_t)(255 - src[(size_t)row * page_w + col + b]) << (8 * b);
        dst[i] = v;
        acc += __builtin_amdgcn_udot4(v, v, 0u, false);
    }
    return acc;
}

// A line's crop as image::crop_imm clamps it: its first pixel and its rows (0 when the crop is empty either way).
__device__ __forceinline__ const uint8_t *score_crop(const uint8_t *__restrict__ pages, const Geometry &g, const TextRec &l, uint32_t *h) {
    const uint32_t yc = std::min(l.y, g.page_h);
    *h = g.w ? std::min(g.line_height, g.page_h - yc) : 0;
    return pages + (size_t)l.page * g.page_w * g.page_h + (size_t)yc * g.page_w + g.x;
}

// The line's font, its y-phase and its rows' move *d: uniform across the workgroup.
__device__ __forceinline__ ScoreFont score_font(const ScoreFonts &fonts, const TextRec &l, int *d) {
    const FontDesc fd = fonts.desc[l.font];
    const uint32_t v = (uint32_t)l.q & ((1u << fonts.bits) - 1);  // 0 for every font but 0 (refused on the host)
    *d = l.q >> fonts.bits;                                       // floor
    if (l.font)
        return ScoreFont{fonts.fglyphs + fd.glyph_base, fonts.foffs + (size_t)fd.glyph_base * 64, fonts.fbitmaps, fonts.fbitmaps + fd.end_dw, fd.origin_x, fd.origin_d};
    if (v) {
        const size_t at = (size_t)(v - 1) * fonts.n_glyphs;
        return ScoreFont{fonts.yglyphs + at, fonts.yoffs + at * 64, fonts.ybitmaps, fonts.ybitmaps + fonts.yn_dw, fd.origin_x, fd.origin_d};
    }
    return ScoreFont{fonts.glyphs, fonts.offs, fonts.bitmaps, fonts.bitmaps + fd.end_dw, fd.origin_x, fd.origin_d};
}

}  // namespace focr_dec
