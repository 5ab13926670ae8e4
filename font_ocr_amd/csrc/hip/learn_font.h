// learn_font.h — focr_decode_font_learn (include/focr_decode.h): the bitmaps of a decode font with every cell (glyph, phase) that a
// trusted reading showed often enough replaced by the mean of the page under it, from focr_decoder_learn_text's sums and counts.
// Per cell: learned when its count reaches min_count and the base phase has ink; its support is the bounding rectangle of the base
// phase's non-zero pixels, grown by `grow` on each side and clipped to the box; inside it the byte is the mean rounded half up,
// everywhere else the base's.  Plain host code, no HIP runtime and no FreeType: libfocr_raster.so exports it, and
// learn_font_check.cpp asserts it at its edges under the sanitizers with a host compiler alone.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "focr_decode.h"

namespace focr_dec {

struct LearnRect {  // columns x0 .. x1 - 1 and rows y0 .. y1 - 1 of a glyph's box; empty when x1 <= x0
    uint32_t x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    bool empty() const { return x1 <= x0 || y1 <= y0; }
};

// The bounding rectangle of the non-zero pixels of one phase (box_h rows of `stride` bytes, box_w of them pixels); empty without ink.
inline LearnRect learn_ink_rect(const uint8_t *phase, uint32_t box_w, uint32_t box_h, uint32_t stride) {
    LearnRect r;
    bool any = false;
    for (uint32_t y = 0; y < box_h; y++)
        for (uint32_t x = 0; x < box_w; x++) {
            if (!phase[(size_t)y * stride + x]) continue;
            r.x0 = any ? std::min(r.x0, x) : x, r.y0 = any ? std::min(r.y0, y) : y;
            r.x1 = any ? std::max(r.x1, x + 1) : x + 1, r.y1 = any ? std::max(r.y1, y + 1) : y + 1;
            any = true;
        }
    return r;
}

// ... grown by `grow` pixels on each side and clipped to the box (an empty rectangle stays empty: no ink, nothing to learn).
inline LearnRect learn_grow_rect(LearnRect r, uint32_t grow, uint32_t box_w, uint32_t box_h) {
    if (r.empty()) return r;
    r.x0 -= std::min(r.x0, grow), r.y0 -= std::min(r.y0, grow);
    r.x1 += std::min(box_w - r.x1, grow), r.y1 += std::min(box_h - r.y1, grow);
    return r;
}

// The mean sum / n rounded half up, n >= 1: at most 255 where every sample is.
inline uint8_t learn_mean(uint64_t sum, uint64_t n) { return (uint8_t)std::min<uint64_t>((2 * sum + n) / (2 * n), 255); }

struct LearnStats {
    size_t learned = 0, inked = 0;  // cells replaced by their mean; cells whose base phase has ink
};

// The learned bitmaps of `base` into *bitmaps (base.bitmaps_len bytes), or the refusal's text (empty: done).
inline std::string learn_font_bitmaps(const focr_decode_font_t &base, const uint64_t *sums, const uint64_t *counts, uint32_t min_count, uint32_t grow,
                                      std::vector<uint8_t> *bitmaps, LearnStats *stats) {
    if ((base.n_glyphs && !base.glyphs) || (base.bitmaps_len && !base.bitmaps)) return "null base font tables";
    if (!sums || !counts) return "null sums or counts";
    if (min_count < 1) return "min_count must be at least 1";
    bitmaps->assign(base.bitmaps, base.bitmaps + base.bitmaps_len);
    *stats = LearnStats{};
    for (size_t i = 0; i < base.n_glyphs; i++) {
        const focr_decode_glyph_t &g = base.glyphs[i];
        const size_t cell = (size_t)g.stride * g.box_h;
        if (g.stride < g.box_w || g.offset > base.bitmaps_len || cell * FOCR_DECODE_PHASES > base.bitmaps_len - g.offset) return "inconsistent glyph table";
        for (uint32_t p = 0; p < FOCR_DECODE_PHASES; p++) {
            const size_t at = (size_t)g.offset + p * cell;
            const LearnRect r = learn_grow_rect(learn_ink_rect(base.bitmaps + at, g.box_w, g.box_h, g.stride), grow, g.box_w, g.box_h);
            if (r.empty()) continue;  // a blank phase stays blank
            stats->inked++;
            const uint64_t n = counts[i * FOCR_DECODE_PHASES + p];
            if (n < min_count) continue;
            stats->learned++;
            for (uint32_t y = r.y0; y < r.y1; y++)
                for (uint32_t x = r.x0; x < r.x1; x++) (*bitmaps)[at + (size_t)y * g.stride + x] = learn_mean(sums[at + (size_t)y * g.stride + x], n);
        }
    }
    return {};
}

}  // namespace focr_dec
