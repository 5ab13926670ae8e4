// refine_plan.h — the host's plan of a repair against the composed line error (focr_decoder_refine_text, decode_refine.hip) on top
// of the reading's own rules (text_plan.h, which it leaves as they are): the two radii against their maxima, the whole origin_x the
// pens placement needs, the rule that the pens of a line do not decrease (what every run produces; it lets the kernel bound which
// characters can reach a step's window: no pen moves more than sweeps * radius from a sorted input), the extent of every font's
// boxes around a pen, and from it the size of the LDS window a step gathers the other characters into.  Pure functions that return
// the refusal's text behind the entry point's prefix (empty: accepted).  Plain host code, no HIP runtime and no decoder:
// refine_plan_check.cpp asserts it at the edges of its arithmetic under the sanitizers with a host compiler alone.
#pragma once

#include "text_plan.h"

#ifdef __HIPCC__
#define REFINE_HD __host__ __device__  // the one function the kernel shares with the plan
#else
#define REFINE_HD
#endif

namespace focr_dec {

constexpr uint32_t REFINE_PEN_END = 1u << 24;   // every pen, given or chosen, stays below this
constexpr int64_t REFINE_REACH_MAX = 1 << 20;   // a box lies at most this many pixels from its pen, either way
constexpr uint32_t REFINE_STRIP_PAD = 4;        // decode_line.h's PAD: the window's rows are laid out as the strip's are
constexpr uint32_t REFINE_LDS_MAX = 65536;      // decode_line.h's LDS_STRIP_MAX: what a workgroup's LDS holds at most

// Where the boxes of one font can lie around a pen, over every glyph and phase: columns shift + x_lo .. shift + x_hi (off_x and
// off_x + stride: a row's pad bytes are read as the tile's), rows y_lo .. y_hi (off_y and off_y + box_h).  A font without glyphs
// has an empty extent at 0.
struct RefineFont {
    int32_t x_lo, x_hi, y_lo, y_hi;
};

// The window of one step, as the kernel lays it out: whole dwords of the strip's own row layout, so that a tile dword meets the
// strip and the window at one and the same byte shift.
struct RefinePlan {
    std::vector<RefineFont> fonts;  // of the fonts 0 ..= K
    uint32_t win_dw = 0;            // dwords per window row at most, over the fonts the lines use
    uint32_t win_rows = 0;          // ... and rows
    size_t win_bytes() const { return (size_t)win_dw * win_rows * 4; }
};

// The radii alone: what is refused whatever the lines.
inline std::string plan_refine_radii(uint32_t radius, uint32_t sweeps) {
    if (radius > FOCR_PEN_SEARCH_MAX) return "the radius is at most 64 (one pixel)";
    if (sweeps > FOCR_REFINE_SWEEPS_MAX) return "at most 8 sweeps";
    return {};
}

// A font's extent, or why it has none the kernel can use.
inline std::string refine_extent(const HostFont &f, RefineFont *out) {
    int64_t x_lo = 0, x_hi = 0, y_lo = 0, y_hi = 0;
    bool any = false;
    for (const focr_decode_glyph_t &s : f.glyphs)
        for (int p = 0; p < FOCR_DECODE_PHASES; p++) {
            const int64_t x0 = s.off_x[p], x1 = x0 + s.stride, y0 = s.off_y[p], y1 = y0 + s.box_h;
            x_lo = any ? std::min(x_lo, x0) : x0, x_hi = any ? std::max(x_hi, x1) : x1;
            y_lo = any ? std::min(y_lo, y0) : y0, y_hi = any ? std::max(y_hi, y1) : y1;
            any = true;
        }
    if (x_lo < -REFINE_REACH_MAX || x_hi > REFINE_REACH_MAX || y_lo < -REFINE_REACH_MAX || y_hi > REFINE_REACH_MAX)
        return "a glyph box of its font lies more than 2^20 px from the pen";
    *out = RefineFont{(int32_t)x_lo, (int32_t)x_hi, (int32_t)y_lo, (int32_t)y_hi};
    return {};
}

// The dwords of a window row that holds the crop columns c0 .. c1 - 1 (0 <= c0 < c1) with every read a tile dword makes there: the
// first is the strip dword of column c0 - 3 (a tile dword that reaches c0 with its last byte), the last the one behind the dword of
// column c1 - 1 (the second dword of an unaligned read).  first is written to *q0.
REFINE_HD inline uint32_t refine_row_dwords(uint32_t c0, uint32_t c1, uint32_t *q0) {
    *q0 = (c0 + REFINE_STRIP_PAD - 3) >> 2;
    return ((c1 - 1 + REFINE_STRIP_PAD) >> 2) + 1 - *q0 + 1;
}

// The lines of an accepted reading (plan_text_lines' records; plan_text_chars has passed, and in.pens is not null) against the fonts
// 0 ..= K: the monotone pens, the whole origin_x, the fonts' extents, and the window of a step of radius N on crops of at most
// line_height rows, which has to fit a workgroup's LDS behind `fixed` bytes.
inline std::string plan_refine(const TextInput &in, const std::vector<TextRec> &lines, const HostFont &font, const std::vector<HostFont> &cands,
                               uint32_t radius, uint32_t line_height, size_t fixed, RefinePlan *out) {
    *out = RefinePlan{};
    out->fonts.assign(cands.size() + 1, RefineFont{0, 0, 0, 0});
    std::vector<uint8_t> seen(cands.size() + 1, 0);
    for (size_t l = 0; l < lines.size(); l++) {
        const TextRec &t = lines[l];
        const std::string pre = "line " + std::to_string(l) + ": ";
        const HostFont &f = t.font ? cands[t.font - 1] : font;
        // defence only: with pens given, plan_text_lines (pen_origin) has refused such a font already, in its own words, and that is
        // the message a caller of focr_decoder_refine_text sees; only a caller of this function alone gets here
        if (!whole_origin(f.origin_x)) return pre + "a repair needs its font's origin_x to be a whole number >= 0 (at most 65536)";
        for (uint32_t g = 1; g < t.n; g++)
            if (in.pens[t.first + g] < in.pens[t.first + g - 1])
                return pre + "the pen of character " + std::to_string(g) + " lies left of the one before it (the pens of a line do not decrease)";
        if (seen[t.font]) continue;
        seen[t.font] = 1;
        RefineFont &e = out->fonts[t.font];
        const std::string no = refine_extent(f, &e);
        if (!no.empty()) return pre + no;
        // the candidates' pens span 2N / 64 px, so their whole-pixel shifts differ by at most (2N >> 6) + 1; the columns of a window
        // of that many start anywhere in a dword
        const uint32_t cols = (uint32_t)(e.x_hi - e.x_lo) + (2 * radius >> 6) + 1;
        uint32_t q0, dw = 0;
        for (uint32_t c0 = 0; c0 < 4; c0++) dw = std::max(dw, refine_row_dwords(c0, c0 + std::max(cols, 1u), &q0));
        out->win_dw = std::max(out->win_dw, dw);
        out->win_rows = std::max(out->win_rows, std::min<uint32_t>(line_height, (uint32_t)(e.y_hi - e.y_lo)));
    }
    if (out->win_bytes() > REFINE_LDS_MAX || fixed + out->win_bytes() > REFINE_LDS_MAX)
        return "the window of a step (" + std::to_string(out->win_dw * 4) + " x " + std::to_string(out->win_rows) +
               " bytes: its fonts' boxes, the radius and the crop's rows) does not fit the workgroup's memory";
    return {};
}

}  // namespace focr_dec
