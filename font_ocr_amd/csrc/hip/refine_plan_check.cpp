// refine_plan_check.cpp — the host plan of a repair (refine_plan.h) at the edges its arithmetic has, without a device: a stand-alone
// program, built with a host compiler under the sanitizers and run by tests/test_refine_plan_host.py.  The fonts are filled by hand,
// origins and glyph boxes only: the plan reads nothing else of a font.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "refine_plan.h"

using namespace focr_dec;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

// A glyph whose box is stride x box_h at (x, y) in every phase but the last, where it lies one column further right.
static focr_decode_glyph_t glyph_of(int32_t x, int32_t y, uint32_t stride, uint32_t box_h) {
    focr_decode_glyph_t s{};
    s.box_w = stride, s.box_h = box_h, s.stride = stride;
    for (int p = 0; p < FOCR_DECODE_PHASES; p++) s.off_x[p] = x + (p == FOCR_DECODE_PHASES - 1), s.off_y[p] = y;
    return s;
}

static HostFont font_of(float origin_x, std::vector<focr_decode_glyph_t> glyphs) {
    HostFont f;
    f.origin_x = origin_x, f.origin_y = 10.f;
    for (const focr_decode_glyph_t &s : glyphs) f.glyphs.push_back(s), f.inc.push_back(1.f);
    return f;
}

// A reading over the fonts 0 ..= 2: the decode font with two glyphs (columns -1 .. 12, rows 2 .. 14 in all), candidate 1 with one
// wide glyph, candidate 2 with a fractional origin_x.
struct Reading {
    std::vector<focr_text_line_t> lines;
    std::vector<uint16_t> chars;
    std::vector<uint32_t> pens;
    HostFont font = font_of(3.f, {glyph_of(-1, 2, 8, 9), glyph_of(0, 4, 12, 10)});
    std::vector<HostFont> cands{font_of(0.f, {glyph_of(-20, -3, 400, 30), glyph_of(0, 0, 4, 1)}), font_of(2.5f, {glyph_of(0, 0, 4, 4), glyph_of(0, 0, 4, 4)})};
    TextPlan text;
    RefinePlan plan;
    void line(uint64_t first, uint32_t n, uint32_t f = 0) { lines.push_back(focr_text_line_t{0, 0, first, n, f}); }
    std::string run(uint32_t radius, uint32_t line_height, size_t fixed = 80) {
        const TextInput in{lines.data(), lines.size(), chars.data(), pens.data(), nullptr, chars.size(), 1};
        TextAsk ask;
        ask.pen_origin = true;
        std::string no = plan_text_lines(in, font, cands, ask, &text);
        if (no.empty()) no = plan_text_chars(in, 2);
        if (no.empty()) no = plan_refine(in, text.recs, font, cands, radius, line_height, fixed, &plan);
        return no;
    }
};

int main() {
    {  // the radii: the maxima are accepted, one more is refused, the radius first
        CHECK(plan_refine_radii(FOCR_PEN_SEARCH_MAX, FOCR_REFINE_SWEEPS_MAX).empty() && plan_refine_radii(0, 0).empty());
        CHECK(plan_refine_radii(FOCR_PEN_SEARCH_MAX + 1, 0) == "the radius is at most 64 (one pixel)");
        CHECK(plan_refine_radii(0, FOCR_REFINE_SWEEPS_MAX + 1) == "at most 8 sweeps");
        CHECK(plan_refine_radii(~0u, ~0u) == "the radius is at most 64 (one pixel)");
    }
    {  // a window row's dwords: the strip dword of column c0 - 3 up to the one behind column c1 - 1's (PAD = 4 bytes in front of column 0)
        uint32_t q0;
        CHECK(refine_row_dwords(0, 1, &q0) == 3 && q0 == 0);    // bytes 1 .. 4 and the second dword of a read at 4: dwords 0 .. 2
        CHECK(refine_row_dwords(3, 4, &q0) == 2 && q0 == 1);    // bytes 4 .. 7, then dword 2
        CHECK(refine_row_dwords(0, 4, &q0) == 3 && q0 == 0);
        CHECK(refine_row_dwords(0, 5, &q0) == 4 && q0 == 0);
        CHECK(refine_row_dwords(7, 8, &q0) == 2 && q0 == 2);
        CHECK(refine_row_dwords(4, 16, &q0) == 5 && q0 == 1);   // bytes 5 .. 19: dwords 1 .. 4, then 5
        CHECK(refine_row_dwords((1u << 22) - 1, 1u << 22, &q0) == 2 && q0 == 1u << 20);
    }
    {  // no lines: accepted, no window
        Reading r;
        CHECK(r.run(64, 1u << 30).empty() && r.plan.win_dw == 0 && r.plan.win_rows == 0 && r.plan.win_bytes() == 0 && r.plan.fonts.size() == 3);
    }
    {  // extents over glyphs and phases; the window's columns grow with the radius, its rows stop at line_height
        Reading r;
        r.chars = {0, 1, 1};
        r.pens = {0, 5, 5};
        r.line(0, 3);
        r.line(1, 0);
        CHECK(r.run(0, 100).empty());
        CHECK(r.plan.fonts[0].x_lo == -1 && r.plan.fonts[0].x_hi == 13 && r.plan.fonts[0].y_lo == 2 && r.plan.fonts[0].y_hi == 14);
        CHECK(r.plan.fonts[1].x_hi == 0 && r.plan.fonts[1].x_lo == 0);  // not used: not measured
        uint32_t q0;  // 14 columns and one more shift: the most dwords are met from column 2 (bytes 3 .. 20, then dword 6)
        CHECK(r.plan.win_rows == 12 && r.plan.win_dw == refine_row_dwords(2, 2 + 15, &q0) && r.plan.win_dw == 7);
        CHECK(r.run(31, 100).empty() && r.plan.win_dw == 7);
        CHECK(r.run(32, 100).empty() && r.plan.win_dw == refine_row_dwords(2, 2 + 16, &q0) && r.plan.win_dw == 7);
        CHECK(r.run(64, 5).empty() && r.plan.win_rows == 5 && r.plan.win_dw == refine_row_dwords(1, 1 + 17, &q0) && r.plan.win_dw == 7);
        r.line(0, 1, 1);  // the wide candidate decides the window
        CHECK(r.run(0, 100).empty() && r.plan.fonts[1].x_lo == -20 && r.plan.fonts[1].x_hi == 381 && r.plan.fonts[1].y_lo == -3 && r.plan.fonts[1].y_hi == 27);
        CHECK(r.plan.win_rows == 30 && r.plan.win_dw == refine_row_dwords(2, 2 + 402, &q0));
    }
    {  // the pens of a line do not decrease: equal pens pass, the first descent is named, lines are apart
        Reading r;
        r.chars = {0, 1, 0, 1};
        r.pens = {7, 7, 6, 9};
        r.line(0, 2);
        r.line(2, 2);
        CHECK(r.run(4, 20).empty());
        r.line(0, 4);
        CHECK(r.run(4, 20) == "line 2: the pen of character 2 lies left of the one before it (the pens of a line do not decrease)");
        r.lines[2] = focr_text_line_t{0, 0, 1, 1, 0};
        CHECK(r.run(4, 20).empty());
        r.pens = {(1u << 24) - 1, (1u << 24) - 1, 0, 0};
        CHECK(r.run(4, 20).empty());
        r.pens[1] = 1u << 24;
        CHECK(r.run(4, 20) == "pen 1 is 2^24 or more (pens must stay exact in f32)");
    }
    {  // origin_x: whole in the line's own font; text_plan.h says it first, for it is given pens
        Reading r;
        r.chars = {0};
        r.pens = {0};
        r.line(0, 1, 2);
        CHECK(r.run(0, 1) == "line 0: pens need its font's origin_x to be a whole number >= 0 (at most 65536)");
        const TextInput in{r.lines.data(), 1, r.chars.data(), r.pens.data(), nullptr, 1, 1};
        std::vector<TextRec> recs{TextRec{0, 0, 1, 2, 0, 0, 0, 0}};
        CHECK(plan_refine(in, recs, r.font, r.cands, 0, 1, 0, &r.plan) == "line 0: a repair needs its font's origin_x to be a whole number >= 0 (at most 65536)");
    }
    {  // a box far from its pen, and a window past the workgroup's memory
        Reading r;
        r.chars = {0};
        r.pens = {0};
        r.line(0, 1);
        r.font.glyphs[1].off_x[5] = (1 << 20) - 12;
        RefineFont e;
        CHECK(refine_extent(r.font, &e).empty() && e.x_hi == 1 << 20 && e.x_lo == -1);
        CHECK(r.run(0, 1).find("does not fit") != std::string::npos);
        r.font.glyphs[1].off_x[5] += 1;
        CHECK(r.run(0, 1) == "line 0: a glyph box of its font lies more than 2^20 px from the pen");
        r.font.glyphs[1].off_x[5] = INT32_MIN;
        CHECK(r.run(0, 1) == "line 0: a glyph box of its font lies more than 2^20 px from the pen");
        r.font.glyphs[1].off_x[5] = 0;
        r.font.glyphs[0].stride = 0xfffffffcu;  // a box of no rows may be that wide
        r.font.glyphs[0].box_h = 0;
        CHECK(r.run(0, 1) == "line 0: a glyph box of its font lies more than 2^20 px from the pen");
        r.font.glyphs[0] = glyph_of(0, -1000, 4000, 2000);
        CHECK(r.run(0, 16).empty() && r.plan.win_rows == 16 && r.plan.win_bytes() <= REFINE_LDS_MAX - 80);
        const std::string no = r.run(0, 17);
        CHECK(no.find("line 0") == std::string::npos && no.find("does not fit the workgroup's memory") != std::string::npos);
        CHECK(r.run(0, 16, REFINE_LDS_MAX).find("does not fit") != std::string::npos);
        r.font.glyphs[0] = glyph_of(-(1 << 20), -(1 << 20), (1 << 21) - 1, 1 << 21);  // the largest extent: no product wraps
        CHECK(r.run(64, ~0u, ~size_t(0) / 2).find("does not fit") != std::string::npos);
    }
    static_assert(sizeof(RefineFont) == 16, "the record the kernel reads");
    if (failures) return 1;
    std::puts("refine plan ok");
    return 0;
}
