// learn_font_check.cpp — the learned font (learn_font.h) at its edges, without a device and without FreeType: a stand-alone program,
// built with a host compiler under the sanitizers and run by tests/test_learn_font_host.py.  The font is filled by hand: one
// glyph of 5 x 4 pixels in rows of 8 bytes, ink in a few phases only; and text_plan.h's two rules of focr_decoder_learn_text.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "learn_font.h"
#include "text_plan.h"

using namespace focr_dec;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

constexpr uint32_t BW = 5, BH = 4, STRIDE = 8, CELL = STRIDE * BH;

struct Font {
    focr_decode_glyph_t glyph{};
    std::vector<uint8_t> bitmaps = std::vector<uint8_t>(4 + (size_t)FOCR_DECODE_PHASES * CELL, 0);  // exactly the table: a byte past it is ASan's
    std::vector<uint64_t> sums = std::vector<uint64_t>(bitmaps.size(), 0), counts = std::vector<uint64_t>(FOCR_DECODE_PHASES, 0);
    focr_decode_font_t f{};
    Font() {
        glyph.box_w = BW, glyph.box_h = BH, glyph.stride = STRIDE, glyph.offset = 4, glyph.increment = 1.f;
        f.glyphs = &glyph, f.n_glyphs = 1, f.bitmaps = bitmaps.data(), f.bitmaps_len = bitmaps.size();
    }
    uint8_t &px(uint32_t p, uint32_t y, uint32_t x) { return bitmaps[4 + (size_t)p * CELL + y * STRIDE + x]; }
    uint64_t &sum(uint32_t p, uint32_t y, uint32_t x) { return sums[4 + (size_t)p * CELL + y * STRIDE + x]; }
    void fill_sums(uint32_t p, uint64_t v) {  // the whole box of phase p, padding columns left 0 as learn_text leaves them
        for (uint32_t y = 0; y < BH; y++)
            for (uint32_t x = 0; x < BW; x++) sum(p, y, x) = v;
    }
};

static uint8_t at(const std::vector<uint8_t> &b, uint32_t p, uint32_t y, uint32_t x) { return b[4 + (size_t)p * CELL + y * STRIDE + x]; }

int main() {
    // the rounding: the mean, half up, at most 255
    CHECK(learn_mean(0, 1) == 0 && learn_mean(255, 1) == 255 && learn_mean(1, 2) == 1 && learn_mean(1, 3) == 0 && learn_mean(2, 3) == 1);
    CHECK(learn_mean(255ull * 7 + 3, 7) == 255 && learn_mean(5, 2) == 3 && learn_mean(3, 2) == 2 && learn_mean(10, 4) == 3 && learn_mean(9, 4) == 2);
    CHECK(learn_mean(255ull << 40, 1ull << 40) == 255 && learn_mean((255ull << 24) - 1, 1ull << 24) == 255 && learn_mean((1ull << 23) - 1, 1ull << 24) == 0);

    // the rectangle: the bounding box of the non-zero pixels, and its growth clipped to the box
    Font t;
    t.px(1, 1, 2) = 9, t.px(1, 2, 3) = 1;  // phase 1: ink in rows 1 .. 2, columns 2 .. 3
    t.px(2, 0, 0) = 200;                    // phase 2: the top-left corner
    t.px(3, 3, 4) = 7;                      // phase 3: the bottom-right corner of the box (column 4 of 5)
    t.px(5, 1, 1) = 50;                     // phase 5: ink, and never seen
    LearnRect r = learn_ink_rect(t.bitmaps.data() + 4 + 1 * CELL, BW, BH, STRIDE);
    CHECK(r.x0 == 2 && r.x1 == 4 && r.y0 == 1 && r.y1 == 3 && !r.empty());
    CHECK(learn_ink_rect(t.bitmaps.data() + 4, BW, BH, STRIDE).empty());
    LearnRect g = learn_grow_rect(r, 1, BW, BH);
    CHECK(g.x0 == 1 && g.x1 == 5 && g.y0 == 0 && g.y1 == 4);
    g = learn_grow_rect(r, 1000, BW, BH);
    CHECK(g.x0 == 0 && g.x1 == BW && g.y0 == 0 && g.y1 == BH);
    g = learn_grow_rect(learn_ink_rect(t.bitmaps.data() + 4 + 3 * CELL, BW, BH, STRIDE), 0xffffffffu, BW, BH);
    CHECK(g.x0 == 0 && g.x1 == BW && g.y0 == 0 && g.y1 == BH);
    CHECK(learn_grow_rect(LearnRect{}, 3, BW, BH).empty());  // no ink: nothing to grow

    // the learned bitmaps: phase 0 blank and seen, phases 1 .. 3 inked and seen, phase 5 inked and unseen, the rest blank and unseen
    for (uint32_t p : {0u, 1u, 2u, 3u}) t.fill_sums(p, 10 * (p + 1)), t.counts[p] = 4;  // means 2.5, 5, 7.5, 10: 3, 5, 8, 10
    std::vector<uint8_t> out;
    LearnStats st;
    CHECK(learn_font_bitmaps(t.f, t.sums.data(), t.counts.data(), 1, 0, &out, &st).empty());
    CHECK(st.inked == 4 && st.learned == 3 && out.size() == t.bitmaps.size());
    CHECK(at(out, 0, 0, 0) == 0 && at(out, 0, 2, 2) == 0);                                  // a blank phase stays blank
    CHECK(at(out, 1, 1, 2) == 5 && at(out, 1, 2, 3) == 5 && at(out, 1, 1, 3) == 5 && at(out, 1, 2, 2) == 5);
    CHECK(at(out, 1, 0, 2) == 0 && at(out, 1, 1, 1) == 0 && at(out, 1, 3, 3) == 0 && at(out, 1, 1, 4) == 0);  // outside the support: the base's
    CHECK(at(out, 2, 0, 0) == 8 && at(out, 2, 0, 1) == 0 && at(out, 2, 1, 0) == 0);
    CHECK(at(out, 3, 3, 4) == 10 && at(out, 3, 3, 3) == 0 && at(out, 3, 3, 5) == 0);         // column 5 is padding
    CHECK(at(out, 5, 1, 1) == 50);                                                          // a zero count: the base's
    CHECK(out[0] == 0 && out[3] == 0);
    // grow at the box's edge: the corner phases grow inwards only, and never into the padding columns
    CHECK(learn_font_bitmaps(t.f, t.sums.data(), t.counts.data(), 1, 1, &out, &st).empty());
    CHECK(at(out, 2, 0, 0) == 8 && at(out, 2, 0, 1) == 8 && at(out, 2, 1, 1) == 8 && at(out, 2, 2, 0) == 0 && at(out, 2, 0, 2) == 0);
    CHECK(at(out, 3, 3, 4) == 10 && at(out, 3, 2, 3) == 10 && at(out, 3, 3, 5) == 0 && at(out, 3, 2, 5) == 0 && at(out, 3, 1, 4) == 0);
    CHECK(at(out, 1, 0, 1) == 5 && at(out, 1, 3, 4) == 5 && at(out, 1, 0, 0) == 0);
    CHECK(st.inked == 4 && st.learned == 3);
    // the min_count edge: a count of 4 is learned at 4 and not at 5
    CHECK(learn_font_bitmaps(t.f, t.sums.data(), t.counts.data(), 4, 0, &out, &st).empty() && st.learned == 3 && at(out, 1, 1, 2) == 5);
    CHECK(learn_font_bitmaps(t.f, t.sums.data(), t.counts.data(), 5, 0, &out, &st).empty() && st.learned == 0 && at(out, 1, 1, 2) == 9 && out == t.bitmaps);
    t.counts[1] = 5, t.sum(1, 1, 2) = 255 * 5;
    CHECK(learn_font_bitmaps(t.f, t.sums.data(), t.counts.data(), 5, 0, &out, &st).empty() && st.learned == 1 && at(out, 1, 1, 2) == 255 && at(out, 1, 2, 3) == 4);
    // refusals
    CHECK(learn_font_bitmaps(t.f, t.sums.data(), t.counts.data(), 0, 0, &out, &st) == "min_count must be at least 1");
    CHECK(learn_font_bitmaps(t.f, nullptr, t.counts.data(), 1, 0, &out, &st) == "null sums or counts");
    focr_decode_font_t bad = t.f;
    bad.bitmaps_len -= 1;
    CHECK(learn_font_bitmaps(bad, t.sums.data(), t.counts.data(), 1, 0, &out, &st) == "inconsistent glyph table");

    // focr_decoder_learn_text's own rules (text_plan.h)
    CHECK(plan_learn(0, 0, 0).empty() && plan_learn(3, 3, (1ull << 24) - 1).empty());
    CHECK(plan_learn(4, 3, 0) == "font 4 to learn with 3 candidates uploaded (focr_decoder_set_font_candidates)");
    CHECK(plan_learn(0, 0, 1ull << 24).find("2^24 or more listed characters") == 0 && !plan_learn(1, 2, ~0ull).empty());
    HostFont h;
    h.glyphs.push_back(t.glyph);
    CHECK(learn_boxes(h).size() == 1 && learn_boxes(h)[0].at == 4 && learn_boxes(h)[0].box_w == BW);

    if (failures) return 1;
    std::puts("learn font ok");
    return 0;
}
