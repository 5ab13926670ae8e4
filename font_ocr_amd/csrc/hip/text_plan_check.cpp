// text_plan_check.cpp — the input rules of a caller's reading (text_plan.h) at the edges their arithmetic has, without a device: a
// stand-alone program, built with a host compiler under the sanitizers and run by tests/test_text_plan_host.py.  The fonts are
// filled by hand, origins only: the plan reads nothing else of a font.
#include <cstdio>
#include <cstdlib>
#include <vector>

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

static HostFont origin(float x, float y) {
    HostFont f;
    f.origin_x = x, f.origin_y = y;
    return f;
}

// A reading over the fonts 0 ..= 2: the decode font and candidate 1 with whole origins, candidate 2 with neither whole.
struct Reading {
    std::vector<focr_text_line_t> lines;
    std::vector<uint16_t> chars;
    std::vector<uint32_t> pens;
    std::vector<int8_t> qs;
    size_t n_pages = 1;
    HostFont font = origin(3.f, 10.f);
    std::vector<HostFont> cands{origin(0.f, 12.f), origin(2.5f, 9.25f)};
    TextPlan plan;
    void line(uint32_t page, uint64_t first, uint32_t n, uint32_t f = 0, uint32_t y = 0) { lines.push_back(focr_text_line_t{page, y, first, n, f}); }
    TextInput in() const { return TextInput{lines.data(), lines.size(), chars.data(), pens.empty() ? nullptr : pens.data(), nullptr, chars.size(), n_pages}; }
    std::string run(bool page_order, bool score = false, uint32_t y_bits = 0) {
        TextAsk ask;
        ask.page_order = page_order;
        ask.pen_origin = score;
        ask.line_q = score && !qs.empty() ? qs.data() : nullptr;
        ask.y_bits = y_bits;
        return plan_text_lines(in(), font, cands, ask, &plan);
    }
};

int main() {
    const std::string past = "its characters end past n_chars";
    {  // no lines: accepted, nothing used, and every page's range is empty
        Reading r;
        r.n_pages = 3;
        CHECK(r.run(true).empty());
        CHECK(r.plan.recs.empty() && r.plan.n_out == 0 && !r.plan.decode_font && !r.plan.candidates);
        CHECK(r.plan.page_first == std::vector<uint32_t>(4, 0));
        CHECK(r.run(false).empty() && r.plan.page_first.empty());
        CHECK(plan_text_chars(r.in(), 4).empty());
        r.n_pages = 0;
        CHECK(r.run(true).empty() && r.plan.page_first == std::vector<uint32_t>(1, 0));
    }
    {  // pages without lines in front, in the middle and at the end
        Reading r;
        r.n_pages = 6;
        r.chars.assign(4, 0);
        r.line(1, 0, 4);
        r.line(1, 0, 2);
        r.line(4, 1, 3);
        CHECK(r.run(true).empty());
        CHECK(r.plan.page_first == (std::vector<uint32_t>{0, 0, 2, 2, 2, 3, 3}));
    }
    {  // two lines sharing characters: `out` is the running sum, not `first`; the record carries the caller's line
        Reading r;
        r.chars.assign(5, 0);
        r.line(0, 1, 4, 0, 7);
        r.line(0, 1, 4, 1, 9);
        r.line(0, 0, 0);
        r.line(0, 0, 5);
        CHECK(r.run(true).empty());
        CHECK(r.plan.n_out == 13 && r.plan.recs.size() == 4);
        const uint64_t outs[4] = {0, 4, 8, 8};
        for (size_t l = 0; l < 4 && l < r.plan.recs.size(); l++) {
            const TextRec &t = r.plan.recs[l];
            const focr_text_line_t &s = r.lines[l];
            CHECK(t.page == s.page && t.y == s.y && t.n == s.n_chars && t.font == s.font && t.first == s.first && t.out == outs[l] && t.q == 0 && t.pad == 0);
        }
    }
    {  // where a line's characters may end
        Reading r;
        r.line(0, 0, 0);  // first == n_chars == 0
        CHECK(r.run(true).empty());
        r.lines[0].first = 1;  // n_chars + 1
        CHECK(r.run(true) == "line 0: " + past);
        r.lines[0] = focr_text_line_t{0, 0, 1ull << 63, 0xffffffffu, 0};  // first + n wraps in no width the check uses
        CHECK(r.run(false) == "line 0: " + past);
        r.chars.assign(3, 0);
        r.lines[0] = focr_text_line_t{0, 0, 3, 0, 0};
        r.line(0, 2, 2);
        CHECK(r.run(true) == "line 1: " + past);
        r.lines[1].n_chars = 1;
        CHECK(r.run(true).empty());
    }
    {  // pages: page == n_pages is refused; page order only where asked for
        Reading r;
        r.n_pages = 2;
        r.line(1, 0, 0);
        r.line(0, 0, 0);
        CHECK(r.run(true) == "line 1: its page lies before the previous line's (lines come in page order)");
        CHECK(r.run(false).empty() && r.plan.recs[1].page == 0);
        r.lines[1].page = 2;
        CHECK(r.run(true) == "line 1: page 2 of 2");
        CHECK(r.run(false) == "line 1: page 2 of 2");
    }
    {  // fonts: K is accepted and K + 1 refused; the used-font flags
        Reading r;
        r.line(0, 0, 0, 0);
        CHECK(r.run(true).empty() && r.plan.decode_font && !r.plan.candidates);
        r.lines[0].font = 2;
        CHECK(r.run(true).empty() && !r.plan.decode_font && r.plan.candidates);
        r.line(0, 0, 0, 0);
        CHECK(r.run(true).empty() && r.plan.decode_font && r.plan.candidates);
        r.lines[1].font = 3;
        CHECK(r.run(true) == "line 1: font 3 with 2 candidates uploaded (focr_decoder_set_font_candidates)");
        r.cands.clear();
        r.lines[1].font = 0;
        CHECK(r.run(true) == "line 0: font 2 with 0 candidates uploaded (focr_decoder_set_font_candidates)");
    }
    {  // characters and pens
        Reading r;
        r.chars = {0, 3, 3, 1};
        CHECK(plan_text_chars(r.in(), 4).empty());
        r.chars[2] = 4;
        CHECK(plan_text_chars(r.in(), 4) == "character 2 is not an index into the alphabet");
        r.chars[2] = 0;
        r.pens = {0, (1u << 24) - 1, 5, 6};
        CHECK(plan_text_chars(r.in(), 4).empty());
        r.pens[3] = 1u << 24;
        CHECK(plan_text_chars(r.in(), 4) == "pen 3 is 2^24 or more (pens must stay exact in f32)");
        r.chars[1] = 9;  // the characters are looked at first
        CHECK(plan_text_chars(r.in(), 4) == "character 1 is not an index into the alphabet");
    }
    {  // 65 537 lines of 65 536 characters over one range: the running sum passes 2^32 - 1
        Reading r;
        r.chars.assign(65536, 0);
        for (int l = 0; l < 65535; l++) r.line(0, 0, 65536);
        r.line(0, 0, 65535);
        CHECK(r.run(true).empty() && r.plan.n_out == 0xffffffffull && r.plan.recs.back().out == (65535ull << 16));  // the last sum accepted
        r.line(0, 0, 1);
        CHECK(r.run(true) == "too many characters in one call");
        r.lines.pop_back();
        r.lines.back().n_chars = 65536;
        r.line(0, 0, 65536);
        CHECK(r.lines.size() == 65537 && r.run(false) == "too many characters in one call");
    }
    {  // score_text's q: whole steps in a candidate, a whole origin_y in any font
        Reading r;
        r.line(0, 0, 0, 1);
        r.qs = {-8};
        CHECK(r.run(false, true, 2).empty() && r.plan.recs[0].q == -8);
        r.qs = {-7};
        CHECK(r.run(false, true, 2) == "line 0: a fractional-phase q in a candidate font (the candidates have one vertical phase)");
        CHECK(r.run(false, true, 0).empty() && r.plan.recs[0].q == -7);  // y_bits 0: every q is whole
        CHECK(r.run(true, false, 2).empty() && r.plan.recs[0].q == 0);   // not asked for: not read
        r.lines[0].font = 0;
        CHECK(r.run(false, true, 2).empty() && r.plan.recs[0].q == -7);  // the decode font has its y-phases
        r.lines[0].font = 2;
        r.qs = {4};
        CHECK(r.run(false, true, 2) == "line 0: line_q needs its font's origin_y to be a whole number >= 0");
        r.qs.clear();
        CHECK(r.run(false, true, 2).empty());
    }
    {  // score_text's pens: a whole origin_x of the line's font
        Reading r;
        r.chars = {0};
        r.pens = {64};
        r.line(0, 0, 1, 1);
        r.line(0, 0, 1, 2);
        CHECK(r.run(false, true) == "line 1: pens need its font's origin_x to be a whole number >= 0 (at most 65536)");
        CHECK(r.run(true, false).empty());  // verify_text draws at any origin
        r.pens.clear();
        CHECK(r.run(false, true).empty());
        r.pens = {64};
        r.lines[1].font = 0;
        CHECK(r.run(false, true).empty());
        r.font.origin_x = 65537.f;
        CHECK(r.run(false, true) == "line 1: pens need its font's origin_x to be a whole number >= 0 (at most 65536)");
    }
    {  // the guards, in their order
        const focr_text_line_t l{0, 0, 0, 0, 0};
        const uint16_t c = 0;
        const uint32_t p = 0;
        const int8_t o = 0;
        const uint8_t page = 0;
        CHECK(text_guards(TextInput{&l, 1, &c, nullptr, nullptr, 1, 1}, &page, nullptr).empty());
        CHECK(text_guards(TextInput{nullptr, 0, nullptr, nullptr, nullptr, 0, 0}, nullptr, nullptr).empty());
        CHECK(text_guards(TextInput{nullptr, 1, nullptr, &p, &o, 1, 1}, nullptr, "out") == "null pages");
        CHECK(text_guards(TextInput{nullptr, 1, nullptr, &p, &o, 1, 1}, &page, "out") == "null lines");
        CHECK(text_guards(TextInput{&l, 1, nullptr, &p, &o, 1, 1}, &page, "out") == "null chars");
        CHECK(text_guards(TextInput{&l, 1, &c, &p, &o, 1, 1}, &page, "out") == "null out");
        CHECK(text_guards(TextInput{&l, 1, &c, &p, &o, 1, 1}, &page, nullptr) == "pens and offsets together (a character is placed by its pen or by its offset)");
    }
    static_assert(sizeof(TextRec) == 40, "the record the kernels read");
    if (failures) return 1;
    std::puts("text plan ok");
    return 0;
}
