// align_plan_check.cpp — the host plan of a forced alignment (align_plan.h) at the edges its arithmetic has, without a device: a
// stand-alone program, built with a host compiler under the sanitizers and run by tests/test_align_plan_host.py.  The fonts are
// filled by hand, origins and increments only: the plan reads nothing else of a font.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "align_plan.h"

using namespace focr_dec;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static HostFont font_of(float origin_x, std::vector<float> inc) {
    HostFont f;
    f.origin_x = origin_x, f.origin_y = 10.f;
    f.inc = std::move(inc);
    return f;
}

// A reading over the fonts 0 ..= 2: the decode font (increments 7.828125 = 501 / 64, 0.5 and one that rounds to even), candidate 1
// with the increments 1, 2 and 4 / 64 px, candidate 2 with a fractional origin_x.
struct Reading {
    std::vector<focr_text_line_t> lines;
    std::vector<uint16_t> chars;
    HostFont font = font_of(3.f, {7.828125f, 0.5f, 0.0390625f});  // inc64 501, 32, rint(2.5) = 2
    std::vector<HostFont> cands{font_of(0.f, {0.015625f, 0.03125f, 0.0625f}), font_of(2.5f, {1.f, 1.f, 1.f})};
    TextPlan text;
    AlignPlan plan;
    void line(uint64_t first, uint32_t n, uint32_t f = 0) { lines.push_back(focr_text_line_t{0, 0, first, n, f}); }
    std::string run(uint32_t start, uint32_t drift) {
        const TextInput in{lines.data(), lines.size(), chars.data(), nullptr, nullptr, chars.size(), 1};
        TextAsk ask;
        ask.pen_origin = true;
        std::string no = plan_text_lines(in, font, cands, ask, &text);
        if (no.empty()) no = plan_text_chars(in, 3);
        if (no.empty()) no = plan_align(in, text.recs, text.n_out, font, cands, start, drift, &plan);
        return no;
    }
};

int main() {
    const std::string pens = "start + the sum of its increments + drift is 2^24 / 64 px or more (pens must stay exact in f32)";
    {  // the radii: the maxima are accepted, one more is refused, the drift first
        CHECK(plan_align_radii(FOCR_ALIGN_DRIFT_MAX, FOCR_PEN_SEARCH_MAX).empty() && plan_align_radii(0, 0).empty());
        CHECK(plan_align_radii(FOCR_ALIGN_DRIFT_MAX + 1, 0) == "the drift radius is at most 1024 (16 pixels)");
        CHECK(plan_align_radii(0, FOCR_PEN_SEARCH_MAX + 1) == "the step radius is at most 64 (one pixel)");
        CHECK(plan_align_radii(~0u, ~0u) == "the drift radius is at most 1024 (16 pixels)");
    }
    {  // inc64: the multiply is exact, the rounding is to nearest even; an increment past every pen is capped, not cast
        CHECK(align_inc64(7.828125f) == 501 && align_inc64(0.0390625f) == 2 && align_inc64(0.0546875f) == 4 && align_inc64(0.001f) == 0);
        CHECK(align_inc64(262143.f) == ALIGN_PEN_END - 64);  // the last increments below the cap are whole multiples of 1/64 px
        CHECK(align_inc64(262144.f) == ALIGN_PEN_END && align_inc64(1e30f) == ALIGN_PEN_END && align_inc64(INFINITY) == ALIGN_PEN_END);
    }
    {  // no lines: accepted and empty, whatever start is
        Reading r;
        CHECK(r.run(~0u, 1024).empty() && r.plan.recs.empty() && r.plan.nominal.empty() && r.plan.back_bytes == 0);
    }
    {  // nominal pens per line from the line's own font, at the running sum; lines share characters; an empty line
        Reading r;
        r.chars = {0, 1, 2, 0, 1};
        r.line(0, 5);
        r.line(1, 3, 1);
        r.line(2, 0);
        r.line(3, 2);
        CHECK(r.run(200, 3).empty());
        CHECK(r.plan.nominal == (std::vector<uint32_t>{200, 701, 733, 735, 1236, 200, 202, 206, 200, 701}));
        CHECK(r.plan.back_bytes == 10 * 7 && r.plan.recs.size() == 4);
        const uint64_t backs[4] = {0, 35, 56, 56};
        for (size_t l = 0; l < 4 && l < r.plan.recs.size(); l++) CHECK(r.plan.recs[l].back == backs[l]);
        CHECK(r.run(0, 0).empty() && r.plan.nominal[0] == 0 && r.plan.nominal[4] == 1036 && r.plan.back_bytes == 10 && r.plan.recs[1].back == 5);
    }
    {  // the 2^24 rule: start + the sum over the whole line + W, the last sum accepted and the first refused
        Reading r;
        r.chars = {0, 0};  // 1002 in all
        r.line(0, 2);
        const uint32_t top = ALIGN_PEN_END - 1002;
        CHECK(r.run(top - 1 - 64, 64).empty() && r.plan.nominal[1] == top - 1 - 64 + 501);
        CHECK(r.run(top - 64, 64) == "line 0: " + pens);
        CHECK(r.run(top - 1, 0).empty());
        CHECK(r.run(top, 0) == "line 0: " + pens);
        CHECK(r.run(~0u, 0) == "line 0: " + pens && r.run(~0u, 1024) == "line 0: " + pens);  // start + W would wrap in 32 bits
        r.lines[0].n_chars = 0;  // a line without characters still has a band around start
        CHECK(r.run(ALIGN_PEN_END - 1, 0).empty() && r.run(ALIGN_PEN_END - 1, 1) == "line 0: " + pens);
        r.line(0, 2);
        CHECK(r.run(top, 0) == "line 1: " + pens);
    }
    {  // a long line of a large increment: the sum is left as soon as it passes, far below any wrap
        Reading r;
        r.font.inc[0] = 1e30f;
        r.chars.assign(70000, 0);
        r.line(0, 70000);
        CHECK(r.run(0, 0) == "line 0: " + pens);
        r.font.inc[0] = 0.001f;  // inc64 0: every character at start
        CHECK(r.run(5, 2).empty() && r.plan.nominal.front() == 5 && r.plan.nominal.back() == 5 && r.plan.back_bytes == 350000);
    }
    {  // origin_x: whole in the line's own font
        Reading r;
        r.chars = {0};
        r.line(0, 1, 1);
        r.line(0, 1, 2);
        CHECK(r.run(0, 1) == "line 1: an alignment needs its font's origin_x to be a whole number >= 0 (at most 65536)");
        r.lines[1].font = 0;
        CHECK(r.run(0, 1).empty());
        r.font.origin_x = -1.f;
        CHECK(r.run(0, 1) == "line 1: an alignment needs its font's origin_x to be a whole number >= 0 (at most 65536)");
    }
    {  // the backpointers' budget: n_out * (2W + 1) <= 256 MiB exactly, by the quotient; refused before the plan allocates
        Reading r;
        r.font.inc[0] = 0.001f;
        r.chars.assign(65536, 0);
        const uint64_t band = 2049, most = ALIGN_BACK_MAX / band;  // 131008 characters
        r.line(0, 65536);
        r.line(0, (uint32_t)(most - 65536));
        CHECK(r.run(0, 1024).empty() && r.text.n_out == most && r.plan.back_bytes == most * band && r.plan.back_bytes <= ALIGN_BACK_MAX);
        r.line(0, 1);
        const std::string no = r.run(0, 1024);
        CHECK(no == "the backpointers of the call (131009 characters x 2049 states) pass 256 MiB: list fewer lines or ask for less drift");
        CHECK(r.plan.nominal.empty() && r.plan.recs.empty());
        CHECK(r.run(0, 1023).empty());
        // the largest call text_plan.h lets through, 2^32 - 1 characters: no product wraps
        r.lines.clear();
        for (int l = 0; l < 65535; l++) r.line(0, 65536);
        r.line(0, 65535);
        CHECK(r.run(0, 1024) == "the backpointers of the call (4294967295 characters x 2049 states) pass 256 MiB: list fewer lines or ask for less drift");
        CHECK(r.run(0, 0) == "the backpointers of the call (4294967295 characters x 1 states) pass 256 MiB: list fewer lines or ask for less drift");
    }
    {  // what text_plan.h refuses comes first
        Reading r;
        r.chars = {0, 3};
        r.line(0, 2);
        CHECK(r.run(0, 0) == "character 1 is not an index into the alphabet");
        r.lines[0].font = 3;
        CHECK(r.run(0, 0) == "line 0: font 3 with 2 candidates uploaded (focr_decoder_set_font_candidates)");
    }
    static_assert(sizeof(AlignRec) == 8, "the record the kernel reads");
    if (failures) return 1;
    std::puts("align plan ok");
    return 0;
}
