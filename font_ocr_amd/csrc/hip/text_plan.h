// text_plan.h — the input rules of a reading the caller supplies, stated once for the two entry points that take one:
// focr_decoder_verify_text (decode_text.hip) draws it, focr_decoder_score_text (decode_score.hip) costs it (and so do
// focr_decoder_align_text and focr_decoder_learn_text, whose own rules, align_plan.h's and plan_learn below, come on top).  Both take
// focr_text_line_t lines into one `chars` array, optional pens or offsets beside the characters, and any uploaded font per line.
// Here: the one record the device reads of a line (TextRec), the guards, the per-line checks with the running sum, and the
// per-character checks, as pure functions that return the refusal's text behind the entry point's prefix (empty: accepted), in the
// order each entry point has always reported its faults.  Plain host code, no HIP runtime and no decoder: text_plan_check.cpp
// asserts it at the edges of its arithmetic under the sanitizers with a host compiler alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "decode_font.h"
#include "focr_decode.h"

namespace focr_dec {

// One listed line as the device reads it: the caller's line, where its per-character results start (the glyph records of
// verify_text, the terms of score_text: a running sum of n over the list, since lines may share characters) and its baseline
// candidate q (0 without line_q).
struct TextRec {
    uint32_t page, y, n, font;
    uint64_t first, out;
    int32_t q;
    uint32_t pad;
};

struct TextInput {  // the caller's reading, as both entry points take it
    const focr_text_line_t *lines;
    size_t n_lines;
    const uint16_t *chars;
    const uint32_t *pens;   // null: none
    const int8_t *offsets;  // null: none
    size_t n_chars, n_pages;
};

struct TextAsk {  // what an entry point asks of the plan beyond the rules both share
    bool page_order = false;         // verify_text: lines come in page order, and the plan returns page_first
    const int8_t *line_q = nullptr;  // score_text: q per line in steps of 2^-y_bits px, with its two refusals
    uint32_t y_bits = 0;
    bool pen_origin = false;         // score_text: pens need a whole origin_x of the line's font
};

struct TextPlan {
    std::vector<TextRec> recs;
    std::vector<uint32_t> page_first;  // with page_order: page p's lines are [page_first[p], page_first[p + 1])
    uint64_t n_out = 0;                // the running sum: every line's characters, shared ones once per line
    bool decode_font = false, candidates = false;  // some line is in font 0 / in a candidate
};

// The null-pointer guards and the one placement per character; no_result names the entry point's missing output (null: it is there).
inline std::string text_guards(const TextInput &in, const void *pages, const char *no_result) {
    if (in.n_pages && !pages) return "null pages";
    if (in.n_lines && !in.lines) return "null lines";
    if (in.n_chars && !in.chars) return "null chars";
    if (no_result) return std::string("null ") + no_result;
    if (in.pens && in.offsets) return "pens and offsets together (a character is placed by its pen or by its offset)";
    return {};
}

// The lines in list order against the fonts 0 ..= K (font 0 is `font`, k >= 1 is cands[k - 1]): the records, the running sum
// and which fonts are used.
inline std::string plan_text_lines(const TextInput &in, const HostFont &font, const std::vector<HostFont> &cands, const TextAsk &ask, TextPlan *out) {
    const size_t K = cands.size();
    *out = TextPlan{};
    out->recs.resize(in.n_lines);
    if (ask.page_order) out->page_first.assign(in.n_pages + 1, 0);
    for (size_t l = 0; l < in.n_lines; l++) {
        const focr_text_line_t &s = in.lines[l];
        const std::string pre = "line " + std::to_string(l) + ": ";
        if (s.font > K) return pre + "font " + std::to_string(s.font) + " with " + std::to_string(K) + " candidates uploaded (focr_decoder_set_font_candidates)";
        if (s.page >= in.n_pages) return pre + "page " + std::to_string(s.page) + " of " + std::to_string(in.n_pages);
        if (ask.page_order && l && s.page < in.lines[l - 1].page) return pre + "its page lies before the previous line's (lines come in page order)";
        if (s.first > in.n_chars || s.n_chars > in.n_chars - s.first) return pre + "its characters end past n_chars";
        const HostFont &f = s.font ? cands[s.font - 1] : font;
        if (ask.pen_origin && in.pens && !whole_origin(f.origin_x)) return pre + "pens need its font's origin_x to be a whole number >= 0 (at most 65536)";
        const int q = ask.line_q ? ask.line_q[l] : 0;
        if (ask.line_q && s.font && (q & ((1 << ask.y_bits) - 1)))
            return pre + "a fractional-phase q in a candidate font (the candidates have one vertical phase)";
        if (ask.line_q && !whole_origin(f.origin_y)) return pre + "line_q needs its font's origin_y to be a whole number >= 0";
        (s.font ? out->candidates : out->decode_font) = true;
        out->recs[l] = TextRec{s.page, s.y, s.n_chars, s.font, s.first, out->n_out, q, 0};
        out->n_out += s.n_chars;  // below 2^31 lines of below 2^32 characters: no wrap
        if (ask.page_order) out->page_first[s.page + 1] = (uint32_t)(l + 1);
    }
    for (size_t p = 1; p < out->page_first.size(); p++) out->page_first[p] = std::max(out->page_first[p], out->page_first[p - 1]);  // a page without lines: an empty range
    if (out->n_out > 0xffffffffull) return "too many characters in one call";
    return {};
}

// The characters and pens, listed or not: every character an index into the alphabet of n_glyphs, every pen exact in f32.
inline std::string plan_text_chars(const TextInput &in, uint32_t n_glyphs) {
    for (size_t i = 0; i < in.n_chars; i++)
        if (in.chars[i] >= n_glyphs) return "character " + std::to_string(i) + " is not an index into the alphabet";
    for (size_t i = 0; in.pens && i < in.n_chars; i++)
        if (in.pens[i] >= (1u << 24)) return "pen " + std::to_string(i) + " is 2^24 or more (pens must stay exact in f32)";
    return {};
}

// One glyph of the font focr_decoder_learn_text learns, as its kernel reads it beside the glyph record: the box's columns (a
// DevGlyph has only the row's dwords) and where the glyph's phase 0 lies in the font's own `bitmaps`, which `sums` mirrors.
struct LearnGlyph {
    uint64_t at;
    uint32_t box_w, pad;
};

inline std::vector<LearnGlyph> learn_boxes(const HostFont &f) {
    std::vector<LearnGlyph> out;
    for (const focr_decode_glyph_t &s : f.glyphs) out.push_back(LearnGlyph{s.offset, s.box_w, 0});
    return out;
}

// focr_decoder_learn_text's two rules beyond the reading's own: the font to learn is one of 0 ..= K, and a sum of n_out samples
// of at most 255 each stays inside a uint32 (n_out is plan_text_lines' running sum: every listed character).
inline std::string plan_learn(uint32_t font, size_t K, uint64_t n_out) {
    if (font > K) return "font " + std::to_string(font) + " to learn with " + std::to_string(K) + " candidates uploaded (focr_decoder_set_font_candidates)";
    if (n_out >= (1ull << 24)) return "2^24 or more listed characters (a cell's sums are 32 bits wide: list fewer lines and add the calls up)";
    return {};
}

}  // namespace focr_dec
