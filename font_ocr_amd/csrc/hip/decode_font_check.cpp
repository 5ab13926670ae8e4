// decode_font_check.cpp — decode_font.h without a device: a stand-alone program, built under the sanitizers by
// tests/test_focr_font_tables_host.py (the Makefile's hip/*.hip wildcard does not pick it up).  It builds real tables of a
// 4-glyph alphabet with libfocr_raster.so, packs them as the five uploaders of the focr decoder do, and compares every record
// with the formulas restated here; then one bent copy per refusal, the order of two faults in one table, and whole_origin.
//   decode_font_check FONT.ttf   ->   "font tables ok"
#include <cstdio>
#include <limits>

#include "decode_font.h"

using namespace focr_dec;

#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                               \
        }                                                           \
    } while (0)

namespace {

constexpr int P = FOCR_DECODE_PHASES;
const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();

// A caller's table with glyph records of its own to bend; the bitmaps stay the original's.
struct Bent {
    focr_decode_font_t f;
    std::vector<focr_decode_glyph_t> g;
    explicit Bent(const focr_decode_font_t &s) : f(s), g(s.glyphs, s.glyphs + s.n_glyphs) { f.glyphs = g.data(); }
    Bent(const Bent &) = delete;
};

struct BentVerify {
    focr_verify_font_t f;
    std::vector<focr_verify_glyph_t> g;
    explicit BentVerify(const focr_verify_font_t &s) : f(s), g(s.glyphs, s.glyphs + s.n_glyphs) { f.glyphs = g.data(); }
    BentVerify(const BentVerify &) = delete;
};

uint64_t term_bound(const focr_decode_glyph_t &s) { return 2ull * s.stride * s.box_h * (255 * 255); }

// The records of font f packed at byte `base`, as out holds them from glyph `at` on.
int same_glyphs(const focr_decode_font_t &f, uint64_t base, const PackedGlyphs &out, size_t at) {
    CHECK(out.glyphs.size() >= at + f.n_glyphs && out.offs.size() == out.glyphs.size() * P);
    for (size_t i = 0; i < f.n_glyphs; i++) {
        const focr_decode_glyph_t &s = f.glyphs[i];
        const DevGlyph &d = out.glyphs[at + i];
        CHECK(d.off_dw == (base + s.offset) / 4 && d.ndw == s.stride / 4 && d.box_h == s.box_h && same_bits(d.inc, s.increment));
        for (int p = 0; p < P; p++) CHECK(out.offs[(at + i) * P + p].x == s.off_x[p] && out.offs[(at + i) * P + p].y == s.off_y[p]);
    }
    return 0;
}

int same_record(const focr_decode_font_t &f, uint64_t base, const HostFont &h) {
    float lo = f.glyphs[0].increment;
    uint64_t T = 0;
    CHECK(h.glyphs.size() == f.n_glyphs && h.inc.size() == f.n_glyphs);
    for (size_t i = 0; i < f.n_glyphs; i++) {
        lo = std::min(lo, f.glyphs[i].increment), T = std::max(T, term_bound(f.glyphs[i]));
        CHECK(same_bits(h.inc[i], f.glyphs[i].increment) && !memcmp(&h.glyphs[i], &f.glyphs[i], sizeof(focr_decode_glyph_t)));
    }
    CHECK(same_bits(h.min_inc, lo) && h.term_bound == T && h.base == base && h.end_dw == (base + f.bitmaps_len) / 4 && h.bitmaps_len == f.bitmaps_len);
    CHECK(same_bits(h.origin_x, f.origin_x) && same_bits(h.origin_y, f.origin_y) && same_bits(h.text_size, f.text_size) && same_bits(h.kerning, f.kerning));
    CHECK(h.hinting == f.hinting);
    return 0;
}

int same_verify(const focr_verify_font_t &v, const focr_decode_font_t &f, uint64_t base, const PackedVerify &out, size_t at, int *y_lo, int *y_hi) {
    CHECK(out.glyphs.size() >= at + v.n_glyphs && out.phases.size() == out.glyphs.size() * P);
    for (size_t i = 0; i < v.n_glyphs; i++) {
        const focr_verify_glyph_t &s = v.glyphs[i];
        const focr_decode_glyph_t &d = f.glyphs[i];
        CHECK(!memcmp(out.glyphs[at + i].box, s.box, sizeof s.box));
        *y_lo = std::min(*y_lo, (int)floorf(s.box[1])), *y_hi = std::max(*y_hi, (int)ceilf(s.box[3]));
        for (int p = 0; p < P; p++) {
            const VerifyPhase &ph = out.phases[(at + i) * P + p];
            CHECK(ph.x == d.off_x[p] + (int)s.rect_x[p] && ph.y == d.off_y[p] + (int)s.rect_y[p] - (int)v.origin_y);
            CHECK(ph.w == s.rect_w[p] && ph.h == s.rect_h[p] && ph.stride == d.stride);
            CHECK(ph.src == base + d.offset + (uint64_t)p * d.stride * d.box_h + (uint64_t)s.rect_y[p] * d.stride + s.rect_x[p]);
        }
    }
    return 0;
}

// ---- each uploader's pack, with fresh outputs: the refusal, or "" ----

std::string set_font(const focr_decode_font_t &f) {
    HostFont h;
    PackedGlyphs out;
    return pack_font(f, nullptr, &h, &out);
}

std::string set_baseline(const focr_decode_font_t *fonts, size_t n, const HostFont &font) {
    PackedGlyphs out;
    uint64_t bound = 0;
    return pack_baseline_fonts(fonts, n, font, &bound, &out);
}

std::string set_candidates(const focr_decode_font_t *fonts, size_t n, const HostFont &font) {
    std::vector<HostFont> cands;
    PackedGlyphs out;
    return pack_candidate_fonts(fonts, n, font, &cands, &out);
}

std::string set_verify(const focr_verify_font_t &v, const HostFont &font, bool candidate = false) {
    PackedVerify out;
    return pack_verify_font(v, font, candidate, &out);
}

const std::string ADVANCE = "a glyph does not advance the pen", TABLE = "inconsistent glyph table", LARGE = "bitmap tables too large";
const std::string Y_COUNT = "a font does not match the decode font (glyph count)", Y_HEAD = "a font does not match the decode font (origin, size, kerning or hinting)",
                  Y_GLYPH = "a font does not match the decode font (code points or increments)", Y_FIRST = "fonts[0] is not the decode font (glyph table)";
const std::string C1 = "candidate 1: ", C2 = "candidate 2: ";

// The faults of one glyph's record that every decode-font uploader sees: `bend` changes glyph i of a fresh copy, `run` uploads it.
template <class Run>
int glyph_faults(const focr_decode_font_t &font, size_t i, const std::string &advance, const std::string &table, Run run) {
    const focr_decode_glyph_t &g = font.glyphs[i];
    const uint64_t phase = (uint64_t)g.stride * g.box_h;
    CHECK(phase > 0 && font.bitmaps_len >= P * phase);
    const auto with = [&](auto bend) {
        Bent b(font);
        bend(b.g[i], b.f);
        return run(b.f);
    };
    CHECK(with([](auto &, auto &) {}).empty());
    CHECK(with([](auto &s, auto &) { s.increment = 0.f; }) == advance);
    CHECK(with([](auto &s, auto &) { s.increment = -0.f; }) == advance);
    CHECK(with([](auto &s, auto &) { s.increment = -4.f; }) == advance);
    CHECK(with([](auto &s, auto &) { s.increment = NaN; }) == advance);
    CHECK(with([](auto &s, auto &) { s.stride += 1; }) == table);
    CHECK(with([](auto &s, auto &) { s.stride += 2; }) == table);
    CHECK(with([](auto &s, auto &) { s.box_w = s.stride + 1; }) == table);
    CHECK(with([](auto &s, auto &) { s.box_w = s.stride; }).empty());
    CHECK(with([](auto &s, auto &) { s.offset += 2; }) == table);
    CHECK(with([&](auto &s, auto &f) { s.offset = f.bitmaps_len - (P - 1) * phase; }) == table);  // one phase past the end
    CHECK(with([&](auto &s, auto &f) { s.offset = f.bitmaps_len - P * phase; }).empty());           // ... and the last that fits
    CHECK(with([](auto &s, auto &) { s.offset = ~0ull - 3; }) == table);                             // offset + phases wraps
    // the int32 term limit, in a table long enough to hold the box (lengths only: no byte of it is read)
    CHECK(with([](auto &s, auto &f) { s.offset = 0, s.box_w = 1, s.stride = 4, s.box_h = 4129, f.bitmaps_len = 1ull << 21; }) == table);  // 2^31 and above
    CHECK(with([](auto &s, auto &f) { s.offset = 0, s.box_w = 1, s.stride = 4, s.box_h = 4128, f.bitmaps_len = 1ull << 21; }).empty());   // the largest below
    CHECK(with([](auto &s, auto &f) { s.offset = 0, s.box_w = 1, s.stride = 1u << 31, s.box_h = 1u << 31, f.bitmaps_len = 1ull << 21; }) == table);  // products past 2^64
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const uint32_t alphabet[4] = {'a', 'n', 'H', ' '};
    char err[256] = "";
    focr_decode_font_t ys[4], c9, c8h;
    focr_verify_font_t v8, v9, v8h;
    CHECK(focr_decode_font_build_y(argv[1], 8.f, 0, 1.f, alphabet, 4, 2, ys, err, sizeof err) == 0);
    CHECK(focr_decode_font_build(argv[1], 9.f, 0, 1.f, alphabet, 4, &c9, err, sizeof err) == 0);
    CHECK(focr_decode_font_build(argv[1], 8.f, 1, 1.f, alphabet, 4, &c8h, err, sizeof err) == 0);
    CHECK(focr_verify_font_build(argv[1], 8.f, 0, 1.f, alphabet, 4, &v8, err, sizeof err) == 0);
    CHECK(focr_verify_font_build(argv[1], 9.f, 0, 1.f, alphabet, 4, &v9, err, sizeof err) == 0);
    CHECK(focr_verify_font_build(argv[1], 8.f, 1, 1.f, alphabet, 4, &v8h, err, sizeof err) == 0);
    const focr_decode_font_t &d8 = ys[0];
    const focr_decode_font_t cs[2] = {c9, c8h};

    // ---- packing: the decode font, its y-phases at a running base, two candidates at a running base, the verify tables ----
    HostFont font;
    {
        PackedGlyphs out;
        CHECK(pack_font(d8, nullptr, &font, &out).empty());
        CHECK(out.glyphs.size() == 4 && out.bytes == d8.bitmaps_len && !same_glyphs(d8, 0, out, 0) && !same_record(d8, 0, font));
    }
    {
        PackedGlyphs out;
        uint64_t bound = 0, base = 0, T = 0;
        CHECK(pack_baseline_fonts(ys, 4, font, &bound, &out).empty());
        CHECK(out.glyphs.size() == 3 * 4);
        for (size_t v = 1; v < 4; v++) {
            CHECK(!same_glyphs(ys[v], base, out, (v - 1) * 4));
            for (size_t i = 0; i < 4; i++) T = std::max(T, term_bound(ys[v].glyphs[i]));
            base += ys[v].bitmaps_len;
        }
        CHECK(out.bytes == base && bound == T && base > ys[1].bitmaps_len);
        PackedGlyphs one;
        CHECK(pack_baseline_fonts(ys, 1, font, &bound, &one).empty() && one.glyphs.empty() && one.offs.empty() && one.bytes == 0);  // y_bits 0
    }
    std::vector<HostFont> cands;
    {
        PackedGlyphs out;
        CHECK(pack_candidate_fonts(cs, 2, font, &cands, &out).empty());
        const uint64_t total = out.bytes;
        CHECK(cands.size() == 2 && out.glyphs.size() == 2 * 4 && total == c9.bitmaps_len + c8h.bitmaps_len);
        CHECK(!same_glyphs(c9, 0, out, 0) && !same_record(c9, 0, cands[0]));
        CHECK(!same_glyphs(c8h, c9.bitmaps_len, out, 4) && !same_record(c8h, c9.bitmaps_len, cands[1]));
        CHECK(cands[1].end_dw == total / 4 && cands[0].min_inc > font.min_inc);
    }
    {
        PackedVerify out;
        int y_lo = 0, y_hi = 0;
        CHECK(pack_verify_font(v8, font, false, &out).empty());
        CHECK(out.glyphs.size() == 4 && !same_verify(v8, d8, 0, out, 0, &y_lo, &y_hi) && out.y_lo == y_lo && out.y_hi == y_hi && y_hi - y_lo >= 6);
        PackedVerify both;
        const focr_verify_font_t vs[2] = {v9, v8h};
        CHECK(pack_verify_fonts(vs, cands, &both).empty() && both.glyphs.size() == 2 * 4);
        CHECK(!same_verify(v9, c9, 0, both, 0, &y_lo, &y_hi) && !same_verify(v8h, c8h, c9.bitmaps_len, both, 4, &y_lo, &y_hi));
    }

    // ---- one bent copy per refusal ----
    CHECK(!glyph_faults(d8, 1, ADVANCE, TABLE, [&](const focr_decode_font_t &f) { return set_font(f); }));
    CHECK(!glyph_faults(ys[2], 1, Y_GLYPH, TABLE, [&](const focr_decode_font_t &f) {
        const focr_decode_font_t fs[4] = {ys[0], ys[1], f, ys[3]};
        return set_baseline(fs, 4, font);
    }));
    CHECK(!glyph_faults(c8h, 2, C2 + ADVANCE, C2 + TABLE, [&](const focr_decode_font_t &f) {
        const focr_decode_font_t fs[2] = {c9, f};
        return set_candidates(fs, 2, font);
    }));
    {  // the tables as a whole
        Bent b(d8);
        b.f.n_glyphs = 65536;
        CHECK(set_font(b.f) == "more than 65535 glyphs");
        b.f.n_glyphs = 4, b.f.bitmaps_len -= 1;
        CHECK(set_font(b.f) == "bad bitmap table");
        b.f.bitmaps_len = 4ull * 0xffffffffull + 4;  // one dword more than 32 bits of them: lengths only
        CHECK(set_font(b.f) == "bad bitmap table");
        b.f.bitmaps_len = 4ull * 0xffffffffull;
        CHECK(set_font(b.f).empty() && table_fits(4ull * 0xffffffffull + 3) && !table_fits(4ull * 0xffffffffull + 4));
        Bent big1(c9);
        big1.f.bitmaps_len = (4ull << 32) - c8h.bitmaps_len;  // a running total of 2^32 dwords
        const focr_decode_font_t fs[2] = {big1.f, c8h};
        CHECK(set_candidates(fs, 2, font) == LARGE);
        big1.f.bitmaps_len -= 4;
        const focr_decode_font_t fits[2] = {big1.f, c8h};
        std::vector<HostFont> hs;
        PackedGlyphs out;
        CHECK(pack_candidate_fonts(fits, 2, font, &hs, &out).empty() && hs[1].end_dw == 0xffffffffu && hs[1].base == big1.f.bitmaps_len);
        CHECK(out.glyphs[4 + 1].off_dw == (big1.f.bitmaps_len + c8h.glyphs[1].offset) / 4);
        Bent y2(ys[2]);
        y2.f.bitmaps_len = (4ull << 32) - ys[1].bitmaps_len - ys[3].bitmaps_len;
        const focr_decode_font_t yl[4] = {ys[0], ys[1], y2.f, ys[3]};
        CHECK(set_baseline(yl, 4, font) == LARGE);
        y2.f.bitmaps_len -= 4;
        const focr_decode_font_t yf[4] = {ys[0], ys[1], y2.f, ys[3]};
        CHECK(set_baseline(yf, 4, font).empty());
    }
    {  // the y-phase fonts against the decode font
        const auto with = [&](size_t v, auto bend) {
            Bent b(ys[v]);
            bend(b.f, b.g);
            focr_decode_font_t fs[4] = {ys[0], ys[1], ys[2], ys[3]};
            fs[v] = b.f;
            return set_baseline(fs, 4, font);
        };
        CHECK(with(1, [](auto &f, auto &) { f.n_glyphs = 3; }) == Y_COUNT);
        CHECK(with(1, [](auto &f, auto &) { f.glyphs = nullptr; }) == Y_COUNT);
        CHECK(with(3, [](auto &f, auto &) { f.bitmaps_len -= 2; }) == Y_COUNT);
        CHECK(with(3, [](auto &f, auto &) { f.bitmaps = nullptr; }) == Y_COUNT);
        CHECK(with(2, [&](auto &f, auto &) { f.origin_x = -font.origin_x; }) == Y_HEAD);  // -0.0f against 0.0f: bits, not values
        CHECK(font.origin_x == 0.f && -font.origin_x == font.origin_x);
        CHECK(with(2, [](auto &f, auto &) { f.origin_y += 1.f; }) == Y_HEAD);
        CHECK(with(2, [](auto &f, auto &) { f.text_size = 9.f; }) == Y_HEAD);
        CHECK(with(2, [](auto &f, auto &) { f.kerning = 1.5f; }) == Y_HEAD);
        CHECK(with(0, [](auto &f, auto &) { f.hinting = 2; }) == Y_HEAD);
        CHECK(with(1, [](auto &, auto &g) { g[3].codepoint += 1; }) == Y_GLYPH);
        CHECK(with(1, [](auto &, auto &g) { g[0].increment = nextafterf(g[0].increment, 0.f); }) == Y_GLYPH);
        CHECK(with(0, [](auto &, auto &g) { g[1].off_x[0] += 1; }) == Y_FIRST);
        CHECK(with(0, [](auto &, auto &g) { g[1].off_y[P - 1] -= 1; }) == Y_FIRST);
        CHECK(with(0, [](auto &, auto &g) { g[2].box_w -= 1; }) == Y_FIRST);
        CHECK(with(1, [](auto &, auto &g) { g[1].off_x[0] += 1; }).empty());  // the other y-phases have boxes of their own
        // two faults: the font's head before its glyphs, a glyph's match before its table, its table before fonts[0]'s comparison,
        // and an earlier font or glyph before a later one
        CHECK(with(1, [](auto &f, auto &g) { f.n_glyphs = 5, f.kerning = 2.f, g[0].stride = 3; }) == Y_COUNT);
        CHECK(with(1, [](auto &f, auto &g) { f.kerning = 2.f, g[0].codepoint = 7; }) == Y_HEAD);
        CHECK(with(1, [](auto &, auto &g) { g[1].codepoint = 7, g[1].stride += 1; }) == Y_GLYPH);
        CHECK(with(1, [](auto &, auto &g) { g[1].stride += 1, g[2].codepoint = 7; }) == TABLE);
        CHECK(with(0, [](auto &, auto &g) { g[1].offset += 2; }) == TABLE);
        CHECK(with(0, [](auto &, auto &g) { g[0].box_w -= 1, g[1].stride += 1; }) == Y_FIRST);
        Bent z(ys[0]), y(ys[2]);
        z.g[3].off_x[5] += 1, y.f.n_glyphs = 2;
        const focr_decode_font_t fs[4] = {z.f, ys[1], y.f, ys[3]};
        CHECK(set_baseline(fs, 4, font) == Y_FIRST);
        // an increment of 0.0f in the decode font's record (no upload leaves one) against -0.0f: they differ
        HostFont zero = font;
        zero.glyphs[1].increment = 0.f;
        Bent nz(ys[0]);
        nz.g[1].increment = -0.f;
        CHECK(set_baseline(&nz.f, 1, zero) == Y_GLYPH);
        nz.g[1].increment = 0.f;
        CHECK(set_baseline(&nz.f, 1, zero).empty());
    }
    {  // the candidates against the decode font
        const auto with = [&](size_t k, auto bend) {
            Bent b(cs[k]);
            bend(b.f, b.g);
            focr_decode_font_t fs[2] = {cs[0], cs[1]};
            fs[k] = b.f;
            return set_candidates(fs, 2, font);
        };
        CHECK(with(0, [](auto &f, auto &) { f.n_glyphs = 3; }) == C1 + "the glyph count differs from the decode font's");
        CHECK(with(1, [](auto &f, auto &) { f.glyphs = nullptr; }) == C2 + "the glyph count differs from the decode font's");
        CHECK(with(1, [](auto &f, auto &) { f.bitmaps_len += 1; }) == C2 + "bad bitmap table");
        CHECK(with(0, [](auto &f, auto &) { f.bitmaps = nullptr; }) == C1 + "bad bitmap table");
        CHECK(with(1, [](auto &, auto &g) { g[2].codepoint += 1; }) == C2 + "a code point differs from the decode font's");
        CHECK(with(0, [](auto &f, auto &g) { f.n_glyphs = 3, f.bitmaps_len += 1, g[0].codepoint = 7; }) == C1 + "the glyph count differs from the decode font's");
        CHECK(with(0, [](auto &f, auto &g) { f.bitmaps_len += 2, g[0].codepoint = 7; }) == C1 + "bad bitmap table");
        CHECK(with(1, [](auto &, auto &g) { g[1].codepoint = 7, g[1].increment = 0.f, g[1].stride += 1; }) == C2 + "a code point differs from the decode font's");
        CHECK(with(1, [](auto &, auto &g) { g[1].increment = 0.f, g[1].stride += 1; }) == C2 + ADVANCE);
        CHECK(with(1, [](auto &, auto &g) { g[1].stride += 1, g[2].codepoint = 7; }) == C2 + TABLE);
        CHECK(with(0, [](auto &f, auto &g) { f.bitmaps_len = 4ull << 32, g[0].offset = 0; }) == LARGE);  // no candidate is named
        Bent b1(c9), b2(c8h);
        b1.g[3].increment = -1.f, b2.f.n_glyphs = 1;
        const focr_decode_font_t fs[2] = {b1.f, b2.f};
        CHECK(set_candidates(fs, 2, font) == C1 + ADVANCE);
    }
    {  // the verify tables against their fonts, in both uploaders' words
        for (int candidate = 0; candidate < 2; candidate++) {
            const focr_verify_font_t &good = candidate ? v8h : v8;
            const HostFont &of = candidate ? cands[1] : font;
            const std::string whose = candidate ? "candidate" : "decode font";
            const std::string head = "the table does not match the " + whose + " (glyph count, size, kerning, hinting or origin)";
            const std::string glyph = "the table does not match the " + whose + " (code points or increments)";
            const std::string box = "bad glyph box", rect = "a phase rectangle leaves the " + whose + "'s box";
            const auto with = [&](auto bend) {
                BentVerify b(good);
                bend(b.f, b.g);
                return set_verify(b.f, of, candidate);
            };
            CHECK(with([](auto &, auto &) {}).empty());
            CHECK(with([](auto &f, auto &) { f.n_glyphs = 3; }) == head);
            CHECK(with([](auto &f, auto &) { f.glyphs = nullptr; }) == head);
            CHECK(with([](auto &f, auto &) { f.text_size += 0.25f; }) == head);
            CHECK(with([](auto &f, auto &) { f.kerning = 1.25f; }) == head);
            CHECK(with([](auto &f, auto &) { f.hinting = !f.hinting; }) == head);
            CHECK(with([](auto &f, auto &) { f.hinting = f.hinting ? 7 : 0; }).empty());  // a truth value
            CHECK(with([](auto &f, auto &) { f.origin_y += 1.f; }) == head);
            CHECK(with([](auto &f, auto &) { f.origin_y = NaN; }) == head);
            CHECK(with([](auto &, auto &g) { g[2].codepoint += 1; }) == glyph);
            CHECK(with([](auto &, auto &g) { g[2].increment = nextafterf(g[2].increment, 9.f); }) == glyph);
            for (int i = 0; i < 4; i++) {
                CHECK(with([&](auto &, auto &g) { g[1].box[i] = NaN; }) == box);
                CHECK(with([&](auto &, auto &g) { g[1].box[i] = i & 1 ? Inf : -Inf; }) == box);
                CHECK(with([&](auto &, auto &g) { g[1].box[i] = i & 1 ? 1048577.f : -1048577.f; }) == box);
            }
            CHECK(with([](auto &, auto &g) { g[1].box[0] = -1048576.f, g[1].box[2] = 1048576.f; }).empty());  // 2^20 itself
            const focr_decode_glyph_t &d = of.glyphs[1];
            CHECK(with([&](auto &, auto &g) { g[1].rect_x[5] = d.box_w - g[1].rect_w[5] + 1; }) == rect);
            CHECK(with([&](auto &, auto &g) { g[1].rect_x[5] = d.box_w - g[1].rect_w[5]; }).empty());
            CHECK(with([&](auto &, auto &g) { g[1].rect_y[63] = d.box_h - g[1].rect_h[63] + 1; }) == rect);
            CHECK(with([&](auto &, auto &g) { g[1].rect_y[63] = d.box_h - g[1].rect_h[63]; }).empty());
            CHECK(with([](auto &, auto &g) { g[1].rect_x[0] = ~0u, g[1].rect_w[0] = 2; }) == rect);  // x + w past 32 bits
            // two faults: the head, then glyph by glyph its match, its box, its rectangles
            CHECK(with([](auto &f, auto &g) { f.kerning = 2.f, g[0].codepoint = 7; }) == head);
            CHECK(with([](auto &, auto &g) { g[1].codepoint = 7, g[1].box[0] = NaN; }) == glyph);
            CHECK(with([](auto &, auto &g) { g[1].box[3] = Inf, g[1].rect_w[0] = 999; }) == box);
            CHECK(with([](auto &, auto &g) { g[0].rect_w[0] = 999, g[1].codepoint = 7; }) == rect);
            HostFont big = of;  // a font whose bitmaps end past 4 GiB: VerifyPhase::src is 32 bits (lengths only)
            big.end_dw = 0x40000001u;
            CHECK(set_verify(good, big, candidate) == (candidate ? "the candidates' bitmaps pass 4 GiB" : "decode font bitmaps over 4 GiB"));
            big.end_dw = 0x3fffffffu;
            CHECK(set_verify(good, big, candidate).empty());
        }
        BentVerify b1(v9), b2(v8h);
        b1.g[3].box[1] = NaN, b2.f.n_glyphs = 3;
        const focr_verify_font_t vs[2] = {b1.f, b2.f};
        PackedVerify out;
        CHECK(pack_verify_fonts(vs, cands, &out) == C1 + "bad glyph box");
        b1.g[3].box[1] = v9.glyphs[3].box[1];
        const focr_verify_font_t vs2[2] = {b1.f, b2.f};
        PackedVerify out2;
        CHECK(pack_verify_fonts(vs2, cands, &out2) == C2 + "the table does not match the candidate (glyph count, size, kerning, hinting or origin)");
    }

    // ---- whole_origin ----
    CHECK(!whole_origin(-1.f) && whole_origin(-0.f) && whole_origin(0.f) && !whole_origin(0.5f) && whole_origin(65536.f) && !whole_origin(65537.f));
    CHECK(!whole_origin(NaN) && !whole_origin(Inf) && whole_origin(7.f) && !whole_origin(nextafterf(65536.f, 0.f)));

    for (focr_decode_font_t &f : ys) focr_decode_font_free(&f);
    focr_decode_font_free(&c9), focr_decode_font_free(&c8h);
    focr_verify_font_free(&v8), focr_verify_font_free(&v9), focr_verify_font_free(&v8h);
    puts("font tables ok");
    return 0;
}
