// decode_font.h — the host's side of every font upload of the `focr` decoder, and nothing of the device's: what the host
// keeps of an uploaded font (HostFont), the records the kernels read of it (DevGlyph, VerifyGlyph, VerifyPhase), and the
// checks and the packing of a caller's tables, each stated once.  The five uploaders (focr_decoder_set_font,
// _set_baseline_fonts, _set_font_candidates, _set_verify_font, _set_verify_font_candidates) call the pack_* functions below; each
// returns the refusal's text behind the entry point's prefix (empty: none), in the order that entry point has always reported its
// faults.  Plain host code over HIP's vector types: decode_font_check.cpp runs it under the sanitizers, without hipcc or a device.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_vector_types.h>

#include "focr_decode.h"

namespace focr_dec {

struct DevGlyph {
    uint32_t off_dw;  // dword offset of phase 0 in the bitmap table
    uint32_t ndw;     // dwords per bitmap row
    uint32_t box_h;
    float inc;
};

struct VerifyGlyph {
    float box[4];      // raster_bounds at the identity before round_out (focr_verify_glyph_t::box)
};

struct VerifyPhase {
    int32_t x, y;      // top-left of the true bitmap on a line canvas at whole-pixel shift 0 and vertical translation 0
    uint32_t w, h;
    uint32_t src;      // byte offset of that top-left pixel in the bitmap table
    uint32_t stride;
};

// "A whole number in 0 ..= 65536": what the whole-line decode asks of origin_x and the baseline modes of origin_y.
inline bool whole_origin(float o) { return o >= 0.f && o <= 65536.f && o == floorf(o); }
inline bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof(float)) == 0; }

// The bound on the magnitude of a glyph's footprint term, c * (c - 2 r) summed over its box (a box of 2^32 px or more is
// above every limit: no product here wraps).
inline uint64_t glyph_term_bound(const focr_decode_glyph_t &s) {
    const uint64_t area = (uint64_t)s.stride * s.box_h;
    return area >> 32 ? ~0ull : area * 2 * 255 * 255;
}

// A glyph's record against the bitmap table of bitmaps_len bytes it points into: rows of whole dwords that hold the box,
// a dword-aligned offset, all 64 phases inside the table, and terms that fit the device's int32 scores.
inline bool glyph_consistent(const focr_decode_glyph_t &s, uint64_t bitmaps_len) {
    const uint64_t phases = (uint64_t)FOCR_DECODE_PHASES * s.stride * s.box_h;  // exact wherever the last clause holds
    return !(s.stride % 4 || s.stride < s.box_w || s.offset % 4 || s.offset > bitmaps_len || phases > bitmaps_len - s.offset ||
             glyph_term_bound(s) >= (1ull << 31));
}

// A bitmap table of this many bytes in all: the kernels address it in dwords, 32 bits of them.
inline bool table_fits(uint64_t bytes) { return bytes / 4 <= 0xffffffffull; }

// One uploaded font as the host keeps it: the decode font (font 0) or a candidate of the font search (1 ..= K); its tables
// are on the device.
struct HostFont {
    float origin_x = 0.f, origin_y = 0.f, text_size = 0.f, kerning = 0.f;
    int hinting = 0;
    float min_inc = 0.f;
    std::vector<float> inc;
    std::vector<focr_decode_glyph_t> glyphs;  // what a verify table is checked and placed against
    uint64_t term_bound = 0;  // the largest glyph_term_bound of its glyphs
    uint64_t base = 0;        // where its bitmaps start in the bitmap table it lies in, in bytes
    uint32_t end_dw = 0;      // ... and where they end, in dwords (footprint_term_wide's guard)
    size_t bitmaps_len = 0;

    HostFont() = default;
    HostFont(const focr_decode_font_t &f, uint64_t base)  // before its glyphs (f.glyphs[0] exists); add() takes them in order
        : origin_x(f.origin_x), origin_y(f.origin_y), text_size(f.text_size), kerning(f.kerning), hinting(f.hinting), min_inc(f.glyphs[0].increment),
          base(base), end_dw((uint32_t)((base + f.bitmaps_len) / 4)), bitmaps_len(f.bitmaps_len) {}
    void add(const focr_decode_glyph_t &s) {
        glyphs.push_back(s);
        inc.push_back(s.increment);
        min_inc = std::min(min_inc, s.increment);
        term_bound = std::max(term_bound, glyph_term_bound(s));
    }
};

// The glyph records and phase offsets of one device table set, font-major (glyph i of the set's font j at j * G + i), and
// the bytes of the fonts' bitmaps behind one another so far: where the next font's start.
struct PackedGlyphs {
    std::vector<DevGlyph> glyphs;
    std::vector<int2> offs;
    uint64_t bytes = 0;
    void add(const focr_decode_glyph_t &s) {  // a glyph of the font whose bitmaps start at `bytes`
        glyphs.push_back(DevGlyph{(uint32_t)((bytes + s.offset) / 4), s.stride / 4, s.box_h, s.increment});
        for (int p = 0; p < FOCR_DECODE_PHASES; p++) offs.push_back(make_int2(s.off_x[p], s.off_y[p]));
    }
};

// A font with increments of its own behind what *out holds, and its record: focr_decoder_set_font's (alphabet null; f.glyphs
// and f.n_glyphs are not), or a candidate of focr_decoder_set_font_candidates over the code points of the decode font `alphabet`.
inline std::string pack_font(const focr_decode_font_t &f, const HostFont *alphabet, HostFont *h, PackedGlyphs *out) {
    if (!alphabet && f.n_glyphs > 65535) return "more than 65535 glyphs";
    if (alphabet && (!f.glyphs || f.n_glyphs != alphabet->glyphs.size())) return "the glyph count differs from the decode font's";
    if (f.bitmaps_len % 4 || (alphabet ? f.bitmaps_len && !f.bitmaps : !table_fits(f.bitmaps_len))) return "bad bitmap table";
    *h = HostFont(f, out->bytes);
    for (size_t i = 0; i < f.n_glyphs; i++) {
        const focr_decode_glyph_t &s = f.glyphs[i];
        if (alphabet && s.codepoint != alphabet->glyphs[i].codepoint) return "a code point differs from the decode font's";
        if (!(s.increment > 0.f)) return "a glyph does not advance the pen";
        if (!glyph_consistent(s, f.bitmaps_len)) return "inconsistent glyph table";
        h->add(s);
        out->add(s);
    }
    out->bytes += f.bitmaps_len;
    return {};
}

// focr_decoder_set_font_candidates' fonts[0 .. n) in turn, in one bitmap table; a candidate's fault names it.
inline std::string pack_candidate_fonts(const focr_decode_font_t *fonts, size_t n, const HostFont &font, std::vector<HostFont> *cands, PackedGlyphs *out) {
    cands->assign(n, HostFont{});
    for (size_t k = 0; k < n; k++) {
        const std::string no = pack_font(fonts[k], &font, &(*cands)[k], out);
        if (!no.empty()) return "candidate " + std::to_string(k + 1) + ": " + no;
        if (!table_fits(out->bytes)) return "bitmap tables too large";
    }
    return {};
}

// focr_decoder_set_baseline_fonts' fonts[0 .. n) against the decode font: fonts[0] is that font itself and packs nothing; the
// y-phases v >= 1 are packed in one bitmap table, and *bound takes the largest term bound among them.
inline std::string pack_baseline_fonts(const focr_decode_font_t *fonts, size_t n, const HostFont &font, uint64_t *bound, PackedGlyphs *out) {
    for (size_t v = 0; v < n; v++) {
        const focr_decode_font_t &f = fonts[v];
        if (!f.glyphs || f.n_glyphs != font.glyphs.size() || f.bitmaps_len % 4 || (f.bitmaps_len && !f.bitmaps))
            return "a font does not match the decode font (glyph count)";
        if (!same_bits(f.origin_x, font.origin_x) || !same_bits(f.origin_y, font.origin_y) || !same_bits(f.text_size, font.text_size) ||
            !same_bits(f.kerning, font.kerning) || f.hinting != font.hinting)
            return "a font does not match the decode font (origin, size, kerning or hinting)";
        for (size_t i = 0; i < f.n_glyphs; i++) {
            const focr_decode_glyph_t &s = f.glyphs[i], &t = font.glyphs[i];
            if (s.codepoint != t.codepoint || !same_bits(s.increment, t.increment)) return "a font does not match the decode font (code points or increments)";
            if (!glyph_consistent(s, f.bitmaps_len)) return "inconsistent glyph table";
            if (v == 0) {
                if (s.box_w != t.box_w || s.box_h != t.box_h || s.stride != t.stride || s.offset != t.offset || memcmp(s.off_x, t.off_x, sizeof s.off_x) ||
                    memcmp(s.off_y, t.off_y, sizeof s.off_y))
                    return "fonts[0] is not the decode font (glyph table)";
                continue;
            }
            *bound = std::max(*bound, glyph_term_bound(s));
            out->add(s);
        }
        if (v) out->bytes += f.bitmaps_len;
        if (!table_fits(out->bytes)) return "bitmap tables too large";
    }
    return {};
}

// The box and phase records of one verify table set, font-major as PackedGlyphs, and the rows y_lo .. y_hi that render()
// gives any line of them.
struct PackedVerify {
    std::vector<VerifyGlyph> glyphs;
    std::vector<VerifyPhase> phases;
    int y_lo = 0, y_hi = 0;
};

// A verify table against the uploaded font it belongs to (focr_decoder_set_verify_font: the decode font;
// _set_verify_font_candidates: a candidate, in whose words the refusals then speak), behind those packed so far.
inline std::string pack_verify_font(const focr_verify_font_t &f, const HostFont &font, bool candidate, PackedVerify *out) {
    const std::string whose = candidate ? "candidate" : "decode font";
    if (!f.glyphs || f.n_glyphs != font.glyphs.size() || f.text_size != font.text_size || f.kerning != font.kerning ||
        (f.hinting != 0) != (font.hinting != 0) || f.origin_y != font.origin_y)
        return "the table does not match the " + whose + " (glyph count, size, kerning, hinting or origin)";
    if ((uint64_t)font.end_dw * 4 > 0xffffffffull) return candidate ? "the candidates' bitmaps pass 4 GiB" : "decode font bitmaps over 4 GiB";  // VerifyPhase::src
    for (size_t i = 0; i < f.n_glyphs; i++) {
        const focr_verify_glyph_t &v = f.glyphs[i];
        const focr_decode_glyph_t &d = font.glyphs[i];
        if (v.codepoint != d.codepoint || !same_bits(v.increment, d.increment)) return "the table does not match the " + whose + " (code points or increments)";
        for (float b : v.box)
            if (!std::isfinite(b) || std::fabs(b) > (float)(1 << 20)) return "bad glyph box";
        out->glyphs.push_back(VerifyGlyph{{v.box[0], v.box[1], v.box[2], v.box[3]}});
        out->y_lo = std::min(out->y_lo, (int)std::floor(v.box[1] + 0.f));
        out->y_hi = std::max(out->y_hi, (int)std::ceil(v.box[3] + 0.f));
        for (int p = 0; p < FOCR_DECODE_PHASES; p++) {
            if ((uint64_t)v.rect_x[p] + v.rect_w[p] > d.box_w || (uint64_t)v.rect_y[p] + v.rect_h[p] > d.box_h)
                return "a phase rectangle leaves the " + whose + "'s box";
            out->phases.push_back(VerifyPhase{d.off_x[p] + (int32_t)v.rect_x[p], d.off_y[p] + (int32_t)v.rect_y[p] - (int32_t)f.origin_y, v.rect_w[p], v.rect_h[p],
                                              (uint32_t)(font.base + d.offset + (uint64_t)p * d.stride * d.box_h + (uint64_t)v.rect_y[p] * d.stride + v.rect_x[p]),
                                              d.stride});
        }
    }
    return {};
}

// focr_decoder_set_verify_font_candidates' tables, one per candidate.
inline std::string pack_verify_fonts(const focr_verify_font_t *fonts, const std::vector<HostFont> &cands, PackedVerify *out) {
    for (size_t k = 0; k < cands.size(); k++) {
        const std::string no = pack_verify_font(fonts[k], cands[k], true, out);
        if (!no.empty()) return "candidate " + std::to_string(k + 1) + ": " + no;
    }
    return {};
}

}  // namespace focr_dec
