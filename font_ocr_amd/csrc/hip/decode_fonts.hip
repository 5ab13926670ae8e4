// decode_fonts.hip — the font search of the `focr` line decoder (focr_decoder_set_font_candidates / _set_font_search; an
// extension, see include/focr_decode.h): every line is decoded once per candidate font k in 0 ..= K (0 is the decode font,
// 1 ..= K the uploaded ones: other sizes, kernings, hintings or faces over the same alphabet), and the candidate with the
// lowest summed footprint term is the line.
//
// line_fonts_kernel takes line_decode_kernel's place as the third launch of a run (decode.hip).  It is built as
// decode_baseline.hip's line_baseline_kernel is; one workgroup of four waves takes a work-list line (grid-stride, so a
// smaller grid takes several):
//   - the strip is staged in LDS once and shared by every candidate (when it fits; else it is read from global memory);
//   - wave w runs the plain pen loop (decode_pen.h) for the candidates w, w + 4, ... with each candidate's own tables,
//     increments and origin_x, and keeps only the lowest (cost, k);
//   - the four waves meet in LDS, and every wave works out the same winner;
//   - one wave decodes the winner once more and writes its characters: no trial buffers, and nothing depends on which
//     wave finished first.
// The uploaded candidates' tables lie concatenated (glyph records and phase offsets k-major, one bitmap table whose dword
// offsets the records carry); a descriptor per candidate (FontDesc, decode_line.h) says where its glyphs start, where its
// bitmaps end and what its origin is.  A wave's k is uniform, so the descriptor comes by scalar loads.
// Everything is exact integer arithmetic but the f32 pen, which is the plain loop's.
//
// Here as well: the upload of the candidates, the switch, the getter, and what both forms of the search (this one and
// decode_whole_fonts.hip's) share on the host: the descriptors of a run and the per-line result buffers.
#include <cstring>

#include "decode_pen.h"

namespace focr_dec {

constexpr uint32_t FONTS_THREADS = 256;  // one workgroup of four waves per work-list line
constexpr uint32_t FONTS_WAVES = FONTS_THREADS / 64;
constexpr uint32_t FONTS_RED_BYTES = FONTS_WAVES * 2 * 8;  // (cost, k) per wave, in front of the strip

// The fonts as a candidate reads them: k = 0 is the decode font, the others lie k-major in tables of their own.
struct FontTables {
    const DevGlyph *glyphs, *fglyphs;
    const int2 *offs, *foffs;
    const uint32_t *bitmaps, *fbitmaps;
    const FontDesc *desc;  // [n_fonts]
    uint32_t n_glyphs, n_fonts;  // K + 1
};

// pen_loop under candidate k of the fonts (k uniform across the wave).
template <bool WRITE>
__device__ __forceinline__ int64_t font_loop(const uint32_t *strip, uint32_t sdw, int w, uint32_t h, uint32_t cap, const FontTables &f, uint32_t k,
                                             uint32_t lane, uint16_t *__restrict__ out, uint32_t *__restrict__ n_out) {
    const FontDesc d = f.desc[k];
    const DevGlyph *glyphs = k ? f.fglyphs + d.glyph_base : f.glyphs;
    const int2 *offs = k ? f.foffs + (size_t)d.glyph_base * 64 : f.offs;
    return pen_loop<WRITE>(strip, sdw, w, h, cap, glyphs, offs, k ? f.fbitmaps : f.bitmaps, d.end_dw, f.n_glyphs, d.origin_x, 0, lane, out, n_out);
}

// 3f. the pen loop under every candidate font, one workgroup per work-list line (grid-stride).  n_fonts >= 2.
template <bool LDS>
__global__ __launch_bounds__(FONTS_THREADS) void line_fonts_kernel(const uint8_t *__restrict__ strips, Geometry g, const uint32_t *__restrict__ work,
                                                                   const uint32_t *__restrict__ count, FontTables f, uint32_t *__restrict__ n_chars,
                                                                   uint16_t *__restrict__ chars, uint32_t *__restrict__ line_font,
                                                                   int64_t *__restrict__ line_cost) {
    extern __shared__ __align__(8) uint32_t lds_fonts[];  // the waves' (cost, k), then (LDS) the strip
    uint64_t *red = (uint64_t *)lds_fonts;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));  // uniform, and the compiler knows it
    const uint32_t sdw = g.stride / 4, n_lines = *count;
    // the winner's decode goes to a wave that has one candidate fewer than wave 0 (wave 0 itself when all have as many)
    const uint32_t writer = f.n_fonts & (FONTS_WAVES - 1);
    for (uint32_t k = blockIdx.x; k < n_lines; k += gridDim.x) {
        const uint32_t slot = work[k];
        uint32_t yc, h;
        slot_rows(g, slot % g.n_slots, &yc, &h);
        const uint32_t *strip = (const uint32_t *)(strips + (size_t)slot * g.stride * g.line_height);
        if (LDS) {
            uint32_t *lds_strip = lds_fonts + FONTS_RED_BYTES / 4;
            for (uint32_t i = tid; i < sdw * h; i += FONTS_THREADS) lds_strip[i] = strip[i];
            __syncthreads();
            strip = lds_strip;
        }
        int64_t best_cost = INT64_MAX;
        uint32_t best_font = ~0u;  // a wave without a candidate: never the winner (wave 0 always has candidate 0)
        for (uint32_t c = wave; c < f.n_fonts; c += FONTS_WAVES) {
            const int64_t cost = font_loop<false>(strip, sdw, (int)g.w, h, g.cap, f, c, lane, nullptr, nullptr);
            if (cost < best_cost) best_cost = cost, best_font = c;  // a wave's candidates ascend: the first of equal costs stays
        }
        if (lane == 0) red[2 * wave] = (uint64_t)best_cost, red[2 * wave + 1] = best_font;
        __syncthreads();
        best_cost = (int64_t)red[0], best_font = (uint32_t)red[1];
        for (uint32_t v = 1; v < FONTS_WAVES; v++) {
            const int64_t c = (int64_t)red[2 * v];
            const uint32_t r = (uint32_t)red[2 * v + 1];
            if (c < best_cost || (c == best_cost && r < best_font)) best_cost = c, best_font = r;
        }
        if (wave == writer) {
            best_font = (uint32_t)__builtin_amdgcn_readfirstlane((int)best_font);
            const int64_t cost = font_loop<true>(strip, sdw, (int)g.w, h, g.cap, f, best_font, lane, chars + (size_t)k * g.cap, n_chars + k);
            if (lane == 0) line_font[k] = best_font, line_cost[k] = cost;
        }
        __syncthreads();  // the strip and the pairs are the next line's from here
    }
}

// ---- the host's side (decode_line.h) ---------------------------------------------------------------------------------

int fonts_plan(focr_decoder *dec, WholePlan *plan) {
    const uint32_t G = dec->n_glyphs;
    plan->fonts.assign(1 + dec->cands.size(), FontDesc{});
    for (size_t k = 0; k < plan->fonts.size(); k++)  // (glyph_base is in the candidates' tables: font 0 has its own)
        plan->fonts[k] = FontDesc{k ? (uint32_t)((k - 1) * G) : 0, dec->font_at(k).end_dw, dec->font_at(k).origin_x, 0, 0, 0, 0};
    return 0;
}

int fonts_reserve(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan) {
    DEC_GROW(dec->d_line_font, g.total);
    if (mode.kind == Kind::fonts) DEC_GROW(dec->d_font_cost, g.total);  // under the whole-line decode the cost is that run's
    DEC_GROW(dec->d_fdesc, plan.fonts.size());
    DEC_CHECK(hipMemcpyAsync(dec->d_fdesc, plan.fonts.data(), plan.fonts.size() * sizeof(FontDesc), hipMemcpyHostToDevice, dec->stream));
    return 0;
}

void fonts_launch(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan, size_t strip_bytes) {
    const bool lds = strip_bytes + FONTS_RED_BYTES <= LDS_STRIP_MAX;  // the strip shares LDS with the waves' pairs
    const size_t lds_bytes = FONTS_RED_BYTES + (lds ? strip_bytes : 0);
    const uint32_t grid = mode.grid ? std::min(mode.grid, g.total) : g.total;
    const GlyphTables &t = dec->tables, &c = dec->ftables;
    const FontTables f{t.glyphs, c.glyphs, t.offs, c.offs, t.bitmaps.as<const uint32_t>(), c.bitmaps.as<const uint32_t>(), dec->d_fdesc, dec->n_glyphs,
                       (uint32_t)plan.fonts.size()};
    (lds ? line_fonts_kernel<true> : line_fonts_kernel<false>)<<<grid, FONTS_THREADS, lds_bytes, dec->stream>>>(
        dec->d_strips, g, dec->d_work, dec->d_count, f, dec->d_nchars, dec->d_chars, dec->d_line_font, dec->d_font_cost);
}

void drop_font_candidates(focr_decoder *dec) {
    dec->cands.clear();
    dec->ftables.release();
    dec->d_fdesc.release();
    dec->d_finc64.release();
    dec->fvtables.release();  // their verify tables (focr_decoder_set_verify_font_candidates) go with them
}

}  // namespace focr_dec

using namespace focr_dec;

extern "C" int focr_decoder_set_font_candidates(focr_decoder_t *dec, const focr_decode_font_t *fonts, uint32_t n) {
    const std::string who = "focr_decoder_set_font_candidates: ";
    if (!dec) return dfail(nullptr, who + "null decoder");
    DEC_CHECK(hipSetDevice(dec->device));
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    drop_font_candidates(dec);
    if (!fonts || !n) return 0;
    if (n > FOCR_FONT_CANDIDATES_MAX - 1) return dfail(dec, who + "at most 15 candidates (FOCR_FONT_CANDIDATES_MAX - 1)");
    if (!dec->n_glyphs) return dfail(dec, who + "no font (focr_decoder_set_font)");
    std::vector<HostFont> cands;
    PackedGlyphs packed;
    GlyphTables tables;
    const std::string no = pack_candidate_fonts(fonts, n, dec->font, &cands, &packed);
    if (!no.empty()) return dfail(dec, who + no);
    std::vector<uint8_t> all;
    all.reserve(packed.bytes);
    for (size_t k = 0; k < n; k++) all.insert(all.end(), fonts[k].bitmaps, fonts[k].bitmaps + fonts[k].bitmaps_len);
    if (tables.upload(packed, all.data()) != hipSuccess) return dfail(dec, who + "hipMalloc / hipMemcpy failed");
    dec->cands = std::move(cands);
    dec->ftables = std::move(tables);
    return 0;
}

extern "C" int focr_decoder_set_font_search(focr_decoder_t *dec, int on) {
    if (!dec) return dfail(nullptr, "focr_decoder_set_font_search: null decoder");
    dec->modes.font_search = on != 0;
    return 0;
}

extern "C" int focr_decoder_get_fonts(const focr_decoder_t *dec, uint8_t *font, int64_t *cost) {
    if (!dec) return dfail(nullptr, "focr_decoder_get_fonts: null decoder");
    if (!(dec->last.ok && dec->last.mode.fonts()))
        return dfail(const_cast<focr_decoder *>(dec), "focr_decoder_get_fonts: the last successful run did not search fonts (focr_decoder_set_font_search)");
    if (font && !dec->line_font.empty()) memcpy(font, dec->line_font.data(), dec->line_font.size());
    if (cost && !dec->font_cost.empty()) memcpy(cost, dec->font_cost.data(), dec->font_cost.size() * sizeof(int64_t));
    return 0;
}

extern "C" int focr_decoder_debug_set_fonts_grid(focr_decoder_t *dec, uint32_t grid) {
    if (!dec) return dfail(nullptr, "focr_decoder_debug_set_fonts_grid: null decoder");
    dec->modes.fonts_grid = grid;
    return 0;
}
