// decode_text.hip — focr_decoder_verify_text (include/focr_decode.h): the verify image and squared error of pages under a
// list of lines the caller supplies, each line in any font the decoder has uploaded: the decode font (0) or a candidate of
// the font search (1 ..= K).  What a font search decoded, or a reading somebody corrected, is drawn with it; focr_decoder_verify
// (decode_images.hip) draws only what the last run itself decoded, in the decode font.
//
// The reading is checked by text_plan.h and staged by stage_text (decode.h), both shared with focr_decoder_score_text.  Two launches, over
// the tile frame of decode.h and in buffers apart from the run's:
//   1. verify_layout_text_kernel: one wave per listed line runs layout_line (decode.h) with the line's own y and the glyph,
//      box and phase tables of the line's font (the candidates' lie k-major behind a per-font base, as their glyph records do), and
//      writes the line's glyph records and its clipped canvas, which carries the font; blocks below n_pages also zero the sums;
//   2. verify_compose_text_kernel: one workgroup per (page, 16 rows, 256 columns) tile walks that page's lines
//      [page_first[p], page_first[p + 1]) in list order.  The lines lie on no grid (any y, in any order, repeated,
//      overlapping, in fonts of different heights), so there is no slot grid to invert: the list itself is walked, and each
//      line's canvas is tested against the tile, uniformly across the workgroup.  A page has tens of lines.  A line that
//      reaches the tile is marked and read as verify_compose_kernel does it (mark_glyphs, glyph_value), from the bitmap table
//      of its font, chosen once per line; the sums are tile_add_sum's.
// Here as well: the upload of the candidates' verify tables (focr_decoder_set_verify_font_candidates).
#include "decode.h"

namespace focr_dec {

// The line grid of a caller's line: its own y, whatever the slot.
struct OwnRow {
    int64_t y;
    __device__ __forceinline__ int64_t row(const Geometry &, uint32_t) const { return y; }
};

// The tables of the fonts 0 ..= K as layout_line reads them: font 0 is the decode font's, the others lie k-major.
struct TextFonts {
    const DevGlyph *glyphs, *fglyphs;
    const VerifyGlyph *vglyphs, *fvglyphs;
    const VerifyPhase *vphases, *fvphases;
    uint32_t n_glyphs;
};

// 1. render()'s layout of every listed line, one wave per line; blocks below n_pages also zero the sums.  g carries the
// page's size and one slot (layout_line reads the line's row from the grid policy).
__global__ __launch_bounds__(64) void verify_layout_text_kernel(Geometry g, uint32_t n_pages, uint32_t n_lines, uint32_t x_start,
                                                                const TextRec *__restrict__ in, const uint16_t *__restrict__ chars,
                                                                const int8_t *__restrict__ offs, const uint32_t *__restrict__ pens, TextFonts f,
                                                                VerifyLine *__restrict__ lines, VerifyRec *__restrict__ recs,
                                                                unsigned long long *__restrict__ sums) {
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (b < n_pages && lane == 0) sums[b] = 0;
    if (b >= n_lines) return;
    const TextRec l = in[b];
    const size_t at = l.font ? (size_t)(l.font - 1) * f.n_glyphs : 0;  // uniform: the per-font base of the k-major tables
    layout_line<false>(g, 0, chars + l.first, offs ? offs + l.first : nullptr, pens ? pens + l.first : nullptr, 0, l.n, l.font, x_start,
                       l.font ? f.fglyphs + at : f.glyphs, l.font ? f.fvglyphs + at : f.vglyphs,
                       l.font ? f.fvphases + at * FOCR_DECODE_PHASES : f.vphases, recs + l.out, lines + b, OwnRow{(int64_t)l.y});
}

// 2. compose the image tile by tile; every thread owns one column of a 16-row, 256-column tile
__global__ __launch_bounds__(VERIFY_TILE_W) void verify_compose_text_kernel(const uint8_t *__restrict__ pages, uint32_t page_w, uint32_t page_h,
                                                                            uint32_t n_pages, uint32_t tiles_x, uint32_t tiles_y,
                                                                            const uint32_t *__restrict__ page_first, const TextRec *__restrict__ in,
                                                                            const VerifyLine *__restrict__ lines, const VerifyRec *__restrict__ recs,
                                                                            const uint8_t *__restrict__ bitmaps, const uint8_t *__restrict__ fbitmaps,
                                                                            uint8_t *__restrict__ rgb, unsigned long long *__restrict__ sums) {
    __shared__ uint32_t win[VERIFY_TILE_H * VERIFY_TILE_W];  // 1 + index of the last glyph of the current line over the pixel
    __shared__ uint8_t blue[VERIFY_TILE_H * VERIFY_TILE_W];
    __shared__ uint32_t part[VERIFY_TILE_W / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y * n_pages;
    const size_t W = page_w, H = page_h;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const Tile T = tile_at(tile, tiles_x, tiles_y, page_w, page_h);
        const auto [page, r0, c0, r1, c1] = T;
        for (uint32_t r = 0; r < VERIFY_TILE_H; r++) {
            win[r * VERIFY_TILE_W + t] = 0;
            blue[r * VERIFY_TILE_W + t] = 0;
        }
        __syncthreads();
        // the page's lines in list order: a later line's ink replaces an earlier line's
        const uint32_t i_lo = page_first[page], i_hi = page_first[page + 1];
        for (uint32_t i = i_lo; i < i_hi; i++) {
            const VerifyLine l = lines[i];
            if (l.n == 0 || l.x0 >= c1 || l.x1 <= c0 || l.y0 >= r1 || l.y1 <= r0) continue;  // uniform across the workgroup
            const VerifyRec *lr = recs + in[i].out;
            const uint8_t *bm = l.k ? fbitmaps : bitmaps;  // per line (l.k is its font), not per pixel
            mark_glyphs(win, lr, l.n, T, lane, wave);
            __syncthreads();
            const int x = c0 + (int)t;
            for (int y = r0; y < r1 && x < c1; y++) {
                const uint32_t idx = (uint32_t)(y - r0) * VERIFY_TILE_W + t, w = win[idx];
                if (!w) continue;
                win[idx] = 0;
                const uint8_t v = glyph_value(w, lr, bm, x, y);
                if (v) blue[idx] = (uint8_t)(255 - v);  // canvas_to_lum8 then draw_verify: only v != 0 reaches the page
            }
            __syncthreads();
        }
        uint32_t acc = 0;
        const int x = c0 + (int)t;
        if (x < c1)
            for (int y = r0; y < r1; y++) {
                const size_t at = ((size_t)page * H + y) * W + x;
                const uint8_t l = pages[at];
                const uint8_t red = l != 255 ? l : 0, b = blue[(uint32_t)(y - r0) * VERIFY_TILE_W + t];
                if (rgb) {
                    rgb[at * 3] = red;
                    rgb[at * 3 + 1] = 0;
                    rgb[at * 3 + 2] = b;
                }
                const int dd = (int)red - (int)b;
                acc += (uint32_t)(dd * dd);  // at most 16 * 255^2 per thread, 2^28 per workgroup
            }
        tile_add_sum(acc, part, &sums[page], t);
    }
}

}  // namespace focr_dec

using namespace focr_dec;

extern "C" int focr_decoder_set_verify_font_candidates(focr_decoder_t *dec, const focr_verify_font_t *fonts, uint32_t n) {
    const std::string who = "focr_decoder_set_verify_font_candidates: ";
    if (!dec) return dfail(nullptr, who + "null decoder");
    DEC_CHECK(hipSetDevice(dec->device));
    dec->fvtables.release();  // (every call that reads them ends with a stream wait)
    if (!fonts || !n) return dfail(dec, who + "bad arguments");
    if (!dec->n_glyphs) return dfail(dec, who + "no decode font (focr_decoder_set_font)");
    if (dec->cands.empty()) return dfail(dec, who + "no font candidates (focr_decoder_set_font_candidates)");
    if (n != dec->cands.size()) return dfail(dec, who + "one table per uploaded candidate: " + std::to_string(dec->cands.size()) + " of them");
    PackedVerify packed;
    const std::string no = pack_verify_fonts(fonts, dec->cands, &packed);
    if (!no.empty()) return dfail(dec, who + no);
    if (dec->fvtables.upload(packed) != hipSuccess) return dfail(dec, who + "hipMalloc / hipMemcpy failed");
    return 0;
}

extern "C" int focr_decoder_verify_text(focr_decoder_t *dec, const uint8_t *pages, int pages_on_device, size_t n_pages, size_t page_w, size_t page_h,
                                        uint32_t x_start, const focr_text_line_t *lines, size_t n_lines, const uint16_t *chars, const uint32_t *pens,
                                        const int8_t *offsets, size_t n_chars, uint8_t *rgb, int rgb_on_device, uint64_t *sq_sums) {
    const std::string who = "focr_decoder_verify_text: ";
    if (!dec) return dfail(nullptr, who + "null decoder");
    dec->vtext.ms = 0.f;
    dec->vtext.launches = 0;
    const TextInput in{lines, n_lines, chars, pens, offsets, n_chars, n_pages};
    std::string no = text_guards(in, pages, n_pages && !sq_sums ? "sq_sums" : nullptr);
    if (!no.empty()) return dfail(dec, who + no);
    if (!dec->n_glyphs) return dfail(dec, who + "no decode font (focr_decoder_set_font)");
    Geometry g{};
    if (batch_geometry(dec, "focr_decoder_verify_text", n_pages, page_w, page_h, x_start, 0, 0, 0, 1, &g)) return 1;
    if (n_lines > 0x7fffffffu || n_pages > 0x7fffffffu) return dfail(dec, who + "too many lines or pages in one call");
    TextAsk ask;
    ask.page_order = true;
    TextPlan plan;
    if (!(no = plan_text_lines(in, dec->font, dec->cands, ask, &plan)).empty()) return dfail(dec, who + no);
    if (plan.decode_font && !dec->vtables.ok) return dfail(dec, who + "a line in font 0 and no verify table of the decode font (focr_decoder_set_verify_font)");
    if (plan.candidates && !dec->fvtables.ok)
        return dfail(dec, who + "a line in a candidate font and no verify tables of the candidates (focr_decoder_set_verify_font_candidates)");
    if (!(no = plan_text_chars(in, dec->n_glyphs)).empty()) return dfail(dec, who + no);
    if (n_pages == 0) return 0;
    g.n_slots = 1;  // layout_line's slot 0; the line's row is its own y
    const size_t px = n_pages * page_w * page_h;
    const TileGrid tg = tile_grid(n_pages, page_w, page_h);
    const size_t layout_blocks = std::max(n_lines, n_pages);
    DEC_CHECK(hipSetDevice(dec->device));
    StagedText t;
    uint8_t *d_rgb = nullptr;
    if (stage_text(dec, in, plan.recs, pages, pages_on_device, px, &t) || stage_out(dec, dec->d_xrgb, rgb, rgb_on_device, px * 3, &d_rgb)) return 1;
    DEC_GROW(dec->d_xfirst, n_pages + 1);
    DEC_GROW(dec->d_xvlines, std::max<size_t>(n_lines, 1));
    DEC_GROW(dec->d_xrecs, std::max<size_t>(plan.n_out, 1));
    DEC_GROW(dec->d_xsums, n_pages);
    DEC_CHECK(hipMemcpyAsync(dec->d_xfirst, plan.page_first.data(), (n_pages + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, dec->stream));
    const TextFonts f{dec->tables.glyphs, dec->ftables.glyphs, dec->vtables.glyphs, dec->fvtables.glyphs, dec->vtables.phases, dec->fvtables.phases, dec->n_glyphs};
    DEC_CHECK(hipEventRecord(dec->vtext.begin, dec->stream));
    verify_layout_text_kernel<<<(uint32_t)layout_blocks, 64, 0, dec->stream>>>(g, (uint32_t)n_pages, (uint32_t)n_lines, x_start, t.recs, t.chars, t.offs, t.pens, f,
                                                                              dec->d_xvlines, dec->d_xrecs, dec->d_xsums);
    DEC_CHECK(hipGetLastError());
    verify_compose_text_kernel<<<tg.grid, VERIFY_TILE_W, 0, dec->stream>>>(t.pages, g.page_w, g.page_h, (uint32_t)n_pages, tg.tiles_x, tg.tiles_y, dec->d_xfirst, t.recs,
                                                                           dec->d_xvlines, dec->d_xrecs, (const uint8_t *)dec->tables.bitmaps,
                                                                           (const uint8_t *)dec->ftables.bitmaps, d_rgb, dec->d_xsums);
    DEC_CHECK(hipGetLastError());
    DEC_CHECK(hipEventRecord(dec->vtext.end, dec->stream));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit sums");
    DEC_CHECK(hipMemcpyAsync(sq_sums, dec->d_xsums, n_pages * sizeof(uint64_t), hipMemcpyDeviceToHost, dec->stream));
    if (fetch_out(dec, rgb, rgb_on_device, d_rgb, px * 3)) return 1;
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    DEC_CHECK(hipEventElapsedTime(&dec->vtext.ms, dec->vtext.begin, dec->vtext.end));
    dec->vtext.launches = 2;
    return 0;
}

extern "C" float focr_decoder_last_verify_text_ms(const focr_decoder_t *dec) { return dec ? dec->vtext.ms : 0.f; }
extern "C" uint32_t focr_decoder_last_verify_text_launches(const focr_decoder_t *dec) { return dec ? dec->vtext.launches : 0; }
