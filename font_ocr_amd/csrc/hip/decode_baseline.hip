// decode_baseline.hip — the baseline search of the `focr` line decoder (focr_decoder_set_baseline_search; an extension, see
// include/focr_decode.h): every line is decoded once per vertical candidate q in -N ..= N, in steps of 2^-B px, and the
// candidate with the lowest summed footprint term is the line.
//
// line_baseline_kernel takes line_decode_kernel's place as the third launch of a run (decode.hip).  One workgroup of four
// waves takes a work-list line (grid-stride, so a smaller grid takes several):
//   - the strip is staged in LDS once and shared by every candidate (when it fits; else it is read from global memory);
//   - wave w runs the plain pen loop for the candidates of rank w, w + 4, ... and keeps only the lowest (cost, rank);
//   - the four waves meet in LDS, and every wave works out the same winner;
//   - one wave decodes the winner once more and writes its characters: no trial buffers, and nothing depends on which
//     wave finished first.
// Candidate q renders from y-phase v = q & (2^B - 1) of the font (phase 0 is the decode font itself; the others are
// focr_decoder_set_baseline_fonts') with every box moved down by d = q >> B rows; footprint_term_wide clips a
// box to the crop's rows on both sides, so rows that d pushes above row 0 or below the last row are never read.
// Everything is exact integer arithmetic but the f32 pen, which is the plain loop's.
// The kernel takes the line grid (decode.h's LineFrac) and serves both: on the fractional grid of focr_decoder_set_line_frac a
// line's candidates lie around its own centre, and at (0, 0), the whole-pixel grid, every centre is 0 and every crop row is
// y_start + i * line_advance.  (verify_compose_moved_kernel, the compose of a verify after a run of either baseline kind, is the
// whole-pixel grid's alone: its restated twin on the fractional grid is decode_line_frac.hip's, and DESIGN.md 4b-7 has the
// measurement that kept the two apart.)
#include <cstring>

#include "decode_pen.h"

namespace focr_dec {

constexpr uint32_t BASE_THREADS = 256;  // one workgroup of four waves per work-list line
constexpr uint32_t BASE_WAVES = BASE_THREADS / 64;
constexpr uint32_t BASE_RED_BYTES = BASE_WAVES * 2 * 8;  // (cost, rank) per wave, in front of the strip

// The font as a candidate reads it: y-phase 0 is the decode font, the others lie v-major in tables of their own.
struct BaseFont {
    const DevGlyph *glyphs, *yglyphs;
    const int2 *offs, *yoffs;
    const uint32_t *bitmaps, *ybitmaps;
    uint32_t n_dw, yn_dw;  // dwords of the two bitmap tables
    uint32_t n_glyphs;
    float origin_x;
    int origin_y;   // a whole number >= 0
    uint32_t bits;  // B
};

// pen_loop under candidate q of the font.
template <bool WRITE>
__device__ __forceinline__ int64_t candidate_loop(const uint32_t *strip, uint32_t sdw, int w, uint32_t h, uint32_t cap, const BaseFont &f, int q,
                                                  uint32_t lane, uint16_t *__restrict__ out, uint32_t *__restrict__ n_out) {
    const uint32_t v = (uint32_t)q & ((1u << f.bits) - 1);
    const int d = q >> f.bits;  // floor
    const DevGlyph *glyphs = v ? f.yglyphs + (size_t)(v - 1) * f.n_glyphs : f.glyphs;
    const int2 *offs = v ? f.yoffs + (size_t)(v - 1) * f.n_glyphs * 64 : f.offs;
    return pen_loop<WRITE>(strip, sdw, w, h, cap, glyphs, offs, v ? f.ybitmaps : f.bitmaps, v ? f.yn_dw : f.n_dw, f.n_glyphs, f.origin_x, d, lane, out,
                           n_out);
}

// 3b. the pen loop under every baseline candidate, one workgroup per work-list line (grid-stride).  radius >= 1.  The crop's
// rows are the line grid's (decode.h: fr is (0, 0) on the whole-pixel grid), and the candidates of a line are
// q = c + rank_offset(rank) around the line's own centre c, worked out again for every line a workgroup takes (a handful of
// scalar integer operations, uniform across the workgroup); c is 0 on the whole-pixel grid.
template <bool LDS>
__global__ __launch_bounds__(BASE_THREADS) void line_baseline_kernel(const uint8_t *__restrict__ strips, Geometry g, LineFrac fr,
                                                                     const uint32_t *__restrict__ work, const uint32_t *__restrict__ count, BaseFont f,
                                                                     uint32_t radius, uint32_t *__restrict__ n_chars, uint16_t *__restrict__ chars,
                                                                     int32_t *__restrict__ line_q, int64_t *__restrict__ line_cost) {
    extern __shared__ __align__(8) uint32_t lds_base[];  // the waves' (cost, rank), then (LDS) the strip
    uint64_t *red = (uint64_t *)lds_base;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t sdw = g.stride / 4, n_cand = 2 * radius + 1, n_lines = *count;
    // the winner's decode goes to a wave that has one candidate fewer than wave 0 (n_cand is odd: wave 1 or 3)
    const uint32_t writer = n_cand & (BASE_WAVES - 1);
    for (uint32_t k = blockIdx.x; k < n_lines; k += gridDim.x) {
        const uint32_t slot = work[k];
        uint32_t yc, h, fi;
        slot_rows_frac(g, fr, slot % g.n_slots, &yc, &h, &fi);
        const int c = frac_centre(fi, f.bits);  // this line's
        const uint32_t *strip = (const uint32_t *)(strips + (size_t)slot * g.stride * g.line_height);
        if (LDS) {
            uint32_t *lds_strip = lds_base + BASE_RED_BYTES / 4;
            for (uint32_t i = tid; i < sdw * h; i += BASE_THREADS) lds_strip[i] = strip[i];
            __syncthreads();
            strip = lds_strip;
        }
        int64_t best_cost = INT64_MAX;
        uint32_t best_rank = ~0u;  // a wave without a candidate: never the winner (rank 0 is never dropped: c >= 0)
        for (uint32_t rank = wave; rank < n_cand; rank += BASE_WAVES) {
            const int q = c + rank_offset(rank);
            if (f.origin_y * (1 << f.bits) + q < 0) continue;  // ty_q < 0: no such rendering
            const int64_t cost = candidate_loop<false>(strip, sdw, (int)g.w, h, g.cap, f, q, lane, nullptr, nullptr);
            if (cost < best_cost) best_cost = cost, best_rank = rank;  // a wave's ranks ascend: the first of equal costs stays
        }
        if (lane == 0) red[2 * wave] = (uint64_t)best_cost, red[2 * wave + 1] = best_rank;
        __syncthreads();
        best_cost = (int64_t)red[0], best_rank = (uint32_t)red[1];
        for (uint32_t v = 1; v < BASE_WAVES; v++) {
            const int64_t cv = (int64_t)red[2 * v];
            const uint32_t r = (uint32_t)red[2 * v + 1];
            if (cv < best_cost || (cv == best_cost && r < best_rank)) best_cost = cv, best_rank = r;
        }
        if (wave == writer) {
            const int q = c + rank_offset(best_rank);  // the absolute q: y + q * 2^-B is the line's top
            const int64_t cost = candidate_loop<true>(strip, sdw, (int)g.w, h, g.cap, f, q, lane, chars + (size_t)k * g.cap, n_chars + k);
            if (lane == 0) line_q[k] = q, line_cost[k] = cost;
        }
        __syncthreads();  // the strip and the pairs are the next line's from here
    }
}

// 5b. decode_images.hip's verify_compose_kernel after a baseline run: the canvases lie up to FOCR_BASELINE_MAX rows above or below their slots, so
// a tile looks that much further for the slots that can reach it; the rest is the same.  (A kernel of its own, not a template
// or a shared body, and in this file: each of the three changes verify_compose_kernel's machine code, tools/isa_hash.py, which
// the plain verify's timing pins.  decode_line_frac.hip's verify_compose_moved_frac_kernel restates this body in turn: a fix here is a fix there.)
__global__ __launch_bounds__(VERIFY_TILE_W) void verify_compose_moved_kernel(const uint8_t *__restrict__ pages, Geometry g, uint32_t n_pages,
                                                                       uint32_t hmax, uint32_t tiles_x, uint32_t tiles_y, const VerifyLine *__restrict__ lines,
                                                                       const VerifyRec *__restrict__ recs, const uint8_t *__restrict__ bitmaps,
                                                                       uint8_t *__restrict__ rgb, unsigned long long *__restrict__ sums) {
    __shared__ uint32_t win[VERIFY_TILE_H * VERIFY_TILE_W];  // 1 + index of the last glyph of the current line over the pixel
    __shared__ uint8_t blue[VERIFY_TILE_H * VERIFY_TILE_W];
    __shared__ uint32_t part[VERIFY_TILE_W / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y * n_pages;
    const size_t W = g.page_w, H = g.page_h;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const Tile T = tile_at(tile, tiles_x, tiles_y, g.page_w, g.page_h);
        const auto [page, r0, c0, r1, c1] = T;
        for (uint32_t r = 0; r < VERIFY_TILE_H; r++) {
            win[r * VERIFY_TILE_W + t] = 0;
            blue[r * VERIFY_TILE_W + t] = 0;
        }
        __syncthreads();
        // the slots whose canvas (at most hmax rows, from the slot's y moved either way) can reach rows r0 .. r1 - 1, in line order
        int64_t i_lo, i_hi;
        slot_range(g, r0, r1 + (int)FOCR_BASELINE_MAX, (int64_t)hmax - 1 + FOCR_BASELINE_MAX, &i_lo, &i_hi);
        for (int64_t i = i_lo; i <= i_hi; i++) {
            const VerifyLine l = lines[(size_t)page * g.n_slots + i];
            if (l.n == 0 || l.x0 >= c1 || l.x1 <= c0 || l.y0 >= r1 || l.y1 <= r0) continue;  // uniform across the workgroup
            const VerifyRec *lr = recs + (size_t)l.k * g.cap;
            mark_glyphs(win, lr, l.n, T, lane, wave);
            __syncthreads();
            const int x = c0 + (int)t;
            for (int y = r0; y < r1 && x < c1; y++) {
                const uint32_t idx = (uint32_t)(y - r0) * VERIFY_TILE_W + t, w = win[idx];
                if (!w) continue;
                win[idx] = 0;
                const uint8_t v = glyph_value(w, lr, bitmaps, x, y);
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

void verify_compose_moved_launch(focr_decoder *dec, const TileGrid &tg, size_t n_pages, uint8_t *d_rgb) {
    verify_compose_moved_kernel<<<tg.grid, VERIFY_TILE_W, 0, dec->stream>>>(dec->last.src, dec->last.g, (uint32_t)n_pages, dec->vtables.hmax, tg.tiles_x, tg.tiles_y,
                                                                            dec->d_vlines, dec->d_vrecs, (const uint8_t *)dec->tables.bitmaps, d_rgb, dec->d_sums);
}

int baseline_reserve(focr_decoder *dec, const Geometry &g) {
    DEC_GROW(dec->d_base_q, g.total);
    DEC_GROW(dec->d_base_cost, g.total);
    return 0;
}

void baseline_launch(focr_decoder *dec, const RunMode &mode, const Geometry &g, size_t strip_bytes) {
    const bool lds = strip_bytes + BASE_RED_BYTES <= LDS_STRIP_MAX;  // the strip shares LDS with the waves' pairs
    const size_t lds_bytes = BASE_RED_BYTES + (lds ? strip_bytes : 0);
    const uint32_t grid = mode.grid ? std::min(mode.grid, g.total) : g.total;
    const GlyphTables &t = dec->tables, &y = dec->yfonts.tables;
    const BaseFont f{t.glyphs, y.glyphs, t.offs, y.offs, t.bitmaps.as<const uint32_t>(), y.bitmaps.as<const uint32_t>(), t.n_dw, y.n_dw, dec->n_glyphs,
                     dec->font.origin_x, (int)dec->font.origin_y, mode.bits};
    (lds ? line_baseline_kernel<true> : line_baseline_kernel<false>)<<<grid, BASE_THREADS, lds_bytes, dec->stream>>>(
        dec->d_strips, g, mode.frac, dec->d_work, dec->d_count, f, mode.radius, dec->d_nchars, dec->d_chars, dec->d_base_q, dec->d_base_cost);
}

void drop_baseline_fonts(focr_decoder *dec) { dec->yfonts = BaseFonts{}; }

}  // namespace focr_dec

using namespace focr_dec;

extern "C" int focr_decoder_set_baseline_fonts(focr_decoder_t *dec, const focr_decode_font_t *fonts, uint32_t y_bits) {
    const std::string who = "focr_decoder_set_baseline_fonts: ";
    if (!dec) return dfail(nullptr, who + "null decoder");
    DEC_CHECK(hipSetDevice(dec->device));
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    drop_baseline_fonts(dec);
    if (!fonts) return dfail(dec, who + "bad arguments");
    if (y_bits > FOCR_BASELINE_Y_BITS_MAX) return dfail(dec, who + "y_bits is at most 3");
    if (!dec->n_glyphs) return dfail(dec, who + "no font (focr_decoder_set_font)");
    const size_t V = (size_t)1 << y_bits;
    BaseFonts y;
    PackedGlyphs packed;
    const std::string no = pack_baseline_fonts(fonts, V, dec->font, &y.term_bound, &packed);
    if (!no.empty()) return dfail(dec, who + no);
    {  // fonts[0]'s bitmaps against the decoder's own copy
        if (fonts[0].bitmaps_len != dec->font.bitmaps_len) return dfail(dec, who + "fonts[0] is not the decode font (bitmaps)");
        std::vector<uint8_t> mine(dec->font.bitmaps_len);
        if (!mine.empty()) DEC_CHECK(hipMemcpy(mine.data(), dec->tables.bitmaps, mine.size(), hipMemcpyDeviceToHost));
        if (!mine.empty() && memcmp(mine.data(), fonts[0].bitmaps, mine.size())) return dfail(dec, who + "fonts[0] is not the decode font (bitmaps)");
    }
    if (V > 1) {
        std::vector<uint8_t> all;
        all.reserve(packed.bytes);
        for (size_t v = 1; v < V; v++) all.insert(all.end(), fonts[v].bitmaps, fonts[v].bitmaps + fonts[v].bitmaps_len);
        if (y.tables.upload(packed, all.data()) != hipSuccess) return dfail(dec, who + "hipMalloc / hipMemcpy failed");
    }
    y.ok = true, y.bits = y_bits;
    dec->yfonts = std::move(y);
    return 0;
}

extern "C" int focr_decoder_set_baseline_search(focr_decoder_t *dec, uint32_t y_bits, uint32_t n) {
    if (!dec) return dfail(nullptr, "focr_decoder_set_baseline_search: null decoder");
    if (y_bits > FOCR_BASELINE_Y_BITS_MAX) return dfail(dec, "focr_decoder_set_baseline_search: y_bits is at most 3");
    if (n > FOCR_BASELINE_MAX) return dfail(dec, "focr_decoder_set_baseline_search: the radius is at most 32 steps");
    dec->modes.base = BaseSearch{y_bits, n};
    return 0;
}

extern "C" int focr_decoder_get_baselines(const focr_decoder_t *dec, int8_t *q, int64_t *cost) {
    if (!dec) return dfail(nullptr, "focr_decoder_get_baselines: null decoder");
    if (!(dec->last.ok && dec->last.mode.base_q()))
        return dfail(const_cast<focr_decoder *>(dec), "focr_decoder_get_baselines: the last successful run did not search baselines (focr_decoder_set_baseline_search, or focr_decoder_set_whole_baseline beside the whole-line decode)");
    if (q && !dec->base_q.empty()) memcpy(q, dec->base_q.data(), dec->base_q.size());
    if (cost && !dec->base_cost.empty()) memcpy(cost, dec->base_cost.data(), dec->base_cost.size() * sizeof(int64_t));
    return 0;
}

extern "C" int focr_decoder_debug_set_baseline_grid(focr_decoder_t *dec, uint32_t grid) {
    if (!dec) return dfail(nullptr, "focr_decoder_debug_set_baseline_grid: null decoder");
    dec->modes.base_grid = grid;
    return 0;
}
