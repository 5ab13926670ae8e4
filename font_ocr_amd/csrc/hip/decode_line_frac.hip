// decode_line_frac.hip — the fractional line grid of the `focr` line decoder's two baseline modes (focr_decoder_set_line_frac;
// an extension, see include/focr_decode.h): its setter, and the compose kernel of a verify after a run on that grid.  The
// grid itself is stated once in decode.h (LineFrac, slot_rows_frac, frac_centre, slot_range_frac).  Of the other kernels that
// read it, line_prepass_frac_kernel (decode.hip) and line_whole_baseline_frac_kernel (decode_whole_baseline.hip) stand beside
// the kernels they restate, and line_baseline_kernel (decode_baseline.hip) and verify_layout_kernel (decode_images.hip) take the
// grid as an argument and serve the whole-pixel grid as well, at (0, 0).
#include "decode.h"

namespace focr_dec {

// 5bf. verify_compose_moved_kernel after a run on the fractional line grid: the slots that can reach a tile come from that
// grid's inverse (slot_range_frac), and a canvas lies up to FOCR_BASELINE_MAX rows above its slot's crop row and, with the
// centre's one row, up to FOCR_BASELINE_MAX + 1 below.  The rest is the same, restated for verify_compose_moved_kernel's own
// reason, and in a file of its own: a shared body changes that kernel's machine code, and so does a second kernel with
// static LDS in its translation unit (the LDS offsets move).
__global__ __launch_bounds__(VERIFY_TILE_W) void verify_compose_moved_frac_kernel(const uint8_t *__restrict__ pages, Geometry g, LineFrac fr, uint32_t n_pages,
                                                                            uint32_t hmax, uint32_t tiles_x, uint32_t tiles_y,
                                                                            const VerifyLine *__restrict__ lines, const VerifyRec *__restrict__ recs,
                                                                            const uint8_t *__restrict__ bitmaps, uint8_t *__restrict__ rgb,
                                                                            unsigned long long *__restrict__ sums) {
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
        int64_t i_lo, i_hi;  // i_hi < n_slots, and the loop tests each line's rectangle
        slot_range_frac(g, fr, r0, r1 + (int)FOCR_BASELINE_MAX, (int64_t)hmax + FOCR_BASELINE_MAX, &i_lo, &i_hi);
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
                if (v) blue[idx] = (uint8_t)(255 - v);
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

void verify_compose_frac_launch(focr_decoder *dec, const TileGrid &tg, size_t n_pages, uint8_t *d_rgb) {
    verify_compose_moved_frac_kernel<<<tg.grid, VERIFY_TILE_W, 0, dec->stream>>>(dec->last.src, dec->last.g, dec->last.mode.frac, (uint32_t)n_pages, dec->vtables.hmax, tg.tiles_x,
                                                                                 tg.tiles_y, dec->d_vlines, dec->d_vrecs, (const uint8_t *)dec->tables.bitmaps, d_rgb,
                                                                                 dec->d_sums);
}

}  // namespace focr_dec

using namespace focr_dec;

extern "C" int focr_decoder_set_line_frac(focr_decoder_t *dec, uint32_t y_frac, uint32_t advance_frac) {
    if (!dec) return dfail(nullptr, "focr_decoder_set_line_frac: null decoder");
    if (y_frac > 63 || advance_frac > 63) return dfail(dec, "focr_decoder_set_line_frac: y_frac and advance_frac are at most 63 (in 1/64 px)");
    dec->modes.frac = LineFrac{y_frac, advance_frac};
    return 0;
}
