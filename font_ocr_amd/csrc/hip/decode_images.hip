// decode_images.hip — the images the `focr` binary draws beside its text, on the device (include/focr_decode.h), over the
// tile frame of decode.h.
//
// focr_decoder_verify draws focr --verify's image of the last run (decode.hip) in two launches, from the run's own buffers:
//   4. verify_layout_kernel: one wave per work-list line repeats render()'s f32 arithmetic (pen, round_out bounds, the
//      26.6 delta of every glyph; after a run with a pen search or a whole-line run (decode_whole.hip), from the pens the run chose;
//      after a baseline run (decode_baseline.hip) with the canvas moved by the nearest whole row of the line's offset) and
//      writes each glyph's
//      true bitmap rectangle, clipped to the canvas and the page; it takes the run's line grid (decode.h's LineFrac), which
//      is (0, 0), the whole-pixel grid, after every run but a baseline kind's on the fractional grid;
//   5. verify_compose_kernel: one workgroup per (page, 16 rows, 256 columns) tile takes, line by line in order, the
//      last glyph covering each pixel (an LDS atomic max of the glyph index, so placement and order do not matter),
//      lets a non-zero value replace the blue of earlier lines, writes RGB and adds the exact sum of (R - B)^2 to the
//      page's total with one 64-bit atomic.
//
// focr_decoder_test_images draws focr --test's two images of a batch in three launches, in buffers of its own:
//   6. test_flags_kernel: the blank test of every slot, as the prepass makes it;
//   7. test_layout_kernel: one wave lays out render() of the whole alphabet at (0, 0), as verify_layout_kernel does a line;
//   8. test_compose_kernel: one workgroup per tile counts, per row, the non-blank boxes with an edge on it and blends each
//      pixel once per edge through it (the rect image), and blends the last alphabet glyph over each pixel (the text
//      image), both from the base RGBA pixel with image's Blend for Rgba<u8> restated in f32 (blend_rgba).
#include "decode.h"

namespace focr_dec {

// (layout_line, render()'s layout of one line by one wave, is decode.h's: decode_text.hip lays out a caller's lines with it.)

// 4. render()'s layout of every decoded line, one wave per work-list line; blocks below n_pages also zero the sums.  Every
// line's y is its slot's crop row on the run's line grid, Y_i >> 6 (decode.h: fr is (0, 0) on the whole-pixel grid, where that is
// y_start + i * line_advance).
__global__ __launch_bounds__(64) void verify_layout_kernel(Geometry g, LineFrac fr, uint32_t n_pages, uint32_t x_start, const uint32_t *__restrict__ flags,
                                                           const uint32_t *__restrict__ work, const uint32_t *__restrict__ count,
                                                           const uint32_t *__restrict__ n_chars, const uint16_t *__restrict__ chars,
                                                           const int8_t *__restrict__ pen_offs, const uint32_t *__restrict__ pens,
                                                           const int32_t *__restrict__ line_q, uint32_t y_bits,
                                                           const DevGlyph *__restrict__ glyphs, const VerifyGlyph *__restrict__ vglyphs,
                                                           const VerifyPhase *__restrict__ vphases, VerifyLine *__restrict__ lines,
                                                           VerifyRec *__restrict__ recs, unsigned long long *__restrict__ sums) {
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (b < n_pages && lane == 0) sums[b] = 0;
    if (b >= g.total) return;
    if (lane == 0 && flags[b] == 0) lines[b] = VerifyLine{0, 0, 0, 0, 0, 0};  // blank slots are in no work-list entry
    if (b >= *count) return;
    const uint32_t k = b, slot = work[k], n = n_chars[k];
    // a baseline run's line (line_q; null: none) is drawn moved by the nearest whole row of its offset q * 2^-y_bits, the
    // absolute one: from the crop row
    const int moved = line_q ? (line_q[k] + (int)((1u << y_bits) >> 1)) >> y_bits : 0;
    layout_line<false>(g, slot, chars + (size_t)k * g.cap, pen_offs ? pen_offs + (size_t)k * g.cap : nullptr,
                       pens ? pens + (size_t)k * g.cap : nullptr, moved, n, k, x_start,
                       glyphs, vglyphs, vphases, recs + (size_t)k * g.cap, lines + slot, FracGrid{fr});
}

// 5. compose the verify image tile by tile; every thread owns one column of a 16-row, 256-column tile
__global__ __launch_bounds__(VERIFY_TILE_W) void verify_compose_kernel(const uint8_t *__restrict__ pages, Geometry g, uint32_t n_pages,
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
        // the slots whose canvas (at most hmax rows, from the slot's y) can reach rows r0 .. r1 - 1, in line order
        int64_t i_lo, i_hi;
        slot_range(g, r0, r1, (int64_t)hmax - 1, &i_lo, &i_hi);
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

// ---- test images (focr --test: draw_test_rectangles, draw_test_text) ------------------------------------------------

// image 0.25's Blend for Rgba<u8> (restated from the published crate, parity unpinned): every step one f32 operation,
// rounded on its own, and the result cast back with NumCast (truncation toward zero; every value lies in [0, 256)).
__device__ __forceinline__ uint32_t blend_rgba(uint32_t bg, uint32_t fg) {
    const uint32_t fa8 = fg >> 24;
    if (fa8 == 0) return bg;     // the crate's shortcuts: a transparent foreground changes nothing,
    if (fa8 == 255) return fg;   // an opaque one replaces the pixel
    const float m = 255.0f;
    const float bg_a = __fdiv_rn((float)(bg >> 24), m), fg_a = __fdiv_rn((float)fa8, m);
    const float a = __fsub_rn(__fadd_rn(bg_a, fg_a), __fmul_rn(bg_a, fg_a));
    if (a == 0.f) return bg;
    const float keep = __fsub_rn(1.0f, fg_a);
    uint32_t out = (uint32_t)__fmul_rn(m, a) << 24;
    for (int c = 0; c < 3; c++) {
        const float b = __fdiv_rn((float)((bg >> (8 * c)) & 255), m), f = __fdiv_rn((float)((fg >> (8 * c)) & 255), m);
        const float v = __fdiv_rn(__fadd_rn(__fmul_rn(f, fg_a), __fmul_rn(__fmul_rn(b, bg_a), keep)), a);
        out |= ((uint32_t)__fmul_rn(m, v) & 255) << (8 * c);
    }
    return out;
}

// focr_decoder_debug_blend: pixel i of out = blend_rgba(bg[i], fg[i]), RGBA bytes packed little-endian
__global__ __launch_bounds__(TEST_THREADS) void debug_blend_kernel(const uint32_t *__restrict__ bg, const uint32_t *__restrict__ fg, size_t n,
                                                                   uint32_t *__restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * TEST_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * TEST_THREADS) out[i] = blend_rgba(bg[i], fg[i]);
}

// 6. the blank test of every (page, slot), as line_prepass_kernel makes it but without the strip: one workgroup per slot
__global__ __launch_bounds__(TEST_THREADS) void test_flags_kernel(const uint8_t *__restrict__ pages, Geometry g, uint32_t *__restrict__ flags) {
    const uint32_t slot = blockIdx.x;
    if (slot >= g.total) return;
    const int ink = __syncthreads_or(slot_has_ink(pages, g, slot));
    if (threadIdx.x == 0) flags[slot] = ink ? 1u : 0u;
}

// 7. render() of the whole alphabet at (0, 0) on a page of g, one wave
__global__ __launch_bounds__(64) void test_layout_kernel(Geometry g, uint32_t n_glyphs, const DevGlyph *__restrict__ glyphs,
                                                         const VerifyGlyph *__restrict__ vglyphs, const VerifyPhase *__restrict__ vphases,
                                                         VerifyRec *__restrict__ recs, VerifyLine *__restrict__ line) {
    layout_line<true>(g, 0, nullptr, nullptr, nullptr, 0, n_glyphs, 0, 0, glyphs, vglyphs, vphases, recs, line);
}

// 8. both test images, tile by tile; every thread owns one column of a 16-row, 256-column tile.  The base pixel is
// base's, or (l, l, l, 255) from the luma without one.  rect: the pixel takes the red blend once per box edge through
// it (a corner is on two edges), counted per tile row from the flags of the slots whose box reaches the row; k blends in
// sequence stop early once one leaves the pixel as it was.  text: the last alphabet glyph over the pixel, as in
// verify_compose_kernel, blends (255 - v, 0, 0, 128) where its value v is not zero.  A null output is not drawn.
__global__ __launch_bounds__(VERIFY_TILE_W) void test_compose_kernel(const uint8_t *__restrict__ pages, const uint32_t *__restrict__ base,
                                                                     Geometry g, uint32_t n_pages, uint32_t x_start, uint32_t width, uint32_t tiles_x, uint32_t tiles_y,
                                                                     const uint32_t *__restrict__ flags, const VerifyLine *__restrict__ line,
                                                                     const VerifyRec *__restrict__ recs, const uint8_t *__restrict__ bitmaps,
                                                                     uint32_t *__restrict__ rect, uint32_t *__restrict__ text) {
    __shared__ uint32_t win[VERIFY_TILE_H * VERIFY_TILE_W];  // 1 + index of the last glyph over the pixel
    __shared__ uint32_t n_h[VERIFY_TILE_H], n_v[VERIFY_TILE_H];  // per tile row: boxes with a horizontal edge on it, boxes spanning it
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y * n_pages;
    const size_t W = g.page_w, H = g.page_h;
    const int64_t X0 = x_start, X1 = (int64_t)x_start + width;
    const VerifyLine l = text ? *line : VerifyLine{0, 0, 0, 0, 0, 0};
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const Tile T = tile_at(tile, tiles_x, tiles_y, g.page_w, g.page_h);
        const auto [page, r0, c0, r1, c1] = T;
        for (uint32_t r = 0; r < VERIFY_TILE_H; r++) win[r * VERIFY_TILE_W + t] = 0;
        if (t < VERIFY_TILE_H) n_h[t] = 0, n_v[t] = 0;
        __syncthreads();
        if (rect && g.n_slots) {  // the slots whose box (rows y_i .. y_i + line_height) reaches rows r0 .. r1 - 1
            int64_t i_lo, i_hi;
            slot_range(g, r0, r1, g.line_height, &i_lo, &i_hi);
            const int64_t n_pairs = (i_hi - i_lo + 1) * VERIFY_TILE_H;
            for (int64_t q = t; q < n_pairs; q += VERIFY_TILE_W) {
                const int64_t i = i_lo + q / VERIFY_TILE_H, y = r0 + q % VERIFY_TILE_H;
                if (y >= r1 || !flags[(size_t)page * g.n_slots + i]) continue;
                const int64_t Y0 = (int64_t)g.y_start + i * g.line_advance, Y1 = Y0 + g.line_height;
                const uint32_t e = (y == Y0) + (y == Y1);
                if (e) atomicAdd(&n_h[y - r0], e);
                if (Y0 <= y && y <= Y1) atomicAdd(&n_v[y - r0], 1u);
            }
        }
        const bool glyphs_here = l.n && l.x0 < c1 && l.x1 > c0 && l.y0 < r1 && l.y1 > r0;  // uniform across the workgroup
        if (glyphs_here) mark_glyphs(win, recs, l.n, T, lane, wave);
        __syncthreads();
        const int x = c0 + (int)t;
        if (x < c1)
            for (int y = r0; y < r1; y++) {
                const size_t at = ((size_t)page * H + y) * W + x;
                uint32_t px;
                if (base) px = base[at];
                else {
                    const uint32_t v = pages[at];
                    px = v * 0x010101u | 0xff000000u;
                }
                const uint32_t row = (uint32_t)(y - r0);
                if (rect) {
                    const uint32_t k = (X0 <= x && x <= X1 ? n_h[row] : 0) + (x == X0 ? n_v[row] : 0) + (x == X1 ? n_v[row] : 0);
                    uint32_t p = px;
                    for (uint32_t q = 0; q < k; q++) {
                        const uint32_t nx = blend_rgba(p, 0x800000ffu);  // Rgba(255, 0, 0, 128)
                        if (nx == p) break;
                        p = nx;
                    }
                    rect[at] = p;
                }
                if (text) {
                    uint32_t p = px;
                    if (glyphs_here)
                        if (const uint32_t w = win[row * VERIFY_TILE_W + t]) {
                            const uint32_t v = glyph_value(w, recs, bitmaps, x, y);
                            if (v) p = blend_rgba(p, 0x80000000u | (255 - v));  // canvas_to_lum8: l = 255 - v, blended where l != 255
                        }
                    text[at] = p;
                }
            }
        __syncthreads();
    }
}

}  // namespace focr_dec

using namespace focr_dec;

extern "C" int focr_decoder_set_verify_font(focr_decoder_t *dec, const focr_verify_font_t *font) {
    const std::string who = "focr_decoder_set_verify_font: ";
    if (!dec) return dfail(nullptr, who + "null decoder");
    dec->vtables.ok = false;
    if (!font || !font->glyphs || !font->n_glyphs) return dfail(dec, who + "bad arguments");
    if (!dec->n_glyphs) return dfail(dec, who + "no decode font (focr_decoder_set_font)");
    PackedVerify packed;
    const std::string no = pack_verify_font(*font, dec->font, false, &packed);
    if (!no.empty()) return dfail(dec, who + no);
    DEC_CHECK(hipSetDevice(dec->device));
    if (dec->vtables.upload(packed) != hipSuccess) return dfail(dec, who + "hipMalloc / hipMemcpy failed");
    return 0;
}

extern "C" int focr_decoder_verify(focr_decoder_t *dec, uint8_t *rgb, int rgb_on_device, uint64_t *sq_sums) {
    if (!dec) return dfail(nullptr, "focr_decoder_verify: null decoder");
    dec->verify.ms = 0.f;
    dec->verify.launches = 0;
    if (!dec->last.ok) return dfail(dec, "focr_decoder_verify: no successful focr_decoder_run since the font was set");
    if (dec->last.mode.fonts())
        return dfail(dec, "focr_decoder_verify: the last run searched fonts (focr_decoder_set_font_search): drawing every line in its own font is a later step");
    if (!dec->vtables.ok) return dfail(dec, "focr_decoder_verify: no verify table (focr_decoder_set_verify_font)");
    if (!sq_sums) return dfail(dec, "focr_decoder_verify: null sq_sums");
    const LastRun &run = dec->last;
    const RunMode &mode = run.mode;
    const Geometry &g = run.g;
    const size_t n_pages = run.n_pages;
    if (n_pages == 0) return 0;
    const size_t W = g.page_w, H = g.page_h, px = n_pages * W * H;
    const TileGrid tg = tile_grid(n_pages, W, H);
    const size_t layout_blocks = std::max<size_t>(g.total, n_pages);
    if (layout_blocks > 0x7fffffffu) return dfail(dec, "focr_decoder_verify: too many pages in one batch");
    DEC_CHECK(hipSetDevice(dec->device));
    DEC_GROW(dec->d_vlines, std::max<size_t>(g.total, 1));
    DEC_GROW(dec->d_vrecs, std::max<size_t>((size_t)g.total * g.cap, 1));
    DEC_GROW(dec->d_sums, n_pages);
    uint8_t *d_rgb = nullptr;
    if (stage_out(dec, dec->d_rgb, rgb, rgb_on_device, px * 3, &d_rgb)) return 1;
    DEC_CHECK(hipEventRecord(dec->verify.begin, dec->stream));
    // what the run wrote: a pen search's offsets (a slack's are in the pens already), a whole-line run's pens, a baseline run's q
    const int8_t *pen_offs = mode.kind == Kind::pen_search ? (const int8_t *)dec->d_pen : nullptr;
    const uint32_t *pens = mode.whole() ? (const uint32_t *)dec->d_pens : nullptr;
    const int32_t *line_q = mode.base_q() ? (const int32_t *)dec->d_base_q : nullptr;
    // mode.frac is the run's line grid: (0, 0), the whole-pixel one, except after a baseline kind on the fractional grid
    verify_layout_kernel<<<(uint32_t)layout_blocks, 64, 0, dec->stream>>>(g, mode.frac, (uint32_t)n_pages, run.x_start, dec->d_flags, dec->d_work, dec->d_count,
                                                                         dec->d_nchars, dec->d_chars, pen_offs, pens, line_q, mode.bits, dec->tables.glyphs,
                                                                         dec->vtables.glyphs, dec->vtables.phases, dec->d_vlines, dec->d_vrecs, dec->d_sums);
    DEC_CHECK(hipGetLastError());
    if (mode.frac.on())  // ... and on the fractional grid the slots that reach a tile come from that grid's inverse
        verify_compose_frac_launch(dec, tg, n_pages, d_rgb);
    else if (mode.base_q())  // the canvases of a baseline run are moved off their slots: decode_baseline.hip's compose finds them
        verify_compose_moved_launch(dec, tg, n_pages, d_rgb);
    else
        verify_compose_kernel<<<tg.grid, VERIFY_TILE_W, 0, dec->stream>>>(run.src, g, (uint32_t)n_pages, dec->vtables.hmax, tg.tiles_x, tg.tiles_y, dec->d_vlines, dec->d_vrecs,
                                                                          (const uint8_t *)dec->tables.bitmaps, d_rgb, dec->d_sums);
    DEC_CHECK(hipGetLastError());
    DEC_CHECK(hipEventRecord(dec->verify.end, dec->stream));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit sums");
    DEC_CHECK(hipMemcpyAsync(sq_sums, dec->d_sums, n_pages * sizeof(uint64_t), hipMemcpyDeviceToHost, dec->stream));
    if (fetch_out(dec, rgb, rgb_on_device, d_rgb, px * 3)) return 1;
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    DEC_CHECK(hipEventElapsedTime(&dec->verify.ms, dec->verify.begin, dec->verify.end));
    dec->verify.launches = 2;
    return 0;
}

extern "C" int focr_decoder_test_images(focr_decoder_t *dec, const uint8_t *pages, const uint8_t *base_rgba, int in_on_device, size_t n_pages,
                                        size_t page_w, size_t page_h, uint32_t x_start, uint32_t y_start, uint32_t width,
                                        uint32_t line_height, uint32_t line_advance, uint8_t *rect_rgba, uint8_t *text_rgba,
                                        int out_on_device) {
    if (!dec) return dfail(nullptr, "focr_decoder_test_images: null decoder");
    dec->test.ms = 0.f;
    dec->test.launches = 0;
    if (n_pages && !pages) return dfail(dec, "focr_decoder_test_images: null pages");
    if (text_rgba && !dec->n_glyphs) return dfail(dec, "focr_decoder_test_images: the text image needs a decode font (focr_decoder_set_font)");
    if (text_rgba && !dec->vtables.ok)
        return dfail(dec, "focr_decoder_test_images: the text image needs a verify table (focr_decoder_set_verify_font)");
    Geometry g{};
    if (batch_geometry(dec, "focr_decoder_test_images", n_pages, page_w, page_h, x_start, y_start, width, line_height, line_advance, &g)) return 1;
    for (const void *p : {in_on_device ? (const void *)base_rgba : nullptr, out_on_device ? (const void *)rect_rgba : nullptr,
                          out_on_device ? (const void *)text_rgba : nullptr})
        if ((uintptr_t)p % 4) return dfail(dec, "focr_decoder_test_images: device RGBA buffers must be 4-byte aligned");
    const size_t px = n_pages * page_w * page_h;
    if (px == 0 || (!rect_rgba && !text_rgba)) return 0;
    const TileGrid tg = tile_grid(n_pages, page_w, page_h);
    DEC_CHECK(hipSetDevice(dec->device));
    const uint8_t *d_src = nullptr;
    const uint32_t *d_base = nullptr;
    uint32_t *d_rect = nullptr, *d_text = nullptr;
    if (stage_in(dec, dec->d_tpages, pages, in_on_device, px, &d_src) || stage_in(dec, dec->d_tbase, base_rgba, in_on_device, px, &d_base) ||
        stage_out(dec, dec->d_trect, rect_rgba, out_on_device, px, &d_rect) || stage_out(dec, dec->d_ttext, text_rgba, out_on_device, px, &d_text))
        return 1;
    if (rect_rgba) DEC_GROW(dec->d_tflags, std::max<size_t>(g.total, 1));
    if (text_rgba) {
        DEC_GROW(dec->d_trecs, dec->n_glyphs);
        DEC_GROW(dec->d_tline, 1);
    }
    uint32_t launches = 0;
    DEC_CHECK(hipEventRecord(dec->test.begin, dec->stream));
    if (rect_rgba) {
        test_flags_kernel<<<std::max<uint32_t>(g.total, 1), TEST_THREADS, 0, dec->stream>>>(d_src, g, dec->d_tflags);
        DEC_CHECK(hipGetLastError());
        launches++;
    }
    if (text_rgba) {
        test_layout_kernel<<<1, 64, 0, dec->stream>>>(g, dec->n_glyphs, dec->tables.glyphs, dec->vtables.glyphs, dec->vtables.phases, dec->d_trecs, dec->d_tline);
        DEC_CHECK(hipGetLastError());
        launches++;
    }
    test_compose_kernel<<<tg.grid, VERIFY_TILE_W, 0, dec->stream>>>(d_src, d_base, g, (uint32_t)n_pages, x_start, width, tg.tiles_x, tg.tiles_y, dec->d_tflags, dec->d_tline, dec->d_trecs,
                                                                    (const uint8_t *)dec->tables.bitmaps, d_rect, d_text);
    DEC_CHECK(hipGetLastError());
    launches++;
    DEC_CHECK(hipEventRecord(dec->test.end, dec->stream));
    if (fetch_out(dec, rect_rgba, out_on_device, d_rect, px) || fetch_out(dec, text_rgba, out_on_device, d_text, px)) return 1;
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    DEC_CHECK(hipEventElapsedTime(&dec->test.ms, dec->test.begin, dec->test.end));
    dec->test.launches = launches;
    return 0;
}

extern "C" int focr_decoder_debug_blend(focr_decoder_t *dec, const uint8_t *bg_rgba, const uint8_t *fg_rgba, size_t n, uint8_t *out_rgba) {
    if (!dec) return dfail(nullptr, "focr_decoder_debug_blend: null decoder");
    if (n && (!bg_rgba || !fg_rgba || !out_rgba)) return dfail(dec, "focr_decoder_debug_blend: null buffer");
    if (!n) return 0;
    DEC_CHECK(hipSetDevice(dec->device));
    focr::DevArray<uint32_t> buf;  // background, foreground, result
    DEC_GROW(buf, 3 * n);
    uint32_t *d = buf;
    hipError_t e = hipMemcpyAsync(d, bg_rgba, n * 4, hipMemcpyHostToDevice, dec->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + n, fg_rgba, n * 4, hipMemcpyHostToDevice, dec->stream);
    if (e == hipSuccess) {
        debug_blend_kernel<<<(uint32_t)std::min<size_t>((n + TEST_THREADS - 1) / TEST_THREADS, 1u << 16), TEST_THREADS, 0, dec->stream>>>(d, d + n, n,
                                                                                                                                       d + 2 * n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out_rgba, d + 2 * n, n * 4, hipMemcpyDeviceToHost, dec->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dec->stream);
    (void)hipStreamSynchronize(dec->stream);
    if (e != hipSuccess) return dfail(dec, std::string("focr_decoder_debug_blend: ") + hipGetErrorString(e));
    return 0;
}
