// ncc_images.hip — focr_verify_images (include/focr_ncc.h): the characters of the last focr_process_hits redrawn over their
// pages on the device, as the line decoder's --verify image (draw_verify + red_blue_mse of the reference's src/main.rs, restated
// by focr_decoder_verify in decode_images.hip), over the tile frame of decode.h.
//
// Per page an RGB image of r_w x r_h from black: red = 255 - ink where the page has ink (the page's luma where it is not 255);
// blue = 255 - v where a character's template byte v is not zero, characters applied in their output order (page, line, x), a
// later one replacing an earlier one's blue only where its own v != 0; green = 0; sq_sums[page] = the exact sum of (R - B)^2.
// The reference's quirks are kept: uncovered paper adds 0, and so does an uncovered pixel of luma 0 (red 0, blue 0).
//
// Two launches, whatever the data:
//   1. ncc_records_kernel: one thread per character writes its VerifyRec (the box clipped to the page, the dense needle of its
//      template as the source) and the first n_pages threads zero the sums;
//   2. ncc_compose_kernel: one workgroup per (page, 16 rows, 256 columns) tile.  The characters of a page are sorted by (line
//      y, x; x only non-decreasing inside a line: with overlap < 0 two templates at one corner are two characters, in template
//      order), so a tile finds those that reach it with a binary search over the page's lines for y in (r0 - max n_h, r1) and,
//      in each such line, one for x in (c0 - max n_w, c1).  Each piece goes through mark_glyphs with its first character's index
//      as the base: the word of a pixel is 1 + the batch-wide index of the last character with INK over it, kept by an LDS
//      atomic max.  The order lives in the word itself, so the pieces need no resolve step between them, nothing is staged and
//      nothing can overflow: a tile takes as many pieces of as many characters as reach it.
#include "common.h"
#include "decode.h"

namespace focr {

using focr_dec::Tile;
using focr_dec::VerifyRec;
using focr_dec::VERIFY_TILE_H;
using focr_dec::VERIFY_TILE_W;

constexpr uint32_t RECORD_THREADS = 256;

// 1. a character's record; threads below n_pages also zero the sums.  A character lies on its page (x < r_w, y < r_h: the scan's
// windows, focr_debug_process_hits' check), so its clipped box is never empty and x0 / y0 stay the keys the tiles search by.
__global__ __launch_bounds__(RECORD_THREADS) void ncc_records_kernel(const focr_hit_t *__restrict__ chars, uint32_t n_chars, uint32_t n_pages, uint32_t r_w,
                                                                     uint32_t r_h, const uint32_t *__restrict__ order_of,
                                                                     const uint32_t *__restrict__ needle_off, VerifyRec *__restrict__ recs,
                                                                     unsigned long long *__restrict__ sums) {
    const uint32_t i = blockIdx.x * RECORD_THREADS + threadIdx.x;
    if (i < n_pages) sums[i] = 0;
    if (i >= n_chars) return;
    const focr_hit_t h = chars[i];
    recs[i] = VerifyRec{(int32_t)h.x, (int32_t)h.y, (int32_t)std::min<uint32_t>((uint32_t)h.x + h.w, r_w), (int32_t)std::min<uint32_t>((uint32_t)h.y + h.h, r_h),
                        needle_off[order_of[h.template_index]], h.w};
}

// the first index in [lo, hi) whose key is not below `bound` (keys ascend)
template <typename Key>
__device__ __forceinline__ uint64_t first_at_least(uint64_t lo, uint64_t hi, int bound, Key key) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (key(mid) < bound) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// 2. compose the image tile by tile; every thread owns one column of a 16-row, 256-column tile.  n_chars == 0: no line tables.
__global__ __launch_bounds__(VERIFY_TILE_W) void ncc_compose_kernel(const uint8_t *__restrict__ pages, size_t pitch, size_t rows_alloc, uint32_t r_w, uint32_t r_h,
                                                                    uint32_t n_pages, uint32_t tiles_x, uint32_t tiles_y, int max_w, int max_h,
                                                                    const uint64_t *__restrict__ page_line_off, const uint64_t *__restrict__ line_char_off,
                                                                    uint64_t n_lines, uint32_t n_chars, const VerifyRec *__restrict__ recs,
                                                                    const uint8_t *__restrict__ needles, uint8_t *__restrict__ rgb,
                                                                    unsigned long long *__restrict__ sums) {
    __shared__ uint32_t win[VERIFY_TILE_H * VERIFY_TILE_W];  // 1 + index in recs of the last character with ink over the pixel
    __shared__ uint32_t part[VERIFY_TILE_W / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t n_tiles = (uint64_t)tiles_x * tiles_y * n_pages;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const Tile T = focr_dec::tile_at(tile, tiles_x, tiles_y, r_w, r_h);
        const auto [page, r0, c0, r1, c1] = T;
        for (uint32_t r = 0; r < VERIFY_TILE_H; r++) win[r * VERIFY_TILE_W + t] = 0;
        __syncthreads();
        if (n_chars) {  // (uniform across the workgroup, as everything up to the marks)
            auto line_y = [&](uint64_t l) { return recs[line_char_off[l]].y0; };  // every character of a line has the line's y
            auto char_x = [&](uint64_t i) { return recs[i].x0; };
            const uint64_t l_end = page_line_off[page + 1];
            const uint64_t l_lo = first_at_least(page_line_off[page], l_end, r0 - max_h + 1, line_y), l_hi = first_at_least(l_lo, l_end, r1, line_y);
            for (uint64_t l = l_lo; l < l_hi; l++) {
                const uint64_t a = line_char_off[l], b = l + 1 < n_lines ? line_char_off[l + 1] : n_chars;  // (the last offset is the host's to add)
                const uint64_t i_lo = first_at_least(a, b, c0 - max_w + 1, char_x), i_hi = first_at_least(i_lo, b, c1, char_x);
                focr_dec::mark_glyphs<true>(win, recs + i_lo, (uint32_t)(i_hi - i_lo), T, lane, wave, (uint32_t)i_lo, needles);
            }
        }
        __syncthreads();
        uint32_t acc = 0;
        const int x = c0 + (int)t;
        if (x < c1)
            for (int y = r0; y < r1; y++) {
                const uint8_t ink = pages[((size_t)page * rows_alloc + y) * pitch + x];
                const uint32_t w = win[(uint32_t)(y - r0) * VERIFY_TILE_W + t];
                const uint8_t red = ink ? (uint8_t)(255 - ink) : 0, blue = w ? (uint8_t)(255 - focr_dec::glyph_value(w, recs, needles, x, y)) : 0;
                if (rgb) {
                    const size_t at = (((size_t)page * r_h + y) * r_w + x) * 3;  // tight rows of any width: bytes
                    rgb[at] = red;
                    rgb[at + 1] = 0;
                    rgb[at + 2] = blue;
                }
                const int dd = (int)red - (int)blue;
                acc += (uint32_t)(dd * dd);  // at most 16 * 255^2 per thread, 2^28 per workgroup
            }
        focr_dec::tile_add_sum(acc, part, &sums[page], t);
    }
}

}  // namespace focr

using namespace focr;

extern "C" {

int focr_verify_images(focr_ctx_t *c, uint8_t *rgb, int rgb_on_device, uint64_t *sq_sums) {
    if (!c) return FOCR_ERR_INVALID;
    c->vimg_ms = 0.f;
    c->vimg_launches = 0;
    if (!rgb && !sq_sums) return fail(c, FOCR_ERR_INVALID, "focr_verify_images: neither an image nor a sum buffer");
    if (!c->scanned || !c->processed) return fail(c, FOCR_ERR_STATE, "focr_verify_images: call focr_process_hits first (after the last scan)");
    if (int rc = finish_results(c)) return rc;  // the batch's own event inside an executor: what follows never waits for the lane's next batch
    const size_t n_pages = c->n_pages, r_w = c->pages.r_w, r_h = c->pages.r_h, px = n_pages * r_w * r_h;
    const size_t n_chars = c->n_chars;  // 0: process_hits may not have run a kernel at all (no hits), its tables are not read
    if (n_chars >= 0xffffffffull) return fail(c, FOCR_ERR_OVERFLOW, "focr_verify_images: more than 2^32 characters in one batch");
    int max_w = 1, max_h = 1;
    for (const SizeClass &sc : c->bank.classes) max_w = std::max(max_w, (int)sc.n_w), max_h = std::max(max_h, (int)sc.n_h);
    const focr_dec::TileGrid tg = focr_dec::tile_grid(n_pages, r_w, r_h);
    FOCR_HIP(c, hipSetDevice(c->device));
    // the call's own buffers: exact, and idle here (every call ends with a wait for the stream they are used on)
    const bool stage = rgb && !rgb_on_device;
    if (c->vimg_recs.reserve(std::max<size_t>(n_chars, 1), Grow::exact, nullptr) != hipSuccess || c->vimg_sums.reserve(n_pages, Grow::exact, nullptr) != hipSuccess ||
        (stage && c->vimg_rgb.reserve(px * 3, Grow::exact, nullptr) != hipSuccess))
        return fail(c, FOCR_ERR_NOMEM, "focr_verify_images: hipMalloc failed");
    uint8_t *d_rgb = stage ? c->vimg_rgb.p : rgb;
    const hipStream_t s = c->io_stream;  // where the results of a finished batch are read (the context's own stream outside an executor)
    FOCR_HIP(c, hipEventRecord(c->vimg_ev[0], s));
    hipLaunchKernelGGL(ncc_records_kernel, dim3((unsigned)((std::max(n_chars, n_pages) + RECORD_THREADS - 1) / RECORD_THREADS)), dim3(RECORD_THREADS), 0, s,
                       (const focr_hit_t *)c->post_chars.p, (uint32_t)n_chars, (uint32_t)n_pages, (uint32_t)r_w, (uint32_t)r_h, (const uint32_t *)c->bank.d_order_of.p,
                       (const uint32_t *)c->bank.d_needle_off.p, c->vimg_recs.p, c->vimg_sums.p);
    FOCR_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(ncc_compose_kernel, dim3(tg.grid), dim3(focr_dec::VERIFY_TILE_W), 0, s, (const uint8_t *)c->pages.u8.p, c->pages.pitch, c->pages.rows_alloc,
                       (uint32_t)r_w, (uint32_t)r_h, (uint32_t)n_pages, tg.tiles_x, tg.tiles_y, max_w, max_h, (const uint64_t *)c->post_page_off.p,
                       (const uint64_t *)c->post_line_off.p, (uint64_t)c->n_lines, (uint32_t)n_chars, (const VerifyRec *)c->vimg_recs.p,
                       (const uint8_t *)c->bank.d_needles.p, d_rgb, c->vimg_sums.p);
    FOCR_HIP(c, hipGetLastError());
    FOCR_HIP(c, hipEventRecord(c->vimg_ev[1], s));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit sums");
    if (sq_sums) FOCR_HIP(c, hipMemcpyAsync(sq_sums, c->vimg_sums.p, n_pages * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (stage) FOCR_HIP(c, hipMemcpyAsync(rgb, d_rgb, px * 3, hipMemcpyDeviceToHost, s));
    FOCR_HIP(c, hipStreamSynchronize(s));
    FOCR_HIP(c, hipEventElapsedTime(&c->vimg_ms, c->vimg_ev[0], c->vimg_ev[1]));
    c->vimg_launches = 2;
    return FOCR_OK;
}

int focr_last_verify_images(focr_ctx_t *c, float *ms, uint32_t *launches) {
    if (!c) return FOCR_ERR_INVALID;
    if (ms) *ms = c->vimg_ms;
    if (launches) *launches = c->vimg_launches;
    return FOCR_OK;
}

}  // extern "C"
