// decode.hip — the `focr` line decoder on the device (include/focr_decode.h; decode_image / decode_line, src/main.rs:112-218).
//
// A batch of equal-size pages runs in three launches, whatever its line count:
//   1. line_prepass_kernel: one workgroup per (page, line) slot crops the line as the image crate does, inverts it
//      (r = 255 - luma) into a zero-padded strip and flags it non-blank (an empty crop counts as all-white);
//   2. line_compact_kernel: one workgroup turns the flags into the work list of non-blank slots, in (page, line) order;
//   3. line_decode_kernel: one wave per work-list line runs the reference's pen loop.  The pen and the step count are
//      uniform across the wave; each lane scores its glyphs (lane, lane + 64, ...) against the strip (LDS when it fits)
//      from the glyph's phase tile, then a wave argmin takes the lowest (score, glyph index).
// The reference scores sum over the canvas of (r - c)^2; that is sum r^2 + sum over the clipped glyph footprint of
// c * (c - 2r), and sum r^2 is the same for every candidate, so the footprint term alone decides the argmin, ties
// included.  It is exact integer arithmetic (v_dot4_u32_u8; the font builder bounds it below 2^31), so neither the
// order of the sums nor the device changes a choice.  The pen update is one f32 add of the host-computed increment.
//
// focr_decoder_verify draws focr --verify's image of the last run in two more launches, from the run's own buffers:
//   4. verify_layout_kernel: one wave per work-list line repeats render()'s f32 arithmetic (pen, round_out bounds, the
//      26.6 delta of every glyph) and writes each glyph's true bitmap rectangle, clipped to the canvas and the page;
//   5. verify_compose_kernel: one workgroup per (page, 16 rows, 256 columns) tile takes, line by line in order, the
//      last glyph covering each pixel (an LDS atomic max of the glyph index, so placement and order do not matter),
//      lets a non-zero value replace the blue of earlier lines, writes RGB and adds the exact sum of (R - B)^2 to the
//      page's total with one 64-bit atomic.
//
// focr_decoder_test_images draws focr --test's two images of a batch in three more launches, in buffers of its own:
//   6. test_flags_kernel: the blank test of every slot, as the prepass makes it;
//   7. test_layout_kernel: one wave lays out render() of the whole alphabet at (0, 0), as verify_layout_kernel does a line;
//   8. test_compose_kernel: one workgroup per tile counts, per row, the non-blank boxes with an edge on it and blends each
//      pixel once per edge through it (the rect image), and blends the last alphabet glyph over each pixel (the text
//      image), both from the base RGBA pixel with image's Blend for Rgba<u8> restated in f32 (blend_rgba).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "devmem.h"
#include "focr_decode.h"

namespace focr_dec {

constexpr uint32_t PAD = 4;                 // zero bytes left of a strip row (reads up to 3 bytes left of column 0)
constexpr uint32_t LDS_STRIP_MAX = 65536;   // the strip is staged in LDS up to this many bytes, else read from global
constexpr uint32_t PREPASS_THREADS = 256;
constexpr uint32_t COMPACT_THREADS = 1024;

struct DevGlyph {
    uint32_t off_dw;  // dword offset of phase 0 in the bitmap table
    uint32_t ndw;     // dwords per bitmap row
    uint32_t box_h;
    float inc;
};

struct Geometry {
    uint32_t page_w, page_h;
    uint32_t x, w;               // clamped crop x and width (equal for every line of the batch)
    uint32_t y_start, line_height, line_advance;
    uint32_t n_slots;            // line slots per page: y_start + i * line_advance < page_h
    uint32_t total;              // n_pages * n_slots
    uint32_t stride;             // bytes per strip row: PAD + w rounded up to dwords, plus two dwords of reach
    uint32_t cap;                // characters per line at most
};

__device__ __forceinline__ void slot_rows(const Geometry &g, uint32_t i, uint32_t *yc, uint32_t *h) {
    const uint64_t y = (uint64_t)g.y_start + (uint64_t)i * g.line_advance;
    *yc = (uint32_t)std::min<uint64_t>(y, g.page_h);
    *h = std::min(g.line_height, g.page_h - *yc);
}

// 1. crop + invert + blank flag, one workgroup per slot
__global__ __launch_bounds__(PREPASS_THREADS) void line_prepass_kernel(const uint8_t *__restrict__ pages, Geometry g,
                                                                       uint8_t *__restrict__ strips, uint32_t *__restrict__ flags) {
    const uint32_t slot = blockIdx.x;
    const uint32_t page = slot / g.n_slots, i = slot % g.n_slots;
    uint32_t yc, h;
    slot_rows(g, i, &yc, &h);
    const uint8_t *src = pages + (size_t)page * g.page_w * g.page_h + (size_t)yc * g.page_w + g.x;
    uint8_t *dst = strips + (size_t)slot * g.stride * g.line_height;
    int ink = 0;
    const uint32_t n = g.stride * h;
    for (uint32_t k = threadIdx.x; k < n; k += PREPASS_THREADS) {
        const uint32_t row = k / g.stride;
        const int col = (int)(k % g.stride) - (int)PAD;
        uint8_t v = 0;
        if (col >= 0 && (uint32_t)col < g.w) {
            const uint8_t l = src[(size_t)row * g.page_w + col];
            v = 255 - l;
            ink |= l != 255;
        }
        dst[k] = v;
    }
    ink = __syncthreads_or(ink);
    if (threadIdx.x == 0) flags[slot] = ink ? 1u : 0u;
}

// 2. order-preserving compaction of the non-blank slots, one workgroup
__global__ __launch_bounds__(COMPACT_THREADS) void line_compact_kernel(const uint32_t *__restrict__ flags, uint32_t total,
                                                                       uint32_t *__restrict__ work, uint32_t *__restrict__ count) {
    __shared__ uint32_t wave_sum[COMPACT_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t base = 0;
    for (uint32_t start = 0; start < total; start += COMPACT_THREADS) {
        const uint32_t s = start + threadIdx.x;
        const bool live = s < total && flags[s] != 0;
        const uint64_t m = __ballot(live);
        if (lane == 0) wave_sum[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < COMPACT_THREADS / 64; w++) {
            before += w < wave ? wave_sum[w] : 0;
            all += wave_sum[w];
        }
        if (live) work[base + before + (uint32_t)__popcll(m & ((1ull << lane) - 1))] = s;
        base += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}

__device__ __forceinline__ uint32_t edge_mask(int base, int w) {
    uint32_t m = 0;
    for (int b = 0; b < 4; b++)
        if (base + b >= 0 && base + b < w) m |= 0xffu << (8 * b);
    return m;
}

// 3. the pen loop, one wave per work-list line
template <bool LDS>
__global__ __launch_bounds__(64) void line_decode_kernel(const uint8_t *__restrict__ strips, Geometry g, const uint32_t *__restrict__ work,
                                                         const uint32_t *__restrict__ count, const DevGlyph *__restrict__ glyphs,
                                                         const int2 *__restrict__ offs, const uint32_t *__restrict__ bitmaps,
                                                         uint32_t n_glyphs, float origin_x, uint32_t *__restrict__ n_chars,
                                                         uint16_t *__restrict__ chars) {
    extern __shared__ uint32_t lds_strip[];
    const uint32_t k = blockIdx.x;
    if (k >= *count) return;
    const uint32_t slot = work[k];
    uint32_t yc, h;
    slot_rows(g, slot % g.n_slots, &yc, &h);
    const uint32_t *strip = (const uint32_t *)(strips + (size_t)slot * g.stride * g.line_height);
    const uint32_t sdw = g.stride / 4;
    if (LDS) {
        for (uint32_t q = threadIdx.x; q < sdw * h; q += 64) lds_strip[q] = strip[q];
        __syncthreads();
        strip = lds_strip;
    }
    const uint32_t lane = threadIdx.x;
    const int w = (int)g.w;
    const float fw = (float)g.w;
    uint16_t *out = chars + (size_t)k * g.cap;
    float pos = 0.f;
    uint32_t n = 0;
    while (pos < fw && n < g.cap) {
        const int d = (int)((origin_x + pos) * 64.0f);  // FreeType's delta: trunc(t * 64)
        const int phase = d & 63, shift = d >> 6;
        uint64_t best = ~0ull;
        for (uint32_t gi = lane; gi < n_glyphs; gi += 64) {
            const DevGlyph gl = glyphs[gi];
            const int2 o = offs[gi * 64 + phase];
            const int x0 = shift + o.x, y0 = o.y;
            const uint32_t *tile = bitmaps + gl.off_dw + (uint32_t)phase * gl.ndw * gl.box_h;
            const int r_lo = std::max(0, -y0), r_hi = std::min((int)gl.box_h, (int)h - y0);
            uint32_t cc = 0, cr = 0;
            for (int r = r_lo; r < r_hi; r++) {
                const uint32_t *srow = strip + (size_t)(y0 + r) * sdw;
                const uint32_t *trow = tile + (size_t)r * gl.ndw;
                for (uint32_t q = 0; q < gl.ndw; q++) {
                    const int base = x0 + 4 * (int)q;
                    if (base <= -4 || base >= w) continue;
                    uint32_t c = trow[q];
                    if (base < 0 || base + 4 > w) c &= edge_mask(base, w);
                    const uint32_t a = (uint32_t)(base + (int)PAD);
                    const uint32_t rv = __builtin_amdgcn_alignbyte(srow[(a >> 2) + 1], srow[a >> 2], a & 3);
                    cr = __builtin_amdgcn_udot4(c, rv, cr, false);
                    cc = __builtin_amdgcn_udot4(c, c, cc, false);
                }
            }
            const int score = (int)cc - 2 * (int)cr;
            const uint64_t key = ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | gi;  // (score, index), lowest first
            best = std::min(best, key);
        }
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t lo = __shfl_xor((uint32_t)best, m, 64), hi = __shfl_xor((uint32_t)(best >> 32), m, 64);
            best = std::min(best, ((uint64_t)hi << 32) | lo);
        }
        const uint32_t gbest = (uint32_t)best;
        if (lane == 0) out[n] = (uint16_t)gbest;
        n++;
        pos = __fadd_rn(pos, glyphs[gbest].inc);
    }
    if (lane == 0) n_chars[k] = n;
}

// ---- verify ------------------------------------------------------------------------------------------------------

constexpr uint32_t VERIFY_TILE_W = 256;     // compose tile: one column per thread
constexpr uint32_t VERIFY_TILE_H = 16;
constexpr uint32_t VERIFY_MAX_GRID = 1u << 20;

struct VerifyGlyph {
    float box[4];      // raster_bounds at the identity before round_out (focr_verify_glyph_t::box)
};

struct VerifyPhase {
    int32_t x, y;      // top-left of the true bitmap on a line canvas at whole-pixel shift 0 and vertical translation 0
    uint32_t w, h;
    uint32_t src;      // byte offset of that top-left pixel in the bitmap table
    uint32_t stride;
};

struct VerifyLine {    // one line slot: its canvas on the page, clipped (empty for a blank slot), and its glyph records
    int32_t x0, y0, x1, y1;
    uint32_t k, n;
};

struct VerifyRec {     // one glyph: its bitmap rectangle on the page, clipped to the canvas and the page
    int32_t x0, y0, x1, y1;
    uint32_t src, stride;  // byte offset in the bitmap table of the pixel at (x0, y0)
};

// render()'s layout of one line of n glyphs on a page of g, by one wave: the pen (f32 adds in text order), the union
// of round_out boxes folded from the empty rect at (0, 0), and each glyph's true bitmap rectangle clipped to the canvas
// and the page, written to out[0 .. n).  The line is cs[0 .. n) at (x_start, y of g's slot), or for IOTA the alphabet
// indices 0 .. n - 1 at (x_start, 0).  Lane 0 writes the line's canvas on the page to *line, clipped (empty when none
// of it is on the page), with k and n.
template <bool IOTA>
__device__ __forceinline__ void layout_line(const Geometry &g, uint32_t slot, const uint16_t *__restrict__ cs, uint32_t n, uint32_t k,
                                            uint32_t x_start, const DevGlyph *__restrict__ glyphs, const VerifyGlyph *__restrict__ vglyphs,
                                            const VerifyPhase *__restrict__ vphases, VerifyRec *__restrict__ out, VerifyLine *__restrict__ line) {
    const uint32_t lane = threadIdx.x;
    float pen = 0.f;
    int ox = 0, oy = 0, lx = 0, ly = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t j = base + lane, m = std::min(64u, n - base);
        const bool live = j < n;
        const uint32_t c = live ? (IOTA ? j : cs[j]) : 0;
        const float inc = live ? glyphs[c].inc : 0.f;
        float pos = 0.f;
        for (uint32_t q = 0; q < m; q++) {
            if (lane == q) pos = pen;
            pen = __fadd_rn(pen, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(inc), q)));
        }
        if (live) {
            const VerifyGlyph v = vglyphs[c];
            ox = std::min(ox, (int)floorf(__fadd_rn(v.box[0], pos)));
            oy = std::min(oy, (int)floorf(__fadd_rn(v.box[1], 0.f)));
            lx = std::max(lx, (int)ceilf(__fadd_rn(v.box[2], pos)));
            ly = std::max(ly, (int)ceilf(__fadd_rn(v.box[3], 0.f)));
            out[j].x0 = __float_as_int(pos);  // kept for the second pass of this same lane
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        ox = std::min(ox, __shfl_xor(ox, s, 64));
        oy = std::min(oy, __shfl_xor(oy, s, 64));
        lx = std::max(lx, __shfl_xor(lx, s, 64));
        ly = std::max(ly, __shfl_xor(ly, s, 64));
    }
    const int cw = lx - ox, ch = ly - oy;
    const int64_t W = g.page_w, H = g.page_h;
    const int64_t line_y = IOTA ? 0 : (int64_t)g.y_start + (int64_t)(slot % g.n_slots) * g.line_advance;
    const float neg_ox = (float)(-ox);
    for (uint32_t j = lane; j < n; j += 64) {
        const float pos = __int_as_float(out[j].x0);
        const int d = (int)__fmul_rn(__fadd_rn(neg_ox, pos), 64.0f);  // FreeType's delta: trunc((-bounds.ox + pos) * 64) >= 0
        const VerifyPhase ph = vphases[(size_t)(IOTA ? j : cs[j]) * FOCR_DECODE_PHASES + (d & 63)];
        const int gx0 = (d >> 6) + ph.x, gy0 = ph.y - oy;  // on the canvas: whole-pixel shift, vertical delta -bounds.oy
        const int ax0 = std::max(gx0, 0), ay0 = std::max(gy0, 0);
        const int ax1 = std::min(gx0 + (int)ph.w, cw), ay1 = std::min(gy0 + (int)ph.h, ch);
        const int64_t X0 = x_start + (int64_t)ax0, Y0 = line_y + ay0;
        const int64_t X1 = std::min<int64_t>(x_start + (int64_t)ax1, W), Y1 = std::min<int64_t>(line_y + ay1, H);
        VerifyRec r{0, 0, 0, 0, 0, 0};
        if (ax0 < ax1 && ay0 < ay1 && X0 < X1 && Y0 < Y1)
            r = VerifyRec{(int32_t)X0, (int32_t)Y0, (int32_t)X1, (int32_t)Y1, ph.src + (uint32_t)(ay0 - gy0) * ph.stride + (uint32_t)(ax0 - gx0),
                          ph.stride};
        out[j] = r;
    }
    if (lane == 0) {
        const int64_t X1 = std::min<int64_t>(x_start + (int64_t)cw, W), Y1 = std::min<int64_t>(line_y + ch, H);
        VerifyLine l{0, 0, 0, 0, k, n};
        if ((int64_t)x_start < X1 && line_y < Y1) l = VerifyLine{(int32_t)x_start, (int32_t)line_y, (int32_t)X1, (int32_t)Y1, k, n};
        *line = l;
    }
}

// 4. render()'s layout of every decoded line, one wave per work-list line; blocks below n_pages also zero the sums
__global__ __launch_bounds__(64) void verify_layout_kernel(Geometry g, uint32_t n_pages, uint32_t x_start, const uint32_t *__restrict__ flags,
                                                           const uint32_t *__restrict__ work, const uint32_t *__restrict__ count,
                                                           const uint32_t *__restrict__ n_chars, const uint16_t *__restrict__ chars,
                                                           const DevGlyph *__restrict__ glyphs, const VerifyGlyph *__restrict__ vglyphs,
                                                           const VerifyPhase *__restrict__ vphases, VerifyLine *__restrict__ lines,
                                                           VerifyRec *__restrict__ recs, unsigned long long *__restrict__ sums) {
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    if (b < n_pages && lane == 0) sums[b] = 0;
    if (b >= g.total) return;
    if (lane == 0 && flags[b] == 0) lines[b] = VerifyLine{0, 0, 0, 0, 0, 0};  // blank slots are in no work-list entry
    if (b >= *count) return;
    const uint32_t k = b, slot = work[k], n = n_chars[k];
    layout_line<false>(g, slot, chars + (size_t)k * g.cap, n, k, x_start, glyphs, vglyphs, vphases, recs + (size_t)k * g.cap, lines + slot);
}

// 5. compose the verify image tile by tile; every thread owns one column of a 16-row, 256-column tile
__global__ __launch_bounds__(VERIFY_TILE_W) void verify_compose_kernel(const uint8_t *__restrict__ pages, Geometry g, uint32_t n_pages,
                                                                       uint32_t hmax, uint32_t tiles_x, uint32_t tiles_y,
                                                                       const VerifyLine *__restrict__ lines, const VerifyRec *__restrict__ recs,
                                                                       const uint8_t *__restrict__ bitmaps, uint8_t *__restrict__ rgb,
                                                                       unsigned long long *__restrict__ sums) {
    __shared__ uint32_t win[VERIFY_TILE_H * VERIFY_TILE_W];  // 1 + index of the last glyph of the current line over the pixel
    __shared__ uint8_t blue[VERIFY_TILE_H * VERIFY_TILE_W];
    __shared__ uint32_t part[VERIFY_TILE_W / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t per_page = (uint64_t)tiles_x * tiles_y, n_tiles = per_page * n_pages;
    const size_t W = g.page_w, H = g.page_h;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t page = (uint32_t)(tile / per_page), rem = (uint32_t)(tile % per_page);
        const int r0 = (int)((rem / tiles_x) * VERIFY_TILE_H), c0 = (int)((rem % tiles_x) * VERIFY_TILE_W);
        const int r1 = std::min<int>(r0 + VERIFY_TILE_H, (int)H), c1 = std::min<int>(c0 + VERIFY_TILE_W, (int)W);
        for (uint32_t r = 0; r < VERIFY_TILE_H; r++) {
            win[r * VERIFY_TILE_W + t] = 0;
            blue[r * VERIFY_TILE_W + t] = 0;
        }
        __syncthreads();
        // the slots whose canvas (at most hmax rows, from the slot's y) can reach rows r0 .. r1 - 1, in line order
        int64_t i_lo = 0, i_hi = -1;
        if (g.n_slots) {
            const int64_t lo = (int64_t)r0 - hmax + 1 - g.y_start, hi = (int64_t)r1 - 1 - g.y_start;
            i_lo = lo <= 0 ? 0 : (lo + g.line_advance - 1) / g.line_advance;
            i_hi = hi < 0 ? -1 : std::min<int64_t>(g.n_slots - 1, hi / g.line_advance);
        }
        for (int64_t i = i_lo; i <= i_hi; i++) {
            const VerifyLine l = lines[(size_t)page * g.n_slots + i];
            if (l.n == 0 || l.x0 >= c1 || l.x1 <= c0 || l.y0 >= r1 || l.y1 <= r0) continue;  // uniform across the workgroup
            const VerifyRec *lr = recs + (size_t)l.k * g.cap;
            for (uint32_t j = wave; j < l.n; j += VERIFY_TILE_W / 64) {
                const VerifyRec r = lr[j];
                const int x0 = std::max(r.x0, c0), x1 = std::min(r.x1, c1), y0 = std::max(r.y0, r0), y1 = std::min(r.y1, r1);
                if (x0 >= x1 || y0 >= y1) continue;
                const int w = x1 - x0, npx = w * (y1 - y0);
                for (int q = (int)lane; q < npx; q += 64)
                    atomicMax(&win[(y0 + q / w - r0) * VERIFY_TILE_W + (x0 + q % w - c0)], j + 1);
            }
            __syncthreads();
            const int x = c0 + (int)t;
            for (int y = r0; y < r1 && x < c1; y++) {
                const uint32_t idx = (uint32_t)(y - r0) * VERIFY_TILE_W + t, w = win[idx];
                if (!w) continue;
                win[idx] = 0;
                const VerifyRec r = lr[w - 1];
                const uint8_t v = bitmaps[r.src + (uint32_t)(y - r.y0) * r.stride + (uint32_t)(x - r.x0)];
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
        for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s, 64);
        if (lane == 0) part[wave] = acc;
        __syncthreads();
        if (t == 0) {
            unsigned long long sum = 0;
            for (uint32_t w = 0; w < VERIFY_TILE_W / 64; w++) sum += part[w];
            if (sum) atomicAdd(&sums[page], sum);
        }
        __syncthreads();
    }
}

// ---- test images (focr --test: draw_test_rectangles, draw_test_text) ------------------------------------------------

constexpr uint32_t TEST_THREADS = 256;

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
    const uint32_t page = slot / g.n_slots, i = slot % g.n_slots;
    uint32_t yc, h;
    slot_rows(g, i, &yc, &h);
    const uint8_t *src = pages + (size_t)page * g.page_w * g.page_h + (size_t)yc * g.page_w + g.x;
    int ink = 0;
    const uint64_t n = (uint64_t)g.w * h;
    for (uint64_t k = threadIdx.x; k < n; k += TEST_THREADS) ink |= src[(k / g.w) * g.page_w + k % g.w] != 255;
    ink = __syncthreads_or(ink);
    if (threadIdx.x == 0) flags[slot] = ink ? 1u : 0u;
}

// 7. render() of the whole alphabet at (0, 0) on a page of g, one wave
__global__ __launch_bounds__(64) void test_layout_kernel(Geometry g, uint32_t n_glyphs, const DevGlyph *__restrict__ glyphs,
                                                         const VerifyGlyph *__restrict__ vglyphs, const VerifyPhase *__restrict__ vphases,
                                                         VerifyRec *__restrict__ recs, VerifyLine *__restrict__ line) {
    layout_line<true>(g, 0, nullptr, n_glyphs, 0, 0, glyphs, vglyphs, vphases, recs, line);
}

// 8. both test images, tile by tile; every thread owns one column of a 16-row, 256-column tile.  The base pixel is
// base's, or (l, l, l, 255) from the luma without one.  rect: the pixel takes the red blend once per box edge through
// it (a corner is on two edges), counted per tile row from the flags of the slots whose box reaches the row; k blends in
// sequence stop early once one leaves the pixel as it was.  text: the last alphabet glyph over the pixel, as in
// verify_compose_kernel, blends (255 - v, 0, 0, 128) where its value v is not zero.  A null output is not drawn.
__global__ __launch_bounds__(VERIFY_TILE_W) void test_compose_kernel(const uint8_t *__restrict__ pages, const uint32_t *__restrict__ base,
                                                                     Geometry g, uint32_t n_pages, uint32_t x_start, uint32_t width,
                                                                     uint32_t tiles_x, uint32_t tiles_y, const uint32_t *__restrict__ flags,
                                                                     const VerifyLine *__restrict__ line, const VerifyRec *__restrict__ recs,
                                                                     const uint8_t *__restrict__ bitmaps, uint32_t *__restrict__ rect,
                                                                     uint32_t *__restrict__ text) {
    __shared__ uint32_t win[VERIFY_TILE_H * VERIFY_TILE_W];  // 1 + index of the last glyph over the pixel
    __shared__ uint32_t n_h[VERIFY_TILE_H], n_v[VERIFY_TILE_H];  // per tile row: boxes with a horizontal edge on it, boxes spanning it
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint64_t per_page = (uint64_t)tiles_x * tiles_y, n_tiles = per_page * n_pages;
    const size_t W = g.page_w, H = g.page_h;
    const int64_t X0 = x_start, X1 = (int64_t)x_start + width;
    const VerifyLine l = text ? *line : VerifyLine{0, 0, 0, 0, 0, 0};
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t page = (uint32_t)(tile / per_page), rem = (uint32_t)(tile % per_page);
        const int r0 = (int)((rem / tiles_x) * VERIFY_TILE_H), c0 = (int)((rem % tiles_x) * VERIFY_TILE_W);
        const int r1 = std::min<int>(r0 + VERIFY_TILE_H, (int)H), c1 = std::min<int>(c0 + VERIFY_TILE_W, (int)W);
        for (uint32_t r = 0; r < VERIFY_TILE_H; r++) win[r * VERIFY_TILE_W + t] = 0;
        if (t < VERIFY_TILE_H) n_h[t] = 0, n_v[t] = 0;
        __syncthreads();
        if (rect && g.n_slots) {  // slots i with y_i <= r1 - 1 and y_i + line_height >= r0
            const int64_t lo = (int64_t)r0 - g.line_height - g.y_start, hi = (int64_t)r1 - 1 - g.y_start;
            const int64_t i_lo = lo <= 0 ? 0 : (lo + g.line_advance - 1) / g.line_advance;
            const int64_t i_hi = hi < 0 ? -1 : std::min<int64_t>(g.n_slots - 1, hi / g.line_advance);
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
        if (glyphs_here)
            for (uint32_t j = wave; j < l.n; j += VERIFY_TILE_W / 64) {
                const VerifyRec r = recs[j];
                const int x0 = std::max(r.x0, c0), x1 = std::min(r.x1, c1), y0 = std::max(r.y0, r0), y1 = std::min(r.y1, r1);
                if (x0 >= x1 || y0 >= y1) continue;
                const int w = x1 - x0, npx = w * (y1 - y0);
                for (int q = (int)lane; q < npx; q += 64)
                    atomicMax(&win[(y0 + q / w - r0) * VERIFY_TILE_W + (x0 + q % w - c0)], j + 1);
            }
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
                            const VerifyRec r = recs[w - 1];
                            const uint32_t v = bitmaps[r.src + (uint32_t)(y - r.y0) * r.stride + (uint32_t)(x - r.x0)];
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

struct focr_decoder {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    // font
    uint32_t n_glyphs = 0;
    float origin_x = 0.f, min_inc = 0.f;
    std::vector<float> inc;
    std::vector<focr_decode_glyph_t> font_glyphs;  // what set_verify_font checks and places the verify table against
    float origin_y = 0.f, text_size = 0.f, kerning = 0.f;
    int hinting = 0;
    size_t bitmaps_len = 0;
    // every device array: exact growth, no stream wait (each call ends with one, so the buffers are idle when the next call grows them)
    focr::DevArray<DevGlyph> d_glyphs;
    focr::DevArray<int2> d_offs;
    focr::DevArray<uint8_t> d_bitmaps;  // dwords (read as uint32_t by the decode kernel, as bytes by the compose kernels)
    // batch buffers (grown on demand)
    focr::DevArray<uint8_t> d_pages, d_strips;
    focr::DevArray<uint32_t> d_flags, d_work, d_nchars, d_count;
    focr::DevArray<uint16_t> d_chars;
    // results of the last run
    std::vector<focr_decoded_line_t> lines;
    std::vector<uint16_t> chars;
    float last_ms = 0.f;
    uint32_t last_launches = 0;
    // verify: the table, what the last successful run left for it, buffers, timing
    hipEvent_t ev2 = nullptr, ev3 = nullptr;
    uint32_t n_vglyphs = 0, hmax = 0;
    focr::DevArray<VerifyGlyph> d_vglyphs;
    focr::DevArray<VerifyPhase> d_vphases;
    bool run_ok = false;
    Geometry run_g{};
    size_t run_pages = 0;
    uint32_t run_x_start = 0;
    const uint8_t *run_src = nullptr;
    focr::DevArray<VerifyLine> d_vlines;
    focr::DevArray<VerifyRec> d_vrecs;
    focr::DevArray<unsigned long long> d_sums;
    focr::DevArray<uint8_t> d_rgb;
    float last_verify_ms = 0.f;
    uint32_t last_verify_launches = 0;
    // test images: buffers of their own, so that a test call leaves the last run and its verify as they were
    hipEvent_t ev4 = nullptr, ev5 = nullptr;
    focr::DevArray<uint8_t> d_tpages;
    focr::DevArray<uint32_t> d_tbase, d_trect, d_ttext, d_tflags;
    focr::DevArray<VerifyRec> d_trecs;
    focr::DevArray<VerifyLine> d_tline;
    float last_test_ms = 0.f;
    uint32_t last_test_launches = 0;
};

namespace {

thread_local std::string g_dec_err;

int dfail(focr_decoder *dec, const std::string &msg) {
    if (dec) dec->err = msg;
    g_dec_err = msg;
    return 1;
}

#define DEC_CHECK(call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) return dfail(dec, std::string(#call ": ") + hipGetErrorString(e_));    \
    } while (0)

// exact growth of a batch buffer / a fresh table from host memory, reported as the allocation they are
#define DEC_GROW(a, want)                                                                                                          \
    do {                                                                                                                           \
        hipError_t e_ = (a).reserve((want), focr::Grow::exact, nullptr);                                                           \
        if (e_ != hipSuccess) return dfail(dec, std::string("hipMalloc((void **)p, want * sizeof(T)): ") + hipGetErrorString(e_)); \
    } while (0)
#define DEC_UPLOAD(a, ...)                                                                                          \
    do {                                                                                                            \
        hipError_t e_ = (a).upload(__VA_ARGS__);                                                                    \
        if (e_ != hipSuccess) return dfail(dec, std::string("hipMalloc / hipMemcpy(" #a "): ") + hipGetErrorString(e_)); \
    } while (0)

// The line slots of a batch as the reference's loop visits them, with image::crop_imm's clamping of every crop.  False
// for line_advance 0 with a non-empty first crop (the reference never ends).
bool slot_geometry(size_t page_w, size_t page_h, uint32_t x_start, uint32_t y_start, uint32_t width, uint32_t line_height,
                   uint32_t line_advance, Geometry *out) {
    Geometry g{};
    g.page_w = (uint32_t)page_w;
    g.page_h = (uint32_t)page_h;
    g.x = std::min<uint32_t>(x_start, g.page_w);  // image::crop_imm's clamping
    g.w = std::min<uint32_t>(width, g.page_w - g.x);
    g.y_start = y_start;
    g.line_height = line_height;
    g.line_advance = line_advance;
    if (line_height == 0 || y_start >= g.page_h) g.n_slots = 0;  // the first crop is empty: the loop ends at once
    else if (line_advance == 0) return false;
    else g.n_slots = (uint32_t)(((uint64_t)g.page_h - y_start + line_advance - 1) / line_advance);
    *out = g;
    return true;
}

// What focr_decoder_verify draws from: the successful run's geometry and its pages on the device.
int remember_run(focr_decoder *dec, const Geometry &g, const uint8_t *d_src, size_t n_pages, uint32_t x_start) {
    dec->run_g = g;
    dec->run_pages = n_pages;
    dec->run_x_start = x_start;
    dec->run_src = d_src;
    dec->run_ok = true;
    return 0;
}

// A run with no line slot launches nothing, but a verify of it still draws the pages: they go to the device here.
int keep_run(focr_decoder *dec, const Geometry &g, const uint8_t *pages, int on_device, size_t n_pages, uint32_t x_start) {
    const uint8_t *d_src = pages;
    const size_t page_bytes = (size_t)g.page_w * g.page_h * n_pages;
    if (!on_device && page_bytes) {
        DEC_CHECK(hipSetDevice(dec->device));
        DEC_GROW(dec->d_pages, page_bytes);
        DEC_CHECK(hipMemcpyAsync(dec->d_pages, pages, page_bytes, hipMemcpyHostToDevice, dec->stream));
        DEC_CHECK(hipStreamSynchronize(dec->stream));
        d_src = dec->d_pages;
    }
    return remember_run(dec, g, d_src, n_pages, x_start);
}

}  // namespace

extern "C" int focr_decoder_create(int device, focr_decoder_t **out) {
    focr_decoder *dec = nullptr;
    if (!out) return dfail(nullptr, "focr_decoder_create: null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return dfail(nullptr, "no HIP device available (the focr decoder has no CPU fallback)");
    if (device < 0 || device >= n) return dfail(nullptr, "focr_decoder_create: device index out of range");
    DEC_CHECK(hipSetDevice(device));
    dec = new focr_decoder;
    dec->device = device;
    if (hipStreamCreateWithFlags(&dec->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&dec->ev0) != hipSuccess ||
        hipEventCreate(&dec->ev1) != hipSuccess || hipEventCreate(&dec->ev2) != hipSuccess || hipEventCreate(&dec->ev3) != hipSuccess ||
        hipEventCreate(&dec->ev4) != hipSuccess || hipEventCreate(&dec->ev5) != hipSuccess) {
        focr_decoder_destroy(dec);
        return dfail(nullptr, "focr_decoder_create: stream / event creation failed");
    }
    *out = dec;
    return 0;
}

extern "C" void focr_decoder_destroy(focr_decoder_t *dec) {
    if (!dec) return;
    (void)hipSetDevice(dec->device);
    if (dec->stream) (void)hipStreamSynchronize(dec->stream);
    for (hipEvent_t e : {dec->ev0, dec->ev1, dec->ev2, dec->ev3, dec->ev4, dec->ev5})
        if (e) (void)hipEventDestroy(e);
    if (dec->stream) (void)hipStreamDestroy(dec->stream);
    delete dec;  // every device array of the decoder dies here, behind the wait above
}

extern "C" const char *focr_decoder_last_error(const focr_decoder_t *dec) { return dec ? dec->err.c_str() : g_dec_err.c_str(); }

extern "C" int focr_decoder_set_font(focr_decoder_t *dec, const focr_decode_font_t *font) {
    if (dec) dec->run_ok = false, dec->n_vglyphs = 0;  // the last run and the verify table belong to the previous font
    if (!dec || !font || !font->glyphs || !font->n_glyphs) return dfail(dec, "focr_decoder_set_font: bad arguments");
    if (font->n_glyphs > 65535) return dfail(dec, "focr_decoder_set_font: more than 65535 glyphs");
    if (font->bitmaps_len % 4 || font->bitmaps_len / 4 > 0xffffffffull) return dfail(dec, "focr_decoder_set_font: bad bitmap table");
    DEC_CHECK(hipSetDevice(dec->device));
    const size_t G = font->n_glyphs;
    std::vector<DevGlyph> gl(G);
    std::vector<int2> offs(G * FOCR_DECODE_PHASES);
    dec->inc.assign(G, 0.f);
    float min_inc = font->glyphs[0].increment;
    for (size_t i = 0; i < G; i++) {
        const focr_decode_glyph_t &s = font->glyphs[i];
        if (!(s.increment > 0.f)) return dfail(dec, "focr_decoder_set_font: a glyph does not advance the pen");
        if (s.stride % 4 || s.stride < s.box_w || s.offset % 4 ||
            s.offset + (uint64_t)FOCR_DECODE_PHASES * s.stride * s.box_h > font->bitmaps_len ||
            (uint64_t)s.stride * s.box_h * 2 * 255 * 255 >= (1ull << 31))
            return dfail(dec, "focr_decoder_set_font: inconsistent glyph table");
        gl[i] = DevGlyph{(uint32_t)(s.offset / 4), s.stride / 4, s.box_h, s.increment};
        for (int p = 0; p < FOCR_DECODE_PHASES; p++) offs[i * FOCR_DECODE_PHASES + p] = make_int2(s.off_x[p], s.off_y[p]);
        dec->inc[i] = s.increment;
        min_inc = std::min(min_inc, s.increment);
    }
    dec->n_glyphs = 0;
    DEC_UPLOAD(dec->d_glyphs, gl.data(), G);
    DEC_UPLOAD(dec->d_offs, offs.data(), offs.size());
    DEC_UPLOAD(dec->d_bitmaps, (const uint8_t *)font->bitmaps, font->bitmaps_len, 4);
    dec->n_glyphs = (uint32_t)G;
    dec->origin_x = font->origin_x;
    dec->min_inc = min_inc;
    dec->font_glyphs.assign(font->glyphs, font->glyphs + G);
    dec->origin_y = font->origin_y;
    dec->text_size = font->text_size;
    dec->kerning = font->kerning;
    dec->hinting = font->hinting;
    dec->bitmaps_len = font->bitmaps_len;
    return 0;
}

extern "C" int focr_decoder_run(focr_decoder_t *dec, const uint8_t *pages, int on_device, size_t n_pages, size_t page_w, size_t page_h,
                                uint32_t x_start, uint32_t y_start, uint32_t width, uint32_t line_height, uint32_t line_advance) {
    if (!dec) return dfail(nullptr, "focr_decoder_run: null decoder");
    dec->run_ok = false;
    dec->lines.clear();
    dec->chars.clear();
    dec->last_ms = 0.f;
    dec->last_launches = 0;
    if (!dec->n_glyphs) return dfail(dec, "focr_decoder_run: no font (focr_decoder_set_font)");
    if (n_pages && !pages) return dfail(dec, "focr_decoder_run: null pages");
    if (page_w > 0xffffu * 16 || page_h > 0xffffu * 16) return dfail(dec, "focr_decoder_run: page too large");
    Geometry g{};
    if (!slot_geometry(page_w, page_h, x_start, y_start, width, line_height, line_advance, &g))
        return dfail(dec, "focr_decoder_run: line_advance 0 (the reference never ends)");
    const uint64_t total = (uint64_t)n_pages * g.n_slots;
    if (total == 0) return keep_run(dec, g, pages, on_device, n_pages, x_start);  // nothing to decode; a verify still draws the pages
    if (total > (1u << 30)) return dfail(dec, "focr_decoder_run: too many lines in one batch");
    g.total = (uint32_t)total;
    g.stride = ((g.w + PAD + 3) / 4 + 2) * 4;
    // characters per line at most: the pen moves at least min_inc per step, and f32 rounding is monotone, so the
    // sequence 0, min_inc, ... reaches w no earlier than any pen does
    {
        float p = 0.f;
        uint32_t steps = 0;
        while (p < (float)g.w) {
            p = p + dec->min_inc;
            if (++steps > (1u << 20)) return dfail(dec, "focr_decoder_run: the pen advance is too small for the line width");
        }
        g.cap = std::max<uint32_t>(steps, 1);
    }
    DEC_CHECK(hipSetDevice(dec->device));
    const size_t page_bytes = page_w * page_h * n_pages;
    const uint8_t *d_src = pages;
    if (!on_device) {
        DEC_GROW(dec->d_pages, std::max<size_t>(page_bytes, 1));
        DEC_CHECK(hipMemcpyAsync(dec->d_pages, pages, page_bytes, hipMemcpyHostToDevice, dec->stream));
        d_src = dec->d_pages;
    }
    const size_t strip_bytes = (size_t)g.stride * g.line_height;
    DEC_GROW(dec->d_strips, strip_bytes * total);
    DEC_GROW(dec->d_flags, total);
    DEC_GROW(dec->d_work, total);
    DEC_GROW(dec->d_nchars, total);
    DEC_GROW(dec->d_count, 1);
    DEC_GROW(dec->d_chars, (size_t)g.cap * total);

    DEC_CHECK(hipEventRecord(dec->ev0, dec->stream));
    line_prepass_kernel<<<g.total, PREPASS_THREADS, 0, dec->stream>>>(d_src, g, dec->d_strips, dec->d_flags);
    DEC_CHECK(hipGetLastError());
    line_compact_kernel<<<1, COMPACT_THREADS, 0, dec->stream>>>(dec->d_flags, g.total, dec->d_work, dec->d_count);
    DEC_CHECK(hipGetLastError());
    if (strip_bytes <= LDS_STRIP_MAX)
        line_decode_kernel<true><<<g.total, 64, strip_bytes, dec->stream>>>(dec->d_strips, g, dec->d_work, dec->d_count, dec->d_glyphs, dec->d_offs,
                                                                         dec->d_bitmaps.as<const uint32_t>(), dec->n_glyphs, dec->origin_x, dec->d_nchars, dec->d_chars);
    else
        line_decode_kernel<false><<<g.total, 64, 0, dec->stream>>>(dec->d_strips, g, dec->d_work, dec->d_count, dec->d_glyphs, dec->d_offs,
                                                                dec->d_bitmaps.as<const uint32_t>(), dec->n_glyphs, dec->origin_x, dec->d_nchars, dec->d_chars);
    DEC_CHECK(hipGetLastError());
    DEC_CHECK(hipEventRecord(dec->ev1, dec->stream));

    uint32_t count = 0;
    std::vector<uint32_t> work(total), nch(total);
    std::vector<uint16_t> all((size_t)g.cap * total);
    DEC_CHECK(hipMemcpyAsync(&count, dec->d_count, 4, hipMemcpyDeviceToHost, dec->stream));
    DEC_CHECK(hipMemcpyAsync(work.data(), dec->d_work, total * 4, hipMemcpyDeviceToHost, dec->stream));
    DEC_CHECK(hipMemcpyAsync(nch.data(), dec->d_nchars, total * 4, hipMemcpyDeviceToHost, dec->stream));
    DEC_CHECK(hipMemcpyAsync(all.data(), dec->d_chars, all.size() * 2, hipMemcpyDeviceToHost, dec->stream));
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    DEC_CHECK(hipEventElapsedTime(&dec->last_ms, dec->ev0, dec->ev1));
    dec->last_launches = 3;
    if (count > total) return dfail(dec, "focr_decoder_run: inconsistent line count from the device");
    dec->lines.resize(count);
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t slot = work[k], n = nch[k];
        if (slot >= total || n > g.cap) return dfail(dec, "focr_decoder_run: inconsistent result from the device");
        focr_decoded_line_t &l = dec->lines[k];
        l.page = slot / g.n_slots;
        l.y = y_start + (slot % g.n_slots) * line_advance;
        l.first = dec->chars.size();
        l.n_chars = n;
        l.pad = 0;
        dec->chars.insert(dec->chars.end(), all.begin() + (size_t)k * g.cap, all.begin() + (size_t)k * g.cap + n);
    }
    return remember_run(dec, g, d_src, n_pages, x_start);
}

extern "C" size_t focr_decoder_n_lines(const focr_decoder_t *dec) { return dec ? dec->lines.size() : 0; }
extern "C" size_t focr_decoder_n_chars(const focr_decoder_t *dec) { return dec ? dec->chars.size() : 0; }

extern "C" int focr_decoder_get(const focr_decoder_t *dec, focr_decoded_line_t *lines, uint16_t *chars) {
    if (!dec) return dfail(nullptr, "focr_decoder_get: null decoder");
    if (lines && !dec->lines.empty()) memcpy(lines, dec->lines.data(), dec->lines.size() * sizeof(focr_decoded_line_t));
    if (chars && !dec->chars.empty()) memcpy(chars, dec->chars.data(), dec->chars.size() * sizeof(uint16_t));
    return 0;
}

extern "C" float focr_decoder_last_ms(const focr_decoder_t *dec) { return dec ? dec->last_ms : 0.f; }
extern "C" uint32_t focr_decoder_last_launches(const focr_decoder_t *dec) { return dec ? dec->last_launches : 0; }

extern "C" int focr_decoder_set_verify_font(focr_decoder_t *dec, const focr_verify_font_t *font) {
    if (!dec) return dfail(nullptr, "focr_decoder_set_verify_font: null decoder");
    dec->n_vglyphs = 0;
    if (!font || !font->glyphs || !font->n_glyphs) return dfail(dec, "focr_decoder_set_verify_font: bad arguments");
    if (!dec->n_glyphs) return dfail(dec, "focr_decoder_set_verify_font: no decode font (focr_decoder_set_font)");
    const size_t G = font->n_glyphs;
    if (G != dec->n_glyphs || font->text_size != dec->text_size || font->kerning != dec->kerning ||
        (font->hinting != 0) != (dec->hinting != 0) || font->origin_y != dec->origin_y)
        return dfail(dec, "focr_decoder_set_verify_font: the table does not match the decode font (glyph count, size, kerning, hinting or origin)");
    if (dec->bitmaps_len > 0xffffffffull) return dfail(dec, "focr_decoder_set_verify_font: decode font bitmaps over 4 GiB");
    std::vector<VerifyGlyph> vg(G);
    std::vector<VerifyPhase> vp(G * FOCR_DECODE_PHASES);
    int y_lo = 0, y_hi = 0;
    for (size_t i = 0; i < G; i++) {
        const focr_verify_glyph_t &v = font->glyphs[i];
        const focr_decode_glyph_t &d = dec->font_glyphs[i];
        if (v.codepoint != d.codepoint || memcmp(&v.increment, &d.increment, sizeof(float)) != 0)
            return dfail(dec, "focr_decoder_set_verify_font: the table does not match the decode font (code points or increments)");
        for (float b : v.box)
            if (!std::isfinite(b) || std::fabs(b) > (float)(1 << 20)) return dfail(dec, "focr_decoder_set_verify_font: bad glyph box");
        memcpy(vg[i].box, v.box, sizeof v.box);
        y_lo = std::min(y_lo, (int)std::floor(v.box[1] + 0.f));  // the rows render() gives any line: at most hmax
        y_hi = std::max(y_hi, (int)std::ceil(v.box[3] + 0.f));
        for (int p = 0; p < FOCR_DECODE_PHASES; p++) {
            if ((uint64_t)v.rect_x[p] + v.rect_w[p] > d.box_w || (uint64_t)v.rect_y[p] + v.rect_h[p] > d.box_h)
                return dfail(dec, "focr_decoder_set_verify_font: a phase rectangle leaves the decode font's box");
            vp[i * FOCR_DECODE_PHASES + p] = VerifyPhase{
                d.off_x[p] + (int32_t)v.rect_x[p], d.off_y[p] + (int32_t)v.rect_y[p] - (int32_t)font->origin_y, v.rect_w[p], v.rect_h[p],
                (uint32_t)(d.offset + (uint64_t)p * d.stride * d.box_h + (uint64_t)v.rect_y[p] * d.stride + v.rect_x[p]), d.stride};
        }
    }
    DEC_CHECK(hipSetDevice(dec->device));
    DEC_UPLOAD(dec->d_vglyphs, vg.data(), G);
    DEC_UPLOAD(dec->d_vphases, vp.data(), vp.size());
    dec->hmax = (uint32_t)(y_hi - y_lo);
    dec->n_vglyphs = (uint32_t)G;
    return 0;
}

extern "C" int focr_decoder_verify(focr_decoder_t *dec, uint8_t *rgb, int rgb_on_device, uint64_t *sq_sums) {
    if (!dec) return dfail(nullptr, "focr_decoder_verify: null decoder");
    dec->last_verify_ms = 0.f;
    dec->last_verify_launches = 0;
    if (!dec->run_ok) return dfail(dec, "focr_decoder_verify: no successful focr_decoder_run since the font was set");
    if (!dec->n_vglyphs) return dfail(dec, "focr_decoder_verify: no verify table (focr_decoder_set_verify_font)");
    if (!sq_sums) return dfail(dec, "focr_decoder_verify: null sq_sums");
    const Geometry &g = dec->run_g;
    const size_t n_pages = dec->run_pages;
    if (n_pages == 0) return 0;
    const size_t W = g.page_w, H = g.page_h, px = n_pages * W * H;
    const size_t tiles_x = (W + VERIFY_TILE_W - 1) / VERIFY_TILE_W, tiles_y = (H + VERIFY_TILE_H - 1) / VERIFY_TILE_H;
    const size_t n_tiles = n_pages * tiles_x * tiles_y;
    const size_t layout_blocks = std::max<size_t>(g.total, n_pages);
    if (layout_blocks > 0x7fffffffu) return dfail(dec, "focr_decoder_verify: too many pages in one batch");
    DEC_CHECK(hipSetDevice(dec->device));
    DEC_GROW(dec->d_vlines, std::max<size_t>(g.total, 1));
    DEC_GROW(dec->d_vrecs, std::max<size_t>((size_t)g.total * g.cap, 1));
    DEC_GROW(dec->d_sums, n_pages);
    uint8_t *d_rgb = rgb_on_device ? rgb : nullptr;
    if (rgb && !rgb_on_device) {
        DEC_GROW(dec->d_rgb, std::max<size_t>(px * 3, 1));
        d_rgb = dec->d_rgb;
    }
    DEC_CHECK(hipEventRecord(dec->ev2, dec->stream));
    verify_layout_kernel<<<(uint32_t)layout_blocks, 64, 0, dec->stream>>>(g, (uint32_t)n_pages, dec->run_x_start, dec->d_flags, dec->d_work,
                                                                         dec->d_count, dec->d_nchars, dec->d_chars, dec->d_glyphs,
                                                                         dec->d_vglyphs, dec->d_vphases, dec->d_vlines, dec->d_vrecs, dec->d_sums);
    DEC_CHECK(hipGetLastError());
    verify_compose_kernel<<<(uint32_t)std::min<size_t>(std::max<size_t>(n_tiles, 1), VERIFY_MAX_GRID), VERIFY_TILE_W, 0, dec->stream>>>(
        dec->run_src, g, (uint32_t)n_pages, dec->hmax, (uint32_t)tiles_x, (uint32_t)tiles_y, dec->d_vlines, dec->d_vrecs,
        (const uint8_t *)dec->d_bitmaps, d_rgb, dec->d_sums);
    DEC_CHECK(hipGetLastError());
    DEC_CHECK(hipEventRecord(dec->ev3, dec->stream));
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit sums");
    DEC_CHECK(hipMemcpyAsync(sq_sums, dec->d_sums, n_pages * sizeof(uint64_t), hipMemcpyDeviceToHost, dec->stream));
    if (rgb && !rgb_on_device) DEC_CHECK(hipMemcpyAsync(rgb, dec->d_rgb, px * 3, hipMemcpyDeviceToHost, dec->stream));
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    DEC_CHECK(hipEventElapsedTime(&dec->last_verify_ms, dec->ev2, dec->ev3));
    dec->last_verify_launches = 2;
    return 0;
}

extern "C" float focr_decoder_last_verify_ms(const focr_decoder_t *dec) { return dec ? dec->last_verify_ms : 0.f; }
extern "C" uint32_t focr_decoder_last_verify_launches(const focr_decoder_t *dec) { return dec ? dec->last_verify_launches : 0; }

extern "C" int focr_decoder_test_images(focr_decoder_t *dec, const uint8_t *pages, const uint8_t *base_rgba, int in_on_device, size_t n_pages,
                                        size_t page_w, size_t page_h, uint32_t x_start, uint32_t y_start, uint32_t width,
                                        uint32_t line_height, uint32_t line_advance, uint8_t *rect_rgba, uint8_t *text_rgba,
                                        int out_on_device) {
    if (!dec) return dfail(nullptr, "focr_decoder_test_images: null decoder");
    dec->last_test_ms = 0.f;
    dec->last_test_launches = 0;
    if (n_pages && !pages) return dfail(dec, "focr_decoder_test_images: null pages");
    if (text_rgba && !dec->n_glyphs) return dfail(dec, "focr_decoder_test_images: the text image needs a decode font (focr_decoder_set_font)");
    if (text_rgba && !dec->n_vglyphs)
        return dfail(dec, "focr_decoder_test_images: the text image needs a verify table (focr_decoder_set_verify_font)");
    if (page_w > 0xffffu * 16 || page_h > 0xffffu * 16) return dfail(dec, "focr_decoder_test_images: page too large");
    Geometry g{};
    if (!slot_geometry(page_w, page_h, x_start, y_start, width, line_height, line_advance, &g))
        return dfail(dec, "focr_decoder_test_images: line_advance 0 (the reference never ends)");
    const uint64_t total = (uint64_t)n_pages * g.n_slots;
    if (total > (1u << 30)) return dfail(dec, "focr_decoder_test_images: too many lines in one batch");
    g.total = (uint32_t)total;
    for (const void *p : {in_on_device ? (const void *)base_rgba : nullptr, out_on_device ? (const void *)rect_rgba : nullptr,
                          out_on_device ? (const void *)text_rgba : nullptr})
        if ((uintptr_t)p % 4) return dfail(dec, "focr_decoder_test_images: device RGBA buffers must be 4-byte aligned");
    const size_t W = page_w, H = page_h, px = n_pages * W * H;
    if (px == 0 || (!rect_rgba && !text_rgba)) return 0;
    const size_t tiles_x = (W + VERIFY_TILE_W - 1) / VERIFY_TILE_W, tiles_y = (H + VERIFY_TILE_H - 1) / VERIFY_TILE_H;
    const size_t n_tiles = n_pages * tiles_x * tiles_y;
    DEC_CHECK(hipSetDevice(dec->device));
    const uint8_t *d_src = pages;
    const uint32_t *d_base = (const uint32_t *)base_rgba;
    if (!in_on_device) {
        DEC_GROW(dec->d_tpages, px);
        DEC_CHECK(hipMemcpyAsync(dec->d_tpages, pages, px, hipMemcpyHostToDevice, dec->stream));
        d_src = dec->d_tpages;
        if (base_rgba) {
            DEC_GROW(dec->d_tbase, px);
            DEC_CHECK(hipMemcpyAsync(dec->d_tbase, base_rgba, px * 4, hipMemcpyHostToDevice, dec->stream));
            d_base = dec->d_tbase;
        }
    }
    uint32_t *d_rect = (uint32_t *)rect_rgba, *d_text = (uint32_t *)text_rgba;
    if (!out_on_device) {
        if (rect_rgba) DEC_GROW(dec->d_trect, px);
        if (text_rgba) DEC_GROW(dec->d_ttext, px);
        d_rect = rect_rgba ? dec->d_trect : nullptr;
        d_text = text_rgba ? dec->d_ttext : nullptr;
    }
    if (rect_rgba) DEC_GROW(dec->d_tflags, std::max<size_t>(total, 1));
    if (text_rgba) {
        DEC_GROW(dec->d_trecs, dec->n_glyphs);
        DEC_GROW(dec->d_tline, 1);
    }
    uint32_t launches = 0;
    DEC_CHECK(hipEventRecord(dec->ev4, dec->stream));
    if (rect_rgba) {
        test_flags_kernel<<<std::max<uint32_t>(g.total, 1), TEST_THREADS, 0, dec->stream>>>(d_src, g, dec->d_tflags);
        DEC_CHECK(hipGetLastError());
        launches++;
    }
    if (text_rgba) {
        test_layout_kernel<<<1, 64, 0, dec->stream>>>(g, dec->n_glyphs, dec->d_glyphs, dec->d_vglyphs, dec->d_vphases, dec->d_trecs, dec->d_tline);
        DEC_CHECK(hipGetLastError());
        launches++;
    }
    test_compose_kernel<<<(uint32_t)std::min<size_t>(n_tiles, VERIFY_MAX_GRID), VERIFY_TILE_W, 0, dec->stream>>>(
        d_src, d_base, g, (uint32_t)n_pages, x_start, width, (uint32_t)tiles_x, (uint32_t)tiles_y, dec->d_tflags, dec->d_tline, dec->d_trecs,
        (const uint8_t *)dec->d_bitmaps, d_rect, d_text);
    DEC_CHECK(hipGetLastError());
    launches++;
    DEC_CHECK(hipEventRecord(dec->ev5, dec->stream));
    if (!out_on_device) {
        if (rect_rgba) DEC_CHECK(hipMemcpyAsync(rect_rgba, d_rect, px * 4, hipMemcpyDeviceToHost, dec->stream));
        if (text_rgba) DEC_CHECK(hipMemcpyAsync(text_rgba, d_text, px * 4, hipMemcpyDeviceToHost, dec->stream));
    }
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    DEC_CHECK(hipEventElapsedTime(&dec->last_test_ms, dec->ev4, dec->ev5));
    dec->last_test_launches = launches;
    return 0;
}

extern "C" float focr_decoder_last_test_ms(const focr_decoder_t *dec) { return dec ? dec->last_test_ms : 0.f; }
extern "C" uint32_t focr_decoder_last_test_launches(const focr_decoder_t *dec) { return dec ? dec->last_test_launches : 0; }

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
