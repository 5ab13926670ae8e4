// decode.h — what the files of the `focr` decoder share:
//   decode.hip                 the font, the settings' resolution into one RunMode, the run in its steps, prepass, compaction,
//                              the pen loop and its search
//   decode_whole.hip           the whole-line decode, with margins or a pen slack
//   decode_baseline.hip        the baseline search on either line grid, its y-phase fonts and the verify's compose after a baseline run
//   decode_whole_baseline.hip  the whole-line decode under every baseline candidate, on either line grid
//   decode_line_frac.hip       the fractional line grid's setter and the verify's compose on that grid
//   decode_fonts.hip           the font search: the pen loop under every candidate font, the candidates' upload, the getter
//   decode_whole_fonts.hip     the whole-line decode under every candidate font
//   decode_images.hip          the verify and --test images
//   decode_text.hip            verify_text: a caller's lines drawn over their pages, each in any uploaded font
//   decode_score.hip           score_text: the decoder's cost of a caller's lines, each in any uploaded font (over decode_pen.h)
//   decode_align.hip           align_text: a caller's lines with every character's pen fitted to the page (over decode_score.h, align_plan.h)
//   decode_learn.hip           learn_text: the page's luma summed under every (glyph, phase) cell of a caller's lines (over decode_score.h)
//   decode_refine.hip          refine_text: a caller's lines repaired against the composed line error (over decode_score.h, refine_plan.h)
// (decode_line.h lies between decode.h and the files of a run; decode_line_frac.hip, decode_images.hip and decode_text.hip include decode.h alone.)
// Below decode.h lie text_plan.h, host code alone (the input rules of a caller's reading and the record the device reads of a line),
// align_plan.h and refine_plan.h on top of it (the host plans of align_text: nominal pens, the 2^24 rule, the backpointers' budget;
// and of refine_text: the monotone pens, the fonts' extents, a step's window), and
// decode_font.h, host code alone: the record of an uploaded font (HostFont), the glyph and verify records the kernels
// read, and the five font uploaders' checks and packing.  Here: the batch geometry, both line grids, the owners of the fonts' device tables, the tile frame of
// the compose kernels (ncc_images.hip is its third user), the blank test's crop, the settings (Modes), what a run resolves
// them to (RunMode), what the last run left (LastRun), the decoder itself, and the host plumbing every entry point repeats
// (errors, stages, staging, refusals).
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "decode_font.h"
#include "devmem.h"
#include "align_plan.h"
#include "focr_decode.h"
#include "refine_plan.h"
#include "text_plan.h"

namespace focr_dec {

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

// The crop of (page, line) slot `slot` < g.total as image::crop_imm clamps it: its first pixel; g.w columns by *h rows.
__device__ __forceinline__ const uint8_t *slot_crop(const uint8_t *__restrict__ pages, const Geometry &g, uint32_t slot, uint32_t *h) {
    uint32_t yc;
    slot_rows(g, slot % g.n_slots, &yc, h);
    return pages + (size_t)(slot / g.n_slots) * g.page_w * g.page_h + (size_t)yc * g.page_w + g.x;
}

// ---- the fractional line grid (focr_decoder_set_line_frac; include/focr_decode.h): slot i's top is at
// Y_i = 64 * y_start + y_frac + i * (64 * line_advance + advance_frac) in 1/64 px.  At (0, 0) it is the whole-pixel grid, integer
// for integer, so a kernel that takes a LineFrac serves both grids: line_baseline_kernel (decode_baseline.hip) and
// verify_layout_kernel (decode_images.hip) do.  Three kernels still have a form of their own on this grid beside the one it
// restates, which keeps its arguments and its instruction stream (tools/isa_hash.py): line_prepass_frac_kernel (the plain decode's
// first launch stays untouched), line_whole_baseline_frac_kernel and verify_compose_moved_frac_kernel (as the only kernel of their
// kind each was measurably slower with the grid off).  The device helpers the forms share (the prepass of a slot,
// whole_stage, layout_line) take the grid as a policy: PixelGrid is the whole-pixel grid of slot_rows, an empty type; FracGrid the
// fractional one ----

struct LineFrac {
    uint32_t y_frac, advance_frac;  // each 0 ..= 63; (0, 0) is off
    __host__ __device__ bool on() const { return (y_frac | advance_frac) != 0; }
    __host__ __device__ uint64_t top(const Geometry &g) const { return 64ull * g.y_start + y_frac; }              // Y_0
    __host__ __device__ uint64_t step(const Geometry &g) const { return 64ull * g.line_advance + advance_frac; }  // L
};

// slot_rows on the fractional grid: the crop row yc_i = Y_i >> 6 (clamped), its rows, and f_i = Y_i & 63, the part of a pixel
// the line sits below its crop's top.  i <= n_slots, so i * L stays below 64 * page_h + L.
__device__ __forceinline__ void slot_rows_frac(const Geometry &g, const LineFrac &fr, uint32_t i, uint32_t *yc, uint32_t *h, uint32_t *f) {
    const uint64_t y = fr.top(g) + (uint64_t)i * fr.step(g);
    *yc = (uint32_t)std::min<uint64_t>(y >> 6, g.page_h);
    *h = std::min(g.line_height, g.page_h - *yc);
    *f = (uint32_t)y & 63;
}

// The centre of a line's baseline candidates, in steps of 2^-bits px, halves up: 0 <= c <= 2^bits.
__device__ __forceinline__ int frac_centre(uint32_t f, uint32_t bits) { return (int)(((f << bits) + 32) >> 6); }

// rows: slot i's crop row and rows, and the centre of its baseline candidates for y_bits `bits` (per line, and uniform across
// the workgroup: a handful of scalar integer operations).  row: the slot's y as the verify draws from it.
struct PixelGrid {
    __device__ __forceinline__ void rows(const Geometry &g, uint32_t i, uint32_t bits, uint32_t *yc, uint32_t *h, int *centre) const {
        slot_rows(g, i, yc, h);
        *centre = 0;
    }
    __device__ __forceinline__ int64_t row(const Geometry &g, uint32_t i) const { return (int64_t)g.y_start + (int64_t)i * g.line_advance; }
};

struct FracGrid {
    LineFrac fr;
    __device__ __forceinline__ void rows(const Geometry &g, uint32_t i, uint32_t bits, uint32_t *yc, uint32_t *h, int *centre) const {
        uint32_t f;
        slot_rows_frac(g, fr, i, yc, h, &f);
        *centre = frac_centre(f, bits);
    }
    __device__ __forceinline__ int64_t row(const Geometry &g, uint32_t i) const { return (int64_t)((fr.top(g) + (uint64_t)i * fr.step(g)) >> 6); }
};

constexpr uint32_t TEST_THREADS = 256;

// The blank test of a slot by a workgroup of TEST_THREADS: this thread's share of "some pixel of the crop is not 255"
// (an empty crop counts as all-white), for the caller's __syncthreads_or.
__device__ __forceinline__ int slot_has_ink(const uint8_t *__restrict__ pages, const Geometry &g, uint32_t slot) {
    uint32_t h;
    const uint8_t *src = slot_crop(pages, g, slot, &h);
    int ink = 0;
    const uint64_t n = (uint64_t)g.w * h;
    for (uint64_t k = threadIdx.x; k < n; k += TEST_THREADS) ink |= src[(k / g.w) * g.page_w + k % g.w] != 255;
    return ink;
}

struct VerifyLine {    // one line slot: its canvas on the page, clipped (empty for a blank slot), and its glyph records
    int32_t x0, y0, x1, y1;
    uint32_t k, n;
};

struct VerifyRec {     // one glyph: its bitmap rectangle on the page, clipped to the canvas and the page
    int32_t x0, y0, x1, y1;
    uint32_t src, stride;  // byte offset in the bitmap table of the pixel at (x0, y0)
};

// ---- the tile frame of the compose kernels: a workgroup of VERIFY_TILE_W threads walks (page, tile row, tile column)
// tiles grid-stride; every thread owns one column of the tile, and `win` (one word per tile pixel) takes the glyphs ----

constexpr uint32_t VERIFY_TILE_W = 256;
constexpr uint32_t VERIFY_TILE_H = 16;
constexpr uint32_t VERIFY_MAX_GRID = 1u << 20;

struct TileGrid {
    uint32_t tiles_x, tiles_y;
    uint64_t n_tiles;  // n_pages * tiles_x * tiles_y
    uint32_t grid;     // workgroups to launch: one per tile up to VERIFY_MAX_GRID, and at least one
};

inline TileGrid tile_grid(size_t n_pages, size_t W, size_t H) {
    const size_t tiles_x = (W + VERIFY_TILE_W - 1) / VERIFY_TILE_W, tiles_y = (H + VERIFY_TILE_H - 1) / VERIFY_TILE_H;
    const size_t n_tiles = n_pages * tiles_x * tiles_y;
    return TileGrid{(uint32_t)tiles_x, (uint32_t)tiles_y, n_tiles, (uint32_t)std::min<size_t>(std::max<size_t>(n_tiles, 1), VERIFY_MAX_GRID)};
}

struct Tile {
    uint32_t page;
    int r0, c0, r1, c1;  // rows r0 .. r1 - 1 and columns c0 .. c1 - 1 of the page
};

__device__ __forceinline__ Tile tile_at(uint64_t tile, uint32_t tiles_x, uint32_t tiles_y, uint32_t page_w, uint32_t page_h) {
    const uint64_t per_page = (uint64_t)tiles_x * tiles_y;
    const uint32_t page = (uint32_t)(tile / per_page), rem = (uint32_t)(tile % per_page);
    const int r0 = (int)((rem / tiles_x) * VERIFY_TILE_H), c0 = (int)((rem % tiles_x) * VERIFY_TILE_W);
    return Tile{page, r0, c0, std::min<int>(r0 + VERIFY_TILE_H, (int)page_h), std::min<int>(c0 + VERIFY_TILE_W, (int)page_w)};
}

// The line slots i of g, in order, with y_i <= r1 - 1 and y_i + reach >= r0, where y_i = y_start + i * line_advance:
// *i_lo .. *i_hi, empty when *i_hi < *i_lo.
__device__ __forceinline__ void slot_range(const Geometry &g, int r0, int r1, int64_t reach, int64_t *i_lo, int64_t *i_hi) {
    *i_lo = 0, *i_hi = -1;
    if (!g.n_slots) return;
    const int64_t lo = (int64_t)r0 - reach - g.y_start, hi = (int64_t)r1 - 1 - g.y_start;
    *i_lo = lo <= 0 ? 0 : (lo + g.line_advance - 1) / g.line_advance;
    *i_hi = hi < 0 ? -1 : std::min<int64_t>(g.n_slots - 1, hi / g.line_advance);
}

// slot_range on the fractional grid, exactly: the slots i with yc_i <= r1 - 1 and yc_i + reach >= r0, where
// yc_i = (Y_0 + i * L) >> 6: yc_i <= r is Y_0 + i * L < 64 * (r + 1), and yc_i >= r is Y_0 + i * L >= 64 * r.  L >= 64 when
// there are slots (line_advance 0 is refused).
__device__ __forceinline__ void slot_range_frac(const Geometry &g, const LineFrac &fr, int r0, int r1, int64_t reach, int64_t *i_lo, int64_t *i_hi) {
    *i_lo = 0, *i_hi = -1;
    if (!g.n_slots) return;
    const int64_t Y0 = (int64_t)fr.top(g), L = (int64_t)fr.step(g);
    const int64_t lo = 64 * ((int64_t)r0 - reach) - Y0, hi = 64 * (int64_t)r1 - 1 - Y0;
    *i_lo = lo <= 0 ? 0 : (lo + L - 1) / L;
    *i_hi = hi < 0 ? -1 : std::min<int64_t>(g.n_slots - 1, hi / L);
}

// Every wave takes glyph records of recs[0 .. n), clips them to the tile and leaves base + 1 + index of the last glyph over each
// pixel in win: an LDS atomic max, so neither placement nor arrival order matters.  INK_ONLY: a glyph counts only where its
// bitmap byte is not zero (the NCC images, where a character's zero pixels leave an earlier character's blue standing); base:
// recs is a piece of a longer array whose index orders the glyphs (the caller reads the word back against that array).
template <bool INK_ONLY = false>
__device__ __forceinline__ void mark_glyphs(uint32_t *win, const VerifyRec *__restrict__ recs, uint32_t n, const Tile &T, uint32_t lane,
                                            uint32_t wave, uint32_t base = 0, const uint8_t *__restrict__ bitmaps = nullptr) {
    for (uint32_t j = wave; j < n; j += VERIFY_TILE_W / 64) {
        const VerifyRec r = recs[j];
        const int x0 = std::max(r.x0, T.c0), x1 = std::min(r.x1, T.c1), y0 = std::max(r.y0, T.r0), y1 = std::min(r.y1, T.r1);
        if (x0 >= x1 || y0 >= y1) continue;
        const int w = x1 - x0, npx = w * (y1 - y0);
        for (int q = (int)lane; q < npx; q += 64) {
            const int x = x0 + q % w, y = y0 + q / w;
            if (INK_ONLY && !bitmaps[r.src + (uint32_t)(y - r.y0) * r.stride + (uint32_t)(x - r.x0)]) continue;
            atomicMax(&win[(y - T.r0) * VERIFY_TILE_W + (x - T.c0)], base + j + 1);
        }
    }
}

// The bitmap byte at page pixel (x, y) of the glyph a non-zero win word w names.
__device__ __forceinline__ uint8_t glyph_value(uint32_t w, const VerifyRec *__restrict__ recs, const uint8_t *__restrict__ bitmaps, int x, int y) {
    const VerifyRec r = recs[w - 1];
    return bitmaps[r.src + (uint32_t)(y - r.y0) * r.stride + (uint32_t)(x - r.x0)];
}

// The workgroup's sum of every thread's acc (at most 2^32 in all), added to *sum with one 64-bit atomic by thread 0; `part` is
// VERIFY_TILE_W / 64 words of LDS.  Ends with a barrier: win and part are free again.
__device__ __forceinline__ void tile_add_sum(uint32_t acc, uint32_t *part, unsigned long long *sum, uint32_t t) {
    for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s, 64);
    if ((t & 63) == 0) part[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        unsigned long long total = 0;
        for (uint32_t w = 0; w < VERIFY_TILE_W / 64; w++) total += part[w];
        if (total) atomicAdd(sum, total);
    }
    __syncthreads();
}

// ---- the layout kernels' line (decode_images.hip: the verify of a run and the alphabet of --test; decode_text.hip: a
// caller's lines) ----

// render()'s layout of one line of n glyphs on a page of g, by one wave: the pen (f32 adds in text order), the union
// of round_out boxes folded from the empty rect at (0, 0), and each glyph's true bitmap rectangle clipped to the canvas
// and the page, written to out[0 .. n).  The line is cs[0 .. n) at (x_start, y of g's slot), or for IOTA the alphabet
// indices 0 .. n - 1 at (x_start, 0).  Lane 0 writes the line's canvas on the page to *line, clipped (empty when none
// of it is on the page), with k and n.  js (null: none) is the run's pen search: glyph q is placed at pen + js[q] / 64
// and the pen advances from there, the decoder's own two f32 adds.  ps (null: none) is a whole-line run's pens in
// 1/64 px: glyph q is placed at ps[q] / 64 (exact), whatever the increments before it.  moved is a baseline run's whole rows
// for this line (0: none): the canvas is drawn that many rows below the slot's y, above it when negative, and is then
// clipped at the page's top as well.  grid is the line grid the slot's y is read from: FracGrid with the run's
// fractions for a run's lines ((0, 0) unless the run was made on the fractional grid), and the default where no slot's y is read
// (the alphabet) or the line brings its own (decode_text.hip).
template <bool IOTA, class Grid = PixelGrid>
__device__ __forceinline__ void layout_line(const Geometry &g, uint32_t slot, const uint16_t *__restrict__ cs,
                                            const int8_t *__restrict__ js, const uint32_t *__restrict__ ps, int moved, uint32_t n, uint32_t k,
                                            uint32_t x_start, const DevGlyph *__restrict__ glyphs, const VerifyGlyph *__restrict__ vglyphs,
                                            const VerifyPhase *__restrict__ vphases, VerifyRec *__restrict__ out, VerifyLine *__restrict__ line,
                                            const Grid &grid = Grid{}) {
    const uint32_t lane = threadIdx.x;
    float pen = 0.f;
    int ox = 0, oy = 0, lx = 0, ly = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t j = base + lane, m = std::min(64u, n - base);
        const bool live = j < n;
        const uint32_t c = live ? (IOTA ? j : cs[j]) : 0;
        const float inc = live ? glyphs[c].inc : 0.f;
        const float dj = live && js ? (float)js[j] * 0.015625f : 0.f;
        float pos = live && ps ? __fmul_rn((float)ps[j], 0.015625f) : 0.f;
        for (uint32_t q = 0; q < m && !ps; q++) {
            if (js) pen = __fadd_rn(pen, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dj), q)));
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
    const int64_t line_y = IOTA ? 0 : grid.row(g, slot % g.n_slots) + moved;
    const int top = IOTA ? 0 : (int)std::max<int64_t>(-line_y, 0);  // the canvas rows above the page (a line moved up)
    const float neg_ox = (float)(-ox);
    for (uint32_t j = lane; j < n; j += 64) {
        const float pos = __int_as_float(out[j].x0);
        const int d = (int)__fmul_rn(__fadd_rn(neg_ox, pos), 64.0f);  // FreeType's delta: trunc((-bounds.ox + pos) * 64) >= 0
        const VerifyPhase ph = vphases[(size_t)(IOTA ? j : cs[j]) * FOCR_DECODE_PHASES + (d & 63)];
        const int gx0 = (d >> 6) + ph.x, gy0 = ph.y - oy;  // on the canvas: whole-pixel shift, vertical delta -bounds.oy
        const int ax0 = std::max(gx0, 0), ay0 = std::max(gy0, top);
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
        if ((int64_t)x_start < X1 && line_y + top < Y1) l = VerifyLine{(int32_t)x_start, (int32_t)(line_y + top), (int32_t)X1, (int32_t)Y1, k, n};
        *line = l;
    }
}

// ---- settings, the mode they resolve to, and the last run ------------------------------------------------------------

struct BaseSearch {
    uint32_t bits = 0, n = 0;  // y_bits and radius; n == 0 is off
};

// What the setters write, as they were given; nothing reads them but resolve_modes (decode.hip), once per run.
struct Modes {
    bool scores = false;      // focr_decoder_set_scores
    uint32_t pen_search = 0;  // focr_decoder_set_pen_search
    bool whole = false;       // focr_decoder_set_whole_line
    bool margins = false;     // focr_decoder_set_whole_margins
    uint32_t slack = 0;       // focr_decoder_set_whole_slack
    BaseSearch base, wbase;   // focr_decoder_set_baseline_search, focr_decoder_set_whole_baseline
    LineFrac frac{0, 0};      // focr_decoder_set_line_frac: (0, 0) is off
    bool font_search = false;  // focr_decoder_set_font_search
    uint32_t whole_grid = 0, base_grid = 0, fonts_grid = 0;  // focr_decoder_debug_set_*_grid: at most this many workgroups (0: no limit of the test's)
};

// The third launch of a run (DESIGN.md has the table: kernel, buffers written, getters that answer).
enum class Kind { pen_loop, pen_search, whole, whole_margins, whole_slack, whole_baseline, baseline, fonts, whole_fonts };

// The settings of one run, resolved: every step of the run, and the verify after it, asks this and nothing else.
struct RunMode {
    Kind kind = Kind::pen_loop;
    bool scores = false;  // d_term, d_runner_term, d_runner and d_base are written (pen_loop and pen_search only)
    uint32_t radius = 0;  // what the kind's kernel takes: the pen search's, the pen slack's or the baseline candidates' radius
    uint32_t bits = 0;    // the baseline kinds: d_base_q is in steps of 2^-bits px
    LineFrac frac{0, 0};  // the line grid in force ((0, 0) except under the baseline kinds)
    uint32_t grid = 0;    // the debug limit on the kind's workgroups (the whole and baseline kinds)
    bool whole() const {  // d_pens, d_cost
        return kind == Kind::whole || kind == Kind::whole_margins || kind == Kind::whole_slack || kind == Kind::whole_baseline || kind == Kind::whole_fonts;
    }
    bool margins() const { return kind == Kind::whole_margins; }                                 // d_mterm, d_mrunner, d_margin
    bool offsets() const { return kind == Kind::pen_search || kind == Kind::whole_slack; }       // d_pen holds offsets
    bool base_q() const { return kind == Kind::baseline || kind == Kind::whole_baseline; }       // d_base_q (and d_base_cost: baseline)
    bool fonts() const { return kind == Kind::fonts || kind == Kind::whole_fonts; }              // d_line_font (and d_font_cost: fonts)
    bool halves() const { return kind == Kind::whole_baseline || kind == Kind::whole_fonts; }    // d_back holds two halves per workgroup
};

// What the last successful run left for the getters and the verify.
struct LastRun {
    bool ok = false;  // a run succeeded since the font was set
    RunMode mode;
    Geometry g{};
    size_t n_pages = 0;
    uint32_t x_start = 0;
    const uint8_t *src = nullptr;  // its pages on the device
};

// One set of glyph tables on the device, all three arrays or none: glyph records and phase offsets font-major (PackedGlyphs), and one bitmap
// table whose dword offsets the records carry (read as uint32_t by the decode kernels, as bytes by the compose kernels).
struct GlyphTables {
    focr::DevArray<DevGlyph> glyphs;
    focr::DevArray<int2> offs;
    focr::DevArray<uint8_t> bitmaps;
    uint32_t n_dw = 0;  // dwords of the bitmap table
    void release() { *this = GlyphTables{}; }
    hipError_t upload(const PackedGlyphs &g, const uint8_t *bytes) {  // g.bytes of them
        hipError_t e = glyphs.upload(g.glyphs.data(), g.glyphs.size());
        if (e == hipSuccess) e = offs.upload(g.offs.data(), g.offs.size());
        if (e == hipSuccess) e = bitmaps.upload(bytes, g.bytes, 4);
        n_dw = (uint32_t)(g.bytes / 4);
        if (e != hipSuccess) release();
        return e;
    }
};

// The verify tables beside a set of glyph tables (the decode font's, the candidates'): boxes and phase rectangles.
struct VerifyTables {
    focr::DevArray<VerifyGlyph> glyphs;
    focr::DevArray<VerifyPhase> phases;
    bool ok = false;    // uploaded for the fonts now beside them
    uint32_t hmax = 0;  // the rows render() gives any line of them at most
    void release() { *this = VerifyTables{}; }
    hipError_t upload(const PackedVerify &v) {
        hipError_t e = glyphs.upload(v.glyphs.data(), v.glyphs.size());
        if (e == hipSuccess) e = phases.upload(v.phases.data(), v.phases.size());
        hmax = (uint32_t)(v.y_hi - v.y_lo);
        if (!(ok = e == hipSuccess)) release();
        return e;
    }
};

// The y-phase fonts v >= 1 of the decode font (focr_decoder_set_baseline_fonts), v-major.
struct BaseFonts {
    GlyphTables tables;
    bool ok = false;          // uploaded for the current decode font, for y_bits `bits`
    uint32_t bits = 0;
    uint64_t term_bound = 0;  // the largest glyph_term_bound among them (box sizes differ between y-phases)
};

// One candidate of a font search as the device reads it (decode_fonts.hip, decode_whole_fonts.hip); [0] is the decode font.
struct FontDesc {
    uint32_t glyph_base;  // its first glyph in the candidates' k-major glyph records (and, times 64, phase offsets)
    uint32_t end_dw;      // the end of its bitmaps in the bitmap table it reads, in dwords (footprint_term_wide's guard)
    float origin_x;
    // the whole-line form only: 64 * origin_x, its batch, its largest inc64 and where its inc64 start in the candidates' table
    int origin_d;
    uint32_t batch, max_inc, inc_base;
};

// The staged reading of a verify_text or score_text call (text_plan.h has its rules): its pages when they come from host memory, its
// records, characters and pens or offsets.  One set serves both entry points: each call ends with a stream wait and keeps nothing
// here between calls, so the arrays are idle when the next call, of either kind, grows and fills them.  They are apart from the
// run's buffers (d_pages, d_chars, ...): a call leaves the last run, its getters and its verify as they were.
struct TextStage {
    focr::DevArray<uint8_t> pages;
    focr::DevArray<TextRec> recs;
    focr::DevArray<uint16_t> chars;
    focr::DevArray<uint32_t> pens;
    focr::DevArray<int8_t> offs;
};

// ... and where one call's kernels read it (stage_text, below): pens and offs are null where the call gave none.
struct StagedText {
    const uint8_t *pages;
    const TextRec *recs;
    const uint16_t *chars;
    const uint32_t *pens;
    const int8_t *offs;
};

struct Stage {  // the kernels of one entry point's last call: device events around them, their time and their number
    hipEvent_t begin = nullptr, end = nullptr;
    float ms = 0.f;
    uint32_t launches = 0;
};

}  // namespace focr_dec

struct focr_decoder {
    int device = 0;
    hipStream_t stream = nullptr;
    focr_dec::Stage run, verify, test, vtext, stext, atext, ltext, rtext;
    std::string err;
    // the fonts (decode_font.h): font k of 0 ..= K is font_at(k).  n_glyphs is the alphabet's size and "a decode font is set": `font` and
    // `tables` are that font's, and a set_font that succeeds replaces all three together
    uint32_t n_glyphs = 0;
    focr_dec::HostFont font;
    std::vector<focr_dec::HostFont> cands;  // the candidates 1 ..= K of the font search (focr_decoder_set_font_candidates)
    const focr_dec::HostFont &font_at(size_t k) const { return k ? cands[k - 1] : font; }
    // every device array: exact growth, no stream wait (each call ends with one, so the buffers are idle when the next call grows them)
    focr_dec::GlyphTables tables, ftables;  // the decode font's, and the candidates' k-major
    focr_dec::VerifyTables vtables, fvtables;  // their verify tables (focr_decoder_set_verify_font, _set_verify_font_candidates)
    focr_dec::BaseFonts yfonts;
    // the settings as the setters wrote them; a run resolves them once (resolve_modes) and reads nothing else of them
    focr_dec::Modes modes;
    // batch buffers (grown on demand)
    focr::DevArray<uint8_t> d_pages, d_strips;
    focr::DevArray<uint32_t> d_flags, d_work, d_nchars, d_count;
    focr::DevArray<uint16_t> d_chars;
    // scores: per step beside d_chars, per work-list line beside d_nchars; grown by a run with scores on
    focr::DevArray<int32_t> d_term, d_runner_term;
    focr::DevArray<uint16_t> d_runner;
    focr::DevArray<uint64_t> d_base;
    // pen search: the chosen offset of every step beside d_chars; grown by a run with a radius
    focr::DevArray<int8_t> d_pen;
    // whole-line decode: inc64 per glyph, the workgroups' backpointer scratch, and the pen of every character beside d_chars
    // and the cost of every work-list line beside d_nchars; grown by a whole-line run
    focr::DevArray<uint32_t> d_inc64, d_pens;
    focr::DevArray<uint16_t> d_back;
    focr::DevArray<int64_t> d_cost;
    // pen slack of a whole-line run: the workgroups' offset scratch beside d_back; the chosen offset of every character goes
    // to d_pen, as a search's does; grown by a run with a slack radius
    focr::DevArray<int8_t> d_woff;
    // margins of a whole-line run: the workgroups' forward keys in d_back's place, and per character beside d_chars the term,
    // the runner and the margin; grown by a run with margins on
    focr::DevArray<uint64_t> d_fwd;
    focr::DevArray<int32_t> d_mterm;
    focr::DevArray<uint16_t> d_mrunner;
    focr::DevArray<int64_t> d_margin;
    // baseline search: per work-list line beside d_nchars the chosen q and its cost; grown by a run with a radius.  The
    // baseline candidates of a whole-line run read the same y-phase tables (yfonts) and write the line's q to d_base_q; their
    // cost is the whole-line run's d_cost
    focr::DevArray<int32_t> d_base_q;
    focr::DevArray<int64_t> d_base_cost;
    // font search: a run's descriptors of the candidates 0 ..= K and, under the whole-line decode, their inc64, and per
    // work-list line beside d_nchars the winner and (pen loop) its cost; grown by a run with the search on
    focr::DevArray<focr_dec::FontDesc> d_fdesc;
    focr::DevArray<uint32_t> d_finc64, d_line_font;
    focr::DevArray<int64_t> d_font_cost;
    // the last run: what it was (for the getters' refusals and the verify) and its results on the host
    focr_dec::LastRun last;
    std::vector<focr_decoded_line_t> lines;
    std::vector<uint16_t> chars;
    std::vector<int8_t> offsets;  // beside chars: all zero after a run without a search
    std::vector<focr_char_score_t> char_scores;  // beside chars (a scores run)
    std::vector<uint64_t> line_base;             // beside lines
    std::vector<uint32_t> pens;   // beside chars: each character's pen in 1/64 px (a whole-line run)
    std::vector<int64_t> line_cost;
    std::vector<focr_char_margin_t> margins;  // beside chars (a margins run)
    std::vector<int8_t> base_q;    // beside lines (a baseline run)
    std::vector<int64_t> base_cost;
    std::vector<uint8_t> line_font;  // beside lines (a font search)
    std::vector<int64_t> font_cost;
    // verify: buffers
    focr::DevArray<focr_dec::VerifyLine> d_vlines;
    focr::DevArray<focr_dec::VerifyRec> d_vrecs;
    focr::DevArray<unsigned long long> d_sums;
    focr::DevArray<uint8_t> d_rgb;
    // test images: buffers of their own, so that a test call leaves the last run and its verify as they were
    focr::DevArray<uint8_t> d_tpages;
    focr::DevArray<uint32_t> d_tbase, d_trect, d_ttext, d_tflags;
    focr::DevArray<focr_dec::VerifyRec> d_trecs;
    focr::DevArray<focr_dec::VerifyLine> d_tline;
    // verify_text (decode_text.hip) and score_text (decode_score.hip): the staged reading both share, and buffers of each one's
    // own beside it (d_sstrips only when a line's strip does not fit in LDS), so that a call leaves the last run and its verify as they were
    focr_dec::TextStage text;
    focr::DevArray<uint8_t> d_xrgb, d_sstrips;
    focr::DevArray<uint32_t> d_xfirst;
    focr::DevArray<focr_dec::VerifyLine> d_xvlines;
    focr::DevArray<focr_dec::VerifyRec> d_xrecs;
    focr::DevArray<unsigned long long> d_xsums;
    focr::DevArray<focr_text_score_t> d_sout;
    focr::DevArray<focr_dec::FontDesc> d_sdesc;
    focr::DevArray<int32_t> d_sterms;
    // align_text (decode_align.hip): the staged reading is the one above; everything else is its own: the plan's records and nominal
    // pens, the backpointers (one byte per character and state), the fitted pens, the terms, the results, the fonts' descriptors and
    // (only when a line's strip and the programme's rows do not fit in LDS together) the strips
    focr::DevArray<focr_dec::AlignRec> d_arecs;
    focr::DevArray<uint32_t> d_anominal, d_apens;
    focr::DevArray<int8_t> d_aback;
    focr::DevArray<int32_t> d_aterms;
    focr::DevArray<focr_text_align_t> d_aout;
    focr::DevArray<focr_dec::FontDesc> d_adesc;
    focr::DevArray<uint8_t> d_astrips;
    // learn_text (decode_learn.hip): the staged reading is the one above; everything else is its own: the learned font's box records,
    // the sums (one uint32 per byte of that font's bitmaps), the counts per (glyph, phase), the `use` mask and the `used` flags, the
    // fonts' descriptors and (only when a line's strip does not fit in LDS) the strips
    focr::DevArray<focr_dec::LearnGlyph> d_lboxes;
    focr::DevArray<uint32_t> d_lsums, d_lcounts;
    focr::DevArray<uint8_t> d_luse, d_lused, d_lstrips;
    focr::DevArray<focr_dec::FontDesc> d_ldesc;
    // refine_text (decode_refine.hip): the staged reading is the one above; everything else is its own: the fonts' extents, the
    // characters and pens as the sweeps leave them, the results, the fonts' descriptors and (only when a line's strip and a step's
    // window do not fit in LDS together) the strips
    focr::DevArray<focr_dec::RefineFont> d_rfonts;
    focr::DevArray<uint16_t> d_rchars;
    focr::DevArray<uint32_t> d_rpens;
    focr::DevArray<focr_text_refine_t> d_rout;
    focr::DevArray<focr_dec::FontDesc> d_rdesc;
    focr::DevArray<uint8_t> d_rstrips;
};

namespace focr_dec {

inline thread_local std::string g_dec_err;

// The second launch of a verify after a baseline run (decode_baseline.hip), on the decoder's stream; the caller checks hipGetLastError.
void verify_compose_moved_launch(focr_decoder *dec, const TileGrid &tg, size_t n_pages, uint8_t *d_rgb);
// ... and after a baseline run on the fractional line grid (decode_line_frac.hip).
void verify_compose_frac_launch(focr_decoder *dec, const TileGrid &tg, size_t n_pages, uint8_t *d_rgb);

inline int dfail(focr_decoder *dec, const std::string &msg) {
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

// A caller's n elements where the kernels read them: a device pointer (or none) is used as it is; host memory is copied
// into `a` on the decoder's stream.
template <typename T>
int stage_in(focr_decoder *dec, focr::DevArray<T> &a, const void *src, int on_device, size_t n, const T **d) {
    *d = (const T *)src;
    if (on_device || !src) return 0;
    DEC_GROW(a, std::max<size_t>(n, 1));
    DEC_CHECK(hipMemcpyAsync(a, src, n * sizeof(T), hipMemcpyHostToDevice, dec->stream));
    *d = a;
    return 0;
}

// Where the kernels write n elements for the caller: its device buffer (or none), or `a` for fetch_out to copy to its
// host memory on the decoder's stream once the kernels are queued.
template <typename T>
int stage_out(focr_decoder *dec, focr::DevArray<T> &a, void *dst, int on_device, size_t n, T **d) {
    *d = (T *)dst;
    if (on_device || !dst) return 0;
    DEC_GROW(a, std::max<size_t>(n, 1));
    *d = a;
    return 0;
}

template <typename T>
int fetch_out(focr_decoder *dec, void *dst, int on_device, const T *d, size_t n) {
    if (dst && !on_device) DEC_CHECK(hipMemcpyAsync(dst, d, n * sizeof(T), hipMemcpyDeviceToHost, dec->stream));
    return 0;
}

// A call's reading where its kernels read it: n_px page bytes through stage_in, the plan's records and the caller's characters,
// pens and offsets into dec->text, the copies queued on the decoder's stream.  What the call did not give is null in *out, whatever
// an earlier call left in the arrays.
inline int stage_text(focr_decoder *dec, const TextInput &in, const std::vector<TextRec> &recs, const uint8_t *pages, int pages_on_device, size_t n_px,
                      StagedText *out) {
    TextStage &t = dec->text;
    *out = StagedText{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (stage_in(dec, t.pages, pages, pages_on_device, n_px, &out->pages)) return 1;
    const size_t n_chars = std::max<size_t>(in.n_chars, 1);
    DEC_GROW(t.recs, std::max<size_t>(recs.size(), 1));
    DEC_GROW(t.chars, n_chars);
    if (in.pens) DEC_GROW(t.pens, n_chars);
    if (in.offsets) DEC_GROW(t.offs, n_chars);
    if (!recs.empty()) DEC_CHECK(hipMemcpyAsync(t.recs, recs.data(), recs.size() * sizeof(TextRec), hipMemcpyHostToDevice, dec->stream));
    if (in.n_chars) DEC_CHECK(hipMemcpyAsync(t.chars, in.chars, in.n_chars * sizeof(uint16_t), hipMemcpyHostToDevice, dec->stream));
    if (in.pens && in.n_chars) DEC_CHECK(hipMemcpyAsync(t.pens, in.pens, in.n_chars * sizeof(uint32_t), hipMemcpyHostToDevice, dec->stream));
    if (in.offsets && in.n_chars) DEC_CHECK(hipMemcpyAsync(t.offs, in.offsets, in.n_chars, hipMemcpyHostToDevice, dec->stream));
    out->recs = t.recs;
    out->chars = t.chars;
    if (in.pens) out->pens = t.pens;
    if (in.offsets) out->offs = t.offs;
    return 0;
}

// The geometry of a batch for the entry point `who`, or its refusal: the page-size limit; the line slots as the
// reference's loop visits them, with image::crop_imm's clamping of every crop (line_advance 0 with a non-empty first
// crop never ends there), or on the fractional grid fr of a run; the limit on the slots of one batch.  stride and cap are
// the line decoder's to fill.
inline int batch_geometry(focr_decoder *dec, const char *who, size_t n_pages, size_t page_w, size_t page_h, uint32_t x_start, uint32_t y_start,
                          uint32_t width, uint32_t line_height, uint32_t line_advance, Geometry *out, const LineFrac &fr = LineFrac{0, 0}) {
    const std::string pre = std::string(who) + ": ";
    if (page_w > 0xffffu * 16 || page_h > 0xffffu * 16) return dfail(dec, pre + "page too large");
    Geometry g{};
    g.page_w = (uint32_t)page_w;
    g.page_h = (uint32_t)page_h;
    g.x = std::min<uint32_t>(x_start, g.page_w);  // image::crop_imm's clamping
    g.w = std::min<uint32_t>(width, g.page_w - g.x);
    g.y_start = y_start;
    g.line_height = line_height;
    g.line_advance = line_advance;
    if (line_height == 0 || y_start >= g.page_h) g.n_slots = 0;  // the first crop is empty: the loop ends at once
    else if (line_advance == 0) return dfail(dec, pre + "line_advance 0 (the reference never ends)");
    else g.n_slots = (uint32_t)((64ull * g.page_h - fr.top(g) + fr.step(g) - 1) / fr.step(g));  // the slots with Y_i >> 6 < page_h; whole pixels off the grid
    const uint64_t total = (uint64_t)n_pages * g.n_slots;
    if (total > (1u << 30)) return dfail(dec, pre + "too many lines in one batch");
    g.total = (uint32_t)total;
    *out = g;
    return 0;
}

}  // namespace focr_dec
