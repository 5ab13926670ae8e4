// decode_pen.h — the plain pen loop as a device function, for the kernels that run it once per candidate and keep the
// cheapest line (decode_baseline.hip: one candidate per vertical offset; decode_fonts.hip: one per font): the footprint
// term with wide tile reads, and the loop by one wave.  Device helpers only (no relocatable device code: they are inlined
// into each kernel).  line_decode_kernel keeps its own loop (decode.hip): its instruction stream is what the plain
// decoder's benchmark pins.
#pragma once

#include "decode_line.h"

namespace focr_dec {

// One dword c of a tile row at canvas column `base` against the strip row srow: footprint_term's inner step.
__device__ __forceinline__ void term_dword(uint32_t c, const uint32_t *srow, int base, int w, uint32_t &cc, uint32_t &cr) {
    if (base <= -4 || base >= w) return;
    if (base < 0 || base + 4 > w) c &= edge_mask(base, w);
    const uint32_t a = (uint32_t)(base + (int)PAD);
    const uint32_t rv = __builtin_amdgcn_alignbyte(srow[(a >> 2) + 1], srow[a >> 2], a & 3);
    cr = __builtin_amdgcn_udot4(c, rv, cr, false);
    cc = __builtin_amdgcn_udot4(c, c, cc, false);
}

// footprint_term (decode_line.h) with a tile row read four dwords at a time: the lanes of a wave read different glyphs, so
// every load of theirs touches up to 64 cache lines, and the loads, not the arithmetic, are what a candidate costs.  A
// read past a short row's end stays inside the table (the dwords of the next row; they are not used), and the table's last
// rows, where it would not, are read dword by dword.  The sums are integer sums: the same term in any order.
__device__ __forceinline__ int footprint_term_wide(const uint32_t *strip, uint32_t sdw, int w, uint32_t h, const uint32_t *__restrict__ tile,
                                                   const uint32_t *__restrict__ table_end, uint32_t ndw, uint32_t box_h, int x0, int y0) {
    const int r_lo = std::max(0, -y0), r_hi = std::min((int)box_h, (int)h - y0);
    uint32_t cc = 0, cr = 0;
    for (int r = r_lo; r < r_hi; r++) {
        const uint32_t *srow = strip + (size_t)(y0 + r) * sdw;
        const uint32_t *trow = tile + (size_t)r * ndw;
        for (uint32_t q = 0; q < ndw; q += 4) {
            uint32_t c0, c1 = 0, c2 = 0, c3 = 0;
            if (trow + q + 4 <= table_end) {
                uint4 t;
                __builtin_memcpy(&t, trow + q, sizeof t);  // dword-aligned
                c0 = t.x, c1 = t.y, c2 = t.z, c3 = t.w;
            } else {
                c0 = trow[q];
                if (q + 1 < ndw) c1 = trow[q + 1];
                if (q + 2 < ndw) c2 = trow[q + 2];
                if (q + 3 < ndw) c3 = trow[q + 3];
            }
            const int base = x0 + 4 * (int)q;
            term_dword(c0, srow, base, w, cc, cr);
            if (q + 1 < ndw) term_dword(c1, srow, base + 4, w, cc, cr);
            if (q + 2 < ndw) term_dword(c2, srow, base + 8, w, cc, cr);
            if (q + 3 < ndw) term_dword(c3, srow, base + 12, w, cc, cr);
        }
    }
    return (int)cc - 2 * (int)cr;
}

// The plain pen loop (line_decode_kernel) by one wave, with every box moved down by d rows: the line's summed footprint
// terms, and with WRITE its characters to out and their number to *n_out (lane 0).  n_dw: the dwords of the bitmap table
// up to the end of this font's bitmaps (footprint_term_wide's guard).  Uniform across the wave.
template <bool WRITE>
__device__ __forceinline__ int64_t pen_loop(const uint32_t *strip, uint32_t sdw, int w, uint32_t h, uint32_t cap, const DevGlyph *__restrict__ glyphs,
                                            const int2 *__restrict__ offs, const uint32_t *__restrict__ bitmaps, uint32_t n_dw, uint32_t n_glyphs,
                                            float origin_x, int d, uint32_t lane, uint16_t *__restrict__ out, uint32_t *__restrict__ n_out) {
    const float fw = (float)w;
    float pos = 0.f;
    uint32_t n = 0;
    int64_t cost = 0;
    while (pos < fw && n < cap) {
        const int dx = (int)((origin_x + pos) * 64.0f);  // FreeType's delta: trunc(t * 64)
        const int phase = dx & 63, shift = dx >> 6;
        uint64_t best = ~0ull;
        for (uint32_t gi = lane; gi < n_glyphs; gi += 64) {
            const DevGlyph gl = glyphs[gi];
            const int2 o = offs[gi * 64 + phase];
            const uint32_t *tile = bitmaps + gl.off_dw + (uint32_t)phase * gl.ndw * gl.box_h;
            const int score = footprint_term_wide(strip, sdw, w, h, tile, bitmaps + n_dw, gl.ndw, gl.box_h, shift + o.x, o.y + d);
            best = std::min(best, ((uint64_t)((uint32_t)score ^ 0x80000000u) << 32) | gi);  // (score, index), lowest first
        }
        for (int m = 32; m >= 1; m >>= 1) best = std::min(best, shfl_xor_u64(best, m));
        const uint32_t gbest = (uint32_t)best;
        cost += (int)((uint32_t)(best >> 32) ^ 0x80000000u);
        if (WRITE && lane == 0) out[n] = (uint16_t)gbest;
        n++;
        pos = __fadd_rn(pos, glyphs[gbest].inc);
    }
    if (WRITE && lane == 0) *n_out = n;
    return cost;
}

}  // namespace focr_dec
