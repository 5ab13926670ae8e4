// decode_refine.hip — focr_decoder_refine_text (include/focr_decode.h): a reading the caller supplies, repaired against the composed
// line error.  Where focr_decoder_score_text sums one footprint term per character, this draws the line's characters together
// (v = the max of their ink) and lets one character at a time take the glyph and the pen that lower the composed cost
// C = sum of v * (v - 2 r) the most: a chain of n * sweeps dependent steps per line.
//
// refine_text_kernel, one workgroup of four waves per listed line:
//   - the line's crop is staged as score_text_kernel stages it (decode_score.h), in LDS behind the step's window, or by
//     refine_strip_kernel in global memory when the two do not fit LDS_STRIP_MAX together;
//   - the characters and pens the sweeps work on are the call's outputs in global memory, copied from the input first: one thread
//     writes a step's result, and the workgroup reads it behind a barrier;
//   - a window is whole dwords of the strip's own row layout (refine_plan.h), so a tile dword meets the strip and the window at one
//     byte shift.  It is gathered by owners: a thread keeps the dwords t, t + 256, ... and takes, character by character, the max of
//     the tile bytes that fall on them: no atomics and no barrier inside, the same bytes in any order;
//   - the composed cost (cost_in before the sweeps, cost after them) is a walk of such windows over the crop's columns, every
//     character gathered, each owner summing v * (v - 2 r) over its own dwords;
//   - step g: (1) the window is the columns and rows any candidate of the step can touch; the others that can reach it are found
//     from the input pens, which do not decrease and from which no pen has moved more than sweeps * radius: a scan outwards from g
//     that ends at the first character too far away; (2) behind a barrier the candidates (a, j) are flattened over the 256 lanes,
//     consecutive lanes taking consecutive glyphs at one pen, and each lane sums its candidates' D over the box with the wide tile
//     reads of footprint_term_wide (decode_pen.h); (3) the lowest (D, rank, a) is one 64-bit key: per lane, per wave, then the four
//     waves in LDS; thread 0 writes the result; three barriers a step.
// Fonts, staging and refusals are score_text's (decode_score.h, text_plan.h, stage_text); the plan is refine_plan.h's.
#include "decode_score.h"

namespace focr_dec {

static_assert(REFINE_STRIP_PAD == PAD && REFINE_LDS_MAX == LDS_STRIP_MAX, "refine_plan.h restates decode_line.h's");

// in front of the window, in 8-byte words: the waves' keys, the incumbent's D, the waves' partial sums
constexpr uint32_t REFINE_RED_KEYS = 0, REFINE_RED_INC = SCORE_WAVES, REFINE_RED_SUMS = SCORE_WAVES + 1;
constexpr uint32_t REFINE_RED_BYTES = (2 * SCORE_WAVES + 2) * 8;

struct RefineWin {  // the strip dwords q0 .. q0 + dw - 1 of the crop rows y0 .. y0 + rows - 1
    int q0, dw, y0, rows;
    __device__ __forceinline__ bool empty() const { return dw <= 0 || rows <= 0; }
};

struct RefineLine {  // the line as the steps see it: its crop's size, its font with the extent, its characters and pens now
    int w, h;
    ScoreFont f;
    RefineFont e;
    const uint16_t *cs;
    const uint32_t *ps;
    uint32_t n;
};

// 1. (only when the strip does not fit in LDS beside the window) every listed line's strip into global memory, one workgroup per line
__global__ __launch_bounds__(SCORE_THREADS) void refine_strip_kernel(const uint8_t *__restrict__ pages, Geometry g, const TextRec *__restrict__ in,
                                                                     uint8_t *__restrict__ strips) {
    const TextRec l = in[blockIdx.x];
    uint32_t h;
    const uint8_t *src = score_crop(pages, g, l, &h);
    (void)score_stage((uint32_t *)(strips + (size_t)blockIdx.x * g.stride * g.line_height), src, g.page_w, g.w, h, g.stride / 4);
}

__device__ __forceinline__ uint32_t max_bytes(uint32_t a, uint32_t b) {
    uint32_t v = 0;
    for (int i = 0; i < 32; i += 8) v |= std::max((a >> i) & 255u, (b >> i) & 255u) << i;
    return v;
}

// The workgroup's sum of every thread's v (mod 2^64), in every thread; ends with a barrier, so `red` is free again.
__device__ __forceinline__ uint64_t block_sum(uint64_t *red, uint64_t v, uint32_t lane, uint32_t wave) {
    v = wave_sum(v);
    if (lane == 0) red[REFINE_RED_SUMS + wave] = v;
    __syncthreads();
    uint64_t s = 0;
    for (uint32_t u = 0; u < SCORE_WAVES; u++) s += red[REFINE_RED_SUMS + u];
    __syncthreads();
    return s;
}

// The window's dwords this thread owns take the max of the characters lo .. hi - 1 but `skip` as they stand: clipped to the crop on
// all four sides, so the bytes of a window dword left of column 0 or right of column w - 1 stay 0.
__device__ __forceinline__ void refine_gather(uint32_t *win, const RefineWin &W, const RefineLine &L, uint32_t lo, uint32_t hi, uint32_t skip) {
    const uint32_t n_dw = (uint32_t)(W.dw * W.rows);
    for (uint32_t i = threadIdx.x; i < n_dw; i += SCORE_THREADS) win[i] = 0;
    const int cx0 = 4 * W.q0 - (int)PAD, cx1 = cx0 + 4 * W.dw;  // the columns its dwords hold
    for (uint32_t k = lo; k < hi; k++) {                         // uniform
        if (k == skip) continue;
        const uint32_t c = L.cs[k];
        const int delta = L.f.origin_d + (int)L.ps[k];
        const uint32_t phase = (uint32_t)delta & 63u;
        const DevGlyph gl = L.f.glyphs[c];
        const int2 o = L.f.offs[c * 64 + phase];
        const int x0 = (delta >> 6) + o.x, y0 = o.y, bw = 4 * (int)gl.ndw;
        const int xa = std::max(std::max(x0, 0), cx0), xb = std::min(std::min(x0 + bw, L.w), cx1);
        const int ya = std::max(std::max(y0, 0), W.y0), yb = std::min(std::min(y0 + (int)gl.box_h, L.h), W.y0 + W.rows);
        if (xa >= xb || ya >= yb) continue;
        const uint8_t *tile = (const uint8_t *)(L.f.bitmaps + gl.off_dw + phase * gl.ndw * gl.box_h);
        for (uint32_t i = threadIdx.x; i < n_dw; i += SCORE_THREADS) {
            const int row = W.y0 + (int)(i / (uint32_t)W.dw), col = cx0 + 4 * (int)(i % (uint32_t)W.dw);
            if (row < ya || row >= yb || col + 4 <= xa || col >= xb) continue;
            const uint8_t *trow = tile + (size_t)(row - y0) * bw;
            uint32_t t = 0;
            for (int b = 0; b < 4; b++)
                if (col + b >= xa && col + b < xb) t |= (uint32_t)trow[col + b - x0] << (8 * b);  // inside the phase's tile
            win[i] = max_bytes(win[i], t);
        }
    }
}

// The composed cost of the line as it stands: windows of win_dw dwords walk the strip's row, each owner sums its own dwords.
__device__ __forceinline__ int64_t refine_compose(uint32_t *win, uint64_t *red, const uint32_t *strip, uint32_t sdw, uint32_t win_dw, const RefineLine &L,
                                                  uint32_t lane, uint32_t wave) {
    int64_t acc = 0;
    const int y0 = std::max(0, L.e.y_lo), rows = std::min(L.h, L.e.y_hi) - y0;
    if (rows > 0 && L.n && win_dw)
        for (uint32_t q = 0; q < sdw; q += win_dw) {
            const RefineWin W{(int)q, (int)std::min(win_dw, sdw - q), y0, rows};
            refine_gather(win, W, L, 0, L.n, ~0u);
            for (uint32_t i = threadIdx.x; i < (uint32_t)(W.dw * W.rows); i += SCORE_THREADS) {  // this thread's own, as it gathered them
                const uint32_t v = win[i], r = strip[(size_t)(y0 + i / (uint32_t)W.dw) * sdw + q + i % (uint32_t)W.dw];
                acc += (int64_t)__builtin_amdgcn_udot4(v, v, 0u, false) - 2 * (int64_t)__builtin_amdgcn_udot4(v, r, 0u, false);
            }
        }
    return (int64_t)block_sum(red, (uint64_t)acc, lane, wave);
}

// One dword c of a tile row at canvas column `base` against the strip row srow and the window row wrow (whose dword 0 is the strip's
// q0): what f(max(c, o)) - f(o) sums to over its four pixels, in the four dot products it is made of.
__device__ __forceinline__ void refine_dword(uint32_t c, const uint32_t *srow, const uint32_t *wrow, int q0, int base, int w, uint32_t &mm, uint32_t &oo,
                                             uint32_t &mr, uint32_t &orr) {
    if (base <= -4 || base >= w) return;
    if (base < 0 || base + 4 > w) c &= edge_mask(base, w);
    if (!c) return;  // m == o: nothing
    const uint32_t a = (uint32_t)(base + (int)PAD);
    const int k = (int)(a >> 2);
    const uint32_t rv = __builtin_amdgcn_alignbyte(srow[k + 1], srow[k], a & 3);
    const uint32_t ov = __builtin_amdgcn_alignbyte(wrow[k + 1 - q0], wrow[k - q0], a & 3);
    const uint32_t m = max_bytes(c, ov);
    mm = __builtin_amdgcn_udot4(m, m, mm, false);
    oo = __builtin_amdgcn_udot4(ov, ov, oo, false);
    mr = __builtin_amdgcn_udot4(m, rv, mr, false);
    orr = __builtin_amdgcn_udot4(ov, rv, orr, false);
}

// D of one candidate: a phase tile at (x0, y0) over the window, the tile's rows read as footprint_term_wide reads them.  Every sum
// is below area * 255^2 < 2^30 (the font upload's box limit), and D fits an int32.
__device__ __forceinline__ int refine_term(const uint32_t *strip, uint32_t sdw, int w, int h, const uint32_t *win, const RefineWin &W,
                                           const uint32_t *__restrict__ tile, const uint32_t *__restrict__ table_end, uint32_t ndw, uint32_t box_h, int x0, int y0) {
    const int r_lo = std::max(0, -y0), r_hi = std::min((int)box_h, h - y0);
    uint32_t mm = 0, oo = 0, mr = 0, orr = 0;
    for (int r = r_lo; r < r_hi; r++) {
        const uint32_t *srow = strip + (size_t)(y0 + r) * sdw;
        const uint32_t *wrow = win + (size_t)(y0 + r - W.y0) * W.dw;
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
            refine_dword(c0, srow, wrow, W.q0, base, w, mm, oo, mr, orr);
            if (q + 1 < ndw) refine_dword(c1, srow, wrow, W.q0, base + 4, w, mm, oo, mr, orr);
            if (q + 2 < ndw) refine_dword(c2, srow, wrow, W.q0, base + 8, w, mm, oo, mr, orr);
            if (q + 3 < ndw) refine_dword(c3, srow, wrow, W.q0, base + 12, w, mm, oo, mr, orr);
        }
    }
    return (int)(((int64_t)mm - (int64_t)oo) - 2 * ((int64_t)mr - (int64_t)orr));
}

// 2. the lines' repairs, one workgroup per listed line
template <bool LDS>
__global__ __launch_bounds__(SCORE_THREADS) void refine_text_kernel(const uint8_t *__restrict__ pages, Geometry g, const TextRec *__restrict__ in,
                                                                    const uint16_t *__restrict__ chars, const uint32_t *__restrict__ pens, ScoreFonts fonts,
                                                                    const RefineFont *__restrict__ extents, uint32_t radius, uint32_t sweeps, uint32_t glyphs,
                                                                    uint32_t win_dw, uint32_t win_rows, const uint8_t *__restrict__ strips, uint16_t *chars_out,
                                                                    uint32_t *pens_out, focr_text_refine_t *__restrict__ out) {
    extern __shared__ __align__(8) uint32_t lds_refine[];  // the waves' keys and partial sums, the window, then (LDS) the strip
    uint64_t *red = (uint64_t *)lds_refine;
    uint32_t *win = lds_refine + REFINE_RED_BYTES / 4;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const TextRec l = in[blockIdx.x];
    const uint32_t sdw = g.stride / 4;
    uint32_t h;
    const uint8_t *src = score_crop(pages, g, l, &h);
    const uint32_t *strip;
    uint64_t acc = 0;
    if (LDS) {
        uint32_t *lds_strip = win + (size_t)win_dw * win_rows;
        acc = score_stage(lds_strip, src, g.page_w, g.w, h, sdw);
        strip = lds_strip;
    } else {  // refine_strip_kernel's: the rows below h hold nothing of this line, and a row's pad bytes are zero
        strip = (const uint32_t *)(strips + (size_t)blockIdx.x * g.stride * g.line_height);
        for (uint32_t i = tid; i < sdw * h; i += SCORE_THREADS) acc += __builtin_amdgcn_udot4(strip[i], strip[i], 0u, false);
    }
    const uint16_t *cs_in = chars + l.first;
    const uint32_t *ps_in = pens + l.first;
    uint16_t *cs = chars_out + l.out;
    uint32_t *ps = pens_out + l.out;
    for (uint32_t i = tid; i < l.n; i += SCORE_THREADS) cs[i] = cs_in[i], ps[i] = ps_in[i];
    const uint64_t base = block_sum(red, acc, lane, wave);  // its barriers: the strip is staged, the line is copied
    int d;
    const RefineLine L{(int)g.w, (int)h, score_font(fonts, l, &d), extents[l.font], cs, ps, l.n};  // d == 0: there is no line_q
    const int64_t cost_in = refine_compose(win, red, strip, sdw, win_dw, L, lane, wave);
    const int N = (int)radius, slack = (int)(radius * sweeps), od = L.f.origin_d;
    const uint32_t A = glyphs ? fonts.n_glyphs : 1, n_cand = A * (2 * radius + 1);
    const int wy0 = std::max(0, L.e.y_lo), wrows = std::min(L.h, L.e.y_hi) - wy0;
    uint32_t run = 0;
    bool moved = false;
    for (uint32_t sweep = 0; sweep < sweeps && wrows > 0 && L.w > 0; sweep++) {  // uniform throughout
        bool any = false;
        for (uint32_t gi = 0; gi < l.n; gi++) {
            const int s = (int)ps[gi];
            const uint32_t ag = cs[gi];
            // the columns any candidate can touch, on the crop
            const int wx0 = std::max(0, ((od + s - N) >> 6) + L.e.x_lo), wx1 = std::min(L.w, ((od + s + N) >> 6) + L.e.x_hi);
            if (wx0 >= wx1 || wrows <= 0) continue;  // every candidate lies off the crop: every D is 0, the character stays
            uint32_t q0;
            const uint32_t dw = refine_row_dwords((uint32_t)wx0, (uint32_t)wx1, &q0);
            const RefineWin W{(int)q0, (int)dw, wy0, wrows};
            const int cx0 = 4 * W.q0 - (int)PAD, cx1 = cx0 + 4 * W.dw;
            uint32_t lo = gi, hi = gi + 1;  // the others that can reach the window's columns, from the sorted input pens
            while (lo > 0 && ((od + (int)ps_in[lo - 1] + slack) >> 6) + L.e.x_hi > cx0) lo--;
            while (hi < l.n && ((od + (int)ps_in[hi] - slack) >> 6) + L.e.x_lo < cx1) hi++;
            refine_gather(win, W, L, lo, hi, gi);
            __syncthreads();  // the window is whole
            uint64_t best = ~0ull;
            for (uint32_t idx = tid; idx < n_cand; idx += SCORE_THREADS) {
                const uint32_t rank = idx / A, a = glyphs ? idx % A : ag;
                const int pen = s + rank_offset(rank);
                if (pen < 0 || pen >= (int)REFINE_PEN_END) continue;
                const int delta = od + pen;
                const uint32_t phase = (uint32_t)delta & 63u;
                const DevGlyph gl = L.f.glyphs[a];
                const int2 o = L.f.offs[a * 64 + phase];
                const uint32_t *tile = L.f.bitmaps + gl.off_dw + phase * gl.ndw * gl.box_h;
                const int D = refine_term(strip, sdw, L.w, L.h, win, W, tile, L.f.end, gl.ndw, gl.box_h, (delta >> 6) + o.x, o.y);
                best = std::min(best, ((uint64_t)((uint32_t)D ^ 0x80000000u) << 32) | (rank << 16) | a);  // (D, rank, a), lowest first
                if (rank == 0 && a == ag) red[REFINE_RED_INC] = (uint64_t)(int64_t)D;                      // the incumbent: one thread's
            }
            for (int m = 32; m >= 1; m >>= 1) best = std::min(best, shfl_xor_u64(best, m));
            if (lane == 0) red[REFINE_RED_KEYS + wave] = best;
            __syncthreads();
            for (uint32_t u = 0; u < SCORE_WAVES; u++) best = std::min(best, red[REFINE_RED_KEYS + u]);
            const int D = (int)((uint32_t)(best >> 32) ^ 0x80000000u), D_inc = (int)(int64_t)red[REFINE_RED_INC];
            if (D < D_inc) {  // strictly: among equal D the incumbent stays
                any = true;
                if (tid == 0) cs[gi] = (uint16_t)(best & 0xffffu), ps[gi] = (uint32_t)(s + rank_offset((uint32_t)(best >> 16) & 0xffffu));
            }
            __syncthreads();  // the step's result is written (the workgroup's own global stores are visible behind its barrier); red and the window are free
        }
        run++;
        moved = moved || any;
        if (!any) break;
    }
    if (sweeps && !run) run = 1;  // no candidate of the line reaches the crop's rows or columns: its first sweep changed nothing
    const int64_t cost = moved ? refine_compose(win, red, strip, sdw, win_dw, L, lane, wave) : cost_in;
    uint64_t changed = 0;
    for (uint32_t i = tid; i < l.n; i += SCORE_THREADS) changed += cs[i] != cs_in[i] || ps[i] != ps_in[i];
    changed = block_sum(red, changed, lane, wave);
    if (tid == 0) out[blockIdx.x] = focr_text_refine_t{base, cost_in, cost, run, (uint32_t)changed};
}

}  // namespace focr_dec

using namespace focr_dec;

extern "C" int focr_decoder_refine_text(focr_decoder_t *dec, const uint8_t *pages, int pages_on_device, size_t n_pages, size_t page_w, size_t page_h,
                                        uint32_t x_start, uint32_t width, uint32_t line_height, const focr_text_line_t *lines, size_t n_lines,
                                        const uint16_t *chars, const uint32_t *pens, size_t n_chars, uint32_t radius, uint32_t sweeps, int glyphs,
                                        uint16_t *chars_out, uint32_t *pens_out, focr_text_refine_t *out) {
    const std::string who = "focr_decoder_refine_text: ";
    if (!dec) return dfail(nullptr, who + "null decoder");
    dec->rtext.ms = 0.f;
    dec->rtext.launches = 0;
    const TextInput in{lines, n_lines, chars, pens, nullptr, n_chars, n_pages};
    std::string no = text_guards(in, pages, !pens ? "pens" : n_lines && !out ? "out" : n_lines && !chars_out ? "chars_out" : n_lines && !pens_out ? "pens_out" : nullptr);
    if (!no.empty()) return dfail(dec, who + no);
    if (!dec->n_glyphs) return dfail(dec, who + "no decode font (focr_decoder_set_font)");
    if (width == 0) return dfail(dec, who + "width 0");
    if (line_height == 0) return dfail(dec, who + "line_height 0");
    if (!(no = plan_refine_radii(radius, sweeps)).empty()) return dfail(dec, who + no);
    Geometry g{};
    if (batch_geometry(dec, "focr_decoder_refine_text", n_pages, page_w, page_h, x_start, 0, width, 0, 1, &g)) return 1;
    if (n_lines > 0x7fffffffu || n_pages > 0x7fffffffu) return dfail(dec, who + "too many lines or pages in one call");
    TextAsk ask;
    ask.pen_origin = true;
    TextPlan text;
    RefinePlan plan;
    if (!(no = plan_text_lines(in, dec->font, dec->cands, ask, &text)).empty() || !(no = plan_text_chars(in, dec->n_glyphs)).empty() ||
        !(no = plan_refine(in, text.recs, dec->font, dec->cands, radius, line_height, REFINE_RED_BYTES, &plan)).empty())
        return dfail(dec, who + no);
    if (n_lines == 0) return 0;
    const uint64_t n_out = text.n_out;
    g.line_height = line_height;
    g.stride = ((g.w + PAD + 3) / 4 + 2) * 4;  // line_cap's
    const size_t strip_bytes = (size_t)g.stride * line_height, fixed = REFINE_RED_BYTES + plan.win_bytes();
    const bool lds = strip_bytes + fixed <= LDS_STRIP_MAX;  // the strip shares LDS with the waves' words and the window
    DEC_CHECK(hipSetDevice(dec->device));
    WholePlan fplan;
    ScoreFonts f;
    if (score_fonts(dec, &fplan, dec->d_rdesc, 0, &f)) return 1;
    StagedText st;
    if (stage_text(dec, in, text.recs, pages, pages_on_device, n_pages * page_w * page_h, &st)) return 1;
    DEC_GROW(dec->d_rfonts, plan.fonts.size());
    DEC_GROW(dec->d_rchars, std::max<size_t>(n_out, 1));
    DEC_GROW(dec->d_rpens, std::max<size_t>(n_out, 1));
    DEC_GROW(dec->d_rout, n_lines);
    if (!lds) DEC_GROW(dec->d_rstrips, strip_bytes * n_lines);
    DEC_CHECK(hipMemcpyAsync(dec->d_rfonts, plan.fonts.data(), plan.fonts.size() * sizeof(RefineFont), hipMemcpyHostToDevice, dec->stream));
    DEC_CHECK(hipEventRecord(dec->rtext.begin, dec->stream));
    if (lds) {
        refine_text_kernel<true><<<(uint32_t)n_lines, SCORE_THREADS, fixed + strip_bytes, dec->stream>>>(
            st.pages, g, st.recs, st.chars, st.pens, f, dec->d_rfonts, radius, sweeps, glyphs != 0, plan.win_dw, plan.win_rows, nullptr, dec->d_rchars,
            dec->d_rpens, dec->d_rout);
    } else {
        refine_strip_kernel<<<(uint32_t)n_lines, SCORE_THREADS, 0, dec->stream>>>(st.pages, g, st.recs, dec->d_rstrips);
        DEC_CHECK(hipGetLastError());
        refine_text_kernel<false><<<(uint32_t)n_lines, SCORE_THREADS, fixed, dec->stream>>>(
            st.pages, g, st.recs, st.chars, st.pens, f, dec->d_rfonts, radius, sweeps, glyphs != 0, plan.win_dw, plan.win_rows, dec->d_rstrips, dec->d_rchars,
            dec->d_rpens, dec->d_rout);
    }
    DEC_CHECK(hipGetLastError());
    DEC_CHECK(hipEventRecord(dec->rtext.end, dec->stream));
    DEC_CHECK(hipMemcpyAsync(out, dec->d_rout, n_lines * sizeof(focr_text_refine_t), hipMemcpyDeviceToHost, dec->stream));
    if (n_out) DEC_CHECK(hipMemcpyAsync(chars_out, dec->d_rchars, n_out * sizeof(uint16_t), hipMemcpyDeviceToHost, dec->stream));
    if (n_out) DEC_CHECK(hipMemcpyAsync(pens_out, dec->d_rpens, n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, dec->stream));
    DEC_CHECK(hipStreamSynchronize(dec->stream));
    DEC_CHECK(hipEventElapsedTime(&dec->rtext.ms, dec->rtext.begin, dec->rtext.end));
    dec->rtext.launches = lds ? 1 : 2;
    return 0;
}

extern "C" float focr_decoder_last_refine_text_ms(const focr_decoder_t *dec) { return dec ? dec->rtext.ms : 0.f; }
extern "C" uint32_t focr_decoder_last_refine_text_launches(const focr_decoder_t *dec) { return dec ? dec->rtext.launches : 0; }
