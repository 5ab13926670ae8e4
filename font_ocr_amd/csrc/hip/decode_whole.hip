// decode_whole.hip — the whole-line decode of the `focr` line decoder (focr_decoder_set_whole_line; an extension, see
// include/focr_decode.h): the third launch of a whole-line run, in line_decode_kernel's place (decode.hip).  line_whole_kernel
// is a dynamic programme over pens in 1/64 px that minimises the sum of the footprint terms along the line;
// line_whole_margins_kernel adds a backward sweep for every character's term, runner-up and margin; line_whole_slack_kernel
// runs the programme over pen offsets as well.  Three kernels and not one with switches: a run without margins or slack
// launches the kernel it always did, and the names stay comparable across commits (tools/isa_hash.py).  They are built from
// the phases and the LDS layout of decode_whole.h, which decode_whole_baseline.hip's kernel shares.  whole_plan,
// whole_reserve and whole_launch are the host's side (decode_line.h).
#include <cmath>

#include "decode_whole.h"

namespace focr_dec {

// ---- the kernels ---------------------------------------------------------------------------------------------------

// 3w. the dynamic programme over pens in 1/64 px, one workgroup per work-list line at a time (k = blockIdx.x, then
// += gridDim.x).  A batch is B <= min inc64 consecutive states; every reachable one leaves its glyph in the workgroup's
// scratch of backpointers and starts edges at the cost its ring slot holds.
template <bool LDS>
__global__ __launch_bounds__(WHOLE_THREADS) void line_whole_kernel(const uint8_t *__restrict__ strips, Geometry g, const uint32_t *__restrict__ work,
                                                                   const uint32_t *__restrict__ count, const DevGlyph *__restrict__ glyphs,
                                                                   const int2 *__restrict__ offs, const uint32_t *__restrict__ bitmaps,
                                                                   const uint32_t *__restrict__ inc64, uint32_t n_glyphs, WholeParams wp,
                                                                   uint16_t *scratch, uint32_t *__restrict__ n_chars, uint16_t *chars,
                                                                   uint32_t *pens, int64_t *__restrict__ costs) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_whole[];
    const WholeLds L = whole_carve(lds_whole, false, wp.ring_mask + 1, 0);
    const uint32_t mask = wp.ring_mask, n_live_states = 64u * g.w;
    TermIn T{nullptr, g.stride / 4, 0, (int)g.w, glyphs, offs, bitmaps};
    uint16_t *back = scratch + (size_t)blockIdx.x * wp.n_states;
    const uint32_t n_lines = *count;
    for (uint32_t k = blockIdx.x; k < n_lines; k += gridDim.x) {
        const size_t row = (size_t)k * g.cap;
        whole_begin_line<LDS>(L, strips, g, work[k], mask, &T);
        whole_forward(
            L, T, wp, inc64, n_glyphs, n_live_states, 0u,
            [&](uint32_t b0, uint32_t j) {
                const uint64_t key = L.ring[(b0 + j) & mask];
                if (key == ~0ull) return;
                back[b0 + j] = (uint16_t)key;
                whole_list(L, j);
            },
            [&](uint32_t, uint32_t s) { return L.ring[s & mask] >> 16; });
        const uint64_t best = whole_end_state(L, wp, n_live_states);
        whole_walk_back(L, wp, best, n_live_states, inc64, n_glyphs, g.cap, row, chars, pens, &n_chars[k], &costs[k],
                        [&](uint32_t t) { return (uint32_t)back[t]; });
        whole_reverse<false>(L, row, chars, pens, nullptr);
    }
}

// What line_whole_margins_kernel needs beyond the plain programme: the workgroups' scratch of 64-bit words (per
// workgroup wp.n_states of them: every live state's forward key, then cap runner keys and cap midpoints for the lines
// whose characters do not fit in LDS), and per character (the layout of chars) the results of include/focr_decode.h.
struct MarginOut {
    uint64_t *scratch;
    int32_t *term;
    uint16_t *runner;
    int64_t *margin;
};

// 3m. line_whole_kernel with margins (the definition is include/focr_decode.h's): the same programme, whose batches leave
// every state's whole key in the workgroup's scratch (~0: not reached, so this scratch is written for every state of the
// line; the low 16 bits of a key are the backpointer), then, line by line, the backward sweep described below.
template <bool LDS, bool CHARS_LDS>
__global__ __launch_bounds__(WHOLE_THREADS) void line_whole_margins_kernel(const uint8_t *__restrict__ strips, Geometry g, const uint32_t *__restrict__ work,
                                                                           const uint32_t *__restrict__ count, const DevGlyph *__restrict__ glyphs,
                                                                           const int2 *__restrict__ offs, const uint32_t *__restrict__ bitmaps,
                                                                           const uint32_t *__restrict__ inc64, uint32_t n_glyphs, WholeParams wp,
                                                                           uint32_t *__restrict__ n_chars, uint16_t *chars, uint32_t *pens,
                                                                           int64_t *__restrict__ costs, MarginOut mo) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_whole[];
    const WholeLds L = whole_carve(lds_whole, false, wp.ring_mask + 1, CHARS_LDS ? whole_chars_dwords(g.cap) : 0);
    const uint32_t tid = threadIdx.x, mask = wp.ring_mask, B = wp.batch, n_live_states = 64u * g.w;
    TermIn T{nullptr, g.stride / 4, 0, (int)g.w, glyphs, offs, bitmaps};
    uint64_t *fwd = mo.scratch + (size_t)blockIdx.x * wp.n_states;  // the forward keys, in the backpointers' place
    const uint32_t n_lines = *count;
    for (uint32_t k = blockIdx.x; k < n_lines; k += gridDim.x) {
        const size_t row = (size_t)k * g.cap;
        whole_begin_line<LDS>(L, strips, g, work[k], mask, &T);
        whole_forward(
            L, T, wp, inc64, n_glyphs, n_live_states, 0u,
            [&](uint32_t b0, uint32_t j) {
                const uint64_t key = L.ring[(b0 + j) & mask];
                fwd[b0 + j] = key;  // every state of the batch: ~0 marks the ones this line did not reach
                if (key != ~0ull) whole_list(L, j);
            },
            [&](uint32_t, uint32_t s) { return L.ring[s & mask] >> 16; });
        const uint64_t best = whole_end_state(L, wp, n_live_states);
        whole_walk_back(L, wp, best, n_live_states, inc64, n_glyphs, g.cap, row, chars, pens, &n_chars[k], &costs[k],
                        [&](uint32_t t) { return (uint32_t)fwd[t] & 0xffffu; });
        if (tid == 0) *L.cost_b = best >> 16;
        const uint32_t n = whole_reverse<false>(L, row, chars, pens, nullptr);
        if (n == 0) continue;  // uniform
        // The backward sweep of include/focr_decode.h.  ring[t & mask] now holds B[t] + 2^47 while t is within ring length
        // of the batch: every slot starts at B = 0 (the states from 64 * w on; the others are cleared before they are
        // used), and the batches are the forward pass's, last to first.  Per batch: its slots are cleared and its reached
        // states listed; barrier; every (state, glyph) edge takes B of its target, which lies above the batch and is
        // final, pushes term + B into its own state's slot, and pushes its through-cost into the runner key of every
        // character whose midpoint it covers and whose glyph is another; barrier; the count is reset; barrier.  The
        // slots of a batch alias states one ring length on, above every target of this and of later batches.
        uint64_t *rkey = CHARS_LDS ? L.rkey : fwd + wp.n_states - whole_chars_dwords(g.cap) / 2;  // [cap]
        uint32_t *mids = (uint32_t *)(rkey + g.cap);                                              // [cap], ascending
        for (uint32_t q = tid; q < n; q += WHOLE_THREADS) {
            mids[q] = pens[row + q] + (inc64[chars[row + q]] >> 1);
            rkey[q] = ~0ull;
        }
        for (uint32_t q = tid; q <= mask; q += WHOLE_THREADS) L.ring[q] = WHOLE_COST_BIAS;
        __syncthreads();
        const uint64_t line_cost = *L.cost_b;
        for (uint32_t b0 = (n_live_states - 1) / B * B;; b0 -= B) {  // n_live_states > 0: a line has characters
            const uint32_t nb = std::min(B, n_live_states - b0);
            for (uint32_t j = tid; j < nb; j += WHOLE_THREADS) {
                L.ring[(b0 + j) & mask] = ~0ull;
                if (fwd[b0 + j] != ~0ull) whole_list(L, j);
            }
            __syncthreads();
            const uint32_t nl = *L.n_live, n_cand = nl * n_glyphs;
            for (uint32_t c = tid; c < n_cand; c += WHOLE_THREADS) {
                const uint32_t gi = c / nl, s = b0 + L.live[c - gi * nl], t = s + inc64[gi];
                const int term = glyph_term_at(T, gi, wp.origin_d + (int)s);
                const uint64_t rest = L.ring[t & mask] + (uint64_t)(int64_t)term;  // term + B[t], biased: in (0, 2^48)
                atomicMin((unsigned long long *)&L.ring[s & mask], (unsigned long long)rest);
                const uint64_t through = (fwd[s] >> 16) + rest - WHOLE_COST_BIAS;  // F[s] + term + B[t], biased: a whole path's cost
                uint32_t lo = 0, hi = n;  // the first midpoint at or after s
                while (lo < hi) {
                    const uint32_t m = (lo + hi) >> 1;
                    if (mids[m] < s) lo = m + 1;
                    else hi = m;
                }
                for (; lo < n && mids[lo] < t; lo++)
                    if (chars[row + lo] != gi) atomicMin((unsigned long long *)&rkey[lo], (unsigned long long)((through << 16) | gi));
            }
            __syncthreads();
            if (tid == 0) *L.n_live = 0;
            __syncthreads();
            if (b0 == 0) break;
        }
        for (uint32_t q = tid; q < n; q += WHOLE_THREADS) {
            mo.term[row + q] = glyph_term_at(T, chars[row + q], wp.origin_d + (int)pens[row + q]);
            const uint64_t key = rkey[q];  // ~0: no edge of another glyph (a one-glyph alphabet); its index reads 0xffff
            mo.runner[row + q] = (uint16_t)key;
            mo.margin[row + q] = key != ~0ull ? (int64_t)((key >> 16) - line_cost) : -1;
        }
        __syncthreads();  // the ring, the characters' keys and the strip are free for the next line
    }
}

// What line_whole_slack_kernel needs beyond the plain programme: the radius, the workgroups' scratch of one offset per
// state beside the backpointers, and per character (the layout of chars) the chosen offset.
struct SlackOut {
    uint32_t radius;   // N >= 1
    int8_t *scratch;   // per workgroup wp.n_states offsets: off[p] of every render pen the line reached
    int8_t *offs;
};

// 3x. line_whole_kernel with pen slack (the definition is include/focr_decode.h's): a step moves the pen by an offset j,
// -N <= j <= N, before the glyph is rendered.  The ring holds the arrival states' keys as before.  A batch is
// B <= min inc64 - N consecutive render pens [b, b + B): their windows read the states [b - N, b + B + N), and the
// shortest edge from a render pen at or above b lands at or above b + min inc64 >= b + B + N, so what the batch reads is
// final when it starts.  Every arrival state of the batch that was reached leaves its glyph in the
// scratch, as in line_whole_kernel; every render pen takes the lowest (cost, rank(j)) over its window, 2N + 1 ring reads
// in rank order with a strict compare, and one that finds a state writes j to the offset scratch, keeps the cost in G and
// joins the live list; the edges are scored at the render pen and pushed from G.  The slots are cleared N late, and a
// slot's next tenant is one ring length >= B + 2N + max inc64 on, beyond every target of the batches that still read the
// slot.  The walk back alternates the two scratches: glyph of t, render pen p = t - inc64, offset of p, arrival state p - j.
template <bool LDS>
__global__ __launch_bounds__(WHOLE_THREADS) void line_whole_slack_kernel(const uint8_t *__restrict__ strips, Geometry g, const uint32_t *__restrict__ work,
                                                                         const uint32_t *__restrict__ count, const DevGlyph *__restrict__ glyphs,
                                                                         const int2 *__restrict__ offs, const uint32_t *__restrict__ bitmaps,
                                                                         const uint32_t *__restrict__ inc64, uint32_t n_glyphs, WholeParams wp,
                                                                         uint16_t *scratch, uint32_t *__restrict__ n_chars, uint16_t *chars,
                                                                         uint32_t *pens, int64_t *__restrict__ costs, SlackOut so) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_whole[];
    const WholeLds L = whole_carve(lds_whole, true, wp.ring_mask + 1, 0);
    const uint32_t mask = wp.ring_mask, n_live_states = 64u * g.w;
    const int N = (int)so.radius, n_rank = 2 * N + 1;
    TermIn T{nullptr, g.stride / 4, 0, (int)g.w, glyphs, offs, bitmaps};
    uint16_t *back = scratch + (size_t)blockIdx.x * wp.n_states;
    int8_t *off = so.scratch + (size_t)blockIdx.x * wp.n_states;
    const uint32_t n_lines = *count;
    for (uint32_t k = blockIdx.x; k < n_lines; k += gridDim.x) {
        const size_t row = (size_t)k * g.cap;
        whole_begin_line<LDS>(L, strips, g, work[k], mask, &T);
        whole_forward(
            L, T, wp, inc64, n_glyphs, n_live_states, (uint32_t)N,
            [&](uint32_t b0, uint32_t q) {
                const int p = (int)(b0 + q);
                const uint64_t here = L.ring[(uint32_t)p & mask];
                if (here != ~0ull) back[p] = (uint16_t)here;  // p as an arrival state
                uint64_t low = ~0ull >> 16;  // what an unreached state reads: above every biased cost
                int at = 0;
                for (int r = 0; r < n_rank; r++) {  // p as a render pen: the lowest (cost, rank)
                    const int j = rank_offset((uint32_t)r), s = p - j;
                    if (s < 0 || s >= (int)n_live_states) continue;
                    const uint64_t c = L.ring[(uint32_t)s & mask] >> 16;
                    if (c < low) low = c, at = j;
                }
                if (low == ~0ull >> 16) return;
                off[p] = (int8_t)at;
                L.G[q] = low;
                whole_list(L, q);
            },
            [&](uint32_t q, uint32_t) { return L.G[q]; });
        const uint64_t best = whole_end_state(L, wp, n_live_states);
        if (threadIdx.x == 0) {
            uint32_t t, n = 0;
            uint32_t gi = whole_walk_start(L, wp, best, n_live_states, &costs[k], &t);
            while (t > 0 && n < g.cap && gi < n_glyphs && inc64[gi] <= t) {  // back to front; all but t > 0 always hold and only guard the accesses
                const uint32_t p = t - inc64[gi];
                if (p >= n_live_states) break;  // never: an edge starts at a render pen below 64 * w
                const int j = off[p];
                if (j > (int)p) break;          // never: the window keeps p - j >= 0
                chars[row + n] = (uint16_t)gi;
                pens[row + n] = p;
                so.offs[row + n] = (int8_t)j;
                n++;
                t = (uint32_t)((int)p - j);
                if (t >= n_live_states) break;  // never: the window keeps p - j below 64 * w
                gi = back[t];
            }
            n_chars[k] = n;
            *L.n_chars_line = n;
        }
        // the line's own pointers and row 0, where the other two kernels pass row: this kernel's time follows how the
        // reversal is addressed, and with row it ran 1.2 to 1.7 % above the parent's span (profiles/focr_whole_refactor_bench.json)
        whole_reverse<true>(L, 0, chars + row, pens + row, so.offs + row);
    }
}

// ---- the host's side: plan, buffers, launch (decode_line.h) ----------------------------------------------------------

int whole_font_plan(focr_decoder *dec, const std::string &pre, const HostFont &f, uint64_t T, uint32_t slack, uint32_t w, WholeFontPlan *fp) {
    if (!whole_origin(f.origin_x)) return dfail(dec, pre + "whole-line decode needs origin_x to be a whole number >= 0 (at most 65536)");
    uint32_t lo = ~0u, hi = 0;
    std::vector<uint32_t> &inc64 = fp->inc64;
    inc64.resize(f.inc.size());
    for (size_t i = 0; i < f.inc.size(); i++) {
        const float v = rintf(f.inc[i] * 64.0f);
        if (!(v >= 1.f)) return dfail(dec, pre + "whole-line decode needs every pen increment to be at least 1/64 px (an inc64 below 1)");
        inc64[i] = v < 16777216.f ? (uint32_t)v : (1u << 24);
        lo = std::min(lo, inc64[i]), hi = std::max(hi, inc64[i]);
    }
    if (64ull * w + hi >= (1ull << 24))
        return dfail(dec, pre + "whole-line decode needs 64 * width + the largest inc64 below 2^24 (pens must stay exact in f32)");
    if (2 * slack > lo)
        return dfail(dec, pre + "whole-line decode: the pen slack is more than half the smallest inc64 (focr_decoder_set_whole_slack; the pen could crawl)");
    const uint32_t gain = lo - slack;  // every character advances the arrival state by at least this from below 64 * w; >= 1
    fp->cap = std::max<uint32_t>((64u * w + gain - 1) / gain, 1);
    if ((uint64_t)fp->cap * T >= (1ull << 47))
        return dfail(dec, pre + "whole-line decode: characters per line times the font's score bound reaches 2^47 (a packed cost could overflow)");
    fp->origin_d = 64 * (int)f.origin_x;
    fp->batch = std::min(gain, WHOLE_BATCH_MAX);
    fp->max_inc = hi;
    uint32_t ring = 64;
    while (ring < fp->batch + 2 * slack + hi && ring <= WHOLE_RING_MAX) ring *= 2;
    if (ring > WHOLE_RING_MAX)
        return dfail(dec, pre + (slack ? "whole-line decode with pen slack: the widest advance and the slack are too large (the cost ring does not fit in LDS)"
                                       : "whole-line decode: the widest advance is too large (the cost ring does not fit in LDS)"));
    fp->ring = ring;
    return 0;
}

void whole_plan_grid(const RunMode &mode, const Geometry &g, bool margins, const WholeScratch &sc, WholePlan *plan) {
    plan->n_states = 64u * g.w + plan->max_inc + (margins ? whole_chars_dwords(plan->cap) / 2 : 0);
    const size_t fit = std::max<size_t>(sc.budget / ((size_t)plan->n_states * sc.state_bytes), 1);
    plan->grid = (uint32_t)std::min<size_t>({g.total, fit, WHOLE_GRID_MAX});
    if (mode.grid) plan->grid = std::min(plan->grid, mode.grid);
}

int whole_plan(focr_decoder *dec, const RunMode &mode, const Geometry &g, WholePlan *plan) {
    if (mode.kind == Kind::whole_fonts) return whole_fonts_plan(dec, mode, g, plan);
    const uint32_t slack = mode.kind == Kind::whole_slack ? mode.radius : 0;
    const bool margins = mode.margins(), candidates = mode.kind == Kind::whole_baseline;
    uint64_t T = dec->font.term_bound;  // set_font's own bound on a term's magnitude
    if (candidates && dec->yfonts.ok) T = std::max(T, dec->yfonts.term_bound);  // box sizes differ between y-phases
    WholeFontPlan fp;
    if (whole_font_plan(dec, "focr_decoder_run: ", dec->font, T, slack, g.w, &fp)) return 1;
    plan->inc64 = std::move(fp.inc64);
    plan->cap = fp.cap, plan->origin_d = fp.origin_d, plan->batch = fp.batch, plan->max_inc = fp.max_inc, plan->ring = fp.ring;
    // a workgroup's scratch: a word per state 0 .. 64 * w + max inc64, with margins then the characters' keys and midpoints;
    // as many workgroups as the mode's budget allows (one always)
    whole_plan_grid(mode, g, margins, margins ? WHOLE_SCRATCH_MARGINS : slack ? WHOLE_SCRATCH_SLACK : candidates ? WHOLE_SCRATCH_BASELINE : WHOLE_SCRATCH_PLAIN, plan);
    return 0;
}

int whole_reserve(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan) {
    const size_t chars = (size_t)g.cap * g.total, scratch = (size_t)plan.grid * plan.n_states;
    if (mode.margins()) {
        DEC_GROW(dec->d_fwd, scratch);
        DEC_GROW(dec->d_mterm, chars);
        DEC_GROW(dec->d_mrunner, chars);
        DEC_GROW(dec->d_margin, chars);
    } else
        DEC_GROW(dec->d_back, mode.halves() ? 2 * scratch : scratch);  // baseline or font candidates: two halves per workgroup
    if (mode.base_q()) DEC_GROW(dec->d_base_q, g.total);
    if (mode.kind == Kind::whole_slack) DEC_GROW(dec->d_woff, scratch);
    DEC_GROW(dec->d_pens, chars);
    DEC_GROW(dec->d_cost, g.total);
    if (!dec->d_inc64.p) DEC_UPLOAD(dec->d_inc64, plan.inc64.data(), plan.inc64.size());
    return mode.kind == Kind::whole_fonts ? whole_fonts_reserve(dec, plan) : 0;
}

// The strip shares LDS with what whole_layout puts before it; with margins the characters' keys and midpoints come first:
// beside the ring when they fit, then the strip when it still fits.
void whole_launch(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan, size_t strip_bytes) {
    const WholeParams wp{plan.origin_d, plan.batch, plan.ring - 1, plan.max_inc, plan.n_states};
    const bool margins = mode.margins(), slack = mode.kind == Kind::whole_slack;
    const uint32_t chars_dwords = whole_chars_dwords(g.cap);
    const bool chars_lds = margins && whole_fixed_bytes(false, plan.ring, chars_dwords) <= LDS_STRIP_MAX;
    const size_t fixed = whole_fixed_bytes(slack, plan.ring, chars_lds ? chars_dwords : 0);
    const bool lds = strip_bytes + fixed <= LDS_STRIP_MAX;
    const size_t lds_bytes = fixed + (lds ? strip_bytes : 0);
    if (margins) {
        const auto kernel = lds ? (chars_lds ? line_whole_margins_kernel<true, true> : line_whole_margins_kernel<true, false>)
                                : (chars_lds ? line_whole_margins_kernel<false, true> : line_whole_margins_kernel<false, false>);
        kernel<<<plan.grid, WHOLE_THREADS, lds_bytes, dec->stream>>>(
            dec->d_strips, g, dec->d_work, dec->d_count, dec->tables.glyphs, dec->tables.offs, dec->tables.bitmaps.as<const uint32_t>(), dec->d_inc64, dec->n_glyphs, wp,
            dec->d_nchars, dec->d_chars, dec->d_pens, dec->d_cost, MarginOut{dec->d_fwd, dec->d_mterm, dec->d_mrunner, dec->d_margin});
    } else if (slack) {
        (lds ? line_whole_slack_kernel<true> : line_whole_slack_kernel<false>)<<<plan.grid, WHOLE_THREADS, lds_bytes, dec->stream>>>(
            dec->d_strips, g, dec->d_work, dec->d_count, dec->tables.glyphs, dec->tables.offs, dec->tables.bitmaps.as<const uint32_t>(), dec->d_inc64, dec->n_glyphs, wp,
            dec->d_back, dec->d_nchars, dec->d_chars, dec->d_pens, dec->d_cost, SlackOut{mode.radius, dec->d_woff, dec->d_pen});
    } else {
        (lds ? line_whole_kernel<true> : line_whole_kernel<false>)<<<plan.grid, WHOLE_THREADS, lds_bytes, dec->stream>>>(
            dec->d_strips, g, dec->d_work, dec->d_count, dec->tables.glyphs, dec->tables.offs, dec->tables.bitmaps.as<const uint32_t>(), dec->d_inc64, dec->n_glyphs, wp,
            dec->d_back, dec->d_nchars, dec->d_chars, dec->d_pens, dec->d_cost);
    }
}

}  // namespace focr_dec
