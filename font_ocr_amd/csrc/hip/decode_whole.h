// decode_whole.h — what the whole-line kernels of the `focr` line decoder are built from (decode_whole.hip: the programme,
// its margins and its pen slack; decode_whole_baseline.hip: the programme under every baseline candidate): the limits, the
// LDS layout, which has one owner, whole_layout (the kernels carve from it and the launches size from it), and the phases
// of a line, each stated once.  Device helpers only (no relocatable device code: they are inlined into each kernel).
#pragma once

#include "decode_line.h"

namespace focr_dec {

constexpr uint32_t WHOLE_THREADS = 256;     // one workgroup of four waves per work-list line at a time
constexpr uint32_t WHOLE_WAVES = WHOLE_THREADS / 64;
constexpr uint32_t WHOLE_BATCH_MAX = 512;   // states per batch at most (and at most the smallest inc64)
constexpr uint32_t WHOLE_RING_MAX = 4096;   // keys of the cost ring at most: ring and the rest stay inside LDS_STRIP_MAX
constexpr uint64_t WHOLE_COST_BIAS = 1ull << 47;
constexpr size_t WHOLE_SCRATCH_BUDGET = 64u << 20;  // bytes of backpointer scratch at most (a single workgroup's may exceed it)
constexpr uint32_t WHOLE_GRID_MAX = 2048;

// Dwords of a line's runner keys (64-bit) and midpoints beside the ring or in the scratch, a multiple of four.
__host__ __device__ constexpr uint32_t whole_chars_dwords(uint32_t cap) { return (3 * cap + 3) & ~3u; }

// ---- the host's plan, as the whole-line files share it (decode_whole.hip has the definitions) ------------------------

// The workgroups' scratch of a mode: bytes per state, and the bytes all workgroups together may take.  Plain: a 16-bit
// backpointer.  Margins: a 64-bit forward key in its place (and the characters' keys and midpoints, counted as states).
// Slack: an 8-bit offset beside every backpointer, and both count.  Baseline or font candidates: two halves of
// backpointers, with twice the budget, so that the grid is the plain run's.
struct WholeScratch {
    size_t state_bytes, budget;
};
constexpr WholeScratch WHOLE_SCRATCH_PLAIN{sizeof(uint16_t), WHOLE_SCRATCH_BUDGET};
constexpr WholeScratch WHOLE_SCRATCH_MARGINS{sizeof(uint64_t), 4 * WHOLE_SCRATCH_BUDGET};
constexpr WholeScratch WHOLE_SCRATCH_SLACK{sizeof(uint16_t) + sizeof(int8_t), WHOLE_SCRATCH_BUDGET / 2 * 3};
constexpr WholeScratch WHOLE_SCRATCH_BASELINE{2 * sizeof(uint16_t), 2 * WHOLE_SCRATCH_BUDGET};

// What the whole-line checks make of one font for a crop of w columns: whole_plan's part that depends on the font alone.
struct WholeFontPlan {
    std::vector<uint32_t> inc64;
    int origin_d = 0;
    uint32_t batch = 0, ring = 0, max_inc = 0, cap = 1;
};

// The font refusals of a whole-line run (include/focr_decode.h) for one font, each message behind `pre`, and its plan.
// T: the bound on a term's magnitude; slack: the pen slack's radius (0 without).
int whole_font_plan(focr_decoder *dec, const std::string &pre, const HostFont &f, uint64_t T, uint32_t slack, uint32_t w, WholeFontPlan *fp);
// The scratch of one workgroup (from plan->max_inc and plan->cap) and the grid the mode's budget allows.
void whole_plan_grid(const RunMode &mode, const Geometry &g, bool margins, const WholeScratch &sc, WholePlan *plan);
// whole_plan, whole_reserve's part and the launch of a whole_fonts run (decode_whole_fonts.hip).
int whole_fonts_plan(focr_decoder *dec, const RunMode &mode, const Geometry &g, WholePlan *plan);
int whole_fonts_reserve(focr_decoder *dec, const WholePlan &plan);

// ---- the LDS of a workgroup ----------------------------------------------------------------------------------------

// Byte offsets into the workgroup's dynamic LDS: a head of 64 bytes (the waves' end keys; the batch's live count and the
// line's character count; the line's cost + 2^47, which the margins sweep reads; the scratch half the next baseline
// candidate writes), the batch's live list, with slack G of the batch's render pens, the cost ring, with margins the
// characters' runner keys and midpoints when they fit (else chars_dwords is 0 and they go to the scratch), and then the
// strip when it fits in what is left of LDS_STRIP_MAX.
struct WholeLayout {
    uint32_t red, n_live, n_chars_line, cost_b, half, live, G, ring, chars, strip;
};

__host__ __device__ constexpr WholeLayout whole_layout(bool slack, uint32_t ring, uint32_t chars_dwords) {
    WholeLayout l{};
    l.red = 0;                                          // uint64_t[WHOLE_WAVES]
    l.n_live = l.red + 8 * WHOLE_WAVES;                 // uint32_t
    l.n_chars_line = l.n_live + 4;                      // uint32_t
    l.cost_b = l.n_chars_line + 4;                      // uint64_t
    l.half = l.cost_b + 8;                              // uint32_t
    l.live = 64;                                        // uint16_t[WHOLE_BATCH_MAX], behind the head padded to 64 bytes
    l.G = l.live + 2 * WHOLE_BATCH_MAX;                 // uint64_t[WHOLE_BATCH_MAX], slack only
    l.ring = l.G + (slack ? 8 * WHOLE_BATCH_MAX : 0);   // uint64_t[ring]
    l.chars = l.ring + 8 * ring;                        // uint64_t[cap], then uint32_t[cap]
    l.strip = l.chars + 4 * chars_dwords;
    return l;
}

// The LDS of a mode before the strip: what the launch asks for beyond the strip, and what decides whether the strip fits.
__host__ __device__ constexpr uint32_t whole_fixed_bytes(bool slack, uint32_t ring, uint32_t chars_dwords) {
    return whole_layout(slack, ring, chars_dwords).strip;
}

static_assert(whole_layout(false, 64, 0).half + 4 <= whole_layout(false, 64, 0).live, "the head fits before the live list");
static_assert(whole_fixed_bytes(false, 64, 0) == 1088 + 8 * 64 && whole_fixed_bytes(false, WHOLE_RING_MAX, 0) == 1088 + 8 * WHOLE_RING_MAX, "plain");
static_assert(whole_fixed_bytes(true, 64, 0) == 5184 + 8 * 64 && whole_fixed_bytes(true, WHOLE_RING_MAX, 0) == 5184 + 8 * WHOLE_RING_MAX, "slack");
static_assert(whole_fixed_bytes(false, 256, whole_chars_dwords(77)) == 1088 + 8 * 256 + 4 * whole_chars_dwords(77), "margins, characters in LDS");
static_assert(whole_layout(true, 64, 0).ring % 16 == 0 && whole_layout(false, 64, 4).strip % 16 == 0, "64-bit keys and the strip stay aligned");

struct WholeLds {
    uint64_t *red;           // [WHOLE_WAVES]
    uint32_t *n_live;        // the batch's live count
    uint32_t *n_chars_line;  // the line's character count, from thread 0 to the workgroup
    uint64_t *cost_b;        // the line's cost + 2^47 (margins)
    uint32_t *half;          // the scratch half the next candidate writes, from thread 0 to the workgroup (baseline candidates)
    uint16_t *live;          // [WHOLE_BATCH_MAX]: the batch's live states, as offsets from its start
    uint64_t *G;             // [WHOLE_BATCH_MAX]: cost + 2^47 at the batch's render pens (slack)
    uint64_t *ring;          // [ring]
    uint64_t *rkey;          // [cap]: the characters' runner keys, then uint32_t[cap] their midpoints (margins with the characters in LDS)
    uint32_t *strip;
};

__device__ __forceinline__ WholeLds whole_carve(uint32_t *lds, bool slack, uint32_t ring, uint32_t chars_dwords) {
    const WholeLayout l = whole_layout(slack, ring, chars_dwords);
    return WholeLds{(uint64_t *)(lds + l.red / 4),  lds + l.n_live / 4,          lds + l.n_chars_line / 4,    (uint64_t *)(lds + l.cost_b / 4),
                    lds + l.half / 4,               (uint16_t *)(lds + l.live / 4), (uint64_t *)(lds + l.G / 4), (uint64_t *)(lds + l.ring / 4),
                    (uint64_t *)(lds + l.chars / 4), lds + l.strip / 4};
}

// ---- the phases ----------------------------------------------------------------------------------------------------

struct WholeParams {
    int origin_d;        // 64 * origin_x
    uint32_t batch;      // B: states per batch, <= the smallest inc64
    uint32_t ring_mask;  // ring length - 1; the length is a power of two >= B + max_inc
    uint32_t max_inc;    // the largest inc64
    uint32_t n_states;   // 64 * w + max_inc: the scratch of one workgroup
};

// What a footprint term is scored from: the line's strip and crop, the font's tables, and the rows every box is moved
// down by (0 but under a baseline candidate, which also brings its y-phase's tables).
struct TermIn {
    const uint32_t *strip;
    uint32_t sdw, h;
    int w;
    const DevGlyph *glyphs;
    const int2 *offs;
    const uint32_t *bitmaps;
    int d;
};

// The footprint term of glyph gi rendered at delta d (pen and origin, in 1/64 px); footprint_term clips the rows that
// T.d pushes out of the crop, on both sides.
__device__ __forceinline__ int glyph_term_at(const TermIn &T, uint32_t gi, int d) {
    const int phase = d & 63, shift = d >> 6;
    const DevGlyph gl = T.glyphs[gi];
    const int2 o = T.offs[gi * 64 + phase];
    return footprint_term(T.strip, T.sdw, T.w, T.h, T.bitmaps + gl.off_dw + (uint32_t)phase * gl.ndw * gl.box_h, gl.ndw, gl.box_h, shift + o.x, o.y + T.d);
}

// A line's rows and its strip, staged in LDS when it fits, on a line grid (decode.h); the centre of the line's baseline
// candidates for y_bits `bits` is returned (0 on the whole-pixel grid).  No barrier: whole_reset's follows.
template <bool LDS, class Grid = PixelGrid>
__device__ __forceinline__ int whole_stage(const WholeLds &L, const uint8_t *__restrict__ strips, const Geometry &g, uint32_t slot, TermIn *T,
                                           const Grid &grid = Grid{}, uint32_t bits = 0) {
    const uint32_t tid = threadIdx.x;
    uint32_t yc;
    int centre;
    grid.rows(g, slot % g.n_slots, bits, &yc, &T->h, &centre);
    T->strip = (const uint32_t *)(strips + (size_t)slot * g.stride * g.line_height);
    if (LDS) {
        for (uint32_t q = tid; q < T->sdw * T->h; q += WHOLE_THREADS) L.strip[q] = T->strip[q];
        T->strip = L.strip;
    }
    return centre;
}

// A programme begins: the ring with cost[0] = 0 and every other state unreachable, no live state.  ring[s & mask] holds
// state s's key ((cost + 2^47) << 16 | remembered glyph; ~0: unreachable) while s is within ring length of the batch.
__device__ __forceinline__ void whole_reset(const WholeLds &L, uint32_t mask) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t q = tid; q <= mask; q += WHOLE_THREADS) L.ring[q] = q ? ~0ull : (WHOLE_COST_BIAS << 16) | 0xffffu;  // cost[0] = 0, no glyph
    if (tid == 0) *L.n_live = 0;
    __syncthreads();
}

// A line begins: its rows and strip, then its one programme.
template <bool LDS>
__device__ __forceinline__ void whole_begin_line(const WholeLds &L, const uint8_t *__restrict__ strips, const Geometry &g, uint32_t slot, uint32_t mask, TermIn *T) {
    whole_stage<LDS>(L, strips, g, slot, T);
    whole_reset(L, mask);
}

// Entry j of the batch joins its live list.
__device__ __forceinline__ void whole_list(const WholeLds &L, uint32_t j) { L.live[atomicAdd(L.n_live, 1u)] = (uint16_t)j; }

// The edges of a batch: the (live entry, glyph) candidates, glyph-major over the lanes (neighbouring lanes share a box),
// are scored at the entry's pen and pushed into the target's slot with an LDS 64-bit atomic min, whose order cannot
// matter.  cost_at(j, s) is the cost + 2^47 of entry j, pen s.
template <typename Cost>
__device__ __forceinline__ void whole_push_edges(const WholeLds &L, const TermIn &T, const WholeParams &wp, const uint32_t *__restrict__ inc64, uint32_t n_glyphs,
                                                 uint32_t b0, Cost cost_at) {
    const uint32_t nl = *L.n_live, n_cand = nl * n_glyphs;  // nl <= 512 and n_glyphs < 65536
    for (uint32_t c = threadIdx.x; c < n_cand; c += WHOLE_THREADS) {
        const uint32_t gi = c / nl, j = L.live[c - gi * nl], s = b0 + j;
        const int term = glyph_term_at(T, gi, wp.origin_d + (int)s);
        const uint64_t cost = cost_at(j, s) + (uint64_t)(int64_t)term;  // biased, mod 2^64: stays in (0, 2^48)
        atomicMin((unsigned long long *)&L.ring[(s + inc64[gi]) & wp.ring_mask], (unsigned long long)((cost << 16) | gi));
    }
}

// The forward pass, batch by batch.  A batch is B consecutive pens, and B is at most the shortest step (less the slack), so
// nothing scored in a batch lands in it: what it reads is final when it starts.  Per batch: collect(b0, j) looks at
// entry j < nb, leaves in the scratch what the walk back needs and lists the entry when an edge can start there
// (whole_list); barrier; the edges; barrier; the batch's slots are cleared for the states one ring length on, `late`
// states behind the batch (the slack's windows still read that many of its last states in the next batch), and the live
// count is reset; barrier.  The targets of a batch reach at most B - 1 + max inc64 past its start, so with a ring of at
// least B + 2 * late + max inc64 slots they never alias a slot that is still read.  When the pass ends the states
// 64 * w .. are all still in the ring.
template <typename Collect, typename Cost>
__device__ __forceinline__ void whole_forward(const WholeLds &L, const TermIn &T, const WholeParams &wp, const uint32_t *__restrict__ inc64, uint32_t n_glyphs,
                                              uint32_t n_live_states, uint32_t late, Collect collect, Cost cost_at) {
    const uint32_t tid = threadIdx.x, B = wp.batch, mask = wp.ring_mask;
    for (uint32_t b0 = 0; b0 < n_live_states; b0 += B) {
        const uint32_t nb = std::min(B, n_live_states - b0);
        for (uint32_t j = tid; j < nb; j += WHOLE_THREADS) collect(b0, j);
        __syncthreads();
        whole_push_edges(L, T, wp, inc64, n_glyphs, b0, cost_at);
        __syncthreads();
        for (uint32_t j = tid; j < nb; j += WHOLE_THREADS)
            if (b0 + j >= late) L.ring[(b0 + j - late) & mask] = ~0ull;
        if (tid == 0) *L.n_live = 0;
        __syncthreads();
    }
}

// The end state: the lowest (cost, t) over t = 64 * w + e, e < max_inc (e < 4096 takes the glyph's place in the key).
// Complete in thread 0 only; ~0: no end state was reached.
__device__ __forceinline__ uint64_t whole_end_state(const WholeLds &L, const WholeParams &wp, uint32_t n_live_states) {
    const uint32_t tid = threadIdx.x;
    uint64_t best = ~0ull;
    for (uint32_t e = tid; e < wp.max_inc; e += WHOLE_THREADS) {
        const uint64_t key = L.ring[(n_live_states + e) & wp.ring_mask];
        if (key != ~0ull) best = std::min<uint64_t>(best, (key & ~(uint64_t)0xffff) | e);
    }
    for (int m = 32; m >= 1; m >>= 1) best = std::min(best, shfl_xor_u64(best, m));
    if ((tid & 63) == 0) L.red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0)
        for (uint32_t v = 1; v < WHOLE_WAVES; v++) best = std::min(best, L.red[v]);
    return best;
}

// Thread 0's walk back starts: the line's cost goes out, *t is the end state and the glyph that reached it is returned.
// Some end state is reachable (every step from a state below 64 * w lands somewhere); without one the line is empty.
__device__ __forceinline__ uint32_t whole_walk_start(const WholeLds &L, const WholeParams &wp, uint64_t best, uint32_t n_live_states, int64_t *cost, uint32_t *t) {
    *t = best != ~0ull ? n_live_states + (uint32_t)(best & 0xffffu) : 0;
    *cost = best != ~0ull ? (int64_t)((best >> 16) - WHOLE_COST_BIAS) : 0;
    return (uint32_t)L.ring[*t & wp.ring_mask] & 0xffffu;
}

// Thread 0's walk back without slack from state t, which glyph gi reached (a programme whose ring is gone: the winner of
// the baseline candidates), back to front: a character's pen is the state
// its glyph's increment below, and glyph_at(t) is the glyph the scratch remembers for state t.  The scratch needs no
// clearing: the walk visits only states this programme reached and wrote.  All of the loop's conditions but t > 0 always
// hold (the host's bound; a reached state's glyph) and only guard the accesses.
template <typename GlyphAt>
__device__ __forceinline__ void whole_walk_from(const WholeLds &L, uint32_t t, uint32_t gi, const uint32_t *__restrict__ inc64, uint32_t n_glyphs, uint32_t cap,
                                                size_t row, uint16_t *chars, uint32_t *pens, uint32_t *n_chars, GlyphAt glyph_at) {
    uint32_t n = 0;
    while (t > 0 && n < cap && gi < n_glyphs && inc64[gi] <= t) {
        t -= inc64[gi];
        chars[row + n] = (uint16_t)gi;
        pens[row + n] = t;
        n++;
        gi = glyph_at(t);
    }
    *n_chars = n;
    *L.n_chars_line = n;
}

// Thread 0's walk back from the end state of the programme whose ring is still in LDS: whole_walk_start, then
// whole_walk_from's loop, restated here: calling whole_walk_from changes line_whole_margins_kernel's machine code
// (tools/isa_hash.py, profiles/focr_whole_baseline_isa.json), which its benchmark pins.
template <typename GlyphAt>
__device__ __forceinline__ void whole_walk_back(const WholeLds &L, const WholeParams &wp, uint64_t best, uint32_t n_live_states, const uint32_t *__restrict__ inc64,
                                                uint32_t n_glyphs, uint32_t cap, size_t row, uint16_t *chars, uint32_t *pens, uint32_t *n_chars, int64_t *cost,
                                                GlyphAt glyph_at) {
    if (threadIdx.x != 0) return;
    uint32_t t, n = 0;
    uint32_t gi = whole_walk_start(L, wp, best, n_live_states, cost, &t);
    while (t > 0 && n < cap && gi < n_glyphs && inc64[gi] <= t) {
        t -= inc64[gi];
        chars[row + n] = (uint16_t)gi;
        pens[row + n] = t;
        n++;
        gi = glyph_at(t);
    }
    *n_chars = n;
    *L.n_chars_line = n;
}

// The walk's n characters (thread 0 left the count in LDS), from chars[row] on, into text order, by the workgroup; the
// count is returned.  The barrier at the end frees the ring, the strip and the counts for what follows.
template <bool OFFS>
__device__ __forceinline__ uint32_t whole_reverse(const WholeLds &L, size_t row, uint16_t *chars, uint32_t *pens, int8_t *offs) {
    __syncthreads();
    const uint32_t n = *L.n_chars_line;
    for (uint32_t q = threadIdx.x; q < n / 2; q += WHOLE_THREADS) {
        const size_t a = row + q, b = row + n - 1 - q;
        const uint16_t ca = chars[a], cb = chars[b];
        const uint32_t pa = pens[a], pb = pens[b];
        const int8_t ja = OFFS ? offs[a] : 0, jb = OFFS ? offs[b] : 0;
        chars[a] = cb, chars[b] = ca;
        pens[a] = pb, pens[b] = pa;
        if (OFFS) offs[a] = jb, offs[b] = ja;
    }
    __syncthreads();
    return n;
}

}  // namespace focr_dec
