// post.hip — process_hits on the device (reference: src/ncc.rs:723-786 + partition_by 1036-1052).
//
//  (1) keep_y: rows y with any hit of similarity >= anchor_threshold (f32 >=), per page   :726-731
//  (2) keep hits on those rows, in get_hits order                                       :732-738
//  (3) stable sort by y, then each equal-y run stable-sorted by x                       :741-752
//      => total order (y, x, get_hits order); get_hits order of two hits with equal
//      (x, y) is their template index, so the sort key is (page, y, x, t).
//  (4) per line, groups anchored on the group's first element: a hit joins while
//      |x - x_first| <= overlap                                                         :755-757, 1042-1048
//  (5) per group the maximum similarity by f32::total_cmp, LAST maximum wins            :761-764
//  (6) lines ascending in y, characters ascending in x.
#include <cstring>

#include "common.h"

namespace focr {

__device__ __forceinline__ int32_t total_key(float f) {  // f32::total_cmp as a signed-int order
    int32_t b = __float_as_int(f);
    return b ^ (int32_t)(((uint32_t)(b >> 31)) >> 1);
}

// (1) keep_y: rows with a kept hit of similarity >= anchor_threshold; also the extent of every (page, row) line in
// the sorted hit list (one thread per hit looks at its neighbours), so that the line walk needs no search.
__global__ void mark_anchor_rows(const uint64_t *__restrict__ hkeys, const float *__restrict__ hsims, const uint8_t *__restrict__ keep,
                                 const uint64_t *__restrict__ n_p, uint64_t ub, KeyFmt fmt, float anchor, uint32_t r_h, uint8_t *__restrict__ keep_row,
                                 uint32_t *__restrict__ line_b, uint32_t *__restrict__ line_e) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t n = (size_t)min(*n_p, ub);  // device-side count, clamped to what the grid and buffers were sized for
    if (i >= n) return;
    const uint64_t k = hkeys[i];
    const size_t row = (size_t)fmt.page(k) * r_h + fmt.y(k);
    if (i == 0 || fmt.line(hkeys[i - 1]) != fmt.line(k)) line_b[row] = (uint32_t)i;
    if (i + 1 == n || fmt.line(hkeys[i + 1]) != fmt.line(k)) line_e[row] = (uint32_t)(i + 1);
    if (keep[i] && hsims[i] >= anchor) keep_row[row] = 1;
}

// wave64 unsigned max via DPP (row_shr 1/2/4/8, row_bcast 15/31): the result is uniform (read from lane 63)
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// One wave per anchored (page, row): walks the row's extent of the (page, y, x, t)-sorted hit list 64 elements at a
// time.  Hits cut off by the per-call cap (keep[i] == 0) are not part of the reference's all_hits and are transparent
// here.  Groups are anchored on their first element (partition_by keeps `last` until a group closes,
// src/ncc.rs:1042-1048), so group boundaries are sequential, but every step is a handful of wave operations: a ballot
// for the group's extent inside the chunk, a DPP max-reduction of the similarity order (f32::total_cmp), and a ballot
// of the lanes that reach it — the highest such lane is the LAST maximum, which is what max_by keeps (:761-764).
// Outputs: choice[b + k] = winning element of the row's k-th group, row_groups[row] = 1<<32 | number of groups.
constexpr uint32_t WALK_ROWS = 16;  // (page, row) entries per wave

// focr_get_runners' second walk (walk_runners below): what the walk carries per open group on top of the winner.  A Top is one
// member: its total_cmp order, its element index in the row and its letter, and what its record needs (template and x: a group's
// close then stores without loading anything); `has` says that there is one at all, because order 0 is a legal similarity (the
// negative NaN with every payload bit set).
struct Top {
    uint32_t ord, idx, letter, t, x;
    bool has;
};
// b takes a's place as the LAST maximum: a higher order, or the same order further on in (x, t)
__device__ __forceinline__ bool top_beats(const Top &a, const Top &b) { return b.has && (!a.has || b.ord > a.ord || (b.ord == a.ord && b.idx > a.idx)); }
struct RunnerArgs {  // RUNNERS only
    const uint32_t *t_letter;  // by global template index
    const uint64_t *scanned;   // the row scan of process_hits: low word = the row's first character
    focr_runner_t *out;
    uint32_t bound;            // records `out` has room for
};
__device__ __forceinline__ void store_runner(const RunnerArgs &ra, uint32_t slot, uint32_t members, const Top &second) {
    if (slot >= ra.bound) return;
    focr_runner_t r;
    r.members = members;
    r.letter = r.template_index = FOCR_NO_RUNNER;
    r.similarity = -__builtin_inff();
    r.x = r.reserved = 0;
    if (second.has) {
        r.letter = second.letter;
        r.template_index = second.t;
        // total_key is its own inverse (the sign bit selects the mask and stays): the similarity's bits as they were, so that a
        // NaN or -inf runner is told from "none" by template_index alone
        r.similarity = __int_as_float(total_key(__int_as_float((int32_t)(second.ord ^ 0x80000000u))));
        r.x = (uint16_t)second.x;
    }
    ra.out[slot] = r;
}

// The walk of both kernels.  RUNNERS = false is walk_lines as it always was (same instruction stream: DESIGN.md 4c); RUNNERS = true
// walks the rows again after process_hits and writes no choice / row_groups but one focr_runner_t per group, at the slot emit_chars
// gave the group's character: the group's size and the last maximum among its members of ANOTHER letter than the winner's.
// Per open group it carries a top-2 over distinct letters (best, second = the best member whose letter differs from best's); a
// chunk gives (m1, m2) the same way, and the merge is exact because whatever a side left out as "same letter as its best" is
// dominated by that best: second' = the last maximum of {loser of best / m1, second, m2} whose letter differs from best'.
struct NoArgs {};
__device__ __forceinline__ NoArgs runner_args() { return {}; }
__device__ __forceinline__ const RunnerArgs &runner_args(const RunnerArgs &ra) { return ra; }
template <bool RUNNERS, typename... Extra>  // Extra: RunnerArgs if RUNNERS, else nothing, so that walk_lines keeps its kernel arguments
__global__ __launch_bounds__(256) void walk_kernel(const uint64_t *__restrict__ keys, const float *__restrict__ sims,
                                                   const uint8_t *__restrict__ keep, KeyFmt fmt, uint32_t n_rows_total,
                                                   int32_t overlap, const uint8_t *__restrict__ keep_row,
                                                   const uint32_t *__restrict__ line_b, const uint32_t *__restrict__ line_e,
                                                   uint32_t *__restrict__ choice, uint64_t *__restrict__ row_groups,
                                                   const Extra... extra) {
    static_assert(sizeof...(Extra) == (RUNNERS ? 1 : 0), "walk_runners takes one RunnerArgs, walk_lines nothing");
    [[maybe_unused]] const auto ra = runner_args(extra...);
    // A wave looks at WALK_ROWS consecutive (page, row) entries at once and walks the anchored ones among them (one text line in
    // fifteen rows at BASELINE configs[1]): one wave per ROW meant 92 160 waves per batch of which 6 000 had work — 77 us alone and
    // 0.33 ms in flight for a few microseconds of arithmetic.
    const uint32_t wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    const uint32_t row_first = wave_id * WALK_ROWS;
    if (row_first >= n_rows_total) return;
    const uint32_t my_row = row_first + lane;
    const bool mine = lane < WALK_ROWS && my_row < n_rows_total && keep_row[my_row] != 0;  // keep_row / line_b / line_e / row_groups are [page][y] with pitch r_h
    const uint32_t my_b = mine ? line_b[my_row] : 0u, my_e = mine ? line_e[my_row] : 0u;  // written by mark_anchor_rows for every row that has hits
    for (uint64_t todo = __builtin_amdgcn_ballot_w64(mine); todo; todo &= todo - 1) {
    const int src = (int)__builtin_ctzll(todo);
    const uint32_t wave = row_first + (uint32_t)src;  // the row this pass walks
    const uint64_t b = (uint32_t)__builtin_amdgcn_readlane((int)my_b, src), e = (uint32_t)__builtin_amdgcn_readlane((int)my_e, src);

    uint32_t groups = 0;
    bool open = false;            // a group is open (carried across chunks)
    int32_t anchor = 0;           // x of the open group's first element
    uint32_t best_ord = 0, best_idx = 0;  // winner so far of the open group: total_cmp order, element index
    Top a1{}, a2{};               // RUNNERS: the open group's best and the best of another letter
    uint32_t members = 0, slot0 = 0;
    if constexpr (RUNNERS) slot0 = (uint32_t)ra.scanned[wave];
    for (uint64_t base = b; base < e; base += 64) {
        const uint64_t i = base + lane;
        const bool valid = i < e && keep[i];
        const int32_t x = valid ? (int32_t)fmt.x(keys[i]) : 0x7fffffff;
        const uint32_t ord = valid ? ((uint32_t)total_key(sims[i]) ^ 0x80000000u) : 0u;  // unsigned order of total_cmp
        uint32_t let = 0, tt = 0;
        if constexpr (RUNNERS) {
            tt = valid ? fmt.t(keys[i]) : 0u;
            let = valid ? ra.t_letter[tt] : 0u;
        }
        const uint64_t vmask = __builtin_amdgcn_ballot_w64(valid);
        uint32_t pos = 0;  // wave-uniform cursor inside the chunk
        int32_t opened_at = -1;  // lane of the element that opened the open group in this chunk; -1: the group was carried in
        // Termination, for every overlap (INT32_MIN included): the opener of a group is always a member (partition_by puts the
        // first element of a slice in it whatever the predicate says, src/ncc.rs:1040-1048), so a trip that opens a group at pos
        // ends with stop > pos.  A trip that opens nothing is the chunk's first, with a carried group: it closes that group at
        // stop >= pos or leaves the chunk.  So every trip but the first consumes an element or leaves: at most 65 trips a chunk.
        while (pos < 64) {
            if (!open) {
                const uint64_t cand = vmask & (~0ull << pos);  // the next kept element opens a group
                if (!cand) break;
                pos = (uint32_t)__builtin_ctzll(cand);
                anchor = __builtin_amdgcn_readlane(x, (int)pos);
                opened_at = (int32_t)pos;
                best_ord = 0;
                best_idx = 0;
                open = true;
                if constexpr (RUNNERS) a1.has = a2.has = false, members = 0;
            }
            // kept members of the open group at/after pos; the first kept non-member closes it.  With overlap < 0 nothing but
            // the opener is a member: every kept hit of an anchored row is a character of its own.
            const bool in = valid && lane >= pos && ((int32_t)lane == opened_at || ((x - anchor <= overlap) && (anchor - x <= overlap)));
            const uint64_t inmask = __builtin_amdgcn_ballot_w64(in);
            const uint64_t brk = vmask & ~inmask & (~0ull << pos);
            const uint32_t stop = brk ? (uint32_t)__builtin_ctzll(brk) : 64u;
            const bool member = in && lane < stop;
            const uint32_t mx = wave_umax(member ? ord : 0u);
            const uint64_t top = __builtin_amdgcn_ballot_w64(member && ord == mx);
            if (top && mx >= best_ord) {  // later elements win ties: this chunk's members come after the carried ones
                best_ord = mx;
                best_idx = (uint32_t)(base - b) + (63u - (uint32_t)__builtin_clzll(top));
            }
            if constexpr (RUNNERS) {
                members += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(member));
                if (top) {  // the chunk's part of the group: m1 its last maximum, m2 the last maximum of another letter
                    const int l1 = 63 - (int)__builtin_clzll(top);
                    const Top m1{mx, (uint32_t)(base - b) + (uint32_t)l1, (uint32_t)__builtin_amdgcn_readlane((int)let, l1),
                                 (uint32_t)__builtin_amdgcn_readlane((int)tt, l1), (uint32_t)__builtin_amdgcn_readlane(x, l1), true};
                    Top m2{};
                    const bool other = member && let != m1.letter;
                    if (__builtin_amdgcn_ballot_w64(other)) {
                        const uint32_t mx2 = wave_umax(other ? ord : 0u);
                        const int l2 = 63 - (int)__builtin_clzll(__builtin_amdgcn_ballot_w64(other && ord == mx2));
                        m2 = Top{mx2, (uint32_t)(base - b) + (uint32_t)l2, (uint32_t)__builtin_amdgcn_readlane((int)let, l2),
                                 (uint32_t)__builtin_amdgcn_readlane((int)tt, l2), (uint32_t)__builtin_amdgcn_readlane(x, l2), true};
                    }
                    Top lose = m1;
                    if (!a1.has || m1.ord >= a1.ord) lose = a1, a1 = m1;  // later elements win ties, as best_ord / best_idx
                    Top s{};
                    if (lose.has && lose.letter != a1.letter) s = lose;
                    if (a2.has && a2.letter != a1.letter && top_beats(s, a2)) s = a2;
                    if (m2.has && m2.letter != a1.letter && top_beats(s, m2)) s = m2;
                    a2 = s;
                }
            }
            if (stop < 64) {  // the group closes inside this chunk
                if constexpr (RUNNERS) {
                    if (lane == 0) store_runner(ra, slot0 + groups, members, a2);
                } else {
                    if (lane == 0) choice[b + groups] = (uint32_t)b + best_idx;
                }
                groups++;
                open = false;
            }
            pos = stop;
        }
    }
    if (open) {  // the row ends with a group still open
        if constexpr (RUNNERS) {
            if (lane == 0) store_runner(ra, slot0 + groups, members, a2);
        } else {
            if (lane == 0) choice[b + groups] = (uint32_t)b + best_idx;
        }
        groups++;
    }
    if constexpr (!RUNNERS)
        if (lane == 0) row_groups[wave] = ((uint64_t)1 << 32) | groups;
    }  // anchored rows of this wave
}

constexpr auto walk_lines = walk_kernel<false>;    // process_hits' walk
constexpr auto walk_runners = walk_kernel<true, RunnerArgs>;   // focr_get_runners' walk over what process_hits left resident

// one thread per hit slot: slot i of a row is the row's (i - line_b)-th output character if the row has that many groups
__global__ void emit_chars(const uint64_t *__restrict__ keys, const float *__restrict__ sims, const uint64_t *__restrict__ n_p, uint64_t ub, KeyFmt fmt, uint32_t r_h,
                           const uint8_t *__restrict__ keep_row, const uint32_t *__restrict__ line_b,
                           const uint32_t *__restrict__ choice, const uint64_t *__restrict__ row_groups,
                           const uint64_t *__restrict__ scanned, const uint32_t *__restrict__ t_w,
                           const uint32_t *__restrict__ t_h, const uint32_t *__restrict__ t_letter,
                           uint64_t *__restrict__ line_char_off, focr_hit_t *__restrict__ chars) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= min(*n_p, ub)) return;
    const uint64_t ki = keys[i];
    const size_t row = (size_t)fmt.page(ki) * r_h + fmt.y(ki);
    if (!keep_row[row]) return;
    const uint32_t k = (uint32_t)i - line_b[row];
    if (k >= (uint32_t)row_groups[row]) return;
    const uint64_t sc = scanned[row];
    const uint64_t off = (sc & 0xffffffffu) + k;
    if (k == 0) line_char_off[sc >> 32] = sc & 0xffffffffu;
    const uint32_t e = choice[i];
    const uint64_t key = keys[e];
    const uint32_t t = fmt.t(key);
    focr_hit_t h;
    h.x = (uint16_t)fmt.x(key);
    h.y = (uint16_t)fmt.y(key);
    h.w = (uint16_t)t_w[t];
    h.h = (uint16_t)t_h[t];
    h.similarity = sims[e];
    h.letter = t_letter[t];
    h.template_index = t;
    chars[off] = h;
}

// page_line_off[p] = number of kept lines on pages < p = the row scan at the page's first row
__global__ void page_offsets(const uint64_t *__restrict__ scanned, uint32_t r_h, uint32_t n_pages, uint64_t *__restrict__ page_line_off) {
    uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n_pages) return;
    page_line_off[p] = scanned[(size_t)min(p, n_pages) * r_h] >> 32;  // p == n_pages: the scan's grand total
}

// the batch's characters to a caller's device buffer, queued behind process_hits on the context's stream: their number is still
// on the device (the low word of the row scan's grand total), so the copy is a kernel that reads it there
__global__ __launch_bounds__(256) void copy_chars_kernel(const uint32_t *__restrict__ src, const uint64_t *__restrict__ total, uint32_t *__restrict__ dst, uint64_t dst_dwords) {
    constexpr uint64_t DW = sizeof(focr_hit_t) / 4;
    const uint64_t n = min((*total & 0xffffffffull) * DW, dst_dwords);  // a buffer that is too small is reported when the batch is completed
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

// Queue the copy of the last focr_process_hits' characters into dst (device memory, dst_bytes) on the context's stream; false if
// there is nothing queued to copy from (no hits at all / results already final): the caller copies after completion instead.
bool post_queue_chars_copy(focr_ctx *c, void *dst, size_t dst_bytes) {
    static_assert(sizeof(focr_hit_t) % 4 == 0, "focr_hit_t is copied as dwords");
    if (!c->post_pending || !c->post_scanned.p || !c->post_chars.p || !dst) return false;
    const size_t n_rows_total = c->n_pages * c->pages.r_h;
    hipLaunchKernelGGL(copy_chars_kernel, dim3(64), dim3(256), 0, c->stream, (const uint32_t *)c->post_chars.p, (const uint64_t *)c->post_scanned.p + n_rows_total,
                       (uint32_t *)dst, (uint64_t)(dst_bytes / 4));
    return hipGetLastError() == hipSuccess;
}

}  // namespace focr

using namespace focr;

extern "C" {

int focr_process_hits(focr_ctx_t *c, float anchor_threshold, int32_t overlap) {
    if (!c) return FOCR_ERR_INVALID;
    if (!c->scanned) return fail(c, FOCR_ERR_STATE, "focr_process_hits: no scan results");
    FOCR_HIP(c, hipSetDevice(c->device));
    c->post_starts();
    c->post_anchor = anchor_threshold;
    c->post_overlap = overlap;
    // all hits in (page, y, x, t) order; d_keep marks the ones that survive their call's cap.  Their number lives on the
    // device (c->d_n_hits); `ub` is what the scan sized its buffers for (the exact count unless the scan ran on estimates)
    const size_t ub = c->ub_hits, n_pages = c->n_pages;
    if (!c->sizes_pending && (c->n_hits == 0 || c->n_matches == 0)) {  // the reference panics on an empty hit list (src/ncc.rs:1040); we return zero lines
        c->processed = true;
        c->ms[MS_POST] = 0.f;
        return FOCR_OK;
    }
    if (ub >= 0xffffffffull) return fail(c, FOCR_ERR_OVERFLOW, "focr_process_hits: more than 2^32 hits in one batch");
    FOCR_HIP(c, hipEventRecord(c->ev[EV_POST_BEGIN], c->stream));
    // grow-only device scratch (no allocation in the steady state); outputs are sized by their bounds: characters <= hits,
    // lines <= page rows
    const size_t n_rows_total = n_pages * c->pages.r_h;
    if (!c->scratch(c->post_keep, n_rows_total + 8) || !c->scratch(c->post_choice, ub + 1) || !c->scratch(c->post_packed, n_rows_total + 1) ||
        !c->scratch(c->post_scanned, n_rows_total + 1) || !c->scratch(c->post_page_off, n_pages + 1) || !c->scratch(c->post_line_be, 2 * n_rows_total) ||
        !c->scratch(c->post_line_off, n_rows_total + 1) || !c->scratch(c->post_chars, ub + 1))
        return fail(c, FOCR_ERR_NOMEM, "focr_process_hits: hipMalloc failed");
    uint8_t *keep_row = c->post_keep;
    uint32_t *choice = c->post_choice, *line_b = c->post_line_be, *line_e = line_b + n_rows_total;
    uint64_t *packed = c->post_packed, *scanned = c->post_scanned;  // packed: per row, 1<<32 | groups
    uint64_t *d_page_off = c->post_page_off, *d_line_off = c->post_line_off;
    focr_hit_t *d_chars = c->post_chars;
    const uint8_t *keep = c->ord_keep;
    {
        ClearList clear{};  // one launch instead of two memsets (common.h)
        if (!clear.add(keep_row, n_rows_total)) return fail(c, FOCR_ERR_INVALID, "focr_process_hits: clear list full or region too large");
        if (!clear.add(packed, (n_rows_total + 1) * 8)) return fail(c, FOCR_ERR_INVALID, "focr_process_hits: clear list full or region too large");
        if (int rc = launch_clear(c, clear)) return rc;
    }
    const unsigned nb = (unsigned)((ub + 255) / 256);
    if (ub)
        hipLaunchKernelGGL(mark_anchor_rows, dim3(nb), dim3(256), 0, c->stream, c->d_hkeys, c->d_hsims, keep, c->d_n_hits, (uint64_t)ub, c->fmt,
                           anchor_threshold, (uint32_t)c->pages.r_h, keep_row, line_b, line_e);
    hipLaunchKernelGGL(walk_lines, dim3((unsigned)(((n_rows_total + WALK_ROWS - 1) / WALK_ROWS * 64 + 255) / 256)), dim3(256), 0, c->stream, c->d_hkeys, c->d_hsims,
                       keep, c->fmt, (uint32_t)n_rows_total, overlap, keep_row, line_b, line_e, choice, packed);
    int rc;
    if ((rc = exclusive_scan_u64(c, packed, scanned, n_rows_total + 1))) return rc;
    // packed[n_rows_total] = 0, so the scan's last entry is the grand total (lines << 32 | characters): into the result block
    FOCR_HIP(c, hipMemcpyAsync(&c->h_res->lines_chars, scanned + n_rows_total, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (ub)
        hipLaunchKernelGGL(emit_chars, dim3(nb), dim3(256), 0, c->stream, c->d_hkeys, c->d_hsims, c->d_n_hits, (uint64_t)ub, c->fmt, (uint32_t)c->pages.r_h,
                           keep_row, line_b, choice, packed, scanned, c->bank.d_t_w, c->bank.d_t_h, c->bank.d_t_letter, d_line_off, d_chars);
    hipLaunchKernelGGL(page_offsets, dim3((unsigned)((n_pages + 1 + 255) / 256)), dim3(256), 0, c->stream, scanned, (uint32_t)c->pages.r_h,
                       (uint32_t)n_pages, d_page_off);
    FOCR_HIP(c, hipGetLastError());
    FOCR_HIP(c, hipEventRecord(c->ev[EV_POST_END], c->stream));
    c->post_pending = true;
    c->processed = true;
    if (!c->sizes_pending) return finish_results(c);  // exact sizes: complete now, as the call always did
    return FOCR_OK;
}

// results stay in HBM until somebody asks for them
static int fetch_lines(focr_ctx *c) {
    int rc0 = finish_results(c);
    if (rc0) return rc0;
    if (c->lines_on_host) return FOCR_OK;
    c->h_page_line_off.assign(c->n_pages + 1, 0);
    c->h_line_char_off.assign(c->n_lines + 1, 0);
    c->h_chars.resize(c->n_chars);
    if (c->n_matches && (c->n_lines || c->n_chars)) {
        FOCR_HIP(c, hipSetDevice(c->device));
        if (c->n_lines)
            FOCR_HIP(c, hipMemcpyAsync(c->h_line_char_off.data(), c->post_line_off.p, c->n_lines * 8, hipMemcpyDeviceToHost, c->io_stream));
        FOCR_HIP(c, hipMemcpyAsync(c->h_page_line_off.data(), c->post_page_off.p, (c->n_pages + 1) * 8, hipMemcpyDeviceToHost, c->io_stream));
        if (c->n_chars)
            FOCR_HIP(c, hipMemcpyAsync(c->h_chars.data(), c->post_chars.p, c->n_chars * sizeof(focr_hit_t), hipMemcpyDeviceToHost, c->io_stream));
        FOCR_HIP(c, hipStreamSynchronize(c->io_stream));
    }
    c->h_line_char_off[c->n_lines] = c->n_chars;
    c->lines_on_host = true;
    return FOCR_OK;
}

size_t focr_total_chars(focr_ctx_t *c) { return (c && c->processed && finish_results(c) == FOCR_OK) ? c->n_chars : 0; }
size_t focr_total_lines(focr_ctx_t *c) { return (c && c->processed && finish_results(c) == FOCR_OK) ? c->n_lines : 0; }

int focr_get_lines(focr_ctx_t *c, uint64_t *page_line_offsets, uint64_t *line_char_offsets, focr_hit_t *chars) {
    if (!c) return FOCR_ERR_INVALID;
    if (!c->processed) return fail(c, FOCR_ERR_STATE, "focr_get_lines: call focr_process_hits first");
    int rc = fetch_lines(c);
    if (rc) return rc;
    if (page_line_offsets) memcpy(page_line_offsets, c->h_page_line_off.data(), c->h_page_line_off.size() * 8);
    if (line_char_offsets) memcpy(line_char_offsets, c->h_line_char_off.data(), c->h_line_char_off.size() * 8);
    if (chars && c->n_chars) memcpy(chars, c->h_chars.data(), c->n_chars * sizeof(focr_hit_t));
    return FOCR_OK;
}

// Same as focr_get_lines but straight from the device into the caller's buffers (page-locked ones make it a plain DMA)
int focr_get_lines_into(focr_ctx_t *c, uint64_t *page_line_offsets, uint64_t *line_char_offsets, focr_hit_t *chars) {
    if (!c || !page_line_offsets || !line_char_offsets || !chars) return FOCR_ERR_INVALID;
    if (!c->processed) return fail(c, FOCR_ERR_STATE, "focr_get_lines_into: call focr_process_hits first");
    int rc = finish_results(c);
    if (rc) return rc;
    FOCR_HIP(c, hipSetDevice(c->device));
    if (c->n_matches && (c->n_lines || c->n_chars)) {
        if (c->n_lines) FOCR_HIP(c, hipMemcpyAsync(line_char_offsets, c->post_line_off.p, c->n_lines * 8, hipMemcpyDeviceToHost, c->io_stream));
        FOCR_HIP(c, hipMemcpyAsync(page_line_offsets, c->post_page_off.p, (c->n_pages + 1) * 8, hipMemcpyDeviceToHost, c->io_stream));
        if (c->n_chars) FOCR_HIP(c, hipMemcpyAsync(chars, c->post_chars.p, c->n_chars * sizeof(focr_hit_t), hipMemcpyDeviceToHost, c->io_stream));
        FOCR_HIP(c, hipStreamSynchronize(c->io_stream));
    } else {
        for (size_t p = 0; p <= c->n_pages; p++) page_line_offsets[p] = 0;
    }
    line_char_offsets[c->n_lines] = c->n_chars;
    return FOCR_OK;
}

const focr_hit_t *focr_lines_device_chars(focr_ctx_t *c) {
    return (c && c->processed && finish_results(c) == FOCR_OK && c->n_chars) ? (const focr_hit_t *)c->post_chars.p : nullptr;
}

// The walk once more over what focr_process_hits left in place (nothing between it and the context's next scan writes any of it:
// the lazy match lists read the hits and write d_matches, focr_verify_images reads post_chars and writes its own buffers, the
// getters copy): one launch on the stream finished results are read on, its counts taken from device memory.
int focr_get_runners(focr_ctx_t *c, focr_runner_t *out) {
    if (!c) return FOCR_ERR_INVALID;
    c->run_ms = 0.f;
    c->run_launches = 0;
    if (!c->scanned || !c->processed) return fail(c, FOCR_ERR_STATE, "focr_get_runners: call focr_process_hits first (after the last scan)");
    if (int rc = finish_results(c)) return rc;  // the batch's own event inside an executor; a redo on exact sizes runs process_hits again
    const size_t n_chars = c->n_chars;
    if (!n_chars) return FOCR_OK;  // process_hits may not have run a kernel at all (no hits): its tables are not read
    if (!out) return fail(c, FOCR_ERR_INVALID, "focr_get_runners: no output buffer");
    FOCR_HIP(c, hipSetDevice(c->device));
    const hipStream_t s = c->io_stream;
    if (!c->runners_valid) {
        const size_t bound = c->ub_hits + 1, n_rows_total = c->n_pages * c->pages.r_h;  // characters <= hits, as post_chars
        if (bound >= 0xffffffffull) return fail(c, FOCR_ERR_OVERFLOW, "focr_get_runners: more than 2^32 hits in one batch");
        if (c->post_runners.reserve(bound, Grow::quarter, nullptr) != hipSuccess) return fail(c, FOCR_ERR_NOMEM, "focr_get_runners: hipMalloc failed");
        FOCR_HIP(c, hipEventRecord(c->run_ev[0], s));
        hipLaunchKernelGGL(walk_runners, dim3((unsigned)(((n_rows_total + WALK_ROWS - 1) / WALK_ROWS * 64 + 255) / 256)), dim3(256), 0, s, (const uint64_t *)c->d_hkeys,
                           (const float *)c->d_hsims, (const uint8_t *)c->ord_keep.p, c->fmt, (uint32_t)n_rows_total, c->post_overlap, (const uint8_t *)c->post_keep.p,
                           (const uint32_t *)c->post_line_be.p, (const uint32_t *)c->post_line_be.p + n_rows_total, (uint32_t *)nullptr, (uint64_t *)nullptr,
                           RunnerArgs{c->bank.d_t_letter.p, c->post_scanned.p, c->post_runners.p, (uint32_t)bound});
        FOCR_HIP(c, hipGetLastError());
        FOCR_HIP(c, hipEventRecord(c->run_ev[1], s));
    }
    FOCR_HIP(c, hipMemcpyAsync(out, c->post_runners.p, n_chars * sizeof(focr_runner_t), hipMemcpyDeviceToHost, s));
    FOCR_HIP(c, hipStreamSynchronize(s));
    if (!c->runners_valid) {
        FOCR_HIP(c, hipEventElapsedTime(&c->run_ms, c->run_ev[0], c->run_ev[1]));
        c->run_launches = 1;
        c->runners_valid = true;
    }
    return FOCR_OK;
}

int focr_last_runners(focr_ctx_t *c, float *ms, uint32_t *launches) {
    if (!c) return FOCR_ERR_INVALID;
    if (ms) *ms = c->run_ms;
    if (launches) *launches = c->run_launches;
    return FOCR_OK;
}

// Test hook: the caller's hits where a scan leaves them for focr_process_hits — keys packed with the batch's KeyFmt, similarities
// and keep flags in the buffers a split scan installs (scan_split, results.hip), the count on the device in the result block's host_hits.
int focr_debug_process_hits(focr_ctx_t *c, const uint32_t *page, const uint32_t *y, const uint32_t *x, const uint32_t *t,
                            const float *similarity, const uint8_t *keep, size_t n) {
    if (!c) return FOCR_ERR_INVALID;
    if (n && (!page || !y || !x || !t || !similarity || !keep)) return fail(c, FOCR_ERR_INVALID, "focr_debug_process_hits: bad arguments");
    if (!c->n_templates || !c->pages.u8) return fail(c, FOCR_ERR_STATE, "focr_debug_process_hits: upload a bank and allocate pages first");
    if (n >= 0xffffffffull) return fail(c, FOCR_ERR_OVERFLOW, "focr_debug_process_hits: more than 2^32 hits in one batch");
    const KeyFmt fmt = key_format(c->n_templates, c->pages.r_w, c->pages.r_h, c->n_pages);
    std::vector<uint64_t> keys(n);
    std::vector<uint8_t> kept(n);
    size_t n_kept = 0;
    for (size_t i = 0; i < n; i++) {
        if (page[i] >= c->n_pages || y[i] >= c->pages.r_h || x[i] >= c->pages.r_w || t[i] >= c->n_templates)
            return fail(c, FOCR_ERR_INVALID, "focr_debug_process_hits: hit " + std::to_string(i) + " lies outside the pages or the bank");
        keys[i] = fmt.pack(page[i], y[i], x[i], t[i]);
        if (i && keys[i] <= keys[i - 1])
            return fail(c, FOCR_ERR_INVALID, "focr_debug_process_hits: hit " + std::to_string(i) + " does not follow its predecessor in (page, y, x, t)");
        kept[i] = keep[i] != 0;
        n_kept += kept[i];
    }
    if (int rc = finish_results(c)) return rc;  // whatever an earlier call queued is done before its buffers are overwritten
    FOCR_HIP(c, hipSetDevice(c->device));
    if (!c->scratch(c->acc_hkeys, n + 1) || !c->scratch(c->acc_hsims, n + 1) || !c->scratch(c->ord_keep, n + 1))
        return fail(c, FOCR_ERR_NOMEM, "focr_debug_process_hits: hipMalloc failed");
    uint64_t *d_keys = c->acc_hkeys;
    float *d_sims = c->acc_hsims;
    uint8_t *d_keep = c->ord_keep;
    if (n) {
        FOCR_HIP(c, hipMemcpyAsync(d_keys, keys.data(), n * 8, hipMemcpyHostToDevice, c->stream));
        FOCR_HIP(c, hipMemcpyAsync(d_sims, similarity, n * 4, hipMemcpyHostToDevice, c->stream));
        FOCR_HIP(c, hipMemcpyAsync(d_keep, kept.data(), n, hipMemcpyHostToDevice, c->stream));
    }
    if (int rc = install_host_hits(c, n)) return rc;
    FOCR_HIP(c, hipStreamSynchronize(c->stream));
    c->fmt = fmt;
    c->d_hkeys = d_keys;
    c->d_hsims = d_sims;
    c->n_hits = c->n_hits_raw = n;
    c->n_matches = n_kept;
    c->sub_p0 = 0;
    c->sub_np = c->n_pages;
    c->estimated = false;
    c->debug_hits_installed();  // no per-call lists stand behind these hits
    return FOCR_OK;
}

}  // extern "C"
