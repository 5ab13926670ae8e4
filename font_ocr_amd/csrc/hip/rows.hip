// rows.hip — the hits-first row tail of the MFMA scan: candidates -> sorted, verified hits, without a global sort.
//
// The prefilter leaves an unordered list of candidate keys (page, y, x, t).  The reference's order (process_hits order:
// page, y, x, template; src/ncc.rs:741-752) used to be restored by a 5-pass radix sort of all candidates, followed by the
// exact verify, a flag scan and a compaction (12 launches, ~0.5 ms alone on the chip at BASELINE configs[1]: the legacy tail,
// still in scan_mfma.hip for banks this file does not cover).  But four candidates in ten fall to the verify, the verify needs
// no sorted input — it needs neighbouring lanes on neighbouring windows, and the scan kernels' flush order has that: the 64 keys
// of a flush are 64 adjacent windows of one page row — and a hit's (page, y) is one of only sub_np * r_h page rows (92 160 at
// configs[1]).  So the candidates are verified where they lie and only the HITS are bucketed by page row — by a segment of 2^k
// pixels of a page row where rows are wide and banks large (row_segments below; "row" in the names of this file means such a
// bucket) — and sorted per bucket:
//
//   verify_list       (verify.hip) the reference arithmetic on every candidate in FLUSH order (verify_candidate_*, verify.h), template rows
//   / verify_chunks   and records from LDS (in chunk passes for banks above it); a hit takes the next free slot of its bucket (one
//                     returning atomic per distinct bucket among the wave's hits) — similarity + slot in place; the kernel's last
//                     workgroup turns the buckets' hit counts into their dense positions, the hit total and the largest bucket
//   hit_scatter       hit -> hbase[bucket] + slot: the dense (key, similarity) arrays in bucket order, arbitrary inside a bucket
//   row_sort          one WAVE per bucket, keys with their similarities, in place: <= 64 keys ranked in registers by lane-to-lane
//                     comparison; else the sub-keys (x, t) in registers, counting sort by x in wave-private LDS, rank inside the
//                     x-bin by t.  Buckets above 1024 go onto a list and through a second launch (capacity 4096) -> (page, y, x, t)
//                     order: what order.hip takes over
//
// Three launches (+ the second capacity class of the sort where such a bucket is expected), no counting in the scan kernels' flush
// path, every pass behind the verify touches hits only.  A bucket above 4096 hits (very low thresholds): the placed hits go
// through the library radix sort; banks with templates taller than 32 px or more than 4096 templates: the legacy tail.  Exact
// mode knows the largest bucket before it chooses; estimated mode goes by the previous scan's, and a bucket that turns out too
// large sets the overflow bit: the batch is redone with exact sizes.  (Round 3's row tail — candidates bucketed, sorted, verified,
// compacted: seven launches — was kept for A/B through round 4; its last commit is 5ed8d3e.)
#include "common.h"

namespace focr {

// Sort every row's candidates by (x, t) — the low bt + bx bits of the key, unique inside a row — in place.  One WAVE per row
// (fixed stride: dense text rows are spread evenly over the waves), wave-private LDS, no workgroup barrier: the row's
// sub-keys come into LDS with all loads in flight at once, then a counting sort by x-bin (bin = x >> xs, at most XBINS bins:
// one x per bin for pages up to 1024 px wide) — count, exclusive prefix, place — and every element finds its rank among the
// few elements of its own bin and goes straight back to the row's slots in global memory.  O(n) LDS operations per row.
//   LIST = false: all rows; a row above CAP goes onto `big` (BASELINE configs[1]: one or two rows per batch exceed 1024).
//   LIST = true : the rows on `big`, with a larger CAP and one wave per workgroup; a row above that CAP sets the overflow bit
//                 (batch redone through the legacy tail).
constexpr uint32_t XBINS = 1024;
//   PAY: every key carries a float (the hits-first tail sorts verified hits with their similarities): loaded with the keys,
//        stored at the key's new place; `limit` = entries the arrays hold (a bucket that would reach past it is left alone: the
//        hit count exceeded its estimate and the batch is redone, record_scan_sizes).
template <int CAP, int WAVES, bool LIST, bool PAY>
__global__ __launch_bounds__(WAVES * 64) void row_sort_kernel(uint32_t n_rows, const uint32_t *__restrict__ base, const uint32_t *__restrict__ fill,
                                                              uint64_t *__restrict__ bucket, uint32_t sub_bits, uint32_t bt, uint32_t seg_mask, uint32_t xs, uint32_t n_bins,
                                                              uint32_t *__restrict__ big, unsigned long long *__restrict__ flags_word, float *__restrict__ pay,
                                                              unsigned long long limit) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sort_lds[];  // per wave: XBINS + 1 bin starts, CAP placed sub-keys
    constexpr int K = CAP / 64;  // sub-keys per lane, in registers
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t *cur = sort_lds + (size_t)wv * (XBINS + 1 + CAP);  // cur[n_bins] = n after the prefix
    uint32_t *out = cur + XBINS + 1;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * WAVES + wv), n_waves = gridDim.x * WAVES;
    const uint64_t sub_mask = (1ull << sub_bits) - 1;
    const uint32_t n_items = LIST ? min(big[0], n_rows) : n_rows;  // the list has room for every row
    // the next row's size and position are fetched (scalar loads) while the current row is sorted
    uint32_t it = wave, r = 0, n = 0, b = 0;
    if (it < n_items) {
        r = LIST ? big[1 + it] : it;
        n = fill[r];
        b = base[r];
    }
    while (it < n_items) {
        const uint32_t it2 = it + n_waves;
        uint32_t r2 = 0, n2 = 0, b2 = 0;
        if (it2 < n_items) {
            r2 = LIST ? big[1 + it2] : it2;
            n2 = fill[r2];
            b2 = base[r2];
        }
        if (PAY && (unsigned long long)b + n > limit) {
            // past the arrays' end (estimated sizes too small): nothing to sort, the batch is redone
        } else if (n > (uint32_t)CAP) {
            if (lane == 0) {
                if (LIST || !big) {  // beyond the last capacity class, or no second launch was planned for this batch (estimated sizes): redo
                    atomicOr(flags_word, RES_FLAG_ROW);
                } else {
                    big[1 + atomicAdd(big, 1u)] = r;  // room for every row
                }
            }
        } else if (n >= 2 && n <= 64 && !LIST) {
            // a row that fits one key per lane (most rows that are not text lines): rank by comparing with every other lane's key
            // — no LDS, no bins; keys are unique, so the rank is the key's place
            uint64_t *row = bucket + b;
            const uint64_t key = row[(uint32_t)lane < n ? lane : n - 1];
            float pv = 0.f;
            if (PAY) pv = pay[b + ((uint32_t)lane < n ? lane : n - 1)];
            const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32);
            uint32_t rank = 0;
            for (uint32_t j = 0; j < n; j++) {  // j is wave-uniform: v_readlane
                const uint64_t other = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)khi, (int)j) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)klo, (int)j);
                rank += other < key;
            }
            if ((uint32_t)lane < n) {
                row[rank] = key;
                if (PAY) pay[b + rank] = pv;
            }
        } else if (n >= 2) {
            uint64_t *row = bucket + b;
            uint32_t sub[K], slot[K];
            uint64_t key[K];
            float pv[PAY ? K : 1];
#pragma unroll
            for (int k = 0; k < K; k++) {  // all of the row's loads in flight at once: nothing but loads in this loop
                const uint32_t j = (uint32_t)lane + 64u * k;
                key[k] = 0;
                if (PAY) pv[k] = 0.f;
                if (64u * k < n) {  // wave-uniform branch; lanes past the end re-read the last key
                    key[k] = row[j < n ? j : n - 1];
                    if (PAY) pv[k] = pay[b + (j < n ? j : n - 1)];
                }
            }
#pragma unroll
            for (int k = 0; k < K; k++) sub[k] = (uint32_t)(key[k] & sub_mask);
            const uint32_t hi32 = (uint32_t)(key[0] >> 32), lo32 = (uint32_t)key[0];
            // (page, y) of the row from lane 0's first key (n >= 2: it has one)
            const uint64_t high = (((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(hi32) << 32) | (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane(lo32)) & ~sub_mask;  // the builtin returns int: no sign extension
            for (uint32_t i = lane; i <= n_bins; i += 64) cur[i] = 0;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
            for (int k = 0; k < K; k++)  // count per x-bin; the returned value is the element's slot inside its bin
                if (64u * k < n && (uint32_t)lane + 64u * k < n) slot[k] = atomicAdd(&cur[((sub[k] >> bt) & seg_mask) >> xs], 1u);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            uint32_t carry = 0;  // exclusive prefix over the bins, 64 at a time; cur[n_bins] = n
            for (uint32_t i0 = 0; i0 <= n_bins; i0 += 64) {
                const uint32_t i = i0 + lane, v = i < n_bins ? cur[i] : 0;
                uint32_t incl = v;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t u = __shfl_up(incl, o);
                    if (lane >= o) incl += u;
                }
                if (i <= n_bins) cur[i] = carry + incl - v;
                carry += __shfl(incl, 63);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
            for (int k = 0; k < K; k++)
                if (64u * k < n && (uint32_t)lane + 64u * k < n) out[cur[((sub[k] >> bt) & seg_mask) >> xs] + slot[k]] = sub[k];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
            for (int k = 0; k < K; k++)
                if (64u * k < n && (uint32_t)lane + 64u * k < n) {  // rank among the few elements of the same bin
                    const uint32_t e = sub[k], bin = ((e >> bt) & seg_mask) >> xs, lo = cur[bin], hi = cur[bin + 1];
                    uint32_t rank = 0;
                    for (uint32_t i = lo; i < hi; i++) rank += out[i] < e;
                    row[lo + rank] = high | e;
                    if (PAY) pay[b + lo + rank] = pv[k];
                }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the next row reuses the LDS buffers
        }
        it = it2, r = r2, n = n2, b = b2;
    }
}

// hit -> its dense place: hbase[bucket] + slot (no atomics: the slots were handed out by the verify)
__global__ __launch_bounds__(256) void hit_scatter_kernel(const uint64_t *__restrict__ cand, const unsigned long long *__restrict__ n_cand_p, unsigned long long cap,
                                                          const RowHist rows, const uint32_t *__restrict__ hbase, const float *__restrict__ sims,
                                                          const uint32_t *__restrict__ slots, uint64_t *__restrict__ hkeys, float *__restrict__ hsims,
                                                          unsigned long long hit_cap) {
    const unsigned long long n = min(*n_cand_p, cap);
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t slot = slots[i];
        if (slot == 0xffffffffu) continue;
        const uint64_t key = cand[i];
        const unsigned long long pos = (unsigned long long)hbase[row_of_key(key, rows)] + slot;
        if (pos < hit_cap) {  // estimated sizes: a hit count above its bound is flagged by record_scan_sizes and the batch redone
            hkeys[pos] = key;
            hsims[pos] = sims[i];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side

// x-segments per page row: a bucket should hold what one wave sorts in registers (<= 1024 candidates; up to 4096 go through
// the second, slower launch).  Candidates per row grow with the row's windows x templates: the first scan of a setup takes one
// segment per <= 2^19 of them (BASELINE configs[1]: 608 x 380 -> one segment, a row or two per batch just above 1024;
// configs[2]: 1200 x 1520 -> 5 segments of 256 px), later scans halve the segments while the largest bucket stays above 2048
// (results.hip, SizeEstimate::update: configs[2] settles at 128 px).  The segmentation never changes a result.
void row_segments(const focr_ctx *c, uint32_t *seg_shift, uint32_t *n_seg) {
    uint32_t sh = c->est.seg_shift;
    if (!sh) {
        while (((size_t)1 << sh) < c->pages.r_w) sh++;  // one segment
        while (sh > 5 && ((size_t)1 << sh) * c->n_templates > ((size_t)1 << 19)) sh--;
    }
    *seg_shift = sh;
    *n_seg = (uint32_t)((c->pages.r_w + ((size_t)1 << sh) - 1) >> sh);
}

size_t row_buckets(const focr_ctx *c) {
    uint32_t sh, ns;
    row_segments(c, &sh, &ns);
    return c->sub_np * c->pages.r_h * ns;
}

bool rows_applicable(const focr_ctx *c) {
    if (c->tail_mode == 0) return false;  // focr_ctx_set_row_tail(0): the legacy tail, for A/B
    for (const SizeClass &sc : c->bank.classes)
        if (sc.tall) return false;  // scan_tall_kernel appends its candidates without counting them per bucket
    return row_buckets(c) <= ((size_t)1 << 22) && c->fmt.bp + c->fmt.by <= 32 && c->n_templates <= 4096;  // 4096 x 32 B of template records in the verify's LDS
}

// hits-first tail, before the scan kernels: zeroed hit counters per bucket; the scan kernels count nothing (row_hist.cnt = null)
int rows2_begin(focr_ctx *c, ClearList &clear) {
    const size_t n_rows = row_buckets(c);
    const size_t padded = (n_rows + 1 + 3) / 4 * 4 + 4;  // row_prefix_block (tail_block.h) moves 16 bytes at a time
    if (!c->scratch(c->rows_hits, padded) || !c->scratch(c->rows_hbase, padded) || !c->scratch(c->rows_big, n_rows + 1 + 2))  // big[0]: length of the list of large buckets
        return fail(c, FOCR_ERR_NOMEM, "rows: hipMalloc failed");
    uint32_t *hits = c->rows_hits, *big = c->rows_big;
    if (!clear.add(hits, padded * 4)) return fail(c, FOCR_ERR_INVALID, "rows: clear list full or region too large");
    if (!clear.add(big, 8)) return fail(c, FOCR_ERR_INVALID, "rows: clear list full or region too large");
    uint32_t seg_shift, n_seg;
    row_segments(c, &seg_shift, &n_seg);
    c->row_hist = RowHist{nullptr, (uint32_t)c->pages.r_h, c->fmt.bt + c->fmt.bx, c->fmt.by, (uint32_t)c->sub_p0, c->fmt.bt, c->fmt.bx, seg_shift, n_seg};
    return FOCR_OK;
}

uint32_t rows_capacity_for(uint64_t row_max) { return row_max <= 4096 ? 4096u : 0u; }  // rows above 1024 take the second sort launch

// test hook (focr_debug_set_tail_grid): the persistent tail kernels' grids scaled by num / den — results must not depend on a grid
unsigned tail_grid(const focr_ctx *c, unsigned blocks) {
    if (!c->dbg_grid_num || !c->dbg_grid_den) return blocks;
    return (unsigned)std::max<uint64_t>(1, (uint64_t)blocks * c->dbg_grid_num / c->dbg_grid_den);
}


// hits-first tail, phase 2: hits to their buckets, every bucket sorted with its similarities -> the dense sorted hits in
// d_hit_keys / d_hit_sims_alt (their number: the result block's tail_hits).  ub_h: bound on the hits (exact sizes: the count itself).
int rows2_place(focr_ctx *c, const unsigned long long *n_cand_p, size_t ub_c, size_t ub_h, bool big_expected, bool sort) {
    const uint32_t n_rows = (uint32_t)row_buckets(c);
    int rc;
    if ((rc = reserve_hits(c, ub_h + 1))) return rc;
    const unsigned cus = c->n_cus;
    const uint32_t *hits = (const uint32_t *)c->rows_hits.p, *hbase = (const uint32_t *)c->rows_hbase.p;
    if (ub_c) {
        const unsigned nb = tail_grid(c, (unsigned)std::max<size_t>(1, std::min<size_t>((ub_c + 255) / 256, (size_t)cus * 16)));
        hipLaunchKernelGGL(hit_scatter_kernel, dim3(nb), dim3(256), 0, c->stream, (const uint64_t *)c->d_cand, n_cand_p, (unsigned long long)ub_c, c->row_hist, hbase,
                           (const float *)c->scan_pos.p, (const uint32_t *)c->scan_flags.p, c->d_hit_keys, c->d_hit_sims_alt, (unsigned long long)c->d_hit_keys.cap);
        FOCR_HIP(c, hipGetLastError());
    }
    if (!sort) return FOCR_OK;  // a bucket beyond the row sort's capacity (exact sizes know): the caller sorts the placed hits with the library sort
    unsigned long long *flags_word = (unsigned long long *)&c->d_res.p->flags;
    const unsigned row_blocks = tail_grid(c, (unsigned)std::max<size_t>(1, std::min<size_t>(((size_t)n_rows + 3) / 4, (size_t)cus * 8)));
    const uint32_t seg_w = 1u << c->row_hist.seg_shift;
    uint32_t xs = 0;
    while ((seg_w >> xs) > XBINS) xs++;
    const uint32_t n_bins = seg_w >> xs;
    uint32_t *big = (uint32_t *)c->rows_big.p;  // allocated and zeroed in rows2_begin
    auto k1 = row_sort_kernel<1024, 4, false, true>;
    auto k2 = row_sort_kernel<4096, 1, true, true>;
    const size_t lds1 = (size_t)4 * (XBINS + 1 + 1024) * 4, lds2 = (size_t)(XBINS + 1 + 4096) * 4;
    hipLaunchKernelGGL(k1, dim3(row_blocks), dim3(256), lds1, c->stream, n_rows, hbase, hits, c->d_hit_keys, c->fmt.bt + c->fmt.bx, c->fmt.bt, seg_w - 1, xs, n_bins,
                       big_expected ? big : (uint32_t *)nullptr, flags_word, c->d_hit_sims_alt, (unsigned long long)c->d_hit_keys.cap);
    FOCR_HIP(c, hipGetLastError());
    // Buckets above 1 024 hits (the list `big`) get a second launch only where one is expected: exact sizes know the largest bucket,
    // estimated sizes go by the previous scan's (+ 25 %).  Without the launch a bucket that lands on the list after all is an
    // overflow like any other estimate that proved too small (flag bit 1: the batch is redone with exact sizes) — even a launch of
    // ONE wave that finds the list empty stood 110 us in a lane's chain of kernels (it needs 20 KB of LDS on a CU the other
    // batches' kernels keep full: profiles/r04_timeline_bench_c2.log), for a list that BASELINE configs[1] and [2] never fill.
    if (big_expected) {
        hipLaunchKernelGGL(k2, dim3(cus), dim3(64), lds2, c->stream, n_rows, hbase, hits, c->d_hit_keys, c->fmt.bt + c->fmt.bx, c->fmt.bt, seg_w - 1, xs, n_bins, big, flags_word,
                           c->d_hit_sims_alt, (unsigned long long)c->d_hit_keys.cap);
        FOCR_HIP(c, hipGetLastError());
    }
    return FOCR_OK;
}

}  // namespace focr
