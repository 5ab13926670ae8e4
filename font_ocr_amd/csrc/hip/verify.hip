// verify.hip — the exact verify of the scan's candidates: its kernels and their host side.
//
// The arithmetic of one candidate, and the frame every form shares, is in verify.h; which form a bank takes is the host's plan
// (verify_plan.h: a pure function of the bank's sizes).  Here are the kernels that walk a candidate list — the row tail's
// verify_list_kernel (the bank's operand staged whole in LDS, or its rows read from global memory) and verify_chunks_kernel (banks
// above the LDS, in chunk passes), the legacy tail's verify_kernel — and rows2_verify, which launches what the plan says.  What
// happens to the hits afterwards (scatter, sort per bucket) is rows.hip's.
//
// The compiler's output for these kernels is sensitive to things that do not change a result: the prefix kernel standing in front of the
// verify kernels in this file, the epilogue taking the template's record by value (verify.h).  tools/isa_hash.py shows whether a
// clean-up kept the instruction streams (profiles/verify_split_isa.json: this file's against the files they came from).
#include "tail_block.h"
#include "verify.h"
#include "verify_plan.h"

namespace focr {

static VerifyArgs verify_args(const focr_ctx *c, double thr_d) {
    return VerifyArgs{c->pages.u8, (uint32_t)c->pages.pitch, (uint32_t)c->pages.rows_alloc, c->fmt, c->bank.d_order_of, c->bank.d_tconst,
                      c->bank.d_needles16.as<const v4i>(), c->bank.d_needle16_row, thr_d, c->bank.d_vmeta.p,
                      (uint32_t)c->n_templates, (uint32_t)c->n_pages,
                      (uint32_t)c->pages.r_w, (uint32_t)c->pages.r_h, (unsigned long long *)&c->d_res.p->flags};
}

// the prefix of the buckets' hit counts as a launch of its own (row_prefix_block, tail_block.h): for a scan without candidates, whose
// verify — the kernel whose last workgroup does it otherwise — is not launched (rows2_verify)
__global__ __launch_bounds__(1024) void row_prefix_kernel(const uint32_t *__restrict__ cnt, uint32_t n, uint32_t *__restrict__ base,
                                                          uint32_t *__restrict__ zero, uint64_t *__restrict__ total_out,
                                                          uint64_t *__restrict__ max_out) {
    __shared__ uint32_t wave_sum[16], wave_max[16];
    row_prefix_block(cnt, n, base, zero, total_out, max_out, wave_sum, wave_max);
}

// The exact verify of the candidate list in flush order.  A candidate costs 15 page-row loads (neighbouring lanes: neighbouring
// windows, a few cache lines per wave instruction) and 15 template-row loads — a 64-way GATHER per wave instruction when they come
// from global memory, which kept the texture addresser busy for most of the kernel's time (round 2: 0.22 ms for 3.8 M candidates).
// MODE 0: template rows from global memory · 1: the bank's verify operand staged in LDS once per workgroup, 16 bytes per row (all
// of it fits 144 KiB) · 2: 12 bytes per row (every template at most 12 px wide and the whole operand within half a CU's LDS): 64
// VGPRs, two workgroups per CU — the kernel waits on memory four fifths of its time, and in flight it has only the CUs the scan
// leaves free, so waves per CU are what it runs on · 3: banks of 8- and 9-wide templates of one height n_h (verify_candidate_w89,
// verify.h): 8 bytes per row and the ninth columns packed, 16 bytes per template; two workgroups per CU like MODE 2.
template <int MODE>
__global__ __launch_bounds__(VERIFY_THREADS, MODE >= 2 ? 8 : 1) void verify_list_kernel(
    const uint64_t *__restrict__ cand, const unsigned long long *__restrict__ n_cand_p, unsigned long long cap, const VerifyArgs va, uint32_t lds_rows, uint32_t n_h,
    const RowHist rows, float *__restrict__ sims, uint32_t *__restrict__ slots, uint32_t *__restrict__ row_hits, const TailWork tw) {
    // LDS: [template records: n_templates x 32 B][template rows, 16 B (MODE 1) or 12 B (MODE 2) each]
    //      MODE 3: [template records][ninth columns: n_templates x 16 B][template rows, 8 B each]
    extern __shared__ __attribute__((aligned(16))) v4i verify_lds[];
    __shared__ uint32_t wave_sum[16], wave_max[16];
    constexpr bool LDS = MODE == 1;
    VerifyMeta *meta = reinterpret_cast<VerifyMeta *>(verify_lds);
    v4i *needle_lds = verify_lds + 2 * va.n_templates;
    uint32_t *needle12 = reinterpret_cast<uint32_t *>(needle_lds);
    v2u *needle8 = reinterpret_cast<v2u *>(needle_lds + va.n_templates);
    for (uint32_t i = threadIdx.x; i < 2 * va.n_templates; i += blockDim.x) verify_lds[i] = reinterpret_cast<const v4i *>(va.vmeta)[i];
    if (MODE == 1)
        for (uint32_t i = threadIdx.x; i < lds_rows; i += blockDim.x) needle_lds[i] = va.needles16[i];
    if (MODE == 2)
        for (uint32_t i = threadIdx.x; i < lds_rows; i += blockDim.x) {
            const v4i r = va.needles16[i];
            needle12[3 * i] = (uint32_t)r[0], needle12[3 * i + 1] = (uint32_t)r[1], needle12[3 * i + 2] = (uint32_t)r[2];
        }
    if (MODE == 3) {
        for (uint32_t i = threadIdx.x; i < lds_rows; i += blockDim.x) {
            const v4i r = va.needles16[i];
            needle8[i] = v2u{(uint32_t)r[0], (uint32_t)r[1]};
        }
        // byte 8 of the template's rows 4q .. 4q + 3 -> dword q of its ninth column (rows at or past n_h: zero)
        for (uint32_t i = threadIdx.x; i < 4 * va.n_templates; i += blockDim.x) {
            const uint32_t t = i >> 2, q = i & 3, row0 = va.vmeta[t].row0;
            uint32_t d = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                if (4 * q + k < n_h) d |= ((uint32_t)va.needles16[row0 + 4 * q + k][2] & 0xffu) << (8 * k);
            reinterpret_cast<uint32_t *>(needle_lds)[i] = d;
        }
    }
    __syncthreads();
    const unsigned long long n = min(*n_cand_p, cap);
    const int lane = threadIdx.x & 63;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    const unsigned long long first = (unsigned long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63u);
    uint64_t key_next = first + lane < n ? cand[first + lane] : 0;  // the next step's key is loaded a step ahead
    for (unsigned long long i0 = first; i0 < n; i0 += stride) {  // wave-uniform trip count
        const unsigned long long i = i0 + lane;
        const bool valid = i < n;
        const uint64_t key = key_next;
        if (i + stride < n) key_next = cand[i + stride];
        float sim = 0.f;
        const bool emit = valid && (MODE == 3   ? verify_candidate_w89(key, va, needle8, needle_lds, meta, &sim)
                                    : MODE == 2 ? verify_candidate_narrow(key, va, needle12, meta, &sim)
                                                : verify_candidate_meta<LDS>(key, va, needle_lds, meta, &sim));
        const uint32_t slot = claim_slot(emit, key, rows, row_hits, lane);
        if (valid) {
            sims[i] = sim;
            slots[i] = slot;
        }
    }
    // the kernel's last workgroup turns the buckets' hit counts into their dense positions (+ the hit total and the largest bucket)
    if (last_workgroup(tw.done)) row_prefix_block(row_hits, tw.n_rows, tw.hbase, nullptr, tw.total_out, tw.max_out, wave_sum, wave_max);
}

// Banks whose verify operand does not fit the LDS whole (BASELINE configs[2]: 1 520 templates, 287 KB of 12-byte rows + 48 KB
// of records): the operand is cut into CHUNKS of consecutive templates (by global template index; d_vrows_t / d_vmeta_t are
// ordered that way) that do fit (ChunkTable, verify_plan.h), and the kernel makes one pass over its candidates per chunk — chunk
// rows and records staged in LDS, every wave walking its own piece of the list, collecting the keys whose template lies in the chunk
// in a wave-private queue in LDS and verifying them 64 at a time, so every verify step runs on full waves whatever the mix of
// templates in the list.  Reading the keys once more per chunk costs 8 B per candidate and pass, so chunks are as large as the LDS
// allows (one workgroup per CU: BASELINE configs[2] in 3 chunks 2.19 ms alone on the chip; 5 chunks of 80 KB 3.14 ms; the template
// rows gathered from global memory, verify_list_kernel<0>, 3.35 ms — a 64-way gather per wave instruction).
template <int ROWB>
__global__ __launch_bounds__(VERIFY_THREADS, 4) void verify_chunks_kernel(
    const uint64_t *__restrict__ cand, const unsigned long long *__restrict__ n_cand_p, unsigned long long cap, const VerifyArgs va, const ChunkTable ct,
    const uint32_t *__restrict__ vrows_t, const VerifyMeta *__restrict__ vmeta_t, const RowHist rows, float *__restrict__ sims, uint32_t *__restrict__ slots,
    uint32_t *__restrict__ row_hits, const TailWork tw) {
    // LDS: [the chunk's records: 32 B each][the chunk's rows: ROWB each] ... at data_bytes: [per wave: CHUNK_QUEUE keys][per wave: CHUNK_QUEUE list positions]
    extern __shared__ __attribute__((aligned(16))) v4i verify_lds[];
    __shared__ uint32_t wave_sum[16], wave_max[16];
    constexpr uint32_t ROWDW = ROWB / 4;
    VerifyMeta *meta = reinterpret_cast<VerifyMeta *>(verify_lds);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint64_t *q_base = reinterpret_cast<uint64_t *>(verify_lds + ct.data_bytes / 16);
    uint64_t *q_key = q_base + (size_t)wv * CHUNK_QUEUE;
    uint32_t *q_pos = reinterpret_cast<uint32_t *>(q_base + (size_t)(VERIFY_THREADS / 64) * CHUNK_QUEUE) + (size_t)wv * CHUNK_QUEUE;
    const unsigned long long n = min(*n_cand_p, cap);
    // the wave's own piece of the list: whole groups of 64
    const unsigned long long n_waves = (unsigned long long)gridDim.x * (VERIFY_THREADS / 64);
    const unsigned long long per_wave = ((n + n_waves - 1) / n_waves + 63) / 64 * 64;
    const unsigned long long wb = min(n, ((unsigned long long)blockIdx.x * (VERIFY_THREADS / 64) + wv) * per_wave), we = min(n, wb + per_wave);
    // one verify step over the first `m` queued candidates (m <= 64): the reference arithmetic, the hit's slot in its bucket
    auto step = [&](uint32_t m, const VerifyMeta *meta_c, const uint32_t *rows_c) {
        const bool valid = (uint32_t)lane < m;
        const uint64_t key = valid ? q_key[lane] : 0;
        const uint32_t pos = valid ? q_pos[lane] : 0;
        float sim = 0.f;
        bool emit = false;
        if (valid) {
            if (ROWB == 12) emit = verify_candidate_narrow(key, va, rows_c, meta_c, &sim);
            else emit = verify_candidate_meta<true>(key, va, reinterpret_cast<const v4i *>(rows_c), meta_c, &sim);
        }
        const uint32_t slot = claim_slot(emit, key, rows, row_hits, lane);
        if (valid && pos < n) {  // (pos comes out of the wave's own queue: always below n — the test costs nothing and a write never leaves the arrays)
            sims[pos] = sim;
            slots[pos] = slot;
        }
    };
    for (uint32_t k = 0; k < ct.n; k++) {
        const uint32_t t_lo = ct.t_lo[k], t_hi = ct.t_lo[k + 1], row_lo = ct.row_lo[k], n_rows_c = ct.row_lo[k + 1] - row_lo;
        uint32_t *rows_lds = reinterpret_cast<uint32_t *>(verify_lds + 2 * (t_hi - t_lo));  // behind THIS chunk's records
        __syncthreads();  // the previous chunk's readers are done
        for (uint32_t i = threadIdx.x; i < 2 * (t_hi - t_lo); i += VERIFY_THREADS) verify_lds[i] = reinterpret_cast<const v4i *>(vmeta_t + t_lo)[i];
        for (uint32_t i = threadIdx.x; i < n_rows_c * ROWDW; i += VERIFY_THREADS) rows_lds[i] = vrows_t[(size_t)row_lo * ROWDW + i];
        __syncthreads();
        // records by global template index and rows by their index in d_vrows_t, as the verify functions address them
        const VerifyMeta *meta_c = meta - t_lo;
        const uint32_t *rows_c = rows_lds - (size_t)row_lo * ROWDW;
        uint32_t count = 0;  // wave-uniform: queued candidates of this chunk
        for (unsigned long long i0 = wb; i0 < we; i0 += 4 * 64) {
            // four groups of keys per round, their loads in flight together (the walk is latency-bound otherwise: one round trip per group and pass)
            uint64_t key4[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const unsigned long long i = i0 + 64 * q + lane;
                key4[q] = i < we ? cand[i] : ~0ull;
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const unsigned long long i = i0 + 64 * q + lane;
                const bool valid = i < we;
                const uint64_t key = key4[q];
                const uint32_t t = va.fmt.t(key);
                // a template index outside the bank belongs to no chunk: such a key (cannot happen) is given to the last chunk, whose
                // verify flags it instead of leaving its outputs unwritten
                const bool in = valid && ((t >= t_lo && t < t_hi) || (k + 1 == ct.n && t >= t_hi));
                const uint64_t mask = __builtin_amdgcn_ballot_w64(in);
                if (mask) {
                    if (in) {
                        const uint32_t p = count + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                        q_key[p] = key;
                        q_pos[p] = (uint32_t)i;
                    }
                    count += (uint32_t)__builtin_popcountll(mask);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    if (count >= 64) {
                        step(64, meta_c, rows_c);
                        const uint32_t rest = count - 64;  // < 64: moves to the front of the queue
                        const uint64_t kk = (uint32_t)lane < rest ? q_key[64 + lane] : 0;
                        const uint32_t pp = (uint32_t)lane < rest ? q_pos[64 + lane] : 0;
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        if ((uint32_t)lane < rest) {
                            q_key[lane] = kk;
                            q_pos[lane] = pp;
                        }
                        count = rest;
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    }
                }
            }
        }
        if (count) step(count, meta_c, rows_c);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (last_workgroup(tw.done)) row_prefix_block(row_hits, tw.n_rows, tw.hbase, nullptr, tw.total_out, tw.max_out, wave_sum, wave_max);
}

// Legacy tail (scan_mfma.hip: the fallback of the row path): candidates arrive radix-sorted by the packed key (page, y, x, t):
// neighbouring lanes verify the same or neighbouring windows (cache-friendly), and the survivors stay in process_hits order,
// so no atomics: flag[i] / sim[i] are written in place and order.hip compacts them and derives the per-call lists.
__global__ __launch_bounds__(256) void verify_kernel(const uint64_t *__restrict__ cand, const unsigned long long *__restrict__ n_cand_p, unsigned long long ub,
                                                     const VerifyArgs va, float *__restrict__ sims, uint64_t *__restrict__ flags) {
    unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > ub) return;  // grid and buffers are sized for `ub` candidates (+ the sentinel at ub)
    if (i >= min(*n_cand_p, ub)) {  // past the device-side count (and the sentinel: the exclusive scan of flags also yields the total)
        flags[i] = 0;
        return;
    }
    float sim;
    const bool emit = verify_candidate(cand[i], va, &sim);
    sims[i] = sim;
    flags[i] = emit ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// host side

int legacy_verify(focr_ctx *c, double thr_d, const unsigned long long *n_cand_p, size_t ub_c, float *sims, uint64_t *flags) {
    hipLaunchKernelGGL(verify_kernel, dim3((unsigned)((ub_c + 1 + 255) / 256)), dim3(256), 0, c->stream, c->d_cand, n_cand_p, (unsigned long long)ub_c,
                       verify_args(c, thr_d), sims, flags);
    FOCR_HIP(c, hipGetLastError());
    return FOCR_OK;
}

// what every launch of the row tail's verify takes
struct VerifyLaunch {
    const unsigned long long *n_cand_p;
    size_t ub_c;
    VerifyArgs va;
    float *sims;
    uint32_t *slots, *hits;
    TailWork tw;
    unsigned blocks(const focr_ctx *c, size_t most) const {
        return tail_grid(c, (unsigned)std::max<size_t>(1, std::min<size_t>((ub_c + VERIFY_THREADS - 1) / VERIFY_THREADS, most)));
    }
};

// The chunk form, one workgroup per CU of the whole chip: at configs[2] the chunk passes are a fifth of a lane's chain, and the lane
// waits for them (half / a third / a quarter of the CUs: 7.25 / 7.21 / 7.12 Gpx/s against 7.28).  False: the device refuses that
// much LDS, nothing was launched.
template <int ROWB>
static bool launch_chunks_rowb(focr_ctx *c, const VerifyPlan &P, const VerifyLaunch &L) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(verify_chunks_kernel<ROWB>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    hipLaunchKernelGGL(verify_chunks_kernel<ROWB>, dim3(L.blocks(c, c->n_cus)), dim3(VERIFY_THREADS), P.lds, c->stream, (const uint64_t *)c->d_cand, L.n_cand_p,
                       (unsigned long long)L.ub_c, L.va, P.chunks, c->bank.d_vrows_t.as<const uint32_t>(), c->bank.d_vmeta_t.p, c->row_hist, L.sims, L.slots, L.hits, L.tw);
    return true;
}
static bool launch_chunks(focr_ctx *c, const VerifyPlan &P, const VerifyLaunch &L) {
    return c->bank.vrow_bytes == 12 ? launch_chunks_rowb<12>(c, P, L) : launch_chunks_rowb<16>(c, P, L);
}

template <int MODE>
static void launch_list_mode(focr_ctx *c, const VerifyPlan &P, const VerifyLaunch &L, unsigned nb) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(verify_list_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds);
    hipLaunchKernelGGL(verify_list_kernel<MODE>, dim3(nb), dim3(VERIFY_THREADS), P.lds, c->stream, (const uint64_t *)c->d_cand, L.n_cand_p, (unsigned long long)L.ub_c, L.va,
                       P.rows, P.n_h, c->row_hist, L.sims, L.slots, L.hits, L.tw);
}
// The whole-bank forms.  Their workgroups are persistent (they walk the list with the grid's stride), so where the scan kernel is
// confined to scan_cus CUs — several batches in flight — the verify asks for no more workgroups than fit the CUs the scan leaves
// free: a verify launched in the gap between two scan launches would otherwise put a workgroup on every CU of the chip and hold it
// until the kernel ends, and the next scan launch's workgroups wait for whole CUs (C2, three in flight, one box, alternating:
// 512 workgroups 32.55 Gpx/s · 64: 32.82 · 32: 31.2 with the scan launch at 1.57 instead of 1.68 ms, but the lane then waits
// for its verify) ...
// ... unless the host has said that nothing follows this batch (focr_pipe_announce_last / _end_of_stream) — nobody will scan behind it while its
// tail runs: then the tail takes the chip (the last batch of a run: a 20-step timed region ends 0.7-1.2 ms earlier)
static void launch_list(focr_ctx *c, const VerifyPlan &P, const VerifyLaunch &L) {
    const unsigned cus = c->n_cus;
    const unsigned vcus = (c->scan_cus && c->scan_cus < cus && !c->tail_full_chip) ? std::max(cus - c->scan_cus, cus / 16) : cus;
    const unsigned nb = L.blocks(c, (size_t)vcus * P.per_cu);
    switch (P.form) {
        case FOCR_VERIFY_FORM_LDS8: launch_list_mode<3>(c, P, L, nb); break;
        case FOCR_VERIFY_FORM_LDS12: launch_list_mode<2>(c, P, L, nb); break;
        case FOCR_VERIFY_FORM_LDS16: launch_list_mode<1>(c, P, L, nb); break;
        default: launch_list_mode<0>(c, P, L, nb); break;
    }
}

// hits-first tail, phase 1 (right behind the scan kernels): exact verify of the candidate list in flush order, hit counts and
// slots per bucket, prefix -> the result block's tail_hits and row_max (the largest bucket).  Records EV_VERIFY_END behind the verify.
int rows2_verify(focr_ctx *c, double thr_d, const unsigned long long *n_cand_p, size_t ub_c) {
    const uint32_t n_rows = (uint32_t)row_buckets(c);
    if (!c->scratch(c->scan_pos, (ub_c + 1) * 4) || !c->scratch(c->scan_flags, (ub_c + 1) * 4)) return fail(c, FOCR_ERR_NOMEM, "rows: hipMalloc failed");
    uint32_t *hits = c->rows_hits, *hbase = c->rows_hbase;
    if (ub_c) {
        VerifyPlan P = plan_verify(c->bank.h_tconst, c->bank.vrow_bytes, c->bank.h_vrow0_t.data(), c->dbg_verify_form);
        // the verify's last workgroup does the prefix
        const VerifyLaunch L{n_cand_p, ub_c, verify_args(c, thr_d), c->scan_pos.as<float>(), c->scan_flags.as<uint32_t>(), hits,
                             TailWork{c->d_counter + TAIL_DONE_WORD, n_rows, hbase, &c->d_res.p->tail_hits, &c->d_res.p->row_max}};
        if (P.form == FOCR_VERIFY_FORM_CHUNKS && !launch_chunks(c, P, L)) P = verify_plan_global(c->n_templates);  // the rows come from global memory instead
        if (P.form != FOCR_VERIFY_FORM_CHUNKS) launch_list(c, P, L);
        FOCR_HIP(c, hipGetLastError());
        c->tail_path.verify_form = P.form;
        c->tail_path.verify_chunks = P.chunks.n;
    }
    FOCR_HIP(c, hipEventRecord(c->ev[EV_VERIFY_END], c->stream));
    if (!ub_c) {  // no candidate can exist (nothing was verified): the prefix of all-zero counts, as a launch of its own
        hipLaunchKernelGGL(row_prefix_kernel, dim3(1), dim3(1024), 0, c->stream, (const uint32_t *)hits, n_rows, hbase, (uint32_t *)nullptr, &c->d_res.p->tail_hits, &c->d_res.p->row_max);
        FOCR_HIP(c, hipGetLastError());
    }
    return FOCR_OK;
}

}  // namespace focr
