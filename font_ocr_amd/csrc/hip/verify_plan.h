// verify_plan.h — the host's choice of the exact verify's form for a bank, as a pure function: which kernel (FOCR_VERIFY_FORM_*), how
// much LDS, how many workgroups per CU and, for the chunk form, which templates make a chunk.  Plain C++, no device types and no
// context: verify.hip launches what the plan says, verify_plan_check.cpp asserts the plan at the edges of its arithmetic with a host
// compiler alone.  The kernels and what each form costs: verify.hip.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "focr_ncc.h"

namespace focr {

constexpr unsigned VERIFY_THREADS = 1024;
constexpr uint32_t MAX_VERIFY_CHUNKS = 16, CHUNK_QUEUE = 128;
struct ChunkTable {
    uint32_t n;
    uint32_t t_lo[MAX_VERIFY_CHUNKS + 1];    // chunk k: templates [t_lo[k], t_lo[k + 1])
    uint32_t row_lo[MAX_VERIFY_CHUNKS + 1];  // ... rows [row_lo[k], row_lo[k + 1]) of d_vrows_t
    // LDS layout, per chunk: [its records: 32 B each][its rows]; behind the LARGEST chunk's data (data_bytes, a multiple of 16) the
    // waves' queues.  (Round 4 laid the rows out behind the largest chunk's RECORDS and sized the data for the largest record count
    // plus the largest row count — two maxima that can come from different chunks: a bank of many short templates followed by
    // tall ones asked for more LDS than a CU has although every chunk fitted.)
    uint32_t data_bytes;
};

constexpr size_t VERIFY_RECORD_BYTES = 32;                      // sizeof(VerifyMeta) (verify.h asserts it)
constexpr size_t VERIFY_LDS_HALF_CU = ((size_t)80 << 10) - 256;  // two workgroups per CU: the 12- and the 8-byte form
constexpr size_t VERIFY_LDS_WHOLE = (size_t)144 << 10;           // one workgroup per CU: the 16-byte form
constexpr size_t VERIFY_LDS_CHUNKS = (size_t)150 << 10;          // one workgroup per CU: fewer, larger chunks beat more waves per CU (verify.hip)
constexpr size_t VERIFY_QUEUE_BYTES = (size_t)(VERIFY_THREADS / 64) * CHUNK_QUEUE * 12 + 64;  // per wave CHUNK_QUEUE keys (8 B) and list positions (4 B)
constexpr size_t VERIFY_GLOBAL_PAIR_RECORDS = (size_t)64 << 10;  // the global form: two workgroups per CU while the records alone stay within this

struct VerifyPlan {
    uint32_t form;    // FOCR_VERIFY_FORM_*
    size_t lds;       // dynamic LDS of the launch
    uint32_t rows;    // template rows the list kernel stages (0: the global form stages none)
    uint32_t n_h;     // the bank's one height (the 8-byte form), else 0
    unsigned per_cu;  // workgroups per CU the grid is sized for
    ChunkTable chunks;  // FOCR_VERIFY_FORM_CHUNKS only
};

// template rows from global memory, the records alone in LDS: what is left when nothing else fits, or when the device refuses the
// chunk form its LDS
inline VerifyPlan verify_plan_global(size_t n_templates) {
    const size_t meta_bytes = n_templates * VERIFY_RECORD_BYTES;
    return VerifyPlan{FOCR_VERIFY_FORM_GLOBAL, meta_bytes, 0, 0, meta_bytes <= VERIFY_GLOBAL_PAIR_RECORDS ? 2u : 1u, ChunkTable{}};
}

// The plan for a bank.  `templates`: any range of records with n_w and n_h, one per template (at most 4096 here: 128 KiB of
// records), in any order; vrow_bytes, vrow0_t: the row size (12, 16, or 0: none) and the n + 1 row offsets, by global template
// index, of the operand the chunk form reads (bank_mfma.hip); debug_form: focr_debug_set_verify_form.
template <class Templates>
VerifyPlan plan_verify(const Templates &templates, uint32_t vrow_bytes, const uint32_t *vrow0_t, int debug_form) {
    size_t all_rows = 0, n_templates = 0;
    uint32_t max_w = 0, min_w = ~0u, h_lo = ~0u, h_hi = 0;
    for (const auto &tc : templates) {
        n_templates++;
        all_rows += (size_t)tc.n_h * (tc.n_w > 16 ? 2u : 1u);
        max_w = std::max<uint32_t>(max_w, tc.n_w);
        min_w = std::min<uint32_t>(min_w, tc.n_w);
        h_lo = std::min<uint32_t>(h_lo, tc.n_h);
        h_hi = std::max<uint32_t>(h_hi, tc.n_h);
    }
    const size_t meta_bytes = n_templates * VERIFY_RECORD_BYTES;
    // the 8-byte form (verify_candidate_w89): every template 8 or 9 px wide — with a ninth column somewhere: a bank of 8-wide templates alone
    // wants 8-byte page loads and no ninth-column stage, a form of its own (not built) — and of one height of at most 16 rows (two groups of
    // eight page rows).  Its sums are u32 like the other forms': 9 * 16 * 255^2 < 2^24.  debug_form 1: the 12-byte form for such a bank too.
    const size_t w89_bytes = meta_bytes + n_templates * 16 + all_rows * 8;
    if (min_w >= 8 && max_w == 9 && h_lo == h_hi && h_hi <= 16 && (uint64_t)max_w * h_hi * 255 * 255 <= 0xffffffffull && w89_bytes <= VERIFY_LDS_HALF_CU &&
        debug_form == 0)
        return VerifyPlan{FOCR_VERIFY_FORM_LDS8, w89_bytes, (uint32_t)all_rows, h_hi, 2, ChunkTable{}};
    if (max_w <= 12 && meta_bytes + all_rows * 12 <= VERIFY_LDS_HALF_CU)
        return VerifyPlan{FOCR_VERIFY_FORM_LDS12, meta_bytes + all_rows * 12, (uint32_t)all_rows, 0, 2, ChunkTable{}};
    if (meta_bytes + all_rows * 16 <= VERIFY_LDS_WHOLE) return VerifyPlan{FOCR_VERIFY_FORM_LDS16, meta_bytes + all_rows * 16, (uint32_t)all_rows, 0, 1, ChunkTable{}};
    if (!vrow_bytes) return verify_plan_global(n_templates);
    // the operand does not fit the LDS whole: chunks of consecutive templates that do (verify_chunks_kernel)
    const size_t budget = VERIFY_LDS_CHUNKS - VERIFY_QUEUE_BYTES;
    ChunkTable ct{};
    size_t bytes = 0;
    uint32_t t0 = 0;
    for (uint32_t t = 0; t <= n_templates; t++) {
        const size_t add = t < n_templates ? VERIFY_RECORD_BYTES + (size_t)(vrow0_t[t + 1] - vrow0_t[t]) * vrow_bytes : 0;
        if (t == n_templates || bytes + add > budget) {
            if (t == t0 || ct.n == MAX_VERIFY_CHUNKS) return verify_plan_global(n_templates);  // a single template above the budget, or too many chunks
            ct.t_lo[ct.n] = t0;
            ct.row_lo[ct.n] = vrow0_t[t0];
            ct.data_bytes = std::max(ct.data_bytes, (uint32_t)((bytes + 15) & ~(size_t)15));  // this chunk's records + rows (bytes <= budget)
            ct.n++;
            t0 = t;
            bytes = 0;
        }
        bytes += add;
    }
    ct.t_lo[ct.n] = (uint32_t)n_templates;
    ct.row_lo[ct.n] = vrow0_t[n_templates];
    // <= VERIFY_LDS_CHUNKS by construction: every chunk's data is within the budget.  One workgroup per CU of the whole chip.
    return VerifyPlan{FOCR_VERIFY_FORM_CHUNKS, (size_t)ct.data_bytes + VERIFY_QUEUE_BYTES, 0, 0, 1, ct};
}

}  // namespace focr
