// verify.h — the exact verify of one candidate: the reference arithmetic, operation for operation (common.h), on the device.
//
// ONE FRAME.  Every form does the same four things around its row loop, and each is stated once here: the candidate frame (key ->
// bounds check -> page pointer), the keep mask of a window's own bytes, the f64 epilogue (sums -> similarity, emit) and, in the row
// tail's kernels, the slot claim (hit -> its place in its bucket).  A form is its row loop and where its template rows and records
// come from:
//   verify_candidate            records by order_of -> tc -> needle16_row, rows of 16 bytes from global memory (verify_kernel: the legacy tail)
//   verify_candidate_meta<LDS>  records from `meta`, rows of 16 bytes from LDS or global memory, 16 page rows in flight
//   verify_candidate_narrow     records from `meta`, rows of 12 bytes from LDS, 8 page rows in flight
//   verify_candidate_w89        banks of 8- and 9-wide templates of one height: rows of 8 bytes, the ninth column packed
// The frame does not decide WHEN a form reads the template's record: verify_candidate_w89 reads it in two parts, on purpose.
#pragma once
#include "common.h"

namespace focr {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef v4i v4i_b1 __attribute__((aligned(1)));  // byte-aligned 16-byte view (gfx950 global loads take any alignment)
typedef int v3i __attribute__((ext_vector_type(3)));
typedef v3i v3i_b1 __attribute__((aligned(1)));
typedef unsigned int v2u __attribute__((ext_vector_type(2)));

// Everything the verify needs to know about a template, by GLOBAL template index, 32 bytes: one LDS read instead of three
// dependent gathers from global memory (order_of -> TemplateConst -> needle16_row).
struct VerifyMeta {
    double s_n, n_recip, rnorm_n;
    uint16_t n_w, n_h;
    uint32_t row0;  // first row of the template in needles16
};
static_assert(sizeof(VerifyMeta) == 32, "VerifyMeta is staged in LDS as two 16-byte words per template (verify_plan.h: VERIFY_RECORD_BYTES)");
struct VerifyArgs {
    const uint8_t *pages;
    uint32_t pitch, rows_alloc;
    KeyFmt fmt;
    const uint32_t *order_of;        // global template index -> class-ordered index
    const TemplateConst *tc;         // class-ordered
    const v4i *needles16;            // every template as n_h rows of 16 bytes (zero padded; two halves per row above 16 px)
    const uint32_t *needle16_row;    // class-ordered first row
    double thr_d;
    const struct VerifyMeta *vmeta;           // by global template index (the row tail's verify stages it in LDS)
    uint32_t n_templates, n_pages, r_w, r_h;  // bounds of a well-formed key
    unsigned long long *flags_word;           // the result block's flags: RES_FLAG_KEY = a key outside those bounds was met (internal error, never a fault)
};

// ---- the frame ----

// The candidate of a key: its fields.  `bad`: the key lies outside the batch's bounds (cannot happen; verifying it would be a wild read)
// — the form then returns verify_reject: RES_FLAG_KEY is set, the similarity written as 0, no emit.
struct VerifyFrame {
    uint32_t page, t, x, y;
    bool bad;
    // the window's first byte: rows have >= 64 readable bytes past r_w, every page 48 readable rows below it
    __device__ __forceinline__ const uint8_t *window(const VerifyArgs &va) const { return va.pages + ((size_t)page * va.rows_alloc + y) * va.pitch + x; }
};
__device__ __forceinline__ VerifyFrame verify_frame(uint64_t key, const VerifyArgs &va) {
    const uint32_t page = va.fmt.page(key), t = va.fmt.t(key), x = va.fmt.x(key), y = va.fmt.y(key);
    return VerifyFrame{page, t, x, y, t >= va.n_templates || page >= va.n_pages || x >= va.r_w || y >= va.r_h};
}
__device__ __forceinline__ bool verify_reject(const VerifyArgs &va, float *sim_out) {
    atomicOr(va.flags_word, RES_FLAG_KEY);
    *sim_out = 0.f;
    return false;
}

// byte mask of a w-wide window's own columns in dword k of its rows (the padded template columns are zero, but s_p / s2_p need the mask)
__device__ __forceinline__ uint32_t keep_mask(uint32_t w, int k) {
    return w >= (uint32_t)(4 * k + 4) ? 0xffffffffu : (w <= (uint32_t)(4 * k) ? 0u : ((1u << (8 * (w - 4 * k))) - 1u));
}

// the f64 epilogue: the window's sums and the template's record (s_n, n_recip, rnorm_n, n_w, n_h: a TemplateConst or a VerifyMeta, by
// value) -> the f32 similarity, "emits"
template <class Record>
__device__ __forceinline__ bool verify_epilogue(uint32_t acc, uint32_t s_p, uint32_t s2_p, const Record c, double thr_d, float *sim_out) {
    const double rnorm_p = window_rnorm(s_p, (uint64_t)s2_p, (double)((uint32_t)c.n_w * c.n_h));
    const double sim = ncc_similarity(acc, s_p, c.s_n, c.n_recip, c.rnorm_n, rnorm_p);
    *sim_out = (float)sim;
    return ncc_emits(sim, thr_d);
}

// A hit's slot inside its bucket, ~0 for a lane without a hit: the wave's 64 candidates come from a handful of page rows, and the claim
// costs one returning atomic per distinct bucket among the wave's hits.  Called by the whole wave.
__device__ __forceinline__ uint32_t claim_slot(bool emit, uint64_t key, const RowHist &rows, uint32_t *row_hits, int lane) {
    const uint32_t r = emit ? row_of_key(key, rows) : 0xffffffffu;
    uint32_t slot = 0xffffffffu;
    uint64_t todo = __builtin_amdgcn_ballot_w64(emit);
    while (todo) {
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r, (int)__builtin_ctzll(todo));
        const uint64_t peers = __builtin_amdgcn_ballot_w64(r == r0);
        uint32_t start = 0;
        if (lane == (int)__builtin_ctzll(peers)) start = atomicAdd(row_hits + r0, (uint32_t)__builtin_popcountll(peers));
        start = (uint32_t)__builtin_amdgcn_readlane((int)start, (int)__builtin_ctzll(peers));
        if (r == r0) slot = start + __builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
        todo &= ~peers;
    }
    return slot;
}

// ---- the forms: each its row loop ----

// The legacy tail's: the record through three dependent gathers, template rows of 16 bytes from global memory (two 16-byte halves per
// row for the 17..32-wide extension), one page row at a time.
__device__ __forceinline__ bool verify_candidate(uint64_t key, const VerifyArgs &va, float *sim_out) {
    const VerifyFrame f = verify_frame(key, va);
    if (f.bad) return verify_reject(va, sim_out);
    const uint32_t ci = va.order_of[f.t];
    const TemplateConst c = va.tc[ci];
    const uint32_t halves = c.n_w > 16 ? 2 : 1;
    const uint32_t row0 = va.needle16_row[ci];
    const v4i *nd = va.needles16 + row0;
    const uint8_t *pg = f.window(va);
    uint32_t acc = 0, s_p = 0, s2_p = 0;
    for (uint32_t hf = 0; hf < halves; hf++) {
        const uint32_t w_here = min(c.n_w - 16 * hf, 16u);
        v4i keep;
#pragma unroll
        for (int k = 0; k < 4; k++) keep[k] = (int)keep_mask(w_here, k);
#pragma unroll 8
        for (uint32_t j = 0; j < c.n_h; j++) {
            const v4i a = *reinterpret_cast<const v4i_b1 *>(pg + (size_t)j * va.pitch + 16 * hf) & keep;
            const v4i b = nd[j * halves + hf];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                acc = __builtin_amdgcn_udot4((uint32_t)a[k], (uint32_t)b[k], acc, false);     // src/ncc.cpp:316-321
                s_p = __builtin_amdgcn_udot4((uint32_t)a[k], 0x01010101u, s_p, false);        // patch_sum, src/ncc.rs:307
                s2_p = __builtin_amdgcn_udot4((uint32_t)a[k], (uint32_t)a[k], s2_p, false);   // sum of squares, src/ncc.rs:308
            }
        }
    }
    return verify_epilogue(acc, s_p, s2_p, c, va.thr_d, sim_out);
}

// The row tail's 16-byte form: the record from `meta` (by global template index: the LDS copy of va.vmeta, or of a chunk's records),
// template rows from LDS at `lds` (LDS = true: indexed like needles16) or from global memory — a compile-time choice, so that every
// template-row load is a plain ds_read or a plain global load, never a per-lane choice between address spaces.  Same arithmetic,
// same order of operations.
template <bool LDS>
__device__ __forceinline__ bool verify_candidate_meta(uint64_t key, const VerifyArgs &va, const v4i *lds, const VerifyMeta *meta, float *sim_out) {
    const VerifyFrame f = verify_frame(key, va);
    if (f.bad) return verify_reject(va, sim_out);
    const VerifyMeta c = meta[f.t];
    const uint32_t halves = c.n_w > 16 ? 2 : 1;
    const v4i *nd = va.needles16 + c.row0;
    const uint8_t *pg = f.window(va);
    uint32_t acc = 0, s_p = 0, s2_p = 0;
    for (uint32_t hf = 0; hf < halves; hf++) {
        const uint32_t w_here = min((uint32_t)c.n_w - 16 * hf, 16u);
        v4i keep;
#pragma unroll
        for (int k = 0; k < 4; k++) keep[k] = (int)keep_mask(w_here, k);
        // 16 page rows in flight at once (the kernel waits on memory four fifths of its time: one round trip per 16 rows, not
        // two); rows past n_h are read but not accumulated
        for (uint32_t j0 = 0; j0 < c.n_h; j0 += 16) {
            v4i a[16];
#pragma unroll
            for (int jj = 0; jj < 16; jj++) a[jj] = *reinterpret_cast<const v4i_b1 *>(pg + (size_t)(j0 + jj) * va.pitch + 16 * hf);
#pragma unroll
            for (int jj = 0; jj < 16; jj++) {
                const uint32_t j = j0 + jj;
                if (j < c.n_h) {
                    const v4i aw = a[jj] & keep;
                    v4i b;
                    if (LDS) b = lds[c.row0 + j * halves + hf];
                    else b = nd[j * halves + hf];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        acc = __builtin_amdgcn_udot4((uint32_t)aw[k], (uint32_t)b[k], acc, false);    // src/ncc.cpp:316-321
                        s_p = __builtin_amdgcn_udot4((uint32_t)aw[k], 0x01010101u, s_p, false);       // patch_sum, src/ncc.rs:307
                        s2_p = __builtin_amdgcn_udot4((uint32_t)aw[k], (uint32_t)aw[k], s2_p, false);  // sum of squares, src/ncc.rs:308
                    }
                }
            }
        }
    }
    return verify_epilogue(acc, s_p, s2_p, c, va.thr_d, sim_out);
}

// The same for banks whose templates are all at most 12 px wide: template rows of 12 bytes (three dwords) from LDS, page rows as
// 12-byte loads, eight in flight — half the LDS and half the registers of the 16-byte form, so that TWO 1 024-thread workgroups
// share a CU (verify_list_kernel<2>, verify.hip).  Same arithmetic, same order of operations.
__device__ __forceinline__ bool verify_candidate_narrow(uint64_t key, const VerifyArgs &va, const uint32_t *lds_rows, const VerifyMeta *meta, float *sim_out) {
    const VerifyFrame f = verify_frame(key, va);
    if (f.bad) return verify_reject(va, sim_out);
    const VerifyMeta c = meta[f.t];
    const uint8_t *pg = f.window(va);
    const uint32_t w = c.n_w;  // <= 12
    uint32_t keep[3];
#pragma unroll
    for (int k = 0; k < 3; k++) keep[k] = keep_mask(w, k);
    const uint32_t *nd = lds_rows + 3 * c.row0;
    uint32_t acc = 0, s_p = 0, s2_p = 0;
    for (uint32_t j0 = 0; j0 < c.n_h; j0 += 8) {  // rows past n_h are read but not accumulated
        v3i a[8];
#pragma unroll
        for (int jj = 0; jj < 8; jj++) a[jj] = *reinterpret_cast<const v3i_b1 *>(pg + (size_t)(j0 + jj) * va.pitch);
#pragma unroll
        for (int jj = 0; jj < 8; jj++) {
            const uint32_t j = j0 + jj;
            if (j < c.n_h) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const uint32_t aw = (uint32_t)a[jj][k] & keep[k], b = nd[3 * j + k];
                    acc = __builtin_amdgcn_udot4(aw, b, acc, false);             // src/ncc.cpp:316-321
                    s_p = __builtin_amdgcn_udot4(aw, 0x01010101u, s_p, false);   // patch_sum, src/ncc.rs:307
                    s2_p = __builtin_amdgcn_udot4(aw, aw, s2_p, false);          // sum of squares, src/ncc.rs:308
                }
            }
        }
    }
    return verify_epilogue(acc, s_p, s2_p, c, va.thr_d, sim_out);
}

// The same for banks of 8- and 9-wide templates of ONE height n_h <= 16 (BASELINE configs[1]: 95 templates of 8 x 15, 285 of 9 x 15),
// where the 12-byte form spends a third of its dot products on a dword that holds one byte or none: the window's first two dwords
// lie inside it whatever its width — no mask — and meet template rows of 8 bytes (`rows8`, indexed like needles16); the ninth
// column is gathered from the third dwords of the loaded page rows, four rows to a dword, and meets the template's ninth column
// packed the same way (`col9`: 16 bytes per template, by global index; zero for an 8-wide template and for rows past n_h).  The
// width never becomes a branch — a wave's 64 candidates mix both — it is folded into the byte selectors of the gather: an 8-wide
// template's lane selects the constant 0 for every byte, and so does every lane for a row at or past n_h, so that s_p and s2_p sum the
// window's own bytes only.  n_h is the bank's, hence wave-uniform: the row loop has a scalar trip count and no per-lane guard.
// acc, s_p, s2_p are sums of the same products as the other forms' — u32 without overflow (n_w * n_h * 255^2 < 2^32: verify_plan.h)
// — so their order does not matter, and the f64 epilogue is the same code: bit-identical results.
__device__ __forceinline__ bool verify_candidate_w89(uint64_t key, const VerifyArgs &va, const v2u *rows8, const v4i *col9, const VerifyMeta *meta, float *sim_out) {
    const VerifyFrame f = verify_frame(key, va);
    if (f.bad) return verify_reject(va, sim_out);
    // the record's doubles are read behind the rows (they would only hold registers until then); its n_h is the bank's: made a scalar HERE,
    // so that every row's "j < n_h" is a scalar compare where it is used (as a kernel argument the sixteen compares are hoisted out of the
    // kernel's loop as sixteen lane masks, more scalar registers than there are)
    const uint32_t t = f.t;
    const uint32_t n_w = meta[t].n_w, n_h = __builtin_amdgcn_readfirstlane((uint32_t)meta[t].n_h), row0 = meta[t].row0;
    const uint8_t *pg = f.window(va);
    const v2u *nd = rows8 + row0;
    const uint32_t *b9 = reinterpret_cast<const uint32_t *>(col9 + t);
    const bool wide = n_w > 8;
    uint32_t acc = 0, s_p = 0, s2_p = 0;
#pragma unroll
    for (int g = 0; g < 2; g++) {
        const uint32_t j0 = 8 * g;
        if (j0 < n_h) {  // wave-uniform; rows past n_h are read but not accumulated
            v3i a[8];
#pragma unroll
            for (int jj = 0; jj < 8; jj++) a[jj] = *reinterpret_cast<const v3i_b1 *>(pg + (size_t)(j0 + jj) * va.pitch);
#pragma unroll
            for (int jj = 0; jj < 8; jj++) {
                if (j0 + jj < n_h) {  // wave-uniform
                    const v2u b = nd[j0 + jj];
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const uint32_t aw = (uint32_t)a[jj][k];
                        acc = __builtin_amdgcn_udot4(aw, b[k], acc, false);          // src/ncc.cpp:316-321
                        s_p = __builtin_amdgcn_udot4(aw, 0x01010101u, s_p, false);   // patch_sum, src/ncc.rs:307
                        s2_p = __builtin_amdgcn_udot4(aw, aw, s2_p, false);          // sum of squares, src/ncc.rs:308
                    }
                }
            }
#pragma unroll
            for (int h = 0; h < 2; h++) {
                // byte 8 of rows j .. j + 3 -> one dword, three v_perm_b32 (selector 0 .. 3 = that byte of the second operand, 4 = byte 0 of
                // the first, 12 = the constant 0).  The last one's selector takes out the rows at or past n_h (scalar) and, per lane, the
                // whole dword for an 8-wide template.
                const uint32_t j = j0 + 4 * h;
                const uint32_t live = (j < n_h ? 0x00u : 0x0cu) | (j + 1 < n_h ? 0x0100u : 0x0c00u) | (j + 2 < n_h ? 0x020000u : 0x0c0000u) |
                                      (j + 3 < n_h ? 0x04000000u : 0x0c000000u);
                uint32_t p = __builtin_amdgcn_perm((uint32_t)a[4 * h + 1][2], (uint32_t)a[4 * h][2], 0x0c0c0400u);
                p = __builtin_amdgcn_perm((uint32_t)a[4 * h + 2][2], p, 0x0c040100u);
                p = __builtin_amdgcn_perm((uint32_t)a[4 * h + 3][2], p, wide ? live : 0x0c0c0c0cu);
                const uint32_t b = b9[2 * g + h];
                acc = __builtin_amdgcn_udot4(p, b, acc, false);
                s_p = __builtin_amdgcn_udot4(p, 0x01010101u, s_p, false);
                s2_p = __builtin_amdgcn_udot4(p, p, s2_p, false);
            }
        }
    }
    return verify_epilogue(acc, s_p, s2_p, meta[t], va.thr_d, sim_out);
}

}  // namespace focr
