// verify_plan_check.cpp — the host's choice of the exact verify's form (verify_plan.h) at the edges its arithmetic has, without a
// device: a stand-alone program, built with a host compiler under the sanitizers and run by tests/test_verify_plan_host.py.
// Every expected figure is worked out from the plan's constants here, not read back from it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "verify_plan.h"

using namespace focr;

struct Size {
    uint32_t n_w, n_h;
};
struct Bank {
    std::vector<Size> t;
    std::vector<uint32_t> vrow0;  // as bank_mfma.hip lays the chunk form's operand out: n_h rows per template, by template index
    uint32_t vrow_bytes = 0;
    void add(uint32_t count, uint32_t n_w, uint32_t n_h) {
        for (uint32_t i = 0; i < count; i++) t.push_back(Size{n_w, n_h});
    }
    VerifyPlan plan(int debug_form = 0) {
        uint32_t max_w = 0;
        for (const Size &s : t) max_w = std::max(max_w, s.n_w);
        vrow_bytes = max_w <= 12 ? 12u : max_w <= 16 ? 16u : 0u;
        vrow0.assign(t.size() + 1, 0);
        if (vrow_bytes)
            for (size_t i = 0; i < t.size(); i++) vrow0[i + 1] = vrow0[i] + t[i].n_h;
        return plan_verify(t, vrow_bytes, vrow0.data(), debug_form);
    }
};
static Bank bank(uint32_t count, uint32_t n_w, uint32_t n_h) {
    Bank b;
    b.add(count, n_w, n_h);
    return b;
}

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

// a whole-bank form: its LDS, the rows the kernel stages, workgroups per CU
static void check_list(const VerifyPlan &p, uint32_t form, size_t lds, uint32_t rows, uint32_t n_h, unsigned per_cu) {
    CHECK(p.form == form);
    CHECK(p.lds == lds);
    CHECK(p.rows == rows);
    CHECK(p.n_h == n_h);
    CHECK(p.per_cu == per_cu);
    CHECK(p.chunks.n == 0);
}

// the chunk form: the chunks tile the bank in order, each within the budget, data_bytes the largest one's
static void check_chunks(Bank &b, const VerifyPlan &p, uint32_t n_chunks) {
    const size_t queue = 16 * 128 * 12 + 64, budget = 150 * 1024 - queue;
    CHECK(p.form == FOCR_VERIFY_FORM_CHUNKS);
    CHECK(p.chunks.n == n_chunks);
    CHECK(p.per_cu == 1 && p.rows == 0 && p.n_h == 0);
    if (p.form != FOCR_VERIFY_FORM_CHUNKS || p.chunks.n > MAX_VERIFY_CHUNKS) return;
    CHECK(p.chunks.t_lo[0] == 0 && p.chunks.t_lo[p.chunks.n] == b.t.size());
    size_t largest = 0;
    for (uint32_t k = 0; k < p.chunks.n; k++) {
        const uint32_t lo = p.chunks.t_lo[k], hi = p.chunks.t_lo[k + 1];
        CHECK(lo < hi);
        CHECK(p.chunks.row_lo[k] == b.vrow0[lo] && p.chunks.row_lo[k + 1] == b.vrow0[hi]);
        const size_t bytes = (size_t)(hi - lo) * 32 + (size_t)(b.vrow0[hi] - b.vrow0[lo]) * b.vrow_bytes;
        CHECK(bytes <= budget);
        // greedy: the next template would not have fitted
        if (hi < b.t.size()) CHECK(bytes + 32 + (size_t)b.t[hi].n_h * b.vrow_bytes > budget);
        largest = std::max(largest, (bytes + 15) / 16 * 16);
    }
    CHECK(p.chunks.data_bytes == largest);
    CHECK(p.lds == largest + queue);
    CHECK(p.lds <= 150 * 1024);
}

int main() {
    const size_t half_cu = 80 * 1024 - 256, whole = 144 * 1024;
    {  // the last bank the 12-byte form takes: 196 x (32 + 32 x 12) = 81 536 <= 81 664 < 197 x 416
        Bank b = bank(196, 12, 32);
        CHECK(196 * 416 <= half_cu && 197 * 416 > half_cu);
        check_list(b.plan(), FOCR_VERIFY_FORM_LDS12, 196 * 416, 196 * 32, 0, 2);
        b = bank(197, 12, 32);
        check_list(b.plan(), FOCR_VERIFY_FORM_LDS16, 197 * (32 + 32 * 16), 197 * 32, 0, 1);
    }
    {  // the last bank the 16-byte form takes: 271 x 544 = 147 424 <= 147 456 < 272 x 544
        Bank b = bank(271, 16, 32);
        CHECK(271 * 544 <= whole && 272 * 544 > whole);
        check_list(b.plan(), FOCR_VERIFY_FORM_LDS16, 271 * 544, 271 * 32, 0, 1);
        b = bank(272, 16, 32);
        const VerifyPlan p = b.plan();
        check_chunks(b, p, 2);  // 237 x 544 = 128 928 <= 128 960 < 238 x 544
        CHECK(p.chunks.t_lo[1] == 237 && p.chunks.t_lo[2] == 272);
        CHECK(b.vrow_bytes == 16);
    }
    {  // the same count 12 wide: 12-byte rows, 272 x 416 = 113 152 in one chunk
        Bank b = bank(272, 12, 32);
        const VerifyPlan p = b.plan();
        check_chunks(b, p, 1);
        CHECK(b.vrow_bytes == 12 && p.chunks.data_bytes == 272 * 416);
    }
    {  // 16 chunks of 237 templates are the most: one template more and the rows come from global memory
        Bank b = bank(16 * 237, 16, 32);
        check_chunks(b, b.plan(), 16);
        b = bank(16 * 237 + 1, 16, 32);
        check_list(b.plan(), FOCR_VERIFY_FORM_GLOBAL, 3793 * 32, 0, 0, 1);  // 121 376 B of records: above 64 KiB, one workgroup per CU
        check_list(verify_plan_global(2048), FOCR_VERIFY_FORM_GLOBAL, 2048 * 32, 0, 0, 2);
        check_list(verify_plan_global(2049), FOCR_VERIFY_FORM_GLOBAL, 2049 * 32, 0, 0, 1);
    }
    {  // BASELINE configs[1]: 95 of 8 x 15 and 285 of 9 x 15 -> 8-byte rows, the ninth columns packed
        Bank b;
        b.add(95, 8, 15);
        b.add(285, 9, 15);
        check_list(b.plan(), FOCR_VERIFY_FORM_LDS8, 380 * (32 + 16 + 15 * 8), 380 * 15, 15, 2);
        check_list(b.plan(1), FOCR_VERIFY_FORM_LDS12, 380 * (32 + 15 * 12), 380 * 15, 0, 2);  // the test hook
        // no ninth column anywhere, two heights, a narrower or a wider template, a height above 16: the 12-byte form
        check_list(bank(95, 8, 15).plan(), FOCR_VERIFY_FORM_LDS12, 95 * (32 + 15 * 12), 95 * 15, 0, 2);
        Bank two = bank(10, 9, 15);
        two.add(1, 9, 14);
        CHECK(two.plan().form == FOCR_VERIFY_FORM_LDS12);
        Bank w7 = bank(10, 9, 15);
        w7.add(1, 7, 15);
        CHECK(w7.plan().form == FOCR_VERIFY_FORM_LDS12);
        Bank w10 = bank(10, 9, 15);
        w10.add(1, 10, 15);
        CHECK(w10.plan().form == FOCR_VERIFY_FORM_LDS12);
        CHECK(bank(10, 9, 16).plan().form == FOCR_VERIFY_FORM_LDS8);
        CHECK(bank(10, 9, 17).plan().form == FOCR_VERIFY_FORM_LDS12);
    }
    {  // many short templates, then tall ones: the two maxima (records, rows) come from different chunks; the LDS is the largest
       // single chunk's, not their sum (which a CU does not have)
        Bank b;
        b.add(1007, 8, 8);
        b.add(310, 12, 32);
        const VerifyPlan p = b.plan();
        check_chunks(b, p, 2);
        CHECK(p.chunks.t_lo[1] == 1007);
        CHECK(p.chunks.data_bytes == 310 * 416);                       // 128 960 (the short ones: 1007 x 128 = 128 896)
        CHECK((size_t)1007 * 32 + (size_t)310 * 32 * 12 > 150 * 1024 - (16 * 128 * 12 + 64));  // the sum of the two maxima would not fit
    }
    {  // templates wider than 16 (the row tail never sees one; the arithmetic is kept): two 16-byte halves per row, no chunk operand
        Bank wide = bank(400, 20, 32);
        const VerifyPlan p = wide.plan();
        CHECK(wide.vrow_bytes == 0 && p.form == FOCR_VERIFY_FORM_GLOBAL && p.per_cu == 2);
        check_list(bank(100, 20, 32).plan(), FOCR_VERIFY_FORM_LDS16, 100 * (32 + 64 * 16), 100 * 64, 0, 1);
    }
    if (failures) return 1;
    std::puts("verify plan ok");
    return 0;
}
