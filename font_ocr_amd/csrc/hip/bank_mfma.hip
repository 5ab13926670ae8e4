// bank_mfma.hip — the MFMA prefilter's bank: K layouts and super-classes, the int8 quantisation, the verify operands, and a
// scan's threshold parameters per size class.  Host code only; what the statistics and scan kernels read is built here.
//
// Every template is mean-centred, scaled by a class-wide constant c/norm_n(t) and rounded
// to int8 with the rounding chosen so that sum_k bq_k = 0.  G(w,t) = sum_k (a_k - 128) bq_k  (= sum_k a_k bq_k) is one
// v_mfma_i32_16x16x64_i8 chain over the window's bytes (16 templates x 16 windows, K = 64 bytes per instruction) with
// C-in = plane value << log2(S), so "D > 0" <=> G > L(w) rounded down to a multiple of S.  Cauchy-Schwarz bounds the rounding error:
//     | c*num/norm_n - G | = | sum_k (a_k - mean_w) e_k | <= norm_p * ||e_t||_2
// hence sim > thr  ==>  G > (c*thr - max_t ||e_t||) * norm_p =: kappa * norm_p; kappa carries an extra relative margin for
// the f64 roundings of the exact formula.  Classes 9 or 13 px wide leave their last column to a second Cauchy-Schwarz term,
// L(w) = kappa * norm_p(w) - c * rho_max * dnorm(w), and take the next narrower K layout (column drop, mfma_common.h).  The
// filter has no false negatives (host model: prefilter_model.hip, tests/test_prefilter_host.py; the device's planes and candidate
// sets against that model: tests/test_gpu_prefilter_model.py).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "mfma_common.h"
#include "verify.h"

namespace focr {

// Size classes -> K layouts, kept widths, super-classes, bank offsets (host only).
void layout_supers(focr_ctx *c) {
    // Column drop (mfma_common.h, "threshold planes"): a class of width 4k + 1 (9, 13) gives its last column to the bound
    // and takes the next narrower K layout — BASELINE configs[1]'s 9x15 templates: 2 K-steps instead of 3.
    for (SizeClass &sc : c->bank.classes) sc.keep_w = (c->column_drop && !sc.tall && (sc.n_w == 9 || sc.n_w == 13)) ? sc.n_w - 1 : sc.n_w;
    // K layout per class (mfma_common.h).  Narrow classes ride the 12-byte-row layout whenever a 9..12-wide
    // class exists, so that all of them share one set of A fragments (one "super-class", one kernel pass).
    bool any_mid = false;
    for (const SizeClass &sc : c->bank.classes) any_mid |= (!sc.tall && sc.keep_w >= 9 && sc.keep_w <= 12);
    c->supers.clear();
    for (size_t k = 0; k < c->bank.classes.size(); k++) {
        SizeClass &sc = c->bank.classes[k];
        if (sc.tall) {  // scanned exactly by scan_tall_kernel; no quantised copy
            sc.layout = LAYOUT_W16;
            sc.k_groups = sc.n_tiles16 = 0;
            continue;
        }
        sc.layout = sc.keep_w >= 13 ? LAYOUT_W16 : (any_mid ? LAYOUT_W12 : LAYOUT_W8);
        if (sc.layout == LAYOUT_W8) sc.k_groups = ((sc.n_h + 1) / 2 + 3) / 4 * 4;   // 2 rows per group
        else if (sc.layout == LAYOUT_W12) sc.k_groups = (sc.n_h + 15) / 16 * 12;    // 16 rows -> 12 groups (3 K-steps)
        else sc.k_groups = (sc.n_h + 3) / 4 * 4;                                    // 1 row per group
        sc.n_tiles16 = (sc.n_templates + 15) / 16;
        size_t si = 0;
        for (; si < c->supers.size(); si++)
            if (c->supers[si].layout == sc.layout && c->supers[si].ksteps == sc.k_groups / 4) break;
        if (si == c->supers.size()) {
            SuperClass su{};
            su.layout = sc.layout;
            su.ksteps = sc.k_groups / 4;
            c->supers.push_back(su);
        }
        SuperClass &su = c->supers[si];
        su.classes.push_back((uint32_t)k);
        su.tile_first.push_back(su.n_tiles);
        su.n_tiles += sc.n_tiles16;
    }
    // Row pairs: a K block covers more rows than a class is tall (BASELINE configs[1]: 15-row classes in LAYOUT_W8's 16 rows), so the
    // fragments a wave loads for window row y also hold the whole of window row y + 1 — against templates that sit one row lower in
    // the block.  A super-class gets that second operand image behind its first one when every class of it leaves the block's last
    // row empty and both images fit the LDS of its one launch (scan_mfma2.hip, PAIR; whether a scan uses it: plan_passes).
    for (SuperClass &su : c->supers) {
        const uint32_t block_rows = su.layout == LAYOUT_W16 ? 4 * su.ksteps : su.layout == LAYOUT_W8 ? 8 * su.ksteps : 16 * (su.ksteps / 3);
        su.pairable = 2 * su.n_tiles <= mfma2_chunk_tiles(su.ksteps);
        for (uint32_t k : su.classes) su.pairable &= c->bank.classes[k].n_h + 1 <= block_rows;
    }
    size_t q_bytes = 0, tg_entries = 0;
    for (SuperClass &su : c->supers) {
        su.q_offset = q_bytes;
        su.tg_offset = tg_entries;
        q_bytes += (size_t)su.n_tiles * su.ksteps * 1024 * (su.pairable ? 2 : 1);
        tg_entries += (size_t)su.n_tiles * 16;
        for (size_t i = 0; i < su.classes.size(); i++) {
            SizeClass &sc = c->bank.classes[su.classes[i]];
            sc.q_offset = (uint32_t)(su.q_offset + (size_t)su.tile_first[i] * su.ksteps * 1024);
            sc.tg_offset = (uint32_t)(su.tg_offset + (size_t)su.tile_first[i] * 16);
        }
    }
}

// Which slot of its class's N-tiles each template takes: the caller's order, except that templates that never emit (constant
// needles: the space glyph) go last, next to the padding — only a class's last tiles hold dead slots then, and the scan kernel
// looks at slot ids in those tiles alone (scan_mfma2.hip, the candidate path).  The candidate KEYS carry the caller's template
// index (tglobal), so nothing outside the scan kernel sees the order.
// (Measured and dropped: grouping look-alike templates into the same tile, greedy by correlation — the four sub-pixel shifts of
// a glyph then share a tile, yet BASELINE configs[1] visits 1.31 M N-tiles per batch either way: DESIGN.md, dead ends.)
static std::vector<uint32_t> live_first_slots(const std::vector<std::vector<double>> &bp) {
    std::vector<uint32_t> slot(bp.size(), 0);
    uint32_t next = 0;
    for (size_t i = 0; i < bp.size(); i++)
        if (!bp[i].empty()) slot[i] = next++;
    for (size_t i = 0; i < bp.size(); i++)
        if (bp[i].empty()) slot[i] = next++;
    return slot;
}

// Quantise the bank (header comment; column drop: mfma_common.h).  `dense` holds the class-ordered dense needles.  Host only:
// fills the per-lane MFMA operand image of every class, the class-ordered template ids (~0 = dead / padding) and
// c->bank.mfma_c_scale / mfma_e_max / mfma_rho_max.
int quantise_bank(focr_ctx *c, const uint8_t *dense, std::vector<int8_t> &qbank, std::vector<uint32_t> &tglobal, std::vector<uint32_t> &order_of) {
    layout_supers(c);
    size_t q_bytes = 0, tg_entries = 0;
    std::vector<size_t> image1(c->bank.classes.size(), 0);  // per class: distance of its bytes in the super-class's second image (0: none)
    for (const SuperClass &su : c->supers) {
        q_bytes += (size_t)su.n_tiles * su.ksteps * 1024 * (su.pairable ? 2 : 1);
        tg_entries += (size_t)su.n_tiles * 16;
        for (uint32_t k : su.classes) image1[k] = su.pairable ? (size_t)su.n_tiles * su.ksteps * 1024 : 0;
    }
    qbank.assign(q_bytes, 0);
    tglobal.assign(tg_entries, 0xffffffffu);
    order_of.assign(c->n_templates, 0);
    c->mfma_slot.assign(c->bank.h_tconst.size(), 0);
    c->bank.mfma_c_scale.clear();
    c->bank.mfma_e_max.clear();
    c->bank.mfma_rho_max.clear();
    for (size_t k = 0; k < c->bank.classes.size(); k++) {
        SizeClass &sc = c->bank.classes[k];
        const uint32_t n = sc.n_w * sc.n_h, ksteps = sc.k_groups / 4, kw = sc.keep_w, n_k = kw * sc.n_h;
        sc.n_live = 0;
        if (sc.tall) {
            for (uint32_t i = 0; i < sc.n_templates; i++) order_of[c->bank.h_tconst[sc.first + i].index] = sc.first + i;
            c->bank.mfma_c_scale.push_back(1.0);
            c->bank.mfma_e_max.push_back(0.0);
            c->bank.mfma_rho_max.push_back(0.0);
            continue;
        }
        // unit mean-centred templates beta; on the kept columns beta' = beta + sigma / n_k (sigma = the dropped column's sum)
        std::vector<std::vector<double>> bp(sc.n_templates);
        double max_ratio = 0.0, rho_max = 0.0;
        for (uint32_t i = 0; i < sc.n_templates; i++) {
            const TemplateConst &tc = c->bank.h_tconst[sc.first + i];
            order_of[tc.index] = sc.first + i;
            const uint8_t *nd = dense + c->bank.h_needle_off[sc.first + i];
            double s = 0, s2 = 0;
            for (uint32_t p = 0; p < n; p++) {
                s += nd[p];
                s2 += (double)nd[p] * nd[p];
            }
            const double mean = s / n, n2 = s2 - s * s / n;
            if (!(n2 > 0.0) || !std::isfinite(tc.rnorm_n)) continue;  // constant needle: rnorm_n = inf, never emits
            const double norm_n = std::sqrt(n2);
            double sigma = 0, rho2 = 0;
            for (uint32_t j = 0; j < sc.n_h; j++)
                for (uint32_t x = kw; x < sc.n_w; x++) {
                    const double b = (nd[j * sc.n_w + x] - mean) / norm_n;
                    sigma += b;
                    rho2 += b * b;
                }
            rho_max = std::max(rho_max, std::sqrt(rho2));
            bp[i].resize(n_k);
            for (uint32_t j = 0; j < sc.n_h; j++)
                for (uint32_t x = 0; x < kw; x++) {
                    const double b = (nd[j * sc.n_w + x] - mean) / norm_n + sigma / n_k;
                    bp[i][j * kw + x] = b;
                    max_ratio = std::max(max_ratio, std::fabs(b));
                }
        }
        const std::vector<uint32_t> slot = live_first_slots(bp);
        for (uint32_t i = 0; i < sc.n_templates; i++) {
            c->mfma_slot[sc.first + i] = slot[i];
            if (bp[i].empty()) continue;
            tglobal[sc.tg_offset + slot[i]] = c->bank.h_tconst[sc.first + i].index;
            sc.n_live++;
        }
        const double c_scale = max_ratio > 0 ? 126.0 / max_ratio : 1.0;
        double e_max = 0.0;
        std::vector<double> rk(n_k);
        std::vector<int> bq(n_k);
        std::vector<uint32_t> idx(n_k);
        for (uint32_t i = 0; i < sc.n_templates; i++) {
            if (bp[i].empty()) continue;
            long sum = 0;
            for (uint32_t p = 0; p < n_k; p++) {
                rk[p] = c_scale * bp[i][p];
                bq[p] = (int)std::floor(rk[p]);
                sum += bq[p];
                idx[p] = p;
            }
            // largest-remainder rounding so that the int8 template sums to exactly zero
            const long deficit = -sum;  // sum(rk) = 0 in exact arithmetic, so 0 <= deficit <= n_k
            if (deficit < 0 || deficit > (long)n_k) return fail(c, FOCR_ERR_INVALID, "mfma bank: rounding deficit out of range");
            std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return rk[a] - bq[a] > rk[b] - bq[b]; });
            for (long d = 0; d < deficit; d++) bq[idx[d]] += 1;
            double e2 = 0;
            long check = 0;
            for (uint32_t p = 0; p < n_k; p++) {
                if (bq[p] > 127 || bq[p] < -127) return fail(c, FOCR_ERR_INVALID, "mfma bank: quantised template out of int8 range");
                double e = rk[p] - bq[p];
                e2 += e * e;
                check += bq[p];
            }
            if (check != 0) return fail(c, FOCR_ERR_INVALID, "mfma bank: quantised template does not sum to zero");
            e_max = std::max(e_max, std::sqrt(e2));
            // scatter into the per-lane MFMA B layout: [n-tile][k-step][g][n][16 bytes]
            const uint32_t nt = slot[i] / 16, nn = slot[i] % 16;
            for (uint32_t j = 0; j < sc.n_h; j++)
                for (uint32_t x = 0; x < kw; x++) {
                    uint32_t ks, g, byte;
                    kgroup_of(sc.layout, j, x, &ks, &g, &byte);
                    qbank[sc.q_offset + ((size_t)(nt * ksteps + ks) * 64 + g * 16 + nn) * 16 + byte] = (int8_t)bq[j * kw + x];
                    if (image1[k]) {  // the second image: the same value one row lower in the K block (its last row is free: layout_supers)
                        kgroup_of(sc.layout, j + 1, x, &ks, &g, &byte);
                        qbank[image1[k] + sc.q_offset + ((size_t)(nt * ksteps + ks) * 64 + g * 16 + nn) * 16 + byte] = (int8_t)bq[j * kw + x];
                    }
                }
        }
        c->bank.mfma_c_scale.push_back(c_scale);
        c->bank.mfma_e_max.push_back(e_max);
        c->bank.mfma_rho_max.push_back(rho_max);
    }
    return FOCR_OK;
}

int build_mfma_bank(focr_ctx *c, const uint8_t *dense) {
    std::vector<int8_t> qbank;
    std::vector<uint32_t> tglobal, order_of;
    if (int rc = quantise_bank(c, dense, qbank, tglobal, order_of)) return rc;
    if (int rc = c->upload(c->bank.d_qbank, qbank.data(), qbank.size(), 16)) return rc;  // (at least 16 bytes: never a null operand)
    if (int rc = c->upload(c->bank.d_tglobal, tglobal.data(), tglobal.size(), 4)) return rc;
    // verify operand: every template as n_h rows of 16 bytes (zero padded), class-ordered
    std::vector<uint8_t> n16;
    std::vector<uint32_t> n16_row(c->bank.h_tconst.size(), 0);
    for (size_t ci = 0; ci < c->bank.h_tconst.size(); ci++) {
        const TemplateConst &tc = c->bank.h_tconst[ci];
        n16_row[ci] = (uint32_t)(n16.size() / 16);
        const uint8_t *nd = dense + c->bank.h_needle_off[ci];
        const uint32_t row_bytes = tc.n_w > 16 ? 32 : 16;
        for (uint32_t j = 0; j < tc.n_h; j++)
            for (uint32_t x = 0; x < row_bytes; x++) n16.push_back(x < tc.n_w ? nd[j * tc.n_w + x] : 0);
    }
    if (int rc = c->upload(c->bank.d_needles16, n16.data(), n16.size(), 16)) return rc;
    {  // the verify's per-template record, by global template index
        std::vector<VerifyMeta> vm(c->n_templates);
        for (size_t ci = 0; ci < c->bank.h_tconst.size(); ci++) {
            const TemplateConst &tc = c->bank.h_tconst[ci];
            vm[tc.index] = VerifyMeta{tc.s_n, tc.n_recip, tc.rnorm_n, (uint16_t)tc.n_w, (uint16_t)tc.n_h, n16_row[ci]};
        }
        if (int rc = c->upload(c->bank.d_vmeta, vm.data(), vm.size())) return rc;
    }
    {  // the same operand by GLOBAL template index, as rows of 12 bytes (every template at most 12 px wide) or 16: chunks of consecutive
       // templates are contiguous there (verify_chunks_kernel, verify.hip: banks whose operand does not fit the LDS whole)
        uint32_t max_w = 0;
        for (const TemplateConst &tc : c->bank.h_tconst) max_w = std::max<uint32_t>(max_w, tc.n_w);
        c->bank.vrow_bytes = max_w <= 12 ? 12u : max_w <= 16 ? 16u : 0u;
        c->bank.h_vrow0_t.assign(c->n_templates + 1, 0);
        if (c->bank.vrow_bytes) {
            std::vector<size_t> ci_of(c->n_templates, 0);
            for (size_t ci = 0; ci < c->bank.h_tconst.size(); ci++) ci_of[c->bank.h_tconst[ci].index] = ci;
            for (size_t t = 0; t < c->n_templates; t++) c->bank.h_vrow0_t[t + 1] = c->bank.h_vrow0_t[t] + c->bank.h_tconst[ci_of[t]].n_h;
            std::vector<uint8_t> rows((size_t)c->bank.h_vrow0_t[c->n_templates] * c->bank.vrow_bytes + 16, 0);
            std::vector<VerifyMeta> vm(c->n_templates);
            for (size_t t = 0; t < c->n_templates; t++) {
                const TemplateConst &tc = c->bank.h_tconst[ci_of[t]];
                const uint8_t *nd = dense + c->bank.h_needle_off[ci_of[t]];
                for (uint32_t j = 0; j < tc.n_h; j++) memcpy(&rows[((size_t)c->bank.h_vrow0_t[t] + j) * c->bank.vrow_bytes], nd + (size_t)j * tc.n_w, tc.n_w);
                vm[t] = VerifyMeta{tc.s_n, tc.n_recip, tc.rnorm_n, (uint16_t)tc.n_w, (uint16_t)tc.n_h, c->bank.h_vrow0_t[t]};
            }
            if (int rc = c->upload(c->bank.d_vrows_t, rows.data(), rows.size())) return rc;
            if (int rc = c->upload(c->bank.d_vmeta_t, vm.data(), vm.size())) return rc;
        }
    }
    if (int rc = c->upload(c->bank.d_needle16_row, n16_row.data(), n16_row.size())) return rc;
    if (int rc = c->upload(c->bank.d_order_of, order_of.data(), order_of.size())) return rc;
    return FOCR_OK;
}

// Threshold parameters of one size class for one scan (mfma_common.h, "threshold planes"): kq towards -inf, crk upwards.
PlaneParams plane_params(const focr_ctx *c, size_t k, double thr_d) {
    const SizeClass &sc = c->bank.classes[k];
    const double cs = c->bank.mfma_c_scale[k], em = c->bank.mfma_e_max[k], rho = c->bank.mfma_rho_max[k];
    const double n = (double)sc.n_w * sc.n_h, n_k = (double)sc.keep_w * sc.n_h, D = n - n_k;
    // kappa carries a relative 1e-4 for the f64 roundings of the reference's formula (its similarity differs from the real
    // number by far less)
    const double kappa = cs * thr_d - em - 1e-4 * (cs * (1.0 + std::fabs(thr_d)) + em);
    PlaneParams p{};
    const double kq_d = kappa / std::sqrt(n);
    float kq = (float)kq_d;
    if ((double)kq > kq_d) kq = std::nextafterf(kq, -INFINITY);
    kq = std::nextafterf(kq, -INFINITY);
    p.kq = std::isfinite(kq) ? kq : -3.0e38f;  // threshold -inf: everything is a candidate
    p.crk = 0.f;
    if (D > 0 && rho > 0) {
        const double cr_d = cs * rho * (1.0 + 1e-4) / n_k;
        float cr = (float)cr_d;
        if ((double)cr < cr_d) cr = std::nextafterf(cr, INFINITY);
        p.crk = std::nextafterf(std::nextafterf(cr, INFINITY), INFINITY);  // also covers a 1-ulp-low square root of W
    }
    // |L| <= |kq| * sqrt(V) + crk * sqrt(W) with sqrt(V) <= 127.5 n, sqrt(W) <= 255 n_k sqrt(D).  The plane's unit S, a power of two
    // (mfma_common.h): every |L - 2| / S within 16384 while |L| < 2^28 (beyond that the plane value's clamp takes over: such
    // thresholds are unreachable or pass everything either way), and S >= K / 2 for the K bytes the MFMA multiplies per window, so
    // that the "never" value -32768 * S lies below every -|G| (|G| <= K * 127 * 128).  S <= 2^14: |C-in| <= 2^29, G + C-in cannot wrap.
    const double l_max = std::min(std::ldexp(1.0, 28), std::fabs((double)p.kq) * 127.5 * n + (double)p.crk * 255.0 * n_k * std::sqrt(std::max(D, 0.0)) + 4.0);
    const double s_min = std::max(l_max / 16384.0, 16.0 * (double)std::max<uint32_t>(sc.k_groups, 4) / 2.0);  // K = 16 bytes per k-group
    uint32_t e = 5;
    while (std::ldexp(1.0, (int)e) < s_min && e < 14) e++;
    p.shift = e;
    p.S = std::ldexp(1.0f, (int)e);
    p.inv_S = std::ldexp(1.0f, -(int)e);
    return p;
}

}  // namespace focr
