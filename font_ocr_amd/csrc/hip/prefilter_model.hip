// prefilter_model.hip — host model of the MFMA prefilter's bound (focr_debug_prefilter, include/focr_ncc.h).
//
// No device call: the quantised bank is built by the very function focr_bank_upload uses (quantise_bank), the threshold of a
// window by the very inline functions the statistics and scan kernels use (mfma_common.h: dropped_column_W, threshold_f32,
// plane_value, prefilter_cin).  The CPU tests check the property the whole fast path rests on — the reference emits
// (sim > thr)  =>  the prefilter flags the pair (G + C-in > 0) — on text, noise, degenerate and adversarial windows, for
// positive and negative thresholds, with and without the column drop (tests/test_prefilter_host.py).
// The model is NOT the device's arithmetic to the bit.  Its f32 square roots are correctly rounded, the device's are the 1-ulp
// instruction (mfma_common.h: sqrt_fast), so a plane value may differ by one unit where (L - 2) / S lies next to an integer; the
// clamp of plane_value is written differently for host and device (compared bit for bit by tests/test_gpu_parity.py::
// test_threshold_plane_values_device_equals_host); and V, W, G come from plain loops here, from sliding sums, 24-bit multiplies
// and byte-unaligned fragment loads over three K layouts in the kernels.  tests/test_gpu_prefilter_model.py closes that gap: the
// device's planes against numpy ("never", conservative against float64) and against this model (equal, or one unit apart where
// the square root explains it), and the device's candidate list against G + C-in formed from the device's own planes.
#include <cmath>
#include <cstring>

#include "mfma_common.h"

using namespace focr;

extern "C" int focr_debug_prefilter(const focr_template_t *templates, size_t n_templates, const uint8_t *needles, size_t needles_len, int column_drop,
                                    const uint8_t *windows, size_t n_windows, uint32_t frame_w, uint32_t frame_h, float threshold, double *sim,
                                    int64_t *d, double *info, size_t n_info) {
    if (!templates || !n_templates || !needles) return FOCR_ERR_INVALID;
    for (size_t t = 0; t < n_templates; t++)
        if (templates[t].n_w == 0 || templates[t].n_h == 0 || templates[t].n_w > 16 || templates[t].n_h > 32 ||
            (size_t)templates[t].offset + (size_t)templates[t].n_w * templates[t].n_h > needles_len ||
            (windows && (templates[t].n_w > frame_w || templates[t].n_h > frame_h)))
            return FOCR_ERR_INVALID;
    focr_ctx ctx;  // host state only
    focr_ctx *c = &ctx;
    c->column_drop = column_drop != 0;
    std::vector<uint32_t> direct, tglobal, order_of;
    std::vector<uint8_t> dense;
    std::vector<int8_t> qbank;
    bank_host_prepare(c, templates, n_templates, needles, direct, dense);
    if (int rc = quantise_bank(c, dense.data(), qbank, tglobal, order_of)) return rc;
    for (size_t k = 0; k < c->bank.classes.size() && info && 4 * k + 3 < n_info; k++) {
        info[4 * k] = c->bank.mfma_c_scale[k];
        info[4 * k + 1] = c->bank.mfma_e_max[k];
        info[4 * k + 2] = c->bank.mfma_rho_max[k];
        info[4 * k + 3] = c->bank.classes[k].keep_w;
    }
    if (!windows || !n_windows || !sim || !d) return FOCR_OK;
    const double thr_d = (double)threshold;
    // int8 templates back out of the per-lane operand image
    std::vector<std::vector<int>> bq(c->bank.h_tconst.size());
    for (size_t k = 0; k < c->bank.classes.size(); k++) {
        const SizeClass &sc = c->bank.classes[k];
        const uint32_t ksteps = sc.k_groups / 4;
        for (uint32_t i = 0; i < sc.n_templates; i++) {
            std::vector<int> &q = bq[sc.first + i];
            const uint32_t slot = c->mfma_slot[sc.first + i];
            q.assign((size_t)sc.keep_w * sc.n_h, 0);
            for (uint32_t j = 0; j < sc.n_h; j++)
                for (uint32_t x = 0; x < sc.keep_w; x++) {
                    uint32_t ks, g, byte;
                    kgroup_of(sc.layout, j, x, &ks, &g, &byte);
                    q[j * sc.keep_w + x] = qbank[sc.q_offset + ((size_t)((slot / 16) * ksteps + ks) * 64 + g * 16 + slot % 16) * 16 + byte];
                }
        }
    }
    for (size_t wi = 0; wi < n_windows; wi++) {
        const uint8_t *a = windows + wi * (size_t)frame_w * frame_h;
        for (size_t k = 0; k < c->bank.classes.size(); k++) {
            const SizeClass &sc = c->bank.classes[k];
            const PlaneParams p = plane_params(c, k, thr_d);
            const uint32_t n = sc.n_w * sc.n_h, kw = sc.keep_w, n_k = kw * sc.n_h;
            uint32_t s = 0, s2 = 0, q1 = 0, q2 = 0;
            for (uint32_t j = 0; j < sc.n_h; j++)
                for (uint32_t x = 0; x < sc.n_w; x++) {
                    const uint32_t v = a[j * frame_w + x];
                    s += v, s2 += v * v;
                    if (x >= kw) q1 += v, q2 += v * v;
                }
            const uint64_t V = (uint64_t)n * s2 - (uint64_t)s * s;
            const float Wf = kw != sc.n_w ? dropped_column_W_upper(n_k, n - n_k, s - q1, q1, q2) : 0.f;
            const float Lf = threshold_f32(p, (float)V, Wf);
            const int16_t plane = V != 0 ? plane_value(p, Lf) : PLANE_NEVER;
            const int cin = prefilter_cin(p.shift, plane);
            const double norm_p = std::sqrt((double)V / (double)n);
            for (uint32_t i = 0; i < sc.n_templates; i++) {
                const TemplateConst &tc = c->bank.h_tconst[sc.first + i];
                const size_t o = wi * n_templates + tc.index;
                sim[o] = NAN;
                d[o] = INT64_MIN;  // dead templates (constant needles) never reach the candidate list
                if (tglobal[sc.tg_offset + c->mfma_slot[sc.first + i]] == 0xffffffffu) continue;
                long G = 0;
                for (uint32_t j = 0; j < sc.n_h; j++)
                    for (uint32_t x = 0; x < kw; x++) G += (long)((int)a[j * frame_w + x] - 128) * bq[sc.first + i][j * kw + x];
                d[o] = (int64_t)G + cin;
                if (V != 0 && std::isfinite(tc.rnorm_n)) {
                    const uint8_t *nd = dense.data() + c->bank.h_needle_off[sc.first + i];
                    double num = 0;
                    for (uint32_t j = 0; j < sc.n_h; j++)
                        for (uint32_t x = 0; x < sc.n_w; x++) num += (double)a[j * frame_w + x] * nd[j * sc.n_w + x];
                    num -= tc.s_n * (double)s * tc.n_recip;
                    sim[o] = num * tc.rnorm_n / norm_p;
                }
            }
        }
    }
    return FOCR_OK;
}

// The same model over every window of one page, with its pieces laid open (focr_debug_prefilter_page, include/focr_ncc.h): the exact
// integer V, the f32 W bound, the f32 L and the int16 plane value per (class, window), the int8 sum G per (template, window), and per
// class the threshold parameters and where the scan puts the class's plane (plan_passes: the very function the scan plans with).
// tests/test_gpu_prefilter_model.py holds the device's planes and candidate sets against it.
extern "C" int focr_debug_prefilter_page(const focr_template_t *templates, size_t n_templates, const uint8_t *needles, size_t needles_len, int column_drop,
                                         int prefilter, const uint8_t *page, uint32_t r_w, uint32_t r_h, float threshold, double *class_info,
                                         size_t class_info_len, size_t *n_classes, int32_t *template_info, int8_t *qtemplates, uint64_t *V,
                                         float *W_upper, float *L, int16_t *plane, int32_t *G, double *sim) {
    if (!templates || !n_templates || !needles || !r_w || !r_h || r_w > 65535 || r_h > 65535) return FOCR_ERR_INVALID;
    if (prefilter != FOCR_PREFILTER_AUTO && prefilter != FOCR_PREFILTER_ONE_STAGE && prefilter != FOCR_PREFILTER_LEGACY) return FOCR_ERR_INVALID;
    for (size_t t = 0; t < n_templates; t++)
        if (templates[t].n_w == 0 || templates[t].n_h == 0 || templates[t].n_w > 16 || templates[t].n_h > 32 ||
            (size_t)templates[t].offset + (size_t)templates[t].n_w * templates[t].n_h > needles_len)
            return FOCR_ERR_INVALID;
    focr_ctx ctx;  // host state only
    focr_ctx *c = &ctx;
    c->column_drop = column_drop != 0;
    c->prefilter = prefilter;
    std::vector<uint32_t> direct, tglobal, order_of;
    std::vector<uint8_t> dense;
    std::vector<int8_t> qbank;
    bank_host_prepare(c, templates, n_templates, needles, direct, dense);
    if (int rc = quantise_bank(c, dense.data(), qbank, tglobal, order_of)) return rc;
    // the passes of a scan of one page of this size, as launch_scan_mfma plans them
    c->pages.r_w = r_w, c->pages.r_h = r_h, c->n_pages = c->sub_np = 1;
    const size_t one_plane = (size_t)((r_w + 63) / 64 * 64 + 64) * ((r_h + 7) / 8 * 8 + 8);
    size_t tiles_total = 0, plane_vals = 0;
    bool need_L = false;
    if (int rc = plan_passes(c, one_plane, tiles_total, plane_vals, need_L)) return rc;
    const size_t n_cls = c->bank.classes.size(), wins = (size_t)r_w * r_h;
    if (n_classes) *n_classes = n_cls;
    const double thr_d = (double)threshold;
    std::vector<PlaneParams> pp(n_cls);
    for (size_t k = 0; k < n_cls; k++) pp[k] = plane_params(c, k, thr_d);
    for (size_t si = 0; si < c->supers.size(); si++) {
        const SuperClass &su = c->supers[si];
        for (size_t v = 0; v < su.classes.size(); v++) {
            const size_t k = su.classes[v];
            const SizeClass &sc = c->bank.classes[k];
            if (!class_info || 16 * k + 15 >= class_info_len) continue;
            double *o = class_info + 16 * k;
            o[0] = sc.n_w, o[1] = sc.n_h, o[2] = sc.keep_w, o[3] = sc.layout, o[4] = su.ksteps, o[5] = (double)si, o[6] = (double)v;
            o[7] = su.mtx && su.planes ? (double)(su.plane_off / one_plane + v) : -1.0;  // the class's plane in focr_debug_planes, in planes of one page
            o[8] = su.mtx, o[9] = su.n_rows, o[10] = pp[k].kq, o[11] = pp[k].crk, o[12] = pp[k].shift;
            o[13] = sc.n_templates, o[14] = sc.n_live, o[15] = su.tile_first[v];
        }
    }
    for (size_t k = 0; k < n_cls; k++) {  // per template: class, slot, live, N-tile inside the super-class; the int8 template itself
        const SizeClass &sc = c->bank.classes[k];
        size_t si = 0, v = 0;
        for (size_t s = 0; s < c->supers.size(); s++)
            for (size_t u = 0; u < c->supers[s].classes.size(); u++)
                if (c->supers[s].classes[u] == k) si = s, v = u;
        const uint32_t ksteps = sc.k_groups / 4;
        for (uint32_t i = 0; i < sc.n_templates; i++) {
            const uint32_t t = c->bank.h_tconst[sc.first + i].index, slot = c->mfma_slot[sc.first + i];
            if (template_info) {
                int32_t *o = template_info + 4 * (size_t)t;
                o[0] = (int32_t)k, o[1] = (int32_t)slot, o[2] = tglobal[sc.tg_offset + slot] != 0xffffffffu, o[3] = (int32_t)(c->supers[si].tile_first[v] + slot / 16);
            }
            if (qtemplates)
                for (uint32_t j = 0; j < 32; j++)
                    for (uint32_t x = 0; x < 16; x++) {
                        int8_t q = 0;
                        if (j < sc.n_h && x < sc.keep_w) {
                            uint32_t ks, g, byte;
                            kgroup_of(sc.layout, j, x, &ks, &g, &byte);
                            q = qbank[sc.q_offset + ((size_t)((slot / 16) * ksteps + ks) * 64 + g * 16 + slot % 16) * 16 + byte];
                        }
                        qtemplates[((size_t)t * 32 + j) * 16 + x] = q;
                    }
        }
    }
    if (!page) return FOCR_OK;
    std::vector<int16_t> a8(wins);  // the page as the MFMA sees it: ink - 128
    for (size_t i = 0; i < wins; i++) a8[i] = (int16_t)((int)page[i] - 128);
    std::vector<uint32_t> S1, S2;  // window sums of the class at hand (for sim)
    for (size_t k = 0; k < n_cls; k++) {
        const SizeClass &sc = c->bank.classes[k];
        const PlaneParams &p = pp[k];
        const uint32_t n = sc.n_w * sc.n_h, kw = sc.keep_w, n_k = kw * sc.n_h, ksteps = sc.k_groups / 4;
        S1.assign(wins, 0), S2.assign(wins, 0);
        for (uint32_t y = 0; y < r_h; y++)
            for (uint32_t x = 0; x < r_w; x++) {
                const size_t w = (size_t)y * r_w + x, o = k * wins + w;
                const bool fits = x + sc.n_w <= r_w && y + sc.n_h <= r_h;
                uint64_t Vw = 0;
                float Wf = 0.f, Lf = 0.f;
                int16_t pl = PLANE_NEVER;
                if (fits) {
                    uint32_t s = 0, s2 = 0, q1 = 0, q2 = 0;
                    for (uint32_t j = 0; j < sc.n_h; j++)
                        for (uint32_t i = 0; i < sc.n_w; i++) {
                            const uint32_t v = page[(size_t)(y + j) * r_w + x + i];
                            s += v, s2 += v * v;
                            if (i >= kw) q1 += v, q2 += v * v;
                        }
                    S1[w] = s, S2[w] = s2;
                    Vw = (uint64_t)n * s2 - (uint64_t)s * s;
                    Wf = kw != sc.n_w ? dropped_column_W_upper(n_k, n - n_k, s - q1, q1, q2) : 0.f;
                    Lf = threshold_f32(p, (float)Vw, Wf);
                    if (x >= 1 && y >= 1 && Vw != 0) pl = plane_value(p, Lf);  // searched windows: src/ncc.rs:279-282
                }
                if (V) V[o] = Vw;
                if (W_upper) W_upper[o] = Wf;
                if (L) L[o] = Lf;
                if (plane) plane[o] = pl;
            }
        if (!G && !sim) continue;
        std::vector<int16_t> bq((size_t)sc.n_h * kw);
        for (uint32_t i = 0; i < sc.n_templates; i++) {
            const TemplateConst &tc = c->bank.h_tconst[sc.first + i];
            const uint32_t slot = c->mfma_slot[sc.first + i];
            const bool live = tglobal[sc.tg_offset + slot] != 0xffffffffu;
            int32_t *Gt = G ? G + (size_t)tc.index * wins : nullptr;
            double *st = sim ? sim + (size_t)tc.index * wins : nullptr;
            for (uint32_t j = 0; j < sc.n_h; j++)  // int8 template back out of the per-lane operand image
                for (uint32_t x = 0; x < kw; x++) {
                    uint32_t ks, g, byte;
                    kgroup_of(sc.layout, j, x, &ks, &g, &byte);
                    bq[(size_t)j * kw + x] = qbank[sc.q_offset + ((size_t)((slot / 16) * ksteps + ks) * 64 + g * 16 + slot % 16) * 16 + byte];
                }
            const uint8_t *nd = dense.data() + c->bank.h_needle_off[sc.first + i];
            for (uint32_t y = 0; y < r_h; y++)
                for (uint32_t x = 0; x < r_w; x++) {
                    const size_t w = (size_t)y * r_w + x;
                    const bool fits = x + sc.n_w <= r_w && y + sc.n_h <= r_h;
                    if (Gt) {
                        int32_t g = INT32_MIN;  // dead templates (constant needles) and windows that leave the page: no sum
                        if (fits && live) {
                            g = 0;
                            for (uint32_t j = 0; j < sc.n_h; j++) {
                                const int16_t *ar = &a8[(size_t)(y + j) * r_w + x], *br = &bq[(size_t)j * kw];
                                int32_t r = 0;
                                for (uint32_t i2 = 0; i2 < kw; i2++) r += (int32_t)ar[i2] * br[i2];
                                g += r;
                            }
                        }
                        Gt[w] = g;
                    }
                    if (st) {
                        double sv = NAN;  // where the reference cannot emit: not searched, zero variance, constant needle
                        const uint64_t Vw = (uint64_t)n * S2[w] - (uint64_t)S1[w] * S1[w];
                        if (fits && live && x >= 1 && y >= 1 && Vw != 0 && std::isfinite(tc.rnorm_n)) {
                            uint32_t acc = 0;
                            for (uint32_t j = 0; j < sc.n_h; j++)
                                for (uint32_t i2 = 0; i2 < sc.n_w; i2++) acc += (uint32_t)page[(size_t)(y + j) * r_w + x + i2] * nd[j * sc.n_w + i2];
                            const double num = (double)acc - tc.s_n * (double)S1[w] * tc.n_recip;
                            sv = num * tc.rnorm_n / std::sqrt((double)Vw / (double)n);
                        }
                        st[w] = sv;
                    }
                }
        }
    }
    return FOCR_OK;
}

// The MFMA operand images of a bank as focr_bank_upload builds them (focr_debug_bank_images, include/focr_ncc.h): the raw bytes of
// d_qbank and, per super-class, where its first image starts and whether a second one follows it (row pairs, layout_supers).
extern "C" int focr_debug_bank_images(const focr_template_t *templates, size_t n_templates, const uint8_t *needles, size_t needles_len, int column_drop,
                                      uint32_t *super_info, size_t super_cap, size_t *n_supers, int8_t *out, size_t capacity, size_t *n_bytes) {
    if (!templates || !n_templates || !needles || !n_supers || !n_bytes) return FOCR_ERR_INVALID;
    for (size_t t = 0; t < n_templates; t++)
        if (templates[t].n_w == 0 || templates[t].n_h == 0 || templates[t].n_w > 16 || templates[t].n_h > 32 ||
            (size_t)templates[t].offset + (size_t)templates[t].n_w * templates[t].n_h > needles_len)
            return FOCR_ERR_INVALID;
    focr_ctx ctx;  // host state only
    focr_ctx *c = &ctx;
    c->column_drop = column_drop != 0;
    std::vector<uint32_t> direct, tglobal, order_of;
    std::vector<uint8_t> dense;
    std::vector<int8_t> qbank;
    bank_host_prepare(c, templates, n_templates, needles, direct, dense);
    if (int rc = quantise_bank(c, dense.data(), qbank, tglobal, order_of)) return rc;
    *n_supers = c->supers.size();
    *n_bytes = qbank.size();
    for (size_t si = 0; si < c->supers.size() && super_info && si < super_cap; si++) {
        const SuperClass &su = c->supers[si];
        const uint32_t v[6] = {su.layout, su.ksteps, su.n_tiles, su.pairable ? 1u : 0u, (uint32_t)su.q_offset, mfma2_chunk_tiles(su.ksteps)};
        memcpy(super_info + 6 * si, v, sizeof v);
    }
    if (out) {
        if (capacity < qbank.size()) return FOCR_ERR_INVALID;
        if (!qbank.empty()) memcpy(out, qbank.data(), qbank.size());
    }
    return FOCR_OK;
}

// the plane value of a threshold L for a unit 2^shift (mfma_common.h: plane_value), host flavour (the device's is checked against it
// on the GPU: test_gpu_parity.py)
extern "C" void focr_debug_plane_value(const float *L, size_t n, uint32_t shift, int16_t *out) {
    PlaneParams p{};
    p.shift = shift;
    p.S = std::ldexp(1.0f, (int)shift);
    p.inv_S = std::ldexp(1.0f, -(int)shift);
    for (size_t i = 0; i < n; i++) out[i] = plane_value(p, L[i]);
}

// ... and the device flavour, for the GPU test that compares the two bit for bit
__global__ void plane_value_kernel(const float *__restrict__ x, size_t n, PlaneParams p, int16_t *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = plane_value(p, x[i]);
}
extern "C" int focr_debug_plane_value_device(focr_ctx_t *c, const float *x, size_t n, uint32_t shift, int16_t *out) {
    if (!c || !x || !out || !n) return fail(c, FOCR_ERR_INVALID, "focr_debug_plane_value_device: bad arguments");
    FOCR_HIP(c, hipSetDevice(c->device));
    PlaneParams p{};
    p.shift = shift;
    p.S = std::ldexp(1.0f, (int)shift);
    p.inv_S = std::ldexp(1.0f, -(int)shift);
    DevArray<float> dx;
    DevArray<int16_t> dout;
    FOCR_HIP(c, dx.reserve(n, Grow::exact, nullptr));
    FOCR_HIP(c, dout.reserve(n, Grow::exact, nullptr));
    FOCR_HIP(c, hipMemcpyAsync(dx, x, n * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(plane_value_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, dx.p, n, p, dout.p);
    FOCR_HIP(c, hipGetLastError());
    FOCR_HIP(c, hipMemcpyAsync(out, dout, n * 2, hipMemcpyDeviceToHost, c->stream));
    FOCR_HIP(c, hipStreamSynchronize(c->stream));
    return FOCR_OK;
}
