// results.hip — the scan driver and everything that reads results back: size estimates, focr_scan and its split-batch fallback,
// finish_results, the result getters and the debug read-backs (include/focr_ncc.h layer 2).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <unordered_map>

#include "common.h"

namespace focr {

// Size estimates shared between the contexts of a process, keyed by the setup's signature (SizeEstimate::publish / adopt)
static std::mutex g_est_mu;
static std::unordered_map<uint64_t, SizeEstimate> g_est;

// per device: the origin of focr_debug_phase_stamps, recorded by the device's first context
static std::mutex g_origin_mu;
static hipEvent_t g_origin[64] = {};

void phase_origin_record(int device, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_origin_mu);
    hipEvent_t &b = g_origin[(unsigned)device % 64];
    if (!b && hipEventCreate(&b) == hipSuccess) (void)hipEventRecord(b, s);
}

// bounds for the next scan of the same setup: this scan's counts + a margin that follows how much the counts have been moving (20 %
// after the first scan of a setup; 4 % once consecutive batches agree to ~1 %): every element of margin is sorted, scanned and stepped
// over by all the later phases
void SizeEstimate::update(const focr_ctx *c, uint64_t n_cand, uint64_t n_hits, uint64_t largest_row) {
    if (last_cand) {
        const auto rel = [](uint64_t a, uint64_t b) { return (double)(a > b ? a - b : b - a) / (double)std::max<uint64_t>(std::min(a, b), 1); };
        var = std::max(var * 0.75, std::max(rel(n_cand, last_cand), rel(n_hits, last_hits)));
    }
    last_cand = n_cand;
    last_hits = n_hits;
    const double m = margin();
    cand = (size_t)n_cand + (size_t)((double)n_cand * m) + 8192;
    hits = (size_t)n_hits + (size_t)((double)n_hits * m) + 8192;
    row_max = c->row_cap ? (uint32_t)std::max<uint64_t>(largest_row, 1) : 0;  // 0: the scan took the legacy tail
    uint32_t sh, ns;
    row_segments(c, &sh, &ns);
    // buckets still well above what a wave sorts in registers: halve the x-segments for the next scan of this setup
    seg_shift = largest_row > 2048 && sh > 5 ? sh - 1 : sh;
}

// the last counts + the widest margin, for the executor's other contexts: only a stream's first batch pays the exact-size scan's waits
void SizeEstimate::publish(uint64_t sig) const {
    std::lock_guard<std::mutex> lk(g_est_mu);
    if (g_est.size() > 256) g_est.clear();
    g_est[sig] = SizeEstimate{(size_t)last_cand + (size_t)last_cand / 5 + 8192, (size_t)last_hits + (size_t)last_hits / 5 + 8192, 0.0667, 0, 0, row_max, seg_shift};
}

void SizeEstimate::adopt(uint64_t sig) {
    std::lock_guard<std::mutex> lk(g_est_mu);
    auto it = g_est.find(sig);
    if (it != g_est.end()) *this = it->second;
}

void SizeEstimate::forget(uint64_t sig) {
    std::lock_guard<std::mutex> lk(g_est_mu);
    g_est.erase(sig);
}

__global__ void debug_rnorm_kernel(const uint32_t *s, const uint64_t *s2, const uint32_t *n, size_t cnt, double *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) out[i] = window_rnorm(s[i], s2[i], (double)n[i]);
}

// split-batch mode: keep only the hits that survive their call's cap, appended in order
__global__ void append_kept_hits(const uint64_t *__restrict__ hkeys, const float *__restrict__ hsims, const uint8_t *__restrict__ keep,
                                 const uint64_t *__restrict__ pos, size_t n, uint64_t *__restrict__ out_keys,
                                 float *__restrict__ out_sims) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    out_keys[pos[i]] = hkeys[i];
    out_sims[pos[i]] = hsims[i];
}

__global__ void widen_u8_to_u64(const uint8_t *__restrict__ in, size_t n, uint64_t *__restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i];
}

__global__ void widen_u32_to_u64(const uint32_t *__restrict__ in, size_t n, uint64_t *__restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) out[i] = i < n ? in[i] : 0;
}

// A hit count the host knows (a direct scan's, a split batch's total, debug hits) as the device-side value the ordering and
// process_hits read: queued on the context's stream, so n_hits_raw_u64 keeps it until the copy has run.
int install_host_hits(focr_ctx *c, uint64_t n) {
    c->n_hits_raw_u64 = n;
    FOCR_HIP(c, hipMemcpyAsync(&c->d_res.p->host_hits, &c->n_hits_raw_u64, sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    c->d_n_hits = &c->d_res.p->host_hits;
    c->ub_hits = (size_t)n;
    return FOCR_OK;
}

}  // namespace focr

using namespace focr;

template <typename Run>
static int scan_split(focr_ctx *c, Run &run) {
    const size_t T = c->n_templates, n_seg_all = c->n_pages * T;
    size_t match_total = 0, hit_total = 0, raw_total = 0, cand_total = 0;
    float ms_acc[N_TIMINGS] = {};
    uint64_t issued = 0;
    if (!c->scratch(c->acc_seg_count, n_seg_all + 1)) return fail(c, FOCR_ERR_NOMEM, "focr_scan: hipMalloc failed");
    uint32_t *acc_cnt = c->acc_seg_count;
    size_t np = std::max<size_t>(1, c->n_pages / 2);
    for (size_t p0 = 0; p0 < c->n_pages;) {
        np = std::min(np, c->n_pages - p0);
        int rc = run(p0, np);
        if ((rc == FOCR_ERR_OVERFLOW || rc == FOCR_ERR_NOMEM) && np > 1) {
            np = (np + 1) / 2;  // still too much: halve and retry the same pages
            continue;
        }
        if (rc) return rc;
        // append: matches, per-call counts, kept hits
        const size_t nm = c->n_matches, nh = c->n_hits;
        if (nm && (rc = materialise_matches(c, c->stream))) return rc;  // the sub-batch's lists are read here
        if (c->acc_matches.reserve(match_total + nm + 1, Grow::half, &c->stream, match_total) ||
            c->acc_hkeys.reserve(hit_total + nm + 1, Grow::half, &c->stream, hit_total) ||
            c->acc_hsims.reserve(hit_total + nm + 1, Grow::half, &c->stream, hit_total))
            return fail(c, FOCR_ERR_NOMEM, "focr_scan: hipMalloc failed");
        focr_match_t *am = c->acc_matches;
        uint64_t *ak = c->acc_hkeys;
        float *as = c->acc_hsims;
        if (nm) FOCR_HIP(c, hipMemcpyAsync(am + match_total, c->d_matches, nm * sizeof(focr_match_t), hipMemcpyDeviceToDevice, c->stream));
        FOCR_HIP(c, hipMemcpyAsync(acc_cnt + p0 * T, c->d_seg_count, np * T * 4, hipMemcpyDeviceToDevice, c->stream));
        if (nh) {
            if (!c->scratch(c->scan_flags, (nh + 1) * 8) || !c->scratch(c->scan_pos, (nh + 1) * 8)) return fail(c, FOCR_ERR_NOMEM, "focr_scan: hipMalloc failed");
            uint64_t *f64 = c->scan_flags.as<uint64_t>(), *pos = c->scan_pos.as<uint64_t>();
            const unsigned nb = (unsigned)((nh + 255) / 256);
            hipLaunchKernelGGL(widen_u8_to_u64, dim3(nb), dim3(256), 0, c->stream, c->ord_keep.p, nh, f64);
            if ((rc = exclusive_scan_u64(c, f64, pos, nh))) return rc;
            hipLaunchKernelGGL(append_kept_hits, dim3(nb), dim3(256), 0, c->stream, c->d_hkeys, c->d_hsims, c->ord_keep.p,
                               pos, nh, ak + hit_total, as + hit_total);
            FOCR_HIP(c, hipGetLastError());
        }
        FOCR_HIP(c, hipStreamSynchronize(c->stream));
        match_total += nm;
        hit_total += nm;  // kept hits == matches
        raw_total += c->n_hits_raw;
        cand_total += c->n_cand;
        issued += c->counters[CNT_ISSUED_MACS];
        for (int i = 0; i < N_TIMINGS; i++) ms_acc[i] += c->ms[i];
        p0 += np;
    }
    // install the accumulated results as the scan's results
    {
        uint64_t *count64 = c->d_seg_start + (n_seg_all + 1);  // seg arrays were sized for the whole batch by the sub-runs
        hipLaunchKernelGGL(widen_u32_to_u64, dim3((unsigned)((n_seg_all + 256) / 256)), dim3(256), 0, c->stream, acc_cnt, n_seg_all, count64);
        int rc = exclusive_scan_u64(c, count64, c->d_seg_offset, n_seg_all + 1);
        if (rc) return rc;
        FOCR_HIP(c, hipMemcpyAsync(c->d_seg_count, acc_cnt, n_seg_all * 4, hipMemcpyDeviceToDevice, c->stream));
        if (!c->scratch(c->ord_keep, hit_total + 1)) return fail(c, FOCR_ERR_NOMEM, "focr_scan: hipMalloc failed");
        FOCR_HIP(c, hipMemsetAsync(c->ord_keep, 1, hit_total + 1, c->stream));
        FOCR_HIP(c, hipStreamSynchronize(c->stream));
        std::swap(c->d_matches, c->acc_matches);  // hand the accumulated list over
        c->lazy.pending = false;                  // ... complete: nothing is left to write on demand
        c->d_hkeys = c->acc_hkeys;
        c->d_hsims = c->acc_hsims;
        // the accumulated hit count as the device-side value process_hits reads
        if ((rc = install_host_hits(c, hit_total))) return rc;
        FOCR_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->sub_p0 = 0;
    c->sub_np = c->n_pages;
    c->n_matches = match_total;
    c->n_hits = hit_total;
    c->n_hits_raw = raw_total;
    c->n_cand = cand_total;
    c->counters[CNT_CANDIDATES] = cand_total;
    c->counters[CNT_HITS] = raw_total;
    c->counters[CNT_ISSUED_MACS] = issued;
    for (int i = 0; i < N_TIMINGS; i++) c->ms[i] = ms_acc[i];
    return FOCR_OK;
}

namespace focr {

// The whole scan pipeline on the resident batch with the parameters stored in the context (focr_scan, and the redo of a
// batch whose estimated sizes turned out too small).
static int scan_now(focr_ctx *c) {
    const float threshold = c->scan_thr;
    const int mode = c->scan_mode;
    c->results_gone();
    for (auto &m : c->ms) m = 0.f;
    c->counters[CNT_ISSUED_MACS] = 0;
    auto run = [&](size_t p0, size_t np) -> int {  // the whole pipeline on pages [p0, p0 + np)
        c->sub_p0 = p0;
        c->sub_np = np;
        c->sub_run_starts();
        int r = mode == FOCR_SCAN_MFMA ? launch_scan_mfma(c, threshold) : launch_scan_direct(c, threshold, mode == FOCR_SCAN_RUST);
        if (r) return r;
        if (!c->ordered && (r = order_hits(c))) return r;
        c->sizes_pending = true;
        return c->estimated ? FOCR_OK : finish_results(c);  // exact sizes: the counts are read here, as they always were
    };
    // focr_debug_force_split (tests): take the split-batch path without waiting for an overflow
    int rc = c->force_split ? FOCR_ERR_OVERFLOW : run(0, c->n_pages);
    if (rc == FOCR_ERR_OVERFLOW || rc == FOCR_ERR_NOMEM) {
        // Too many candidates for one pass (very low thresholds): scan the batch in page sub-ranges and append the
        // results.  Only hits that survive the per-call cap are kept, so the totals stay bounded by pages x T x cap.
        c->estimated = false;
        c->sizes_pending = false;
        rc = scan_split(c, run);
        if (rc) return rc;
        c->cand_intact = false;  // d_cand holds the last page sub-range's candidates only
        // the sub-runs left the size estimates at the counts of the LAST page sub-range: a following scan of this setup, here or on
        // another context, must not run "estimated" on them (it would overflow, redo exact, overflow again and only then split)
        c->est.reset();
        SizeEstimate::forget(c->est_sig);
    } else if (rc) {
        return rc;
    }
    c->scanned = true;
    return FOCR_OK;
}

// ms[slot] = the time from one phase event to another, by TimingSlot
static constexpr struct { PhaseEvent begin, end; } PHASE_SPAN[N_TIMINGS] = {{EV_STATS_BEGIN, EV_STATS_END}, {EV_STATS_END, EV_SCAN_END}, {EV_SCAN_END, EV_VERIFY_END},
                                                                            {EV_VERIFY_END, EV_ORDER_END}, {EV_POST_BEGIN, EV_POST_END}, {EV_STATS_BEGIN, EV_ORDER_END}};
static hipError_t read_phase(focr_ctx *c, TimingSlot m) { return hipEventElapsedTime(&c->ms[m], c->ev[PHASE_SPAN[m].begin], c->ev[PHASE_SPAN[m].end]); }

int finish_results(focr_ctx *c) {
    if (!c->sizes_pending && !c->post_pending) return FOCR_OK;
    FOCR_HIP(c, hipSetDevice(c->device));
    if (int rc = wait_batch(c)) return rc;
    if (c->sizes_pending) {
        c->sizes_pending = false;
        const ResultBlock &r = *c->h_res;
        const uint64_t n_cand = r.candidates, n_hits = r.hits, total = r.matches;
        if (r.flags & RES_FLAG_KEY) return fail(c, FOCR_ERR_STATE, "internal error: a candidate key outside the batch reached the verify stage");
        if (c->estimated && (r.flags & (RES_FLAG_COUNT | RES_FLAG_ROW))) {
            // a count exceeded the bound taken from the previous scan: redo this batch with exact sizes (and its
            // process_hits, if that was queued behind it)
            const bool redo_post = c->post_pending;
            c->post_pending = false;
            c->estimated = false;
            c->est.reset();  // back to the 20 % margin
            c->counters_redone++;
            int rc = scan_now(c);
            if (rc) return rc;
            return redo_post ? focr_process_hits(c, c->post_anchor, c->post_overlap) : FOCR_OK;
        }
        if (c->scan_mode == FOCR_SCAN_MFMA) {
            c->n_cand = (size_t)n_cand;
            c->counters[CNT_CANDIDATES] = n_cand;
            for (TimingSlot m : {MS_STATS, MS_SCAN, MS_VERIFY}) FOCR_HIP(c, read_phase(c, m));  // (a direct scan times its kernels itself, scan_direct.hip)
            c->counters[CNT_ISSUED_MACS] = 0;
            for (size_t i = 0; i < c->launches.size(); i++) {  // issued MACs follow the number of live M-tiles (known only now)
                if (c->launch_super[i] != focr_ctx::NO_SUPER) c->launches[i].issued_macs *= c->h_live[c->launch_super[i]];
                c->counters[CNT_ISSUED_MACS] += c->launches[i].issued_macs;
            }
            c->launches_collect();
            c->est.update(c, n_cand, n_hits, r.row_max);
            // for the other contexts that scan this setup — counts of a page sub-range of a split batch are no bound for a whole batch
            if (c->est_sig && c->sub_np == c->n_pages) c->est.publish(c->est_sig);
        }
        c->counters[CNT_HITS] = n_hits;
        c->n_hits = c->n_hits_raw = (size_t)n_hits;
        c->n_matches = (size_t)total;
        for (TimingSlot m : {MS_ORDER, MS_TOTAL}) FOCR_HIP(c, read_phase(c, m));
    }
    if (c->post_pending) {
        c->post_pending = false;
        const uint64_t tot = c->h_res->lines_chars;
        c->n_lines = (size_t)(tot >> 32);
        c->n_chars = (size_t)(tot & 0xffffffffu);
        FOCR_HIP(c, read_phase(c, MS_POST));
    }
    return FOCR_OK;
}

}  // namespace focr

extern "C" {

size_t focr_last_launches(focr_ctx_t *c, focr_launch_info_t *out, size_t cap) {
    if (!c || finish_results(c) != FOCR_OK) return 0;
    for (size_t i = 0; out && i < c->launches.size() && i < cap; i++) out[i] = c->launches[i];
    return c->launches.size();
}

// Diagnostic: where the phases of the context's last batch lie on the DEVICE's clock — milliseconds since a per-device base event
// (recorded when the first context of the device is created): [0] statistics start, [1] statistics end, [2] scan kernels end,
// [3] verify end, [4] ordering end, [5] process_hits start, [6] process_hits end, [7] start of the dominant scan launch, [8] its end.
// What a kernel trace shows, without a profiler in the process (tools/r5_phase_dump: the two rhythms of DESIGN.md section 5).
int focr_debug_phase_stamps(focr_ctx_t *c, double out[9]) {
    if (!c || !out) return FOCR_ERR_INVALID;
    if (int rc = finish_results(c)) return rc;
    FOCR_HIP(c, hipSetDevice(c->device));
    hipEvent_t base = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_origin_mu);
        base = g_origin[(unsigned)c->device % 64];
    }
    for (int i = 0; i < 9; i++) out[i] = -1.0;
    if (!base) return FOCR_OK;
    for (int i = 0; i < N_PHASE_EVENTS; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, base, c->ev[i]) == hipSuccess) out[i] = ms;
        else (void)hipGetLastError();
    }
    size_t best = 0;
    for (size_t i = 1; i < c->launches.size(); i++)
        if (c->launches[i].alg_macs > c->launches[best].alg_macs) best = i;
    if (!c->launches.empty() && c->launch_events.size() >= 2 * c->launches.size()) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, base, c->launch_events[2 * best]) == hipSuccess) out[N_PHASE_EVENTS] = ms;
        if (hipEventElapsedTime(&ms, base, c->launch_events[2 * best + 1]) == hipSuccess) out[N_PHASE_EVENTS + 1] = ms;
        (void)hipGetLastError();
    }
    return FOCR_OK;
}

int focr_debug_tail_path(focr_ctx_t *c, uint32_t out[8]) {
    if (!c || !out) return fail(c, FOCR_ERR_INVALID, "focr_debug_tail_path: bad arguments");
    if (!c->scanned) return fail(c, FOCR_ERR_STATE, "focr_debug_tail_path: no scan results");
    if (int rc = finish_results(c)) return rc;  // (an estimated scan whose counts exceeded their bounds is redone here: the redo's path is the scan's)
    const focr_ctx::TailPath &p = c->tail_path;
    const uint32_t v[8] = {p.tail, p.big_launch, p.library_sort, p.order_form, p.seg_shift, p.n_seg, p.verify_form, p.verify_chunks};
    memcpy(out, v, sizeof v);
    return FOCR_OK;
}

int focr_debug_scan_paired(focr_ctx_t *c, uint32_t out[2]) {
    if (!c || !out) return fail(c, FOCR_ERR_INVALID, "focr_debug_scan_paired: bad arguments");
    if (!c->scanned) return fail(c, FOCR_ERR_STATE, "focr_debug_scan_paired: no scan results");
    if (int rc = finish_results(c)) return rc;  // (a redone scan's launches are the scan's)
    out[0] = out[1] = 0;
    for (const focr_launch_info_t &li : c->launches) {  // the per-launch records: the plane kernel's launches, and those of its paired form
        if (strncmp(li.name, "scan_mfma2s_kernel<", 19) != 0) continue;
        out[0]++;
        if (strstr(li.name, ",pair>")) out[1]++;
    }
    return FOCR_OK;
}

int focr_debug_planes(focr_ctx_t *c, uint16_t *out, size_t capacity, size_t *n_values) {
    if (!c || !n_values) return FOCR_ERR_INVALID;
    FOCR_HIP(c, hipSetDevice(c->device));
    if (int rc = focr_sync(c)) return rc;
    *n_values = c->d_planes.cap;
    if (!out) return FOCR_OK;
    if (capacity < *n_values) return fail(c, FOCR_ERR_INVALID, "focr_debug_planes: buffer too small");
    if (*n_values) FOCR_HIP(c, hipMemcpy(out, c->d_planes, *n_values * 2, hipMemcpyDeviceToHost));
    return FOCR_OK;
}

// Test hook: the candidate keys of the last MFMA scan, unpacked.  Nothing is kept for it during a scan: the hits-first tail only reads
// d_cand, so the keys are still where the scan kernels' flushes left them; the legacy tail sorts and compacts them in place, and a
// split batch leaves only its last page sub-range there — both are refused.
int focr_debug_candidates(focr_ctx_t *c, uint32_t *out, size_t capacity, size_t *n) {
    if (!c || !n) return fail(c, FOCR_ERR_INVALID, "focr_debug_candidates: bad arguments");
    if (!c->scanned) return fail(c, FOCR_ERR_STATE, "focr_debug_candidates: no scan results");
    if (c->debug_hits) return fail(c, FOCR_ERR_STATE, "focr_debug_candidates: the hits came from focr_debug_process_hits, not from a scan");
    if (c->scan_mode != FOCR_SCAN_MFMA) return fail(c, FOCR_ERR_STATE, "focr_debug_candidates: the last scan was not an MFMA scan (no candidate list)");
    if (int rc = finish_results(c)) return rc;  // (an estimated scan whose counts exceeded their bounds is redone here, with exact sizes)
    if (!c->cand_intact)
        return fail(c, FOCR_ERR_STATE, "focr_debug_candidates: the last scan's candidates are gone (legacy tail: sorted and compacted in place; split batch: only the last page sub-range is left)");
    *n = c->n_cand;
    if (!out) return FOCR_OK;
    if (capacity < c->n_cand) return fail(c, FOCR_ERR_INVALID, "focr_debug_candidates: buffer too small");
    if (c->n_cand > c->d_cand.cap) return fail(c, FOCR_ERR_STATE, "focr_debug_candidates: internal: more candidates than the list holds");
    FOCR_HIP(c, hipSetDevice(c->device));
    std::vector<uint64_t> keys(c->n_cand);
    if (c->n_cand) {
        FOCR_HIP(c, hipMemcpyAsync(keys.data(), c->d_cand, c->n_cand * 8, hipMemcpyDeviceToHost, c->io_stream));
        FOCR_HIP(c, hipStreamSynchronize(c->io_stream));
    }
    for (size_t i = 0; i < keys.size(); i++) {
        out[4 * i] = c->fmt.page(keys[i]), out[4 * i + 1] = c->fmt.y(keys[i]);
        out[4 * i + 2] = c->fmt.x(keys[i]), out[4 * i + 3] = c->fmt.t(keys[i]);
    }
    return FOCR_OK;
}

int focr_scan(focr_ctx_t *c, float threshold, uint32_t cap, int mode) {
    if (!c) return FOCR_ERR_INVALID;
    if (!c->n_templates) return fail(c, FOCR_ERR_STATE, "focr_scan: no bank uploaded");
    if (!c->pages.u8) return fail(c, FOCR_ERR_STATE, "focr_scan: no pages resident");
    if (cap == 0) return fail(c, FOCR_ERR_INVALID, "focr_scan: cap must be >= 1 (src/ncc.cpp:43-46)");
    if (mode != FOCR_SCAN_MFMA && mode != FOCR_SCAN_DIRECT && mode != FOCR_SCAN_RUST) return fail(c, FOCR_ERR_INVALID, "focr_scan: bad mode");
    if (std::isnan(threshold)) threshold = INFINITY;  // `sim > NaN` is never true in the reference (src/ncc.cpp:362-366): no hits
    FOCR_HIP(c, hipSetDevice(c->device));
    c->cap = cap;
    c->scan_thr = threshold;
    c->scan_mode = mode;
    // algorithmic MACs, SURVEY.md section 8(d): true template area x searched windows
    uint64_t macs = 0;
    for (const SizeClass &sc : c->bank.classes) {
        if (sc.n_w > c->pages.r_w || sc.n_h > c->pages.r_h) continue;
        uint64_t wx = c->pages.r_w - sc.n_w, wy = c->pages.r_h - sc.n_h;  // x in [1, r_w-n_w], y in [1, r_h-n_h]
        macs += wx * wy * (uint64_t)sc.n_w * sc.n_h * sc.n_templates;
    }
    c->counters[CNT_ALG_MACS] = macs * c->n_pages;
    c->fmt = key_format(c->n_templates, c->pages.r_w, c->pages.r_h, c->n_pages);
    // Size estimates are reused only for the very same setup (bank, batch geometry, threshold, cap, prefilter)
    uint32_t tb;
    memcpy(&tb, &threshold, 4);
    uint64_t sig = 1469598103934665603ull;
    for (uint64_t v : {(uint64_t)c->bank_hash, (uint64_t)c->device, (uint64_t)c->tail_mode, (uint64_t)c->n_pages, (uint64_t)c->pages.r_w, (uint64_t)c->pages.r_h, (uint64_t)tb, (uint64_t)cap, (uint64_t)mode,
                       (uint64_t)c->prefilter})
        sig = (sig ^ v) * 1099511628211ull;
    if (sig != c->est_sig) c->est.reset();
    c->est_sig = sig;
    if (c->est.cand == 0 && c->estimates_enabled && mode == FOCR_SCAN_MFMA) c->est.adopt(sig);  // none of its own yet: a neighbour's, if any
    c->estimated = c->estimates_enabled && mode == FOCR_SCAN_MFMA && !c->force_split && c->est.cand != 0;
    return scan_now(c);
}

int focr_size_estimate_stats(focr_ctx_t *c, uint64_t *redone, double *margin, uint32_t *row_max) {
    if (!c) return FOCR_ERR_INVALID;
    if (int rc = finish_results(c)) return rc;
    if (redone) *redone = c->counters_redone;
    if (margin) *margin = c->est.margin();
    if (row_max) *row_max = c->est.row_max;
    return FOCR_OK;
}

int focr_ctx_set_size_estimates(focr_ctx_t *c, int on) {
    if (!c) return FOCR_ERR_INVALID;
    c->estimates_enabled = on != 0;
    return FOCR_OK;
}

int focr_get_counts(focr_ctx_t *c, uint32_t *counts) {
    if (!c || !counts) return fail(c, FOCR_ERR_INVALID, "focr_get_counts: bad arguments");
    if (!c->scanned) return fail(c, FOCR_ERR_STATE, "focr_get_counts: no scan results");
    if (c->debug_hits) return fail(c, FOCR_ERR_STATE, "focr_get_counts: the hits came from focr_debug_process_hits, not from a scan");
    if (int rc = finish_results(c)) return rc;
    FOCR_HIP(c, hipSetDevice(c->device));
    // (finished results are read back on io_stream: inside an executor the context's own stream already holds the lane's next batch)
    FOCR_HIP(c, hipMemcpyAsync(counts, c->d_seg_count, c->n_pages * c->n_templates * 4, hipMemcpyDeviceToHost, c->io_stream));
    FOCR_HIP(c, hipStreamSynchronize(c->io_stream));
    return FOCR_OK;
}

size_t focr_total_matches(focr_ctx_t *c) { return (c && c->scanned && finish_results(c) == FOCR_OK) ? c->n_matches : 0; }

int focr_get_matches(focr_ctx_t *c, uint64_t *offsets, focr_match_t *matches) {
    if (!c) return FOCR_ERR_INVALID;
    if (!c->scanned) return fail(c, FOCR_ERR_STATE, "focr_get_matches: no scan results");
    if (c->debug_hits) return fail(c, FOCR_ERR_STATE, "focr_get_matches: the hits came from focr_debug_process_hits, not from a scan");
    if (int rc = finish_results(c)) return rc;
    FOCR_HIP(c, hipSetDevice(c->device));
    if (offsets)
        FOCR_HIP(c, hipMemcpyAsync(offsets, c->d_seg_offset, (c->n_pages * c->n_templates + 1) * 8, hipMemcpyDeviceToHost,
                                   c->io_stream));
    if (matches && c->n_matches) {
        if (int rc = materialise_matches(c, c->io_stream)) return rc;  // the first reader of this scan's lists writes them (order.hip)
        FOCR_HIP(c, hipMemcpyAsync(matches, c->d_matches, c->n_matches * sizeof(focr_match_t), hipMemcpyDeviceToHost,
                                   c->io_stream));
    }
    FOCR_HIP(c, hipStreamSynchronize(c->io_stream));
    return FOCR_OK;
}

int focr_last_timings(focr_ctx_t *c, float ms[N_TIMINGS]) {
    if (!c || !ms) return FOCR_ERR_INVALID;
    if (int rc = finish_results(c)) return rc;
    for (int i = 0; i < N_TIMINGS; i++) ms[i] = c->ms[i];
    return FOCR_OK;
}

int focr_last_counters(focr_ctx_t *c, uint64_t out[N_COUNTERS]) {
    if (!c || !out) return FOCR_ERR_INVALID;
    if (int rc = finish_results(c)) return rc;
    for (int i = 0; i < N_COUNTERS; i++) out[i] = c->counters[i];
    return FOCR_OK;
}

int focr_debug_rnorm(focr_ctx_t *c, const uint32_t *s, const uint64_t *s2, const uint32_t *n, size_t n_items, double *out) {
    if (!c || !s || !s2 || !n || !out) return fail(c, FOCR_ERR_INVALID, "focr_debug_rnorm: bad arguments");
    FOCR_HIP(c, hipSetDevice(c->device));
    DevArray<uint32_t> ds, dn;
    DevArray<uint64_t> ds2;
    DevArray<double> dout;
    FOCR_HIP(c, ds.reserve(n_items, Grow::exact, nullptr));
    FOCR_HIP(c, dn.reserve(n_items, Grow::exact, nullptr));
    FOCR_HIP(c, ds2.reserve(n_items, Grow::exact, nullptr));
    FOCR_HIP(c, dout.reserve(n_items, Grow::exact, nullptr));
    FOCR_HIP(c, hipMemcpyAsync(ds, s, n_items * 4, hipMemcpyHostToDevice, c->stream));
    FOCR_HIP(c, hipMemcpyAsync(dn, n, n_items * 4, hipMemcpyHostToDevice, c->stream));
    FOCR_HIP(c, hipMemcpyAsync(ds2, s2, n_items * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(debug_rnorm_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, c->stream, ds.p, ds2.p, dn.p, n_items, dout.p);
    FOCR_HIP(c, hipGetLastError());
    FOCR_HIP(c, hipMemcpyAsync(out, dout, n_items * 8, hipMemcpyDeviceToHost, c->stream));
    FOCR_HIP(c, hipStreamSynchronize(c->stream));
    return FOCR_OK;
}

}  // extern "C"
