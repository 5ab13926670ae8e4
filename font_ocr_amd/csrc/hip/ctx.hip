// ctx.hip — the error store, context life cycle and setters, per-launch timing, bank upload (include/focr_ncc.h layer 2).
// Resident pages: pages.hip.  The scan driver and every result getter: results.hip.
// The context's device memory is DevArray members (devmem.h, common.h): nothing here frees a buffer by name.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

#include "common.h"

namespace focr {

static std::mutex g_err_mu;
static std::string g_err;

void set_global_error(const std::string &s) {
    std::lock_guard<std::mutex> lk(g_err_mu);
    g_err = s;
}

int fail(focr_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg;
    set_global_error(msg);
    return code;
}

static void free_bank(focr_ctx *c) {
    c->bank = {};
    c->n_templates = 0;
}

}  // namespace focr

using namespace focr;

void focr_ctx::launch_begin(const char *name, uint32_t n_t, uint64_t alg, uint64_t issued, uint32_t super_index) {
    focr_launch_info_t li{};
    snprintf(li.name, sizeof li.name, "%s", name);
    li.n_templates = n_t;
    li.alg_macs = alg;
    li.issued_macs = issued;
    launches.push_back(li);
    launch_super.push_back(super_index);
    while (launch_events.size() < 2 * launches.size()) {
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        launch_events.push_back(e);
    }
    (void)hipEventRecord(launch_events[2 * (launches.size() - 1)], stream);
}

void focr_ctx::launch_end() { (void)hipEventRecord(launch_events[2 * (launches.size() - 1) + 1], stream); }

void focr_ctx::launches_collect() {
    for (size_t i = 0; i < launches.size(); i++)
        if (hipEventElapsedTime(&launches[i].ms, launch_events[2 * i], launch_events[2 * i + 1]) != hipSuccess) launches[i].ms = 0.f;
}

extern "C" {

const char *focr_last_error_global(void) {
    static thread_local std::string copy;
    std::lock_guard<std::mutex> lk(g_err_mu);
    copy = g_err;
    return copy.c_str();
}

const char *focr_last_error(const focr_ctx_t *ctx) { return ctx ? ctx->err.c_str() : focr_last_error_global(); }

int focr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int focr_ctx_create(int device, focr_ctx_t **out) {
    if (!out) return fail(nullptr, FOCR_ERR_INVALID, "focr_ctx_create: null out");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, FOCR_ERR_NO_DEVICE,
                    std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0") +
                        "); this library has no CPU fallback");
    if (device < 0 || device >= n) return fail(nullptr, FOCR_ERR_INVALID, "focr_ctx_create: bad device index");
    focr_ctx *c = new focr_ctx();
    c->device = device;
    auto init = [&]() -> int {
        FOCR_HIP(c, hipSetDevice(device));
        int cus = 0;
        FOCR_HIP(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        c->n_cus = (unsigned)std::max(cus, 1);
        FOCR_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->io_stream = c->stream;
        phase_origin_record(device, c->stream);
        for (auto &ev : c->ev) FOCR_HIP(c, hipEventCreate(&ev));
        for (auto &ev : c->vimg_ev) FOCR_HIP(c, hipEventCreate(&ev));
        for (auto &ev : c->run_ev) FOCR_HIP(c, hipEventCreate(&ev));
        FOCR_HIP(c, c->d_counter.reserve(COUNTER_BYTES / sizeof(uint32_t), Grow::exact, nullptr));
        FOCR_HIP(c, hipMemsetAsync(c->d_counter, 0, COUNTER_BYTES, c->stream));
        FOCR_HIP(c, c->d_res.reserve(1, Grow::exact, nullptr));
        FOCR_HIP(c, hipMemsetAsync(c->d_res, 0, sizeof(ResultBlock), c->stream));
        FOCR_HIP(c, hipHostMalloc((void **)&c->h_res, sizeof(ResultBlock), hipHostMallocDefault));
        FOCR_HIP(c, hipHostMalloc((void **)&c->h_live, LIVE_WORDS * sizeof(uint32_t), hipHostMallocDefault));
        memset(c->h_res, 0, sizeof(ResultBlock));
        memset(c->h_live, 0, LIVE_WORDS * sizeof(uint32_t));
        return FOCR_OK;
    };
    int rc = init();
    if (rc != FOCR_OK) {  // the message is already in focr_last_error_global()
        focr_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return FOCR_OK;
}

void focr_ctx_destroy(focr_ctx_t *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->h_res) (void)hipHostFree(c->h_res);
    if (c->h_live) (void)hipHostFree(c->h_live);
    for (auto &ev : c->ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto &ev : c->vimg_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto &ev : c->run_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto &ev : c->launch_events)
        if (ev) (void)hipEventDestroy(ev);
    if (c->stream && c->owns_stream) (void)hipStreamDestroy(c->stream);
    delete c;  // every device array of the context dies here, behind the wait above
}

size_t focr_debug_device_bytes(void) { return g_device_bytes.load(); }

int focr_ctx_set_scan_cus(focr_ctx_t *c, unsigned max_cus) {
    if (!c) return fail(c, FOCR_ERR_INVALID, "focr_ctx_set_scan_cus: null context");
    c->scan_cus = max_cus;
    return FOCR_OK;
}

int focr_ctx_set_prefilter(focr_ctx_t *c, int mode) {
    if (!c || (mode != FOCR_PREFILTER_AUTO && mode != FOCR_PREFILTER_ONE_STAGE && mode != FOCR_PREFILTER_LEGACY))
        return fail(c, FOCR_ERR_INVALID, "focr_ctx_set_prefilter: bad arguments");
    c->prefilter = mode;
    return FOCR_OK;
}

int focr_ctx_set_row_tail(focr_ctx_t *c, int on) {
    if (!c) return fail(c, FOCR_ERR_INVALID, "focr_ctx_set_row_tail: null context");
    if (on < 0 || on > 1) return fail(c, FOCR_ERR_INVALID, "focr_ctx_set_row_tail: 0 (legacy tail) or 1 (hits-first row tail, the default)");
    c->tail_mode = on;
    c->est.reset();  // the next scan runs with exact sizes
    return FOCR_OK;
}

int focr_ctx_set_column_drop(focr_ctx_t *c, int on) {
    if (!c) return fail(c, FOCR_ERR_INVALID, "focr_ctx_set_column_drop: null context");
    c->column_drop = on != 0;
    return FOCR_OK;
}

int focr_debug_force_split(focr_ctx_t *c, int on) {
    if (!c) return FOCR_ERR_INVALID;
    c->force_split = on != 0;
    return FOCR_OK;
}

int focr_debug_set_tail_grid(focr_ctx_t *c, uint32_t num, uint32_t den) {
    if (!c) return FOCR_ERR_INVALID;
    c->dbg_grid_num = num;
    c->dbg_grid_den = den;
    return FOCR_OK;
}

int focr_debug_set_stats_form(focr_ctx_t *c, int form) {
    if (!c || form < 0 || form > 1) return FOCR_ERR_INVALID;
    c->dbg_stats_form = form;
    return FOCR_OK;
}

int focr_debug_set_verify_form(focr_ctx_t *c, int form) {
    if (!c || form < 0 || form > 1) return FOCR_ERR_INVALID;
    c->dbg_verify_form = form;
    return FOCR_OK;
}

int focr_sync(focr_ctx_t *c) {
    if (!c) return FOCR_ERR_INVALID;
    FOCR_HIP(c, hipSetDevice(c->device));
    if (c->sizes_pending || c->post_pending) return finish_results(c);  // waits for the batch itself
    return wait_batch(c);
}

int focr_bank_upload(focr_ctx_t *c, const focr_template_t *templates, size_t n_templates, const uint8_t *needles,
                     size_t needles_len) {
    if (!c || !templates || !n_templates || !needles) return fail(c, FOCR_ERR_INVALID, "focr_bank_upload: bad arguments");
    if (n_templates > 65535) return fail(c, FOCR_ERR_INVALID, "focr_bank_upload: more than 65535 templates");
    for (size_t t = 0; t < n_templates; t++) {
        const focr_template_t &d = templates[t];
        if (d.n_w == 0 || d.n_h == 0) return fail(c, FOCR_ERR_INVALID, "focr_bank_upload: empty template");
        if (d.n_w > 32)  // the reference panics above 16 ("not handled", src/ncc.rs:392); 17..32 is this build's extension
            return fail(c, FOCR_ERR_INVALID, "focr_bank_upload: template wider than 32 px is not handled");
        if (d.n_h > 255) return fail(c, FOCR_ERR_INVALID, "focr_bank_upload: template taller than 255 px is not handled");
        if ((size_t)d.offset + (size_t)d.n_w * d.n_h > needles_len)
            return fail(c, FOCR_ERR_INVALID, "focr_bank_upload: template offset out of range");
    }
    FOCR_HIP(c, hipSetDevice(c->device));
    FOCR_HIP(c, hipStreamSynchronize(c->stream));
    free_bank(c);
    c->results_gone();
    c->bank_gen++;
    {  // content id of the bank (FNV-1a over the records and the pixels): contexts that hold the same bank share their size estimates
        uint64_t h = 1469598103934665603ull;
        auto mix = [&](const void *p, size_t n) {
            const uint8_t *b = (const uint8_t *)p;
            for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
        };
        for (size_t t = 0; t < n_templates; t++) {
            const focr_template_t &d = templates[t];
            const uint32_t rec[3] = {d.letter, (uint32_t)d.n_w << 16 | d.n_h, d.offset};
            mix(rec, sizeof rec);
        }
        mix(needles, needles_len);
        c->bank_hash = h ^ (uint64_t)c->column_drop;
    }
    std::vector<uint32_t> direct;
    std::vector<uint8_t> dense;
    bank_host_prepare(c, templates, n_templates, needles, direct, dense);
    std::vector<uint32_t> tw(n_templates), th(n_templates), tl(n_templates);
    for (size_t t = 0; t < n_templates; t++) {
        tw[t] = templates[t].n_w;
        th[t] = templates[t].n_h;
        tl[t] = templates[t].letter;
    }
    focr_ctx::Bank &b = c->bank;
    if (int rc = c->upload(b.d_tconst, b.h_tconst.data(), b.h_tconst.size())) return rc;
    if (int rc = c->upload(b.d_direct_bank, direct.data(), direct.size())) return rc;
    if (int rc = c->upload(b.d_needles, dense.data(), dense.size())) return rc;
    if (int rc = c->upload(b.d_needle_off, b.h_needle_off.data(), b.h_needle_off.size())) return rc;
    if (int rc = c->upload(b.d_t_w, tw.data(), tw.size())) return rc;
    if (int rc = c->upload(b.d_t_h, th.data(), th.size())) return rc;
    if (int rc = c->upload(b.d_t_letter, tl.data(), tl.size())) return rc;
    return build_mfma_bank(c, dense.data());
}

}  // extern "C"

namespace focr {
// Host-only part of the bank upload: size classes, class order, per-template constants, dense / direct-kernel needles.
void bank_host_prepare(focr_ctx *c, const focr_template_t *templates, size_t n_templates, const uint8_t *needles,
                       std::vector<uint32_t> &direct, std::vector<uint8_t> &dense) {
    c->n_templates = n_templates;
    c->bank.h_templates.assign(templates, templates + n_templates);

    // size classes in order of first appearance
    std::vector<std::vector<uint32_t>> members;
    for (size_t t = 0; t < n_templates; t++) {
        size_t k = 0;
        for (; k < c->bank.classes.size(); k++)
            if (c->bank.classes[k].n_w == templates[t].n_w && c->bank.classes[k].n_h == templates[t].n_h) break;
        if (k == c->bank.classes.size()) {
            SizeClass sc{};
            sc.n_w = templates[t].n_w;
            sc.n_h = templates[t].n_h;
            sc.ndw = (sc.n_w + 3) / 4;
            sc.tall = sc.n_h > 32 || sc.n_w > 16;
            sc.maxh = sc.tall ? sc.n_h : (sc.n_h <= 16 ? 16 : 32);
            c->bank.classes.push_back(sc);
            members.emplace_back();
        }
        members[k].push_back((uint32_t)t);
    }

    // Inside a class, order templates by (letter, shift): the sub-pixel variants of one glyph fire on the
    // same windows, so they should share a 16-template MFMA N-tile (fewer prefilter slow-path visits).
    // Results are keyed by the global template index, so this order is invisible to callers.
    for (auto &mem : members)
        std::stable_sort(mem.begin(), mem.end(), [&](uint32_t a, uint32_t b) {
            if (templates[a].letter != templates[b].letter) return templates[a].letter < templates[b].letter;
            if (templates[a].shift_x != templates[b].shift_x) return templates[a].shift_x < templates[b].shift_x;
            return templates[a].shift_y < templates[b].shift_y;
        });

    uint32_t first = 0;
    for (size_t k = 0; k < c->bank.classes.size(); k++) {
        SizeClass &sc = c->bank.classes[k];
        sc.first = first;
        sc.n_templates = (uint32_t)members[k].size();
        first += sc.n_templates;
        c->bank.direct_bank_off.push_back(direct.size());
        const uint32_t n = sc.n_w * sc.n_h;
        for (uint32_t t : members[k]) {
            const uint8_t *nd = needles + templates[t].offset;
            // reference kernel prologue, src/ncc.cpp:73-86 / 278-291 (host IEEE double)
            uint32_t s_n = 0, s2_n = 0;
            for (uint32_t i = 0; i < n; i++) {
                s_n += nd[i];
                s2_n += (uint32_t)nd[i] * nd[i];
            }
            double norm2_n = (double)s2_n - (double)((uint64_t)s_n * (uint64_t)s_n) / (double)n;
            TemplateConst tc{};
            tc.s_n = (double)s_n;
            tc.n_recip = 1. / (double)n;
            tc.rnorm_n = 1. / std::sqrt(norm2_n);
            tc.norm2_n = norm2_n;
            tc.index = t;
            tc.n_w = sc.n_w;
            tc.n_h = sc.n_h;
            c->bank.h_tconst.push_back(tc);
            // direct-kernel layout: maxh rows of ndw dwords, zero padded
            for (uint32_t j = 0; j < sc.maxh; j++)
                for (uint32_t k4 = 0; k4 < sc.ndw; k4++) {
                    uint32_t w = 0;
                    for (uint32_t b = 0; b < 4; b++) {
                        uint32_t i = k4 * 4 + b;
                        if (j < sc.n_h && i < sc.n_w) w |= (uint32_t)nd[j * sc.n_w + i] << (8 * b);
                    }
                    direct.push_back(w);
                }
            c->bank.h_needle_off.push_back((uint32_t)dense.size());
            dense.insert(dense.end(), nd, nd + n);
        }
    }
}

// The context joins a lane of an executor (pipe.hip): it works on the lane's stream from now on (its own, idle, is destroyed) and reads
// results back on the lane's side stream.
void ctx_share_stream(focr_ctx *c, hipStream_t lane_stream, hipStream_t io_stream) {
    (void)hipSetDevice(c->device);
    if (c->stream && c->owns_stream && c->stream != lane_stream) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamDestroy(c->stream);
    }
    c->owns_stream = false;
    c->stream = lane_stream;
    c->io_stream = io_stream ? io_stream : lane_stream;
}

// Until the work this context has queued is done.  Inside an executor that is the context's OWN batch (the event the executor
// recorded behind its last kernel; consumed here) — the lane's stream already holds the next batch of another context; a context
// with a stream of its own waits for the stream.
int wait_batch(focr_ctx *c) {
    if (c->batch_event) {
        hipEvent_t e = c->batch_event;
        c->batch_event = nullptr;
        FOCR_HIP(c, hipEventSynchronize(e));
        return FOCR_OK;
    }
    FOCR_HIP(c, hipStreamSynchronize(c->stream));
    return FOCR_OK;
}

}  // namespace focr
