// compat.hip — the reference's own FFI symbols on the GPU: ncc_8_u8 / ncc_16_u8
// (replaces src/ncc.cpp:48-251 and 253-396; declared in src/ncc.rs:92-126).
//
// One call = one template over one page, with the caller's window tables
// (patch_sum, patch_rnorm, start_end) honoured exactly as the reference kernel
// reads them.  The page and the tables stay resident per calling thread and are
// uploaded again only when their content changes (64-bit content hash), so the
// reference's own call pattern — hundreds of templates over one page — pays the
// 13 B/px of PCIe traffic once per page and size class, not once per call.
// Throughput proper goes through the batched API.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "common.h"

namespace focr {

typedef int v4i_c __attribute__((ext_vector_type(4), aligned(1)));
typedef int v2i_c __attribute__((ext_vector_type(2), aligned(1)));

// one lane per window (x, y), x in [start_y, end_y), y in [1, y_searches): the padded needle row (N = 8 or 16 bytes, zero
// past n_w as the caller built it, src/ncc.rs:925-935) against the N bytes at the window's row start, v_dot4_u32_u8.  Like the
// reference kernel the loads run up to N - n_w bytes past the window (src/ncc.cpp:315-318 loads 16 bytes whatever n_w is);
// those bytes meet the needle's zero padding.  d_ref carries 64 spare bytes behind the page.
template <int N>
__global__ __launch_bounds__(256) void compat_kernel(const uint8_t *__restrict__ ref, uint32_t r_w, uint32_t r_h,
                                                     const uint32_t *__restrict__ needle, uint32_t n_w, uint32_t n_h,
                                                     const uint32_t *__restrict__ patch_sum,
                                                     const double *__restrict__ patch_rnorm,
                                                     const uint16_t *__restrict__ start_end, double s_n, double n_recip,
                                                     double rnorm_n, double thr_d, uint64_t *__restrict__ hit_keys,
                                                     float *__restrict__ hit_sims, unsigned long long *__restrict__ counter,
                                                     unsigned long long capacity) {
    const uint32_t x = blockIdx.x * 256 + threadIdx.x;
    const uint32_t y = 1 + blockIdx.y;  // src/ncc.cpp:98, 302
    const uint32_t start = start_end[2 * y], end = start_end[2 * y + 1];
    if (x < start || x >= end || x + n_w > r_w) return;  // the last clause only guards insane caller tables
    uint32_t acc = 0;
    const uint8_t *r = ref + (size_t)y * r_w + x;
    for (uint32_t j = 0; j < n_h; j++, r += r_w) {
        const uint32_t *t = needle + j * (N / 4);  // uniform address: scalar loads
        if (N == 8) {
            const v2i_c w = *reinterpret_cast<const v2i_c *>(r);
            acc = __builtin_amdgcn_udot4((uint32_t)w[0], t[0], acc, false);
            acc = __builtin_amdgcn_udot4((uint32_t)w[1], t[1], acc, false);
        } else {
            const v4i_c w = *reinterpret_cast<const v4i_c *>(r);
#pragma unroll
            for (int k = 0; k < 4; k++) acc = __builtin_amdgcn_udot4((uint32_t)w[k], t[k], acc, false);
        }
    }
    const size_t o = (size_t)y * r_w + x;
    const double sim = ncc_similarity(acc, patch_sum[o], s_n, n_recip, rnorm_n, patch_rnorm[o]);
    if (ncc_emits(sim, thr_d)) {
        unsigned long long idx = atomicAdd(counter, 1ull);
        if (idx < capacity) {
            hit_keys[idx] = ((uint64_t)y << 16) | (uint64_t)x;
            hit_sims[idx] = (float)sim;
        }
    }
}

__global__ void compat_pack(const uint64_t *__restrict__ keys, const float *__restrict__ sims, size_t n,
                            focr_match_t *__restrict__ out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    focr_match_t m;
    m.x = (uint16_t)(keys[i] & 0xffff);
    m.y = (uint16_t)((keys[i] >> 16) & 0xffff);
    m.similarity = sims[i];
    out[i] = m;
}

// 64-bit content hash: 8 independent multiply-xorshift lanes over 8-byte words (the multiplies of eight lanes overlap: 14-25 GB/s
// on one core, twice the four-lane form of rounds 1-4) — ~0.25 ms for the 5.7 MB a 608x720 page's inputs have, against ~2 ms to
// push them over PCIe from pageable memory.  Still the largest item of a call (the kernel itself takes a few microseconds).
static uint64_t content_hash(const void *p, size_t n) {
    const uint8_t *b = (const uint8_t *)p;
    uint64_t h[8] = {0x9e3779b97f4a7c15ull, 0xbf58476d1ce4e5b9ull, 0x94d049bb133111ebull, 0x2545f4914f6cdd1dull,
                     0xd6e8feb86659fd93ull, 0xa0761d6478bd642full, 0xe7037ed1a0b428dbull, 0x8ebc6af09c88c6e3ull};
    auto block = [&](const uint8_t *src) {
        uint64_t v[8];
        memcpy(v, src, 64);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            h[k] = (h[k] ^ v[k]) * 0x9fb21c651e98df25ull;
            h[k] ^= h[k] >> 29;
        }
    };
    size_t i = 0;
    for (; i + 64 <= n; i += 64) block(b + i);
    if (i < n) {  // the last n % 64 bytes, zero-padded to a block of their own: every byte keeps its position (the length is mixed in below)
        uint8_t last[64] = {0};
        memcpy(last, b + i, n - i);
        block(last);
    }
    uint64_t r = (uint64_t)n * 0xd6e8feb86659fd93ull;
    for (int k = 0; k < 8; k++) r = (r ^ h[k]) * 0x9fb21c651e98df25ull + (uint64_t)k;
    r ^= r >> 32;
    r *= 0xd6e8feb86659fd93ull;
    return r ^ (r >> 29);
}

struct CompatState {
    focr_ctx *ctx = nullptr;
    // what is resident on the device: the reference's host calls ncc_N_u8 once per template with the SAME page, and the
    // same window tables for every template of a size class (src/ncc.rs:264-268, 332-404), so each input is hashed and
    // uploaded again only when its content (or geometry) changed
    uint64_t h_ref = 0, h_ps = 0, h_pr = 0, h_se = 0;
    size_t res_w = 0, res_h = 0;
    DevArray<uint8_t> d_ref, d_needle;  // (all exact growth, behind the context's stream)
    DevArray<uint32_t> d_ps;
    DevArray<double> d_pr;
    DevArray<uint16_t> d_se;
    DevArray<focr_match_t> d_out;
    // the call's hits land in page-locked host memory as the kernel finds them (a call emits tens to a few thousand): ONE wait per
    // call, then a host sort of those few — instead of a count read-back, a device radix sort (a dozen launches), a pack kernel and
    // a second read-back.  A call with more hits than the block holds takes the device path.
    unsigned long long *h_count = nullptr;  // [0]: hits found (copied out of device memory behind the kernel)
    uint64_t *h_keys = nullptr;
    float *h_sims = nullptr;
    static constexpr size_t PIN_HITS = 1u << 16;
};

// One per thread, deliberately never destroyed (its arrays stay live, and counted, past the thread's end): thread-exit / process-exit
// order against the HIP runtime's own teardown is unspecified, and the driver reclaims everything anyway.
static thread_local CompatState &tl = *new CompatState;

template <int N>
static size_t compat_call(uint8_t *reference, size_t r_w, size_t r_h, uint8_t *needle_u8, size_t n_w, size_t n_h,
                          uint32_t *acc, size_t acc_len, uint32_t *patch_sum, double *patch_rnorm, uint16_t *start_end,
                          float threshold, focr_match_t *out, size_t n_out) {
    if (acc && acc_len) memset(acc, 0, sizeof(uint32_t) * acc_len);  // src/ncc.cpp:67, 272
    if (!reference || !needle_u8 || !patch_sum || !patch_rnorm || !start_end || !out || n_out == 0) {
        set_global_error("ncc_N_u8: null argument or n_out == 0");
        return 0;
    }
    if (n_w == 0 || n_w > (size_t)N || n_h == 0 || n_h > r_h || n_w > r_w || r_w > 65535 || r_h > 65535) {
        set_global_error("ncc_N_u8: unsupported geometry");
        return 0;
    }
    const size_t y_searches = r_h - n_h + 1;
    if (y_searches <= 1) return 0;
    if (!tl.ctx) {
        int dev = 0;
        if (const char *e = getenv("FOCR_DEVICE")) dev = atoi(e);
        if (focr_ctx_create(dev, &tl.ctx) != FOCR_OK) {
            tl.ctx = nullptr;
            return 0;  // focr_last_error_global() has the reason; no CPU fallback
        }
    }
    focr_ctx *c = tl.ctx;
    auto bail = [&](const char *what, hipError_t e) -> size_t {
        fail(c, FOCR_ERR_NO_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
        return 0;
    };
#define CK(expr)                                   \
    do {                                           \
        hipError_t e_ = (expr);                    \
        if (e_ != hipSuccess) return bail(#expr, e_); \
    } while (0)
    CK(hipSetDevice(c->device));
    const size_t npx = r_w * r_h;
    if (tl.d_ref.cap < npx + 64 || tl.d_ps.cap < npx || tl.d_pr.cap < npx) {  // any of the three (a grow that failed half-way leaves them unequal)
        tl.res_w = tl.res_h = 0;  // nothing is resident from here on, whether the grow succeeds or not
        CK(tl.d_ref.reserve(npx + 64, Grow::exact, &c->stream));
        CK(hipMemsetAsync(tl.d_ref, 0, npx + 64, c->stream));
        CK(tl.d_ps.reserve(npx, Grow::exact, &c->stream));
        CK(tl.d_pr.reserve(npx, Grow::exact, &c->stream));
    }
    if (tl.d_se.cap < r_h * 2) {
        tl.res_w = tl.res_h = 0;
        CK(tl.d_se.reserve(r_h * 2, Grow::exact, &c->stream));
    }
    CK(tl.d_needle.reserve(16 * 65536, Grow::exact, nullptr));
    if (n_h * N > 16 * 65536) {
        set_global_error("ncc_N_u8: needle too tall");
        return 0;
    }

    // kernel prologue, src/ncc.cpp:73-86 / 278-291, in host IEEE double
    uint32_t s_n = 0, s2_n = 0;
    for (size_t i = 0; i < n_h; i++)
        for (size_t j = 0; j < (size_t)N; j++) {
            s_n += needle_u8[i * N + j];
            s2_n += (uint32_t)needle_u8[i * N + j] * (uint32_t)needle_u8[i * N + j];
        }
    const size_t n = n_w * n_h;
    const double norm2_n = (double)s2_n - (double)((uint64_t)s_n * (uint64_t)s_n) / (double)n;
    const double rnorm_n = 1. / std::sqrt(norm2_n);
    const double n_recip = 1. / (double)n;

    {
        // Residency rests on a 64-bit NON-cryptographic content hash of each input: two different pages (or tables) of one
        // geometry with equal hashes would be scanned with the stale copy — accepted for this plumbing path (the ABI has no
        // error channel and no generation counter to key on).  Every byte enters the hash through
        // a multiply of its own position's lane and block, the last n % 64 bytes included (a plain XOR fold of those would
        // not see two of them swapped), so unrelated inputs collide with probability ~2^-64 per pair; an input built to
        // collide still can.
        // FOCR_COMPAT_ALWAYS_UPLOAD=1 switches it off: every call re-uploads every input.
        static const bool always_upload = getenv("FOCR_COMPAT_ALWAYS_UPLOAD") != nullptr;
        const bool geo = always_upload || tl.res_w != r_w || tl.res_h != r_h;
        const uint64_t hr = always_upload ? 0 : content_hash(reference, npx), hs = always_upload ? 0 : content_hash(patch_sum, npx * 4),
                       hp = always_upload ? 0 : content_hash(patch_rnorm, npx * 8), he = always_upload ? 0 : content_hash(start_end, r_h * 2 * sizeof(uint16_t));
        if (geo || hr != tl.h_ref) CK(hipMemcpyAsync(tl.d_ref, reference, npx, hipMemcpyHostToDevice, c->stream));
        if (geo || hs != tl.h_ps) CK(hipMemcpyAsync(tl.d_ps, patch_sum, npx * 4, hipMemcpyHostToDevice, c->stream));
        if (geo || hp != tl.h_pr) CK(hipMemcpyAsync(tl.d_pr, patch_rnorm, npx * 8, hipMemcpyHostToDevice, c->stream));
        if (geo || he != tl.h_se) CK(hipMemcpyAsync(tl.d_se, start_end, r_h * 2 * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        tl.h_ref = hr, tl.h_ps = hs, tl.h_pr = hp, tl.h_se = he;
        tl.res_w = r_w, tl.res_h = r_h;
    }
    CK(hipMemcpyAsync(tl.d_needle, needle_u8, n_h * N, hipMemcpyHostToDevice, c->stream));

    if (!tl.h_count) {
        void *blk = nullptr;
        if (hipHostMalloc(&blk, 64 + CompatState::PIN_HITS * 12, hipHostMallocDefault) == hipSuccess) {
            tl.h_count = (unsigned long long *)blk;
            tl.h_keys = (uint64_t *)((char *)blk + 64);
            tl.h_sims = (float *)((char *)blk + 64 + CompatState::PIN_HITS * 8);
        }
    }
    if (tl.h_count) {  // the fast form: hits straight into page-locked host memory
        // (the counter stays in device memory — an atomic per hit across PCIe is neither fast nor everywhere supported — and is copied
        // out behind the kernel; the hits themselves are plain stores into the page-locked block)
        CK(hipMemsetAsync(c->d_counter, 0, 64 * sizeof(uint32_t), c->stream));
        dim3 grid((unsigned)((r_w + 255) / 256), (unsigned)(y_searches - 1));
        hipLaunchKernelGGL((compat_kernel<N>), grid, dim3(256), 0, c->stream, tl.d_ref, (uint32_t)r_w, (uint32_t)r_h,
                           tl.d_needle.as<const uint32_t>(), (uint32_t)n_w, (uint32_t)n_h, tl.d_ps, tl.d_pr, tl.d_se, (double)s_n, n_recip,
                           rnorm_n, (double)threshold, tl.h_keys, tl.h_sims, c->d_counter.as<unsigned long long>(), (unsigned long long)CompatState::PIN_HITS);
        CK(hipGetLastError());
        CK(hipMemcpyAsync(tl.h_count, c->d_counter, 8, hipMemcpyDeviceToHost, c->stream));
        CK(hipStreamSynchronize(c->stream));
        const unsigned long long cnt = *tl.h_count;
        if (cnt <= CompatState::PIN_HITS) {
            if (cnt == 0) return 0;
            // (y, x) order, src/ncc.cpp:302-375: the key is y << 16 | x
            std::vector<std::pair<uint64_t, float>> hits((size_t)cnt);
            for (size_t i = 0; i < (size_t)cnt; i++) hits[i] = {tl.h_keys[i], tl.h_sims[i]};
            std::sort(hits.begin(), hits.end(), [](const std::pair<uint64_t, float> &a, const std::pair<uint64_t, float> &b) { return a.first < b.first; });
            const size_t keep = std::min<size_t>((size_t)cnt, n_out);  // src/ncc.cpp:225-227, 371-373
            for (size_t i = 0; i < keep; i++) {
                out[i].x = (uint16_t)(hits[i].first & 0xffff);
                out[i].y = (uint16_t)((hits[i].first >> 16) & 0xffff);
                out[i].similarity = hits[i].second;
            }
            return keep;
        }
        // more hits than the block holds (very low thresholds): the device path below counts and sorts them all
    }
    size_t want = std::max<size_t>(c->d_hit_keys.cap, std::max<size_t>(1u << 16, n_out * 4));
    for (int attempt = 0; attempt < 3; attempt++) {
        if (reserve_hits(c, want) != FOCR_OK) return 0;
        CK(hipMemsetAsync(c->d_counter, 0, 64 * sizeof(uint32_t), c->stream));
        dim3 grid((unsigned)((r_w + 255) / 256), (unsigned)(y_searches - 1));
        hipLaunchKernelGGL((compat_kernel<N>), grid, dim3(256), 0, c->stream, tl.d_ref, (uint32_t)r_w, (uint32_t)r_h,
                           tl.d_needle.as<const uint32_t>(), (uint32_t)n_w, (uint32_t)n_h, tl.d_ps, tl.d_pr, tl.d_se, (double)s_n, n_recip,
                           rnorm_n, (double)threshold, c->d_hit_keys, c->d_hit_sims, c->d_counter.as<unsigned long long>(),
                           (unsigned long long)c->d_hit_keys.cap);
        CK(hipGetLastError());
        unsigned long long cnt = 0;
        CK(hipMemcpyAsync(&cnt, c->d_counter, 8, hipMemcpyDeviceToHost, c->stream));
        CK(hipStreamSynchronize(c->stream));
        if (cnt > c->d_hit_keys.cap) {
            want = (size_t)cnt + 1024;
            continue;
        }
        if (cnt == 0) return 0;
        if (sort_pairs_u64_f32(c, c->d_hit_keys, c->d_hit_keys_alt, c->d_hit_sims, c->d_hit_sims_alt, (size_t)cnt, 32) != FOCR_OK)
            return 0;
        const size_t keep = std::min<size_t>((size_t)cnt, n_out);  // src/ncc.cpp:225-227, 371-373
        CK(tl.d_out.reserve(keep, Grow::exact, &c->stream));
        hipLaunchKernelGGL(compat_pack, dim3((unsigned)((keep + 255) / 256)), dim3(256), 0, c->stream, c->d_hit_keys,
                           c->d_hit_sims, keep, tl.d_out);
        CK(hipGetLastError());
        CK(hipMemcpyAsync(out, tl.d_out, keep * sizeof(focr_match_t), hipMemcpyDeviceToHost, c->stream));
        CK(hipStreamSynchronize(c->stream));
        return keep;
    }
#undef CK
    set_global_error("ncc_N_u8: hit buffer kept overflowing");
    return 0;
}

}  // namespace focr

extern "C" {

size_t ncc_8_u8(uint8_t *reference, size_t r_w, size_t r_h, uint8_t *needle_u8, size_t n_w, size_t n_h, uint32_t *acc,
                size_t acc_len, uint32_t *patch_sum, double *patch_rnorm, uint16_t *start_end, float threshold,
                focr_match_t *out, size_t n_out) {
    return focr::compat_call<8>(reference, r_w, r_h, needle_u8, n_w, n_h, acc, acc_len, patch_sum, patch_rnorm, start_end,
                                threshold, out, n_out);
}

size_t ncc_16_u8(uint8_t *reference, size_t r_w, size_t r_h, uint8_t *needle_u8, size_t n_w, size_t n_h, uint32_t *acc,
                 size_t acc_len, uint32_t *patch_sum, double *patch_rnorm, uint16_t *start_end, float threshold,
                 focr_match_t *out, size_t n_out) {
    return focr::compat_call<16>(reference, r_w, r_h, needle_u8, n_w, n_h, acc, acc_len, patch_sum, patch_rnorm, start_end,
                                 threshold, out, n_out);
}

}  // extern "C"
