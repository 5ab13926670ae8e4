// pages.hip — the resident page sets: allocation, ingest of uploaded pages, the executor's alternate set, page-locked host memory
// (include/focr_ncc.h layer 2).
#include <algorithm>

#include "common.h"

namespace focr {

// tight luma8 pages -> pitched ink-high pages (image_to_u8, src/ncc.rs:887-892, on the device) + their int8 copy.
// One workgroup of 64 threads per page row; 4 pixels per thread and step when the rows are dword-aligned, else bytes.
__global__ __launch_bounds__(64) void ingest_pages(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint8_t *__restrict__ dst_i8, uint32_t r_w,
                                                   uint32_t r_h, size_t pitch, size_t rows_alloc, size_t first, size_t n_rows, int invert, int dwords) {
    const uint32_t flip = invert ? 0xffffffffu : 0u;
    for (size_t row = blockIdx.x; row < n_rows; row += gridDim.x) {
        const size_t p = row / r_h, y = row % r_h;
        const uint8_t *s = src + row * r_w;
        const size_t o = ((first + p) * rows_alloc + y) * pitch;
        if (dwords) {  // r_w % 4 == 0 and src 4-byte aligned (pitch is a multiple of 64)
            for (uint32_t x = threadIdx.x; x < r_w / 4; x += 64) {
                const uint32_t v = reinterpret_cast<const uint32_t *>(s)[x] ^ flip;  // 255 - v per byte
                reinterpret_cast<uint32_t *>(dst + o)[x] = v;
                reinterpret_cast<uint32_t *>(dst_i8 + o)[x] = v ^ 0x80808080u;  // ink - 128 as int8: the prefilter's operand
            }
        } else {
            for (uint32_t x = threadIdx.x; x < r_w; x += 64) {
                const uint8_t v = (uint8_t)(s[x] ^ (uint8_t)flip);
                dst[o + x] = v;
                dst_i8[o + x] = v ^ 0x80;
            }
        }
    }
}

// A fresh set of n pages of r_w x r_h, all paper: every row is followed by >= 64 zero bytes, every page by 48 zero rows (0x80 in
// the int8 copy), written on stream s.  The caller has made sure nothing reads the set's previous arrays.  On failure the set is empty.
static hipError_t page_set_alloc(focr_ctx::PageSet &ps, size_t n, size_t r_w, size_t r_h, hipStream_t s) {
    ps = {};
    const size_t pitch = (r_w + 64 + 63) / 64 * 64, rows_alloc = r_h + 48, bytes = n * rows_alloc * pitch;
    if (ps.u8.reserve(bytes, Grow::exact, nullptr) || ps.i8.reserve(bytes, Grow::exact, nullptr)) {
        ps = {};
        return hipErrorOutOfMemory;  // (whatever the allocator said: the callers report "hipMalloc failed", as they always did)
    }
    hipError_t e = hipMemsetAsync(ps.u8, 0, bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(ps.i8, 0x80, bytes, s);  // paper (0) as int8
    if (e != hipSuccess) {
        ps = {};
        return e;
    }
    ps.capacity = n, ps.r_w = r_w, ps.r_h = r_h, ps.pitch = pitch, ps.rows_alloc = rows_alloc;
    return hipSuccess;
}

// `count` tight luma8 pages at d_src (device memory) -> pages [first, first + count) of the set, on stream s
static hipError_t page_set_ingest(const focr_ctx::PageSet &ps, const uint8_t *d_src, size_t first, size_t count, int invert, hipStream_t s) {
    const size_t n_rows = count * ps.r_h;
    const unsigned blocks = (unsigned)std::min<size_t>(n_rows, (size_t)1 << 20);
    const int dwords = ps.r_w % 4 == 0 && (reinterpret_cast<uintptr_t>(d_src) & 3) == 0;
    hipLaunchKernelGGL(ingest_pages, dim3(blocks), dim3(64), 0, s, d_src, ps.u8.p, ps.i8.p, (uint32_t)ps.r_w, (uint32_t)ps.r_h, ps.pitch, ps.rows_alloc, first,
                       n_rows, invert, dwords);
    return hipGetLastError();
}

}  // namespace focr

using namespace focr;

extern "C" {

int focr_pages_alloc(focr_ctx_t *c, size_t n_pages, size_t r_w, size_t r_h) {
    if (!c || !n_pages || !r_w || !r_h) return fail(c, FOCR_ERR_INVALID, "focr_pages_alloc: bad arguments");
    if (r_w > 65535 || r_h > 65535)  // Match.x/y and start_end are u16, src/ncc.cpp:7-10, src/ncc.rs:313-314
        return fail(c, FOCR_ERR_INVALID, "focr_pages_alloc: page side above 65535 px");
    if (n_pages > 65535) return fail(c, FOCR_ERR_INVALID, "focr_pages_alloc: more than 65535 pages per batch");
    FOCR_HIP(c, hipSetDevice(c->device));
    c->results_gone();  // (pending sizes included: a later focr_sync must not complete a batch whose pages are gone)
    c->n_pages = n_pages;
    if (c->pages.holds(n_pages, r_w, r_h)) return FOCR_OK;  // same geometry, no more pages than before: keep the buffer (its zero padding is never written)
    FOCR_HIP(c, hipStreamSynchronize(c->stream));
    const hipError_t e = page_set_alloc(c->pages, n_pages, r_w, r_h, c->stream);
    if (e != hipSuccess) c->n_pages = 0;
    if (e == hipErrorOutOfMemory) return fail(c, FOCR_ERR_NOMEM, "focr_pages_alloc: hipMalloc failed");
    FOCR_HIP(c, e);
    return FOCR_OK;
}

static int ingest(focr_ctx *c, const uint8_t *d_src, size_t first, size_t count, int invert) {
    FOCR_HIP(c, page_set_ingest(c->pages, d_src, first, count, invert, c->stream));
    c->results_gone();  // results of the previous batch are gone with its pages
    return FOCR_OK;
}

}  // extern "C"

namespace focr {

// The executor's early ingest (pipe.hip): n_pages tight luma8 pages at d_luma (device memory) become the ALTERNATE page set of the
// context, on stream s — not the context's own: the context may be scanning its current pages meanwhile.  The caller orders s behind
// the arrival of d_luma and the context's stream behind s (an event) before pages_alt_swap makes the set current.  The alternate set
// is free whenever this is called: it was current two batches ago, and every batch of a lane ends with focr_sync.
int pages_alt_ingest(focr_ctx *c, const void *d_luma, size_t n_pages, size_t r_w, size_t r_h, int invert, hipStream_t s) {
    if (!c || !d_luma || !n_pages || !r_w || !r_h || r_w > 65535 || r_h > 65535 || n_pages > 65535)
        return fail(nullptr, FOCR_ERR_INVALID, "pages_alt_ingest: bad arguments");
    // (errors go to the process-wide message only: the context's own belongs to the lane's thread, which may be running a batch)
    if (!c->alt.holds(n_pages, r_w, r_h)) {  // (freeing the old set waits for the device: a change of geometry, not the steady state)
        const hipError_t e = page_set_alloc(c->alt, n_pages, r_w, r_h, s);
        if (e == hipErrorOutOfMemory) return fail(nullptr, FOCR_ERR_NOMEM, "pages_alt_ingest: hipMalloc failed");
        FOCR_HIP((focr_ctx *)nullptr, e);
    }
    FOCR_HIP((focr_ctx *)nullptr, page_set_ingest(c->alt, (const uint8_t *)d_luma, 0, n_pages, invert, s));
    return FOCR_OK;
}

// The alternate set becomes the context's pages (n_pages of r_w x r_h, as ingested by pages_alt_ingest), the previous pages the
// alternate set.  Host state only: the caller has ordered the context's stream behind the ingest.
int pages_alt_swap(focr_ctx *c, size_t n_pages, size_t r_w, size_t r_h) {
    if (!c->alt.holds(n_pages, r_w, r_h)) return fail(c, FOCR_ERR_STATE, "pages_alt_swap: no such alternate page set");
    std::swap(c->pages, c->alt);
    c->n_pages = n_pages;
    c->results_gone();  // results of the previous batch are gone with its pages
    return FOCR_OK;
}

}  // namespace focr

extern "C" {

int focr_pages_upload(focr_ctx_t *c, size_t first, size_t count, const uint8_t *luma, int invert) {
    if (!c || !luma) return fail(c, FOCR_ERR_INVALID, "focr_pages_upload: bad arguments");
    if (!c->pages.u8) return fail(c, FOCR_ERR_STATE, "focr_pages_upload: call focr_pages_alloc first");
    if (first + count > c->n_pages) return fail(c, FOCR_ERR_INVALID, "focr_pages_upload: page range out of bounds");
    FOCR_HIP(c, hipSetDevice(c->device));
    const size_t page_bytes = c->pages.r_w * c->pages.r_h;
    const size_t chunk_pages = std::max<size_t>(1, (256u << 20) / page_bytes);
    size_t need = std::min(count, chunk_pages) * page_bytes;
    FOCR_HIP(c, c->d_stage.reserve(need, Grow::exact, &c->stream));
    for (size_t done = 0; done < count; done += chunk_pages) {
        size_t n = std::min(chunk_pages, count - done);
        FOCR_HIP(c, hipMemcpyAsync(c->d_stage, luma + done * page_bytes, n * page_bytes, hipMemcpyHostToDevice, c->stream));
        int rc = ingest(c, c->d_stage, first + done, n, invert);
        if (rc) return rc;
        if (done + chunk_pages < count) FOCR_HIP(c, hipStreamSynchronize(c->stream));  // staging buffer reuse
    }
    return FOCR_OK;
}

int focr_host_alloc(size_t bytes, void **out) {
    if (!out || !bytes) return fail(nullptr, FOCR_ERR_INVALID, "focr_host_alloc: bad arguments");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        *out = nullptr;
        return fail(nullptr, e == hipErrorOutOfMemory ? FOCR_ERR_NOMEM : FOCR_ERR_NO_DEVICE,
                    std::string("focr_host_alloc: ") + hipGetErrorString(e));
    }
    return FOCR_OK;
}

void focr_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

int focr_host_register(void *p, size_t bytes) {
    if (!p || !bytes) return fail(nullptr, FOCR_ERR_INVALID, "focr_host_register: bad arguments");
    hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) return fail(nullptr, FOCR_ERR_NO_DEVICE, std::string("focr_host_register: ") + hipGetErrorString(e));
    return FOCR_OK;
}

void focr_host_unregister(void *p) {
    if (p) (void)hipHostUnregister(p);
}

int focr_pages_upload_device(focr_ctx_t *c, size_t first, size_t count, const void *d_luma, int invert) {
    if (!c || !d_luma) return fail(c, FOCR_ERR_INVALID, "focr_pages_upload_device: bad arguments");
    if (!c->pages.u8) return fail(c, FOCR_ERR_STATE, "focr_pages_upload_device: call focr_pages_alloc first");
    if (first + count > c->n_pages) return fail(c, FOCR_ERR_INVALID, "focr_pages_upload_device: page range out of bounds");
    FOCR_HIP(c, hipSetDevice(c->device));
    return ingest(c, (const uint8_t *)d_luma, first, count, invert);
}

}  // extern "C"
