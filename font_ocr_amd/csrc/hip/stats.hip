// stats.hip — phase 1 of the fast scan (scan_mfma.hip): window statistics -> threshold planes, and the scan's work list.
//
// Per size class and window, the exact integer sums s_p, s2_p, V = n*s2 - s^2 (V > 0 <=> the
// reference's rnorm is finite, src/ncc.rs:309-311) and — for a class whose last column the MFMA does not multiply — that
// column's sums.  From them the window's prefilter THRESHOLD L(w) in f32 (mfma_common.h, "threshold planes"), stored as the
// MFMA's C-in in units of a per-class power of two, rounded TOWARDS -INF as a threshold ("threshold plane", an int16 per window
// and class); the most negative value where the reference never emits (x = 0, y = 0, out of range, zero variance => rnorm = inf/NaN).  A lower threshold only admits more
// candidates, so the directed rounding has no sign cases: the filter is conservative for negative --threshold too (round 2
// stored the window norm rounded towards zero and multiplied by kappa in the scan kernel, which RAISED the threshold for
// kappa < 0).  (Legacy form, still used for size classes with more than 4 K-steps: negL(w) = -(floor(L) - 2) as int32, or
// -REJECT.)  The kernel also marks every 16-window M-tile that has a live window; compact_live_tiles makes the work list.
//
// The driver sees two functions: launch_clear, the one launch in front of a scan's statistics (post.hip clears with it too), and
// pass_stats, which queues the statistics launches and the work list of one scan pass.
#include <algorithm>
#include <type_traits>

#include "mfma_common.h"

namespace focr {

// Everything a scan needs zeroed, in one launch (ClearList, common.h)
__global__ __launch_bounds__(256) void clear_kernel(const ClearList l) {
    const uint32_t tid = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
    for (uint32_t r = 0; r < l.n; r++) {
        uint64_t *p = reinterpret_cast<uint64_t *>(l.p[r]);
        for (uint32_t i = tid; i < l.n8[r]; i += step) p[i] = 0;
    }
}
int launch_clear(focr_ctx *c, const ClearList &l) {
    size_t words = 0;
    for (uint32_t r = 0; r < l.n; r++) words += l.n8[r];
    if (!words) return FOCR_OK;
    hipLaunchKernelGGL(clear_kernel, dim3((unsigned)std::min<size_t>(1024, (words + 1023) / 1024)), dim3(256), 0, c->stream, l);
    FOCR_HIP(c, hipGetLastError());
    return FOCR_OK;
}

// Separable sliding sums: a block stages a (64 + n_w) x (32 + n_h - 1) byte tile, computes the horizontal
// n_w-sums H (and H2 of squares) of every tile row once (v_dot4 on masked dwords), then each thread slides a
// vertical n_h-window down its column: S(y+1) = S(y) + H(y+n_h) - H(y).  ~40 instructions per window instead
// of ~300 for the direct evaluation.  Everything up to the square roots is exact integer arithmetic (V, W of
// mfma_common.h, "threshold planes"); window is live  <=>  V > 0, which is exactly the reference's "norm > 0"
// (src/ncc.rs:309: (f64)s2 - (f64)(s*s)/(f64)n is > 0 iff V > 0, = 0 iff V = 0, because V/n >= 1/n is far above the
// rounding error of the division).
//   DROP: the class's last column is bounded, not multiplied: the horizontal sums run over the KEPT width (round 5: two dwords
//         instead of three for BASELINE configs[1]'s 9-wide class) and the thread also slides the sums of the dropped column (bytes
//         of the tile) down; the full box's sums are the two added, W comes from both.
//   PAIR: the kept box is itself a size class of the pass (BASELINE configs[1]: 8x15 beside 9x15): its plane comes out of
//         the same launch (its statistics are the kept box's), one launch instead of two.
constexpr int STX = 64, STY = 32, SLDW = 21;  // 32 window rows per block (64 = less halo, fewer blocks per CU: measured, no gain)
static inline size_t stats_lds_bytes(uint32_t n_h) { return (size_t)(STY + n_h - 1) * (SLDW * 4 + STX * 4 + STX * 2); }

struct StatsOut {  // what a statistics launch writes for one size class
    PlaneParams p;
    void *out;     // OUT = 1: int16 threshold plane, OUT = 0: int32 negL table; [page][Lrows][Lpitch]
};

// IDX: uint32_t on the plane path (a pass's planes span < 4 GiB: launch_scan_mfma), size_t for the int32 tables
template <int OUT, typename IDX>
__device__ __forceinline__ void stats_store(const StatsOut &o, IDX idx, bool emit, float Lf) {
    if (OUT) {
        // a pass's planes span < 4 GiB (launch_scan_mfma), so the entry's BYTE offset fits 32 bits: uniform base + 32-bit lane offset,
        // no 64-bit vector add per store
        const uint32_t byte_off = (uint32_t)idx * 2u;
        *reinterpret_cast<int16_t *>(reinterpret_cast<char *>(o.out) + byte_off) = emit ? plane_value(o.p, Lf) : PLANE_NEVER;
    } else {
        reinterpret_cast<int32_t *>(o.out)[idx] = emit ? threshold_negL(Lf) : -REJECT;
    }
}

template <int NDW, bool SMALLN, int OUT, bool DROP, bool PAIR>  // NDW: dwords of the KEPT width (n_w, or n_w - 1 with DROP)
__global__ __launch_bounds__(256) void stats_kernel(const uint8_t *__restrict__ pages, uint32_t pitch, uint32_t rows_alloc,
                                                    uint32_t r_w, uint32_t r_h, uint32_t n_w, uint32_t n_h, const StatsOut A,
                                                    const StatsOut B, uint32_t Lpitch, uint32_t Lrows,
                                                    uint8_t *__restrict__ live, uint32_t mtx, uint32_t n_rows) {
    // dynamic LDS, sized for this class's n_h (stats_lds_bytes): ~21 KB at n_h = 15 -> 7 blocks per CU; the kernel
    // lives on that occupancy (global-load latency, two barriers per tile)
    extern __shared__ uint32_t stats_lds[];
    const uint32_t page = blockIdx.z, x0 = blockIdx.x * STX, y0 = blockIdx.y * STY;
    const uint32_t rows = STY + n_h - 1;
    uint32_t (*tile)[SLDW] = reinterpret_cast<uint32_t (*)[SLDW]>(stats_lds);
    uint32_t (*H2)[STX] = reinterpret_cast<uint32_t (*)[STX]>(stats_lds + rows * SLDW);
    uint16_t (*H)[STX] = reinterpret_cast<uint16_t (*)[STX]>(stats_lds + rows * (SLDW + STX));  // row sums <= 16 * 255
    const uint8_t *pg = pages + (size_t)page * rows_alloc * pitch;
    uint32_t any_ink = 0;
    for (uint32_t i = threadIdx.x; i < rows * SLDW; i += 256) {
        uint32_t r = i / SLDW, cdw = i % SLDW;
        uint32_t gy = y0 + r, gx = x0 + cdw * 4;
        uint32_t v = 0;
        if (gy < rows_alloc && gx + 4 <= pitch) v = *reinterpret_cast<const uint32_t *>(pg + (size_t)gy * pitch + gx);
        tile[r][cdw] = v;
        any_ink |= v;
    }
    // Blank paper under the whole tile (page margins: ~1 block in 10): every window here has zero variance — "never emits",
    // no M-tile marked live — so the sliding sums are skipped and the entries just say so (an M-tile of this block can still be
    // live through another size class of the pass, whose launch stages a wider tile: its reads must find a defined value).
    if (!__syncthreads_or((int)(any_ink != 0))) {
        const uint32_t col = threadIdx.x & 63, x = x0 + col;
        if (x < Lpitch)
            for (uint32_t k = 0; k < STY / 4; k++) {
                const uint32_t y = y0 + (threadIdx.x >> 6) * (STY / 4) + k;
                if (y >= Lrows) break;
                const size_t idx = ((size_t)page * Lrows + y) * Lpitch + x;
                stats_store<OUT, size_t>(A, idx, false, 0.f);
                if (PAIR) stats_store<OUT, size_t>(B, idx, false, 0.f);
            }
        return;
    }
    const uint32_t kw = DROP ? n_w - 1 : n_w;  // the kept width: what the horizontal sums cover
    {  // horizontal sums
        const uint32_t lane = threadIdx.x & 63, cb = lane >> 2, sh = lane & 3;
        for (uint32_t r = threadIdx.x >> 6; r < rows; r += 4) {
            uint32_t h = 0, h2 = 0;
#pragma unroll
            for (int k = 0; k < NDW; k++) {
                uint32_t lo = tile[r][cb + k], hi = tile[r][cb + k + 1];
                uint32_t w = __builtin_amdgcn_alignbyte(hi, lo, sh);
                uint32_t keep = kw >= (uint32_t)(4 * k + 4) ? 0xffffffffu
                                : (kw <= (uint32_t)(4 * k) ? 0u : ((1u << (8 * (kw - 4 * k))) - 1u));
                w &= keep;
                h = __builtin_amdgcn_udot4(w, 0x01010101u, h, false);
                h2 = __builtin_amdgcn_udot4(w, w, h2, false);
            }
            H[r][lane] = (uint16_t)h;
            H2[r][lane] = h2;
        }
    }
    __syncthreads();
    // the wave's strip of window rows as a scalar: row numbers, LDS row offsets and the "row exists" tests below stay out of the vector unit
    const uint32_t col = threadIdx.x & 63, strip = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t x = x0 + col;
    if (x >= Lpitch) return;
    constexpr uint32_t PER = STY / 4;  // window rows per thread
    const uint32_t r0 = strip * PER;
    // the class's last column as bytes of the tile (DROP): column x + n_w - 1 of the page = byte col + n_w - 1 of a tile row
    const uint8_t *lastc = reinterpret_cast<const uint8_t *>(&tile[0][0]) + col + n_w - 1;
    uint32_t s_k = 0, s2_k = 0, q1 = 0, q2 = 0;  // sums of the kept box and of the dropped column
    for (uint32_t j = 0; j < n_h; j++) {
        s_k += H[r0 + j][col];
        s2_k += H2[r0 + j][col];
        if (DROP) {
            const uint32_t b = lastc[(size_t)(r0 + j) * (SLDW * 4)];
            q1 += b;
            q2 += __umul24(b, b);
        }
    }
    const uint32_t n = n_w * n_h, n_k = (n_w - 1) * n_h;
    // searched windows: x in [1, r_w - n_w], y in [1, r_h - n_h]  (src/ncc.rs:279-282, src/ncc.cpp:302)
    const bool x_ok = x >= 1 && x + n_w <= r_w, xk_ok = x >= 1 && x + n_w - 1 <= r_w;
    const uint32_t ya = y0 + r0;
    // M-tile marks: one store per 16-lane group and window row, decided by ballot (blank paper is never scanned;
    // the reference prunes it too, src/ncc.rs:280-301).  Row y of the image is tile row y - 1.
    const bool mark_lane = (col & 15) == 0 && (x >> 4) < mtx;
    const uint32_t live_i = (page * n_rows + ya) * mtx + (x >> 4);  // entry of image row ya + 1 (a pass has < 2^31 M-tiles: launch_scan_mfma)
    typedef typename std::conditional<OUT == 1, uint32_t, size_t>::type idx_t;
    idx_t idx = ((idx_t)page * Lrows + ya) * Lpitch + x;  // the window's entry in the planes; one row further per step
#pragma unroll
    for (uint32_t k = 0; k < PER; k++, idx += Lpitch) {
        const uint32_t y = ya + k;
        if (y < Lrows) {
            // V = n*s2 - s*s, exact; V > 0 <=> the reference's rnorm is finite.  SMALLN (n <= 256): both products
            // fit 32 bits (n*s2 <= n^2 * 255^2 < 2^32, s <= 255 n < 2^16).
            const uint32_t s = DROP ? s_k + q1 : s_k, s2 = DROP ? s2_k + q2 : s2_k;  // the full box
            bool nz;
            float Vf;
            if (SMALLN) {  // n <= 256: n, s, s2 < 2^24 -> full-rate 24-bit multiplies (a 32-bit v_mul_lo is a quarter-rate instruction)
                const uint32_t V = __umul24(n, s2) - __umul24(s, s);
                nz = V != 0;
                Vf = (float)V;
            } else {
                const uint64_t V = (uint64_t)n * s2 - (uint64_t)s * s;
                nz = V != 0;
                Vf = (float)V;
            }
            const bool y_ok = y >= 1 && y + n_h <= r_h;
            const bool emit = x_ok && y_ok && nz;
            bool any = emit;
            stats_store<OUT, idx_t>(A, idx, emit, DROP ? threshold_f32(A.p, Vf, dropped_column_W_upper(n_k, n_h, s_k, q1, q2)) : threshold_f32_nodrop(A.p, Vf));
            if (PAIR) {  // the kept box as a size class of its own: (n_w - 1) x n_h, nothing dropped
                bool nzk;
                float Vkf;
                if (SMALLN) {
                    const uint32_t Vk = __umul24(n_k, s2_k) - __umul24(s_k, s_k);
                    nzk = Vk != 0;
                    Vkf = (float)Vk;
                } else {
                    const uint64_t Vk = (uint64_t)n_k * s2_k - (uint64_t)s_k * s_k;
                    nzk = Vk != 0;
                    Vkf = (float)Vk;
                }
                const bool emit_k = xk_ok && y_ok && nzk;
                any |= emit_k;
                stats_store<OUT, idx_t>(B, idx, emit_k, threshold_f32_nodrop(B.p, Vkf));
            }
            const uint64_t lm = __builtin_amdgcn_ballot_w64(any);
            if (mark_lane && ((lm >> col) & 0xffffu) && y >= 1 && y <= n_rows) live[live_i + k * mtx - mtx] = 1;
        }
        if (k + 1 < PER) {  // slide down one row
            s_k += H[r0 + k + n_h][col] - H[r0 + k][col];
            s2_k += H2[r0 + k + n_h][col] - H2[r0 + k][col];
            if (DROP) {
                const uint32_t bi = lastc[(size_t)(r0 + k + n_h) * (SLDW * 4)], bo = lastc[(size_t)(r0 + k) * (SLDW * 4)];
                q1 += bi - bo;
                q2 += __umul24(bi, bi) - __umul24(bo, bo);
            }
        }
    }
}

// The same statistics for kept widths of 4, 8, 12 and 16 columns (8: BASELINE configs[1] and [2], 8-wide classes and 9-wide ones with
// their last column dropped; the description below is for 8, template parameter KQ = 2), VERTICAL sums first and no LDS: a lane owns four neighbouring columns (one dword of every page row), slides the
// n_h-row sums of its four columns down S8_ROWS window rows — C1 = sum of bytes, C2 = sum of squares, from the row that enters and
// the row that leaves: d = in - out, C1 += d, C2 += d * (in + out) — and the horizontal 8-sums come out of the lanes' registers:
// window x = 4L + i covers columns 4L + i .. 4L + i + 7 = the rest of lane L's dword, all of lane L + 1's, the first i columns
// of lane L + 2's; the dropped ninth column is column i of lane L + 2.  Two row sums from lane L + 1 and eight column sums from
// lane L + 2 per row (ds_bpermute), no tile staging, no barrier, four plane values per 8-byte store.  A wave is a strip of 240
// window columns (lanes 60..63 only feed their neighbours) x S8_ROWS rows of one page; a row of the strip whose 8 + 256 columns
// are blank over the n_h rows (every C2 zero) stores "never" without the arithmetic.  Results: the same exact integers s, s2, q1,
// q2 as stats_kernel, then the same code — plane for plane identical (tests/test_gpu_parity.py: the planes of both kernels, and every parity test).
constexpr uint32_t S8_COLS = 240, S8_ROWS = 16;  // (8 / 24 / 32 rows per wave: 133 / 130 / 141 us against 130 before the rows were prefetched; 16 and 24 level after)
//   APPEND: the launch is the only statistics launch of its scan pass (BASELINE configs[1]: both classes in one PAIR launch), so a
//   marked M-tile is final: instead of a mark byte for compact_live_tiles the wave remembers its marks (16 rows x 15 M-tiles: one
//   bit per row in each quad's first lane) and appends them to the pass's work list itself, in row-major order, behind ONE atomic
//   per workgroup — no mark bytes, no compaction launch between the statistics and the scan kernel.
//   KQ = kept width / 4 (1 .. 4: kept widths 4, 8, 12, 16): window 4L + i then covers the rest of lane L's dword, lanes L + 1 .. L + KQ - 1
//   whole and the first i columns of lane L + KQ, and the dropped column is column i of lane L + KQ.
//   A workgroup is GS neighbouring strips x GB bands one below the other (up to 16 waves), and it appends in the order (band, window
//   row, strip): the work list then holds a page in blocks of whole page rows, GB x 16 rows tall, as compact_live_tiles' did (4 096
//   M-tiles per block) — the scan kernel's neighbouring items share the page rows their windows overlap in and the planes' cache lines.
template <int KQ, bool SMALLN, bool DROP, bool PAIR, bool APPEND>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) void stats8_kernel(const uint8_t *__restrict__ pages, uint32_t pitch, uint32_t rows_alloc, uint32_t r_w, uint32_t r_h,
                                                      uint32_t n_w, uint32_t n_h, const StatsOut A, const StatsOut B, uint32_t Lpitch, uint32_t Lrows,
                                                      uint8_t *__restrict__ live, uint32_t mtx, uint32_t n_rows, uint32_t strips_x, uint32_t bands_y,
                                                      uint32_t GS, uint32_t GB, uint32_t sgroups, uint32_t bgroups, uint64_t *__restrict__ list,
                                                      uint32_t *__restrict__ list_count, uint32_t pair_rows) {
    __shared__ uint32_t wg_cnt[16][S8_ROWS], wg_off[16][S8_ROWS];  // [wave][window row]: live M-tiles, and where they go inside the workgroup's block
    __shared__ uint32_t wg_wsum[4];
    __shared__ uint32_t wg_base;
    const uint32_t lane = threadIdx.x & 63, wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t per_page = sgroups * bgroups, in_page = blockIdx.x % per_page;
    const uint32_t band = (in_page / sgroups) * GB + wv / GS, strip = (in_page % sgroups) * GS + wv % GS;
    uint32_t mymask = 0, page = blockIdx.x / per_page, y0 = band * S8_ROWS, xl = 0;  // APPEND: bit k = the M-tile of this quad is live in window row y0 + k
    if (strip < strips_x && band < bands_y) {  // wave-uniform (the workgroup's last strips / bands may lie outside the page)
    const uint32_t x0 = strip * S8_COLS;
    xl = x0 + 4 * lane;  // the lane's first column = its first window
    // lanes right of the row read its zero padding (>= 64 zero bytes right of every row, focr_pages_alloc)
    const uint32_t off = xl + 4 <= pitch ? xl : pitch - 4;
    const uint8_t *pg = pages + (size_t)page * rows_alloc * pitch;
    auto load_row = [&](uint32_t y) -> uint32_t {  // wave-uniform row test (pages end with >= 48 zero rows: never taken at the sizes the MFMA path covers)
        return y < rows_alloc ? *reinterpret_cast<const uint32_t *>(pg + (size_t)y * pitch + off) : 0u;
    };
    uint32_t c1[4] = {0, 0, 0, 0}, c2[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; j < n_h; j += 8) {  // the first window row's sums: eight page rows per round trip to memory
        uint32_t v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = load_row(y0 + j + i);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (j + i >= n_h) v[i] = 0;  // wave-uniform
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const uint32_t b = (v[i] >> (8 * m)) & 0xffu;
                c1[m] += b;
                c2[m] += __umul24(b, b);
            }
        }
    }
    int an[KQ + 1];  // ds_bpermute addresses of lanes L + 1 .. L + KQ
#pragma unroll
    for (int q = 1; q <= KQ; q++) an[q] = (int)(lane + q < 64 ? lane + q : 63) * 4;
    const uint32_t n = n_w * n_h, n_k = (n_w - 1) * n_h;
    const bool store_lane = lane < S8_COLS / 4 && xl < Lpitch;
    const bool mark_lane = (lane & 3) == 0 && lane < S8_COLS / 4 && (xl >> 4) < mtx;  // a quad's first lane speaks for its M-tile; lanes 60..63 belong to the next strip
    char *outA = reinterpret_cast<char *>(A.out), *outB = reinterpret_cast<char *>(B.out);
    const uint32_t k_end = y0 < Lrows ? (Lrows - y0 < S8_ROWS ? Lrows - y0 : S8_ROWS) : 0u;  // wave-uniform: the band's rows inside the planes
    auto window_row = [&](uint32_t k) __attribute__((always_inline)) {
        const uint32_t y = y0 + k;
        // the rows that enter and leave when the window slides down: asked for now, used behind this row's arithmetic
        const uint32_t vi = load_row(y + n_h), vo = load_row(y);
        const uint32_t entry = ((page * Lrows + y) * Lpitch + xl) * 2u;  // byte offset of the lane's four values in a plane (a pass's planes span < 4 GiB)
        const bool y_ok = y >= 1 && y + n_h <= r_h;
        const uint32_t nzc = c2[0] | c2[1] | c2[2] | c2[3];
        if (__builtin_amdgcn_ballot_w64(nzc != 0) == 0 || !y_ok) {
            // nothing but paper under the strip's windows of this row (or a row the reference never searches): "never", no marks
            if (store_lane) {
                const uint32_t nv = (uint32_t)(uint16_t)PLANE_NEVER * 0x10001u;
                *reinterpret_cast<uint2 *>(outA + entry) = uint2{nv, nv};
                if (PAIR) *reinterpret_cast<uint2 *>(outB + entry) = uint2{nv, nv};
            }
        } else {
            const uint32_t R1 = c1[0] + c1[1] + c1[2] + c1[3], R2 = c2[0] + c2[1] + c2[2] + c2[3];
            uint32_t s_k = R1, s2_k = R2;
#pragma unroll
            for (int q = 1; q < KQ; q++) {  // the whole lanes between
                s_k += (uint32_t)__builtin_amdgcn_ds_bpermute(an[q], (int)R1);
                s2_k += (uint32_t)__builtin_amdgcn_ds_bpermute(an[q], (int)R2);
            }
            uint32_t e1[4], e2[4];
#pragma unroll
            for (int m = 0; m < 4; m++) {
                e1[m] = (uint32_t)__builtin_amdgcn_ds_bpermute(an[KQ], (int)c1[m]);
                e2[m] = (uint32_t)__builtin_amdgcn_ds_bpermute(an[KQ], (int)c2[m]);
            }
            int16_t va[4], vb[4];
            bool any = false;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t x = xl + i, q1 = e1[i], q2 = e2[i];
                const bool x_ok = x >= 1 && x + n_w <= r_w, xk_ok = x >= 1 && x + n_w - 1 <= r_w;
                const uint32_t s = DROP ? s_k + q1 : s_k, s2 = DROP ? s2_k + q2 : s2_k;  // the full box
                bool nz;
                float Vf;
                if (SMALLN) {
                    const uint32_t V = __umul24(n, s2) - __umul24(s, s);
                    nz = V != 0;
                    Vf = (float)V;
                } else {
                    const uint64_t V = (uint64_t)n * s2 - (uint64_t)s * s;
                    nz = V != 0;
                    Vf = (float)V;
                }
                const bool emit = x_ok && nz;
                any |= emit;
                const float La = DROP ? threshold_f32(A.p, Vf, dropped_column_W_upper(n_k, n_h, s_k, q1, q2)) : threshold_f32_nodrop(A.p, Vf);
                va[i] = emit ? plane_value(A.p, La) : PLANE_NEVER;
                if (PAIR) {
                    bool nzk;
                    float Vkf;
                    if (SMALLN) {
                        const uint32_t Vk = __umul24(n_k, s2_k) - __umul24(s_k, s_k);
                        nzk = Vk != 0;
                        Vkf = (float)Vk;
                    } else {
                        const uint64_t Vk = (uint64_t)n_k * s2_k - (uint64_t)s_k * s_k;
                        nzk = Vk != 0;
                        Vkf = (float)Vk;
                    }
                    const bool emit_k = xk_ok && nzk;
                    any |= emit_k;
                    vb[i] = emit_k ? plane_value(B.p, threshold_f32_nodrop(B.p, Vkf)) : PLANE_NEVER;
                }
                s_k += e1[i] - c1[i];  // one column to the right
                s2_k += e2[i] - c2[i];
            }
            if (store_lane) {
                *reinterpret_cast<uint2 *>(outA + entry) = uint2{(uint32_t)(uint16_t)va[0] | ((uint32_t)(uint16_t)va[1] << 16), (uint32_t)(uint16_t)va[2] | ((uint32_t)(uint16_t)va[3] << 16)};
                if (PAIR) *reinterpret_cast<uint2 *>(outB + entry) = uint2{(uint32_t)(uint16_t)vb[0] | ((uint32_t)(uint16_t)vb[1] << 16), (uint32_t)(uint16_t)vb[2] | ((uint32_t)(uint16_t)vb[3] << 16)};
            }
            // M-tile marks: an M-tile is the 16 windows of four lanes (x0 is a multiple of 16)
            const uint64_t lm = __builtin_amdgcn_ballot_w64(any && store_lane);
            if (mark_lane && ((lm >> lane) & 0xfu) && y <= n_rows) {
                if (APPEND) mymask |= 1u << k;
                else live[(page * n_rows + y - 1) * mtx + (xl >> 4)] = 1;
            }
        }
        // APPEND behind other statistics launches of the pass (their marks are in `live`): an M-tile they marked is live too
        if (APPEND && live && mark_lane && y >= 1 && y <= n_rows && live[(page * n_rows + y - 1) * mtx + (xl >> 4)]) mymask |= 1u << k;
        {  // slide down one row
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const uint32_t bi = (vi >> (8 * m)) & 0xffu, bo = (vo >> (8 * m)) & 0xffu;
                const int d = (int)bi - (int)bo;
                c1[m] += (uint32_t)d;
                c2[m] += (uint32_t)__mul24(d, (int)(bi + bo));
            }
        }
    };
    uint32_t k = 0;
    for (; k + 2 <= k_end; k += 2) {  // two window rows per trip: the second row's loads and lane exchanges overlap the first row's arithmetic
        window_row(k);
        window_row(k + 1);
    }
    if (k < k_end) window_row(k);
    }  // a strip and a band of the page
    if (APPEND) {
        // pair_rows: an entry stands for the image rows (y, y + 1), y even — live if either row is; a band starts at a multiple of 16, so
        // a pair never leaves its wave.  The pair's bit sits at its even row: the odd rows count nothing and append nothing.
        const uint32_t kstep = pair_rows ? 2u : 1u;
        if (pair_rows) mymask = (mymask | (mymask >> 1)) & 0x5555u;
        uint32_t mycnt = 0;  // lane k < 16: this wave's live M-tiles in window row k
        for (uint32_t k = 0; k < S8_ROWS; k += kstep) {
            const uint32_t cnt = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64((mymask >> k) & 1u));
            if (lane == k) mycnt = cnt;
        }
        if (lane < S8_ROWS) wg_cnt[wv][lane] = mycnt;
        if (threadIdx.x < 4) wg_wsum[threadIdx.x] = 0;  // (a workgroup may have fewer than four waves)
        __syncthreads();
        // exclusive prefix of the counts in the block's order (band, window row, strip): cell o = (band * 16 + row) * GS + strip, one
        // thread of the first four waves per cell (at most 16 waves x 16 rows = 256 cells)
        const uint32_t o = threadIdx.x, n_cells = GS * GB * S8_ROWS;
        uint32_t cw = 0, ck = 0, v = 0;
        if (o < 256 && o < n_cells) {
            const uint32_t s_ = o % GS, bk = o / GS;
            ck = bk % S8_ROWS;
            cw = (bk / S8_ROWS) * GS + s_;
            v = wg_cnt[cw][ck];
        }
        if (o < 256) {  // wave-uniform: waves 0 .. 3
            uint32_t incl = v;
#pragma unroll
            for (uint32_t d = 1; d < 64; d <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
                if (lane >= d) incl += t;
            }
            if (lane == 63) wg_wsum[wv] = incl;
            v = incl - v;  // exclusive inside the wave
        }
        __syncthreads();
        if (o < 256) {
            uint32_t before = 0;
            for (uint32_t q = 0; q < wv; q++) before += wg_wsum[q];
            if (o < n_cells) wg_off[cw][ck] = before + v;
            if (o == 0) {
                const uint32_t t = wg_wsum[0] + wg_wsum[1] + wg_wsum[2] + wg_wsum[3];
                wg_base = t ? atomicAdd(list_count, t) : 0u;
            }
        }
        __syncthreads();
        const uint32_t base = wg_base;
        const uint32_t myoff = lane < S8_ROWS ? wg_off[wv][lane] : 0u;
        for (uint32_t k = 0; k < S8_ROWS; k += kstep) {
            const bool mine = (mymask >> k) & 1u;
            const uint64_t m = __builtin_amdgcn_ballot_w64(mine);
            if (m == 0) continue;  // wave-uniform
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            const uint32_t row_at = base + (uint32_t)__builtin_amdgcn_readlane((int)myoff, (int)k);
            // the scan kernel's entry: page << 32 | tile row (image row y - 1) << 12 | M-tile column (compact_live_tiles);
            // pair_rows: the pair's even image row y itself (the pair (0, 1) has no row "- 1")
            if (mine) list[row_at + rank] = ((uint64_t)page << 32) | ((uint64_t)(pair_rows ? y0 + k : y0 + k - 1) << 12) | (xl >> 4);
        }
    }
}

// Live M-tiles -> packed work list (page << 32 | row << 12 | col).  A block compacts 4096 consecutive tiles
// (16 per thread) with one global atomic, so the shared counter sees ~1 atomic per 4096 tiles.  The order of the
// list does not matter for the results (every M-tile is independent; hits are sorted later).
constexpr uint32_t CLT_PER_THREAD = 16;
__global__ __launch_bounds__(256) void compact_live_tiles(const uint8_t *__restrict__ live, uint32_t n_tiles, uint32_t mtx,
                                                          uint32_t n_rows, uint32_t skip_blank, uint64_t *__restrict__ list,
                                                          uint32_t *__restrict__ count) {
    __shared__ uint32_t wave_tot[4];
    __shared__ uint32_t block_base;
    const uint32_t first = (blockIdx.x * 256 + threadIdx.x) * CLT_PER_THREAD;
    uint32_t bits = 0;
    if (first + CLT_PER_THREAD <= n_tiles) {  // the thread's 16 marks in one (byte-aligned) 16-byte load
        typedef unsigned int clt_v4 __attribute__((ext_vector_type(4), aligned(1)));
        const clt_v4 m = *reinterpret_cast<const clt_v4 *>(live + first);
#pragma unroll
        for (uint32_t k = 0; k < CLT_PER_THREAD; k++)
            if (((m[k / 4] >> (8 * (k % 4))) & 0xffu) || !skip_blank) bits |= 1u << k;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < CLT_PER_THREAD; k++) {
            const uint32_t i = first + k;
            if (i < n_tiles && (live[i] || !skip_blank)) bits |= 1u << k;
        }
    }
    const uint32_t cnt = (uint32_t)__builtin_popcount(bits);
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t incl = cnt;  // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        if ((int)lane >= o) incl += v;
    }
    if (lane == 63) wave_tot[wv] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tot = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        block_base = tot ? atomicAdd(count, tot) : 0;
    }
    __syncthreads();
    uint32_t pos = block_base + incl - cnt;
    for (uint32_t q = 0; q < wv; q++) pos += wave_tot[q];
    for (uint32_t k = 0; k < CLT_PER_THREAD; k++)
        if (bits & (1u << k)) {
            const uint32_t i = first + k;
            const uint32_t col = i % mtx, rowp = i / mtx, row = rowp % n_rows, page = rowp / n_rows;
            list[pos++] = ((uint64_t)page << 32) | ((uint64_t)row << 12) | col;
        }
}

// whether a size class's statistics take the register form (stats8_kernel): threshold planes, a kept width of 4, 8, 12 or 16 px
// (focr_debug_set_stats_form(1): the LDS-tiled kernel for every class)
static bool stats_register_form(const focr_ctx *c, const SizeClass &sc) {
    // (a dropped column only exists for 9 -> 8 and 13 -> 12: layout_supers)
    return sc.keep_w % 4 == 0 && sc.keep_w >= 4 && sc.keep_w <= 16 && c->dbg_stats_form == 0;
}

// whether the statistics of a plane pass end in a register-form launch that appends the work list itself (pass_stats: such a launch
// goes last) — the only work list that can hold row pairs (plan_passes)
bool pass_appends(const focr_ctx *c, const SuperClass &su) {
    for (uint32_t k : su.classes)
        if (stats_register_form(c, c->bank.classes[k])) return true;
    return false;
}

// bands per workgroup of stats8_kernel, at most: 1 .. 5 measured 34.15 / 34.60 / 33.89 / 34.23 / 33.70 Gpx/s
constexpr uint32_t S8_BANDS_MAX = 2;

// THE choice of a statistics kernel's form, for both kernels: (pair -> DROP and PAIR; else drop -> DROP; else plain) x small.
// f(SMALLN, DROP, PAIR) gets the flags as std::integral_constants.  DROPS = false: a kept width that no class with a dropped column
// has (4 and 16 in the register form: a dropped column only exists for 9 -> 8 and 13 -> 12, layout_supers) — the plain forms alone.
template <bool DROPS, typename F>
static void stats_form(bool pair, bool drop, bool small, F f) {
    const auto sized = [&](auto dr, auto pr) { small ? f(std::true_type{}, dr, pr) : f(std::false_type{}, dr, pr); };
    if constexpr (DROPS) {
        if (pair) return sized(std::true_type{}, std::true_type{});
        if (drop) return sized(std::true_type{}, std::false_type{});
    }
    sized(std::false_type{}, std::false_type{});
}
// f(std::integral_constant<int, v>) for v = 1 .. 4 (a kept width in dwords); false: v is none of them
template <typename F>
static bool with_1_to_4(uint32_t v, F f) {
    switch (v) {
        case 1: return f(std::integral_constant<int, 1>{}), true;
        case 2: return f(std::integral_constant<int, 2>{}), true;
        case 3: return f(std::integral_constant<int, 3>{}), true;
        case 4: return f(std::integral_constant<int, 4>{}), true;
        default: return false;
    }
}

// one statistics launch: class k (full box), optionally together with its kept box as class `pair` (< 0: none); planes: int16 threshold
// planes, else the int32 tables; append_list / append_count: the launch is the pass's only one and appends its live M-tiles to the work
// list itself (stats8_kernel, APPEND)
static int launch_stats(focr_ctx *c, bool planes, size_t k, int pair, double thr_d, void *out, void *out_pair, uint32_t Lpitch, uint32_t Lrows, uint8_t *live,
                        uint32_t mtx, uint32_t n_rows, uint64_t *append_list, uint32_t *append_count, bool pair_rows) {
    const SizeClass &sc = c->bank.classes[k];
    // only what the scan kernels read: the windows of the pass's M-tiles (x < 16 * mtx) in the searched rows (y <= n_rows)
    dim3 grid(std::min<unsigned>(Lpitch / STX, (16 * mtx + STX - 1) / STX), std::min<unsigned>((Lrows + STY - 1) / STY, (n_rows + 1 + STY - 1) / STY),
              (unsigned)c->sub_np);
    StatsOut A{plane_params(c, k, thr_d), out}, B{};
    if (pair >= 0) B = StatsOut{plane_params(c, (size_t)pair, thr_d), out_pair};
    const bool drop = sc.keep_w != sc.n_w, small = sc.n_w * sc.n_h <= 256, reg = planes && stats_register_form(c, sc);
    if (append_list && !reg) return fail(c, FOCR_ERR_INVALID, "scan_mfma: internal: direct append without the register form");
    if (pair_rows && !append_list) return fail(c, FOCR_ERR_INVALID, "scan_mfma: internal: row pairs without the direct append");
    if (reg) {  // kept width 4, 8, 12, 16: the register form (stats8_kernel)
        const uint32_t cols = std::min<uint32_t>(Lpitch, 16 * mtx), rows_n = std::min<uint32_t>(Lrows, n_rows + 1);
        const uint32_t strips_x = (cols + S8_COLS - 1) / S8_COLS, bands_y = (rows_n + S8_ROWS - 1) / S8_ROWS;
        // a workgroup: GS neighbouring strips x GB bands, at most 16 waves (stats8_kernel)
        const uint32_t GS = std::min<uint32_t>(strips_x, 16), GB = std::max<uint32_t>(1, std::min<uint32_t>(std::min<uint32_t>(16 / GS, S8_BANDS_MAX), bands_y));
        const uint32_t sgroups = (strips_x + GS - 1) / GS, bgroups = (bands_y + GB - 1) / GB;
        const uint64_t n_wgs = (uint64_t)sgroups * bgroups * c->sub_np;
        if (n_wgs >= 0x7fffffffull) return fail(c, FOCR_ERR_INVALID, "scan_mfma: batch too large for 32-bit tile ids; scan fewer pages per call");
        auto launch8 = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3((unsigned)n_wgs), dim3(GS * GB * 64), 0, c->stream, c->pages.u8 + c->sub_p0 * c->pages.rows_alloc * c->pages.pitch, (uint32_t)c->pages.pitch,
                               (uint32_t)c->pages.rows_alloc, (uint32_t)c->pages.r_w, (uint32_t)c->pages.r_h, sc.n_w, sc.n_h, A, B, Lpitch, Lrows, live, mtx, n_rows, strips_x, bands_y,
                               GS, GB, sgroups, bgroups, append_list, append_count, pair_rows ? 1u : 0u);
        };
        with_1_to_4(sc.keep_w / 4, [&](auto kq) {  // KQ = kept width / 4
            constexpr int KQ = decltype(kq)::value;
            stats_form<KQ == 2 || KQ == 3>(pair >= 0, drop, small, [&](auto sm, auto dr, auto pr) {
                append_list ? launch8(stats8_kernel<KQ, sm, dr, pr, true>) : launch8(stats8_kernel<KQ, sm, dr, pr, false>);
            });
        });
        FOCR_HIP(c, hipGetLastError());
        return FOCR_OK;
    }
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, grid, dim3(256), stats_lds_bytes(sc.n_h), c->stream, c->pages.u8 + c->sub_p0 * c->pages.rows_alloc * c->pages.pitch, (uint32_t)c->pages.pitch,
                           (uint32_t)c->pages.rows_alloc, (uint32_t)c->pages.r_w, (uint32_t)c->pages.r_h, sc.n_w, sc.n_h, A, B, Lpitch, Lrows, live, mtx, n_rows);
    };
    const bool known = with_1_to_4((sc.keep_w + 3) / 4, [&](auto ndw) {  // NDW = dwords of the kept width (keep_w = n_w unless the class's last column is dropped)
        constexpr int NDW = decltype(ndw)::value;
        stats_form<true>(pair >= 0, drop, small, [&](auto sm, auto dr, auto pr) {
            planes ? launch(stats_kernel<NDW, sm, 1, dr, pr>) : launch(stats_kernel<NDW, sm, 0, dr, pr>);
        });
    });
    if (!known) return fail(c, FOCR_ERR_INVALID, "scan_mfma: unsupported box width");
    FOCR_HIP(c, hipGetLastError());
    return FOCR_OK;
}

// The statistics launches of one scan pass (super-class si: size classes that share the scan kernel's A fragments) and its work list,
// queued on the context's stream.  Whether they write planes or int32 tables is su.planes (plan_passes).
int pass_stats(focr_ctx *c, const ScanPlan &P, size_t si, double thr_d) {
    const SuperClass &su = c->supers[si];
    uint8_t *lv = P.live + su.live_offset;
    std::vector<char> done(su.classes.size(), 0);
    std::vector<size_t> order;  // classes whose last column is dropped first: they can take their kept box along
    for (int pass = 0; pass < 2; pass++)
        for (size_t v = 0; v < su.classes.size(); v++)
            if ((c->bank.classes[su.classes[v]].keep_w != c->bank.classes[su.classes[v]].n_w) == (pass == 0)) order.push_back(v);
    struct StatsLaunch {
        size_t v, k, pv;
        int pair;
    };
    std::vector<StatsLaunch> todo;  // the pass's statistics launches
    for (size_t v : order) {
        if (done[v]) continue;
        const size_t k = su.classes[v];
        const SizeClass &sc = c->bank.classes[k];
        if (!su.planes && (sc.n_w >= c->pages.r_w || sc.n_h >= c->pages.r_h)) continue;  // nothing searchable: its tiles are skipped by the scan
        // a class whose last column is dropped computes its kept box's statistics anyway: if that box is a size class
        // of this pass too, both come out of one launch
        int pair = -1;
        size_t pv = 0;
        if (sc.keep_w != sc.n_w)
            for (size_t u = 0; u < su.classes.size(); u++) {
                const SizeClass &o = c->bank.classes[su.classes[u]];
                if (u != v && !done[u] && o.n_w == sc.keep_w && o.n_h == sc.n_h && o.keep_w == o.n_w) pair = (int)su.classes[u], pv = u;
            }
        todo.push_back(StatsLaunch{v, k, pv, pair});
        done[v] = 1;
        if (pair >= 0) done[pv] = 1;
    }
    // ONE launch for the whole pass, in the register form: its marks are final and it appends the live M-tiles to the work
    // list itself (stats8_kernel, APPEND) — no mark bytes, no compaction launch in front of the scan kernel
    // (several launches: one in the register form goes LAST and merges the marks the others left in `live`)
    for (size_t i = 0; i + 1 < todo.size(); i++)
        if (stats_register_form(c, c->bank.classes[todo[i].k]) && !stats_register_form(c, c->bank.classes[todo.back().k])) std::swap(todo[i], todo.back());
    const bool direct = su.planes && !todo.empty() && stats_register_form(c, c->bank.classes[todo.back().k]);
    for (const StatsLaunch &L : todo) {
        const bool last = direct && &L == &todo.back();
        // where the class's values go, and its pair's: the pass's threshold planes, or the int32 tables by class
        void *out = su.planes ? (void *)(c->d_planes + su.plane_off + L.v * P.plane) : (void *)(c->d_L + L.k * P.L_per_class);
        void *out_pair = L.pair < 0 ? nullptr : su.planes ? (void *)(c->d_planes + su.plane_off + L.pv * P.plane) : (void *)(c->d_L + (size_t)L.pair * P.L_per_class);
        if (int rc = launch_stats(c, su.planes, L.k, L.pair, thr_d, out, out_pair, P.Lpitch, P.Lrows, last && todo.size() == 1 ? nullptr : lv, su.mtx, su.n_rows,
                                  last ? P.live_list + su.live_offset : nullptr, last ? c->d_counter + LIVE_WORD0 + si : nullptr, last && su.paired)) return rc;
    }
    if (su.paired && !direct) return fail(c, FOCR_ERR_INVALID, "scan_mfma: internal: row pairs planned for a pass whose statistics do not append");
    if (direct) return FOCR_OK;
    const uint32_t nt = (uint32_t)((uint64_t)su.mtx * su.n_rows * c->sub_np);
    hipLaunchKernelGGL(compact_live_tiles, dim3((nt + 256 * CLT_PER_THREAD - 1) / (256 * CLT_PER_THREAD)), dim3(256), 0, c->stream, lv, nt, su.mtx,
                       su.n_rows, 1u, P.live_list + su.live_offset, c->d_counter + LIVE_WORD0 + si);
    FOCR_HIP(c, hipGetLastError());
    return FOCR_OK;
}

}  // namespace focr
