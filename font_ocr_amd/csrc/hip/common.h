// common.h — shared declarations of libfocr_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <vector>

#include "devmem.h"
#include "focr_ncc.h"

namespace focr_dec {
struct VerifyRec;  // decode.h
}

namespace focr {

struct VerifyMeta;  // verify.h

// ---- geometry of one size class -------------------------------------------
// A size class is the set of templates that share (n_w, n_h); window statistics
// depend only on the class (reference: prepare_for_size is cached per size,
// src/ncc.rs:264-268).
struct SizeClass {
    uint32_t n_w, n_h;
    uint32_t ndw;          // dwords per padded template row in the direct kernels (1..4; 5..8 for wide classes)
    uint32_t maxh;         // padded row count in the direct kernel (16 or 32; = n_h for tall classes)
    bool tall;             // n_h > 32 or n_w > 16: scanned by scan_tall_kernel in both modes (no MFMA layout)
    uint32_t n_templates;  // templates in this class
    uint32_t first;        // index of the class's first entry in the class-ordered arrays
    // MFMA prefilter layout
    uint32_t keep_w;          // columns the MFMA multiplies: n_w, or n_w - 1 for a class whose last column is bounded instead
                              // (n_w = 9, 13: one K layout narrower; mfma_common.h, "threshold planes")
    uint32_t layout;          // K layout of the MFMA prefilter (LAYOUT_W8 / W12 / W16, mfma_common.h)
    uint32_t k_groups;        // 16-byte k-groups per window (multiple of 4)
    uint32_t n_tiles16;       // ceil(n_templates / 16)
    uint32_t q_offset;        // byte offset of the class's quantised templates in d_qbank
    uint32_t tg_offset;       // entry offset of the class's template ids in d_tglobal (16 per N-tile, ~0 = padding/dead)
    uint32_t n_live;          // templates that can emit: they take the class's first n_live slots (dead ones and padding follow)
};

// Classes whose A fragments are identical (same K layout, same number of K-steps) are scanned in one kernel
// pass: their N-tiles are concatenated; only the C-in table (negL) changes from class to class.
struct SuperClass {
    uint32_t layout, ksteps;
    std::vector<uint32_t> classes;     // indices into focr_ctx::bank.classes
    std::vector<uint32_t> tile_first;  // first N-tile of each class inside the super-class
    uint32_t n_tiles;
    size_t q_offset, tg_offset;
    // Row pairs (scan_mfma2.hip, PAIR): every class leaves the last row of its K block empty and twice the N-tiles fit one launch, so
    // d_qbank holds a second operand image right behind the first, every template one row lower in its K block (layout_supers)
    bool pairable;
    // per scan (plan_scan): window enumeration of the pass (smallest searchable template), its live-tile list, its threshold planes
    uint32_t min_w, min_h, mtx, n_rows;
    size_t live_offset, plane_off;  // plane_off: first value in d_planes, if `planes` (else the legacy path: int32 tables in d_L)
    bool planes;
    bool paired;  // this scan's work list holds row pairs and the scan kernel takes both images (plan_passes: pairable, planes, the statistics append)
};

// What a scan of the batch launches, decided before anything is enqueued (plan_scan, scan_mfma.hip: also every buffer sized)
struct ScanPlan {
    uint32_t Lpitch = 0, Lrows = 0;
    size_t L_per_class = 0;      // int32 values of one class's table in d_L ([class][page][Lrows][Lpitch]; legacy passes)
    size_t plane = 0;            // int16 values of one threshold plane ([page][Lrows][Lpitch] of the pages scanned)
    size_t tiles_total = 0;      // M-tiles of all passes (SuperClass::live_offset)
    uint8_t *live = nullptr;     // per M-tile mark bytes
    uint64_t *live_list = nullptr;
};

// Per-template constants, computed once on the host in IEEE double exactly as
// the reference's kernel prologue does (src/ncc.cpp:73-86, 278-291).
struct TemplateConst {
    double s_n;      // (double)s_n
    double n_recip;  // 1 / n
    double rnorm_n;  // 1 / sqrt(norm2_n)   (+inf for a constant needle)
    double norm2_n;  // s2_n - s_n^2 / n, for the scalar Rust scan's formula (src/ncc.rs:455)
    uint32_t index;  // global template index (get_hits order)
    uint32_t n_w, n_h;
    uint32_t pad;
};

// Device-side key of a candidate / hit: (page, y, x, t) packed with the minimal field widths of the batch, so that
// one radix sort over bits [0, bits()) puts hits in process_hits order (page, y, x, template) with few passes.
struct KeyFmt {
    uint32_t bt, bx, by, bp;  // bits of template index, x, y, page
    __host__ __device__ uint32_t bits() const { return bt + bx + by + bp; }
    __host__ __device__ uint64_t pack(uint32_t page, uint32_t y, uint32_t x, uint32_t t) const {
        return ((((uint64_t)page << by | y) << bx | x) << bt) | t;
    }
    __host__ __device__ uint32_t t(uint64_t k) const { return (uint32_t)(k & ((1ull << bt) - 1)); }
    __host__ __device__ uint32_t x(uint64_t k) const { return (uint32_t)((k >> bt) & ((1ull << bx) - 1)); }
    __host__ __device__ uint32_t y(uint64_t k) const { return (uint32_t)((k >> (bt + bx)) & ((1ull << by) - 1)); }
    __host__ __device__ uint32_t page(uint64_t k) const { return (uint32_t)(k >> (bt + bx + by)); }
    __host__ __device__ uint64_t line(uint64_t k) const { return k >> (bt + bx); }  // (page << by) | y
};

// The batch's key format: the fewest bits that hold every template index, x, y and page of the batch.
inline KeyFmt key_format(size_t n_templates, size_t r_w, size_t r_h, size_t n_pages) {
    auto nbits = [](size_t n) {
        uint32_t b = 1;
        while (((size_t)1 << b) < n) b++;
        return b;
    };
    return KeyFmt{nbits(n_templates), nbits(r_w), nbits(r_h), nbits(n_pages)};
}

// The BUCKETS of the row path of the tail (rows.hip).  A bucket is a page row cut into n_seg segments of
// 2^seg_shift pixels (x >> seg_shift): one segment for narrow pages and small banks, more where a whole row would hold
// more candidates than one wave sorts in LDS (BASELINE configs[2]: 1200-px rows x 1520 templates).  Buckets ascend with the
// key: (page, y, x-segment).  (cnt: round 3's tail counted every flushed candidate towards its bucket in the scan kernels' flush
// path; always null since round 5 — the hits-first tail counts hits, in the verify.)
struct RowHist {
    uint32_t *cnt;       // [sub_np * r_h * n_seg], zeroed at the start of the scan
    uint32_t r_h;
    uint32_t shift;      // bt + bx: key >> shift = (page << by) | y   (at most 32 bits)
    uint32_t by;
    uint32_t page_base;  // first page of the sub-batch (keys carry absolute page numbers)
    uint32_t bt, bx;     // x = (key >> bt) & (2^bx - 1)
    uint32_t seg_shift, n_seg;
};
// Everything a scan needs zeroed, in ONE launch (clear_kernel, stats.hip).  A hipMemsetAsync costs the submitting thread several
// times a kernel launch (six of them stood between a batch's hand-over and its first kernel: ~0.3 ms of a 1.9 ms step).
struct ClearList {
    void *p[8];       // 8-byte aligned
    uint32_t n8[8];   // 8-byte words
    uint32_t n;
    bool add(void *ptr, size_t bytes) {  // the region is zeroed in whole 8-byte words: its owner allocates up to 7 bytes of slack
        if (n >= 8 || bytes / 8 >= 0xffffffffull) return false;
        p[n] = ptr;
        n8[n] = (uint32_t)((bytes + 7) / 8);
        n++;
        return true;
    }
};

__host__ __device__ inline uint32_t row_of_key(uint64_t key, const RowHist &h) {
    const uint32_t line = (uint32_t)(key >> h.shift), x = (uint32_t)(key >> h.bt) & ((1u << h.bx) - 1u);
    return (((line >> h.by) - h.page_base) * h.r_h + (line & ((1u << h.by) - 1u))) * h.n_seg + (x >> h.seg_shift);
}

// Size estimates of one setup (focr_ctx::est_sig: bank, device, geometry, threshold, cap, mode) for its next scan (results.hip: focr_scan,
// finish_results).  Bounds only: a count above its bound redoes the batch with exact sizes.
struct SizeEstimate {
    size_t cand = 0, hits = 0;  // bounds of the next scan: the last counts + margin() (0: none, exact sizes)
    double var = 0.0667;        // how much the counts of consecutive scans have differed lately (relative; decays by a quarter per scan)
    uint64_t last_cand = 0, last_hits = 0;
    uint32_t row_max = 0;    // largest row of the last scan (estimated mode picks the row capacity from it; 0: it took the legacy tail)
    uint32_t seg_shift = 0;  // log2 of the x-segment width of the row buckets (0: not chosen yet; rows.hip, row_segments)
    void reset() { *this = SizeEstimate{}; }
    double margin() const { return std::min(0.2, std::max(0.04, 3.0 * var)); }  // 4 .. 20 %
    uint64_t row_bound() const { return (uint64_t)row_max + row_max / 4 + 16; }   // the next scan's largest row: the last + 25 %
    void update(const focr_ctx *c, uint64_t n_cand, uint64_t n_hits, uint64_t largest_row);  // a finished batch's counts and its largest row bucket
    void adopt(uint64_t sig);  // shared with the other contexts of the process that scan the same setup (results.hip: g_est)
    void publish(uint64_t sig) const;
    static void forget(uint64_t sig);
};

}  // namespace focr

// Item queues of the persistent scan kernels (scan_mfma2.hip): one per launch, QUEUE_XCDS counters QUEUE_STRIDE dwords
// apart, all zeroed with the counters by the clear launch at the start of a scan (ClearList).
constexpr uint32_t COUNTER_WORDS = 64, QUEUE_XCDS = 8, QUEUE_STRIDE = 32, MAX_SCAN_QUEUES = 128;
constexpr uint32_t TAIL_DONE_WORD = 56, ORDER_DONE_WORD = 57;  // d_counter words: workgroups of the verify / of unit_prefix that have finished ("last workgroup" work)
constexpr uint32_t LIVE_WORD0 = 8, LIVE_WORDS = 40;  // d_counter words: the live M-tile count of each super-class's pass (written by pass_stats, read by its scan launches; h_live is their pinned copy)
static_assert(LIVE_WORD0 + LIVE_WORDS <= TAIL_DONE_WORD && ORDER_DONE_WORD < COUNTER_WORDS, "d_counter's named words overlap");
constexpr size_t COUNTER_BYTES = (COUNTER_WORDS + (size_t)MAX_SCAN_QUEUES * QUEUE_XCDS * QUEUE_STRIDE) * sizeof(uint32_t);

// ---- the result block -------------------------------------------------------
// The sizes and flags of a scan and its process_hits: one block on the device (focr_ctx::d_res) and its pinned host copy (h_res, filled
// by the copy behind record_scan_sizes and read by finish_results once the batch is done).  Kernels take a pointer to one field.  The
// scan's clear launch zeroes everything in front of host_hits.
struct ResultBlock {
    uint64_t candidates;   // written: record_scan_sizes (order.hip; MFMA scans only).  Read: finish_results
    uint64_t hits;         // written: record_scan_sizes.  Read: finish_results
    uint64_t matches;      // hits that survive their call's cap.  Written: record_scan_sizes.  Read: finish_results
    uint64_t lines_chars;  // lines << 32 | chars.  Written: focr_process_hits, into the HOST copy only (the row scan's grand total).  Read: finish_results
    uint64_t flags;        // RES_FLAG_*.  Written: record_scan_sizes, row_sort_kernel (rows.hip), verify_reject (verify.h).  Read: finish_results
    uint64_t row_max;      // largest row bucket.  Written: the row prefix (verify.hip: the verify's last workgroup, or row_prefix_kernel).  Read: row_tail (exact sizes), finish_results for SizeEstimate::update
    uint64_t tail_hits;    // hits the row tail's verify counted.  Written: the same prefix.  Read: row_tail (exact sizes); as d_n_hits by every kernel behind it
    uint64_t host_hits;    // a hit count the HOST knows (direct scan, split batch, debug hits).  Written: install_host_hits.  Read: as d_n_hits by the ordering and process_hits
};
// record_scan_sizes addresses the block as eight words
enum ResSlot : uint32_t { RES_CANDIDATES, RES_HITS, RES_MATCHES, RES_LINES_CHARS, RES_FLAGS, RES_ROW_MAX, RES_TAIL_HITS, RES_HOST_HITS, RES_SLOTS };
static_assert(sizeof(ResultBlock) == 64 && sizeof(ResultBlock) == RES_SLOTS * sizeof(uint64_t), "the result block is eight words");
static_assert(offsetof(ResultBlock, candidates) == 8 * RES_CANDIDATES && offsetof(ResultBlock, hits) == 8 * RES_HITS && offsetof(ResultBlock, matches) == 8 * RES_MATCHES &&
                  offsetof(ResultBlock, lines_chars) == 8 * RES_LINES_CHARS && offsetof(ResultBlock, flags) == 8 * RES_FLAGS && offsetof(ResultBlock, row_max) == 8 * RES_ROW_MAX &&
                  offsetof(ResultBlock, tail_hits) == 8 * RES_TAIL_HITS && offsetof(ResultBlock, host_hits) == 8 * RES_HOST_HITS,
              "the result block's layout is shared by host code and kernels");
constexpr unsigned long long RES_FLAG_COUNT = 1;  // a count above the bound its phase ran with (estimated sizes): the batch is redone with exact sizes
constexpr unsigned long long RES_FLAG_ROW = 2;    // a row bucket above the row kernel's capacity: redone likewise
constexpr unsigned long long RES_FLAG_KEY = 4;    // a candidate key outside the batch reached the verify: internal error

// focr_ctx::ev, ::ms and ::counters, numbered as include/focr_ncc.h documents them (focr_debug_phase_stamps [0..6], focr_last_timings,
// focr_last_counters)
enum PhaseEvent { EV_STATS_BEGIN, EV_STATS_END, EV_SCAN_END, EV_VERIFY_END, EV_ORDER_END, EV_POST_BEGIN, EV_POST_END, N_PHASE_EVENTS };
enum TimingSlot { MS_STATS, MS_SCAN, MS_VERIFY, MS_ORDER, MS_POST, MS_TOTAL, N_TIMINGS };
enum CounterSlot { CNT_CANDIDATES, CNT_HITS, CNT_ALG_MACS, CNT_ISSUED_MACS, N_COUNTERS };
static_assert(N_PHASE_EVENTS + 2 == 9 && N_TIMINGS == 6 && N_COUNTERS == 4, "focr_debug_phase_stamps (the events + the dominant launch's two), focr_last_timings and focr_last_counters fill arrays of 9, 6 and 4");

struct focr_ctx {
    int device = -1;
    hipStream_t stream = nullptr;
    // An executor (pipe.hip) runs the contexts of one LANE on one stream: a lane's batches follow each other in stream order with no
    // host round trip in between, each in a context of its own (its own pages, scratch and results).  Such a context does not own
    // its stream, waits for ITS batch's last kernel (batch_event, recorded by the executor) instead of for the whole stream —
    // the lane's next batch is queued behind it — and reads results back on the lane's side stream (io_stream) for the same reason.
    bool owns_stream = true;
    hipStream_t io_stream = nullptr;    // device -> host / device -> device copies of finished results (== stream for a context of its own)
    hipEvent_t batch_event = nullptr;   // set by the executor behind a batch's last kernel; consumed by the first wait (wait_batch, ctx.hip)
    bool tail_full_chip = false;        // the executor says nothing scans behind this batch (focr_pipe_end_of_stream / _announce_last): its tail may take every CU (rows2_verify)
    std::string err;

    // bank: everything focr_bank_upload builds.  Replaced as a whole (ctx.hip: c->bank = {}), so an array added here cannot leak.
    struct Bank {
        std::vector<focr_template_t> h_templates;
        std::vector<focr::SizeClass> classes;
        std::vector<focr::TemplateConst> h_tconst;         // class-ordered
        focr::DevArray<focr::TemplateConst> d_tconst;      // class-ordered
        focr::DevArray<uint32_t> d_direct_bank;            // class-ordered, [maxh][ndw] dwords each
        std::vector<size_t> direct_bank_off;               // dword offset per class
        focr::DevArray<int8_t> d_qbank;                    // quantised i8 templates for the MFMA prefilter (per-lane B layout)
        focr::DevArray<uint32_t> d_tglobal;                // class-ordered -> global template index, 0xffffffff = never emits
        focr::DevArray<uint32_t> d_order_of;               // global template index -> class-ordered index
        std::vector<double> mfma_c_scale, mfma_e_max, mfma_rho_max;  // per class: quantisation scale, max rounding-error norm, max norm of a unit template's dropped column
        focr::DevArray<uint8_t> d_needles;                 // dense needles (class-ordered, for verify)
        std::vector<uint32_t> h_needle_off;                // class-ordered byte offsets into d_needles
        focr::DevArray<uint32_t> d_needle_off;
        focr::DevArray<uint8_t> d_needles16;               // class-ordered, n_h rows of 16 bytes each (verify operand)
        focr::DevArray<uint32_t> d_needle16_row;           // class-ordered first row index into d_needles16
        focr::DevArray<focr::VerifyMeta> d_vmeta;          // by GLOBAL template index (verify.h): what the verify needs about a template, 32 B
        // the verify operand once more, ordered by GLOBAL template index, for banks that do not fit the LDS whole: a chunk of
        // consecutive templates is then one contiguous piece (verify_chunks_kernel, verify.hip)
        focr::DevArray<uint8_t> d_vrows_t;                 // rows of vrow_bytes each (12 when every template is at most 12 px wide, else 16), by global index
        focr::DevArray<focr::VerifyMeta> d_vmeta_t;        // VerifyMeta by global index whose row0 counts rows of d_vrows_t
        std::vector<uint32_t> h_vrow0_t;                   // [n_templates + 1] first row of every template in d_vrows_t
        uint32_t vrow_bytes = 0;                           // 0: no such copy (a template wider than 16 px)
        focr::DevArray<uint32_t> d_t_w, d_t_h, d_t_letter;  // by global template index
    } bank;
    size_t n_templates = 0;
    std::vector<focr::SuperClass> supers;
    bool column_drop = true;                    // bound the last column of 9- / 13-wide classes instead of multiplying it (takes effect at the next bank upload)
    std::vector<uint32_t> mfma_slot;            // per class-ordered template: its slot inside its class's N-tiles (tile = slot / 16)
    // ---- result sizes (results.hip: finish_results) ----
    // Every phase after the scan kernel takes its element count from device memory; the host only supplies upper bounds for
    // grids and buffers.  Exact mode reads the counts between the phases (as round 1 did); estimated mode (same bank,
    // geometry, threshold, cap as the previous scan) bounds them by the previous scan's counts + a margin (4 .. 20 %), launches everything
    // without waiting, and reads all sizes once at the end; a count above its bound redoes the batch in exact mode.
    focr::DevArray<ResultBlock> d_res;  // one block (above)
    ResultBlock *h_res = nullptr;  // pinned copy
    uint32_t *h_live = nullptr;    // pinned copy of the live M-tile counts (d_counter words LIVE_WORD0 ..), LIVE_WORDS entries
    const uint64_t *d_n_hits = nullptr;  // view, not an owner: the device-side number of hits of the last scan (in d_res, or in scan_pos)
    size_t ub_hits = 0;                  // the bound its buffers were sized for
    uint64_t n_hits_raw_u64 = 0;
    bool estimated = false, estimates_enabled = true;
    focr::SizeEstimate est;
    size_t ub_cand = 0;
    uint64_t est_sig = 0, bank_gen = 0, bank_hash = 0, counters_redone = 0;
    float scan_thr = 0.f, post_anchor = 0.f;
    int scan_mode = 0;
    int32_t post_overlap = 0;
    bool force_split = false;                   // tests: take scan_split without waiting for an overflow (focr_debug_force_split)
    int dbg_verify_form = 0;  // tests / A-B: 1 = the 12-byte verify form also for a bank that would take the 8-byte one (focr_debug_set_verify_form; verify_plan.h)
    int dbg_stats_form = 0;  // tests / A-B: 1 = the LDS-tiled statistics kernel for every class (focr_debug_set_stats_form; 0: the register form where it applies)
    uint32_t dbg_grid_num = 0, dbg_grid_den = 0;  // tests: the tail's persistent kernels on num / den times their workgroups (focr_debug_set_tail_grid; 0: as designed)
    int prefilter = 0;                          // FOCR_PREFILTER_*: auto / plane kernel / legacy kernel (focr_ctx_set_prefilter)
    focr::DevArray<uint16_t> d_planes;          // threshold planes, int16: [super-class][value][page][Lrows][Lpitch] (mfma_common.h); exact, grow-only

    // pages: the resident set the scans read, and the executor's second set (pipe.hip, focr_pipe_prefetch): the NEXT batch of a
    // lane is ingested into `alt`, on the lane's copy stream, while the lane still scans `pages`; the two change places when that
    // batch starts (pages_alt_swap, pages.hip)
    struct PageSet {  // [capacity][rows_alloc][pitch] ink-high u8, zero padded (pages.hip: page_set_alloc)
        focr::DevArray<uint8_t> u8;
        focr::DevArray<uint8_t> i8;  // the same pages as int8 (ink - 128, i.e. byte ^ 0x80; padding = 0x80): the MFMA prefilter's window operand,
                                     // written at ingest so that the scan kernels need no v_xor per fragment dword
        size_t capacity = 0, r_w = 0, r_h = 0, pitch = 0, rows_alloc = 0;  // capacity: pages the arrays were allocated for
        bool holds(size_t n, size_t w, size_t h) const { return u8 && r_w == w && r_h == h && n <= capacity; }
    } pages, alt;
    size_t n_pages = 0;         // pages of the batch (<= pages.capacity)
    unsigned n_cus = 0;         // compute units of the device (read once, focr_ctx_create)
    unsigned scan_cus = 0;      // CUs the persistent scan kernel may occupy, 0 = all (focr_ctx_set_scan_cus)
    focr::DevArray<uint8_t> d_stage;  // device staging for uploads (exact)

    // scan results (every reserve waits for the context's stream first)
    size_t sub_p0 = 0, sub_np = 0;  // page range the scan pipeline is currently working on (normally the whole batch)
    focr::KeyFmt fmt{};
    uint32_t cap = FOCR_MAX_MATCHES;
    focr::DevArray<uint64_t> d_hit_keys, d_hit_keys_alt;  // the four hit arrays have one length (reserve_hits, scan_direct.hip)
    focr::DevArray<float> d_hit_sims, d_hit_sims_alt;
    focr::DevArray<uint32_t> d_counter;  // COUNTER_BYTES: u64 [0] hits, u64 [1] candidates, u32 [LIVE_WORD0 ..] live M-tile counts, then the scan kernels' item queues
    uint32_t scan_queues_used = 0;  // item queues handed out since the last reset (launch_scan_mfma)
    focr::DevArray<uint64_t> d_cand, d_cand_alt;
    focr::DevArray<int32_t> d_L;  // prefilter thresholds [class][page][r_h][pitchL]
    focr::DevArray<uint8_t> d_sort_tmp;  // rocPRIM's temporary storage
    size_t n_hits_raw = 0;    // hits before the cap
    size_t n_cand = 0;
    focr::DevArray<uint32_t> d_seg_count;   // [n_pages*T] capped counts
    focr::DevArray<uint64_t> d_seg_start;   // [n_pages*T] start in the sorted arrays
    focr::DevArray<uint64_t> d_seg_offset;  // [n_pages*T + 1] CSR offsets of the capped lists
    focr::DevArray<focr_match_t> d_matches;  // capped, ordered by (page, template, y, x); Grow::eighth
    // views, not owners: all hits (before the cap) in process_hits order (page, y, x, t), in the hit arrays or in acc_hkeys / acc_hsims
    uint64_t *d_hkeys = nullptr;
    float *d_hsims = nullptr;
    size_t n_hits = 0;
    size_t n_matches = 0;

    // grow-only scratch (Grow::quarter at every reserve).  scan_flags / scan_pos and ord_k2 / ord_v are bytes: their readers disagree
    // about the type (u64 flags and positions in scan_split and the legacy tail, u32 slots / f32 similarities in verify.hip and rows.hip; u64 keys /
    // f32 values in order.hip's sorting form, u32 tables in its counting form)
    focr::DevArray<uint8_t> scan_flags, scan_pos, scan_live;
    focr::DevArray<uint64_t> scan_live_list;
    // row path of the tail (rows.hip): candidates bucketed by page row, sorted + verified per row
    focr::RowHist row_hist{};   // what the scan kernels' flush path counts into (cnt == nullptr: legacy tail)
    focr::DevArray<uint32_t> rows_hits, rows_hbase, rows_big;
    uint32_t row_cap = 0;       // per-row candidate capacity the row kernel was instantiated for in the last scan
    int tail_mode = 1;          // focr_ctx_set_row_tail(): 0 = the legacy tail (radix sort + verify + compaction), 1 = hits-first row tail
                                // (verify in flush order, hits bucketed + sorted: the default)
    focr::DevArray<uint8_t> ord_k2, ord_k2_alt, ord_v, ord_v_alt, ord_keep;
    // split-batch mode: results appended sub-batch by sub-batch (scan_split: Grow::half, what is there kept)
    focr::DevArray<focr_match_t> acc_matches;
    focr::DevArray<uint64_t> acc_hkeys;
    focr::DevArray<float> acc_hsims;
    focr::DevArray<uint32_t> acc_seg_count;

    // process_hits results (device-resident; copied to the host on focr_get_lines)
    focr::DevArray<uint32_t> post_line_be, post_choice;
    focr::DevArray<uint8_t> post_keep;
    focr::DevArray<uint64_t> post_packed, post_scanned, post_page_off, post_line_off;
    focr::DevArray<focr_hit_t> post_chars;
    size_t n_chars = 0, n_lines = 0;
    std::vector<uint64_t> h_page_line_off, h_line_char_off;
    std::vector<focr_hit_t> h_chars;

    // focr_verify_images (ncc_images.hip): buffers of its own, exact growth, idle between two calls (each ends with a wait for io_stream)
    focr::DevArray<focr_dec::VerifyRec> vimg_recs;
    focr::DevArray<unsigned long long> vimg_sums;
    focr::DevArray<uint8_t> vimg_rgb;  // the image on its way to host memory
    hipEvent_t vimg_ev[2] = {};
    float vimg_ms = 0.f;
    uint32_t vimg_launches = 0;

    // focr_get_runners (post.hip): one record per character of the last process_hits, written by the first call after it
    focr::DevArray<focr_runner_t> post_runners;  // post_chars' bound, Grow::quarter; used on io_stream only, idle between two calls
    hipEvent_t run_ev[2] = {};
    float run_ms = 0.f;
    uint32_t run_launches = 0;

    // ---- validity of the results: every flag that says what of the last scan / process_hits still stands, and the four transitions
    // that withdraw results as a whole.  Elsewhere a flag changes only where the pipeline produces or consumes what it describes
    // (finish_results reads the pending sizes, materialise_matches writes the pending lists, a split batch leaves d_cand incomplete).
    bool scanned = false;        // a scan's results (or debug hits) stand: focr_scan, focr_debug_process_hits
    bool processed = false;      // ... and a focr_process_hits of them
    bool sizes_pending = false;  // the scan's sizes are still to be read from h_res (finish_results)
    bool post_pending = false;   // ... and those of its process_hits
    bool debug_hits = false;     // tests: the hits came from focr_debug_process_hits, no per-call lists stand behind them
    bool cand_intact = false;    // tests: d_cand still holds the last MFMA scan's candidates as the scan kernels left them (focr_debug_candidates)
    bool ordered = false;        // the scan path already ran the ordering pass (MFMA path); order_hits is skipped
    bool lines_on_host = false;  // h_page_line_off / h_line_char_off / h_chars hold the last process_hits' lines (fetch_lines, post.hip)
    bool runners_valid = false;  // post_runners' records belong to the last focr_process_hits
    // order.hip's counting form writes d_matches on demand (materialise_matches): pending = nobody has read the last scan's lists yet;
    // the rest is the geometry of the tables the ordering left in ord_v / ord_k2 (pages of the scan, unit capacity, the unit kernels' grid)
    struct LazyMatches {
        bool pending = false;
        uint32_t n_pages = 0;
        size_t max_units = 0;
        unsigned blocks = 0;
    } lazy;
    // tests: what the last scan's tail chose (focr_debug_tail_path; host bookkeeping, written by launch_scan_mfma, row_tail, rows2_verify and
    // the ordering pass): the values of FOCR_TAIL_* / FOCR_ORDER_* / FOCR_VERIFY_FORM_* in include/focr_ncc.h
    struct TailPath {
        uint32_t tail = 0, big_launch = 0, library_sort = 0, order_form = 0, seg_shift = 0, n_seg = 0, verify_form = 0, verify_chunks = 0;
    } tail_path;
    void sub_run_starts() {  // the pipeline starts on a page range (scan_now's run): what the previous range left behind is not this one's
        ordered = lazy.pending = false;
        tail_path = {};
    }
    void results_gone() {  // the bank or the pages changed, or a new scan starts: nothing stands
        scanned = processed = sizes_pending = post_pending = debug_hits = cand_intact = lines_on_host = runners_valid = false;
        sub_run_starts();
    }
    void post_starts() {  // focr_process_hits: the previous call's lines and runners are replaced
        processed = lines_on_host = runners_valid = false;
        n_chars = n_lines = 0;
    }
    void debug_hits_installed() {  // the caller's hits stand in for a scan's; the last scan's tail_path stays readable, as it always did
        sizes_pending = post_pending = processed = lines_on_host = runners_valid = cand_intact = lazy.pending = false;
        scanned = debug_hits = true;
    }
    // ---- end of validity ----

    template <typename T>
    bool scratch(focr::DevArray<T> &a, size_t want) {  // grow-only scratch: Grow::quarter, behind the context's stream
        return a.reserve(want, focr::Grow::quarter, &stream) == hipSuccess;
    }

    template <typename T>
    int upload(focr::DevArray<T> &a, const T *src, size_t n, size_t at_least = 0);  // a bank array from host memory (ctx.hip: fail() on error)

    hipEvent_t ev[N_PHASE_EVENTS] = {};  // PhaseEvent
    float ms[N_TIMINGS] = {};            // TimingSlot
    uint64_t counters[N_COUNTERS] = {};  // CounterSlot

    // per-launch timing of the scan kernels (focr_last_launches)
    static constexpr uint32_t NO_SUPER = 0xffffffffu;
    std::vector<focr_launch_info_t> launches;  // the public records, as focr_last_launches copies them out
    std::vector<uint32_t> launch_super;        // beside them: the super-class whose live M-tile count scales the launch's issued_macs (NO_SUPER: none)
    std::vector<hipEvent_t> launch_events;     // pool, two per launch
    void launch_begin(const char *name, uint32_t n_templates, uint64_t alg, uint64_t issued, uint32_t super_index = NO_SUPER);
    void launch_end();
    void launches_reset() { launches.clear(), launch_super.clear(); }
    void launches_collect();  // after a stream sync: fill ms
};

namespace focr {

void set_global_error(const std::string &s);
int fail(focr_ctx *ctx, int code, const std::string &msg);

}  // namespace focr
template <typename T>
int focr_ctx::upload(focr::DevArray<T> &a, const T *src, size_t n, size_t at_least) {
    const hipError_t e = a.upload(src, n, at_least);
    return e == hipSuccess ? FOCR_OK : focr::fail(this, FOCR_ERR_NO_DEVICE, std::string("bank upload: hipMalloc / hipMemcpy: ") + hipGetErrorString(e));
}
namespace focr {

#define FOCR_HIP(ctx, expr)                                                                       \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return focr::fail((ctx), FOCR_ERR_NO_DEVICE,                                          \
                              std::string(#expr) + ": " + hipGetErrorString(e_));                 \
    } while (0)

// Every function one .hip file defines and another calls (the decoder's: decode.h; those that need mfma_common.h's types: there).
// The defining file includes this header too, so a signature that drifts is a compile error, not a link error at the call site.
// scan_direct.hip
int launch_scan_direct(focr_ctx *ctx, float threshold, int rust_formula);
int launch_scan_tall(focr_ctx *c, size_t k, double thr_d, uint64_t *keys, float *sims, unsigned long long *counter,
                     unsigned long long capacity, int rust);
int reserve_hits(focr_ctx *c, size_t want);
// scan_mfma.hip
int launch_scan_mfma(focr_ctx *ctx, float threshold);
// stats.hip
int launch_clear(focr_ctx *c, const focr::ClearList &l);  // zero every region of the list in one launch
int pass_stats(focr_ctx *c, const ScanPlan &P, size_t si, double thr_d);  // one scan pass's statistics launches and its work list, queued on the context's stream
bool pass_appends(const focr_ctx *c, const SuperClass &su);               // a plane pass's statistics append the work list themselves (no mark bytes)
// bank_mfma.hip (host only)
int build_mfma_bank(focr_ctx *ctx, const uint8_t *needles);
void layout_supers(focr_ctx *c);  // size classes -> super-classes, MFMA K layouts, bank offsets
int quantise_bank(focr_ctx *c, const uint8_t *dense, std::vector<int8_t> &qbank, std::vector<uint32_t> &tglobal, std::vector<uint32_t> &order_of);
// rows.hip: the row path of the tail
bool rows_applicable(const focr_ctx *c);
uint32_t rows_capacity_for(uint64_t row_max);
void row_segments(const focr_ctx *c, uint32_t *seg_shift, uint32_t *n_seg);
size_t row_buckets(const focr_ctx *c);
unsigned tail_grid(const focr_ctx *c, unsigned blocks);  // a persistent tail kernel's grid under the test hook focr_debug_set_tail_grid
int rows2_begin(focr_ctx *c, ClearList &clear);  // the hits-first tail: verify in flush order, then only hits are placed and sorted
int rows2_place(focr_ctx *c, const unsigned long long *n_cand_p, size_t ub_c, size_t ub_h, bool big_expected, bool sort);
// verify.hip: the exact verify of the candidate list
int rows2_verify(focr_ctx *c, double thr_d, const unsigned long long *n_cand_p, size_t ub_c);  // the hits-first tail's: slots per bucket, their prefix
int legacy_verify(focr_ctx *c, double thr_d, const unsigned long long *n_cand_p, size_t ub_c, float *sims, uint64_t *flags);  // the legacy tail's: flags in place
// order.hip
int sort_keys_u64(focr_ctx *c, DevArray<uint64_t> &keys, DevArray<uint64_t> &keys_alt, size_t n, unsigned end_bit);
int sort_pairs_u64_f32(focr_ctx *c, DevArray<uint64_t> &keys, DevArray<uint64_t> &keys_alt, DevArray<float> &vals, DevArray<float> &vals_alt, size_t n, unsigned end_bit);
int exclusive_scan_u64(focr_ctx *c, const uint64_t *in, uint64_t *out, size_t n);
int compact_candidates(focr_ctx *c, const uint64_t *keys, const float *sims, const uint64_t *flags, uint64_t *pos,
                       const unsigned long long *n_cand_p, size_t ub_c);
int order_sorted_hits(focr_ctx *c, uint64_t *hkeys, float *hsims, const uint64_t *n_p, size_t ub, const unsigned long long *n_cand_p, size_t ub_c);
int order_hits(focr_ctx *ctx);  // direct path: unordered hits in d_hit_keys / d_hit_sims -> everything below
int materialise_matches(focr_ctx *c, hipStream_t s);  // d_matches of the last scan, if still to be written, on stream s (after finish_results)
// ctx.hip
void bank_host_prepare(focr_ctx *c, const focr_template_t *templates, size_t n_templates, const uint8_t *needles,
                       std::vector<uint32_t> &direct, std::vector<uint8_t> &dense);
void ctx_share_stream(focr_ctx *c, hipStream_t lane_stream, hipStream_t io_stream);  // the context joins an executor's lane
int wait_batch(focr_ctx *c);  // until the context's queued work is done (its batch's event inside an executor, else its stream)
// pages.hip
int pages_alt_ingest(focr_ctx *c, const void *d_luma, size_t n_pages, size_t r_w, size_t r_h, int invert, hipStream_t s);
int pages_alt_swap(focr_ctx *c, size_t n_pages, size_t r_w, size_t r_h);
// results.hip
int finish_results(focr_ctx *c);  // wait for the stream once and read the result sizes of the last scan / process_hits
int install_host_hits(focr_ctx *c, uint64_t n);  // n, a count the host knows, becomes the device-side hit count (d_n_hits, ub_hits): a copy queued on the context's stream
void phase_origin_record(int device, hipStream_t s);  // the device's first context stamps the origin of focr_debug_phase_stamps
// post.hip
bool post_queue_chars_copy(focr_ctx *c, void *dst, size_t dst_bytes);  // the batch's characters to a device buffer, queued on the context's stream

// ---- device helpers: the reference's f64 epilogue, operation for operation ----
// Compiled with -ffp-contract=off: the only fused operation is the explicit fma.

// patch_rnorm, src/ncc.rs:309-311: 1 / sqrt(s2 - (s*s)/n), IEEE division and sqrt.
__device__ __forceinline__ double window_rnorm(uint32_t s_p, uint64_t s2_p, double n_d) {
    double norm = (double)s2_p - ((double)((uint64_t)s_p * (uint64_t)s_p)) / n_d;
    return 1.0 / __builtin_sqrt(norm);
}

// similarity, src/ncc.cpp:352-361 (== 207-215): fnmadd(s_n * s_p, 1/n, acc) * (rnorm_n * rnorm_p)
// with the vector path's signed int32 -> f64 conversions (_mm256_cvtepi32_pd).
__device__ __forceinline__ double ncc_similarity(uint32_t acc, uint32_t s_p, double s_n_d, double n_recip,
                                                 double rnorm_n, double rnorm_p) {
    double num = __builtin_fma(-(s_n_d * (double)(int32_t)s_p), n_recip, (double)(int32_t)acc);
    double den = rnorm_n * rnorm_p;
    return num * den;
}

// The scalar Rust scan's arithmetic and skips (`ncc --rust`, src/ncc.rs:431-433, 445-470): returns "emits".
__device__ __forceinline__ bool rust_similarity(uint32_t acc, uint32_t s_p, uint64_t s2_p, double s_n_d, double norm2_n,
                                                double n_d, double thr_d, double *sim) {
    if (s_n_d == 0.0 || s_p == 0) return false;                                          // :431-433, :447-449
    const double num = (double)acc - (double)((uint64_t)s_n_d * (uint64_t)s_p) / n_d;    // :450
    if (num < 0.) return false;                                                          // :451-453
    const double norm2_p = (double)s2_p - (double)((uint64_t)s_p * (uint64_t)s_p) / n_d;  // :456
    const double den = __builtin_sqrt(norm2_n * norm2_p);                                // :459
    *sim = num / den;                                                                    // :460
    return !(*sim == __builtin_inf()) && *sim > thr_d;                                   // :466
}

// emit test, src/ncc.cpp:362-366: (sim > thr) && !(sim == +inf); NaN fails both compares.
__device__ __forceinline__ bool ncc_emits(double sim, double thr_d) {
    return (sim > thr_d) && !(sim == __builtin_inf());
}

}  // namespace focr
