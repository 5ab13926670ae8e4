// scan_mfma.hip — the fast scan's host driver: i8 MFMA conservative prefilter + exact verify.
//
// The reference evaluates, for every window w and template t (src/ncc.cpp:302-392),
//     sim = num / (norm_n * norm_p),  num = sum_k a_k b_k - s_n s_p / n = sum_k a_k (b_k - mean_t)
// and emits iff sim > thr.  Almost no (w, t) pair passes, so the device splits the work:
//
//  1. window statistics (stats.hip): per size class and window the prefilter THRESHOLD L(w) as an int16 "threshold plane"
//     (mfma_common.h; int32 tables on the legacy path), and the work list of the 16-window M-tiles that have a live window.
//  2. MFMA prefilter (scan_mfma2.hip) against the quantised bank (bank_mfma.hip: the bound, and why it has no false negatives).
//     Survivors go to a candidate list.
//  3. the hits-first row tail: candidates verified exactly where they lie (verify.hip) — the reference formula, operation for
//     operation (verify.h / common.h) — hits bucketed by page row and sorted per bucket (rows.hip); order.hip derives
//     the per-call ranks and the cap.  (verify_kernel, verify.hip, + the library radix sort = the legacy tail, kept as a fallback.)
//
// Sizes: every phase behind the scan kernel takes its element count from device memory; exact / estimated mode: see
// launch_scan_mfma and results.hip (finish_results).
//
// Layout: one operand = windows (fragments straight from the page's int8 copy), the other = the quantised bank staged once per
// block in LDS in exactly the per-lane order the MFMA wants; the K layouts (how image rows map to 16-byte k-groups) are
// in mfma_common.h.
#include <algorithm>
#include <cmath>
#include <mutex>

#include "mfma_common.h"

namespace focr {

// Process-wide hand-over between the contexts of one device (events are never destroyed).  A Turn holds the chain's lock from its wait
// on the previous turn (begin) to the record of its own when it goes out of scope, error returns included; nothing in it waits on the host.
struct TurnChain {
    std::mutex mu;
    static constexpr unsigned RING = 8;
    hipEvent_t ev[RING] = {};
    unsigned n = 0;
};
static TurnChain scan_turns[64], stats_turns[64];  // per device: the scan kernels', and the statistics' in front of them

struct Turn {
    focr_ctx *c;
    TurnChain &chain;
    std::lock_guard<std::mutex> lock;
    bool entered = false;
    Turn(focr_ctx *c, TurnChain &chain) : c(c), chain(chain), lock(chain.mu) {}
    int begin() {
        for (hipEvent_t &e : chain.ev)
            if (!e) FOCR_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        if (chain.n) FOCR_HIP(c, hipStreamWaitEvent(c->stream, chain.ev[(chain.n - 1) % TurnChain::RING], 0));
        entered = true;
        return FOCR_OK;
    }
    ~Turn() { if (entered) (void)hipEventRecord(chain.ev[chain.n++ % TurnChain::RING], c->stream); }
};

// THE decision whether a pass takes the threshold planes: the planes it takes (the kernel is instantiated for 1 / 2 / 4 values), or
// 0 for the legacy path — more than 4 K-steps or 4 size classes, the legacy prefilter asked for, or planes beyond 32-bit offsets
static size_t pass_planes(const focr_ctx *c, const SuperClass &su, size_t plane) {
    const size_t nv = su.classes.size(), n = nv <= 1 ? 1 : nv <= 2 ? 2 : 4;
    const bool ok = su.ksteps <= 4 && nv <= (size_t)MAX_PLANE_VALUES && c->prefilter != FOCR_PREFILTER_LEGACY && n * plane * 2 < ((size_t)1 << 32);
    return ok ? n : 0;
}

// The passes of a scan of c->sub_np pages of c->pages.r_w x c->pages.r_h (host only; also what the host model reports, prefilter_model.hip): per
// super-class the window enumeration, the offset of its M-tiles in the work list and of its planes in d_planes (`plane`: int16 values
// of one plane).  Totals: M-tiles of all passes, plane values, and whether a pass takes the int32 tables.
int plan_passes(focr_ctx *c, size_t plane, size_t &tiles_total, size_t &plane_vals, bool &need_L) {
    tiles_total = plane_vals = 0;
    need_L = false;
    for (SuperClass &su : c->supers) {
        // windows of the pass: those of its smallest searchable class
        su.min_w = su.min_h = 0xffffffffu;
        for (uint32_t k : su.classes) {
            const SizeClass &sc = c->bank.classes[k];
            if (sc.n_w >= c->pages.r_w || sc.n_h >= c->pages.r_h) continue;
            su.min_w = std::min(su.min_w, sc.n_w);
            su.min_h = std::min(su.min_h, sc.n_h);
        }
        su.mtx = su.n_rows = 0;
        su.live_offset = tiles_total;
        su.planes = su.paired = false;
        if (su.min_w == 0xffffffffu) continue;  // nothing searchable
        su.mtx = (uint32_t)((c->pages.r_w - su.min_w + 1 + 15) / 16);  // windows x in [0, r_w - min n_w]
        su.n_rows = (uint32_t)(c->pages.r_h - su.min_h);               // y in [1, r_h - min n_h]
        const uint64_t nt = (uint64_t)su.mtx * su.n_rows * c->sub_np;
        if (nt >= 0x7fffffffull) return fail(c, FOCR_ERR_INVALID, "scan_mfma: batch too large for 32-bit tile ids; scan fewer pages per call");
        tiles_total += (size_t)nt;
        const size_t n_planes = pass_planes(c, su, plane);
        su.planes = n_planes != 0;
        // THE decision whether the pass scans two window rows per fragment load (scan_mfma2.hip, PAIR): the bank holds the second operand
        // image (layout_supers), the pass is the plane kernel's one launch, and its work list comes from the statistics' own append — the
        // only list made of row pairs (stats.hip; the mark bytes of compact_live_tiles stay per row)
        su.paired = su.pairable && su.planes && pass_appends(c, su);
        su.plane_off = plane_vals;
        plane_vals += n_planes * plane;
        need_L |= !su.planes;
    }
    return FOCR_OK;
}

static int plan_scan(focr_ctx *c, bool nothing, size_t want_cand, ScanPlan &P) {
    // the buffers the scan sizes itself: exactly what is wanted, unless they already hold that much
    const auto exact = [c](auto &a, size_t want, const char *what) {
        return a.reserve(want, Grow::exact, &c->stream) ? fail(c, FOCR_ERR_NOMEM, std::string("scan_mfma: hipMalloc(") + what + ") failed") : FOCR_OK;
    };
    if (int rc = exact(c->d_cand, want_cand, "cand")) return rc;
    if (nothing) return FOCR_OK;  // no statistics, no scan
    if (c->supers.size() > LIVE_WORDS) return fail(c, FOCR_ERR_INVALID, "scan_mfma: too many super-classes");
    P.Lpitch = (uint32_t)((c->pages.r_w + 63) / 64 * 64 + 64);
    P.Lrows = (uint32_t)((c->pages.r_h + 7) / 8 * 8 + 8);
    P.L_per_class = c->n_pages * (size_t)P.Lrows * P.Lpitch;
    P.plane = c->sub_np * (size_t)P.Lrows * P.Lpitch;
    size_t plane_vals = 0;
    bool need_L = false;
    if (int rc = plan_passes(c, P.plane, P.tiles_total, plane_vals, need_L)) return rc;
    if (int rc = exact(c->d_L, need_L ? P.L_per_class * c->bank.classes.size() : 0, "negL")) return rc;
    if (int rc = exact(c->d_planes, plane_vals, "planes")) return rc;
    if (!c->scratch(c->scan_live, P.tiles_total + 24) || !c->scratch(c->scan_live_list, P.tiles_total + 16)) return fail(c, FOCR_ERR_NOMEM, "scan_mfma: hipMalloc failed");
    P.live = c->scan_live;
    P.live_list = c->scan_live_list;
    return FOCR_OK;
}

// 1. the clear launch, then statistics + live-tile work lists per super-class (classes that share one scan pass: pass_stats, stats.hip).
// The statistics of the batches of one device take turns (an event chain like the scan kernels'): two lanes that start their
// statistics at the same moment — a pipeline filling up from a drained state does that — share the free CUs, finish together, then
// wait for their scan turns one behind the other, and their tails overlap again: a second steady state with the same work and 7 % less
// throughput (two batches completing together, then 2.5 and 3.0 ms: DESIGN.md section 5, "two rhythms").  In the staggered state a
// batch's statistics never meet another's, and the chain costs nothing.
static int stats_phase(focr_ctx *c, const ScanPlan &P, ClearList &clear, double thr_d) {
    if (!clear.add(P.live, P.tiles_total + 16)) return fail(c, FOCR_ERR_INVALID, "scan_mfma: clear list full or region too large");
    Turn turn(c, stats_turns[(unsigned)c->device % 64]);
    int rc = turn.begin();
    if (rc || (rc = launch_clear(c, clear))) return rc;
    for (size_t si = 0; si < c->supers.size(); si++)
        if (c->supers[si].mtx && (rc = pass_stats(c, P, si, thr_d))) return rc;
    FOCR_HIP(c, hipEventRecord(c->ev[EV_STATS_END], c->stream));
    return FOCR_OK;
}

// 2. MFMA prefilter: one launch per (super-class, bank chunk that fits the LDS budget), then the tall classes.
// With several contexts in flight on one GPU the persistent scan kernels take turns: each context's launches wait (on the device,
// hipStreamWaitEvent) for the previous context's to finish.  Two of them sharing the MFMA pipes finish no sooner than one after the
// other; in turn each runs at its full rate while the other contexts' small kernels use the CUs left free by focr_ctx_set_scan_cus.
// (An executor queues its batches from ONE thread in ticket order, pipe.hip: its scans enter this chain in that order with no
// host-side gate; contexts driven by threads of their own take their turn in the order they get here.)
static int scan_phase(focr_ctx *c, const ScanPlan &P, double thr_d) {
    int rc = FOCR_OK;
    {
        Turn turn(c, scan_turns[(unsigned)c->device % 64]);
        if ((rc = turn.begin())) return rc;
        for (size_t si = 0; si < c->supers.size(); si++) {
            const SuperClass &su = c->supers[si];
            if (!su.mtx) continue;
            const uint32_t chunk_tiles = mfma2_chunk_tiles(su.ksteps);
            uint32_t t0 = 0;
            while (t0 < su.n_tiles) {
                MfmaLaunch L{};
                L.layout = su.layout;
                L.ksteps = su.ksteps;
                L.Lpitch = P.Lpitch;
                L.Lrows = P.Lrows;
                L.mtx = su.mtx;
                L.n_rows = su.n_rows;
                L.live_list = P.live_list + su.live_offset;
                L.live_count = c->d_counter + LIVE_WORD0 + si;
                L.super_index = (uint32_t)si;
                const uint32_t t_limit = std::min(su.n_tiles, t0 + chunk_tiles);
                uint32_t t1 = t0;
                PlaneArgs A3{};
                for (size_t i = 0; i < su.classes.size() && L.segs.n < (uint32_t)MAX_SEGS; i++) {
                    const SizeClass &sc = c->bank.classes[su.classes[i]];
                    const uint32_t cb = su.tile_first[i], ce = cb + sc.n_tiles16;
                    const uint32_t b = std::max(cb, t1), e = std::min(ce, t_limit);
                    if (b >= e || b != t1) continue;  // segments must tile [t0, t1) contiguously
                    if (!su.planes && (sc.n_w >= c->pages.r_w || sc.n_h >= c->pages.r_h)) {  // no searchable window: skip the class's tiles
                        if (L.segs.n == 0) {
                            t0 = t1 = e;
                            continue;
                        }
                        break;
                    }
                    A3.shift[L.segs.n] = plane_params(c, su.classes[i], thr_d).shift;  // the unit of the class's plane
                    A3.seg_value[L.segs.n] = (uint32_t)i;
                    A3.seg_full[L.segs.n] = (su.layout == LAYOUT_W12 && sc.keep_w <= 8) ? 0u : 1u;  // mfma_common.h: K layouts
                    const uint32_t dead = cb + sc.n_live / 16;  // tiles of the class from n_live / 16 on hold dead / padding slots
                    A3.seg_dead_from[L.segs.n] = dead > t0 ? dead - t0 : 0u;  // chunk-local numbering
                    MfmaSeg &sg = L.segs.s[L.segs.n++];
                    sg.negL = c->d_L + su.classes[i] * P.L_per_class;
                    sg.tile_end = e - t0;
                    const uint32_t real = std::min(sc.n_templates, (e - cb) * 16) - (b - cb) * 16;
                    L.n_templates += real;
                    if (sc.n_w < c->pages.r_w && sc.n_h < c->pages.r_h)
                        L.alg_macs += (uint64_t)(c->pages.r_w - sc.n_w) * (c->pages.r_h - sc.n_h) * sc.n_w * sc.n_h * real * c->sub_np;
                    t1 = e;
                }
                if (L.segs.n == 0) {
                    if (t1 == t0) break;
                    continue;
                }
                L.n_tiles16 = t1 - t0;
                L.q_offset = su.q_offset + (size_t)t0 * su.ksteps * 1024;
                L.tg_offset = su.tg_offset + (size_t)t0 * 16;
                const unsigned cus = c->scan_cus ? std::min(c->scan_cus, c->n_cus) : c->n_cus;
                if (c->scan_queues_used >= MAX_SCAN_QUEUES) return fail(c, FOCR_ERR_INVALID, "scan_mfma: too many scan passes for one call (bank too large)");
                L.queue = c->d_counter + COUNTER_WORDS + (size_t)(c->scan_queues_used++) * QUEUE_XCDS * QUEUE_STRIDE;
                if (su.paired && (t0 != 0 || t1 != su.n_tiles)) return fail(c, FOCR_ERR_INVALID, "scan_mfma: internal: a paired pass in more than one launch");
                L.paired = su.paired;
                if (su.planes) {
                    A3.planes = c->d_planes + su.plane_off;
                    A3.stride = P.plane;
                    A3.nv = (uint32_t)su.classes.size();
                    rc = dispatch_mfma_v2s(c, L, A3, cus);
                } else {
                    rc = dispatch_mfma_v2(c, L, cus);
                }
                if (rc) return rc;
                t0 = t1;
            }
        }
    }
    // tall classes: exact scan straight into the candidate list
    for (size_t k = 0; k < c->bank.classes.size(); k++) {
        const SizeClass &sc = c->bank.classes[k];
        if (!sc.tall || sc.n_w >= c->pages.r_w || sc.n_h >= c->pages.r_h) continue;
        if ((rc = launch_scan_tall(c, k, thr_d, c->d_cand, nullptr, c->d_counter.as<unsigned long long>() + 1, (unsigned long long)c->ub_cand, 0))) return rc;
    }
    return FOCR_OK;
}

// 3a. hits-first row tail: verify the candidates where they lie (verify.hip), then bucket + sort the hits only (rows.hip)
static int row_tail(focr_ctx *c, double thr_d, const unsigned long long *n_cand_p, size_t ub_c) {
    int rc = rows2_verify(c, thr_d, n_cand_p, ub_c);
    if (rc) return rc;
    size_t ub_h = std::min(ub_c, c->est.hits);
    uint64_t row_max = c->est.row_bound();
    if (!c->estimated) {  // exact number of hits and the largest bucket
        uint64_t hits = 0;
        FOCR_HIP(c, hipMemcpyAsync(&hits, &c->d_res.p->tail_hits, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        FOCR_HIP(c, hipMemcpyAsync(&row_max, &c->d_res.p->row_max, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        FOCR_HIP(c, hipStreamSynchronize(c->stream));
        ub_h = (size_t)hits;
    }
    // buckets above the row sort's first capacity class get a second launch (rows.hip); a bucket beyond the sort's largest capacity
    // (exact sizes only: launch_scan_mfma): library sort of the placed hits
    c->row_cap = rows_capacity_for(row_max);
    const bool big_expected = row_max > 1024, sort_rows = c->row_cap != 0;
    c->tail_path.big_launch = sort_rows && big_expected;
    c->tail_path.library_sort = !sort_rows && ub_h >= 2;
    c->tail_path.seg_shift = c->row_hist.seg_shift;
    c->tail_path.n_seg = c->row_hist.n_seg;
    if ((rc = rows2_place(c, n_cand_p, ub_c, ub_h, big_expected, sort_rows))) return rc;
    if (!sort_rows && (rc = sort_pairs_u64_f32(c, c->d_hit_keys, c->d_hit_keys_alt, c->d_hit_sims_alt, c->d_hit_sims, ub_h, c->fmt.bits()))) return rc;
    return order_sorted_hits(c, c->d_hit_keys, c->d_hit_sims_alt, &c->d_res.p->tail_hits, ub_h, n_cand_p, ub_c);
}

// 3b. legacy tail: sort the candidates into emission order, verify them exactly in place (verify.hip), compact + cap (order.hip)
static int legacy_tail(focr_ctx *c, double thr_d, const unsigned long long *n_cand_p, size_t ub_c) {
    c->row_cap = 0;
    int rc = reserve_hits(c, ub_c + 1);
    if (rc) return rc;
    if (!c->scratch(c->scan_flags, (ub_c + 1) * 8) || !c->scratch(c->scan_pos, (ub_c + 1) * 8)) return fail(c, FOCR_ERR_NOMEM, "scan_mfma: hipMalloc failed");
    uint64_t *flags = c->scan_flags.as<uint64_t>(), *pos = c->scan_pos.as<uint64_t>();
    if (c->d_cand_alt.reserve(c->d_cand.cap, Grow::exact, &c->stream)) return fail(c, FOCR_ERR_NOMEM, "scan_mfma: hipMalloc(cand_alt) failed");
    if ((rc = sort_keys_u64(c, c->d_cand, c->d_cand_alt, ub_c, c->fmt.bits()))) return rc;
    if ((rc = legacy_verify(c, thr_d, n_cand_p, ub_c, c->d_hit_sims, flags))) return rc;
    FOCR_HIP(c, hipEventRecord(c->ev[EV_VERIFY_END], c->stream));
    if ((rc = compact_candidates(c, c->d_cand, c->d_hit_sims, flags, pos, n_cand_p, ub_c))) return rc;
    size_t ub_h = std::min(ub_c, c->est.hits);
    if (!c->estimated) {  // exact number of hits for the ordering pass
        uint64_t hits = 0;
        FOCR_HIP(c, hipMemcpyAsync(&hits, pos + ub_c, 8, hipMemcpyDeviceToHost, c->stream));
        FOCR_HIP(c, hipStreamSynchronize(c->stream));
        ub_h = (size_t)hits;
    }
    return order_sorted_hits(c, c->d_hit_keys, c->d_hit_sims_alt, pos + ub_c, ub_h, n_cand_p, ub_c);
}

int launch_scan_mfma(focr_ctx *c, float threshold) {
    const double thr_d = (double)threshold;  // src/ncc.cpp:83, 288
    // `sim > +inf` is never true (NaN thresholds arrive here as +inf, focr_scan): no statistics, no scan, zero candidates
    // (kappa would be inf - inf = NaN and every window of every live tile a candidate for verify to reject)
    const bool nothing = !(thr_d < (double)INFINITY);
    int rc = reserve_hits(c, std::max<size_t>(1u << 20, c->sub_np * 65536));
    if (rc) return rc;
    size_t want_cand = std::max<size_t>(c->d_cand.cap, std::max<size_t>(1u << 21, c->sub_np * 131072));
    if (c->estimated) want_cand = std::max(want_cand, c->est.cand);
    for (int attempt = 0; attempt < 4; attempt++) {
        ScanPlan P;
        if ((rc = plan_scan(c, nothing, want_cand, P))) return rc;
        c->counters[CNT_ISSUED_MACS] = 0;
        c->launches_reset();
        ClearList clear{};  // everything the scan needs zeroed: one launch (launch_clear), in front of the first kernel
        if (!clear.add(c->d_counter, COUNTER_BYTES) || !clear.add(c->d_res, offsetof(ResultBlock, host_hits)))  // counters + the scan kernels' item queues, the result block up to the host's own slot
            return fail(c, FOCR_ERR_INVALID, "scan_mfma: clear list full or region too large");
        c->scan_queues_used = 0;
        // Sizes.  Exact mode: the host reads the candidate count after the scan kernels and the hit count after the
        // verify (two waits), so every later phase runs on exact sizes.  Estimated mode (results.hip: same setup as the
        // previous scan): the counts stay on the device, grids and buffers take the previous counts + a margin (4 .. 20 %, results.hip) as bounds,
        // unused candidate slots hold the largest key so that the sort leaves them at the end; nothing waits.
        c->ub_cand = c->estimated ? std::min(c->est.cand, c->d_cand.cap) : c->d_cand.cap;
        // Tail: the row path (rows.hip) unless a row could exceed its capacity — exact mode finds out after the scan kernels,
        // estimated mode goes by the previous scan's largest row + 25 % (a larger one sets the overflow bit: batch redone).
        bool use_rows = rows_applicable(c);
        if (use_rows && c->estimated) use_rows = c->est.row_max != 0 && rows_capacity_for(c->est.row_bound()) != 0;
        c->row_hist = RowHist{};
        if (use_rows && (rc = rows2_begin(c, clear))) return rc;  // hits-first row tail: verify in flush order (verify.hip), only hits are bucketed and sorted (rows.hip)
        // legacy tail, estimated sizes: unused candidate slots hold the largest key so that the radix sort leaves them at the end
        if (c->estimated && !use_rows) FOCR_HIP(c, hipMemsetAsync(c->d_cand, 0xff, c->ub_cand * 8, c->stream));
        FOCR_HIP(c, hipEventRecord(c->ev[EV_STATS_BEGIN], c->stream));
        if (nothing) {
            if ((rc = launch_clear(c, clear))) return rc;
            FOCR_HIP(c, hipEventRecord(c->ev[EV_STATS_END], c->stream));
            use_rows = false;
        } else if ((rc = stats_phase(c, P, clear, thr_d)) || (rc = scan_phase(c, P, thr_d))) {
            return rc;
        }
        FOCR_HIP(c, hipEventRecord(c->ev[EV_SCAN_END], c->stream));
        FOCR_HIP(c, hipMemcpyAsync(c->h_live, c->d_counter + LIVE_WORD0, LIVE_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        const unsigned long long *n_cand_p = c->d_counter.as<const unsigned long long>() + 1;
        size_t ub_c = c->ub_cand;
        if (!c->estimated) {
            unsigned long long n_cand = 0;
            FOCR_HIP(c, hipMemcpyAsync(&n_cand, n_cand_p, 8, hipMemcpyDeviceToHost, c->stream));
            FOCR_HIP(c, hipStreamSynchronize(c->stream));
            if (n_cand > c->d_cand.cap) {
                if (n_cand > ((unsigned long long)1 << 31)) return fail(c, FOCR_ERR_OVERFLOW, "scan_mfma: more than 2^31 candidates in one pass");
                want_cand = (size_t)n_cand + (size_t)n_cand / 8 + 1024;
                continue;
            }
            ub_c = (size_t)n_cand;
        }
        c->cand_intact = use_rows;  // the row tail only reads d_cand; the legacy tail sorts and compacts it in place (focr_debug_candidates)
        c->tail_path.tail = use_rows ? FOCR_TAIL_ROWS : FOCR_TAIL_LEGACY;
        return use_rows ? row_tail(c, thr_d, n_cand_p, ub_c) : legacy_tail(c, thr_d, n_cand_p, ub_c);
    }
    return fail(c, FOCR_ERR_OVERFLOW, "scan_mfma: candidate buffer kept overflowing");
}

}  // namespace focr
