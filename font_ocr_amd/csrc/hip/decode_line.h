// decode_line.h — what the translation units of the `focr` line decoder share (decode.hip: prepass, compaction, the pen
// loop and its search, and the run itself; decode_whole.hip: the whole-line decode; decode_baseline.hip: the baseline
// search; decode_whole_baseline.hip: the whole-line decode under every baseline candidate; decode_fonts.hip and
// decode_whole_fonts.hip: the pen loop and the whole-line decode under every candidate font): the strip's constants, the
// device helpers the files' kernels call (no relocatable device code: they are inlined into each), and the steps of a run
// that live beside their kernels: the whole-line decode's plan, buffers and launch, and the baseline search's buffers and
// launch.  Each takes the run's RunMode (decode.h) and reads no setting.
#pragma once

#include "decode.h"

namespace focr_dec {

constexpr uint32_t PAD = 4;                 // zero bytes left of a strip row (reads up to 3 bytes left of column 0)
constexpr uint32_t LDS_STRIP_MAX = 65536;   // the strip is staged in LDS up to this many bytes, else read from global

__device__ __forceinline__ uint32_t edge_mask(int base, int w) {
    uint32_t m = 0;
    for (int b = 0; b < 4; b++)
        if (base + b >= 0 && base + b < w) m |= 0xffu << (8 * b);
    return m;
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}

// The pen offset of a rank, lowest rank first: rank(0) = 0, rank(-1) = 1, rank(+1) = 2, ...
__device__ __forceinline__ int rank_offset(uint32_t rank) { return rank & 1 ? -(int)((rank + 1) >> 1) : (int)(rank >> 1); }

// The footprint term of one glyph rendering against a strip: the sum over the bitmap's pixels inside the crop (w columns,
// h rows) of c * (c - 2 r), the inner loop of line_decode_kernel.  line_decode_kernel and line_search_kernel keep their own
// copy: calling this from them changes their machine code (tools/isa_hash.py), and the plain decoder's instruction stream
// is what its benchmark pins.
__device__ __forceinline__ int footprint_term(const uint32_t *strip, uint32_t sdw, int w, uint32_t h, const uint32_t *__restrict__ tile,
                                              uint32_t ndw, uint32_t box_h, int x0, int y0) {
    const int r_lo = std::max(0, -y0), r_hi = std::min((int)box_h, (int)h - y0);
    uint32_t cc = 0, cr = 0;
    for (int r = r_lo; r < r_hi; r++) {
        const uint32_t *srow = strip + (size_t)(y0 + r) * sdw;
        const uint32_t *trow = tile + (size_t)r * ndw;
        for (uint32_t q = 0; q < ndw; q++) {
            const int base = x0 + 4 * (int)q;
            if (base <= -4 || base >= w) continue;
            uint32_t c = trow[q];
            if (base < 0 || base + 4 > w) c &= edge_mask(base, w);
            const uint32_t a = (uint32_t)(base + (int)PAD);
            const uint32_t rv = __builtin_amdgcn_alignbyte(srow[(a >> 2) + 1], srow[a >> 2], a & 3);
            cr = __builtin_amdgcn_udot4(c, rv, cr, false);
            cc = __builtin_amdgcn_udot4(c, c, cc, false);
        }
    }
    return (int)cc - 2 * (int)cr;
}

// ---- the whole-line decode as focr_decoder_run sees it (decode_whole.hip) --------------------------------------------

// The plan of a whole-line run: what whole_plan works out from the font, the mode and the geometry before anything is
// launched, and the launch launches from.  A font search (pen loop or whole-line) also plans its candidates here.
struct WholePlan {
    std::vector<FontDesc> fonts;        // a font search: the candidates 0 ..= K (fonts_plan; whole_plan fills the whole-line part)
    std::vector<uint32_t> fonts_inc64;  // ... and under the whole-line form their inc64, candidate-major
    std::vector<uint32_t> inc64;  // per glyph: the pen increment in 1/64 px
    int origin_d = 0;             // 64 * origin_x
    uint32_t batch = 0;           // B: states per batch
    uint32_t ring = 0;            // keys of the cost ring, a power of two
    uint32_t max_inc = 0;         // the largest inc64
    uint32_t n_states = 0;        // words of one workgroup's scratch
    uint32_t cap = 1;             // characters per line at most
    uint32_t grid = 0;            // workgroups
};

// The font and width refusals of a whole-line run of any kind (include/focr_decode.h) and its plan for the batch of
// geometry g (g.w and g.total).
int whole_plan(focr_decoder *dec, const RunMode &mode, const Geometry &g, WholePlan *plan);
// The run's scratch and result buffers and the font's inc64 table; g.cap is the plan's.
int whole_reserve(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan);
// The third launch of a whole, whole_margins or whole_slack run, on the decoder's stream; the caller checks hipGetLastError.
void whole_launch(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan, size_t strip_bytes);
// ... and of a whole_baseline run (decode_whole_baseline.hip): line_whole_baseline_kernel, or its form on the fractional grid.
void whole_baseline_launch(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan, size_t strip_bytes);

// ---- the baseline search as focr_decoder_run sees it (decode_baseline.hip) -------------------------------------------

// The run's per-line result buffers.
int baseline_reserve(focr_decoder *dec, const Geometry &g);
// The third launch of a baseline run, on the decoder's stream: line_baseline_kernel, or its form on the fractional grid;
// the caller checks hipGetLastError.
void baseline_launch(focr_decoder *dec, const RunMode &mode, const Geometry &g, size_t strip_bytes);

// ---- the font search as focr_decoder_run sees it (decode_fonts.hip, decode_whole_fonts.hip) ----------------------------

// The candidates' descriptors into plan->fonts: the decode font, then the uploaded ones.
int fonts_plan(focr_decoder *dec, WholePlan *plan);
// The run's per-line result buffers and the descriptors on the device.
int fonts_reserve(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan);
// The third launch of a fonts run, on the decoder's stream: line_fonts_kernel; the caller checks hipGetLastError.
void fonts_launch(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan, size_t strip_bytes);
// ... and of a whole_fonts run (decode_whole_fonts.hip): line_whole_fonts_kernel.
void whole_fonts_launch(focr_decoder *dec, const RunMode &mode, const Geometry &g, const WholePlan &plan, size_t strip_bytes);
// The uploaded candidates and their device tables, gone (focr_decoder_set_font).
void drop_font_candidates(focr_decoder *dec);
// ... and the y-phase fonts (decode_baseline.hip).
void drop_baseline_fonts(focr_decoder *dec);

}  // namespace focr_dec
