// align_plan.h — the host's plan of a forced alignment (focr_decoder_align_text, decode_align.hip) on top of the reading's own
// rules (text_plan.h, which it leaves as they are): the two radii against their maxima, every listed character's nominal pen
// m_g = start + the running sum of inc64 from the host font records' increments, the rule that keeps every pen of the band exact in
// f32 and in the device's int arithmetic (start + sum of inc64 + W < 2^24 per line), the whole origin_x the pens placement needs, the
// budget of the call's backpointers, and the record the device reads of a line beside its TextRec.  Pure functions that return the
// refusal's text behind the entry point's prefix (empty: accepted).  Plain host code, no HIP runtime and no decoder:
// align_plan_check.cpp asserts it at the edges of its arithmetic under the sanitizers with a host compiler alone.
#pragma once

#include <cmath>

#include "text_plan.h"

namespace focr_dec {

constexpr uint64_t ALIGN_BACK_MAX = 256ull << 20;  // bytes of backpointers one call may ask for
constexpr uint32_t ALIGN_PEN_END = 1u << 24;       // every pen of every band stays below this

// One listed line as the device reads it beside its TextRec: where its backpointers start in the call's scratch, one byte per
// state, character-major: (out + g) * (2W + 1) + (e + W).
struct AlignRec {
    uint64_t back;
};

struct AlignPlan {
    std::vector<uint32_t> nominal;  // m_g of every listed character, line l's at recs[l].out (the running sum of n)
    std::vector<AlignRec> recs;
    uint64_t back_bytes = 0;        // n_out * (2W + 1)
};

// (int)rintf(increment * 64), the whole-line programme's inc64, as far as a pen below 2^24 can use it: ALIGN_PEN_END for an
// increment that alone passes it (the cast would not be defined there).
inline uint32_t align_inc64(float increment) {
    const float v = rintf(increment * 64.0f);
    return v < (float)ALIGN_PEN_END ? (uint32_t)(int)v : ALIGN_PEN_END;  // increments are > 0 (pack_font)
}

// The radii alone: what is refused whatever the lines.
inline std::string plan_align_radii(uint32_t drift, uint32_t step) {
    if (drift > FOCR_ALIGN_DRIFT_MAX) return "the drift radius is at most 1024 (16 pixels)";
    if (step > FOCR_PEN_SEARCH_MAX) return "the step radius is at most 64 (one pixel)";
    return {};
}

// The lines of an accepted reading (plan_text_lines' records; plan_text_chars has passed, so every character indexes a font's
// increments) against the fonts 0 ..= K, from `start` with drift radius W = drift.
inline std::string plan_align(const TextInput &in, const std::vector<TextRec> &lines, uint64_t n_out, const HostFont &font, const std::vector<HostFont> &cands,
                              uint32_t start, uint32_t drift, AlignPlan *out) {
    *out = AlignPlan{};
    const uint64_t band = 2ull * drift + 1;
    // before anything of the call's size is allocated, on the host as well; the quotient, so that no product can wrap
    if (n_out > ALIGN_BACK_MAX / band)
        return "the backpointers of the call (" + std::to_string(n_out) + " characters x " + std::to_string(band) +
               " states) pass 256 MiB: list fewer lines or ask for less drift";
    out->back_bytes = n_out * band;
    out->recs.resize(lines.size());
    out->nominal.resize(n_out);
    for (size_t l = 0; l < lines.size(); l++) {
        const TextRec &t = lines[l];
        const std::string pre = "line " + std::to_string(l) + ": ";
        const HostFont &f = t.font ? cands[t.font - 1] : font;
        if (!whole_origin(f.origin_x)) return pre + "an alignment needs its font's origin_x to be a whole number >= 0 (at most 65536)";
        uint64_t pen = start;  // below 2^32; every step adds at most 2^24 and is checked: no wrap
        for (uint32_t g = 0; g < t.n; g++) {
            if (pen + drift >= ALIGN_PEN_END) break;
            out->nominal[t.out + g] = (uint32_t)pen;
            pen += align_inc64(f.inc[in.chars[t.first + g]]);
        }
        if (pen + drift >= ALIGN_PEN_END) return pre + "start + the sum of its increments + drift is 2^24 / 64 px or more (pens must stay exact in f32)";
        out->recs[l] = AlignRec{t.out * band};  // below 2^32 * 2049
    }
    return {};
}

}  // namespace focr_dec
