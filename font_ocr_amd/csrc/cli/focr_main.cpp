// focr — the reference's default binary (src/main.rs: Args at 343-385, main at 387-470) on top of the MI355X line decoder.
//
// Same flags, defaults and stdout as the reference.  Differences, all deliberate:
//   * glyphs are rasterised once per run into 64 sub-pixel phases (focr_decode_font_build), not once per candidate;
//   * pages of equal size are decoded as one device batch on one GPU; stdout is still in the order of -i;
//   * kerning <= 0 or a glyph that does not advance the pen is an error (the reference never finishes a line);
//   * --verify clips rendered text that falls outside the page (the reference panics there); its images are drawn on the
//     device (focr_decoder_verify) and written on up to 16 threads;
//   * --test draws its two images on the device (focr_decoder_test_images) from the first -i image only, as the reference
//     does; boxes that fall outside the page are clipped (the reference panics in get_pixel_mut), the decode font's
//     refusals apply (kerning <= 0, a glyph that does not advance; the reference's --test decodes nothing), line_advance 0
//     is refused, and its blend is image's Blend for Rgba<u8> restated in f32 (parity unpinned);
//   * --scores PATH is an extension: a CSV row per decoded character with its score, the runner-up and the margin between
//     them (focr_decoder_get_scores); stdout and the --verify files are the same with and without it;
//   * --pen-search N is an extension: every step also searches the pen offsets -N ..= N (in 1/64 px, at most 64) and
//     carries the chosen one forward (focr_decoder_set_pen_search); stdout stays text only, the --verify files and MSEs
//     come from the searched positions, and --scores gains a trailing pen_offset column;
//   * --whole-line is an extension for proportional fonts: every line is the text that minimises the whole line's squared
//     error over pens on the 1/64 px grid (focr_decoder_set_whole_line), not the pen loop's greedy choice; stdout stays
//     text only and --verify draws every character at its pen; with --scores or --pen-search it is a usage error;
//   * --margins PATH is an extension of --whole-line: a CSV row per decoded character with its pen, its term, and the
//     glyph and margin of the best whole line that reads another glyph over its middle (focr_decoder_get_margins);
//     stdout and the --verify files are the same with and without it; without --whole-line it is a usage error;
//   * --pen-slack N is an extension of --whole-line for text off the 1/64 px grid: every step of the whole-line decode may
//     move the pen by an offset of -N ..= N (in 1/64 px, at most 64) before its glyph is rendered
//     (focr_decoder_set_whole_slack); stdout stays text only and --verify draws every character where it was decoded;
//     without --whole-line, or with --margins or --pen-search, it is a usage error;
//   * --baseline-search N [--y-bits B] is an extension: every line is decoded at the vertical offsets -N ..= N (in steps of
//     2^-B px, N <= 32, B <= 3) and the one with the lowest summed footprint term is kept (focr_decoder_set_baseline_search);
//     stdout stays text only, --verify draws every line moved by the nearest whole row of its offset, and --baselines PATH
//     writes a CSV row per decoded line: image_index,y,q,offset_px,cost; with --scores, --pen-search or --whole-line it is a
//     usage error, and so are --y-bits and --baselines without it (or without --whole-baseline);
//   * --whole-line --whole-baseline N [--y-bits B] is an extension of --whole-line: the whole-line decode under every vertical
//     offset -N ..= N (in steps of 2^-B px), the candidate whose whole line costs least kept (focr_decoder_set_whole_baseline):
//     proportional text whose baseline is off the crop grid; stdout stays text only, --verify draws every character at its
//     pen on a canvas moved by the nearest whole row of the offset, and --baselines PATH writes its CSV; without --whole-line,
//     or with --margins or --pen-slack, it is a usage error;
//   * --y-frac N --line-advance-frac N (each in 1/64 px, N <= 63) are an extension of those two: the sub-pixel parts of --y
//     and --line-advance (focr_decoder_set_line_frac), for a leading that is not a whole number of pixels; every line is
//     cropped at the whole row of its own top and searched around its own sub-pixel part; stdout, --verify and --baselines
//     keep their formats (y is the line's crop row, q the absolute offset); without --baseline-search or --whole-baseline,
//     or with --test, they are usage errors;
//   * --font-candidate SPEC (repeatable, at most 15 times) is an extension: every line is decoded in the font of -f, -t,
//     --kerning and --hinting (candidate 0) and in every candidate, and the cheapest reading is kept
//     (focr_decoder_set_font_candidates, focr_decoder_set_font_search), by the pen loop or, with --whole-line, by the
//     whole-line decode.  SPEC is a comma-separated list of f=PATH, t=SIZE, k=KERNING and h=0|1; omitted keys take the
//     values of -f, -t, --kerning and --hinting; a path may not contain a comma.  stdout stays text only, and --fonts PATH
//     writes a CSV row per decoded line: image_index,y,font,cost (font is the candidate's index).  With --scores,
//     --pen-search, --pen-slack, --margins, --baseline-search, --whole-baseline or --verify it is a usage error, and so is
//     --fonts without it.  --verify-fonts DIR is --verify's picture of such a run (focr_decoder_verify_text): DIR/<stem>.png and
//     "<image> <mse>" on stderr exactly as --verify writes them, with every line drawn in its winning font and, under
//     --whole-line, every character at its pen; without --font-candidate it is a usage error, and --verify stays one beside it.
//   * --rank-text TEXT [--rank-shift N] is an extension that decodes nothing: TEXT, a line somebody read off the page, is
//     scored at the first line slot (-x, -y, --width, --line-height) of the first -i image under the font of -f, -t, --kerning
//     and --hinting (font 0) and under every --font-candidate (focr_decoder_score_text), each at the rigid shifts -N ..= N in
//     1/64 px (N <= 64, default 0).  stdout is a CSV: the header font,shift,cost,line_base,error and one row per font, error =
//     line_base + cost; the row with the lowest cost is the font (and its shift what to add to -x).  A character of TEXT
//     outside the alphabet is a usage error, and so is --rank-shift without --rank-text.
//   * --rank-text TEXT --rank-drift W [--rank-step N] fits every character's pen under each font instead
//     (focr_decoder_align_text from start 0: offsets of up to W / 64 px from the font's own pens, W <= 1024, consecutive
//     characters' offsets at most N / 64 px apart, N <= 64, default 2), for a page whose kerning or x is not the font's.  The CSV
//     is font,first,last,cost,line_base,error,scale,x64: the first and the last character's offset, and the least-squares line
//     of the fitted pens on the font's own (include/focr_decode.h has the sums): scale (%.6f) is the page's kerning relative to
//     the font's, x64 (%.2f) what to add to -x in 1/64 px; both are empty without two inked characters.  --rank-drift without
//     --rank-text or beside --rank-shift is a usage error, and so is --rank-step without --rank-drift.
//   * --learn FILE [--learn-min-count M] [--learn-grow G] is an extension for pages another renderer or another cut of the font
//     drew: FILE is a reading somebody TRUSTS (a few corrected pages, or a text that is known) in focr's own stdout format, one
//     line per non-blank line slot in -i order; it may stop early, and an empty line skips its slot.  The run finds the slots
//     with a plain run, learns font 0's glyph tables from the paired lines at the pen loop's placements
//     (focr_decoder_learn_text, focr_decode_font_learn: a cell with at least M samples, default 1, takes the mean of the page
//     under it inside its own ink's bounding rectangle grown by G pixels, default 0), sets the learned font, and then decodes and
//     prints everything as usual.  stderr gets one line: the characters used and skipped and the cells learned out of those with
//     ink.  Tables learned from the decoder's own reading reproduce its errors: FILE has to be right.  Plain pen loop only: with
//     --pen-search, --whole-line, --baseline-search, --whole-baseline, --font-candidate, --test or --rank-text it is a usage
//     error, and so are --learn-min-count and --learn-grow without it and a character of FILE outside the alphabet (the message
//     names the line).
//   * --refine S [--refine-radius N] is an extension for tight proportional text, where glyph footprints overlap and the sum of
//     per-glyph terms every mode minimises is no longer the page's error: after the run (the plain pen loop, --pen-search,
//     --whole-line or --pen-slack) every line's reading goes through focr_decoder_refine_text at the run's own pens: the line is
//     drawn with all its glyphs together, and in at most S <= 8 sweeps each character takes the glyph and the offset within N/64 px
//     (N <= 64, default 4) that lower the composed error the most.  stdout carries the repaired text; stderr gets one line: how
//     many characters in how many of the lines changed; --verify and every CSV stay the run's.  With --font-candidate,
//     --baseline-search, --whole-baseline, --test or --rank-text it is a usage error, and so is --refine-radius without it.
// There is no CPU fallback: without a device it exits non-zero with the error.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include "cli_common.h"
#include "focr_decode.h"
#include "focr_host.h"

namespace {

using cli::utf8_decode;
using cli::utf8_encode;
using cli::verify_path;

const char *DEFAULT_ALPHABET = "> =ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";  // src/main.rs:13-14
const size_t BATCH_PAGES = 256;

struct FontSpec {  // one --font-candidate
    std::string font;
    float text_size, kerning;
    bool hinting;
};

struct Args {
    std::vector<std::string> img, candidate_specs;
    std::vector<FontSpec> candidates;
    std::string fonts, verify_fonts, rank_text;
    bool have_fonts = false, have_verify_fonts = false, have_rank_text = false, have_rank_shift = false, have_rank_drift = false, have_rank_step = false;
    uint32_t rank_shift = 0, rank_drift = 0, rank_step = 2;
    std::string font, alphabet = DEFAULT_ALPHABET, verify, test, scores, margins, baselines;
    bool hinting = false, have_verify = false, have_test = false, have_scores = false, whole_line = false, have_margins = false;
    bool have_baselines = false, have_y_bits = false;
    uint32_t baseline_search = 0, y_bits = 0, whole_baseline = 0;
    uint32_t y_frac = 0, line_advance_frac = 0;
    bool have_y_frac = false, have_line_advance_frac = false;
    float text_size = 0.f, kerning = 1.f;
    uint32_t x = 0, y = 0, width = 0, line_height = 0, line_advance = 0, pen_search = 0, pen_slack = 0;
    bool have_text_size = false, have_width = false, have_line_height = false, have_line_advance = false;
    std::string learn;
    bool have_learn = false, have_learn_min_count = false, have_learn_grow = false;
    uint32_t learn_min_count = 1, learn_grow = 0;
    bool have_refine = false, have_refine_radius = false;
    uint32_t refine = 0, refine_radius = 4;
};

const char *USAGE =
    "Usage: focr [OPTIONS] --font <FONT> --text-size <TEXT_SIZE> --width <WIDTH> --line-height <LINE_HEIGHT> --line-advance <LINE_ADVANCE>";

[[noreturn]] void usage_error(const std::string &msg) { cli::usage_error(USAGE, msg); }
[[noreturn]] void die(const std::string &msg, int code = 101) { cli::die("focr", msg, code); }  // 101: a Rust panic's exit status

void print_help() {
    printf("%s\n\nOptions:\n"
           "  -i, --img <IMG>...                   \n"
           "  -f, --font <FONT>                    \n"
           "  -a, --alphabet <ALPHABET>            [default: %s]\n"
           "      --hinting                        \n"
           "  -t, --text-size <TEXT_SIZE>          \n"
           "  -k, --kerning <KERNING>              [default: 1]\n"
           "  -x, --x <X>                          [default: 0]\n"
           "  -y, --y <Y>                          [default: 0]\n"
           "  -w, --width <WIDTH>                  \n"
           "      --line-height <LINE_HEIGHT>      \n"
           "      --line-advance <LINE_ADVANCE>    \n"
           "      --test <TEST>                    Prefix for output test images\n"
           "      --verify <VERIFY>                Dir for verify images. Red is reference, Blue is rendered\n"
           "      --scores <SCORES>                [extension] CSV of every decoded character's score, runner-up and margin\n"
           "      --pen-search <N>                 [extension] Also search pen offsets of up to N/64 px at every step, N <= 64 [default: 0]\n"
           "      --whole-line                     [extension] Decode each line as a whole, for proportional fonts (not with scores or a pen search)\n"
           "      --margins <MARGINS>              [extension] CSV of every character's pen, term, runner-up and margin (only with the whole-line decode)\n"
           "      --pen-slack <N>                  [extension] Let every step of the whole-line decode move the pen by up to N/64 px, N <= 64 (not with margins or a pen search) [default: 0]\n"
           "      --baseline-search <N>            [extension] Decode every line at the vertical offsets -N ..= N, in steps of 2^-B px (--y-bits), and keep the best, N <= 32 (only with the plain pen loop) [default: 0]\n"
           "      --whole-baseline <N>             [extension] Run the whole-line decode under the vertical offsets -N ..= N, in steps of 2^-B px, and keep the line that costs least, N <= 32 (only with the whole-line decode; not with margins or a pen slack) [default: 0]\n"
           "      --y-bits <B>                     [extension] Sub-pixel bits of the baseline search's step, B <= 3 [default: 0]\n"
           "      --baselines <BASELINES>          [extension] CSV of every line's chosen vertical offset and cost (only with a baseline search)\n"
           "      --y-frac <N>                     [extension] Sub-pixel part of --y in 1/64 px, N <= 63 (only with a baseline search or --whole-baseline) [default: 0]\n"
           "      --line-advance-frac <N>          [extension] Sub-pixel part of --line-advance in 1/64 px, N <= 63 (only with a baseline search or --whole-baseline) [default: 0]\n"
           "      --font-candidate <SPEC>...       [extension] Also decode every line in this font and keep the cheapest reading; SPEC is f=PATH,t=SIZE,k=KERNING,h=0|1, omitted keys as -f, -t, --kerning, --hinting; at most 15 (only with the plain pen loop or the plain whole-line decode; not with --verify)\n"
           "      --fonts <FONTS>                  [extension] CSV of every line's winning font candidate and cost (only with --font-candidate)\n"
           "      --verify-fonts <DIR>             [extension] Dir for verify images of a --font-candidate run: every line drawn in its winning font (only with --font-candidate)\n"
           "      --rank-text <TEXT>               [extension] Decode nothing: score TEXT at the first line slot of the first image under -f and every --font-candidate, a CSV row per font on stdout\n"
           "      --rank-shift <N>                 [extension] Score TEXT at the rigid shifts -N ..= N in 1/64 px and keep the best, N <= 64 (only with --rank-text) [default: 0]\n"
           "      --rank-drift <W>                 [extension] Fit every character's pen of TEXT instead: offsets of up to W/64 px from the font's own pens, W <= 1024; the CSV gains first,last,scale,x64 (only with --rank-text, not with --rank-shift)\n"
           "      --rank-step <N>                  [extension] Consecutive characters' offsets differ by at most N/64 px, N <= 64 (only with --rank-drift) [default: 2]\n"
           "      --refine <S>                     [extension] Repair the reading against the line with all its glyphs drawn together, one character at a time, in at most S <= 8 sweeps; stdout carries the repaired text (after the plain pen loop, a pen search, the whole-line decode or a pen slack)\n"
           "      --refine-radius <N>              [extension] Let a repaired character move by up to N/64 px, N <= 64 (only with --refine) [default: 4]\n"
           "      --learn <FILE>                   [extension] Learn the glyph tables from FILE, a reading you trust in focr's own output format (one line per non-blank line slot in -i order; it may stop early, an empty line skips its slot), then decode with them; learning from the decoder's own reading reproduces its errors (only with the plain pen loop)\n"
           "      --learn-min-count <M>            [extension] Learn a (glyph, phase) cell from at least M samples, M >= 1 (only with --learn) [default: 1]\n"
           "      --learn-grow <G>                 [extension] Grow every learned cell's support by G pixels a side; above 0 neighbours overlap and costs drop below the objective's limit (only with --learn) [default: 0]\n"
           "  -h, --help                           Print help\n"
           "  -V, --version                        Print version\n",
           USAGE, DEFAULT_ALPHABET);
}

// One --font-candidate SPEC: key=value pairs separated by commas over the defaults of a; an unknown, empty or repeated key,
// or a value that does not parse, is a usage error.
FontSpec parse_font_spec(const std::string &spec, const Args &a) {
    const auto bad = [&](const std::string &why) { usage_error("invalid value '" + spec + "' for '--font-candidate <SPEC>': " + why); };
    FontSpec out{a.font, a.text_size, a.kerning, a.hinting};
    std::string seen;
    for (size_t at = 0; at <= spec.size();) {
        const size_t end = std::min(spec.find(',', at), spec.size());
        const std::string item = spec.substr(at, end - at);
        at = end + 1;
        if (item.size() < 2 || item[1] != '=' || !strchr("ftkh", item[0])) bad("'" + item + "' is not one of f=PATH, t=SIZE, k=KERNING, h=0|1");
        const std::string val = item.substr(2);
        if (val.empty()) bad(std::string("the key '") + item[0] + "' has no value");
        if (seen.find(item[0]) != std::string::npos) bad(std::string("the key '") + item[0] + "' is given twice");
        seen += item[0];
        if (item[0] == 'f') out.font = val;
        else if (item[0] == 'h' && (val == "0" || val == "1")) out.hinting = val == "1";
        else if (item[0] == 't' && cli::parse_f32(val, &out.text_size)) continue;
        else if (item[0] == 'k' && cli::parse_f32(val, &out.kerning)) continue;
        else bad("'" + val + "' is not a value for the key '" + item[0] + "'");
    }
    return out;
}

Args parse_args(int argc, char **argv) {
    Args a;
    for (cli::ArgCursor c(argc, argv, USAGE); c.next();) {
        const std::string &k = c.key;
        if (k == "-i" || k == "--img") c.need_all(a.img);
        else if (k == "-f" || k == "--font") a.font = c.need();
        else if (k == "-a" || k == "--alphabet") a.alphabet = c.need();
        else if (k == "--hinting") a.hinting = true;
        else if (k == "-t" || k == "--text-size") a.text_size = c.f32(), a.have_text_size = true;
        else if (k == "-k" || k == "--kerning") a.kerning = c.f32();
        else if (k == "-x" || k == "--x") a.x = c.u32();
        else if (k == "-y" || k == "--y") a.y = c.u32();
        else if (k == "-w" || k == "--width") a.width = c.u32(), a.have_width = true;
        else if (k == "--line-height") a.line_height = c.u32(), a.have_line_height = true;
        else if (k == "--line-advance") a.line_advance = c.u32(), a.have_line_advance = true;
        else if (k == "--test") a.test = c.need(), a.have_test = true;
        else if (k == "--verify") a.verify = c.need(), a.have_verify = true;
        else if (k == "--scores") a.scores = c.need(), a.have_scores = true;
        else if (k == "--pen-search") a.pen_search = c.u32_at_most(FOCR_PEN_SEARCH_MAX, "the radius is at most 64");
        else if (k == "--pen-slack") a.pen_slack = c.u32_at_most(FOCR_PEN_SEARCH_MAX, "the radius is at most 64");
        else if (k == "--baseline-search") a.baseline_search = c.u32_at_most(FOCR_BASELINE_MAX, "the radius is at most 32");
        else if (k == "--whole-baseline") a.whole_baseline = c.u32_at_most(FOCR_BASELINE_MAX, "the radius is at most 32");
        else if (k == "--y-bits") a.y_bits = c.u32_at_most(FOCR_BASELINE_Y_BITS_MAX, "at most 3"), a.have_y_bits = true;
        else if (k == "--y-frac") a.y_frac = c.u32_at_most(63, "at most 63"), a.have_y_frac = true;
        else if (k == "--line-advance-frac") a.line_advance_frac = c.u32_at_most(63, "at most 63"), a.have_line_advance_frac = true;
        else if (k == "--baselines") a.baselines = c.need(), a.have_baselines = true;
        else if (k == "--whole-line") a.whole_line = true;
        else if (k == "--margins") a.margins = c.need(), a.have_margins = true;
        else if (k == "--font-candidate") a.candidate_specs.push_back(c.need());
        else if (k == "--fonts") a.fonts = c.need(), a.have_fonts = true;
        else if (k == "--verify-fonts") a.verify_fonts = c.need(), a.have_verify_fonts = true;
        else if (k == "--rank-text") a.rank_text = c.need(), a.have_rank_text = true;
        else if (k == "--rank-shift") a.rank_shift = c.u32_at_most(FOCR_PEN_SEARCH_MAX, "the radius is at most 64"), a.have_rank_shift = true;
        else if (k == "--rank-drift") a.rank_drift = c.u32_at_most(FOCR_ALIGN_DRIFT_MAX, "the radius is at most 1024"), a.have_rank_drift = true;
        else if (k == "--rank-step") a.rank_step = c.u32_at_most(FOCR_PEN_SEARCH_MAX, "the radius is at most 64"), a.have_rank_step = true;
        else if (k == "--refine") a.refine = c.u32_at_most(FOCR_REFINE_SWEEPS_MAX, "at most 8 sweeps"), a.have_refine = true;
        else if (k == "--refine-radius") a.refine_radius = c.u32_at_most(FOCR_PEN_SEARCH_MAX, "the radius is at most 64"), a.have_refine_radius = true;
        else if (k == "--learn") a.learn = c.need(), a.have_learn = true;
        else if (k == "--learn-min-count") a.learn_min_count = c.u32(), a.have_learn_min_count = true;
        else if (k == "--learn-grow") a.learn_grow = c.u32(), a.have_learn_grow = true;
        else if (k == "-h" || k == "--help") {
            print_help();
            exit(0);
        } else if (k == "-V" || k == "--version") {
            puts("font-ocr 0.1.0");
            exit(0);
        } else c.unexpected();
    }
    std::string missing;
    if (a.font.empty()) missing += "\n  --font <FONT>";
    if (!a.have_text_size) missing += "\n  --text-size <TEXT_SIZE>";
    if (!a.have_width) missing += "\n  --width <WIDTH>";
    if (!a.have_line_height) missing += "\n  --line-height <LINE_HEIGHT>";
    if (!a.have_line_advance) missing += "\n  --line-advance <LINE_ADVANCE>";
    if (!missing.empty()) usage_error("the following required arguments were not provided:" + missing);
    if (a.whole_line && a.have_scores) usage_error("the argument '--whole-line' cannot be used with '--scores <SCORES>'");
    if (a.whole_line && a.pen_search) usage_error("the argument '--whole-line' cannot be used with '--pen-search <N>'");
    if (a.have_margins && !a.whole_line) usage_error("the argument '--margins <MARGINS>' cannot be used without '--whole-line'");
    if (a.pen_slack && a.pen_search) usage_error("the argument '--pen-slack <N>' cannot be used with '--pen-search <N>'");
    if (a.pen_slack && !a.whole_line) usage_error("the argument '--pen-slack <N>' cannot be used without '--whole-line'");
    if (a.pen_slack && a.have_margins) usage_error("the argument '--pen-slack <N>' cannot be used with '--margins <MARGINS>'");
    if (a.baseline_search && a.have_scores) usage_error("the argument '--baseline-search <N>' cannot be used with '--scores <SCORES>'");
    if (a.baseline_search && a.pen_search) usage_error("the argument '--baseline-search <N>' cannot be used with '--pen-search <N>'");
    if (a.baseline_search && a.whole_line) usage_error("the argument '--baseline-search <N>' cannot be used with '--whole-line'");
    if (a.whole_baseline && !a.whole_line) usage_error("the argument '--whole-baseline <N>' cannot be used without '--whole-line'");
    if (a.whole_baseline && a.have_margins) usage_error("the argument '--whole-baseline <N>' cannot be used with '--margins <MARGINS>'");
    if (a.whole_baseline && a.pen_slack) usage_error("the argument '--whole-baseline <N>' cannot be used with '--pen-slack <N>'");
    if (a.have_y_bits && !a.baseline_search && !a.whole_baseline) usage_error("the argument '--y-bits <B>' cannot be used without '--baseline-search <N>'");
    if (a.have_baselines && !a.baseline_search && !a.whole_baseline) usage_error("the argument '--baselines <BASELINES>' cannot be used without '--baseline-search <N>'");
    for (const auto &[have, name] : {std::pair<bool, const char *>{a.have_y_frac, "--y-frac <N>"}, {a.have_line_advance_frac, "--line-advance-frac <N>"}}) {
        if (have && !a.baseline_search && !a.whole_baseline)
            usage_error(std::string("the argument '") + name + "' cannot be used without '--baseline-search <N>' or '--whole-baseline <N>'");
        if (have && a.have_test) usage_error(std::string("the argument '") + name + "' cannot be used with '--test <TEST>'");
    }
    if (a.candidate_specs.size() > FOCR_FONT_CANDIDATES_MAX - 1) usage_error("the argument '--font-candidate <SPEC>' cannot be used more than 15 times");
    for (const std::string &spec : a.candidate_specs) a.candidates.push_back(parse_font_spec(spec, a));
    if (a.have_fonts && a.candidates.empty()) usage_error("the argument '--fonts <FONTS>' cannot be used without '--font-candidate <SPEC>'");
    if (a.have_verify_fonts && a.candidates.empty())
        usage_error("the argument '--verify-fonts <DIR>' cannot be used without '--font-candidate <SPEC>'");
    if (a.have_rank_shift && !a.have_rank_text) usage_error("the argument '--rank-shift <N>' cannot be used without '--rank-text <TEXT>'");
    if (a.have_rank_drift && !a.have_rank_text) usage_error("the argument '--rank-drift <W>' cannot be used without '--rank-text <TEXT>'");
    if (a.have_rank_drift && a.have_rank_shift) usage_error("the argument '--rank-drift <W>' cannot be used with '--rank-shift <N>'");
    if (a.have_rank_step && !a.have_rank_drift) usage_error("the argument '--rank-step <N>' cannot be used without '--rank-drift <W>'");
    for (const auto &[with, name] : {std::pair<bool, const char *>{a.have_scores, "--scores <SCORES>"}, {a.pen_search != 0, "--pen-search <N>"},
                                     {a.pen_slack != 0, "--pen-slack <N>"}, {a.have_margins, "--margins <MARGINS>"},
                                     {a.baseline_search != 0, "--baseline-search <N>"}, {a.whole_baseline != 0, "--whole-baseline <N>"},
                                     {a.have_verify, "--verify <VERIFY>"}})
        if (with && !a.candidates.empty()) usage_error(std::string("the argument '--font-candidate <SPEC>' cannot be used with '") + name + "'");
    for (const auto &[with, name] : {std::pair<bool, const char *>{a.pen_search != 0, "--pen-search <N>"}, {a.whole_line, "--whole-line"},
                                     {a.baseline_search != 0, "--baseline-search <N>"}, {a.whole_baseline != 0, "--whole-baseline <N>"},
                                     {!a.candidates.empty(), "--font-candidate <SPEC>"}, {a.have_test, "--test <TEST>"},
                                     {a.have_rank_text, "--rank-text <TEXT>"}})
        if (with && a.have_learn) usage_error(std::string("the argument '--learn <FILE>' cannot be used with '") + name + "'");
    for (const auto &[with, name] : {std::pair<bool, const char *>{!a.candidates.empty(), "--font-candidate <SPEC>"}, {a.baseline_search != 0, "--baseline-search <N>"},
                                     {a.whole_baseline != 0, "--whole-baseline <N>"}, {a.have_test, "--test <TEST>"}, {a.have_rank_text, "--rank-text <TEXT>"}})
        if (with && a.have_refine) usage_error(std::string("the argument '--refine <S>' cannot be used with '") + name + "'");
    if (a.have_refine_radius && !a.have_refine) usage_error("the argument '--refine-radius <N>' cannot be used without '--refine <S>'");
    if (a.have_learn_min_count && !a.have_learn) usage_error("the argument '--learn-min-count <M>' cannot be used without '--learn <FILE>'");
    if (a.have_learn_grow && !a.have_learn) usage_error("the argument '--learn-grow <G>' cannot be used without '--learn <FILE>'");
    if (a.have_learn_min_count && a.learn_min_count < 1) usage_error("invalid value '0' for '--learn-min-count <M>': at least 1");
    return a;
}

// 8-bit RGB or RGBA PNG (focr_image_save_png, the host library's writer)
bool write_png(const std::string &path, const uint8_t *px, uint32_t w, uint32_t h, bool alpha) {
    return focr_image_save_png(path.c_str(), px, w, h, alpha ? 4 : 3) == 0;
}

struct Line {
    uint32_t y;
    std::vector<uint32_t> text;  // code points
    std::vector<focr_char_score_t> scores;  // --scores: one per code point
    std::vector<int8_t> offsets;            // --scores with --pen-search: one per code point
    std::vector<uint32_t> pens;             // --margins: one per code point, in 1/64 px
    std::vector<focr_char_margin_t> margins;
    int q = 0;                              // --baselines: the line's chosen vertical offset, in steps of 2^-B px
    long long cost = 0;
    int font = 0;                           // --fonts: the line's winning candidate, and its cost
    long long font_cost = 0;
    bool refined = false;                   // --refine: stdout carries `repaired` in the text's place
    std::vector<uint32_t> repaired{};
};

// Writes the batch's verify images (the device's draw_verify, n x H x W x 3 bytes) as PNGs on at most 16 threads, and
// no more than the batch's pages; ok[j] says whether page j's file was written.
std::vector<char> write_verify_pngs(const std::vector<std::string> &paths, const uint8_t *rgb, uint32_t W, uint32_t H) {
    const size_t n = paths.size(), page = (size_t)W * H * 3;
    std::vector<char> ok(n, 0);
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t j; (j = next.fetch_add(1)) < n;) ok[j] = write_png(paths[j], rgb + j * page, W, H, false);
    };
    std::vector<std::thread> pool;
    for (size_t t = 1; t < std::min<size_t>(16, n); t++) pool.emplace_back(work);
    work();
    for (std::thread &t : pool) t.join();
    return ok;
}

// --test PREFIX (src/main.rs:416-425): PREFIX-rect.png (the box of every non-blank line slot) and PREFIX-text.png (the
// alphabet rendered at the top-left corner), both over the first -i image as RGBA, drawn on the device; nothing on stdout.
int run_test(const Args &args, const std::vector<uint32_t> &alphabet) {
    if (args.img.empty()) die("--test: no -i image to draw on");
    const std::string &img = args.img[0];
    char err[256] = {0};
    uint8_t *luma = nullptr, *rgba = nullptr;
    size_t W = 0, H = 0, w2 = 0, h2 = 0;
    if (focr_image_load_luma8(img.c_str(), &luma, &W, &H, err, sizeof err) != 0 ||
        focr_image_load_rgba8(img.c_str(), &rgba, &w2, &h2, err, sizeof err) != 0)
        die("--test: called `Result::unwrap()` on an `Err` value: " + std::string(err) + " (" + img + ")");
    if (w2 != W || h2 != H) die("--test: image size changed while reading " + img);
    focr_decode_font_t font{};
    if (focr_decode_font_build(args.font.c_str(), args.text_size, args.hinting, args.kerning, alphabet.data(), alphabet.size(), &font, err,
                               sizeof err) != 0)
        die(std::string("--test: decode font: ") + err);
    focr_verify_font_t vfont{};
    if (focr_verify_font_build(args.font.c_str(), args.text_size, args.hinting, args.kerning, alphabet.data(), alphabet.size(), &vfont, err,
                               sizeof err) != 0)
        die(std::string("--test: verify font: ") + err);
    focr_decoder_t *dec = nullptr;
    if (focr_decoder_create(0, &dec) != 0) die(std::string("--test: no usable GPU: ") + focr_decoder_last_error(nullptr), 1);
    if (focr_decoder_set_font(dec, &font) != 0 || focr_decoder_set_verify_font(dec, &vfont) != 0)
        die(std::string("--test: ") + focr_decoder_last_error(dec), 1);
    std::vector<uint8_t> rect(W * H * 4), text(W * H * 4);
    if (focr_decoder_test_images(dec, luma, rgba, 0, 1, W, H, args.x, args.y, args.width, args.line_height, args.line_advance, rect.data(),
                                 text.data(), 0) != 0)
        die(std::string("--test: focr_decoder_test_images: ") + focr_decoder_last_error(dec), 1);
    focr_decoder_destroy(dec);
    focr_verify_font_free(&vfont);
    focr_decode_font_free(&font);
    free(luma);
    free(rgba);
    for (const auto &out : {std::make_pair(args.test + "-rect.png", rect.data()), std::make_pair(args.test + "-text.png", text.data())})
        if (!write_png(out.first, out.second, (uint32_t)W, (uint32_t)H, true)) die("--test: cannot write " + out.first);
    return 0;
}

// --rank-text TEXT: TEXT at the first line slot of the first -i image under font 0 and every --font-candidate, the same line
// listed K + 1 times in one focr_decoder_score_text call; a CSV row per font on stdout.  Nothing is decoded.
int run_rank(const Args &args, const std::vector<uint32_t> &alphabet, const std::vector<uint16_t> &text) {
    if (args.img.empty()) die("--rank-text: no -i image to score against");
    const std::string &img = args.img[0];
    char err[256] = {0};
    uint8_t *luma = nullptr;
    size_t W = 0, H = 0;
    if (focr_image_load_luma8(img.c_str(), &luma, &W, &H, err, sizeof err) != 0)
        die("--rank-text: called `Result::unwrap()` on an `Err` value: " + std::string(err) + " (" + img + ")");
    std::vector<focr_decode_font_t> fonts(1 + args.candidates.size());
    for (size_t k = 0; k < fonts.size(); k++) {
        const FontSpec c = k ? args.candidates[k - 1] : FontSpec{args.font, args.text_size, args.kerning, args.hinting};
        if (focr_decode_font_build(c.font.c_str(), c.text_size, c.hinting, c.kerning, alphabet.data(), alphabet.size(), &fonts[k], err, sizeof err) != 0)
            die((k ? "--rank-text: font candidate " + std::to_string(k) : std::string("--rank-text")) + ": decode font: " + err);
    }
    focr_decoder_t *dec = nullptr;
    if (focr_decoder_create(0, &dec) != 0) die(std::string("--rank-text: no usable GPU: ") + focr_decoder_last_error(nullptr), 1);
    if (focr_decoder_set_font(dec, &fonts[0]) != 0 ||
        (fonts.size() > 1 && focr_decoder_set_font_candidates(dec, fonts.data() + 1, (uint32_t)fonts.size() - 1) != 0))
        die(std::string("--rank-text: ") + focr_decoder_last_error(dec), 1);
    std::vector<focr_text_line_t> lines(fonts.size());
    for (size_t k = 0; k < lines.size(); k++) lines[k] = focr_text_line_t{0, args.y, 0, (uint32_t)text.size(), (uint32_t)k};
    if (args.have_rank_drift) {  // the pens fitted under every font, and the line through them
        std::vector<focr_text_align_t> fit(lines.size());
        std::vector<uint32_t> pens(std::max<size_t>(lines.size() * text.size(), 1));
        std::vector<int32_t> terms(pens.size());
        if (focr_decoder_align_text(dec, luma, 0, 1, W, H, args.x, args.width, args.line_height, lines.data(), lines.size(), text.data(), text.size(), nullptr, 0,
                                    0, args.rank_drift, args.rank_step, pens.data(), terms.data(), fit.data()) != 0)
            die(std::string("--rank-text: focr_decoder_align_text: ") + focr_decoder_last_error(dec), 1);
        focr_decoder_destroy(dec);
        printf("font,first,last,cost,line_base,error,scale,x64\n");
        for (size_t k = 0; k < fit.size(); k++) {
            // include/focr_decode.h's sums, in list order: u the nominal pen (start 0), p the fitted one, over the inked characters
            double n = 0, su = 0, sp = 0, suu = 0, sup = 0;
            uint64_t nominal = 0;
            for (size_t g = 0; g < text.size(); g++) {
                if (terms[k * text.size() + g] != 0) {
                    const double u = (double)nominal, p = (double)pens[k * text.size() + g];
                    n += 1, su += u, sp += p, suu += u * u, sup += u * p;
                }
                nominal += (uint64_t)(int)rintf(fonts[k].glyphs[text[g]].increment * 64.0f);  // below 2^24: the call accepted the line
            }
            const double d = n * suu - su * su;
            printf("%zu,%d,%d,%lld,%llu,%lld,", k, (int)fit[k].first, (int)fit[k].last, (long long)fit[k].cost, (unsigned long long)fit[k].line_base,
                   (long long)fit[k].line_base + (long long)fit[k].cost);
            if (n < 2 || d == 0) printf(",\n");
            else {
                const double scale = (n * sup - su * sp) / d;
                printf("%.6f,%.2f\n", scale, (sp - scale * su) / n);
            }
        }
        for (focr_decode_font_t &f : fonts) focr_decode_font_free(&f);
        free(luma);
        return 0;
    }
    std::vector<focr_text_score_t> got(lines.size());
    if (focr_decoder_score_text(dec, luma, 0, 1, W, H, args.x, args.width, args.line_height, lines.data(), lines.size(), text.data(), nullptr, nullptr,
                                text.size(), nullptr, 0, args.rank_shift, nullptr, got.data()) != 0)
        die(std::string("--rank-text: focr_decoder_score_text: ") + focr_decoder_last_error(dec), 1);
    focr_decoder_destroy(dec);
    for (focr_decode_font_t &f : fonts) focr_decode_font_free(&f);
    free(luma);
    printf("font,shift,cost,line_base,error\n");
    for (size_t k = 0; k < got.size(); k++)
        printf("%zu,%d,%lld,%llu,%lld\n", k, (int)got[k].shift, (long long)got[k].cost, (unsigned long long)got[k].line_base,
               (long long)got[k].line_base + (long long)got[k].cost);
    return 0;
}

// --learn FILE as alphabet indices (the first of equal characters), one entry per line of FILE; an empty line is an empty entry.
std::vector<std::vector<uint16_t>> read_reading(const std::string &path, const std::vector<uint32_t> &alphabet) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) usage_error("cannot read '" + path + "' for '--learn'");
    std::string all;
    char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) all.append(buf, n);
    fclose(f);
    std::vector<std::vector<uint16_t>> out;
    for (size_t at = 0; at < all.size();) {
        const size_t end = std::min(all.find('\n', at), all.size());
        std::vector<uint16_t> line;
        for (uint32_t cp : utf8_decode(all.substr(at, end - at))) {
            const auto hit = std::find(alphabet.begin(), alphabet.end(), cp);
            if (hit == alphabet.end())
                usage_error("invalid value '" + path + "' for '--learn <FILE>': line " + std::to_string(out.size() + 1) + ": '" + utf8_encode(cp) + "' is not in the alphabet");
            line.push_back((uint16_t)(hit - alphabet.begin()));
        }
        out.push_back(std::move(line));
        at = end + 1;
    }
    return out;
}

}  // namespace

int main(int argc, char **argv) {
    Args args = parse_args(argc, argv);
    if (args.have_verify) {
        struct stat st;
        if (stat(args.verify.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) die("--verify should be a dir");  // src/main.rs:389-391
    }
    if (args.have_verify_fonts) {
        struct stat st;
        if (stat(args.verify_fonts.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) die("--verify-fonts should be a dir");
    }
    std::vector<uint32_t> alphabet = utf8_decode(args.alphabet);
    std::vector<uint16_t> rank_text;  // --rank-text as alphabet indices (the first of equal characters)
    for (uint32_t cp : utf8_decode(args.rank_text)) {
        const auto at = std::find(alphabet.begin(), alphabet.end(), cp);
        if (at == alphabet.end()) usage_error("invalid value '" + args.rank_text + "' for '--rank-text <TEXT>': '" + utf8_encode(cp) + "' is not in the alphabet");
        rank_text.push_back((uint16_t)(at - alphabet.begin()));
    }
    std::vector<std::vector<uint16_t>> reading;
    if (args.have_learn) reading = read_reading(args.learn, alphabet);
    if (args.have_test) return run_test(args, alphabet);
    if (args.have_rank_text) return run_rank(args, alphabet, rank_text);
    FILE *csv = nullptr;
    if (args.have_scores && !(csv = fopen(args.scores.c_str(), "w"))) usage_error("cannot write '" + args.scores + "' for '--scores'");
    FILE *mcsv = nullptr;
    if (args.have_margins && !(mcsv = fopen(args.margins.c_str(), "w"))) usage_error("cannot write '" + args.margins + "' for '--margins'");
    FILE *bcsv = nullptr;
    if (args.have_baselines && !(bcsv = fopen(args.baselines.c_str(), "w"))) usage_error("cannot write '" + args.baselines + "' for '--baselines'");
    FILE *fcsv = nullptr;
    if (args.have_fonts && !(fcsv = fopen(args.fonts.c_str(), "w"))) usage_error("cannot write '" + args.fonts + "' for '--fonts'");
    if (args.img.empty()) return 0;

    char err[256] = {0};
    const bool y_fonts = (args.baseline_search || args.whole_baseline) && args.y_bits;  // the y-phase fonts; fonts[0] is the plain decode font
    std::vector<focr_decode_font_t> fonts((size_t)1 << (y_fonts ? args.y_bits : 0));
    if ((y_fonts ? focr_decode_font_build_y(args.font.c_str(), args.text_size, args.hinting, args.kerning, alphabet.data(), alphabet.size(), args.y_bits,
                                            fonts.data(), err, sizeof err)
                 : focr_decode_font_build(args.font.c_str(), args.text_size, args.hinting, args.kerning, alphabet.data(), alphabet.size(), fonts.data(),
                                          err, sizeof err)) != 0)
        die(std::string("decode font: ") + err);
    focr_decode_font_t &font = fonts[0];

    // sizes first, so that pages of one size form one batch
    const size_t n_img = args.img.size();
    std::vector<std::pair<size_t, size_t>> dims(n_img);
    std::map<std::pair<size_t, size_t>, std::vector<size_t>> groups;
    for (size_t i = 0; i < n_img; i++) {
        if (focr_image_probe(args.img[i].c_str(), &dims[i].first, &dims[i].second, err, sizeof err) != 0)
            die("called `Result::unwrap()` on an `Err` value: " + std::string(err) + " (" + args.img[i] + ")");
        groups[dims[i]].push_back(i);
    }

    focr_decoder_t *dec = nullptr;
    if (focr_decoder_create(0, &dec) != 0) die(std::string("no usable GPU: ") + focr_decoder_last_error(nullptr), 1);
    // a setter that refuses ends the program: "<setter>: <the library's message>", exit code 1
    const auto set = [&](const char *setter, int rc) { if (rc != 0) die(std::string(setter) + ": " + focr_decoder_last_error(dec), 1); };
    set("focr_decoder_set_font", focr_decoder_set_font(dec, &font));
    const auto set_verify_font = [&]() {  // font 0's verify table (a learned font keeps the boxes and rectangles of the font it came from)
        focr_verify_font_t vfont{};
        if (focr_verify_font_build(args.font.c_str(), args.text_size, args.hinting, args.kerning, alphabet.data(), alphabet.size(), &vfont, err,
                                   sizeof err) != 0)
            die(std::string("verify font: ") + err);
        set("focr_decoder_set_verify_font", focr_decoder_set_verify_font(dec, &vfont));
        focr_verify_font_free(&vfont);
    };
    if (args.have_verify || args.have_verify_fonts) set_verify_font();
    if (csv) set("focr_decoder_set_scores", focr_decoder_set_scores(dec, 1));
    set("focr_decoder_set_pen_search", focr_decoder_set_pen_search(dec, args.pen_search));
    set("focr_decoder_set_whole_line", focr_decoder_set_whole_line(dec, args.whole_line));
    set("focr_decoder_set_whole_slack", focr_decoder_set_whole_slack(dec, args.pen_slack));
    if (mcsv) set("focr_decoder_set_whole_margins", focr_decoder_set_whole_margins(dec, 1));
    if (y_fonts) set("focr_decoder_set_baseline_fonts", focr_decoder_set_baseline_fonts(dec, fonts.data(), args.y_bits));
    set("focr_decoder_set_baseline_search", focr_decoder_set_baseline_search(dec, args.baseline_search ? args.y_bits : 0, args.baseline_search));
    set("focr_decoder_set_whole_baseline", focr_decoder_set_whole_baseline(dec, args.whole_baseline ? args.y_bits : 0, args.whole_baseline));
    set("focr_decoder_set_line_frac", focr_decoder_set_line_frac(dec, args.y_frac, args.line_advance_frac));
    if (!args.candidates.empty()) {  // built over the decode font's alphabet; the decoder keeps its own copy
        std::vector<focr_decode_font_t> cands(args.candidates.size());
        for (size_t k = 0; k < cands.size(); k++) {
            const FontSpec &c = args.candidates[k];
            if (focr_decode_font_build(c.font.c_str(), c.text_size, c.hinting, c.kerning, alphabet.data(), alphabet.size(), &cands[k], err, sizeof err) != 0)
                die("font candidate " + std::to_string(k + 1) + ": decode font: " + err);
        }
        set("focr_decoder_set_font_candidates", focr_decoder_set_font_candidates(dec, cands.data(), (uint32_t)cands.size()));
        set("focr_decoder_set_font_search", focr_decoder_set_font_search(dec, 1));
        if (args.have_verify_fonts) {  // every candidate's verify table, for focr_decoder_verify_text
            std::vector<focr_verify_font_t> vcands(cands.size());
            for (size_t k = 0; k < vcands.size(); k++) {
                const FontSpec &c = args.candidates[k];
                if (focr_verify_font_build(c.font.c_str(), c.text_size, c.hinting, c.kerning, alphabet.data(), alphabet.size(), &vcands[k], err, sizeof err) != 0)
                    die("font candidate " + std::to_string(k + 1) + ": verify font: " + err);
            }
            set("focr_decoder_set_verify_font_candidates", focr_decoder_set_verify_font_candidates(dec, vcands.data(), (uint32_t)vcands.size()));
            for (focr_verify_font_t &f : vcands) focr_verify_font_free(&f);
        }
        for (focr_decode_font_t &f : cands) focr_decode_font_free(&f);
    }
    const bool csv_offsets = csv && args.pen_search > 0;
    size_t refine_chars = 0, refine_lines = 0, refine_listed = 0;

    std::vector<std::vector<Line>> lines(n_img);
    std::vector<uint8_t> batch, rgb;
    std::vector<uint64_t> sums;
    const auto load_batch = [&](const std::vector<size_t> &idx, size_t b0, size_t nb, size_t W, size_t H) {  // the images idx[b0 .. b0 + nb) into `batch`
        batch.assign(nb * W * H, 255);
        for (size_t j = 0; j < nb; j++) {
            const size_t i = idx[b0 + j];
            uint8_t *px = nullptr;
            size_t w = 0, h = 0;
            if (focr_image_load_luma8(args.img[i].c_str(), &px, &w, &h, err, sizeof err) != 0)
                die("called `Result::unwrap()` on an `Err` value: " + std::string(err) + " (" + args.img[i] + ")");
            if (w != W || h != H) die("image size changed while reading " + args.img[i]);
            memcpy(batch.data() + j * W * H, px, W * H);
            free(px);
        }
    };
    if (args.have_learn) {
        // 1. the slots: a plain run of every batch, the rows of its non-blank line slots kept per image
        std::vector<std::vector<uint32_t>> slots(n_img);
        for (const auto &grp : groups)
            for (size_t b0 = 0; b0 < grp.second.size(); b0 += BATCH_PAGES) {
                const size_t nb = std::min(BATCH_PAGES, grp.second.size() - b0), W = grp.first.first, H = grp.first.second;
                load_batch(grp.second, b0, nb, W, H);
                if (focr_decoder_run(dec, batch.data(), 0, nb, W, H, args.x, args.y, args.width, args.line_height, args.line_advance) != 0)
                    die(std::string("--learn: focr_decoder_run: ") + focr_decoder_last_error(dec), 1);
                std::vector<focr_decoded_line_t> dl(focr_decoder_n_lines(dec));
                std::vector<uint16_t> dc(focr_decoder_n_chars(dec));
                focr_decoder_get(dec, dl.data(), dc.data());
                for (const focr_decoded_line_t &l : dl) slots[grp.second[b0 + l.page]].push_back(l.y);
            }
        // 2. slot k in -i order reads line k of FILE; the paired lines are learned batch by batch and added up
        std::vector<size_t> first_slot(n_img + 1, 0);
        for (size_t i = 0; i < n_img; i++) first_slot[i + 1] = first_slot[i] + slots[i].size();
        std::vector<uint64_t> lsums(font.bitmaps_len, 0), lcounts(font.n_glyphs * FOCR_DECODE_PHASES, 0);
        std::vector<uint32_t> s32(std::max<size_t>(lsums.size(), 1)), c32(std::max<size_t>(lcounts.size(), 1));
        size_t n_used = 0, n_listed = 0;
        for (const auto &grp : groups)
            for (size_t b0 = 0; b0 < grp.second.size(); b0 += BATCH_PAGES) {
                const size_t nb = std::min(BATCH_PAGES, grp.second.size() - b0), W = grp.first.first, H = grp.first.second;
                std::vector<focr_text_line_t> tl;
                std::vector<uint16_t> tc;
                for (size_t j = 0; j < nb; j++) {
                    const size_t i = grp.second[b0 + j];
                    for (size_t q = 0; q < slots[i].size(); q++) {
                        const size_t k = first_slot[i] + q;
                        if (k >= reading.size() || reading[k].empty()) continue;
                        tl.push_back(focr_text_line_t{(uint32_t)j, slots[i][q], tc.size(), (uint32_t)reading[k].size(), 0});
                        tc.insert(tc.end(), reading[k].begin(), reading[k].end());
                    }
                }
                if (tl.empty()) continue;
                load_batch(grp.second, b0, nb, W, H);
                std::vector<uint8_t> used(tc.size());
                if (focr_decoder_learn_text(dec, batch.data(), 0, nb, W, H, args.x, args.width, args.line_height, tl.data(), tl.size(), tc.data(), nullptr, nullptr,
                                            nullptr, tc.size(), 0, s32.data(), c32.data(), used.data()) != 0)
                    die(std::string("--learn: focr_decoder_learn_text: ") + focr_decoder_last_error(dec), 1);
                for (size_t e = 0; e < lsums.size(); e++) lsums[e] += s32[e];
                for (size_t e = 0; e < lcounts.size(); e++) lcounts[e] += c32[e];
                n_listed += used.size();
                n_used += (size_t)std::count(used.begin(), used.end(), 1);
            }
        // 3. the learned font replaces font 0: everything below decodes with it
        focr_decode_font_t learned{};
        size_t n_learned = 0, n_inked = 0;
        if (focr_decode_font_learn(&font, lsums.data(), lcounts.data(), args.learn_min_count, args.learn_grow, &learned, &n_learned, &n_inked, err, sizeof err) != 0)
            die(std::string("--learn: ") + err);
        fprintf(stderr, "learn: %zu characters used, %zu skipped, %zu of %zu cells with ink learned\n", n_used, n_listed - n_used, n_learned, n_inked);
        focr_decode_font_free(&font);
        font = learned;
        set("focr_decoder_set_font", focr_decoder_set_font(dec, &font));
        if (args.have_verify) set_verify_font();  // set_font drops the table with the previous font
    }
    for (const auto &grp : groups) {
        const size_t W = grp.first.first, H = grp.first.second;
        for (size_t b0 = 0; b0 < grp.second.size(); b0 += BATCH_PAGES) {
            const size_t nb = std::min(BATCH_PAGES, grp.second.size() - b0);
            load_batch(grp.second, b0, nb, W, H);
            if (focr_decoder_run(dec, batch.data(), 0, nb, W, H, args.x, args.y, args.width, args.line_height, args.line_advance) != 0)
                die(std::string("focr_decoder_run: ") + focr_decoder_last_error(dec), 1);
            std::vector<focr_decoded_line_t> dl(focr_decoder_n_lines(dec));
            std::vector<uint16_t> dc(focr_decoder_n_chars(dec));
            focr_decoder_get(dec, dl.data(), dc.data());
            std::vector<focr_char_score_t> ds(csv ? dc.size() : 0);
            if (csv && focr_decoder_get_scores(dec, ds.data(), nullptr) != 0)
                die(std::string("focr_decoder_get_scores: ") + focr_decoder_last_error(dec), 1);
            std::vector<int8_t> dj(csv_offsets ? dc.size() : 0);
            if (csv_offsets && focr_decoder_get_offsets(dec, dj.data()) != 0)
                die(std::string("focr_decoder_get_offsets: ") + focr_decoder_last_error(dec), 1);
            std::vector<uint32_t> dp(mcsv ? dc.size() : 0);
            std::vector<focr_char_margin_t> dm(mcsv ? dc.size() : 0);
            if (mcsv && (focr_decoder_get_pens(dec, dp.data(), nullptr) != 0 || focr_decoder_get_margins(dec, dm.data()) != 0))
                die(std::string("focr_decoder_get_margins: ") + focr_decoder_last_error(dec), 1);
            std::vector<int8_t> bq(bcsv ? dl.size() : 0);
            std::vector<int64_t> bc(bcsv ? dl.size() : 0);
            if (bcsv && focr_decoder_get_baselines(dec, bq.data(), bc.data()) != 0)
                die(std::string("focr_decoder_get_baselines: ") + focr_decoder_last_error(dec), 1);
            const bool want_fonts = fcsv || args.have_verify_fonts;
            std::vector<uint8_t> fk(want_fonts ? dl.size() : 0);
            std::vector<int64_t> fc(want_fonts ? dl.size() : 0);
            if (want_fonts && focr_decoder_get_fonts(dec, fk.data(), fc.data()) != 0)
                die(std::string("focr_decoder_get_fonts: ") + focr_decoder_last_error(dec), 1);
            std::vector<uint16_t> rc(args.have_refine ? dc.size() : 0);  // --refine: the repaired characters, line li's at the running sum of n_chars
            std::vector<focr_text_refine_t> rr(args.have_refine ? dl.size() : 0);
            if (args.have_refine && !dl.empty()) {  // the reading repaired against the composed line error; the run's own results stay what they were
                std::vector<uint32_t> tp(dc.size()), rp(dc.size());
                if (args.whole_line) {
                    if (focr_decoder_get_pens(dec, tp.data(), nullptr) != 0) die(std::string("focr_decoder_get_pens: ") + focr_decoder_last_error(dec), 1);
                } else {  // the pen loop's f32 walk, with the pen search's offsets: delta - 64 * origin_x
                    std::vector<int8_t> tj(dc.size(), 0);
                    if (args.pen_search && focr_decoder_get_offsets(dec, tj.data()) != 0)
                        die(std::string("focr_decoder_get_offsets: ") + focr_decoder_last_error(dec), 1);
                    for (const focr_decoded_line_t &l : dl) {
                        float pos = 0.f;
                        for (uint32_t c = 0; c < l.n_chars; c++) {
                            const float at = pos + (float)tj[l.first + c] * 0.015625f;
                            tp[l.first + c] = (uint32_t)((int)((font.origin_x + at) * 64.0f) - 64 * (int)font.origin_x);
                            pos = at + font.glyphs[dc[l.first + c]].increment;
                        }
                    }
                }
                std::vector<focr_text_line_t> tl(dl.size());
                for (size_t li = 0; li < dl.size(); li++) tl[li] = focr_text_line_t{dl[li].page, dl[li].y, dl[li].first, dl[li].n_chars, 0};
                if (focr_decoder_refine_text(dec, batch.data(), 0, nb, W, H, args.x, args.width, args.line_height, tl.data(), tl.size(), dc.data(), tp.data(), dc.size(),
                                             args.refine_radius, args.refine, 1, rc.data(), rp.data(), rr.data()) != 0)
                    die(std::string("--refine: focr_decoder_refine_text: ") + focr_decoder_last_error(dec), 1);
                refine_listed += dl.size();
            }
            size_t rat = 0;
            for (size_t li = 0; li < dl.size(); li++) {
                const focr_decoded_line_t &l = dl[li];
                Line out{l.y, {}, {}, {}, {}, {}};
                if (args.have_refine) {
                    out.refined = true;
                    for (uint32_t c = 0; c < l.n_chars; c++) out.repaired.push_back(alphabet[rc[rat + c]]);
                    rat += l.n_chars;
                    refine_chars += rr[li].changed, refine_lines += rr[li].changed != 0;
                }
                if (bcsv) out.q = bq[li], out.cost = (long long)bc[li];
                if (fcsv) out.font = fk[li], out.font_cost = (long long)fc[li];
                if (mcsv) out.pens.assign(dp.begin() + l.first, dp.begin() + l.first + l.n_chars);
                if (mcsv) out.margins.assign(dm.begin() + l.first, dm.begin() + l.first + l.n_chars);
                for (uint32_t c = 0; c < l.n_chars; c++) out.text.push_back(alphabet[dc[l.first + c]]);
                if (csv) out.scores.assign(ds.begin() + l.first, ds.begin() + l.first + l.n_chars);
                if (csv_offsets) out.offsets.assign(dj.begin() + l.first, dj.begin() + l.first + l.n_chars);
                lines[grp.second[b0 + l.page]].push_back(std::move(out));
            }
            if (args.have_verify_fonts) {  // the same picture of a font search: every line in its winner's font, at its pens under --whole-line
                std::vector<focr_text_line_t> tl(dl.size());
                for (size_t li = 0; li < dl.size(); li++) tl[li] = focr_text_line_t{dl[li].page, dl[li].y, dl[li].first, dl[li].n_chars, fk[li]};
                std::vector<uint32_t> tp(args.whole_line ? dc.size() : 0);
                if (args.whole_line && focr_decoder_get_pens(dec, tp.data(), nullptr) != 0)
                    die(std::string("focr_decoder_get_pens: ") + focr_decoder_last_error(dec), 1);
                rgb.resize(nb * W * H * 3);
                sums.assign(nb, 0);
                if (focr_decoder_verify_text(dec, batch.data(), 0, nb, W, H, args.x, tl.data(), tl.size(), dc.data(), args.whole_line ? tp.data() : nullptr,
                                             nullptr, dc.size(), rgb.data(), 0, sums.data()) != 0)
                    die(std::string("focr_decoder_verify_text: ") + focr_decoder_last_error(dec), 1);
                std::vector<std::string> paths(nb);
                for (size_t j = 0; j < nb; j++) paths[j] = verify_path(args.verify_fonts, args.img[grp.second[b0 + j]]);
                const std::vector<char> ok = write_verify_pngs(paths, rgb.data(), (uint32_t)W, (uint32_t)H);
                for (size_t j = 0; j < nb; j++) {
                    if (!ok[j]) die("cannot write " + paths[j]);
                    const float mse = (float)sums[j] / (float)(uint32_t)(W * H);
                    fprintf(stderr, "%s %.6f\n", args.img[grp.second[b0 + j]].c_str(), (double)mse);
                }
            }
            if (args.have_verify) {  // draw_verify + red_blue_mse (src/main.rs:300-329, 518-524) on the device
                rgb.resize(nb * W * H * 3);
                sums.assign(nb, 0);
                if (focr_decoder_verify(dec, rgb.data(), 0, sums.data()) != 0)
                    die(std::string("focr_decoder_verify: ") + focr_decoder_last_error(dec), 1);
                std::vector<std::string> paths(nb);
                for (size_t j = 0; j < nb; j++) paths[j] = verify_path(args.verify, args.img[grp.second[b0 + j]]);
                const std::vector<char> ok = write_verify_pngs(paths, rgb.data(), (uint32_t)W, (uint32_t)H);
                for (size_t j = 0; j < nb; j++) {
                    if (!ok[j]) die("cannot write " + paths[j]);
                    const float mse = (float)sums[j] / (float)(uint32_t)(W * H);
                    fprintf(stderr, "%s %.6f\n", args.img[grp.second[b0 + j]].c_str(), (double)mse);
                }
            }
        }
    }
    focr_decoder_destroy(dec);
    for (focr_decode_font_t &f : fonts) focr_decode_font_free(&f);
    if (args.have_refine) fprintf(stderr, "refine: %zu characters in %zu of %zu lines changed\n", refine_chars, refine_lines, refine_listed);

    std::string out;
    for (size_t i = 0; i < n_img; i++)
        for (const Line &l : lines[i]) {
            for (uint32_t cp : l.refined ? l.repaired : l.text) out += utf8_encode(cp);
            out += '\n';
        }
    fwrite(out.data(), 1, out.size(), stdout);
    if (csv) {  // one row per decoded character, in the order of stdout; a one-glyph alphabet has no runner-up and no margin
        fprintf(csv, "image_index,y,column,codepoint,score,runner_codepoint,runner_score,margin%s\n", csv_offsets ? ",pen_offset" : "");
        for (size_t i = 0; i < n_img; i++)
            for (const Line &l : lines[i])
                for (size_t c = 0; c < l.text.size(); c++) {
                    const focr_char_score_t &sc = l.scores[c];
                    fprintf(csv, "%zu,%u,%zu,%u,%lld,", i, l.y, c, l.text[c], (long long)sc.score);
                    if (sc.runner < alphabet.size())
                        fprintf(csv, "%u,%lld,%lld", alphabet[sc.runner], (long long)sc.runner_score, (long long)(sc.runner_score - sc.score));
                    else fprintf(csv, ",%lld,", (long long)sc.runner_score);
                    if (csv_offsets) fprintf(csv, ",%d", (int)l.offsets[c]);
                    fputc('\n', csv);
                }
        if (fclose(csv) != 0) die("cannot write " + args.scores);
    }
    if (bcsv) {  // one row per decoded line, in the order of stdout
        fprintf(bcsv, "image_index,y,q,offset_px,cost\n");
        for (size_t i = 0; i < n_img; i++)
            for (const Line &l : lines[i]) fprintf(bcsv, "%zu,%u,%d,%g,%lld\n", i, l.y, l.q, (double)l.q / (double)(1u << args.y_bits), l.cost);
        if (fclose(bcsv) != 0) die("cannot write " + args.baselines);
    }
    if (fcsv) {  // one row per decoded line, in the order of stdout
        fprintf(fcsv, "image_index,y,font,cost\n");
        for (size_t i = 0; i < n_img; i++)
            for (const Line &l : lines[i]) fprintf(fcsv, "%zu,%u,%d,%lld\n", i, l.y, l.font, l.font_cost);
        if (fclose(fcsv) != 0) die("cannot write " + args.fonts);
    }
    if (mcsv) {  // one row per decoded character, in the order of stdout; a one-glyph alphabet has no runner-up and no margin
        fprintf(mcsv, "image_index,y,column,codepoint,pen,term,runner_codepoint,margin\n");
        for (size_t i = 0; i < n_img; i++)
            for (const Line &l : lines[i])
                for (size_t c = 0; c < l.text.size(); c++) {
                    const focr_char_margin_t &m = l.margins[c];
                    fprintf(mcsv, "%zu,%u,%zu,%u,%u,%d,", i, l.y, c, l.text[c], l.pens[c], (int)m.term);
                    if (m.runner < alphabet.size()) fprintf(mcsv, "%u,%lld\n", alphabet[m.runner], (long long)m.margin);
                    else fprintf(mcsv, ",\n");
                }
        if (fclose(mcsv) != 0) die("cannot write " + args.margins);
    }
    return 0;
}
