// ncc — the reference's `ncc` command line (src/ncc.rs:486-542, 788-878) on top of the MI355X scan.
//
// Same flags, defaults and output formats as the reference binary (clap derive struct `Args`,
// src/ncc.rs:486-542).  Differences, all deliberate:
//   * the template bank is rasterised once per run, not once per page (src/ncc.rs:561, 587-639);
//   * pages of equal size are scanned as one device batch instead of one rayon task per page
//     (src/ncc.rs:839-847); output order is still the order of -i;
//   * --rust runs the exact v_dot4 device kernel with the arithmetic and skips of the reference's scalar Rust
//     scan and without the 1024 cap (FOCR_SCAN_RUST; src/ncc.rs:320-330, 406-483);
//   * a page without any hit prints nothing (the reference panics in partition_by, src/ncc.rs:1040);
//   * --verify DIR (extension) writes, per input image, the device's verify image (focr_verify_images: the page in red, the
//     decoded characters' templates in blue) as DIR/<file stem>.png and prints "<image> <mse>" on stderr, as `focr --verify` does;
//   * --scores PATH (extension) writes a CSV row per output character: the character, the size of its overlap group and the best
//     hit of another letter in it (focr_get_runners), as `focr --scores` does for the line decoder.  stdout is unchanged.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include "cli_common.h"
#include "focr_host.h"
#include "page_feed.h"

namespace {

using cli::utf8_decode;
using cli::utf8_encode;

const char *DEFAULT_ALPHABET = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789=+<>(){};:/-";  // src/ncc.rs:28-29

struct Args {
    std::vector<std::string> img;
    std::string font;
    float text_size = 0.f;
    bool have_text_size = false;
    uint32_t x_bits = 0, y_bits = 0;
    bool hinting = false;
    float threshold = 0.8f, anchor_threshold = 0.95f;
    int overlap = 5;
    std::string alphabet = DEFAULT_ALPHABET;
    std::string box_size = "alphabet";
    uint32_t x_padding = 0, y_padding = 0;
    bool save_letters = false, rust = false, verbose = false, csv = false, raw = false;
    bool allow_wide = false;  // extension: templates 17..32 px wide instead of the reference's panic (src/ncc.rs:392)
    bool spaces = false;  // extension: fill gaps between characters with blanks (the reference does not, README.md:46)
    std::string verify;   // extension: directory for the verify images (focr_verify_images), as `focr --verify`
    bool have_verify = false;
    std::string scores;   // extension: CSV of per-character scores and runner-ups (focr_get_runners), as `focr --scores`
    bool have_scores = false;
};

const char *USAGE = "Usage: ncc [OPTIONS] --font <FONT> --text-size <TEXT_SIZE>";

[[noreturn]] void die(const std::string &msg) { cli::die("ncc", msg, 101); }  // 101: a Rust panic's exit status

void print_help() {
    puts("Usage: ncc [OPTIONS] --font <FONT> --text-size <TEXT_SIZE>\n\nOptions:\n"
         "  -i, --img <IMG>...                         \n"
         "  -f, --font <FONT>                          \n"
         "  -t, --text-size <TEXT_SIZE>                \n"
         "      --x-bits <X_BITS>                      [default: 0]\n"
         "      --y-bits <Y_BITS>                      [default: 0]\n"
         "      --hinting                              \n"
         "      --threshold <THRESHOLD>                [default: 0.8]\n"
         "      --anchor-threshold <ANCHOR_THRESHOLD>  [default: 0.95]\n"
         "      --overlap <OVERLAP>                    [default: 5]\n"
         "  -a, --alphabet <ALPHABET>                  [default: ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789=+<>(){};:/-]\n"
         "      --box-size <BOX_SIZE>                  [default: alphabet]\n"
         "      --x-padding <X_PADDING>                [default: 0]\n"
         "      --y-padding <Y_PADDING>                [default: 0]\n"
         "      --save-letters                         \n"
         "      --rust                                 \n"
         "  -v, --verbose                              \n"
         "      --csv                                  \n"
         "      --raw                                  \n"
         "      --spaces                               [extension] print blanks for gaps of whole advances\n"
         "      --allow-wide                           [extension] accept templates 17..32 px wide\n"
         "      --verify <VERIFY>                      [extension] Dir for verify images. Red is the page, Blue the decoded characters\n"
         "      --scores <SCORES>                      [extension] CSV of every character's similarity, overlap group size and runner-up\n"
         "  -h, --help                                 Print help\n"
         "  -V, --version                              Print version");
}

Args parse_args(int argc, char **argv) {
    Args a;
    for (cli::ArgCursor c(argc, argv, USAGE); c.next();) {
        const std::string &k = c.key;
        if (k == "-i" || k == "--img") c.need_all(a.img);
        else if (k == "-f" || k == "--font") a.font = c.need();
        else if (k == "-t" || k == "--text-size") a.text_size = c.f32(), a.have_text_size = true;
        else if (k == "--x-bits") a.x_bits = c.u32();
        else if (k == "--y-bits") a.y_bits = c.u32();
        else if (k == "--hinting") a.hinting = true;
        else if (k == "--threshold") a.threshold = c.f32();
        else if (k == "--anchor-threshold") a.anchor_threshold = c.f32();
        else if (k == "--overlap") {  // an i32 (src/ncc.rs:514): clap refuses what does not fit, negative values included
            const std::string &s = c.need();
            char *e = nullptr;
            long long r = strtoll(s.c_str(), &e, 10);  // saturates beyond 64 bits, which is outside the i32 range too
            if (!e || *e || s.empty()) c.fail("invalid value '" + s + "' for '--overlap <OVERLAP>'");
            if (r > INT32_MAX) c.fail("invalid value '" + s + "' for '--overlap <OVERLAP>': number too large to fit in target type");
            if (r < INT32_MIN) c.fail("invalid value '" + s + "' for '--overlap <OVERLAP>': number too small to fit in target type");
            a.overlap = (int)r;
        } else if (k == "-a" || k == "--alphabet") a.alphabet = c.need();
        else if (k == "--box-size") a.box_size = c.need();
        else if (k == "--x-padding") a.x_padding = c.u32();
        else if (k == "--y-padding") a.y_padding = c.u32();
        else if (k == "--save-letters") a.save_letters = true;
        else if (k == "--rust") a.rust = true;
        else if (k == "-v" || k == "--verbose") a.verbose = true;
        else if (k == "--csv") a.csv = true;
        else if (k == "--raw") a.raw = true;
        else if (k == "--spaces") a.spaces = true;
        else if (k == "--allow-wide") a.allow_wide = true;
        else if (k == "--verify") a.verify = c.need(), a.have_verify = true;
        else if (k == "--scores") a.scores = c.need(), a.have_scores = true;
        else if (k == "-h" || k == "--help") {
            print_help();
            exit(0);
        } else if (k == "-V" || k == "--version") {
            puts("ncc 0.1.0");
            exit(0);
        } else c.unexpected();
    }
    const auto usage_error = [](const std::string &msg) { cli::usage_error(USAGE, msg); };
    if (a.font.empty()) usage_error("the following required arguments were not provided:\n  --font <FONT>");
    if (!a.have_text_size) usage_error("the following required arguments were not provided:\n  --text-size <TEXT_SIZE>");
    if (a.have_verify) {  // refused here, before the bank is rasterised or a device is touched
        if (a.raw) usage_error("the argument '--verify <VERIFY>' cannot be used with '--raw' (no characters are decoded in that mode)");
        struct stat st;
        if (stat(a.verify.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) usage_error("--verify should be a dir: '" + a.verify + "'");
    }
    if (a.have_scores) {  // as --verify: refused before the bank is rasterised or a device is touched
        if (a.raw) usage_error("the argument '--scores <SCORES>' cannot be used with '--raw' (no characters are decoded in that mode)");
        if (a.scores.empty()) usage_error("a value is required for '--scores <SCORES>' but none was supplied");
    }
    return a;
}

std::string f32s(float v);
std::string f32dbg(float v) {  // Rust `{:?}` of an f32: as `{}`, with ".0" on whole numbers
    std::string t = f32s(v);
    if (t.find_first_of(".eEn") == std::string::npos) t += ".0";  // n: inf / NaN
    return t;
}
std::string f32s(float v) {  // Rust `{}` of an f32
    char buf[64];
    focr_format_f32(v, buf, sizeof buf);
    return buf;
}

// --scores: one row per output character.  Floats as %.9g (a float32 reads back exactly); margin in double; no runner: four empty fields.
const char *SCORES_HEADER = "image_index,line,column,codepoint,x,y,similarity,members,runner_codepoint,runner_x,runner_similarity,margin\n";
void scores_row(std::string &out, size_t image, size_t line, size_t column, const focr_hit_t &c, const focr_runner_t &r) {
    char row[256];
    int n = snprintf(row, sizeof row, "%zu,%zu,%zu,%u,%u,%u,%.9g,%u,", image, line, column, c.letter, c.x, c.y, (double)c.similarity, r.members);
    out.append(row, (size_t)n);
    if (r.template_index == FOCR_NO_RUNNER) {
        out += ",,,\n";  // runner_codepoint, runner_x, runner_similarity, margin: empty
        return;
    }
    n = snprintf(row, sizeof row, "%u,%u,%.9g,%.9g\n", r.letter, r.x, (double)r.similarity, (double)c.similarity - (double)r.similarity);
    out.append(row, (size_t)n);
}

[[noreturn]] void fatal(PageFeed &feed, const std::string &msg) {  // panic with the decoders stopped first
    feed.stop();
    die(msg);
}

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

struct PhaseClock {  // -v: wall time of each host phase, on stderr
    bool on;
    Clock::time_point t0 = Clock::now(), t = t0;
    void lap(const char *what) {
        const auto n = Clock::now();
        if (on) fprintf(stderr, "phase %-14s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

struct Run {  // what a run fixes before its first batch; read-only from then on
    const Args &args;
    const focr_bank_t &bank;
    const std::vector<uint32_t> &alphabet;
    focr_fleet_t *fleet;
    FILE *scores_file;  // --scores, or null
    size_t batch_pages;
    // --rust: the scalar scan's arithmetic and its missing cap (src/ncc.rs:320-330, 406-483) on the exact device kernel
    int mode() const { return args.rust ? FOCR_SCAN_RUST : FOCR_SCAN_MFMA; }
    uint32_t cap() const { return args.rust ? 0xffffffffu : (uint32_t)FOCR_MAX_MATCHES; }
};

struct Totals {  // what retiring a batch adds to
    double ms_wait = 0, ms_results = 0, ms_format = 0, ms_device = 0;
    std::vector<uint64_t> hits_by_letter;  // -v: hits per alphabet letter over all pages (src/ncc.rs:703-718)
    std::string out;                       // stdout, not yet written
};

// the reference's -v preamble, src/ncc.rs:791-802: font.metrics() and what follows from it at --text-size
void print_metrics_preamble(const Args &args, const focr_bank_t &bank, size_t n_letters) {
    focr_font_metrics_t fm{};
    char err[256] = {0};
    if (focr_font_metrics(args.font.c_str(), &fm, err, sizeof err) != 0) die(std::string("font metrics: ") + err);
    const float to_px = (1.f / (float)fm.units_per_em) * args.text_size;
    const float line_space = fm.ascent - fm.descent + fm.line_gap;
    fprintf(stderr, "metrics Metrics { units_per_em: %u, ascent: %s, descent: %s, line_gap: %s, underline_position: %s, underline_thickness: %s, "
                    "cap_height: %s, x_height: %s, bounding_box: RectF(<%s, %s>, <%s, %s>) }\n",
            fm.units_per_em, f32dbg(fm.ascent).c_str(), f32dbg(fm.descent).c_str(), f32dbg(fm.line_gap).c_str(), f32dbg(fm.underline_position).c_str(),
            f32dbg(fm.underline_thickness).c_str(), f32dbg(fm.cap_height).c_str(), f32dbg(fm.x_height).c_str(), f32s(fm.bbox[0]).c_str(),
            f32s(fm.bbox[1]).c_str(), f32s(fm.bbox[2]).c_str(), f32s(fm.bbox[3]).c_str());
    fprintf(stderr, "ascent  %spx\n", f32s(fm.ascent * to_px).c_str());
    fprintf(stderr, "descent %spx\n", f32s(fm.descent * to_px).c_str());
    fprintf(stderr, "font_bbox size <%s, %s>px\n", f32s(fm.bbox[2] * to_px - fm.bbox[0] * to_px).c_str(), f32s(fm.bbox[3] * to_px - fm.bbox[1] * to_px).c_str());
    fprintf(stderr, "line_space %s %spx\n", f32s(line_space).c_str(), f32s(line_space * to_px).c_str());
    fprintf(stderr, "bank: %zu templates (%zu letters x %u x %u sub-pixel offsets), advance %spx\n", bank.n_templates, n_letters,
            1u << args.x_bits, 1u << args.y_bits, f32s(bank.advance_px).c_str());
}

void save_letters(const focr_bank_t &bank) {
    mkdir("letters", 0777);
    for (size_t t = 0; t < bank.n_templates; t++) {
        const focr_template_t &d = bank.templates[t];
        std::string path = "letters/" + utf8_encode(d.letter) + "-" + std::to_string((size_t)(d.off_x * 1000.f)) + "_" +
                           std::to_string((size_t)(d.off_y * 1000.f)) + ".png";
        if (focr_image_save_png(path.c_str(), bank.needles + d.offset, d.n_w, d.n_h, 1) != 0) die("cannot write " + path);  // 8-bit grey, src/ncc.rs:642-649
    }
}

// decoder threads: the host's cores, at most 64 (more only fight over the address space), within the container's quota
unsigned feed_threads() {
    unsigned n = std::min(64u, std::max(1u, std::thread::hardware_concurrency()));
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // a container's CPU quota: threads beyond it only get throttled (measured: 4 096
        unsigned long long quota = 0, period = 0;           // headers in 15 ms with 16 threads on a 16-CPU quota, 130 ms with 64)
        if (fscanf(f, "%llu %llu", &quota, &period) == 2 && period) n = std::min<unsigned>(n, (unsigned)std::max<unsigned long long>(1, quota / period));
        fclose(f);
    }
    if (const char *e = getenv("FOCR_CLI_THREADS")) n = std::max(1u, (unsigned)strtoul(e, nullptr, 10));
    return n;
}

size_t env_count(const char *name, size_t otherwise) {  // a count of at least 1 from the environment
    const char *e = getenv(name);
    return e ? std::max<size_t>(1, strtoul(e, nullptr, 10)) : otherwise;
}

// One executor per device behind one handle (focr_fleet_*, include/focr_ncc.h): contexts and banks are set up in
// parallel, batch b goes to device b % n_dev, fleet tickets are 1, 2, 3 ... in submission order.
focr_fleet_t *open_fleet(PageFeed &feed, const focr_bank_t &bank, size_t n_dev, size_t n_lanes) {
    focr_fleet_t *fleet = nullptr;
    std::vector<int> devs(n_dev);
    for (size_t d = 0; d < n_dev; d++) devs[d] = (int)d;
    if (focr_fleet_create(devs.data(), (unsigned)n_dev, (unsigned)n_lanes, &fleet) != FOCR_OK) fatal(feed, std::string("no usable GPU: ") + focr_last_error_global());
    if (focr_fleet_bank_upload(fleet, bank.templates, bank.n_templates, bank.needles, bank.needles_len) != FOCR_OK)
        fatal(feed, std::string("focr_bank_upload: ") + focr_last_error_global());
    focr_fleet_set_fetch(fleet, 1);  // every lane copies its batch's counts and lines to page-locked memory itself
    return fleet;
}

void warn_capped(const Args &args, const uint32_t *counts, size_t n) {  // src/ncc.rs:395-397
    for (size_t q = 0; q < n; q++)
        if (!args.rust && counts[q] == FOCR_MAX_MATCHES) fprintf(stderr, "WARN got >= %d matches\n", FOCR_MAX_MATCHES);
}

// --raw, src/ncc.rs:683-698: every pre-NMS hit of the one image, in get_hits order, then exit without process_hits
[[noreturn]] void run_raw(const Run &run, PageFeed &feed) {
    const Args &args = run.args;
    const PageFeed::Decoded page = feed.wait_decoded(0);
    if (!page.err.empty()) fatal(feed, "cannot open image: " + page.err);
    uint64_t ticket = 0;
    focr_ctx_t *ctx = nullptr;
    if (focr_fleet_submit(run.fleet, page.slab, 0, 1, feed.batch(0).w, feed.batch(0).h, 1, args.threshold, run.cap(), run.mode(), 0, args.anchor_threshold,
                          args.overlap, &ticket) != FOCR_OK ||
        focr_fleet_wait(run.fleet, ticket, &ctx) != FOCR_OK)
        fatal(feed, std::string("scan: ") + (ctx ? focr_last_error(ctx) : focr_last_error_global()));
    // `what` is the call's text, as the messages have always named it: fixed strings, not to be kept in step with the calls
    const auto ck = [&](const char *what, int rc) { if (rc != FOCR_OK) die(std::string(what) + ": " + focr_last_error(ctx)); };
    const size_t T = run.bank.n_templates;
    std::vector<uint32_t> counts(T);
    ck("focr_get_counts(ctx, counts.data())", focr_get_counts(ctx, counts.data()));
    warn_capped(args, counts.data(), T);
    std::vector<uint64_t> off(T + 1);
    std::vector<focr_match_t> m(focr_total_matches(ctx));
    ck("focr_get_matches(ctx, off.data(), m.data())", focr_get_matches(ctx, off.data(), m.data()));
    std::string out;
    for (size_t t = 0; t < T; t++) {
        const focr_template_t &d = run.bank.templates[t];
        for (uint64_t q = off[t]; q < off[t + 1]; q++) {
            float cx = (float)m[q].x + (float)d.n_w * 0.5f, cy = (float)m[q].y + (float)d.n_h * 0.5f;
            char row[256];
            snprintf(row, sizeof row, "%u,%s,%s,%u,%u,%u,%u,%s,%s,%s,%s\n", d.letter, f32s(cx).c_str(), f32s(cy).c_str(), m[q].x, m[q].y, d.n_w,
                     d.n_h, f32s(d.bearing_x).c_str(), f32s(d.corrected_off_y).c_str(), f32s(d.off_x).c_str(), f32s(d.off_y).c_str());
            out += row;
        }
    }
    fwrite(out.data(), 1, out.size(), stdout);
    focr_fleet_release(run.fleet, ticket);
    feed.stop();
    fflush(stdout);
    fflush(stderr);
    _exit(0);
}

// -v, the reference's per-template line (src/ncc.rs:657-666); one device pass scans every template of every page of
// the batch, so "elapsed" is the batch's device time divided evenly over its (page, template) pairs
void print_template_lines(const Run &run, const PageFeed::Batch &B, const focr_host_results_t &R, std::vector<uint64_t> &hits_by_letter) {
    const size_t T = run.bank.n_templates;
    const double per_pair_ms = (double)R.device_ms / (double)(B.n * T);
    for (size_t k = 0; k < B.n; k++) {
        uint64_t page_hits = 0;
        for (size_t t = 0; t < T; t++) {
            const focr_template_t &d = run.bank.templates[t];
            const uint32_t cnt = R.counts[k * T + t];
            page_hits += cnt;
            hits_by_letter[t % run.alphabet.size()] += cnt;
            fprintf(stderr, "`%s` [%s, %s] needle size %ux%u hits %u elapsed %.4fms (%.4f ns/pixel, batch average)\n",
                    utf8_encode(d.letter).c_str(), f32s(d.off_x).c_str(), f32s(d.off_y).c_str(), d.n_w, d.n_h, cnt, per_pair_ms,
                    per_pair_ms * 1e6 / (double)(B.w * B.h));
        }
        fprintf(stderr, "overall %.4fms\nhits: %llu\n", (double)R.device_ms / (double)B.n, (unsigned long long)page_hits);
    }
}

// The context a completed batch ran in, for what is read between its wait and its release (focr_fleet_host_results
// completed the batch: this wait returns at once).
focr_ctx_t *batch_ctx(const Run &run, PageFeed &feed, uint64_t ticket) {
    focr_ctx_t *ctx = nullptr;
    if (focr_fleet_wait(run.fleet, ticket, &ctx) != FOCR_OK) fatal(feed, std::string("scan: ") + focr_last_error_global());
    return ctx;
}

// --verify: the batch's images from the device it ran on, "<image> <mse>" on stderr, the PNGs queued for the feed's threads
// so that the device loop does not wait for zlib
void write_verify(const Run &run, PageFeed &feed, const PageFeed::Batch &B, uint64_t ticket) {
    focr_ctx_t *ctx = batch_ctx(run, feed, ticket);
    // at most two batches of images in host memory; a full disk stops the run here, not after every batch
    if (const std::string failed = feed.png_throttle(run.batch_pages); !failed.empty()) fatal(feed, "cannot write " + failed);
    auto rgb = std::make_shared<std::vector<uint8_t>>(B.n * B.w * B.h * 3);
    std::vector<uint64_t> sums(B.n, 0);
    if (focr_verify_images(ctx, rgb->data(), 0, sums.data()) != FOCR_OK) fatal(feed, std::string("focr_verify_images: ") + focr_last_error(ctx));
    std::vector<std::string> paths(B.n);
    for (size_t k = 0; k < B.n; k++) {  // red_blue_mse's quotient and `focr --verify`'s line
        const float mse = (float)sums[k] / (float)(uint32_t)(B.w * B.h);
        fprintf(stderr, "%s %.6f\n", run.args.img[B.p0 + k].c_str(), (double)mse);
        paths[k] = cli::verify_path(run.args.verify, run.args.img[B.p0 + k]);
    }
    feed.queue_pngs(paths, rgb, B.w, B.h);
}

// --scores: the batch's runner-ups, read where --verify reads its images.  Batches retire in input order, so the file is
// in input order whatever the device count.
void write_scores(const Run &run, PageFeed &feed, const PageFeed::Batch &B, const focr_host_results_t &R, uint64_t ticket) {
    focr_ctx_t *ctx = batch_ctx(run, feed, ticket);
    std::vector<focr_runner_t> runners(R.n_chars);
    if (focr_get_runners(ctx, runners.data()) != FOCR_OK) fatal(feed, std::string("focr_get_runners: ") + focr_last_error(ctx));
    std::string rows;
    for (size_t k = 0; k < B.n; k++)
        for (uint64_t l = R.page_line_off[k]; l < R.page_line_off[k + 1]; l++)
            for (uint64_t q = R.line_char_off[l]; q < R.line_char_off[l + 1]; q++)
                scores_row(rows, B.p0 + k, (size_t)(l - R.page_line_off[k]), (size_t)(q - R.line_char_off[l]), R.chars[q], runners[q]);
    if (fwrite(rows.data(), 1, rows.size(), run.scores_file) != rows.size()) fatal(feed, "cannot write " + run.args.scores);
}

// the batch's lines in page order, src/ncc.rs:849-877: text (with --spaces: blanks for gaps) or --csv rows
void format_lines(const Run &run, const PageFeed::Batch &B, const focr_host_results_t &R, std::string &out) {
    const Args &args = run.args;
    const uint64_t *line_off = R.line_char_off;
    const focr_hit_t *chars = R.chars;
    for (size_t k = 0; k < B.n; k++) {
        for (uint64_t l = R.page_line_off[k]; l < R.page_line_off[k + 1]; l++) {
            const size_t nq = line_off[l + 1] - line_off[l];
            if (args.verbose) {  // process_hits' per-line histogram of the x distance between consecutive characters (src/ncc.rs:767-778)
                std::map<int, int> dx_counts;
                for (uint64_t q = line_off[l] + 1; q < line_off[l + 1]; q++) dx_counts[(int)chars[q].x - (int)chars[q - 1].x]++;
                std::string h = "{";
                for (auto &kv : dx_counts) h += (h.size() > 1 ? ", " : "") + std::to_string(kv.first) + ": " + std::to_string(kv.second);
                fprintf(stderr, "%s}\n", h.c_str());
            }
            if (!args.csv) {
                const size_t at = out.size();
                out.resize(at + 4 * nq + (args.spaces ? 4096 : 0) + 1);
                size_t need = focr_line_text(chars + line_off[l], nq, run.bank.advance_px, args.spaces, &out[at], out.size() - at);
                if (need + 1 > out.size() - at) {  // a very wide gap: size exactly and redo
                    out.resize(at + need + 1);
                    need = focr_line_text(chars + line_off[l], nq, run.bank.advance_px, args.spaces, &out[at], out.size() - at);
                }
                out.resize(at + need);
                out += '\n';
                continue;
            }
            for (uint64_t q = line_off[l]; q < line_off[l + 1]; q++) {
                const focr_hit_t &c = chars[q];
                float cx = (float)c.x + (float)c.w * 0.5f, cy = (float)c.y + (float)c.h * 0.5f;
                char row[160];
                snprintf(row, sizeof row, "%zu,%u,%s,%s,%u,%u,%u,%u\n", B.p0 + k, c.letter, f32s(cx).c_str(), f32s(cy).c_str(), c.x, c.y, c.w,
                         c.h);
                out += row;
            }
        }
    }
}

// results of batch b: read from its lane's context, formatted in page order, lane and slab released
void retire_batch(const Run &run, PageFeed &feed, Totals &sums, size_t b, uint64_t ticket) {
    const PageFeed::Batch &B = feed.batch(b);
    focr_host_results_t R{};
    auto t0 = Clock::now();
    if (focr_fleet_host_results(run.fleet, ticket, &R) != FOCR_OK) fatal(feed, std::string("scan: ") + focr_last_error_global());
    warn_capped(run.args, R.counts, B.n * run.bank.n_templates);
    sums.ms_device += R.device_ms;
    if (run.args.verbose) print_template_lines(run, B, R, sums.hits_by_letter);
    if (run.args.have_verify) write_verify(run, feed, B, ticket);
    if (run.scores_file) write_scores(run, feed, B, R, ticket);
    sums.ms_results += ms_since(t0);
    t0 = Clock::now();
    format_lines(run, B, R, sums.out);
    if (focr_fleet_release(run.fleet, ticket) != FOCR_OK) fatal(feed, "focr_fleet_release failed");  // the lane's result buffers are free again
    if (sums.out.size() > (1u << 20) || b + 1 == feed.n_batches()) {
        fwrite(sums.out.data(), 1, sums.out.size(), stdout);
        sums.out.clear();
    }
    sums.ms_format += ms_since(t0);
    feed.retired(b);
}

// Steps 3 + 4 of the pipeline: submit in batch order (device b % n_dev, lanes round-robin inside the executor), retire in
// batch order.
void run_batches(const Run &run, PageFeed &feed, Totals &sums, size_t n_dev) {
    const Args &args = run.args;
    const size_t n_batches = feed.n_batches();
    const size_t max_inflight = focr_fleet_slots(run.fleet);  // devices x lanes x contexts per lane
    std::vector<uint64_t> tickets(n_batches, 0);
    size_t next_retire = 0;
    for (size_t b = 0; b < n_batches; b++) {
        for (; b - next_retire >= max_inflight; next_retire++) retire_batch(run, feed, sums, next_retire, tickets[next_retire]);  // the context batch b maps to still holds batch b - max_inflight
        if (b + n_dev == n_batches) (void)focr_fleet_announce_last(run.fleet);  // the devices' last batches: their tails need not leave room for a next scan
        const auto t0 = Clock::now();
        const PageFeed::Decoded pages = feed.wait_decoded(b);
        sums.ms_wait += ms_since(t0);
        if (!pages.err.empty()) fatal(feed, "cannot open image: " + pages.err);  // image::open(..).unwrap(), src/ncc.rs:575
        if (focr_fleet_submit(run.fleet, pages.slab, 0, feed.batch(b).n, feed.batch(b).w, feed.batch(b).h, 1, args.threshold, run.cap(), run.mode(), 1,
                              args.anchor_threshold, args.overlap, &tickets[b]) != FOCR_OK)
            fatal(feed, std::string("focr_fleet_submit: ") + focr_last_error_global());
    }
    for (; next_retire < n_batches; next_retire++) retire_batch(run, feed, sums, next_retire, tickets[next_retire]);
}

void print_letter_totals(const std::vector<uint32_t> &alphabet, const std::vector<uint64_t> &hits_by_letter) {
    std::vector<std::pair<uint64_t, uint32_t>> by;  // src/ncc.rs:711-718: (count, char) ascending, zero counts skipped
    for (size_t a = 0; a < alphabet.size(); a++)
        if (hits_by_letter[a]) by.push_back({hits_by_letter[a], alphabet[a]});
    std::sort(by.begin(), by.end());
    for (auto &kv : by) fprintf(stderr, "`%s` %llu\n", utf8_encode(kv.second).c_str(), (unsigned long long)kv.first);
}

}  // namespace

// Pipeline (the reference's page parallelism, src/ncc.rs:839-847, on the GPU's terms):
//   1. all host cores read the image headers, then the batch plan is fixed: consecutive pages of one size, at most
//      FOCR_CLI_BATCH per batch, each batch owning one page-aligned slab slot per page (PageFeed::plan);
//   2. the same cores decode, in index order, straight into their page's slot (binary PGM: one fread), while the
//      main thread brings the HIP runtime up and page-locks the slabs (PageFeed::start, focr_host_register);
//   3. a decoded batch goes to the next device round-robin (every visible GPU, FOCR_CLI_DEVICES caps the count) as
//      ONE upload + scan + process_hits in one context of that device's executor (focr_pipe_*: FOCR_CLI_CONTEXTS lanes
//      per device, default 3, two contexts each), queued on the device at once: a batch's DMA and small kernels run under
//      other batches' MFMA scans and no lane waits for this thread between two batches;
//   4. results are retired in batch order and written in page order: the bytes on stdout are those of the
//      reference's sorted print (src/ncc.rs:845-877) whatever the device count.
int main(int argc, char **argv) {
    setenv("GPU_MAX_HW_QUEUES", "8", 0);  // more streams than the default 4 hardware queues must not share one
    const Args args = parse_args(argc, argv);
    const bool timing = args.verbose || getenv("FOCR_CLI_TIMING") != nullptr;  // phase / pipeline summary lines on stderr
    PhaseClock clk{timing};
    int box = args.box_size == "font" ? FOCR_BOX_FONT : args.box_size == "alphabet" ? FOCR_BOX_ALPHABET : args.box_size == "char" ? FOCR_BOX_CHAR : -1;
    if (box < 0) die("called `Result::unwrap()` on an `Err` value: () (--box-size must be font, alphabet or char)");  // src/ncc.rs:559
    if (args.raw && args.img.size() != 1) die("assertion failed: args.img.len() == 1");  // src/ncc.rs:834

    // template bank, once (get_hits re-does this per page: src/ncc.rs:561, 587-639)
    const std::vector<uint32_t> alphabet = utf8_decode(args.alphabet);
    focr_bank_t bank{};
    char err[256] = {0};
    if (focr_raster_bank(args.font.c_str(), args.text_size, args.x_bits, args.y_bits, args.hinting, alphabet.data(), alphabet.size(),
                         box, args.x_padding, args.y_padding, &bank, err, sizeof err) != 0)
        die(std::string("rasterising the template bank failed: ") + err);
    clk.lap("bank raster");
    if (args.verbose) print_metrics_preamble(args, bank, alphabet.size());
    for (size_t t = 0; t < bank.n_templates; t++)
        if (bank.templates[t].n_w > 16 && !args.allow_wide) die("not handled");  // src/ncc.rs:392
    if (args.save_letters) save_letters(bank);
    if (args.img.empty()) return 0;
    FILE *scores_file = nullptr;
    if (args.have_scores) {
        if (!(scores_file = fopen(args.scores.c_str(), "w"))) die("cannot write " + args.scores);
        fputs(SCORES_HEADER, scores_file);
    }

    // 1. headers and plan
    const size_t batch_pages = env_count("FOCR_CLI_BATCH", 128);
    PageFeed feed(args.img, batch_pages, feed_threads(), args.have_verify);
    if (const std::string e = feed.plan(); !e.empty()) die("cannot open image: " + e);  // image::open(..).unwrap(), src/ncc.rs:575
    const size_t n_batches = feed.n_batches();
    clk.lap("headers + plan");

    // 2. decoders may fill the first slabs while the HIP runtime comes up: plain page-aligned memory now, page-locked below
    if (const std::string e = feed.start(4); !e.empty()) die(e);
    const size_t dev_cap = args.raw ? 1 : env_count("FOCR_CLI_DEVICES", ~(size_t)0);
    const size_t n_dev = std::min<size_t>({(size_t)std::max(0, focr_device_count()), dev_cap, n_batches});
    if (n_dev == 0) fatal(feed, std::string("no usable GPU: ") + focr_last_error_global());
    const size_t n_lanes = std::min(args.raw ? 1 : std::min<size_t>(8, env_count("FOCR_CLI_CONTEXTS", 3)), (n_batches + n_dev - 1) / n_dev);
    const Run run{args, bank, alphabet, open_fleet(feed, bank, n_dev, n_lanes), scores_file, batch_pages};
    // the remaining slabs: enough for every context of every device's executor to hold one batch plus a few being decoded
    // ahead; then page-lock all of them (a slab that cannot be locked still works, through a staged copy)
    if (const std::string e = feed.grow(focr_fleet_slots(run.fleet) + 4); !e.empty()) fatal(feed, e);
    for (uint8_t *p : feed.slabs()) (void)focr_host_register(p, feed.slab_bytes());
    clk.lap("ctx + bank");

    if (args.raw) run_raw(run, feed);
    Totals sums;
    if (args.verbose) sums.hits_by_letter.assign(alphabet.size(), 0);
    run_batches(run, feed, sums, n_dev);
    // --verify: every image is on disk before the pool goes
    if (const std::string failed = feed.close_pngs(); !failed.empty()) fatal(feed, "cannot write " + failed);
    feed.stop();
    if (scores_file && fclose(scores_file) != 0) die("cannot write " + args.scores);
    if (args.verbose) print_letter_totals(alphabet, sums.hits_by_letter);
    if (timing) {
        fprintf(stderr, "pipeline: %zu batch(es) of <= %zu pages on %zu device(s) x %zu lane(s); main thread waited %.2f ms for decode; sums: device %.2f ms, "
                        "results (wait + counts + lines) %.2f ms, format %.2f ms\n",
                n_batches, batch_pages, n_dev, n_lanes, sums.ms_wait, sums.ms_device, sums.ms_results, sums.ms_format);
    }
    clk.lap("pages");
    fflush(stdout);
    // Everything is written.  The executors' contexts (a dozen streams, some gigabytes of device memory) are NOT taken apart call by
    // call — 80 ms of hipFree / hipStreamDestroy in front of a process exit that reclaims all of it at once; FOCR_CLI_TEARDOWN=1 keeps
    // the orderly teardown (leak checks).
    if (getenv("FOCR_CLI_TEARDOWN")) {
        focr_fleet_destroy(run.fleet);
        focr_bank_free(&bank);
        clk.lap("teardown");
    }
    if (timing) fprintf(stderr, "total since main() %8.2f ms\n", ms_since(clk.t0));
    // Everything is flushed and the contexts are gone: leave without the HIP runtime's exit handlers (~170 ms).
    fflush(stdout);
    fflush(stderr);
    _exit(0);
}
