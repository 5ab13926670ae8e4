#!/usr/bin/env python3
"""Throughput of the focr line decoder: one JSON line for a batch of synthetic 608x720 pages (DejaVu Sans Mono 13 px,
focr's default alphabet, 40 text lines at line_advance 15, decoded at x 45, y 39, width 608, line height 12).

  host_table_ms        building the 64-phase decode font on the host (FreeType)
  device_ms_per_batch  median over --steps runs after --warmup, device events around the batch's kernels
  wall_ms_per_batch    median host time of one decode() call (upload, launches, read-back)
  pages/s, lines/s and page Mpx/s from the device time
With --verify, also focr --verify's images of the batch on the device (focr_decoder_verify):
  verify_device_ms_per_batch  median device time of the verify's kernels
  verify_launches             their launch count
  verify_wall_ms              median host time of one verify call with the images read back to the host
With --scores, also the decode with per-character scores on (LineDecoder.decode(scores=True)), in runs that alternate with
plain ones so that both see the same clocks:
  scores_device_ms_per_batch  median device time of the batch's kernels with scores on (the same 3 launches)
  scores_plain_device_ms      median device time of the plain runs in between
  scores_over_plain           the ratio of the two
  scores_wall_ms_per_batch    median host time of one decode(scores=True) call (more to read back and to unpack)
With --pen-search N, also the decode with a pen search of N/64 px (LineDecoder.decode(pen_search=N)), in runs that
alternate with plain ones:
  search_device_ms_per_batch  median device time of the batch's kernels with the search on (the same 3 launches)
  search_plain_device_ms      median device time of the plain runs in between
  search_over_plain           the ratio of the two, beside search_candidates = 2 N + 1 offsets per glyph
  search_wall_ms_per_batch    median host time of one decode(pen_search=N) call, offsets read back and unpacked
  search_lines_changed        lines of the batch the search decodes differently from the plain run
With --whole-line, also the whole-line decode (LineDecoder.decode(whole_line=True)), in runs that alternate with plain
ones; --font PATH sets the pages and decodes them in another font than DejaVu Sans Mono (a proportional one is what the
mode is for: nearly every 1/64 px pen is then a state, where a monospace line has one state per character):
  whole_device_ms_per_batch   median device time of the batch's kernels with the mode on (the same 3 launches)
  whole_plain_device_ms       median device time of the plain runs in between
  whole_over_plain            the ratio of the two
  whole_wall_ms_per_batch     median host time of one decode(whole_line=True) call, pens and costs read back and unpacked
  whole_lines_changed         lines of the batch the mode decodes differently from the plain run
With --whole-line --margins, also the whole-line decode with per-character margins (LineDecoder.decode(whole_line=True,
margins=True)), in runs that alternate with whole-line runs without them:
  margins_device_ms_per_batch median device time of the batch's kernels with margins on (the same 3 launches)
  margins_whole_device_ms     median device time of the whole-line runs in between
  margins_over_whole          the ratio of the two
  margins_wall_ms_per_batch   median host time of one decode(whole_line=True, margins=True) call, margins read back and unpacked
  margins_text_equal          the margins runs return the whole-line runs' lines, pens and costs
With --whole-line --pen-slack N, also the whole-line decode with a pen slack of N/64 px (LineDecoder.decode(whole_line=True,
pen_slack=N)), in runs that alternate with whole-line runs without it:
  slack_device_ms_per_batch   median device time of the batch's kernels with the slack on (the same 3 launches)
  slack_whole_device_ms       median device time of the whole-line runs in between
  slack_over_whole            the ratio of the two
  slack_wall_ms_per_batch     median host time of one decode(whole_line=True, pen_slack=N) call, offsets read back and unpacked
  slack_lines_changed         lines of the batch the slack decodes differently from the whole-line run
  slack_chars_offset          characters of the batch that took an offset other than 0
With --baseline-search N [--y-bits B], also the decode with a baseline search of N steps of 2^-B px either way
(LineDecoder.decode(baseline_search=N) with the font's y-phase tables of B), in runs that alternate with plain ones:
  base_device_ms_per_batch    median device time of the batch's kernels with the search on (the same 3 launches)
  base_plain_device_ms        median device time of the plain runs in between
  base_over_plain             the ratio of the two, beside base_candidates = 2 N + 1 decodes per line and base_ceiling =
                              2 N + 2, what one plain run per candidate and one more for the winner would cost
  base_wall_ms_per_batch      median host time of one decode(baseline_search=N) call, offsets and costs read back
  base_lines_changed          lines of the batch the search decodes differently from the plain run
  base_lines_offset           lines of the batch that took an offset other than 0
With --whole-line --whole-baseline N [--y-bits B], also the whole-line decode under the 2 N + 1 baseline candidates
(LineDecoder.decode(whole_line=True, whole_baseline=N)), in runs that alternate with whole-line runs without it:
  wbase_device_ms_per_batch   median device time of the batch's kernels with the candidates on (the same 3 launches)
  wbase_whole_device_ms       median device time of the whole-line runs in between
  wbase_over_whole            the ratio of the two, beside wbase_candidates = wbase_ceiling = 2 N + 1: one whole-line run
                              per candidate (the winner is not decoded again)
  wbase_wall_ms_per_batch     median host time of one such decode call, pens, costs and offsets read back
  wbase_lines_changed         lines of the batch the mode decodes differently from the whole-line run
  wbase_lines_offset          lines of the batch that took an offset other than 0
With --verify beside --baseline-search or --whole-baseline, also the verify of that baseline run (its moved compose):
  base_verify_device_ms, wbase_verify_device_ms            median device time of the verify's two kernels, the images drawn
  base_verify_sums_device_ms, wbase_verify_sums_device_ms  ... and of the verify that draws no image, in alternating calls
With --line-frac Y,A beside --baseline-search or --whole-line --whole-baseline, the pages are drawn on the fractional line
grid y + Y/64 + i * (line_advance + A/64) px (every glyph rasterised at its line's sub-pixel row), every section above runs
on those pages, and the mode in force is also timed with the grid on (LineDecoder.decode(..., y_frac=Y,
line_advance_frac=A)), in runs that alternate with the same mode at the same radius on the whole-pixel grid:
  frac_device_ms_per_batch    median device time of the batch's kernels with the grid on (the same 3 launches)
  frac_off_device_ms          median device time of the whole-pixel runs in between
  frac_over_off               the ratio of the two (the candidate count is the same)
  frac_wall_ms_per_batch      median host time of one decode call with the grid on
  frac_lines, frac_off_lines  non-blank lines found on either grid
  frac_lines_changed          lines of the batch whose text differs between the two grids (by position in the page)
With --font-candidates SIZES (comma-separated text sizes, K of them), also the decode with the font search on
(LineDecoder.decode(font_search=True)) over the decode font and K candidates of the same face at those sizes, in runs that
alternate with plain ones; with --whole-line as well, the same under the whole-line decode, alternating with whole-line runs:
  fonts_device_ms_per_batch   median device time of the batch's kernels with the search on (the same 3 launches)
  fonts_plain_device_ms       median device time of the plain runs in between
  fonts_over_plain            the ratio of the two, beside fonts_candidates = K + 1 decodes per line and fonts_ceiling = K + 2,
                              what one plain run per candidate and one more for the winner would cost
  fonts_wall_ms_per_batch     median host time of one decode(font_search=True) call, winners and costs read back
  fonts_lines_changed         lines of the batch the search decodes differently from the plain run
  fonts_lines_other           lines of the batch won by another candidate than the decode font
  wfonts_*                    the same under the whole-line decode, over wfonts_whole_device_ms; wfonts_ceiling = K + 1: one
                              whole-line run per candidate (the winner is not decoded again)
With --verify-text, also focr_decoder_verify_text (LineDecoder.verify_text) over the plain run's decoded lines, in calls that
alternate with focr_decoder_verify of the same run, both with the images read back:
  vtext_device_ms_per_batch   median device time of verify_text's two kernels
  vtext_verify_device_ms      median device time of the verify's two kernels in between
  vtext_over_verify           the ratio of the two
  vtext_wall_ms               median host time of one verify_text call (the lines packed in Python, uploads, images read back)
  vtext_equal                 verify_text's images and sums equal the verify's
and with --font-candidates SIZES as well, one mixed-font call over the same lines, line q of a page drawn in font q mod (K + 1):
  vtext_mixed_device_ms       median device time of its two kernels, beside vtext_mixed_fonts = K + 1
With --score-text, also focr_decoder_score_text (LineDecoder.score_text) over the plain run's decoded lines at the shift radii
0, 8 and 64, in calls that alternate with the plain decode of the same batch:
  stext_device_ms             median device time of score_text's launch per radius: {"0": .., "8": .., "64": ..}
  stext_device_ms_min         ... and the lowest
  stext_plain_device_ms       median device time of the plain decodes in between
  stext_over_plain            stext_device_ms["0"] over it: one glyph per character against the alphabet per step
  stext_over_radius0          per radius N the ratio to radius 0, beside stext_ceiling = 2N + 1
  stext_wall_ms               median host time of one radius-0 call (the lines packed in Python, uploads, results read back)
  stext_equal                 at radius 0 every line's terms and line_base equal the scores run's (decode(scores=True))
With --align-text, also focr_decoder_align_text (LineDecoder.align_text) over the plain run's decoded lines at the (drift, step)
pairs (0, 0), (16, 2) and (128, 8) from start 128 (every state of every band live), in calls that alternate with score_text at radius 0
on the same lines; the result also goes to profiles/focr_align_text_bench.json:
  atext_device_ms             median device time of align_text's launch per pair: {"0,0": .., "16,2": .., "128,8": ..}
  atext_device_ms_min         ... and the lowest
  atext_score_device_ms       median device time of the score_text calls in between (one term per character)
  atext_states                per pair the states of the band, 2 * drift + 1: the yardstick is that many score_text calls
  atext_over_yardstick        per pair atext_device_ms over atext_states x atext_score_device_ms
  atext_wall_ms               median host time of one (16, 2) call (the lines packed in Python, uploads, results read back)
  atext_equal                 at (0, 0) every line's cost and terms equal score_text's at the nominal pens
With --learn-text, also focr_decoder_learn_text (LineDecoder.learn_text) of font 0 over the plain run's decoded lines (its own reading:
what is timed is the work, not what the tables are worth), in calls that alternate with score_text at radius 0 on the same lines, at the
--steps and --warmup of the align_text run; the result also goes to profiles/focr_learn_text_bench.json:
  ltext_device_ms             median device time of learn_text's launch and the zeroing of its sums and counts in front of it
  ltext_device_ms_min         ... and the lowest
  ltext_score_device_ms       median device time of the score_text calls in between: the same strip and the same walk, without the adds
  ltext_over_score            ltext_device_ms over ltext_score_device_ms
  ltext_form                  how the sums are accumulated ("atomic": no-return 32-bit integer atomic adds straight to the cell)
  ltext_characters            the listed characters, ltext_used those whose box lay inside their crop, ltext_cells the cells seen
  ltext_wall_ms               median host time of one call (the lines packed in Python, uploads, sums and counts read back and added in uint64)
  ltext_equal                 a second call gives the same sums and counts, and the counts add up to the used characters
With --refine-text, also focr_decoder_refine_text (LineDecoder.refine_text) over the plain run's decoded lines at placed_pens(), at the
(radius, sweeps) pairs (0, 0), (4, 1) and (8, 1), in calls that alternate with decode(pen_search=radius) on the same pages: one sweep
evaluates the n * A * (2N + 1) candidates one pen-search run evaluates, so that run is the yardstick; the result also goes to
profiles/focr_refine_text_bench.json:
  rtext_device_ms             median device time of refine_text's launch per pair: {"0,0": .., "4,1": .., "8,1": ..}
  rtext_device_ms_min         ... and the lowest
  rtext_search_device_ms      median device time of the decode(pen_search=radius) runs in between (radius 0: the plain run)
  rtext_over_search           per pair rtext_device_ms over it
  rtext_candidates_per_character   A * (2N + 1)
  rtext_lines_cost_in_is_score_text   the lines whose composed cost equals score_text's at the same pens (no two footprints meet)
  rtext_characters_changed, rtext_lines_text_changed, rtext_cost_drop   per pair what the call changed, and the summed cost_in - cost
  rtext_wall_ms               median host time of one (4, 1) call (the lines packed in Python, uploads, results read back)
With --test-images, also focr --test's two RGBA images of the batch on the device (focr_decoder_test_images, over the
grey pages):
  test_device_ms_per_batch    median device time of its kernels (2 x pages x 608 x 720 x 4 bytes written)
  test_launches               their launch count
  test_wall_ms                median host time of one test_images call (upload, launches, both images read back)
  test_write_gb_per_s         the RGBA bytes written per second of device time

No reference number: the reference's Rust / font-kit build is not available to run beside it.  Kernel times per
launch come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from font_ocr_amd import FOCR_DEFAULT_ALPHABET, DecodeFont, LineDecoder  # noqa: E402
from font_ocr_amd.decoder import nominal_pens, placed_pens, raster_glyph, render_text  # noqa: E402

FONT = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")


def synth(n_pages, seed, W=608, H=720, x=45, y=39, n_lines=40, advance=15, size=13.0, font=FONT):
    rng = np.random.default_rng(seed)
    ink = FOCR_DEFAULT_ALPHABET.replace(" ", "")
    pages = np.full((n_pages, H, W), 255, dtype=np.uint8)
    for p in range(n_pages):
        for i in range(n_lines):
            words = [''.join(rng.choice(list(ink), int(rng.integers(2, 10)))) for _ in range(12)]
            c = render_text(font, size, " ".join(words)[:68])
            ly = y + i * advance
            hh, ww = min(c.shape[0], H - ly), min(c.shape[1], W - x)
            pages[p, ly: ly + hh, x: x + ww] = np.minimum(pages[p, ly: ly + hh, x: x + ww], 255 - c[:hh, :ww])
    return pages


def synth_frac(n_pages, seed, frac, W=608, H=720, x=45, y=39, n_lines=40, advance=15, size=13.0, font=FONT):
    """synth()'s pages on the fractional grid frac = (y_frac, advance_frac): line i's top at
    Y_i = 64 * y + y_frac + i * (64 * advance + advance_frac) in 1/64 px, every glyph rasterised by FreeType on the decoder's
    own line canvas at the row Y_i >> 6 with the vertical translation origin_y + (Y_i & 63) / 64."""
    rng = np.random.default_rng(seed)
    ink = FOCR_DEFAULT_ALPHABET.replace(" ", "")
    f = DecodeFont(font, size, FOCR_DEFAULT_ALPHABET)
    inc, (ox, oy) = f.increments(), f.origin
    f.close()
    pages = np.full((n_pages, H, W), 255, dtype=np.uint8)
    g = np.zeros((int(size) + 8, 2 * int(size) + 8), dtype=np.uint8)
    for p in range(n_pages):
        for i in range(n_lines):
            words = [''.join(rng.choice(list(ink), int(rng.integers(2, 10)))) for _ in range(12)]
            Y = 64 * y + frac[0] + i * (64 * advance + frac[1])
            ly, pen = Y >> 6, np.float32(0)
            for ch in " ".join(words)[:68]:
                col = int(pen)
                if ch != " ":
                    g[:] = 0
                    raster_glyph(font, size, ch, np.float32(ox + np.float32(4) + (pen - np.float32(col))), np.float32(oy + np.float32((Y & 63) / 64.0)), g)
                    x0 = x + col - 4
                    hh, ww = min(g.shape[0], H - ly), min(g.shape[1], W - x0)
                    if hh > 0 and ww > 0 and x0 >= 0:
                        pages[p, ly: ly + hh, x0: x0 + ww] = np.minimum(pages[p, ly: ly + hh, x0: x0 + ww], 255 - g[:hh, :ww])
                pen = np.float32(pen + inc[FOCR_DEFAULT_ALPHABET.index(ch)])
    return pages


def moved_verify(dec, a):
    """Device ms of the verify of the decoder's last run, a baseline one, with the images and without, in alternating calls."""
    with_images, without = [], []
    for i in range(a.warmup + a.steps):
        dec.verify()
        with_images.append(dec.last_verify_ms)
        dec.verify(images=False)
        without.append(dec.last_verify_ms)
    return with_images[a.warmup:], without[a.warmup:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--verify", action="store_true", help="also time the device verify of the batch")
    ap.add_argument("--test-images", action="store_true", help="also time focr --test's images of the batch")
    ap.add_argument("--verify-text", action="store_true", help="also time verify_text over the decoded lines against the verify of the same run")
    ap.add_argument("--score-text", action="store_true", help="also time score_text over the decoded lines at shift radii 0, 8 and 64 against the plain decode")
    ap.add_argument("--align-text", action="store_true", help="also time align_text over the decoded lines at (drift, step) (0, 0), (16, 2) and (128, 8) against score_text")
    ap.add_argument("--learn-text", action="store_true", help="also time learn_text over the decoded lines against score_text")
    ap.add_argument("--refine-text", action="store_true",
                    help="also time refine_text over the decoded lines at (radius, sweeps) (0, 0), (4, 1) and (8, 1) against decode(pen_search=radius)")
    ap.add_argument("--scores", action="store_true", help="also time the decode with per-character scores on")
    ap.add_argument("--pen-search", type=int, default=0, metavar="N", help="also time the decode with a pen search of N/64 px")
    ap.add_argument("--whole-line", action="store_true", help="also time the whole-line decode")
    ap.add_argument("--margins", action="store_true", help="with --whole-line: also time the whole-line decode with margins")
    ap.add_argument("--pen-slack", type=int, default=0, metavar="N", help="with --whole-line: also time the whole-line decode with a pen slack of N/64 px")
    ap.add_argument("--baseline-search", type=int, default=0, metavar="N", help="also time the decode with a baseline search of N steps either way")
    ap.add_argument("--whole-baseline", type=int, default=0, metavar="N",
                    help="with --whole-line: also time the whole-line decode under the baseline candidates of N steps either way")
    ap.add_argument("--y-bits", type=int, default=0, metavar="B", help="with --baseline-search or --whole-baseline: steps of 2^-B px")
    ap.add_argument("--line-frac", default=None, metavar="Y,A",
                    help="with --baseline-search or --whole-baseline: draw the pages on the fractional line grid and also time the mode with the grid on")
    ap.add_argument("--font-candidates", default=None, metavar="SIZES",
                    help="also time the font search over the decode font and candidates of the same face at these sizes (comma-separated)")
    ap.add_argument("--font", default=FONT, metavar="PATH", help="the font of the pages and of the decoder [DejaVu Sans Mono]")
    a = ap.parse_args()
    if a.margins and not a.whole_line:
        ap.error("--margins needs --whole-line")
    if a.pen_slack and not a.whole_line:
        ap.error("--pen-slack needs --whole-line")
    if a.whole_baseline and not a.whole_line:
        ap.error("--whole-baseline needs --whole-line")
    if a.y_bits and not (a.baseline_search or a.whole_baseline):
        ap.error("--y-bits needs --baseline-search or --whole-baseline")
    sizes = []
    if a.font_candidates:
        try:
            sizes = [float(v) for v in a.font_candidates.split(",")]
        except ValueError:
            ap.error("--font-candidates takes comma-separated text sizes")
        if not 1 <= len(sizes) <= 15:
            ap.error("--font-candidates takes 1 .. 15 sizes")
    frac = None
    if a.line_frac is not None:
        try:
            frac = tuple(int(v) for v in a.line_frac.split(","))
        except ValueError:
            frac = ()
        if len(frac) != 2 or not all(0 <= v <= 63 for v in frac):
            ap.error("--line-frac takes Y,A, each 0 .. 63 (1/64 px)")
        if not (a.baseline_search or a.whole_baseline):
            ap.error("--line-frac needs --baseline-search or --whole-baseline")
    pages = synth_frac(a.pages, a.seed, frac, font=a.font) if frac else synth(a.pages, a.seed, font=a.font)
    geo = (45, 39, 608, 12, 15)
    t0 = time.perf_counter()
    font = DecodeFont(a.font, 13.0, FOCR_DEFAULT_ALPHABET, y_bits=a.y_bits)
    host_ms = (time.perf_counter() - t0) * 1e3
    with LineDecoder(0) as dec:
        dec.set_font(font, 13.0)
        for _ in range(a.warmup):
            out = dec.decode(pages, *geo)
        dev, wall = [], []
        for _ in range(a.steps):
            t = time.perf_counter()
            out = dec.decode(pages, *geo)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(dec.last_ms)
        launches = int(dec._lib.focr_decoder_last_launches(dec._h))
        if a.verify:
            for _ in range(a.warmup):
                dec.verify()
            vdev, vwall = [], []
            for _ in range(a.steps):
                t = time.perf_counter()
                dec.verify()
                vwall.append((time.perf_counter() - t) * 1e3)
                vdev.append(dec.last_verify_ms)
            vlaunches = int(dec._lib.focr_decoder_last_verify_launches(dec._h))
        if a.verify_text:
            for _ in range(a.warmup):
                want = dec.verify()
                xgot = dec.verify_text(pages, out, geo[0])
            xequal = np.array_equal(want[0], xgot[0]) and all(np.array_equal(p, q) for p, q in zip(want[1], xgot[1]))
            xdev, xwall, xvdev = [], [], []
            for _ in range(a.steps):
                dec.verify()
                xvdev.append(dec.last_verify_ms)
                t = time.perf_counter()
                dec.verify_text(pages, out, geo[0])
                xwall.append((time.perf_counter() - t) * 1e3)
                xdev.append(dec.last_verify_text_ms)
            xlaunches = int(dec._lib.focr_decoder_last_verify_text_launches(dec._h))
        if a.score_text:
            crop = (geo[0], geo[2], geo[3])
            _, want = dec.decode(pages, *geo, scores=True)
            zgot = dec.score_text(pages, out, *crop)
            zequal = all(g.base == w.base and np.array_equal(g.terms, w.score - w.base) for pg, pw in zip(zgot, want) for g, w in zip(pg, pw))
            radii = (0, 8, 64)
            for _ in range(a.warmup):
                dec.decode(pages, *geo)
                for n in radii:
                    dec.score_text(pages, out, *crop, shift=n, terms=False)
            zdev, zpdev, zwall = {n: [] for n in radii}, [], []
            for _ in range(a.steps):
                for n in radii:
                    dec.decode(pages, *geo)
                    zpdev.append(dec.last_ms)
                    t = time.perf_counter()
                    dec.score_text(pages, out, *crop, shift=n, terms=False)
                    if n == 0:
                        zwall.append((time.perf_counter() - t) * 1e3)
                    zdev[n].append(dec.last_score_text_ms)
            zlaunches = int(dec._lib.focr_decoder_last_score_text_launches(dec._h))
        if a.align_text:
            crop = (geo[0], geo[2], geo[3])
            pairs, a_start = ((0, 0), (16, 2), (128, 8)), 128
            noms = [[nominal_pens(font, t, a_start) for _, t in pg] for pg in out]
            agot = dec.align_text(pages, out, *crop, start=a_start, drift=0, step=0)
            awant = dec.score_text(pages, out, *crop, pens=noms)
            aequal = all(g.base == w.base and g.cost == w.cost and np.array_equal(g.terms, w.terms) for pg, pw in zip(agot, awant) for g, w in zip(pg, pw))
            for _ in range(a.warmup):
                for w, n in pairs:
                    dec.score_text(pages, out, *crop, terms=False)
                    dec.align_text(pages, out, *crop, start=a_start, drift=w, step=n, terms=False)
            adev, asdev, awall = {pr: [] for pr in pairs}, [], []
            for _ in range(a.steps):
                for w, n in pairs:
                    dec.score_text(pages, out, *crop, terms=False)
                    asdev.append(dec.last_score_text_ms)
                    t = time.perf_counter()
                    dec.align_text(pages, out, *crop, start=a_start, drift=w, step=n, terms=False)
                    if (w, n) == pairs[1]:
                        awall.append((time.perf_counter() - t) * 1e3)
                    adev[(w, n)].append(dec.last_align_text_ms)
            alaunches = int(dec._lib.focr_decoder_last_align_text_launches(dec._h))
        if a.learn_text:
            crop = (geo[0], geo[2], geo[3])
            lgot = dec.learn_text(pages, out, *crop)
            lagain = dec.learn_text(pages, out, *crop)
            n_used = int(sum(int(u.sum()) for pg in lgot.used for u in pg))
            lequal = np.array_equal(lgot.sums, lagain.sums) and np.array_equal(lgot.counts, lagain.counts) and int(lgot.counts.sum()) == n_used
            for _ in range(a.warmup):
                dec.score_text(pages, out, *crop, terms=False)
                dec.learn_text(pages, out, *crop)
            ldev, lsdev, lwall = [], [], []
            for _ in range(a.steps):
                dec.score_text(pages, out, *crop, terms=False)
                lsdev.append(dec.last_score_text_ms)
                t = time.perf_counter()
                dec.learn_text(pages, out, *crop)
                lwall.append((time.perf_counter() - t) * 1e3)
                ldev.append(dec.last_learn_text_ms)
            llaunches = int(dec._lib.focr_decoder_last_learn_text_launches(dec._h))
        if a.refine_text:
            crop = (geo[0], geo[2], geo[3])
            rpairs = ((0, 0), (4, 1), (8, 1))
            placed = [[placed_pens(font, t) for _, t in pg] for pg in out]
            rgot = {pr: dec.refine_text(pages, out, *crop, placed, radius=pr[0], sweeps=pr[1]) for pr in rpairs}
            rwant = dec.score_text(pages, out, *crop, pens=placed, terms=False)
            rsame = sum(g.cost_in == w.cost for pg, pw in zip(rgot[rpairs[0]], rwant) for g, w in zip(pg, pw))
            for _ in range(a.warmup):
                for n, sw in rpairs:
                    dec.decode(pages, *geo, pen_search=n)
                    dec.refine_text(pages, out, *crop, placed, radius=n, sweeps=sw)
            rdev, rsdev, rwall = {pr: [] for pr in rpairs}, {pr: [] for pr in rpairs}, []
            for _ in range(a.steps):
                for n, sw in rpairs:
                    dec.decode(pages, *geo, pen_search=n)
                    rsdev[(n, sw)].append(dec.last_ms)
                    t = time.perf_counter()
                    dec.refine_text(pages, out, *crop, placed, radius=n, sweeps=sw)
                    if (n, sw) == rpairs[1]:
                        rwall.append((time.perf_counter() - t) * 1e3)
                    rdev[(n, sw)].append(dec.last_refine_text_ms)
            rlaunches = int(dec._lib.focr_decoder_last_refine_text_launches(dec._h))
            dec.decode(pages, *geo)  # the plain run is the last run again
        if a.scores:
            for _ in range(a.warmup):
                dec.decode(pages, *geo, scores=True)
            sdev, swall, pdev = [], [], []
            for _ in range(a.steps):
                dec.decode(pages, *geo)
                pdev.append(dec.last_ms)
                t = time.perf_counter()
                dec.decode(pages, *geo, scores=True)
                swall.append((time.perf_counter() - t) * 1e3)
                sdev.append(dec.last_ms)
            slaunches = int(dec._lib.focr_decoder_last_launches(dec._h))
        if a.pen_search:
            for _ in range(a.warmup):
                dec.decode(pages, *geo, pen_search=a.pen_search)
            ndev, nwall, npdev = [], [], []
            for _ in range(a.steps):
                dec.decode(pages, *geo)
                npdev.append(dec.last_ms)
                t = time.perf_counter()
                dec.decode(pages, *geo, pen_search=a.pen_search)
                nwall.append((time.perf_counter() - t) * 1e3)
                ndev.append(dec.last_ms)
            found, _ = dec.decode(pages, *geo, pen_search=a.pen_search)
            nlaunches = int(dec._lib.focr_decoder_last_launches(dec._h))
        if a.whole_line:
            for _ in range(a.warmup):
                dec.decode(pages, *geo, whole_line=True)
            wdev, wwall, wpdev = [], [], []
            for _ in range(a.steps):
                dec.decode(pages, *geo)
                wpdev.append(dec.last_ms)
                t = time.perf_counter()
                whole = dec.decode(pages, *geo, whole_line=True)[0]
                wwall.append((time.perf_counter() - t) * 1e3)
                wdev.append(dec.last_ms)
            wlaunches = int(dec._lib.focr_decoder_last_launches(dec._h))
        if a.margins:
            for _ in range(a.warmup):
                dec.decode(pages, *geo, whole_line=True, margins=True)
            mdev, mwall, mwdev = [], [], []
            for _ in range(a.steps):
                ref = dec.decode(pages, *geo, whole_line=True)
                mwdev.append(dec.last_ms)
                t = time.perf_counter()
                got = dec.decode(pages, *geo, whole_line=True, margins=True)
                mwall.append((time.perf_counter() - t) * 1e3)
                mdev.append(dec.last_ms)
            mlaunches = int(dec._lib.focr_decoder_last_launches(dec._h))
            mequal = got[0] == ref[0] and got[2] == ref[2] and all(np.array_equal(x, y) for pa, pb in zip(got[1], ref[1]) for x, y in zip(pa, pb))
        if a.pen_slack:
            for _ in range(a.warmup):
                dec.decode(pages, *geo, whole_line=True, pen_slack=a.pen_slack)
            kdev, kwall, kwdev = [], [], []
            for _ in range(a.steps):
                kref = dec.decode(pages, *geo, whole_line=True)
                kwdev.append(dec.last_ms)
                t = time.perf_counter()
                kgot = dec.decode(pages, *geo, whole_line=True, pen_slack=a.pen_slack)
                kwall.append((time.perf_counter() - t) * 1e3)
                kdev.append(dec.last_ms)
            klaunches = int(dec._lib.focr_decoder_last_launches(dec._h))
        if a.baseline_search:
            for _ in range(a.warmup):
                dec.decode(pages, *geo, baseline_search=a.baseline_search)
            bdev, bwall, bpdev = [], [], []
            for _ in range(a.steps):
                dec.decode(pages, *geo)
                bpdev.append(dec.last_ms)
                t = time.perf_counter()
                bgot = dec.decode(pages, *geo, baseline_search=a.baseline_search)
                bwall.append((time.perf_counter() - t) * 1e3)
                bdev.append(dec.last_ms)
            blaunches = int(dec._lib.focr_decoder_last_launches(dec._h))
            if a.verify:
                bvdev, bvndev = moved_verify(dec, a)
        if a.whole_baseline:
            for _ in range(a.warmup):
                dec.decode(pages, *geo, whole_line=True, whole_baseline=a.whole_baseline)
            cdev, cwall, cwdev = [], [], []
            for _ in range(a.steps):
                cref = dec.decode(pages, *geo, whole_line=True)
                cwdev.append(dec.last_ms)
                t = time.perf_counter()
                cgot = dec.decode(pages, *geo, whole_line=True, whole_baseline=a.whole_baseline)
                cwall.append((time.perf_counter() - t) * 1e3)
                cdev.append(dec.last_ms)
            claunches = int(dec._lib.focr_decoder_last_launches(dec._h))
            if a.verify:
                cvdev, cvndev = moved_verify(dec, a)
        if frac:
            mode = dict(whole_line=True, whole_baseline=a.whole_baseline) if a.whole_baseline else dict(baseline_search=a.baseline_search)
            on = dict(mode, y_frac=frac[0], line_advance_frac=frac[1])
            for _ in range(a.warmup):
                dec.decode(pages, *geo, **on)
            fdev, fwall, fodev = [], [], []
            for _ in range(a.steps):
                foff = dec.decode(pages, *geo, **mode)
                fodev.append(dec.last_ms)
                t = time.perf_counter()
                fgot = dec.decode(pages, *geo, **on)
                fwall.append((time.perf_counter() - t) * 1e3)
                fdev.append(dec.last_ms)
            flaunches = int(dec._lib.focr_decoder_last_launches(dec._h))
        if sizes:
            dec.set_font_candidates([(a.font, t, False, 1.0) for t in sizes])
            for _ in range(a.warmup):
                dec.decode(pages, *geo, font_search=True)
            gdev, gwall, gpdev = [], [], []
            for _ in range(a.steps):
                dec.decode(pages, *geo)
                gpdev.append(dec.last_ms)
                t = time.perf_counter()
                ggot = dec.decode(pages, *geo, font_search=True)
                gwall.append((time.perf_counter() - t) * 1e3)
                gdev.append(dec.last_ms)
            glaunches = int(dec._lib.focr_decoder_last_launches(dec._h))
            if a.verify_text:  # the same lines, line q of a page in font q mod (K + 1)
                mixed = [[q % (len(sizes) + 1) for q in range(len(pg))] for pg in out]
                ydev = []
                for _ in range(a.warmup + a.steps):
                    dec.verify_text(pages, out, geo[0], fonts=mixed)
                    ydev.append(dec.last_verify_text_ms)
                ydev = ydev[a.warmup:]
        if sizes and a.whole_line:
            for _ in range(a.warmup):
                dec.decode(pages, *geo, whole_line=True, font_search=True)
            hdev, hwall, hwdev = [], [], []
            for _ in range(a.steps):
                href = dec.decode(pages, *geo, whole_line=True)
                hwdev.append(dec.last_ms)
                t = time.perf_counter()
                hgot = dec.decode(pages, *geo, whole_line=True, font_search=True)
                hwall.append((time.perf_counter() - t) * 1e3)
                hdev.append(dec.last_ms)
            hlaunches = int(dec._lib.focr_decoder_last_launches(dec._h))
        if a.test_images:
            for _ in range(a.warmup):
                dec.test_images(pages, *geo)
            tdev, twall = [], []
            for _ in range(a.steps):
                t = time.perf_counter()
                dec.test_images(pages, *geo)
                twall.append((time.perf_counter() - t) * 1e3)
                tdev.append(dec.last_test_ms)
            tlaunches = int(dec._lib.focr_decoder_last_test_launches(dec._h))
    n_lines = sum(len(p) for p in out)
    n_chars = sum(len(t) for p in out for _, t in p)
    ms = float(np.median(dev))
    res = {
        "bench": "focr_decode", "pages": a.pages, "page_w": 608, "page_h": 720, "lines": n_lines, "chars": n_chars,
        "font": os.path.splitext(os.path.basename(a.font))[0] + " 13px", "alphabet_len": len(FOCR_DEFAULT_ALPHABET), "launches_per_batch": launches,
        "host_table_ms": round(host_ms, 2), "device_ms_per_batch": round(ms, 4), "device_ms_min": round(float(min(dev)), 4),
        "wall_ms_per_batch": round(float(np.median(wall)), 3), "steps": a.steps, "warmup": a.warmup,
        "pages_per_s": round(a.pages / ms * 1e3, 1), "lines_per_s": round(n_lines / ms * 1e3, 1),
        "page_mpx_per_s": round(a.pages * 608 * 720 / ms / 1e3, 1),
    }
    if a.verify:
        res.update({"verify_device_ms_per_batch": round(float(np.median(vdev)), 4), "verify_launches": vlaunches,
                    "verify_wall_ms": round(float(np.median(vwall)), 3)})
    if a.verify_text:
        xms, xvms = float(np.median(xdev)), float(np.median(xvdev))
        res.update({"vtext_device_ms_per_batch": round(xms, 4), "vtext_device_ms_min": round(float(min(xdev)), 4),
                    "vtext_verify_device_ms": round(xvms, 4), "vtext_over_verify": round(xms / xvms, 3), "vtext_launches": xlaunches,
                    "vtext_wall_ms": round(float(np.median(xwall)), 3), "vtext_equal": bool(xequal)})
        if sizes:
            res.update({"vtext_mixed_fonts": len(sizes) + 1, "vtext_mixed_device_ms": round(float(np.median(ydev)), 4),
                        "vtext_mixed_device_ms_min": round(float(min(ydev)), 4)})
    if a.score_text:
        zms, zpms = {n: float(np.median(v)) for n, v in zdev.items()}, float(np.median(zpdev))
        res.update({"stext_device_ms": {str(n): round(v, 4) for n, v in zms.items()}, "stext_device_ms_min": {str(n): round(float(min(v)), 4) for n, v in zdev.items()},
                    "stext_plain_device_ms": round(zpms, 4), "stext_over_plain": round(zms[0] / zpms, 3),
                    "stext_over_radius0": {str(n): round(zms[n] / zms[0], 2) for n in zms}, "stext_ceiling": {str(n): 2 * n + 1 for n in zms},
                    "stext_launches": zlaunches, "stext_wall_ms": round(float(np.median(zwall)), 3), "stext_equal": bool(zequal)})
    if a.align_text:
        ams, asms = {pr: float(np.median(v)) for pr, v in adev.items()}, float(np.median(asdev))
        name = lambda pr: "%d,%d" % pr  # noqa: E731
        res.update({"atext_device_ms": {name(pr): round(v, 4) for pr, v in ams.items()},
                    "atext_device_ms_min": {name(pr): round(float(min(v)), 4) for pr, v in adev.items()},
                    "atext_score_device_ms": round(asms, 4), "atext_states": {name(pr): 2 * pr[0] + 1 for pr in ams},
                    "atext_over_yardstick": {name(pr): round(v / ((2 * pr[0] + 1) * asms), 3) for pr, v in ams.items()},
                    "atext_start": a_start, "atext_launches": alaunches, "atext_wall_ms": round(float(np.median(awall)), 3), "atext_equal": bool(aequal)})
        with open(os.path.join(ROOT, "profiles", "focr_align_text_bench.json"), "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    if a.learn_text:
        lms, lsms = float(np.median(ldev)), float(np.median(lsdev))
        res.update({"ltext_device_ms": round(lms, 4), "ltext_device_ms_min": round(float(min(ldev)), 4), "ltext_score_device_ms": round(lsms, 4),
                    "ltext_over_score": round(lms / lsms, 2), "ltext_form": "atomic", "ltext_launches": llaunches,
                    "ltext_characters": int(sum(len(t) for pg in out for _, t in pg)), "ltext_used": n_used,
                    "ltext_cells": int((lgot.counts > 0).sum()), "ltext_wall_ms": round(float(np.median(lwall)), 3), "ltext_equal": bool(lequal)})
        with open(os.path.join(ROOT, "profiles", "focr_learn_text_bench.json"), "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    if a.refine_text:
        rms, rsms = {pr: float(np.median(v)) for pr, v in rdev.items()}, {pr: float(np.median(v)) for pr, v in rsdev.items()}
        name = lambda pr: "%d,%d" % pr  # noqa: E731
        flat = lambda got: [g for pg in got for g in pg]  # noqa: E731
        res.update({"rtext_device_ms": {name(pr): round(v, 4) for pr, v in rms.items()},
                    "rtext_device_ms_min": {name(pr): round(float(min(v)), 4) for pr, v in rdev.items()},
                    "rtext_search_device_ms": {name(pr): round(v, 4) for pr, v in rsms.items()},
                    "rtext_over_search": {name(pr): round(rms[pr] / rsms[pr], 3) for pr in rms},
                    "rtext_candidates_per_character": {name(pr): len(FOCR_DEFAULT_ALPHABET) * (2 * pr[0] + 1) for pr in rms},
                    "rtext_lines": len(flat(rgot[(0, 0)])), "rtext_characters": int(sum(len(g.text) for g in flat(rgot[(0, 0)]))),
                    "rtext_lines_cost_in_is_score_text": int(rsame),
                    "rtext_characters_changed": {name(pr): int(sum(g.changed for g in flat(got))) for pr, got in rgot.items()},
                    "rtext_lines_text_changed": {name(pr): int(sum(g.text != t for pg, po in zip(got, out) for g, (_, t) in zip(pg, po))) for pr, got in rgot.items()},
                    "rtext_cost_drop": {name(pr): int(sum(g.cost_in - g.cost for g in flat(got))) for pr, got in rgot.items()},
                    "rtext_launches": rlaunches, "rtext_wall_ms": round(float(np.median(rwall)), 3)})
        with open(os.path.join(ROOT, "profiles", "focr_refine_text_bench.json"), "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
    if a.scores:
        sms, pms = float(np.median(sdev)), float(np.median(pdev))
        res.update({"scores_device_ms_per_batch": round(sms, 4), "scores_device_ms_min": round(float(min(sdev)), 4),
                    "scores_plain_device_ms": round(pms, 4), "scores_over_plain": round(sms / pms, 4), "scores_launches": slaunches,
                    "scores_wall_ms_per_batch": round(float(np.median(swall)), 3)})
    if a.pen_search:
        nms, npms = float(np.median(ndev)), float(np.median(npdev))
        changed = sum(ta != tb for pa, pb in zip(out, found) for (_, ta), (_, tb) in zip(pa, pb))
        res.update({"pen_search": a.pen_search, "search_candidates": 2 * a.pen_search + 1, "search_device_ms_per_batch": round(nms, 4),
                    "search_device_ms_min": round(float(min(ndev)), 4), "search_plain_device_ms": round(npms, 4),
                    "search_over_plain": round(nms / npms, 3), "search_launches": nlaunches,
                    "search_wall_ms_per_batch": round(float(np.median(nwall)), 3), "search_lines_changed": changed})
    if a.whole_line:
        wms, wpms = float(np.median(wdev)), float(np.median(wpdev))
        changed = sum(ta != tb for pa, pb in zip(out, whole) for (_, ta), (_, tb) in zip(pa, pb))
        res.update({"whole_device_ms_per_batch": round(wms, 4), "whole_device_ms_min": round(float(min(wdev)), 4),
                    "whole_plain_device_ms": round(wpms, 4), "whole_over_plain": round(wms / wpms, 3), "whole_launches": wlaunches,
                    "whole_wall_ms_per_batch": round(float(np.median(wwall)), 3), "whole_lines_changed": changed})
    if a.margins:
        mms, mwms = float(np.median(mdev)), float(np.median(mwdev))
        res.update({"margins_device_ms_per_batch": round(mms, 4), "margins_device_ms_min": round(float(min(mdev)), 4),
                    "margins_whole_device_ms": round(mwms, 4), "margins_over_whole": round(mms / mwms, 3), "margins_launches": mlaunches,
                    "margins_wall_ms_per_batch": round(float(np.median(mwall)), 3), "margins_text_equal": bool(mequal)})
    if a.pen_slack:
        kms, kwms = float(np.median(kdev)), float(np.median(kwdev))
        changed = sum(ta != tb for pa, pb in zip(kref[0], kgot[0]) for (_, ta), (_, tb) in zip(pa, pb))
        moved = sum(int(np.count_nonzero(o)) for pg in kgot[3] for o in pg)
        res.update({"pen_slack": a.pen_slack, "slack_device_ms_per_batch": round(kms, 4), "slack_device_ms_min": round(float(min(kdev)), 4),
                    "slack_whole_device_ms": round(kwms, 4), "slack_over_whole": round(kms / kwms, 3), "slack_launches": klaunches,
                    "slack_wall_ms_per_batch": round(float(np.median(kwall)), 3), "slack_lines_changed": changed, "slack_chars_offset": moved})
    if a.baseline_search:
        bms, bpms = float(np.median(bdev)), float(np.median(bpdev))
        changed = sum(ta != tb for pa, pb in zip(out, bgot[0]) for (_, ta), (_, tb) in zip(pa, pb))
        moved = sum(q != 0 for pg in bgot[1] for q in pg)
        res.update({"baseline_search": a.baseline_search, "y_bits": a.y_bits, "base_candidates": 2 * a.baseline_search + 1,
                    "base_ceiling": 2 * a.baseline_search + 2, "base_device_ms_per_batch": round(bms, 4),
                    "base_device_ms_min": round(float(min(bdev)), 4), "base_plain_device_ms": round(bpms, 4),
                    "base_over_plain": round(bms / bpms, 3), "base_launches": blaunches,
                    "base_wall_ms_per_batch": round(float(np.median(bwall)), 3), "base_lines_changed": changed, "base_lines_offset": moved})
        if a.verify:
            res.update({"base_verify_device_ms": round(float(np.median(bvdev)), 4), "base_verify_sums_device_ms": round(float(np.median(bvndev)), 4)})
    if a.whole_baseline:
        cms, cwms = float(np.median(cdev)), float(np.median(cwdev))
        changed = sum(ta != tb for pa, pb in zip(cref[0], cgot[0]) for (_, ta), (_, tb) in zip(pa, pb))
        moved = sum(q != 0 for pg in cgot[3] for q in pg)
        res.update({"whole_baseline": a.whole_baseline, "y_bits": a.y_bits, "wbase_candidates": 2 * a.whole_baseline + 1,
                    "wbase_ceiling": 2 * a.whole_baseline + 1, "wbase_device_ms_per_batch": round(cms, 4),
                    "wbase_device_ms_min": round(float(min(cdev)), 4), "wbase_whole_device_ms": round(cwms, 4),
                    "wbase_over_whole": round(cms / cwms, 3), "wbase_launches": claunches,
                    "wbase_wall_ms_per_batch": round(float(np.median(cwall)), 3), "wbase_lines_changed": changed, "wbase_lines_offset": moved})
        if a.verify:
            res.update({"wbase_verify_device_ms": round(float(np.median(cvdev)), 4), "wbase_verify_sums_device_ms": round(float(np.median(cvndev)), 4)})
    if frac:
        fms, foms = float(np.median(fdev)), float(np.median(fodev))
        changed = sum(ta != tb for pa, pb in zip(foff[0], fgot[0]) for (_, ta), (_, tb) in zip(pa, pb))
        res.update({"line_frac": list(frac), "frac_mode": "whole_baseline" if a.whole_baseline else "baseline_search",
                    "frac_radius": a.whole_baseline or a.baseline_search, "y_bits": a.y_bits, "frac_device_ms_per_batch": round(fms, 4),
                    "frac_device_ms_min": round(float(min(fdev)), 4), "frac_off_device_ms": round(foms, 4), "frac_over_off": round(fms / foms, 4),
                    "frac_launches": flaunches, "frac_wall_ms_per_batch": round(float(np.median(fwall)), 3),
                    "frac_lines": sum(len(pg) for pg in fgot[0]), "frac_off_lines": sum(len(pg) for pg in foff[0]), "frac_lines_changed": changed})
    if sizes:
        gms, gpms = float(np.median(gdev)), float(np.median(gpdev))
        changed = sum(ta != tb for pa, pb in zip(out, ggot[0]) for (_, ta), (_, tb) in zip(pa, pb))
        other = sum(k != 0 for pg in ggot[1] for k in pg)
        res.update({"font_candidate_sizes": sizes, "fonts_candidates": len(sizes) + 1, "fonts_ceiling": len(sizes) + 2,
                    "fonts_device_ms_per_batch": round(gms, 4), "fonts_device_ms_min": round(float(min(gdev)), 4),
                    "fonts_plain_device_ms": round(gpms, 4), "fonts_over_plain": round(gms / gpms, 3), "fonts_launches": glaunches,
                    "fonts_wall_ms_per_batch": round(float(np.median(gwall)), 3), "fonts_lines_changed": changed, "fonts_lines_other": other})
    if sizes and a.whole_line:
        hms, hwms = float(np.median(hdev)), float(np.median(hwdev))
        changed = sum(ta != tb for pa, pb in zip(href[0], hgot[0]) for (_, ta), (_, tb) in zip(pa, pb))
        other = sum(k != 0 for pg in hgot[3] for k in pg)
        res.update({"wfonts_candidates": len(sizes) + 1, "wfonts_ceiling": len(sizes) + 1, "wfonts_device_ms_per_batch": round(hms, 4),
                    "wfonts_device_ms_min": round(float(min(hdev)), 4), "wfonts_whole_device_ms": round(hwms, 4),
                    "wfonts_over_whole": round(hms / hwms, 3), "wfonts_launches": hlaunches,
                    "wfonts_wall_ms_per_batch": round(float(np.median(hwall)), 3), "wfonts_lines_changed": changed, "wfonts_lines_other": other})
    if a.test_images:
        tms = float(np.median(tdev))
        res.update({"test_device_ms_per_batch": round(tms, 4), "test_launches": tlaunches, "test_wall_ms": round(float(np.median(twall)), 3),
                    "test_write_gb_per_s": round(2 * a.pages * 608 * 720 * 4 / tms / 1e6, 1)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
