/*
 * focr_decode.h — C ABI of the `focr` line decoder (the upstream package's default binary, src/main.rs).
 *
 * The reference decodes a text line by rasterising every alphabet glyph at the current pen position with FreeType,
 * scoring it by the sum of squared differences against the whole line canvas, taking the first minimum and moving the
 * pen by that glyph's advance (decode_line, src/main.rs:112-181).  The 26.6 translation FreeType receives is
 * trunc(t * 64), so a glyph has at most 64 distinct sub-pixel renderings and a whole-pixel shift only moves the bitmap:
 * the decode font below holds those 64 phases per glyph, built once on the host, and the device does an exact integer
 * argmin with them.
 *
 * libfocr_raster.so : focr_raster_glyph, focr_glyph_metrics, focr_render_text, focr_decode_font_build/build_y/free,
 *                     focr_verify_font_build/free (FreeType)
 * libfocr_hip.so    : focr_decoder_* (gfx950), including the device verify of a run (--verify) and the test images
 *                     (--test)
 */
#ifndef FOCR_DECODE_H
#define FOCR_DECODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- host: rasterisation (libfocr_raster.so) --------------------------------------------------------------------- */

/* font-kit's rasterize_glyph for a pure translation (tx, ty) onto a zero-or-not caller canvas of w x h bytes (A8,
 * row-major): FreeType delta = (trunc(tx * 64), -trunc(ty * 64)), the bitmap copied (not blended) at
 * (bitmap_left, -bitmap_top), clipped to the canvas.  The face is cached per thread and font path.  Returns 0, or
 * non-zero with a message in err (no glyph for the code point, unreadable font). */
int focr_raster_glyph(const char *font_path, float text_size, int hinting, uint32_t codepoint, float tx, float ty,
                      uint8_t *canvas, size_t w, size_t h, char *err, size_t errlen);

/* The glyph queries decode_line makes: font.advance(gid).x in font units, units_per_em, and
 * raster_bounds(gid, size, identity) as (origin x, origin y, lower-right x, lower-right y) in px. */
int focr_glyph_metrics(const char *font_path, float text_size, uint32_t codepoint, float *advance, uint32_t *units_per_em,
                       int32_t bounds[4], char *err, size_t errlen);

/* render() (src/main.rs:40-85) of a whole string: pen positions advance by font.advance / upem * size * kerning (f32),
 * the canvas is the rounded union of every glyph's raster bounds at its pen position, each glyph is copied in turn at
 * -bounds.origin + pos.  *canvas is malloc'ed (w x h A8 bytes, 255 = ink; free with free()). */
int focr_render_text(const char *font_path, float text_size, int hinting, float kerning, const uint32_t *text, size_t n,
                     uint8_t **canvas, size_t *w, size_t *h, char *err, size_t errlen);

/* ---- host: the decode font (libfocr_raster.so) ------------------------------------------------------------------- */

enum { FOCR_DECODE_PHASES = 64 };

/* One alphabet glyph.  Phase p is the rendering at 26.6 delta x = p (and the font's fixed delta y): a box_h x stride
 * byte bitmap at bitmaps + offset + p * box_h * stride, whose top-left pixel lands on the canvas at
 * (shift + off_x[p], off_y[p]) for a delta x of 64 * shift + p.  All 64 phases share the box size. */
typedef struct focr_decode_glyph {
    uint32_t codepoint;
    float increment;                         /* pen increment in px: advance / upem * size * kerning, f32, left to right */
    uint32_t box_w, box_h, stride;           /* box in px; stride = box_w rounded up to 4 bytes */
    uint64_t offset;                         /* byte offset of phase 0 in bitmaps */
    int32_t off_x[FOCR_DECODE_PHASES];
    int32_t off_y[FOCR_DECODE_PHASES];
} focr_decode_glyph_t;

typedef struct focr_decode_font {
    focr_decode_glyph_t *glyphs;             /* alphabet order */
    size_t n_glyphs;
    uint8_t *bitmaps;
    size_t bitmaps_len;
    float origin_x, origin_y;                /* -bbox.origin, bbox = union of raster_bounds(identity) with the empty rect at 0 */
    float text_size, kerning;
    int hinting;
    float min_increment;
} focr_decode_font_t;

/* Build the decode font for an alphabet (code points, in order).  Fails with a message if a code point has no glyph,
 * if kerning <= 0 or if any increment is <= 0 (the reference loops forever there), or if a glyph's box is too large for
 * the device's 32-bit scores.  Free with focr_decode_font_free. */
int focr_decode_font_build(const char *font_path, float text_size, int hinting, float kerning, const uint32_t *alphabet,
                           size_t n_alphabet, focr_decode_font_t *out, char *err, size_t errlen);
void focr_decode_font_free(focr_decode_font_t *font);

/* ---- host: the verify table (libfocr_raster.so) ------------------------------------------------------------------ */

/* What render() needs beyond the decode font, for one alphabet glyph.  box is raster_bounds at the identity before
 * round_out: (nox, noy, nox + width, noy + height) in px, each an f32 as the host computes it, so that raster_bounds at
 * a translation (tx, ty) is round_out(box + (tx, ty)) in f32.  rect_* is phase p's true FreeType bitmap inside the
 * decode font's box (box-relative, zeros included); render() copies exactly that rectangle and nothing of the padding. */
typedef struct focr_verify_glyph {
    uint32_t codepoint;
    float increment;                         /* equal to the decode font's, bitwise */
    float box[4];
    uint32_t rect_x[FOCR_DECODE_PHASES], rect_y[FOCR_DECODE_PHASES];
    uint32_t rect_w[FOCR_DECODE_PHASES], rect_h[FOCR_DECODE_PHASES];
} focr_verify_glyph_t;

typedef struct focr_verify_font {
    focr_verify_glyph_t *glyphs;             /* alphabet order */
    size_t n_glyphs;
    float origin_y;                          /* the vertical translation the decode font's phases are rendered at */
    float text_size, kerning;
    int hinting;
} focr_verify_font_t;

/* Build the verify table for the same arguments as focr_decode_font_build (and with the same refusals).  Free with
 * focr_verify_font_free. */
int focr_verify_font_build(const char *font_path, float text_size, int hinting, float kerning, const uint32_t *alphabet,
                           size_t n_alphabet, focr_verify_font_t *out, char *err, size_t errlen);
void focr_verify_font_free(focr_verify_font_t *font);

/* ---- device: the decoder (libfocr_hip.so) ------------------------------------------------------------------------ */

typedef struct focr_decoder focr_decoder_t;

/* One decoded, non-blank line: page index in the batch, crop y, and n_chars alphabet indices at chars + first. */
typedef struct focr_decoded_line {
    uint32_t page, y;
    uint64_t first;
    uint32_t n_chars;
    uint32_t pad;
} focr_decoded_line_t;

/* A decoder on one device.  Non-zero (message in focr_decoder_last_error(NULL)) if there is no usable device: there is
 * no CPU fallback. */
int focr_decoder_create(int device, focr_decoder_t **out);
void focr_decoder_destroy(focr_decoder_t *dec);
/* The last error of dec, or of the calling thread's last failed create when dec is NULL. */
const char *focr_decoder_last_error(const focr_decoder_t *dec);
/* Upload a decode font (the decoder keeps its own copy). */
int focr_decoder_set_font(focr_decoder_t *dec, const focr_decode_font_t *font);
/* Decode a batch of n_pages equal-size luma pages (page_h rows of page_w bytes, 255 = paper, pages back to back) from
 * host memory, or from device memory of the decoder's device when on_device != 0 (the caller orders its writes before
 * the call).  Line geometry as the reference's DecodeOptions.  Runs a fixed number of launches and returns when the
 * results are on the host.  line_advance == 0 with a non-empty first crop is refused (the reference never ends). */
int focr_decoder_run(focr_decoder_t *dec, const uint8_t *pages, int on_device, size_t n_pages, size_t page_w, size_t page_h,
                     uint32_t x_start, uint32_t y_start, uint32_t width, uint32_t line_height, uint32_t line_advance);
/* Results of the last run: number of lines, total characters, and a copy into caller arrays (lines[n_lines],
 * chars[n_chars], in (page, line) order). */
size_t focr_decoder_n_lines(const focr_decoder_t *dec);
size_t focr_decoder_n_chars(const focr_decoder_t *dec);
int focr_decoder_get(const focr_decoder_t *dec, focr_decoded_line_t *lines, uint16_t *chars);
/* Device time of the last run's kernels (prepass, compaction, decode) in ms, from events. */
float focr_decoder_last_ms(const focr_decoder_t *dec);
/* Kernel launches of the last run (constant per batch). */
uint32_t focr_decoder_last_launches(const focr_decoder_t *dec);

/* ---- device: per-character scores of a run (an extension: the reference prints the text only) -------------------- */

/* What the argmin knew about one decoded character.  score is the reference's score of the chosen glyph (score_glyph,
 * src/main.rs:87-110: the sum over the whole line canvas of (r - c)^2); runner is the alphabet index of the glyph the
 * argmin would have taken next, the lowest (score, index) among all the others, and runner_score its score.  Glyphs
 * with identical bitmaps tie: runner_score == score.  A one-glyph alphabet has no runner: 0xFFFF and INT64_MAX. */
typedef struct focr_char_score {
    int64_t score, runner_score;
    uint16_t runner;
    uint16_t pad[3];
} focr_char_score_t;

/* Switch the scores of later runs on or off (off when the decoder is created; a state of the decoder, not of the
 * font).  With scores on a run takes the same launches and returns the same lines, verify and test images. */
int focr_decoder_set_scores(focr_decoder_t *dec, int on);
/* The scores of the last run, in the order of focr_decoder_get: scores[n_chars], and line_base[n_lines], each line's sum
 * of r^2 over its crop (the part of a score every candidate shares: score - line_base is the footprint term the
 * device compares).  Either may be NULL.  Fails with a message unless the last successful run had scores on. */
int focr_decoder_get_scores(const focr_decoder_t *dec, focr_char_score_t *scores, uint64_t *line_base);

/* ---- device: pen search (an extension: the reference's pen is never corrected) ------------------------------------ */

/* The reference moves the pen by the chosen glyph's increment and never corrects it, so text whose advance is not
 * quite the font's, or whose glyphs were snapped to the pixel grid, loses the line.  With a search radius N (in 1/64 px,
 * 0 <= N <= FOCR_PEN_SEARCH_MAX) every step takes the argmin over (glyph i, offset j), j in -N ..= N, instead of over the
 * glyphs alone.  All of it is exact:
 *   - the candidate's pen is p_j = pos + (float)j * 0.015625f, one f32 add (pos is the f32 pen, 0 at the line's start);
 *   - a candidate whose origin_x + p_j (an f32 add) is negative is dropped;
 *   - otherwise its score is the reference's score_glyph with the pen at p_j: delta trunc((origin_x + p_j) * 64), phase
 *     delta & 63, whole-pixel shift delta >> 6;
 *   - the step takes the lowest (score, rank(j), i) with rank(0) = 0, rank(-1) = 1, rank(+1) = 2, rank(-2) = 3, ...: on
 *     a tie the offset nearest 0 wins, negative before positive, then the first glyph in alphabet order; a blank glyph
 *     scores the same at every offset and so takes j = 0;
 *   - the pen becomes p_j + increment[i], one f32 add on the winning candidate's pen: the offset is carried forward.
 * The loop still runs while pos < width.  N = 0 is the plain decoder, choice for choice and launch for launch.
 * With scores on (focr_decoder_set_scores), score is the chosen candidate's, and runner / runner_score are the best
 * candidate, at any offset, of another glyph: the other offsets of the chosen glyph never count. */
enum { FOCR_PEN_SEARCH_MAX = 64 };
/* Set the search radius of later runs (0 when the decoder is created; a state of the decoder, not of the font).  n above
 * FOCR_PEN_SEARCH_MAX is refused.  focr_decoder_run refuses, with a message, a radius of more than half the font's
 * smallest increment (n / 64 > min_increment / 2): the pen could crawl. */
int focr_decoder_set_pen_search(focr_decoder_t *dec, uint32_t n);
/* The chosen offset j of every character of the last run, in the order of focr_decoder_get: offsets[n_chars], all zero
 * after a run with the search off (unless it was a whole-line run with pen slack, focr_decoder_set_whole_slack, whose
 * offsets these then are). */
int focr_decoder_get_offsets(const focr_decoder_t *dec, int8_t *offsets);

/* ---- device: whole-line decode (an extension: the reference's pen loop is greedy) ---------------------------------- */

/* The reference takes, at every pen position, the glyph with the lowest score, and that score is not normalised by the
 * glyph's area: in a proportional font a wide glyph that covers two narrow ones ("rn" -> "m", "cl" -> "d") collects more
 * matching ink than either and wins, and the pen is lost from then on.  The objective behind the loop is the whole
 * line's squared error, sum over the canvas of (r - render(text))^2 = sum r^2 + the sum over the characters of the
 * footprint term the decoder already compares (exact while footprints do not overlap; the true text makes it zero).
 * With the mode on, a run minimises that sum by a dynamic programme over pens on FreeType's own 1/64 px grid:
 *   - inc64[i] = (int)rintf(increment[i] * 64);
 *   - states are pens s in 1/64 px, starting at s = 0;
 *   - the rendering at state s is the plain decoder's at pos = s / 64: delta 64 * origin_x + s, phase delta & 63, whole-
 *     pixel shift delta >> 6;
 *   - term(i, s) is the int32 footprint term of glyph i there: the sum over the glyph's bitmap, clipped to the crop, of
 *     c * (c - 2 r), the plain decoder's score less the crop's sum of r^2;
 *   - cost[0] = 0; for t > 0, cost[t] is the minimum of cost[s] + term(i, s) over glyphs i and reachable states
 *     s = t - inc64[i] with 0 <= s < 64 * width (the reference's loop runs while pos < width);
 *   - the glyph remembered for t is the one with the lowest (cost, i);
 *   - the line ends in the reachable state t >= 64 * width with the lowest (cost[t], t);
 *   - the text is read back along the remembered glyphs.
 * A run returns, beside the lines of focr_decoder_get, each character's pen s and each line's final cost, the sum of its
 * characters' terms: the line's squared error is line_base + cost.  Prepass and compaction are the plain run's and the
 * launch count stays 3.  focr_decoder_run refuses, with a message:
 *   - an origin_x that is not a whole number >= 0;
 *   - any inc64 < 1;
 *   - 64 * width + max inc64 >= 2^24 (pens must stay exact in f32);
 *   - ceil(64 * width / min inc64) * T >= 2^47, T = max stride * box_h * 2 * 255^2 (set_font's own bound on a term): a
 *     packed cost could overflow; the first factor is the exact bound on a line's characters;
 *   - a widest advance so large that the device's cost ring does not fit in LDS (min(min inc64, 512) + max inc64 > 4096);
 *   - scores on (a runner-up has no definition under a dynamic programme yet);
 *   - a pen search radius (the pen loop's search; the programme over offsets as well is focr_decoder_set_whole_slack).
 * With the mode off a run launches and returns what it did before the mode existed. */
/* Switch the whole-line decode of later runs on or off (off when the decoder is created; a state of the decoder, not of
 * the font). */
int focr_decoder_set_whole_line(focr_decoder_t *dec, int on);
/* The pens of the last run, in the order of focr_decoder_get: pens[n_chars], each character's state s (its pen is
 * s / 64 px), and line_cost[n_lines].  Either may be NULL.  Fails with a message unless the last successful run was a
 * whole-line run. */
int focr_decoder_get_pens(const focr_decoder_t *dec, uint32_t *pens, int64_t *line_cost);
/* Debug: at most `grid` workgroups for later whole-line runs (0: the decoder's own choice), so that a test can make one
 * workgroup take several lines. */
int focr_decoder_debug_set_whole_grid(focr_decoder_t *dec, uint32_t grid);

/* ---- device: per-character margins of a whole-line run (an extension of the extension) ----------------------------- */

/* Which characters of a whole line to doubt.  Scores stay refused beside the whole-line decode (the plain decoder's
 * runner-up is the second glyph at one pen, and the programme has no one pen), but a runner-up does have an exact
 * definition under the programme.  Take a point of the line: every complete pen path has exactly one character whose span
 * [start pen, end pen) contains it, so the paths split by that covering character, and the best whole line that reads a
 * different glyph over the middle of a decoded character is a minimum over covering edges.  In the names of the
 * whole-line definition above (states s in 1/64 px, term(i, s), inc64, n_live = 64 * width):
 *   - F[t] is the forward cost the programme already has (cost[t] above); F[0] = 0; unreachable states carry no cost;
 *   - B[t] = 0 for every t >= n_live; for s < n_live, B[s] is the minimum over glyphs i of term(i, s) + B[s + inc64[i]];
 *     it follows that B[0] equals the line's cost;
 *   - a decoded character k has glyph i_k, pen s_k and midpoint m_k = s_k + (inc64[i_k] >> 1);
 *   - an edge (s, i) covers m_k when s is reachable and s <= m_k < s + inc64[i];
 *   - its through-cost is T(s, i) = F[s] + term(i, s) + B[s + inc64[i]], the cost of the best complete path that uses it.
 * Per character a margins run returns:
 *   - term   = term(i_k, s_k); the terms of a line sum to its cost;
 *   - runner = the glyph i != i_k with the lowest (T, i) over the edges that cover m_k.  Edges of the chosen glyph at
 *              other pens never count, as with the pen search's runner.  The runner's pen is not reported;
 *   - margin = that T less the line's cost: >= 0, and 0 for glyphs with identical bitmaps and advances;
 *   - runner = 0xFFFF and margin = -1 when there is no such edge (a one-glyph alphabet).
 * |T| stays below the bound a whole-line run already checks (characters per line times T < 2^47): it is the cost of a
 * complete path.  Forbidding glyph i_k at every state that covers m_k and decoding the line again costs exactly
 * cost + margin.  The text, pens, costs, verify and launch count (3) of the run are the whole-line run's. */
typedef struct focr_char_margin {
    int32_t term;
    uint16_t runner;
    uint16_t pad;
    int64_t margin;
} focr_char_margin_t;

/* Switch the margins of later whole-line runs on or off (off when the decoder is created; a state of the decoder, not
 * of the font).  focr_decoder_run refuses, before anything is launched and with a message that names both, margins on
 * with the whole-line decode off.  With margins off a whole-line run launches what it did before they existed. */
int focr_decoder_set_whole_margins(focr_decoder_t *dec, int on);
/* The margins of the last run, in the order of focr_decoder_get and focr_decoder_get_pens: out[n_chars] (may be NULL).
 * Fails with a message unless the last successful run was a whole-line run with margins on. */
int focr_decoder_get_margins(const focr_decoder_t *dec, focr_char_margin_t *out);

/* ---- device: pen slack of a whole-line run (an extension of the extension) ------------------------------------------- */

/* The whole-line programme only allows pens that are exact sums of inc64, so it reads pages whose glyphs sit exactly
 * where this FreeType build puts them.  Pages snapped to the pixel grid, or set with a slightly different advance, do
 * not.  The pen loop's remedy is the pen search; this is the programme's.  In the names of the whole-line definition
 * (states in 1/64 px, term(i, s), inc64, n_live = 64 * width), with a slack radius N (0 <= N <= FOCR_PEN_SEARCH_MAX) a
 * step moves the pen by an offset j, -N <= j <= N, before the glyph is rendered, and the offset is carried forward, as
 * in the pen search:
 *   - cost[0] = 0; every other state starts unreachable;
 *   - for a render pen p, 0 <= p < n_live: G[p] is the lowest (cost[p - j], rank(j)) over j in -N ..= N for which
 *     0 <= p - j < n_live and p - j is reachable; rank is the pen search's (0, -1, +1, -2, ...); off[p] is that j; a
 *     pen p with no such j renders nothing;
 *   - for t > 0: cost[t] is the minimum over glyphs i of G[t - inc64[i]].cost + term(i, t - inc64[i]); the glyph
 *     remembered for t is the one with the lowest (cost, i);
 *   - the line ends in the reachable t >= n_live with the lowest (cost[t], t);
 *   - read-back from t: i = glyph[t], p = t - inc64[i], j = off[p]; emit character i with pen p and offset j, then
 *     continue from t = p - j.
 * A run returns, per character, the alphabet index, the render pen p (focr_decoder_get_pens) and j
 * (focr_decoder_get_offsets), so focr_decoder_verify draws every character where it was decoded.  pens[0] ==
 * offsets[0], and pens[q + 1] - offsets[q + 1] == pens[q] + inc64[idx[q]].  A line's cost is the sum of its terms: an
 * offset costs nothing, and on a tie the offset nearest 0 wins, so a blank stretch takes none.  N = 0 is the plain
 * whole-line run: the same text, pens, costs and launches.  With N > 0 prepass and compaction are still the plain run's
 * and the launch count stays 3.  focr_decoder_run refuses, before anything is launched and each with its own message:
 *   - slack on with the whole-line decode off (the message names both setters);
 *   - slack on with margins on (margins under slack are a later step; the message names both setters);
 *   - 2 * N > min inc64: the pen could crawl (the pen search's rule);
 *   - a cost ring that does not fit in LDS: min(min inc64 - N, 512) + 2 * N + max inc64 > 4096;
 *   - ceil(64 * width / (min inc64 - N)) * T >= 2^47: a step gains at least min inc64 - N, so the first factor is now the
 *     exact bound on a line's characters, and a packed cost could overflow;
 * and what a whole-line run refuses anyway. */
/* Set the slack radius of later whole-line runs (0 when the decoder is created; a state of the decoder, not of the
 * font).  n above FOCR_PEN_SEARCH_MAX is refused here. */
int focr_decoder_set_whole_slack(focr_decoder_t *dec, uint32_t n);

/* ---- baseline search (an extension: the reference renders every glyph at one vertical position) ------------------- */

/* The reference renders every glyph at the crop's top plus origin_y, and the crop's y is a whole pixel: a line whose
 * baseline sits elsewhere (a y that is a pixel off, lines a renderer snapped one by one, a leading that is not a whole
 * number of pixels) loses its text.  The pen search corrects the pen in x; this is its counterpart in y, per line.  With
 * y_bits B (0 <= B <= FOCR_BASELINE_Y_BITS_MAX) and a radius N (0 <= N <= FOCR_BASELINE_MAX, in steps of 2^-B px) a run
 * decodes every line once per candidate q in -N ..= N and keeps one of them.  All of it is exact:
 *   - candidate q renders every glyph at the vertical translation ty_q = origin_y + q * 2^-B (exact in f32): FreeType
 *     receives delta y = -trunc(ty_q * 64);
 *   - a candidate with ty_q < 0 is dropped (q = 0 never is);
 *   - origin_y must be a whole number >= 0 (the font builder's always is; the run refuses otherwise), so that rendering
 *     is y-phase v = q & (2^B - 1) of the font (focr_decode_font_build_y) moved down by d = q >> B rows (floor; up for
 *     d < 0);
 *   - under candidate q the line is decoded by the plain pen loop, unchanged: the f32 pen, delta x =
 *     trunc((origin_x + pos) * 64), the first minimum over the glyphs, while pos < width;
 *   - bitmaps are clipped to the crop on all four sides: rows that d pushes above row 0 or below the crop's last row do
 *     not count;
 *   - cost_q is the int64 sum of the chosen glyphs' int32 footprint terms (score less line_base); line_base + cost_q is
 *     the line's squared error while footprints do not overlap;
 *   - the line is the candidate with the lowest (cost_q, rank(q)), rank as in the pen search (0, -1, +1, -2, ...): on a
 *     tie the offset nearest 0 wins, so a line no glyph reaches takes q = 0.
 * A run returns that candidate's text, and per line its q and its cost (focr_decoder_get_baselines); q * 2^-B px is how
 * far below the crop's own baseline the line sits.  N = 0 is the plain decoder, choice for choice and launch for launch,
 * whatever fonts are uploaded.  With N > 0 prepass and compaction are the plain run's and the launch count stays 3.
 * focr_decoder_run refuses, before anything is launched and each with a message that names both setters, N > 0 with
 * scores, a pen search, the whole-line decode, margins or a pen slack; it also refuses N > 0 with B > 0 unless y-phase
 * fonts of that B are uploaded (focr_decoder_set_baseline_fonts), and an origin_y that is not a whole number >= 0.
 * What it does not cure: a leading that drifts past the radius down a page (every line searches around the same crop
 * grid; the offset is not carried from line to line): a leading that is known goes into focr_decoder_set_line_frac. */
enum { FOCR_BASELINE_MAX = 32, FOCR_BASELINE_Y_BITS_MAX = 3 };

/* host (libfocr_raster.so): the 1 << y_bits y-phase fonts of an alphabet.  out[v] is what focr_decode_font_build
 * produces with the vertical translation origin_y + v * 2^-y_bits in origin_y's place: all fonts share glyph order,
 * increments (bitwise), origin (origin_y stays the line's), size, kerning and hinting; out[0] equals the plain build
 * byte for byte; box sizes may differ between v; each font passes the build's own int32 bound.  Same refusals as
 * focr_decode_font_build, and y_bits > FOCR_BASELINE_Y_BITS_MAX.  Free each font with focr_decode_font_free. */
int focr_decode_font_build_y(const char *font_path, float text_size, int hinting, float kerning, const uint32_t *alphabet,
                             size_t n_alphabet, uint32_t y_bits, focr_decode_font_t *out, char *err, size_t errlen);

/* Upload the y-phase fonts fonts[0 .. 1 << y_bits) of the current decode font (the decoder keeps its own copy of the
 * phases v >= 1).  Refused unless every one matches the decode font: glyph count, code points, increments (bitwise),
 * origin, size, kerning and hinting, and fonts[0]'s glyph table and bitmaps byte for byte.  focr_decoder_set_font drops
 * them, and so does a failed upload. */
int focr_decoder_set_baseline_fonts(focr_decoder_t *dec, const focr_decode_font_t *fonts, uint32_t y_bits);
/* Set y_bits and the radius of later runs (0, 0 when the decoder is created; a state of the decoder, not of the font).
 * y_bits above FOCR_BASELINE_Y_BITS_MAX and n above FOCR_BASELINE_MAX are refused here. */
int focr_decoder_set_baseline_search(focr_decoder_t *dec, uint32_t y_bits, uint32_t n);
/* The chosen q and cost of every line of the last run, in the order of focr_decoder_get: q[n_lines], cost[n_lines].
 * Either may be NULL.  Fails with a message unless the last successful run searched (n > 0), as a baseline search or as
 * a whole-line run under baseline candidates (focr_decoder_set_whole_baseline). */
int focr_decoder_get_baselines(const focr_decoder_t *dec, int8_t *q, int64_t *cost);
/* Debug: at most `grid` workgroups for later baseline runs (0: one per line slot), so that a test can make one workgroup
 * take several lines. */
int focr_decoder_debug_set_baseline_grid(focr_decoder_t *dec, uint32_t grid);

/* ---- device: baseline candidates of a whole-line run (the two extensions together) ---------------------------------- */

/* The baseline search runs the greedy pen loop under every candidate, so it finds the offset of a proportional line and
 * still loses its text, and on such lines the loop's own cost often picks a wrong offset as well; the whole-line decode
 * reads proportional text but renders at the crop's top plus origin_y only.  With y_bits B and a radius N (the baseline
 * search's limits) a whole-line run decodes every line by the dynamic programme once per vertical candidate and keeps the
 * candidate whose whole line costs least.  Candidates, y-phases, the row shift d, the four-sided clipping, dropped
 * candidates and rank are the baseline search's; states, inc64, cost, the end state and the read-back are the whole-line
 * decode's:
 *   - candidate q in -N ..= N renders every glyph at ty_q = origin_y + q * 2^-B: y-phase v = q & (2^B - 1) of the fonts
 *     of focr_decoder_set_baseline_fonts, every glyph moved down by d = q >> B rows (floor), bitmaps clipped to the crop
 *     on all four sides;
 *   - a candidate with ty_q < 0 is dropped (q = 0 never is);
 *   - term_q(i, s) is the int32 footprint term of glyph i of y-phase v at state s under that move; inc64 is the same for
 *     every candidate (the fonts share increments bitwise);
 *   - under candidate q the line is decoded by the whole-line programme exactly as defined above, with term_q in term's
 *     place; cost_q is its end state's cost;
 *   - the line is the candidate with the lowest (cost_q, rank(q)), rank 0, -1, +1, -2, ...: on a tie the offset nearest 0
 *     wins.
 * A run returns that candidate's text, pens and cost: focr_decoder_get_pens returns the pens and the line's cost, and
 * focr_decoder_get_baselines its q and the same cost.  N = 0 is the plain whole-line run: the same text, pens, costs and
 * launches (and focr_decoder_get_baselines fails after it).  With N > 0 prepass and compaction are unchanged and the
 * launch count stays 3.  focr_decoder_run refuses N > 0, before anything is launched and each with its own message that
 * names the setters involved:
 *   - with the whole-line decode off;
 *   - with margins on;
 *   - with a pen slack;
 *   - with B > 0 unless y-phase fonts of that B are uploaded (focr_decoder_set_baseline_fonts);
 *   - with an origin_y that is not a whole number >= 0;
 * and whatever a whole-line run refuses anyway; focr_decoder_set_baseline_search with n > 0 stays refused beside the
 * whole-line decode.  The whole-line bound ceil(64 * width / min inc64) * T < 2^47 takes T over the glyph boxes of every
 * uploaded y-phase as well, because box sizes differ between v.  focr_decoder_verify then combines its two rules: every
 * character at pos = s / 64 of its returned pen, the line's canvas moved by (q + (1 << B >> 1)) >> B rows and clipped at
 * the page's top and bottom.  What it does not cure: a leading that drifts past the radius, and lines that are off the
 * 1/64 px grid in x as well (those need the pen slack under every candidate, a later step). */
/* Set y_bits and the radius of later whole-line runs (0, 0 when the decoder is created; a state of the decoder, not of
 * the font).  y_bits above FOCR_BASELINE_Y_BITS_MAX and n above FOCR_BASELINE_MAX are refused here. */
int focr_decoder_set_whole_baseline(focr_decoder_t *dec, uint32_t y_bits, uint32_t n);

/* ---- device: a fractional line grid for the two baseline modes (an extension of the extensions) ---------------------- */

/* line_advance is a whole number of pixels, in the reference and here, but the leading of a rendered page seldom is (13 px
 * text at 1.2 line spacing: 15.6 px), so down such a page the lines drift off the crop grid by the leading's fraction per
 * line and past any radius after a few.  The two baseline modes (focr_decoder_set_baseline_search and
 * focr_decoder_set_whole_baseline) are the modes with sub-pixel vertical phases; with a fractional grid they search around
 * where each line is, not around the whole-pixel grid.  y_frac and advance_frac are the sub-pixel parts of y_start and
 * line_advance in 1/64 px, the unit of pens and of FreeType.  All of it is exact integer arithmetic:
 *   - L = 64 * line_advance + advance_frac; slot i of a page has its top at Y_i = 64 * y_start + y_frac + i * L (64 bits);
 *   - its crop starts at row yc_i = Y_i >> 6, clamped as image::crop_imm clamps it, and has
 *     h_i = min(line_height, page_h - yc_i) rows; f_i = Y_i & 63 is the part of a pixel the line sits below its crop's top;
 *   - a page has the slots i with yc_i < page_h: n_slots = ceil((64 * page_h - Y_0) / L) when y_start < page_h and
 *     line_height > 0, else 0; the blank test, the compaction, the (page, line) order and focr_decoded_line_t::y = yc_i
 *     follow that grid;
 *   - the line's centre is c_i = ((f_i << B) + 32) >> 6, in steps of 2^-B px, halves up: 0 <= c_i <= 2^B (a centre of 2^B is
 *     one whole row, which q >> B handles);
 *   - the candidates of line i are q = c_i + rank_offset(rank), rank in 0 ..= 2 N, in rank order (offsets 0, -1, +1, -2, ...);
 *     everything else is the mode's own: y-phase q & (2^B - 1), every box moved down by q >> B rows, the four-sided clipping,
 *     and a candidate with ty_q = origin_y + q * 2^-B < 0 dropped (rank 0 never is: c_i >= 0 and origin_y >= 0);
 *   - the line is the candidate with the lowest (cost_q, rank): on a tie the offset nearest the centre wins;
 *   - the returned q is the absolute one, -FOCR_BASELINE_MAX ..= 2^B + FOCR_BASELINE_MAX (at most 40: it fits the int8_t):
 *     focr_decoder_get_baselines keeps its format, and y + q * 2^-B px stays the line's true top.
 * focr_decoder_verify keeps its two rules with yc_i as the line's y: the canvas moved by (q + (1 << B >> 1)) >> B rows, which
 * may now be up to FOCR_BASELINE_MAX + 1 rows below its slot, clipped at the page's top and bottom, and after a whole-line
 * run every character at its returned pen.  The launch count stays 3 (2 for the verify).  focr_decoder_run refuses, before
 * anything is launched and with a message that names the setters, a fractional grid without a baseline search or baseline
 * candidates of a whole-line run at a radius >= 1: the plain loop, scores, the pen search, the whole-line decode without
 * candidates, margins and the pen slack have no sub-pixel row to render at (giving them the grid is a later step).  Whatever
 * the mode in force refuses is still refused, and so is line_advance == 0, whatever advance_frac.  focr_decoder_test_images
 * takes its own geometry and knows no grid.  With (0, 0) every run launches and returns what it did before the grid existed.
 * What it does not cure: an unknown leading still has to be read off the returned q of the first lines (y + q * 2^-B), and
 * the other modes stay on the whole-pixel grid. */
/* Set the sub-pixel parts of y_start and line_advance of later runs, each 0 ..= 63 in 1/64 px ((0, 0), off, when the decoder
 * is created; a state of the decoder, not of the font).  A value above 63 is refused here. */
int focr_decoder_set_line_frac(focr_decoder_t *dec, uint32_t y_frac, uint32_t advance_frac);

/* ---- device: font candidates (an extension: the reference decodes every line in one font) --------------------------- */

/* The reference, and every mode above, assumes that every line of every page is set in one font at one size, one kerning
 * and one hinting setting.  Someone looking for those parameters runs the whole job once per guess and compares verify
 * MSEs by eye; someone whose pages mix fonts (a bold or monospace line inside body text, a heading one size up) gets
 * garbage for every line that is not in the decode font, and nothing says which lines those are.  The quantity that
 * separates fonts is the one the decoder already computes: a line's summed footprint terms, its squared error less
 * line_base.  With the font search on, a run decodes every line once per candidate font and keeps the cheapest.
 * A candidate font is a focr_decode_font_t with the decode font's glyph count and code points, in the same order;
 * everything else may differ: size, kerning, hinting, increments, boxes, origin_x and origin_y.  Candidate 0 is the decode
 * font of focr_decoder_set_font; candidates 1 ..= K are the uploaded ones, K <= FOCR_FONT_CANDIDATES_MAX - 1 = 15.
 * All of it is exact:
 *   - plain run: every non-blank line is decoded once per candidate k by the plain pen loop, unchanged: the f32 pen,
 *     delta x = trunc((origin_x_k + pos) * 64), the first minimum over the glyphs, while pos < width, with candidate k's
 *     own tables, increments and origin_x; cost_k is the int64 sum of the chosen glyphs' int32 footprint terms;
 *   - whole-line run (focr_decoder_set_whole_line): every line is decoded once per candidate by the whole-line programme
 *     exactly as defined above, with candidate k's own inc64, origin_x, terms and end state; cost_k is the end state's cost;
 *   - the line is the candidate with the lowest (cost_k, k): on a tie the first candidate wins, so candidate 0 beats an
 *     identical upload;
 *   - the run returns that candidate's text as indices into the common alphabet, and per line k and cost_k
 *     (focr_decoder_get_fonts); a whole-line run also returns the winner's pens and the same cost (focr_decoder_get_pens);
 *   - prepass and compaction are unchanged and the launch count stays 3;
 *   - the characters per line at most are the largest of the candidates' own bounds: the pen loop's walk with each
 *     candidate's smallest increment, ceil(64 * width / min inc64_k) under the whole-line form.
 * With the search off every run launches and returns what it did before the search existed, whatever is uploaded.
 * focr_decoder_run refuses, before anything is launched and each with a message:
 *   - the search on with no candidates uploaded (the message names the switch and the upload call);
 *   - the search on beside scores, a pen search, margins, a pen slack, a baseline search or baseline candidates of a
 *     whole-line run (each message names both setters and ends in "yet"); a fractional line grid is refused by its own rule;
 *   - under the whole-line form, any candidate that fails one of the whole-line run's own checks with its own font: an
 *     origin_x that is not a whole number >= 0, an inc64 < 1, 64 * width + max inc64_k >= 2^24,
 *     ceil(64 * width / min inc64_k) * T_k >= 2^47, or a cost ring that does not fit in LDS; the message names the
 *     candidate's index.
 * focr_decoder_verify after a font-search run is refused with a message: drawing every line in its own font is a later
 * step.  That step is focr_decoder_verify_text (below), which takes the run's lines and their winners and draws each line in
 * its own font.  focr_decoder_test_images knows no candidates.
 * What it does not cure: under the pen loop it is a monospace tool, as the greedy loop itself is (a proportional line is
 * lost under every candidate, and the cheapest wrong reading picks the font: that case needs the whole-line form);
 * focr --verify of a mixed-font run; candidates under scores, the pen search, margins, the pen slack or the baseline modes;
 * and candidates with different alphabets.  (The picture of a mixed-font run is focr --verify-fonts, over
 * focr_decoder_verify_text; --verify itself stays refused beside --font-candidate.) */
enum { FOCR_FONT_CANDIDATES_MAX = 16 };
/* Upload candidates 1 ..= n (the decoder keeps its own copy); n == 0 or NULL drops them; focr_decoder_set_font drops them,
 * and so does a failed upload.  Refused: n > 15, a glyph count or code point that differs from the decode font's, a glyph
 * table that fails set_font's own consistency and int32 checks, an increment <= 0. */
int focr_decoder_set_font_candidates(focr_decoder_t *dec, const focr_decode_font_t *fonts, uint32_t n);
/* Switch the search of later runs on or off (off when the decoder is created; a state of the decoder, not of the font). */
int focr_decoder_set_font_search(focr_decoder_t *dec, int on);
/* The winner k and cost of every line of the last run, in the order of focr_decoder_get: font[n_lines], cost[n_lines].
 * Either may be NULL.  Fails with a message unless the last successful run searched fonts. */
int focr_decoder_get_fonts(const focr_decoder_t *dec, uint8_t *font, int64_t *cost);
/* Debug: at most `grid` workgroups for later font-search runs (0: the decoder's own choice), so that a test can make one
 * workgroup take several lines. */
int focr_decoder_debug_set_fonts_grid(focr_decoder_t *dec, uint32_t grid);

/* ---- device: verify images of the last run (draw_verify + red_blue_mse, src/main.rs:300-329, 518-524) ------------ */

/* Upload the verify table of the current decode font (the decoder keeps its own copy).  Refused unless it matches the
 * decode font: glyph count, code points, increments (bitwise), origin, size, kerning and hinting.  focr_decoder_set_font
 * drops the verify table, and so does a failed upload. */
int focr_decoder_set_verify_font(focr_decoder_t *dec, const focr_verify_font_t *font);
/* The verify image and squared error of every page of the last successful focr_decoder_run, on the decoder's stream:
 * red = the page's luma where it is not 255, blue = 255 - v where the decoded line rendered at (x_start, line y) as
 * render() does has v != 0 (later lines over earlier ones, clipped to the page), green = 0.  rgb receives
 * n_pages x page_h x page_w x 3 bytes, in host memory, or in device memory of the decoder's device when
 * rgb_on_device != 0, or nothing when NULL; sq_sums[n_pages] receives the exact sum over the page of (R - B)^2 (the
 * reference's MSE is (float)sum / (float)(uint32_t)(page_w * page_h)).  For a run from device-memory pages, the
 * caller's page buffer must still hold those pages.  After a run with a pen search every character is rendered at
 * the pen the run chose for it (pen + j / 64, then the increment from there), and after a whole-line run at
 * pos = s / 64 of its returned pen s (with pen slack that is the render pen), so the image shows the line where it was decoded.
 * After a run with a baseline search every line's canvas is drawn moved by the nearest whole row of its offset,
 * (q + (1 << B >> 1)) >> B rows down (up when negative), and clipped at the page's top as well as its bottom; the
 * sub-pixel part of the offset is not drawn (the verify table has one vertical phase).  After a whole-line run under
 * baseline candidates (focr_decoder_set_whole_baseline) both rules hold: every character at pos = s / 64 of its returned
 * pen, on a canvas moved and clipped in that way.  Runs a fixed number of launches and returns when the results are in rgb and sq_sums.  Fails with a message
 * without a successful run since the last set_font, without a verify table, or after a run that searched fonts
 * (focr_decoder_set_font_search): the table has one font, and drawing every line in its own is a later step. */
int focr_decoder_verify(focr_decoder_t *dec, uint8_t *rgb, int rgb_on_device, uint64_t *sq_sums);
/* Device time of the last verify's kernels in ms (events), and their launch count (constant per batch). */
float focr_decoder_last_verify_ms(const focr_decoder_t *dec);
uint32_t focr_decoder_last_verify_launches(const focr_decoder_t *dec);

/* ---- device: verify images of a caller's text (an extension: the verify above draws only what the last run decoded) ---- */

/* focr_decoder_verify draws the last run's own lines in the decode font, so two readings of a page have no picture: what a
 * font search decoded (every line in its winner's font), and a reading that somebody corrected after looking at scores,
 * margins or a checksum.  focr_decoder_verify_text draws the same image and the same sums for a list of lines the caller
 * supplies, each line in any font the decoder has uploaded.  All of it is exact:
 *   - line l is drawn in font lines[l].font: 0 is the decode font of focr_decoder_set_font with the verify table of
 *     focr_decoder_set_verify_font; 1 ..= K are the candidates of focr_decoder_set_font_candidates with the verify tables of
 *     focr_decoder_set_verify_font_candidates;
 *   - its text is chars[first .. first + n_chars), alphabet indices, rendered as render() renders a string: the f32 pen, the
 *     union of the glyphs' round_out boxes, FreeType's delta trunc((-bounds.ox + pos) * 64) per glyph, all with that font's
 *     increments, boxes, phase rectangles and origin_y;
 *   - the canvas's top-left goes at (x_start, y) on page `page` and is clipped at the page's right and bottom edges; a line
 *     with n_chars == 0 or y >= page_h draws nothing;
 *   - pens and offsets both NULL: the pen of a glyph is the f32 sum of the increments before it, in text order;
 *   - pens (1/64 px, beside chars, each below 2^24): glyph q of a line is placed at pens[first + q] / 64, whatever the
 *     increments, as focr_decoder_verify places it after a whole-line run;
 *   - offsets (1/64 px, beside chars): glyph q is placed at pen + offsets[first + q] / 64 and the pen advances from there by
 *     its increment, as focr_decoder_verify does after a run with a pen search; pens and offsets together are refused;
 *   - lines come in non-decreasing page order; within a page the list order is the drawing order: a later line's non-zero
 *     pixels replace an earlier line's blue; y may come in any order and repeat, and lines may overlap and share characters;
 *   - the image and the sums are focr_decoder_verify's: red = the page's luma where it is not 255, blue = 255 - v where the
 *     last line over the pixel has v != 0, green = 0; rgb (n_pages x page_h x page_w x 3 bytes) in host memory, in device
 *     memory of the decoder's device when rgb_on_device != 0, or NULL; sq_sums[n_pages] the exact sum of (R - B)^2; a page
 *     without a line still gets its image and its sum.  pages as for focr_decoder_run.
 * Refused, each with its own message and before anything is launched: NULL pages, lines, chars or sq_sums where there are
 * pages, lines or characters; no decode font; a font above K (the message names the line's index); a font whose verify table
 * is not uploaded (the message names the setter to call); a page index that decreases or is >= n_pages; first + n_chars past
 * the n_chars of the call; a character index >= the alphabet's size; a pen >= 2^24 (all n_chars entries of chars and pens are
 * checked); a page too large for focr_decoder_run.
 * The call runs two launches in buffers of its own, as focr_decoder_test_images does: the last run, its getters, its timing
 * and its focr_decoder_verify answer as they did before, and it needs no run at all.  Returns when rgb and sq_sums are
 * written.  What it does not do: a per-line x, lines at sub-pixel rows, per-line sums (the decoder's
 * per-line cost is focr_decoder_score_text, below). */
/* focr_decoded_line_t with the font in pad's place: a caller can pass focr_decoder_get's lines unchanged (font 0). */
typedef struct focr_text_line {
    uint32_t page, y;
    uint64_t first;
    uint32_t n_chars;
    uint32_t font;
} focr_text_line_t;

/* Upload the verify tables of the candidates 1 ..= n (the decoder keeps its own copy), fonts[k - 1] for candidate k.  Refused
 * unless n is the number of uploaded candidates and every table matches its candidate: glyph count, code points, increments
 * (bitwise), origin_y, size, kerning and hinting, and no phase rectangle leaves the candidate's box.
 * focr_decoder_set_font, focr_decoder_set_font_candidates and a failed upload drop the tables. */
int focr_decoder_set_verify_font_candidates(focr_decoder_t *dec, const focr_verify_font_t *fonts, uint32_t n);
int focr_decoder_verify_text(focr_decoder_t *dec, const uint8_t *pages, int pages_on_device, size_t n_pages,
                             size_t page_w, size_t page_h, uint32_t x_start,
                             const focr_text_line_t *lines, size_t n_lines,
                             const uint16_t *chars, const uint32_t *pens, const int8_t *offsets, size_t n_chars,
                             uint8_t *rgb, int rgb_on_device, uint64_t *sq_sums);
/* Device time of the last verify_text's kernels in ms (events), and their launch count (constant: 2; 0 after a refusal). */
float focr_decoder_last_verify_text_ms(const focr_decoder_t *dec);
uint32_t focr_decoder_last_verify_text_launches(const focr_decoder_t *dec);

/* ---- device: the cost of a caller's text (an extension: verify_text above gives a picture and one sum per page) ---- */

/* Every mode of the decoder minimises a sum of footprint terms and returns it: scores, whole-line costs, the margins'
 * terms, baseline costs, font costs.  focr_decoder_score_text computes that sum for lines the caller supplies, each in any
 * font the decoder has uploaded: of a reading that was decoded (it then equals what the run returned), of one somebody
 * corrected (is the edited line better or worse than the decoded one?), or of a string somebody typed in, under every
 * candidate font (the font that renders a known first line closest to the page is the font: no decoding, exact for
 * proportional fonts too).  There is one glyph per character to evaluate, not one alphabet per step, and no dynamic
 * programme.  All of it is exact integer and f32 arithmetic:
 *   - lines are focr_text_line_t, as for focr_decoder_verify_text, so focr_decoder_get's lines go in unchanged; unlike there
 *     they may come in any page order; they may repeat and share characters;
 *   - line l's crop is the decoder's: rows y .. y + min(line_height, page_h - y), columns x_start .. x_start + min(width,
 *     page_w - x_start), clamped as image::crop_imm clamps; out[l].line_base is its sum of r^2, r = 255 - luma; an empty
 *     crop has line_base 0 and every term 0;
 *   - font k = lines[l].font: 0 is the decode font, 1 ..= K the candidates of focr_decoder_set_font_candidates, each with its
 *     own glyph tables, increments and origin_x; no verify table is needed;
 *   - pens and offsets both NULL: the pen loop's placement: pos starts at 0, glyph g is rendered at FreeType's delta
 *     trunc((origin_x_k + pos) * 64) in f32, then pos = pos + increment, one f32 add;
 *   - offsets (1/64 px, beside chars): the pen search's placement: p = pos + (float)offsets[g] * 0.015625f, the delta comes
 *     from p, and pos = p + increment;
 *   - pens (1/64 px, beside chars, each below 2^24): the whole-line programme's placement: delta = 64 * origin_x_k + pens[g],
 *     which needs an origin_x_k that is a whole number >= 0; pens and offsets together are refused;
 *   - the phase is delta & 63 and the whole-pixel shift delta >> 6 (an arithmetic shift), so a negative delta is what
 *     FreeType would receive and nothing is dropped; the line does not end at pos >= width: a glyph wholly outside the crop
 *     has term 0;
 *   - line_q (NULL: none; else one per line): the line is rendered as the baseline modes render candidate q = line_q[l], in
 *     steps of 2^-B px, B = y_bits <= FOCR_BASELINE_Y_BITS_MAX: from y-phase v = q & (2^B - 1) of the fonts of
 *     focr_decoder_set_baseline_fonts, every box moved down q >> B rows (floor); bitmaps are clipped to the crop on all four
 *     sides; on a fractional line grid pass the lines' y = yc_i and the run's absolute q;
 *   - a character's term is the int32 footprint term the decoder compares: the sum of c * (c - 2 r) over the clipped bitmap;
 *     out[l].cost is their sum over the line; terms (NULL: not wanted) takes one entry per listed character in list order,
 *     line l's at the running sum of n_chars over the lines before it;
 *   - shift_radius N, 0 <= N <= FOCR_PEN_SEARCH_MAX: every line is scored once per j in -N ..= N with the whole line moved
 *     by j / 64 px: the pen-loop and offsets placements start from p_0 = (float)(offsets[0] + j) * 0.015625f (offsets[0] = 0
 *     without offsets), the pens placement uses pens[g] + j for every glyph; the line's result is the lowest
 *     (cost_j, rank(j)) with the pen search's rank (0, -1, +1, -2, ...); out[l].shift is that j, and cost and terms are its.
 *     N = 0 scores once.
 * Refused, each with its own message and before anything is launched: NULL pages, lines, chars or out where there are
 * pages, lines or characters; pens and offsets together; no decode font; width 0 or line_height 0; a shift_radius or
 * y_bits above its maximum; a page too large for focr_decoder_run; line_q with y_bits > 0 and no y-phase fonts of that
 * y_bits; and per line (the message names its index) a font above K, a page index >= n_pages, first + n_chars past the
 * n_chars of the call, pens with a font whose origin_x is fractional or negative, line_q with a fractional-phase q on a
 * font other than 0 (the candidates have one vertical phase), line_q with a font whose origin_y is not a whole number
 * >= 0; a character index >= the alphabet's size; a pen >= 2^24 (all n_chars entries of chars and pens are checked).
 * The call runs one launch, or two when a line's strip does not fit in LDS (the strips are then built in global memory
 * first), whatever the lines, the placement and the radius, in buffers of its own: the last run, its getters, its verify and
 * their timings answer as they did before, and it needs no run at all.  pages as for focr_decoder_run.  Returns when out
 * and terms are written; with n_lines == 0 nothing is launched.
 * What it does not do: a per-line x; a vertical search (list the line at several (y, q)); a forced alignment that fits
 * each character's offset to a known text (that is focr_decoder_align_text, below); the true composed error where footprints overlap (line_base + cost counts an
 * overlap once per glyph; the composed error stays focr_decoder_verify_text's page sum); any change to focr_decoder_run. */
typedef struct focr_text_score {
    uint64_t line_base;   /* sum of r^2 over the line's crop, r = 255 - luma */
    int64_t  cost;        /* sum of the line's footprint terms at the winning shift */
    int32_t  shift;       /* the winning rigid shift j in 1/64 px (0 when shift_radius == 0) */
    uint32_t pad;
} focr_text_score_t;

int focr_decoder_score_text(focr_decoder_t *dec, const uint8_t *pages, int pages_on_device, size_t n_pages,
                            size_t page_w, size_t page_h, uint32_t x_start, uint32_t width, uint32_t line_height,
                            const focr_text_line_t *lines, size_t n_lines,
                            const uint16_t *chars, const uint32_t *pens, const int8_t *offsets, size_t n_chars,
                            const int8_t *line_q, uint32_t y_bits, uint32_t shift_radius,
                            int32_t *terms, focr_text_score_t *out);
/* Device time of the last score_text's kernels in ms (events), and their launch count (1, or 2 with global strips; 0 after a
 * refusal or a call without lines). */
float    focr_decoder_last_score_text_ms(const focr_decoder_t *dec);
uint32_t focr_decoder_last_score_text_launches(const focr_decoder_t *dec);

/* ---- device: a forced alignment (an extension: the fit score_text above leaves out) ------------------------------- */

/* focr_decoder_score_text costs a known line at pens it is given, or at the font's own advances moved rigidly by at most one
 * pixel.  A page set at another kerning, moved by a fraction of a pixel or snapped to the pixel grid loses its own font
 * there.  focr_decoder_align_text fits every character's pen to the page instead: a banded dynamic programme over offsets
 * from the font's own pens, one line per listed line, exact integer arithmetic throughout.
 *   - lines, chars, line_q / y_bits, the crop (x_start, width, line_height at the line's y) and line_base are
 *     focr_decoder_score_text's; the listed line l has characters c_0 .. c_{n-1} in font k = lines[l].font;
 *   - inc64[i] = (int)rintf(increment[i] * 64) of font k, the whole-line programme's; the nominal pen of character g is
 *     m_g = start + sum over h < g of inc64[c_h], in 1/64 px;
 *   - a state is (g, e) with -W <= e <= W, W = drift <= FOCR_ALIGN_DRIFT_MAX; it is live when m_g + e >= 0;
 *   - its placement is focr_decoder_score_text's pens placement at the pen m_g + e: delta = 64 * origin_x_k + m_g + e, phase
 *     delta & 63, whole-pixel shift delta >> 6; the line's q applies as there (y-phase q & (2^B - 1), rows moved q >> B);
 *     the bitmap is clipped to the crop on all four sides; T(g, e) is the int32 footprint term there;
 *   - F(0, e) = T(0, e) for live e; for g > 0, F(g, e) = T(g, e) + the lowest (F(g - 1, e - d), rank(d)) over d in -N ..= N,
 *     N = step <= FOCR_PEN_SEARCH_MAX, with (g - 1, e - d) inside the band, live and reachable; rank is the pen search's
 *     (0, -1, +1, -2, ...); back(g, e) is that d, and a state without such a d is unreachable;
 *   - the line ends in the reachable e with the lowest (F(n - 1, e), rank(e)); the walk back is e_{g-1} = e_g - back(g, e_g);
 *   - out[l] = { line_base, cost = F(n - 1, e_{n-1}), first = e_0, last = e_{n-1} }; per listed character, line l's at the
 *     running sum of n_chars over the lines before it (as score_text's terms): pens_out takes the pen m_g + e_g, terms
 *     (NULL: not wanted) the term T(g, e_g); the terms of a line sum to its cost, and focr_decoder_score_text and
 *     focr_decoder_verify_text take the pens as they are;
 *   - n == 0 gives cost 0 and first = last = 0; an empty crop has every term 0, so the ranks give e_g = 0 throughout (e = 0
 *     is live whatever start is); an offset costs nothing; N = 0 is a rigid
 *     search of radius W (with start >= W and W <= 64 it is score_text's shift search over the nominal pens).
 * The fit of the pens (what the kerning and x of the page were): over the characters g of a line whose term is not 0 (a space
 * never has one), in list order and in double arithmetic, with u_g = (double)(m_g - start) and p_g = (double)pen_g and k their
 * number: Su = sum u_g, Sp = sum p_g, Suu = sum u_g * u_g, Sup = sum u_g * p_g, D = k * Suu - Su * Su;
 * scale = (k * Sup - Su * Sp) / D and x64 = (Sp - scale * Su) / k, each product and sum rounded once, left to right as written;
 * there is no fit when k < 2 or D == 0.  scale is the page's kerning relative to the font's, x64 the pen of a character at
 * nominal `start`, in 1/64 px.
 * Refused, each with its own message and before anything is launched: what focr_decoder_score_text refuses of the same
 * arguments; NULL pens_out where there are lines; drift or step above its maximum; per line (the message names its index) a
 * font whose origin_x is fractional or negative, and start + the sum of its inc64 + drift >= 2^24; the backpointers of the
 * call (one byte per listed character and state of the band, n_out * (2 * drift + 1)) above 256 MiB: the message says to list
 * fewer lines or ask for less drift.
 * The call runs one launch, or two when a line's strip and the programme's two cost rows do not fit in LDS together (the strips
 * are then built in global memory first), in buffers of its own: the last run, its getters, its verify, and score_text's and
 * verify_text's last timings answer as they did before, and it needs no run at all.  pages as for focr_decoder_run.  Returns
 * when out, pens_out and terms are written; with n_lines == 0 nothing is launched.
 * What it does not do: a per-line start; a vertical fit (list the line at several q); alignment inside focr_decoder_run; a
 * penalty on offsets. */
enum { FOCR_ALIGN_DRIFT_MAX = 1024 };
typedef struct focr_text_align {
    uint64_t line_base;   /* sum of r^2 over the line's crop, r = 255 - luma */
    int64_t  cost;        /* F(n - 1, e_{n-1}): the sum of the line's footprint terms at the fitted pens */
    int32_t  first, last; /* e_0 and e_{n-1} in 1/64 px */
} focr_text_align_t;

int focr_decoder_align_text(focr_decoder_t *dec, const uint8_t *pages, int pages_on_device, size_t n_pages,
                            size_t page_w, size_t page_h, uint32_t x_start, uint32_t width, uint32_t line_height,
                            const focr_text_line_t *lines, size_t n_lines,
                            const uint16_t *chars, size_t n_chars,
                            const int8_t *line_q, uint32_t y_bits, uint32_t start, uint32_t drift, uint32_t step,
                            uint32_t *pens_out, int32_t *terms, focr_text_align_t *out);
/* Device time of the last align_text's kernels in ms (events), and their launch count (1, or 2 with global strips; 0 after a
 * refusal or a call without lines). */
float    focr_decoder_last_align_text_ms(const focr_decoder_t *dec);
uint32_t focr_decoder_last_align_text_launches(const focr_decoder_t *dec);

/* ---- device: glyph tables from a trusted reading (an extension: the tables are what score_text and align_text leave wrong) ---- */

/* Every mode compares the page with what this FreeType build draws; a page from another renderer or another cut of the font is
 * "very close but not identical".  Once font, size, kerning and x are right (focr_decoder_score_text, focr_decoder_align_text), the
 * glyph tables are what is still wrong.  The least-squares template of a cell (glyph i, phase p) is the mean of the page's
 * inverted luma under every occurrence of that cell.  focr_decoder_learn_text computes the sums and the counts of those means from
 * a reading the caller TRUSTS (a few corrected pages, or a text that is known); focr_decode_font_learn (below) turns them into a
 * focr_decode_font_t, and the remaining pages are decoded with it.  All of it is exact integer arithmetic but the f32 pen:
 *   - lines, chars, pens, offsets, the crop (x_start, width, line_height at the line's y, clamped) and the three placements are
 *     focr_decoder_score_text's at shift 0; there is no line_q: a line moved by whole rows is a line at another y, and the
 *     y-phase tables are not learned;
 *   - font k, 0 <= k <= K, is the font to learn: 0 the decode font, 1 ..= K a candidate.  Only the listed lines with
 *     lines[l].font == k contribute; the others are accepted (and checked) and contribute nothing;
 *   - use (NULL: every character) has one byte per entry of chars; 0 leaves that character out, and it still moves the pen;
 *   - character g of a contributing line, glyph i of font k, has its delta as score_text computes it, phase p = delta & 63 and
 *     whole-pixel shift delta >> 6; its box is box_w x box_h at crop column shift + off_x[p] and crop row off_y[p];
 *   - it contributes iff it is in use and that box lies wholly inside the crop (there are no partial boxes); an empty crop holds
 *     no box, not even a blank glyph's box without pixels;
 *   - a contributing character adds 1 to counts[i * 64 + p], and for row < box_h and col < box_w the value r = 255 - luma of the
 *     crop pixel under it to sums[offset_i + (p * box_h + row) * stride + col]: font k's own `bitmaps` layout, one uint32 per
 *     byte, so sums has bitmaps_len entries and counts 64 * n_glyphs; the padding columns col >= box_w stay 0;
 *   - used (NULL: not wanted) takes 1 or 0 per listed character, line l's at the running sum of n_chars over the lines before
 *     it (as score_text's terms), 0 throughout a line of another font;
 *   - repeated lines and shared characters count once per listing;
 *   - sums, counts and used are this call's alone: they are zeroed first, and the caller adds calls up (in 64 bits).
 * Refused, each with its own message and before anything is launched: what focr_decoder_score_text refuses of the same
 * arguments (NULL pages, lines or chars; pens and offsets together; no decode font; width 0 or line_height 0; a page too
 * large; per line a font above K, a page index >= n_pages, characters past n_chars, pens with a fractional or negative
 * origin_x; a character index >= the alphabet's size; a pen >= 2^24); NULL sums or NULL counts, whatever n_lines; a font to learn
 * above K; 2^24 or more listed characters in one call (255 * 2^24 is the bound of a uint32 sum).
 * The call runs one launch, or two when a line's strip does not fit in LDS (the strips are then built in global memory first;
 * the zeroing of its outputs lies inside the measured time and is no launch of the count), in buffers of its own: the last
 * run, its getters, its verify, and the other text calls' last timings answer as they did before, and it needs no run at all.
 * pages as for focr_decoder_run.  Returns when sums, counts and used are written; with n_lines == 0 nothing is launched and sums
 * and counts are zeros.
 * What it does not do: y-phase tables; pooling of neighbouring phases; weights; an NCC bank from the result; and learning from
 * an untrusted reading: measured on 8 px hinted pages, tables learned from the decoder's own reading of those pages reproduce that
 * reading's errors (no fewer wrong characters after than before), and gating the samples by score margin does not help. */
int focr_decoder_learn_text(focr_decoder_t *dec, const uint8_t *pages, int pages_on_device, size_t n_pages,
                            size_t page_w, size_t page_h, uint32_t x_start, uint32_t width, uint32_t line_height,
                            const focr_text_line_t *lines, size_t n_lines,
                            const uint16_t *chars, const uint32_t *pens, const int8_t *offsets, const uint8_t *use, size_t n_chars,
                            uint32_t font, uint32_t *sums, uint32_t *counts, uint8_t *used);
/* Device time of the last learn_text's kernels and of the zeroing in front of them in ms (events), and the kernels' launch
 * count (1, or 2 with global strips; 0 after a refusal or a call without lines). */
float    focr_decoder_last_learn_text_ms(const focr_decoder_t *dec);
uint32_t focr_decoder_last_learn_text_launches(const focr_decoder_t *dec);

/* The learned font (host, libfocr_raster.so): `base` with the cells that were seen replaced by their means.  sums and counts are
 * focr_decoder_learn_text's of `base`, calls added up in 64 bits (sums: base->bitmaps_len entries, counts: 64 * n_glyphs).
 *   - cell (i, p) is learned when counts[i * 64 + p] >= min_count (min_count >= 1) and phase p of glyph i has ink in base;
 *   - its support is the bounding rectangle of the base phase's non-zero pixels, grown by `grow` pixels on each side and clipped
 *     to the box; inside it the byte is (2 * sum + n) / (2 * n), n the cell's count: the mean rounded half up, at most 255;
 *   - an unlearned cell, everything outside a support and every other field are base's: increments, boxes, offsets, origin,
 *     size, kerning, hinting.  A blank glyph stays blank, and base's verify table still matches.
 * With grow = 0 a glyph never claims ink outside its own extent.  With grow = 1 the measured cost of a page drops below
 * -line_base: neighbouring supports overlap more, and the objective counts an overlap once per glyph (its known limit), so 0 is
 * the default of every caller (where the boxes themselves overlap, as at 8 px, a cost slightly below -line_base is met at 0 too).  *learned (NULL: not wanted) takes the number of learned cells, *inked the number of cells with ink.
 * out owns its tables: free with focr_decode_font_free.  Fails with a message on a NULL argument, min_count 0 or no memory. */
int focr_decode_font_learn(const focr_decode_font_t *base, const uint64_t *sums, const uint64_t *counts, uint32_t min_count,
                           uint32_t grow, focr_decode_font_t *out, size_t *learned, size_t *inked, char *err, size_t errlen);

/* ---- device: a reading repaired against the composed line error (an extension: the step score_text above leaves out) ---- */

/* Every mode minimises a sum of per-glyph footprint terms, which is the page's squared error only while footprints do not
 * overlap: where they do, an overlap is counted once per glyph, and tight proportional text is misread (`born` for `burn`,
 * `cIIp` for `clip`).  focr_decoder_refine_text takes a reading a run produced, holds it against the line with all its glyphs
 * drawn together, and repairs one character at a time.  Exact integer arithmetic throughout:
 *   - lines and chars are focr_decoder_score_text's, in any page order; the crop (x_start, width, line_height at the line's y,
 *     clamped) and line_base are its; font k = lines[l].font is 0 or a candidate, with its own tables; pens (1/64 px, beside
 *     chars, each below 2^24) are required, and the placement is score_text's pens placement: delta = 64 * origin_x_k + s_g,
 *     phase delta & 63, whole-pixel shift delta >> 6, the phase bitmap clipped to the crop on all four sides: c_g(p);
 *   - the composed canvas is v(p) = max over the line's characters of c_g(p), 0 where none reaches (the max of ink: what
 *     np.minimum of luma draws), and with r = 255 - luma the composed cost is C = sum over p of v(p) * (v(p) - 2 r(p)), so
 *     line_base + C = sum of (r - v)^2 >= 0; where no two glyphs put ink on one pixel C is score_text's cost;
 *   - one step, for character g with glyph a_g at pen s_g: o(p) is the max over all characters but g as they stand now, and
 *     with f(v) = v * (v - 2 r), D(a, j) = sum over the clipped box of glyph a at pen s_g + j of f(max(c, o)) - f(o): what the
 *     composed cost gains when (a, j) is drawn over the others.  The candidates are every glyph a of the font (only a_g when
 *     glyphs == 0) times j in -N ..= N, N = radius <= FOCR_PEN_SEARCH_MAX, with 0 <= s_g + j < 2^24; the incumbent is (a_g, 0).
 *     If some candidate has D strictly below the incumbent's, character g becomes the lowest (D, rank(j), a) among the
 *     candidates, rank the pen search's (0, -1, +1, -2, ...); otherwise it stays;
 *   - a sweep takes g = 0 .. n - 1 in order, each step seeing the earlier steps' results; a line stops after a sweep that
 *     changed nothing or after `sweeps` <= FOCR_REFINE_SWEEPS_MAX sweeps; sweeps == 0 only evaluates;
 *   - a pixel's f(max(c, o)) - f(o) = (m - o) * (m + o - 2 r), m = max(c, o), is at most 2 * 255^2 in magnitude, and every font
 *     upload refuses a glyph whose box area times 2 * 255^2 reaches 2^31: D fits an int32 and is kept in one; C, summed over the
 *     crop, is kept in 64 bits;
 *   - out[l] = { line_base, cost_in (C of the input), cost (C of the output), sweeps_run (the sweeps made, the one that changed
 *     nothing included), changed (the characters whose glyph or pen differs from the input) }; chars_out and pens_out take the
 *     output per listed character, line l's at the running sum of n_chars over the lines before it (as align_text's pens_out).
 *     No other pen moves when a glyph with another advance is chosen.  focr_decoder_score_text, focr_decoder_verify_text and
 *     focr_decoder_learn_text take chars_out and pens_out as they are; cost <= cost_in always.
 * Refused, each with its own message and before anything is launched: what focr_decoder_score_text refuses of the same
 * arguments; NULL pens, and NULL chars_out, pens_out or out where there are lines; radius or sweeps above its maximum; per line
 * (the message names its index) a font whose origin_x is fractional or negative, pens that decrease within the line (the
 * message names the character), a font with a glyph box more than 2^20 px from its pen; and fonts whose boxes span so many
 * columns and rows that the window of one step does not fit a workgroup's memory.  Non-decreasing pens are what every run
 * produces; the rule lets the kernel bound which characters can reach a step's window, since no pen moves more than
 * sweeps * radius from a sorted input.
 * The call runs one launch, or two when a line's strip and a step's window do not fit in LDS together (the strips are then built
 * in global memory first), in buffers of its own: the last run, its getters, its verify and the other text calls' last timings
 * answer as they did before, and it needs no run at all.  pages as for focr_decoder_run.  Returns when out, chars_out and
 * pens_out are written; with n_lines == 0 nothing is launched.
 * What it does not do: insertions and deletions (`rn` against `m` stays the whole-line decode's job); baseline candidates or
 * line_q; a per-line x; any change to focr_decoder_run; render()'s copy rule, under which a later glyph's blank margin erases an
 * earlier glyph's ink (that picture stays focr_decoder_verify_text's). */
enum { FOCR_REFINE_SWEEPS_MAX = 8 };
typedef struct focr_text_refine {
    uint64_t line_base;   /* sum of r^2 over the line's crop, r = 255 - luma */
    int64_t  cost_in;     /* the composed cost C of the input */
    int64_t  cost;        /* ... and of the output */
    uint32_t sweeps_run;  /* sweeps made */
    uint32_t changed;     /* characters whose glyph or pen differs from the input */
} focr_text_refine_t;

int focr_decoder_refine_text(focr_decoder_t *dec, const uint8_t *pages, int pages_on_device, size_t n_pages,
                             size_t page_w, size_t page_h, uint32_t x_start, uint32_t width, uint32_t line_height,
                             const focr_text_line_t *lines, size_t n_lines,
                             const uint16_t *chars, const uint32_t *pens, size_t n_chars,
                             uint32_t radius, uint32_t sweeps, int glyphs,
                             uint16_t *chars_out, uint32_t *pens_out, focr_text_refine_t *out);
/* Device time of the last refine_text's kernels in ms (events), and their launch count (1, or 2 with global strips; 0 after a
 * refusal or a call without lines). */
float    focr_decoder_last_refine_text_ms(const focr_decoder_t *dec);
uint32_t focr_decoder_last_refine_text_launches(const focr_decoder_t *dec);

/* ---- device: test images (focr --test: draw_test_rectangles, draw_test_text, src/main.rs:241-298) ---------------- */

/* focr --test's two images of each page of a batch of n_pages equal-size pages, drawn on the decoder's stream.  Both
 * start from base_rgba (n_pages x page_h x page_w x 4 bytes, RGBA), or from (l, l, l, 255) of the luma pages when
 * base_rgba is NULL (into_rgba8 of a grey image):
 *   rect_rgba: for every line slot whose crop is not blank (the decoder's crop and blank test on the luma pages), the
 *              box x_start ..= x_start + width by y ..= y + line_height, each edge pixel blended once with
 *              Rgba(255, 0, 0, 128) per edge through it (corners twice, shared rows of overlapping boxes more); pixels
 *              outside the page are skipped (the reference panics there);
 *   text_rgba: render() of the whole alphabet of the decode font at (0, 0), clipped to the page: where the canvas has
 *              v != 0, the pixel is blended once with Rgba(255 - v, 0, 0, 128).
 * The blend is image 0.25's Blend for Rgba<u8>, restated in f32 (parity unpinned).  A NULL output is not drawn.
 * Inputs are in host memory, or in device memory of the decoder's device when in_on_device != 0; outputs likewise with
 * out_on_device (n_pages x page_h x page_w x 4 bytes each); device RGBA buffers must be 4-byte aligned.  text_rgba
 * needs a decode font and a verify table (focr_decoder_set_verify_font); rect_rgba needs neither.  line_advance == 0
 * with a non-empty first crop is refused, as in focr_decoder_run.  Runs a fixed number of launches, in buffers of its
 * own: the last run's results, timing and verify stay as they were.  Returns when the images are written. */
int focr_decoder_test_images(focr_decoder_t *dec, const uint8_t *pages, const uint8_t *base_rgba, int in_on_device,
                             size_t n_pages, size_t page_w, size_t page_h, uint32_t x_start, uint32_t y_start,
                             uint32_t width, uint32_t line_height, uint32_t line_advance,
                             uint8_t *rect_rgba, uint8_t *text_rgba, int out_on_device);
/* Device time of the last test_images' kernels in ms (events), and their launch count (constant per batch: 3 with
 * both images, one less without either). */
float focr_decoder_last_test_ms(const focr_decoder_t *dec);
uint32_t focr_decoder_last_test_launches(const focr_decoder_t *dec);
/* Debug: out[i] = the device's blend of fg[i] onto bg[i], for n RGBA pixels in host memory (the function
 * focr_decoder_test_images blends with). */
int focr_decoder_debug_blend(focr_decoder_t *dec, const uint8_t *bg_rgba, const uint8_t *fg_rgba, size_t n, uint8_t *out_rgba);

#ifdef __cplusplus
}
#endif
#endif /* FOCR_DECODE_H */
