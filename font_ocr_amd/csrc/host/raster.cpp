// raster.cpp — CPU rasterisation of the glyph-template bank (libfocr_raster.so).
//
// Follows get_hits' bank loop and render() of the reference
// (src/ncc.rs:563-573 offsets, 587-628 box size, 629-641 per-letter render,
// 143-196 render) on top of FreeType directly.  The reference goes through
// font-kit 0.14 (freetype loader) + pathfinder_geometry 0.5, neither of which
// is vendored in /root/reference; their behaviour is restated from their
// published semantics (DESIGN.md "third-party arithmetic"):
//   * typographic_bounds: FT_Load_Glyph(NO_HINTING) at char size = units_per_em,
//     rect (horiBearingX, horiBearingY - height, width, height) / 64.
//   * raster_bounds: typographic bounds * (size / upem), y flipped to
//     top-left origin, translated, round_out.
//   * rasterize_glyph: FT_Set_Transform(identity, delta = trunc(t * 64) with y
//     negated), FT_Set_Char_Size(size * 64), FT_Load_Glyph(RENDER | flags),
//     copy the 8-bit bitmap at (bitmap_left, -bitmap_top), clipped to the canvas.
// Parity of the rasterised bytes with the reference is unpinned (no fixtures
// upstream); the scan's parity contract is on identical (page, bank) bytes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <ft2build.h>
#include FT_FREETYPE_H
#include FT_TRUETYPE_TABLES_H

#include "focr_decode.h"
#include "focr_host.h"
#include "../hip/learn_font.h"

namespace {

struct RectF {
    float ox = 0, oy = 0, lx = 0, ly = 0;  // origin, lower-right (pathfinder RectF layout)
    float width() const { return lx - ox; }
    float height() const { return ly - oy; }
};

RectF scale(const RectF &r, float f) { return {r.ox * f, r.oy * f, r.lx * f, r.ly * f}; }
RectF union_rect(const RectF &a, const RectF &b) {
    return {std::fmin(a.ox, b.ox), std::fmin(a.oy, b.oy), std::fmax(a.lx, b.lx), std::fmax(a.ly, b.ly)};
}
struct RectI {
    int ox, oy, lx, ly;
    int width() const { return lx - ox; }
    int height() const { return ly - oy; }
};
RectI round_out(const RectF &r) {
    return {(int)std::floor(r.ox), (int)std::floor(r.oy), (int)std::ceil(r.lx), (int)std::ceil(r.ly)};
}

struct Face {
    FT_Library lib = nullptr;
    FT_Face face = nullptr;
    ~Face() {
        if (face) FT_Done_Face(face);
        if (lib) FT_Done_FreeType(lib);
    }
    void reset_size() {  // font-kit keeps the face at char size = units_per_em between calls
        FT_Set_Char_Size(face, (FT_F26Dot6)face->units_per_EM << 6, 0, 0, 0);
        FT_Set_Transform(face, nullptr, nullptr);
    }
    bool typographic_bounds(FT_UInt gid, RectF *out) {
        reset_size();
        if (FT_Load_Glyph(face, gid, FT_LOAD_DEFAULT | FT_LOAD_NO_HINTING) != 0) return false;
        const FT_Glyph_Metrics &m = face->glyph->metrics;
        int ox = (int)m.horiBearingX, oy = (int)(m.horiBearingY - m.height);
        int w = (int)m.width, h = (int)m.height;
        out->ox = ox / 64.0f;
        out->oy = oy / 64.0f;
        out->lx = (ox + w) / 64.0f;
        out->ly = (oy + h) / 64.0f;
        return true;
    }
    // Loader::raster_bounds before the translation: (nox, noy, nox + width, noy + height), each rounded to f32.
    bool raster_box(FT_UInt gid, float size, RectF *out) {
        RectF tb;
        if (!typographic_bounds(gid, &tb)) return false;
        RectF trb = scale(tb, size / (float)face->units_per_EM);
        float nox = trb.ox, noy = -trb.oy - trb.height();
        *out = RectF{nox, noy, nox + trb.width(), noy + trb.height()};
        return true;
    }
    // Loader::raster_bounds default implementation for a pure translation.
    bool raster_bounds(FT_UInt gid, float size, float tx, float ty, RectI *out) {
        RectF b;
        if (!raster_box(gid, size, &b)) return false;
        *out = round_out(RectF{b.ox + tx, b.oy + ty, b.lx + tx, b.ly + ty});
        return true;
    }
};

int fail(char *err, size_t errlen, const char *msg) {
    if (err && errlen) snprintf(err, errlen, "%s", msg);
    return 1;
}

}  // namespace

extern "C" int focr_raster_bank(const char *font_path, float text_size, uint32_t x_bits,
                                uint32_t y_bits, int hinting, const uint32_t *alphabet,
                                size_t n_alphabet, int box_size, uint32_t x_padding,
                                uint32_t y_padding, focr_bank_t *out, char *err, size_t errlen) {
    if (!font_path || !alphabet || !n_alphabet || !out) return fail(err, errlen, "bad arguments");
    if (x_bits > 8 || y_bits > 8) return fail(err, errlen, "x_bits / y_bits too large");
    Face f;
    if (FT_Init_FreeType(&f.lib) != 0) return fail(err, errlen, "FT_Init_FreeType failed");
    if (FT_New_Face(f.lib, font_path, 0, &f.face) != 0) return fail(err, errlen, "cannot open font");
    const float upem = (float)f.face->units_per_EM;
    const float to_px = (1.f / upem) * text_size;  // src/ncc.rs:579

    std::vector<FT_UInt> gids(n_alphabet);
    for (size_t i = 0; i < n_alphabet; i++) {
        gids[i] = FT_Get_Char_Index(f.face, alphabet[i]);
        if (gids[i] == 0) return fail(err, errlen, "alphabet character missing from font");  // unwrap() at :154
    }

    const size_t nx = (size_t)1 << x_bits, ny = (size_t)1 << y_bits;
    const float x_div = 1.f / (float)nx, y_div = 1.f / (float)ny;  // src/ncc.rs:565-566

    std::vector<focr_template_t> templates;
    std::vector<uint8_t> needles;

    for (size_t sx = 0; sx < nx; sx++)
        for (size_t sy = 0; sy < ny; sy++) {  // x-major, src/ncc.rs:567-571
            const float off[2] = {(float)sx * x_div, (float)sy * y_div};
            float y_offset = 0.f;
            bool have_size = false;
            int cw = 0, ch = 0;
            if (box_size == FOCR_BOX_FONT) {  // src/ncc.rs:589-599
                RectF bbox{(float)f.face->bbox.xMin, (float)f.face->bbox.yMin, (float)f.face->bbox.xMax,
                           (float)f.face->bbox.yMax};
                RectI r = round_out(scale(bbox, to_px));
                cw = r.width();
                ch = r.height();
                y_offset = std::ceil((float)f.face->ascender * to_px);
                have_size = true;
            } else if (box_size == FOCR_BOX_ALPHABET) {  // src/ncc.rs:600-626
                RectF bounds;
                for (size_t i = 0; i < n_alphabet; i++) {
                    RectF tb;
                    if (!f.typographic_bounds(gids[i], &tb)) return fail(err, errlen, "glyph load failed");
                    RectF gb = scale(tb, to_px);
                    float bearing_y = gb.oy + gb.height();
                    RectI rr;
                    if (!f.raster_bounds(gids[i], text_size, off[0], off[1], &rr))
                        return fail(err, errlen, "glyph load failed");
                    y_offset = std::fmax(y_offset, std::ceil(bearing_y));
                    bounds = union_rect(bounds, RectF{(float)rr.ox, (float)rr.oy, (float)rr.lx, (float)rr.ly});
                }
                RectI r = round_out(bounds);
                cw = r.width();
                ch = r.height();
                have_size = true;
            }
            const float corrected[2] = {off[0], off[1] + y_offset};  // src/ncc.rs:629

            for (size_t i = 0; i < n_alphabet; i++) {  // render(), src/ncc.rs:143-196
                RectI rb;
                if (!f.raster_bounds(gids[i], text_size, corrected[0], corrected[1], &rb))
                    return fail(err, errlen, "glyph load failed");
                int w = (have_size ? cw : rb.width()) + 2 * (int)x_padding;
                int h = (have_size ? ch : rb.height()) + 2 * (int)y_padding;
                float origin_x = have_size ? 0.f : -(float)rb.ox;
                float origin_y = have_size ? 0.f : -(float)rb.oy;
                if (w < 0) w = 0;
                if (h < 0) h = 0;
                if (w > 0xffff || h > 0xffff) return fail(err, errlen, "canvas too large");
                std::vector<uint8_t> canvas((size_t)w * (size_t)h, 0);

                // transform vector = origin + padding + pos
                float tvx = origin_x + (float)x_padding + corrected[0];
                float tvy = origin_y + (float)y_padding + corrected[1];
                FT_Vector delta;
                delta.x = (FT_Pos)(int32_t)(tvx * 64.0f);
                delta.y = -(FT_Pos)(int32_t)(tvy * 64.0f);
                FT_Matrix shape{65536, 0, 0, 65536};
                FT_Set_Transform(f.face, &shape, &delta);
                if (FT_Set_Char_Size(f.face, (FT_F26Dot6)(int32_t)(text_size * 64.0f), 0, 0, 0) != 0)
                    return fail(err, errlen, "FT_Set_Char_Size failed");
                FT_Int32 flags = FT_LOAD_DEFAULT | FT_LOAD_RENDER;
                flags |= hinting ? FT_LOAD_TARGET_NORMAL : (FT_LOAD_TARGET_NORMAL | FT_LOAD_NO_HINTING);
                if (FT_Load_Glyph(f.face, gids[i], flags) != 0) return fail(err, errlen, "FT_Load_Glyph failed");
                const FT_GlyphSlot slot = f.face->glyph;
                const FT_Bitmap &bm = slot->bitmap;
                if (bm.buffer && bm.width && bm.rows) {
                    if (bm.pixel_mode != FT_PIXEL_MODE_GRAY) return fail(err, errlen, "unexpected pixel mode");
                    int dx = slot->bitmap_left, dy = -slot->bitmap_top;
                    for (int y = 0; y < (int)bm.rows; y++) {
                        int cy = dy + y;
                        if (cy < 0 || cy >= h) continue;
                        const uint8_t *src = bm.buffer + (ptrdiff_t)y * bm.pitch;
                        for (int x = 0; x < (int)bm.width; x++) {
                            int cx = dx + x;
                            if (cx < 0 || cx >= w) continue;
                            canvas[(size_t)cy * w + cx] = src[x];
                        }
                    }
                }
                f.reset_size();

                RectF tb;
                f.typographic_bounds(gids[i], &tb);
                focr_template_t t{};
                t.letter = alphabet[i];
                t.n_w = (uint16_t)w;
                t.n_h = (uint16_t)h;
                t.offset = (uint32_t)needles.size();
                t.shift_x = (uint16_t)sx;
                t.shift_y = (uint16_t)sy;
                t.off_x = off[0];
                t.off_y = off[1];
                t.corrected_off_y = corrected[1];
                t.bearing_x = scale(tb, to_px).ox;  // src/ncc.rs:671-673
                templates.push_back(t);
                needles.insert(needles.end(), canvas.begin(), canvas.end());
            }
        }

    // advance of the first alphabet glyph (font.advance * to_px, src/ncc.rs:807)
    f.reset_size();
    float advance_px = 0.f;
    if (FT_Load_Glyph(f.face, gids[0], FT_LOAD_DEFAULT | FT_LOAD_NO_HINTING) == 0)
        advance_px = (float)f.face->glyph->metrics.horiAdvance / 64.0f * to_px;

    out->n_templates = templates.size();
    out->templates = (focr_template_t *)malloc(sizeof(focr_template_t) * (templates.size() ? templates.size() : 1));
    out->needles_len = needles.size();
    out->needles = (uint8_t *)malloc(needles.size() ? needles.size() : 1);
    if (!out->templates || !out->needles) return fail(err, errlen, "out of memory");
    memcpy(out->templates, templates.data(), sizeof(focr_template_t) * templates.size());
    memcpy(out->needles, needles.data(), needles.size());
    out->n_alphabet = (uint32_t)n_alphabet;
    out->x_bits = x_bits;
    out->y_bits = y_bits;
    out->text_size = text_size;
    out->advance_px = advance_px;
    return 0;
}

// font.metrics() as font-kit's FreeType loader reports it (src/ncc.rs:791-802 prints it under -v); from memory, unpinned
extern "C" int focr_font_metrics(const char *font_path, focr_font_metrics_t *out, char *err, size_t errlen) {
    auto fail = [&](const char *m) {
        if (err && errlen) snprintf(err, errlen, "%s", m);
        return 1;
    };
    if (!font_path || !out) return fail("focr_font_metrics: bad arguments");
    Face f;
    if (FT_Init_FreeType(&f.lib) != 0) return fail("FT_Init_FreeType failed");
    if (FT_New_Face(f.lib, font_path, 0, &f.face) != 0) return fail("cannot open font");  // Font::from_path(..).unwrap(), src/ncc.rs:792
    const FT_Face fc = f.face;
    memset(out, 0, sizeof *out);
    out->units_per_em = fc->units_per_EM;
    out->ascent = (float)fc->ascender;
    out->descent = (float)fc->descender;
    out->line_gap = (float)(fc->height + fc->descender - fc->ascender);
    out->underline_position = (float)(fc->underline_position + fc->underline_thickness / 2);
    out->underline_thickness = (float)fc->underline_thickness;
    if (const TT_OS2 *os2 = (const TT_OS2 *)FT_Get_Sfnt_Table(fc, FT_SFNT_OS2)) {
        out->cap_height = (float)os2->sCapHeight;
        out->x_height = (float)os2->sxHeight;
    }
    out->bbox[0] = (float)fc->bbox.xMin;
    out->bbox[1] = (float)fc->bbox.yMin;
    out->bbox[2] = (float)fc->bbox.xMax;
    out->bbox[3] = (float)fc->bbox.yMax;
    return 0;
}

// ---- the `focr` line decoder's host side (include/focr_decode.h; src/main.rs) ---------------------------------------

namespace {

struct Bitmap {  // one FreeType rendering: bitmap_left, -bitmap_top, rows of `w` bytes
    int left = 0, top = 0, w = 0, h = 0;
    std::vector<uint8_t> px;
};

// rasterize_glyph for a pure translation given as FreeType's 26.6 delta (y already negated)
bool render_delta(Face &f, FT_UInt gid, float size, int hinting, FT_Pos dx, FT_Pos dy, Bitmap *out) {
    FT_Vector delta{dx, dy};
    FT_Matrix shape{65536, 0, 0, 65536};
    FT_Set_Transform(f.face, &shape, &delta);
    bool ok = FT_Set_Char_Size(f.face, (FT_F26Dot6)(int32_t)(size * 64.0f), 0, 0, 0) == 0;
    FT_Int32 flags = FT_LOAD_DEFAULT | FT_LOAD_RENDER;
    flags |= hinting ? FT_LOAD_TARGET_NORMAL : (FT_LOAD_TARGET_NORMAL | FT_LOAD_NO_HINTING);
    ok = ok && FT_Load_Glyph(f.face, gid, flags) == 0;
    if (ok) {
        const FT_GlyphSlot slot = f.face->glyph;
        const FT_Bitmap &bm = slot->bitmap;
        out->left = slot->bitmap_left;
        out->top = -slot->bitmap_top;
        out->w = out->h = 0;
        out->px.clear();
        if (bm.buffer && bm.width && bm.rows) {
            ok = bm.pixel_mode == FT_PIXEL_MODE_GRAY;
            out->w = (int)bm.width;
            out->h = (int)bm.rows;
            out->px.resize((size_t)out->w * out->h);
            for (int y = 0; ok && y < out->h; y++)
                memcpy(&out->px[(size_t)y * out->w], bm.buffer + (ptrdiff_t)y * bm.pitch, out->w);
        }
    }
    f.reset_size();
    return ok;
}

FT_Pos delta_of(float t) { return (FT_Pos)(int32_t)(t * 64.0f); }  // trunc(t * 64), as raster.cpp does for the bank

// Canvas::blit_from: copy (not blend), clipped
void blit(const Bitmap &b, int x0, int y0, uint8_t *canvas, size_t w, size_t h) {
    for (int y = 0; y < b.h; y++) {
        long cy = (long)y0 + y;
        if (cy < 0 || cy >= (long)h) continue;
        for (int x = 0; x < b.w; x++) {
            long cx = (long)x0 + x;
            if (cx < 0 || cx >= (long)w) continue;
            canvas[(size_t)cy * w + cx] = b.px[(size_t)y * b.w + x];
        }
    }
}

// font.advance(gid).x in font units (loaded unhinted at char size = units_per_em, as font-kit keeps the face)
bool advance_units(Face &f, FT_UInt gid, float *out) {
    f.reset_size();
    if (FT_Load_Glyph(f.face, gid, FT_LOAD_DEFAULT | FT_LOAD_NO_HINTING) != 0) return false;
    *out = (float)f.face->glyph->advance.x / 64.0f;
    return true;
}

// font.advance(gid) / units_per_em * size * kern_x, f32, left to right (src/main.rs:52-54, 177-179)
float increment_of(float advance, float upem, float size, float kerning) { return advance / upem * size * kerning; }

// One open face per thread and font path, for callers that rasterise glyph by glyph (the test model).
struct CachedFace {
    std::string path;
    Face f;
};
thread_local CachedFace *g_cached = nullptr;

Face *cached_face(const char *path) {
    if (g_cached && g_cached->path == path) return &g_cached->f;
    delete g_cached;
    g_cached = new CachedFace;
    g_cached->path = path;
    if (FT_Init_FreeType(&g_cached->f.lib) != 0 || FT_New_Face(g_cached->f.lib, path, 0, &g_cached->f.face) != 0) {
        delete g_cached;
        g_cached = nullptr;
        return nullptr;
    }
    return &g_cached->f;
}

bool open_face(Face &f, const char *path) {
    return FT_Init_FreeType(&f.lib) == 0 && FT_New_Face(f.lib, path, 0, &f.face) == 0;
}

}  // namespace

extern "C" int focr_raster_glyph(const char *font_path, float text_size, int hinting, uint32_t codepoint, float tx,
                                 float ty, uint8_t *canvas, size_t w, size_t h, char *err, size_t errlen) {
    if (!font_path || (!canvas && w && h)) return fail(err, errlen, "focr_raster_glyph: bad arguments");
    Face *f = cached_face(font_path);
    if (!f) return fail(err, errlen, "cannot open font");
    FT_UInt gid = FT_Get_Char_Index(f->face, codepoint);
    if (gid == 0) return fail(err, errlen, "character missing from font");
    Bitmap b;
    if (!render_delta(*f, gid, text_size, hinting, delta_of(tx), -delta_of(ty), &b))
        return fail(err, errlen, "FT_Load_Glyph failed");
    blit(b, b.left, b.top, canvas, w, h);
    return 0;
}

extern "C" int focr_glyph_metrics(const char *font_path, float text_size, uint32_t codepoint, float *advance,
                                  uint32_t *units_per_em, int32_t bounds[4], char *err, size_t errlen) {
    if (!font_path || !advance || !units_per_em || !bounds) return fail(err, errlen, "focr_glyph_metrics: bad arguments");
    Face *f = cached_face(font_path);
    if (!f) return fail(err, errlen, "cannot open font");
    FT_UInt gid = FT_Get_Char_Index(f->face, codepoint);
    if (gid == 0) return fail(err, errlen, "character missing from font");
    RectI r;
    if (!advance_units(*f, gid, advance) || !f->raster_bounds(gid, text_size, 0.f, 0.f, &r))
        return fail(err, errlen, "glyph load failed");
    *units_per_em = f->face->units_per_EM;
    bounds[0] = r.ox, bounds[1] = r.oy, bounds[2] = r.lx, bounds[3] = r.ly;
    return 0;
}

extern "C" int focr_render_text(const char *font_path, float text_size, int hinting, float kerning, const uint32_t *text,
                                size_t n, uint8_t **canvas, size_t *w, size_t *h, char *err, size_t errlen) {
    if (!font_path || (!text && n) || !canvas || !w || !h) return fail(err, errlen, "focr_render_text: bad arguments");
    *canvas = nullptr;
    Face f;
    if (!open_face(f, font_path)) return fail(err, errlen, "cannot open font");
    const float upem = (float)f.face->units_per_EM;
    std::vector<FT_UInt> gids(n);
    std::vector<float> pos(n);
    float pen = 0.f;
    for (size_t i = 0; i < n; i++) {  // src/main.rs:48-55
        gids[i] = FT_Get_Char_Index(f.face, text[i]);
        if (gids[i] == 0) return fail(err, errlen, "character missing from font");  // glyph_for_char(..).unwrap()
        pos[i] = pen;
        float adv;
        if (!advance_units(f, gids[i], &adv)) return fail(err, errlen, "glyph load failed");
        pen = pen + increment_of(adv, upem, text_size, kerning);
    }
    RectF bounds;  // src/main.rs:57-70: the fold starts from the empty rect at (0, 0)
    for (size_t i = 0; i < n; i++) {
        RectI r;
        if (!f.raster_bounds(gids[i], text_size, pos[i], 0.f, &r)) return fail(err, errlen, "glyph load failed");
        bounds = union_rect(bounds, RectF{(float)r.ox, (float)r.oy, (float)r.lx, (float)r.ly});
    }
    // bounds.round().to_i32().size()
    const long cw = std::lround(bounds.lx) - std::lround(bounds.ox), ch = std::lround(bounds.ly) - std::lround(bounds.oy);
    if (cw < 0 || ch < 0 || cw > 1 << 20 || ch > 1 << 16) return fail(err, errlen, "canvas too large");
    *w = (size_t)cw;
    *h = (size_t)ch;
    *canvas = (uint8_t *)calloc((size_t)cw * ch + 1, 1);
    if (!*canvas) return fail(err, errlen, "out of memory");
    for (size_t i = 0; i < n; i++) {  // src/main.rs:74-83: translation -bounds.origin + pos
        Bitmap b;
        if (!render_delta(f, gids[i], text_size, hinting, delta_of(-bounds.ox + pos[i]), -delta_of(-bounds.oy + 0.f), &b)) {
            free(*canvas);
            *canvas = nullptr;
            return fail(err, errlen, "FT_Load_Glyph failed");
        }
        blit(b, b.left, b.top, *canvas, *w, *h);
    }
    return 0;
}

namespace {

// What both tables of an alphabet start from: the open face, the glyph ids and the line origin of decode_line
struct Alphabet {
    Face f;
    std::vector<FT_UInt> gids;
    float upem = 0.f, origin_x = 0.f, origin_y = 0.f;
};

int open_alphabet(const char *font_path, float text_size, float kerning, const uint32_t *alphabet, size_t n_alphabet, Alphabet *a,
                  char *err, size_t errlen) {
    // DIVERGENCE: the reference's pen loop never ends for kerning <= 0 or a glyph that does not advance
    if (!(kerning > 0.f)) return fail(err, errlen, "kerning must be > 0 (the reference never finishes a line otherwise)");
    if (!open_face(a->f, font_path)) return fail(err, errlen, "cannot open font");
    a->upem = (float)a->f.face->units_per_EM;
    a->gids.resize(n_alphabet);
    RectF bbox;  // src/main.rs:136-147: union of raster_bounds(identity), folded from the empty rect at (0, 0)
    for (size_t i = 0; i < n_alphabet; i++) {
        a->gids[i] = FT_Get_Char_Index(a->f.face, alphabet[i]);
        if (a->gids[i] == 0) {
            char m[96];
            snprintf(m, sizeof m, "alphabet character U+%04X missing from font", (unsigned)alphabet[i]);
            return fail(err, errlen, m);
        }
        RectI r;
        if (!a->f.raster_bounds(a->gids[i], text_size, 0.f, 0.f, &r)) return fail(err, errlen, "glyph load failed");
        bbox = union_rect(bbox, RectF{(float)r.ox, (float)r.oy, (float)r.lx, (float)r.ly});
    }
    a->origin_x = -bbox.ox;
    a->origin_y = -bbox.oy;
    return 0;
}

// glyph i's pen increment, refused if it does not advance the pen
int glyph_increment(Alphabet &a, size_t i, uint32_t codepoint, float text_size, float kerning, float *inc, char *err, size_t errlen) {
    float adv;
    if (!advance_units(a.f, a.gids[i], &adv)) return fail(err, errlen, "glyph load failed");
    *inc = increment_of(adv, a.upem, text_size, kerning);
    if (!(*inc > 0.f)) {
        char m[128];
        snprintf(m, sizeof m, "glyph of U+%04X does not advance the pen (the reference never finishes a line)", (unsigned)codepoint);
        return fail(err, errlen, m);
    }
    return 0;
}

// The 64 phases of glyph i (26.6 delta x = p, delta y of the line origin) and the box they share
struct Phases {
    std::vector<Bitmap> ph = std::vector<Bitmap>(FOCR_DECODE_PHASES);
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
};

// FreeType's delta y of the line origin: origin + pos, pos.y = 0
FT_Pos origin_dy(const Alphabet &a) { return -delta_of(a.origin_y + 0.f); }

int render_phases(Alphabet &a, size_t i, float text_size, int hinting, FT_Pos dy, Phases *out, char *err, size_t errlen) {
    bool any = false;
    for (int p = 0; p < FOCR_DECODE_PHASES; p++) {
        if (!render_delta(a.f, a.gids[i], text_size, hinting, p, dy, &out->ph[p])) return fail(err, errlen, "FT_Load_Glyph failed");
        const Bitmap &b = out->ph[p];
        if (!b.w || !b.h) continue;
        out->x0 = any ? std::min(out->x0, b.left) : b.left;
        out->y0 = any ? std::min(out->y0, b.top) : b.top;
        out->x1 = any ? std::max(out->x1, b.left + b.w) : b.left + b.w;
        out->y1 = any ? std::max(out->y1, b.top + b.h) : b.top + b.h;
        any = true;
    }
    return 0;
}

// The decode font of an open alphabet with every phase rendered at FreeType's delta y = dy
int build_decode_font(Alphabet &a, float text_size, int hinting, float kerning, const uint32_t *alphabet, size_t n_alphabet, FT_Pos dy,
                      focr_decode_font_t *out, char *err, size_t errlen) {
    std::vector<focr_decode_glyph_t> glyphs(n_alphabet);
    std::vector<uint8_t> bitmaps;
    float min_inc = 0.f;
    for (size_t i = 0; i < n_alphabet; i++) {
        focr_decode_glyph_t &g = glyphs[i];
        memset(&g, 0, sizeof g);
        g.codepoint = alphabet[i];
        if (glyph_increment(a, i, alphabet[i], text_size, kerning, &g.increment, err, errlen)) return 1;
        min_inc = i == 0 ? g.increment : std::fmin(min_inc, g.increment);
        Phases ph;
        if (render_phases(a, i, text_size, hinting, dy, &ph, err, errlen)) return 1;
        g.box_w = (uint32_t)(ph.x1 - ph.x0);
        g.box_h = (uint32_t)(ph.y1 - ph.y0);
        g.stride = (g.box_w + 3) & ~3u;
        // the device keeps sum c^2 and sum c*r of a glyph in 32 bits: score = sum c^2 - 2 sum c*r, |score| <= 2 * 255^2 * area
        if ((uint64_t)g.stride * g.box_h * 2 * 255 * 255 >= (1ull << 31)) return fail(err, errlen, "glyph box too large for the decoder");
        g.offset = bitmaps.size();
        bitmaps.resize(bitmaps.size() + (size_t)FOCR_DECODE_PHASES * g.stride * g.box_h, 0);
        for (int p = 0; p < FOCR_DECODE_PHASES; p++) {
            g.off_x[p] = ph.x0;
            g.off_y[p] = ph.y0;
            const Bitmap &b = ph.ph[p];
            uint8_t *dst = bitmaps.data() + g.offset + (size_t)p * g.stride * g.box_h;
            for (int y = 0; y < b.h; y++)
                memcpy(dst + (size_t)(b.top - ph.y0 + y) * g.stride + (b.left - ph.x0), &b.px[(size_t)y * b.w], b.w);
        }
    }
    out->glyphs = (focr_decode_glyph_t *)malloc(sizeof(focr_decode_glyph_t) * n_alphabet);
    out->bitmaps = (uint8_t *)malloc(bitmaps.size() ? bitmaps.size() : 1);
    if (!out->glyphs || !out->bitmaps) {
        focr_decode_font_free(out);
        return fail(err, errlen, "out of memory");
    }
    memcpy(out->glyphs, glyphs.data(), sizeof(focr_decode_glyph_t) * n_alphabet);
    if (!bitmaps.empty()) memcpy(out->bitmaps, bitmaps.data(), bitmaps.size());
    out->n_glyphs = n_alphabet;
    out->bitmaps_len = bitmaps.size();
    out->origin_x = a.origin_x;
    out->origin_y = a.origin_y;
    out->text_size = text_size;
    out->kerning = kerning;
    out->hinting = hinting;
    out->min_increment = min_inc;
    return 0;
}

}  // namespace

extern "C" int focr_decode_font_build(const char *font_path, float text_size, int hinting, float kerning,
                                      const uint32_t *alphabet, size_t n_alphabet, focr_decode_font_t *out, char *err,
                                      size_t errlen) {
    if (!font_path || !alphabet || !n_alphabet || !out) return fail(err, errlen, "focr_decode_font_build: bad arguments");
    memset(out, 0, sizeof *out);
    Alphabet a;
    if (open_alphabet(font_path, text_size, kerning, alphabet, n_alphabet, &a, err, errlen)) return 1;
    return build_decode_font(a, text_size, hinting, kerning, alphabet, n_alphabet, origin_dy(a), out, err, errlen);
}

extern "C" int focr_decode_font_build_y(const char *font_path, float text_size, int hinting, float kerning,
                                        const uint32_t *alphabet, size_t n_alphabet, uint32_t y_bits, focr_decode_font_t *out,
                                        char *err, size_t errlen) {
    if (!font_path || !alphabet || !n_alphabet || !out) return fail(err, errlen, "focr_decode_font_build_y: bad arguments");
    if (y_bits > FOCR_BASELINE_Y_BITS_MAX) return fail(err, errlen, "focr_decode_font_build_y: y_bits is at most 3");
    const uint32_t n_v = 1u << y_bits;
    memset(out, 0, sizeof *out * n_v);
    Alphabet a;
    if (open_alphabet(font_path, text_size, kerning, alphabet, n_alphabet, &a, err, errlen)) return 1;
    for (uint32_t v = 0; v < n_v; v++) {  // v * 2^-B and the sum are exact in f32 for a whole origin_y
        const float ty = a.origin_y + (float)v / (float)n_v;
        if (build_decode_font(a, text_size, hinting, kerning, alphabet, n_alphabet, -delta_of(ty), &out[v], err, errlen)) {
            for (uint32_t u = 0; u <= v; u++) focr_decode_font_free(&out[u]);
            return 1;
        }
    }
    return 0;
}

extern "C" void focr_decode_font_free(focr_decode_font_t *font) {
    if (!font) return;
    free(font->glyphs);
    free(font->bitmaps);
    memset(font, 0, sizeof *font);
}

// The learned font (../hip/learn_font.h has the rule): base's records and the learned bitmaps, in tables of its own.
extern "C" int focr_decode_font_learn(const focr_decode_font_t *base, const uint64_t *sums, const uint64_t *counts, uint32_t min_count, uint32_t grow,
                                      focr_decode_font_t *out, size_t *learned, size_t *inked, char *err, size_t errlen) {
    if (!base || !out) return fail(err, errlen, "focr_decode_font_learn: bad arguments");
    std::vector<uint8_t> bitmaps;
    focr_dec::LearnStats stats;
    const std::string no = focr_dec::learn_font_bitmaps(*base, sums, counts, min_count, grow, &bitmaps, &stats);
    if (!no.empty()) return fail(err, errlen, ("focr_decode_font_learn: " + no).c_str());
    *out = *base;
    out->glyphs = (focr_decode_glyph_t *)malloc(sizeof(focr_decode_glyph_t) * (base->n_glyphs ? base->n_glyphs : 1));
    out->bitmaps = (uint8_t *)malloc(bitmaps.size() ? bitmaps.size() : 1);
    if (!out->glyphs || !out->bitmaps) {
        focr_decode_font_free(out);
        return fail(err, errlen, "out of memory");
    }
    if (base->n_glyphs) memcpy(out->glyphs, base->glyphs, sizeof(focr_decode_glyph_t) * base->n_glyphs);
    if (!bitmaps.empty()) memcpy(out->bitmaps, bitmaps.data(), bitmaps.size());
    if (learned) *learned = stats.learned;
    if (inked) *inked = stats.inked;
    return 0;
}

extern "C" int focr_verify_font_build(const char *font_path, float text_size, int hinting, float kerning,
                                      const uint32_t *alphabet, size_t n_alphabet, focr_verify_font_t *out, char *err,
                                      size_t errlen) {
    if (!font_path || !alphabet || !n_alphabet || !out) return fail(err, errlen, "focr_verify_font_build: bad arguments");
    memset(out, 0, sizeof *out);
    Alphabet a;
    if (open_alphabet(font_path, text_size, kerning, alphabet, n_alphabet, &a, err, errlen)) return 1;
    std::vector<focr_verify_glyph_t> glyphs(n_alphabet);
    for (size_t i = 0; i < n_alphabet; i++) {
        focr_verify_glyph_t &g = glyphs[i];
        memset(&g, 0, sizeof g);
        g.codepoint = alphabet[i];
        if (glyph_increment(a, i, alphabet[i], text_size, kerning, &g.increment, err, errlen)) return 1;
        RectF box;
        if (!a.f.raster_box(a.gids[i], text_size, &box)) return fail(err, errlen, "glyph load failed");
        g.box[0] = box.ox, g.box[1] = box.oy, g.box[2] = box.lx, g.box[3] = box.ly;
        Phases ph;
        if (render_phases(a, i, text_size, hinting, origin_dy(a), &ph, err, errlen)) return 1;
        for (int p = 0; p < FOCR_DECODE_PHASES; p++) {  // an empty bitmap is the empty rectangle at the box's corner
            const Bitmap &b = ph.ph[p];
            const bool ink = b.w && b.h;
            g.rect_x[p] = ink ? (uint32_t)(b.left - ph.x0) : 0;
            g.rect_y[p] = ink ? (uint32_t)(b.top - ph.y0) : 0;
            g.rect_w[p] = ink ? (uint32_t)b.w : 0;
            g.rect_h[p] = ink ? (uint32_t)b.h : 0;
        }
    }
    out->glyphs = (focr_verify_glyph_t *)malloc(sizeof(focr_verify_glyph_t) * n_alphabet);
    if (!out->glyphs) return fail(err, errlen, "out of memory");
    memcpy(out->glyphs, glyphs.data(), sizeof(focr_verify_glyph_t) * n_alphabet);
    out->n_glyphs = n_alphabet;
    out->origin_y = a.origin_y;
    out->text_size = text_size;
    out->kerning = kerning;
    out->hinting = hinting;
    return 0;
}

extern "C" void focr_verify_font_free(focr_verify_font_t *font) {
    if (!font) return;
    free(font->glyphs);
    memset(font, 0, sizeof *font);
}
