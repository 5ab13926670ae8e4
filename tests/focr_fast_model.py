"""A fast, exact restatement of the reference's focr decoder for the tests, from the 64-phase table.

It decodes a line as tests/focr_line_model.py does (the first minimum of the full-canvas SSD wins, the pen advances by
the f32 increment), but takes each candidate's raster from DecodeFont.phase instead of calling FreeType again.  At a
pen step the delta is trunc((origin_x + pos) * 64) in f32, as FreeType receives it; its phase selects one bitmap per
glyph and its whole-pixel shift places them.  Every glyph is scored at once in int64 over the canvas: inside the part
of the glyph box that lies on the canvas, (r - c)^2; everywhere else on the canvas, r^2.  Off-canvas pixels of a glyph
do not count.  Nothing here comes from the device path.

The phases are built on first use and kept as uint8 stacks (one per phase, all glyphs in one frame), widened to int64
only on the canvas window of each step: at sizes near the decoder's bound all 64 int64 stacks would not fit in memory.
tests/test_focr_fast_model.py proves it equal to the brute-force model on every configuration the GPU tests use.
"""
import numpy as np

from font_ocr_amd.decoder import DecodeFont, raster_glyph

F32 = np.float32


class FastModel:
    """decode_line / decode_image of one (font, size, alphabet, hinting, kerning), from its DecodeFont."""

    def __init__(self, font_path, text_size, alphabet, hinting=False, kerning=1.0):
        self.alphabet = alphabet
        self.font = DecodeFont(font_path, text_size, alphabet, hinting, kerning)
        self.ox = self.font.origin[0]
        self.incs = self.font.increments()
        self._phases = {}

    def _phase(self, p):
        """(stack G x FH x FW uint8, frame top fy, frame left fx at shift 0) of phase p: each glyph's bitmap placed at
        its (off_x, off_y) in one frame that holds them all."""
        if p not in self._phases:
            ph = [self.font.phase(i, p) for i in range(len(self.alphabet))]
            fy0 = min(oy for _, _, oy in ph)
            fx0 = min(ox for _, ox, _ in ph)
            fy1 = max(oy + bm.shape[0] for bm, _, oy in ph)
            fx1 = max(ox + bm.shape[1] for bm, ox, _ in ph)
            st = np.zeros((len(ph), fy1 - fy0, fx1 - fx0), dtype=np.uint8)
            for i, (bm, ox, oy) in enumerate(ph):
                st[i, oy - fy0: oy - fy0 + bm.shape[0], ox - fx0: ox - fx0 + bm.shape[1]] = bm
            self._phases[p] = (st, fy0, fx0)
        return self._phases[p]

    def scores(self, r, pos):
        """Full-canvas SSD of every glyph at pen position pos on the inverted line r (h x w int64)."""
        h, w = r.shape
        total = int((r * r).sum())
        d = int(F32(F32(self.ox + F32(pos)) * F32(64)))  # trunc: origin_x >= 0 and pos >= 0
        st, fy0, fx0 = self._phase(d & 63)
        sx = (d >> 6) + fx0
        y0, y1 = max(0, fy0), min(h, fy0 + st.shape[1])
        x0, x1 = max(0, sx), min(w, sx + st.shape[2])
        if y0 >= y1 or x0 >= x1:
            return np.full(st.shape[0], total, dtype=np.int64)
        win = r[y0:y1, x0:x1]
        c = st[:, y0 - fy0: y1 - fy0, x0 - sx: x1 - sx].astype(np.int64)
        return ((win - c) ** 2).sum(axis=(1, 2)) + (total - int((win * win).sum()))

    def decode_line(self, ref):
        """decode_line on one cropped luma line (h x w uint8) -> the text."""
        h, w = ref.shape
        r = 255 - ref.astype(np.int64)
        pos, out = F32(0), []
        while pos < F32(w):
            i = int(np.argmin(self.scores(r, pos)))  # the first minimum
            out.append(self.alphabet[i])
            pos = F32(pos + self.incs[i])
        return "".join(out)

    def decode_image(self, page, x, y, width, line_height, line_advance):
        """decode_image: [(y, text)] of every non-blank line, crops clamped as image::DynamicImage::crop_imm does."""
        out = []
        i = 0
        while True:
            ly = y + i * line_advance
            i += 1
            line = crop(page, x, ly, width, line_height)
            if line.shape[0] == 0:
                return out
            if np.all(line == 255):
                continue
            out.append((ly, self.decode_line(line)))

    def close(self):
        self._phases = {}
        self.font.close()


def crop(page, x, y, width, height):
    """image::DynamicImage::crop_imm's clamping."""
    H, W = page.shape
    x, y = min(x, W), min(y, H)
    return page[y: y + min(height, H - y), x: x + min(width, W - x)]


ASCII95 = "".join(chr(c) for c in range(32, 127))
# 319 glyphs: ASCII95, U+00A0 .. U+017B, and look-alikes that DejaVu draws exactly as Latin letters
ALPHABET_319 = ASCII95 + "".join(chr(c) for c in range(0xA0, 0x17C)) + "\u0391\u03bf\u0410\u043e"
# glyphs identical in every phase and increment (tests/test_focr_fast_model.py checks it), first listed in ALPHABET_319 first
TIE_GROUPS = ("A\u0391\u0410", "o\u03bf\u043e", " \u00a0")
# the largest sizes focr_decode_font_build accepts (its int32 score bound), on a whole-pixel grid
LARGEST_SIZE = {("DejaVuSansMono.ttf", "default"): 191.0, ("DejaVuSansMono.ttf", "ascii95"): 182.0,
                ("DejaVuSansMono.ttf", "319"): 168.0, ("DejaVuSans.ttf", "default"): 154.0,
                ("DejaVuSans.ttf", "ascii95"): 146.0, ("DejaVuSans.ttf", "319"): 137.0}


def permuted_319(seed=3):
    """ALPHABET_319 shuffled, with each tie group on one lane of the device's argmin in consecutive 64-glyph stripes
    (indices i, i + 64, i + 128) and listed in another order than in ALPHABET_319: Cyrillic A, Latin A, Greek Alpha at
    5, 69, 133; Greek omicron, Cyrillic o, Latin o at 10, 74, 138; U+00A0 and U+0020 at 20 and 276."""
    fixed = {5: "\u0410", 69: "A", 133: "\u0391", 10: "\u03bf", 74: "\u043e", 138: "o", 20: "\u00a0", 276: " "}
    rest = [c for c in ALPHABET_319 if c not in fixed.values()]
    rest = [rest[i] for i in np.random.default_rng(seed).permutation(len(rest))]
    out = [fixed[i] if i in fixed else rest.pop() for i in range(len(ALPHABET_319))]
    return "".join(out)


def line_cap(increments, w):
    """The decoder's characters-per-line bound for a crop of width w: steps of the smallest increment from 0 to w in f32."""
    m, p, n = F32(np.min(increments)), F32(0), 0
    while p < F32(w):
        p = F32(p + m)
        n += 1
    return max(n, 1)


def narrowest_glyph_line(font_path, text_size, alphabet, w, h=16):
    """A w-px line of the alphabet's narrowest glyph, each copy drawn with FreeType at the decoder's own pen position
    (kerning 1.0, unhinted).  Returns (h x w luma page, the glyph, line_cap of the alphabet for w)."""
    f = DecodeFont(font_path, text_size, alphabet)
    inc, (ox, oy) = f.increments(), f.origin
    f.close()
    ch, m = alphabet[int(np.argmin(inc))], F32(inc.min())
    page = np.full((h, w), 255, dtype=np.uint8)
    pos = F32(0)
    while pos < F32(w):
        g = np.zeros((h, w), dtype=np.uint8)
        raster_glyph(font_path, text_size, ch, F32(ox + pos), oy, g)
        page = np.minimum(page, 255 - g)
        pos = F32(pos + m)
    return page, ch, line_cap(inc, w)
