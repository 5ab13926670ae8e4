"""Host side of focr_decoder_learn_text and focr_decode_font_learn (include/focr_decode.h): the entry points declared, bound and
exported, the header's definition, LineDecoder.learn_text's and DecodeFont.learned's signatures and the refusals they make before
they touch a device, LearnedGlyphs' sum, the learned font on the host against the numpy restatement, and the CLI's usage errors
and --help lines before it touches a device.  No GPU needed."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import focr_learn_model as L
from font_ocr_amd import DecodeFont, LearnedGlyphs, LineDecoder
from font_ocr_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MONO = os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")
FOCR = os.path.join(ROOT, "font_ocr_amd", "bin", "focr")
SYMBOLS = {"focr_decoder_learn_text": (r"int", r"\(focr_decoder_t \*dec, const uint8_t \*pages, int pages_on_device, size_t n_pages,\s*"
                                       r"size_t page_w, size_t page_h, uint32_t x_start, uint32_t width, uint32_t line_height,\s*"
                                       r"const focr_text_line_t \*lines, size_t n_lines,\s*"
                                       r"const uint16_t \*chars, const uint32_t \*pens, const int8_t \*offsets, const uint8_t \*use, size_t n_chars,\s*"
                                       r"uint32_t font, uint32_t \*sums, uint32_t \*counts, uint8_t \*used\);"),
           "focr_decoder_last_learn_text_ms": (r"float", r"\(const focr_decoder_t \*dec\);"),
           "focr_decoder_last_learn_text_launches": (r"uint32_t", r"\(const focr_decoder_t \*dec\);")}


def exported(lib):
    path = os.path.join(N.LIB_DIR, lib)
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "hip" if "hip" in lib else "raster"], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r" T (focr_\w+)", out))


def test_symbols_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "focr_decode.h")).read()
    hip = exported("libfocr_hip.so")
    for name, (ret, args) in SYMBOLS.items():
        assert re.search(r"\b%s\s+%s\s*%s" % (ret, name, args), header), name
        assert name in N.DECODE_HIP_SYMBOLS and len(N.DECODE_HIP_SYMBOLS[name][1]) == args.count(",") + 1, name
        assert name in hip, name
    assert header.index("focr_decoder_last_align_text_launches(const") < header.index("int focr_decoder_learn_text(") < header.index("device: test images")
    assert "focr_decode_font_learn" in exported("libfocr_raster.so") and len(N.DECODE_RASTER_SYMBOLS["focr_decode_font_learn"][1]) == 10
    assert re.search(r"int focr_decode_font_learn\(const focr_decode_font_t \*base, const uint64_t \*sums, const uint64_t \*counts, uint32_t min_count,\s*"
                     r"uint32_t grow, focr_decode_font_t \*out, size_t \*learned, size_t \*inked, char \*err, size_t errlen\);", header)
    # the definition: whom it is for, the placements, the font, the mask, the box, what is added, the outputs, refusals, state, scope
    flat = lambda text: re.sub(r"\s*\n \*\s*", " ", text)  # noqa: E731  (the comment's line breaks are not part of the definition)
    section = flat(header[header.index("device: glyph tables from a trusted reading"): header.index("int focr_decoder_learn_text(")])
    for word in ("TRUSTS", "a few corrected pages", "focr_decoder_score_text's at shift 0", "there is no line_q", "y-phase tables are not learned",
                 "lines[l].font == k", "contribute nothing", "it still moves the pen", "delta & 63", "delta >> 6", "shift + off_x[p]", "off_y[p]",
                 "wholly inside the crop", "no partial boxes", "counts[i * 64 + p]", "r = 255 - luma", "offset_i + (p * box_h + row) * stride + col",
                 "padding columns", "running sum of n_chars", "once per listing", "zeroed first", "before anything is launched", "NULL sums or NULL counts",
                 "a font to learn above K", "2^24 or more listed characters", "255 * 2^24", "buffers of its own", "needs no run", "What it does not do",
                 "y-phase tables;", "pooling of neighbouring phases", "weights", "an NCC bank", "untrusted reading", "reproduce that reading's errors",
                 "score margin does not help"):
        assert word in section, word
    learned = flat(header[header.index("The learned font (host"): header.index("int focr_decode_font_learn(")])
    for word in ("min_count >= 1", "has ink in base", "bounding rectangle", "grown by `grow`", "clipped to the box", "(2 * sum + n) / (2 * n)", "at most 255",
                 "A blank glyph stays blank", "verify table still matches", "below -line_base", "known limit", "focr_decode_font_free"):
        assert word in learned, word


def test_python_signatures_and_refusals():
    sig = inspect.signature(LineDecoder.learn_text)
    assert list(sig.parameters) == ["self", "luma_pages", "lines", "x", "width", "line_height", "fonts", "pens", "offsets", "use", "font"]
    assert [sig.parameters[p].default for p in ("fonts", "pens", "offsets", "use", "font")] == [None, None, None, None, 0]
    sig = inspect.signature(DecodeFont.learned)
    assert list(sig.parameters) == ["self", "glyphs", "min_count", "grow"] and (sig.parameters["min_count"].default, sig.parameters["grow"].default) == (1, 0)
    assert LearnedGlyphs._fields == ("sums", "counts", "used")
    dec = object.__new__(LineDecoder)  # no device: these refusals come before anything touches the library

    class Font:
        alphabet = "ab c"

    dec.font, dec._candidates = None, []
    page = np.full((16, 40), 255, dtype=np.uint8)
    with pytest.raises(RuntimeError, match=r"set_font\(\) first"):
        dec.learn_text([page], [[(0, "ab")]], 0, 40, 16)
    dec.font, dec._candidates = Font(), [object()]
    with pytest.raises(ValueError, match="pens or offsets, not both"):
        dec.learn_text([page], [[(0, "ab")]], 0, 40, 16, pens=[[[0, 64]]], offsets=[[[0, 0]]])
    for bad in (-1, 2):
        with pytest.raises(ValueError, match=r"font must be 0 \.\. 1"):
            dec.learn_text([page], [[(0, "ab")]], 0, 40, 16, font=bad)
    for w, lh in ((0, 16), (40, 0)):
        with pytest.raises(ValueError, match="width and line_height must be positive"):
            dec.learn_text([page], [[(0, "ab")]], 0, w, lh)
    with pytest.raises(ValueError, match="one list per page"):
        dec.learn_text([page], [[(0, "ab")], []], 0, 40, 16)
    with pytest.raises(ValueError, match="use must hold one entry per line"):
        dec.learn_text([page], [[(0, "ab"), (8, "c")]], 0, 40, 16, use=[[[1, 1]]])
    dec._h = None


def test_learned_glyphs_add_and_the_learned_font_on_the_host():
    """LearnedGlyphs.__add__, and focr_decode_font_learn against the numpy restatement on sums nobody measured: random ones."""
    font = DecodeFont(MONO, 9.0, "ab H")
    rng = np.random.default_rng(11)
    n = font.s.bitmaps_len
    counts = rng.integers(0, 4, 64 * 4).astype(np.uint64)
    sums = np.zeros(n, dtype=np.uint64)  # any sums of samples of at most 255 do: the rule is per byte
    for i, (off, stride, box_h, _) in enumerate(L.layout(font)[0]):
        for p in range(64):
            cell = stride * box_h
            sums[off + p * cell: off + (p + 1) * cell] = rng.integers(0, 255 * int(counts[i * 64 + p]) + 1, cell)
    a = LearnedGlyphs(sums, counts, [[np.ones(2, dtype=np.uint8)]])
    b = LearnedGlyphs(sums // 2, counts, [[np.zeros(3, dtype=np.uint8)], []])
    total = a + b
    assert np.array_equal(total.sums, sums + sums // 2) and np.array_equal(total.counts, 2 * counts) and len(total.used) == 3
    with pytest.raises(ValueError, match="different fonts"):
        a + LearnedGlyphs(sums[:-4], counts, [])
    for min_count, grow in ((1, 0), (2, 0), (3, 1), (1, 5)):
        learned = font.learned(a, min_count=min_count, grow=grow)
        cells, inked = L.learned_phases(font, L.Learned(sums, counts, []), min_count, grow)
        assert (learned.n_learned, learned.n_inked) == (len(cells), inked) and 0 < len(cells) < inked
        want = L.Tables(font, cells)
        for i in range(4):
            for p in range(64):
                got, ref = learned.phase(i, p), want.phase(i, p)
                assert got[1:] == ref[1:] and np.array_equal(got[0], ref[0]), (min_count, grow, i, p)
        assert not learned.phase(2, 0)[0].any()  # the space stays blank
        assert learned.y_bits == 0 and np.array_equal(learned.increments(), font.increments()) and learned.origin == font.origin
        assert (learned.s.text_size, learned.s.kerning, learned.s.hinting, learned.s.bitmaps_len) == (font.s.text_size, font.s.kerning, font.s.hinting, n)
        learned.close()
        learned.close()
    for kw, words in ((dict(min_count=0), "min_count must be at least 1"), (dict(grow=-1), "grow at least 0")):
        with pytest.raises(ValueError, match=words):
            font.learned(a, **kw)
    with pytest.raises(ValueError, match="not this font's"):
        font.learned(LearnedGlyphs(sums, counts[:-1], []))
    font.close()


@pytest.fixture(scope="module")
def focr_bin():
    if not os.path.exists(FOCR):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "font_ocr_amd", "csrc"), "cli"], check=True)
    return FOCR


def test_cli_help_and_usage_errors(focr_bin, tmp_path):
    r = subprocess.run([focr_bin, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    line, = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("--learn ")]
    assert "[extension]" in line and "<FILE>" in line and "a reading you trust" in line and "reproduces its errors" in line and "plain pen loop" in line
    line, = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("--learn-min-count ")]
    assert "[extension]" in line and "M >= 1" in line and "only with --learn" in line
    line, = [ln for ln in r.stdout.splitlines() if ln.lstrip().startswith("--learn-grow ")]
    assert "[extension]" in line and "only with --learn" in line and "overlap" in line
    reading = str(tmp_path / "reading.txt")
    open(reading, "w").write("AB\n\nA~B\n")
    base = ["-f", MONO, "-t", "13", "-w", "100", "--line-height", "12", "--line-advance", "15"]
    img = ["-i", "/nonexistent/page.pgm"]  # a run that got past the arguments would fail on it with another exit code
    for extra, words in ((["--learn-min-count", "2"], ("--learn-min-count <M>", "cannot be used without", "--learn <FILE>")),
                         (["--learn-grow", "1"], ("--learn-grow <G>", "cannot be used without", "--learn <FILE>")),
                         (["--learn", reading, "--learn-min-count", "0"], ("--learn-min-count <M>", "at least 1")),
                         (["--learn", reading, "--pen-search", "1"], ("--learn <FILE>", "cannot be used with", "--pen-search <N>")),
                         (["--learn", reading, "--whole-line"], ("--learn <FILE>", "cannot be used with", "--whole-line")),
                         (["--learn", reading, "--baseline-search", "1"], ("--learn <FILE>", "cannot be used with", "--baseline-search <N>")),
                         (["--learn", reading, "--font-candidate", "t=12"], ("--learn <FILE>", "cannot be used with", "--font-candidate <SPEC>")),
                         (["--learn", reading, "--test", "t"], ("--learn <FILE>", "cannot be used with", "--test <TEST>")),
                         (["--learn", reading, "--rank-text", "AB"], ("--learn <FILE>", "cannot be used with", "--rank-text <TEXT>")),
                         (["--learn", reading], ("--learn <FILE>", "line 3", "'~' is not in the alphabet")),
                         (["--learn", str(tmp_path / "none.txt")], ("cannot read", "--learn"))):
        r = subprocess.run([focr_bin] + base + extra + img, capture_output=True, text=True)
        assert r.returncode == 2 and "error:" in r.stderr and "Usage: focr" in r.stderr and r.stdout == "", (extra, r.stderr)
        assert all(w in r.stderr for w in words), (extra, r.stderr)
    open(reading, "w").write("AB\n\nAB")  # no newline at the end: still three lines
    r = subprocess.run([focr_bin] + base + ["--learn", reading] + img, capture_output=True, text=True)  # past the arguments: the image is probed next
    assert r.returncode == 101 and "/nonexistent/page.pgm" in r.stderr and r.stdout == "", r.stderr
