"""Small batches for the executor's host results (tests/test_gpu_host_results.py, tools/host_results_check.py) and what the ORACLE
says they give: counts [n_pages][n_templates], page and line offsets, character records — the content of a focr_host_results_t,
byte for byte.  Nothing here asks the library under test for a result: pages come from synth_pages, matches from O.scan_page (the
compiled reference kernels where they are built), lines from O.process_hits over O.raw_hits' order.

tests/test_executor_cases_host.py proves, on the oracle alone, that every batch is what its name says (CONDITIONS below)."""
import os

import numpy as np

from font_ocr_amd import Bank, synth_pages
from font_ocr_amd.bank import HIT_DTYPE
from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

THR, CAP, ANCHOR, OVERLAP = 0.8, 1024, 0.95, 5
R_W, R_H = 300, 130            # the fleet test's geometry; nothing here is larger
ODD_W, DWORD_W, SRC_H = 297, 296, 110  # page sources on a plain Scanner: r_w % 4 != 0 and == 0
NO_LINES_ANCHOR = 1.5          # above every similarity (<= 1): hits, but no anchored row
LINES_THR = 0.5                # small / big: threshold = anchor threshold, so every page row with a hit is a line
HIT_BYTES = HIT_DTYPE.itemsize


def bank():
    """74 templates of the golden x2 bank: 37 glyphs at both x shifts, 8 and 9 px wide (test_fleet_orders_batches_over_devices' subset)."""
    full = Bank.load(os.path.join(GOLD, "bank_dejavu13_ascii95_x2.bin"))
    return full, full.subset(list(range(33, 70)) + list(range(95 + 33, 95 + 70)))


def pinbuf_capacity(want):
    """What PinBuf::ensure (pipe.hip) allocates for a first request of `want` bytes."""
    return want + want // 4 + 4096


def build():
    """name -> dict(pages, thr, cap, anchor, overlap).  Pages are luma8, 255 = paper."""
    full, _ = bank()
    text = synth_pages(full, 2, R_W, R_H, first=9500)
    more = synth_pages(full, 14, R_W, R_H, first=9520)
    blank = np.full((2, R_H, R_W), 255, np.uint8)
    std = dict(thr=THR, cap=CAP, anchor=ANCHOR, overlap=OVERLAP)
    cases = {
        "text": dict(std, pages=text),
        "blank": dict(std, pages=blank),
        "no-lines": dict(std, pages=text, anchor=NO_LINES_ANCHOR),
        "one-blank-page": dict(std, pages=np.stack([text[0], blank[0], text[1]])),
        "cap1": dict(std, pages=text, cap=1),
    }
    # small / big: one geometry and setup; `small` keeps a piece of the first text line of one page (synthetic pages carry their
    # text below a 40 px margin)
    small = np.full_like(more, 255)
    small[0, 36:56, :140] = more[0, 36:56, :140]
    cases["small"] = dict(std, pages=small, thr=LINES_THR, anchor=LINES_THR)
    cases["big"] = dict(std, pages=more, thr=LINES_THR, anchor=LINES_THR)
    # sparse / dense: as test_pipeline_chars_out_with_estimated_and_redone_batches, smaller pages and a lower threshold
    dense = synth_pages(full, 3, R_W, R_H, first=9540)
    sparse = dense.copy()
    sparse[:, 56:, :] = 255  # the first text line only
    cases["sparse"] = dict(std, pages=sparse, thr=0.4)
    cases["dense"] = dict(std, pages=dense, thr=0.4)
    cases["odd-width"] = dict(std, pages=synth_pages(full, 4, ODD_W, SRC_H, first=9560))
    cases["dword-width"] = dict(std, pages=synth_pages(full, 4, DWORD_W, SRC_H, first=9570))
    for c in cases.values():
        c["pages"] = np.ascontiguousarray(c["pages"])
    return cases


def scan(pages, bk, thr, cap):
    """The oracle's scan of every page -> (counts [n_pages][T] uint32, per page the raw hits in get_hits order with the TEMPLATE
    INDEX in `letter`: process_hits carries that field through untouched, which is how the expected template_index is known)."""
    counts, hits = [], []
    for pg in pages:
        c, m = O.scan_page(O.invert(pg), bk, thr, cap, use_ref=O.have_ref())
        counts.append(np.asarray(c, np.uint32))
        h = O.raw_hits(c, m, bk)
        h["letter"] = np.repeat(np.arange(len(c), dtype=np.uint32), np.asarray(c, np.int64))
        hits.append(h)
    return np.stack(counts), hits


def records(oracle_hits, bk):
    """Oracle hit records (template index in `letter`) -> focr_hit_t records."""
    out = np.zeros(len(oracle_hits), HIT_DTYPE)
    t = oracle_hits["letter"].astype(np.int64)
    for f in ("x", "y", "w", "h"):
        out[f] = oracle_hits[f]
    out["similarity"] = oracle_hits["similarity"]
    out["letter"] = bk.templates["letter"][t]
    out["template_index"] = t
    return out


class Expected:
    """What focr_host_results_t must hold for one batch."""

    def __init__(self, counts, hits, bk, post, anchor, overlap):
        self.n_pages, self.n_templates = counts.shape
        self.counts = counts
        self.n_matches = int(counts.sum(dtype=np.uint64))
        self.hits = hits  # per page, oracle records (for the conditions)
        self.post = post
        page_off, line_off, chars = [0], [0], []
        if post:
            for h in hits:
                for line in O.process_hits(h, anchor, overlap):
                    chars.append(records(line, bk))
                    line_off.append(line_off[-1] + len(line))
                page_off.append(len(line_off) - 1)
        self.n_lines = len(line_off) - 1 if post else 0
        self.page_line_off = np.asarray(page_off, np.uint64) if post else None
        self.line_char_off = np.asarray(line_off, np.uint64) if post else None
        self.chars = (np.concatenate(chars) if chars else np.zeros(0, HIT_DTYPE)) if post else None
        self.n_chars = len(self.chars) if post else 0

    def matches_flat(self, bk):
        """Every match in (page, template, y, x) order as focr_match_t records (Scanner.matches()[1])."""
        out = []
        for h in self.hits:
            m = np.zeros(len(h), O.MATCH_DTYPE)
            m["x"], m["y"], m["similarity"] = h["x"], h["y"], h["similarity"]
            out.append(m)
        return np.concatenate(out) if out else np.zeros(0, O.MATCH_DTYPE)


def expected(case, bk, post=True):
    counts, hits = scan(case["pages"], bk, case["thr"], case["cap"])
    return Expected(counts, hits, bk, post, case["anchor"], case["overlap"])


_cache = {}


def all_expected():
    """(bank, cases, name -> Expected), computed once per process and never changed."""
    if not _cache:
        _, bk = bank()
        cases = build()
        _cache["v"] = (bk, cases, {name: expected(c, bk) for name, c in cases.items()})
    return _cache["v"]


def conditions(cases, exp):
    """Every property the GPU tests rely on, from the oracle alone -> list of (name, holds, detail)."""
    out = []

    def add(name, ok, detail):
        out.append((name, bool(ok), detail))

    e = exp["text"]
    add("text: lines on every page", np.all(np.diff(e.page_line_off.astype(np.int64)) > 0) and e.n_chars > e.n_lines, (e.page_line_off, e.n_chars))
    e = exp["blank"]
    add("blank: nothing", e.n_matches == 0 and e.n_lines == 0 and e.n_chars == 0, e.n_matches)
    e = exp["no-lines"]
    top = max(float(h["similarity"].max()) for h in e.hits if len(h))
    add("no-lines: hits, no line", e.n_matches > 0 and e.n_lines == 0 and e.n_chars == 0 and top < NO_LINES_ANCHOR, (e.n_matches, e.n_lines, top))
    e = exp["one-blank-page"]
    p = e.page_line_off.astype(np.int64)
    add("one-blank-page: equal offsets around the middle page", e.n_pages == 3 and p[1] == p[2] and p[1] > 0 and p[3] > p[2] and e.counts[1].sum() == 0, p)
    s, b = exp["small"], exp["big"]
    same = cases["small"]["pages"].shape == cases["big"]["pages"].shape
    add("small / big: chars buffer must grow", same and s.n_chars > 0 and (b.n_chars + 1) * HIT_BYTES > pinbuf_capacity((s.n_chars + 1) * HIT_BYTES),
        (s.n_chars, b.n_chars))
    add("small / big: line_char_off buffer must grow", s.n_lines > 0 and (b.n_lines + 1) * 8 > pinbuf_capacity((s.n_lines + 1) * 8), (s.n_lines, b.n_lines))
    s, d = exp["sparse"], exp["dense"]
    same = cases["sparse"]["pages"].shape == cases["dense"]["pages"].shape
    uncapped = s.counts.max() < CAP and d.counts.max() < CAP  # so the counts are the hits before the cap, which the estimates bound
    # SizeEstimate::update (results.hip): the next scan's bound is hits + 20 % + 8192 at the widest margin
    add("sparse / dense: dense overflows sparse's widest bound", same and uncapped and s.n_chars > 0 and d.n_matches > s.n_matches + s.n_matches // 5 + 8192
        and d.n_chars > 2 * s.n_chars, (s.n_matches, d.n_matches, s.n_chars, d.n_chars))
    e, t = exp["cap1"], exp["text"]
    add("cap1: counts at the cap", e.counts.max() == 1 and t.counts.max() > 1 and e.n_matches < t.n_matches and e.n_lines > 0, (e.n_matches, t.n_matches))
    for name, rem in (("odd-width", False), ("dword-width", True)):
        e, pg = exp[name], cases[name]["pages"]
        per_page = e.counts.sum(axis=1)
        add(f"{name}: four different pages with lines", pg.shape[0] == 4 and (pg.shape[2] % 4 == 0) == rem and np.all(per_page > 0)
            and len({pg[i].tobytes() for i in range(4)}) == 4 and np.all(np.diff(e.page_line_off.astype(np.int64)) > 0), (pg.shape, per_page))
    for name, c in cases.items():
        add(f"{name}: at most {R_W}x{R_H}", c["pages"].shape[1] <= R_H and c["pages"].shape[2] <= R_W, c["pages"].shape)
    return out
