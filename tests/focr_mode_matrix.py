"""The focr decoder's mode matrix: what focr_decoder_run answers under every combination of its eight settings, and after a
few sequences of calls, as a list of plain records.  tools/record_focr_modes.py wrote the walk of the commit before the
host side's refactor to tests/golden/focr_mode_matrix.json; tests/test_gpu_focr_mode_matrix.py walks the tree's library
and requires the same records, messages byte for byte.  Only the public C API (include/focr_decode.h) is called, through
ctypes, so the same walk runs against any build of the library (FOCR_HIP_LIB; font_ocr_amd/_native.py)."""
import ctypes as C
import itertools

import numpy as np

import focr_line_frac_cases as K
from font_ocr_amd import _native as N
from font_ocr_amd.decoder import DecodeFont, VerifyFont

KINDS = {  # the seven kinds of a run: the settings that select each (everything else off)
    "pen_loop": {},
    "pen_search": {"pen_search": 4},
    "whole": {"whole_line": 1},
    "whole_margins": {"whole_line": 1, "margins": 1},
    "whole_slack": {"whole_line": 1, "whole_slack": 4},
    "whole_baseline": {"whole_line": 1, "whole_baseline": (2, 1)},
    "baseline": {"baseline_search": (2, 1)},
}
N_COMBINATIONS = 256
N_SEQUENCES = 2 + 2 + 1 + 1 + len(KINDS)
MARGIN = np.dtype([("term", "<i4"), ("runner", "<u2"), ("pad", "<u2"), ("margin", "<i8")])
SCORE = np.dtype([("score", "<i8"), ("runner_score", "<i8"), ("runner", "<u2"), ("pad", "<u2", 3)])


class Walker:
    def __init__(self, device=0):
        self.lib = N.decode_hip()
        self.case = c = K.std_case(False, 2, 1)
        self.pages = np.ascontiguousarray(np.stack(c.pages))
        self.font = DecodeFont(c.font, c.size, c.alphabet, y_bits=2)
        self.vfont = VerifyFont(c.font, c.size, c.alphabet)
        self.h = C.c_void_p()
        assert self.lib.focr_decoder_create(device, C.byref(self.h)) == 0, self.lib.focr_decoder_last_error(None)
        self.set_font(self.font)

    def close(self):
        self.lib.focr_decoder_destroy(self.h)
        self.font.close()
        self.vfont.close()

    def set_font(self, font, y_fonts=True, verify=True):
        lib, h = self.lib, self.h
        assert lib.focr_decoder_set_font(h, C.byref(font.s)) == 0, self.error()
        if y_fonts:
            assert lib.focr_decoder_set_baseline_fonts(h, font.fonts, font.y_bits) == 0, self.error()
        if verify:
            assert lib.focr_decoder_set_verify_font(h, C.byref(self.vfont.s)) == 0, self.error()

    def error(self):
        return self.lib.focr_decoder_last_error(self.h).decode()

    def settings(self, scores=0, pen_search=0, whole_line=0, margins=0, whole_slack=0, baseline_search=(0, 0), whole_baseline=(0, 0),
                 line_frac=(0, 0)):
        lib, h = self.lib, self.h
        for rc in (lib.focr_decoder_set_scores(h, scores), lib.focr_decoder_set_pen_search(h, pen_search),
                   lib.focr_decoder_set_whole_line(h, whole_line), lib.focr_decoder_set_whole_margins(h, margins),
                   lib.focr_decoder_set_whole_slack(h, whole_slack), lib.focr_decoder_set_baseline_search(h, *baseline_search),
                   lib.focr_decoder_set_whole_baseline(h, *whole_baseline), lib.focr_decoder_set_line_frac(h, *line_frac)):
            assert rc == 0, self.error()

    def run(self, y=None):
        x, y0, width, line_height, line_advance = self.case.geo
        n, ph, pw = self.pages.shape
        return self.lib.focr_decoder_run(self.h, C.c_void_p(self.pages.ctypes.data), 0, n, pw, ph, x, y0 if y is None else y, width,
                                         line_height, line_advance)

    def getters(self):
        """The return code of every getter that can refuse, with null outputs."""
        lib, h = self.lib, self.h
        return {"get_scores": lib.focr_decoder_get_scores(h, None, None), "get_pens": lib.focr_decoder_get_pens(h, None, None),
                "get_margins": lib.focr_decoder_get_margins(h, None), "get_baselines": lib.focr_decoder_get_baselines(h, None, None)}

    def verify(self):
        """focr_decoder_verify without images: its return code and the per-page sums."""
        sums = np.zeros(len(self.pages), dtype=np.uint64)
        rc = self.lib.focr_decoder_verify(self.h, None, 0, sums.ctypes.data)
        return {"rc": rc, "sums": [int(s) for s in sums]} if rc == 0 else {"rc": rc, "error": self.error()}

    def outcome(self, rc):
        """The record of a run that returned rc: the refusal, or everything the getters give."""
        lib, h = self.lib, self.h
        rec = {"rc": rc, "launches": lib.focr_decoder_last_launches(h), "n_lines": lib.focr_decoder_n_lines(h)}
        if rc != 0:
            rec["error"] = self.error()
            return rec
        nl, nc = rec["n_lines"], lib.focr_decoder_n_chars(h)
        lines = (N.DecodedLine * max(1, nl))()
        chars = np.zeros(max(1, nc), dtype=np.uint16)
        offsets = np.zeros(max(1, nc), dtype=np.int8)
        assert lib.focr_decoder_get(h, lines, chars.ctypes.data) == 0 and lib.focr_decoder_get_offsets(h, offsets.ctypes.data) == 0
        al = self.case.alphabet
        rec["lines"] = [[ln.page, ln.y, "".join(al[c] for c in chars[ln.first: ln.first + ln.n_chars])] for ln in lines[:nl]]
        rec["offsets"] = [int(v) for v in offsets[:nc]]
        scores, base = np.zeros(max(1, nc), dtype=SCORE), np.zeros(max(1, nl), dtype=np.uint64)
        pens, costs = np.zeros(max(1, nc), dtype=np.uint32), np.zeros(max(1, nl), dtype=np.int64)
        margins = np.zeros(max(1, nc), dtype=MARGIN)
        q, qcost = np.zeros(max(1, nl), dtype=np.int8), np.zeros(max(1, nl), dtype=np.int64)
        rec["getters"] = g = {"get_scores": lib.focr_decoder_get_scores(h, scores.ctypes.data_as(C.POINTER(N.CharScore)), base.ctypes.data),
                              "get_pens": lib.focr_decoder_get_pens(h, pens.ctypes.data, costs.ctypes.data),
                              "get_margins": lib.focr_decoder_get_margins(h, margins.ctypes.data),
                              "get_baselines": lib.focr_decoder_get_baselines(h, q.ctypes.data, qcost.ctypes.data)}
        ints = lambda a, n: [int(v) for v in a[:n]]  # noqa: E731
        if g["get_scores"] == 0:
            rec["scores"] = {"base": ints(base, nl), "score": ints(scores["score"], nc), "runner": ints(scores["runner"], nc),
                             "runner_score": ints(scores["runner_score"], nc)}
        if g["get_pens"] == 0:
            rec["pens"], rec["costs"] = ints(pens, nc), ints(costs, nl)
        if g["get_margins"] == 0:
            rec["margins"] = {"term": ints(margins["term"], nc), "runner": ints(margins["runner"], nc), "margin": ints(margins["margin"], nc)}
        if g["get_baselines"] == 0:
            rec["baselines"] = {"q": ints(q, nl), "cost": ints(qcost, nl)}
        rec["verify"] = self.verify()
        return rec

    def combinations(self):
        frac = tuple(self.case.frac)
        axes = ((0, 1), (0, 4), (0, 1), (0, 1), (0, 4), ((0, 0), (2, 1)), ((0, 0), (2, 1)), ((0, 0), frac))
        for s, p, w, m, k, b, wb, f in itertools.product(*axes):
            self.settings(s, p, w, m, k, b, wb, f)
            name = (f"scores={s} pen_search={p} whole_line={w} margins={m} whole_slack={k} baseline_search={b[1]} whole_baseline={wb[1]} "
                    f"line_frac={int(f != (0, 0))}")
            yield {"name": name, **self.outcome(self.run())}

    def sequences(self):
        base_kinds = ("baseline", "whole_baseline")
        plain = DecodeFont(self.case.font, self.case.size, self.case.alphabet)
        self.set_font(plain, y_fonts=False)
        for kind in base_kinds:  # the baseline modes without y-phase fonts
            self.settings(**KINDS[kind])
            yield {"name": f"no y-phase fonts: {kind}", **self.outcome(self.run())}
        bent = DecodeFont(self.case.font, self.case.size, self.case.alphabet, y_bits=2)
        for f in bent.fonts:  # a caller-built font: the builder's origin_y is always a whole number
            f.origin_y += 0.5
        self.set_font(bent, verify=False)
        for kind in base_kinds:
            self.settings(**KINDS[kind])
            yield {"name": f"fractional origin_y: {kind}", **self.outcome(self.run())}
        self.set_font(self.font)
        self.settings(**KINDS["whole_margins"])
        first = self.run()
        self.settings(margins=1)
        yield {"name": "an accepted run, then a refused one", "first": first, **self.outcome(self.run()), "getters": self.getters(),
               "verify": self.verify()}
        self.settings(scores=1)
        first = self.run()
        self.set_font(self.font)
        yield {"name": "a scores run, then set_font", "first": first, "getters": self.getters(), "n_lines": self.lib.focr_decoder_n_lines(self.h),
               "verify": self.verify()}
        for kind, on in KINDS.items():  # no slot at all: nothing is launched, and a verify still draws the pages
            self.settings(**on)
            yield {"name": f"zero slots: {kind}", **self.outcome(self.run(y=self.pages.shape[1]))}
        for f in (plain, bent):
            f.close()

    def walk(self):
        return list(self.combinations()) + list(self.sequences())


def walk(device=0):
    w = Walker(device)
    try:
        return w.walk()
    finally:
        w.close()
