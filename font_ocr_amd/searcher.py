"""Host-side mirror of the reference's Searcher / get_hits / process_hits for the device path.

Everything here is a thin ctypes call into libfocr_hip.so (include/focr_ncc.h).  Names follow the
reference (src/ncc.rs): `Searcher.search_c_u8` is the per-template drop-in (FFI symbols
ncc_8_u8 / ncc_16_u8), `Scanner` is the batched form of get_hits' search loop over resident pages,
`process_hits` the anchor/line/overlap pass.  There is no CPU fallback: a missing library or
device raises.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .bank import HIT_DTYPE, MATCH_DTYPE

MAX_MATCHES = 1024  # src/ncc.rs:31
SCAN_MFMA, SCAN_DIRECT, SCAN_RUST = 0, 1, 2
PREFILTER_AUTO, PREFILTER_ONE_STAGE, PREFILTER_LEGACY = 0, 1, 3
NO_RUNNER = 0xFFFFFFFF  # FOCR_NO_RUNNER
# focr_runner_t: a character's overlap group (members) and the best hit of another letter in it (NO_RUNNER: there is none)
RUNNER_DTYPE = np.dtype([("members", "<u4"), ("letter", "<u4"), ("template_index", "<u4"), ("similarity", "<f4"), ("x", "<u2"), ("reserved", "<u2")])
assert RUNNER_DTYPE.itemsize == 20


class FocrError(RuntimeError):
    pass


def device_count():
    return int(N.hip().focr_device_count())


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _overlap_i32(overlap):
    """overlap is the reference's i32 (src/ncc.rs:514); ctypes would wrap a wider value into the int32_t argument silently."""
    o = int(overlap)
    if not -(1 << 31) <= o < (1 << 31):
        raise ValueError(f"overlap {o} is outside the i32 range")
    return o


CLASS_INFO_FIELDS = ("n_w", "n_h", "keep_w", "layout", "ksteps", "super", "value", "plane_slot", "mtx", "n_rows", "kq", "crk", "shift",
                     "n_templates", "n_live", "tile_first")


def prefilter_page_model(bank, page_ink, threshold, column_drop=True, prefilter=PREFILTER_AUTO, want=("V", "W_upper", "L", "plane", "G", "sim")):
    """Host model of the MFMA prefilter over every window of one ink-high page (focr_debug_prefilter_page; no device).  Returns a dict:
    'classes' (list of dicts, CLASS_INFO_FIELDS), 'templates' ((T, 4) int32: class, slot, live, N-tile), 'q' ((T, 32, 16) int8) and,
    if page_ink is given, the arrays named in `want`: V / W_upper / L / plane as (classes, r_h, r_w), G / sim as (T, r_h, r_w)."""
    lib = N.hip()
    T = len(bank.templates)
    info = np.zeros(16 * T, np.float64)
    n_cls = C.c_size_t(0)
    tinfo = np.zeros((T, 4), np.int32)
    q = np.zeros((T, 32, 16), np.int8)
    page = None if page_ink is None else np.ascontiguousarray(page_ink, np.uint8)
    r_h, r_w = (1, 1) if page is None else page.shape

    def call(pg, outs):
        rc = lib.focr_debug_prefilter_page(_ptr(bank.templates), T, _ptr(bank.needles), bank.needles.size, int(bool(column_drop)), int(prefilter),
                                           None if pg is None else _ptr(pg), r_w, r_h, float(threshold), _ptr(info), info.size, C.byref(n_cls),
                                           _ptr(tinfo), _ptr(q), *[None if a is None else _ptr(a) for a in outs])
        if rc != 0:
            raise FocrError(f"[{rc}] focr_debug_prefilter_page")

    if page is None:
        call(None, [None] * 6)
        out = {}
    else:
        call(None, [None] * 6)  # the number of classes first
        k = n_cls.value
        shapes = {"V": ((k, r_h, r_w), np.uint64), "W_upper": ((k, r_h, r_w), np.float32), "L": ((k, r_h, r_w), np.float32),
                  "plane": ((k, r_h, r_w), np.int16), "G": ((T, r_h, r_w), np.int32), "sim": ((T, r_h, r_w), np.float64)}
        out = {name: np.zeros(*shapes[name]) for name in want}
        call(page, [out.get(name) for name in ("V", "W_upper", "L", "plane", "G", "sim")])
    out["classes"] = [dict(zip(CLASS_INFO_FIELDS, info[16 * k: 16 * k + 16])) for k in range(n_cls.value)]
    out["templates"], out["q"] = tinfo, q
    return out


SUPER_INFO_FIELDS = ("layout", "ksteps", "n_tiles", "pairable", "q_offset", "chunk_tiles")


def bank_images(bank, column_drop=True):
    """The MFMA operand images of a bank as the upload lays them out (focr_debug_bank_images; no device): (list of per-super-class dicts,
    SUPER_INFO_FIELDS, in pass order; the raw int8 bytes)."""
    lib = N.hip()
    T = len(bank.templates)
    n_su, n_b = C.c_size_t(0), C.c_size_t(0)
    args = (_ptr(bank.templates), T, _ptr(bank.needles), bank.needles.size, int(bool(column_drop)))
    rc = lib.focr_debug_bank_images(*args, None, 0, C.byref(n_su), None, 0, C.byref(n_b))
    if rc != 0:
        raise FocrError(f"[{rc}] focr_debug_bank_images")
    info = np.zeros((max(n_su.value, 1), 6), np.uint32)
    q = np.zeros(max(n_b.value, 1), np.int8)
    rc = lib.focr_debug_bank_images(*args, _ptr(info), n_su.value, C.byref(n_su), _ptr(q), q.size, C.byref(n_b))
    if rc != 0:
        raise FocrError(f"[{rc}] focr_debug_bank_images")
    return [dict(zip(SUPER_INFO_FIELDS, (int(v) for v in info[i]))) for i in range(n_su.value)], q[: n_b.value]


class PinnedPages:
    """(n, r_h, r_w) uint8 array in page-locked host memory (focr_host_alloc): `.array` is a numpy view.
    Scanner.upload_pages from it is an asynchronous DMA (see include/focr_ncc.h)."""

    def __init__(self, n, r_h, r_w):
        self._lib = N.hip()
        p = C.c_void_p()
        rc = self._lib.focr_host_alloc(n * r_h * r_w, C.byref(p))
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")
        self._p = p
        self.array = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n, r_h, r_w))

    def close(self):
        if self._p is not None:
            self.array = None
            self._lib.focr_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RegisteredPages:
    """Context manager that page-locks an existing C-contiguous numpy array for as long as the `with` block lasts
    (focr_host_register on entry, focr_host_unregister on exit): uploads, Pipeline.prefetch and Pipeline.submit from `.array` are then
    asynchronous DMAs, as from PinnedPages memory.  The C call takes a page-aligned start, so the whole pages the array lies in are
    locked (two arrays that share a page cannot both be registered).  Leave the block only after the wait() / host_results() of every batch that reads the array has returned."""

    PAGE = 4096

    def __init__(self, array):
        if not isinstance(array, np.ndarray) or not array.flags["C_CONTIGUOUS"] or array.nbytes == 0:
            raise ValueError("RegisteredPages: a non-empty C-contiguous numpy array")
        self._lib = N.hip()
        self.array = array
        self._base = array.ctypes.data // self.PAGE * self.PAGE
        self._bytes = (array.ctypes.data + array.nbytes + self.PAGE - 1) // self.PAGE * self.PAGE - self._base
        self._on = False

    def __enter__(self):
        rc = self._lib.focr_host_register(C.c_void_p(self._base), self._bytes)
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")
        self._on = True
        return self

    def __exit__(self, *a):
        if self._on:
            self._lib.focr_host_unregister(C.c_void_p(self._base))
            self._on = False


class HostResults:
    """One batch's results in the page-locked buffers of its context (focr_host_results_t; Pipeline.host_results,
    Fleet.host_results).  n_pages, n_templates, n_matches, n_lines, n_chars, device_ms are plain numbers.  counts ((n_pages,
    n_templates) uint32), page_line_off ((n_pages + 1,) uint64), line_char_off ((n_lines + 1,) uint64) and chars ((n_chars,)
    HIT_DTYPE) are numpy VIEWS of the executor's own memory, None where the C field is NULL (the three line fields of a batch
    submitted with process_hits=False); `addresses` holds the four raw pointers (0 = NULL).  The views die at the ticket's
    release: the context's next batch overwrites or frees the buffers.  copy() gives a record that owns its arrays."""

    FIELDS = ("counts", "page_line_off", "line_char_off", "chars")

    def __init__(self, n_pages, n_templates, n_matches, n_lines, n_chars, device_ms, arrays, addresses):
        self.n_pages, self.n_templates, self.n_matches, self.n_lines, self.n_chars = n_pages, n_templates, n_matches, n_lines, n_chars
        self.device_ms = device_ms
        self.counts, self.page_line_off, self.line_char_off, self.chars = arrays
        self.addresses = dict(addresses)

    @staticmethod
    def _view(addr, dtype, n):
        if not addr:
            return None
        dtype = np.dtype(dtype)
        if n == 0:
            return np.zeros(0, dtype)
        return np.frombuffer((C.c_uint8 * (n * dtype.itemsize)).from_address(addr), dtype)

    @classmethod
    def _from_struct(cls, r):
        arrays = (cls._view(r.counts, np.uint32, r.n_pages * r.n_templates), cls._view(r.page_line_off, np.uint64, r.n_pages + 1),
                  cls._view(r.line_char_off, np.uint64, r.n_lines + 1), cls._view(r.chars, HIT_DTYPE, r.n_chars))
        if arrays[0] is not None:
            arrays = (arrays[0].reshape(r.n_pages, r.n_templates),) + arrays[1:]
        return cls(int(r.n_pages), int(r.n_templates), int(r.n_matches), int(r.n_lines), int(r.n_chars), float(r.device_ms), arrays,
                   {k: int(getattr(r, k) or 0) for k in cls.FIELDS})

    def copy(self):
        """The same record detached from the executor's buffers (it outlives the ticket's release; `addresses` stay what they were)."""
        return HostResults(self.n_pages, self.n_templates, self.n_matches, self.n_lines, self.n_chars, self.device_ms,
                           tuple(None if a is None else a.copy() for a in (self.counts, self.page_line_off, self.line_char_off, self.chars)),
                           self.addresses)

    def lines_flat_bytes(self):
        """The batch's characters in the layout of Scanner.lines_flat().tobytes() (b"" without process_hits)."""
        return b"" if self.chars is None else self.chars.tobytes()


class Searcher:
    """Per-page state of the reference (src/ncc.rs:128-141, 231-261) for the drop-in FFI symbols.

    The caller supplies the window tables exactly as the reference's prepare_for_size produces
    them (src/ncc.rs:263-318); search_c_u8 then does what src/ncc.rs:332-404 does, with the kernel
    call landing on the GPU through the reference's own symbol names.
    """

    def __init__(self, page_inv):
        self.reference_u8 = np.ascontiguousarray(page_inv, np.uint8)
        r_h, r_w = self.reference_u8.shape
        self.acc_u32 = np.zeros(r_w * 8 + 8, np.uint32)  # src/ncc.rs:242
        self.matches_c = np.zeros(MAX_MATCHES, MATCH_DTYPE)  # src/ncc.rs:240

    def search_c_u8(self, needle, stats, threshold, n_out=MAX_MATCHES):
        """needle: (n_h, n_w) uint8; stats = (patch_sum, patch_rnorm, start_end).  Returns MATCH_DTYPE[]."""
        lib = N.hip()
        if lib.focr_device_count() <= 0:  # the FFI signature has no error channel: fail loudly here
            raise FocrError("no HIP device available; the ncc_*_u8 symbols have no CPU fallback")
        needle = np.ascontiguousarray(needle, np.uint8)
        n_h, n_w = needle.shape
        if n_w <= 8:  # src/ncc.rs:337
            width, fn = 8, lib.ncc_8_u8
        elif n_w <= 16:  # src/ncc.rs:364
            width, fn = 16, lib.ncc_16_u8
        else:
            raise FocrError("not handled")  # panic!("not handled"), src/ncc.rs:392
        padded = np.zeros((n_h, width), np.uint8)  # copy_needle_n_u8, src/ncc.rs:925-935
        padded[:, :n_w] = needle
        patch_sum, patch_rnorm, start_end = stats
        patch_sum = np.ascontiguousarray(patch_sum, np.uint32)
        patch_rnorm = np.ascontiguousarray(patch_rnorm, np.float64)
        start_end = np.ascontiguousarray(start_end, np.uint16)
        r_h, r_w = self.reference_u8.shape
        out = self.matches_c if n_out == MAX_MATCHES else np.zeros(n_out, MATCH_DTYPE)
        n = fn(_ptr(self.reference_u8), r_w, r_h, _ptr(padded), n_w, n_h, _ptr(self.acc_u32), self.acc_u32.size,
               _ptr(patch_sum), _ptr(patch_rnorm), _ptr(start_end), float(threshold), _ptr(out), n_out)
        return out[:n].copy()


class Scanner:
    """Batched device scan: one bank, N resident pages (get_hits' loop, src/ncc.rs:576-701)."""

    def __init__(self, device=0, _borrowed=None):
        self._lib = N.hip()
        self._owned = _borrowed is None
        if _borrowed is None:
            h = C.c_void_p()
            rc = self._lib.focr_ctx_create(int(device), C.byref(h))
            if rc != 0:
                raise FocrError(self._lib.focr_last_error_global().decode())
        else:  # a context that belongs to a Pipeline
            h = C.c_void_p(_borrowed)
        self._h = h
        self.bank = None
        self.n_pages = self.r_w = self.r_h = 0

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                self._lib.focr_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc != 0:
            raise FocrError(f"[{rc}] " + self._lib.focr_last_error(self._h).decode())

    def set_bank(self, bank):
        self._ck(self._lib.focr_bank_upload(self._h, _ptr(bank.templates), len(bank.templates), _ptr(bank.needles),
                                            bank.needles.size))
        self.bank = bank

    def alloc_pages(self, n_pages, r_w, r_h):
        self._ck(self._lib.focr_pages_alloc(self._h, n_pages, r_w, r_h))
        self.n_pages, self.r_w, self.r_h = n_pages, r_w, r_h

    def upload_pages(self, luma, first=0, invert=True):
        """luma: (n, r_h, r_w) uint8 as the image decoder gives it (255 = paper)."""
        luma = np.ascontiguousarray(luma, np.uint8)
        if luma.ndim == 2:
            luma = luma[None]
        assert luma.shape[1:] == (self.r_h, self.r_w)
        self._ck(self._lib.focr_pages_upload(self._h, first, luma.shape[0], _ptr(luma), int(bool(invert))))

    def upload_pages_device(self, dev_ptr, count, first=0, invert=True):
        """Pages already in HBM (e.g. tensor.data_ptr() of a uint8 CUDA tensor)."""
        self._ck(self._lib.focr_pages_upload_device(self._h, first, count, C.c_void_p(int(dev_ptr)), int(bool(invert))))

    def set_pages(self, luma, invert=True):
        luma = np.ascontiguousarray(luma, np.uint8)
        if luma.ndim == 2:
            luma = luma[None]
        self.alloc_pages(luma.shape[0], luma.shape[2], luma.shape[1])
        self.upload_pages(luma, 0, invert)

    def scan(self, threshold=0.8, cap=MAX_MATCHES, mode=SCAN_MFMA):
        """mode: SCAN_MFMA / SCAN_DIRECT / SCAN_RUST, or (SCAN_MFMA, PREFILTER_*) to pick the MFMA prefilter too."""
        if isinstance(mode, tuple):
            mode, prefilter = mode
            self.set_prefilter(prefilter)
        self._ck(self._lib.focr_scan(self._h, float(threshold), int(cap), int(mode)))

    def set_prefilter(self, prefilter):
        """PREFILTER_AUTO / PREFILTER_ONE_STAGE / PREFILTER_LEGACY (focr_ctx_set_prefilter); results never change."""
        self._ck(self._lib.focr_ctx_set_prefilter(self._h, int(prefilter)))

    def set_row_tail(self, on):
        """focr_ctx_set_row_tail: True / 1 = hits-first row tail (default), False / 0 = the legacy radix-sort tail; results never change."""
        self._ck(self._lib.focr_ctx_set_row_tail(self._h, int(on)))

    def set_column_drop(self, on):
        """focr_ctx_set_column_drop: bound the last column of 9- / 13-wide classes instead of multiplying it (default on);
        takes effect at the next set_bank; results never change."""
        self._ck(self._lib.focr_ctx_set_column_drop(self._h, int(bool(on))))

    def set_size_estimates(self, on):
        """focr_ctx_set_size_estimates: repeat scans of one setup queue every phase without host waits (default on)."""
        self._ck(self._lib.focr_ctx_set_size_estimates(self._h, int(bool(on))))

    def size_estimate_stats(self):
        """focr_size_estimate_stats: {'redone': batches redone with exact sizes, 'margin': next estimate's margin, 'row_max': ...}."""
        r, m, x = C.c_uint64(), C.c_double(), C.c_uint32()
        self._ck(self._lib.focr_size_estimate_stats(self._h, C.byref(r), C.byref(m), C.byref(x)))
        return {"redone": int(r.value), "margin": float(m.value), "row_max": int(x.value)}

    def force_split(self, on):
        """Test hook (focr_debug_force_split): scan the batch in page sub-ranges as after a candidate overflow."""
        self._ck(self._lib.focr_debug_force_split(self._h, int(bool(on))))

    def phase_stamps(self):
        """focr_debug_phase_stamps: the last batch's phases on the device's clock (ms since the device's first context was created)."""
        out = (C.c_double * 9)()
        self._ck(self._lib.focr_debug_phase_stamps(self._h, out))
        return dict(zip(("stats_start", "stats_end", "scan_end", "verify_end", "order_end", "post_start", "post_end", "scan_launch_start", "scan_launch_end"),
                        [float(v) for v in out]))

    def set_tail_grid(self, num, den):
        """Test hook (focr_debug_set_tail_grid): the tail's persistent kernels on num / den times their workgroups (0, 0: as designed)."""
        self._ck(self._lib.focr_debug_set_tail_grid(self._h, int(num), int(den)))

    def tail_path(self):
        """Test hook (focr_debug_tail_path): what the last scan's tail chose: {'tail': 'rows' / 'legacy' / 'none', 'big_launch': the row
        sort's second launch ran, 'library_sort': the placed hits went through the library sort, 'order': 'counting' / 'sorting' / 'none',
        'seg_shift', 'n_seg': the row buckets' x-segments, 'verify': 'global' / 'lds16' / 'lds12' / 'chunks' / 'lds8' / 'none', 'verify_chunks'}."""
        out = (C.c_uint32 * 8)()
        self._ck(self._lib.focr_debug_tail_path(self._h, out))
        return {"tail": ("none", "rows", "legacy")[out[0]], "big_launch": bool(out[1]), "library_sort": bool(out[2]),
                "order": ("none", "counting", "sorting")[out[3]], "seg_shift": int(out[4]), "n_seg": int(out[5]),
                "verify": ("none", "global", "lds16", "lds12", "chunks", "lds8")[out[6]], "verify_chunks": int(out[7])}

    def scan_paired(self):
        """Test hook (focr_debug_scan_paired): (launches of the plane prefilter kernel in the last scan, those in the paired form)."""
        out = (C.c_uint32 * 2)()
        self._ck(self._lib.focr_debug_scan_paired(self._h, out))
        return int(out[0]), int(out[1])

    def set_stats_form(self, form):
        """Test hook (focr_debug_set_stats_form): 1 = the LDS-tiled statistics kernel for every class, 0 = the register form where it applies."""
        self._ck(self._lib.focr_debug_set_stats_form(self._h, int(form)))

    def set_verify_form(self, form):
        """Test hook (focr_debug_set_verify_form): 1 = the 12-byte verify form also for a bank that would take the 8-byte one, 0 = as designed."""
        self._ck(self._lib.focr_debug_set_verify_form(self._h, int(form)))

    def planes(self):
        """Test hook (focr_debug_planes): the int16 threshold planes of the last MFMA scan, flat."""
        n = C.c_size_t(0)
        self._ck(self._lib.focr_debug_planes(self._h, None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.int16)
        if n.value:
            self._ck(self._lib.focr_debug_planes(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def candidates(self):
        """Test hook (focr_debug_candidates): the last MFMA scan's candidates as an (n, 4) uint32 array of (page, y, x, global
        template index), in no particular order.  Raises after a scan that took the legacy tail, a split batch, a direct scan."""
        n = C.c_size_t(0)
        self._ck(self._lib.focr_debug_candidates(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 4), np.uint32)
        if n.value:
            self._ck(self._lib.focr_debug_candidates(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def set_scan_cus(self, max_cus):
        """Upper bound on the CUs the persistent scan kernel occupies (0 = all)."""
        self._ck(self._lib.focr_ctx_set_scan_cus(self._h, int(max_cus)))

    def sync(self):
        self._ck(self._lib.focr_sync(self._h))

    def counts(self):
        out = np.zeros((self.n_pages, len(self.bank)), np.uint32)
        self._ck(self._lib.focr_get_counts(self._h, _ptr(out)))
        return out

    def total_matches(self):
        return int(self._lib.focr_total_matches(self._h))

    def matches(self):
        """(offsets[n_pages*T+1], matches[total]) in (page, template, y, x) order."""
        n_seg = self.n_pages * len(self.bank)
        offsets = np.zeros(n_seg + 1, np.uint64)
        m = np.zeros(self.total_matches(), MATCH_DTYPE)
        self._ck(self._lib.focr_get_matches(self._h, _ptr(offsets), _ptr(m)))
        return offsets, m

    def process_hits(self, anchor_threshold=0.95, overlap=5):
        overlap = _overlap_i32(overlap)
        self._ck(self._lib.focr_process_hits(self._h, float(anchor_threshold), overlap))

    def debug_process_hits(self, page, y, x, t, similarity, keep):
        """Test hook (focr_debug_process_hits): these hits, strictly increasing in (page, y, x, t), become the context's hits as if
        a scan had found them (keep = 0: cut off by the cap); process_hits() and lines() then run as usual."""
        cols = [np.ascontiguousarray(a, np.uint32) for a in (page, y, x, t)]
        sims = np.ascontiguousarray(similarity, np.float32)
        kp = np.ascontiguousarray(keep, np.uint8)
        n = len(sims)
        if any(len(a) != n for a in cols + [kp]):
            raise ValueError("debug_process_hits: fields of different lengths")
        self._ck(self._lib.focr_debug_process_hits(self._h, *[_ptr(a) for a in cols], _ptr(sims), _ptr(kp), n))

    def lines(self, runners=False):
        """-> list over pages of list over lines of HIT_DTYPE arrays; runners=True: (lines, runners), the second nested alike
        with RUNNER_DTYPE arrays (runners())."""
        n_lines = int(self._lib.focr_total_lines(self._h))
        n_chars = int(self._lib.focr_total_chars(self._h))
        page_off = np.zeros(self.n_pages + 1, np.uint64)
        line_off = np.zeros(n_lines + 1, np.uint64)
        chars = np.zeros(n_chars, HIT_DTYPE)
        self._ck(self._lib.focr_get_lines(self._h, _ptr(page_off), _ptr(line_off), _ptr(chars)))
        out = []
        for p in range(self.n_pages):
            out.append([chars[int(line_off[k]): int(line_off[k + 1])] for k in range(int(page_off[p]), int(page_off[p + 1]))])
        if runners:
            r = self.runners()
            return out, [[r[int(line_off[k]): int(line_off[k + 1])] for k in range(int(page_off[p]), int(page_off[p + 1]))]
                         for p in range(self.n_pages)]
        return out

    def lines_flat(self):
        """All post-processed characters of the batch as one HIT_DTYPE array (page, line, x order)."""
        n_chars = int(self._lib.focr_total_chars(self._h))
        chars = np.zeros(n_chars, HIT_DTYPE)
        self._ck(self._lib.focr_get_lines(self._h, None, None, _ptr(chars)))
        return chars

    def lines_into(self):
        """focr_get_lines_into: the lines of the last process_hits() copied from the device straight into freshly allocated numpy
        buffers -> (page_line_off[n_pages + 1], line_char_off[total_lines + 1], chars[total_chars]) (uint64, uint64, HIT_DTYPE)."""
        n_lines = int(self._lib.focr_total_lines(self._h))
        n_chars = int(self._lib.focr_total_chars(self._h))
        # (every entry is the call's to write: a pattern, not zeros, so that one it leaves out cannot pass for an offset)
        page_off = np.full(self.n_pages + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
        line_off = np.full(n_lines + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
        chars = np.zeros(max(n_chars, 1), HIT_DTYPE)  # (the C call wants all three pointers, also for zero characters)
        self._ck(self._lib.focr_get_lines_into(self._h, _ptr(page_off), _ptr(line_off), _ptr(chars)))
        return page_off, line_off, chars[:n_chars]

    def runners(self):
        """focr_get_runners: one RUNNER_DTYPE record per character of the last process_hits(), aligned with lines_flat(): the size
        of the character's overlap group (`members`) and the group's best hit of ANOTHER letter than the winner's (the last maximum
        by f32::total_cmp; other shifts of the winner's glyph never count): its letter, template_index, similarity and x.  No such
        hit: letter = template_index = NO_RUNNER, similarity = -inf, x = 0.  Computed on the device at the first call after a
        process_hits() (one launch; later calls only copy).  Works the same on the Scanner that Pipeline.wait / Fleet.wait return,
        until the ticket's release.

            sc.scan(0.8); sc.process_hits(0.95, 5)
            c, r = sc.lines_flat(), sc.runners()
            has = r["template_index"] != NO_RUNNER
            doubt = np.flatnonzero(has & (c["similarity"] - r["similarity"] < 0.01))   # characters that won narrowly
        """
        out = np.zeros(int(self._lib.focr_total_chars(self._h)), RUNNER_DTYPE)
        self._ck(self._lib.focr_get_runners(self._h, _ptr(out) if len(out) else None))
        return out

    def last_runners(self):
        """focr_last_runners: {'ms': device time of the last runners()' kernel, 'launches': 1 if it computed the records, 0 if it only copied}."""
        ms, n = C.c_float(), C.c_uint32()
        self._ck(self._lib.focr_last_runners(self._h, C.byref(ms), C.byref(n)))
        return {"ms": float(ms.value), "launches": int(n.value)}

    def device_chars(self):
        """(device pointer, count) of the post-processed characters still resident in HBM (HIT_DTYPE records)."""
        ptr = self._lib.focr_lines_device_chars(self._h)
        return (int(ptr) if ptr else 0), int(self._lib.focr_total_chars(self._h))

    def total_chars(self):
        return int(self._lib.focr_total_chars(self._h))

    def verify_images(self, rgb=True, out=None, sq_sums=True):
        """focr_verify_images: the characters of the last process_hits() redrawn over their pages on the device, read like
        `focr --verify`'s image: red = the page (255 - ink), blue = 255 - v of the decoded characters' templates where v != 0
        (later characters win where they have ink), green = 0.  Returns (rgb, sq_sums): an (n_pages, r_h, r_w, 3) uint8 array
        and the per-page exact uint64 sums of (R - B)^2 (verify_mse turns them into the reference's f32 quotient).
        rgb=False / None: sums only (rgb is None); sq_sums=False / None: image only.  out: where the image goes instead of a
        fresh array, either a C-contiguous uint8 numpy array of that shape or a device pointer (int, e.g. tensor.data_ptr() of
        a uint8 tensor of n_pages * r_h * r_w * 3 elements on the context's device), which is then returned as it is.
        Works the same on the Scanner that Pipeline.wait / Fleet.wait return, until the ticket's release.

            sc.scan(0.8); sc.process_hits(0.95, 5)
            rgb, sums = sc.verify_images()
            worst = int(np.argmax(verify_mse(sums, sc.r_w, sc.r_h)))   # the page to look at first
        """
        shape = (self.n_pages, self.r_h, self.r_w, 3)
        want_rgb = out is not None or (rgb is not None and rgb is not False)
        sums = np.zeros(self.n_pages, np.uint64) if (sq_sums is not None and sq_sums is not False) else None
        img, ptr, on_dev = None, None, 0
        if out is not None and not isinstance(out, np.ndarray):
            img, ptr, on_dev = out, C.c_void_p(int(out)), 1
        elif want_rgb:
            img = np.empty(shape, np.uint8) if out is None else out
            if img.dtype != np.uint8 or not img.flags["C_CONTIGUOUS"] or img.shape != shape:
                raise ValueError(f"verify_images: out must be a C-contiguous uint8 array of shape {shape}")
            ptr = _ptr(img)
        self._ck(self._lib.focr_verify_images(self._h, ptr, on_dev, None if sums is None else _ptr(sums)))
        return img, sums

    def last_verify_images(self):
        """focr_last_verify_images: {'ms': device time of the last verify_images' kernels, 'launches': their number}."""
        ms, n = C.c_float(), C.c_uint32()
        self._ck(self._lib.focr_last_verify_images(self._h, C.byref(ms), C.byref(n)))
        return {"ms": float(ms.value), "launches": int(n.value)}

    def timings(self):
        ms = (C.c_float * 6)()
        self._lib.focr_last_timings(self._h, ms)
        return dict(zip(("stats", "scan", "verify", "order", "process_hits", "total"), [float(v) for v in ms]))

    def counters(self):
        c = (C.c_uint64 * 4)()
        self._lib.focr_last_counters(self._h, c)
        return dict(zip(("candidates", "raw_hits", "algorithmic_macs", "issued_macs"), [int(v) for v in c]))

    def launches(self):
        """Per-launch records of the last scan's scan kernels: list of dicts (name, ms, n_templates, macs)."""
        n = int(self._lib.focr_last_launches(self._h, None, 0))
        arr = (N.LaunchInfo * max(n, 1))()
        self._lib.focr_last_launches(self._h, arr, n)
        return [dict(name=arr[i].name.decode(), ms=float(arr[i].ms), n_templates=int(arr[i].n_templates),
                     alg_macs=int(arr[i].alg_macs), issued_macs=int(arr[i].issued_macs)) for i in range(n)]

    def debug_rnorm(self, s, s2, n):
        s = np.ascontiguousarray(s, np.uint32)
        s2 = np.ascontiguousarray(s2, np.uint64)
        n = np.ascontiguousarray(n, np.uint32)
        out = np.zeros(len(s), np.float64)
        self._ck(self._lib.focr_debug_rnorm(self._h, _ptr(s), _ptr(s2), _ptr(n), len(s), _ptr(out)))
        return out


class Pipeline:
    """Batches in flight (focr_pipe_*, include/focr_ncc.h): `n_lanes` streams on one device, `depth` contexts per lane; a batch is
    queued on the device the moment it is submitted.  submit() hands batches out round-robin over the n_lanes * depth contexts
    (`scanners`), wait() returns the Scanner view of the context holding a batch's results, release() frees that context for its
    next batch.  Calls block in native code with the GIL released."""

    def __init__(self, device=0, n_lanes=3, depth=None):
        self._lib = N.hip()
        h = C.c_void_p()
        if depth is None:
            rc = self._lib.focr_pipe_create(int(device), int(n_lanes), C.byref(h))
        else:
            rc = self._lib.focr_pipe_create2(int(device), int(n_lanes), int(depth), C.byref(h))
        if rc != 0:
            raise FocrError(self._lib.focr_last_error_global().decode())
        self._h = h
        self.n_lanes = int(self._lib.focr_pipe_lanes(h))
        self.scanners = [Scanner(device, _borrowed=self._lib.focr_pipe_context(h, i)) for i in range(int(self._lib.focr_pipe_contexts(h)))]
        self._keep = {}  # ticket -> host array kept alive while its batch is in flight

    def close(self):
        if getattr(self, "_h", None):
            for sc in self.scanners:
                sc.close()
            self._lib.focr_pipe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_bank(self, bank):
        rc = self._lib.focr_pipe_bank_upload(self._h, _ptr(bank.templates), len(bank.templates), _ptr(bank.needles), bank.needles.size)
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")
        for sc in self.scanners:
            sc.bank = bank

    def submit(self, luma=None, threshold=0.8, cap=MAX_MATCHES, mode=SCAN_MFMA, process_hits=True, anchor_threshold=0.95,
               overlap=5, invert=True, device_ptr=None, shape=None, chars_out=None):
        """luma: (n, r_h, r_w) uint8 host pages; or device_ptr + shape=(n, r_h, r_w); or neither = rescan the lane's
        resident pages.  chars_out=(device pointer, bytes): also copy the batch's characters there.  Returns the ticket."""
        overlap = _overlap_i32(overlap)
        t = C.c_uint64()
        if luma is not None:
            luma = np.ascontiguousarray(luma, np.uint8)
            if luma.ndim == 2:
                luma = luma[None]
            n, r_h, r_w = luma.shape
            ptr, on_dev = _ptr(luma), 0
        elif device_ptr is not None:
            n, r_h, r_w = shape
            ptr, on_dev = C.c_void_p(int(device_ptr)), 1
        else:
            n = r_h = r_w = 0
            ptr, on_dev = None, 0
        rc = self._lib.focr_pipe_submit(self._h, ptr, on_dev, n, r_w, r_h, int(bool(invert)), float(threshold), int(cap), int(mode),
                                        int(bool(process_hits)), float(anchor_threshold), overlap,
                                        C.c_void_p(int(chars_out[0])) if chars_out else None, int(chars_out[1]) if chars_out else 0,
                                        C.byref(t))
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")
        if luma is not None:
            self._keep[t.value] = luma
            if getattr(self, "_announced", None):
                self._announced.pop(0)
        lane = self.scanners[(t.value - 1) % len(self.scanners)]
        if n:
            lane.n_pages, lane.r_w, lane.r_h = n, r_w, r_h
        return t.value

    def prefetch(self, luma, invert=True):
        """focr_pipe_prefetch: announce the host pages (n, r_h, r_w) uint8 of the batch that will be submitted after everything
        announced or submitted so far, and start their copy to the device and their ingest now (page-locked memory: PinnedPages).
        The matching submit must bring the same array (and the same `invert`, or the lane uploads the batch itself)."""
        if luma.dtype != np.uint8 or not luma.flags["C_CONTIGUOUS"] or luma.ndim != 3:
            raise ValueError("prefetch: a C-contiguous (n, r_h, r_w) uint8 array")
        n, r_h, r_w = luma.shape
        rc = self._lib.focr_pipe_prefetch(self._h, _ptr(luma), n, r_w, r_h, int(bool(invert)))
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")
        self._announced = getattr(self, "_announced", [])
        self._announced.append(luma)  # kept alive until its submit takes over

    def announce_last(self):
        """focr_pipe_announce_last: the NEXT batch submitted is the stream's last for now: its tail may take the whole GPU."""
        self._lib.focr_pipe_announce_last(self._h)

    def end_of_stream(self):
        """focr_pipe_end_of_stream: nothing follows the newest batch for now — effective only if the executor has not queued that
        batch yet (say it before the last submit with announce_last)."""
        self._lib.focr_pipe_end_of_stream(self._h)

    def set_fetch(self, on=True):
        """focr_pipe_set_fetch: completing a batch also copies its counts and lines into page-locked host memory of its context
        (host_results).  Read when a batch is completed: set it before submitting."""
        rc = self._lib.focr_pipe_set_fetch(self._h, int(bool(on)))
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")

    def host_results(self, ticket):
        """focr_pipe_host_results: blocks until the batch is done, like wait(); returns its HostResults, whose arrays are views of
        the context's page-locked buffers — valid until release(ticket), copy() what has to live longer.  Raises the batch's own
        error if it failed, and FocrError unless fetch was on when the batch was completed (set_fetch)."""
        r = N.HostResults()
        rc = self._lib.focr_pipe_host_results(self._h, int(ticket), C.byref(r))
        self._keep.pop(ticket, None)
        if rc != 0:
            sc = self.scanners[(ticket - 1) % len(self.scanners)]
            raise FocrError(f"[{rc}] " + self._lib.focr_last_error(sc._h).decode())
        return HostResults._from_struct(r)

    def ticket_times(self, ticket):
        """focr_pipe_ticket_times (after wait, before release): dict of host stamps (us since the executor was created) and the
        device-side interval to the previous ticket's completion (ms; < 0: not available)."""
        t = N.TicketTimes()
        rc = self._lib.focr_pipe_ticket_times(self._h, int(ticket), C.byref(t))
        if rc != 0:
            raise FocrError(f"[{rc}] focr_pipe_ticket_times: ticket is not complete and unreleased")
        return {k: float(getattr(t, k)) for k, _ in N.TicketTimes._fields_}

    def wait(self, ticket):
        """Blocks until the batch is done; returns the Scanner whose getters (matches, lines, counts...) see it."""
        h = C.c_void_p()
        rc = self._lib.focr_pipe_wait(self._h, int(ticket), C.byref(h))
        self._keep.pop(ticket, None)
        sc = self.scanners[(ticket - 1) % len(self.scanners)]
        if rc != 0:
            raise FocrError(f"[{rc}] " + self._lib.focr_last_error(sc._h).decode())
        return sc

    def release(self, ticket):
        rc = self._lib.focr_pipe_release(self._h, int(ticket))
        if rc != 0:
            raise FocrError(f"[{rc}] focr_pipe_release: ticket is not outstanding")


def verify_mse(sq_sums, r_w, r_h):
    """The reference's red_blue_mse of verify_images' sums: (float)sum / (float)(uint32_t)(r_w * r_h), one f32 division per page."""
    n = np.float32(np.uint32((int(r_w) * int(r_h)) & 0xFFFFFFFF))
    return np.asarray(sq_sums, np.uint64).astype(np.float32) / n


def text_of(lines, advance_px=None):
    """Default `ncc` output of one page: letters of each line concatenated (src/ncc.rs:869-876).  With advance_px
    (extension): blanks are inserted where consecutive origins are more than one advance apart."""
    host = N.host()
    out = []
    for line in lines:
        line = np.ascontiguousarray(line, HIT_DTYPE)
        buf = C.create_string_buffer(8 * len(line) * 4 + 16)
        host.focr_line_text(_ptr(line), len(line), float(advance_px or 0.0), int(advance_px is not None), buf, len(buf))
        out.append(buf.value.decode("utf-8"))
    return "\n".join(out)


class Fleet:
    """Every GPU of the node (focr_fleet_*, include/focr_ncc.h): one Pipeline-like executor per device, batch k -> device
    k % n_devices; retire the tickets in submission order.  devices=None: all visible devices (the same device may be
    listed more than once: several executors share it — what the one-GPU tests do)."""

    def __init__(self, devices=None, lanes=3):
        self._lib = N.hip()
        h = C.c_void_p()
        if devices:
            arr = (C.c_int * len(devices))(*devices)
            rc = self._lib.focr_fleet_create(arr, len(devices), int(lanes), C.byref(h))
        else:
            rc = self._lib.focr_fleet_create(None, 0, int(lanes), C.byref(h))
        if rc != 0:
            raise FocrError(self._lib.focr_last_error_global().decode())
        self._h = h
        self.n_devices = int(self._lib.focr_fleet_devices(h))
        self.lanes = int(self._lib.focr_fleet_lanes(h))
        self.slots = int(self._lib.focr_fleet_slots(h))  # batches that can be outstanding
        self._views = {}  # context handle -> Scanner view
        self._keep = {}
        self.bank = None

    def close(self):
        if getattr(self, "_h", None):
            for sc in self._views.values():
                sc.close()
            self._lib.focr_fleet_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_bank(self, bank):
        rc = self._lib.focr_fleet_bank_upload(self._h, _ptr(bank.templates), len(bank.templates), _ptr(bank.needles), bank.needles.size)
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")
        self.bank = bank

    def device_of(self, ticket):
        return int(self._lib.focr_fleet_device_of(self._h, int(ticket)))

    def submit(self, luma, threshold=0.8, cap=MAX_MATCHES, mode=SCAN_MFMA, process_hits=True, anchor_threshold=0.95, overlap=5, invert=True):
        overlap = _overlap_i32(overlap)
        luma = np.ascontiguousarray(luma, np.uint8)
        if luma.ndim == 2:
            luma = luma[None]
        n, r_h, r_w = luma.shape
        t = C.c_uint64()
        rc = self._lib.focr_fleet_submit(self._h, _ptr(luma), 0, n, r_w, r_h, int(bool(invert)), float(threshold), int(cap), int(mode),
                                         int(bool(process_hits)), float(anchor_threshold), overlap, C.byref(t))
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")
        self._keep[t.value] = luma
        return t.value

    def set_fetch(self, on=True):
        """focr_fleet_set_fetch: Pipeline.set_fetch on every device's executor (before the first submit)."""
        rc = self._lib.focr_fleet_set_fetch(self._h, int(bool(on)))
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")

    def host_results(self, ticket):
        """focr_fleet_host_results: Pipeline.host_results for a fleet ticket; the views die at release(ticket)."""
        r = N.HostResults()
        rc = self._lib.focr_fleet_host_results(self._h, int(ticket), C.byref(r))
        self._keep.pop(ticket, None)
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")
        return HostResults._from_struct(r)

    def announce_last(self):
        """focr_fleet_announce_last: the next n_devices batches end their devices' streams (call before submitting them)."""
        rc = self._lib.focr_fleet_announce_last(self._h)
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")

    def end_of_stream(self):
        """focr_fleet_end_of_stream: Pipeline.end_of_stream on every device's executor (right after the last submit)."""
        rc = self._lib.focr_fleet_end_of_stream(self._h)
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")

    def pipe(self, index):
        """focr_fleet_pipe: the raw handle (an int) of the index-th device's executor, for the focr_pipe_* getters (it belongs to
        the fleet: submit to it only through the fleet)."""
        h = self._lib.focr_fleet_pipe(self._h, int(index))
        if not h:
            raise IndexError(f"Fleet.pipe: no executor {index} (the fleet has {self.n_devices})")
        return int(h)

    def wait(self, ticket):
        """Blocks until the batch is done; returns a Scanner view of the context holding its results."""
        h = C.c_void_p()
        rc = self._lib.focr_fleet_wait(self._h, int(ticket), C.byref(h))
        luma = self._keep.pop(ticket, None)
        if rc != 0:
            raise FocrError(f"[{rc}] {self._lib.focr_last_error_global().decode()}")
        sc = self._views.get(h.value)
        if sc is None:
            sc = self._views[h.value] = Scanner(self.device_of(ticket), _borrowed=h.value)
        sc.bank = self.bank
        if luma is not None:
            sc.n_pages, sc.r_h, sc.r_w = luma.shape
        return sc

    def release(self, ticket):
        rc = self._lib.focr_fleet_release(self._h, int(ticket))
        if rc != 0:
            raise FocrError(f"[{rc}] focr_fleet_release: ticket is not outstanding")
