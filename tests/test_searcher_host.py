"""Argument checks of the Python API (font_ocr_amd/searcher.py) that happen before any native call.  No GPU."""
import numpy as np
import pytest

from font_ocr_amd.searcher import Fleet, Pipeline, Scanner


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: the argument should have been refused first")


class _Recorder:
    def __init__(self):
        self.overlaps = []

    def focr_process_hits(self, h, anchor, overlap):
        self.overlaps.append(overlap)
        return 0


def _bare(cls, lib):
    obj = cls.__new__(cls)  # no device: only the argument handling runs
    obj._lib, obj._h = lib, None
    return obj


@pytest.mark.parametrize("overlap", [1 << 31, (1 << 32) - 1, 1 << 32, -(1 << 31) - 1, -(1 << 40)])
def test_overlap_outside_i32_is_refused(overlap):
    """The reference's overlap is an i32 (src/ncc.rs:514); ctypes would wrap these into the int32_t argument silently."""
    with pytest.raises(ValueError, match="i32"):
        _bare(Scanner, _NoLib()).process_hits(0.95, overlap)
    with pytest.raises(ValueError, match="i32"):
        _bare(Pipeline, _NoLib()).submit(np.zeros((1, 8, 8), np.uint8), overlap=overlap)
    with pytest.raises(ValueError, match="i32"):
        _bare(Fleet, _NoLib()).submit(np.zeros((1, 8, 8), np.uint8), overlap=overlap)


def test_overlap_inside_i32_reaches_the_library():
    lib = _Recorder()
    sc = _bare(Scanner, lib)
    for o in (-(1 << 31), -5, -1, 0, 5, (1 << 31) - 1):
        sc.process_hits(0.95, o)
    assert lib.overlaps == [-(1 << 31), -5, -1, 0, 5, (1 << 31) - 1]
