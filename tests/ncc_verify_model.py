"""Numpy model of focr_verify_images (include/focr_ncc.h): red = the page's luma where it is not 255, blue = 255 - v where a
character's template has v != 0, characters in output order (a later one wins only where its own v != 0), green 0, and the exact
sum of (R - B)^2 per page.  Fed with the device's own characters, it isolates the image kernels from the scan."""
import numpy as np

from font_ocr_amd.bank import HIT_DTYPE


def verify_model(pages_ink, bank, page_line_off, line_char_off, chars, reverse=False):
    """pages_ink: (n, r_h, r_w) uint8, 255 = full ink.  -> (rgb (n, r_h, r_w, 3) uint8, sq_sums (n,) uint64).
    reverse=True applies every page's characters in the opposite order (the tests' proof that a case can tell the orders apart)."""
    pages_ink = np.asarray(pages_ink, np.uint8)
    n, H, W = pages_ink.shape
    rgb = np.zeros((n, H, W, 3), np.uint8)
    rgb[..., 0] = np.where(pages_ink != 0, 255 - pages_ink, 0)
    for p in range(n):
        mine = chars[int(line_char_off[int(page_line_off[p])]): int(line_char_off[int(page_line_off[p + 1])])]
        for c in (mine[::-1] if reverse else mine):
            x, y = int(c["x"]), int(c["y"])
            v = bank.needle(int(c["template_index"]))[: H - y, : W - x]  # canvas bytes verbatim, clipped to the page
            blue = rgb[p, y: y + v.shape[0], x: x + v.shape[1], 2]
            blue[v != 0] = 255 - v[v != 0]
    d = rgb[..., 0].astype(np.int64) - rgb[..., 2].astype(np.int64)
    return rgb, (d * d).sum(axis=(1, 2)).astype(np.uint64)


def triple_of(lines):
    """Scanner.lines() (pages of lines of HIT_DTYPE arrays) -> (page_line_off, line_char_off, chars) as focr_get_lines lays them out."""
    page_off, line_off, parts = [0], [0], []
    for page in lines:
        for line in page:
            parts.append(np.asarray(line, HIT_DTYPE))
            line_off.append(line_off[-1] + len(line))
        page_off.append(len(line_off) - 1)
    chars = np.concatenate(parts) if parts else np.zeros(0, HIT_DTYPE)
    return np.asarray(page_off, np.uint64), np.asarray(line_off, np.uint64), chars
