#!/usr/bin/env python3
"""Time of Scanner.verify_images on bench.py's own batch: 128 synthetic 608x720 pages (BASELINE configs[1]: the 380-template
DejaVu Sans Mono 13 px bank), scanned at 0.8, process_hits(0.95, 5).  One JSON line, also written to --out:

  device_ms_rgb / device_ms_sums   median device time of the call's two kernels (focr_last_verify_images) with the image written
                                   to a device buffer / with the sums alone (no image written)
  wall_ms_device_rgb               median host time of the call with the image left on the device (a caller's buffer)
  wall_ms_host_rgb                 ... with the image read back into pageable host memory (n x 608 x 720 x 3 bytes)
  wall_ms_sums                     ... with the sums alone
Each median is over --steps calls after --warmup untimed ones; min and max beside it.  The scan and process_hits are outside
every timed region.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from font_ocr_amd import Bank, synth_pages  # noqa: E402
from font_ocr_amd.searcher import Scanner, verify_mse  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ncc_verify_bench.json"))
    args = ap.parse_args()
    import torch

    R_W, R_H = 608, 720
    bank = Bank.load(os.path.join(ROOT, "tests", "golden", "bank_dejavu13_ascii95_x2.bin"))
    pages = synth_pages(bank, args.pages, R_W, R_H)
    sc = Scanner(0)
    sc.set_bank(bank)
    sc.set_pages(pages)
    sc.scan(0.8)
    sc.process_hits(0.95, 5)
    n_chars = sc.total_chars()
    n_lines = sum(len(p) for p in sc.lines())
    dev = torch.empty((args.pages, R_H, R_W, 3), dtype=torch.uint8, device="cuda:0")
    host = np.empty((args.pages, R_H, R_W, 3), np.uint8)
    torch.cuda.synchronize()

    def run(**kw):
        wall, device = [], []
        for i in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            sc.verify_images(**kw)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                wall.append(dt)
                device.append(sc.last_verify_images()["ms"])
        return wall, device

    def stats(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    w_dev, d_rgb = run(out=dev.data_ptr())
    w_host, _ = run(out=host)
    w_sums, d_sums = run(rgb=None)
    _, sums = sc.verify_images(rgb=None)
    assert np.array_equal(dev.cpu().numpy(), host)
    out = {"bench": "ncc_verify_images", "pages": args.pages, "page_w": R_W, "page_h": R_H, "templates": len(bank), "lines": n_lines, "chars": n_chars,
           "launches": sc.last_verify_images()["launches"], "steps": args.steps, "warmup": args.warmup,
           "device_ms_rgb": stats(d_rgb), "device_ms_sums": stats(d_sums), "wall_ms_device_rgb": stats(w_dev), "wall_ms_host_rgb": stats(w_host),
           "wall_ms_sums": stats(w_sums), "rgb_bytes": int(host.nbytes), "mse_mean": float(verify_mse(sums, R_W, R_H).mean()),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sc.close()


if __name__ == "__main__":
    main()
