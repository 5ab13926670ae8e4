#!/usr/bin/env python3
"""Time of Scanner.runners() on bench.py's own batch: 128 synthetic 608x720 pages (BASELINE configs[1]: the 380-template
DejaVu Sans Mono 13 px bank), scanned at 0.8, process_hits(0.95, 5).  One JSON line, also written to --out:

  device_ms        median device time of the call's one kernel (focr_last_runners)
  wall_ms          median host time of Scanner.runners() with the records computed and read back into pageable host memory
  wall_ms_copy     ... of a second call after the same process_hits: the copy alone, no launch
Each median is over --steps calls after --warmup untimed ones; min and max beside it.  Only the first call after a process_hits
computes, so every step runs process_hits again (and waits for it) outside the timed region; the scan is outside it too.
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
from font_ocr_amd.searcher import NO_RUNNER, Scanner  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ncc_runners_bench.json"))
    args = ap.parse_args()
    import torch

    R_W, R_H = 608, 720
    bank = Bank.load(os.path.join(ROOT, "tests", "golden", "bank_dejavu13_ascii95_x2.bin"))
    pages = synth_pages(bank, args.pages, R_W, R_H)
    sc = Scanner(0)
    sc.set_bank(bank)
    sc.set_pages(pages)
    sc.scan(0.8)
    wall, wall_copy, device, walk = [], [], [], []
    first = None
    for i in range(args.warmup + args.steps):
        sc.process_hits(0.95, 5)
        n_chars = sc.total_chars()  # waits for process_hits
        t0 = time.perf_counter()
        r = sc.runners()
        t1 = time.perf_counter()
        last = sc.last_runners()
        assert last["launches"] == 1 and len(r) == n_chars
        t2 = time.perf_counter()
        again = sc.runners()
        t3 = time.perf_counter()
        assert sc.last_runners()["launches"] == 0
        if first is None:
            first = r
        assert r.tobytes() == first.tobytes() == again.tobytes()
        if i >= args.warmup:
            wall.append((t1 - t0) * 1e3)
            wall_copy.append((t3 - t2) * 1e3)
            device.append(last["ms"])
            walk.append(sc.timings()["process_hits"])

    def stats(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    has = first["template_index"] != NO_RUNNER
    out = {"bench": "ncc_runners", "pages": args.pages, "page_w": R_W, "page_h": R_H, "templates": len(bank), "hits": sc.counters()["raw_hits"],
           "chars": int(len(first)), "with_runner": int(has.sum()), "members_max": int(first["members"].max()), "launches": 1,
           "steps": args.steps, "warmup": args.warmup, "device_ms": stats(device), "wall_ms": stats(wall), "wall_ms_copy": stats(wall_copy),
           "process_hits_device_ms": stats(walk), "record_bytes": int(first.nbytes), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sc.close()


if __name__ == "__main__":
    main()
