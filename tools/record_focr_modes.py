"""Record the focr decoder's mode matrix (tests/focr_mode_matrix.py) to tests/golden/focr_mode_matrix.json, the table
tests/test_gpu_focr_mode_matrix.py holds the tree to.  Run it against a build of the commit whose behaviour is to be kept:
    FOCR_HIP_LIB=<that build>/font_ocr_amd/lib/libfocr_hip.so python tools/record_focr_modes.py --commit <its hash> [--out FILE]
Without --commit the hash is the checkout's HEAD, which is right only when the library loaded is that checkout's own."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import focr_mode_matrix as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit")
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "focr_mode_matrix.json"))
args = ap.parse_args()
commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
records = M.walk()
assert len(records) == M.N_COMBINATIONS + M.N_SEQUENCES, len(records)
with open(args.out, "w") as f:  # one compact record per line
    f.write('{"commit": "%s", "records": [\n' % commit)
    f.write(",\n".join(json.dumps(r, sort_keys=True, separators=(",", ":")) for r in records))
    f.write("\n]}\n")
accepted = sum(r.get("rc") == 0 for r in records[: M.N_COMBINATIONS])
print(f"recorded {len(records)} records ({accepted} of {M.N_COMBINATIONS} combinations accepted) against commit {commit} -> {args.out}")
