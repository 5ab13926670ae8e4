"""The HIP library's device memory has one owner, csrc/hip/devmem.h: no other file there calls the runtime's allocator, so
focr_debug_device_bytes (tests/test_gpu_device_memory.py) sees every allocation.  The one exception starts the runtime."""
import glob
import os
import re

HIP_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "font_ocr_amd", "csrc", "hip")


def test_only_devmem_h_allocates_device_memory():
    calls = []
    for path in sorted(glob.glob(os.path.join(HIP_DIR, "*"))):
        name = os.path.basename(path)
        if name == "devmem.h":
            continue
        with open(path, encoding="utf-8") as f:
            for no, line in enumerate(f, 1):
                code = re.sub(r'"(?:[^"\\]|\\.)*"', '""', line).split("//")[0]  # error texts and comments may name the calls
                for m in re.finditer(r"\bhip(Malloc|MallocAsync|MallocManaged|Free|FreeAsync)\s*\(", code):
                    calls.append((name, no, code[m.start():].strip()))
    assert [c for c in calls if not (c[0] == "pipe.hip" and c[2].startswith("hipFree(nullptr)"))] == []
    assert len(calls) == 1  # pipe.hip: hipFree(nullptr) brings the runtime up once
