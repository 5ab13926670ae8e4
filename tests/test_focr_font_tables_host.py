"""The host side of every font upload of the focr decoder (csrc/hip/decode_font.h: the record of an uploaded font, the
glyph-table checks, the packing of the device records) without a device: csrc/hip/decode_font_check.cpp is built as a
stand-alone program under the sanitizers, with a host compiler alone, and run directly."""
import os
import subprocess

from test_cli_page_feed_host import CSRC, LIB, ROOT, own_env

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FT_LIB = os.path.join(os.environ.get("FT_PREFIX", "/opt/conda"), "lib")


def test_font_tables_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    env = own_env(cxx)
    exe = str(tmp_path / "decode_font_check")
    # the runtimes are linked statically: the program then runs whatever else the loader brings in before it
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(CSRC, "hip", "decode_font_check.cpp"), "-L" + LIB, "-lfocr_raster",
                    "-Wl,-rpath," + LIB, "-Wl,-rpath-link," + FT_LIB], check=True, env=env)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "DejaVuSansMono.ttf")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stderr == "", r.stderr  # no sanitizer report
    assert r.stdout == "font tables ok\n"
