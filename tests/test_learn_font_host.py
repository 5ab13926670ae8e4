"""The learned font (csrc/hip/learn_font.h: the bounding rectangle of a phase's ink, its growth clipped to the box, the mean rounded
half up, the min_count edge, a zero count, the refusals; focr_decode_font_learn calls it) and focr_decoder_learn_text's own two
rules (text_plan.h: the font to learn, the 2^24 listed characters) without a device: csrc/hip/learn_font_check.cpp asserts them on
a font filled by hand.  It is built as a stand-alone program under the sanitizers, with a host compiler alone, and run directly."""
import os
import subprocess

from test_cli_page_feed_host import CSRC, ROOT, own_env

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_learn_font_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    env = own_env(cxx)
    exe = str(tmp_path / "learn_font_check")
    # the runtimes are linked statically: the program then runs whatever else the loader brings in before it
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(CSRC, "hip", "learn_font_check.cpp")], check=True, env=env)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stderr == "", r.stderr  # no sanitizer report
    assert r.stdout == "learn font ok\n"
