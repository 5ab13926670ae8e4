"""The host plan of a forced alignment (csrc/hip/align_plan.h: the radii, the nominal pens from the host font records' increments,
the 2^24 rule, the whole origin_x, the backpointers' budget and the record the device reads; focr_decoder_align_text calls it)
without a device: csrc/hip/align_plan_check.cpp asserts the plan at the edges its arithmetic has.  It is built as a stand-alone
program under the sanitizers, with a host compiler alone, and run directly."""
import os
import subprocess

from test_cli_page_feed_host import CSRC, ROOT, own_env

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_align_plan_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    env = own_env(cxx)
    exe = str(tmp_path / "align_plan_check")
    # the runtimes are linked statically: the program then runs whatever else the loader brings in before it
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(CSRC, "hip", "align_plan_check.cpp")], check=True, env=env)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stderr == "", r.stderr  # no sanitizer report
    assert r.stdout == "align plan ok\n"
