"""The input rules of a reading the caller supplies (csrc/hip/text_plan.h: the guards, the per-line checks with the running sum
and the page ranges, the per-character checks; focr_decoder_verify_text and focr_decoder_score_text both call them) without a
device: csrc/hip/text_plan_check.cpp asserts the plan at the edges its arithmetic has.  It is built as a stand-alone program under
the sanitizers, with a host compiler alone, and run directly."""
import os
import subprocess

from test_cli_page_feed_host import CSRC, ROOT, own_env

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_text_plan_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    env = own_env(cxx)
    exe = str(tmp_path / "text_plan_check")
    # the runtimes are linked statically: the program then runs whatever else the loader brings in before it
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(CSRC, "hip", "text_plan_check.cpp")], check=True, env=env)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stderr == "", r.stderr  # no sanitizer report
    assert r.stdout == "text plan ok\n"
