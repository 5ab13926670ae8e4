"""The host plan of a repair against the composed line error (csrc/hip/refine_plan.h: the radii, the whole origin_x, the rule that a
line's pens do not decrease, the fonts' extents and the window of a step with its LDS sizing; focr_decoder_refine_text calls it)
without a device: csrc/hip/refine_plan_check.cpp asserts the plan at the edges its arithmetic has.  It is built as a stand-alone
program under the sanitizers, with a host compiler alone, and run directly."""
import os
import subprocess

from test_cli_page_feed_host import CSRC, ROOT, own_env

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_refine_plan_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    env = own_env(cxx)
    exe = str(tmp_path / "refine_plan_check")
    # the runtimes are linked statically: the program then runs whatever else the loader brings in before it
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(CSRC, "hip", "refine_plan_check.cpp")], check=True, env=env)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stderr == "", r.stderr  # no sanitizer report
    assert r.stdout == "refine plan ok\n"
