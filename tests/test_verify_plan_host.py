"""The host's choice of the exact verify's form for a bank (csrc/hip/verify_plan.h: which kernel, how much LDS, which templates
make a chunk) without a device: csrc/hip/verify_plan_check.cpp asserts the plan at the edges its arithmetic has (the last bank of
each whole-bank form, the first and the last chunked one, the bank whose largest record count and largest row count lie in
different chunks).  It is built as a stand-alone program under the sanitizers, with a host compiler alone, and run directly."""
import os
import subprocess

from test_cli_page_feed_host import CSRC, ROOT, own_env


def test_verify_plan_under_sanitizers(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    env = own_env(cxx)
    exe = str(tmp_path / "verify_plan_check")
    # the runtimes are linked statically: the program then runs whatever else the loader brings in before it
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(CSRC, "hip", "verify_plan_check.cpp")], check=True, env=env)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    assert r.stderr == "", r.stderr  # no sanitizer report
    assert r.stdout == "verify plan ok\n"
