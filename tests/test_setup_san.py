"""The host stages of lba_set_problem (amc-slam_amd/csrc/lba_setup.hpp) under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program (tests/native/setup_san.cpp): three synthetic windows (GP
observations with a heavy landmark in several segment tiles and enough landmarks for a multi-piece cut, a free
extrinsic, an empty window) through every stage and the layout fingerprint, with 1 and with 8 set-up threads.  The
program exits non-zero on a sanitizer report or when a window's fingerprint depends on the thread count.  (The
sanitizer runtimes are linked statically, so the program starts whatever else the environment preloads.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_stages_sanitized():
    hip_inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
    src = os.path.join(ROOT, "tests", "native", "setup_san.cpp")
    out = os.path.join(ROOT, "tests", "native", "_build", "setup_san")
    csrc = os.path.join(ROOT, "amc-slam_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "amc_lba.h")] + [
        os.path.join(csrc, h) for h in ("lba_setup.hpp", "lba_device.hpp", "lba_math.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I" + hip_inc, "-pthread",
                               src, "-o", out])
    r = subprocess.run([out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    one, eight = r.stdout.split("8 threads:\n")
    rows = re.findall(r"^(\w+) hash ([0-9a-f]{8}) tiles (\d+) heavy (\d+) segments (\d+)$", eight, re.M)
    assert [n for n, *_ in rows] == ["gp_heavy", "free_extrinsic", "empty"]
    assert one == "1 thread:\n" + eight
    assert int(rows[0][3]) >= 1 and int(rows[0][4]) >= 2 and int(rows[0][2]) > int(rows[0][4])
    assert int(rows[2][2]) == 0
