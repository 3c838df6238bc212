"""The temporal upscaler's host arbiter and arctic_taa_upscale_jitter under the address and undefined-behaviour sanitizers, in a program of its
own (tests/cpp/taa_upscale_sanitize.cpp; the sanitizers' runtime is never loaded into python)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
PAIRS = ("1x1-1x1", "1x1-4x4", "8x8-16x16", "17x9-29x14", "40x24-64x40", "37x23-148x92")
CASES = ("empty", "ordinary", "luma", "no-clamp", "no-velocity", "outside", "nan", "inf", "1e30", "limits-a", "limits-b")


def test_arbiter_and_jitter_under_sanitizers():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    driver = os.path.join(ROOT, "tests", "cpp", "taa_upscale_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "taa_upscale_sanitize.cpp"), os.path.join(CSRC, "taa_upscale.cpp")]
    deps = src + [os.path.join(CSRC, h) for h in ("ray_query.h", "taa.h", "taa_upscale.h")] + [os.path.join(ROOT, "include", "arctic_hip.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(PAIRS) * len(CASES) + 2 and all(l.startswith("ok") for l in lines), lines
    for pair in PAIRS:
        for case in CASES:
            assert any(l.startswith(f"ok {case}-{pair}:") for l in lines), (case, pair)
    assert any(l.startswith("ok jitter") for l in lines) and any(l.startswith("ok refusals: 33") for l in lines)
    # the hostile cases did what they are for: a full history blends, and velocities that point far outside blend nothing
    blended = {l.split(":")[0][3:]: int(l.split("flags")[1].split(":")[1].split("blended")[0]) for l in lines if " blended" in l}
    assert blended["ordinary-40x24-64x40"] > 1000 and blended["outside-40x24-64x40"] == 0 and blended["empty-37x23-148x92"] == 0
