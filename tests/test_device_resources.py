"""The owning resource types of arctic-renderer_amd/csrc/device_resources.h on a machine without a GPU: the sequence of runtime calls each owner makes and
that everything is released exactly once -- over a fake runtime, under the address and undefined-behaviour sanitizers, in a program of its own
(tests/cpp/resources_sanitize.cpp) -- and that the host units of the handle (renderer_state.h and whatever includes it) release nothing by hand any more."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
CASES = ("devbuf-ensure-and-exact", "ring3-seven-uploads", "ring1-waits-only-when-pending", "ring-slot-grows-and-is-kept", "move-vector-growth",
         "failed-allocation-leaves-empty", "stream-waits-then-goes-once", "mark-never-recorded-never-waited-for", "mark-same-stream-elided-others-wait",
         "mark-forget", "mark-generations", "mark-ring-of-three-sets", "reader-table", "mark-moves-and-release", "all-released-once")


def test_owners_under_sanitizers():
    """tests/cpp/resources_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python); it links no HIP library"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if not os.path.exists(os.path.join(HIP_INCLUDE, "hip", "hip_runtime_api.h")):
        pytest.skip("no HIP headers")
    driver = os.path.join(ROOT, "tests", "cpp", "resources_sanitize")
    src = os.path.join(ROOT, "tests", "cpp", "resources_sanitize.cpp")
    deps = [src, os.path.join(CSRC, "device_resources.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE, "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-o", driver, src])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=120, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert lines and all(l.startswith("ok ") for l in lines), report[-3000:]
    assert [l[3:] for l in lines] == list(CASES)


def test_renderer_releases_nothing_by_hand():
    """the handle's units -- renderer_state.h and every host unit that includes it -- hold what the runtime gave them in owners only: no release call
    of their own, and arctic_destroy names no buffer"""
    units = sorted(n for n in os.listdir(CSRC) if n.endswith(".cpp") and re.search(r'#include\s+"renderer_state\.h"', open(os.path.join(CSRC, n)).read()))
    assert {"renderer.cpp", "ray_calls.cpp", "exchange_calls.cpp"} <= set(units), units
    text = "".join(open(os.path.join(CSRC, n)).read() for n in ["renderer_state.h"] + units)
    for call in ("hipFree", "hipHostFree", "hipEventDestroy", "hipStreamDestroy"):
        assert not re.search(r"\b" + call + r"\b", text), call
    m = re.findall(r"^void arctic_destroy\(ArcticRenderer \*r\) \{\n(.*?)^\}\n", text, flags=re.S | re.M)
    assert len(m) == 1, "arctic_destroy not found (once)"
    body = m[0]
    assert "delete r;" in body and "arctic_comm_destroy(r)" in body
    assert not re.search(r"\bd_\w+", body), body
    # ... and order their streams through marks only (device_resources.h StreamMark, ReaderTable): no wait of their own, no record but the timing
    # events of arctic_time_shade, none of the companion state the marks replaced
    assert "hipStreamWaitEvent" not in text
    timing = re.findall(r"^int arctic_time_shade\(.*?^\}\n", text, flags=re.S | re.M)
    assert len(timing) == 1, "arctic_time_shade not found (once)"
    assert "hipEventRecord" in timing[0] and "hipEventRecord" not in text.replace(timing[0], "")
    for gone in ("released_valid", "shadow_released_valid", "shadow_scratch_stream", "shadow_scratch_valid", "skin_seq"):
        assert gone not in text, gone
    # the header the owners live in stays free of the project: nothing but the HIP runtime's API and the standard library
    header = open(os.path.join(CSRC, "device_resources.h")).read()
    assert re.findall(r'#include\s+"([^"]+)"', header) == []
    assert [h for h in re.findall(r"#include\s+<([^>]+)>", header) if h.startswith("hip")] == ["hip/hip_runtime_api.h"]
