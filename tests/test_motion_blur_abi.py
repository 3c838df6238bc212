"""The motion blur on a machine without a GPU: the entry points (header, binding, C++ mirror, python wrappers), the record's layout, the definition
in the header in front of the calls, the build rules, the kernels' resource figures, every refusal that needs no device, and the arbiters under
the address and undefined-behaviour sanitizers in a program of its own (tests/cpp/motion_blur_sanitize.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
ENTRY_POINTS = {"arctic_motion_blur_device": 7, "arctic_motion_blur": 7, "arctic_depth_plane_device": 2, "arctic_pass_motion_blur": 5, "arctic_read_motion_blur": 7,
                "arctic_motion_blur_info": 2, "arctic_motion_blur_prepare": 8, "arctic_motion_blur_pixels": 9}
MODULE_LEVEL = ("motion_blur_prepare", "motion_blur_pixels")
NO_HANDLE = ("arctic_motion_blur_prepare", "arctic_motion_blur_pixels")
HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")
INVALID = -1


@pytest.fixture(scope="module")
def lib(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def test_entry_points_binding_and_mirror(pkg, lib):
    text = open(os.path.join(ROOT, "include", "arctic_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = lib.lib()
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m and len(m.group(1).split(",")) == arity, name
        assert name in lib.header_symbols() and hasattr(L, name)
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == arity
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True) if shutil.which("nm") else None
    if exported is not None:
        for name in ENTRY_POINTS:
            assert re.search(r" T " + name + r"$", exported, re.M), name
    hpp = open(os.path.join(ROOT, "arctic-renderer_amd", "host", "renderer.hpp")).read()
    for method in [n[len("arctic_"):] for n in ENTRY_POINTS]:
        assert re.search(r"\[\[nodiscard\]\]\s+(static\s+)?bool\s+" + method + r"\s*\(", hpp), method
        assert hasattr(pkg.renderer, method) if method in MODULE_LEVEL else hasattr(pkg.renderer.Renderer, method), method
    # the record: 32 bytes, the fields where the header puts them, the flags
    m = re.search(r"typedef struct ArcticMotionBlur \{(.*?)\} ArcticMotionBlur;", header, re.S)
    assert [f.split()[-1] for f in m.group(1).split(";") if f.strip()] == ["flags", "shutter", "max_radius", "samples", "depth_extent", "reserved[3]"]
    dt = pkg.scene.MOTION_BLUR_DTYPE
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in ("flags", "shutter", "max_radius", "samples", "depth_extent", "reserved")] == [0, 4, 8, 12, 16, 20]
    for name, value in (("DITHER", 1), ("SOURCE_COMPOSED", 2), ("SOURCE_TAA", 4)):
        assert re.search(r"#define ARCTIC_MB_" + name + r"\s+" + str(value) + "u", header) and getattr(lib, "MB_" + name) == value
    # the definition stands in the header, in front of the calls
    for phrase in ("clamp01(x) = !(x > 0) ? 0 : (x > 1 ? 1 : x)", "h_p = velocity2[p] * (0.5 * shutter)", "If either component of h_p is not finite, h_p = (0, 0)",
                   "s = max_radius / len", "l_p = max(sqrt(l2_p), 0.5)", "P[p] = {l_p, z_p}", "lowest lane index (py & 7) * 8 + (px & 7) wins", "Rt = ceil(max_radius / 8)",
                   "visited row-major (dy outer); the first among equals wins", "If !(dl > 0.5):  out = C[p], bit for bit", "w = 1 / l_p, acc = C[p] * w",
                   "o = ((B[py & 3][px & 3] + 0.5) / 16) - 0.5", "{0, 8, 2, 10}, {12, 4, 14, 6}, {3, 11, 1, 9}, {15, 7, 13, 5}", "t = (((i + 0.5) + o) / samples) * 2 - 1",
                   "tested in float before any conversion; a NaN fails", "dist = |t| * dl", "f = clamp01(1 - (z_q - z_p) / depth_extent)", "b = clamp01(1 - (z_p - z_q) / depth_extent)",
                   "cone(l) = clamp01(1 - dist / l)", "cyl(l) = 1 - (s*s) * (3 - 2*s)", "s = clamp01((dist - 0.95*l) / (0.1*l))",
                   "a = (f * cone(l_q) + b * cone(l_p)) + (cyl(l_q) * cyl(l_p)) * 2", "is a SELECT with weight 0", "a NaN colour never spreads through a zero weight",
                   "out = acc / w", "as k_compose and k_taa_resolve carry it out", "non-linear depth", "The sky has\n *   velocity2 = 0", "the paper's behaviour",
                   "every refusal comes before anything is enqueued", "it makes NO motion call", "the frame still has one motion call"):
        assert phrase in text, phrase
    assert text.index("out = acc / w") < text.index("int arctic_motion_blur_device(") < text.index("int arctic_pass_motion_blur(") < text.index("int arctic_motion_blur_pixels(")
    assert text.index("int arctic_taa_pixels(") < text.index("typedef struct ArcticMotionBlur")
    assert "no motion blur" not in text and "motion blur would read" not in text    # the two sentences that said it does not exist
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "arctic_motion_blur_device" in open(os.path.join(ROOT, name)).read(), name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "\n## 6t." in design and "Motion blur;" not in design.split("\n## 6s.")[1].split("\n## 6t.")[0]
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^motion_blur\.o: motion_blur\.hip.*motion_blur\.h.*post_process\.h.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M) and "asm-motion-blur:" in make
    assert re.search(r"^motion_blur_host\.o: motion_blur\.cpp.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M)
    objs = make.split("OBJS")[1].split("\n")[0]
    assert " motion_blur.o " in objs and " motion_blur_host.o" in objs
    # one copy of the arithmetic: the kernels and the arbiters call motion_blur.h's functions; one copy of the tonemapper
    for unit in ("motion_blur.hip", "motion_blur.cpp"):
        source = open(os.path.join(CSRC, unit)).read()
        for fn in ("mb_half_velocity(", "mb_neighbour_max(", "mb_pixel("):
            assert fn in source, (unit, fn)
    hip = open(os.path.join(CSRC, "motion_blur.hip")).read()
    assert '#include "post_process.h"' in hip and "rrt_odt" not in hip and not re.search(r"atomic\w*\s*\(", hip) and "__shared__" not in hip
    # the one TAA flag the pass reads lives on the host: taa.hip is what it was
    assert "by_pass" in open(os.path.join(CSRC, "renderer_state.h")).read() and "by_pass" not in open(os.path.join(CSRC, "taa.hip")).read()


def test_refusals_of_the_host_functions_and_of_a_null_handle(pkg, lib):
    L = lib.lib()
    R = pkg.renderer
    v, c = np.zeros((2, 2, 2), np.float32), np.ones((2, 2, 3), np.float32)
    tile, near, P = R.motion_blur_prepare(v)
    assert tile.shape == near.shape == (1, 1, 2) and P.tolist() == [[[0.5, 0.0]] * 2] * 2
    assert R.motion_blur_pixels(np.zeros((0, 2)), c, P, near).shape == (0, 3)
    for bad in (dict(flags=8), dict(flags=6), dict(shutter=-0.5), dict(shutter=4.5), dict(shutter=np.nan), dict(max_radius=0.5), dict(max_radius=65.0), dict(max_radius=np.nan),
                dict(samples=0), dict(samples=65), dict(depth_extent=0.0), dict(depth_extent=np.nan), dict(depth_extent=np.inf)):
        with pytest.raises(R.ArcticError):
            R.motion_blur_prepare(v, **bad)
        with pytest.raises(R.ArcticError):
            R.motion_blur_pixels([[0, 0]], c, P, near, **bad)
    for xy in ([[2, 0]], [[0, 2]], [[-1, 0]]):
        with pytest.raises(R.ArcticError):
            R.motion_blur_pixels(xy, c, P, near)
    with pytest.raises(R.ArcticError):
        R.motion_blur_pixels([[0, 0]], c, P[:1], near)
    with pytest.raises(R.ArcticError):
        R.motion_blur_prepare(v, depth=np.zeros((2, 3)))
    assert R.motion_blur_pixels([[1, 1]], c, P, near, shutter=4.0, max_radius=64.0, samples=64, depth_extent=1e-30, flags=5).tolist() == [[1.0, 1.0, 1.0]]
    # a null handle, before any device is touched
    for name, arity in ENTRY_POINTS.items():
        if name not in NO_HANDLE:
            assert getattr(L, name)(*([None] * arity)) == INVALID, name


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_the_kernels_use_no_scratch_no_stack_and_no_lds(tmp_path):
    """k_mb_depth, k_mb_tile_max, k_mb_neighbour_max and the two forms of k_motion_blur: no scratch, no stack frame and no call in any of them,
    no LDS in k_mb_tile_max (its reduction is wave-wide shuffles) nor in the others, 8 waves per SIMD.  The figures DESIGN.md 6t quotes are
    checked against the compiler's"""
    log = subprocess.run(["make", "-C", CSRC, "asm-motion-blur", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    names = re.findall(r"Function Name: (\S+)", remarks)
    grab = lambda what: [int(x) for x in re.findall(what + r": (\d+)", remarks)]
    r = dict(vgprs=grab(r" VGPRs"), sgprs=grab(r"TotalSGPRs"), scratch=grab(r"ScratchSize \[bytes/lane\]"), lds=grab(r"LDS Size \[bytes/block\]"), waves=grab(r"Occupancy \[waves/SIMD\]"))
    assert len(names) == 5 and [k for k in ("k_mb_depth", "k_mb_tile_max", "k_mb_neighbour_max", "k_motion_blur") if not any(k in n for n in names)] == [], names
    assert sum("k_motion_blur" in n for n in names) == 2                          # row-major float3, and the anti-aliasing's tile-major float4
    assert r["scratch"] == [0] * 5 and r["lds"] == [0] * 5 and r["waves"] == [8] * 5 and max(r["vgprs"]) <= 64, r
    assert "Dynamic Stack: True" not in remarks
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n, v, s in zip(names, r["vgprs"], r["sgprs"]):
        short = re.search(r"k_m[a-z_]+", n).group(0) + (" (history)" if "HistoryColor" in n else "")
        assert f"{short}: {v} VGPRs, {s} SGPRs" in design, (short, v, s)
    frame = []
    for line in open(str(tmp_path / "motion_blur-hip-amdgcn-amd-amdhsa-gfx950.s")):
        m = re.match(r"\s+\.amdhsa_(private_segment_fixed_size|uses_dynamic_stack) (\d+)", line)
        if m:
            frame.append(int(m.group(2)))
        assert "swappc" not in line
    assert frame == [0] * 10, frame


def test_arbiters_under_sanitizers():
    """tests/cpp/motion_blur_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    driver = os.path.join(ROOT, "tests", "cpp", "motion_blur_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "motion_blur_sanitize.cpp"), os.path.join(CSRC, "motion_blur.cpp")]
    deps = src + [os.path.join(CSRC, h) for h in ("ray_query.h", "motion_blur.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 42 and all(l.startswith("ok") for l in lines), lines
    for name in ("ordinary-1x1", "no-depth-17x9", "one-tap-8x8", "64-taps-72x40", "beyond-40x24", "nan-17x9", "inf-8x8", "1e30-72x40", "odd-planes", "refusals"):
        assert any(l.startswith("ok " + name) for l in lines), name
