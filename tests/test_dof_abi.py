"""Depth of field on a machine without a GPU: the entry points (header, binding, C++ mirror, python wrappers), the record's layout, the definition
in the header in front of the calls, the build rules, the kernels' resource figures, every refusal that needs no device, and the arbiters under
the address and undefined-behaviour sanitizers in a program of its own (tests/cpp/dof_sanitize.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
ENTRY_POINTS = {"arctic_dof_device": 7, "arctic_dof": 7, "arctic_pass_dof": 6, "arctic_read_dof": 7, "arctic_dof_info": 2, "arctic_dof_prepare": 7, "arctic_dof_pixels": 10,
                "arctic_dof_coc_scale": 6, "arctic_dof_focus_at": 6}
MODULE_LEVEL = ("dof_prepare", "dof_pixels", "dof_coc_scale")
NO_HANDLE = ("arctic_dof_prepare", "arctic_dof_pixels", "arctic_dof_coc_scale")
FIELDS = ["flags", "focus_distance", "coc_scale", "max_radius", "samples", "depth_extent", "z_near", "z_far"]
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
    assert hasattr(pkg.renderer, "dof_taps")
    # the record: 32 bytes, the fields where the header puts them, the flags
    m = re.search(r"typedef struct ArcticDof \{(.*?)\} ArcticDof;", header, re.S)
    assert [f.split()[-1] for f in m.group(1).split(";") if f.strip()] == FIELDS
    dt = pkg.scene.DOF_DTYPE
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert "static_assert(sizeof(ArcticDof) == 32" in open(os.path.join(CSRC, "dof.cpp")).read()
    for name, value in (("SOURCE_COMPOSED", 1), ("SOURCE_TAA", 2), ("SOURCE_MOTION_BLUR", 4)):
        assert re.search(r"#define ARCTIC_DOF_" + name + r"\s+" + str(value) + "u", header) and getattr(lib, "DOF_" + name) == value
    # the motion blur's record is what it was: depth of field is the stage behind it, not a flag of it
    assert "#define ARCTIC_MB_SOURCE_TAA       4u" in text and "ARCTIC_MB_SOURCE_DOF" not in text
    # the definition stands in the header, in front of the calls
    for phrase in ("den = f - d * (f - n)", "zv = (n * f) / den if den > 0", "else zv = f (a NaN fails the test)", "f / (f - n) * (1 - n / dist)",
                   "s = coc_scale * (1 - focus_distance / zv)", "If s is not finite, s = 0", "s = min(max(s, -max_radius), max_radius)", "a_p = max(|s_p|, A0) with A0 = 0.5641896f",
                   "P[p] = {s_p, zv_p}", "the largest |s_p| over the tile's pixels inside the frame", "Rt = ceil(max_radius / 8)", "If !(R > 0.5):  out = C[p], bit for bit",
                   "k = (R * R) / samples, w = 0.31830987f / (a_p * a_p), acc = C[p] * w, entered = false", "ox = u.x * R, oy = u.y * R", "qx = floor((px + 0.5) + ox)",
                   "tested in float before any conversion; a NaN fails", "dist = sqrt(ox*ox + oy*oy)", "behind = clamp01((z_q - z_p) / depth_extent)",
                   "e = a_q - behind * (a_q - min(a_q, a_p))", "cover = clamp01(e - dist)", "a = (cover * k) / (a_q * a_q)", "is a SELECT: nothing of it is read",
                   "a NaN colour never spreads through a zero weight", "out = entered ? acc / w : C[p]", "as k_motion_blur carries it out", "sampled sparsely",
                   "normalised, not alpha-composited", "The sky sits at about z_far", "every refusal comes before anything is enqueued", "only this call accepts zeros there",
                   "fl = focal_length_mm * 0.001", "c = (fl * fl) / (f_number * (focus_distance - fl))", "((0.5 * c) / (sensor_height_mm * 0.001)) * height_px"):
        assert phrase in text, phrase
    assert text.index("out = entered ? acc / w : C[p]") < text.index("int arctic_dof_device(") < text.index("int arctic_pass_dof(") < text.index("int arctic_dof_pixels(")
    assert text.index("int arctic_motion_blur_pixels(") < text.index("typedef struct ArcticDof")
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "arctic_dof_device" in open(os.path.join(ROOT, name)).read(), name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "\n## 6u." in design and design.index("\n## 6t.") < design.index("\n## 6u.")
    for name, needle in (("tools/README.md", "dof_time.py"), ("profiles/README.md", "dof_cost.json")):
        assert needle in open(os.path.join(ROOT, name)).read(), name
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^dof\.o: dof\.hip.*dof\.h.*post_process\.h.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M) and "asm-dof:" in make
    assert re.search(r"^dof_host\.o: dof\.cpp.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M)
    objs = make.split("OBJS")[1].split("\n")[0]
    assert " dof.o " in objs and " dof_host.o" in objs
    # one copy of the arithmetic: the kernels and the arbiters call dof.h's functions; one copy of the tonemapper
    for unit in ("dof.hip", "dof.cpp"):
        source = open(os.path.join(CSRC, unit)).read()
        for fn in ("dof_signed_radius(", "dof_neighbour_max(", "dof_pixel("):
            assert fn in source, (unit, fn)
    hip = open(os.path.join(CSRC, "dof.hip")).read()
    assert '#include "post_process.h"' in hip and "rrt_odt" not in hip and not re.search(r"atomic\w*\s*\(", hip) and "__shared__" not in hip and "__syncthreads" not in hip
    assert "hip" not in re.sub(r"//.*", "", open(os.path.join(CSRC, "dof.cpp")).read()).replace("arctic_hip.h", "")    # no HIP type in the host unit


def test_refusals_of_the_host_functions_and_of_a_null_handle(pkg, lib):
    L = lib.lib()
    R = pkg.renderer
    z, c = np.full((2, 2), 0.5, np.float32), np.ones((2, 2, 3), np.float32)
    tile, near, P = R.dof_prepare(z)
    assert tile.shape == near.shape == (1, 1) and P.shape == (2, 2, 2) and tile[0, 0] == 16.0 and (P[..., 0] == -16.0).all()
    assert R.dof_pixels(np.zeros((0, 2)), c, P, near).shape == (0, 3)
    for bad in (dict(flags=8), dict(flags=3), dict(flags=6), dict(flags=5), dict(flags=7), dict(focus_distance=0.0), dict(focus_distance=-1.0), dict(focus_distance=np.nan),
                dict(focus_distance=np.inf), dict(coc_scale=-0.5), dict(coc_scale=4097.0), dict(coc_scale=np.nan), dict(coc_scale=np.inf), dict(max_radius=0.5), dict(max_radius=65.0),
                dict(max_radius=np.nan), dict(samples=0), dict(samples=65), dict(depth_extent=0.0), dict(depth_extent=-1.0), dict(depth_extent=np.nan), dict(depth_extent=np.inf),
                dict(z_near=0.0), dict(z_near=-1.0), dict(z_near=np.nan), dict(z_far=0.05), dict(z_far=0.1), dict(z_far=np.inf), dict(z_far=np.nan), dict(z_near=0.0, z_far=0.0)):
        with pytest.raises(R.ArcticError):
            R.dof_prepare(z, **bad)
        with pytest.raises(R.ArcticError):
            R.dof_pixels([[0, 0]], c, P, near, **bad)
    for taps in ([[np.nan, 0.0]], [[0.0, np.inf]], [[0.8, 0.8]], [[0.0, -1.0000002]], np.zeros((0, 2))):
        with pytest.raises(R.ArcticError):
            R.dof_pixels([[0, 0]], c, P, near, taps, samples=1)
    assert R.dof_pixels([[0, 0]], c, P, near, [[0.0, -1.0], [1.0, 0.0]], samples=2).shape == (1, 3)      # the rim is inside
    for xy in ([[2, 0]], [[0, 2]], [[-1, 0]]):
        with pytest.raises(R.ArcticError):
            R.dof_pixels(xy, c, P, near)
    with pytest.raises(R.ArcticError):
        R.dof_pixels([[0, 0]], c, P[:1], near)
    with pytest.raises(R.ArcticError):
        R.dof_prepare(np.zeros((2, 2, 1)))
    assert R.dof_pixels([[1, 1]], c, P, near, focus_distance=1e30, coc_scale=4096.0, max_radius=64.0, samples=64, depth_extent=1e-30, flags=4).tolist() == [[1.0, 1.0, 1.0]]
    # the thin lens
    assert abs(R.dof_coc_scale(2.0, 50.0, 24.0, 2.0, 1080) - 14.4231) < 1e-3
    fl = np.float32(50.0) * np.float32(0.001)
    want = ((np.float32(0.5) * ((fl * fl) / (np.float32(2.0) * (np.float32(2.0) - fl)))) / (np.float32(24.0) * np.float32(0.001))) * np.float32(1080)
    assert np.float32(R.dof_coc_scale(2.0, 50.0, 24.0, 2.0, 1080)) == want
    for bad in ((0.0, 50.0, 24.0, 2.0, 1080), (np.nan, 50.0, 24.0, 2.0, 1080), (2.0, 0.0, 24.0, 2.0, 1080), (2.0, np.inf, 24.0, 2.0, 1080), (2.0, 50.0, -1.0, 2.0, 1080),
                (2.0, 50.0, 24.0, 0.05, 1080), (2.0, 50.0, 24.0, np.nan, 1080), (2.0, 50.0, 24.0, np.inf, 1080), (2.0, 50.0, 24.0, 2.0, 0), (2.0, 50.0, 24.0, 2.0, 16385)):
        with pytest.raises(R.ArcticError):
            R.dof_coc_scale(*bad)
    assert L.arctic_dof_coc_scale(2.0, 50.0, 24.0, 2.0, 1080, None) == INVALID
    # a null handle, before any device is touched
    for name, arity in ENTRY_POINTS.items():
        if name not in NO_HANDLE:
            args = [None, 0.1, 1000.0, 0, 0, None] if name == "arctic_dof_focus_at" else [None] * arity
            assert getattr(L, name)(*args) == INVALID, name


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_the_kernels_use_no_scratch_no_stack_and_no_lds(tmp_path):
    """k_dof_prepare, k_dof_neighbour_max and the two forms of k_dof_gather: no scratch, no stack frame and no call in any of them, no LDS in
    k_dof_prepare (its reduction is wave-wide shuffles) nor in the others, 8 waves per SIMD.  The figures DESIGN.md 6u quotes are checked
    against the compiler's"""
    log = subprocess.run(["make", "-C", CSRC, "asm-dof", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    names = re.findall(r"Function Name: (\S+)", remarks)
    grab = lambda what: [int(x) for x in re.findall(what + r": (\d+)", remarks)]
    r = dict(vgprs=grab(r" VGPRs"), sgprs=grab(r"TotalSGPRs"), scratch=grab(r"ScratchSize \[bytes/lane\]"), lds=grab(r"LDS Size \[bytes/block\]"), waves=grab(r"Occupancy \[waves/SIMD\]"))
    assert len(names) == 4 and [k for k in ("k_dof_prepare", "k_dof_neighbour_max", "k_dof_gather") if not any(k in n for n in names)] == [], names
    assert sum("k_dof_gather" in n for n in names) == 2                           # row-major float3, and the anti-aliasing's tile-major float4
    assert r["scratch"] == [0] * 4 and r["lds"] == [0] * 4 and r["waves"] == [8] * 4 and max(r["vgprs"]) <= 64, r
    assert "Dynamic Stack: True" not in remarks
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n, v, s in zip(names, r["vgprs"], r["sgprs"]):
        short = re.search(r"k_dof_[a-z_]+", n).group(0) + (" (history)" if "HistoryColor" in n else "")
        assert f"{short}: {v} VGPRs, {s} SGPRs" in design, (short, v, s)
    frame = []
    for line in open(str(tmp_path / "dof-hip-amdgcn-amd-amdhsa-gfx950.s")):
        m = re.match(r"\s+\.amdhsa_(private_segment_fixed_size|uses_dynamic_stack) (\d+)", line)
        if m:
            frame.append(int(m.group(2)))
        assert "swappc" not in line
    assert frame == [0] * 8, frame


def test_arbiters_under_sanitizers():
    """tests/cpp/dof_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    driver = os.path.join(ROOT, "tests", "cpp", "dof_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "dof_sanitize.cpp"), os.path.join(CSRC, "dof.cpp")]
    deps = src + [os.path.join(CSRC, h) for h in ("ray_query.h", "dof.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 43 and all(l.startswith("ok") for l in lines), lines
    for name in ("ordinary-1x1", "rim-17x9", "one-tap-8x8", "64-taps-72x40", "planes-40x24", "nan-17x9", "inf-8x8", "1e30-72x40", "odd-planes", "thin-lens", "refusals"):
        assert any(l.startswith("ok " + name) for l in lines), name
