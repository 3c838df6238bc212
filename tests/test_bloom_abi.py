"""Bloom on a machine without a GPU: the entry points (header, binding, C++ mirror, python wrappers), the record's layout, the definition in the
header in front of the calls, the records of the stages in front unchanged, the build rules, one copy of the arithmetic and of the tonemapper,
the kernels' resource figures, every refusal that needs no device, and the arbiters under the address and undefined-behaviour sanitizers in a
program of its own (tests/cpp/bloom_sanitize.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
ENTRY_POINTS = {"arctic_bloom_device": 5, "arctic_bloom": 5, "arctic_read_bloom": 6, "arctic_bloom_info": 2, "arctic_bloom_layout": 4, "arctic_bloom_pyramid": 6,
                "arctic_bloom_pixels": 8}
MODULE_LEVEL = ("bloom_layout", "bloom_pyramid", "bloom_pixels")
NO_HANDLE = ("arctic_bloom_layout", "arctic_bloom_pyramid", "arctic_bloom_pixels")
FIELDS = ["flags", "threshold", "soft_knee", "clamp_max", "intensity", "spread", "levels", "reserved"]
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
    m = re.search(r"typedef struct ArcticBloom \{(.*?)\} ArcticBloom;", header, re.S)
    assert [f.split()[-1] for f in m.group(1).split(";") if f.strip()] == FIELDS
    dt = pkg.scene.BLOOM_DTYPE
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert dt.fields["flags"][0] == dt.fields["levels"][0] == dt.fields["reserved"][0] == np.dtype("<u4")
    assert "static_assert(sizeof(ArcticBloom) == 32" in open(os.path.join(CSRC, "bloom.cpp")).read()
    for name, value in (("SOURCE_COMPOSED", 1), ("SOURCE_TAA", 2), ("SOURCE_MOTION_BLUR", 4), ("SOURCE_DOF", 8)):
        assert re.search(r"#define ARCTIC_BLOOM_" + name + r"\s+" + str(value) + "u", header) and getattr(lib, "BLOOM_" + name) == value
    # the stages in front are what they were: bloom is the stage behind them, not a flag of any
    assert "#define ARCTIC_MB_SOURCE_TAA       4u" in text and "#define ARCTIC_DOF_SOURCE_MOTION_BLUR  4u   /* a NULL colour = the latest motion blur's HDR output; at most one of the three */" in text
    assert not re.search(r"ARCTIC_(MB|DOF|TAA|COMPOSE)_SOURCE_BLOOM", text)
    dof = re.search(r"typedef struct ArcticDof \{(.*?)\} ArcticDof;", header, re.S).group(1)
    assert [f.split()[-1] for f in dof.split(";") if f.strip()] == ["flags", "focus_distance", "coc_scale", "max_radius", "samples", "depth_extent", "z_near", "z_far"]
    assert pkg.scene.DOF_DTYPE.itemsize == 32 and pkg.scene.MOTION_BLUR_DTYPE.itemsize == 32
    # the definition stands in the header, in front of the calls
    for phrase in ("W_k = (W_{k-1} + 1) / 2, H_k = (H_{k-1} + 1) / 2 in integer division", "a level of 1 x 1 is valid", "x = C[q] > 0 ? min(C[q], clamp_max) : 0",
                   "a NaN fails the test and becomes 0", "br = max(x.r, max(x.g, x.b))", "knee = threshold * soft_knee", "t = br - (threshold - knee)", "t = min(max(t, 0), 2 * knee)",
                   "soft = (t * t) / (4 * knee + 1e-5f)", "m = max(soft, br - threshold)", "contrib = min(m / max(br, 1e-5f), 1)", "b[q] = x * contrib",
                   "S~(i, j) = S[clamp(2x - 2 + i, 0, Ws - 1), clamp(2y - 2 + j, 0, Hs - 1)]", "Box(a, b) = ((S~(a,b) + S~(a+1,b)) + (S~(a,b+1) + S~(a+1,b+1))) * 0.25",
                   "Group(a, b) = ((Box(a,b) + Box(a+2,b)) + (Box(a,b+2) + Box(a+2,b+2))) * 0.25", "G0 = Group(1,1), G1 = Group(0,0), G2 = Group(2,0), G3 = Group(0,2), G4 = Group(2,2)",
                   "36 texels and 13 distinct boxes", "out = G0 * 0.5 + ((G1 + G2) + (G3 + G4)) * 0.125", "l_g = (0.2126f * G.r + 0.7152f * G.g) + 0.0722f * G.b",
                   "w_0 = 0.5f / (1 + l_0), w_g = 0.125f / (1 + l_g) for g = 1..4", "num = w_0 * G0 + ((w_1 * G1 + w_2 * G2) + (w_3 * G3 + w_4 * G4))",
                   "den = w_0 + ((w_1 + w_2) + (w_3 + w_4)); out = num / den", "D_1 = DOWN_karis(b, W, H), and D_k = DOWN(D_{k-1}, W_{k-1}, H_{k-1}) for k = 2..L",
                   "With h = x >> 1: even x has base = h - 2", "wx = (0.0625f, 0.3125f, 0.4375f, 0.1875f)", "odd x has base = h - 1 and wx = (0.1875f, 0.4375f, 0.3125f, 0.0625f)",
                   "its weights are exact sixteenths", "T~(i, j) = T[clamp(bx + i, 0, Wt - 1), clamp(by + j, 0, Ht - 1)]",
                   "r_j = (wx0 * T~(0,j) + wx1 * T~(1,j)) + (wx2 * T~(2,j) + wx3 * T~(3,j))", "out = (wy0 * r_0 + wy1 * r_1) + (wy2 * r_2 + wy3 * r_3)",
                   "U_L = D_L.  For k = L-1 .. 1, U_k = D_k + spread * UP(U_{k+1}) at level k's size", "B = UP(U_1, W_1, H_1) at the frame's size", "a = intensity * B per channel",
                   "out = a > 0 ? C[p] + a : C[p]", "a pixel that no bloom reaches keeps its bits, a NaN included", "exactly as k_dof_gather carries it out",
                   "Every D_k and U_k is finite and >= 0 whatever C holds", "If every pixel has br <= threshold - knee, every plane is +0 and out equals C by bits",
                   "corner-centred", "no lens dirt and no per-level tint", "Only whole frames are handled", "every refusal comes before anything is enqueued", "reserved != 0",
                   "min and max are the motion blur's", "Every clamp(i, lo, hi) of an index is an integer clamp"):
        assert phrase in text, phrase
    assert text.index("int arctic_dof_focus_at(") < text.index("out = a > 0 ? C[p] + a : C[p]") < text.index("typedef struct ArcticBloom") < text.index("int arctic_bloom_device(")
    assert text.index("int arctic_bloom_device(") < text.index("int arctic_read_bloom(") < text.index("int arctic_bloom_layout(") < text.index("int arctic_bloom_pixels(")
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "arctic_bloom_device" in open(os.path.join(ROOT, name)).read(), name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "\n## 6v." in design and design.index("\n## 6u.") < design.index("\n## 6v.")
    for name, needle in (("tools/README.md", "bloom_time.py"), ("profiles/README.md", "bloom_cost.json")):
        assert needle in open(os.path.join(ROOT, name)).read(), name
    # the build rules
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^bloom\.o: bloom\.hip.*bloom\.h.*post_process\.h.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M) and "asm-bloom:" in make
    assert re.search(r"^bloom_host\.o: bloom\.cpp.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M)
    assert re.search(r"^bloom_calls\.o: bloom_calls\.cpp renderer_state\.h.*bloom\.h.*\n\t\$\(HIPCC\) \$\(COMMON\) -c ", make, flags=re.M)
    objs = make.split("OBJS")[1].split("\n")[0]
    assert objs.rstrip().endswith(" dof_host.o bloom.o bloom_calls.o bloom_host.o") and " dof.o " in objs             # appended, nothing reordered
    assert re.search(r"^\.PHONY:.* asm-bloom\b", make, flags=re.M) and "ARCTIC_BLOOM_UNSTAGED" not in make
    # one copy of the arithmetic: the kernels and the arbiters call bloom.h's functions; one copy of the tonemapper
    for unit in ("bloom.hip", "bloom.cpp"):
        source = open(os.path.join(CSRC, unit)).read()
        for fn in ("bloom_prefilter(", "bloom_down<true>(", "bloom_down<false>(", "bloom_up(", "bloom_up_add(", "bloom_composite("):
            assert fn in source, (unit, fn)
        for literal in ("0.2126f", "0.4375f", "1e-5f", "0.125f"):                # the definition's numbers live in bloom.h alone
            assert literal not in source, (unit, literal)
    hip = open(os.path.join(CSRC, "bloom.hip")).read()
    assert '#include "post_process.h"' in hip and "rrt_odt" not in hip and not re.search(r"atomic\w*\s*\(", hip)
    code = re.sub(r"//.*", "", hip)
    assert code.count("__syncthreads()") == 1 and code.count("__shared__") == 1 and "extern __shared__" not in code             # one barrier, static LDS, in the first kernel
    first = code[code.index("#else"):code.index("#endif")]
    assert "__syncthreads()" in first and "return" not in first[:first.index("__syncthreads()")]                                # every thread reaches it
    assert "hip" not in re.sub(r"//.*", "", open(os.path.join(CSRC, "bloom.cpp")).read()).replace("arctic_hip.h", "")          # no HIP type in the host unit
    calls = open(os.path.join(CSRC, "bloom_calls.cpp")).read()
    assert '#include "renderer_state.h"' in calls and all(("int " + n + "(") in calls for n in ENTRY_POINTS if n not in NO_HANDLE)
    ray_calls = open(os.path.join(CSRC, "ray_calls.cpp")).read()
    assert "bloom" not in ray_calls.lower()                                      # a unit of its own: nothing moved into or out of the largest one
    state = open(os.path.join(CSRC, "renderer_state.h")).read()
    assert re.search(r"struct Bloom \{.*?StreamMark written;.*?device_bytes\(\).*?\} bloom;", state, re.S)
    assert "r->bloom.valid = false;" in open(os.path.join(CSRC, "renderer.cpp")).read()


def test_refusals_of_the_host_functions_and_of_a_null_handle(pkg, lib):
    L = lib.lib()
    R = pkg.renderer
    c = np.full((2, 2, 3), 4.0, np.float32)
    lay = R.bloom_layout(17, 9, 8)
    assert lay["sizes"] == [(9, 5), (5, 3), (3, 2), (2, 1), (1, 1), (1, 1), (1, 1), (1, 1)] and lay["offsets"][:3] == [0, 135, 180]
    assert lay["down_floats"] == 135 + 45 + 18 + 6 + 4 * 3 and lay["up_floats"] == lay["down_floats"] - 3
    assert R.bloom_layout(1, 1, 1) == {"sizes": [(1, 1)], "offsets": [0], "down_floats": 3, "up_floats": 0}
    down, up = R.bloom_pyramid(c, levels=2)
    assert [d.shape for d in down] == [(1, 1, 3), (1, 1, 3)] and [u.shape for u in up] == [(1, 1, 3)]
    assert R.bloom_pixels(np.zeros((0, 2)), c, up[0]).shape == (0, 3)
    assert R.bloom_pyramid(c, levels=1)[1] == []
    for bad in (dict(flags=16), dict(flags=3), dict(flags=6), dict(flags=9), dict(flags=12), dict(flags=15), dict(flags=0x80000000), dict(threshold=-0.5), dict(threshold=65505.0),
                dict(threshold=np.nan), dict(threshold=np.inf), dict(soft_knee=-0.5), dict(soft_knee=1.5), dict(soft_knee=np.nan), dict(clamp_max=0.0), dict(clamp_max=-1.0),
                dict(clamp_max=65505.0), dict(clamp_max=np.nan), dict(clamp_max=np.inf), dict(intensity=-0.5), dict(intensity=16.5), dict(intensity=np.nan), dict(spread=-0.5),
                dict(spread=1.5), dict(spread=np.nan), dict(levels=0), dict(levels=9)):
        with pytest.raises(R.ArcticError):
            R.bloom_pyramid(c, **bad)
        with pytest.raises(R.ArcticError):
            R.bloom_pixels([[0, 0]], c, up[0], **bad)
    reserved = R._bloom_arguments(0, 1.0, 0.5, 65504.0, 0.5, 1.0, 2)
    reserved["reserved"] = 7
    with pytest.raises(R.ArcticError):
        R.bloom_pyramid(c, bloom=reserved)
    with pytest.raises(R.ArcticError):
        R.bloom_pixels([[0, 0]], c, up[0], bloom=reserved)
    for flags in (0, 1, 2, 4, 8):                                                # every single source flag is a valid record
        assert R.bloom_pixels([[1, 1]], c, up[0], flags=flags, levels=2).shape == (1, 3)
    for xy in ([[2, 0]], [[0, 2]], [[-1, 0]]):
        with pytest.raises(R.ArcticError):
            R.bloom_pixels(xy, c, up[0])
    with pytest.raises(R.ArcticError):
        R.bloom_pixels([[0, 0]], c, np.zeros((2, 2, 3), np.float32))             # U_1 is level 1's size
    with pytest.raises(R.ArcticError):
        R.bloom_pyramid(np.zeros((2, 2, 1)))
    for size in ((0, 4, 1), (4, 0, 1), (16385, 4, 1), (4, 16385, 1), (4, 4, 0), (4, 4, 9)):
        with pytest.raises(R.ArcticError):
            R.bloom_layout(*size)
    good = R._bloom_arguments(0, 1.0, 0.5, 65504.0, 0.5, 1.0, 2)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    d, u, o = np.full(6, 77, np.float32), np.full(3, 77, np.float32), np.full(3, 77, np.float32)
    xy = np.zeros(2, np.int32)
    assert L.arctic_bloom_layout(4, 4, 1, None) == INVALID
    assert L.arctic_bloom_pyramid(None, 2, 2, hp(c), hp(d), hp(u)) == INVALID and L.arctic_bloom_pyramid(hp(good), 2, 2, None, hp(d), hp(u)) == INVALID
    assert L.arctic_bloom_pyramid(hp(good), 2, 2, hp(c), None, hp(u)) == INVALID and L.arctic_bloom_pyramid(hp(good), 2, 2, hp(c), hp(d), None) == INVALID
    assert L.arctic_bloom_pyramid(hp(good), 0, 2, hp(c), hp(d), hp(u)) == INVALID and L.arctic_bloom_pyramid(hp(good), 2, 16385, hp(c), hp(d), hp(u)) == INVALID
    assert L.arctic_bloom_pixels(None, 1, hp(xy), 2, 2, hp(c), hp(u), hp(o)) == INVALID and L.arctic_bloom_pixels(hp(good), 1, None, 2, 2, hp(c), hp(u), hp(o)) == INVALID
    assert L.arctic_bloom_pixels(hp(good), 1, hp(xy), 2, 2, None, hp(u), hp(o)) == INVALID and L.arctic_bloom_pixels(hp(good), 1, hp(xy), 2, 2, hp(c), None, hp(o)) == INVALID
    assert L.arctic_bloom_pixels(hp(good), 1, hp(xy), 2, 2, hp(c), hp(u), None) == INVALID
    assert (d == 77).all() and (u == 77).all() and (o == 77).all()               # a refused call writes nothing
    # a null handle, before any device is touched
    for name, arity in ENTRY_POINTS.items():
        if name not in NO_HANDLE:
            assert getattr(L, name)(*([None] * arity)) == INVALID, name


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_the_kernels_resource_figures(tmp_path):
    """the two forms of k_bloom_down_first and of k_bloom_composite, k_bloom_down and k_bloom_up: no scratch, no stack frame and no call in any
    of them; static LDS in the first kernel alone -- 3 planes x 36 rows x 48 floats = 20736 bytes, far below the 64 KiB a workgroup gets
    without asking -- and none elsewhere.  The figures DESIGN.md 6v quotes are checked against the compiler's"""
    log = subprocess.run(["make", "-C", CSRC, "asm-bloom", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    names = re.findall(r"Function Name: (\S+)", remarks)
    grab = lambda what: [int(x) for x in re.findall(what + r": (\d+)", remarks)]
    r = dict(vgprs=grab(r" VGPRs"), sgprs=grab(r"TotalSGPRs"), scratch=grab(r"ScratchSize \[bytes/lane\]"), lds=grab(r"LDS Size \[bytes/block\]"), waves=grab(r"Occupancy \[waves/SIMD\]"))
    assert len(names) == 6 and [k for k in ("k_bloom_down_first", "k_bloom_downE", "k_bloom_up", "k_bloom_composite") if not any(k in n for n in names)] == [], names
    assert sum("k_bloom_down_first" in n for n in names) == 2 and sum("k_bloom_composite" in n for n in names) == 2      # row-major float3, and the anti-aliasing's tile-major float4
    assert r["scratch"] == [0] * 6, r
    assert [l for n, l in zip(names, r["lds"])] == [20736 if "k_bloom_down_first" in n else 0 for n in names], r
    assert 3 * 36 * 48 * 4 == 20736 and max(r["vgprs"]) <= 160 and min(r["waves"]) >= 3, r
    assert "Dynamic Stack: True" not in remarks
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for n, v, s, w in zip(names, r["vgprs"], r["sgprs"], r["waves"]):
        short = re.search(r"k_bloom_(down_first|down|up|composite)", n).group(0) + (" (history)" if "HistoryColor" in n else "")
        assert f"{short}: {v} VGPRs, {s} SGPRs, {w} waves" in design, (short, v, s, w)
    frame = []
    for line in open(str(tmp_path / "bloom-hip-amdgcn-amd-amdhsa-gfx950.s")):
        m = re.match(r"\s+\.amdhsa_(private_segment_fixed_size|uses_dynamic_stack) (\d+)", line)
        if m:
            frame.append(int(m.group(2)))
        assert "swappc" not in line
    assert frame == [0] * 12, frame


def test_arbiters_under_sanitizers():
    """tests/cpp/bloom_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    driver = os.path.join(ROOT, "tests", "cpp", "bloom_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "bloom_sanitize.cpp"), os.path.join(CSRC, "bloom.cpp")]
    deps = src + [os.path.join(CSRC, h) for h in ("ray_query.h", "bloom.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 49 and all(l.startswith("ok") for l in lines), lines
    for name in ("ordinary-1x1-1", "odd-1x1-8", "ordinary-3x5-5", "odd-17x9-8", "odd-40x24-2", "ordinary-72x40-8", "refusals"):
        assert any(l.startswith("ok " + name) for l in lines), name
