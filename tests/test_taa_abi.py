"""The temporal anti-aliasing on a machine without a GPU: the entry points (header, binding, C++ mirror, python wrappers), the record's layout, the
definition in the header in front of the calls, the build rules, the kernel's resource figures, every refusal that needs no device, and the
arbiter under the address and undefined-behaviour sanitizers in a program of its own (tests/cpp/taa_sanitize.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
ENTRY_POINTS = {"arctic_set_camera_jitter": 3, "arctic_jitter_proj_view": 5, "arctic_taa_resolve_device": 6, "arctic_taa_resolve": 6, "arctic_pass_taa": 5,
                "arctic_taa_reset": 1, "arctic_read_taa": 5, "arctic_taa_info": 2, "arctic_taa_pixels": 9}
MODULE_LEVEL = ("jitter_proj_view", "taa_pixels")
NO_HANDLE = ("arctic_jitter_proj_view", "arctic_taa_pixels")
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
    assert hasattr(pkg.renderer, "taa_jitter")
    # the record: 32 bytes, the fields where the header puts them, the flags
    m = re.search(r"typedef struct ArcticTaa \{(.*?)\} ArcticTaa;", header, re.S)
    assert [f.split()[-1] for f in m.group(1).split(";") if f.strip()] == ["flags", "max_history", "min_weight", "jitter[2]", "reserved[3]"]
    dt = pkg.scene.TAA_DTYPE
    assert dt.itemsize == 32 and [dt.fields[n][1] for n in ("flags", "max_history", "min_weight", "jitter", "reserved")] == [0, 4, 8, 12, 20]
    assert re.search(r"#define ARCTIC_TAA_LUMA_WEIGHT\s+1u", header) and re.search(r"#define ARCTIC_TAA_SOURCE_COMPOSED\s+2u", header)
    assert (lib.TAA_LUMA_WEIGHT, lib.TAA_SOURCE_COMPOSED) == (1, 2)
    # the definition stands in the header, in front of the calls
    for phrase in ("m[4c+0] = m[4c+0] + kx * m[4c+3]", "m[4c+1] = m[4c+1] - ky * m[4c+3]", "kx = (2*jx)/W", "is drawn at s + j", "is NOT CALLED", "arctic_resize keeps the jitter",
                   "velocity2 of a still scene is -j", "off by less than one pixel", "TWO SETS", "32 bytes per pixel", "after arctic_taa_reset and after arctic_resize",
                   "NO G-BUFFER", "lo = (x < lo) ? x : lo and hi = (x > hi) ? x : hi", "a NaN neighbour is ignored", "hx = ((px + 0.5) + vx) + jx",
                   "tested in float before any conversion", "a rejected tap is a SELECT", "S = ((k0 + k1) + k2) + k3", "If !(S > min_weight)",
                   "h = (h < lo) ? lo : h, then h = (h > hi) ? hi : h", "N = min(hn + 1, max_history); a = 1 / N", "out = h + (c - h) * a",
                   "wc = 1 / (1 + max(max(max(c.r, c.g), c.b), 0))", "out = (c*kc + h*kh) / (kc + kh)", "as k_compose carries it out", "the frame's ONE motion call",
                   "leaves T as it was", "every refusal comes before anything is enqueued", "the sky is not reprojected under camera rotation"):
        assert phrase in text, phrase
    assert text.index("out = h + (c - h) * a") < text.index("int arctic_taa_resolve_device(") < text.index("int arctic_pass_taa(") < text.index("int arctic_taa_pixels(")
    assert text.index("int arctic_pass_ray_effects_motion(") < text.index("int arctic_set_camera_jitter(") < text.index("int arctic_jitter_proj_view(") < text.index("typedef struct ArcticTaa")
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "arctic_taa_resolve_device" in open(os.path.join(ROOT, name)).read(), name
    assert "k_taa_resolve" in open(os.path.join(ROOT, "profiles", "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "\n## 6s." in design and "temporal anti-aliasing" not in design.split("\n## 6r.")[1].split("\n## 6s.")[0].split("**Not provided.**")[-1]
    assert "**Not provided.**" in design.split("\n## 6s.")[1].split("\n## 7.")[0]
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^taa\.o: taa\.hip.*taa\.h.*post_process\.h.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M) and "asm-taa:" in make
    assert re.search(r"^taa_host\.o: taa\.cpp.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M)
    assert re.search(r"^compose\.o: compose\.hip.*post_process\.h", make, flags=re.M)
    objs = make.split("OBJS")[1].split("\n")[0]
    assert " taa.o " in objs and " taa_host.o" in objs
    # one copy of the arithmetic: the kernel and the arbiter call taa.h's function; one copy of the tonemapper for the two streaming kernels
    for unit in ("taa.hip", "taa.cpp"):
        assert "taa_pixel(" in open(os.path.join(CSRC, unit)).read(), unit
    for unit in ("taa.hip", "compose.hip"):
        source = open(os.path.join(CSRC, unit)).read()
        assert '#include "post_process.h"' in source and "rrt_odt" not in source, unit
    # the jitter is applied once, immediately behind camera_proj_view in the forward branch, through the public function
    renderer = open(os.path.join(CSRC, "renderer.cpp")).read()
    assert renderer.count("arctic_jitter_proj_view(") == 1
    at = renderer.index("arctic_jitter_proj_view(")
    between = renderer[renderer.rindex("camera_proj_view(", 0, at):at]
    assert between.count("\n") <= 2 and "gp.clip_from_world" in between and "!= 0.0f" in between


def test_refusals_of_the_host_functions_and_of_a_null_handle(pkg, lib):
    L = lib.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)
    m = np.arange(16, dtype=np.float32)
    kept = m.copy()
    for args in ((None, 4, 4, 0.0, 0.0), (p(m), 0, 4, 0.0, 0.0), (p(m), 4, 16385, 0.0, 0.0), (p(m), 4, 4, 1.25, 0.0), (p(m), 4, 4, 0.0, float("nan")), (p(m), 4, 4, float("-inf"), 0.0)):
        assert L.arctic_jitter_proj_view(*args) == INVALID and (m == kept).all()
    assert L.arctic_jitter_proj_view(p(m), 4, 4, 1.0, -1.0) == 0 and (m != kept).any()
    R = pkg.renderer
    cur = np.zeros((2, 2, 3), np.float32)
    assert R.taa_pixels(np.zeros((0, 2)), cur).shape == (0, 4)
    for bad in (dict(flags=4), dict(max_history=0.5), dict(max_history=65536.5), dict(max_history=np.nan), dict(min_weight=1.0), dict(min_weight=-1e-9), dict(jitter=(1.5, 0)),
                dict(jitter=(0, np.nan))):
        with pytest.raises(R.ArcticError):
            R.taa_pixels([[0, 0]], cur, **bad)
    for xy in ([[2, 0]], [[0, 2]], [[-1, 0]]):
        with pytest.raises(R.ArcticError):
            R.taa_pixels(xy, cur)
    with pytest.raises(R.ArcticError):
        R.taa_pixels([[0, 0]], cur, velocity2=np.zeros((2, 2)))
    with pytest.raises(R.ArcticError):
        R.taa_pixels([[0, 0]], cur, prev=np.zeros((2, 3, 4)))
    assert R.taa_pixels([[1, 1]], cur, max_history=65536.0, min_weight=0.999, jitter=(-1.0, 1.0), flags=3).tolist() == [[0.0, 0.0, 0.0, 1.0]]
    # a null handle, before any device is touched
    for name, arity in ENTRY_POINTS.items():
        if name not in NO_HANDLE:
            args = [None, 0.25, 0.25] if name == "arctic_set_camera_jitter" else [None] * arity
            assert getattr(L, name)(*args) == INVALID, name


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_the_kernel_uses_no_scratch_no_stack_and_one_apron_of_lds(tmp_path):
    """k_taa_resolve: no scratch, no stack frame and no call, 8 waves per SIMD, and four aprons of 10 x 10 x 3 floats of LDS per workgroup (4800
    bytes: 8 waves per SIMD take 38400 of a CU's 160 KiB).  The compiler's figures when this was written: 60 VGPRs and 48 SGPRs -- the bound below is what 8 waves per SIMD need, the figures DESIGN.md 6s quotes are checked against the compiler's"""
    log = subprocess.run(["make", "-C", CSRC, "asm-taa", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    names = re.findall(r"Function Name: (\S+)", remarks)
    grab = lambda what: [int(x) for x in re.findall(what + r": (\d+)", remarks)]
    r = dict(vgprs=grab(r" VGPRs"), sgprs=grab(r"TotalSGPRs"), scratch=grab(r"ScratchSize \[bytes/lane\]"), lds=grab(r"LDS Size \[bytes/block\]"), waves=grab(r"Occupancy \[waves/SIMD\]"))
    assert len(names) == 1 and "k_taa_resolve" in names[0], names
    assert r["scratch"] == [0] and r["lds"] == [4 * 10 * 10 * 3 * 4] and r["waves"] == [8] and r["vgprs"][0] <= 64, r
    assert "Dynamic Stack: True" not in remarks
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"k_taa_resolve: {r['vgprs'][0]} VGPRs, {r['sgprs'][0]} SGPRs, scratch 0, {r['lds'][0]} bytes of LDS per workgroup, 8 waves per SIMD" in design, r
    frame = []
    for line in open(str(tmp_path / "taa-hip-amdgcn-amd-amdhsa-gfx950.s")):
        m = re.match(r"\s+\.amdhsa_(private_segment_fixed_size|uses_dynamic_stack) (\d+)", line)
        if m:
            frame.append(int(m.group(2)))
        assert "swappc" not in line
    assert frame == [0, 0], frame


def test_arbiter_under_sanitizers():
    """tests/cpp/taa_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    driver = os.path.join(ROOT, "tests", "cpp", "taa_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "taa_sanitize.cpp"), os.path.join(CSRC, "taa.cpp")]
    deps = src + [os.path.join(CSRC, h) for h in ("ray_query.h", "taa.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 34 and all(l.startswith("ok") for l in lines), lines
    for name in ("empty-1x1", "ordinary-17x9", "luma-40x24", "no-velocity-8x8", "outside-40x24", "nan-17x9", "inf-8x8", "1e30-40x24", "jitter", "refusals"):
        assert any(l.startswith("ok " + name) for l in lines), name
