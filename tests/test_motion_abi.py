"""The motion vectors on a machine without a GPU: the entry points (header, binding, C++ mirror, python wrappers), the definition in the header in
front of the calls, the build rules, the three kernels' resource figures, every refusal that needs no device, and the arbiters under the address
and undefined-behaviour sanitizers in a program of its own (tests/cpp/motion_sanitize.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
ENTRY_POINTS = {"arctic_motion_vectors_device": 4, "arctic_motion_vectors": 6, "arctic_motion_reset": 1, "arctic_motion_info": 2, "arctic_motion_pixels": 12,
                "arctic_accumulate_ambient_occlusion_motion_device": 6, "arctic_accumulate_ambient_occlusion_motion": 6, "arctic_accumulate_pixels_motion": 19,
                "arctic_pass_ray_effects_motion": 8}
MODULE_LEVEL = ("motion_pixels", "accumulate_pixels_motion")
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
    # the definition stands in the header, in front of the calls
    for phrase in ("X_k[j] = ((T[j]*x + T[4+j]*y) + T[8+j]*z) + T[12+j]*1", "pw[j] = (B0*X_0[j] + B1*X_1[j]) + B2*X_2[j]", "c[i] = ((P[i]*pw0 + P[4+i]*pw1) + P[8+i]*pw2) + P[12+i]",
                   "velocity2 = {sx - (px + 0.5), sy - (py + 0.5)}, flag = 2", "HAS A PREVIOUS iff M is not empty", "to where the point WAS",
                   "pw equals the G-buffer's world (attributes 11..13) bit for bit", "after arctic_motion_reset and after arctic_resize", "leaves M as it was",
                   "|dot(m_p, w_q - pw_p)| <= plane_dist", "unless flag_p >= 1", "a surface that ROTATES between frames", "ONCE per frame"):
        assert phrase in text, phrase
    assert text.index("pw[j] = (B0*X_0[j]") < text.index("int arctic_motion_vectors_device(") < text.index("int arctic_accumulate_ambient_occlusion_motion_device(")
    assert text.index("int arctic_pass_ray_effects_temporal(") < text.index("int arctic_motion_vectors_device(") < text.index("int arctic_pass_ray_effects_motion(")
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "arctic_motion_vectors_device" in open(os.path.join(ROOT, name)).read(), name
    assert "k_motion" in open(os.path.join(ROOT, "profiles", "README.md")).read()
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^motion\.o: motion\.hip.*motion\.h.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M) and "asm-motion:" in make
    assert re.search(r"^motion_host\.o: motion\.cpp.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M)
    objs = make.split("OBJS")[1].split("\n")[0]
    assert " motion.o " in objs and " motion_host.o" in objs
    # one copy of the arithmetic: the kernels and the arbiters call motion.h's functions, which stand on the accumulation's and the hit attributes'
    head = open(os.path.join(CSRC, "motion.h")).read()
    for name in ("ha_mat_vec(", "aoh_reproject(", "ao_accepts(", "ao_normal(", "aoh_byte("):
        assert name in head, name
    for unit in ("motion.hip", "motion.cpp"):
        source = open(os.path.join(CSRC, unit)).read()
        assert "mo_pixel(" in source and "aoh_pixel_motion(" in source, unit
    assert "source_barycentrics(" in open(os.path.join(CSRC, "motion.hip")).read()


def test_refusals_of_the_arbiters_and_of_a_null_handle(pkg, lib):
    L = lib.lib()
    f, u, i = np.zeros(16, np.float32), np.zeros(4, np.uint32), np.zeros(2, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)
    P = np.eye(4, dtype=np.float32)
    assert L.arctic_motion_pixels(0, None, None, None, None, None, 0, None, 1, 1, None, None) == 0
    assert L.arctic_motion_pixels(1, p(f), p(u), p(f), p(i), p(f), 1, p(P), 0, 1, p(f), None) == INVALID
    assert L.arctic_motion_pixels(1, p(f), p(u), p(f), p(i), p(f), 1, p(P), 1, 16385, p(f), None) == INVALID
    for missing in range(4):
        args = [p(f), p(u), p(f), p(i)]
        args[missing] = None
        assert L.arctic_motion_pixels(1, *args, p(f), 1, p(P), 4, 4, p(f), None) == INVALID
    assert L.arctic_motion_pixels(1, p(f), p(u), p(f), p(i), p(f), 1, p(P), 4, 4, None, p(f)) == INVALID
    assert L.arctic_motion_pixels(1, p(f), p(u), p(f), p(i), None, 1, p(P), 4, 4, p(f), None) == INVALID
    assert L.arctic_motion_pixels(1, p(f), p(u), p(f), p(i), None, 1, None, 4, 4, p(f), None) == 0          # M empty: the table is not looked at
    with pytest.raises(pkg.renderer.ArcticError):
        pkg.renderer.motion_pixels(np.zeros((2, 3)), np.zeros(1), np.zeros((2, 3, 3)), np.zeros((2, 2)), np.zeros((1, 16)))
    with pytest.raises(pkg.renderer.ArcticError):
        pkg.renderer.accumulate_pixels_motion(np.zeros((2, 3)), np.zeros((1, 4)), np.zeros((2, 3)), np.ones(2), np.zeros(2))
    for bad in (dict(max_history=0.5), dict(plane_dist=-1.0), dict(min_weight=1.0), dict(normal_cos=np.nan)):
        with pytest.raises(pkg.renderer.ArcticError):
            pkg.renderer.accumulate_pixels_motion(np.zeros((1, 3)), np.zeros((1, 4)), np.zeros((1, 3)), [1], [0], **bad)
    with pytest.raises(pkg.renderer.ArcticError):                                                           # a previous matrix without a previous history
        pkg.renderer.accumulate_pixels_motion(np.zeros((1, 3)), np.zeros((1, 4)), np.zeros((1, 3)), [1], [0], P, 4, 4, prev=(np.zeros(3),) * 4)
    b = np.zeros(4, np.uint8)
    assert L.arctic_accumulate_pixels_motion(None, 1, p(f), p(f), p(f), p(b), p(b), None, 4, 4, None, None, None, None, p(b), None, None, None, None) == INVALID
    h = pkg.renderer._ao_history_arguments(8.0, 0.9, 0.05, 0.1)
    assert L.arctic_accumulate_pixels_motion(p(h), 1, p(f), None, p(f), p(b), p(b), None, 4, 4, None, None, None, None, p(b), None, None, None, None) == INVALID
    assert L.arctic_accumulate_pixels_motion(p(h), 1, p(f), p(f), p(f), p(b), p(b), None, 4, 4, None, None, None, None, p(b), None, None, None, None) == 0
    # a null handle, before any device is touched
    for name, arity in ENTRY_POINTS.items():
        if name not in ("arctic_motion_pixels", "arctic_accumulate_pixels_motion"):
            assert getattr(L, name)(*([None] * arity)) == INVALID, name


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_the_kernels_use_no_scratch_no_lds_no_stack(tmp_path):
    """k_motion, k_motion_snapshot, k_ao_accumulate_motion: no scratch, no LDS, no stack frame and no call, 8 waves per SIMD.  The compiler's
    figures when this was written: k_motion 58 VGPRs and 38 SGPRs, k_motion_snapshot 8 and 12, k_ao_accumulate_motion 44 and 58 (k_ao_accumulate:
    44 VGPRs) -- the bound below is what 8 waves per SIMD need, the figures DESIGN.md 6r quotes are checked against the compiler's"""
    log = subprocess.run(["make", "-C", CSRC, "asm-motion", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    names = re.findall(r"Function Name: (\S+)", remarks)
    grab = lambda what: [int(x) for x in re.findall(what + r": (\d+)", remarks)]
    r = dict(vgprs=grab(r" VGPRs"), sgprs=grab(r"TotalSGPRs"), scratch=grab(r"ScratchSize \[bytes/lane\]"), lds=grab(r"LDS Size \[bytes/block\]"), waves=grab(r"Occupancy \[waves/SIMD\]"))
    assert len(names) == 3 and [k for n in names for k in ("8k_motionE", "k_motion_snapshot", "k_ao_accumulate_motion") if k in n] == ["8k_motionE", "k_motion_snapshot", "k_ao_accumulate_motion"], names
    assert r["scratch"] == [0, 0, 0] and r["lds"] == [0, 0, 0] and r["waves"] == [8, 8, 8] and max(r["vgprs"]) <= 64, r
    assert "Dynamic Stack: True" not in remarks
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for k, kernel in enumerate(("k_motion", "k_motion_snapshot", "k_ao_accumulate_motion")):
        assert f"{kernel}: {r['vgprs'][k]} VGPRs, {r['sgprs'][k]} SGPRs, scratch 0, 8 waves per SIMD" in design, (kernel, r)
    frame = []
    for line in open(str(tmp_path / "motion-hip-amdgcn-amd-amdhsa-gfx950.s")):
        m = re.match(r"\s+\.amdhsa_(private_segment_fixed_size|uses_dynamic_stack) (\d+)", line)
        if m:
            frame.append(int(m.group(2)))
        assert "swappc" not in line
    assert frame == [0] * 6, frame


def test_arbiters_under_sanitizers():
    """tests/cpp/motion_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    driver = os.path.join(ROOT, "tests", "cpp", "motion_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "motion_sanitize.cpp"), os.path.join(CSRC, "motion.cpp"), os.path.join(CSRC, "ao_history.cpp")]
    deps = src + [os.path.join(CSRC, h) for h in ("ray_query.h", "ray_ao.h", "ao_history.h", "hit_attributes.h", "motion.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 10 and all(l.startswith("ok") for l in lines), lines
    for name in ("motion-ordinary", "motion-empty", "motion-nan", "motion-inf", "motion-1e30", "accumulate-ordinary", "accumulate-nan", "accumulate-inf", "accumulate-1e30", "refusals"):
        assert any(l.startswith("ok " + name) for l in lines), name
