"""The temporal accumulation on a machine without a GPU: the entry points (header, binding, C++ mirror), ArcticAoHistory's layout through a C
compiler, the definition in the header in front of the calls, k_ao_accumulate's resource figures, and the arbiter under the address and
undefined-behaviour sanitizers in a program of its own (tests/cpp/ao_history_sanitize.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
ENTRY_POINTS = {"arctic_accumulate_ambient_occlusion_device": 5, "arctic_accumulate_ambient_occlusion": 5, "arctic_ao_history_reset": 1, "arctic_read_ao_history": 5,
                "arctic_ao_history_info": 2, "arctic_accumulate_pixels": 18, "arctic_pass_ray_effects_temporal": 8}
FIELDS = ("max_history", "normal_cos", "plane_dist", "min_weight", "reserved")
HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


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
    methods = [n[len("arctic_"):] for n in ENTRY_POINTS]
    for method in methods:
        assert re.search(r"\[\[nodiscard\]\]\s+(static\s+)?bool\s+" + method + r"\s*\(", hpp), method
    for method in methods:
        assert hasattr(pkg.renderer, method) if method == "accumulate_pixels" else hasattr(pkg.renderer.Renderer, method), method
    # the definition stands in the header, in front of the calls
    for phrase in ("c[i] = ((P[i]*w0 + P[4+i]*w1) + P[8+i]*w2) + P[12+i]", "c3 > 0 and c0, c1, c3 are finite", "sx = (nx + 1) * (0.5*W);  sy = (1 - ny) * (0.5*H)",
                   "-1 <= ix <= W-1 and -1 <= iy <= H-1", "(1-ax)*(1-ay), ax*(1-ay), (1-ax)*ay, ax*ay", "S = ((k0 + k1) + k2) + k3", "!(S > min_weight)",
                   "N = min(hn + 1, max_history);  a = 1 / N;  value = hv + (cur - hv) * a", "a SELECT, not a product by zero", "PREVIOUS call's matrix",
                   "no per-object motion vectors", "531 MB at 3840 x 2160", "leaves H as it was"):
        assert phrase in text, phrase
    assert text.index("S = ((k0 + k1) + k2) + k3") < text.index("int arctic_accumulate_ambient_occlusion_device(") < text.index("int arctic_pass_ray_effects_temporal(")
    assert text.index("int arctic_pass_ray_effects(") < text.index("int arctic_accumulate_ambient_occlusion_device(")
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "arctic_accumulate_ambient_occlusion_device" in open(os.path.join(ROOT, name)).read(), name
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^ao_history\.o: ao_history\.hip.*ao_history\.h.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M) and "asm-ao-history:" in make
    assert re.search(r"^ao_history_host\.o: ao_history\.cpp.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M)
    # one copy of the arithmetic: the kernel and the arbiter both call ao_history.h's function, which uses ray_ao.h's two
    head = open(os.path.join(CSRC, "ao_history.h")).read()
    assert "ao_normal(" in head and "ao_accepts(" in head
    for unit in ("ao_history.hip", "ao_history.cpp"):
        assert "aoh_pixel(" in open(os.path.join(CSRC, unit)).read(), unit


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no C compiler")
def test_struct_size_and_offsets(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "arctic_hip.h"\nint main(void) {\n  printf("%zu", sizeof(ArcticAoHistory));\n'
                   + "".join(f'  printf(" %zu", offsetof(ArcticAoHistory, {f}));\n' for f in FIELDS)
                   + '  printf(" %zu", sizeof(((ArcticAoHistory *)0)->reserved));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([shutil.which("cc") or shutil.which("gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [32, 0, 4, 8, 12, 16, 16]
    d = pkg.scene.AO_HISTORY_DTYPE
    assert [d.itemsize] + [d.fields[n][1] for n in FIELDS] == got[:6] and d.names == FIELDS
    assert [d.fields[n][0].base.kind for n in FIELDS] == ["f", "f", "f", "f", "u"] and d.fields["reserved"][0].shape == (4,)
    assert re.search(r"typedef struct ArcticAoHistory \{\s*/\* 32 bytes \*/", open(os.path.join(ROOT, "include", "arctic_hip.h")).read())


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_k_ao_accumulate_uses_no_scratch_no_lds_no_stack(tmp_path):
    """k_ao_accumulate: no scratch, no LDS, no stack frame and no call, the 8 waves per SIMD of a streaming kernel, and vector stores only -- the
    byte and the two history planes, 16 bytes at a time.  The figures DESIGN.md 6q quotes are the compiler's"""
    log = subprocess.run(["make", "-C", CSRC, "asm-ao-history", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    names = re.findall(r"Function Name: (\S+)", remarks)
    grab = lambda what: [int(x) for x in re.findall(what + r": (\d+)", remarks)]
    r = dict(vgprs=grab(r" VGPRs"), sgprs=grab(r"TotalSGPRs"), scratch=grab(r"ScratchSize \[bytes/lane\]"), lds=grab(r"LDS Size \[bytes/block\]"), waves=grab(r"Occupancy \[waves/SIMD\]"))
    assert len(names) == 1 and "k_ao_accumulate" in names[0], names
    assert r["scratch"] == [0] and r["lds"] == [0] and r["waves"] == [8] and r["vgprs"][0] <= 64, r
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"{r['vgprs'][0]} VGPRs, {r['sgprs'][0]} SGPRs, scratch 0, 8 waves per SIMD" in design, r
    name, ops, frame = None, {}, {}
    for line in open(str(tmp_path / "ao_history-hip-amdgcn-amd-amdhsa-gfx950.s")):
        m = re.match(r"(_Z\w+):", line)
        if m:
            name = m.group(1)
        op = line.split()[0] if line.strip() else ""
        if name and ("store" in op or "swappc" in op):
            ops.setdefault(name, set()).add(op)
        m = re.match(r"\s+\.amdhsa_(private_segment_fixed_size|uses_dynamic_stack) (\d+)", line)
        if m:
            frame[m.group(1)] = int(m.group(2))
    assert list(ops.values()) == [{"global_store_byte", "global_store_dwordx4"}], ops
    assert frame == {"private_segment_fixed_size": 0, "uses_dynamic_stack": 0}, frame


def test_arbiter_under_sanitizers():
    """tests/cpp/ao_history_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    driver = os.path.join(ROOT, "tests", "cpp", "ao_history_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "ao_history_sanitize.cpp"), os.path.join(CSRC, "ao_history.cpp")]
    deps = src + [os.path.join(CSRC, h) for h in ("ray_query.h", "ray_ao.h", "ao_history.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 7 and all(l.startswith("ok") for l in lines), lines
    for name in ("one-pixel", "small-7x5", "ragged-61x37", "huge-1e30", "tiny-1e-30", "one-call", "refusals"):
        assert any(l.startswith("ok " + name) for l in lines), name
