"""The composition on a machine without a GPU: the entry points (header, binding, C++ mirror), ArcticRayCompose's layout through a C compiler, the
definition in the header in front of the calls, k_compose's resource figures (and those of the hit kernels, which share its sampler through
material_sampler.h and have to keep theirs), and the arbiter under the address and undefined-behaviour sanitizers in a program of its own
(tests/cpp/compose_sanitize.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
ENTRY_POINTS = {"arctic_compose_planes_device": 7, "arctic_pass_ray_effects": 7, "arctic_read_composed": 4, "arctic_compose_pixels": 14, "arctic_compose_info": 2}
FIELDS = ("flags", "ao_strength", "reflection_strength", "reflection_bias", "reserved")
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
    for method in ("compose_planes_device", "pass_ray_effects", "read_composed", "compose_pixels", "compose_info"):
        assert re.search(r"\[\[nodiscard\]\]\s+(static\s+)?bool\s+" + method + r"\s*\(", hpp), method
    for method in ("compose_planes_device", "pass_ray_effects", "read_composed", "compose_info"):
        assert hasattr(pkg.renderer.Renderer, method)
    assert hasattr(pkg.renderer, "compose_pixels") and (lib.COMPOSE_AO, lib.COMPOSE_REFLECTIONS) == (1, 2)
    assert re.search(r"#define ARCTIC_COMPOSE_AO\s+1u", text) and re.search(r"#define ARCTIC_COMPOSE_REFLECTIONS\s+2u", text)
    # the definition stands in the header, in front of the calls, and says what is refused instead of approximated
    for phrase in ("vis = ao / 255", "ka = 1 - ao_strength * (1 - vis)", "C = hdr + (ambient * base) * (ka - 1)", "F0 = 0.04 + (base - 0.04) * metal",
                   "F = F0 + (1 - F0) * (1 - c)^5", "g  = (1 - rough)^2", "C += reflection_strength * refl.a * g * F * refl.rgb", "a SELECT, not a product by zero",
                   "NOT COVERED", "INTERPOLATED VERTEX NORMAL", "ARCTIC_OPT_KEEP_FLOAT_OUTPUT off", "ARCTIC_OPT_HDR16 = 1", "refused, not approximated",
                   "ARCTIC_OPT_ANTIALIAS is not applied"):
        assert phrase in text, phrase
    assert text.index("vis = ao / 255") < text.index("int arctic_compose_planes_device(") < text.index("int arctic_pass_ray_effects(") < text.index("int arctic_read_composed(")
    # nobody says any more that the planes have no consumer
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("include", "arctic_hip.h")):
        t = open(os.path.join(ROOT, name)).read()
        assert "multiplies it into its indirect term" not in t, name
        assert "arctic_pass_ray_effects" in t, name
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^compose\.o:.*material_sampler\.h.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M) and "asm-compose:" in make
    assert re.search(r"^compose_host\.o: compose\.cpp.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M)
    assert re.search(r"^hit_shade\.o:.*material_sampler\.h", make, flags=re.M)


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no C compiler")
def test_struct_size_and_offsets(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "arctic_hip.h"\nint main(void) {\n  printf("%zu", sizeof(ArcticRayCompose));\n'
                   + "".join(f'  printf(" %zu", offsetof(ArcticRayCompose, {f}));\n' for f in FIELDS)
                   + '  printf(" %zu %u %u", sizeof(((ArcticRayCompose *)0)->reserved), ARCTIC_COMPOSE_AO, ARCTIC_COMPOSE_REFLECTIONS);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([shutil.which("cc") or shutil.which("gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [32, 0, 4, 8, 12, 16, 16, 1, 2]
    c = pkg.scene.COMPOSE_DTYPE
    assert [c.itemsize] + [c.fields[n][1] for n in FIELDS] == got[:6] and c.names == FIELDS
    assert [c.fields[n][0].base.kind for n in FIELDS] == ["u", "f", "f", "f", "u"] and c.fields["reserved"][0].shape == (4,)
    assert re.search(r"typedef struct ArcticRayCompose \{\s*/\* 32 bytes \*/", open(os.path.join(ROOT, "include", "arctic_hip.h")).read())


def _resources(target, tmp_path):
    log = subprocess.run(["make", "-C", CSRC, target, f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    names = re.findall(r"Function Name: (\S+)", remarks)
    grab = lambda what: [int(x) for x in re.findall(what + r": (\d+)", remarks)]
    return names, dict(vgprs=grab(r" VGPRs"), scratch=grab(r"ScratchSize \[bytes/lane\]"), lds=grab(r"LDS Size \[bytes/block\]"), waves=grab(r"Occupancy \[waves/SIMD\]"))


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_k_compose_uses_no_scratch_no_lds_no_stack(tmp_path):
    """k_compose: no scratch, no LDS, no stack frame and no call, the 8 waves per SIMD of a streaming kernel, and vector stores only -- the RGBA8 word
    and the two float planes, 12 bytes at a time"""
    names, r = _resources("asm-compose", tmp_path)
    assert len(names) == 1 and "k_compose" in names[0], names
    assert r["scratch"] == [0] and r["lds"] == [0] and r["waves"] == [8] and r["vgprs"][0] <= 64, r
    name, ops, frame = None, {}, {}
    for line in open(str(tmp_path / "compose-hip-amdgcn-amd-amdhsa-gfx950.s")):
        m = re.match(r"(_Z\w+):", line)
        if m:
            name = m.group(1)
        op = line.split()[0] if line.strip() else ""
        if name and ("store" in op or "swappc" in op):
            ops.setdefault(name, set()).add(op)
        m = re.match(r"\s+\.amdhsa_(private_segment_fixed_size|uses_dynamic_stack) (\d+)", line)
        if m:
            frame[m.group(1)] = int(m.group(2))
    assert list(ops.values()) == [{"global_store_dword", "global_store_dwordx3"}], ops
    assert frame == {"private_segment_fixed_size": 0, "uses_dynamic_stack": 0}, frame


@pytest.mark.skipif(not HAVE_HIPCC, reason="no hipcc")
def test_the_hit_kernels_keep_their_registers(tmp_path):
    """the sampler moved from hit_shade.hip into material_sampler.h unchanged: k_hit_attributes, k_shade_hits and k_reflect_rays compile to the
    register counts they had (93 / 112 / 30 VGPRs, no scratch: DESIGN.md 6o and 6p)"""
    names, r = _resources("asm-hit", tmp_path)
    got = {k: r["vgprs"][i] for i, n in enumerate(names) for k in ("k_hit_attributes", "k_shade_hits", "k_reflect_rays") if k in n}
    assert got == {"k_hit_attributes": 93, "k_shade_hits": 112, "k_reflect_rays": 30} and r["scratch"] == [0, 0, 0], (got, r)
    hit = open(os.path.join(CSRC, "hit_shade.hip")).read()
    assert '#include "material_sampler.h"' in hit and "sample_material(" in hit and "Channels sample_material" not in hit
    assert "Channels sample_material" in open(os.path.join(CSRC, "material_sampler.h")).read()
    assert "sample_material(" in open(os.path.join(CSRC, "compose.hip")).read()


def test_arbiter_under_sanitizers():
    """tests/cpp/compose_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    driver = os.path.join(ROOT, "tests", "cpp", "compose_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "compose_sanitize.cpp"), os.path.join(CSRC, "compose.cpp")]
    deps = src + [os.path.join(CSRC, h) for h in ("ray_query.h", "ray_ao.h", "compose.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 16 and all(l.startswith("ok") for l in lines), lines
    for name in ("no-pixel-flags-1", "one-pixel-flags-2", "many-20000-flags-3", "huge-1e30-flags-3", "tiny-1e-40-flags-1", "refusals"):
        assert any(l.startswith("ok " + name) for l in lines), name
