"""The refit of the ray structure on a machine without a GPU: the entry points (header, binding, C++ mirror), ARCTIC_OPT_RAY_REFIT, the published
records' layout through a C compiler, arctic_refit_triangles' refusals, the kernels' resource figures (make asm-refit), and bvh_refit, the
schedule and its validation under the address and undefined-behaviour sanitizers in a program of their own (tests/cpp/bvh_refit_sanitize.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ray_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"arctic_ray_refit_info": 2, "arctic_ray_scene_reset": 1, "arctic_read_ray_structure": 5, "arctic_refit_triangles": 12}
INVALID, CAPACITY = -1, -5


@pytest.fixture(scope="module")
def lib(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def test_entry_points_option_and_binding(pkg, lib):
    text = open(os.path.join(ROOT, "include", "arctic_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = lib.lib()
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m and len(m.group(1).split(",")) == arity, name
        assert name in lib.header_symbols() and hasattr(L, name)
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == arity
    assert re.search(r"#define\s+ARCTIC_OPT_RAY_REFIT\s+7\b", header) and lib.OPTIONS["ray_refit"] == 7
    ids = [int(v) for v in re.findall(r"#define\s+ARCTIC_OPT_\w+\s+(\d+)", header)]
    assert ids.count(7) == 1 and list(lib.OPTIONS.values()).count(7) == 1
    assert L.arctic_version() == 340 and max(lib.OPTIONS.values()) == 27                 # recognised by its entry points, like the features before it
    hpp = open(os.path.join(ROOT, "arctic-renderer_amd", "host", "renderer.hpp")).read()
    for method, arity in (("ray_refit_info", 1), ("ray_scene_reset", 0), ("read_ray_structure", 4), ("refit_triangles", 12)):
        m = re.search(r"\[\[nodiscard\]\]\s+(static\s+)?bool\s+" + method + r"\s*\(([^)]*)\)", hpp)
        assert m and len([a for a in m.group(2).split(",") if a.strip()]) == arity, method
    for method in ("ray_refit_info", "ray_scene_reset", "read_ray_structure"):
        assert hasattr(pkg.renderer.Renderer, method)
    assert hasattr(pkg.renderer, "refit_triangles")
    # the definition stands in the header, next to the ray-query text
    for phrase in ("A REFITTED STRUCTURE", "nine quiet NaNs", "0x7FC00000", "bmin = +inf, bmax = -inf", "the empty box is the identity",
                   "Compare boxes by value, triangles by bytes", "does not count as a build"):
        assert phrase in text, phrase
    assert text.index("THE DEFINITION.") < text.index("A REFITTED STRUCTURE") < text.index("int arctic_owner_grid")
    # the kernels live in a translation unit of their own, built with contraction off; the world-vertex transform exists once
    mk = open(os.path.join(ROOT, "arctic-renderer_amd", "csrc", "Makefile")).read()
    assert re.search(r"ray_refit\.o: ray_refit\.hip.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\)", mk) and "asm-refit" in mk
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    assert "rq_world_vertex" in open(os.path.join(csrc, "ray_refit.hip")).read() and "rq_world_vertex" in open(os.path.join(csrc, "bvh.cpp")).read()
    assert "k_ray_refit" not in open(os.path.join(csrc, "trace.hip")).read()


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no C compiler")
def test_published_records_through_a_c_compiler(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "arctic_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu ", sizeof(ArcticRayNode), offsetof(ArcticRayNode, bmin), offsetof(ArcticRayNode, skip), offsetof(ArcticRayNode, bmax),\n'
                   "         offsetof(ArcticRayNode, leaf));\n"
                   '  printf("%zu %zu %zu %zu %zu %zu %d", sizeof(ArcticRayTri), offsetof(ArcticRayTri, p0), offsetof(ArcticRayTri, p1), offsetof(ArcticRayTri, p2),\n'
                   "         offsetof(ArcticRayTri, prim), offsetof(ArcticRayTri, pad), ARCTIC_OPT_RAY_REFIT);\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([shutil.which("cc") or shutil.which("gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [32, 0, 12, 16, 28, 48, 0, 12, 24, 36, 40, 7]
    node, tri = pkg.scene.RAY_NODE_DTYPE, pkg.scene.RAY_TRI_DTYPE
    assert [node.itemsize] + [node.fields[n][1] for n in ("bmin", "skip", "bmax", "leaf")] == got[:5]
    assert [tri.itemsize] + [tri.fields[n][1] for n in ("p0", "p1", "p2", "prim", "pad")] == got[5:11]
    # ... and they are the internal records: the library's own static_asserts say so
    bvh = open(os.path.join(ROOT, "arctic-renderer_amd", "csrc", "bvh.cpp")).read()
    assert "sizeof(ArcticRayNode) == sizeof(RayNode) && sizeof(ArcticRayTri) == sizeof(RayTri)" in bvh and "offsetof(ArcticRayTri, prim) == offsetof(RayTri, prim)" in bvh


def test_refit_triangles_refusals_write_nothing(pkg, lib):
    L = lib.lib()
    tris, rays = R.soup(np.random.default_rng(5), 5, 64)
    hits = np.zeros(len(rays), R.HIT_DTYPE)
    nodes, slots, counts = np.zeros(8, pkg.scene.RAY_NODE_DTYPE), np.zeros(8, pkg.scene.RAY_TRI_DTYPE), np.zeros(2, np.uint64)
    p = lambda a: a.ctypes.data

    def poison():
        hits["t"], nodes["skip"], slots["prim"], counts[:] = 77, 77, 77, 77

    def call(a=p(tris), b=p(tris), nt=5, r=p(rays), n=64, flags=0, h=p(hits), nd=p(nodes), nc=8, sl=p(slots), sc=8, cn=p(counts)):
        return L.arctic_refit_triangles(a, b, nt, r, n, flags, h, nd, nc, sl, sc, cn)

    poison()
    assert call() == 0 and tuple(counts) == (3, 5) and (hits["t"] != 77).any() and (nodes["skip"][:3] != 77).all()
    assert hits.tobytes() == R.brute(tris, rays).tobytes()
    poison()
    for kw in (dict(a=None), dict(b=None), dict(r=None), dict(h=None), dict(flags=4), dict(flags=0x80000001)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(nt=0xFFFFFFFF), dict(nc=2), dict(sc=4)):
        assert call(**kw) == CAPACITY, kw                                               # (the first is refused before anything is read)
    assert (hits["t"] == 77).all() and (nodes["skip"] == 77).all() and (slots["prim"] == 77).all() and (counts == 77).all()
    assert call(nd=None, nc=0, sl=None, sc=0, cn=None) == 0                              # the structure is optional
    assert L.arctic_refit_triangles(None, None, 0, None, 0, 0, None, None, 0, None, 0, None) == 0
    # the handle's calls refuse a null handle without touching it
    out = np.zeros(4, np.uint64)
    assert L.arctic_ray_refit_info(None, p(out)) == INVALID and L.arctic_ray_scene_reset(None) == INVALID
    assert L.arctic_read_ray_structure(None, None, 0, None, 0) == INVALID and L.arctic_set_option(None, 7, 1) == INVALID


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_refit_kernels_use_no_scratch(tmp_path):
    """k_ray_refit_leaves and k_ray_refit_upper: no scratch, 3 KiB of LDS for the task's boxes, vector stores only, no atomic"""
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    log = subprocess.run(["make", "-C", csrc, "asm-refit", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    names = re.findall(r"Function Name: (\S+)", remarks)
    assert len(names) == 2 and sum("k_ray_refit_leaves" in n for n in names) == 1 and sum("k_ray_refit_upper" in n for n in names) == 1, names
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)] == [0, 0]
    assert [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)] == [127 * 24, 127 * 24]
    assert all(int(x) >= 4 for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", remarks))
    name, scratch, stores, other = None, {}, {}, set()
    for line in open(str(tmp_path / "ray_refit-hip-amdgcn-amd-amdhsa-gfx950.s")):
        m = re.match(r"(_Z\w+):", line)
        if m:
            name = m.group(1)
        op = line.split()[0] if line.strip() else ""
        if name and "store" in op:
            stores.setdefault(name, set()).add(op)
        if name and ("atomic" in op or op.startswith("buffer_") or op.startswith("scratch_") or op.startswith("flat_")):
            other.add(op)
        if name and line.startswith("; ScratchSize:"):
            scratch[name] = int(line.split(":")[1].split()[0])
    assert len(scratch) == 2 and all(v == 0 for v in scratch.values()), scratch
    assert not other, other
    for k, ops in stores.items():
        assert ops and all(o.startswith("global_store_dword") for o in ops), (k, ops)    # vector stores to memory only
        assert "global_store_dwordx3" in ops                                            # a box is two 12-byte stores: skip and leaf are never written
        assert ("global_store_dwordx4" in ops) == ("leaves" in k)                        # the slots' 16-byte pieces


def test_host_refit_under_sanitizers():
    """tests/cpp/bvh_refit_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    driver = os.path.join(ROOT, "tests", "cpp", "bvh_refit_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "bvh_refit_sanitize.cpp"), os.path.join(ROOT, "arctic-renderer_amd", "csrc", "bvh.cpp")]
    deps = src + [os.path.join(ROOT, "arctic-renderer_amd", "csrc", "ray_query.h"), os.path.join(ROOT, "include", "arctic_hip.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) >= 13 and all(l.startswith("ok") for l in lines)
    for name in ("empty", "one", "all-dead", "to-1e30", "moved-20000-three-stages", "shorter-b-refused", "schedule-validation", "refusals"):
        assert any(l.startswith("ok " + name) for l in lines), name
    assert any(l.startswith("ok moved-20000-three-stages") and " 3 stages" in l for l in lines)
