"""The re-split of the ray structure on a machine without a GPU: the entry points (header, binding, C++ mirror), the definition's place in the
header, arctic_resplit_triangles' refusals, the resource figures of ray_resplit.hip's own kernels (make asm-resplit), and bvh_resplit with the
segment arithmetic and the key mapping under the address and undefined-behaviour sanitizers in a program of their own
(tests/cpp/resplit_sanitize.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ray_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"arctic_ray_scene_resplit": 2, "arctic_ray_resplit_info": 2, "arctic_resplit_triangles": 12}
INVALID, CAPACITY = -1, -5


@pytest.fixture(scope="module")
def lib(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def test_entry_points_binding_and_definition(pkg, lib):
    text = open(os.path.join(ROOT, "include", "arctic_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = lib.lib()
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m and len(m.group(1).split(",")) == arity, name
        assert name in lib.header_symbols() and hasattr(L, name)
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == arity
    assert lib.SIGNATURES["arctic_resplit_triangles"] == lib.SIGNATURES["arctic_refit_triangles"]     # shaped like the refit's arbiter
    # the version the earlier ABI tests pin: the feature is recognised by its entry points, like the features before it, and adds no option
    assert L.arctic_version() == 340 and max(lib.OPTIONS.values()) == 27
    hpp = open(os.path.join(ROOT, "arctic-renderer_amd", "host", "renderer.hpp")).read()
    for method, arity in (("ray_scene_resplit", 1), ("ray_resplit_info", 1), ("resplit_triangles", 12)):
        m = re.search(r"\[\[nodiscard\]\]\s+(static\s+)?bool\s+" + method + r"\s*\(([^)]*)\)", hpp)
        assert m and len([a for a in m.group(2).split(",") if a.strip()]) == arity, method
    for method in ("ray_scene_resplit", "ray_resplit_info"):
        assert hasattr(pkg.renderer.Renderer, method)
    assert hasattr(pkg.renderer, "resplit_triangles")
    # the definition stands in the header, behind the refit's
    for phrase in ("A RE-SPLIT STRUCTURE", "0.5f*lo + 0.5f*hi", "strict >", "the lowest axis wins", "-0 and +0 tie and fall to the prim",
                   "a dead triangle orders behind every live one", "a segment with no live member takes axis 0", "overflows to +inf still orders",
                   "triangles, skip and leaf compare by bytes, boxes compare by value", "counts neither as a build"):
        assert phrase in text, phrase
    assert text.index("A REFITTED STRUCTURE") < text.index("A RE-SPLIT STRUCTURE") < text.index("int arctic_owner_grid")
    # a translation unit of its own, built with contraction off; no existing kernel file knows of it
    mk = open(os.path.join(ROOT, "arctic-renderer_amd", "csrc", "Makefile")).read()
    assert re.search(r"ray_resplit\.o: ray_resplit\.hip.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\)", mk) and "ray_resplit.o" in mk.split("OBJS")[1].split("\n")[0]
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    for other in ("trace.hip", "ray_refit.hip", "shade.hip", "geometry.hip"):
        assert "resplit" not in open(os.path.join(csrc, other)).read(), other
    src = open(os.path.join(csrc, "ray_resplit.hip")).read()
    assert "rq_world_vertex" in src and "rocprim::radix_sort_pairs" in src and "hipStreamSynchronize" not in src and "hipMemcpy" not in src
    assert "bvh_build" not in open(os.path.join(csrc, "bvh.cpp")).read().split("bool bvh_resplit(")[1].split("\n}\n")[0]   # carried out directly


def test_resplit_triangles_refusals_write_nothing(pkg, lib):
    L = lib.lib()
    tris, rays = R.soup(np.random.default_rng(5), 5, 64)
    hits = np.zeros(len(rays), R.HIT_DTYPE)
    nodes, slots, counts = np.zeros(8, pkg.scene.RAY_NODE_DTYPE), np.zeros(8, pkg.scene.RAY_TRI_DTYPE), np.zeros(2, np.uint64)
    p = lambda a: a.ctypes.data

    def poison():
        hits["t"], nodes["skip"], slots["prim"], counts[:] = 77, 77, 77, 77

    def call(a=p(tris), b=p(tris), nt=5, r=p(rays), n=64, flags=0, h=p(hits), nd=p(nodes), nc=8, sl=p(slots), sc=8, cn=p(counts)):
        return L.arctic_resplit_triangles(a, b, nt, r, n, flags, h, nd, nc, sl, sc, cn)

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
    assert L.arctic_resplit_triangles(None, None, 0, None, 0, 0, None, None, 0, None, 0, None) == 0
    # the handle's calls refuse a null handle without touching it
    out = np.zeros(4, np.uint64)
    assert L.arctic_ray_resplit_info(None, p(out)) == INVALID and L.arctic_ray_scene_resplit(None, None) == INVALID and not out.any()


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_resplit_kernels_use_no_scratch(tmp_path):
    """the five kernels of ray_resplit.hip: no scratch, no LDS, vector stores only, and no atomic but the 32-bit vector min / max of the extents.
    (The radix sort's kernels are rocprim's, compiled into the same unit; they are not judged here.)"""
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    log = subprocess.run(["make", "-C", csrc, "asm-resplit", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    own = {}
    for block in remarks.split("Function Name: ")[1:]:
        name = block.split()[0]
        if "k_resplit_" in name and name not in own:
            own[name] = {k: int(re.search(re.escape(k) + r": (\d+)", block).group(1)) for k in ("ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")}
    kernels = ("k_resplit_prims", "k_resplit_centroids", "k_resplit_assign", "k_resplit_keys", "k_resplit_apply")
    assert len(own) == 5 and all(sum(k in n for n in own) == 1 for k in kernels), list(own)
    for name, f in own.items():
        assert f["ScratchSize [bytes/lane]"] == 0 and f["LDS Size [bytes/block]"] == 0 and f["Occupancy [waves/SIMD]"] >= 4, (name, f)
    name, ops = None, {}
    for line in open(str(tmp_path / "ray_resplit-hip-amdgcn-amd-amdhsa-gfx950.s")):
        m = re.match(r"(_Z\w+):", line)
        if m:
            name = m.group(1)
        op = line.split()[0] if line.strip() else ""
        if name and "k_resplit_" in name and ("store" in op or "atomic" in op or op.startswith(("buffer_", "scratch_", "flat_"))):
            ops.setdefault(name, set()).add(op)
    assert len(ops) == 5
    for k, o in ops.items():
        stores = {x for x in o if "store" in x}
        assert stores and all(x.startswith("global_store_dword") for x in stores), (k, o)   # vector stores to memory only
        rest = o - stores
        assert rest == ({"global_atomic_umin", "global_atomic_umax"} if "k_resplit_assign" in k else set()), (k, o)


def test_host_resplit_under_sanitizers():
    """tests/cpp/resplit_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    driver = os.path.join(ROOT, "tests", "cpp", "resplit_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "resplit_sanitize.cpp"), os.path.join(ROOT, "arctic-renderer_amd", "csrc", "bvh.cpp")]
    deps = src + [os.path.join(ROOT, "arctic-renderer_amd", "csrc", "ray_query.h"), os.path.join(ROOT, "include", "arctic_hip.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert all(l.startswith("ok") for l in lines)
    for n in (1, 4, 5, 8, 9, 255, 256, 257, 4097, 16385):
        for kind in ("moved", "ties", "some-dead", "all-dead"):
            assert any(l.startswith(f"ok {kind}-{n}:") for l in lines), (kind, n)
    for name in ("empty", "to-3e38", "keys", "refusals"):
        assert any(l.startswith("ok " + name) for l in lines), name
    assert any(l.startswith("ok moved-16385:") and " 13 levels" in l for l in lines)
