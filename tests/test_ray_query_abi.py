"""Ray queries on a machine without a GPU: the entry points (header, binding, C++ mirror), the records' layout through a C compiler,
arctic_trace_triangles -- the library's own builder, walk and intersection code on the host -- against the numpy arbiter bit for bit, its
refusals, the kernels' resource figures, and the builder and host walk under the address and undefined-behaviour sanitizers in a program of
their own (tests/cpp/bvh_sanitize.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ray_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"arctic_trace_rays": 6, "arctic_trace_rays_device": 6, "arctic_trace_sun_visibility": 4, "arctic_trace_triangles": 6, "arctic_ray_scene_info": 2}
INVALID, CAPACITY = -1, -5


@pytest.fixture(scope="module")
def lib(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def test_entry_points_and_binding(pkg, lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arctic_hip.h")).read(), flags=re.S)
    L = lib.lib()
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m and len(m.group(1).split(",")) == arity, name
        assert name in lib.header_symbols() and hasattr(L, name)
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == arity
    assert re.search(r"#define\s+ARCTIC_TRACE_ANY\s+1u", header) and re.search(r"#define\s+ARCTIC_TRACE_BRUTE\s+2u", header)
    assert (lib.TRACE_ANY, lib.TRACE_BRUTE) == (1, 2)
    hpp = open(os.path.join(ROOT, "arctic-renderer_amd", "host", "renderer.hpp")).read()
    for method in ("trace_rays", "trace_rays_device", "trace_sun_visibility", "trace_triangles", "ray_scene_info"):
        assert re.search(r"\[\[nodiscard\]\]\s+(static\s+)?bool\s+" + method + r"\s*\(", hpp), method       # the C++ mirror has the same calls
    for method in ("trace_rays", "trace_rays_device", "trace_sun_visibility", "ray_scene_info"):
        assert hasattr(pkg.renderer.Renderer, method)
    assert hasattr(pkg.renderer, "trace_triangles")
    assert L.arctic_version() == 340 and max(lib.OPTIONS.values()) == 27                 # the feature is recognised by its entry points
    # the definition stands in the header, next to the calls
    text = open(os.path.join(ROOT, "include", "arctic_hip.h")).read()
    for phrase in ("t = min(max(tm, tn), tf)", "MONOTONE in box inclusion", "NOT watertight", "two-sided", "The comparison is strict"):
        assert phrase in text, phrase


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no C compiler")
def test_struct_sizes_and_offsets(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "arctic_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu ", sizeof(ArcticRay), offsetof(ArcticRay, origin), offsetof(ArcticRay, t_min), offsetof(ArcticRay, direction),\n'
                   "         offsetof(ArcticRay, t_max));\n"
                   '  printf("%zu %zu %zu %zu %zu", sizeof(ArcticHit), offsetof(ArcticHit, t), offsetof(ArcticHit, u), offsetof(ArcticHit, v), offsetof(ArcticHit, prim));\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([shutil.which("cc") or shutil.which("gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [32, 0, 12, 16, 28, 16, 0, 4, 8, 12]
    ray, hit = pkg.scene.RAY_DTYPE, pkg.scene.HIT_DTYPE
    assert [ray.itemsize] + [ray.fields[n][1] for n in ("origin", "t_min", "direction", "t_max")] == got[:5]
    assert [hit.itemsize] + [hit.fields[n][1] for n in ("t", "u", "v", "prim")] == got[5:]
    assert ray == R.RAY_DTYPE and hit == R.HIT_DTYPE
    header = open(os.path.join(ROOT, "include", "arctic_hip.h")).read()
    assert re.search(r"\} ArcticRay;\s*/\* 32 bytes \*/", header) and re.search(r"\} ArcticHit;\s*/\* 16 bytes \*/", header)


_CASES = {}


def case(n_tris, n_rays):
    """one soup per size, the arbiter's answers computed once and shared by the four modes"""
    key = (n_tris, n_rays)
    if key not in _CASES:
        tris, rays = R.soup(np.random.default_rng(100000 + 1000 * n_tris + n_rays), n_tris, n_rays)
        _CASES[key] = (tris, rays, {a: R.brute(tris, rays, any_hit=a) for a in (False, True)})
    return _CASES[key]


@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("n_tris", [1, 4, 5, 64, 1000])
def test_host_trace_matches_the_arbiter_bit_for_bit(pkg, lib, n_tris, n_rays):
    tris, rays, want = case(n_tris, n_rays)
    for any_hit in (False, True):
        for brute in (False, True):
            got = pkg.renderer.trace_triangles(tris, rays, any_hit=any_hit, brute=brute)
            assert got.tobytes() == want[any_hit].tobytes(), (any_hit, brute)
    if n_rays >= 63:
        # not vacuous: at least a quarter of the rays hit ...
        hit, tie = R.tied(tris, rays)
        assert hit.sum() * 4 >= n_rays
        assert (want[False]["prim"][hit] < n_tris).all() and (want[False]["prim"][~hit] == R.NO_PRIM).all()
        if n_tris >= 64:
            # ... a closest t is shared by two triangles (that takes triangles that touch: the soup has them from a few dozen on), and the pruned
            # walk visits fewer nodes than the tree has (that takes a tree: 1, 4 and 5 triangles are one or three nodes)
            assert tie.sum() >= 1
            bvh = R.build_bvh(tris)
            w, visits = R.walk(bvh, rays)
            assert w.tobytes() == want[False].tobytes()
            assert visits.max() <= len(bvh.skip) and visits.mean() < len(bvh.skip)


def test_host_trace_edge_rays_and_unaligned_records(pkg, lib):
    tris, rays, _ = case(64, 65)
    rays = rays.copy()
    rays["direction"][0] = 0
    rays["direction"][1, 0] = np.nan
    rays["origin"][2, 2] = np.inf
    rays["t_max"][3] = np.nan
    rays["t_min"][4] = -np.inf
    rays["direction"][5] = (0, 0, 1e-45)
    big = np.concatenate([tris, np.full((3, 9), np.nan, np.float32), tris[:5] * np.float32(1e30)])
    for any_hit in (False, True):
        want = R.brute(big, rays, any_hit=any_hit)
        assert (want["prim"][:4] == R.NO_PRIM).all()
        for brute in (False, True):
            assert pkg.renderer.trace_triangles(big, rays, any_hit=any_hit, brute=brute).tobytes() == want.tobytes()
    # records at an address that is not 16-byte aligned
    raw = np.zeros(len(rays) * 32 + 4, np.uint8)
    raw[4:] = rays.view(np.uint8)
    out = np.zeros(len(rays) * 16 + 4, np.uint8)
    assert lib.lib().arctic_trace_triangles(big.ctypes.data, len(big), raw.ctypes.data + 4, len(rays), 0, out.ctypes.data + 4) == 0
    assert out[4:].tobytes() == R.brute(big, rays).tobytes()
    # no triangle at all: every ray misses
    none = pkg.renderer.trace_triangles(np.zeros((0, 9), np.float32), rays)
    assert (none["prim"] == R.NO_PRIM).all() and not none["t"].any()


def test_trace_triangles_refusals(pkg, lib):
    L = lib.lib()
    tris, rays, _ = case(5, 64)
    hits = np.zeros(len(rays), R.HIT_DTYPE)
    hits["t"] = 77
    call = lambda t, nt, r, n, flags, h: L.arctic_trace_triangles(t, nt, r, n, flags, h)
    p = lambda a: a.ctypes.data
    assert call(p(tris), 5, p(rays), 64, 0, p(hits)) == 0
    hits["t"] = 77
    for args in [(None, 5, p(rays), 64, 0, p(hits)), (p(tris), 5, None, 64, 0, p(hits)), (p(tris), 5, p(rays), 64, 0, None),
                 (p(tris), 5, p(rays), 64, 4, p(hits)), (p(tris), 5, p(rays), 64, 0x80000001, p(hits))]:
        assert call(*args) == INVALID
    assert call(p(tris), 0xFFFFFFFF, p(rays), 64, 0, p(hits)) == CAPACITY              # refused before anything is read
    assert (hits["t"] == 77).all()                                                      # nothing written by a refused call
    assert call(None, 0, None, 0, 0, None) == 0


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_trace_kernels_use_no_scratch_and_no_lds(tmp_path):
    """k_trace<closest>, k_trace<any> and k_trace_sun: no scratch (the walk has no stack, no runtime-indexed array), no LDS, and every store a
    vector store of the result's width"""
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    log = subprocess.run(["make", "-C", csrc, "asm-trace", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    names = re.findall(r"Function Name: (\S+)", remarks)
    assert len(names) == 3 and sum("k_trace_sun" in n for n in names) == 1 and sum("7k_traceILb" in n for n in names) == 2, names
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)] == [0, 0, 0]
    assert [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)] == [0, 0, 0]
    assert all(int(x) >= 4 for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", remarks))
    path = str(tmp_path / "trace-hip-amdgcn-amd-amdhsa-gfx950.s")
    name, scratch, stores, loads16 = None, {}, {}, {}
    for line in open(path):
        m = re.match(r"(_Z\w+):", line)
        if m:
            name = m.group(1)
        op = line.split()[0] if line.strip() else ""
        if name and "store" in op:
            stores.setdefault(name, set()).add(op)
        if name and op == "global_load_dwordx4":
            loads16[name] = loads16.get(name, 0) + 1
        if name and line.startswith("; ScratchSize:"):
            scratch[name] = int(line.split(":")[1].split()[0])
    assert len(scratch) == 3 and all(v == 0 for v in scratch.values()), scratch
    for k, ops in stores.items():
        assert ops == ({"global_store_byte"} if "k_trace_sun" in k else {"global_store_dwordx4"}), (k, ops)
    # a ray is two 16-byte loads, a node two, a triangle two and a half (the compiler narrows the third to the 8 bytes in use), in each of the two walks
    assert all(loads16.get(k, 0) >= 8 for k in scratch), loads16


def test_builder_and_host_walk_under_sanitizers():
    """tests/cpp/bvh_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    driver = os.path.join(ROOT, "tests", "cpp", "bvh_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "bvh_sanitize.cpp"), os.path.join(ROOT, "arctic-renderer_amd", "csrc", "bvh.cpp")]
    deps = src + [os.path.join(ROOT, "arctic-renderer_amd", "csrc", "ray_query.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) >= 15 and all(l.startswith("ok") for l in lines)
    for name in ("empty", "identical-1000", "nan-and-inf-vertices", "huge-1e30", "validation", "walk-ends-on-a-broken-tree"):
        assert any(l.startswith("ok " + name) for l in lines), name
