"""Ambient occlusion on a machine without a GPU: the entry points (header, binding, C++ mirror), the record's layout through a C compiler,
arctic_ambient_occlusion_points -- the library's own frame, rays, builder and walk on the host -- against the numpy arbiter bit for bit, its
refusals, the kernels' resource figures, and the arbiter under the address and undefined-behaviour sanitizers in a program of its own
(tests/cpp/ao_sanitize.cpp)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ao_reference as A
import ray_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"arctic_trace_ambient_occlusion": 5, "arctic_trace_ambient_occlusion_device": 5, "arctic_ambient_occlusion_points": 9}
INVALID, CAPACITY = -1, -5
FIELDS = ("n_rays", "pattern", "radius", "bias", "filter", "normal_cos", "plane_dist", "reserved")


@pytest.fixture(scope="module")
def lib(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def test_entry_points_and_binding(pkg, lib):
    text = open(os.path.join(ROOT, "include", "arctic_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = lib.lib()
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m and len(m.group(1).split(",")) == arity, name
        assert name in lib.header_symbols() and hasattr(L, name)
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == arity
    hpp = open(os.path.join(ROOT, "arctic-renderer_amd", "host", "renderer.hpp")).read()
    for method in ("trace_ambient_occlusion", "trace_ambient_occlusion_device", "ambient_occlusion_points"):
        assert re.search(r"\[\[nodiscard\]\]\s+(static\s+)?bool\s+" + method + r"\s*\(", hpp), method
    for method in ("trace_ambient_occlusion", "trace_ambient_occlusion_device"):
        assert hasattr(pkg.renderer.Renderer, method)
    assert hasattr(pkg.renderer, "ambient_occlusion_points") and hasattr(pkg.renderer, "ao_directions")
    # the definition stands in the header, in front of the calls
    for phrase in ("s = copysign(1.0f, m2)", "a = -1.0f / (s + m2)", "(510*(n_rays - hits) + n_rays) / (2*n_rays)", "(510*V + T) / (2*T)", "p itself is always accepted",
                   "(y % P) * P + x % P", "NOT COVERED", "the row of the FRAME"):
        assert phrase in text, phrase
    assert text.index("s = copysign(1.0f, m2)") < text.index("int arctic_trace_ambient_occlusion(")


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no C compiler")
def test_struct_size_and_offsets(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "arctic_hip.h"\nint main(void) {\n  printf("%zu", sizeof(ArcticAmbientOcclusion));\n'
                   + "".join(f'  printf(" %zu", offsetof(ArcticAmbientOcclusion, {f}));\n' for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([shutil.which("cc") or shutil.which("gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [32, 0, 4, 8, 12, 16, 20, 24, 28]
    ao = pkg.scene.AO_DTYPE
    assert [ao.itemsize] + [ao.fields[n][1] for n in FIELDS] == got and ao.names == FIELDS
    assert [ao.fields[n][0].kind for n in FIELDS] == ["u", "u", "f", "f", "u", "f", "f", "u"]
    assert re.search(r"typedef struct ArcticAmbientOcclusion \{\s*/\* 32 bytes \*/", open(os.path.join(ROOT, "include", "arctic_hip.h")).read())


# ---- the arbiter against the reference ----------------------------------------------------------------------------------------------------------
_SCENES = {}


def scene(n_tris):
    """soup triangles and 300 points: half on the triangles, with general normals, the others with normals along the axes (whose frames turn a local
    direction with a zero component into a world direction with one: the odd walk) and with the degenerate normals of the definition"""
    if n_tris not in _SCENES:
        rng = np.random.default_rng(31000 + n_tris)
        tris = R.soup_triangles(rng, n_tris)
        t = tris.reshape(-1, 3, 3)
        n = 300
        world = (t[rng.integers(0, len(t), n)] * rng.dirichlet(np.ones(3), n).astype(np.float32)[:, :, None]).sum(1).astype(np.float32)
        nrm = rng.normal(size=(n, 3)).astype(np.float32) * rng.uniform(0.2, 4.0, (n, 1)).astype(np.float32)   # (not unit vectors)
        special = [(0, 0, 1), (0, 0, -1), (0, 0, -0.0), (0.6, 0.8, -0.0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, 0), (3e19, 3e19, 3e19), (1e-30, 1e-30, 0),
                   (np.nan, 0, 1), (0, -np.inf, 0), (3, 0, 4)]
        for k in range(n // 2, n):
            nrm[k] = special[k % len(special)]
        world[7, 1], world[8, 0] = np.nan, np.inf                                            # covered, every ray invalid
        _SCENES[n_tris] = (tris, np.concatenate([world, nrm], 1))
    return _SCENES[n_tris]


def directions(n_rays, P):
    """a table with general directions, directions with one and two zero components, one at the subnormal edge, and one below the horizon"""
    rng = np.random.default_rng(n_rays * 10 + P)
    d = rng.normal(size=(P * P, n_rays, 3)).astype(np.float32)
    d[..., 2] = np.abs(d[..., 2])
    d[0, 0] = (0, 0, 1)
    d[-1, -1] = (0.5, 0, 0.5)
    if n_rays >= 4:
        d[0, 1], d[0, 2], d[0, 3] = (1e-45, 0.5, 0.7), (0.3, 0.2, -0.4), (0, 0, 0)          # (a zero direction: an invalid ray, a miss)
    return d


@pytest.mark.parametrize("radius", [1.5, np.inf])
@pytest.mark.parametrize("pattern", [1, 2, 4])
@pytest.mark.parametrize("n_rays", [1, 4, 5, 64])
@pytest.mark.parametrize("n_tris", [1, 5, 1000])
def test_the_arbiter_equals_the_reference_bit_for_bit(pkg, lib, n_tris, n_rays, pattern, radius):
    tris, points = scene(n_tris)
    dirs = directions(n_rays, pattern)
    sets = (np.arange(len(points)) * 7) % (pattern * pattern)
    want = A.point_hits(tris, points, sets, dirs, n_rays, radius, 1e-3, brute=n_tris < 1000)
    for brute in (False, True):
        got = pkg.renderer.ambient_occlusion_points(tris, points, sets, dirs, radius=radius, bias=1e-3, brute=brute)
        assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), (brute, np.nonzero(got != want)[0][:8].tolist())
    # not vacuous: points that are hit and points that are not, the points that are not covered among the latter, and odd rays among those cast
    _, ok = A.normal(points[:, 3:6])
    assert (~ok).sum() >= 20 and (want[~ok] == 0).all() and (want[[7, 8]] == 0).all()
    if n_tris >= 5:
        assert (want[ok] > 0).mean() >= 0.2 and (want[ok] < n_rays).mean() >= 0.2
    ry, _ = A.point_rays(points, sets, dirs, n_rays, radius, 1e-3)
    cast = ry[ok].reshape(-1)
    assert (R.ray_odd(cast) & R.ray_valid(cast)).sum() >= 3 and (~R.ray_odd(cast)).sum() >= 3


def test_the_radius_and_the_bias_matter(pkg, lib):
    tris, points = scene(1000)
    dirs = directions(5, 2)
    sets = np.arange(len(points)) % 4
    a = pkg.renderer.ambient_occlusion_points(tris, points, sets, dirs, radius=0.5)
    assert (a != pkg.renderer.ambient_occlusion_points(tris, points, sets, dirs)).mean() >= 0.05
    assert (a != pkg.renderer.ambient_occlusion_points(tris, points, sets, dirs, radius=0.5, bias=0.0)).mean() >= 0.05
    assert (a != pkg.renderer.ambient_occlusion_points(tris, points, (sets + 1) % 4, dirs, radius=0.5)).mean() >= 0.05


def test_refusals_write_nothing(pkg, lib):
    L = lib.lib()
    tris, points = scene(5)
    points = np.ascontiguousarray(points[:32])
    dirs = directions(4, 2).reshape(-1)
    sets = (np.arange(32) % 4).astype(np.uint32)
    good = np.zeros(1, pkg.scene.AO_DTYPE)
    good["n_rays"], good["pattern"], good["radius"], good["bias"] = 4, 2, np.inf, 1e-3
    hits = np.full(32, 77, np.uint8)
    p = lambda a: a.ctypes.data

    def call(ao=good, t=p(tris), nt=5, pts=p(points), st=p(sets), n=32, d=p(dirs), flags=0, h=p(hits)):
        return L.arctic_ambient_occlusion_points(t, nt, pts, st, n, None if ao is None else p(ao), d, flags, h)

    def changed(**kw):
        ao = good.copy()
        for k, v in kw.items():
            ao[k] = v
        return ao
    assert call() == 0 and (hits <= 4).all()
    hits[:] = 77
    nan, inf = np.nan, np.inf
    for ao in [None, changed(n_rays=0), changed(n_rays=65), changed(pattern=0), changed(pattern=3), changed(pattern=8), changed(radius=0.0), changed(radius=-1.0),
               changed(radius=nan), changed(bias=inf), changed(bias=nan), changed(filter=2), changed(reserved=1), changed(filter=1, normal_cos=nan),
               changed(filter=1, normal_cos=inf), changed(filter=1, plane_dist=-1e-9), changed(filter=1, plane_dist=nan)]:
        assert call(ao=ao) == INVALID, None if ao is None else ao.tolist()
    assert call(ao=changed(filter=1, normal_cos=0.5, plane_dist=0.0)) == 0                    # (the filter's own parameters are checked and otherwise unused)
    assert call(ao=changed(normal_cos=nan, plane_dist=-1.0)) == 0                             # ... and not looked at with the filter off
    hits[:] = 77
    for kw in [dict(d=None), dict(t=None), dict(pts=None), dict(st=None), dict(h=None), dict(flags=1), dict(flags=4), dict(flags=0x80000002)]:
        assert call(**kw) == INVALID, kw
    for k, v in ((0, nan), (5, inf), (len(dirs) - 1, -inf)):
        bad = dirs.copy()
        bad[k] = v
        assert call(d=p(bad)) == INVALID, k
    bad = sets.copy()
    bad[31] = 4
    assert call(st=p(bad)) == INVALID
    assert call(nt=0xFFFFFFFF) == CAPACITY
    assert (hits == 77).all()                                                                 # nothing written by a refused call
    assert call(t=None, nt=0, pts=None, st=None, n=0, h=None) == 0
    with pytest.raises(pkg.renderer.ArcticError):
        pkg.renderer.ambient_occlusion_points(tris, points, sets, dirs.reshape(4, 4, 3), radius=-1.0)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_ao_kernels_use_no_scratch(tmp_path):
    """k_trace_ao and k_ao_filter: no scratch (the walk has no stack, the frame and the ray no runtime-indexed array), no LDS, at least 4 waves per
    SIMD, and every store a vector store of one byte"""
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    log = subprocess.run(["make", "-C", csrc, "asm-ao", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    names = re.findall(r"Function Name: (\S+)", remarks)
    assert len(names) == 2 and sum("k_trace_ao" in n for n in names) == 1 and sum("k_ao_filter" in n for n in names) == 1, names
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)] == [0, 0]
    assert [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)] == [0, 0]
    occupancy = [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", remarks)]
    assert len(occupancy) == 2 and all(x >= 4 for x in occupancy), occupancy
    path = str(tmp_path / "ray_ao-hip-amdgcn-amd-amdhsa-gfx950.s")
    name, scratch, stores = None, {}, {}
    for line in open(path):
        m = re.match(r"(_Z\w+):", line)
        if m:
            name = m.group(1)
        op = line.split()[0] if line.strip() else ""
        if name and "store" in op:
            stores.setdefault(name, set()).add(op)
        if name and line.startswith("; ScratchSize:"):
            scratch[name] = int(line.split(":")[1].split()[0])
    assert len(scratch) == 2 and all(v == 0 for v in scratch.values()), scratch
    assert len(stores) == 2 and all(ops == {"global_store_byte"} for ops in stores.values()), stores


def test_arbiter_under_sanitizers():
    """tests/cpp/ao_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    driver = os.path.join(ROOT, "tests", "cpp", "ao_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "ao_sanitize.cpp"), os.path.join(csrc, "ray_ao.cpp"), os.path.join(csrc, "bvh.cpp")]
    deps = src + [os.path.join(csrc, "ray_query.h"), os.path.join(csrc, "ray_ao.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) >= 13 and all(l.startswith("ok") for l in lines)
    for name in ("empty", "no-points", "large-20000", "nan-and-inf-vertices", "huge-1e30", "refusals", "nothing-to-do"):
        assert any(l.startswith("ok " + name) for l in lines), name
