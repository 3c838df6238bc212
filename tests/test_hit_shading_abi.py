"""Hit attributes, hit shading and the reflection plane on a machine without a GPU: the entry points (header, binding, C++ mirror, Python
surface), the definition standing in the header in front of the calls, the refusals that need no device -- a null handle, and everything
arctic_interpolate_hits refuses, each leaving the outputs untouched --, and the kernels' resource figures (make asm-hit)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"arctic_hit_attributes": 6, "arctic_interpolate_hits": 12, "arctic_shade_hits": 7, "arctic_shade_hits_device": 7,
                "arctic_trace_reflections": 4, "arctic_trace_reflections_device": 4, "arctic_hit_shading_info": 2}
INVALID, CAPACITY = -1, -5


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
    hpp = open(os.path.join(ROOT, "arctic-renderer_amd", "host", "renderer.hpp")).read()
    for method in ("hit_attributes", "interpolate_hits", "shade_hits", "shade_hits_device", "trace_reflections", "trace_reflections_device", "hit_shading_info"):
        assert re.search(r"\[\[nodiscard\]\]\s+(static\s+)?bool\s+" + method + r"\s*\(", hpp), method
    for method in ("hit_attributes", "shade_hits", "shade_hits_device", "trace_reflections", "trace_reflections_device", "hit_shading_info"):
        assert hasattr(pkg.renderer.Renderer, method)
    assert hasattr(pkg.renderer, "interpolate_hits")
    # the definition stands in the header, in front of the calls, and says what is out of scope
    for phrase in ("w0 = (1.0f - u) - v", "(w0*a0 + u*a1) + v*a2", "skipped but numbered", "NOT transformed by trs", "IN USE", "eye := rays[k].origin",
                   "OUT OF SCOPE at hits", "spot lights, shadow-casting point lights, image-based ambient", "d[j] = i[j] - (2.0f*k)*m[j]", "k >= 0",
                   "INTERPOLATED VERTEX NORMAL", "never\n *   drawn or written", "ARCTIC_OPT_SHADOW_SHARDED"):
        assert phrase in text, phrase
    assert text.index("w0 = (1.0f - u) - v") < text.index("int arctic_hit_attributes(") < text.index("int arctic_shade_hits(") < text.index("int arctic_trace_reflections(")
    make = open(os.path.join(ROOT, "arctic-renderer_amd", "csrc", "Makefile")).read()
    assert re.search(r"^hit_shade\.o:.*\n\t\$\(HIPCC\) \$\(COMMON\) \$\(EXACT\) ", make, flags=re.M) and "asm-hit:" in make


def test_a_null_handle_is_refused_before_anything_is_touched(pkg, lib):
    L = lib.lib()
    s = pkg.scene.CScene()
    rays, hits = np.zeros(4, pkg.scene.RAY_DTYPE), np.zeros(4, pkg.scene.HIT_DTYPE)
    attrs, mat, rgba = np.full((4, 18), 77, np.float32), np.full(4, 77, np.uint32), np.full((4, 4), 77, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.arctic_hit_attributes(None, C.byref(s), p(hits), 4, p(attrs), p(mat)) == INVALID
    assert L.arctic_shade_hits(None, C.byref(s), p(rays), p(hits), 4, 0, p(rgba)) == INVALID
    assert L.arctic_shade_hits_device(None, C.byref(s), p(rays), p(hits), 4, 0, p(rgba)) == INVALID
    assert L.arctic_trace_reflections(None, C.byref(s), 1e-3, p(rgba)) == INVALID
    assert L.arctic_trace_reflections_device(None, C.byref(s), 1e-3, p(rgba)) == INVALID
    info = np.full(4, 77, np.uint64)
    assert L.arctic_hit_shading_info(None, p(info)) == INVALID
    assert (attrs == 77).all() and (mat == 77).all() and (rgba == 77).all() and (info == 77).all()


def test_the_arbiter_refuses_and_writes_nothing(pkg, lib):
    L = lib.lib()
    v = np.zeros(3, pkg.scene.VERTEX_DTYPE)
    v["position"] = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    v["normal"], v["tangent"], v["bitangent"] = (0, 0, 2), (3, 0, 0), (0, 4, 0)
    v["tex_coords"] = [(0, 0), (1, 0), (0, 1)]
    ix = np.array([0, 1, 2, 0, 1, 3], np.uint32)                                 # the second triangle has an index out of range
    eye = np.eye(4, dtype=np.float32).reshape(16)
    hits = np.zeros(3, pkg.scene.HIT_DTYPE)
    hits["u"], hits["v"], hits["prim"] = 0.25, 0.5, [10, 11, 12]                # the object's prims are 10 and 11
    attrs, mat = np.full((3, 18), 77, np.float32), np.full(3, 77, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(vv=p(v), nv=3, ii=p(ix), ni=6, trs=p(eye), lpv=p(eye), first=10, hh=p(hits), n=3, aa=p(attrs), mm=p(mat)):
        return L.arctic_interpolate_hits(vv, nv, ii, ni, trs, lpv, 5, first, hh, n, aa, mm)
    for kw in (dict(vv=None), dict(ii=None), dict(trs=None), dict(lpv=None), dict(hh=None), dict(aa=None), dict(mm=None)):
        assert call(**kw) == INVALID, kw
    assert call(nv=1 << 32) == CAPACITY and call(first=0xFFFFFFFE) == CAPACITY
    assert (attrs == 77).all() and (mat == 77).all()
    assert call() == 0
    assert mat.tolist() == [5, 0xFFFFFFFF, 77] and not attrs[1].any() and (attrs[2] == 77).all()     # resolved; skipped but numbered; another object's: left as it is
    want = np.array([0.25, 0.5, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.25, 0.5, 0, 0.25, 0.5, 0, 1], np.float32)   # uv, unit t / b / n, world, light space (identity, w = 1)
    assert np.array_equal(attrs[0], want), attrs[0].tolist()
    assert call(vv=None, nv=0, ii=None, ni=0, hh=None, n=0, aa=None, mm=None) == 0


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_hit_kernels_use_no_scratch(tmp_path):
    """k_hit_attributes, k_shade_hits and k_reflect_rays: no scratch (no runtime-indexed array: the attributes, the footprint and the taps are
    unrolled) and no LDS"""
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    log = subprocess.run(["make", "-C", csrc, "asm-hit", f"OUT={tmp_path}"], capture_output=True, text=True, check=True)
    remarks = log.stdout + log.stderr
    names = re.findall(r"Function Name: (\S+)", remarks)
    assert len(names) == 3 and all(sum(k in n for n in names) == 1 for k in ("k_hit_attributes", "k_shade_hits", "k_reflect_rays")), names
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)] == [0, 0, 0]
    assert [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", remarks)] == [0, 0, 0]
    path = str(tmp_path / "hit_shade-hip-amdgcn-amd-amdhsa-gfx950.s")
    scratch = [int(line.split(":")[1].split()[0]) for line in open(path) if line.startswith("; ScratchSize:")]
    assert scratch == [0, 0, 0], scratch
