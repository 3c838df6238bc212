"""Morph targets on a machine without a GPU: arctic_morph_vertices against the numpy arbiter bit for bit, every refusal of
arctic_check_morph_targets / arctic_morph_vertices, the struct size and offsets (header, C compiler, numpy dtype), the entry points."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import morph_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"arctic_set_mesh_morph_targets": 5, "arctic_set_mesh_morph_weights": 4, "arctic_check_morph_targets": 3, "arctic_morph_vertices": 6}
INVALID = -1


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
        assert hasattr(L, name)
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == arity
    hpp = open(os.path.join(ROOT, "arctic-renderer_amd", "host", "renderer.hpp")).read()
    for method in ("set_mesh_morph_targets", "set_mesh_morph_weights", "check_morph_targets", "morph_vertices"):
        assert re.search(r"\bbool\s+" + method + r"\s*\(", hpp), method              # the C++ mirror has the same calls
    for method in ("set_mesh_morph_targets", "set_mesh_morph_weights"):
        assert hasattr(pkg.renderer.Renderer, method)
    assert hasattr(pkg.renderer, "morph_vertices") and hasattr(pkg.renderer, "check_morph_targets")
    assert L.arctic_version() == 340 and max(lib.OPTIONS.values()) == 27             # the feature is recognised by its entry points


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no C compiler")
def test_struct_size_and_offsets(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "arctic_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu", sizeof(ArcticMorphDelta), offsetof(ArcticMorphDelta, position), offsetof(ArcticMorphDelta, normal),\n'
                   "         offsetof(ArcticMorphDelta, tangent), offsetof(ArcticMorphDelta, bitangent));\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([shutil.which("cc") or shutil.which("gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    dt = pkg.scene.MORPH_DELTA_DTYPE
    assert got == [48, 0, 12, 24, 36]
    assert [dt.itemsize] + [dt.fields[n][1] for n in R.VERTEX_FIELDS] == got
    assert dt == R.MORPH_DTYPE
    header = open(os.path.join(ROOT, "include", "arctic_hip.h")).read()
    assert re.search(r"typedef struct ArcticMorphDelta \{\s*/\* 48 bytes \*/", header)


@pytest.mark.parametrize("n_targets", [1, 2, 3, 4, 5, 64, 65])
@pytest.mark.parametrize("n_vertices", [1, 63, 64, 65, 257, 1000])
def test_host_morph_matches_the_arbiter_bit_for_bit(pkg, lib, n_vertices, n_targets):
    rng = np.random.default_rng(1000 * n_targets + n_vertices)
    v, d, w = R.random_case(rng, n_vertices, n_targets, pkg.scene.VERTEX_DTYPE)
    assert (w < 0).any() or (w > 1).any() or n_targets < 3
    want = R.morph_vertices(v, d, w)
    got = pkg.renderer.morph_vertices(v, d, w)
    assert got.tobytes() == want.tobytes()
    assert got["position"].tobytes() != v["position"].tobytes() and got["tex_coords"].tobytes() == v["tex_coords"].tobytes()
    # in place
    x = v.copy()
    assert lib.lib().arctic_morph_vertices(x.ctypes.data, d.ctypes.data, len(x), n_targets, w.ctypes.data, x.ctypes.data) == 0
    assert x.tobytes() == want.tobytes()
    # all zero, of either sign: the input's bytes, its -0.0 included
    z = np.zeros(n_targets, np.float32); z[::2] = -0.0
    assert pkg.renderer.morph_vertices(v, d, z).tobytes() == v.tobytes()


def _case(pkg, n=9, nt=4):
    return R.random_case(np.random.default_rng(5), n, nt, pkg.scene.VERTEX_DTYPE)


def test_check_morph_targets_refusals(pkg, lib):
    L = lib.lib()
    v, d, w = _case(pkg)
    ok = lambda dd, n, nt: L.arctic_check_morph_targets(dd.ctypes.data if dd is not None else None, n, nt)
    assert ok(d, len(v), 4) == 0
    assert ok(None, len(v), 4) == INVALID
    assert ok(d, 0, 4) == INVALID
    assert ok(d, len(v), 0) == INVALID
    assert ok(d, len(v), 65536) == INVALID
    assert ok(d, 2 ** 62, 65535) == INVALID                            # a byte count that does not fit: refused before anything is read
    big = np.zeros((65535, 1), R.MORPH_DTYPE)
    assert ok(big, 1, 65535) == 0                                      # the largest legal target count
    for x in (np.nan, np.inf, -np.inf):
        for name in R.VERTEX_FIELDS:
            bad = d.copy(); bad[name][3, 8, 2] = x
            assert ok(bad, len(v), 4) == INVALID
    assert pkg.renderer.check_morph_targets(d) and not pkg.renderer.check_morph_targets(d[:0])


def test_morph_vertices_refusals(pkg, lib):
    L = lib.lib()
    v, d, w = _case(pkg)
    out = np.full(len(v), 0, v.dtype); out["position"] = 77
    p = lambda x: x.ctypes.data
    call = lambda a, b, n, nt, ww, o: L.arctic_morph_vertices(a, b, n, nt, ww, o)
    assert call(p(v), p(d), len(v), 4, p(w), p(out)) == 0
    out["position"] = 77
    for args in [(None, p(d), len(v), 4, p(w), p(out)), (p(v), None, len(v), 4, p(w), p(out)), (p(v), p(d), len(v), 4, None, p(out)),
                 (p(v), p(d), len(v), 4, p(w), None), (p(v), p(d), 0, 4, p(w), p(out)), (p(v), p(d), len(v), 0, p(w), p(out)),
                 (p(v), p(d), len(v), 65536, p(w), p(out))]:
        assert call(*args) == INVALID
    for x in (np.nan, np.inf, -np.inf):
        bad = d.copy(); bad["bitangent"][1, 0, 0] = x
        assert call(p(v), p(bad), len(v), 4, p(w), p(out)) == INVALID
        wb = w.copy(); wb[3] = x                                        # even at a target whose delta is all zero
        assert call(p(v), p(d), len(v), 4, p(wb), p(out)) == INVALID
    assert (out["position"] == 77).all()                                # nothing written by a refused call
    with pytest.raises(pkg.renderer.ArcticError):
        pkg.renderer.morph_vertices(v, d, wb)
    with pytest.raises(pkg.renderer.ArcticError):
        pkg.renderer.morph_vertices(v, d, w[:3])
