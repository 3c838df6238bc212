"""Shadow-casting point lights on a machine without a GPU: the ArcticPointShadowLight layout (header, C compiler, numpy dtype), the
exported entry points, the face matrices against float64 numpy, the validation rules, and the ISA of the k_cubelit kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["position", "z_near", "color", "z_far"]
ENTRY_POINTS = ("arctic_update_point_shadow_lights", "arctic_point_shadow_matrices", "arctic_pass_point_shadows",
                "arctic_read_point_shadow", "arctic_write_point_shadow")
# face k: the axis it looks along, lookAtRH's up, and the documented rows s (clip x) and u (clip y) of the lookup
DIRS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
UPS = np.array([[0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, -1, 0]], np.float64)
S_ROWS = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], np.float64)
U_ROWS = np.array([[0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, -1, 0]], np.float64)


@pytest.fixture(scope="module")
def lib(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def light(pkg, position=(0.5, 1.25, -2.0), z_near=0.1, z_far=25.0, color=(1, 2, 3)):
    a = np.zeros(1, pkg.scene.POINT_SHADOW_LIGHT_DTYPE)
    a["position"], a["z_near"], a["z_far"], a["color"] = position, z_near, z_far, color
    return a


def matrices(lib, a):
    out = np.full(96, np.nan, np.float32)
    rc = lib.lib().arctic_point_shadow_matrices(np.ascontiguousarray(a).ctypes.data, out.ctypes.data)
    return rc, out.reshape(6, 4, 4).transpose(0, 2, 1)   # [face][row][col]


def reference(p, zn, zf):
    """float64 perspectiveRH_ZO(90 deg, 1, zn, zf) * lookAtRH(p, p + dir_k, up_k), [face][row][col]"""
    out = []
    for k in range(6):
        f = DIRS[k]
        s = np.cross(f, UPS[k]); s /= np.linalg.norm(s)
        u = np.cross(s, f)
        view = np.eye(4)
        view[0, :3], view[1, :3], view[2, :3] = s, u, -f
        view[0, 3], view[1, 3], view[2, 3] = -s @ p, -u @ p, f @ p
        proj = np.zeros((4, 4))
        proj[0, 0] = proj[1, 1] = 1.0
        proj[2, 2] = zf / (zn - zf)
        proj[3, 2] = -1.0
        proj[2, 3] = -(zf * zn) / (zf - zn)
        out.append(proj @ view)
    return np.array(out)


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no C compiler")
def test_layout_matches_header_and_dtype(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "arctic_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(ArcticPointShadowLight));\n' +
                   "".join(f'  printf(" %zu", offsetof(ArcticPointShadowLight, {f}));\n' for f in FIELDS) +
                   '  printf(" %d", ARCTIC_OPT_POINT_SHADOW_SIZE);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call([shutil.which("cc") or shutil.which("gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    dt = pkg.scene.POINT_SHADOW_LIGHT_DTYPE
    assert got[0] == 32 == dt.itemsize
    assert got[1:5] == [dt.fields[f][1] for f in FIELDS] == [0, 12, 16, 28]
    assert got[5] == 26
    assert pkg.renderer.POINT_SHADOW_LIGHT_DTYPE is dt


def test_library_exports_point_shadow_entry_points(lib):
    L = lib.lib()
    for n in ENTRY_POINTS:
        assert hasattr(L, n) and n in lib.header_symbols() and n in lib.SIGNATURES
    assert lib.OPTIONS["point_shadow_size"] == 26
    assert L.arctic_version() >= 300


def test_matrices_match_float64(pkg, lib):
    rng = np.random.default_rng(11)
    for _ in range(40):
        p = rng.uniform(-20, 20, 3)
        zn = rng.uniform(0.01, 1.0)
        zf = zn + rng.uniform(0.5, 100.0)
        a = light(pkg, p, zn, zf)
        rc, M = matrices(lib, a)
        assert rc == 0
        ref = reference(a["position"][0].astype(np.float64), float(a["z_near"][0]), float(a["z_far"][0]))
        # 1e-6 relative to the size of the terms an entry is made of
        scale = np.maximum(np.abs(ref), 1e-6 * 0 + np.abs(ref[:, :, :3]).max(axis=2, keepdims=True) * (1 + np.abs(a["position"][0]).max()))
        assert (np.abs(M - ref) <= 1e-6 * scale).all()
        structural = (ref == 0) | (np.abs(ref) == 1)
        structural[:, :3, 3] = False          # translations: rounded products of p
        np.testing.assert_array_equal(M[structural], ref[structural])


def test_faces_project_axis_to_centre_and_rows_to_edges(pkg, lib):
    p = np.array([0.5, 1.25, -2.0])
    a = light(pkg, p, 0.1, 25.0)
    rc, M = matrices(lib, a)
    assert rc == 0
    M = M.astype(np.float64)
    for k in range(6):
        dist = 3.0
        for off_s, off_u, want_x, want_y in [(0, 0, 0.5, 0.5), (1, 0, 1.0, 0.5), (-1, 0, 0.0, 0.5), (0, 1, 0.5, 0.0), (0, -1, 0.5, 1.0)]:
            w = p + DIRS[k] * dist + (S_ROWS[k] * off_s + U_ROWS[k] * off_u) * dist   # s / u offsets of one m land on the edges
            c = M[k] @ np.append(w, 1.0)
            px, py, pz = 0.5 + 0.5 * c[0] / c[3], 0.5 - 0.5 * c[1] / c[3], c[2] / c[3]
            assert abs(px - want_x) < 1e-6 and abs(py - want_y) < 1e-6, (k, off_s, off_u, px, py)
            zn, zf = 0.1, 25.0
            assert abs(pz - float(np.float32(zf / (zf - zn))) * (1 - zn / dist)) < 1e-6


@pytest.mark.parametrize("field,value", [("position", (np.nan, 0, 0)), ("position", (0, np.inf, 0)), ("color", (1, np.nan, 1)),
                                         ("color", (1, 1, -np.inf)), ("z_near", 0.0), ("z_near", -1.0), ("z_near", np.nan),
                                         ("z_far", 0.1), ("z_far", 0.05), ("z_far", np.inf), ("z_far", np.nan)])
def test_invalid_lights_are_refused(pkg, lib, field, value):
    good = light(pkg, z_near=0.1, z_far=25.0)
    assert matrices(lib, good)[0] == 0
    bad = good.copy()
    bad[0][field] = value
    rc, out = matrices(lib, bad)
    assert rc == -1 and np.isnan(out).all()    # nothing written
    with pytest.raises(pkg.renderer.ArcticError):
        pkg.renderer.point_shadow_matrices(bad[0])


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_cubelit_kernels_are_clean(tmp_path):
    """the ISA of k_cubelit / k_cubelit_vis (both ENV variants, both light loops): tools/isa_lint.py finds no hazard, and none spills"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "asm", f"OUT={tmp_path}"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    path = str(tmp_path / "shade-hip-amdgcn-amd-amdhsa-gfx950.s")
    rep = isa_lint.lint(path, match="k_cubelit")
    assert rep.problems == [], "\n".join(rep.problems)
    assert rep.kernels == 8
    name, scratch = None, {}
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            name = m.group(1)
        if name and line.startswith("; ScratchSize:"):
            scratch[name] = int(line.split(":")[1].split()[0])
    cube_k = {k: v for k, v in scratch.items() if "k_cubelit" in k}
    assert len(cube_k) == 8 and all(v == 0 for v in cube_k.values()), cube_k
