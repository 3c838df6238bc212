"""Spot lights on a machine without a GPU: the ArcticSpotLight layout (header, C compiler, numpy dtype), the exported entry points, the
host-side derivation of the device constants against float64 numpy, the validation rules, and the ISA of the spot kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["position", "range", "direction", "inner_cone_angle", "color", "outer_cone_angle"]
PI_F = float(np.float32(np.pi))   # "pi" of the API: the fp32 value nearest pi


@pytest.fixture(scope="module")
def lib(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def constants(lib, lights):
    L = lib.lib()
    lights = np.ascontiguousarray(lights)
    out = np.full((len(lights), 12), np.nan, np.float32)
    rc = L.arctic_spot_light_constants(lights.ctypes.data if len(lights) else None, len(lights), out.ctypes.data)
    return rc, out


def spot(pkg, position=(0, 0, 0), rng_=0.0, direction=(0, -1, 0), inner=0.2, outer=0.5, color=(1, 2, 3)):
    a = np.zeros(1, pkg.scene.SPOT_LIGHT_DTYPE)
    a["position"], a["range"], a["direction"] = position, rng_, direction
    a["inner_cone_angle"], a["outer_cone_angle"], a["color"] = inner, outer, color
    return a


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no C compiler")
def test_layout_matches_header_and_dtype(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "arctic_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(ArcticSpotLight));\n' +
                   "".join(f'  printf(" %zu", offsetof(ArcticSpotLight, {f}));\n' for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([shutil.which("cc") or shutil.which("gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    dt = pkg.scene.SPOT_LIGHT_DTYPE
    assert got[0] == 48 == dt.itemsize
    assert got[1:] == [dt.fields[f][1] for f in FIELDS] == [0, 12, 16, 28, 32, 44]
    assert pkg.renderer.SPOT_LIGHT_DTYPE is dt


def test_library_exports_spot_entry_points(lib):
    L = lib.lib()
    for n in ("arctic_update_spot_lights", "arctic_spot_light_constants"):
        assert hasattr(L, n) and n in lib.header_symbols() and n in lib.SIGNATURES
    assert L.arctic_version() >= 200


def test_host_derivation_matches_float64(pkg, lib):
    rng = np.random.default_rng(5)
    n = 64
    a = np.zeros(n, pkg.scene.SPOT_LIGHT_DTYPE)
    a["position"] = rng.uniform(-10, 10, (n, 3))
    a["direction"] = rng.standard_normal((n, 3)) * rng.uniform(1e-3, 1e3, (n, 1))
    outer = rng.uniform(0.01, 3.0, n)
    a["outer_cone_angle"] = outer
    a["inner_cone_angle"] = outer * rng.uniform(0, 1, n)
    a["inner_cone_angle"][:4] = a["outer_cone_angle"][:4]     # hard cones: scale = 1000
    a["outer_cone_angle"][4:8] = PI_F                        # omnidirectional
    a["range"] = np.where(rng.random(n) < 0.5, 0.0, rng.uniform(0.1, 50, n))
    a["color"] = rng.uniform(0, 100, (n, 3))
    rc, out = constants(lib, a)
    assert rc == 0
    d = a["direction"].astype(np.float64)
    s = d / np.linalg.norm(d, axis=1, keepdims=True)
    ci, co = np.cos(a["inner_cone_angle"].astype(np.float64)), np.cos(a["outer_cone_angle"].astype(np.float64))
    scale = 1.0 / np.maximum(1e-3, ci - co)
    offset = -co * scale
    omni = a["outer_cone_angle"] == np.float32(np.pi)
    scale, offset = np.where(omni, 0.0, scale), np.where(omni, 1.0, offset)
    r = a["range"].astype(np.float64)
    ir2 = np.where(r > 0, 1.0 / np.where(r > 0, r, 1.0) ** 2, 0.0)
    want = np.concatenate([a["position"], scale[:, None], s, offset[:, None], a["color"], ir2[:, None]], 1).astype(np.float32)
    np.testing.assert_array_equal(out, want)
    assert (out[:4, 3] == np.float32(1000.0)).all()
    assert (out[4:8, 3] == 0).all() and (out[4:8, 7] == 1).all()


@pytest.mark.parametrize("field,value", [("position", (np.nan, 0, 0)), ("color", (1, np.inf, 1)), ("range", -1.0),
                                         ("range", np.inf), ("direction", (0, 0, 0)), ("inner_cone_angle", 0.6),
                                         ("inner_cone_angle", -0.1), ("outer_cone_angle", 0.0),
                                         ("outer_cone_angle", 3.2), ("outer_cone_angle", np.nan)])
def test_invalid_lights_are_refused(pkg, lib, field, value):
    good = spot(pkg)
    assert constants(lib, good)[0] == 0
    bad = np.concatenate([good, spot(pkg)])
    bad[1][field] = value
    rc, out = constants(lib, bad)
    assert rc == -1 and np.isnan(out).all()    # nothing written


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_spotlit_kernels_are_clean(tmp_path):
    """the ISA of k_spotlit / k_spotlit_vis (both ENV variants, both light loops): tools/isa_lint.py finds no hazard, and none spills"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "asm", f"OUT={tmp_path}"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    path = str(tmp_path / "shade-hip-amdgcn-amd-amdhsa-gfx950.s")
    rep = isa_lint.lint(path, match="k_spotlit")
    assert rep.problems == [], "\n".join(rep.problems)
    assert rep.kernels == 8
    name, scratch = None, {}
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            name = m.group(1)
        if name and line.startswith("; ScratchSize:"):
            scratch[name] = int(line.split(":")[1].split()[0])
    spot_k = {k: v for k, v in scratch.items() if "k_spotlit" in k}
    assert len(spot_k) == 8 and all(v == 0 for v in spot_k.values()), spot_k
