"""arctic_set_material_extras / arctic_check_material_params on a machine without a GPU: the ArcticMaterialParams layout (header, C compiler,
numpy dtype), the entry points in the header, the ctypes binding and the C++ mirror, the validation rules, the version, no new option id, and
the ISA of the k_pbrlit kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["base_color_factor", "metallic_factor", "roughness_factor", "normal_scale", "occlusion_strength", "emissive_factor", "reserved"]
ENTRY_POINTS = {"arctic_set_material_extras": 9, "arctic_check_material_params": 1}


@pytest.fixture(scope="module")
def lib(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arctic_hip.h")).read(), flags=re.S)


def test_header_binding_and_cpp_mirror_agree(pkg, lib):
    header, hpp = _header(), open(os.path.join(ROOT, "arctic-renderer_amd", "host", "renderer.hpp")).read()
    L = lib.lib()
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name
        assert len(m.group(1).split(",")) == arity
        assert name in lib.header_symbols() and hasattr(L, name)
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == arity
        call = re.search(name + r"\s*\(([^;]*)\)\s*[;)=]", hpp)
        assert call and len(call.group(1).split(",")) == arity, name
    for method in ("set_material_extras", "check_material_params"):
        assert re.search(r"\bbool\s+" + method + r"\s*\(", hpp), method
        assert hasattr(pkg.renderer.Renderer, method) or hasattr(pkg.renderer, method)
    assert hasattr(pkg.renderer.Renderer, "set_material_extras") and hasattr(pkg.renderer, "check_material_params")
    assert L.arctic_version() >= 320


@pytest.mark.skipif(shutil.which("cc") is None and shutil.which("gcc") is None, reason="no C compiler")
def test_layout_matches_header_and_dtype(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "arctic_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(ArcticMaterialParams));\n' +
                   "".join(f'  printf(" %zu", offsetof(ArcticMaterialParams, {f}));\n' for f in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([shutil.which("cc") or shutil.which("gcc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    dt = pkg.scene.MATERIAL_PARAMS_DTYPE
    assert got[0] == 48 == dt.itemsize
    assert got[1:] == [dt.fields[f][1] for f in FIELDS] == [0, 12, 16, 20, 24, 28, 40]
    assert pkg.renderer.MATERIAL_PARAMS_DTYPE is dt


def _check(lib, p):
    return lib.lib().arctic_check_material_params(np.ascontiguousarray(p).ctypes.data)


def test_neutral_and_in_range_blocks_are_accepted(pkg, lib):
    n = pkg.scene.neutral_material_params()
    assert n.tobytes() == np.float32([1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]).tobytes()
    assert _check(lib, n) == 0 and pkg.renderer.check_material_params(n[0])
    p = n.copy()
    p["base_color_factor"], p["metallic_factor"], p["roughness_factor"], p["occlusion_strength"] = (0, 0.5, 1), 0, 0, 0
    p["normal_scale"], p["emissive_factor"] = -3.5, (0, 40.0, 1e6)          # any finite scale; emission may exceed 1
    assert _check(lib, p) == 0
    assert lib.lib().arctic_check_material_params(None) == -1


BAD = [(f, i, v) for f, idx in (("base_color_factor", (0, 1, 2)), ("metallic_factor", (None,)), ("roughness_factor", (None,)), ("occlusion_strength", (None,)))
       for i in idx for v in (-0.01, 1.01, np.nan, np.inf, -np.inf)]
BAD += [("normal_scale", None, v) for v in (np.nan, np.inf, -np.inf)]
BAD += [("emissive_factor", i, v) for i in (0, 1, 2) for v in (-0.01, np.nan, np.inf, -np.inf)]
BAD += [("reserved", i, v) for i in (0, 1) for v in (1.0, -1.0, 1e-30, np.nan, np.inf)]


@pytest.mark.parametrize("field,index,value", BAD)
def test_each_field_out_of_range_is_refused(pkg, lib, field, index, value):
    p = pkg.scene.neutral_material_params()
    if index is None:
        p[field] = value
    else:
        p[field][0, index] = value
    assert _check(lib, p) == -1
    assert not pkg.renderer.check_material_params(p[0])


def test_no_option_id_above_texture_mips(lib):
    ids = {name: int(v) for name, v in re.findall(r"#define\s+(ARCTIC_OPT_\w+)\s+(\d+)", open(os.path.join(ROOT, "include", "arctic_hip.h")).read())}
    assert ids["ARCTIC_OPT_TEXTURE_MIPS"] == max(ids.values()) == lib.OPTIONS["texture_mips"] == max(lib.OPTIONS.values())


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_pbrlit_kernels_are_clean(tmp_path):
    """the ISA of k_pbrlit / k_pbrlit_vis (ENV x MIP, both light loops): tools/isa_lint.py finds no hazard, and none spills"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "asm", f"OUT={tmp_path}"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    path = str(tmp_path / "shade-hip-amdgcn-amd-amdhsa-gfx950.s")
    rep = isa_lint.lint(path, match="k_pbrlit")
    assert rep.problems == [], "\n".join(rep.problems)
    assert rep.kernels == 16
    name, scratch = None, {}
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            name = m.group(1)
        if name and line.startswith("; ScratchSize:"):
            scratch[name] = int(line.split(":")[1].split()[0])
    pbr = {k: v for k, v in scratch.items() if "k_pbrlit" in k}
    assert len(pbr) == 16 and all(v == 0 for v in pbr.values()), pbr
    # the families the existing tests count by name are what they were
    for family in ("k_envlit", "k_spotlit", "k_cubelit", "k_miplit"):
        assert sum(family in k for k in scratch) in (4, 8), family
