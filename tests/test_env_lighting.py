"""ARCTIC_OPT_ENV_LIGHTING without a GPU: the C-ABI declares and exports it, the float64 numpy reference the GPU tests
compare against gives the known answers of its own semantics, and the new shading kernels' ISA is clean."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import env_reference as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_defines_the_option_and_the_read_back():
    text = open(os.path.join(ROOT, "include", "arctic_hip.h")).read()
    m = re.search(r"#define ARCTIC_OPT_ENV_LIGHTING\s+(\d+)", text)
    assert m and int(m.group(1)) == 25
    assert "int arctic_read_env_lighting(ArcticRenderer *r, float *sh27, float *lut, uint32_t level, float *texels, uint32_t *dims);" in text


def test_library_exports_the_read_back(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    L = b.lib()
    assert hasattr(L, "arctic_read_env_lighting")
    assert b.OPTIONS["env_lighting"] == 25
    # without a handle the call is refused, not crashed
    assert L.arctic_read_env_lighting(None, None, None, 0, None, None) == -1


def test_constant_map_irradiance_is_pi_c():
    """E(n) = pi c for a constant map c, within what the rounded constants add: the weights sum to 4 pi (1 + 3.5e-4), and the azimuths
    overlap by 3.5e-4 of a turn at the map's seam (phi = +-pi, direction -x), which weighs the seam twice -- a dipole that puts E(-x) at
    pi c (1 + 1.1e-3)"""
    c = np.array([0.7, 1.3, 2.0])
    env = np.ones((64, 128, 4), np.float32)
    env[..., :3] = c
    sh = ER.sh_project(env)
    d, ct = ER.texel_dirs(128, 64)
    total = (np.maximum(ct, 0) / (ER.C_U * 128) / (ER.C_V * 64)).sum()
    assert 3.4e-4 < total / (4 * np.pi) - 1 < 4.6e-4    # (3.5e-4 in the limit; the midpoint rule over 64 rows adds 1e-4)
    rng = np.random.default_rng(1)
    n = rng.standard_normal((200, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    E = ER.sh_irradiance(sh, n)
    np.testing.assert_allclose(E, np.pi * c[None] * np.ones((200, 1)), rtol=1.2e-3)
    np.testing.assert_allclose(E.mean(0), np.pi * c, rtol=5e-4)


def test_constant_map_prefilters_to_itself():
    c = np.array([0.25, 0.5, 4.0])
    env = np.ones((32, 64, 4), np.float32)
    env[..., :3] = c
    for k in range(1, ER.LEVELS):
        lv = ER.prefilter_level(env, k)
        np.testing.assert_allclose(lv, np.broadcast_to(c, lv.shape), rtol=1e-12)


def test_brdf_table_smallest_roughness_row_sums_to_one():
    """a near-mirror reflects everything: A + B = 1 wherever n.v >= 0.1 (Smith's term keeps it just below 1 at grazing angles)"""
    lut = ER.brdf_lut()
    nv = (np.arange(ER.LUT_N) + 0.5) / ER.LUT_N
    s = lut[0, :, 0] + lut[0, :, 1]
    assert np.all(np.abs(s[nv >= 0.1] - 1) < 1e-3), s
    assert np.all(s <= 1 + 1e-9)
    assert np.all(lut >= 0) and np.all(lut[..., 0] + lut[..., 1] <= 1 + 1e-9)


def test_mip_chain_sizes_and_mean():
    env = np.random.default_rng(2).random((33, 70, 4)).astype(np.float32)
    chain = ER.mip_chain(env)
    assert [m.shape[:2] for m in chain] == [(33, 70), (16, 35), (8, 17), (4, 8), (2, 4), (1, 2), (1, 1)]


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_envlit_kernels_are_clean(tmp_path):
    """the ISA of k_envlit / k_envlit_vis: tools/isa_lint.py finds no hazard, and neither kernel spills"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_lint
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "asm", f"OUT={tmp_path}"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    path = str(tmp_path / "shade-hip-amdgcn-amd-amdhsa-gfx950.s")
    rep = isa_lint.lint(path, match="k_envlit")
    assert rep.problems == [], "\n".join(rep.problems)
    assert rep.kernels >= 2
    name, scratch = None, {}
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            name = m.group(1)
        if name and line.startswith("; ScratchSize:"):
            scratch[name] = int(line.split(":")[1].split()[0])
    env = {k: v for k, v in scratch.items() if "k_envlit" in k}
    assert len(env) >= 2 and all(v == 0 for v in env.values()), env
