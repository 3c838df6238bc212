"""ARCTIC_OPT_ENV_LIGHTING without a GPU: the C-ABI declares and exports it, the float64 numpy reference the GPU tests
compare against gives the known answers of its own semantics, and the new shading kernels' ISA is clean."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import env_reference as ER
import env_shapes as ES

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


# ---- what the reference can see at the shapes of tests/test_gpu_env_shapes.py (tests/env_shapes.py) -----------------------------------
# A GPU comparison guards a kernel's rule only if breaking the rule moves the reference at the compared shape by much more than the
# comparison's tolerance.  Each test here breaks one rule in the reference and asks for 100 x the GPU test's tolerance.

def _ceil_mip_chain(env):
    """ER.mip_chain with the wrong halving rule: ceil, so an odd side keeps its last column / row (clamped 2x2 taps) where the true rule drops it"""
    out = [np.ascontiguousarray(env, np.float32)]
    while out[-1].shape[0] > 1 or out[-1].shape[1] > 1:
        s = out[-1]
        sh, sw = s.shape[:2]
        dh, dw = (sh + 1) >> 1, (sw + 1) >> 1
        ys0, ys1 = np.minimum(2 * np.arange(dh), sh - 1), np.minimum(2 * np.arange(dh) + 1, sh - 1)
        xs0, xs1 = np.minimum(2 * np.arange(dw), sw - 1), np.minimum(2 * np.arange(dw) + 1, sw - 1)
        a, b = s[ys0][:, xs0], s[ys0][:, xs1]
        c, d = s[ys1][:, xs0], s[ys1][:, xs1]
        out.append(((a + b) + (c + d)) * np.float32(0.25))
    return out


def _mip_rule_sensitivity(pkg, monkeypatch, name):
    """per level, the largest relative change of the compared texels (one in about 64 of them) when the mip rule is broken"""
    env = ES.make_map(pkg.scenes, name)
    W, H, _ = ES.MAPS[name]
    out = []
    for k in range(1, ER.LEVELS):
        w, h = ER.level_size(W, H, k)
        texels = ES.level_texels(name, k) or [(r, c) for r in range(h) for c in range(w)]
        texels = texels[::max(1, len(texels) // 64)]
        want = ER.prefilter_level(env, k, texels=texels)
        with monkeypatch.context() as mp:
            mp.setattr(ER, "mip_chain", _ceil_mip_chain)
            broken = ER.prefilter_level(env, k, texels=texels)
        out.append((np.abs(broken - want) / want).max())
    return out


@pytest.mark.parametrize("name", ["odd", "wide", "tall", "big"])
def test_reference_sees_the_mip_rule(pkg, monkeypatch, name):
    """every map with an odd-sided mip level above the levels' floor: a ceil-halving chain moves every prefiltered level by more than
    100 x the GPU test's rtol of 1e-4 (measured: 97 x 41 0.17-0.32, 300 x 20 0.12-0.49, 40 x 300 0.05-0.13, 1040 x 520 0.20-0.30; the
    64 x 32 map of the first prefilter test: exactly 0)"""
    sens = _mip_rule_sensitivity(pkg, monkeypatch, name)
    assert min(sens) > 100 * 1e-4, sens


def test_tiny_maps_do_not_guard_the_mip_rule(pkg, monkeypatch):
    """1 x 7 and 3 x 5 have odd sides too, but a texel of theirs is so large (omega_p = 4 pi / (W H)) that nearly every sample's lod is 0:
    the broken rule moves level 1 by 1e-2 at the most and levels 2 to 5 by nothing.  They are in the GPU tests for the one-texel wraps
    and the short chains, not for the mip rule: pinned here so that they are never taken for its guard."""
    for name in ("1x7", "3x5"):
        sens = _mip_rule_sensitivity(pkg, monkeypatch, name)
        assert max(sens[1:]) < 1e-4 and sens[0] < 2e-2, (name, sens)


def test_reference_sees_the_sh_trips(pkg):
    """k_env_sh_rows' second trip is columns >= 256, k_env_sh_final's is rows >= 256: without them the coefficients move by more than
    100 x the SH tolerance of 1e-6 max|want[0]| (measured: 300 x 20 columns 0.13, 40 x 300 rows 0.012, 1040 x 520 0.76 and 0.13)"""
    for name, cols, rows in (("wide", True, False), ("tall", False, True), ("big", True, True)):
        env = ES.make_map(pkg.scenes, name)
        want = ER.sh_project(env)
        for on, cut in ((cols, (slice(None), slice(256, None))), (rows, (slice(256, None), slice(None)))):
            if on:
                z = env.copy()
                z[cut] = 0
                assert np.abs(ER.sh_project(z) - want).max() > 100 * 1e-6 * np.abs(want[0]).max(), name


def test_prefilter_texel_subset_is_the_whole_level_there(pkg):
    env = pkg.scenes.synthetic_hdri(33, 17)
    whole = ER.prefilter_level(env, 1)
    assert whole.shape == (17, 33, 3)
    rng = np.random.default_rng(4)
    texels = [(0, 0), (16, 32), (16, 0), (7, 24)] + [(int(rng.integers(17)), int(rng.integers(33))) for _ in range(300)]   # more than one chunk of 256
    sub = ER.prefilter_level(env, 1, texels=texels)
    rc = np.array(texels)
    np.testing.assert_array_equal(sub, whole[rc[:, 0], rc[:, 1]])
    np.testing.assert_array_equal(ER.prefilter_level(env, 1, texels=texels[:1]), whole[0, 0][None])


def test_texel_subsets_are_fixed_and_hold_the_edges():
    for name, k in sorted(ES.SUBSET_LEVELS):
        W, H, _ = ES.MAPS[name]
        w, h = ER.level_size(W, H, k)
        t = ES.level_texels(name, k)
        if w * h <= ES.SUBSET_CAP:
            assert t is None
            continue
        assert t == ES.level_texels(name, k) and len(t) == len(set(t)) == ES.SUBSET_CAP
        rc = np.array(t)
        assert rc.min() >= 0 and rc[:, 0].max() == h - 1 and rc[:, 1].max() == w - 1
        assert {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)} <= set(t)
        assert (rc[:, 0] == h - 1).sum() >= min(w, 128) and (rc[:, 1] == w - 1).sum() >= 64
        for col in (255, 256, 257):
            assert col >= w or (rc[:, 1] == col).sum() >= 64, (name, k, col)
    assert all(ES.level_texels(name, k) is None for name in ES.MAPS for k in range(1, ER.LEVELS) if (name, k) not in ES.SUBSET_LEVELS)


@pytest.mark.parametrize("size,rough,angles", [((128, 64), ES.ROUGH_EDGES, True), ((97, 41), ES.ROUGH_EDGES, True), ((2048, 1024), ES.ROUGH_LEVEL0, False)])
def test_crafted_gbuffer_reaches_the_wraps_and_clamps(size, rough, angles):
    """the input of the GPU lookup tests, from the reference's own arithmetic: among the pixels where level 0 weighs in (roughness < 0.2)
    at least 32 take the u seam's wrap and 32 the v wrap at each pole; a pixel one texel off would not (the fans' outer ends are there for
    the coarser levels); n.wo takes each listed value with every material; one tile has one material, the others mix them"""
    w0, h0 = size
    attrs, mat, mats, kind = ES.crafted_gbuffer(w0, h0, rough, angles=angles)
    assert attrs.shape == (64, 96, 18) and attrs.dtype == np.float32 and np.isfinite(attrs).all()
    assert min(ES.wrap_counts(attrs, mat, mats, kind, w0, h0)) >= 32
    n, wo, _, metal, r, cov = ES.pixel_inputs(attrs, mat, mats)
    assert cov[kind > 0].all() and not cov[kind == 0].all()
    fan = (kind == 1) | (kind == 2)
    assert np.sum(n * wo, -1)[fan].min() > 1 - 1e-12                       # n = wo: R = wo
    assert set(np.round(r[fan] * 255).astype(int)) == set(rough)             # every fan meets every roughness byte
    assert set(metal[fan]) == {0.0, 1.0}
    # the outer ends of the fans do not wrap at level 0: the fans cross the wrap, they do not sit inside it
    R = 2 * np.sum(n * wo, -1)[..., None] * n - wo
    x0, x1, _ = ER._wrap(ER.dir_uv(R)[0], w0)
    y0, y1, _ = ER._wrap(ER.dir_uv(R)[1], h0)
    assert ((kind == 1) & (x1 == x0 + 1)).sum() >= 32 and ((kind == 2) & (y1 == y0 + 1)).sum() >= 32
    assert len(set(mat[24:32, 40:48].ravel())) == 1 and (kind[24:32, 40:48] == 4).all()
    assert all(len(set(mat[y:y + 8, x:x + 8].ravel())) > 1 for y in range(0, 64, 8) for x in range(0, 96, 8) if (y, x) != (24, 40))
    if angles:
        c = np.sum(n * wo, -1)[kind == 3]
        m = mat[kind == 3]
        for want in ES.COSINES:
            hit = np.abs(c - want) < 1e-6
            assert set(m[hit]) == set(range(len(mats))), want
        assert np.abs(c[np.abs(c) < 1e-6]).max() < 1e-7                      # "0 to rounding": either sign may come out
        assert (np.round(r[kind == 3] * 255) == 255).any() and (c > 1 - 1e-6).any()   # the LUT's last cell: roughness 1, n.wo 1


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
