"""ARCTIC_OPT_TEXTURE_MIPS on the device: the chain bit for bit against tests/mip_reference.py, mode 0 untouched, a zero plane = mode 0,
trilinear sampling and the level-of-detail plane against binary64, the paths agreeing bit for bit, composition with the other lighting
features, and the one assertion that a chain that is built is also used."""
import json
import os

import numpy as np
import pytest

import env_reference as ER
import mip_reference as MR

pytestmark = pytest.mark.gpu
TOL = 1e-4   # the project's parity gate on float LDR (tools/fuzz_parity.py, README)
# The level-of-detail plane against the binary64 reference: the largest |delta lambda| measured over the scenes of
# test_lod_plane_matches_float64 (fronto-parallel quads, the oblique floor, config 2 and config 3 at test scale) is recorded in
# profiles/texture_mips_lod_error.json; the gate is twice that, rounded up to one digit (the scenes are seeded and one camera each).
LOD_TOL = 0.05    # measured maximum 2.09e-2 levels (config 2; config 3 1.2e-3, the oblique floor 8.6e-4, the quads 8.8e-5)
NO_MAT = 0xFFFFFFFF


def _images(rng, w, h):
    d = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    n = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    m = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return d, n, m


def _read_chain(r, material):
    out = [r.read_material_mip(material, 0)]
    for k in range(1, len(MR.level_sizes(out[0].shape[1], out[0].shape[0]))):
        out.append(r.read_material_mip(material, k))
    return out


def _mip_renderer(hip, sc, mips=1, **kw):
    r = hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights, **kw)
    r.set_option("texture_mips", mips)
    return sc.upload(r)


# ---- 3: the chain, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiling", [-1, 0, 1])
def test_chain_matches_reference_bit_for_bit(hip, tiling):
    rng = np.random.default_rng(5)
    r = hip.Renderer(16, 8, 0, 16)
    r.set_option("texture_mips", 1)
    r.set_option("texture_tiling", tiling)
    sizes = [(1, 1), (5, 3), (16, 16), (64, 8), (33, 17), (1, 7), (7, 1), (130, 67)]
    if tiling == -1:
        sizes.append((2048, 2048))   # the library's choice tiles this one: the reduction reads the tiled layout
    for i, (w, h) in enumerate(sizes):
        d, n, m = _images(rng, w, h)
        assert r.create_material(d, n, m) == i
        want = MR.chain(MR.pack(d, n, m))
        assert [lv.shape[:2][::-1] for lv in want] == MR.level_sizes(w, h)
        for k, lv in enumerate(want):
            got = r.read_material_mip(i, k)
            assert got.shape == lv.shape, (w, h, k)
            np.testing.assert_array_equal(got, lv, err_msg=f"{w}x{h} level {k}")
        with pytest.raises(hip.ArcticError):
            r.read_material_mip(i, len(want))
    r.close()


# ---- 4: mode 0 untouched ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,scale", [(1, 0.5), (2, 0.25), (3, 0.1)])
def test_mode0_untouched_by_chains(pkg, hip, cfg, scale):
    sc = pkg.scenes.CONFIGS[cfg](scale=scale)
    a = _mip_renderer(hip, sc, 1)          # chains built ...
    a.set_option("texture_mips", 0)        # ... option 0 at shading time
    b = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))   # never heard of the option
    outs = []
    for r in (a, b):
        r.set_option("keep_float_output", 1)
        img = r.render_frame(sc.desc, sc.settings)
        ldr, hdr, rgba = r.read_output()
        attrs, mat, depth, tri = r.read_gbuffer()
        r.pass_shade(sc.desc, sc.settings)
        ldr2, _, rgba2 = r.read_output()
        outs.append((img, ldr, hdr, rgba, attrs, mat, depth, tri, ldr2, rgba2))
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)
    a.close(); b.close()


# ---- 5: a plane of zeroes = mode 0 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [0, 1])
def test_zero_plane_renders_mode0_bits(pkg, hip, sampler):
    sc = pkg.scenes.config3(scale=0.1)
    r = _mip_renderer(hip, sc, 1)
    r.set_option("keep_float_output", 1)
    r.set_option("sampler", sampler)
    r.pass_shadow_map(sc.desc)
    r.pass_gbuffer(sc.desc)
    assert r.read_lod().max() > 0.0
    r.write_lod(np.zeros((sc.height, sc.width), np.float32))
    r.pass_shade(sc.desc, sc.settings)
    got = r.read_output()
    r.set_option("texture_mips", 0)
    r.pass_shade(sc.desc, sc.settings)
    want = r.read_output()
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
    r.close()


# ---- float64 shading of a G-buffer whose eight material channels are given per pixel -----------------------------------------------
def _shade64(pkg, oracle, sc, attrs, ch, lit, lights):
    """ps_main + post_process in float64 (forward.hlsl:126-235 as shade.hip documents it): ch = (..., 8) base rgb, normal rgb on the
    0..255 scale, roughness, metalness; lit = 1 - shadow per pixel"""
    a = attrs.astype(np.float64)
    base, rough, metal = ch[..., :3], ch[..., 6:7], ch[..., 7:8]
    ts = np.stack([ch[..., 3] * 2 / 255 - 1, -(ch[..., 4] * 2 / 255 - 1), ch[..., 5] * 2 / 255 - 1], -1)
    n = a[..., 2:5] * ts[..., :1] + a[..., 5:8] * ts[..., 1:2] + a[..., 8:11] * ts[..., 2:3]
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    world = a[..., 11:14]
    wo = np.asarray(sc.desc.camera["eye"], np.float64) - world
    wo /= np.linalg.norm(wo, axis=-1, keepdims=True)
    PI = 3.14159265
    F0 = 0.04 + (base - 0.04) * metal
    al = rough * rough
    a2 = al * al
    k = (rough + 1) ** 2 / 8
    ndwo = np.maximum((n * wo).sum(-1, keepdims=True), 0)

    def radiance(wi, Li):
        h = wo + wi
        h /= np.linalg.norm(h, axis=-1, keepdims=True)
        F = F0 + (1 - F0) * (1 - np.maximum((h * wo).sum(-1, keepdims=True), 0)) ** 5
        ndh = np.maximum((n * h).sum(-1, keepdims=True), 0)
        ndwi = np.maximum((n * wi).sum(-1, keepdims=True), 0)
        D = a2 / (PI * (ndh * ndh * (a2 - 1) + 1) ** 2)
        G = (ndwo / (ndwo * (1 - k) + k)) * (ndwi / (ndwi * (1 - k) + k))
        spec = D * G * F / (4 * ndwo * ndwi + 1e-4)
        return ((1 - F) * (1 - metal) * base / PI + spec) * Li * ndwi
    sun_dir = oracle.dir_from_rot(sc.desc.sun["rotation"]).astype(np.float64)
    Lo = radiance(np.broadcast_to(-sun_dir, world.shape), np.asarray(sc.desc.sun["color"], np.float64))
    for L in lights:
        d = np.asarray(L["position"], np.float64) - world
        d2 = (d * d).sum(-1, keepdims=True)
        Lo = Lo + radiance(d / np.sqrt(d2), np.asarray(L["color"], np.float64) / d2)
    color = Lo * lit[..., None] + float(sc.desc.ambient) * base
    tm, gamma, exposure = sc.settings
    return ER.tonemap(tm, color, gamma, exposure)


# ---- 6: trilinear against float64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", [0, 1])
def test_trilinear_matches_float64(pkg, oracle, hip, sampler):
    rng = np.random.default_rng(17)
    W, H = 96, 64
    sc = pkg.scenes.config2(scale=0.05)
    r = hip.Renderer(W, H, 0, 16)
    r.set_option("texture_mips", 1)
    r.set_option("keep_float_output", 1)
    r.set_option("sampler", sampler)
    d, n, m = pkg.scenes.make_material_textures(rng, 64)
    n[..., :3] = rng.integers(96, 160, n[..., :3].shape)   # a rough normal map: every texel its own direction
    r.create_material(d, n, m)
    levels = len(MR.level_sizes(64, 64))
    attrs, mat = pkg.scenes.random_gbuffer(rng, H, W, 1, coverage=0.95)
    attrs[..., 0] = np.linspace(-1.5, 2.5, W, dtype=np.float32)[None, :]   # the uv sweep the texture, wrap included
    attrs[..., 1] = np.linspace(-0.7, 1.9, H, dtype=np.float32)[:, None]
    lod = np.linspace(-1.0, levels + 0.5, W * H, dtype=np.float32).reshape(H, W)   # beyond both ends ...
    lod[:, ::7] = np.round(lod[:, ::7])                                            # ... exact integers ...
    lod[3, 5] = np.nan                                                             # ... and a NaN (counts as 0)
    r.write_gbuffer(attrs, mat)
    r.write_lod(lod)
    np.testing.assert_array_equal(r.read_lod()[mat != NO_MAT][:50], lod[mat != NO_MAT][:50])
    r.pass_shade(sc.desc, sc.settings)
    ldr, _, _ = r.read_output()
    chain = _read_chain(r, 0)
    ch = MR.trilinear(chain, attrs[..., 0], attrs[..., 1], lod, q8=bool(sampler))
    want = _shade64(pkg, oracle, sc, attrs, ch, np.ones((H, W)), [])
    cov = mat != NO_MAT
    err = np.abs(ldr.astype(np.float64) - want)[cov]
    print(f"trilinear, sampler {sampler}: max |ldr - float64| = {err.max():.3e}")
    assert err.max() <= TOL, err.max()
    # an integer lambda equals a plain bilinear lookup of that level exactly: the same pixels with the level alone as a one-level material
    k = 2
    r2 = hip.Renderer(W, H, 0, 16)
    r2.set_option("keep_float_output", 1)
    r2.set_option("sampler", sampler)
    lv = chain[k]
    img = lambda c3: np.concatenate([c3, np.full(c3.shape[:2] + (1,), 255, np.uint8)], -1)
    mr = np.zeros(lv.shape[:2] + (4,), np.uint8); mr[..., 1:3] = lv[..., 6:8]; mr[..., 3] = 255
    r2.create_material(img(lv[..., :3]), img(lv[..., 3:6]), mr)
    r2.write_gbuffer(attrs, mat)
    r2.pass_shade(sc.desc, sc.settings)
    plain, _, _ = r2.read_output()
    r.write_lod(np.full((H, W), float(k), np.float32))
    r.pass_shade(sc.desc, sc.settings)
    at_k, _, _ = r.read_output()
    np.testing.assert_array_equal(at_k, plain)
    r.close(); r2.close()


# ---- 7: the plane against float64 ------------------------------------------------------------------------------------------------------
def _lod_reference(pkg, sc, r, tri, mat, pv=None):
    """lambda per pixel in binary64 from the visibility's triangle ids, the scene's vertices and the camera: the finite-difference definition
    of include/arctic_hip.h on the triangle's projective interpolation (vertices snapped to 1/256 pixel as set-up snaps them).  pv: the matrix
    the prepass drew with, [col][row], where that is not the camera's (arctic_set_camera_jitter)"""
    pv = (pkg.renderer.frame_constants(sc.desc)[0] if pv is None else np.asarray(pv).reshape(4, 4)).astype(np.float64)      # [col][row]
    H, W = tri.shape
    lam = np.zeros((H, W)); rho2 = np.zeros((H, W)); uv00 = np.zeros((H, W, 2))
    first = 0
    for o in sc.desc.objects:
        v, idx, m = sc.meshes[int(o["mesh_idx"])]
        idx = np.asarray(idx).reshape(-1, 3)
        n_tri = len(idx)
        sel = (tri >= first) & (tri < first + n_tri) & (tri != NO_MAT)
        if sel.any():
            trs = np.asarray(o["trs"], np.float64).reshape(4, 4)          # [col][row]
            pos = np.concatenate([v["position"].astype(np.float64), np.ones((len(v), 1))], 1)
            clip = pos @ trs @ pv                                         # row vectors: (M_pv M_trs p)^T
            uv = v["tex_coords"].astype(np.float64)
            tw, th = sc.materials[m][0].shape[1], sc.materials[m][0].shape[0]
            levels = len(MR.level_sizes(tw, th))
            ys, xs = np.nonzero(sel)
            t_local = tri[ys, xs] - first
            for t in np.unique(t_local):
                p = t_local == t
                c3, uv3 = clip[idx[t]].copy(), uv[idx[t]]
                iw = 1.0 / c3[:, 3]
                sx = np.floor((c3[:, 0] * iw + 1) * (0.5 * W) * 256 + 0.5) / 256
                sy = np.floor((1 - c3[:, 1] * iw) * (0.5 * sc.height) * 256 + 0.5) / 256
                c3[:, 0] = (sx / (0.5 * W) - 1) * c3[:, 3]
                c3[:, 1] = (1 - sy / (0.5 * sc.height)) * c3[:, 3]
                x, y = xs[p], ys[p] + r.row_begin
                a = MR.perspective_uv(c3, uv3, x, y, W, sc.height)
                b = MR.perspective_uv(c3, uv3, x + 1, y, W, sc.height)
                c = MR.perspective_uv(c3, uv3, x, y + 1, W, sc.height)
                l, r2_ = MR.lod_from_uv(a, b, c, tw, th, levels)
                lam[ys[p], xs[p]] = l; rho2[ys[p], xs[p]] = r2_; uv00[ys[p], xs[p]] = a
        first += n_tri
    return lam, rho2, uv00


def _lod_error(pkg, sc, r, pv=None):
    r.pass_gbuffer(sc.desc)
    got = r.read_lod().astype(np.float64)
    attrs, mat, _, tri = r.read_gbuffer()
    want, rho2, uv00 = _lod_reference(pkg, sc, r, tri, mat, pv)
    cov = mat != NO_MAT
    assert np.all(got[~cov] == 0.0)
    # the reference sees the triangles the device drew: its uv00 is the G-buffer's (clipped triangles excepted: their ids are sub-triangles of the source)
    assert np.abs(uv00 - attrs[..., :2])[cov].max() < 1e-3, np.abs(uv00 - attrs[..., :2])[cov].max()
    err = np.abs(got - want)   # (both clamped to 0 where rho < 1 on both sides: equal)
    return err[cov].max(), got, want, cov


def _quad_scene(pkg, oracle, W, H, tex, ratio):
    """a screen-filling fronto-parallel quad with `ratio` texels per pixel along both axes"""
    rng = np.random.default_rng(3)
    eye, rot, fov = np.array([0.5, 1.0, 2.0]), (-10.0, 25.0), 45.0
    fwd = oracle.dir_from_rot(rot).astype(np.float64)
    right = np.cross(fwd, [0, 1, 0]); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    dist = 3.0
    px_per_world = H / (2 * dist * np.tan(np.deg2rad(fov) / 2))
    side = 2.0 * W / px_per_world                  # twice the visible width
    uv_scale = ratio * side * px_per_world / tex   # texels across the quad / texture side
    origin = eye + fwd * dist - right * side / 2 - up * side / 2
    mesh = pkg.scenes.quad(origin, right * side, up * side, 4, 4, (uv_scale, uv_scale))
    S = pkg.scenes
    desc = S.SceneDesc(camera=dict(eye=tuple(eye), rotation=rot, aspect=W / H, fov_y=fov, z_near_far=(0.1, 1000.0)), ambient=0.1,
                       sun=S.DEFAULT_SUN, objects=S.make_objects([(np.eye(4), 0)]))
    return S.SyntheticScene("quad", W, H, 0, 16, [S.make_material_textures(rng, tex)], [mesh + (0,)], desc, np.zeros(0, S.LIGHT_DTYPE), (0, 2.2, 1.0))


def test_lod_plane_matches_float64(pkg, oracle, hip):
    W, H = 192, 128
    worst = {}
    # known answers first: 4 texels per pixel -> lambda = 2 in the interior; 1 / 2 -> clamped to 0
    for ratio, expect in ((4.0, 2.0), (0.5, 0.0)):
        sc = _quad_scene(pkg, oracle, W, H, 256, ratio)
        r = _mip_renderer(hip, sc, 1)
        e, got, want, cov = _lod_error(pkg, sc, r)
        assert cov.all()
        assert np.abs(got - expect).max() <= LOD_TOL, (ratio, np.abs(got - expect).max())
        worst[f"quad_ratio_{ratio}"] = e
        r.close()
    # a floor seen obliquely: per column lambda does not decrease with distance (up the screen)
    S = pkg.scenes
    rng = np.random.default_rng(4)
    floor = S.quad((-40, 0, 40), (80, 0, 0), (0, 0, -80), 8, 8, (40.0, 40.0))
    desc = S.SceneDesc(camera=dict(eye=(0.0, 2.0, 0.0), rotation=(-20.0, 0.0), aspect=W / H, fov_y=45.0, z_near_far=(0.1, 1000.0)), ambient=0.1,
                       sun=S.DEFAULT_SUN, objects=S.make_objects([(np.eye(4), 0)]))
    sc = S.SyntheticScene("floor", W, H, 0, 16, [S.make_material_textures(rng, 256)], [floor + (0,)], desc, np.zeros(0, S.LIGHT_DTYPE), (0, 2.2, 1.0))
    r = _mip_renderer(hip, sc, 1)
    e, got, want, cov = _lod_error(pkg, sc, r)
    worst["oblique_floor"] = e
    assert cov.sum() > W * H // 4
    for x in range(W):
        col = got[:, x][cov[:, x]]                 # top of the screen (far) first
        assert np.all(np.diff(col) <= LOD_TOL), x
    assert got[cov].max() > got[cov].min() + 1.0
    r.close()
    for name, sc in (("config2", pkg.scenes.config2(scale=0.25)), ("config3", pkg.scenes.config3(scale=0.1))):
        r = _mip_renderer(hip, sc, 1)
        e, got, want, cov = _lod_error(pkg, sc, r)
        worst[name] = e
        r.close()
    print("lod plane, max |delta lambda| against binary64:", json.dumps({k: float(f"{v:.3e}") for k, v in worst.items()}))
    out = os.environ.get("ARCTIC_LOD_ERROR_JSON")
    if out:
        json.dump({"max_abs_delta_lambda": {k: float(v) for k, v in worst.items()}, "gate": LOD_TOL}, open(out, "w"), indent=1)
    assert max(worst.values()) <= LOD_TOL, worst


# ---- 8: the whole image with the device's own plane and chain ------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,scale", [(2, 0.25), (3, 0.1)])
def test_whole_image_matches_float64(pkg, oracle, hip, cfg, scale):
    sc = pkg.scenes.CONFIGS[cfg](scale=scale)
    r = _mip_renderer(hip, sc, 1)
    r.set_option("keep_float_output", 1)
    r.pass_shadow_map(sc.desc)
    r.pass_gbuffer(sc.desc)
    r.pass_shade(sc.desc, sc.settings)
    ldr, _, _ = r.read_output()
    lod = r.read_lod()
    attrs, mat, _, _ = r.read_gbuffer()
    cov = mat != NO_MAT
    ch = np.zeros(mat.shape + (8,))
    for m in np.unique(mat[cov]):
        p = mat == m
        ch[p] = MR.trilinear(_read_chain(r, int(m)), attrs[..., 0][p], attrs[..., 1][p], lod[p])
    smap = r.read_shadow_map()
    ls = attrs[..., 14:18]
    lit = np.ones(mat.shape)
    for y, x in zip(*np.nonzero(cov)):
        lit[y, x] = 1.0 - oracle.calculate_shadow(smap, ls[y, x])
    want = _shade64(pkg, oracle, sc, attrs, ch, lit, sc.lights)
    err = np.abs(ldr.astype(np.float64) - want)[cov]
    print(f"config {cfg}, mode 1: max |ldr - float64| = {err.max():.3e}")
    assert err.max() <= TOL, err.max()
    r.close()


# ---- 9: the paths agree bit for bit in mode 1 ----------------------------------------------------------------------------------------
def test_paths_agree_bit_for_bit(pkg, hip):
    sc = pkg.scenes.config3(scale=0.1)
    ref = None
    for tiling in (0, 1):
        r = hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights)
        r.set_option("texture_mips", 1)
        r.set_option("texture_tiling", tiling)
        sc.upload(r)
        r.set_option("visbuffer", 1)
        a = r.render_frame(sc.desc, sc.settings).copy()
        r.set_option("visbuffer", 0)
        b = r.render_frame(sc.desc, sc.settings).copy()
        np.testing.assert_array_equal(a, b)
        for path in (1, 2):   # scalar against packed light loop: equal within the float budget (the existing tests' bar), each path bit-stable
            r.set_option("light_path", path)
            r.set_option("visbuffer", 1)
            c = r.render_frame(sc.desc, sc.settings).copy()
            r.set_option("visbuffer", 0)
            np.testing.assert_array_equal(c, r.render_frame(sc.desc, sc.settings))
            assert np.abs(c.astype(int) - a.astype(int)).max() <= 1
        r.set_option("light_path", 0)
        if ref is None:
            ref = a
        np.testing.assert_array_equal(a, ref)   # tiled against row-major level 0
        r.close()
    # frames in flight over a moving camera
    import copy
    frames = {}
    for fif in (1, 2):
        r = _mip_renderer(hip, sc, 1)
        r.set_option("frames_in_flight", fif)
        out = []
        for k in range(4):
            d = copy.deepcopy(sc.desc)
            d.camera["rotation"] = (-15.0 + k, 3.0 * k)
            out.append(r.render_frame(d, sc.settings).copy())
        r.flush()
        frames[fif] = out
        r.close()
    for x, y in zip(frames[1], frames[2]):
        np.testing.assert_array_equal(x, y)
    # row-band shards against the whole frame
    for cuts in ([0, 37, sc.height], [0, 64, 128, sc.height]):
        parts = []
        for b, e in zip(cuts, cuts[1:]):
            r = _mip_renderer(hip, sc, 1, row_begin=b, row_end=e)
            parts.append(r.render_frame(sc.desc, sc.settings))
            r.close()
        np.testing.assert_array_equal(np.concatenate(parts, 0), ref)


# ---- 10: composition ---------------------------------------------------------------------------------------------------------------
def test_composes_with_env_spot_and_point_shadows(pkg, hip):
    sc = pkg.scenes.config3(scale=0.1)
    sc.environment = pkg.scenes.synthetic_hdri(64, 32)
    r = _mip_renderer(hip, sc, 1)
    r.set_option("keep_float_output", 1)
    r.set_option("env_lighting", 1)
    r.set_option("point_shadow_size", 64)
    r.update_spot_lights(pkg.scenes.spot_lights(1))
    r.update_point_shadow_lights(pkg.scenes.point_shadow_lights(1))
    r.pass_shadow_map(sc.desc)
    r.pass_point_shadows(sc.desc)
    r.pass_gbuffer(sc.desc)
    r.pass_shade(sc.desc, sc.settings)
    mode1 = r.read_output()
    r.write_lod(np.zeros((sc.height, sc.width), np.float32))
    r.pass_shade(sc.desc, sc.settings)
    zero = r.read_output()
    r.set_option("texture_mips", 0)
    r.pass_shade(sc.desc, sc.settings)
    mode0 = r.read_output()
    for x, y in zip(zero, mode0):
        np.testing.assert_array_equal(x, y)
    assert np.abs(mode1[0] - mode0[0]).max() > 1e-3   # ... and the plane does something
    r.close()


# ---- 11: it does what it is for ----------------------------------------------------------------------------------------------------
def test_minified_checkerboard_is_filtered(pkg, oracle, hip):
    W, H, T = 256, 256, 2048
    ratio = 7.3   # about 8x, and not an integer: at a whole ratio every pixel meets the checkerboard at the same phase
    sc = _quad_scene(pkg, oracle, W, H, T, ratio)
    yy, xx = np.mgrid[0:T, 0:T]
    d = np.zeros((T, T, 4), np.uint8); d[..., :3] = (((xx + yy) & 1) * 255)[..., None]; d[..., 3] = 255
    n = np.zeros((T, T, 4), np.uint8); n[..., :3] = (128, 128, 255); n[..., 3] = 255
    m = np.zeros((T, T, 4), np.uint8); m[..., 1] = 200; m[..., 3] = 255
    sc.materials = [(d, n, m)]
    sc.desc.ambient = 1.0
    sc.desc.sun = dict(position=(0.0, 10.0, 0.0), rotation=(-70.0, 12.0), color=(0.0, 0.0, 0.0))   # colour = base
    r = _mip_renderer(hip, sc, 1)
    r.set_option("keep_float_output", 1)
    r.pass_gbuffer(sc.desc)
    lod = r.read_lod()
    inner = (slice(16, H - 16), slice(16, W - 16))
    assert np.abs(lod[inner] - np.log2(ratio)).max() <= LOD_TOL
    r.pass_shade(sc.desc, sc.settings)
    _, hdr1, _ = r.read_output()
    r.set_option("texture_mips", 0)
    r.pass_shade(sc.desc, sc.settings)
    _, hdr0, _ = r.read_output()
    assert hdr0[inner][..., 0].std() > 0.05          # mode 0: the base colour varies from pixel to pixel
    table = MR.srgb_table().astype(np.float64)
    lo_hi = []
    for k in (int(np.floor(lod[inner].min())), int(np.floor(lod[inner].max())) + 1):
        lv = table[r.read_material_mip(0, k)[..., :3]]
        lo_hi += [lv.min(), lv.max()]
    assert min(lo_hi) - 1e-6 <= hdr1[inner].min() and hdr1[inner].max() <= max(lo_hi) + 1e-6, (hdr1[inner].min(), hdr1[inner].max(), lo_hi)
    assert max(lo_hi) - min(lo_hi) < 0.1             # ... and those levels are grey: the checkerboard is gone
    r.close()


# ---- 12: errors --------------------------------------------------------------------------------------------------------------------
def test_errors(pkg, hip):
    sc = pkg.scenes.config3(scale=0.05)
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.pass_gbuffer(sc.desc)
    for call in (r.read_lod, lambda: r.write_lod(np.zeros((sc.height, sc.width), np.float32))):
        with pytest.raises(hip.ArcticError) as e:
            call()
        assert e.value.code == -4       # ARCTIC_E_STATE: the option is off
    with pytest.raises(hip.ArcticError) as e:
        r.read_material_mip(0, 1)       # a material created under 0 has one level
    assert e.value.code == -1
    r.read_material_mip(0, 0)
    with pytest.raises(hip.ArcticError) as e:
        r.set_option("texture_mips", 2)
    assert e.value.code == -1
    r.set_option("texture_mips", 1)
    # an over-size chain: level 0 fits (below 2^29 texels), the chain does not fit in 2^32 bytes; nothing is read before the check
    big = np.zeros((6300, 65535, 4), np.uint8)
    with pytest.raises(hip.ArcticError) as e:
        r.create_material(big, big, big)
    assert e.value.code == -5           # ARCTIC_E_CAPACITY
    del big
    rng = np.random.default_rng(1)
    i = r.create_material(*_images(rng, 8, 8))            # the handle is still usable
    assert len(_read_chain(r, i)) == 4
    r.pass_gbuffer(sc.desc)
    r.pass_shade(sc.desc, sc.settings)
    for opt in ("count_light_evals", "tile_trace"):
        r.set_option(opt, 1)
        with pytest.raises(hip.ArcticError) as e:
            r.pass_shade(sc.desc, sc.settings)
        assert e.value.code == -4
        r.set_option(opt, 0)
    r.pass_shade(sc.desc, sc.settings)
    r.close()
