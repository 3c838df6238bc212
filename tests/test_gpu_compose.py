"""arctic_compose_planes_device, arctic_pass_ray_effects and arctic_read_composed on the device (needs an MI355X): k_compose on injected planes
against the float64 composition of tests/compose_reference.py at the project's two standing bars (HDR_REL and TOL of
tests/test_gpu_extended_shading.py, taken over unchanged) with RGBA8 within one step of the reference's quantisation and NO pixel left out; the
one call against the three public calls made by hand, byte for byte; the identities; pixels without geometry and degenerate normals; a ragged
frame; shards; the three texture layouts; the refusals, which write nothing; the G-buffer resolved on demand after a whole frame; and that a
handle which never makes these calls is what it was.

Frames of 96 x 64 on ao_scenes.raster_scene with the handle of tests/test_gpu_reflections.py -- 5 lights, a 64 x 32 environment map, a 64^2 sun
map -- but with a material of noise images (32 x 16; roughness bytes 13..255, every metalness): the fallback material of that file has roughness
1, under which the reflection's gate (1 - rough)^2 is zero everywhere.  The frame is shaded from the G-buffer as rasterised; THEN the degenerate
normals and the pixels without geometry are written over it (arctic_write_gbuffer), so the HDR plane is finite everywhere and every pixel is judged.

The occlusion strength of the float64 cases is 0.8, not 1: at 1 a shadowed pixel with ao = 0 composes to ambient * base - ambient * base, a zero
with an fp32 residue of 1e-9, and the gamma curve's slope at zero is unbounded -- the float LDR of such a pixel is ill-conditioned in any
precision of the inputs.  At 0.8 the composed colour keeps a fifth of the ambient term and nothing is left out."""
import numpy as np
import pytest

import ao_scenes as AS
import compose_reference as CR
import hit_reference as HR
import ray_scenes as S
import test_gpu_extended_shading as G
import test_gpu_reflections as TR

pytestmark = pytest.mark.gpu
F = np.float32
WIDTH, HEIGHT = TR.WIDTH, TR.HEIGHT
BIAS = TR.BIAS
SETTINGS = (0, 2.2, 1.0)
SHARDS = TR.SHARDS
INVALID, STATE = -1, -4
AO_KW = dict(n_rays=4, pattern=2, radius=0.75, bias=1e-3)


def images(kind="packed"):
    rng = np.random.default_rng(4100)
    if kind == "plain":                                                          # images of unequal sizes: the plain layout
        d, _, _ = G._random_images(rng, 16, 16)
        _, n, _ = G._random_images(rng, 8, 8)
        _, _, m = G._random_images(rng, 4, 4)
        return G._well_conditioned((d, n, m))
    return G._well_conditioned(G._random_images(rng, 32, 16))


def handle(pkg, hip, imgs=None, tiling=None, width=WIDTH, height=HEIGHT, keep_float=True, **kw):
    """test_gpu_reflections.handle with a material of its own (imgs None: that file's handle as it is)"""
    if imgs is None:
        r = TR.handle(pkg, hip, **kw)
    else:
        r = hip.Renderer(width, height, 64, 16, **kw)
        if tiling is not None:
            r.set_option("texture_tiling", tiling)                               # before the material is created
        r.create_material(*imgs)
        for v, i in AS.raster_scene(pkg).meshes:
            r.create_mesh(v, i, 0)
        r.update_lights(pkg.scenes.random_lights(np.random.default_rng(64), 5, (-3, 0.5, -3), (3, 3, 3), intensity=6.0))
        r.create_hdri(pkg.scenes.synthetic_hdri(64, 32))
    if keep_float:
        r.set_option("keep_float_output", 1)
    return r


def scene(pkg, width=WIDTH, height=HEIGHT):
    sc = AS.raster_scene(pkg)
    return pkg.scenes.SceneDesc(camera=dict(sc.desc.camera, aspect=width / height), ambient=0.1, sun=sc.desc.sun, objects=sc.desc.objects)


def planes(rows, width, seed):
    """the byte plane: random, with 0 and 255; the float plane: random colours, a in {0, 0.5, 1}, NaN colours where a == 0"""
    rng = np.random.default_rng(seed)
    ao = rng.integers(0, 256, (rows, width)).astype(np.uint8)
    ao[rng.uniform(size=ao.shape) < 0.1] = 0
    ao[rng.uniform(size=ao.shape) < 0.1] = 255
    refl = np.concatenate([rng.uniform(0, 3, (rows, width, 3)), rng.choice([0.0, 0.5, 1.0], (rows, width, 1))], -1).astype(F)
    refl[refl[..., 3] == 0, :3] = np.nan
    return ao, refl


def inject(attrs, mat, seed=65):
    """degenerate normals over some covered pixels, normals turned away from the eye, and pixels without geometry (test_gpu_reflections' kinds)"""
    attrs, mat = attrs.copy(), mat.copy()
    rng = np.random.default_rng(seed)
    cov = np.nonzero((mat != HR.NO_MATERIAL).reshape(-1))[0]
    px = rng.choice(cov, 40 + 60, replace=False)
    flat = attrs.reshape(-1, 18)
    for k, n in enumerate([(0, 0, 0), (np.nan, 0, 1), (3e19, 3e19, 3e19), (1e-30, 1e-30, 0)]):
        flat[px[10 * k:10 * k + 10], 8:11] = np.array(n, F)
    flat[rng.choice(cov, 200, replace=False), 8:11] *= F(-1.0)
    mat.reshape(-1)[px[40:]] = HR.NO_MATERIAL
    return attrs, mat, px[:40], px[40:]


def device(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return out


def shaded(pkg, hip, imgs, desc, tiling=None, width=WIDTH, height=HEIGHT):
    """a handle with the frame shaded from its rasterised G-buffer -> (handle, attrs, mat, hdr)"""
    r = handle(pkg, hip, imgs, tiling=tiling, width=width, height=height)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    r.pass_shade(desc, SETTINGS)
    attrs, mat, _, _ = r.read_gbuffer(want=("attrs", "material"))
    _, hdr, _ = r.read_output(want=("hdr",))
    return r, attrs, mat, hdr


def judge(name, got, want):
    """composed HDR at HDR_REL, float LDR at TOL, RGBA8 within one step of the reference's quantisation: every pixel"""
    ldr, hdr, rgba8 = got
    assert np.isfinite(want["hdr"]).all() and np.isfinite(want["ldr"]).all()
    rel = CR.rel_err(hdr, want["hdr"]).max()
    err = np.abs(ldr.astype(np.float64) - want["ldr"]).max()
    step = np.abs(rgba8.astype(np.int32) - want["rgba8"].astype(np.int32)).max()
    print(f"{name}: hdr relative {rel:.3e}, ldr {err:.3e}, rgba8 steps {step}, exact rgba8 {(rgba8 == want['rgba8']).all(-1).mean():.4f}")
    assert rel <= G.HDR_REL, (name, float(rel))
    assert err <= G.TOL, (name, float(err))
    assert step <= 1 and (rgba8[..., 3] == 255).all(), (name, int(step))


@pytest.fixture(scope="module")
def whole(pkg, hip):
    desc = scene(pkg)
    imgs = images()
    r, clean_attrs, clean_mat, hdr = shaded(pkg, hip, imgs, desc)
    attrs, mat, degenerate, removed = inject(clean_attrs, clean_mat)
    r.write_gbuffer(attrs, mat)
    ao, refl = planes(HEIGHT, WIDTH, 66)
    yield dict(desc=desc, r=r, imgs=imgs, materials=G.host_materials([imgs], False), clean=(clean_attrs, clean_mat), attrs=attrs, mat=mat, hdr=hdr, ao=ao, refl=refl,
               degenerate=degenerate, removed=removed, eye=desc.camera["eye"])
    r.close()


def reference(w, settings=SETTINGS, ao=None, refl=None, attrs=None, mat=None, hdr=None, materials=None, **kw):
    return CR.compose_gbuffer(w["materials"] if materials is None else materials, w["attrs"] if attrs is None else attrs, w["mat"] if mat is None else mat,
                              w["hdr"] if hdr is None else hdr, w["eye"], w["desc"].ambient, settings, ao=ao, refl=refl, **kw)


@pytest.mark.parametrize("flags", ["ao", "reflections", "both"])
def test_injected_planes_against_float64(pkg, hip, whole, flags):
    w, r = whole, whole["r"]
    d_ao, d_refl = device(w["ao"], w["refl"])
    ao, refl = (w["ao"] if flags != "reflections" else None), (w["refl"] if flags != "ao" else None)
    kw = dict(ao_strength=0.8, reflection_strength=1.3)
    for settings in (SETTINGS, (1, 2.2, 0.7), (2, 2.4, 1.0)):                    # Reinhard, exposure, ACES: the HDR plane is the same, the tonemapper differs
        r.compose_planes_device(w["desc"], settings, d_ao.data_ptr() if ao is not None else None, d_refl.data_ptr() if refl is not None else None, **kw)
        judge(f"{flags}, tonemapper {settings[0]}", r.read_composed(), reference(w, settings, ao=ao, refl=refl, **kw))
    # not vacuous: both terms move pixels by far more than the bar, and the frame holds every class
    _, hdr, _ = r.read_composed()
    moved = (CR.rel_err(hdr, w["hdr"].astype(np.float64)).max(-1) > 100 * G.HDR_REL).reshape(-1)
    cov = (w["mat"] != HR.NO_MATERIAL).reshape(-1)
    assert cov.sum() >= 3000 and moved[cov].mean() >= (0.6 if flags != "reflections" else 0.25), float(moved[cov].mean())
    assert (w["ao"] == 0).sum() >= 300 and (w["ao"] == 255).sum() >= 300 and np.isnan(w["refl"][w["refl"][..., 3] == 0, :3]).all()
    assert sorted(np.unique(w["refl"][..., 3]).tolist()) == [0.0, 0.5, 1.0]


def test_pixels_without_geometry_and_degenerate_normals_come_through(pkg, hip, whole):
    w, r = whole, whole["r"]
    d_ao, d_refl = device(w["ao"], np.where(np.isnan(w["refl"]), F(1.5), w["refl"]) * np.array([1, 1, 1, 0], F) + np.array([0, 0, 0, 1], F))   # a = 1 everywhere
    hdr_in = w["hdr"].reshape(-1, 3)
    r.compose_planes_device(w["desc"], SETTINGS, None, d_refl.data_ptr(), reflection_strength=2.0)
    _, hdr, _ = r.read_composed()
    out = hdr.reshape(-1, 3)
    assert out[w["removed"]].tobytes() == hdr_in[w["removed"]].tobytes()         # no geometry: C = hdr
    assert out[w["degenerate"]].tobytes() == hdr_in[w["degenerate"]].tobytes()   # NOT COVERED by step 1: no reflection, whatever refl.a says
    _, covered = HR.unit_normal(w["attrs"].reshape(-1, 18)[:, 8:11])
    has = covered & (w["mat"] != HR.NO_MATERIAL).reshape(-1)
    assert (out[has] != hdr_in[has]).any(1).mean() >= 0.8                        # everybody else has one
    sky = (w["clean"][1] == HR.NO_MATERIAL).reshape(-1)
    assert sky.sum() >= 100 and out[sky].tobytes() == hdr_in[sky].tobytes()
    r.compose_planes_device(w["desc"], SETTINGS, d_ao.data_ptr(), None, ao_strength=1.0)
    _, hdr, _ = r.read_composed()
    gone = np.concatenate([w["removed"], np.nonzero(sky)[0]])
    assert hdr.reshape(-1, 3)[gone].tobytes() == hdr_in[gone].tobytes()
    # NaN colours behind a == 0 and NaN normals stay out of the picture
    r.compose_planes_device(w["desc"], SETTINGS, d_ao.data_ptr(), device(w["refl"])[0].data_ptr(), ao_strength=0.8)
    ldr, hdr, _ = r.read_composed()
    assert np.isfinite(hdr).all() and np.isfinite(ldr).all()


def test_identities(pkg, hip, whole):
    """a plane of 255s and a plane of zeros: the composed HDR is read_output's HDR by bytes, and the tonemapper gives the frame's own RGBA8"""
    w, r = whole, whole["r"]
    d_ao, d_refl = device(np.full((HEIGHT, WIDTH), 255, np.uint8), np.zeros((HEIGHT, WIDTH, 4), F))
    r.compose_planes_device(w["desc"], SETTINGS, d_ao.data_ptr(), d_refl.data_ptr(), ao_strength=1.0, reflection_strength=3.0)
    ldr, hdr, rgba8 = r.read_composed()
    assert hdr.tobytes() == w["hdr"].tobytes()
    d_ao, d_refl = device(w["ao"], w["refl"])
    r.compose_planes_device(w["desc"], SETTINGS, d_ao.data_ptr(), d_refl.data_ptr(), ao_strength=0.0, reflection_strength=0.0)
    assert r.read_composed()[1].tobytes() == w["hdr"].tobytes()
    frame_ldr, frame_hdr, frame_rgba8 = r.read_output()
    assert frame_hdr.tobytes() == w["hdr"].tobytes()                             # the shading pass's own planes are not touched
    assert np.abs(ldr.astype(np.float64) - frame_ldr).max() <= G.TOL and np.abs(rgba8.astype(np.int32) - frame_rgba8).max() <= 1


@pytest.mark.parametrize("flags", ["ao", "reflections", "both, filtered"])
def test_the_one_call_equals_the_three_by_hand(pkg, hip, whole, flags):
    import torch
    w, r, desc = whole, whole["r"], whole["desc"]
    dirs = pkg.renderer.ao_directions(4, 2, seed=3)
    ao_kw = dict(AO_KW, filter=flags.endswith("filtered"))
    with_ao, with_refl = flags != "reflections", flags != "ao"
    d_ao = torch.full((HEIGHT, WIDTH), 77, dtype=torch.uint8, device="cuda")
    d_refl = torch.full((HEIGHT, WIDTH, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    if with_ao:
        r.trace_ambient_occlusion_device(desc, dirs, d_ao.data_ptr(), **ao_kw)
    if with_refl:
        r.trace_reflections_device(desc, BIAS, d_refl.data_ptr())
    kw = dict(ao_strength=0.9, reflection_strength=1.2)
    r.compose_planes_device(desc, SETTINGS, d_ao.data_ptr() if with_ao else None, d_refl.data_ptr() if with_refl else None, **kw)
    by_hand = r.read_composed()
    got_rgba8 = r.pass_ray_effects(desc, SETTINGS, dirs=dirs if with_ao else None, reflection_bias=BIAS if with_refl else None, **kw, **(ao_kw if with_ao else {}))
    one = r.read_composed()
    for a, b in zip(one, by_hand):
        assert a.tobytes() == b.tobytes(), (flags, int((a != b).sum()))
    assert got_rgba8.tobytes() == by_hand[2].tobytes() and got_rgba8.shape == (HEIGHT, WIDTH, 4)
    # ... which is the float64 composition of the traced planes, and not the frame as it was
    judge("the one call, " + flags, one, reference(w, ao=d_ao.cpu().numpy() if with_ao else None, refl=d_refl.cpu().numpy() if with_refl else None, **kw))
    assert (one[2] != r.read_output(want=("rgba8",))[2]).any(-1).mean() >= 0.05
    # into the caller's buffer: the same bytes, nothing beyond them
    out = torch.full((HEIGHT * WIDTH + 16, 4), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert r.pass_ray_effects(desc, SETTINGS, dirs=dirs if with_ao else None, reflection_bias=BIAS if with_refl else None, d_out_ptr=out.data_ptr(), **kw,
                              **(ao_kw if with_ao else {})) is None
    r.flush()
    host = out.cpu().numpy()
    assert host[:HEIGHT * WIDTH].tobytes() == by_hand[2].tobytes() and (host[HEIGHT * WIDTH:] == 0x5A).all()
    with pytest.raises(hip.ArcticError) as e:                                    # the handle's own RGBA8 is not the latest composition's
        r.read_composed(want=("rgba8",))
    assert e.value.code == STATE
    assert r.read_composed(want=("hdr",))[1].tobytes() == by_hand[1].tobytes()


def test_ragged_frame(pkg, hip):
    width, height = 61, 37
    desc = scene(pkg, width, height)
    imgs = images()
    r, attrs, mat, hdr = shaded(pkg, hip, imgs, desc, width=width, height=height)
    ao, refl = planes(height, width, 67)
    d_ao, d_refl = device(ao, refl)
    import torch
    out = torch.full((height * width + 16, 4), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    kw = dict(ao_strength=0.8, reflection_strength=1.3)
    r.compose_planes_device(desc, SETTINGS, d_ao.data_ptr(), d_refl.data_ptr(), d_out_ptr=out.data_ptr(), **kw)
    r.compose_planes_device(desc, SETTINGS, d_ao.data_ptr(), d_refl.data_ptr(), **kw)
    got = r.read_composed()
    assert got[2].shape == (height, width, 4)
    w = dict(materials=G.host_materials([imgs], False), attrs=attrs, mat=mat, hdr=hdr, eye=desc.camera["eye"], desc=desc)
    judge("61 x 37", got, reference(w, ao=ao, refl=refl, **kw))
    host = out.cpu().numpy()
    assert host[:height * width].tobytes() == got[2].tobytes() and (host[height * width:] == 0x5A).all()   # nothing written past the last pixel
    assert (mat != HR.NO_MATERIAL).sum() >= 1000
    r.close()


@pytest.mark.parametrize("sharding", list(SHARDS))
def test_shards_compose_their_rows_of_the_frame(pkg, hip, whole, sharding):
    w, desc = whole, whole["desc"]
    dirs = pkg.renderer.ao_directions(4, 2, seed=3)
    kw = dict(ao_strength=0.9, reflection_strength=1.2, **AO_KW)
    w["r"].pass_ray_effects(desc, SETTINGS, dirs=dirs, reflection_bias=BIAS, **kw)
    want = w["r"].read_composed()
    seen = []
    for shard in SHARDS[sharding]:
        r = handle(pkg, hip, w["imgs"], **shard)
        rows = S.owned(pkg, HEIGHT, shard)
        r.pass_shadow_map(desc)
        r.write_gbuffer(w["clean"][0][rows], w["clean"][1][rows])
        r.pass_shade(desc, SETTINGS)
        assert r.read_output(want=("hdr",))[1].tobytes() == w["hdr"][rows].tobytes()             # the precondition, from existing code only
        r.write_gbuffer(w["attrs"][rows], w["mat"][rows])
        r.pass_ray_effects(desc, SETTINGS, dirs=dirs, reflection_bias=BIAS, **kw)
        got = r.read_composed()
        for a, b in zip(got, want):
            assert a.shape[0] == len(rows) and a.tobytes() == b[rows].tobytes(), (sharding, shard)
        with pytest.raises(hip.ArcticError) as e:                                                # the occlusion's filter on a shard: refused as ever
            r.pass_ray_effects(desc, SETTINGS, dirs=dirs, reflection_bias=BIAS, filter=True, **kw)
        assert e.value.code == STATE and r.read_composed()[1].tobytes() == got[1].tobytes()
        seen.append(rows)
        r.close()
    assert 0 < len(np.concatenate(seen)) <= HEIGHT


def test_the_three_texture_layouts(pkg, hip, whole):
    """packed images row-major and in 4 x 4 tiles: the same bytes; plain images (unequal sizes): within the bars"""
    w, desc = whole, whole["desc"]
    d_ao, d_refl = device(w["ao"], w["refl"])
    kw = dict(ao_strength=0.8, reflection_strength=1.3)
    got = {}
    for name, imgs, tiling in (("row-major", w["imgs"], 0), ("tiled", w["imgs"], 1), ("plain", images("plain"), None)):
        r, attrs, mat, hdr = shaded(pkg, hip, imgs, desc, tiling=tiling)
        assert attrs.tobytes() == w["clean"][0].tobytes()
        r.write_gbuffer(w["attrs"], w["mat"])
        r.compose_planes_device(desc, SETTINGS, d_ao.data_ptr(), d_refl.data_ptr(), **kw)
        got[name] = (r.read_composed(), hdr)
        if name != "tiled":
            judge(name, got[name][0], reference(w, ao=w["ao"], refl=w["refl"], hdr=hdr, materials=G.host_materials([imgs], False), **kw))
        r.close()
    assert got["tiled"][1].tobytes() == got["row-major"][1].tobytes()                            # the precondition, from existing code only
    for a, b in zip(got["tiled"][0], got["row-major"][0]):
        assert a.tobytes() == b.tobytes()
    assert (got["plain"][0][2] != got["row-major"][0][2]).any(-1).mean() >= 0.3                  # other images: another picture


def test_refusals_write_nothing(pkg, hip, whole):
    import torch
    w, desc = whole, whole["desc"]
    d_ao, d_refl = device(w["ao"], w["refl"])
    out = torch.full((HEIGHT * WIDTH, 4), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dirs = pkg.renderer.ao_directions(4, 2, seed=3)
    r = handle(pkg, hip, w["imgs"])

    def refused(code, call):
        with pytest.raises(hip.ArcticError) as e:
            call()
        assert e.value.code == code, e.value
    both = lambda **kw: r.compose_planes_device(desc, SETTINGS, d_ao.data_ptr(), d_refl.data_ptr(), d_out_ptr=out.data_ptr(), **kw)
    only_ao = lambda: r.compose_planes_device(desc, SETTINGS, d_ao.data_ptr(), None, d_out_ptr=out.data_ptr())
    only_refl = lambda: r.compose_planes_device(desc, SETTINGS, None, d_refl.data_ptr(), d_out_ptr=out.data_ptr())
    one_call = lambda **kw: r.pass_ray_effects(desc, SETTINGS, dirs=dirs, reflection_bias=BIAS, d_out_ptr=out.data_ptr(), **dict(AO_KW, **kw))
    r.pass_shadow_map(desc)
    refused(STATE, both)                                                         # no G-buffer
    refused(STATE, one_call)
    r.write_gbuffer(*w["clean"])                                                 # (the fixture's order: shaded as rasterised, the injected pixels behind it)
    refused(STATE, both)                                                         # no HDR plane: nothing shaded yet
    r.set_option("keep_float_output", 0)
    r.pass_shade(desc, SETTINGS)
    refused(STATE, both)                                                         # float output off
    r.set_option("keep_float_output", 1)
    refused(STATE, both)                                                         # ... and on again, but nothing shaded since
    refused(STATE, one_call)
    r.pass_shade(desc, SETTINGS)
    r.set_option("hdr16", 1)
    refused(STATE, both)
    refused(STATE, only_refl)
    r.set_option("hdr16", 0)
    # what changes the ambient term is refused with the occlusion flag
    for on, off in ((lambda: r.set_option("env_lighting", 1), lambda: r.set_option("env_lighting", 0)),
                    (lambda: r.set_option("texture_mips", 1), lambda: r.set_option("texture_mips", 0))):
        on()
        refused(STATE, both)
        refused(STATE, only_ao)
        refused(STATE, one_call)
        off()
    params = pkg.scene.neutral_material_params(1)
    params["base_color_factor"] = (0.5, 0.25, 0.75)
    r.set_material_extras(0, params)
    refused(STATE, only_ao)
    refused(STATE, both)
    r.set_material_extras(0)
    # the block, the planes, the other calls' own refusals
    for kw in (dict(flags=0), dict(flags=4), dict(flags=7), dict(ao_strength=-0.1), dict(ao_strength=1.5), dict(ao_strength=np.nan), dict(reflection_strength=-1.0),
               dict(reflection_strength=np.inf), dict(reflection_strength=np.nan)):
        refused(INVALID, lambda: both(**kw))
    refused(INVALID, lambda: r.compose_planes_device(desc, SETTINGS, None, d_refl.data_ptr(), flags=3, d_out_ptr=out.data_ptr()))
    refused(INVALID, lambda: r.compose_planes_device(desc, SETTINGS, d_ao.data_ptr(), None, flags=3, d_out_ptr=out.data_ptr()))
    refused(INVALID, lambda: r.compose_planes_device(desc, SETTINGS, d_ao.data_ptr(), d_refl.data_ptr() + 8, d_out_ptr=out.data_ptr()))
    refused(INVALID, lambda: one_call(n_rays=65))
    refused(INVALID, lambda: one_call(radius=-1.0))
    refused(INVALID, lambda: r.pass_ray_effects(desc, SETTINGS, dirs=dirs, reflection_bias=np.nan, d_out_ptr=out.data_ptr(), **AO_KW))
    r.set_option("shadow_sharded", 1)
    refused(STATE, one_call)                                                     # the sun map's states of the hit shading
    r.set_option("shadow_sharded", 0)
    c = np.zeros(1, pkg.scene.COMPOSE_DTYPE)
    c["flags"], c["ao_strength"], c["reserved"] = 1, 0.5, (0, 1, 0, 0)
    import ctypes as C
    s, st = desc.fill(pkg.scene.CScene()), pkg.scene.CSettings(0, 2.2, 1.0)
    vp = C.c_void_p
    assert r.L.arctic_compose_planes_device(r.h, C.byref(s), C.byref(st), vp(c.ctypes.data), vp(d_ao.data_ptr()), None, vp(out.data_ptr())) == INVALID    # reserved
    c["reserved"] = 0
    assert r.L.arctic_compose_planes_device(r.h, None, C.byref(st), vp(c.ctypes.data), vp(d_ao.data_ptr()), None, vp(out.data_ptr())) == INVALID
    assert r.L.arctic_compose_planes_device(r.h, C.byref(s), None, vp(c.ctypes.data), vp(d_ao.data_ptr()), None, vp(out.data_ptr())) == INVALID
    assert r.L.arctic_compose_planes_device(r.h, C.byref(s), C.byref(st), None, vp(d_ao.data_ptr()), None, vp(out.data_ptr())) == INVALID
    refused(STATE, lambda: r.read_composed())                                    # nothing composed yet
    r.flush()
    assert (out.cpu().numpy() == 0x5A).all()                                     # a refused call writes nothing ...
    assert r.compose_info() == (0, 0, 0, 0) and r.hit_shading_info() == (0, 0, 0, 0)   # ... and holds nothing, its tracing calls included
    # the same handle, every state put right: it composes what the fixture's handle composes
    r.write_gbuffer(w["attrs"], w["mat"])
    assert r.L.arctic_compose_planes_device(r.h, C.byref(s), C.byref(st), vp(c.ctypes.data), vp(d_ao.data_ptr()), None, vp(out.data_ptr())) == 0
    w["r"].compose_planes_device(desc, SETTINGS, d_ao.data_ptr(), None, ao_strength=0.5)
    r.flush()
    assert out.cpu().numpy().tobytes() == w["r"].read_composed(want=("rgba8",))[2].tobytes()
    r.resize(WIDTH, HEIGHT)
    refused(STATE, both)                                                         # a resize: no G-buffer, no HDR plane, nothing composed
    refused(STATE, lambda: r.read_composed())
    r.close()


def test_after_a_whole_frame_the_gbuffer_is_resolved_on_demand(pkg, hip, whole):
    """a frame is shaded from the visibility plane; the call resolves the G-buffer behind it -- the same result as with arctic_pass_gbuffer's"""
    w, desc = whole, whole["desc"]
    dirs = pkg.renderer.ao_directions(4, 2, seed=3)
    kw = dict(ao_strength=0.9, reflection_strength=1.2, **AO_KW)
    r = handle(pkg, hip, w["imgs"])
    frame = r.render_frame(desc, SETTINGS).copy()
    r.pass_ray_effects(desc, SETTINGS, dirs=dirs, reflection_bias=BIAS, **kw)
    on_demand = r.read_composed()
    r.pass_gbuffer(desc)                                                         # the G-buffer pass by pass; the HDR plane is still the frame's
    r.pass_ray_effects(desc, SETTINGS, dirs=dirs, reflection_bias=BIAS, **kw)
    for a, b in zip(r.read_composed(), on_demand):
        assert a.tobytes() == b.tobytes()
    _, hdr, rgba8 = r.read_output(want=("hdr", "rgba8"))
    assert rgba8.tobytes() == frame.tobytes()
    judge("after a frame", on_demand, reference(w, attrs=w["clean"][0], mat=w["clean"][1], hdr=hdr, ao=r.trace_ambient_occlusion(desc, dirs, **AO_KW),
                                                refl=r.trace_reflections(desc, BIAS), ao_strength=0.9, reflection_strength=1.2))
    r.close()


def test_nothing_else_moved(pkg, hip):
    """a frame's RGBA8 and arctic_stats are the same before the first call, after it, and on a handle that never calls; arctic_compose_info is
    zeros before the first call and after a refused one; the first call holds what it needs and at most DevBuf's quarter of headroom over that;
    a warm handle's second call allocates nothing"""
    desc = scene(pkg)
    dirs = pkg.renderer.ao_directions(4, 2, seed=3)
    a = handle(pkg, hip)                                                         # test_gpu_reflections' handle as it is
    first = a.render_frame(desc, SETTINGS).copy()
    before = a.stats().copy()
    assert a.compose_info() == (0, 0, 0, 0)
    with pytest.raises(hip.ArcticError):
        a.pass_ray_effects(desc, SETTINGS, dirs=dirs, reflection_bias=BIAS, ao_strength=2.0, **AO_KW)
    assert a.compose_info() == (0, 0, 0, 0) and a.hit_shading_info() == (0, 0, 0, 0)
    a.pass_ray_effects(desc, SETTINGS, dirs=dirs, reflection_bias=BIAS, read=False, **AO_KW)
    held = a.compose_info()
    n = WIDTH * HEIGHT
    need = [n * 4, n * 12, n * 12]
    assert sum(need) <= held[0] <= sum(x + x // 4 + 256 for x in need) and held[1:] == (1, 1, 0), (held, need)
    a.pass_ray_effects(desc, SETTINGS, dirs=dirs, reflection_bias=BIAS, read=False, **AO_KW)
    assert a.compose_info() == (held[0], 2, 2, 0)
    after = a.render_frame(desc, SETTINGS).copy()
    assert first.tobytes() == after.tobytes() and (a.stats()[:2] == before[:2]).all()
    b = handle(pkg, hip, keep_float=False)                                       # a handle that never makes the calls, and never kept a float plane
    assert b.render_frame(desc, SETTINGS).tobytes() == first.tobytes()
    assert (b.stats()[:8] == before[:8]).all() and b.compose_info() == (0, 0, 0, 0)
    assert len(np.unique(first.reshape(-1, 4), axis=0)) >= 100
    a.close(); b.close()
