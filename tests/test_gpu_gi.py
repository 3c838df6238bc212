"""The indirect diffuse light on the device (needs an MI355X): arctic_gi_rays and arctic_trace_gi against the numpy arbiter
(tests/gi_reference.py), bytes throughout.

On the scene of tests/hit_scenes.py at 64 x 48 and 37 x 21 pixels (neither height a multiple of 8, one width odd), from a G-buffer read back,
given hostile normals, positions and holes (tests/gi_scenes.py) and written again: every round's records for P in {1, 2, 4} and n_rays in
{1, 3}; the estimate end to end -- the published records traced by arctic_trace_rays and shaded by arctic_shade_hits on the same handle, summed
and averaged by numpy, filtered and not -- ; a floor under a sky of one colour, and in a closed box; shards; the refusals; and that a handle is
otherwise what it was.  tests/test_gi_reference.py checks on the CPU that the inputs are what they are taken for."""
import numpy as np
import pytest

import compose_reference as CR
import gi_reference as GI
import gi_scenes as GS
import hit_scenes as HS
import ray_reference as R
import shading_reference as SR
import test_gpu_extended_shading as G

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = [(64, 48), (37, 21)]
BIAS, MAX_DISTANCE = 2e-3, 40.0
INVALID, STATE = -1, -4
FILTER = dict(normal_cos=0.9, plane_dist=0.1)
HIST = dict(max_history=3.0, normal_cos=0.9, plane_dist=0.1, min_weight=0.1)
SETTINGS = (0, 2.2, 1.0)


def _desc(pkg, c, width, height):
    return pkg.scenes.SceneDesc(camera=dict(c.desc.camera, aspect=width / height), ambient=HS.AMBIENT, sun=c.desc.sun, objects=c.g.objects)


def _handle(pkg, hip, c, width, height, **kw):
    return HS.upload(pkg, hip.Renderer(width, height, HS.SHADOW, HS.MAX_LIGHTS, **kw), c)


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: "%dx%d" % s)
def frame(pkg, hip, request):
    """a handle with the hit scene's G-buffer, made hostile and written back"""
    width, height = request.param
    c = HS.scene(pkg, list(HS.ASSIGNMENTS)[0])
    desc = _desc(pkg, c, width, height)
    r = _handle(pkg, hip, c, width, height)
    r.set_option("keep_float_output", 1)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    r.pass_shade(desc, SETTINGS)                                                 # the float HDR plane the composition reads, shaded from the clean G-buffer
    _, hdr, _ = r.read_output(want=("hdr",))
    attrs, mat, _, _ = r.read_gbuffer(want=("attrs", "material"))
    assert (mat != GS.NO_MATERIAL).mean() > 0.4 and (mat == GS.NO_MATERIAL).mean() > 0.02
    attrs, mat, marks = GS.hostile_gbuffer(attrs, mat)
    r.write_gbuffer(attrs, mat)
    yield dict(r=r, c=c, desc=desc, attrs=attrs, mat=mat, marks=marks, width=width, height=height, hdr=hdr)
    r.close()


def differ(got, want):
    at = np.argwhere(got != want)
    return len(at), at[:6].tolist()


@pytest.mark.parametrize("P", [1, 2, 4])
@pytest.mark.parametrize("n_rays", [1, 3])
def test_rays_of_every_round_equal_numpy(hip, frame, P, n_rays):
    f, r = frame, frame["r"]
    dirs = GS.cosine_table(n_rays, P, 11)
    for round in range(n_rays):
        want, had = GI.image_rays(f["attrs"], f["mat"], dirs, n_rays, P, round, MAX_DISTANCE, BIAS)
        got = r.gi_rays(dirs, round, max_distance=MAX_DISTANCE, bias=BIAS)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (P, n_rays, round) + differ(got, want)
        flat = had.reshape(-1)
        assert not flat[f["marks"]["holes"]].any() and flat[f["marks"]["normal 0"]].all() and not flat[f["marks"]["normal 2"]].any()
        assert flat[f["marks"]["world 0"]].all() and 0.3 < flat.mean() < 1.0


@pytest.fixture(scope="module")
def by_hand(hip, frame):
    """rounds of published records, traced and shaded on the same handle"""
    f, r = frame, frame["r"]
    n_rays, P = 3, 4
    dirs = GS.cosine_table(n_rays, P, 12)
    kw = dict(max_distance=MAX_DISTANCE, bias=BIAS, clamp_max=8.0)
    rays = np.stack([r.gi_rays(dirs, k, **kw) for k in range(n_rays)])
    hits = np.stack([r.trace_rays(f["desc"], rays[k].ravel()).reshape(rays[k].shape) for k in range(n_rays)])
    colors = np.stack([r.shade_hits(f["desc"], rays[k].ravel(), hits[k].ravel()).reshape(rays[k].shape + (4,)) for k in range(n_rays)])
    return dict(n_rays=n_rays, P=P, dirs=dirs, kw=kw, rays=rays, hits=hits, colors=colors, S=GI.add(rays, colors, kw["clamp_max"]))


def test_the_estimate_is_the_rounds_by_hand(hip, frame, by_hand):
    f, r, b = frame, frame["r"], by_hand
    had, hit = b["rays"]["t_max"] > 0, b["hits"]["prim"] != R.NO_PRIM
    # not vacuous: rays that hit and rays that see the sky, colours that vary, colours the clamp cuts
    assert (had & hit).sum() >= 150 and (had & ~hit).sum() >= 150 and not hit[~had].any()
    assert len(np.unique(b["colors"][had][:, :3], axis=0)) >= 300 and (b["colors"][had][:, :3] > 8.0).any()
    assert not b["colors"][~had].any()
    want = GI.estimate(b["S"])
    got = r.trace_gi(f["desc"], b["dirs"], **b["kw"])
    assert got.shape == (f["height"], f["width"], 4) and got.dtype == F
    assert got.tobytes() == want.tobytes(), differ(got, want)
    planes = r.read_gi_estimate()
    assert planes["sum"].tobytes() == b["S"].tobytes() and planes["estimate"].tobytes() == want.tobytes()
    assert (got[had[0]][:, 3] == b["n_rays"]).all() and not got[~had[0]].any() and (got[..., :3] <= 8.0).all()
    wantf = GI.estimate(b["S"], f["attrs"], f["mat"], b["P"], filter=True, **FILTER)
    gotf = r.trace_gi(f["desc"], b["dirs"], filter=True, **b["kw"], **FILTER)
    assert gotf.tobytes() == wantf.tobytes(), differ(gotf, wantf)
    assert (gotf[..., 3] > b["n_rays"]).mean() > 0.3 and (gotf != got).any(-1).mean() > 0.3
    assert (gotf[had[0]][:, 3] < b["n_rays"] * 16).any()                         # windows cut by an edge, a hole or the frame
    assert (GI.estimate(b["S"], f["attrs"], f["mat"], b["P"], filter=True, defect="p_first", **FILTER) != wantf).any()
    # a second call on the warm handle gives the same bytes and allocates nothing
    held = r.gi_info()
    assert r.trace_gi(f["desc"], b["dirs"], **b["kw"]).tobytes() == want.tobytes() and r.gi_info()[0] == held[0]


@pytest.mark.parametrize("P", [1, 2])
def test_the_filter_at_the_smaller_patterns(hip, frame, P):
    f, r = frame, frame["r"]
    n_rays = 2
    dirs = GS.cosine_table(n_rays, P, 13)
    kw = dict(max_distance=MAX_DISTANCE, bias=BIAS, clamp_max=8.0)
    rays = np.stack([r.gi_rays(dirs, k, **kw) for k in range(n_rays)])
    colors = np.stack([r.shade_hits(f["desc"], rays[k].ravel(), r.trace_rays(f["desc"], rays[k].ravel())).reshape(rays[k].shape + (4,)) for k in range(n_rays)])
    S = GI.add(rays, colors, 8.0)
    want = GI.estimate(S, f["attrs"], f["mat"], P, filter=True, **FILTER)
    got = r.trace_gi(f["desc"], dirs, filter=True, **kw, **FILTER)
    assert got.tobytes() == want.tobytes(), (P,) + differ(got, want)


def test_the_device_form_and_the_plane_left_on_the_device(hip, frame, by_hand):
    import torch
    f, r, b = frame, frame["r"], by_hand
    n = f["height"] * f["width"]
    want = GI.estimate(b["S"])
    out = torch.full((n + 8, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.trace_gi_device(f["desc"], b["dirs"], out.data_ptr(), **b["kw"])
    r.flush()
    host = out.cpu().numpy()
    assert host[:n].tobytes() == want.tobytes() and (host[n:] == -7.0).all()
    with pytest.raises(hip.ArcticError) as e:                                    # the estimate went to the caller's plane
        r.read_gi_estimate(want=("estimate",))
    assert e.value.code == STATE
    assert r.read_gi_estimate(want=("sum",))["sum"].tobytes() == b["S"].tobytes()
    assert r.trace_gi(f["desc"], b["dirs"], read=False, **b["kw"]) is None
    assert r.read_gi_estimate()["estimate"].tobytes() == want.tobytes()


def test_refusals_write_nothing(pkg, hip, frame, by_hand):
    import torch
    f, b = frame, by_hand
    r = _handle(pkg, hip, f["c"], f["width"], f["height"])
    n = f["height"] * f["width"]
    out = torch.full((n, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def refused(code, call):
        with pytest.raises(hip.ArcticError) as e:
            call()
        assert e.value.code == code, e.value
    dirs = b["dirs"]
    r.pass_shadow_map(f["desc"])
    refused(STATE, lambda: r.trace_gi(f["desc"], dirs))                          # no G-buffer yet
    refused(STATE, lambda: r.gi_rays(dirs, 0))
    n_fresh = _handle(pkg, hip, f["c"], f["width"], f["height"])                 # a sun map never drawn or written
    n_fresh.write_gbuffer(f["attrs"], f["mat"])
    refused(STATE, lambda: n_fresh.trace_gi(f["desc"], dirs))
    assert n_fresh.gi_rays(dirs, 0).shape == (f["height"], f["width"])           # the records need no map
    n_fresh.close()
    r.write_gbuffer(f["attrs"], f["mat"])
    assert r.gi_info() == (0, 0, 0, 0)
    for bad in (dict(n_rays=0), dict(n_rays=17), dict(pattern=3), dict(max_distance=0.0), dict(max_distance=np.nan), dict(bias=np.inf), dict(clamp_max=0.0),
                dict(clamp_max=np.inf), dict(clamp_max=np.nan), dict(filter=2), dict(filter=True, normal_cos=np.nan), dict(filter=True, plane_dist=-1.0)):
        refused(INVALID, lambda: r.trace_gi_device(f["desc"], np.zeros((16, 17, 3), F), out.data_ptr(), **dict(dict(n_rays=3, pattern=4), **bad)))
    poisoned = dirs.copy()
    poisoned[5, 1, 2] = np.nan
    refused(INVALID, lambda: r.trace_gi_device(f["desc"], poisoned, out.data_ptr()))
    # the stated order, by behaviour: of two faults the earlier kind is the one the message names
    big = np.zeros((16, 17, 3), F)
    for two, named in ((dict(n_rays=0, pattern=3), "n_rays"), (dict(pattern=3, max_distance=0.0), "pattern"), (dict(max_distance=0.0, bias=np.nan), "max_distance"),
                       (dict(bias=np.nan, clamp_max=0.0), "bias"), (dict(clamp_max=0.0, filter=2), "clamp_max")):
        with pytest.raises(hip.ArcticError) as e:
            r.trace_gi(f["desc"], big, **dict(dict(n_rays=3, pattern=4), **two))
        assert e.value.code == INVALID and named in str(e.value), (two, str(e.value))
    with pytest.raises(hip.ArcticError) as e:                                    # a fault of the block comes before one of the table
        r.trace_gi(f["desc"], poisoned, clamp_max=np.inf)
    assert "clamp_max" in str(e.value)
    q = _handle(pkg, hip, f["c"], f["width"], f["height"])                       # ... and ARCTIC_E_INVALID before ARCTIC_E_STATE: a bad block on a handle without a G-buffer
    refused(INVALID, lambda: q.trace_gi(f["desc"], dirs, clamp_max=0.0))
    refused(STATE, lambda: q.trace_gi(f["desc"], dirs))
    q.close()
    refused(INVALID, lambda: r.trace_gi_device(f["desc"], dirs, 0))
    refused(INVALID, lambda: r.trace_gi_device(f["desc"], dirs, out.data_ptr() + 8))
    refused(INVALID, lambda: r.gi_rays(dirs, 3))
    r.set_option("shadow_sharded", 1)
    refused(STATE, lambda: r.trace_gi_device(f["desc"], dirs, out.data_ptr()))
    r.set_option("shadow_sharded", 0)
    refused(STATE, lambda: r.read_gi_estimate())
    r.flush()
    assert (out.cpu().numpy() == -7.0).all() and r.gi_info() == (0, 0, 0, 0) and r.hit_shading_info() == (0, 0, 0, 0)
    r.close()


def test_a_shard_follows_the_rows_of_the_frame_and_refuses_the_filter(pkg, hip, frame, by_hand):
    import ray_scenes as S
    f, b = frame, by_hand
    shard = dict(row_begin=3, row_end=f["height"] - 5)
    rows = S.owned(pkg, f["height"], shard)
    r = _handle(pkg, hip, f["c"], f["width"], f["height"], **shard)
    r.pass_shadow_map(f["desc"])
    r.write_gbuffer(f["attrs"][rows], f["mat"][rows])
    got = r.trace_gi(f["desc"], b["dirs"], **b["kw"])
    want = GI.estimate(b["S"])[rows]
    assert got.shape == (len(rows), f["width"], 4) and got.tobytes() == want.tobytes(), differ(got, want)
    with pytest.raises(hip.ArcticError) as e:
        r.trace_gi(f["desc"], b["dirs"], filter=True, **b["kw"])
    assert e.value.code == STATE
    assert r.read_gi_estimate()["estimate"].tobytes() == want.tobytes()          # the refused call wrote nothing
    r.close()


def _sky_scene(pkg, hip, boxed, width=40, height=24):
    """a floor, a sky of one colour L0, no light: the sun is black, there are no point lights, ambient is 0 -- unless `boxed`, where a closed box
    stands around floor and camera and the flat ambient is what its walls return"""
    sc = pkg.scenes
    L0 = np.array([0.7, 1.9, 0.2], F)
    r = hip.Renderer(width, height, 64, 16)
    r.create_material(*sc.fallback_textures())
    r.create_mesh(*sc.quad((-5, 0, 5), (10, 0, 0), (0, 0, -10), 4, 4), 0)
    places = [(np.eye(4), 0)]
    if boxed:
        r.create_mesh(*sc.box(12.0, 6.0, 12.0, 2), 0)
        lift = np.eye(4)
        lift[1, 3] = 2.5
        places.append((lift, 1))
    env = np.ones((16, 32, 4), F)
    env[..., :3] = L0
    r.create_hdri(env)
    desc = sc.SceneDesc(camera=dict(eye=(-3.2, 2.9, 4.2), rotation=(-27.0, -52.0), aspect=width / height, fov_y=45.0, z_near_far=(0.1, 100.0)),
                        ambient=0.25 if boxed else 0.0, sun=dict(sc.DEFAULT_SUN, color=(0.0, 0.0, 0.0)), objects=pkg.scene.make_objects(places))
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    return r, desc, L0


def test_a_floor_under_a_sky_of_one_colour(pkg, hip):
    r, desc, L0 = _sky_scene(pkg, hip, False)
    _, mat, _, _ = r.read_gbuffer(want=("attrs", "material"))
    covered = mat != GS.NO_MATERIAL
    assert covered.mean() > 0.3
    n_rays = 3
    for P in (1, 4):
        E = r.trace_gi(desc, hip.gi_directions(n_rays, P), max_distance=np.inf, bias=BIAS)
        assert (E[covered][:, 3] == n_rays).all() and not E[~covered].any()
        # the bound: the four bilinear weights' products sum to 1 within 3 * 2^-24; n <= 3 equal terms summed in order and divided by n add
        # (n - 1) * 2^-24 and one rounding of the exact division: 7 * 2^-24 in all, inside 4 * 2^-23
        err = np.abs(E[covered][:, :3].astype(np.float64) - L0.astype(np.float64))
        print("P = %d: largest |E - L0| / L0 = %.3g (bound %.3g)" % (P, (err / L0).max(), 4 * 2.0 ** -23))
        assert (err <= 4 * 2.0 ** -23 * L0.astype(np.float64)).all()
    r.close()


def test_the_same_floor_in_a_closed_box(pkg, hip):
    r, desc, L0 = _sky_scene(pkg, hip, True)
    _, mat, _, _ = r.read_gbuffer(want=("attrs", "material"))
    covered = mat != GS.NO_MATERIAL                                              # (the walls are seen from behind: the rasteriser may cull them, the rays do not)
    assert covered.mean() > 0.3
    n_rays, P = 3, 2
    dirs = hip.gi_directions(n_rays, P)
    for k in range(n_rays):
        rays = r.gi_rays(dirs, k, bias=BIAS)
        assert ((rays["t_max"] == np.inf) == covered).all()
        assert (r.trace_rays(desc, rays[covered])["prim"] != R.NO_PRIM).all()    # no ray misses
    E = r.trace_gi(desc, dirs, bias=BIAS)
    # every ray returns the flat ambient of a white, black-lit surface: 0.25 * base = 0.25, never the sky
    assert (E[covered][:, 3] == n_rays).all() and np.abs(E[covered][:, :3] - 0.25).max() <= 0.25 * 4 * 2.0 ** -23 and not E[~covered].any()
    r.close()


def test_nothing_else_moved(pkg, hip, frame, by_hand):
    """a frame, a reflection plane and an occlusion plane are the same bytes before and after the calls, on a handle that makes them and on one
    that never does; the hit layers hold no more than the reflection plane needs"""
    f, b = frame, by_hand
    settings = (2, 2.2, 1.0)
    a = _handle(pkg, hip, f["c"], f["width"], f["height"])
    first = a.render_frame(f["desc"], settings).copy()
    refl = a.trace_reflections(f["desc"], BIAS).copy()
    ao = a.trace_ambient_occlusion(f["desc"], b["dirs"], radius=1.5, bias=BIAS).copy()
    held = a.hit_shading_info()
    assert a.gi_info() == (0, 0, 0, 0)
    E = a.trace_gi(f["desc"], b["dirs"], **b["kw"])
    a.trace_gi(f["desc"], b["dirs"], filter=True, **b["kw"], **FILTER)
    device, launches, calls, _ = a.gi_info()
    n = f["width"] * f["height"]
    need = [16 * 16 * 3 * 4, n * 16, n * 16]                                     # the largest table, S, E
    assert sum(need) <= device <= sum(x + x // 4 + 256 for x in need) and calls == 2 and launches == 2 * (2 * b["n_rays"] + 1)
    assert a.hit_shading_info()[0] == held[0]                                    # the rounds ran in the reflection plane's buffers
    assert a.render_frame(f["desc"], settings).tobytes() == first.tobytes()
    assert a.trace_reflections(f["desc"], BIAS).tobytes() == refl.tobytes()
    assert a.trace_ambient_occlusion(f["desc"], b["dirs"], radius=1.5, bias=BIAS).tobytes() == ao.tobytes()
    assert len(np.unique(first.reshape(-1, 4), axis=0)) >= 100 and E[..., 3].max() == b["n_rays"]
    a.resize(f["width"], f["height"])                                            # a resize empties the stage's planes
    with pytest.raises(hip.ArcticError):
        a.read_gi_estimate()
    a.close()


def _moved(pkg, f, k):
    """frame k's scene: the camera of the fixture, moved and turned a little more each frame"""
    cam = dict(f["desc"].camera)
    cam["eye"] = tuple(np.array(cam["eye"]) + k * np.array([0.06, 0.02, -0.04]))
    cam["rotation"] = (cam["rotation"][0] + 0.5 * k, cam["rotation"][1] - 0.9 * k)
    return pkg.scenes.SceneDesc(camera=cam, ambient=HS.AMBIENT, sun=f["desc"].sun, objects=f["c"].g.objects)


def test_four_frames_of_a_moving_camera_accumulate_as_numpy_does(pkg, hip, frame):
    f = frame
    r = _handle(pkg, hip, f["c"], f["width"], f["height"])
    r.pass_shadow_map(f["desc"])
    assert r.gi_info()[3] == 0
    prev, seen = None, np.zeros(6, np.int64)
    for k in range(4):
        desc = _moved(pkg, f, k)
        r.pass_gbuffer(desc)
        attrs, mat, _, _ = r.read_gbuffer(want=("attrs", "material"))
        E = r.trace_gi(desc, hip.gi_directions(1, 4, seed=k), max_distance=MAX_DISTANCE, bias=BIAS, clamp_max=8.0, filter=True, **FILTER)   # the table turned per frame
        got = r.accumulate_gi(desc, E, **HIST)
        want, prev, accepted = GI.accumulate_frame(attrs, mat, E, prev, hip.frame_constants(desc)[0], HIST)
        assert got.tobytes() == want.tobytes(), (k,) + differ(got, want)
        h = r.read_gi_history()
        for name in ("acc", "count", "world", "normal"):
            assert h[name].tobytes() == prev[name].tobytes(), (k, name)
        seen += np.bincount(accepted.reshape(-1) + 1, minlength=6)
        assert (got[..., 3] == prev["count"]).all() and (got[..., 3] <= HIST["max_history"]).all()
    # not vacuous: pixels without a history, taps all accepted, taps some of which an edge rejected, and counts that reached the cap
    assert seen[5] >= 300 and seen[2:5].sum() >= 100 and seen[1] >= 1 and (prev["count"] == HIST["max_history"]).sum() >= 50, seen
    n_tiles = ((f["width"] + 7) // 8) * ((f["height"] + 7) // 8)
    assert r.gi_info()[3] == 6 * n_tiles * 64 * 16                               # two sets of three float4 planes, tile-major: 96 bytes per pixel
    # a reset empties it: the next call is a first call; so does a resize
    desc = _moved(pkg, f, 3)
    r.gi_history_reset()
    with pytest.raises(hip.ArcticError) as e:
        r.read_gi_history()
    assert e.value.code == STATE
    first = r.accumulate_gi(desc, E, **HIST)
    assert first.tobytes() == GI.accumulate_frame(attrs, mat, E, None, hip.frame_constants(desc)[0], HIST)[0].tobytes() and (first[..., 3] <= 1).all()
    r.resize(f["width"], f["height"])
    with pytest.raises(hip.ArcticError):
        r.read_gi_history()
    r.close()
    # a row shard has no neighbours' rows: refused, like the filter
    shard = hip.Renderer(f["width"], f["height"], HS.SHADOW, HS.MAX_LIGHTS, row_begin=3, row_end=f["height"] - 5)
    shard.write_gbuffer(f["attrs"][3:f["height"] - 5], f["mat"][3:f["height"] - 5])
    with pytest.raises(hip.ArcticError) as e:
        shard.accumulate_gi(desc, E[3:f["height"] - 5], **HIST)
    assert e.value.code == STATE
    shard.close()


def test_the_composition_against_float64(pkg, hip, frame, by_hand):
    """the references: shading_reference's sampler and the header's two terms in float64; E read back from the handle is an input.  Every pixel is
    judged at both of the project's standing bars (test_gpu_compose's rule: the HDR plane was shaded from the clean G-buffer and is finite
    everywhere, and none is left out).  As there, the cases keep part of the ambient term -- ambient_scale 0.2, 0.5 and 1 --: at ambient_scale = 0
    a shadowed pixel whose rays brought nothing is the difference of two equal numbers, 0 on the device and a residue of 1e-8 in float64, which
    the gamma curve turns into 2e-4 of LDR whatever the kernel does.  ambient_scale = 0 is held by bytes instead, through the arbiter below and
    in tests/test_gi_reference.py"""
    f, r, b = frame, frame["r"], by_hand
    E = r.trace_gi(f["desc"], b["dirs"], filter=True, **b["kw"], **FILTER)
    assert np.isfinite(f["hdr"]).all() and np.isfinite(E).all()
    ch = SR.material_channels(f["c"].materials, f["attrs"], f["mat"]).reshape(-1, 8)
    geometry = (f["mat"] != GS.NO_MATERIAL).reshape(-1)
    for settings, strength, scale in ((SETTINGS, 1.0, 0.2), ((1, 2.2, 0.7), 0.6, 0.5), ((2, 2.4, 1.0), 2.0, 1.0)):
        r.gi_compose_device(f["desc"], settings, gi_strength=strength, ambient_scale=scale)
        got = r.read_gi()
        C = GI.compose(f["hdr"], ch[:, 0:3], ch[:, 7], E, geometry, HS.AMBIENT, strength, scale, dtype=np.float64)
        ldr, rgba8 = CR.tonemap(C, settings)
        rel = CR.rel_err(got["hdr"].reshape(-1, 3), C).max()
        err = np.abs(got["ldr"].reshape(-1, 3).astype(np.float64) - ldr).max()
        step = np.abs(got["rgba8"].reshape(-1, 4).astype(np.int32) - rgba8.astype(np.int32)).max()
        print(f"tonemapper {settings[0]}, strength {strength}, scale {scale}: hdr relative {rel:.3e}, ldr {err:.3e}, rgba8 steps {step}")
        assert rel <= G.HDR_REL == 1e-4 and err <= G.TOL == 1e-4 and step <= 1
        moved = (CR.rel_err(got["hdr"], f["hdr"].astype(np.float64)).max(-1) > 100 * G.HDR_REL).reshape(-1)
        assert moved[geometry & (E[..., 3].reshape(-1) > 0)].mean() >= 0.6         # not vacuous: the terms move pixels by far more than the bar
        assert got["hdr"].reshape(-1, 3)[~geometry].tobytes() == f["hdr"].reshape(-1, 3)[~geometry].tobytes()   # a pixel without geometry keeps its C
    # with gi_strength = 0 and ambient_scale = 1 the composed HDR is C by bits, and the tonemapper gives the frame's own planes
    r.gi_compose_device(f["desc"], SETTINGS, gi_strength=0.0, ambient_scale=1.0)
    got = r.read_gi()
    ldr, hdr, rgba8 = r.read_output()
    assert got["hdr"].tobytes() == f["hdr"].tobytes() == hdr.tobytes() and got["ldr"].tobytes() == ldr.tobytes() and got["rgba8"].tobytes() == rgba8.tobytes()
    # the arbiter carries out the same two terms on this frame's channels, ambient_scale = 0 included: numpy's fp32 result by bytes
    for strength, scale in ((0.6, 0.5), (1.0, 0.0)):
        host = hip.gi_compose_pixels(f["hdr"], ch[:, 0:3].astype(F), ch[:, 7].astype(F), E, geometry, HS.AMBIENT, gi_strength=strength, ambient_scale=scale)
        want = GI.compose(f["hdr"], ch[:, 0:3].astype(F), ch[:, 7].astype(F), E, geometry, HS.AMBIENT, strength, scale)
        assert host.tobytes() == want.tobytes(), (strength, scale)
    # refusals: parameters, and an ambient correction on a term that is not the flat one
    for bad in (dict(gi_strength=-1.0), dict(gi_strength=np.inf), dict(ambient_scale=1.5), dict(ambient_scale=np.nan), dict(flags=2)):
        with pytest.raises(hip.ArcticError) as e:
            r.gi_compose_device(f["desc"], SETTINGS, **bad)
        assert e.value.code == INVALID, bad
    r.set_option("env_lighting", 1)
    with pytest.raises(hip.ArcticError) as e:
        r.gi_compose_device(f["desc"], SETTINGS, ambient_scale=0.5)
    assert e.value.code == STATE
    r.set_option("env_lighting", 0)
    with pytest.raises(hip.ArcticError) as e:                                    # nothing composed on this handle: the composed plane is no source
        r.gi_compose_device(f["desc"], SETTINGS, flags=hip.binding.GI_SOURCE_COMPOSED)
    assert e.value.code == STATE
    assert r.read_gi()["hdr"].tobytes() == f["hdr"].tobytes()                    # the refused calls wrote nothing


def test_the_one_call_is_the_calls_by_hand(pkg, hip, frame, by_hand):
    import torch
    f, b = frame, by_hand
    n = f["width"] * f["height"]
    hist, comp = hip.gi_history_arguments(**HIST), hip.gi_compose_arguments(0.8, 0.25)
    results = []
    for one_call in (False, True):
        r = _handle(pkg, hip, f["c"], f["width"], f["height"])
        r.set_option("keep_float_output", 1)
        r.pass_shadow_map(f["desc"])
        planes = []
        for k in range(2):                                                       # two frames: the second one reads a history
            desc = _moved(pkg, f, k)
            r.pass_gbuffer(desc)
            r.pass_shade(desc, SETTINGS)
            kw = dict(b["kw"], filter=True, **FILTER)
            if one_call:
                r.pass_gi(desc, SETTINGS, b["dirs"], hist=hist, compose=comp, **kw)
            else:
                plane = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                r.trace_gi_device(desc, b["dirs"], plane.data_ptr(), **kw)
                r.accumulate_gi_device(desc, plane.data_ptr(), plane.data_ptr(), hist=hist)
                r.gi_compose_device(desc, SETTINGS, d_gi_ptr=plane.data_ptr(), compose=comp)
            got = r.read_gi()
            planes.append((got["hdr"].copy(), got["ldr"].copy(), got["rgba8"].copy(), r.read_gi_history()))
        results.append(planes)
        if one_call:                                                             # the HDR plane goes on as a later stage's explicit colour
            hdr = torch.from_numpy(planes[-1][0]).cuda()
            torch.cuda.synchronize()
            r.bloom_device(SETTINGS, d_hdr_ptr=hdr.data_ptr())
            r.flush()
            with pytest.raises(hip.ArcticError):                                 # every refusal comes before anything is enqueued
                r.pass_gi(desc, SETTINGS, b["dirs"], hist=hist, compose=hip.gi_compose_arguments(-1.0), **kw)
            assert r.read_gi()["hdr"].tobytes() == planes[-1][0].tobytes()
        r.close()
    for k in range(2):
        by, one = results[0][k], results[1][k]
        assert all(by[i].tobytes() == one[i].tobytes() for i in range(3)), k
        assert all(by[3][name].tobytes() == one[3][name].tobytes() for name in by[3]), k
    assert (results[1][1][3]["count"] > 1).sum() >= 100 and (results[1][1][0] != results[1][0][0]).any()
