"""arctic_trace_reflections on the device (needs an MI355X): the plane against the composition done by hand -- the rays of
tests/hit_reference.py's restatement of the ray rule, arctic_trace_rays, arctic_shade_hits -- bit for bit; where a is 0; shards; the device
form; the G-buffer resolved on demand after a whole frame; and that a handle which never makes these calls is what it was: the same RGBA8, and
nothing allocated before the first call (arctic_hit_shading_info)."""
import numpy as np
import pytest

import ao_scenes as AS
import hit_reference as HR

pytestmark = pytest.mark.gpu
F = np.float32
WIDTH, HEIGHT = 96, 64
BIAS = 1e-3
SHARDS = {"rows 13..45": [dict(row_begin=13, row_end=45)], "bands of 8, 2 shards": [dict(band_rows=8, shard=(k, 2)) for k in range(2)]}
INVALID, STATE = -1, -4


def scene(pkg):
    sc = AS.raster_scene(pkg)
    return pkg.scenes.SceneDesc(camera=dict(sc.desc.camera, aspect=WIDTH / HEIGHT), ambient=0.1, sun=sc.desc.sun, objects=sc.desc.objects)


def handle(pkg, hip, env=True, **kw):
    r = AS.raster_upload(pkg, hip.Renderer(WIDTH, HEIGHT, 64, 16, **kw))
    r.update_lights(pkg.scenes.random_lights(np.random.default_rng(64), 5, (-3, 0.5, -3), (3, 3, 3), intensity=6.0))
    if env:
        r.create_hdri(pkg.scenes.synthetic_hdri(64, 32))
    return r


@pytest.fixture(scope="module")
def whole(pkg, hip):
    """the whole frame's plane, its G-buffer, and the composition by hand"""
    desc = scene(pkg)
    r = handle(pkg, hip)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    attrs, mat, _, _ = r.read_gbuffer(want=("attrs", "material"))
    # degenerate normals over some covered pixels, and pixels without geometry: the G-buffer is written back
    rng = np.random.default_rng(65)
    cov = np.nonzero((mat != HR.NO_MATERIAL).reshape(-1))[0]
    px = rng.choice(cov, 40, replace=False).reshape(4, 10)
    flat = attrs.reshape(-1, 18)
    for k, n in enumerate([(0, 0, 0), (np.nan, 0, 1), (3e19, 3e19, 3e19), (1e-30, 1e-30, 0)]):
        flat[px[k], 8:11] = np.array(n, F)
    flat[rng.choice(cov, 200, replace=False), 8:11] *= F(-1.0)                   # ... and normals turned away from the eye
    r.write_gbuffer(attrs, mat)
    plane = r.trace_reflections(desc, BIAS)
    rays, has = HR.reflection_rays(attrs, mat, desc.camera["eye"], BIAS)
    hits = r.trace_rays(desc, rays)
    by_hand = r.shade_hits(desc, rays, hits)
    yield dict(desc=desc, r=r, attrs=attrs, mat=mat, plane=plane, rays=rays, has=has, hits=hits, by_hand=by_hand, degenerate=px)
    r.close()


def test_the_plane_is_the_composition_by_hand(pkg, hip, whole):
    w = whole
    assert w["plane"].shape == (HEIGHT, WIDTH, 4) and w["plane"].dtype == np.float32
    differ = np.nonzero((w["plane"].reshape(-1, 4) != w["by_hand"]).any(1))[0]
    assert w["plane"].tobytes() == w["by_hand"].tobytes(), (len(differ), differ[:8].tolist())
    # not vacuous: pixels with a ray and without, reflections that show geometry, the sky, and a shaded colour that varies
    has, hit = w["has"], w["hits"]["prim"] != HR.NO_PRIM
    assert has.mean() >= 0.3 and (~has).mean() >= 0.1 and (has & hit).sum() >= 300 and (has & ~hit).sum() >= 300
    assert len(np.unique(w["plane"][..., :3].reshape(-1, 3)[has & hit], axis=0)) >= 200


def test_where_a_is_zero(pkg, hip, whole):
    w = whole
    flat = w["plane"].reshape(-1, 4)
    has, hit = w["has"], w["hits"]["prim"] != HR.NO_PRIM
    assert (flat[has & hit, 3] == 1).all() and (flat[~(has & hit), 3] == 0).all()
    assert not flat[~has].any()                                                  # no geometry, a degenerate normal, facing away: {0, 0, 0, 0}
    no_geometry = (w["mat"] == HR.NO_MATERIAL).reshape(-1)
    assert no_geometry.sum() >= 100 and not has[no_geometry].any() and not has[w["degenerate"].reshape(-1)].any()
    _, covered = HR.unit_normal(w["attrs"].reshape(-1, 18)[:, 8:11])
    away = ~no_geometry & covered & ~has
    assert away.sum() >= 150                                                     # the turned normals, and the faces seen at a slant from behind their vertex normal
    assert (flat[has & ~hit, :3] > 0).all()                                      # the environment map along the ray


@pytest.mark.parametrize("sharding", list(SHARDS))
def test_shards_return_their_rows_of_the_frame(pkg, hip, whole, sharding):
    import ray_scenes as S
    w = whole
    seen = []
    for shard in SHARDS[sharding]:
        r = handle(pkg, hip, **shard)
        rows = S.owned(pkg, HEIGHT, shard)
        r.pass_shadow_map(w["desc"])
        r.write_gbuffer(w["attrs"][rows], w["mat"][rows])
        got = r.trace_reflections(w["desc"], BIAS)
        assert got.shape == (len(rows), WIDTH, 4) and got.tobytes() == w["plane"][rows].tobytes(), (sharding, shard)
        seen.append(rows)
        r.close()
    assert 0 < len(np.concatenate(seen)) <= HEIGHT


def test_the_device_form_and_the_plane_left_on_the_device(pkg, hip, whole):
    import torch
    w, r = whole, whole["r"]
    out = torch.full((HEIGHT * WIDTH + 8, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.trace_reflections_device(w["desc"], BIAS, out.data_ptr())
    r.flush()
    host = out.cpu().numpy()
    assert host[:HEIGHT * WIDTH].tobytes() == w["plane"].tobytes() and (host[HEIGHT * WIDTH:] == -7.0).all()
    assert r.trace_reflections(w["desc"], BIAS, read=False) is None
    assert r.trace_reflections(w["desc"], BIAS).tobytes() == w["plane"].tobytes()
    other = r.trace_reflections(w["desc"], 0.05)                                 # the bias matters
    assert (other != w["plane"]).any(-1).mean() >= 0.05


def test_refusals_write_nothing(pkg, hip, whole):
    import torch
    desc = whole["desc"]
    r = handle(pkg, hip)
    out = torch.full((HEIGHT * WIDTH, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def refused(code, call):
        with pytest.raises(hip.ArcticError) as e:
            call()
        assert e.value.code == code, e.value
    r.pass_shadow_map(desc)
    refused(STATE, lambda: r.trace_reflections(desc, BIAS))                      # no G-buffer yet
    refused(STATE, lambda: r.trace_reflections_device(desc, BIAS, out.data_ptr()))
    r.write_gbuffer(whole["attrs"], whole["mat"])
    for bias in (np.nan, np.inf, -np.inf):
        refused(INVALID, lambda: r.trace_reflections_device(desc, bias, out.data_ptr()))
    refused(INVALID, lambda: r.trace_reflections_device(desc, BIAS, 0))
    refused(INVALID, lambda: r.trace_reflections_device(desc, BIAS, out.data_ptr() + 8))
    r.set_option("shadow_sharded", 1)
    refused(STATE, lambda: r.trace_reflections_device(desc, BIAS, out.data_ptr()))
    r.set_option("shadow_sharded", 0)
    r.flush()
    assert (out.cpu().numpy() == -7.0).all()
    assert r.trace_reflections(desc, BIAS).tobytes() == whole["plane"].tobytes()
    r.close()
    n = handle(pkg, hip)                                                         # a sun map never drawn or written
    n.write_gbuffer(whole["attrs"], whole["mat"])
    refused(STATE, lambda: n.trace_reflections(desc, BIAS))
    n.close()


def test_after_a_whole_frame_the_gbuffer_is_resolved_on_demand(pkg, hip):
    desc = scene(pkg)
    r = handle(pkg, hip)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    want = r.trace_reflections(desc, BIAS)
    r.close()
    r = handle(pkg, hip)
    r.render_frame(desc, (0, 2.2, 1.0))                      # shaded from the visibility plane: no explicit G-buffer pass; the frame drew the sun's map
    assert r.trace_reflections(desc, BIAS).tobytes() == want.tobytes()
    r.close()


def test_nothing_else_moved(pkg, hip):
    """a frame is the same bytes on a handle that never makes these calls, before the first of them, and after it; the counters arctic_stats
    reports for a frame do not move either"""
    desc, settings = scene(pkg), (2, 2.2, 1.0)
    a = handle(pkg, hip)
    first = a.render_frame(desc, settings).copy()
    before = a.stats().copy()
    a.trace_reflections(desc, BIAS)
    attrs, mat = a.hit_attributes(desc, np.zeros(3, pkg.scene.HIT_DTYPE))
    assert (mat != HR.NO_MATERIAL).all()
    after = a.render_frame(desc, settings).copy()
    assert first.tobytes() == after.tobytes() and (a.stats()[:2] == before[:2]).all()
    b = handle(pkg, hip)                                                         # a handle that never makes the calls
    assert b.render_frame(desc, settings).tobytes() == first.tobytes()
    assert (b.stats()[:8] == before[:8]).all()
    assert len(np.unique(first.reshape(-1, 4), axis=0)) >= 100                   # (a frame with something in it)
    a.close(); b.close()


def test_nothing_is_allocated_before_the_first_call(pkg, hip):
    """arctic_hit_shading_info: what the three layers hold.  Nothing on a warm handle -- frames rendered, the sun's map drawn, the G-buffer
    resident, the ray structure built and walked by the calls that were there before --, nothing after a refused call; the first call makes what
    it needs and no more than DevBuf's quarter of headroom over that; a warm handle's next call makes nothing"""
    desc = scene(pkg)
    r = handle(pkg, hip)
    r.render_frame(desc, (2, 2.2, 1.0))
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    r.trace_sun_visibility(desc, BIAS)                                           # builds the ray structure: not this feature's
    assert r.ray_scene_info()[2] == 1 and r.hit_shading_info() == (0, 0, 0, 0)
    with pytest.raises(hip.ArcticError):
        r.trace_reflections(desc, np.nan)
    with pytest.raises(hip.ArcticError):
        r.trace_reflections_device(desc, BIAS, 0)
    assert r.hit_shading_info() == (0, 0, 0, 0)
    r.trace_reflections(desc, BIAS, read=False)
    device, pinned, prims, made = r.hit_shading_info()
    n, n_obj = WIDTH * HEIGHT, len(desc.objects)
    assert prims >= r.ray_scene_info()[0] > 0 and made == 1 and r.ray_scene_info()[2] == 1
    need = [prims * 16, n_obj * 80, n * 32, n * 16, n * 16]                      # the source table, the object records, the rays, the hits, the colours
    assert sum(need) <= device <= sum(x + x // 4 + 256 for x in need), (device, need)
    assert n_obj * 80 <= pinned <= 3 * n_obj * 80, pinned                        # one slot of the ring so far; three at the most
    r.trace_reflections(desc, BIAS, read=False)                                  # warm: nothing more on the device, the ring's next slot
    assert r.hit_shading_info() == (device, 2 * pinned, prims, 1)
    r.hit_attributes(desc, np.zeros(3, pkg.scene.HIT_DTYPE))                     # its own two outputs, once
    more = [3 * 72, 3 * 4]
    held = r.hit_shading_info()
    assert device + sum(more) <= held[0] <= device + sum(x + x // 4 + 256 for x in more) and held[1:] == (3 * pinned, prims, 1)
    r.hit_attributes(desc, np.zeros(3, pkg.scene.HIT_DTYPE))
    r.trace_reflections(desc, BIAS, read=False)
    assert r.hit_shading_info() == held
    r.close()
