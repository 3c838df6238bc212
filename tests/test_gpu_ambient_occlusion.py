"""Ambient occlusion on the device (needs an MI355X): arctic_trace_ambient_occlusion / arctic_trace_ambient_occlusion_device against the numpy
arbiter (tests/ao_reference.py), bytes throughout.

From an injected G-buffer of 52 x 37 pixels (7 x 5 tiles; the width no multiple of 8) over the 5- and the 1000-triangle scene, every n_rays x
pattern x radius of tests/ao_scenes.py, and a table with zero and subnormal direction components that sends whole tiles down the odd walk; from a
rasterised G-buffer, unfiltered and filtered; on a row range that cuts tiles and on interleaved bands, where the pattern has to follow the FRAME's
rows and the filter is refused; into a torch buffer; the refusals; the structure's reuse, rebuild and refit; and after a whole frame.
tests/test_ao_reference.py checks on the CPU that the inputs are what they are taken for; the conditions that make a comparison mean something
are asserted here again, on the same objects."""
import numpy as np
import pytest

import ao_reference as A
import ao_scenes as AS
import ray_reference as R
import ray_scenes as S

pytestmark = pytest.mark.gpu

INVALID, STATE = -1, -4


def injected_handle(pkg, hip, c, shard=None):
    width, height = S.SUN_SIZE
    rows = np.arange(height) if not shard else S.owned(pkg, height, shard)
    r = c.data.handle(pkg, hip, width, height, **(shard or {}))
    r.write_gbuffer(c.attrs[rows], c.material[rows])                                          # (a sharded handle takes its own rows)
    return r, rows


def differ(got, want):
    at = np.argwhere(got != want)
    return len(at), at[:6].tolist(), got[got != want][:6].tolist(), want[got != want][:6].tolist()


@pytest.mark.parametrize("n_tris", [5, 1000])
def test_unfiltered_from_an_injected_gbuffer(pkg, hip, n_tris):
    c = AS.injected_case(pkg, n_tris)
    for key, v in AS.check_injected_conditions(c).items():
        print(n_tris, "triangles, pattern %d, %d rays, radius %s: no hit / every ray hits / between =" % key, v)
    r, _ = injected_handle(pkg, hip, c)
    for P in AS.PATTERNS:
        for n in AS.N_RAYS:
            for radius in (c.radius, np.inf):
                _, covered, want = AS.injected_want(c, n, P, radius)
                got = r.trace_ambient_occlusion(c.data.desc, AS.table(c.master, n, P), radius=radius, bias=AS.BIAS)
                assert got.shape == want.shape and got.dtype == np.uint8
                assert got.tobytes() == want.tobytes(), (P, n, radius) + differ(got, want)
                assert (got[~covered] == 255).all()
    assert r.ray_scene_info()[2] == 1                                                         # one structure served every call
    r.close()


def test_zero_and_subnormal_directions_take_the_odd_walk(pkg, hip):
    c, o = AS.injected_case(pkg, 1000), AS.odd_case(pkg)
    print("tiles x rays of the odd table:", AS.check_odd_conditions(o))
    r, _ = injected_handle(pkg, hip, c)
    got = r.trace_ambient_occlusion(c.data.desc, o.dirs, radius=np.inf, bias=AS.BIAS)
    assert got.tobytes() == o.want.tobytes(), differ(got, o.want)
    r.close()


@pytest.fixture(scope="module")
def raster(pkg, hip):
    width, height = S.SUN_SIZE
    r = AS.raster_upload(pkg, hip.Renderer(width, height, 64, 16))
    sc = AS.raster_scene(pkg)
    r.pass_gbuffer(sc.desc)
    attrs, material, _, _ = r.read_gbuffer(want=("attrs", "material"))
    yield r, sc, attrs, material, AS.raster_want(pkg, sc.desc, attrs, material)
    r.close()


def test_rasterised_gbuffer_unfiltered_and_filtered(pkg, hip, raster):
    r, sc, attrs, material, want = raster
    for P, v in AS.check_raster_conditions(want).items():
        print("pattern %d: windows that accept all / some / only themselves =" % P, v)
    f = AS.FILTER
    for P, w in want.items():
        got = r.trace_ambient_occlusion(sc.desc, w.dirs, radius=f["radius"], bias=AS.BIAS)
        assert got.tobytes() == w.unfiltered.tobytes(), (P,) + differ(got, w.unfiltered)
        got = r.trace_ambient_occlusion(sc.desc, w.dirs, radius=f["radius"], bias=AS.BIAS, filter=True, normal_cos=f["normal_cos"], plane_dist=f["plane_dist"])
        assert got.tobytes() == w.filtered.tobytes(), (P,) + differ(got, w.filtered)
        assert (got[~w.covered] == 255).all()
        # thresholds that accept everything covered and finite: the plain mean over the window
        loose, _, _ = A.filtered(w.hits, w.covered, attrs, f["n_rays"], P, -2.0, 1e30)
        got = r.trace_ambient_occlusion(sc.desc, w.dirs, radius=f["radius"], bias=AS.BIAS, filter=True, normal_cos=-2.0, plane_dist=1e30)
        assert got.tobytes() == loose.tobytes() and (loose != w.filtered).any()
    assert r.ray_scene_info()[2] == 1


def test_device_variant_through_torch(pkg, hip, raster):
    import torch
    r, sc, _, _, want = raster
    width, height = S.SUN_SIZE
    f = AS.FILTER
    w = want[4]
    for filt, expect in ((False, w.unfiltered), (True, w.filtered)):
        out = torch.full((height * width + 64,), 0xCD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r.trace_ambient_occlusion_device(sc.desc, w.dirs, out.data_ptr(), radius=f["radius"], bias=AS.BIAS, filter=filt, normal_cos=f["normal_cos"], plane_dist=f["plane_dist"])
        r.flush()
        host = out.cpu().numpy()
        assert host[:height * width].tobytes() == expect.tobytes() and (host[height * width:] == 0xCD).all()
    assert r.trace_ambient_occlusion(sc.desc, w.dirs, radius=f["radius"], bias=AS.BIAS, read=False) is None     # left on the device
    assert r.trace_ambient_occlusion(sc.desc, w.dirs, radius=f["radius"], bias=AS.BIAS).tobytes() == w.unfiltered.tobytes()


@pytest.mark.parametrize("sharding", list(AS.SHARDS))
def test_shards_follow_the_rows_of_the_frame(pkg, hip, sharding):
    import torch
    c = AS.injected_case(pkg, 1000)
    width, height = S.SUN_SIZE
    r, rows = injected_handle(pkg, hip, c, AS.SHARDS[sharding])
    assert len(rows) < height
    for n, P in ((4, 4), (5, 2), (64, 4)):
        dirs = AS.table(c.master, n, P)
        _, _, want = AS.injected_want(c, n, P, c.radius, rows)
        got = r.trace_ambient_occlusion(c.data.desc, dirs, radius=c.radius, bias=AS.BIAS)
        assert got.shape == (len(rows), width) and got.tobytes() == want.tobytes(), (n, P) + differ(got, want)
        if sharding.startswith("rows") and n == 4:                                            # the range starts at row 3: the shard's own rows give another image
            hits, covered = A.image_hits(c.data.tris, c.attrs[rows], c.material[rows], dirs, n, P, c.radius, AS.BIAS, frame_rows=rows, defect="local_row", bvh=c.bvh)
            assert (A.result(hits, n, covered) != want).sum() >= 20
    # the filter needs the neighbours' rows: refused, nothing written
    out = torch.full((len(rows) * width,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for call in (lambda: r.trace_ambient_occlusion(c.data.desc, AS.table(c.master, 4, 4), filter=True),
                 lambda: r.trace_ambient_occlusion_device(c.data.desc, AS.table(c.master, 4, 4), out.data_ptr(), filter=True)):
        with pytest.raises(hip.ArcticError) as e:
            call()
        assert e.value.code == STATE
    r.flush()
    assert (out.cpu().numpy() == 0xCD).all()
    r.close()


def test_refusals_on_the_handle(pkg, hip):
    import torch
    c = AS.injected_case(pkg, 5)
    width, height = S.SUN_SIZE
    r = c.data.handle(pkg, hip, width, height)
    dirs = AS.table(c.master, 4, 2)
    with pytest.raises(hip.ArcticError) as e:
        r.trace_ambient_occlusion(c.data.desc, dirs)                                          # no G-buffer yet
    assert e.value.code == STATE
    r.write_gbuffer(c.attrs, c.material)
    good = r.trace_ambient_occlusion(c.data.desc, dirs, radius=c.radius, bias=AS.BIAS)
    out = torch.full((height * width,), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    bad_dirs = dirs.copy()
    bad_dirs[3, 3, 2] = np.nan
    for kw in (dict(n_rays=0), dict(n_rays=65), dict(pattern=3), dict(radius=0.0), dict(radius=np.nan), dict(bias=np.inf), dict(filter=2),
               dict(filter=True, normal_cos=np.nan), dict(filter=True, plane_dist=-1.0), dict(filter=True, plane_dist=np.nan), dict(dirs=bad_dirs)):
        kw = dict(kw)
        d = kw.pop("dirs", dirs if kw.get("n_rays", 4) <= 4 else np.zeros((4, 65, 3), np.float32))
        with pytest.raises(hip.ArcticError) as e:
            r.trace_ambient_occlusion_device(c.data.desc, d, out.data_ptr(), **kw)
        assert e.value.code == INVALID, kw
    with pytest.raises(hip.ArcticError) as e:
        r.trace_ambient_occlusion_device(c.data.desc, dirs, 0)
    assert e.value.code == INVALID
    r.flush()
    assert (out.cpu().numpy() == 0xCD).all()                                                  # a refused call writes nothing
    assert r.trace_ambient_occlusion(c.data.desc, dirs, radius=c.radius, bias=AS.BIAS).tobytes() == good.tobytes()
    r.close()


@pytest.mark.parametrize("refit", [0, 1])
def test_the_structure_is_reused_and_follows_the_scene(pkg, hip, refit):
    width, height = S.SUN_SIZE
    r = AS.raster_upload(pkg, hip.Renderer(width, height, 64, 16))
    r.set_option("ray_refit", refit)
    sc = AS.raster_scene(pkg)
    r.pass_gbuffer(sc.desc)
    attrs, material, _, _ = r.read_gbuffer(want=("attrs", "material"))
    dirs = pkg.renderer.ao_directions(4, 2, seed=1)
    first = r.trace_ambient_occlusion(sc.desc, dirs, radius=1.0, bias=AS.BIAS)
    assert r.trace_sun_visibility(sc.desc, 1e-3).shape == first.shape                         # the sun mask walks the same structure
    assert r.trace_ambient_occlusion(sc.desc, dirs, radius=1.0, bias=AS.BIAS).tobytes() == first.tobytes()
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info()[0] == 0
    # a box moves: the G-buffer in place stays as it is, the structure follows -- by a build, or by a refit under the option
    got = r.trace_ambient_occlusion(sc.moved, dirs, radius=1.0, bias=AS.BIAS)
    assert (r.ray_scene_info()[2], r.ray_refit_info()[0]) == ((1, 1) if refit else (2, 0))
    tris, prims = AS.raster_tris(pkg, sc.moved)
    hits, covered = A.image_hits(tris, attrs, material, dirs, 4, 2, 1.0, AS.BIAS, bvh=R.build_bvh(tris, prims))
    want = A.result(hits, 4, covered)
    assert got.tobytes() == want.tobytes(), differ(got, want)
    assert (got != first).sum() >= 5
    r.close()


def test_after_a_whole_frame_the_gbuffer_is_resolved_on_demand(pkg, hip):
    sc = pkg.scenes.config3(scale=0.1)
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    dirs = pkg.renderer.ao_directions(4, 4)
    r.pass_gbuffer(sc.desc)
    want = r.trace_ambient_occlusion(sc.desc, dirs, radius=2.0)
    soft = r.trace_ambient_occlusion(sc.desc, dirs, radius=2.0, filter=True)
    assert len(np.unique(want)) == 5 and (soft != want).any()
    r.close()
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    r.render_frame(sc.desc, sc.settings)                     # shaded from the visibility plane: no explicit G-buffer pass
    assert r.trace_ambient_occlusion(sc.desc, dirs, radius=2.0).tobytes() == want.tobytes()
    assert r.trace_ambient_occlusion(sc.desc, dirs, radius=2.0, filter=True).tobytes() == soft.tobytes()
    r.close()
