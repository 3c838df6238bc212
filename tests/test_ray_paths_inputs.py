"""The inputs of tests/test_gpu_ray_paths.py, checked on the CPU: every set of rays gives the same bytes in the numpy arbiter's loop over every
triangle, in its pruned walk and in the library's host arbiter (arctic_trace_triangles, with and without its structure), and every set IS what
the device test takes it for -- each wave holds the kinds of rays its layout claims (so the device runs the walk the test means it to run), rays
hit and miss, closest hits are shared, edge lanes miss, origins lie in box planes.  A device test whose input lost one of these properties
would pass for the wrong reason."""
import numpy as np
import pytest

import ray_reference as R
import ray_scenes as S
from test_ray_reference import TRI

F = np.float32


def all_arbiters_agree(pkg, data, rays, want):
    """numpy's loop (want) = numpy's walk = the host arbiter's walk = the host arbiter's loop, in bytes"""
    bvh = R.build_bvh(data.tris, data.prims)
    for any_hit in (False, True):
        assert R.walk(bvh, rays, any_hit=any_hit)[0].tobytes() == want[any_hit].tobytes()
        for brute in (False, True):
            h = pkg.renderer.trace_triangles(data.tris, rays, any_hit=any_hit, brute=brute)   # (its prims are array indices)
            hit = h["prim"] != R.NO_PRIM
            if not any_hit:
                h["prim"][hit] = data.prims[h["prim"][hit]]
            assert h.tobytes() == want[any_hit].tobytes(), (any_hit, brute)


def lane_kinds(c):
    """per ray of a wave case: the lane's kind as the layout states it"""
    return np.array([k if isinstance(k, str) else "edge" for w in c.waves for k in w["lanes"]])


@pytest.mark.parametrize("layout", S.LAYOUTS)
@pytest.mark.parametrize("n_tris", S.TRI_COUNTS)
def test_wave_layouts_hold_what_they_claim(pkg, n_tris, layout):
    c = S.wave_case(pkg, n_tris, layout)
    rays, kinds = c.rays, lane_kinds(c)
    valid, odd = R.ray_valid(rays), R.ray_odd(rays)
    assert len(rays) == len(kinds) == {1: 529, 2: 145}[layout] and len(c.waves) == {1: 9, 2: 3}[layout]
    assert [w["stop"] - w["start"] for w in c.waves] == [len(w) for w in R.WAVE_LAYOUTS[layout]]
    assert [w["start"] for w in c.waves] == [64 * k for k in range(len(c.waves))]
    # every lane is of its kind ...
    assert (valid & ~odd)[kinds == "plain"].all() and (valid & odd)[kinds == "odd"].all()
    assert (~valid & ~odd)[kinds == "bad_plain"].all() and (~valid & odd)[kinds == "bad_odd"].all()
    assert (kinds == "bad_plain").sum() == (kinds == "bad_odd").sum() == (32 if layout == 1 else 0)
    # ... so every wave takes the walk the layout means it to take
    assert R.wave_walks(rays) == [w["walk"] for w in c.waves]
    assert [w["walk"] for w in c.waves] == {1: ["plain", "odd", "odd", "odd", "plain", "none", "plain", "plain", "plain"], 2: ["plain", "odd", "odd"]}[layout]
    for w in c.waves:
        for lane, k in w["edges"].items():
            r = rays[w["start"] + lane]
            assert R.edge_records(r)[k].tobytes() == r.tobytes()                        # the record's defect is in it: writing it again changes nothing
            assert bool(valid[w["start"] + lane]) == (k >= R.EDGE_INVALID)
    if layout == 1:
        assert c.waves[4]["edges"] == {0: 0, 1: 5, 2: 3, 31: 8, 32: 11, 63: 12}
        assert odd[c.waves[4]["start"] + 0] and odd[c.waves[4]["start"] + 1]             # invalid AND odd lanes in a wave that has to stay plain
    else:
        assert sorted(c.waves[0]["edges"].values()) == sorted(c.waves[1]["edges"].values()) == list(range(14))
        assert kinds[-17:].tolist() == ["plain"] * 16 + ["odd"]


@pytest.mark.parametrize("layout", S.LAYOUTS)
@pytest.mark.parametrize("n_tris", S.TRI_COUNTS)
def test_wave_layouts_in_every_arbiter_and_their_conditions(pkg, n_tris, layout):
    c = S.wave_case(pkg, n_tris, layout)
    all_arbiters_agree(pkg, c.data, c.rays, c.want)
    S.check_wave_conditions(c, n_tris)


def test_wave_layouts_tell_the_walks_apart(pkg):
    """a plain walk that prunes at equality, and an odd ray in a walk that does not look for 0 * inf, change results of these very rays"""
    for n_tris in S.TRI_COUNTS:
        for layout in S.LAYOUTS:
            c = S.wave_case(pkg, n_tris, layout)
            bvh = R.build_bvh(c.data.tris, c.data.prims)
            flawed = R.walk(bvh, c.rays, defect="nan_prunes")[0]
            differ = flawed != c.want[False]
            assert differ.sum() >= 2 and R.ray_odd(c.rays)[differ].all(), (n_tris, layout)
    # ... in waves that take the plain walk (a plain ray in an odd wave is tested by the other node test).  Four triangles are one leaf under a
    # root with an extent on every axis: no node test of that scene ever meets equality
    for n_tris in (1, 5, 1000):
        for layout in S.LAYOUTS:
            c = S.wave_case(pkg, n_tris, layout)
            differ = R.walk(R.build_bvh(c.data.tris, c.data.prims), c.rays, defect="prune_nonstrict")[0] != c.want[False]
            in_plain_wave = np.concatenate([np.full(w["stop"] - w["start"], w["walk"] == "plain") for w in c.waves])
            assert (differ & in_plain_wave).sum() >= 8, (n_tris, layout)


@pytest.mark.parametrize("which", [1000, "tri"])
def test_subnormal_directions(pkg, which):
    c = S.subnormal_case(pkg, which, TRI)
    for name, patterns in (("plain", R.SUBNORMAL_PLAIN), ("odd", R.SUBNORMAL_ODD)):
        s = c.sets[name]
        all_arbiters_agree(pkg, c.data, s.rays, s.want)
        assert len(s.rays) % 64 == 0 and set(R.wave_walks(s.rays)) == {name}             # whole waves, each of the one walk
        S.check_subnormal_conditions(s, patterns)
        bits = np.abs(s.rays["direction"]).view(np.uint32)
        real = s.pattern >= 0
        assert ((bits[real] == s.pattern[real, None]).sum(1) == 1).all()                # one component at the pattern, the others general
        assert (np.abs(s.rays["direction"][real]) > 0.5).sum(1).tolist() == [2] * int(real.sum())
        assert np.signbit(s.rays["direction"][real]).any(0).all() and (~np.signbit(s.rays["direction"][real])).any(0).all()
    with np.errstate(over="ignore"):
        assert np.isfinite(F(1) / c.sets["plain"].rays["direction"]).all()
    # an odd ray of this set in a walk that does not look for the NaN is pruned where the definition says "no constraint"
    odd = c.sets["odd"]
    assert R.walk(R.build_bvh(c.data.tris, c.data.prims), odd.rays, defect="nan_prunes")[0].tobytes() != odd.want[False].tobytes()


def test_the_injected_gbuffer_and_its_suns(pkg):
    c = S.sun_case(pkg)
    width, height = S.SUN_SIZE
    assert (width % 8, (-(-width // 8) * -(-height // 8)) % 4) == (4, 3)               # a tail in x, and a workgroup of 4 tiles that is not full
    mat = c.material
    assert (mat[8:16, 16:24] == R.NO_PRIM).all() and (mat[20] == R.NO_PRIM).all() and 0.10 <= (mat == R.NO_PRIM).mean() <= 0.25
    world, nrm = c.attrs[..., 11:14].reshape(-1, 3), c.attrs[..., 8:11].reshape(-1, 3)
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)
    bad = ~np.isfinite(world).all(1)
    assert (bad & c.covered).sum() == 6 and np.isnan(world).any() and np.isposinf(world).any() and np.isneginf(world).any()
    S.check_sun_conditions(c)
    for name, s in c.suns.items():
        cov = c.covered & ~bad
        loop = S.arbiter(c.data, s.rays[cov])                                            # the walk that made the mask is the loop ...
        assert (np.where(loop[True]["prim"] == 0, 0, 255) == s.mask.reshape(-1)[cov]).all()
        all_arbiters_agree(pkg, c.data, s.rays[cov], loop)                               # ... and the host arbiter's, with its structure and without
        assert (s.mask.reshape(-1)[~c.covered | bad] == 255).all()


def test_the_shards_cover_every_row_once(pkg):
    width, height = S.SUN_SIZE
    for name, shards in S.SHARDS.items():
        rows = np.concatenate([S.owned(pkg, height, s) for s in shards])
        if name.startswith("bands"):
            assert sorted(rows.tolist()) == list(range(height)), name
        else:
            assert rows.tolist() == list(range(5, 30)) and 5 % 8 and 30 % 8             # the range cuts tiles at both ends


def test_the_scene_with_an_object_gone(pkg):
    c, d = S.wave_case(pkg, 1000, 1), S.dead_case(pkg)
    S.check_dead_conditions(c, d)
    all_arbiters_agree(pkg, d.data, c.rays, d.want)                                      # (the host arbiter is given the dead triangles too)
    live = np.isfinite(d.data.tris).all(1)
    for any_hit in (False, True):                                                        # dead triangles are never hit: the live ones alone give the same
        assert R.brute(d.data.tris[live], c.rays, any_hit=any_hit, prims=d.data.prims[live]).tobytes() == d.want[any_hit].tobytes()
    assert d.here.objects["trs"][0, 12] == c.data.desc.objects["trs"][0, 12] and d.away.objects["trs"][0, 12] == np.inf


def test_tile_walks_by_hand():
    # 3 rows of 9 pixels that begin at row 6 of their tile row: 2 x 2 tiles; pixel (0, 8) lies in tile (0, 1), pixel (2, 0) -- tile-row pixel 8 -- in (1, 0)
    rays = R.make_rays(np.zeros((27, 3)), np.tile([1.0, 2.0, 3.0], (27, 1)))
    rays["direction"][8, 1] = 0                                                          # an odd ray at (0, 8)
    active = np.zeros(27, bool)
    active[[8, 18]] = True
    assert R.tile_walks(rays, active, 3, 9, 6) == ["none", "odd", "plain", "none"]
    assert R.tile_walks(rays, active, 3, 9) == ["plain", "odd"]                          # from the top of a tile row: one tile row
    rays["origin"][8, 2] = np.nan                                                        # an invalid lane does not count
    assert R.tile_walks(rays, active, 3, 9, 6) == ["none", "none", "plain", "none"]
    active[:] = True                                                                     # ... and an odd ray that is not active (no geometry) does not either
    active[8] = False
    assert R.tile_walks(rays, active, 3, 9, 6) == ["plain", "plain", "plain", "plain"]


def test_every_shard_sees_both_answers_and_walks_as_the_frame_does(pkg):
    c = S.sun_case(pkg)
    width, height = S.SUN_SIZE
    for shards in S.SHARDS.values():
        for shard in shards:
            rows = S.owned(pkg, height, shard)
            for name, s in c.suns.items():
                assert len(np.unique(s.mask[rows])) == 2
                walks = S.shard_walks(pkg, c, name, shard)
                assert len(walks) == 7 * -(-(len(rows) + shard.get("row_begin", 0) % 8) // 8)
                assert ("plain" if name == "axis" else "odd") not in walks and walks.count("odd" if name == "axis" else "plain") >= 7
    assert "none" in S.shard_walks(pkg, c, "axis", S.SHARDS["rows 5..30"][0])            # the tile without geometry lies in rows 8..15
