"""The paths of trace.hip that tests/test_gpu_ray_query.py's rays do not reach (needs an MI355X).

walk_wave chooses the walk per WAVE: the one that looks for 0 * inf when a valid lane carries an odd ray (a zero direction component, or one
whose reciprocal overflows: ray_reference.ray_odd), the plain one otherwise.  A quarter of soup_rays is odd, so a wave of them is next to never
plain.  Here the rays are laid out by wave (ray_reference.wave_rays): whole plain waves, whole odd waves, one odd lane at either end of a plain
wave, the edge rays of the definition in a plain and in an odd wave, a wave of invalid rays, a partial wave behind a workgroup boundary;
direction components at the subnormal bit patterns around 2^-128, where 1.0f / d stops being finite and the two walks meet; dead slots and empty
boxes under the plain walk; and arctic_trace_sun_visibility from an injected G-buffer of 52 x 37 pixels -- a width that is no multiple of 8, a
tile count that is no multiple of a workgroup's 4 -- under a general sun, a sun along an axis (every tile odd) and one a hair off an axis, on
the whole frame, on a row range and on interleaved bands.

Every comparison is of bytes against the numpy arbiter.  tests/test_ray_paths_inputs.py checks on the CPU that the inputs are what they are
taken for; the conditions that make a comparison mean something are asserted here again.  Which walk a wave takes is computed from ray_odd, not
read from the kernel, and printed per scene."""
import numpy as np
import pytest

import ray_reference as R
import ray_scenes as S
from test_ray_reference import TRI

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def handles(pkg, hip):
    """one 64 x 64 handle per scene, made on first use"""
    made = {}

    def get(key, data):
        if key not in made:
            made[key] = data.handle(pkg, hip)
        return made[key]
    yield get
    for r in made.values():
        r.close()


def trace_both_ways(r, desc, rays, want):
    """arctic_trace_rays from host memory and arctic_trace_rays_device between torch buffers, closest hit and any hit: the arbiter's bytes"""
    import torch
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    for any_hit in (False, True):
        got = r.trace_rays(desc, rays, any_hit=any_hit)
        differ = np.nonzero(got != want[any_hit])[0]
        assert got.tobytes() == want[any_hit].tobytes(), (any_hit, differ[:8].tolist(), got[differ[:4]].tolist(), want[any_hit][differ[:4]].tolist())
        d_hits = torch.full((len(rays) * 16,), 0xCD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        r.trace_rays_device(desc, d_rays.data_ptr(), len(rays), d_hits.data_ptr(), any_hit=any_hit)
        r.flush()
        assert d_hits.cpu().numpy().tobytes() == want[any_hit].tobytes(), any_hit


@pytest.mark.parametrize("layout", S.LAYOUTS)
@pytest.mark.parametrize("n_tris", S.TRI_COUNTS)
def test_wave_layouts(pkg, handles, n_tris, layout):
    c = S.wave_case(pkg, n_tris, layout)
    assert R.wave_walks(c.rays) == [w["walk"] for w in c.waves]
    seen = S.check_wave_conditions(c, n_tris)
    print(f"{n_tris} triangles, layout {layout}: {len(c.rays)} rays in {len(c.waves)} waves -- {seen['plain']} plain, {seen['odd']} odd, {seen['none']} without a valid lane; "
          f"{seen['hits']} rays hit, {seen['ties']} plain rays with a shared closest hit")
    r = handles(n_tris, c.data)
    trace_both_ways(r, c.data.desc, c.rays, c.want)
    got = r.trace_rays(c.data.desc, c.rays)
    for w in c.waves:
        for lane, k in w["edges"].items():
            at = w["start"] + lane
            if k != 13:
                assert got[at:at + 1].tobytes() == S.MISS_RECORD, (w["start"], lane, R.EDGE_NAMES[k])
            for near in (at - 1, at + 1):                                               # the lanes next to an edge lane are the arbiter's
                if w["start"] <= near < w["stop"]:
                    assert got[near].tobytes() == c.want[False][near].tobytes()
        if w["walk"] == "none":
            assert got[w["start"]:w["stop"]].tobytes() == S.MISS_RECORD * 64
    assert r.ray_scene_info()[2] == 1


@pytest.mark.parametrize("which", [1000, "tri"])
def test_subnormal_direction_components(pkg, handles, which):
    """|d| at 0, 1e-45 and 2^-128 (1.0f / d is infinite: the odd walk) and one step above, at 2^-127, at the largest subnormal and the smallest
    normal number (finite: the plain walk), of both signs on each axis, from origins in, one ulp outside and inside a triangle's box"""
    c = S.subnormal_case(pkg, which, TRI)
    r = handles(which, c.data)                                                           # (1000: the handle of the wave layouts)
    for name, patterns in (("plain", R.SUBNORMAL_PLAIN), ("odd", R.SUBNORMAL_ODD)):
        s = c.sets[name]
        assert set(R.wave_walks(s.rays)) == {name}
        S.check_subnormal_conditions(s, patterns)
        hit = s.want[False]["prim"] != NONE
        print(f"subnormal directions, {len(c.data.tris)} triangle(s), {name} walk: {len(s.rays) // 64} waves, {int((s.pattern >= 0).sum())} rays at the patterns, "
              f"{int(hit[s.pattern >= 0].sum())} of them hit")
        trace_both_ways(r, c.data.desc, s.rays, s.want)


@pytest.mark.parametrize("resplit", [False, True], ids=["refit", "resplit"])
def test_dead_slots_and_empty_boxes_under_the_plain_walk(pkg, hip, resplit):
    """an object leaves the finite numbers and comes back (tests/test_gpu_ray_refit.py's test_dead_and_back), traced with layout 1: its whole plain
    waves walk the dead slots and the empty boxes"""
    c, d = S.wave_case(pkg, 1000, 1), S.dead_case(pkg)
    S.check_dead_conditions(c, d)
    r = d.data.handle(pkg, hip)
    r.set_option("ray_refit", 1)
    trace_both_ways(r, d.here, c.rays, c.want)
    if resplit:
        r.ray_scene_resplit(d.away)
        assert r.ray_resplit_info()[0] == 1 and r.ray_resplit_info()[2] == 0
    trace_both_ways(r, d.away, c.rays, d.want)                                           # the arbiter for the triangles live at this moment
    nodes, _ = r.read_ray_structure()
    assert (nodes["bmin"][:, 0] == np.inf).any() and np.isfinite(nodes["bmin"][0]).all()   # empty boxes, below a root that is not empty
    trace_both_ways(r, d.here, c.rays, c.want)                                           # and back: a refit
    refits, refittable, _, _ = r.ray_refit_info()
    assert (refits, refittable) == ((1, 1) if resplit else (2, 1)) and r.ray_scene_info()[2] == 1   # refits, not builds
    r.close()


def sun_masks(pkg, hip, c, shard):
    """the masks of the three suns on one handle of the 52 x 37 frame: the whole of it (shard = {}) or a shard, which is fed its own rows"""
    width, height = S.SUN_SIZE
    rows = np.arange(height) if not shard else S.owned(pkg, height, shard)
    r = c.data.handle(pkg, hip, width, height, **shard)
    # (arctic_write_gbuffer takes a shard's rows on a sharded handle: no arctic_pass_gbuffer is needed for these cases)
    r.write_gbuffer(c.attrs[rows], c.material[rows])
    out = {}
    for name, s in c.suns.items():
        out[name] = r.trace_sun_visibility(s.desc, S.SUN_BIAS)
        assert out[name].shape == (len(rows), width) and out[name].dtype == np.uint8
    assert r.ray_scene_info()[2] == 1                                                    # (the sun is no part of the structure)
    r.close()
    return rows, out


def test_sun_visibility_from_an_injected_gbuffer(pkg, hip):
    c = S.sun_case(pkg)
    seen = S.check_sun_conditions(c)
    for name, n in seen.items():
        print(f"sun '{name}' on 52 x 37 (35 tiles): {n['plain']} tiles plain, {n['odd']} odd, {n['none']} without a valid lane; {n['occluded %']} % of the covered pixels occluded")
    _, masks = sun_masks(pkg, hip, c, {})
    bad = ~np.isfinite(c.attrs[..., 11:14]).all(-1)
    for name, s in c.suns.items():
        differ = np.argwhere(masks[name] != s.mask)
        assert masks[name].tobytes() == s.mask.tobytes(), (name, len(differ), differ[:8].tolist())
        assert (masks[name][(c.material == NONE) | bad] == 255).all()


@pytest.mark.parametrize("sharding", list(S.SHARDS))
def test_sun_visibility_on_shards(pkg, hip, sharding):
    c = S.sun_case(pkg)
    width, height = S.SUN_SIZE
    covered = []
    for shard in S.SHARDS[sharding]:
        rows, masks = sun_masks(pkg, hip, c, shard)
        covered += rows.tolist()
        for name, s in c.suns.items():
            walks = S.shard_walks(pkg, c, name, shard)
            assert ("plain" if name == "axis" else "odd") not in walks
            print(f"sun '{name}', {shard}: {len(rows)} rows in {len(walks)} tiles -- {walks.count('plain')} plain, {walks.count('odd')} odd, {walks.count('none')} without a valid lane")
            assert masks[name].tobytes() == s.mask[rows].tobytes(), (shard, name)
            assert len(np.unique(masks[name])) == 2                                      # both answers in every shard
    assert sorted(covered) == (list(range(5, 30)) if sharding.startswith("rows") else list(range(height)))
