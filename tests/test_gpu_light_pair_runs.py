"""ARCTIC_OPT_LIGHT_PAIR_RUNS on the device (needs an MI355X): the packed light loop walking its pair table in runs that skip a colour channel
against the float64 oracle, bit identity with the table in caller order where the exactness contract (shade.hip, accumulate_pair) promises it,
the caller's view (statistics, the scalar loop, a second update_lights) untouched by the layout, the counter that shows the runs are
walked, and the visibility-plane walk."""
import colorsys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-4   # the suite's bar on float LDR
W, H = 64, 48
BOX_LO, BOX_HI = (-15, 0, -7), (15, 12, 7)   # the world box of scenes.random_gbuffer
SETTINGS = (2, 2.2, 1.0)


def _hsv_lights(pkg, rng, hues):
    col = np.array([colorsys.hsv_to_rgb(h, 1.0, 1.0) for h in hues], np.float32).reshape(-1, 3) * 10.0
    lo, hi = np.asarray(BOX_LO, np.float32), np.asarray(BOX_HI, np.float32)
    return pkg.scene.make_lights(lo + rng.random((len(col), 3), dtype=np.float32) * (hi - lo), col)


def _light_sets(pkg):
    rng = np.random.default_rng(77)
    sets = {}
    # 13 lights the way the reference app draws them: an odd count, a mixed pair at a class boundary, the black partner
    sets["hsv13"] = pkg.scenes.random_lights(rng, 13, BOX_LO, BOX_HI)
    # 5 zero-R, 4 zero-G, 5 zero-B ... (hues inside the sextants whose named channel is 0)
    hues = [0.40, 0.45, 0.50, 0.55, 0.60] + [0.70, 0.80, 0.90, 0.95] + [0.05, 0.10, 0.20, 0.25, 0.30]
    l14 = _hsv_lights(pkg, rng, hues)
    masks = [[int(c == 0.0) for c in l["color"]] for l in l14]
    assert masks == [[1, 0, 0]] * 5 + [[0, 1, 0]] * 4 + [[0, 0, 1]] * 5
    # ... plus 2 white lights, shuffled in: 16 lights
    white = pkg.scene.make_lights(rng.uniform(BOX_LO, BOX_HI, (2, 3)), [[6, 6, 6], [9, 9, 9]])
    mixed = np.concatenate([l14, white])
    sets["mixed14+2"] = mixed[rng.permutation(len(mixed))]
    # 16 lights with the values that must NOT count as zero, a black light and one with a single channel
    odd = pkg.scenes.random_lights(rng, 16, BOX_LO, BOX_HI)
    odd["color"][0] = (0.0, 0.0, 0.0)
    odd["color"][3] = (-0.0, 4.0, 7.0)
    odd["color"][6] = (1e-45, 0.0, 8.0)
    odd["color"][9] = (0.0, 0.0, 12.0)
    odd["color"][12] = (5.0, -0.0, 1e-45)
    sets["odd16"] = odd
    return sets


class Inputs:
    pass


@pytest.fixture(scope="module")
def inputs(pkg, oracle):
    """one random G-buffer frame, no shadow map, and the float64 oracle's LDR per light set (computed once, never modified)"""
    I = Inputs()
    rng = np.random.default_rng(78)
    I.mats = [pkg.scenes.make_material_textures(rng, 32) for _ in range(3)]
    I.attrs, I.mat = pkg.scenes.random_gbuffer(rng, H, W, len(I.mats), coverage=0.9)
    I.desc = pkg.scene.SceneDesc(camera=dict(eye=(0, 6, 0), rotation=(-20, -90), aspect=W / H, fov_y=60.0, z_near_far=(0.1, 100.0)),
                                 ambient=0.05, sun=dict(position=(0, 30, 0), rotation=(-60, 20), color=(3, 3, 3)),
                                 objects=np.zeros(0, pkg.scene.OBJECT_DTYPE))
    I.sets = _light_sets(pkg)
    I.ref = {}
    o = oracle.Oracle(W, H, 0, 16)
    for m in I.mats:
        o.create_material(*m)
    for name, lights in I.sets.items():
        o.update_lights(lights)
        I.ref[name] = o.shade_gbuffer(I.desc, SETTINGS, I.attrs, I.mat, want=("ldr",))["ldr"]
        I.ref[name].setflags(write=False)
    o.close()
    return I


def _handle(hip, I, runs=1, path=2):
    r = hip.Renderer(W, H, 0, 16)
    for m in I.mats:
        r.create_material(*m)
    r.write_gbuffer(I.attrs, I.mat)
    r.set_option("keep_float_output", 1)
    r.set_option("light_path", path)
    r.set_option("light_pair_runs", runs)   # (always said, never left to the default)
    return r


def _shade(r, I, lights):
    r.update_lights(lights)
    r.pass_shade(I.desc, SETTINGS)
    return [x.copy() for x in r.read_output()]


def _same_bits(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


@pytest.mark.parametrize("name", ["hsv13", "mixed14+2", "odd16"])
def test_runs_against_the_float64_oracle(hip, inputs, name):
    """the packed loop forced, the runs on (the default) and off: float LDR within the suite's bar of the oracle; the two layouts within
    fp32 summation-order noise of each other"""
    I = inputs
    outs = {}
    for runs in (1, 0):
        r = _handle(hip, I, runs)
        outs[runs] = _shade(r, I, I.sets[name])
        r.close()
        err = float(np.abs(outs[runs][0] - I.ref[name]).max())
        print(f"light_pair_runs={runs} {name}: max |ldr - oracle| = {err:.3e}")
        assert err <= TOL
    assert outs[1][1].max() > 0
    assert np.abs(outs[1][0] - outs[0][0]).max() <= 3e-6   # (the bar test_light_paths_agree puts between the scalar and the packed loop)


def test_bit_identity_where_the_contract_promises_it(pkg, hip, inputs):
    """a list ordered by class (R, G, B, none; even counts but for the last), one and two lights: the table is the caller's, so RGBA8 and
    the float planes have the bits of the table without runs"""
    I = inputs
    rng = np.random.default_rng(79)
    ordered = _hsv_lights(pkg, rng, [0.40, 0.45, 0.55, 0.60] + [0.70, 0.95] + [0.05, 0.10, 0.20, 0.30])
    ordered = np.concatenate([ordered, pkg.scene.make_lights(rng.uniform(BOX_LO, BOX_HI, (3, 3)), [[6, 6, 6], [2, 9, 4], [1, 1, 8]])])
    one_class = _hsv_lights(pkg, rng, [0.05, 0.10, 0.15, 0.20, 0.25, 0.30, 0.12])
    lists = [ordered, one_class, I.sets["hsv13"][:1], I.sets["hsv13"][:2], I.sets["mixed14+2"][:2], I.sets["odd16"][:1]]
    a, b = _handle(hip, I, 1), _handle(hip, I, 0)
    for lights in lists:
        oa, ob = _shade(a, I, lights), _shade(b, I, lights)
        assert oa[1].max() > 0
        _same_bits(oa, ob)
    a.close(); b.close()


def test_the_callers_view_does_not_depend_on_the_layout(hip, inputs):
    """statistics and the scalar loop read the lights in caller order: unchanged by the option.  A second update_lights with other class
    sizes on one handle gives the frames of a fresh handle (stale run boundaries would show), and so does switching the option on a live handle."""
    I = inputs
    lights = I.sets["hsv13"]
    # the scalar loop
    a, b = _handle(hip, I, 1, path=1), _handle(hip, I, 0, path=1)
    _same_bits(_shade(a, I, lights), _shade(b, I, lights))
    # the counters of the packed loop's counting variant
    stats = []
    for r in (a, b):
        r.set_option("light_path", 2); r.set_option("count_light_evals", 1)
        r.pass_shade(I.desc, SETTINGS)
        stats.append(r.stats().copy())
        r.set_option("count_light_evals", 0)
    assert int(stats[0][5]) == int(stats[0][6]) * len(lights) and int(stats[0][7]) > 0
    np.testing.assert_array_equal(stats[0][5:10], stats[1][5:10])
    # ... and the runs ARE walked: every lit tile makes the table's skip-run pairs in a loop body that leaves a channel out, none without runs
    from importlib import import_module
    L = import_module("arctic_renderer_amd.binding").lib()
    n_pairs = (len(lights) + 1) // 2
    slots, masks, run_end = np.zeros(2 * n_pairs, np.uint32), np.zeros(n_pairs, np.uint32), np.zeros(3, np.uint32)
    assert L.arctic_light_pair_table(lights.ctypes.data, len(lights), 1, slots.ctypes.data, masks.ctypes.data, run_end.ctypes.data) == 0
    assert 0 < int(run_end[2]) < n_pairs                               # (a mixed pair and the partner's pair are general)
    assert int(stats[0][4]) == int(stats[0][9]) * int(run_end[2]) and int(stats[1][4]) == 0
    # one handle, different class sizes one after the other
    first = _shade(a, I, I.sets["mixed14+2"])
    second = _shade(a, I, lights)
    fresh = _handle(hip, I, 1)
    _same_bits(second, _shade(fresh, I, lights))
    _same_bits(first, _shade(fresh, I, I.sets["mixed14+2"]))
    # the option on a live handle rebuilds the table: b (0) becomes 1, a (1) becomes 0
    b.set_option("light_pair_runs", 1)
    b.pass_shade(I.desc, SETTINGS)
    _same_bits(second, [x.copy() for x in b.read_output()])
    a.set_option("light_pair_runs", 0)
    off = _shade(_handle(hip, I, 0), I, lights)
    a.pass_shade(I.desc, SETTINGS)
    _same_bits(off, [x.copy() for x in a.read_output()])
    a.close(); b.close(); fresh.close()


def test_whole_frames_through_the_visibility_plane(pkg, oracle, hip):
    """the same 13 lights over a floor of 24 x 24 quads, arctic_render_frame (k_material_vis): within the bar of the oracle's frame, runs on and off"""
    white, normal, mr = pkg.scenes.fallback_textures()
    floor = pkg.scenes.quad((-6, 0, 6), (12, 0, 0), (0, 0, -12), 24, 24) + (0,)
    rng = np.random.default_rng(80)
    lights = pkg.scenes.random_lights(rng, 13, (-6, 0.5, -6), (6, 4, 6))
    objs = pkg.scene.make_objects([(np.eye(4, dtype=np.float32), 0)])
    desc = pkg.scene.SceneDesc(camera=dict(eye=(0, 7, 7), rotation=(-45, -90), aspect=W / H, fov_y=60.0, z_near_far=(0.1, 100.0)),
                               ambient=0.05, sun=dict(position=(0, 10, 0), rotation=(-60, 0), color=(2, 2, 2)), objects=objs, point_lights=lights)
    outs = []
    for cls, runs in ((oracle.Oracle, None), (hip.Renderer, 1), (hip.Renderer, 0)):
        r = cls(W, H, 0, 16)
        r.create_material(white, normal, mr)
        r.create_mesh(*floor)
        r.update_lights(lights)
        if cls is hip.Renderer:
            r.set_option("keep_float_output", 1); r.set_option("light_path", 2); r.set_option("light_pair_runs", runs)
        img = r.render_frame(desc, SETTINGS)
        outs.append((img, r.read_output()[0].copy()))
        r.close()
    (oi, ol), (i1, l1), (i0, l0) = outs
    assert (oi[..., :3].max(-1) > 0).mean() > 0.5
    for img, ldr in ((i1, l1), (i0, l0)):
        err = float(np.abs(ldr - ol).max())
        print(f"whole frame, 13 lights: max |ldr - oracle| = {err:.3e}")
        assert err <= TOL
        assert np.abs(img.astype(np.int16) - oi.astype(np.int16)).max() <= 1
