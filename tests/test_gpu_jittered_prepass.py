"""The forward prepass under arctic_set_camera_jitter, bit for bit on every prepass path (needs an MI355X).

With a jitter that is not (0, 0) run_geometry replaces the one matrix that k_vertex, box_outside (cluster and vertex-block culling), k_setup and
the clipper, the binary64, int32 and int64 rasterisers, the block owners, the shard scissor and -- through the set-up records -- the resolve,
the level-of-detail plane and k_material_vis all read.  Every guarantee the suite holds for that code it holds with j = (0, 0), where the
matrix is not touched.  Here the same guarantees under the jitters of tests/jitter_cases.py: the oracle draws with the matrix numpy makes of
its own camera matrix (Oracle.set_proj_view; tests/test_oracle_jitter.py checks that hook on the CPU and that no case below is vacuous), and
all comparisons are by bytes over every pixel, nothing masked, unless a bar is named.  The groups a to g are jitter_cases' groups."""
from importlib import import_module

import numpy as np
import pytest

import jitter_cases as J
import test_gpu_cluster_cull as CL
import test_gpu_edge_cases as E
import test_gpu_texture_mips as M

pytestmark = pytest.mark.gpu
TOL = 1e-4      # the standing bar on the float LDR image (tests/test_gpu_parity.py)
U32 = np.uint32


@pytest.fixture(scope="module")
def cases(pkg, oracle):
    """cases(group): jitter_cases' list for a group, built once"""
    built = {}
    make = {"a": lambda: J.parity_cases(pkg), "b": lambda: J.ragged_cases(pkg), "c": lambda: J.shard_cases(pkg), "d": lambda: J.cull_cases(pkg),
            "e": lambda: J.clip_cases(pkg, oracle), "f": lambda: J.lod_cases(pkg, oracle), "g": lambda: J.state_cases(pkg)}

    def get(group):
        if group not in built:
            built[group] = make[group]()
        return built[group]
    return get


def handle(hip, sc, jitter=None, **options):
    r = sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights))
    for name, value in options.items():
        r.set_option(name, value)
    if jitter is not None:
        r.set_camera_jitter(*jitter)
    return r


def not_vacuous(case, oracle, j, jittered):
    n, differ, bits, ok = case.conditions(oracle, j, jittered)
    print(f"{case.id} {J.jid(j)}: {n} covered pixels, {differ:.4f} of them differ from the unjittered frame")
    assert ok, (case.id, j, n, differ, bits)


def bits_of(gbuffer):
    return [np.ascontiguousarray(x).view(U32) for x in gbuffer]


# ---- a. oracle parity -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(3), ids=lambda k: f"jitter{k}")
@pytest.mark.parametrize("i", range(len(J.PARITY)), ids=lambda i: "config%d-x%s" % J.PARITY[i][0][:2] + ("-owners" if J.PARITY[i][0][2] else ""))
def test_a_oracle_parity(pkg, oracle, hip, cases, i, k):
    """the 18 attributes, material, depth and triangle id are the oracle's under set_proj_view; the shadow map is that of a handle that never set
    a jitter; the float LDR stays within 1e-4 of the oracle's shading of its own jittered G-buffer; arctic_render_frame (visibility plane,
    k_material_vis) gives the bytes of pass_gbuffer + pass_shade; the 64-bit integer rasteriser (debug bit 5) gives the same planes"""
    case = cases("a")[i]
    sc, j = case.sc, case.jitters[k]
    o = J.oracle_prepass(oracle, sc, j)
    want = J.planes(o)
    not_vacuous(case, oracle, j, want)
    r = handle(hip, sc, j, keep_float_output=1, **case.options)
    r.pass_shadow_map(sc.desc); r.pass_gbuffer(sc.desc)
    J.same_planes(want, J.planes(r), f"{case.id} {J.jid(j)}")
    assert o.stats()[0] == r.stats()[0] and o.stats()[2] == r.stats()[2]          # the same number of set-up triangles (forward, shadow)
    shadow = None
    if sc.shadow_size:
        never = handle(hip, sc)
        never.pass_shadow_map(sc.desc)
        shadow = r.read_shadow_map().copy()
        assert (shadow < 1.0).any() and shadow.tobytes() == never.read_shadow_map().tobytes() == o.read_shadow_map().tobytes()
        never.close()
    o.pass_shade(sc.desc, sc.settings); r.pass_shade(sc.desc, sc.settings)
    ldr, hdr, rgba8 = (x.copy() for x in r.read_output())
    err = np.abs(ldr - o.read_output()[0]).max()
    print(f"{case.id} {J.jid(j)}: max |ldr - oracle| = {err:.3e}")
    assert np.isfinite(ldr).all() and err <= TOL, float(err)
    frame = r.render_frame(sc.desc, sc.settings)                                  # through the visibility plane
    assert frame.tobytes() == rgba8.tobytes()
    for a, b in zip((ldr, hdr, rgba8), r.read_output()):
        assert a.tobytes() == b.tobytes()
    J.same_planes(want, J.planes(r), f"{case.id} {J.jid(j)}, resolved after the frame")
    r.set_option("debug", 32)
    r.pass_shadow_map(sc.desc); r.pass_gbuffer(sc.desc)
    J.same_planes(want, J.planes(r), f"{case.id} {J.jid(j)}, integer rasteriser")
    if sc.shadow_size:
        assert r.read_shadow_map().tobytes() == shadow.tobytes()
    r.close(); o.close()


# ---- b. ragged and non-square frames ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(J.RAGGED_JITTERS)), ids=lambda k: J.jid(J.RAGGED_JITTERS[k]))
@pytest.mark.parametrize("i", range(len(J.RAGGED_SIZES)), ids=lambda i: "%dx%d" % J.RAGGED_SIZES[i])
def test_b_ragged_and_non_square_frames(pkg, oracle, hip, cases, i, k):
    """a triangle across each of the four sides, the corner and the one-axis jitters: these tell W from H and jx from jy"""
    case = cases("b")[i]
    j = case.jitters[k]
    outs = E.both(pkg, oracle, hip, *case.both_args, jitter=j, desc=case.desc)
    not_vacuous(case, oracle, j, bits_of(outs[0][2]))
    E.check(outs)


# ---- c. shards --------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_frames(pkg, hip, cases):
    """full(k): planes, shadow map, counts and two frames of the whole jittered frame on a handle of its own (cluster_cull 0)"""
    done = {}

    def get(k):
        if k not in done:
            case = cases("c")[0]
            done[k] = CL.prepass(hip, case.sc, 0, jitter=case.jitters[k])[0]
        return done[k]
    return get


@pytest.mark.parametrize("k", range(len(J.SHARD_JITTERS)), ids=lambda k: J.jid(J.SHARD_JITTERS[k]))
def test_c_the_full_frame_meets_the_oracle(pkg, oracle, hip, cases, full_frames, k):
    case = cases("c")[0]
    sc, j = case.sc, case.jitters[k]
    full = full_frames(k)
    o = J.oracle_prepass(oracle, sc, j)
    want = J.planes(o)
    not_vacuous(case, oracle, j, want)
    J.same_planes(want, full[:4], f"{case.id} {J.jid(j)}")
    assert full[4].tobytes() == o.read_shadow_map().tobytes() and full[5][0] == o.stats()[0] and full[5][2] == o.stats()[2]
    ref = o.render_frame(sc.desc, sc.settings)
    for frame in full[6:]:
        d = np.abs(frame.astype(np.int16) - ref.astype(np.int16))
        assert d.max() <= 1 and (d != 0).mean() < 2e-3                            # tests/test_gpu_parity.py's bar on a whole RGBA8 frame
    o.close()


@pytest.mark.parametrize("k", range(len(J.SHARD_JITTERS)), ids=lambda k: J.jid(J.SHARD_JITTERS[k]))
@pytest.mark.parametrize("kw", J.SHARDS, ids=lambda kw: "-".join(f"{a}{b}" for a, b in kw.items()))
def test_c_shards_equal_the_rows_of_the_full_jittered_frame(pkg, hip, cases, full_frames, kw, k):
    """the jitter is scaled by the FRAME's height whatever rows a handle owns: a shard's planes, shadow map and frames are the same rows of the
    full jittered frame of a second handle"""
    case = cases("c")[0]
    sc, j = case.sc, case.jitters[k]
    full = full_frames(k)
    shard, _ = CL.prepass(hip, sc, 3, jitter=j, **kw)
    if "row_begin" in kw:
        rows = np.arange(kw["row_begin"], kw["row_end"])
    else:
        rows = np.asarray(import_module("arctic_renderer_amd.sharding").owned_rows(sc.height, kw["shard"][0], kw["shard"][1], kw["band_rows"]))
    for name, a, b in zip(("attributes", "material", "depth", "triangle id"), full[:4], shard[:4]):
        assert b.shape[0] == len(rows) and a[rows].tobytes() == b.tobytes(), (name, kw, j, int((a[rows] != b).sum()))
    assert full[4].tobytes() == shard[4].tobytes()
    for a, b in zip(full[6:], shard[6:]):
        assert a[rows].tobytes() == b.tobytes(), ("frame", kw, j, int((a[rows] != b).sum()))


# ---- d. culling -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(J.CULL_CAMERAS)), ids=lambda i: "camera%d%s-%s" % (J.CULL_CAMERAS[i][0], "-far-plane" if J.CULL_CAMERAS[i][1] else "", J.jid(J.CULL_CAMERAS[i][2])))
def test_d_culling_tests_the_matrix_that_is_drawn(pkg, oracle, hip, cases, i):
    """cluster_cull 0, 1 and 3 give the same planes, shadow map, arctic_stats[:4] and frames under jitter, and the oracle's planes"""
    case = cases("d")[i]
    sc, j = case.sc, case.jitters[0]
    (off, c0), (setup_only, c1), (both, c3) = (CL.prepass(hip, sc, m, case.desc, jitter=j) for m in (0, 1, 3))
    CL.same(off, setup_only)
    CL.same(off, both)
    o = J.oracle_prepass(oracle, sc, j, case.desc)
    want = J.planes(o)
    not_vacuous(case, oracle, j, want)
    J.same_planes(want, off[:4], f"{case.id} {J.jid(j)}")
    assert off[4].tobytes() == o.read_shadow_map().tobytes() and off[5][0] == o.stats()[0] and off[5][2] == o.stats()[2]
    o.close()
    print(f"{case.id} {J.jid(j)}: forward pass skips {c3[0][1]} of {c3[0][0]} clusters and {c3[0][3]} of {c3[0][2]} vertex blocks")
    assert c0[0][1] == 0 and c0[0][3] == 0 and c1[0][3] == 0 and c1[0][1] == c3[0][1]
    if J.CULL_CAMERAS[i][0] % 4 != 1:                  # (far outside, the whole hall is a few dozen pixels wide and in view)
        assert c3[0][1] > 0 and c3[0][3] > 0           # a camera inside the hall has clusters and blocks behind it and beside its view


@pytest.mark.parametrize("k", range(len(J.SWEEP_JITTERS)), ids=lambda k: J.jid(J.SWEEP_JITTERS[k]))
def test_d_objects_on_the_scissors_sides(pkg, oracle, hip, k):
    """tests/test_gpu_cluster_cull.py's sweep under the corner jitters: a jitter of one pixel decides whether the quad is drawn.  The planes
    are the unculled handle's and the oracle's, and the number of clusters skipped is what box_outside skips under the DRAWN matrix: with the
    scissor's sides one pixel out and |j| <= 1 a test against the camera's matrix would still skip nothing that is drawn, so only that count
    tells the two matrices apart (jitter_cases.sweep_expected_skips)"""
    S = pkg.scenes
    j = J.SWEEP_JITTERS[k]
    found = J.sweep_tells_the_matrices_apart(pkg, oracle)
    assert all(found.get(side) for side in CL.SWEEP_SIDES), found
    sc = J.sweep_scene(pkg)
    ra, rb = [hip.Renderer(sc.width, sc.height, 0, 16) for _ in range(2)]
    for r, cull in ((ra, 0), (rb, 3)):
        sc.upload(r)
        r.set_option("cluster_cull", cull); r.set_option("debug", CL.COUNT)
        r.set_camera_jitter(*j)
    hits = seen = counted = 0
    for (side, d, desc, want, n_records), (skips, skips_camera, safe) in zip(J.oracle_sweep(pkg, oracle, j), J.sweep_expected_skips(pkg, oracle, j)):
        out = []
        for r in (ra, rb):
            r.pass_gbuffer(desc)
            out.append(J.planes(r) + [r.stats()[:2].copy()])
        CL.same(out[0], out[1])
        J.same_planes(want, out[0][:4], f"sweep {J.jid(j)}, {side} {d}")
        assert int(out[0][4][0]) == n_records
        n = rb.cull_counts(False)
        drawn = (out[0][3] != J.NO).any()
        assert not (drawn and n[1] == n[0])
        seen += int(drawn)
        hits += int(drawn and n[1] > 0)      # partly in, and some of its strips skipped
        if safe:                             # what is skipped is what box_outside skips under the DRAWN matrix (jitter_cases.sweep_expected_skips)
            assert int(n[0]) == 5 and int(n[1]) == skips, (side, d, j, n, skips, skips_camera)
            counted += int(skips != skips_camera)
    assert seen >= 12 and hits >= 4 and counted >= 8, (seen, hits, counted)
    ra.close(); rb.close()


# ---- e. clipping and the wide-coordinate path -------------------------------------------------------------------------------------------------------
CLIP_SCENES = ("near-plane-triangle", "clipped-into-three", "guard-band-3840x64")


@pytest.mark.parametrize("owner", [0, 1], ids=["atomics", "owners"])
@pytest.mark.parametrize("k", range(len(J.CLIP_JITTERS)), ids=lambda k: J.jid(J.CLIP_JITTERS[k]))
@pytest.mark.parametrize("i", range(len(CLIP_SCENES)), ids=lambda i: CLIP_SCENES[i])
def test_e_clipping_and_wide_coordinates(pkg, oracle, hip, cases, i, k, owner):
    """the clip list (a triangle through the camera's plane; triangles clipped into three, the record table not overflowed) and the int64
    rasteriser behind the guard band, drawn by atomics and by block owners"""
    case = cases("e")[i]
    assert case.name == CLIP_SCENES[i]
    j = case.jitters[k]
    outs = E.both(pkg, oracle, hip, *case.both_args, jitter=j, options={"raster_owner": owner}, desc=case.desc)
    not_vacuous(case, oracle, j, bits_of(outs[0][2]))
    assert int(outs[0][3].stats()[0]) == int(outs[1][3].stats()[0])               # the same number of set-up records
    E.check(outs)


# ---- f. level of detail -----------------------------------------------------------------------------------------------------------------------------
LOD_RECORDED = {"quad-ratio-4.0": 8.8e-5, "quad-ratio-0.5": 8.8e-5, "config3-x0.1": 1.2e-3}      # tests/test_gpu_texture_mips.py's maxima with j = 0


@pytest.mark.parametrize("k", range(len(J.LOD_JITTERS)), ids=lambda k: J.jid(J.LOD_JITTERS[k]))
def test_f_lod_plane_matches_float64(pkg, oracle, hip, cases, k):
    """the level-of-detail plane against the binary64 reference of tests/test_gpu_texture_mips.py evaluated with the jittered matrix; the gate
    is that file's LOD_TOL"""
    worst = {}
    for case, (_, expect) in zip(cases("f"), J.LOD_QUADS + ((None, None),)):
        sc, j = case.sc, case.jitters[k]
        r = M._mip_renderer(hip, sc, 1)
        r.set_camera_jitter(*j)
        e, got, want, cov = M._lod_error(pkg, sc, r, pv=J.proj_view(oracle, sc.desc, sc.width, sc.height, j))
        not_vacuous(case, oracle, j, None)
        if expect is not None:
            assert cov.all()
            assert np.abs(got - expect).max() <= M.LOD_TOL, (case.id, j, np.abs(got - expect).max())
        else:
            assert got[cov].max() > got[cov].min() + 1.0
        worst[case.name] = float(e)
        r.close()
    print(f"lod plane under {J.jid(case.jitters[k])}, max |delta lambda| against binary64:", {n: f"{v:.3e} (j = 0: {LOD_RECORDED[n]:.1e})" for n, v in worst.items()})
    assert max(worst.values()) <= M.LOD_TOL, worst


# ---- g. state ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fresh_frames(pkg, hip, cases):
    """fresh(j): the frame of a handle of its own that only ever had jitter j (None: arctic_set_camera_jitter never called)"""
    done = {}

    def get(j):
        if j not in done:
            sc = cases("g")[0].sc
            r = handle(hip, sc, j)
            done[j] = r.render_frame(sc.desc, sc.settings).copy()
            r.close()
        return done[j]
    return get


@pytest.mark.parametrize("in_flight", [1, 2, 3])
def test_g_a_sequence_of_jitters_with_frames_in_flight(pkg, hip, cases, fresh_frames, in_flight):
    """j0, j1, (0, 0), j0 on one handle with cluster_cull 3, every frame enqueued without waiting for the one before (the handle's table sets
    alternate): each frame is that of a fresh handle that only ever had that jitter, the (0, 0) frame that of a handle that never made the call"""
    import torch
    sc = cases("g")[0].sc
    j0, j1 = cases("g")[0].jitters
    sequence = (j0, j1, (0.0, 0.0), j0)
    r = handle(hip, sc, cluster_cull=3, frames_in_flight=in_flight)
    outs = [torch.empty((sc.height, sc.width, 4), dtype=torch.uint8, device="cuda") for _ in sequence]
    for out, j in zip(outs, sequence):                      # no flush inside the loop: frames are in flight
        r.set_camera_jitter(*j)
        r.render_frame_device(sc.desc, sc.settings, out.data_ptr())
    r.flush()
    for n, (out, j) in enumerate(zip(outs, sequence)):
        want = fresh_frames(None if J.is_zero(j) else j)
        got = out.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (in_flight, n, j, int((got != want).sum()))
    assert len({fresh_frames(j).tobytes() for j in (j0, j1, None)}) == 3
    r.close()


def test_g_a_jitter_set_between_the_passes_changes_nothing(pkg, hip, cases, fresh_frames):
    """the jitter is read when the prepass is enqueued: arctic_set_camera_jitter between pass_gbuffer and pass_shade changes no byte of that frame"""
    sc = cases("g")[0].sc
    j0, j1 = cases("g")[0].jitters
    a, b = (handle(hip, sc, j0, keep_float_output=1) for _ in range(2))
    for r in (a, b):
        r.pass_shadow_map(sc.desc); r.pass_gbuffer(sc.desc)
    a.set_camera_jitter(*j1)
    for r in (a, b):
        r.pass_shade(sc.desc, sc.settings)
    for x, y in zip(a.read_output(), b.read_output()):
        assert x.tobytes() == y.tobytes()
    J.same_planes(J.planes(b), J.planes(a), "jitter set between the passes")
    rgba8 = a.read_output(want=("rgba8",))[2]
    assert rgba8.tobytes() == fresh_frames(j0).tobytes() and rgba8.tobytes() != fresh_frames(j1).tobytes()
    a.close(); b.close()
