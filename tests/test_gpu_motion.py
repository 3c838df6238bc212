"""arctic_motion_vectors(_device), arctic_motion_reset / _info, arctic_accumulate_ambient_occlusion_motion(_device) and
arctic_pass_ray_effects_motion on the device (needs an MI355X), against the numpy definition of tests/motion_reference.py BY BYTES, no pixel left
out: k_motion on the rasterised scene of tests/hit_scenes.py (four object entries over two meshes, one missing mesh, one skipped triangle) --
bary3 and source4 first, held against arctic_read_gbuffer, then prev_world4 and velocity2 of every call --, an independent float64 check of the
moved box, a skinned bar and a morphed quad of more than 256 vertices (the snapshots), k_ao_accumulate_motion on the analytic moving-box
sequences of tests/motion_scenes.py, and the other cases: lists that shrink or swap a mesh, reset and resize, shards, the device form, the
refusals, the one call against the calls by hand, and a handle that never makes these calls."""
import numpy as np
import pytest

import ao_history_reference as HR
import ao_history_scenes as HS
import hit_scenes
import motion_reference as MR
import motion_scenes as MS
import ray_scenes as S
import test_gpu_ao_history as TH
import test_gpu_compose as TC
import test_gpu_skinning as TS

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, STATE = -1, -4
SENTINEL = F(-77.0)
PAD = 16


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got.view(np.uint8).reshape(got.shape[0], got.shape[1], -1) != want.view(np.uint8).reshape(got.shape[0], got.shape[1], -1)).any(-1))
        raise AssertionError((what, len(bad[0]), [(int(y), int(x), got[y, x].tolist(), want[y, x].tolist()) for y, x in zip(bad[0][:3], bad[1][:3])]))


# ---- the restatement: everything from bary3 and source4, no rasteriser ---------------------------------------------------------------------------
def seen(desc, positions):
    """what a motion call saw: the scene's objects, the (n, 3) positions of every mesh in use, and the camera's matrix"""
    return dict(objects=desc.objects.copy(), positions=positions, desc=desc)


def restate(pkg, bary, src, rows, now, before, W, H, defect=None, current_positions=None):
    """prev_world4 and velocity2 of a call from its bary3 and source4: `now` and `before` are what this call and the previous one saw (seen();
    before None: M is empty); rows: the frame's rows the handle owns, in its order"""
    n_rows = len(rows)
    pw4, vel = np.zeros((n_rows, W, 4), F), np.zeros((n_rows, W, 2), F)
    if before is None:
        return pw4, vel
    P = pkg.renderer.frame_constants(before["desc"])[0]
    xy = np.stack(np.broadcast_arrays(np.arange(W)[None, :], np.asarray(rows)[:, None]), -1)
    obj = src[..., 0]
    for o in np.unique(obj[obj != MR.NO_OBJECT]):
        o = int(o)
        mesh = int(now["objects"][o]["mesh_idx"])
        if not (o < len(before["objects"]) and int(before["objects"][o]["mesh_idx"]) == mesh):
            continue
        sel = obj == o
        trs = (now if defect == "current trs" else before)["objects"][o]["trs"]
        pos = (current_positions if defect == "current positions" else before["positions"])[mesh]
        q = pos[src[sel][:, 1:4]]
        n = int(sel.sum())
        a, b = MR.motion(bary[sel], np.ones(n, bool), np.tile(trs, (n, 1)), q, xy[sel], P, W, H, defect)
        pw4[sel], vel[sel] = a, b
    return pw4, vel


def gbuffer_from(pkg, bary, src, now, vertices):
    """the 18 attributes of every pixel from bary3 and source4: numpy's vertex attributes of the CURRENT scene, interpolated"""
    lpv = pkg.renderer.frame_constants(now["desc"])[1]
    attrs = np.zeros(bary.shape[:2] + (18,), F)
    obj = src[..., 0]
    for o in np.unique(obj[obj != MR.NO_OBJECT]):
        sel = obj == o
        a = MR.vertex_attributes(now["objects"][int(o)]["trs"], lpv, vertices[int(now["objects"][int(o)]["mesh_idx"])])
        ix = src[sel][:, 1:4]
        attrs[sel] = MR.interpolate(bary[sel], a[ix[:, 0]], a[ix[:, 1]], a[ix[:, 2]])
    return attrs


def draw_and_call(r, desc):
    """a prepass and the host form -> (prev_world4, velocity2, bary3, source4, attrs, material)"""
    r.pass_gbuffer(desc)
    out = r.motion_vectors(desc)
    attrs, material, _, _ = r.read_gbuffer()
    return out + (attrs, material)


# ---- the rasterised scene of the hit tests --------------------------------------------------------------------------------------------------------
def hit_handle(pkg, hip, size, **kw):
    g = hit_scenes.geometry(pkg)
    r = hip.Renderer(size[0], size[1], 64, 16, **kw)
    r.create_material(*pkg.scenes.make_material_textures(np.random.default_rng(9), 32))
    for v, i in g.meshes:
        r.create_mesh(v, i, 0)
    return r


def hit_desc(pkg, objects, size):
    d = hit_scenes.description(pkg, objects)
    return pkg.scenes.SceneDesc(camera=dict(d.camera, aspect=size[0] / size[1]), ambient=d.ambient, sun=d.sun, objects=objects)


def hit_positions(pkg):
    return {k: v["position"] for k, (v, _) in enumerate(hit_scenes.geometry(pkg).meshes)}


@pytest.fixture(scope="module")
def three_calls(pkg, hip):
    """per size: the three calls of the rasterised scene -- `objects`, `moved`, `moved` again -- as draw_and_call returns them"""
    out = {}
    g = hit_scenes.geometry(pkg)
    for size in HS.SIZES:
        r = hit_handle(pkg, hip, size)
        descs = [hit_desc(pkg, g.objects, size), hit_desc(pkg, g.moved, size), hit_desc(pkg, g.moved, size)]
        out[tuple(size)] = ([draw_and_call(r, d) for d in descs], descs, r.motion_info())
        r.close()
    return out


@pytest.mark.parametrize("size", HS.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rasterised_scene_every_call_equals_numpy_by_bytes(pkg, three_calls, size):
    W, H = size
    g = hit_scenes.geometry(pkg)
    calls, descs, info = three_calls[tuple(size)]
    pos, vertices = hit_positions(pkg), {k: v for k, (v, _) in enumerate(g.meshes)}
    before = None
    for k, ((pw4, vel, bary, src, attrs, material), desc) in enumerate(zip(calls, descs)):
        now = seen(desc, pos)
        covered = material != HR.NO_MATERIAL
        # bary3 and source4 are held first: they reproduce the G-buffer
        assert ((src[..., 0] != MR.NO_OBJECT) == covered).all() and not bary[~covered].any() and not src[~covered][:, 1:].any()
        same(gbuffer_from(pkg, bary, src, now, vertices), attrs, (size, k, "the G-buffer from bary3 and source4"))
        objects = set(np.unique(src[covered][:, 0]).tolist())
        assert objects == {0, 2, 3}, objects                                     # the scene's numbering: entry 1 has no mesh and no pixel
        # then the motion planes
        want_pw, want_vel = restate(pkg, bary, src, np.arange(H), now, before, W, H)
        same(pw4, want_pw, (size, k, "prev_world4"))
        same(vel, want_vel, (size, k, "velocity2"))
        if k == 0:
            assert not pw4.any() and not vel.any()                               # M was empty
        else:
            assert (pw4[covered][:, 3] == 2).all() and not pw4[~covered].any()
        if k == 1:                                                               # what moved has a velocity, and every defect would show
            box = src[..., 0] == 0
            assert box.sum() >= 100 and (np.abs(vel[box]).max(-1) > 0.5).mean() > 0.9
            for defect in ("current trs", "B permuted", "velocity sign", "y not flipped"):
                bad = restate(pkg, bary, src, np.arange(H), now, before, W, H, defect)
                assert bad[0].tobytes() + bad[1].tobytes() != want_pw.tobytes() + want_vel.tobytes(), defect
        if k == 2:                                                               # nothing changed: the point is where it is, bit for bit
            assert pw4[covered][:, :3].tobytes() == attrs[covered][:, 11:14].tobytes()
            # ... and it is seen where it was: the rasteriser snaps a vertex to 1/256 pixel, so the surface point under a pixel's centre projects
            # back within 1/512 pixel of it per axis, and fp32 adds a few 2^-24 * 96 to sx: 1/256 holds both
            assert (np.abs(vel[covered]) <= 1.0 / 256).all(), float(np.abs(vel[covered]).max())
        before = now
    assert info[1:] == (3, 0, 3)                                                 # three launches of k_motion, no snapshot for a rigid scene


def test_the_moved_box_against_float64(pkg, three_calls):
    """call 2, the pixels of the moved box: pw against T_prev * inverse(T_cur) * w in float64, per component within 32 * 2^-24 * M, M the largest
    magnitude among the terms of the two products (about a dozen roundings of at most half an ulp of M on each side).  The figure is printed;
    when this was written: 874 pixels, worst error 4.5 * 2^-24 * M"""
    g = hit_scenes.geometry(pkg)
    pw4, _, _, src, attrs, _ = three_calls[tuple(HS.SIZES[0])][0][1]
    box = src[..., 0] == 0
    w = attrs[box][:, 11:14].astype(np.float64)
    Tp = g.objects[0]["trs"].astype(np.float64).reshape(4, 4).T
    Tc = g.moved[0]["trs"].astype(np.float64).reshape(4, 4).T
    inv = np.linalg.inv(Tc)
    w1 = np.concatenate([w, np.ones((len(w), 1))], 1)
    x = w1 @ inv.T
    want = (x @ Tp.T)[:, :3]
    M = np.maximum(np.abs(inv[None, :3, :] * w1[:, None, :]).max((1, 2)), np.abs(Tp[None, :3, :] * x[:, None, :]).max((1, 2)))
    err = np.abs(pw4[box][:, :3].astype(np.float64) - want)
    print("moved box:", int(box.sum()), "pixels, worst error / (2^-24 M):", float((err / (2.0 ** -24 * M[:, None])).max()))
    assert box.sum() >= 100 and (err <= 32 * 2.0 ** -24 * M[:, None]).all(), float((err / (2.0 ** -24 * M[:, None])).max())


# ---- deformed meshes: the snapshots ---------------------------------------------------------------------------------------------------------------
SIZE = HS.SIZES[0]


def bar_scene(pkg, hip, morph=False):
    """a skinned bar of 1014 vertices over a floor (test_gpu_skinning's), optionally with two morph targets -> (handle, desc, bar, deltas)"""
    bar = TS.Bar(pkg)
    mats, meshes, desc, _ = TS.make_scene(pkg, bar)
    desc = pkg.scenes.SceneDesc(camera=dict(desc.camera, aspect=SIZE[0] / SIZE[1]), ambient=desc.ambient, sun=desc.sun, objects=desc.objects)
    r = hip.Renderer(SIZE[0], SIZE[1], 64, 16)
    for m in mats:
        r.create_material(*m)
    for v, i, mat in meshes:
        r.create_mesh(v, i, mat)
    r.set_mesh_skin(0, bar.skin, bar.n_joints)
    deltas = None
    if morph:
        rng = np.random.default_rng(31)
        deltas = np.zeros((2, len(bar.vertices)), pkg.scene.MORPH_DELTA_DTYPE)
        deltas["position"] = rng.normal(0, 0.08, (2, len(bar.vertices), 3)).astype(F)
        r.set_mesh_morph_targets(0, deltas)
    assert len(bar.vertices) >= 300
    return r, desc, bar, deltas, meshes[1][0]["position"]


def judge_sequence(pkg, r, desc, shapes, what):
    """shapes: per call the (n, 3) positions mesh 0 has when the call is made (set by the caller through `apply`) or None = nothing changed"""
    W, H = SIZE
    before, last = None, None
    for k, (apply, pos0, floor) in enumerate(shapes):
        apply()
        pw4, vel, bary, src, attrs, material = draw_and_call(r, desc)
        now = seen(desc, {0: pos0, 1: floor})
        want_pw, want_vel = restate(pkg, bary, src, np.arange(H), now, before, W, H)
        same(pw4, want_pw, (what, k, "prev_world4"))
        same(vel, want_vel, (what, k, "velocity2"))
        covered = material != HR.NO_MATERIAL
        bar = src[..., 0] == 0
        assert bar.sum() >= 100, (what, k, int(bar.sum()))
        if before is not None and before["positions"][0].tobytes() == pos0.tobytes():   # no change: pw == w
            assert pw4[covered][:, :3].tobytes() == attrs[covered][:, 11:14].tobytes(), (what, k)
        elif before is not None:                                                 # a change: the snapshot is what was read, not the current pose
            bad = restate(pkg, bary, src, np.arange(H), now, before, W, H, "current positions", {0: pos0, 1: floor})
            assert bad[0].tobytes() != want_pw.tobytes(), (what, k)
            assert (pw4[bar][:, :3] != attrs[bar][:, 11:14]).any(-1).mean() > 0.5
        before = now


def test_a_skinned_bar_reads_the_previous_pose(pkg, hip):
    r, desc, bar, _, floor = bar_scene(pkg, hip)
    A, B = bar.pose(25.0), bar.pose(-30.0, (0.2, 0.1, 0.0))
    posed = lambda m: pkg.renderer.skin_vertices(bar.vertices, bar.skin, m)["position"]
    judge_sequence(pkg, r, desc, [(lambda: r.set_mesh_pose(0, A), posed(A), floor), (lambda: r.set_mesh_pose(0, B), posed(B), floor), (lambda: None, posed(B), floor)], "skinned")
    assert r.motion_info()[1:] == (3, 2, 3)                                      # a snapshot per new pose, none for the third call
    need = len(bar.vertices) * 16
    assert r.motion_info()[0] >= need                                            # the bar's snapshot; the floor has none
    # back to the bind pose: the previous positions are the snapshot of pose B, the mesh is rigid again and needs no new snapshot
    W, H = SIZE
    r.set_mesh_pose(0, None)
    pw4, vel, bary, src, attrs, material = draw_and_call(r, desc)
    want = restate(pkg, bary, src, np.arange(H), seen(desc, {0: bar.vertices["position"], 1: floor}), seen(desc, {0: posed(B), 1: floor}), W, H)
    same(pw4, want[0], ("skinned", "bind pose after B", "prev_world4"))
    same(vel, want[1], ("skinned", "bind pose after B", "velocity2"))
    assert r.motion_info()[1:] == (4, 2, 4)
    r.close()


def test_a_morphed_quad_and_morph_then_skin(pkg, hip):
    # a morphed quad of 441 vertices, alone in the scene
    v, ix = pkg.scenes.quad((-2, -1.5, 0), (4, 0, 0), (0, 3, 0), 20, 20)
    assert len(v) >= 300
    rng = np.random.default_rng(32)
    deltas = np.zeros((3, len(v)), pkg.scene.MORPH_DELTA_DTYPE)
    deltas["position"] = rng.normal(0, 0.1, (3, len(v), 3)).astype(F)
    r = hip.Renderer(SIZE[0], SIZE[1], 64, 16)
    r.create_material(*pkg.scenes.make_material_textures(np.random.default_rng(9), 32))
    r.create_mesh(v, ix, 0)
    r.set_mesh_morph_targets(0, deltas)
    cam = dict(eye=(0.3, 0.2, 5.0), rotation=(-2.0, -93.0), aspect=SIZE[0] / SIZE[1], fov_y=45.0, z_near_far=(0.1, 50.0))
    desc = pkg.scenes.SceneDesc(camera=cam, ambient=0.1, sun=pkg.scenes.DEFAULT_SUN, objects=pkg.scene.make_objects([(np.eye(4, dtype=F), 0)]))
    wA, wB = F([0.7, 0.0, -0.4]), F([0.1, 0.9, 0.3])
    blend = lambda w: pkg.renderer.morph_vertices(v, deltas, w)["position"]
    judge_sequence(pkg, r, desc, [(lambda: r.set_mesh_morph_weights(0, wA), blend(wA), None), (lambda: r.set_mesh_morph_weights(0, wB), blend(wB), None),
                                  (lambda: None, blend(wB), None)], "morphed")
    assert r.motion_info()[1:] == (3, 2, 3)
    r.close()
    # morph, then skin: the previous positions are skin(morph(v, previous weights), previous pose)
    r, desc, bar, deltas, floor = bar_scene(pkg, hip, morph=True)
    A, B = bar.pose(20.0), bar.pose(-15.0)
    w1, w2 = F([0.8, -0.3]), F([-0.2, 0.6])
    both = lambda w, m: pkg.renderer.skin_vertices(pkg.renderer.morph_vertices(bar.vertices, deltas, w), bar.skin, m)["position"]

    def first():
        r.set_mesh_morph_weights(0, w1)
        r.set_mesh_pose(0, A)
    judge_sequence(pkg, r, desc, [(first, both(w1, A), floor), (lambda: r.set_mesh_morph_weights(0, w2), both(w2, A), floor), (lambda: r.set_mesh_pose(0, B), both(w2, B), floor),
                                  (lambda: None, both(w2, B), floor)], "morph then skin")
    assert r.motion_info()[1:] == (4, 3, 4)
    r.close()


def test_a_first_pose_between_two_calls_reads_the_bind_pose(pkg, hip):
    r, desc, bar, _, floor = bar_scene(pkg, hip)
    A = bar.pose(35.0)
    posed = pkg.renderer.skin_vertices(bar.vertices, bar.skin, A)["position"]
    judge_sequence(pkg, r, desc, [(lambda: None, bar.vertices["position"], floor), (lambda: r.set_mesh_pose(0, A), posed, floor)], "first pose")
    assert r.motion_info()[1:] == (2, 1, 2)                                      # no snapshot while the mesh was rigid; one for the pose
    r.close()


# ---- the accumulation with motion -----------------------------------------------------------------------------------------------------------------
def floats_on_device(plane, pad=PAD):
    import torch
    t = torch.full((plane.size + pad,), float(SENTINEL), dtype=torch.float32, device="cuda")
    t[:plane.size] = torch.from_numpy(np.ascontiguousarray(plane).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return t


def accumulate_call(r, c, k, motion=True, in_place=False, host=False):
    """call k of a case on the device -> (bytes (H, W), the pad behind them, (value, count, world, normal))"""
    import torch
    attrs, material, _ = c["frames"][k]
    r.write_gbuffer(attrs, material)
    if host:
        byte = r.accumulate_ambient_occlusion_motion(c["descs"][k], c["motions"][k], c["planes"][k], **HR.HIST)
        return byte, np.full(1, TH.SENTINEL, np.uint8), r.read_ao_history()
    d_in = TH.on_device(c["planes"][k])
    d_out = d_in if in_place else torch.full_like(d_in, TH.SENTINEL)
    d_pw = floats_on_device(c["motions"][k])
    if motion:
        r.accumulate_ambient_occlusion_motion_device(c["descs"][k], d_pw.data_ptr(), d_in.data_ptr(), d_out.data_ptr(), **HR.HIST)
    else:
        r.accumulate_ambient_occlusion_device(c["descs"][k], d_in.data_ptr(), d_out.data_ptr(), **HR.HIST)
    r.flush()
    host_pw = d_pw.cpu().numpy()
    assert host_pw[:c["motions"][k].size].tobytes() == c["motions"][k].tobytes() and (host_pw[c["motions"][k].size:] == SENTINEL).all()   # the plane is only read
    out = d_out.cpu().numpy()
    n = material.size
    return out[:n].reshape(material.shape), out[n:], r.read_ao_history()


def judge(step, want, what):
    byte, pad, planes = step
    same(byte, want[0], what + ("bytes",))
    assert (pad == TH.SENTINEL).all(), what                                      # nothing past the last pixel
    for name, plane in zip(TH.PLANES, planes):
        same(plane, want[1][name], what + (name,))


@pytest.mark.parametrize("size", HS.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("camera", MS.CAMERAS)
def test_accumulation_sequences_equal_numpy_by_bytes(pkg, hip, camera, size):
    c = MS.case(pkg, camera, *size)
    want = MR.run_sequence(c["frames"], c["motions"], c["planes"])
    r = TH.handle(hip, size)
    for n in HS.CALLS:
        r.ao_history_reset()
        for k in range(n):
            judge(accumulate_call(r, c, k), want[k], (camera, size, n, k))
    for defect in MR.ACCUMULATE_DEFECTS:                                         # on these very inputs each defect shows
        bad = MR.run_sequence(c["frames"], c["motions"], c["planes"], defect=defect)
        assert b"".join(w[0].tobytes() for w in want) != b"".join(b[0].tobytes() for b in bad), defect
    r.close()


def test_accumulation_in_place_host_form_and_mixed_with_the_plain_call(pkg, hip):
    size = HS.SIZES[1]
    c = MS.case(pkg, "translated", *size)
    want = MR.run_sequence(c["frames"], c["motions"], c["planes"])
    r = TH.handle(hip, size)
    for k in range(3):
        judge(accumulate_call(r, c, k, in_place=True), want[k], ("in place", k))
    r.ao_history_reset()
    for k in range(3):
        judge(accumulate_call(r, c, k, host=True), want[k], ("host form", k))
    mixed = MR.run_sequence(c["frames"], c["motions"], c["planes"], mixed=(1, 3))
    r.ao_history_reset()
    for k in range(5):
        judge(accumulate_call(r, c, k, motion=k not in (1, 3)), mixed[k], ("mixed", k))
    assert mixed[4][0].tobytes() != want[4][0].tobytes()
    assert r.ao_history_info()[1:] == (11, 5, 0)                                 # either kernel counts as a launch of the accumulation
    r.close()


# ---- other cases ----------------------------------------------------------------------------------------------------------------------------------
def test_lists_that_shrink_or_swap_a_mesh_reset_and_resize(pkg, hip):
    g = hit_scenes.geometry(pkg)
    size, small = HS.SIZES
    W, H = size
    r = hit_handle(pkg, hip, size)
    pos = hit_positions(pkg)
    full = hit_desc(pkg, g.objects, size)
    draw_and_call(r, hit_desc(pkg, g.objects[:3], size))                         # the previous list ends before the floor's entry
    pw4, vel, bary, src, _, material = draw_and_call(r, full)
    floor = src[..., 0] == 3
    assert floor.sum() >= 500 and not pw4[floor].any() and not vel[floor].any() and (pw4[src[..., 0] == 0][:, 3] == 2).all()
    same(pw4, restate(pkg, bary, src, np.arange(H), seen(full, pos), seen(hit_desc(pkg, g.objects[:3], size), pos), W, H)[0], ("shrunk list", "prev_world4"))
    swapped = g.objects.copy()
    swapped["mesh_idx"][2] = 1                                                   # entry 2 names the floor's mesh now
    swapped["trs"][2] = np.eye(4, dtype=F).reshape(16)
    swapped["trs"][2][13] = 0.4
    d = hit_desc(pkg, swapped, size)
    pw4, vel, bary, src, _, _ = draw_and_call(r, d)
    there = src[..., 0] == 2
    assert there.sum() >= 200 and not pw4[there].any() and (pw4[src[..., 0] == 3][:, 3] == 2).all()
    same(pw4, restate(pkg, bary, src, np.arange(H), seen(d, pos), seen(full, pos), W, H)[0], ("swapped mesh", "prev_world4"))
    # a reset: the next call is a first call; so is the first call after a resize, and after resizing back
    calls = r.motion_info()
    r.motion_reset()
    assert r.motion_info() == calls[:3] + (0,)                                   # a reset frees nothing
    def every_covered_pixel_has_flag_two(out):
        covered = out[5] != HR.NO_MATERIAL
        return covered.sum() >= 100 and (out[0][covered][:, 3] == 2).all()
    assert not draw_and_call(r, full)[0].any()
    assert every_covered_pixel_has_flag_two(draw_and_call(r, full))
    r.resize(*small)
    ds = hit_desc(pkg, g.objects, small)
    assert not draw_and_call(r, ds)[0].any()
    assert every_covered_pixel_has_flag_two(draw_and_call(r, ds))
    r.resize(*size)
    assert not draw_and_call(r, full)[0].any()
    r.close()


@pytest.mark.parametrize("sharding", list(TC.SHARDS))
def test_a_row_range_and_a_band_shard_equal_the_whole_frames_rows(pkg, hip, three_calls, sharding):
    g = hit_scenes.geometry(pkg)
    size = HS.SIZES[0]
    whole = three_calls[tuple(size)][0][1]
    descs = three_calls[tuple(size)][1]
    for shard in TC.SHARDS[sharding]:
        r = hit_handle(pkg, hip, size, **shard)
        rows = S.owned(pkg, size[1], shard)
        draw_and_call(r, descs[0])
        got = draw_and_call(r, descs[1])
        for a, b, what in zip(got[:4], whole[:4], ("prev_world4", "velocity2", "bary3", "source4")):
            same(a, b[rows], (sharding, shard, what))
        r.close()


def test_the_device_form_with_and_without_velocity(pkg, hip, three_calls):
    import torch
    g = hit_scenes.geometry(pkg)
    size = HS.SIZES[1]                                                           # the ragged frame
    n = size[0] * size[1]
    calls, descs, _ = three_calls[tuple(size)]
    for with_velocity in (True, False):
        r = hit_handle(pkg, hip, size)
        d_pw, d_vel = floats_on_device(np.zeros(n * 4, F)), floats_on_device(np.zeros(n * 2, F))
        for k in range(2):
            r.pass_gbuffer(descs[k])
            r.motion_vectors_device(descs[k], d_pw.data_ptr(), d_vel.data_ptr() if with_velocity else None)
        r.flush()
        pw, vel = d_pw.cpu().numpy(), d_vel.cpu().numpy()
        assert pw[:n * 4].tobytes() == calls[1][0].tobytes() and (pw[n * 4:] == SENTINEL).all()      # nothing behind the last pixel
        assert (vel[n * 2:] == SENTINEL).all()
        assert vel[:n * 2].tobytes() == (calls[1][1].tobytes() if with_velocity else np.zeros(n * 2, F).tobytes())
        assert r.motion_info()[1:] == (2, 0, 2)
        r.close()


def test_the_stream_changes_between_two_calls(pkg, hip):
    """pose A on the handle's stream, the call; then the caller's stream: pose B, draw, the call -- the snapshot of pose A is what it reads"""
    import torch
    r, desc, bar, _, floor = bar_scene(pkg, hip)
    A, B = bar.pose(25.0), bar.pose(-30.0)
    posed = lambda m: pkg.renderer.skin_vertices(bar.vertices, bar.skin, m)["position"]
    stream = torch.cuda.Stream()
    steps = [(lambda: r.set_mesh_pose(0, A), posed(A), floor), (lambda: (r.set_stream(stream.cuda_stream), r.set_mesh_pose(0, B)), posed(B), floor),
             (lambda: (r.set_stream(None), r.set_mesh_pose(0, A)), posed(A), floor)]
    judge_sequence(pkg, r, desc, steps, "stream change")
    r.close()


def test_refusals_write_nothing_and_leave_the_state(pkg, hip):
    import ctypes as C
    g = hit_scenes.geometry(pkg)
    size = HS.SIZES[0]
    n = size[0] * size[1]
    r = hit_handle(pkg, hip, size)
    descs = [hit_desc(pkg, g.objects, size), hit_desc(pkg, g.moved, size)]
    d_pw = floats_on_device(np.full(n * 4, SENTINEL, F))

    def refused(code, fn):
        with pytest.raises(hip.ArcticError) as e:
            fn()
        assert e.value.code == code, e.value
    assert r.motion_info() == (0, 0, 0, 0)
    refused(STATE, lambda: r.motion_vectors(descs[0]))                           # nothing drawn
    refused(STATE, lambda: r.motion_vectors_device(descs[0], d_pw.data_ptr()))
    assert r.motion_info() == (0, 0, 0, 0)                                       # a refused call holds nothing
    first = draw_and_call(r, descs[0])
    s = descs[1].fill(pkg.scene.CScene())
    refused(INVALID, lambda: r.motion_vectors_device(descs[1], None))
    refused(INVALID, lambda: r.motion_vectors_device(descs[1], d_pw.data_ptr() + 4))
    refused(INVALID, lambda: r.motion_vectors_device(descs[1], d_pw.data_ptr(), d_pw.data_ptr() + 4))
    assert r.L.arctic_motion_vectors_device(r.h, None, C.c_void_p(d_pw.data_ptr()), None) == INVALID
    assert r.L.arctic_motion_vectors(r.h, None, None, None, None, None) == INVALID
    attrs, material, _, _ = r.read_gbuffer()
    r.write_gbuffer(attrs, material)                                             # an injected G-buffer leaves no visibility
    refused(STATE, lambda: r.motion_vectors(descs[1]))
    refused(STATE, lambda: r.motion_vectors_device(descs[1], d_pw.data_ptr()))
    # the accumulation's motion form: the plain call's refusals and a null or misaligned plane
    d_ao = TH.on_device(np.zeros(size[::-1], np.uint8))
    go = lambda pw=d_pw.data_ptr(), **kw: r.accumulate_ambient_occlusion_motion_device(descs[1], pw, d_ao.data_ptr(), d_ao.data_ptr(), **dict(HR.HIST, **kw))
    refused(INVALID, lambda: go(pw=None))
    refused(INVALID, lambda: go(pw=d_pw.data_ptr() + 4))
    refused(INVALID, lambda: go(max_history=0.5))
    refused(INVALID, lambda: go(plane_dist=np.nan))
    refused(INVALID, lambda: r.accumulate_ambient_occlusion_motion_device(descs[1], d_pw.data_ptr(), None, d_ao.data_ptr(), **HR.HIST))
    h = pkg.renderer._ao_history_arguments(**HR.HIST)
    assert r.L.arctic_accumulate_ambient_occlusion_motion(r.h, C.byref(s), C.c_void_p(h.ctypes.data), None, None, None) == INVALID
    # the one call: without ARCTIC_COMPOSE_AO, with a bad history block, without a visibility plane, in a state the composition refuses
    dirs = pkg.renderer.ao_directions(1, 2, seed=0)
    refused(INVALID, lambda: r.pass_ray_effects_motion(descs[1], TC.SETTINGS, None, reflection_bias=1e-3))
    refused(INVALID, lambda: r.pass_ray_effects_motion(descs[1], TC.SETTINGS, dirs, max_history=0.0))
    refused(STATE, lambda: r.pass_ray_effects_motion(descs[1], TC.SETTINGS, dirs))
    r.pass_gbuffer(descs[1])
    refused(STATE, lambda: r.pass_ray_effects_motion(descs[1], TC.SETTINGS, dirs))   # no float HDR plane
    r.flush()
    assert (d_pw.cpu().numpy() == SENTINEL).all() and (d_ao.cpu().numpy()[:n] == 0).all()   # a refused call writes nothing ...
    assert r.motion_info()[1:] == (1, 0, 1) and r.ao_history_info() == (0, 0, 0, 0)
    got = r.motion_vectors(descs[1])                                             # ... and M is what the last good call left: call 2 as if nothing had been tried
    pos = hit_positions(pkg)
    want = restate(pkg, got[2], got[3], np.arange(size[1]), seen(descs[1], pos), seen(descs[0], pos), *size)
    same(got[0], want[0], ("after the refusals", "prev_world4"))
    assert (got[0][..., 3] == 2).sum() >= 1000 and not first[0].any()
    r.close()


def test_the_one_call_equals_the_public_calls_by_hand_over_two_frames(pkg, hip):
    """arctic_pass_ray_effects_motion on ao_scenes.raster_scene with an object that moves between two frames, against motion vectors + trace +
    accumulate (motion form) + reflections + compose made by hand on a second handle: RGBA8, float LDR, composed HDR and the history, byte for
    byte; and the motion form is not the plain one there"""
    import torch
    imgs = TC.images()
    desc0 = TC.scene(pkg)
    objects = desc0.objects.copy()
    objects["trs"][1][12:15] += F([-0.1, 0.0, 0.1])                              # a box, along the normals of the two sides the camera sees: twice plane_dist
    desc1 = pkg.scenes.SceneDesc(camera=desc0.camera, ambient=desc0.ambient, sun=desc0.sun, objects=objects)
    one, hand, plain = TC.handle(pkg, hip, imgs), TC.handle(pkg, hip, imgs), TC.handle(pkg, hip, imgs)
    kw = dict(ao_strength=0.9, reflection_strength=1.2)
    ao_kw = dict(n_rays=1, pattern=2, radius=0.75, bias=1e-3, filter=True)
    hist = dict(max_history=16.0, normal_cos=0.9, plane_dist=0.05, min_weight=0.05)
    hist_kw = dict(max_history=hist["max_history"], history_normal_cos=hist["normal_cos"], history_plane_dist=hist["plane_dist"], min_weight=hist["min_weight"])
    d_ao = torch.full((TC.HEIGHT, TC.WIDTH), 77, dtype=torch.uint8, device="cuda")
    d_refl = torch.full((TC.HEIGHT, TC.WIDTH, 4), -7.0, dtype=torch.float32, device="cuda")
    d_pw = torch.full((TC.HEIGHT, TC.WIDTH, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for frame, desc in enumerate((desc0, desc1)):
        dirs = pkg.renderer.ao_directions(1, 2, seed=frame)
        for r in (one, hand, plain):
            r.pass_shadow_map(desc)
            r.pass_gbuffer(desc)
            r.pass_shade(desc, TC.SETTINGS)
        rgba8 = one.pass_ray_effects_motion(desc, TC.SETTINGS, dirs, reflection_bias=TC.BIAS, **kw, **ao_kw, **hist_kw)
        hand.motion_vectors_device(desc, d_pw.data_ptr())
        hand.trace_ambient_occlusion_device(desc, dirs, d_ao.data_ptr(), **ao_kw)
        hand.accumulate_ambient_occlusion_motion_device(desc, d_pw.data_ptr(), d_ao.data_ptr(), d_ao.data_ptr(), **hist)
        hand.trace_reflections_device(desc, TC.BIAS, d_refl.data_ptr())
        hand.compose_planes_device(desc, TC.SETTINGS, d_ao.data_ptr(), d_refl.data_ptr(), **kw)
        want = hand.read_composed()
        for a, b in zip(one.read_composed(), want):
            assert a.tobytes() == b.tobytes(), (frame, int((a != b).sum()))
        assert rgba8.tobytes() == want[2].tobytes()
        for a, b in zip(one.read_ao_history(), hand.read_ao_history()):
            assert a.tobytes() == b.tobytes(), frame
        plain.pass_ray_effects_temporal(desc, TC.SETTINGS, dirs, reflection_bias=TC.BIAS, **kw, **ao_kw, **hist_kw)
    count_motion, count_plain = one.read_ao_history()[1], plain.read_ao_history()[1]
    assert ((count_motion == 2) & (count_plain == 1)).sum() >= 50                # the moved object keeps its history only with motion
    assert one.ao_history_info()[1:] == (2, 2, 0) and one.compose_info()[2] == 2 and one.motion_info()[1:] == (2, 0, 2)
    one.close(); hand.close(); plain.close()


def test_nothing_else_moved(pkg, hip):
    """a frame's RGBA8 and arctic_stats are the same before the first motion call, after it, and on a handle that never calls;
    arctic_motion_info is zeros until the first call"""
    desc = TC.scene(pkg)
    a = TC.handle(pkg, hip)
    first = a.render_frame(desc, TC.SETTINGS).copy()
    before = a.stats().copy()
    held = a.compose_info(), a.hit_shading_info(), a.ao_history_info()
    assert a.motion_info() == (0, 0, 0, 0)
    pw4 = a.motion_vectors(desc, want=("prev_world",))[0]                         # behind a frame: the visibility plane is the frame's
    assert not pw4.any()
    pw4 = a.motion_vectors(desc, want=("prev_world",))[0]
    attrs, material, _, _ = a.read_gbuffer()
    covered = material != HR.NO_MATERIAL
    assert covered.sum() >= 1000 and pw4[covered][:, :3].tobytes() == attrs[covered][:, 11:14].tobytes()
    assert a.motion_info()[1:] == (2, 0, 2)
    assert (a.compose_info(), a.hit_shading_info(), a.ao_history_info()) == held
    after = a.render_frame(desc, TC.SETTINGS).copy()
    assert first.tobytes() == after.tobytes() and (a.stats()[:2] == before[:2]).all()
    b = TC.handle(pkg, hip, keep_float=False)                                    # a handle that never makes the calls
    assert b.render_frame(desc, TC.SETTINGS).tobytes() == first.tobytes()
    assert (b.stats()[:8] == before[:8]).all() and b.motion_info() == (0, 0, 0, 0)
    a.close(); b.close()
