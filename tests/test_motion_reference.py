"""The motion vectors and the accumulation's motion form on a machine without a GPU: the numpy restatement (tests/motion_reference.py) pinned on
pixels worked by hand, the host arbiters arctic_motion_pixels and arctic_accumulate_pixels_motion against it BY BYTES, every deliberate defect
shown to change output bytes, and what the feature is for: a face that moves along its own normal keeps its history with motion and loses it
every frame without."""
import numpy as np
import pytest

import ao_history_reference as HR
import ao_history_scenes as HS
import hit_scenes
import motion_reference as MR
import motion_scenes as MS

F = np.float32
IDENTITY = np.eye(4, dtype=F).reshape(16)
LONG = dict(HR.HIST, max_history=32.0, min_weight=0.0)      # a cap five calls do not reach, and no weight floor: a new edge pixel keeps what its accepted taps hold


def translation(x, y, z):
    t = np.eye(4, dtype=F)
    t[3, :3] = (x, y, z)                     # [col][row]: the fourth column
    return t.reshape(16)


def test_pixels_worked_by_hand():
    q = np.array([[[0.5, 0.25, 0.125], [1.5, 0.25, 0.125], [0.5, 2.25, 0.125]]], F)
    xy = np.array([[10, 20]], np.int32)
    one = lambda B, T, P=IDENTITY, has=True: MR.motion(np.array([B], F), [has], T[None], q, xy, P, 96, 64)
    # identity motion: the point itself
    pw4, vel = one((1, 0, 0), IDENTITY)
    assert pw4.tolist() == [[0.5, 0.25, 0.125, 2.0]]
    assert vel.tolist() == [[(0.5 + 1) * 48 - 10.5, (1 - 0.25) * 32 - 20.5]]     # sx = 72, sy = 24: from the pixel's centre to where the point was
    pw4, _ = one((0.25, 0.5, 0.25), IDENTITY)
    assert pw4.tolist() == [[(0.25 * 0.5 + 0.5 * 1.5) + 0.25 * 0.5, (0.25 * 0.25 + 0.5 * 0.25) + 0.25 * 2.25, 0.125, 2.0]]
    # a pure translation of the previous trs
    pw4, vel = one((0, 1, 0), translation(-1.0, 0.5, 0.25))
    assert pw4.tolist() == [[0.5, 0.75, 0.375, 2.0]]
    assert vel.tolist() == [[1.5 * 48 - 10.5, 0.25 * 32 - 20.5]]
    # c3 <= 0: the point, flag 1, no velocity
    behind = IDENTITY.copy()
    behind[15] = -1.0
    pw4, vel = one((1, 0, 0), IDENTITY, behind)
    assert pw4.tolist() == [[0.5, 0.25, 0.125, 1.0]] and vel.tolist() == [[0.0, 0.0]]
    zero_w = IDENTITY.copy()
    zero_w[15] = 0.0
    assert one((1, 0, 0), IDENTITY, zero_w)[0][0, 3] == 1.0
    # no previous: the object has none, or M is empty
    for pw4, vel in (one((1, 0, 0), IDENTITY, has=False), one((1, 0, 0), IDENTITY, P=None)):
        assert not pw4.any() and not vel.any()
    # a NaN previous position stays inside pw: flag 1, no velocity, and the accumulation rejects everything for it
    q[0, 0, 1] = np.nan
    pw4, vel = one((1, 0, 0), IDENTITY)
    assert np.isnan(pw4[0, :3]).all() and pw4[0, 3] == 1.0 and vel.tolist() == [[0.0, 0.0]]   # (0 * NaN: every row of the product holds it)
    prev = dict(P=IDENTITY.reshape(4, 4), value=np.full((64, 96), 9, F), count=np.full((64, 96), 3, F), world=np.zeros((64, 96, 3), F), normal=np.tile(F([0, 0, 1]), (64, 96, 1)))
    r = MR.accumulate([[0.5, 0.25, 0.0]], pw4, [[0, 0, 2]], [1], [200], prev, 96, 64)
    assert r["byte"].tolist() == [200] and r["count"].tolist() == [1.0] and r["world"].tolist() == [[0.5, 0.25, 0.0]]
    # ... while the same pixel with its point known takes the history: N = 3 + 1, value = 9 + (200 - 9) / 4
    good = np.array([[0.5, 0.25, 0.0, 2.0]], F)
    r = MR.accumulate([[0.5, 0.25, 0.0]], good, [[0, 0, 2]], [1], [200], prev, 96, 64)
    assert r["count"].tolist() == [4.0] and r["value"].tolist() == [9 + 191 / 4] and r["byte"].tolist() == [57]


# ---- the motion pass: pixels over hit_scenes.geometry, as the device test rasterises it ---------------------------------------------------------
def motion_inputs(pkg, n=6000, seed=5):
    """n pixels on random triangles of the scene's objects, call 2 of the device test: the previous call saw `objects`, this one `moved`; the
    floor's previous positions differ from its current ones (a pose between the calls)"""
    g = hit_scenes.geometry(pkg)
    rng = np.random.default_rng(seed)
    W, H = HS.SIZES[0]
    P = pkg.renderer.frame_constants(hit_scenes.description(pkg, g.objects))[0]
    obj = rng.choice([0, 2, 3], n).astype(np.uint32)
    q_prev, q_now = np.zeros((n, 3, 3), F), np.zeros((n, 3, 3), F)
    for k, o in enumerate(obj):
        v, ix = g.meshes[int(g.objects[o]["mesh_idx"])]
        while True:
            tri = ix[3 * rng.integers(len(ix) // 3):][:3]
            if (tri < len(v)).all():
                break
        q_now[k] = v["position"][tri]
    q_prev[:] = q_now
    floor = obj == 3
    q_prev[floor] += rng.normal(0, 0.05, (int(floor.sum()), 3, 3)).astype(F)
    B = rng.dirichlet(np.ones(3), n).astype(F)
    xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int32)
    obj[:40] = MR.NO_OBJECT
    obj[40:80] = 1000                                                            # beyond the previous list: no previous
    q_prev[80:90, 1, 2] = np.nan
    q_prev[90:100] *= F(1e30)
    return dict(g=g, B=B, obj=obj, q_prev=q_prev, q_now=q_now, xy=xy, P=P, W=W, H=H, prev_trs=g.objects["trs"], cur_trs=g.moved["trs"])


def numpy_motion(c, defect=None):
    has = (c["obj"] != MR.NO_OBJECT) & (c["obj"] < len(c["prev_trs"]))
    trs = c["cur_trs"] if defect == "current trs" else c["prev_trs"]
    T = trs[np.where(has, c["obj"], 0)]
    q = c["q_now"] if defect == "current positions" else c["q_prev"]
    return MR.motion(c["B"], has, T, q, c["xy"], c["P"], c["W"], c["H"], defect)


def test_the_motion_arbiter_equals_numpy_by_bytes(pkg):
    c = motion_inputs(pkg)
    want = numpy_motion(c)
    got = pkg.renderer.motion_pixels(c["B"], c["obj"], c["q_prev"], c["xy"], c["prev_trs"], c["P"], c["W"], c["H"])
    for a, b, what in zip(got, want, ("prev_world4", "velocity2")):
        assert a.tobytes() == b.tobytes(), (what, int((a.view(np.uint32) != b.view(np.uint32)).any(-1).sum()))
    assert (want[0][:, 3] == 2).sum() >= 5000 and (want[0][:, 3] == 0).sum() == 80 and (want[0][:, 3] == 1).sum() >= 10
    assert np.isnan(want[0][80:90, :3]).any(1).all() and not want[1][80:90].any()
    # M empty: all zero
    empty = pkg.renderer.motion_pixels(c["B"], c["obj"], c["q_prev"], c["xy"], c["prev_trs"], None, c["W"], c["H"])
    assert not empty[0].any() and not empty[1].any()
    # identity motion: pw is the interpolated current world, bit for bit
    same = pkg.renderer.motion_pixels(c["B"], c["obj"], c["q_now"], c["xy"], c["cur_trs"], c["P"], c["W"], c["H"])[0]
    has = same[:, 3] > 0
    world = MR.interpolate(c["B"][has], *[MR.mat_rows(c["cur_trs"][c["obj"][has]], c["q_now"][has, k]) for k in range(3)])
    assert same[has, :3].tobytes() == world.tobytes()


@pytest.mark.parametrize("defect", MR.MOTION_DEFECTS)
def test_every_motion_defect_changes_bytes(pkg, defect):
    c = motion_inputs(pkg)
    want, bad = numpy_motion(c), numpy_motion(c, defect)
    assert want[0].tobytes() + want[1].tobytes() != bad[0].tobytes() + bad[1].tobytes()
    changed = (want[0].view(np.uint32) != bad[0].view(np.uint32)).any(1) | (want[1].view(np.uint32) != bad[1].view(np.uint32)).any(1)
    assert changed.sum() >= 500, int(changed.sum())


# ---- the accumulation with motion: the analytic moving-box sequences the device test injects ----------------------------------------------------
@pytest.mark.parametrize("size", HS.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("camera", MS.CAMERAS)
def test_the_accumulation_arbiter_equals_numpy_by_bytes(pkg, camera, size):
    W, H = size
    c = MS.case(pkg, camera, W, H)
    prev = None
    for k, ((attrs, material, P), pw4, cur) in enumerate(zip(c["frames"], c["motions"], c["planes"])):
        byte, state = MR.accumulate_frame(attrs, material, pw4, cur, prev, P)
        a = attrs.reshape(-1, 18)
        got = pkg.renderer.accumulate_pixels_motion(a[:, 11:14], pw4, a[:, 8:11], material.reshape(-1) != HR.NO_MATERIAL, cur, None if prev is None else prev["P"], W, H,
                                                    None if prev is None else (prev["value"], prev["count"], prev["world"], prev["normal"]), **HR.HIST)
        for x, y, what in zip(got, (byte, state["value"], state["count"], state["world"], state["normal"]), ("byte", "value", "count", "world", "normal")):
            assert x.tobytes() == np.ascontiguousarray(y).tobytes(), (camera, size, k, what)
        prev = state
    assert (prev["count"] >= 4).sum() >= 200                                       # the cap is reached, history is used


@pytest.mark.parametrize("defect", MR.ACCUMULATE_DEFECTS)
def test_every_accumulation_defect_changes_bytes(pkg, defect):
    for size in HS.SIZES:
        c = MS.case(pkg, "translated", *size)
        want = MR.run_sequence(c["frames"], c["motions"], c["planes"])
        bad = MR.run_sequence(c["frames"], c["motions"], c["planes"], defect=defect)
        assert b"".join(w[0].tobytes() for w in want) != b"".join(b[0].tobytes() for b in bad), (defect, size)
    # the plain definition is not the motion form either, and a mixed sequence is a third thing
    plain = HR.run_sequence(c["frames"], c["planes"])
    mixed = MR.run_sequence(c["frames"], c["motions"], c["planes"], mixed=(2,))
    assert want[4][0].tobytes() != plain[4][0].tobytes() and mixed[4][0].tobytes() not in (want[4][0].tobytes(), plain[4][0].tobytes())


def test_what_it_is_for_a_face_moving_along_its_normal_keeps_its_history(pkg):
    """the box's front face comes STEP = 0.08 closer per call, plane_dist is 0.05, the camera stands still: on the face pixels whose four taps lay
    on the face in the previous frame the history's count after call 5 is above 4.5 with motion (5: every call accepted) and exactly 1 with the
    plain definition, which finds the face a step behind the point it tests and rejects it every frame"""
    W, H = HS.SIZES[0]
    c = MS.case(pkg, "still", W, H, odd=False)
    assert MS.STEP > LONG["plane_dist"]
    moved = MR.run_sequence(c["frames"], c["motions"], c["planes"], LONG)
    plain = HR.run_sequence(c["frames"], c["planes"], LONG)
    face = MS.taps_on_front_face(c, 4)
    assert face.sum() >= 50, int(face.sum())
    assert (moved[4][1]["count"][face] > 4.5).all(), moved[4][1]["count"][face].min()
    assert (plain[4][1]["count"][face] == 1).all(), plain[4][1]["count"][face].max()
    still = ~MS.on_box(c["frames"][4][0]) & (plain[4][1]["count"] > 4.5)            # what stands still accumulates either way, to the same bytes
    assert still.sum() >= 1000 and (moved[4][1]["count"][still] == plain[4][1]["count"][still]).all()
