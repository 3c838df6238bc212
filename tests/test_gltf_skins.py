"""Skins and animations in the glTF loader stand-in (include/arctic_gltf.h) on a machine without a GPU: JOINTS_0 / WEIGHTS_0 in every storage
the specification allows, skins with and without inverseBindMatrices, a skinned node under a transformed parent, and poses at rest, at keyframes,
between them, under STEP and clamped outside the sampler's range -- against a float64 numpy evaluation of the same definition
(tests/gltf_skin_files.py).  The definition lets a pose round once, from binary64 to fp32: every element must be within one fp32 ulp of the
matrix's largest magnitude."""
import numpy as np
import pytest

import skin_reference as R
from gltf_skin_files import write_skinned
from test_gltf_loader import write_scene


@pytest.fixture(scope="module")
def gltf(pkg):
    from importlib import import_module
    m = import_module("arctic_renderer_amd.gltf")
    m.build(force=True)
    return m


def check_pose(sc, rig, animation, t):
    got = sc.joint_matrices(0, animation, t)
    want = rig.pose(animation, t)                                        # (n, 4, 4) float64, math order
    got_m = got.reshape(-1, 4, 4).transpose(0, 2, 1).astype(np.float64)    # glm memory order -> math order
    for k in range(len(want)):
        bound = float(np.spacing(np.float32(np.abs(want[k]).max())))       # one fp32 ulp of the matrix's largest magnitude
        err = np.abs(got_m[k] - want[k]).max()
        assert err <= bound, (animation, t, k, err, bound)
    return got_m


@pytest.mark.parametrize("joints_type,weights", [(5121, "float"), (5123, "float"), (5121, "u8"), (5123, "u16")])
def test_joints_and_weights_in_every_storage(gltf, tmp_path, joints_type, weights):
    path, rig, data = write_skinned(tmp_path, joints_type=joints_type, weights=weights)
    sc = gltf.load(path)
    assert len(sc.meshes) == 1 and len(sc.objects) == 1 and sc.skin_joint_counts == [3] and len(sc.animation_durations) == 4
    skin, index, n_joints = sc.mesh_skins[0]
    assert index == 0 and n_joints == 3 and skin.dtype == R.SKIN_DTYPE and len(skin) == len(sc.meshes[0][0])
    np.testing.assert_array_equal(skin["joints"], data["joints"])
    if weights == "float":
        want = data["weights"].astype(np.float32)
    else:                                                                # normalised integers: c / 255.0f, c / 65535.0f
        want = data["weights_written"].astype(np.float32) / np.float32(255 if weights == "u8" else 65535)
    assert skin["weights"].tobytes() == want.astype(np.float32).tobytes()
    assert (skin["weights"] == 0).any() and (skin["weights"] == 1).any()


@pytest.mark.parametrize("parent", [False, True], ids=["plain-parent", "transformed-parent"])
@pytest.mark.parametrize("inverse_bind", [True, False], ids=["inverse-bind", "no-inverse-bind"])
def test_poses(gltf, tmp_path, parent, inverse_bind):
    path, rig, _ = write_skinned(tmp_path, parent=parent, inverse_bind=inverse_bind)
    sc = gltf.load(path)
    assert sc.animation_durations[:2] == [2.0, 2.0]
    rest = check_pose(sc, rig, -1, 0.0)
    if inverse_bind:                                                     # the file's inverse bind matrices make the rest pose the identity
        assert np.abs(rest - np.eye(4)).max() < 1e-5
    else:
        assert np.abs(rest - np.eye(4)).max() > 0.5
    for animation in (0, 1):
        for t in (0.0, 0.25, 0.5, 1.0, 1.5, 1.75, 2.0,                    # keyframes of one channel or another
                  0.1, 0.3333, 0.77, 1.2, 1.999,                          # between keyframes: LINEAR interpolates, STEP holds
                  -3.0, 2.5, 1e6):                                        # outside: clamped
            check_pose(sc, rig, animation, t)
    # clamping and STEP, stated directly
    assert sc.joint_matrices(0, 0, -3.0).tobytes() == sc.joint_matrices(0, 0, 0.0).tobytes()
    assert sc.joint_matrices(0, 0, 9.0).tobytes() == sc.joint_matrices(0, 0, 2.0).tobytes()
    # animation 1 rotates joint 1's node under STEP (keyframes at 0.25, 1.0, 1.75) while joint 0's node slides linearly: the rotation part of
    # joint 1's matrix holds between keyframes and jumps at them, the translation part moves all the time
    rot = lambda t: sc.joint_matrices(0, 1, t).reshape(-1, 4, 4)[1, :3, :3].astype(np.float64)
    assert np.abs(rot(0.3) - rot(0.9)).max() < 1e-6 and np.abs(rot(0.9) - rot(1.0)).max() > 0.1
    assert not np.array_equal(sc.joint_matrices(0, 1, 0.3), sc.joint_matrices(0, 1, 0.9))
    assert not np.array_equal(sc.joint_matrices(0, 0, 0.3), sc.joint_matrices(0, 0, 0.9))


def test_unsupported_animations_only_fail_when_posed(gltf, tmp_path):
    path, rig, _ = write_skinned(tmp_path)
    sc = gltf.load(path)                                                 # the file loads
    for animation, word in ((2, "CUBICSPLINE"), (3, "weights")):
        with pytest.raises(ValueError, match=word):
            sc.joint_matrices(0, animation, 0.5)
    for bad in (dict(skin=1), dict(skin=0, animation=4), dict(skin=0, animation=-2), dict(skin=0, animation=0, time=float("nan"))):
        with pytest.raises(ValueError):
            sc.joint_matrices(**bad)
    check_pose(sc, rig, 0, 0.5)                                          # ... and the others still pose


def test_a_mesh_under_two_skins_is_two_loader_meshes(gltf, tmp_path):
    path, rig, _ = write_skinned(tmp_path, second_skin=True)
    sc = gltf.load(path)
    assert len(sc.meshes) == 2 and sc.skin_joint_counts == [3, 4]
    assert sorted(int(o["mesh_idx"]) for o in sc.objects) == [0, 1]
    assert sorted(ms[1:] for ms in sc.mesh_skins) == [(0, 3), (1, 4)]     # (which of the two keeps the file's slot follows the node walk's order)
    assert sc.meshes[0][0].tobytes() == sc.meshes[1][0].tobytes() and sc.mesh_skins[0][0].tobytes() == sc.mesh_skins[1][0].tobytes()
    assert sc.joint_matrices(1).shape == (4, 16)


def test_files_without_skins_load_as_before(gltf, tmp_path):
    """the scene of tests/test_gltf_loader.py: no skins, no animations, the same meshes and objects; and a skinned file with its skins,
    animations and vertex attributes taken out gives the meshes and objects of the skinned one, in the same order"""
    path, _, geo = write_scene(str(tmp_path))
    sc = gltf.load(path)
    assert sc.mesh_skins == [None] * 3 and sc.skin_joint_counts == [] and sc.animation_durations == [] and sc._handle is None
    assert [int(o["mesh_idx"]) for o in sc.objects] == [2, 2, 0, 1] and [len(m[0]) for m in sc.meshes] == [4, 3, 6]
    with pytest.raises(ValueError):
        sc.joint_matrices(0)

    def strip(doc):
        del doc["skins"], doc["animations"]
        for n in doc["nodes"]:
            n.pop("skin", None)
        for k in ("JOINTS_0", "WEIGHTS_0"):
            del doc["meshes"][0]["primitives"][0]["attributes"][k]
    skinned = gltf.load(write_skinned(tmp_path, "a.gltf")[0])
    plain = gltf.load(write_skinned(tmp_path, "b.gltf", edit=strip)[0])
    assert plain.mesh_skins == [None] and len(plain.meshes) == len(skinned.meshes) == 1
    for (v, i, m), (v2, i2, m2) in zip(plain.meshes, skinned.meshes):
        assert v.tobytes() == v2.tobytes() and i.tobytes() == i2.tobytes() and m == m2
    assert plain.objects.tobytes() == skinned.objects.tobytes()


def test_pose_drives_any_renderer(gltf, tmp_path):
    """GltfScene.pose: skins attached once per renderer, a pose per call; a refused animation changes nothing"""
    path, rig, _ = write_skinned(tmp_path)
    sc = gltf.load(path)

    class Recorder:
        def __init__(self):
            self.calls = []

        def set_mesh_skin(self, mesh, skin, n_joints):
            self.calls.append(("skin", mesh, len(skin), n_joints))

        def set_mesh_pose(self, mesh, joints):
            self.calls.append(("pose", mesh, joints.copy()))

    r = Recorder()
    sc.pose(r, 0, 0.5, first_mesh=3)
    sc.pose(r, 0, 1.5, first_mesh=3)
    assert [c[:2] for c in r.calls] == [("skin", 3), ("pose", 3), ("pose", 3)] and r.calls[0][2:] == (len(sc.meshes[0][0]), 3)
    assert r.calls[1][2].tobytes() == sc.joint_matrices(0, 0, 0.5).tobytes() and r.calls[2][2].tobytes() == sc.joint_matrices(0, 0, 1.5).tobytes()
    with pytest.raises(ValueError):
        sc.pose(r, 2, 0.0, first_mesh=3)
    assert len(r.calls) == 3


def test_loaded_skin_poses_through_the_host_arithmetic(pkg, gltf, tmp_path):
    """loader -> arctic_skin_vertices: the records the loader makes are valid for the library, and the rest pose leaves the bar where it was"""
    path, rig, _ = write_skinned(tmp_path)
    sc = gltf.load(path)
    v, _, _ = sc.meshes[0]
    skin, _, n_joints = sc.mesh_skins[0]
    assert pkg.renderer.check_mesh_skin(skin, n_joints)
    rest = pkg.renderer.skin_vertices(v, skin, sc.joint_matrices(0))
    assert np.abs(rest["position"] - v["position"]).max() < 1e-5
    bent = pkg.renderer.skin_vertices(v, skin, sc.joint_matrices(0, 0, 1.0))
    assert bent.tobytes() == R.skin_vertices(v, skin, sc.joint_matrices(0, 0, 1.0)).tobytes()
    assert np.abs(bent["position"] - v["position"]).max() > 0.5
