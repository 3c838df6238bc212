"""Morph targets in the glTF loader stand-in (include/arctic_gltf.h) on a machine without a GPU, on files the test writes itself
(tests/gltf_morph_files.py): dense and sparse target accessors, POSITION-only / +NORMAL / +TANGENT targets, the derived-delta rule, weights
from the mesh, the node and animations, and what stays refused."""
import hashlib

import numpy as np
import pytest

import morph_reference as M
from gltf_morph_files import KEY_TIMES, KEY_WEIGHTS, weights_at, write_morphed
from test_gltf_loader import write_scene

F = np.float32


@pytest.fixture(scope="module")
def gltf(pkg):
    from importlib import import_module
    m = import_module("arctic_renderer_amd.gltf")
    m.build(force=True)
    return m


def test_dense_targets(gltf, tmp_path):
    path, data = write_morphed(tmp_path)
    sc = gltf.load(path)
    assert len(sc.meshes) == 1 and sc.mesh_morphs[0].shape == (2, 18) and sc.mesh_morphs[0].dtype == M.MORPH_DTYPE
    d = sc.mesh_morphs[0]
    assert d["position"].tobytes() == data["dp"].tobytes() and d["normal"].tobytes() == data["dn"].tobytes()
    assert d["tangent"].tobytes() == data["dt"].tobytes()
    assert (d["bitangent"] != 0).any()
    assert sc.morph_weights(0).tobytes() == np.zeros(2, F).tobytes()                 # the default is zeros


@pytest.mark.parametrize("base_view", [False, True], ids=["zeros-base", "view-base"])
@pytest.mark.parametrize("index_type", [5121, 5123, 5125], ids=["u8", "u16", "u32"])
def test_sparse_targets_equal_dense_targets(gltf, tmp_path, index_type, base_view):
    dense = gltf.load(write_morphed(tmp_path, "dense.gltf")[0])
    path, data = write_morphed(tmp_path, "sparse.gltf", storage="sparse", index_type=index_type, base_view=base_view)
    assert "sparse" in data["doc"]["accessors"][data["doc"]["meshes"][0]["primitives"][0]["targets"][0]["POSITION"]]
    sparse = gltf.load(path)
    assert sparse.mesh_morphs[0].tobytes() == dense.mesh_morphs[0].tobytes()
    assert sparse.meshes[0][0].tobytes() == dense.meshes[0][0].tobytes()


@pytest.mark.parametrize("tangent_attr", [True, False], ids=["file-tangents", "computed-tangents"])
@pytest.mark.parametrize("with_normal,with_tangent", [(False, False), (True, False), (True, True)], ids=["position", "+normal", "+tangent"])
def test_derived_deltas_reproduce_the_baked_file(gltf, pkg, tmp_path, with_normal, with_tangent, tangent_attr):
    """the rule of include/arctic_gltf.h -- the value with target k alone at weight 1, minus the base value: arctic_morph_vertices with that
    weight vector gives the loader's own vertices for the file that has target k baked in.  BIT FOR BIT in position, normal and the file's
    tangent (base + 1 * d is the float32 sum the baked file was written with); the derived vectors -- the bitangent, and without a TANGENT
    attribute the tangent too -- within ONE fp32 ulp of the component's magnitude (b + fl(B - b) rounds twice where the baked file has B)."""
    path, data = write_morphed(tmp_path, with_normal=with_normal, with_tangent=with_tangent, tangent_attr=tangent_attr)
    sc = gltf.load(path)
    v, d = sc.meshes[0][0], sc.mesh_morphs[0]
    if not with_normal:
        assert (d["normal"] == 0).all()                                              # a missing attribute means zero deltas
    if tangent_attr and not with_tangent:
        assert (d["tangent"] == 0).all()
    for k in range(2):
        bpath, _ = write_morphed(tmp_path, f"baked{k}.gltf", baked=k, with_normal=with_normal, with_tangent=with_tangent, tangent_attr=tangent_attr)
        want = gltf.load(bpath).meshes[0][0]
        w = np.zeros(2, F); w[k] = 1
        got = pkg.renderer.morph_vertices(v, d, w)
        assert got.tobytes() == M.morph_vertices(v, d, w).tobytes()
        assert got["position"].tobytes() == want["position"].tobytes() and got["position"].tobytes() != v["position"].tobytes()
        assert got["normal"].tobytes() == want["normal"].tobytes()
        derived = ["bitangent"] if tangent_attr else ["tangent", "bitangent"]
        if tangent_attr:
            assert got["tangent"].tobytes() == want["tangent"].tobytes()
        for name in derived:
            bound = np.spacing(np.maximum(np.abs(want[name]), np.abs(v[name])).astype(F))
            assert (np.abs(got[name].astype(np.float64) - want[name].astype(np.float64)) <= bound).all(), name
        if with_normal or not tangent_attr:
            assert got["bitangent"].tobytes() != v["bitangent"].tobytes()            # ... and the derived part is not nothing
        assert got["tex_coords"].tobytes() == v["tex_coords"].tobytes()


def test_node_weights_override_mesh_weights_and_a_second_node_is_a_second_mesh(gltf, tmp_path):
    sc = gltf.load(write_morphed(tmp_path, "m.gltf", mesh_weights=[0.5, -1.0])[0])
    np.testing.assert_array_equal(sc.morph_weights(0), F([0.5, -1.0]))
    sc = gltf.load(write_morphed(tmp_path, "n.gltf", mesh_weights=[0.5, -1.0], node_weights=[2.0, 0.125])[0])
    np.testing.assert_array_equal(sc.morph_weights(0), F([2.0, 0.125]))
    one = gltf.load(write_morphed(tmp_path, "one.gltf", mesh_weights=[0.5, -1.0])[0])
    two = gltf.load(write_morphed(tmp_path, "two.gltf", mesh_weights=[0.5, -1.0], two_nodes=True)[0])
    assert len(one.meshes) == 1 and len(two.meshes) == 2 and len(two.objects) == 2
    assert sorted(int(o["mesh_idx"]) for o in two.objects) == [0, 1]
    assert two.meshes[1][0].tobytes() == two.meshes[0][0].tobytes() and two.mesh_morphs[1].tobytes() == two.mesh_morphs[0].tobytes()
    by_weights = sorted(two.morph_weights(i).tolist() for i in range(2))
    assert by_weights == [[0.25, 0.5], [0.5, -1.0]]                                  # the twin's own node.weights, the body's mesh.weights
    # the animation targets the body's node alone
    body = [i for i in range(2) if two.morph_weights(i).tolist() == [0.5, -1.0]][0]
    np.testing.assert_array_equal(two.morph_weights(body, 0, 1.0), F(KEY_WEIGHTS[1]))
    np.testing.assert_array_equal(two.morph_weights(1 - body, 0, 1.0), F([0.25, 0.5]))


@pytest.mark.parametrize("animation,step", [(0, False), (1, True)], ids=["LINEAR", "STEP"])
def test_animated_weights(gltf, tmp_path, animation, step):
    """at keyframes, between them and clamped outside, against the float64 evaluation of a + (b - a) u.  The binary64 error is far below half
    an fp32 ulp, so the one rounding to fp32 lands on the nearest value or its neighbour: at most one fp32 ulp of max(|a|, |b|)."""
    sc = gltf.load(write_morphed(tmp_path, node_weights=[0.3, 0.6])[0])
    assert len(sc.animation_durations) == 4 and sc.animation_durations[0] == 2.0
    np.testing.assert_array_equal(sc.morph_weights(0, -1, 1.0), F([0.3, 0.6]))
    between = 0
    for t in (-1.0, 0.0, 0.5, 0.6, 0.75, 0.999, 1.0, 1.3, 1.9999, 2.0, 7.0):
        got = sc.morph_weights(0, animation, t)
        want, a, b = weights_at(KEY_TIMES, KEY_WEIGHTS, t, step)
        bound = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(F)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want) <= bound).all(), (t, got, want)
        if t in KEY_TIMES or t < KEY_TIMES[0] or t > KEY_TIMES[-1] or step:
            assert got.tobytes() == want.astype(F).tobytes()                         # a keyframe's own values, exactly
        else:
            between += 1
            assert got.tobytes() != F(a).tobytes() and got.tobytes() != F(b).tobytes()
    assert step or between == 5


def test_an_animation_with_joint_and_weights_channels_poses_both(gltf, tmp_path):
    sc = gltf.load(write_morphed(tmp_path, skin=True)[0])
    assert sc.mesh_skins[0] is not None and sc.mesh_morphs[0] is not None
    rest, moved = sc.joint_matrices(0, -1, 0.0), sc.joint_matrices(0, 0, 1.0)
    assert not np.array_equal(rest, moved)
    np.testing.assert_array_equal(sc.morph_weights(0, 0, 1.0), F(KEY_WEIGHTS[1]))

    class Recorder:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda *a: self.calls.append((name, a))

    r = Recorder()
    sc.pose(r, 0, 1.0)
    sc.pose(r, 0, 2.0)
    names = [c[0] for c in r.calls]
    assert names == ["set_mesh_skin", "set_mesh_morph_targets", "set_mesh_morph_weights", "set_mesh_pose", "set_mesh_morph_weights", "set_mesh_pose"]
    np.testing.assert_array_equal(r.calls[2][1][1], F(KEY_WEIGHTS[1]))
    np.testing.assert_array_equal(r.calls[3][1][1], moved)
    np.testing.assert_array_equal(r.calls[4][1][1], F(KEY_WEIGHTS[2]))
    assert r.calls[1][1][1].tobytes() == sc.mesh_morphs[0].tobytes()


def test_what_stays_refused_at_pose_time(gltf, tmp_path):
    """CUBICSPLINE refused; weights channel without targets refused with 'weights' -- only that animation, the file loads"""
    sc = gltf.load(write_morphed(tmp_path, skin=True)[0])
    for animation, word in ((2, "CUBICSPLINE"), (3, "weights")):
        with pytest.raises(ValueError, match=word):
            sc.morph_weights(0, animation, 0.5)
        with pytest.raises(ValueError, match=word):
            sc.joint_matrices(0, animation, 0.5)
        with pytest.raises(ValueError, match=word):
            sc.pose(object(), animation, 0.5)                                         # evaluated first: the renderer is never touched
    with pytest.raises(ValueError):
        sc.morph_weights(0, 9, 0.0)
    with pytest.raises(ValueError):
        sc.morph_weights(0, 0, float("nan"))
    with pytest.raises(ValueError):
        sc.morph_weights(5, 0, 0.0)


def test_files_without_targets_load_as_before(gltf, tmp_path):
    """test_gltf_loader.py's scene: the same meshes, objects and materials -- the digest is that of the loader before it read morph targets"""
    path, _, _ = write_scene(str(tmp_path), embed=True)
    sc = gltf.load(path)
    assert sc.mesh_morphs == [None, None, None] and sc.mesh_skins == [None, None, None]
    h = hashlib.sha256()
    for v, i, mat in sc.meshes:
        h.update(v.tobytes()); h.update(i.tobytes()); h.update(bytes([mat]))
    h.update(sc.objects.tobytes())
    for m in sc.materials:
        for img in m:
            h.update(img.tobytes())
    h.update(sc.material_params.tobytes())
    assert h.hexdigest() == PARENT_DIGEST


PARENT_DIGEST = "06b037ea5a963f653ae960aecf608a77b5cefc6dc9e19bf645a39a6832dd57c0"
