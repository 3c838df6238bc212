"""KHR_lights_punctual in the scene-loader stand-in (host/gltf_loader.cpp): lights placed by the same node walk and the same accumulated
matrix a mesh on the node gets (assimp_to_mat4's transpose included), the extension's defaults, colour x intensity, the point-with-range
-> omnidirectional spot rule, shared lights, files without lights, and hostile light blocks through the sanitizer build."""
import copy
import json

import numpy as np
import pytest

from test_gltf_loader import gltf, write_scene  # noqa: F401  (the module-scoped fixture)
from test_gltf_malformed import driver, run  # noqa: F401

PI_F = np.float32(np.pi)


def local(n):
    """the node's local matrix as glTF defines it (math convention), fp32 -- as test_gltf_loader computes it"""
    if "matrix" in n:
        return np.float32(n["matrix"]).reshape(4, 4).T
    m = np.eye(4, dtype=np.float32)
    x, y, z, w = np.float32(n.get("rotation", [0, 0, 0, 1]))
    r = np.float32([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                    [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                    [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    m[:3, :3] = r * np.float32(n.get("scale", [1, 1, 1]))[None, :]
    m[:3, 3] = np.float32(n.get("translation", [0, 0, 0]))
    return m


def place(M):
    """position = (M (0,0,0,1)).xyz, direction = (M (0,0,-1,0)).xyz"""
    return M[:3, 3], -M[:3, 2]


def with_lights(tmp_path):
    path, _, _ = write_scene(str(tmp_path))
    doc = json.load(open(path))
    doc["extensionsUsed"] = ["KHR_lights_punctual"]
    doc["extensions"] = {"KHR_lights_punctual": {"lights": [
        {"type": "spot", "color": [0.5, 0.25, 1.0], "intensity": 3.0, "range": 20.0, "spot": {"innerConeAngle": 0.1, "outerConeAngle": 0.6}},
        {"type": "point", "intensity": 2.0, "range": 7.5},
        {"type": "point", "color": [0.2, 0.4, 0.6], "intensity": 10.0},
        {"type": "directional", "intensity": 5.0},
        {"type": "area", "intensity": 1.0},
    ]}}
    nodes = doc["nodes"]
    nodes[0].setdefault("extensions", {})["KHR_lights_punctual"] = {"light": 3}     # a: directional (counted only)
    nodes[1]["extensions"] = {"KHR_lights_punctual": {"light": 0}}                  # b: rotated, scaled, nested under a
    nodes[1]["children"] = [4]
    nodes[2]["extensions"] = {"KHR_lights_punctual": {"light": 1}}                  # c: matrix node, point with range
    nodes[3]["extensions"] = {"KHR_lights_punctual": {"light": 2}}                  # d: root, plain point light
    nodes.append({"name": "e", "translation": [0.5, -1.0, 2.0], "rotation": [0.2705981, 0.0, 0.0, 0.9626950],
                  "extensions": {"KHR_lights_punctual": {"light": 0}}})              # e: the same spot light again, one level deeper
    nodes.append({"name": "f", "extensions": {"KHR_lights_punctual": {"light": 4}}})   # unknown type: skipped
    nodes[4].setdefault("children", [5])
    json.dump(doc, open(path, "w"))
    return path, doc


def test_lights_follow_the_node_walk(gltf, tmp_path):  # noqa: F811
    path, doc = with_lights(tmp_path)
    sc = gltf.load(path)
    nodes = doc["nodes"]
    A, B, Cn, E = (local(nodes[i]) for i in (0, 1, 2, 4))
    Mb = A.T @ B.T          # the loader's convention (test_gltf_loader: objects' matrices)
    Mc = A.T @ Cn.T
    Me = Mb @ E.T
    # the meshes' objects are what they were without lights
    assert len(sc.objects) == 4
    np.testing.assert_allclose(sc.objects[2]["trs"].reshape(4, 4).T, Mb, atol=1e-6)
    # walk order: d, a, c, b, e, f -> points [d], spots [c (omni), b, e], one directional, the unknown type skipped
    assert sc.directional_lights == 1
    assert len(sc.point_lights) == 1 and len(sc.spot_lights) == 3
    p = sc.point_lights[0]
    np.testing.assert_array_equal(p["position"], [0, 0, 0])
    np.testing.assert_array_equal(p["color"], np.float32(np.array([0.2, 0.4, 0.6]) * 10.0))
    omni, sb, se = sc.spot_lights
    pos, _ = place(Mc)
    np.testing.assert_allclose(omni["position"], pos, atol=1e-6)
    assert omni["outer_cone_angle"] == PI_F and omni["inner_cone_angle"] == 0 and omni["range"] == np.float32(7.5)
    np.testing.assert_array_equal(omni["color"], [2, 2, 2])
    assert np.linalg.norm(omni["direction"]) > 0
    for s, M in ((sb, Mb), (se, Me)):
        pos, d = place(M)
        np.testing.assert_allclose(s["position"], pos, atol=1e-5)
        np.testing.assert_allclose(s["direction"], d, atol=1e-5)
        assert s["inner_cone_angle"] == np.float32(0.1) and s["outer_cone_angle"] == np.float32(0.6) and s["range"] == np.float32(20.0)
        np.testing.assert_array_equal(s["color"], np.float32(np.array([0.5, 0.25, 1.0]) * 3.0))
    # the two placements of light 0 differ: e's rotation about x turns the direction
    assert not np.allclose(sb["direction"], se["direction"])
    # the loaded records pass the library's validation
    from importlib import import_module
    L = import_module("arctic_renderer_amd.binding").lib()
    out = np.zeros((3, 12), np.float32)
    assert L.arctic_spot_light_constants(sc.spot_lights.ctypes.data, 3, out.ctypes.data) == 0


def test_khr_defaults_and_no_extension(gltf, tmp_path):  # noqa: F811
    path, _, _ = write_scene(str(tmp_path))
    sc = gltf.load(path)
    assert len(sc.spot_lights) == 0 and len(sc.point_lights) == 0 and sc.directional_lights == 0
    doc = json.load(open(path))
    doc["extensions"] = {"KHR_lights_punctual": {"lights": [{"type": "spot"}, {"type": "point"}]}}
    doc["nodes"][3]["extensions"] = {"KHR_lights_punctual": {"light": 0}}
    doc["nodes"][2]["extensions"] = {"KHR_lights_punctual": {"light": 1}}
    json.dump(doc, open(path, "w"))
    sc = gltf.load(path)
    assert len(sc.spot_lights) == 1 and len(sc.point_lights) == 1
    s = sc.spot_lights[0]
    np.testing.assert_array_equal(s["color"], [1, 1, 1])
    assert s["inner_cone_angle"] == 0 and s["outer_cone_angle"] == np.float32(np.pi / 4) and s["range"] == 0
    np.testing.assert_array_equal(s["position"], [0, 0, 0])
    np.testing.assert_array_equal(s["direction"], [0, 0, -1])        # an identity node points down -Z
    np.testing.assert_array_equal(sc.point_lights[0]["color"], [1, 1, 1])
    # lights in the file but on no node: nothing placed
    del doc["nodes"][3]["extensions"], doc["nodes"][2]["extensions"]
    json.dump(doc, open(path, "w"))
    sc = gltf.load(path)
    assert len(sc.spot_lights) == 0 and len(sc.point_lights) == 0


def hostile_docs(doc):
    def lights(ls, node_light=0):
        d = copy.deepcopy(doc)
        d["extensions"] = {"KHR_lights_punctual": {"lights": ls}}
        d["nodes"][3]["extensions"] = {"KHR_lights_punctual": {"light": node_light}}
        return d
    spot = {"type": "spot", "spot": {"innerConeAngle": 0.1, "outerConeAngle": 0.5}}
    return {
        "index_out_of_range": lights([spot], 1),
        "index_negative": lights([spot], -1),
        "index_huge": lights([spot], 1e300),
        "index_string": lights([spot], "0"),
        "negative_range": lights([dict(spot, range=-1.0)]),
        "zero_range": lights([{"type": "point", "range": 0.0}]),
        "inner_above_outer": lights([{"type": "spot", "spot": {"innerConeAngle": 0.6, "outerConeAngle": 0.5}}]),
        "outer_above_half_pi": lights([{"type": "spot", "spot": {"outerConeAngle": 2.0}}]),
        "negative_inner": lights([{"type": "spot", "spot": {"innerConeAngle": -0.1}}]),
        "intensity_string": lights([dict(spot, intensity="x")]),
        "color_strings": lights([dict(spot, color=["a", 1, 1])]),
        "color_short": lights([dict(spot, color=[1, 1])]),
        "color_negative": lights([dict(spot, color=[1, -1, 1])]),
        "type_number": lights([{"type": 3}]),
        "lights_not_array": (lambda d: (d.update(extensions={"KHR_lights_punctual": {"lights": {"type": "spot"}}}), d)[1])(copy.deepcopy(doc)),
        "no_lights_key": (lambda d: (d.update(extensions={"KHR_lights_punctual": {}}), d)[1])(copy.deepcopy(doc)),
    }


def test_hostile_light_blocks_are_refused(gltf, tmp_path):  # noqa: F811
    path, _, _ = write_scene(str(tmp_path))
    doc = json.load(open(path))
    for name, d in hostile_docs(doc).items():
        json.dump(d, open(path, "w"))
        with pytest.raises(ValueError, match="glTF"):
            gltf.load(path)


def test_hostile_light_blocks_under_the_sanitizer(driver, tmp_path):  # noqa: F811
    path, _, _ = write_scene(str(tmp_path))
    doc = json.load(open(path))
    paths = []
    for name, d in hostile_docs(doc).items():
        p = tmp_path / f"{name}.gltf"
        json.dump(d, open(p, "w"))
        paths.append(p)
    (tmp_path / "good").mkdir()
    good, _ = with_lights(tmp_path / "good")
    lines = run(driver, paths + [good])
    assert all(l.startswith("refused") for l in lines[:-1]), lines
    assert lines[-1].startswith("ok"), lines[-1]
