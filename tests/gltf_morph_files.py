"""glTF files with morph targets, written by the tests that read them (test_gltf_morph.py, test_gltf_morph_malformed.py, test_gpu_morph.py),
and the float64 evaluation of their animated weights the loader is checked against."""
import base64
import json
import os

import numpy as np

from gltf_skin_files import bar_geometry, quat_z

F = np.float32
KEY_TIMES = [0.5, 1.0, 2.0]
KEY_WEIGHTS = [[0.0, 1.0], [0.75, -0.25], [1.5, 0.1]]               # keyframes x targets


def weights_at(times, values, t, step):
    """include/arctic_gltf.h, arctic_gltf_morph_weights, in float64: a + (b - a) u, time clamped; returns (w, a, b) -- the two keyframes for
    the tolerance"""
    times = np.asarray(times, F).astype(np.float64)
    values = np.asarray(values, F).astype(np.float64)
    if t <= times[0]:
        return values[0], values[0], values[0]
    if t >= times[-1]:
        return values[-1], values[-1], values[-1]
    k = int(np.searchsorted(times, t, side="right")) - 1
    a, b = values[k], values[k + 1]
    if step or t == times[k]:
        return a, a, a
    u = (t - times[k]) / (times[k + 1] - times[k])
    return a + (b - a) * u, a, b


def targets(n_vertices=18):
    """two targets of the bar: 0 lifts a few vertices in the middle (few rows are not zero: what a sparse accessor is for), 1 bends the right end"""
    p, nrm, uv, idx, joints, w = bar_geometry()
    assert len(p) == n_vertices
    dp, dn, dt = np.zeros((2, len(p), 3), F), np.zeros((2, len(p), 3), F), np.zeros((2, len(p), 3), F)
    mid = [6, 7, 8, 9, 11]
    dp[0, mid] = [(0.0, 0.35, 0.5), (0.1, 0.25, 0.5), (0.0, 0.4, 0.75), (-0.1, 0.3, 0.75), (0.0, 0.125, 0.25)]
    dn[0, mid] = [(0.3, 0.0, -0.1), (0.3, 0.1, -0.1), (0.0, 0.2, -0.05), (-0.3, 0.0, -0.1), (-0.3, 0.1, 0.0)]
    dt[0, mid] = [(-0.05, 0.0, 0.3), (-0.05, 0.0, 0.3), (0.0, 0.0, 0.1), (-0.05, 0.1, -0.3), (0.0, 0.0, -0.2)]
    right = np.arange(12, len(p))
    dp[1, right, 1] = (0.5 * (p[right, 0] - 1.0)).astype(F)
    dp[1, right, 2] = F(-0.25)
    dn[1, right] = (0.0, -0.2, 0.05)
    dt[1, right] = (0.0, 0.25, 0.0)
    return dp, dn, dt


def write_morphed(tmp, name="morphed.gltf", storage="dense", index_type=5121, base_view=False, with_normal=True, with_tangent=True,
                  tangent_attr=True, baked=None, skin=False, two_nodes=False, node_weights=None, mesh_weights=None, animations=True, edit=None):
    """returns (path, dict of what was written).  storage "dense" / "sparse" (index_type u8 5121 / u16 5123 / u32 5125; base_view: the sparse
    accessor has a dense base whose replaced rows hold junk); baked = k: no targets, target k -- the parts of it with_normal / with_tangent select -- applied to the attributes in float32 instead.
    `edit(doc)` may change the JSON document before it is written (malformed files)."""
    p, nrm, uv, idx, joints, w = bar_geometry()
    tan = np.tile(F([1, 0, 0, 1]), (len(p), 1))
    tan[1::2, 3] = -1                                                        # both handednesses
    dp, dn, dt = targets(len(p))
    blobs, views, accessors = [], [], []

    def view(data):
        off = sum(len(b) for b in blobs)
        pad = (-off) % 4
        blobs.append(b"\0" * pad + data)
        views.append({"buffer": 0, "byteOffset": off + pad, "byteLength": len(data)})
        return len(views) - 1

    def add(arr, type_, ctype):
        accessors.append({"bufferView": view(np.ascontiguousarray(arr).tobytes()), "componentType": ctype, "count": len(arr), "type": type_})
        return len(accessors) - 1

    def add_delta(d):
        if storage == "dense":
            return add(d, "VEC3", 5126)
        rows = np.flatnonzero((d != 0).any(axis=1))
        it = {5121: np.uint8, 5123: np.uint16, 5125: np.uint32}[index_type]
        acc = {"componentType": 5126, "count": len(d), "type": "VEC3",
               "sparse": {"count": len(rows), "indices": {"bufferView": view(rows.astype(it).tobytes()), "componentType": index_type},
                          "values": {"bufferView": view(np.ascontiguousarray(d[rows]).tobytes())}}}
        if base_view:
            junk = d.copy(); junk[rows] = 99.0
            acc["bufferView"] = view(junk.tobytes())
        accessors.append(acc)
        return len(accessors) - 1

    if baked is not None:
        p = (p + dp[baked]).astype(F)                                        # (float32 sums: what a weight of exactly 1 computes)
        if with_normal:
            nrm = (nrm + dn[baked]).astype(F)
        if with_tangent:
            tan = tan.copy(); tan[:, :3] = (tan[:, :3] + dt[baked]).astype(F)
    attrs = {"POSITION": add(p, "VEC3", 5126), "NORMAL": add(nrm, "VEC3", 5126), "TEXCOORD_0": add(uv, "VEC2", 5126)}
    if tangent_attr:
        attrs["TANGENT"] = add(tan, "VEC4", 5126)
    if skin:
        attrs["JOINTS_0"], attrs["WEIGHTS_0"] = add(joints.astype(np.uint8), "VEC4", 5121), add(w.astype(F), "VEC4", 5126)
    prim = {"attributes": attrs, "indices": add(idx, "SCALAR", 5123)}
    if baked is None:
        prim["targets"] = []
        for k in range(2):
            t = {"POSITION": add_delta(dp[k])}
            if with_normal:
                t["NORMAL"] = add_delta(dn[k])
            if with_tangent and tangent_attr:
                t["TANGENT"] = add_delta(dt[k])
            prim["targets"].append(t)
    mesh = {"primitives": [prim]}
    if mesh_weights is not None:
        mesh["weights"] = mesh_weights
    body = {"name": "body", "mesh": 0, "translation": [0.0, 0.5, 0.25]}
    if node_weights is not None:
        body["weights"] = node_weights
    nodes = [{"name": "root", "children": [1]}, body]
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": nodes, "meshes": [mesh]}
    if skin:
        body["skin"] = 0
        nodes += [{"name": "j0", "translation": [-2.0, 0.0, 0.0], "children": [3]},
                  {"name": "j1", "translation": [2.0, 0.0, 0.0], "rotation": quat_z(10.0), "children": [4]}, {"name": "j2", "translation": [2.0, 0.0, 0.0]}]
        nodes[0]["children"].append(2)
        doc["skins"] = [{"joints": [2, 3, 4]}]
    if two_nodes:
        nodes.append({"name": "twin", "mesh": 0, "translation": [0.0, -1.0, 0.0], "weights": [0.25, 0.5]})
        nodes[0]["children"].append(len(nodes) - 1)
    if animations and baked is None:
        times = add(F(KEY_TIMES), "SCALAR", 5126)
        out = add(F(KEY_WEIGHTS).reshape(-1), "SCALAR", 5126)
        linear = {"samplers": [{"input": times, "output": out, "interpolation": "LINEAR"}], "channels": [{"sampler": 0, "target": {"node": 1, "path": "weights"}}]}
        step = {"samplers": [{"input": times, "output": out, "interpolation": "STEP"}], "channels": [{"sampler": 0, "target": {"node": 1, "path": "weights"}}]}
        if skin:                                                            # joint channels and a weights channel in ONE animation
            rt = add(F([0.0, 1.0, 2.0]), "SCALAR", 5126)
            rv = add(F([quat_z(0), quat_z(50), quat_z(-30)]), "VEC4", 5126)
            linear["samplers"].append({"input": rt, "output": rv})
            linear["channels"].append({"sampler": 1, "target": {"node": 3, "path": "rotation"}})
        cubic = {"samplers": [{"input": add(F([0.0, 1.0]), "SCALAR", 5126), "output": add(np.zeros(12, F), "SCALAR", 5126), "interpolation": "CUBICSPLINE"}],
                 "channels": [{"sampler": 0, "target": {"node": 1, "path": "weights"}}]}
        stray = {"samplers": [{"input": times, "output": out}], "channels": [{"sampler": 0, "target": {"node": 0, "path": "weights"}}]}    # the root has no mesh
        doc["animations"] = [linear, step, cubic, stray]
    binary = b"".join(blobs)
    doc.update(bufferViews=views, accessors=accessors,
               buffers=[{"byteLength": len(binary), "uri": "data:application/octet-stream;base64," + base64.b64encode(binary).decode()}])
    if edit is not None:
        edit(doc)
    path = os.path.join(str(tmp), name)
    json.dump(doc, open(path, "w"))
    return path, dict(dp=dp, dn=dn, dt=dt, tangent=tan, doc=doc)
