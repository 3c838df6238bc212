"""glTF files with a skin and animations, written by the tests that read them (test_gltf_skins.py, test_gltf_skins_malformed.py,
test_gpu_skinning.py), and the float64 evaluation of their poses the loader is checked against."""
import base64
import json
import os

import numpy as np


# ---- float64 reference of arctic_gltf_pose ---------------------------------------------------------------------------------------------
def quat_z(deg):
    a = np.radians(deg) / 2
    return [0.0, 0.0, float(np.sin(a)), float(np.cos(a))]


def unit(q):
    q = np.asarray(q, np.float64)
    l = np.sqrt((q * q).sum())
    return q / l if l > 0 and np.isfinite(l) else np.array([0.0, 0.0, 0.0, 1.0])


def trs(t, q, s):
    x, y, z, w = q
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)
    m = np.eye(4)
    m[:3, :3] = r * np.asarray(s, np.float64)[None, :]
    m[:3, 3] = t
    return m


def slerp(a, b, u):
    d = float((a * b).sum())
    if d < 0:
        b, d = -b, -d
    if d > 1 - 1e-12:
        return unit(a + (b - a) * u)
    th = np.arccos(d)
    return (np.sin((1 - u) * th) * a + np.sin(u * th) * b) / np.sin(th)


def sample(times, values, t, step, rotation):
    times = np.asarray(times, np.float32).astype(np.float64)
    values = np.asarray(values, np.float32).astype(np.float64)
    if rotation:
        values = np.stack([unit(v) for v in values])
    if t <= times[0]:
        return values[0]
    if t >= times[-1]:
        return values[-1]
    k = int(np.searchsorted(times, t, side="right")) - 1
    if step or t == times[k]:
        return values[k]
    u = (t - times[k]) / (times[k + 1] - times[k])
    return slerp(values[k], values[k + 1], u) if rotation else values[k] + (values[k + 1] - values[k]) * u


class Rig:
    """the document's nodes, skin and animations as Python data; pose() is the definition of include/arctic_gltf.h in float64"""

    def __init__(self, nodes, joints, inverse_bind, mesh_node, animations):
        self.nodes, self.joints, self.inverse_bind, self.mesh_node, self.animations = nodes, joints, inverse_bind, mesh_node, animations
        self.parent = {}
        for i, n in enumerate(nodes):
            for c in n.get("children", []):
                self.parent[c] = i

    def local(self, i, over):
        n = self.nodes[i]
        if "matrix" in n and i not in over:
            return np.asarray(n["matrix"], np.float64).reshape(4, 4).T
        o = over.get(i, {})
        return trs(o.get("translation", n.get("translation", [0, 0, 0])), o.get("rotation", unit(n.get("rotation", [0, 0, 0, 1]))),
                   o.get("scale", n.get("scale", [1, 1, 1])))

    def world(self, i, over):
        m = self.local(i, over)
        while i in self.parent:
            i = self.parent[i]
            m = self.local(i, over) @ m
        return m

    def pose(self, animation, t):
        over = {}
        if animation >= 0:
            for node, path, times, values, interp in self.animations[animation]:
                over.setdefault(node, {})[path] = sample(times, values, t, interp == "STEP", path == "rotation")
        inv_mesh = np.linalg.inv(self.world(self.mesh_node, over))
        return np.stack([inv_mesh @ self.world(j, over) @ self.inverse_bind[k] for k, j in enumerate(self.joints)])     # math matrices [row][col]


# ---- the file ----------------------------------------------------------------------------------------------------------------------------
def bar_geometry(n=9):
    """a strip along x from -2 to 2 in the plane z = 0, facing +z; three joints at x = -2, 0, 2"""
    x = np.linspace(-2, 2, n)
    p = np.array([(xi, y, 0.0) for xi in x for y in (-0.3, 0.3)], np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (len(p), 1))
    uv = np.array([((xi + 2) / 4, 0.5 - y) for xi in x for y in (-0.3, 0.3)], np.float32)
    idx = []
    for k in range(n - 1):
        a = 2 * k
        idx += [a, a + 2, a + 1, a + 1, a + 2, a + 3]
    t = (p[:, 0].astype(np.float64) + 2) / 2
    k = np.clip(np.floor(t), 0, 1).astype(np.int64)
    f = t - k
    joints = np.zeros((len(p), 4), np.int64)
    weights = np.zeros((len(p), 4), np.float64)
    joints[:, 0], joints[:, 1], weights[:, 0], weights[:, 1] = k, k + 1, 1 - f, f
    return p, nrm, uv, np.array(idx, np.uint16), joints, weights


def write_skinned(tmp, name="skinned.gltf", joints_type=5121, weights="float", inverse_bind=True, parent=True, second_skin=False, extra_animations=True,
                  edit=None):
    """returns (path, Rig, dict of the arrays written).  `edit(doc)` may change the JSON document before it is written (malformed files)."""
    p, nrm, uv, idx, joints, w = bar_geometry()
    blobs, views, accessors = [], [], []

    def add(arr, type_, ctype, normalized=False):
        data = np.ascontiguousarray(arr).tobytes()
        off = sum(len(b) for b in blobs)
        pad = (-off) % 4
        blobs.append(b"\0" * pad + data)
        views.append({"buffer": 0, "byteOffset": off + pad, "byteLength": len(data)})
        acc = {"bufferView": len(views) - 1, "componentType": ctype, "count": len(arr), "type": type_}
        if normalized:
            acc["normalized"] = True
        accessors.append(acc)
        return len(accessors) - 1

    if weights == "float":
        w_arr, w_acc = w.astype(np.float32), (5126, False)
    elif weights == "u8":
        w_arr, w_acc = np.round(w * 255).astype(np.uint8), (5121, True)
    else:
        w_arr, w_acc = np.round(w * 65535).astype(np.uint16), (5123, True)
    j_arr = joints.astype(np.uint8 if joints_type == 5121 else np.uint16)
    a = dict(p=add(p, "VEC3", 5126), n=add(nrm, "VEC3", 5126), uv=add(uv, "VEC2", 5126), i=add(idx, "SCALAR", 5123),
             j=add(j_arr, "VEC4", joints_type), w=add(w_arr, "VEC4", *w_acc))
    root = {"name": "root", "children": [1, 4]}
    if parent:
        root.update(translation=[0.5, 1.25, -0.75], rotation=[0.0, 0.3826834323650898, 0.0, 0.9238795325112867], scale=[1.5, 1.5, 1.5])
    nodes = [root,
             {"name": "j0", "translation": [-2.0, 0.0, 0.0], "children": [2]},
             {"name": "j1", "translation": [2.0, 0.0, 0.0], "rotation": quat_z(10.0), "children": [3]},
             {"name": "j2", "translation": [2.0, 0.0, 0.0]},
             {"name": "body", "mesh": 0, "skin": 0, "translation": [0.0, 0.5, 0.25]}]
    joint_nodes = [1, 2, 3]
    rig = Rig(nodes, joint_nodes, None, 4, [])
    bind = [np.linalg.inv(rig.world(j, {})) @ rig.world(4, {}) for j in joint_nodes]       # the rest pose is then the identity (up to rounding)
    bind32 = np.stack([b.T.reshape(16) for b in bind]).astype(np.float32)                   # column-major, as the file stores them
    skin = {"joints": joint_nodes}
    if inverse_bind:
        skin["inverseBindMatrices"] = add(bind32, "MAT4", 5126)
        rig.inverse_bind = [bind32[k].astype(np.float64).reshape(4, 4).T for k in range(3)]
    else:
        rig.inverse_bind = [np.eye(4)] * 3
    anims = [
        [(2, "rotation", [0.0, 1.0, 2.0], [quat_z(0), quat_z(60), quat_z(-30)], "LINEAR"),
         (3, "translation", [0.5, 1.5], [[2.0, 0.0, 0.0], [2.0, 1.0, 0.5]], "LINEAR"),
         (2, "scale", [0.0, 1.0], [[1, 1, 1], [1.5, 1.25, 1.0]], "STEP")],
        [(2, "rotation", [0.25, 1.0, 1.75], [quat_z(20), [0.0, 0.0, 2.0, 2.0], quat_z(170)], "STEP"),      # a keyframe that is not unit length
         (1, "translation", [0.0, 2.0], [[-2.0, 0.0, 0.0], [-2.0, 0.5, 0.0]], "LINEAR")],
    ]
    rig.animations = anims
    doc_anims = []
    for chans in anims:
        samplers, channels = [], []
        for node, path, times, values, interp in chans:
            samplers.append({"input": add(np.asarray(times, np.float32), "SCALAR", 5126),
                             "output": add(np.asarray(values, np.float32), "VEC4" if path == "rotation" else "VEC3", 5126), "interpolation": interp})
            channels.append({"sampler": len(samplers) - 1, "target": {"node": node, "path": path}})
        doc_anims.append({"samplers": samplers, "channels": channels})
    if extra_animations:   # they do not refuse the file: only posing with them fails
        t3 = add(np.float32([0.0, 1.0]), "SCALAR", 5126)
        cubic = add(np.zeros((6, 3), np.float32), "VEC3", 5126)
        doc_anims.append({"samplers": [{"input": t3, "output": cubic, "interpolation": "CUBICSPLINE"}],
                          "channels": [{"sampler": 0, "target": {"node": 3, "path": "translation"}}]})
        morph = add(np.float32([0.0, 1.0]), "SCALAR", 5126)
        doc_anims.append({"samplers": [{"input": t3, "output": morph}], "channels": [{"sampler": 0, "target": {"node": 4, "path": "weights"}}]})
    skins = [skin]
    if second_skin:        # the same mesh under another skin (two joints, no inverse bind matrices): a second loader mesh
        nodes.append({"name": "body2", "mesh": 0, "skin": 1})
        nodes[0]["children"].append(5)
        skins.append({"joints": [1, 2, 3, 0]})
    prim = {"attributes": {"POSITION": a["p"], "NORMAL": a["n"], "TEXCOORD_0": a["uv"], "JOINTS_0": a["j"], "WEIGHTS_0": a["w"]}, "indices": a["i"]}
    binary = b"".join(blobs)
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": nodes, "meshes": [{"primitives": [prim]}],
           "skins": skins, "animations": doc_anims, "bufferViews": views, "accessors": accessors,
           "buffers": [{"byteLength": len(binary), "uri": "data:application/octet-stream;base64," + base64.b64encode(binary).decode()}]}
    if edit is not None:
        edit(doc)
    path = os.path.join(str(tmp), name)
    json.dump(doc, open(path, "w"))
    return path, rig, dict(position=p, joints=joints, weights=w, weights_written=w_arr, doc=doc)
