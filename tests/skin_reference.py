"""The arbiter of skeletal skinning (include/arctic_hip.h, arctic_set_mesh_pose): numpy in float32, every operation rounded once, in the
header's order.  The device kernel (csrc/skin.hip) and the host restatement (arctic_skin_vertices) must reproduce it bit for bit.

    S[e]  = ((w0*J[j0][e] + w1*J[j1][e]) + w2*J[j2][e]) + w3*J[j3][e]
    pos'  = ((S[i]*x + S[4+i]*y) + S[8+i]*z) + S[12+i]*1.0f          i = 0..2
    v'    =  (S[i]*x + S[4+i]*y) + S[8+i]*z                          normal, tangent, bitangent
    uv'   = uv
"""
import numpy as np

SKIN_DTYPE = np.dtype([("joints", "<u2", 4), ("weights", "<f4", 4)])
VERTEX_FIELDS = ("position", "normal", "tangent", "bitangent")
F = np.float32


def blended(skin, joints):
    """(n, 16) float32: S per vertex; joints (n_joints, 16) float32 in glm memory order (element 4 * column + row)"""
    J = np.ascontiguousarray(joints, F).reshape(-1, 16)
    j, w = skin["joints"].astype(np.int64), skin["weights"].astype(F)
    S = w[:, 0:1] * J[j[:, 0]]
    S = S + w[:, 1:2] * J[j[:, 1]]
    S = S + w[:, 2:3] * J[j[:, 2]]
    S = S + w[:, 3:4] * J[j[:, 3]]
    assert S.dtype == F
    return S


def skin_vertices(vertices, skin, joints):
    """the posed copy of `vertices` (records with position, normal, tangent, bitangent, tex_coords)"""
    S = blended(skin, joints)
    out = vertices.copy()
    for name in VERTEX_FIELDS:
        v = vertices[name].astype(F)
        x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]
        r = (S[:, 0:3] * x + S[:, 4:7] * y) + S[:, 8:11] * z
        if name == "position":
            r = r + S[:, 12:15] * F(1.0)
        assert r.dtype == F
        out[name] = r
    return out


def random_case(rng, n_vertices, n_joints, vertex_dtype):
    """vertices, skin records and joint matrices for the bit-exactness tests: weights include exact 0 and 1 and the same joint in several
    slots; the matrices are rotations with scale and translation (nothing special: the arithmetic is what is tested)"""
    v = np.zeros(n_vertices, vertex_dtype)
    for name in VERTEX_FIELDS:
        v[name] = rng.normal(size=(n_vertices, 3)).astype(F)
    v["tex_coords"] = rng.uniform(size=(n_vertices, 2)).astype(F)
    s = np.zeros(n_vertices, SKIN_DTYPE)
    s["joints"] = rng.integers(0, n_joints, size=(n_vertices, 4))
    w = rng.uniform(size=(n_vertices, 4)).astype(F)
    w /= w.sum(axis=1, keepdims=True)
    kind = np.arange(n_vertices) % 5
    w[kind == 1] = (1, 0, 0, 0)                       # one joint, weight exactly 1, the others exactly 0
    w[kind == 2, 2:] = 0                              # two joints
    same = kind == 3                                  # the same joint in several slots
    s["joints"][same, 1] = s["joints"][same, 0]
    s["joints"][same, 3] = s["joints"][same, 0]
    s["weights"] = w
    J = np.zeros((n_joints, 4, 4), F)                 # math matrices M[row][col]
    for k in range(n_joints):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        J[k, :3, :3] = (q * rng.uniform(0.5, 1.5)).astype(F)
        J[k, :3, 3] = rng.uniform(-2, 2, size=3).astype(F)
        J[k, 3, 3] = 1
    return v, s, np.ascontiguousarray(J.transpose(0, 2, 1)).reshape(n_joints, 16)
