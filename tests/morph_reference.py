"""The arbiter of morph targets (include/arctic_hip.h, arctic_set_mesh_morph_weights): numpy in float32, the product rounded once, then the
sum rounded once, per element, over the targets of non-zero weight in ascending index.  The device kernel (csrc/morph.hip) and the host
restatement (arctic_morph_vertices) must reproduce it bit for bit.

    m[e] = base[e];   for k in k0 < k1 < ... (w[k] != 0):   m[e] = m[e] + w[k] * delta[k][v][e]        e = the 12 floats of the four vectors
    uv'  = uv
"""
import numpy as np

MORPH_DTYPE = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("tangent", "<f4", 3), ("bitangent", "<f4", 3)])
VERTEX_FIELDS = ("position", "normal", "tangent", "bitangent")
F = np.float32


def morph_vertices(vertices, deltas, weights):
    """the blended copy of `vertices` (records with position, normal, tangent, bitangent, tex_coords); deltas (n_targets, n_vertices)
    MORPH_DTYPE records, weights n_targets float32"""
    w = np.asarray(weights, F).ravel()
    assert deltas.shape == (len(w), len(vertices))
    out = vertices.copy()
    for k in range(len(w)):
        if w[k] == 0:                                  # either sign of zero: the target is skipped, not added as 0 * d
            continue
        for name in VERTEX_FIELDS:
            p = w[k] * deltas[k][name]                 # the product, rounded to float32 ...
            assert p.dtype == F
            out[name] = out[name] + p                  # ... then the sum, rounded to float32
    return out


def random_case(rng, n_vertices, n_targets, vertex_dtype):
    """vertices, deltas and weights for the bit-exactness tests: weights include negatives, values above 1, exact zeros of both signs and a
    denormal; some base elements are -0.0"""
    v = np.zeros(n_vertices, vertex_dtype)
    for name in VERTEX_FIELDS:
        v[name] = rng.normal(size=(n_vertices, 3)).astype(F)
    v["tex_coords"] = rng.uniform(size=(n_vertices, 2)).astype(F)
    v["normal"][::3, 1] = F(-0.0)
    d = np.zeros((n_targets, n_vertices), MORPH_DTYPE)
    for name in VERTEX_FIELDS:
        d[name] = rng.normal(scale=0.3, size=(n_targets, n_vertices, 3)).astype(F)
    w = rng.uniform(-1.5, 2.5, size=n_targets).astype(F)
    kind = np.arange(n_targets) % 7
    w[kind == 3] = F(0.0)
    w[kind == 5] = F(-0.0)
    if n_targets > 6:
        w[6] = F(1e-41)                                # a denormal weight
    if (w == 0).all():
        w[0] = F(0.75)
    return v, d, w
