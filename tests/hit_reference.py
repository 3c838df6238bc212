"""The attributes at a ray hit and the reflection ray in numpy float32, written from include/arctic_hip.h alone ("what is AT a hit"): every
operation rounds once, in the header's order.  It never calls the product library.  tests/test_hit_reference.py compares the host arbiter
arctic_interpolate_hits with it bit for bit, tests/test_gpu_hit_attributes.py the device.

`hit_attributes(..., defect=...)` evaluates a deliberately WRONG variant (DEFECTS), as ray_reference and ao_reference do: the CPU tests use them
to show that the test scene's inputs tell each such defect from the truth."""
import numpy as np

F = np.float32
NO_PRIM = 0xFFFFFFFF
NO_MATERIAL = 0xFFFFFFFF
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("t_min", "<f4"), ("direction", "<f4", 3), ("t_max", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4")])
DEFECTS = ("uv_swapped", "w0_on_wrong_vertex", "other_instance_trs", "skipped_triangle_not_counted", "tangent_bitangent_swapped", "light_space_from_wrong_matrix")


def _mat_vec(M, x, y, z, w):
    """((M[i]*x + M[4+i]*y) + M[8+i]*z) + M[12+i]*w for i = 0..3: M = 16 floats in glm order"""
    M = np.asarray(M, F).reshape(16)
    return [((M[i] * x + M[4 + i] * y) + M[8 + i] * z) + M[12 + i] * w for i in range(4)]


def _normalize(v):
    inv = F(1.0) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return v * inv[:, None]


def vertex_attributes(vertices, trs, light_proj_view, defect=None):
    """(n, 18) float32: what the vertex kernel writes per vertex (uv2, t3, b3, n3, world3, light_space4)"""
    with np.errstate(all="ignore"):
        p = np.ascontiguousarray(vertices["position"], F)
        world = _mat_vec(trs, p[:, 0], p[:, 1], p[:, 2], F(1.0))
        L = np.asarray(light_proj_view, F).reshape(16)
        if defect == "light_space_from_wrong_matrix":
            L = L.reshape(4, 4).T.reshape(16).copy()
        ls = _mat_vec(L, world[0], world[1], world[2], world[3])
        t, b, n = (_normalize(np.ascontiguousarray(vertices[k], F)) for k in ("tangent", "bitangent", "normal"))
        if defect == "tangent_bitangent_swapped":
            t, b = b, t
        uv = np.ascontiguousarray(vertices["tex_coords"], F)
        return np.concatenate([uv, t, b, n, np.stack(world[:3], -1), np.stack(ls, -1)], 1).astype(F)


def prim_sources(objects, meshes, defect=None):
    """the scene's triangles in prim order: (object, indices (m, 3), ok) -- objects in order, an object without a mesh has none, the triangle
    with an index out of range is skipped (ok False) but numbered"""
    obj, idx, ok = [], [], []
    for k, ob in enumerate(objects):
        if int(ob["mesh_idx"]) >= len(meshes):
            continue
        verts, ind = meshes[int(ob["mesh_idx"])]
        ix = np.asarray(ind, np.int64).reshape(-1, 3)
        good = (ix < len(verts)).all(1)
        if defect == "skipped_triangle_not_counted":
            ix, good = ix[good], good[good]
        obj.append(np.full(len(ix), k, np.int64)); idx.append(ix); ok.append(good)
    if not obj:
        return np.zeros(0, np.int64), np.zeros((0, 3), np.int64), np.zeros(0, bool)
    return np.concatenate(obj), np.concatenate(idx), np.concatenate(ok)


def hit_attributes(objects, meshes, mesh_materials, light_proj_view, hits, defect=None):
    """-> ((n, 18) float32, (n,) uint32).  objects: records with "trs" and "mesh_idx"; meshes: (vertices IN USE, indices) per mesh;
    mesh_materials: the material of each mesh; light_proj_view: 16 floats, glm order; hits: HIT_DTYPE records"""
    assert defect is None or defect in DEFECTS, defect
    hits = np.asarray(hits, HIT_DTYPE).ravel()
    attrs, material = np.zeros((len(hits), 18), F), np.full(len(hits), NO_MATERIAL, np.uint32)
    obj, idx, ok = prim_sources(objects, meshes, defect)
    prim = hits["prim"].astype(np.int64)
    resolved = (prim != NO_PRIM) & (prim < len(obj))
    resolved[resolved] = ok[prim[resolved]]
    u, v = (hits["v"], hits["u"]) if defect == "uv_swapped" else (hits["u"], hits["v"])
    for k in np.unique(obj[prim[resolved]]) if resolved.any() else []:
        sel = np.nonzero(resolved)[0]
        sel = sel[obj[prim[sel]] == k]
        ob = objects[int(k)]
        trs = ob["trs"]
        if defect == "other_instance_trs":
            others = [o for j, o in enumerate(objects) if j != k and int(o["mesh_idx"]) == int(ob["mesh_idx"])]
            trs = others[0]["trs"] if others else trs
        va = vertex_attributes(meshes[int(ob["mesh_idx"])][0], trs, light_proj_view, defect)
        i0, i1, i2 = (idx[prim[sel], c] for c in range(3))
        if defect == "w0_on_wrong_vertex":
            i0, i1, i2 = i1, i2, i0
        with np.errstate(all="ignore"):
            w0 = (F(1.0) - u[sel]) - v[sel]
            attrs[sel] = (w0[:, None] * va[i0] + u[sel][:, None] * va[i1]) + v[sel][:, None] * va[i2]
        material[sel] = mesh_materials[int(ob["mesh_idx"])]
    return attrs, material


def same_bytes(a):
    """the bytes to compare attributes by: every NaN as ONE pattern -- a NaN u or v propagates into a NaN whose sign and payload the header leaves
    undefined (they differ between the host's and the device's arithmetic); everything else, zeros' signs included, bit for bit"""
    a = np.asarray(a, F)
    return np.where(np.isnan(a), F(np.nan), a).tobytes()


def unit_normal(n):
    """step 1 of the ambient occlusion: m = n / len and whether the pixel is covered by it"""
    n = np.asarray(n, F)
    with np.errstate(all="ignore"):
        ln = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
        m = n / ln[..., None]
    return m, (ln != 0) & np.isfinite(ln) & np.isfinite(m).all(-1)


def reflection_rays(attrs, material, eye, bias):
    """arctic_trace_reflections' rays from arctic_read_gbuffer's attributes (rows, width, 18) and materials: RAY_DTYPE (rows * width,), the
    all-zero record for a pixel without a ray; also the mask of the pixels that have one"""
    a = np.asarray(attrs, F).reshape(-1, 18)
    world, eye = a[:, 11:14], np.asarray(eye, F)
    m, ok = unit_normal(a[:, 8:11])
    with np.errstate(all="ignore"):
        i = world - eye
        k = (m[:, 0] * i[:, 0] + m[:, 1] * i[:, 1]) + m[:, 2] * i[:, 2]
        d = i - (F(2.0) * k)[:, None] * m
        o = world + F(bias) * m
    has = (np.asarray(material).reshape(-1) != NO_MATERIAL) & ok & ~(k >= 0)
    rays = np.zeros(len(a), RAY_DTYPE)
    rays["origin"][has], rays["direction"][has], rays["t_max"][has] = o[has], d[has], np.inf
    return rays, has
