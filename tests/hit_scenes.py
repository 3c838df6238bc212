"""The scene of the hit tests (tests/test_hit_reference.py on the CPU; tests/test_gpu_hit_attributes.py, tests/test_gpu_hit_shading.py and
tests/test_gpu_reflections.py on the device), made once per material assignment and never changed, with the conditions that keep a comparison
from being vacuous, asserted by both sides.

Small, but every mapping that can go wrong is in it: four entries in the object list over two meshes -- two instances of a box (one under a
rotation and a non-uniform scale, one under another rotation), an entry whose mesh does not exist BETWEEN them (it has no triangles and takes no
prim numbers), and a floor under the identity with one index triple out of range in the middle of its index buffer (skipped, but numbered) --,
195 prims in all; tangent frames that are neither unit nor orthogonal and differ from vertex to vertex; four materials as in
test_gpu_extended_shading._materials (64 x 64 packed, 32 x 16 packed, unequal sizes, 1 x 1), two of them in use per ASSIGNMENT of materials to
the two meshes; a 64 x 64 sun map, 5 point lights, a 64 x 32 environment map; 4096 rays from 8 origins (one below the floor: back faces) with
misses, NaN, infinite and zero directions, hit records moved onto the edges u = 0, v = 0 and u + v = 1, and hand-made records whose prim is
the skipped triangle's, the scene's count, beyond it, and 0xFFFFFFFE."""
from types import SimpleNamespace

import numpy as np

import hit_reference as HR
import ray_reference as R
import shading_reference as SR
import test_gpu_extended_shading as G

F = np.float32
SHADOW, MAX_LIGHTS, ENV_SIZE = 64, 16, (64, 32)
ASSIGNMENTS = {"packed 64 / unequal": (0, 2), "packed 32x16 / 1x1": (1, 3)}   # the materials of (box, floor)
N_ORIGINS, RAYS_PER_ORIGIN = 8, 512
MISSING_MESH = 7
LEFT_OUT_CAP = 0.05          # share of the covered hits a test may leave out (grazing views)
AMBIENT = 0.3
SETTINGS = (0, 2.2, 1.0)
_made = {}


def _skew_frames(rng, v):
    """tangent frames that are neither unit nor orthogonal, each vertex its own: what normalize3 and the interpolation have to carry"""
    for k in ("normal", "tangent", "bitangent"):
        a = v[k].astype(np.float64)
        a = a / np.linalg.norm(a, axis=1, keepdims=True) + 0.15 * rng.normal(size=a.shape)
        v[k] = (a * rng.uniform(0.5, 2.0, (len(a), 1))).astype(F)
    v["tex_coords"] += rng.uniform(-0.05, 0.05, v["tex_coords"].shape).astype(F)
    return v


def geometry(pkg):
    """-> Case(meshes, objects, moved, tris, prims, n_prims, skipped): moved = the object list with the rotated box elsewhere (the refit)"""
    def make():
        sc = pkg.scenes
        rng = np.random.default_rng(61001)
        bv, bi = sc.box(1.6, 1.2, 1.0, 2, 2.0)
        fv, fi = sc.quad((-3, 0, 3), (6, 0, 0), (0, 0, -6), 7, 7, (3.0, 3.0))
        mid = 3 * (len(fi) // 6)
        fi = np.concatenate([fi[:mid], np.array([0, 1, len(fv)], np.uint32), fi[mid:]])        # skipped, but it takes a prim number
        meshes = [(_skew_frames(rng, bv), bi), (_skew_frames(rng, fv), fi)]
        c, s = np.cos(0.6), np.sin(0.6)
        turned = np.array([[c, 0, s, -1.1], [0, 1, 0, 1.0], [-s, 0, c, 0.3], [0, 0, 0, 1]]) @ np.diag([1.3, 0.7, 1.1, 1.0])   # a rotation and a non-uniform scale
        c, s = np.cos(-1.1), np.sin(-1.1)
        other = np.array([[1, 0, 0, 1.2], [0, c, -s, 1.4], [0, s, c, -0.8], [0, 0, 0, 1]])
        places = [(turned, 0), (np.eye(4), MISSING_MESH), (other, 0), (np.eye(4), 1)]
        objects = pkg.scene.make_objects(places)
        places[0] = (np.array([[c, 0, s, -0.6], [0, 1, 0, 1.3], [-s, 0, c, 0.9], [0, 0, 0, 1]]) @ np.diag([1.1, 0.9, 1.2, 1.0]), 0)
        moved = pkg.scene.make_objects(places)
        tris, prims = R.world_triangles(objects, meshes)
        first_floor = 2 * (len(bi) // 3)
        return SimpleNamespace(meshes=meshes, objects=objects, moved=moved, tris=tris, prims=prims, n_prims=first_floor + len(fi) // 3,
                               skipped=first_floor + mid // 3)
    if "geometry" not in _made:
        _made["geometry"] = make()
    return _made["geometry"]


def description(pkg, objects):
    camera = dict(eye=(-3.2, 2.9, 4.2), rotation=(-27.0, -52.0), aspect=1.5, fov_y=45.0, z_near_far=(0.1, 100.0))
    return pkg.scenes.SceneDesc(camera=camera, ambient=AMBIENT, sun=pkg.scenes.DEFAULT_SUN, objects=objects)


def _aimed(rng, tris, origins, n):
    """n rays per origin towards random points of random triangles"""
    t = tris.reshape(-1, 3, 3)
    pick = t[rng.integers(0, len(t), (len(origins), n))]
    bary = rng.dirichlet(np.ones(3), (len(origins), n)).astype(F)
    target = (pick * bary[..., None]).sum(2)
    return (target - origins[:, None, :]).astype(F)


def _trace(pkg, g, rays):
    hits = pkg.renderer.trace_triangles(g.tris, rays)
    found = hits["prim"] != HR.NO_PRIM
    hits["prim"][found] = g.prims[hits["prim"][found]]                      # the arbiter numbers the triangles it is given; the scene numbers the skipped one too
    return hits


def scene(pkg, assignment):
    """-> Case(g, desc, images, materials, mesh_materials, lights, env_map, rays, hits, origin_of, edge, handmade)"""
    def make():
        g = geometry(pkg)
        rng = np.random.default_rng(62000 + list(ASSIGNMENTS).index(assignment))
        images = G._materials(pkg, np.random.default_rng(62999))
        c = SimpleNamespace(g=g, desc=description(pkg, g.objects), images=images, materials=G.host_materials(images, False),
                            mesh_materials=ASSIGNMENTS[assignment], env_map=pkg.scenes.synthetic_hdri(*ENV_SIZE),
                            lights=pkg.scenes.random_lights(rng, 5, (-3, 0.5, -3), (3, 3, 3), intensity=10.0))
        ang = np.linspace(0, 2 * np.pi, N_ORIGINS - 1, endpoint=False)
        origins = np.stack([5.0 * np.cos(ang), rng.uniform(1.0, 4.0, len(ang)), 5.0 * np.sin(ang)], 1)
        origins = np.concatenate([origins, [[0.3, -2.0, 0.2]]]).astype(F)        # ... and one below the floor: its back face
        n_aimed = RAYS_PER_ORIGIN * 3 // 4
        d = np.concatenate([_aimed(rng, g.tris, origins, n_aimed), rng.normal(size=(N_ORIGINS, RAYS_PER_ORIGIN - n_aimed, 3)).astype(F)], 1)
        c.origin_of = np.repeat(np.arange(N_ORIGINS), RAYS_PER_ORIGIN)
        rays = R.make_rays(np.repeat(origins, RAYS_PER_ORIGIN, 0), d.reshape(-1, 3))
        # invalid rays (misses by definition): the last eight of every origin's random block
        bad = [(np.nan, 0, 1), (0, 0, 0), (-0.0, 0, 0), (np.inf, 1, 0), (0, -np.inf, 0), (1, np.nan, np.nan), (0, 0, np.nan), (np.inf, np.inf, np.inf)]
        for k in range(N_ORIGINS):
            rays["direction"][(k + 1) * RAYS_PER_ORIGIN - len(bad):(k + 1) * RAYS_PER_ORIGIN] = np.array(bad, F)
        lpv = pkg.renderer.frame_constants(c.desc)[1].reshape(16)
        for _ in range(20):                                                  # steer clear of grazing views, with the reference alone
            hits = _trace(pkg, g, rays)
            attrs, mat = HR.hit_attributes(g.objects, g.meshes, c.mesh_materials, lpv, hits)
            graze = grazing(c, rays, attrs, mat)
            if not graze.any():
                break
            again = np.nonzero(graze)[0]
            rays["direction"][again] = _aimed(rng, g.tris, rays["origin"][again], 1)[:, 0]
        hits = _trace(pkg, g, rays)
        # hit records moved onto the triangle's edges, and hand-made ones (inputs like any other: the attributes take u, v and prim as given)
        found = np.nonzero(hits["prim"] != HR.NO_PRIM)[0]
        edge = rng.choice(found, 48, replace=False).reshape(3, 16)
        hits["u"][edge[0]] = 0.0
        hits["v"][edge[1]] = 0.0
        hits["v"][edge[2]] = F(1.0) - hits["u"][edge[2]]
        miss = np.nonzero(hits["prim"] == HR.NO_PRIM)[0]
        handmade = miss[:6]
        hits["prim"][handmade] = [g.skipped, g.n_prims, g.n_prims + 5, 0xFFFFFFFE, g.n_prims, g.skipped]
        hits["u"][handmade], hits["v"][handmade], hits["t"][handmade] = 0.25, 0.5, 1.0
        nan_uv = found[~np.isin(found, edge)][:2]                              # a NaN propagates
        hits["u"][nan_uv[0]], hits["v"][nan_uv[1]] = np.nan, np.nan
        c.rays, c.hits, c.edge, c.handmade, c.nan_uv, c.origins, c.lpv = rays, hits, edge, handmade, nan_uv, origins, lpv
        return c
    if assignment not in _made:
        _made[assignment] = make()
    return _made[assignment]


def grazing(c, rays, attrs, mat):
    """the covered hits whose |n.wo| is below GRAZING (test_gpu_extended_shading: the specular term there is proportional to an n.wo that fp32
    carries to parts in a thousand), n the normal-mapped normal, wo towards the ray's origin"""
    ch = SR.material_channels(c.materials, attrs, mat)
    with np.errstate(all="ignore"):
        n = SR.surface_normal(attrs, ch)
        wo = rays["origin"].astype(np.float64) - attrs[:, 11:14].astype(np.float64)
        wo /= np.linalg.norm(wo, axis=-1, keepdims=True)
        ndwo = np.abs((n * wo).sum(-1))
    return (mat != HR.NO_MATERIAL) & ~(ndwo >= G.GRAZING)


def sun_lit(oracle, shadow, attrs, mat):
    """1 - shadow per covered hit from the oracle's calculate_shadow on the given map (test_gpu_extended_shading.sun_lit); a hit whose attributes
    are not finite (a NaN u or v propagates) is not asked: it is not judged either"""
    ask = np.where(np.isfinite(attrs).all(1), mat, HR.NO_MATERIAL)
    return G.sun_lit(oracle, shadow, attrs[None], ask[None])[0]


def shade_reference(c, rays, attrs, mat, lit, eyes=None, env=True):
    """the float64 pixel per hit (shading_reference.shade per origin group, eye = the group's origin) and the environment along every other ray:
    -> Case(rgba (n, 4) float64, covered, judged).  eyes: an eye per origin instead of the origins themselves (the CPU test's wrong-eye variant)"""
    n = len(rays)
    rgba = np.zeros((n, 4))
    covered = mat != HR.NO_MATERIAL
    ch = SR.material_channels(c.materials, attrs, mat)
    for k in range(N_ORIGINS):
        sel = np.nonzero((c.origin_of == k) & covered)[0]
        eye = c.origins[k] if eyes is None else eyes[k]
        ref = SR.shade(attrs[sel], mat[sel], ch[sel], lit[sel], eye, c.desc.sun["rotation"], c.desc.sun["color"], c.desc.ambient, SETTINGS, points=c.lights)
        rgba[sel, :3], rgba[sel, 3] = ref["hdr"], 1.0
    d = rays["direction"].astype(np.float64)
    with np.errstate(all="ignore"):
        valid = np.isfinite(d).all(1) & (d != 0).any(1)
    sky = ~covered & valid
    if env and sky.any():
        import env_reference as ER
        u, v = ER.dir_uv(d[sky])
        rgba[sky, :3] = ER.sample_uv(c.env_map, u, v)
    judged = covered & ~grazing(c, rays, attrs, mat) & np.isfinite(attrs).all(1)
    return SimpleNamespace(rgba=rgba, covered=covered, judged=judged, sky=sky, invalid=~covered & ~valid)


def check_conditions(c, attrs, mat, judged=None):
    """what the inputs have to be for the comparisons to mean something"""
    g = c.g
    covered = mat != HR.NO_MATERIAL
    prim = c.hits["prim"]
    assert g.n_prims == 195 and len(g.tris) == 194
    assert covered.mean() >= 0.5 and (prim == HR.NO_PRIM).mean() >= 0.1                       # hits, and misses
    obj, _, _ = HR.prim_sources(g.objects, g.meshes)
    seen = np.bincount(obj[prim[covered]], minlength=4)
    assert (seen[[0, 2, 3]] >= 200).all() and seen[1] == 0                                    # every object that has triangles is hit, often
    assert (prim[covered] > g.skipped).sum() >= 100                                           # ... behind the skipped triangle as well
    assert not covered[c.handmade].any() and (attrs[c.handmade] == 0).all()
    assert covered[c.edge].all() and covered[c.nan_uv].all() and np.isnan(attrs[c.nan_uv]).any(1).all()
    d = c.rays["direction"]
    assert np.isnan(d).any(1).sum() >= N_ORIGINS and (d == 0).all(1).sum() >= N_ORIGINS and np.isinf(d).any(1).sum() >= N_ORIGINS
    used = set(np.unique(mat[covered]).tolist())
    assert used == set(c.mesh_materials), used
    below = c.origin_of == N_ORIGINS - 1
    assert (covered & below).sum() >= 100                                                     # the floor's back face
    if judged is not None:
        assert (covered & ~judged).sum() <= LEFT_OUT_CAP * covered.sum(), ((covered & ~judged).sum(), covered.sum())
    return {"covered": int(covered.sum()), "per object": seen.tolist()}


def upload(pkg, r, c, env=True):
    """materials, meshes, lights and the environment map of c into a handle"""
    for d, n, m in c.images:
        r.create_material(d, n, m)
    for (v, i), m in zip(c.g.meshes, c.mesh_materials):
        r.create_mesh(v, i, m)
    r.update_lights(c.lights)
    if env:
        r.create_hdri(c.env_map)
    return r


def arbiter_attributes(pkg, objects, meshes, mesh_materials, lpv, hits):
    """arctic_interpolate_hits chained over the objects, as the header describes"""
    attrs, material = np.zeros((len(hits), 18), F), np.full(len(hits), HR.NO_MATERIAL, np.uint32)
    prim = 0
    for ob in objects:
        if int(ob["mesh_idx"]) >= len(meshes):
            continue
        v, ix = meshes[int(ob["mesh_idx"])]
        pkg.renderer.interpolate_hits(v, ix, ob["trs"], lpv, mesh_materials[int(ob["mesh_idx"])], prim, hits, attrs, material)
        prim += len(ix) // 3
    return attrs, material
