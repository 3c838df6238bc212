"""The inputs of the ambient-occlusion tests (tests/test_ao_reference.py on the CPU, tests/test_gpu_ambient_occlusion.py on the device) with their
expected results, each made once and never changed, and the conditions that keep a comparison from being vacuous, asserted by both.

Injected G-buffers: ray_reference.soup_gbuffer of ray_scenes.SUN_SIZE over the 5- and the 1000-triangle scene of ray_scenes, with normals that are
not unit vectors, normals along +-z, and normals that are zero, underflow, overflow or are not finite written over some pixels.  Their direction
tables are cones (ao_reference.cone_directions) chosen per scene so that pixels with no hit, with every ray hitting and in between all occur --
in five triangles a cosine hemisphere almost never has all 64 rays hit, so that scene's cone points DOWN, back through the triangle the pixel
lies on (the library takes any table: no sign check).  ONE table of 16 sets x 64 directions per scene: the table of a case with n_rays = n and
pattern P is its first P * P sets and first n directions, so ray k of a pixel is the same ray in every n and the reference walks each (pattern,
radius) once, with 64 rays.

The rasterised scene: a floor, three boxes and a tilted quad; its G-buffer comes from the CPU oracle here and from the device in the device test,
bit for bit the same (tests/test_gpu_parity.py)."""
import numpy as np

import ao_reference as A
import ray_reference as R
import ray_scenes as S

F = np.float32
BIAS = 1e-3
N_RAYS = [1, 4, 5, 64]
PATTERNS = [1, 2, 4]
# per scene: the cone (half angle in degrees, pointing down?) and the finite radius
INJECTED = {5: dict(half=35.0, down=True, radius=4e-3), 1000: dict(half=20.0, down=False, radius=1.0)}
# directions with a zero component, and one at the subnormal edge (1e-45: its reciprocal overflows), next to a general one: for a pixel whose normal
# is +-x the world direction is (m0 * l2, l1, -m0 * l0), so these stay zero or subnormal there and the pixel's whole tile takes the odd walk
ODD_LOCAL = np.array([[0.0, 0.0, 1.0], [0.3, 0.4, 0.8], [1e-45, 0.5, 0.7], [0.0, 0.6, 0.8]], F)
SHARDS = {"rows 3..30": dict(row_begin=3, row_end=30), "bands of 8, shard 1 of 2": dict(band_rows=8, shard=(1, 2))}
FILTER = dict(normal_cos=0.9, plane_dist=0.05, radius=0.75, n_rays=4)


def table(master, n_rays, P):
    """the table of the case (n_rays, P): the master's first P * P sets and first n_rays directions, packed"""
    return np.ascontiguousarray(master[:P * P, :n_rays])


def degenerate_normals(attrs, material, rng):
    """normals written over covered pixels: (kind, pixels) -- the first five kinds leave the pixel covered, the others do not"""
    kinds = [("+z", (0, 0, 1)), ("-z", (0, 0, -1)), ("m2 = -0.0", (0.6, 0.8, -0.0)), ("not unit", None),
             ("zero", (0, 0, 0)), ("zero, -0.0", (0, 0, -0.0)), ("underflow", (1e-30, -1e-30, 1e-30)), ("overflow", (3e19, 3e19, -3e19)), ("nan", (np.nan, 0, 1)), ("inf", (0, np.inf, 0))]
    flat = attrs.reshape(-1, 18)
    covered = np.nonzero((material.reshape(-1) != R.NO_PRIM) & np.isfinite(flat[:, 11:14]).all(1))[0]
    chosen = rng.choice(covered, 12 * len(kinds), replace=False).reshape(len(kinds), 12)
    for (name, n), px in zip(kinds, chosen):
        if n is None:
            flat[px, 8:11] *= rng.uniform(0.3, 3.0, (len(px), 1)).astype(F)
        else:
            flat[px, 8:11] = np.array(n, F)
    return {name: px for (name, _), px in zip(kinds, chosen)}


def injected_case(pkg, n_tris):
    """-> Case(data, attrs, material, master, radius, kinds, rays = {(P, radius): (hit (pixels, 64) bool, covered (pixels,), rays (pixels, 64))})"""
    def make():
        data = S.scene_data(pkg, n_tris)
        width, height = S.SUN_SIZE
        rng = np.random.default_rng(77000 + n_tris)
        attrs, material = R.soup_gbuffer(rng, data.tris, height, width)
        kinds = degenerate_normals(attrs, material, rng)
        spec = INJECTED[n_tris]
        master = A.cone_directions(64, 4, spec["half"], spec["down"], seed=n_tris)
        bvh = R.build_bvh(data.tris, data.prims)
        walked = {}
        for P in PATTERNS:
            for radius in (spec["radius"], np.inf):
                walked[(P, radius)] = A.image_ray_hits(data.tris, attrs, material, table(master, 64, P), 64, P, radius, BIAS, bvh=bvh)
        return S.Case(data=data, attrs=attrs, material=material, master=master, radius=spec["radius"], kinds=kinds, rays=walked, bvh=bvh)
    return S.once(("ao injected", n_tris), make)


def injected_want(c, n_rays, P, radius, rows=None):
    """-> (hits, covered, result), each (rows, width), of the case (n_rays, P, radius); rows: the frame's rows a shard owns"""
    width, height = S.SUN_SIZE
    hit, covered, _ = c.rays[(P, radius)]
    hits = hit[:, :n_rays].sum(1).astype(np.uint8).reshape(height, width)
    covered = covered.reshape(height, width)
    out = A.result(hits, n_rays, covered)
    rows = np.arange(height) if rows is None else rows
    return hits[rows], covered[rows], out[rows]


def check_injected_conditions(c):
    width, height = S.SUN_SIZE
    seen = {}
    for P in PATTERNS:
        _, covered, _ = injected_want(c, 64, P, np.inf)
        cov = covered.reshape(-1)
        assert (~cov).mean() >= 0.05                                                         # pixels that are not covered ...
        for name in ("zero", "zero, -0.0", "underflow", "overflow", "nan", "inf"):              # ... the degenerate normals among them
            assert not cov[c.kinds[name]].any(), name
        for name in ("+z", "-z", "m2 = -0.0", "not unit"):
            assert cov[c.kinds[name]].all(), name
        for n in N_RAYS:
            per_radius = []
            for radius in (c.radius, np.inf):
                hits, _, out = injected_want(c, n, P, radius)
                h = hits.reshape(-1)[cov]
                per_radius.append(out)
                if n >= 4:
                    none, every, between = (h == 0).mean(), (h == n).mean(), ((h > 0) & (h < n)).mean()
                    assert none >= 0.05 and every >= 0.05 and between >= 0.10, (P, n, radius, none, every, between)
                    seen[(P, n, radius)] = (round(float(none), 3), round(float(every), 3), round(float(between), 3))
                assert (out[~covered] == 255).all()
            if n >= 4:
                assert (per_radius[0] != per_radius[1]).reshape(-1)[cov].mean() >= 0.05, (P, n)   # the radius matters
        _, _, ry = c.rays[(P, np.inf)]
        walks = sum(A.tile_walks(ry[:, :5], cov, height, width), [])
        assert "plain" in walks and "none" in walks, P
    return seen


def odd_case(pkg):
    """the table of ODD_LOCAL (4 rays, pattern 2: the four sets are the list with the signs of x and y varied, so ray 1 is general in every set) over the 1000-triangle scene's injected G-buffer"""
    def make():
        c = injected_case(pkg, 1000)
        width, height = S.SUN_SIZE
        dirs = np.stack([ODD_LOCAL * np.array(sign, F) for sign in ((1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 1))])
        hit, covered, ry = A.image_ray_hits(c.data.tris, c.attrs, c.material, dirs, 4, 2, np.inf, BIAS, bvh=c.bvh)
        hits = hit.sum(1).astype(np.uint8).reshape(height, width)
        return S.Case(dirs=dirs, hits=hits, covered=covered.reshape(height, width), rays=ry, want=A.result(hits, 4, covered.reshape(height, width)))
    return S.once(("ao odd",), make)


def check_odd_conditions(o):
    width, height = S.SUN_SIZE
    walks = sum(A.tile_walks(o.rays, o.covered.reshape(-1), height, width), [])
    assert walks.count("odd") >= 35 and walks.count("plain") >= 1 and "none" in walks         # whole tiles on the odd walk, and one on the plain walk
    valid = R.ray_valid(o.rays.reshape(-1)) & np.repeat(o.covered.reshape(-1), 4)
    d = o.rays.reshape(-1)["direction"][valid]
    assert (d == 0).any() and ((d != 0) & (np.abs(d) < 1e-38)).any()                          # zero components and subnormal ones
    h = o.hits[o.covered]
    assert (h == 0).mean() >= 0.05 and (h > 0).mean() >= 0.3
    return {k: walks.count(k) for k in ("plain", "odd", "none")}


# ---- the rasterised scene -------------------------------------------------------------------------------------------------------------------------
def raster_scene(pkg):
    """-> Case(desc, moved, meshes): a floor with a wall behind it, three boxes on the floor, a tilted quad leaning over one of them, and a scatter of
    boxes about a pixel in size above the floor (the pixels that accept nobody but themselves); moved: the same with one box elsewhere"""
    def make():
        sc = pkg.scenes
        width, height = S.SUN_SIZE
        meshes = [sc.quad((-3, 0, 3), (6, 0, 0), (0, 0, -6), 4, 4), sc.box(1.2, 1.0, 1.2, 2), sc.box(0.8, 1.6, 0.8, 2), sc.box(2.0, 0.5, 0.7, 2),
                  sc.quad((-0.9, 0.0, 0.3), (1.8, 0, 0), (0, 1.5, -0.9), 2, 2), sc.box(0.13, 0.13, 0.13, 1), sc.quad((-3, 0, -3), (3.5, 0, 0), (0, 5, 0), 2, 2)]
        places = [(np.eye(4), 0), (sc.translation(-1.2, 0.5, 0.6), 1), (sc.translation(0.7, 0.8, -0.8) @ sc.rotation_y(30), 2),
                  (sc.translation(1.0, 0.25, 1.4) @ sc.rotation_y(-20), 3), (sc.translation(-0.2, 0.0, 1.9), 4), (np.eye(4), 6)]
        rng = np.random.default_rng(31)
        for _ in range(40):
            x, y, z = rng.uniform(-2.5, 2.5), rng.uniform(0.3, 1.2), rng.uniform(-2.5, 2.5)
            places.append((sc.translation(x, y, z) @ sc.rotation_y(rng.uniform(0, 90)), 5))
        camera = dict(eye=(-3.2, 2.9, 4.2), rotation=(-27.0, -52.0), aspect=width / height, fov_y=45.0, z_near_far=(0.1, 100.0))
        desc = sc.SceneDesc(camera=camera, ambient=0.1, sun=sc.DEFAULT_SUN, objects=pkg.scene.make_objects(places))
        places[1] = (sc.translation(-1.5, 0.5, 0.1), 1)
        moved = sc.SceneDesc(camera=camera, ambient=0.1, sun=sc.DEFAULT_SUN, objects=pkg.scene.make_objects(places))
        return S.Case(desc=desc, moved=moved, meshes=meshes)
    return S.once(("ao raster scene",), make)


def raster_upload(pkg, r):
    c = raster_scene(pkg)
    r.create_material(*pkg.scenes.fallback_textures())
    for v, i in c.meshes:
        r.create_mesh(v, i, 0)
    return r


def raster_tris(pkg, desc):
    c = raster_scene(pkg)
    return R.world_triangles(desc.objects, c.meshes)


def raster_want(pkg, desc, attrs, material):
    """the reference for the rasterised scene from a G-buffer read back: {P: Case(dirs, hits, covered, unfiltered, filtered, accepted, cut)}, with
    ao_directions' cosine hemisphere, FILTER's radius and thresholds"""
    tris, prims = raster_tris(pkg, desc)
    bvh = R.build_bvh(tris, prims)
    out = {}
    for P in (2, 4):
        dirs = pkg.renderer.ao_directions(FILTER["n_rays"], P, seed=3)
        hits, covered = A.image_hits(tris, attrs, material, dirs, FILTER["n_rays"], P, FILTER["radius"], BIAS, bvh=bvh)
        res, accepted, cut = A.filtered(hits, covered, attrs, FILTER["n_rays"], P, FILTER["normal_cos"], FILTER["plane_dist"])
        out[P] = S.Case(dirs=dirs, hits=hits, covered=covered, unfiltered=A.result(hits, FILTER["n_rays"], covered), filtered=res, accepted=accepted, cut=cut)
    return out


def check_raster_conditions(want):
    seen = {}
    for P, w in want.items():
        cov = w.covered
        acc = w.accepted[cov]
        whole, some, alone = (acc == P * P).mean(), ((acc > 1) & (acc < P * P)).mean(), (acc == 1).mean()
        assert whole >= 0.10 and some >= 0.10 and alone >= 0.01, (P, whole, some, alone)
        assert (~cov).mean() >= 0.05
        for border in range(4) if P == 4 else (0, 2):                                         # (the window of P = 2 is -1..0: it reaches over the left and the top only)
            assert (w.cut[..., border] & cov).any(), (P, border)                              # a covered pixel's window is cut by each border
        h = w.hits[cov]
        assert (h == 0).mean() >= 0.05 and (h > 0).mean() >= 0.05
        assert (w.filtered != w.unfiltered).mean() >= 0.05
        seen[P] = (round(float(whole), 3), round(float(some), 3), round(float(alone), 3))
    return seen
