"""The scenes of the device's ray tests (tests/test_gpu_ray_query.py, tests/test_gpu_ray_paths.py): the soup of tests/ray_reference.py as one to
three meshes with transforms of their own, on a 64 x 64 handle -- and the inputs of tests/test_gpu_ray_paths.py with their expected results, each
made once: tests/test_ray_paths_inputs.py checks on the CPU that they are what the device tests take them for."""
import numpy as np

import ray_reference as R

F = np.float32
CAMERA = dict(eye=(0, 0, 9), rotation=(0, -90), aspect=1.0, fov_y=60.0, z_near_far=(0.1, 50.0))
N_OBJECTS = {1: 1, 4: 2, 5: 3, 1000: 3}


def transforms():
    """three object transforms: one of exactly representable entries (a quarter turn about y, scales 2 / 1 / 0.5, a translation in quarters: the
    soup's shared edges, grid and axis-aligned planes stay exactly shared, on the grid and axis-aligned in world space), two general ones"""
    a = np.array([[0, 0, 0.5, 1.5], [0, 1, 0, -0.25], [-2, 0, 0, 2], [0, 0, 0, 1]], np.float64)
    c, s = np.cos(0.7), np.sin(0.7)
    b = np.array([[c, -s, 0, -1.3], [s, c, 0, 0.4], [0, 0, 1, 0.9], [0, 0, 0, 1]]) @ np.diag([1.1, 0.8, 1.3, 1.0])
    c, s = np.cos(-1.9), np.sin(-1.9)
    d = np.array([[1, 0, 0, 0.2], [0, c, -s, -0.6], [0, s, c, 1.7], [0, 0, 0, 1]]) @ np.diag([0.6, 1.7, 0.9, 1.0])
    return [m.astype(F) for m in (a, b, d)]


def soup_meshes(pkg, rng, n_tris, n_objects):
    """the soup's triangles as n_objects meshes (three vertices per triangle; vertices of grid triangles repeat the same coordinates, so shared
    edges stay shared); the second mesh, where there is one, carries a triangle with an index out of range in its middle"""
    tris = R.soup_triangles(rng, n_tris).reshape(-1, 3, 3)
    cuts = np.linspace(0, n_tris, n_objects + 1).astype(int)
    meshes = []
    for k in range(n_objects):
        part = tris[cuts[k]:cuts[k + 1]]
        v = np.zeros(3 * len(part), pkg.scene.VERTEX_DTYPE)
        v["position"] = part.reshape(-1, 3)
        v["normal"], v["tangent"], v["bitangent"] = (0, 1, 0), (1, 0, 0), (0, 0, 1)
        ind = np.arange(3 * len(part), dtype=np.uint32)
        if k == 1 and len(part) >= 2:
            mid = 3 * (len(part) // 2)
            ind = np.concatenate([ind[:mid], np.array([0, 1, 3 * len(part)], np.uint32), ind[mid:]])   # skipped, but it takes a prim number
        meshes.append((v, ind))
    return meshes


def triangle_mesh(pkg, tris):
    """(n, 9) triangles as one mesh of three vertices each"""
    part = np.asarray(tris, F).reshape(-1, 3)
    v = np.zeros(len(part), pkg.scene.VERTEX_DTYPE)
    v["position"] = part
    v["normal"], v["tangent"], v["bitangent"] = (0, 1, 0), (1, 0, 0), (0, 0, 1)
    return v, np.arange(len(part), dtype=np.uint32)


class SceneData:
    """the scene of n_tris soup triangles without a handle: meshes, the scene description, the world-space triangles and their prim numbers.
    triangles: instead of the soup, these (n, 9) triangles as one object in place"""
    def __init__(self, pkg, n_tris, seed=7000, sun=None, triangles=None):
        if triangles is None:
            n_objects = N_OBJECTS[n_tris]
            self.meshes = soup_meshes(pkg, np.random.default_rng(seed + n_tris), n_tris, n_objects)
            places = transforms()[:n_objects]
        else:
            self.meshes, places = [triangle_mesh(pkg, triangles)], [np.eye(4, dtype=F)]
        self.desc = pkg.scenes.SceneDesc(camera=CAMERA, ambient=0.1, sun=pkg.scenes.DEFAULT_SUN if sun is None else sun,
                                         objects=pkg.scene.make_objects([(m, k) for k, m in enumerate(places)]))
        self.tris, self.prims = R.world_triangles(self.desc.objects, self.meshes)
        self.n_prims = sum(len(i) // 3 for _, i in self.meshes)

    def handle(self, pkg, hip, width=64, height=64, **kw):
        r = hip.Renderer(width, height, 64, 16, **kw)
        r.create_material(*pkg.scenes.fallback_textures())
        for v, i in self.meshes:
            r.create_mesh(v, i, 0)
        return r


class Scene(SceneData):
    def __init__(self, pkg, hip, n_tris):
        SceneData.__init__(self, pkg, n_tris)
        self.r = self.handle(pkg, hip)
        self.rays, self.want = {}, {}

    def case(self, n_rays):
        if n_rays not in self.rays:
            self.rays[n_rays] = R.soup_rays(np.random.default_rng(9000 + n_rays), self.tris, n_rays)
            self.want[n_rays] = {a: R.brute(self.tris, self.rays[n_rays], any_hit=a, prims=self.prims) for a in (False, True)}
        return self.rays[n_rays], self.want[n_rays]


# ---- the inputs of tests/test_gpu_ray_paths.py: made once per session, never changed ---------------------------------------------------------
TRI_COUNTS = [1, 4, 5, 1000]
LAYOUTS = [1, 2]
SUN_SIZE = (52, 37)                                                  # 7 x 5 tiles: the width is no multiple of 8, the tile count none of 4
SUN_BIAS = 1e-3
SUNS = {"default": None,                                             # three general components: every tile takes the plain walk
        "axis": (0.0, 0.0),                                          # sun_dir = (1, 0, 0): two zero components, every tile takes the odd walk
        "grazing": (-90.0, 37.0)}                                    # no zero component, two of about 3e-8: the plain walk with reciprocals near 3e7
SHARDS = {"rows 5..30": [dict(row_begin=5, row_end=30)],
          "bands of 8, 3 shards": [dict(band_rows=8, shard=(k, 3)) for k in range(3)],
          "bands of 16, 2 shards": [dict(band_rows=16, shard=(k, 2)) for k in range(2)]}
_made = {}


def once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def scene_data(pkg, n_tris):
    return once(("scene", n_tris), lambda: SceneData(pkg, n_tris))


class Case:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def arbiter(data, rays):
    return {a: R.brute(data.tris, rays, any_hit=a, prims=data.prims) for a in (False, True)}


def wave_case(pkg, n_tris, layout):
    """-> Case(data, rays, waves, want = {any_hit: hits}): R.wave_rays, from the pool of seed 424242 + n_tris that both layouts share, against the
    scene of n_tris triangles"""
    def make():
        data = scene_data(pkg, n_tris)
        pool = once(("pool", n_tris), lambda: R.wave_pool(np.random.default_rng(424242 + n_tris), data.tris, data.prims))
        rays, waves = R.wave_rays(None, data.tris, layout, pool=pool)
        return Case(data=data, rays=rays, waves=waves, want=arbiter(data, rays))
    return once(("waves", n_tris, layout), make)


def subnormal_case(pkg, which, triangle=None):
    """-> Case(data, sets = {"plain" / "odd": Case(rays, pattern, want)}): R.subnormal_rays against the 1000-triangle scene (which = 1000) or
    against the one triangle given (which = "tri")"""
    def make():
        data = scene_data(pkg, 1000) if which == 1000 else SceneData(pkg, 1, triangles=triangle)
        sets = {}
        for name, (rays, pattern) in zip(("plain", "odd"), R.subnormal_rays(data.tris)):
            sets[name] = Case(rays=rays, pattern=pattern, want=arbiter(data, rays))
        return Case(data=data, sets=sets)
    return once(("subnormal", which), make)


def dead_case(pkg):
    """-> Case(data, here, away, first, want, plain): layout 1 against the 1000-triangle scene after object 0 (prims [0, first)) has left the
    finite numbers, as tests/test_gpu_ray_refit.py's test_dead_and_back sends it away.  here / away: two scene descriptions, with the object
    in place and gone, neither ever changed; data: the scene whose tris are the triangles with the object gone (its meshes and prims are the
    scene's); plain: the indices of the rays in waves of the plain walk"""
    def make():
        import copy
        c = wave_case(pkg, 1000, 1)
        data = SceneData(pkg, 1000)
        here, away = data.desc, copy.copy(data.desc)
        away.objects = here.objects.copy()
        away.objects["trs"][0, 12] = np.inf
        data.desc = None                                             # (use here / away)
        data.tris, prims = R.world_triangles(away.objects, data.meshes)
        assert (prims == c.data.prims).all() and R.world_triangles(here.objects, data.meshes)[0].tobytes() == c.data.tris.tobytes()
        plain = np.concatenate([np.arange(w["start"], w["stop"]) for w in c.waves if w["walk"] == "plain"])
        return Case(data=data, here=here, away=away, first=len(data.meshes[0][1]) // 3, want=arbiter(data, c.rays), plain=plain)
    return once(("dead",), make)


def check_dead_conditions(c, d):
    """c: wave_case(pkg, 1000, 1); d: dead_case(pkg)"""
    assert not np.isfinite(d.data.tris[:d.first]).all(1).any() and np.isfinite(d.data.tris[d.first:]).all()
    assert (c.want[False]["prim"][d.plain] < d.first).sum() >= 32                        # rays of the plain waves hit the object that goes ...
    assert not (d.want[False]["prim"] < d.first).any()                                   # ... nothing hits it once it is gone ...
    assert (d.want[False]["prim"][d.plain] != R.NO_PRIM).sum() >= 64                     # ... and the plain waves still hit the others


def owned(pkg, height, shard):
    """the rows of the frame that a handle created with these arguments holds, in its order"""
    if "band_rows" in shard:
        from importlib import import_module
        return import_module(pkg.__name__ + ".sharding").owned_rows(height, shard["shard"][0], shard["shard"][1], shard["band_rows"])
    return np.arange(shard["row_begin"], shard["row_end"])


def shard_walks(pkg, c, sun, shard):
    """the walks of the 8 x 8 tiles of one shard of the sun's frame (c: sun_case): a row range keeps its place inside its first tile row,
    interleaved bands are packed from the top"""
    width, height = SUN_SIZE
    rows = owned(pkg, height, shard)
    rays, active = c.suns[sun].rays.reshape(height, width)[rows], c.covered.reshape(height, width)[rows]
    return R.tile_walks(rays.reshape(-1), active.reshape(-1), len(rows), width, shard.get("row_begin", 0) % 8)


def sun_case(pkg):
    """-> Case(data, attrs, material, covered, suns = {name: Case(desc, rays, mask, flawed)}): the injected G-buffer of SUN_SIZE for the
    1000-triangle scene; mask: what arctic_trace_sun_visibility has to return for the whole frame; flawed: the mask under the arbiter's defect
    nan_prunes"""
    def make():
        data = scene_data(pkg, 1000)
        width, height = SUN_SIZE
        attrs, material = R.soup_gbuffer(np.random.default_rng(52037), data.tris, height, width)
        covered = material.reshape(-1) != R.NO_PRIM
        bvh = R.build_bvh(data.tris, data.prims)
        suns = {}
        for name, rotation in SUNS.items():
            sun = pkg.scenes.DEFAULT_SUN if rotation is None else dict(pkg.scenes.DEFAULT_SUN, rotation=rotation)
            desc = SceneData(pkg, 1000, sun=sun).desc
            rays = R.sun_rays(attrs, pkg.renderer.frame_constants(desc)[2], SUN_BIAS)
            masks = []
            for defect in (None, "nan_prunes"):
                hits, _ = R.walk(bvh, rays[covered], any_hit=True, defect=defect)
                m = np.full(height * width, 255, np.uint8)
                m[covered] = np.where(hits["prim"] == 0, 0, 255)
                masks.append(m.reshape(height, width))
            suns[name] = Case(desc=desc, rays=rays, mask=masks[0], flawed=masks[1])
        return Case(data=data, attrs=attrs, material=material, covered=covered, suns=suns)
    return once(("sun",), make)


# ---- what these inputs have to be for the device tests to mean something: asserted by the CPU test and by the device tests alike ------------------
MISS_RECORD = np.array([(0.0, 0.0, 0.0, R.NO_PRIM)], R.HIT_DTYPE).tobytes()


def check_wave_conditions(c, n_tris):
    want = c.want[False]
    hit = want["prim"] != R.NO_PRIM
    kinds = [k if isinstance(k, str) else "edge" for w in c.waves for k in w["lanes"]]
    for w in c.waves:
        n_hit, lanes = int(hit[w["start"]:w["stop"]].sum()), w["lanes"]
        if len(lanes) == 64 and w["walk"] == "plain":
            assert n_hit >= 16, w                                                       # every full plain wave
        if len(lanes) == 64 and w["walk"] == "odd":
            # every full wave of the odd walk; one that is a plain wave but for a lane (plain rays under the odd node test) as a plain wave
            assert n_hit >= (16 if lanes.count("plain") >= 63 else 8), w
        if len(lanes) < 64 and w["walk"] != "none":
            assert 4 * n_hit >= len(lanes), w                                           # a partial wave, of either walk: the full plain wave's quarter
        if w["walk"] == "none":
            assert want[w["start"]:w["stop"]].tobytes() == MISS_RECORD * 64             # the all-invalid wave
        for lane, k in w["edges"].items():                                              # every edge lane is the exact miss record, but the one that admits every t
            one = want[w["start"] + lane:w["start"] + lane + 1]
            assert (one.tobytes() == MISS_RECORD) == (k != 13), (w, lane)
            for a in (True, False):
                assert (c.want[a][w["start"] + lane]["prim"] == R.NO_PRIM) == (k != 13)
    plain = np.array([k == "plain" for k in kinds])
    _, tie = R.tied(c.data.tris, c.rays[plain])
    # closest hits shared by two triangles, among the rays of the plain walk.  The 1- and the 5-triangle scene have none to offer: no two of the
    # five triangles share a vertex, an edge or a plane, so no ray at all has a tied closest hit there (== 0: a change of scene shows up here)
    if n_tris in (1, 5):
        assert tie.sum() == 0, n_tris
    else:
        assert tie.sum() >= 1, n_tris
    return {"plain": [w["walk"] for w in c.waves].count("plain"), "odd": [w["walk"] for w in c.waves].count("odd"),
            "none": [w["walk"] for w in c.waves].count("none"), "hits": int(hit.sum()), "ties": int(tie.sum())}


def check_subnormal_conditions(s, patterns):
    hit = s.want[False]["prim"] != R.NO_PRIM
    assert sorted(set(s.pattern[s.pattern >= 0].tolist())) == sorted(patterns)
    for bits in patterns:                                                               # every bit pattern hits, and misses
        m = s.pattern == bits
        assert hit[m].any() and not hit[m].all(), hex(bits)


def check_sun_conditions(c):
    out = {}
    width, height = SUN_SIZE
    for name, s in c.suns.items():
        occluded = (s.mask.reshape(-1)[c.covered] == 0).mean()
        assert 0.05 <= occluded <= 0.95, (name, occluded)
        walks = R.tile_walks(s.rays, c.covered, height, width)
        valid = R.ray_valid(s.rays) & c.covered
        if name == "axis":                                                              # every ray is odd: every tile that walks takes the odd walk
            assert R.ray_odd(s.rays)[valid].all() and "plain" not in walks and walks.count("odd") >= 30
            assert (s.rays["direction"][0] == 0).sum() == 2
            assert (s.mask != s.flawed).sum() >= 8                                      # ... and a walk that does not look for the NaN gives another mask
        else:                                                                           # no ray is odd
            assert not R.ray_odd(s.rays)[valid].any() and "odd" not in walks and walks.count("plain") >= 30
            assert (s.mask == s.flawed).all()
        if name == "grazing":
            d = np.abs(s.rays["direction"][0])
            assert (d > 0).all() and ((d > 1e-8) & (d < 1e-7)).sum() == 2
        assert walks.count("none") >= 1                                                 # the tile without geometry
        out[name] = {k: walks.count(k) for k in ("plain", "odd", "none")}
        out[name]["occluded %"] = round(100 * float(occluded), 1)
    return out
