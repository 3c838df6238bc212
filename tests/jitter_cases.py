"""What tests/test_oracle_jitter.py (CPU) and tests/test_gpu_jittered_prepass.py (GPU) share: the camera jitters, the scenes of every case with
the jitters each one takes, the matrix a jittered prepass draws with, and the oracle's side of every comparison.  No device, no test in here.

The matrix is tests/taa_reference.py's float32 restatement of arctic_jitter_proj_view (tests/test_taa_reference.py holds the two equal by bits)
applied to the ORACLE's camera matrix, with the FRAME's width and height -- also for a shard.  The oracle draws with it through
Oracle.set_proj_view; no expected value comes from a HIP handle.

A case is not vacuous when (conditions()): the jittered oracle frame has at least `floor` covered pixels, and its triangle-id or depth plane
differs from the unjittered oracle frame's in at least 1 % of them -- except under TINY, whose matrix differs from the camera's in a few bits:
there only the matrices' bytes must differ.  floor is 300, but for the 17 x 9 frame, which has 153 pixels in all: there it is a quarter of the
frame (38), which still leaves every side of the frame crossed by a triangle's edge.
"""
import copy

import numpy as np

import cluster_cull_cases as CC
import taa_reference as T

NO = 0xFFFFFFFF
EXISTING = (0.4, -0.3)                                     # tests/test_gpu_taa.py's
HALTON_1, HALTON_2, HALTON_5 = (T.taa_jitter(k) for k in (1, 2, 5))
CORNER_A, CORNER_B = (1.0, -1.0), (-1.0, 1.0)               # the corners of the accepted range; each is the other's opposite
AXIS_X, AXIS_Y = (0.25, 0.0), (0.0, -0.25)                  # the host's condition is jx != 0 || jy != 0
TINY = (2.0 ** -12, 2.0 ** -12)                             # the matrix differs from the camera's in a few bits only
JITTERS = (EXISTING, HALTON_1, HALTON_2, HALTON_5, CORNER_A, CORNER_B, AXIS_X, AXIS_Y, TINY)
FLOOR, DIFFER = 300, 0.01


def jid(j):
    return "j(%+.4g,%+.4g)" % tuple(j)


def is_zero(j):
    return j is None or (float(j[0]) == 0.0 and float(j[1]) == 0.0)


def proj_view(O, desc, width, height, j):
    """the [col][row] float32 matrix of the forward prepass under jitter j: the oracle's camera matrix, and for a j that is not (0, 0) numpy's
    arctic_jitter_proj_view of it.  width, height: the FRAME's"""
    m = O.frame_constants(desc)[0]
    return m if is_zero(j) else T.jitter_proj_view(m, width, height, float(j[0]), float(j[1]))


def oracle_prepass(O, sc, j=None, desc=None, shadow=True, **kw):
    """an oracle with sc uploaded that has drawn desc's prepass (and the shadow map) under jitter j; kw: row_begin, row_end"""
    desc = desc or sc.desc
    o = sc.upload(O.Oracle(sc.width, sc.height, sc.shadow_size, sc.max_lights, **kw))
    if not is_zero(j):
        o.set_proj_view(proj_view(O, desc, sc.width, sc.height, j))
    if shadow:
        o.pass_shadow_map(desc)
    o.pass_gbuffer(desc)
    return o


def planes(x):
    """[attributes, material, depth, triangle id] of an oracle's or a HIP handle's G-buffer, the floats as their bits"""
    attrs, mat, depth, tri = x.read_gbuffer()
    return [attrs.view(np.uint32).copy(), mat.copy(), depth.view(np.uint32).copy(), tri.copy()]


def same_planes(want, got, what=""):
    for name, a, b in zip(("attributes", "material", "depth", "triangle id"), want, got):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name, a.shape, b.shape)
        n = int((a != b).sum())
        assert n == 0, f"{what}: {name}: {n} of {a.size} elements differ"


def distance_to_sample(O, desc, attrs, material, width, height, j, row_begin=0):
    """per covered pixel: how far the float64 projection of the G-buffer's world position through the UNJITTERED matrix lies from p + 0.5 - j, in
    pixels (tests/test_gpu_taa.py's measure, on the oracle's matrix)"""
    M = O.frame_constants(desc)[0].astype(np.float64)                             # [col][row]
    covered = material != NO
    w = np.concatenate([attrs.view(np.float32)[..., 11:14].astype(np.float64), np.ones(attrs.shape[:2] + (1,))], -1)
    clip = w @ M
    sx, sy = (clip[..., 0] / clip[..., 3] + 1.0) * (0.5 * width), (1.0 - clip[..., 1] / clip[..., 3]) * (0.5 * height)
    ys, xs = np.mgrid[0:attrs.shape[0], 0:attrs.shape[1]]
    d = np.hypot(sx - (xs + 0.5 - j[0]), sy - (ys + row_begin + 0.5 - j[1]))
    return d[covered]


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """one scene of one group of the GPU file with the jitters it takes.  both_args: tests/test_gpu_edge_cases.py both()'s arguments from the
    width on, for the groups that go through it; options: arctic_set_option pairs of the device's handle"""

    def __init__(self, group, name, sc, jitters, desc=None, floor=FLOOR, options=None, both_args=None):
        self.group, self.name, self.sc, self.jitters = group, name, sc, tuple(jitters)
        self.desc = desc or sc.desc
        self.floor, self.options, self.both_args = floor, dict(options or {}), both_args
        self._zero = None

    @property
    def id(self):
        return f"{self.group}-{self.name}"

    def unjittered(self, O):
        if self._zero is None:
            o = oracle_prepass(O, self.sc, None, self.desc, shadow=False)
            self._zero = planes(o)
            o.close()
        return self._zero

    def conditions(self, O, j, jittered=None):
        """(covered pixels, the fraction of them whose triangle id or depth differs from the unjittered frame's, whether the matrices' bytes
        differ, ok) from the oracle alone"""
        if jittered is None:
            o = oracle_prepass(O, self.sc, j, self.desc, shadow=False)
            jittered = planes(o)
            o.close()
        zero = self.unjittered(O)
        covered = jittered[1] != NO
        n = int(covered.sum())
        differ = float(((jittered[3] != zero[3]) | (jittered[2] != zero[2]))[covered].mean()) if n else 0.0
        a, b = (proj_view(O, self.desc, self.sc.width, self.sc.height, x) for x in (None, j))
        bits = a.tobytes() != b.tobytes()
        ok = n >= self.floor and bits and (tuple(j) == TINY or differ >= DIFFER)
        return n, differ, bits, ok


def _scene_of(pkg, name, both_args, desc=None, settings=(0, 2.2, 1.0)):
    """both()'s arguments as a SyntheticScene, so that the oracle alone can draw them"""
    import test_gpu_edge_cases as E
    w, h, shadow, mats, meshes, objs, lights = both_args
    desc = desc or E.camera_scene(pkg, pkg.scene.make_objects(objs), w, h, lights)
    return pkg.scenes.SyntheticScene(name, w, h, shadow, 16, mats, meshes, desc, lights, settings)


# a. oracle parity: four scenes of tests/test_gpu_parity.py's SCENES, three jitters each; every jitter of the list is taken at least once
PARITY = (((1, 0.5, {}), (EXISTING, HALTON_1, TINY)),
          ((2, 0.25, {}), (HALTON_2, CORNER_A, AXIS_X)),
          ((3, 0.1, {}), (HALTON_5, CORNER_B, AXIS_Y)),
          ((3, 0.15, {"raster_owner": 1, "tiles_per_wave": 2}), (EXISTING, CORNER_A, HALTON_2)))


def parity_cases(pkg):
    import test_gpu_parity as P
    out = []
    for (cfg, scale, options), jitters in PARITY:
        assert (cfg, scale, options) in P.SCENES
        name = f"config{cfg}-x{scale}" + ("-large-frame-defaults" if options else "")
        out.append(Case("a", name, pkg.scenes.CONFIGS[cfg](scale=scale), jitters, options=options))
    return out


# b. ragged and non-square frames: one triangle across each side of the frame, its inner corner near the middle, at depths of their own
PINWHEEL = [(0.3, 0.2, 0.0), (5.0, -1.5, -1.0), (5.0, 1.8, 0.5),            # across the right side
            (-0.2, 0.3, 0.2), (2.0, 3.5, -0.5), (-2.5, 3.5, 0.6),           # the top
            (-0.3, -0.2, 0.1), (-5.5, 1.6, 0.4), (-5.5, -1.9, -0.8),        # the left side
            (0.1, -0.3, 0.0), (-2.2, -3.4, 0.5), (2.6, -3.4, -0.7)]         # the bottom
RAGGED_SIZES = ((100, 70), (17, 9))
RAGGED_JITTERS = (CORNER_A, CORNER_B, AXIS_X, AXIS_Y)


def ragged_cases(pkg):
    import test_gpu_edge_cases as E
    out = []
    for w, h in RAGGED_SIZES:
        rng = np.random.default_rng(8)
        mats = [pkg.scenes.make_material_textures(rng, 32)]
        lights = pkg.scenes.random_lights(rng, 3, (-2, -2, 0.5), (2, 2, 3))
        args = (w, h, 96, mats, [(E.tri_mesh(pkg, PINWHEEL), list(range(12)), 0)], [(np.eye(4), 0)], lights)
        out.append(Case("b", f"{w}x{h}", _scene_of(pkg, f"pinwheel-{w}x{h}", args), RAGGED_JITTERS, floor=min(FLOOR, w * h // 4), both_args=args))
    return out


# c. shards, d. culling, g. state: config 3 x 0.25
SHARD_JITTERS = (EXISTING, CORNER_B)
SHARDS = (dict(row_begin=0, row_end=48), dict(row_begin=96, row_end=160), dict(row_begin=263, row_end=264), dict(row_begin=13, row_end=77),
          dict(band_rows=16, shard=(1, 3)))
STATE_JITTERS = (EXISTING, HALTON_2)                                       # j0, j1 of the sequence j0, j1, (0, 0), j0


def hall(pkg):
    return pkg.scenes.config3(scale=0.25)


def shard_cases(pkg):
    return [Case("c", "config3-x0.25", hall(pkg), SHARD_JITTERS)]


def state_cases(pkg):
    return [Case("g", "config3-x0.25", hall(pkg), STATE_JITTERS)]


# d. one camera of each of the four kinds of tests/test_gpu_cluster_cull.py's cameras() -- inside the hall, far outside looking at it, nose on
# the floor, straight down -- and the far plane that cuts the hall; (index into cameras(default_rng(20251), 32), far plane, jitter).  The first
# 16 of these are test_random_cameras' own; none of its four cameras far outside sees the hall (they look past it), the first that does is the 30th
CULL_CAMERAS = ((0, False, EXISTING), (29, False, HALTON_1), (2, False, CORNER_A), (7, False, AXIS_X), (4, True, CORNER_B))


def cull_cases(pkg):
    import test_gpu_cluster_cull as CL
    sc = hall(pkg)
    cams = CL.cameras(np.random.default_rng(20251), 32)
    out = []
    for k, far, j in CULL_CAMERAS:
        desc = copy.deepcopy(sc.desc)
        desc.camera["eye"], desc.camera["rotation"] = cams[k]
        if far:
            desc.camera["z_near_far"] = (0.5, 12.0)
        out.append(Case("d", f"camera{k}-kind{k % 4}" + ("-far-plane" if far else ""), sc, (j,), desc=desc))
    return out


# e. clipping and the wide-coordinate path
CLIP_JITTERS = (EXISTING, CORNER_B)
NEAR_SIZE = 128                                                             # (tests/test_oracle_raster.py draws it at 64 x 64: under 300 covered pixels)
CLIPPED_TRIANGLES = 1200                                                    # 3 records each < 2 n + 4096: the record table's first size holds them


def clip_cases(pkg, O):
    import test_gpu_edge_cases as E
    import test_oracle_raster as R
    out = []
    pts = [(-1, -1, 0.0), (1, -1, 0.0), (0, -1, 10.0)]                      # test_near_plane_clipping's floor triangle, under and behind the eye
    desc = R.ortho_scene(pkg, pkg.scene.make_objects([(np.eye(4), 0)]))
    args = (NEAR_SIZE, NEAR_SIZE, 0, [R.flat_material(pkg)], [(R.tri_mesh(pkg, pts), [0, 2, 1], 0)], [(np.eye(4), 0)], np.zeros(0, pkg.scene.LIGHT_DTYPE))
    out.append(Case("e", "near-plane-triangle", _scene_of(pkg, "near-plane", args, desc), CLIP_JITTERS, both_args=args))
    v, idx, mats, desc, n_recs, _ = E.clipped_scene(pkg, O, CLIPPED_TRIANGLES)
    assert 2 * CLIPPED_TRIANGLES < n_recs <= 2 * CLIPPED_TRIANGLES + 4096, n_recs      # heavily clipped, and the table is not overflowed
    args = (160, 96, 0, mats, [(v, idx, 0)], [(np.eye(4, dtype=np.float32), 0)], np.zeros(0, pkg.scene.LIGHT_DTYPE))
    out.append(Case("e", "clipped-into-three", _scene_of(pkg, "clipped", args, desc), CLIP_JITTERS, both_args=args))
    args = E.guard_band_scene(pkg)
    out.append(Case("e", "guard-band-3840x64", _scene_of(pkg, "guard-band", args), CLIP_JITTERS, both_args=args))
    return out


# f. level of detail: the two known-answer quads of tests/test_gpu_texture_mips.py (texels per pixel, lambda) and config 3 x 0.1
LOD_JITTERS = (EXISTING, CORNER_B)
LOD_QUADS = ((4.0, 2.0), (0.5, 0.0))
LOD_W, LOD_H = 192, 128


def lod_cases(pkg, O):
    import test_gpu_texture_mips as M
    out = [Case("f", f"quad-ratio-{ratio}", M._quad_scene(pkg, O, LOD_W, LOD_H, 256, ratio), LOD_JITTERS) for ratio, _ in LOD_QUADS]
    out.append(Case("f", "config3-x0.1", pkg.scenes.config3(scale=0.1), LOD_JITTERS))
    return out


def all_cases(pkg, O):
    return parity_cases(pkg) + ragged_cases(pkg) + shard_cases(pkg) + cull_cases(pkg) + clip_cases(pkg, O) + lod_cases(pkg, O) + state_cases(pkg)


# ---- d. the sweep across the scissor's sides --------------------------------------------------------------------------------------------------------
SWEEP_JITTERS = (CORNER_A, CORNER_B)
SWEEP_STEPS = None          # {side: steps} where the eleven steps of the existing sweep hold no offset that tells j from -j for a side; none needed


def sweep_scene(pkg, off=(0.0, 0.0, 0.0)):
    """tests/test_gpu_cluster_cull.py's small dense quad, translated by off, as a scene of its 256 x 144 frame"""
    import test_gpu_cluster_cull as CL
    S = pkg.scenes
    mats = [S.make_material_textures(np.random.default_rng(7), 64)]
    desc = S.SceneDesc(camera=CL.SWEEP_CAMERA, ambient=0.1, sun=S.DEFAULT_SUN, objects=S.make_objects([(S.translation(*off), 0)]))
    return S.SyntheticScene("sweep", CL.SWEEP_W, CL.SWEEP_H, 0, 16, mats, [CC.small_quad(S) + (0,)], desc, np.zeros(0, S.LIGHT_DTYPE), (0, 2.2, 1.0))


_sweeps = {}


def oracle_sweep(pkg, O, j):
    """[(side, d, desc, the oracle's planes, its set-up triangles)] of the sweep under jitter j"""
    import test_gpu_cluster_cull as CL
    if tuple(j) not in _sweeps:
        sc = sweep_scene(pkg)
        o = sc.upload(O.Oracle(sc.width, sc.height, 0, 16))
        out = []
        for side, d, off in CL.sweep_offsets(SWEEP_STEPS):
            desc = sweep_scene(pkg, off).desc
            if not is_zero(j):
                o.set_proj_view(proj_view(O, desc, sc.width, sc.height, j))
            o.pass_gbuffer(desc)
            out.append((side, d, desc, planes(o), int(o.stats()[0])))
        o.close()
        _sweeps[tuple(j)] = out
    return _sweeps[tuple(j)]


def sweep_tells_the_matrices_apart(pkg, O):
    """{side: [(j, d), ...]}: the offsets at which the quad covers a pixel under corner jitter j and none under -j, the other corner -- where
    the jitter decides whether the quad is drawn.  A corner jitter moves the picture towards two of the four sides, so each side has such
    offsets under one of the two corners; every side must have one"""
    found = {}
    for j, minus in ((CORNER_A, CORNER_B), (CORNER_B, CORNER_A)):
        for (side, d, _, a, _), (_, _, _, b, _) in zip(oracle_sweep(pkg, O, j), oracle_sweep(pkg, O, minus)):
            if side != "depth" and (a[1] != NO).any() and not (b[1] != NO).any():
                found.setdefault(side, []).append((jid(j), d))
    return found


def sweep_expected_skips(pkg, O, j):
    """[(clusters box_outside skips under the DRAWN matrix, under the camera's, whether the count is safe to compare)] per offset of the sweep,
    from cluster_cull_cases' float64 replay of geometry.hip's box_outside on the quad's five cluster boxes.  Safe: the replay gives the same
    count with half and with twice the kernel's rounding margin E, so no corner is near enough to a plane for fp32 to decide otherwise.
    The image cannot tell the two matrices apart: box_outside moves the scissor's sides out by one pixel and |j| <= 1, so a box beyond a
    side under the camera's matrix is beyond the last pixel centre under the drawn one too -- a test against the camera's matrix skips
    nothing that is drawn, it only skips other clusters.  The counts of arctic_read_cull_counts do tell"""
    import test_gpu_cluster_cull as CL
    tb = CC.cluster_boxes(*CC.small_quad(pkg.scenes))
    size = (CL.SWEEP_W, CL.SWEEP_H, (0, 0, CL.SWEEP_W, CL.SWEEP_H))
    out = []
    for _, _, desc, _, _ in oracle_sweep(pkg, O, j):
        trs = desc.objects[0]["trs"]
        drawn, camera = (proj_view(O, desc, CL.SWEEP_W, CL.SWEEP_H, x).ravel() for x in (j, None))
        n = [int(CC.box_outside(tb, trs, drawn, *size, strict).sum()) for strict in (0.5, 1.0, 2.0)]
        n0 = [int(CC.box_outside(tb, trs, camera, *size, strict).sum()) for strict in (0.5, 1.0, 2.0)]
        out.append((n[1], n0[1], len(set(n)) == 1 and len(set(n0)) == 1))
    return out
