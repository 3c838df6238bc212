"""The extended shading kernels (k_envlit, k_spotlit, k_cubelit, k_miplit and their _vis forms) against ONE independent float64 pixel:
tests/shading_reference.py, written from include/arctic_hip.h and pinned on the CPU by tests/test_shading_reference.py.

Every injected case writes its inputs (G-buffer, sun map, cube faces, level-of-detail plane), runs arctic_pass_shade with float outputs and
compares the judged pixels' float LDR with the reference at TOL = 1e-4 (the project's standing bar) and HDR relatively at
1e-4 against |want| + 1e-3 (the bar of test_injected_faces_against_float64).  No expected value comes from a HIP handle: what is read back
are inputs (G-buffer, maps, faces, chains, lambda, environment tables).

Measured on the first full run (profiles/extended_shading_parity.json, 152 figures): float LDR at most 4.9e-6, relative HDR at most 4.6e-5
(the half-shadowed all-features case), the binary16 cases 2.6e-7 at the 99.9 % quantile and 2.2e-4 at most; the mask leaves out at most 0.8 % of
a case's covered pixels.  The gates stay where they are.

The builders of the cases (CASES, build_inputs, reference_for) need no device: tests/test_shading_reference.py imports them and shows on
the CPU that each case's inputs tell a list of deliberate defects from the truth, and how many pixels the mask leaves out.
"""
import json
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest

import env_reference as ER
import mip_reference as MR
import shading_reference as SR

pytestmark = pytest.mark.gpu
TOL = 1e-4          # float LDR: the project's standing bar (README, every parity test)
HDR_REL = 1e-4      # |hdr - want| / (|want| + 1e-3): test_injected_faces_against_float64's bar
HDR16_MAX = 1e-3    # binary16 colour target: 99.9 % of the pixels within TOL, all within 1e-3 (test_reference_quantised_mode's bar)
W, H, S, F = 96, 64, 64, 32
NO_MAT = 0xFFFFFFFF
FEATURES = ("env", "spot", "cube", "mip")
ALL = frozenset(FEATURES)
SUBSETS = [frozenset(f for i, f in enumerate(FEATURES) if k >> i & 1) for k in range(16)]
ENV_SIZE = (64, 32)
BOX_LO, BOX_HI = (-15, 0, -7), (15, 12, 7)   # the world box of scenes.random_gbuffer


def _tag(fs):
    return "+".join(f for f in FEATURES if f in fs) or "none"


class Case:
    def __init__(self, name, features, light_path=0, n_points=5, culling=1, width=W, rows=H, row_begin=0, frame_rows=None, sampler=0, hdr16=0,
                 half_shadow=False, full_lists=False, tm=2, seed=0):
        self.name, self.features, self.light_path, self.n_points, self.culling = name, frozenset(features), light_path, n_points, culling
        self.width, self.rows, self.row_begin, self.frame_rows = width, rows, row_begin, frame_rows or rows
        self.sampler, self.hdr16, self.half_shadow, self.full_lists, self.tm, self.seed = sampler, hdr16, half_shadow, full_lists, tm, seed

    def __repr__(self):
        return self.name


def _lattice():
    """all 16 subsets of {ENV, SPOT, CUBE, MIP}, each with the scalar and the packed light loop: with 5 point lights in front, every branch
    of launch_variant's G-buffer half is taken by construction (8 kernel shapes x 2 loops)"""
    return [Case(f"lattice-{_tag(fs)}-path{lp}", fs, light_path=lp, n_points=5, seed=k) for k, fs in enumerate(SUBSETS) for lp in (1, 2)]


def _edges():
    out = []
    for k, fs in enumerate([ALL] + [frozenset([f]) for f in FEATURES]):
        t, s = _tag(fs), 100 + 20 * k
        out += [Case(f"edge-{t}-points{n}", fs, n_points=n, tm=n % 3, seed=s + i) for i, n in enumerate((0, 1, 5, 13))]   # 13: automatic switch to the packed loop, odd tail
        out += [Case(f"edge-{t}-culling0", fs, culling=0, light_path=2, seed=s + 4),
                Case(f"edge-{t}-100x70", fs, width=100, rows=70, tm=0, seed=s + 5),                           # ragged right and bottom tiles
                Case(f"edge-{t}-rows13to77", fs, row_begin=13, frame_rows=96, tm=1, seed=s + 6),              # a shard cut inside a tile row
                Case(f"edge-{t}-sampler1", fs, sampler=1, seed=s + 7),
                Case(f"edge-{t}-hdr16", fs, hdr16=1, seed=s + 8),
                Case(f"edge-{t}-half-shadowed", fs, half_shadow=True, n_points=13, seed=s + 9)]
        if fs & {"spot", "cube"}:
            out.append(Case(f"edge-{t}-lists-at-max-lights", fs, full_lists=True, n_points=16, light_path=0, seed=s + 10))
    return out


LATTICE, EDGES = _lattice(), _edges()
CASES = LATTICE + EDGES


# ---- inputs (no device) ------------------------------------------------------------------------------------------------------------
def _random_images(rng, w, h):
    out = []
    for _ in range(3):
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        a[..., 3] = 255
        out.append(a)
    return tuple(out)


def _well_conditioned(images):
    """Normal maps with b in [200, 251] and r, g in [96, 159], roughness bytes in [13, 255] (the ranges of scenes.make_material_textures).
    A normal map whose three channels all straddle 128 filters to a nearly null vector at the coarse levels of its chain, and normalising a
    vector of length L multiplies the fp32 rounding of the filtered bytes by 1 / L: with per-channel noise around 128, pixels at L = 1e-3 ... 5e-3
    were off by 1.2e-4 ... 1.9e-4 of their HDR value on the device, one pixel per frame, at any lambda.  Here L >= 0.56."""
    d, n, m = (x.copy() for x in images)
    n[..., :2] = 96 + n[..., :2] // 4
    n[..., 2] = 200 + n[..., 2] // 5
    m[..., 1] = 13 + (m[..., 1].astype(np.uint32) * 242 // 255).astype(np.uint8)
    return d, n, m


def _materials(pkg, rng):
    """0: 64 x 64 with a rough normal map, every texel its own direction (a chain of 7 levels); 1: 32 x 16 noise (6 levels); 2: images of unequal
    sizes (never a chain: the plain path); 3: 1 x 1 (a chain of one level)"""
    d, n, m = pkg.scenes.make_material_textures(rng, 64)
    n[..., :3] = rng.integers(0, 256, n[..., :3].shape)
    d2, _, _ = _random_images(rng, 16, 16)
    _, n2, _ = _random_images(rng, 8, 8)
    _, _, m2 = _random_images(rng, 4, 4)
    one = (np.array([[[200, 120, 60, 255]]], np.uint8), np.array([[[120, 140, 250, 255]]], np.uint8), np.array([[[255, 90, 255, 255]]], np.uint8))
    return [_well_conditioned((d, n, m)), _well_conditioned(_random_images(rng, 32, 16)), _well_conditioned((d2, n2, m2)), one]


GRAZING = 4e-3


def _steer_clear_of_grazing_views(rng, case, I):
    """Redraw the world position of the few pixels (0.4 %) whose |n.wo| is below GRAZING, n being the normal the case's own material sampling gives.
    calculate_outgoing_radiance divides by 4 (n.wo)(n.wi) + 1e-4: for 0 < n.wo < 1e-4 the specular term is proportional to n.wo itself, and the
    fp32 n.wo of two unit vectors carries about 4 ulps = 2.4e-7 of absolute error, i.e. parts in a thousand of such a value -- of the base model
    (k_material) as much as of the extended kernels: the frame of seed 7146 had one pixel with n.wo = 4.2e-5 that the device shaded 1.3e-3 of its HDR value
    (2.1e-4 in LDR) away from float64, every feature off.  At |n.wo| >= 4e-3 the same rounding moves the term by less than 1e-5 of itself; a
    negative n.wo is kept away from zero as well, for fp32 may round it to a tiny positive one."""
    materials = host_materials(I.images, "mip" in case.features)
    ch = SR.material_channels(materials, I.attrs, I.mat, lod=I.lod if "mip" in case.features else None, q8=bool(case.sampler & 1))
    n = SR.surface_normal(I.attrs, ch)
    lo, hi = np.asarray(BOX_LO, np.float32), np.asarray(BOX_HI, np.float32)
    for _ in range(100):
        wo = SR.f32(I.eye) - I.attrs[..., 11:14].astype(np.float64)
        wo /= np.linalg.norm(wo, axis=-1, keepdims=True)
        bad = (I.mat != NO_MAT) & (np.abs((n * wo).sum(-1)) < GRAZING)
        if not bad.any():
            return
        I.attrs[bad, 11:14] = lo + rng.random((int(bad.sum()), 3), dtype=np.float32) * (hi - lo)
    raise AssertionError("grazing views left")


def _spots(pkg, rng, n):
    a = np.zeros(n, pkg.scene.SPOT_LIGHT_DTYPE)
    pos = rng.uniform((-14, 1, -6), (14, 11, 6), (n, 3))
    target = rng.uniform(BOX_LO, BOX_HI, (n, 3))
    outer = rng.uniform(0.3, 1.2, n)
    inner = outer * rng.uniform(0, 0.9, n)
    inner[0] = outer[0]                                                       # a hard cone (scale 1000)
    a["position"], a["direction"], a["color"] = pos, target - pos, rng.uniform(20, 80, (n, 3))
    a["outer_cone_angle"], a["inner_cone_angle"] = outer, inner
    a["range"] = np.where(np.arange(n) % 2 == 0, rng.uniform(4, 12, n), 0.0)   # ranges that cut through the scene, and none
    if n > 1:                                                                 # omnidirectional with a range: no cone at all
        a[1]["outer_cone_angle"], a[1]["range"] = np.float32(np.pi), 9.0
    return a


def _cubes(pkg, rng, n):
    """light 0: faces of per-texel noise (most pixels in a penumbra: the PCF weights matter); light 2: a near plane beyond some pixels and a
    far plane in front of others, depths over the whole [0, 1]; the others: blocks of 4 x 4 texels around the pixels' pz"""
    a = np.zeros(n, pkg.scene.POINT_SHADOW_LIGHT_DTYPE)
    a["position"], a["color"] = rng.uniform((-8, 3, -3), (8, 9, 3), (n, 3)), rng.uniform(20, 60, (n, 3))
    a["z_near"], a["z_far"] = 0.1, 40.0
    faces = []
    for i in range(n):
        if i == 0:
            f = rng.uniform(0.975, 1.0, (6, F, F))
        elif i == 2:
            a[i]["z_near"], a[i]["z_far"] = 6.0, 14.0
            f = np.repeat(np.repeat(rng.uniform(0.0, 1.0, (6, F // 2, F // 2)), 2, 1), 2, 2)
        else:
            f = np.repeat(np.repeat(rng.uniform(0.975, 1.0, (6, F // 4, F // 4)), 4, 1), 4, 2)
        faces.append(np.ascontiguousarray(f, np.float32))
    return a, faces


def build_inputs(pkg, case):
    """everything a case injects, from its seed alone"""
    rng = np.random.default_rng(7000 + case.seed)
    I = SimpleNamespace()
    I.images = _materials(pkg, rng)
    rows, width = case.rows, case.width
    attrs, mat = pkg.scenes.random_gbuffer(rng, rows, width, len(I.images), coverage=0.9)   # every tile mixes the four materials ...
    mat[:, :24] = np.where(mat[:, :24] != NO_MAT, 0, NO_MAT)                                 # ... but three tile columns of material 0 alone
    mat[:8, 24:40] = 1                                                                       # ... and two tiles wholly covered by material 1
    shadow = rng.random((S, S), dtype=np.float32) * 0.6 + 0.3
    if case.half_shadow:   # the left half of the frame wholly in the sun's shadow (all 25 taps): only the ambient / environment term is left there
        half = width // 2
        attrs[:, :half, 14:18] = np.float32([-0.5, 0.0, 0.9, 1.0])
        attrs[:, :half, 15] = np.linspace(-0.9, 0.9, rows, dtype=np.float32)[:, None]
        shadow[:, :S // 2 + 2] = 0.0
    lod = rng.uniform(-1.0, 8.0, (rows, width)).astype(np.float32)       # fractions, negatives and values beyond every chain ...
    lod[:, ::7] = np.round(lod[:, ::7])                                   # ... exact integers ...
    lod[5::11, :] = 6.0                                                   # ... the last level of the longest chain ...
    lod[: rows // 2, :24] = 2.0 + 0.9 * np.linspace(0, 1, 24, dtype=np.float32)[None, :]   # ... tiles whose lanes agree on floor(lambda) ...
    lod[3, 5] = np.nan                                                    # ... and a NaN (counts as 0)
    I.attrs, I.mat, I.shadow, I.lod = attrs, mat, shadow, lod
    I.points = pkg.scenes.random_lights(rng, case.n_points, (-14, 1, -6), (14, 11, 6), intensity=30.0)
    I.spots = _spots(pkg, rng, 16 if case.full_lists else 6)
    I.cubes, I.faces = _cubes(pkg, rng, 16 if case.full_lists else 3)
    I.env_map = pkg.scenes.synthetic_hdri(*ENV_SIZE)
    I.eye, I.sun, I.ambient = (0.0, 5.0, 0.0), dict(pkg.scenes.DEFAULT_SUN), 0.3
    I.settings = (case.tm, 2.2, 1.0)
    _steer_clear_of_grazing_views(rng, case, I)
    I.desc = pkg.scene.SceneDesc(camera=dict(eye=I.eye, rotation=(-15.0, 0.0), aspect=width / case.frame_rows, fov_y=45.0, z_near_far=(0.1, 1000.0)),
                                 ambient=I.ambient, sun=I.sun, objects=pkg.scene.make_objects([]))
    return I


def sun_lit(oracle, shadow, attrs, mat):
    """1 - shadow per covered pixel from the oracle's calculate_shadow on the given map (1 where nothing is covered)"""
    lit = np.ones(mat.shape)
    ls = np.ascontiguousarray(attrs[..., 14:18], np.float32)
    smap = None if shadow is None else np.ascontiguousarray(shadow, np.float32)
    for y, x in zip(*np.nonzero(mat != NO_MAT)):
        lit[y, x] = 1.0 - oracle.calculate_shadow(smap, ls[y, x])
    return lit


def host_materials(images, mips):
    """what the handle holds, built on the host (tests/mip_reference.py reproduces the device's chains bit for bit)"""
    out = []
    for d, n, m in images:
        if d.shape == n.shape == m.shape:
            out.append(MR.chain(MR.pack(d, n, m)) if mips else [MR.pack(d, n, m)])
        else:
            out.append((d, n, m))
    return out


_host_env = {}


def host_env_tables(env_map):
    """the tables of ARCTIC_OPT_ENV_LIGHTING from tests/env_reference.py (the device's own are within 1e-4 of these: test_gpu_env_lighting.py)"""
    key = env_map.shape
    if key not in _host_env:
        Hh, Ww = env_map.shape[:2]
        levels = [env_map.astype(np.float64)] + [ER.prefilter_level(env_map, k) for k in range(1, ER.LEVELS)]
        _host_env[key] = (ER.sh_project(env_map), ER.brdf_lut(), levels)
    return _host_env[key]


def reference_for(case, I, lit, materials, env_tables, on=None, attrs=None, mutate=()):
    on = case.features if on is None else on
    attrs = I.attrs if attrs is None else attrs
    ch = SR.material_channels(materials, attrs, I.mat, lod=I.lod if "mip" in on else None, q8=bool(case.sampler & 1), mutate=mutate)
    return SR.shade(attrs, I.mat, ch, lit, I.eye, I.sun["rotation"], I.sun["color"], I.ambient, I.settings, points=I.points,
                    spots=I.spots if "spot" in on else (), cubes=I.cubes if "cube" in on else (), faces=I.faces if "cube" in on else (),
                    env=env_tables if "env" in on else None, hdr16=bool(case.hdr16), mutate=mutate)


def mutations_for(features, n_points):
    """the deliberate defects (shading_reference.MUTATIONS) a case with these features and this many point lights must notice"""
    have = set(features) | ({"point"} if n_points % 2 else set())
    return [m for m, f in SR.MUTATIONS.items() if f in have]


def sensitivity(features, n_points, truth, mutated):
    """{defect: share of the truth's judged pixels whose LDR it moves by more than 10 x TOL}; mutated(m) evaluates the reference with defect m"""
    j = truth["judged"]
    return {m: float((np.abs(mutated((m,))["ldr"] - truth["ldr"]).max(-1)[j] > 10 * TOL).mean()) for m in mutations_for(features, n_points)}


# ---- the record ----------------------------------------------------------------------------------------------------------------------
_record = {}


@pytest.fixture(scope="module", autouse=True)
def _parity_record():
    t0 = time.time()
    yield
    out = os.environ.get("ARCTIC_EXTENDED_PARITY_JSON")
    if out and _record:
        import __graft_entry__ as entry
        json.dump({"source": entry.source_id(), "gate_ldr": TOL, "gate_hdr_rel": HDR_REL, "gate_hdr16_max": HDR16_MAX, "wall_s": round(time.time() - t0, 1),
                   "cases": _record}, open(out, "w"), indent=1)


def judge(name, ref, ldr, hdr, hdr16=False):
    """print and record the case's largest errors over the judged pixels, then assert the bars"""
    j = ref["judged"]
    assert j.sum() > 0
    err = np.abs(ldr.astype(np.float64) - ref["ldr"])[j]
    rel = (np.abs(hdr.astype(np.float64) - ref["hdr"]) / (np.abs(ref["hdr"]) + 1e-3))[j]
    rec = {"judged": int(j.sum()), "left_out": int(ref["covered"].sum() - j.sum())}
    if hdr16:   # the binary16 rounding is a discontinuity: a pixel on a rounding boundary moves by half an ulp of binary16
        rec.update(ldr_q999_binary16=float(np.quantile(err, 0.999)), ldr_max_binary16=float(err.max()))
    else:
        rec.update(ldr=float(err.max()), hdr_rel=float(rel.max()))
    _record[name] = rec
    print(f"{name}: " + ", ".join(f"{k} = {v:.3e}" if isinstance(v, float) else f"{k} = {v}" for k, v in rec.items()))
    for what, e in (("ldr", np.abs(ldr.astype(np.float64) - ref["ldr"])), ("hdr relative", np.abs(hdr.astype(np.float64) - ref["hdr"]) / (np.abs(ref["hdr"]) + 1e-3))):
        y, x, c = np.unravel_index(np.argmax(np.where(j[..., None], e, -1.0)), e.shape)
        if e[y, x, c] > 0.5 * TOL:   # the worst pixel of a case that comes near a bar, for whoever has to explain it
            print(f"  worst {what} at ({y}, {x}) channel {c}: roughness {ref['rough'][y, x]:.4f}, metalness {ref['metal'][y, x]:.3f}, 1 - shadow {ref['lit'][y, x]:.3f}, "
                  f"hdr want {ref['hdr'][y, x]} got {hdr[y, x]}, ldr want {ref['ldr'][y, x]} got {ldr[y, x]}")
    if hdr16:
        assert rec["ldr_q999_binary16"] <= TOL and rec["ldr_max_binary16"] <= HDR16_MAX, (name, rec)
    else:
        assert rec["ldr"] <= TOL, (name, rec)
        assert rec["hdr_rel"] <= HDR_REL, (name, rec)
    return rec


# ---- the device side -----------------------------------------------------------------------------------------------------------------
def _configure(r, I, on):
    """switch the features of `on` on and every other one off"""
    r.set_option("env_lighting", int("env" in on))
    r.update_spot_lights(I.spots if "spot" in on else I.spots[:0])
    r.update_point_shadow_lights(I.cubes if "cube" in on else I.cubes[:0])
    if "cube" in on and I.faces is not None:
        for i, f in enumerate(I.faces):
            r.write_point_shadow(i, f)
    r.set_option("texture_mips", int("mip" in on))
    if "mip" in on and I.lod is not None:
        r.write_lod(I.lod)


def _device_materials(r, images, first=0, chains=True):
    """what the handle holds: the chains read back; a material of unequal image sizes has none to read (the images as uploaded)"""
    out = []
    for i, (d, n, m) in enumerate(images, first):
        if d.shape == n.shape == m.shape:
            lv = [r.read_material_mip(i, 0)]
            for k in range(1, len(MR.level_sizes(lv[0].shape[1], lv[0].shape[0])) if chains else 1):   # (created under mode 0: one level)
                lv.append(r.read_material_mip(i, k))
            out.append(lv)
        else:
            out.append((d, n, m))
    return out


def _injected_handle(hip, case, I):
    kw = dict(row_begin=case.row_begin, row_end=case.row_begin + case.rows) if case.frame_rows != case.rows else {}
    r = hip.Renderer(case.width, case.frame_rows, S, 16, **kw)
    r.set_option("texture_mips", int("mip" in case.features))     # chains are built when a material is created
    for d, n, m in I.images:
        r.create_material(d, n, m)
    r.create_hdri(I.env_map)                                     # uncovered pixels take the skybox in every case
    r.update_lights(I.points)
    r.write_gbuffer(I.attrs, I.mat)
    r.write_shadow_map(I.shadow)
    for opt, v in (("keep_float_output", 1), ("point_shadow_size", F), ("sampler", case.sampler), ("hdr16", case.hdr16), ("culling", case.culling),
                   ("light_path", case.light_path)):
        r.set_option(opt, v)
    return r


def _shade(r, I):
    r.pass_shade(I.desc, I.settings)
    return [x.copy() for x in r.read_output()]


def _run_injected(pkg, oracle, hip, case):
    I = build_inputs(pkg, case)
    r = _injected_handle(hip, case, I)
    _configure(r, I, case.features)
    ldr, hdr, rgba = _shade(r, I)
    attrs = r.read_gbuffer(want=("attrs",))[0]                   # the G-buffer the kernels read (an input, read back)
    cov = I.mat != NO_MAT
    np.testing.assert_array_equal(attrs[cov], I.attrs[cov])
    if "mip" in case.features:
        got, want = r.read_lod()[cov], I.lod[cov]
        np.testing.assert_array_equal(got[~np.isnan(want)], want[~np.isnan(want)])
    env_tables = r.read_env_lighting() if "env" in case.features else None
    materials = _device_materials(r, I.images, chains="mip" in case.features)
    if "mip" in case.features:
        assert [len(m) for m in materials if not isinstance(m, tuple)] == [7, 6, 1]
    lit = sun_lit(oracle, I.shadow, attrs, I.mat)
    if case.half_shadow:
        assert (lit[:, : case.width // 2][cov[:, : case.width // 2]] == 0).all()
    ref = reference_for(case, I, lit, materials, env_tables, attrs=attrs)
    # it did not silently fall back: each feature switched off alone changes the judged pixels; all off = the control, and pixels without
    # geometry are the control's bits
    for f in sorted(case.features):
        _configure(r, I, case.features - {f})
        off = _shade(r, I)
        assert np.abs(off[1] - hdr)[ref["judged"]].max() > 1e-3, (case.name, f)
    _configure(r, I, frozenset())
    control = _shade(r, I)
    for got, base in zip((ldr, hdr, rgba), control):
        np.testing.assert_array_equal(got[~cov], base[~cov])
    r.close()
    judge(case.name, ref, ldr, hdr, hdr16=bool(case.hdr16))


@pytest.mark.parametrize("case", LATTICE, ids=repr)
def test_feature_lattice(pkg, oracle, hip, case):
    _run_injected(pkg, oracle, hip, case)


@pytest.mark.parametrize("case", EDGES, ids=repr)
def test_edges(pkg, oracle, hip, case):
    _run_injected(pkg, oracle, hip, case)


# ---- the visibility path: real geometry, real shadow edges, the device's own lambda ------------------------------------------------------
def _frame_scene(pkg, cfg, scale, env_size=ENV_SIZE):
    sc = pkg.scenes.CONFIGS[cfg](scale=scale)
    sc.environment = pkg.scenes.synthetic_hdri(*env_size)
    if cfg == 2:   # the lights among config 2's objects (a few metres around the origin)
        box = dict(lo=(-3.0, 0.5, -3.0), hi=(3.0, 4.0, 3.0))
        spots, cubes = pkg.scenes.spot_lights(4, seed=31, **box), pkg.scenes.point_shadow_lights(2, seed=32, z_far=20.0, **box)
    else:
        spots, cubes = pkg.scenes.spot_lights(4, seed=33), pkg.scenes.point_shadow_lights(2, seed=34)
    return sc, spots, cubes


def _frame_inputs(sc, spots, cubes):
    """the scene's side of the reference's inputs: the lists and constants the caller hands to the library"""
    I = SimpleNamespace(spots=spots, cubes=cubes, faces=None, lod=None, points=sc.lights, eye=sc.desc.camera["eye"], sun=sc.desc.sun,
                        ambient=sc.desc.ambient, settings=sc.settings, images=sc.materials)
    return I


def _frame_reference_inputs(r, I):
    """what the handle holds after a frame with every feature on, read back"""
    attrs, mat, _, _ = r.read_gbuffer(want=("attrs", "material"))
    lod = r.read_lod()
    faces = [r.read_point_shadow(i) for i in range(len(I.cubes))]
    smap = r.read_shadow_map() if r.shadow_size else None
    return attrs, mat, lod, faces, smap


class _FrameRef:
    """the reference of one frame under any feature set: the light sums and the environment bracket evaluated once per material sampling
    (mips on / off)"""

    def __init__(self, I, attrs, mat, lod, faces, lit, materials, env_tables):
        self.I, self.attrs, self.mat, self.lod, self.faces, self.lit, self.materials, self.env_tables = I, attrs, mat, lod, faces, lit, materials, env_tables
        self.memo, self.ch = {False: {}, True: {}}, {}

    def __call__(self, on, mutate=()):
        mip, I = "mip" in on, self.I
        if mutate:
            ch, memo = SR.material_channels(self.materials, self.attrs, self.mat, lod=self.lod if mip else None, mutate=mutate), None
        else:
            if mip not in self.ch:
                self.ch[mip] = SR.material_channels(self.materials, self.attrs, self.mat, lod=self.lod if mip else None)
            ch, memo = self.ch[mip], self.memo[mip]
        return SR.shade(self.attrs, self.mat, ch, self.lit, I.eye, I.sun["rotation"], I.sun["color"], I.ambient, I.settings, points=I.points,
                        spots=I.spots if "spot" in on else (), cubes=I.cubes if "cube" in on else (), faces=self.faces if "cube" in on else (),
                        env=self.env_tables if "env" in on else None, mutate=mutate, memo=memo)

    def report_sensitivity(self, name, step):
        """what the deliberate defects of shading_reference.MUTATIONS would move in this frame (every step-th pixel each way): reported, not
        asserted -- the device drew these inputs"""
        sub = (slice(None, None, step), slice(None, None, step))
        few = _FrameRef(self.I, self.attrs[sub], self.mat[sub], self.lod[sub], self.faces, self.lit[sub], self.materials, self.env_tables)
        shares = sensitivity(ALL, len(self.I.points), few(ALL), lambda m: few(ALL, mutate=m))
        print(f"{name}: share of the judged pixels a defect moves by more than {10 * TOL:g}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
        return shares


@pytest.mark.parametrize("cfg,scale", [(2, 0.25), (3, 0.1)])
def test_visibility_path(pkg, oracle, hip, cfg, scale):
    """render_frame through k_*_vis = pass_gbuffer + pass_shade bit for bit, and the latter against the reference built from what the handle
    itself holds, for the 16 feature sets and both light loops"""
    sc, spots, cubes = _frame_scene(pkg, cfg, scale)
    r = hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights)
    r.set_option("texture_mips", 1)
    sc.upload(r)
    r.set_option("keep_float_output", 1)
    r.set_option("point_shadow_size", 64)
    I = _frame_inputs(sc, spots, cubes)
    _configure(r, I, ALL)
    r.render_frame(sc.desc, sc.settings)       # draws the sun's map, the cube faces, and (read below) the G-buffer with its lambda plane
    attrs, mat, lod, faces, smap = _frame_reference_inputs(r, I)
    assert lod.max() > 0.5 and all((f < 1).any() for f in faces)
    materials = _device_materials(r, sc.materials)
    ref_of = _FrameRef(I, attrs, mat, lod, faces, sun_lit(oracle, smap, attrs, mat), materials, r.read_env_lighting())
    cov = mat != NO_MAT
    shares = {}
    for fs in SUBSETS:
        r.set_option("env_lighting", int("env" in fs))
        r.update_spot_lights(spots if "spot" in fs else spots[:0])
        r.update_point_shadow_lights(cubes if "cube" in fs else cubes[:0])
        r.set_option("texture_mips", int("mip" in fs))
        ref = ref_of(fs)
        shares[_tag(fs)] = 1 - ref["judged"].sum() / cov.sum()
        for lp in (1, 2):
            r.set_option("light_path", lp)
            r.set_option("visbuffer", 1)
            img = r.render_frame(sc.desc, sc.settings)
            vis = [x.copy() for x in r.read_output()]
            np.testing.assert_array_equal(img, vis[2])
            if "cube" in fs:   # the faces the frame drew are the ones the reference read
                np.testing.assert_array_equal(r.read_point_shadow(0), faces[0])
            r.pass_gbuffer(sc.desc)
            r.pass_shade(sc.desc, sc.settings)
            gb = r.read_output()
            for a, b in zip(vis, gb):
                np.testing.assert_array_equal(a, b)
            if "mip" in fs:
                np.testing.assert_array_equal(r.read_lod(), lod)
            judge(f"visibility-config{cfg}-{_tag(fs)}-path{lp}", ref, gb[0], gb[1])
    ref_of.report_sensitivity(f"visibility-config{cfg}", 4)
    print(f"config {cfg}: share of covered pixels left out per feature set:", {k: round(float(v), 5) for k, v in shares.items()})
    assert max(shares.values()) <= 0.10
    r.close()


def test_config3_4k_all_features_stripes(pkg, oracle, hip):
    """config 3 at its real size with every feature on; the reference on three stripes of rows (ceiling / far wall, the middle of the atrium, the
    sunlit floor), as the whole-frame oracle tests bound their host time"""
    sc, spots, cubes = _frame_scene(pkg, 3, 1.0, env_size=(512, 256))
    assert (sc.width, sc.height) == (3840, 2160)
    r = hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights)
    r.set_option("texture_mips", 1)
    sc.upload(r)
    r.set_option("keep_float_output", 1)
    r.set_option("point_shadow_size", 256)
    I = _frame_inputs(sc, spots, cubes)
    _configure(r, I, ALL)
    img = r.render_frame(sc.desc, sc.settings)
    vis = [x.copy() for x in r.read_output()]
    attrs, mat, lod, faces, smap = _frame_reference_inputs(r, I)
    r.pass_shade(sc.desc, sc.settings)
    gb = r.read_output()
    for a, b in zip(vis, gb):
        np.testing.assert_array_equal(a, b)
    env_tables = r.read_env_lighting()
    chains = {}
    left_out = covered = 0
    for y0 in (300, 1050, 1850):
        sl = slice(y0, y0 + 8)
        a, m, l = attrs[sl], mat[sl], lod[sl]
        for k in (int(k) for k in np.unique(m[m != NO_MAT])):   # the chains of the materials the stripes meet
            if k not in chains:
                chains[k] = _device_materials(r, sc.materials[k:k + 1], first=k)[0]
        materials = chains
        ch = SR.material_channels(materials, a, m, lod=l)
        ref = SR.shade(a, m, ch, sun_lit(oracle, smap, a, m), I.eye, I.sun["rotation"], I.sun["color"], I.ambient, I.settings, points=I.points,
                       spots=spots, cubes=cubes, faces=faces, env=env_tables)
        judge(f"config3-4k-all-rows{y0}", ref, gb[0][sl], gb[1][sl])
        left_out += int(ref["covered"].sum() - ref["judged"].sum()); covered += int(ref["covered"].sum())
    print(f"config 3 at 4K: {left_out} of {covered} covered stripe pixels left out ({left_out / covered:.4%})")
    r.close()
