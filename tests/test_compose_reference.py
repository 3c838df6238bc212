"""The composition on a machine without a GPU: arctic_compose_pixels -- the library's own two terms on the host, the functions k_compose runs --
against the float64 restatement of tests/compose_reference.py at HDR_REL, the project's standing bar (tests/test_gpu_extended_shading.py, taken
over unchanged); that the bar would notice each deliberate defect of compose_reference.MUTATIONS; the exact properties, by bytes; the refusals.

The sample: 6000 pixels with every class the definition names -- refl.a == 0 with NaN colours, normals that are zero, overflow, underflow or are
not finite, ao 0 and 255, views that graze the surface or see it from behind (c clamped to 0), pixels without geometry whose every other input
is a NaN.  hdr = ambient * base + a lit part that is zero for a third of the pixels: the frame's own ambient term is in it, as in a shaded frame,
so the occlusion can take it away entirely (ao = 0, strength 1 on a shadowed pixel) and no more."""
import numpy as np
import pytest

import ao_reference as A
import compose_reference as CR

HDR_REL = 1e-4      # test_gpu_extended_shading.HDR_REL (importing that module would import the device tests' helpers: the value is restated, and asserted equal below)
INVALID = -1
N = 6000
EYE = (0.4, 2.0, 3.0)
AMBIENT = 0.1


@pytest.fixture(scope="module")
def lib(pkg):
    import os
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


def sample(seed=2024):
    rng = np.random.default_rng(seed)
    F = np.float32
    s = {}
    s["base"] = rng.uniform(0, 1, (N, 3)).astype(F)
    s["metal"] = rng.choice([0.0, 1.0, 0.5], N).astype(F) * rng.uniform(0.9, 1.0, N).astype(F)
    s["rough"] = rng.uniform(0, 1, N).astype(F)
    s["world"] = rng.uniform(-3, 3, (N, 3)).astype(F)
    wo = np.asarray(EYE, np.float64) - s["world"]
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    nrm = wo + rng.normal(size=(N, 3)) * rng.choice([0.1, 0.6, 2.0], (N, 1))               # towards the eye, more or less
    t = np.cross(wo, rng.normal(size=(N, 3)))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    graze = np.arange(N) % 10 == 3
    nrm[graze] = t[graze] + wo[graze] * rng.uniform(-2e-3, 2e-3, (graze.sum(), 1))          # grazing: |c| <= 2e-3, either sign
    s["normal"] = (nrm * rng.uniform(0.2, 4.0, (N, 1))).astype(F)                           # (not unit vectors)
    special = [(0, 0, 0), (0, 0, -0.0), (3e19, 3e19, 3e19), (1e-30, 1e-30, 0), (np.nan, 0, 1), (0, -np.inf, 0)]
    degenerate = np.arange(N) % 25 == 7
    s["normal"][degenerate] = np.array([special[k % len(special)] for k in range(degenerate.sum())], F)
    s["ao"] = rng.integers(0, 256, N).astype(np.uint8)
    s["ao"][np.arange(N) % 7 == 0] = 0
    s["ao"][np.arange(N) % 7 == 1] = 255
    refl = np.concatenate([rng.uniform(0, 3, (N, 3)), rng.choice([0.0, 0.5, 1.0], (N, 1))], 1).astype(F)
    refl[refl[:, 3] == 0, :3] = np.nan
    s["refl"] = refl
    s["geometry"] = np.arange(N) % 11 != 5
    lit = rng.uniform(0, 4, (N, 3)) * (rng.uniform(size=(N, 1)) > 0.33)
    s["hdr"] = (F(AMBIENT) * s["base"] + lit.astype(F)).astype(F)
    for k in ("base", "metal", "rough", "world", "normal", "refl"):                          # a pixel without geometry: nothing but hdr is looked at
        s[k][~s["geometry"]] = np.nan
    s["hdr"][~s["geometry"]] = rng.uniform(0, 4, ((~s["geometry"]).sum(), 3)).astype(F)
    s["graze"], s["degenerate"] = graze & s["geometry"], degenerate & s["geometry"]
    return s


@pytest.fixture(scope="module")
def S():
    return sample()


def args(s):
    return (s["hdr"], s["base"], s["metal"], s["rough"], s["normal"], s["world"], s["geometry"], EYE, AMBIENT)


CASES = {"ao": dict(ao=True, refl=False, ao_strength=1.0), "ao at 0.6": dict(ao=True, refl=False, ao_strength=0.6),
         "reflections": dict(ao=False, refl=True, reflection_strength=1.0), "both": dict(ao=True, refl=True, ao_strength=0.8, reflection_strength=1.7)}


def planes(s, case):
    kw = {k: v for k, v in case.items() if k not in ("ao", "refl")}
    return dict(ao=s["ao"] if case["ao"] else None, refl=s["refl"] if case["refl"] else None, **kw)


def standing_bar():
    import re, os
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_extended_shading.py")).read()
    return float(re.search(r"^HDR_REL = (\S+)", text, re.M).group(1))


@pytest.mark.parametrize("case", list(CASES))
def test_the_arbiter_against_float64(pkg, lib, S, case):
    assert HDR_REL == standing_bar()
    kw = planes(S, CASES[case])
    got = pkg.renderer.compose_pixels(*args(S), **kw)
    want = CR.compose(*args(S), **kw)
    assert got.shape == (N, 3) and got.dtype == np.float32 and np.isfinite(want).all() and np.isfinite(got).all()
    rel = CR.rel_err(got, want)
    print(case, "largest relative error", float(rel.max()))
    assert rel.max() <= HDR_REL, (case, float(rel.max()), int(np.argmax(rel.max(1))))
    # not vacuous: the sample holds every class, and the terms are there
    g = S["geometry"]
    _, covered = A.normal(S["normal"])
    assert (~g).sum() >= 300 and (S["degenerate"] & ~covered).sum() >= 100 and S["graze"].sum() >= 300
    assert (S["ao"][g] == 0).sum() >= 300 and (S["ao"][g] == 255).sum() >= 300
    none = g & (S["refl"][:, 3] == 0)
    assert none.sum() >= 1000 and np.isnan(S["refl"][none, :3]).all()
    moved = (got != S["hdr"]).any(1)
    assert moved[g].mean() >= 0.5 and not moved[~g].any()
    if CASES[case]["refl"] and not CASES[case]["ao"]:
        assert not moved[none].any() and not moved[S["degenerate"] & ~covered].any()         # the select: by bytes
        wo = np.asarray(EYE, np.float64) - S["world"].astype(np.float64)
        c = (S["normal"].astype(np.float64) * wo).sum(1)
        assert (S["graze"] & (c < 0)).sum() >= 50 and (S["graze"] & (c > 0)).sum() >= 50     # grazing views from either side of the horizon


@pytest.mark.parametrize("defect", list(CR.MUTATIONS))
def test_the_bar_would_notice(pkg, lib, S, defect):
    """each deliberate defect moves at least 5 % of the pixels its term is present in by more than 10 x the gate -- away from the truth, and
    away from what the arbiter computes: a library with that defect would not have passed"""
    flag = CR.MUTATIONS[defect]
    kw = planes(S, CASES["ao" if flag == CR.AO else "reflections"])
    truth = CR.compose(*args(S), **kw)
    _, covered = A.normal(S["normal"])
    rng = np.random.default_rng(5)
    with np.errstate(invalid="ignore"):
        m = S["normal"].astype(np.float64) / np.linalg.norm(S["normal"].astype(np.float64), axis=1, keepdims=True)
        mapped = m + 0.25 * rng.normal(size=m.shape)                                        # what a normal map does to a vertex normal
        mapped /= np.linalg.norm(mapped, axis=1, keepdims=True)
    mutated = CR.compose(*args(S), mutate=(defect,), mapped_normal=mapped, **kw)
    affected = S["geometry"] if flag == CR.AO else S["geometry"] & covered & (S["refl"][:, 3] > 0)
    if defect == "alpha_ignored":
        affected = affected & (S["refl"][:, 3] != 1)
    share = float((CR.rel_err(mutated, truth).max(1)[affected] > 10 * HDR_REL).mean())
    print(defect, "moves", round(share, 3), "of", int(affected.sum()), "pixels by more than", 10 * HDR_REL)
    assert affected.sum() >= 1000 and share >= 0.05, (defect, share)
    got = pkg.renderer.compose_pixels(*args(S), **kw)
    assert CR.rel_err(got, truth).max() <= HDR_REL and (CR.rel_err(got, mutated).max(1)[affected] > 10 * HDR_REL).mean() >= 0.05, defect


def test_exact_properties_by_bytes(pkg, lib, S):
    hdr = S["hdr"].tobytes()
    # strengths 0 give hdr back
    assert pkg.renderer.compose_pixels(*args(S), ao=S["ao"], refl=S["refl"], ao_strength=0.0, reflection_strength=0.0).tobytes() == hdr
    # ao == 255 everywhere gives hdr back, at any strength
    open_ = np.full(N, 255, np.uint8)
    for k in (1.0, 0.37):
        assert pkg.renderer.compose_pixels(*args(S), ao=open_, ao_strength=k).tobytes() == hdr
    # a pixel without geometry gives hdr back
    nothing = dict(S, geometry=np.zeros(N, bool))
    assert pkg.renderer.compose_pixels(*args(nothing), ao=S["ao"], refl=S["refl"], ao_strength=1.0, reflection_strength=2.0).tobytes() == hdr
    both = pkg.renderer.compose_pixels(*args(S), ao=S["ao"], refl=S["refl"])
    assert both[~S["geometry"]].tobytes() == S["hdr"][~S["geometry"]].tobytes() and (both != S["hdr"]).any(1)[S["geometry"]].mean() >= 0.5
    # the reference has the same properties
    assert (CR.compose(*args(S), ao=S["ao"], refl=S["refl"], ao_strength=0.0, reflection_strength=0.0) == S["hdr"]).all()
    assert (CR.compose(*args(S), ao=open_) == S["hdr"]).all()


def test_refusals_write_nothing(pkg, lib, S):
    L = lib.lib()
    n = 16
    a = {k: np.ascontiguousarray(S[k][:n]) for k in ("hdr", "base", "metal", "rough", "normal", "world", "ao", "refl")}
    a["geometry"] = np.ones(n, np.uint8)
    eye = np.array(EYE, np.float32)
    out = np.full((n, 3), -7.0, np.float32)
    good = np.zeros(1, pkg.scene.COMPOSE_DTYPE)
    good["flags"], good["ao_strength"], good["reflection_strength"] = 3, 0.5, 1.0
    p = lambda x: None if x is None else x.ctypes.data

    def call(c=good, e=eye, o=out, **kw):
        b = dict(a, **kw)
        return L.arctic_compose_pixels(p(c), p(e), AMBIENT, n, p(b["hdr"]), p(b["base"]), p(b["metal"]), p(b["rough"]), p(b["normal"]), p(b["world"]), p(b["ao"]),
                                       p(b["refl"]), p(b["geometry"]), p(o))

    def changed(**kw):
        c = good.copy()
        for k, v in kw.items():
            c[k] = v
        return c
    assert call() == 0 and (out != -7.0).all()
    out[:] = -7.0
    nan, inf = np.nan, np.inf
    # the header's order: the block, the flags, ao_strength, reflection_strength, reserved, the planes
    for c in [None, changed(flags=0), changed(flags=4), changed(flags=7), changed(flags=0x80000001), changed(ao_strength=-1e-9), changed(ao_strength=1.0000001),
              changed(ao_strength=nan), changed(ao_strength=inf), changed(reflection_strength=-1e-9), changed(reflection_strength=inf), changed(reflection_strength=nan),
              changed(reserved=(1, 0, 0, 0)), changed(reserved=(0, 0, 0, 9))]:
        assert call(c=c) == INVALID, None if c is None else c.tolist()
    for kw in [dict(ao=None), dict(refl=None), dict(hdr=None), dict(base=None), dict(metal=None), dict(rough=None), dict(normal=None), dict(world=None), dict(geometry=None)]:
        assert call(**kw) == INVALID, kw
    assert call(e=None) == INVALID and call(o=None) == INVALID
    assert (out == -7.0).all()                                                              # nothing written by a refused call
    # a plane whose flag is absent may be null; reflection_bias is the one call's and is not looked at here
    assert call(c=changed(flags=1, reflection_bias=nan), refl=None) == 0 and call(c=changed(flags=2), ao=None) == 0
    assert call(c=changed(ao_strength=0.0)) == 0 and call(c=changed(ao_strength=1.0, reflection_strength=0.0)) == 0
    with pytest.raises(pkg.renderer.ArcticError):
        pkg.renderer.compose_pixels(*args(S), ao=S["ao"], ao_strength=2.0)
    # the calls that need a handle refuse a null one before anything else
    assert L.arctic_compose_planes_device(None, None, None, None, None, None, None) == INVALID
    assert L.arctic_pass_ray_effects(None, None, None, None, None, None, None) == INVALID
    assert L.arctic_read_composed(None, None, None, None) == INVALID and L.arctic_compose_info(None, None) == INVALID
