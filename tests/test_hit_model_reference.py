"""The inputs of tests/test_gpu_hit_model.py, fixed on a machine without a GPU from the reference alone (tests/hit_model_scenes.py): the scene of
tests/hit_scenes.py under both assignments with 4 spot lights, 2 shadow-casting point lights whose 32 x 32 faces the host arbiter of the ray
queries traced, material extras in both storage layouts and the image-based ambient's tables from tests/env_reference.py.

Asserted here and again on the device: at most LEFT_OUT_CAP of the covered hits are left out with all four features on (grazing views under the
scaled normal, the hard cone ramp, the cube lookup's decisions, attributes that are not finite); every term is really there -- at least 200 judged
hits with a spot term, 200 that a cube light reaches, 50 from which one is hidden, 200 that emit --; and every deliberate defect of
tests/shading_reference.py (spot, cube, env, point) and of tests/material_reference.py moves the float64 colour by more than ten times the bar on at
least 20 judged hits of a case the device test runs, so a pass there tells each of them from the truth."""
import numpy as np
import pytest

import hit_model_scenes as HM
import hit_reference as HR
import hit_scenes as HS
import material_reference as XR
import shading_reference as SR
import test_gpu_extended_shading as G
import test_hit_reference as THR

ASSIGNMENTS = list(HS.ASSIGNMENTS)
SR_DEFECTS = [(m, f) for m, f in SR.MUTATIONS.items() if f in ("spot", "cube", "env", "point")]


@pytest.fixture(scope="module")
def lib(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    import os
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


@pytest.fixture(scope="module")
def truth(pkg, lib, oracle):
    """per assignment: the inputs, the attributes at the hits, 1 - shadow on the oracle's map, the tables, and the float64 colour per feature set"""
    out = {}
    for a in ASSIGNMENTS:
        I = HM.inputs(pkg, a)
        c = I.c
        attrs, mat = HR.hit_attributes(c.g.objects, c.g.meshes, c.mesh_materials, c.lpv, c.hits)
        lit = THR._lit(pkg, oracle, c, attrs, mat)
        env = HM.host_env(c)
        refs = {name: HM.reference(I, attrs, mat, lit, on, env=env) for name, on in dict(HM.SETS, none=()).items()}
        out[a] = dict(I=I, attrs=attrs, mat=mat, lit=lit, env=env, refs=refs)
    return out


def conditions(I, attrs, mat, lit, refs, faces=None):
    """what both sides assert of the inputs; refs: {feature set: HM.reference(...)} with "all", "none", "spot" and "extras" """
    full, none = refs["all"], refs["none"]
    cov = full.covered
    assert full.left_out <= HS.LEFT_OUT_CAP * cov.sum(), (full.left_out, int(cov.sum()), full.reasons)
    j = full.judged
    spot = (refs["spot"].rgba[:, :3] != none.rgba[:, :3]).any(1)
    some, hidden = HM.cube_terms(I, attrs, mat, lit, faces)
    emit = (refs["extras"].E != 0).any(1)
    counts = {"spot": int((spot & j).sum()), "cube, 0 < v": int((some & j).sum()), "cube, v = 0": int((hidden & j).sum()), "emission": int((emit & j).sum())}
    assert counts["spot"] >= 200 and counts["cube, 0 < v"] >= 200 and counts["cube, v = 0"] >= 50 and counts["emission"] >= 200, counts
    return dict(counts, covered=int(cov.sum()), left_out=full.left_out, reasons=full.reasons)


def defects_told_apart(I, attrs, mat, lit, env, refs):
    """every defect of the two references against the truth `refs` on the given inputs (the device test hands in what it read back): each moves at
    least 20 judged hits by more than ten times the bar -- a lighting defect on the case with its feature alone, a material defect with the extras
    alone and with all four features.  -> {defect: the smallest count}"""
    sets = dict(HM.SETS, none=())
    out = {}
    for defect, feature in SR_DEFECTS:
        name = feature if feature in HM.SETS else "none"
        bad = HM.reference(I, attrs, mat, lit, sets[name], env=env, sr_mutate=(defect,))
        out[defect] = int(((HM.rel_err(bad.rgba[:, :3], refs[name].rgba[:, :3]).max(1) > 10 * G.HDR_REL) & refs[name].judged).sum())
    for defect in XR.MUTATIONS:
        counts = []
        for name in ("extras", "all"):
            bad = HM.reference(I, attrs, mat, lit, sets[name], env=env, mutate=(defect,))
            counts.append(int(((HM.rel_err(bad.rgba[:, :3], refs[name].rgba[:, :3]).max(1) > 10 * G.HDR_REL) & refs[name].judged).sum()))
        out[defect] = min(counts)
    assert min(out.values()) >= 20, out
    return out


@pytest.mark.parametrize("assignment", ASSIGNMENTS)
def test_the_inputs_are_what_the_device_test_takes_them_for(pkg, truth, assignment):
    t = truth[assignment]
    I, refs = t["I"], t["refs"]
    HS.check_conditions(I.c, t["attrs"], t["mat"])
    print(assignment, conditions(I, t["attrs"], t["mat"], t["lit"], refs))
    print(assignment, defects_told_apart(I, t["attrs"], t["mat"], t["lit"], t["env"], refs))   # (the device test's form of the two tests below)
    # the re-aimed spot's axis meets the floor well inside it, and its rim crosses the floor: floor hits inside the cone and outside it
    inside, outside, axis = HM.rim_on_the_floor(I, t["attrs"], t["mat"])
    print(assignment, "re-aimed spot: floor hits inside", inside, "outside", outside, "hard cone ramp", refs["spot"].reasons["hard cone ramp"])
    assert inside >= 50 and outside >= 50 and abs(axis[0]) < 2 and abs(axis[2]) < 2 and abs(axis[1]) < 1e-6, (inside, outside, axis.tolist())
    assert SR.spot_constants(I.spots)[0]["hard"] and not any(k["hard"] for k in SR.spot_constants(I.spots)[1:])
    # the lights and the faces: 4 spot lights, 2 cube lights, faces of 32 x 32
    assert len(I.spots) == 4 and len(I.cubes) == 2 and all(f.shape == (6, HM.FACE, HM.FACE) and f.dtype == np.float32 for f in I.faces)
    for f in I.faces:   # traced: surfaces at many depths, and texels that see nothing
        assert (f < 1).mean() >= 0.3 and (f == 1).mean() >= 0.1 and len(np.unique(f)) >= 100
    lo, hi = I.c.g.tris.reshape(-1, 3).min(0), I.c.g.tris.reshape(-1, 3).max(0)
    assert all((lo < L["position"]).all() and (L["position"] < hi).all() for L in I.cubes)            # inside the scene
    # the three kinds of extras: neutral; every factor off neutral with both images at the packed size; images of unequal sizes
    assert I.extras[3] is None and XR.is_neutral(I.extras_ref[3])
    p, e, o = I.extras[0]
    d0 = I.c.images[0][0]
    assert e.shape == o.shape == d0.shape and all(np.any(np.asarray(p[f]) != np.asarray(XR.NEUTRAL[f], np.float32)) for f in XR.FIELDS)
    assert I.extras[1][1].shape != I.extras[1][2].shape
    # a feature that is on moves the colour of most judged hits; the misses are the base model's
    none = refs["none"]
    for name in HM.FEATURES:
        moved = (HM.rel_err(refs[name].rgba[:, :3], none.rgba[:, :3]).max(1) > 10 * G.HDR_REL) & refs[name].judged & none.judged
        used = (np.isin(t["mat"], [m for m, x in enumerate(I.extras) if x is not None]) if name == "extras" else np.ones(len(moved), bool))
        assert moved[used].sum() >= 200, (name, int(moved.sum()))
        assert np.array_equal(refs[name].rgba[~none.covered], none.rgba[~none.covered])


@pytest.mark.parametrize("defect,feature", SR_DEFECTS, ids=[m for m, _ in SR_DEFECTS])
def test_every_lighting_defect_is_told_from_the_truth(pkg, truth, defect, feature):
    """on the case the device test runs with that feature alone (a point light's defect: with none)"""
    seen = 0
    for a in ASSIGNMENTS:
        t = truth[a]
        name = feature if feature in HM.SETS else "none"
        ref = t["refs"][name]
        bad = HM.reference(t["I"], t["attrs"], t["mat"], t["lit"], dict(HM.SETS, none=())[name], env=t["env"], sr_mutate=(defect,))
        moved = (HM.rel_err(bad.rgba[:, :3], ref.rgba[:, :3]).max(1) > 10 * G.HDR_REL) & ref.judged
        print(a, defect, int(moved.sum()))
        assert moved.sum() >= 20, (a, defect, int(moved.sum()))
        seen += int(moved.sum())
    assert seen


@pytest.mark.parametrize("defect", XR.MUTATIONS)
def test_every_material_defect_is_told_from_the_truth(pkg, truth, defect):
    """with the extras alone and with all four features, on the assignment that uses the materials with extras of every kind between them"""
    for a in ASSIGNMENTS:
        t = truth[a]
        used = [m for m in t["I"].c.mesh_materials if t["I"].extras[m] is not None]
        for name in ("extras", "all"):
            ref = t["refs"][name]
            bad = HM.reference(t["I"], t["attrs"], t["mat"], t["lit"], HM.SETS[name], env=t["env"], mutate=(defect,))
            moved = (HM.rel_err(bad.rgba[:, :3], ref.rgba[:, :3]).max(1) > 10 * G.HDR_REL) & ref.judged
            print(a, name, defect, int(moved.sum()), used)
            assert moved.sum() >= 20, (a, name, defect, int(moved.sum()))
