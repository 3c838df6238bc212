"""ARCTIC_OPT_HIT_MODEL = 1 on the device (needs an MI355X): k_shade_hits_ext against the independent float64 pixel of tests/material_reference.py
on tests/shading_reference.py at the project's standing HDR bar, |got - want| / (|want| + 1e-3) <= 1e-4 (HDR_REL of
tests/test_gpu_extended_shading.py), on the inputs tests/hit_model_scenes.py makes and tests/test_hit_model_reference.py pins on the CPU: the scene
of tests/hit_scenes.py under both assignments, each of material extras, spot lights, shadow-casting point lights and the image-based ambient alone
and all four together, the packed images row-major and in 4 x 4 tiles (the same bytes).  64 x 64 handle, 4096 rays, sun map 64 x 64, environment
map 64 x 32, cube faces 32 x 32, written with arctic_write_point_shadow as the host traced them -- and once drawn by the handle itself.

What is read back from the handle are inputs: the attributes at the hits, the sun's map, the tables of the image-based ambient, the drawn faces.
Bytes where bytes are promised: a handle with none of the four features gives the base model's bytes under option 1 (host and device forms); back
at option 0 a handle with all of them gives the bytes of one that never set it; arctic_trace_gi at n_rays = 1 is its published rays traced and
shaded through the public calls; arctic_trace_reflections is arctic_shade_hits_device of its rays and hits.  Cube lights whose faces were never
filled are refused with ARCTIC_E_STATE and nothing is written.

Measured (profiles/hit_model_parity.json, written when ARCTIC_HIT_MODEL_PARITY_JSON names a file): relative HDR error at most 4.5e-6 over the five
feature sets of the first assignment and 1.8e-5 of the second (all four together), the sky 2.5e-7; 76 of 3176 and 64 of 3150 covered hits left
out with all four on (56 and 48 of them the cube lookup's decisions, 11 and 7 the hard cone's ramp); faces drawn by the handle 1.9e-6, 15 left
out.  The gate stays at the project's bar.  Every deliberate defect of the two float64 references is also evaluated on the attributes, the map
and the tables read back here (test_hit_model_reference.defects_told_apart): each moves at least 20 judged hits by ten times the bar."""
import json
import os

import numpy as np
import pytest

import gi_reference as GI
import gi_scenes as GS
import hit_model_scenes as HM
import hit_reference as HR
import hit_scenes as HS
import test_gpu_extended_shading as G
import test_hit_model_reference as TR

pytestmark = pytest.mark.gpu
F = np.float32
ASSIGNMENTS = list(HS.ASSIGNMENTS)
INVALID, STATE = -1, -4
BIAS = 2e-3
_record = {}


@pytest.fixture(scope="module", autouse=True)
def _parity_record():
    yield
    out = os.environ.get("ARCTIC_HIT_MODEL_PARITY_JSON")
    if out and _record:
        import __graft_entry__ as entry
        json.dump({"source": entry.source_id(), "gate_hdr_rel": G.HDR_REL, "grazing": G.GRAZING, "left_out_cap": HS.LEFT_OUT_CAP, "cases": _record}, open(out, "w"), indent=1)


def handle(pkg, hip, c, tiling=0, width=64, height=64):
    r = hip.Renderer(width, height, HS.SHADOW, HS.MAX_LIGHTS)
    r.set_option("texture_tiling", tiling)      # before the materials are created
    r.set_option("point_shadow_size", HM.FACE)
    HS.upload(pkg, r, c)
    return r


def configure(r, I, on, write_faces=True):
    """the handle's tables for the feature set `on`, everything else cleared"""
    r.update_spot_lights(I.spots if "spot" in on else I.spots[:0])
    r.update_point_shadow_lights(I.cubes if "cube" in on else I.cubes[:0])
    if "cube" in on and write_faces:
        for i, f in enumerate(I.faces):
            r.write_point_shadow(i, f)
    r.set_option("env_lighting", int("env" in on))
    for m, x in enumerate(I.extras):
        r.set_material_extras(m, *((x if "extras" in on else None) or (None, None, None)))


def device_form(r, c, n=None):
    import torch
    n = len(c.rays) if n is None else n
    d_rays = torch.from_numpy(c.rays[:n].view(np.float32).reshape(-1, 8).copy()).cuda()
    d_hits = torch.from_numpy(c.hits[:n].view(np.uint32).reshape(-1, 4).copy().view(np.int32)).cuda()
    d_out = torch.full((n + 4, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return d_rays, d_hits, d_out


def judge(name, got, ref):
    """the bar on the judged hits and along the sky; exact zeros where nothing is to be seen; alpha"""
    rel = HM.rel_err(got[:, :3], ref.rgba[:, :3])
    j, cov = ref.judged, ref.covered
    rec = {"covered": int(cov.sum()), "judged": int(j.sum()), "left_out": ref.left_out, "reasons": ref.reasons, "hdr_rel": float(rel[j].max()),
           "sky": int(ref.sky.sum()), "sky_rel": float(rel[ref.sky].max())}
    _record[name] = rec
    print(name, rec)
    assert (got[cov, 3] == 1).all() and (got[~cov, 3] == 0).all(), name
    assert not got[ref.invalid].any(), name                                      # an invalid direction: exactly {0, 0, 0, 0}
    worst = int(np.argmax(np.where(j, rel.max(1), -1)))
    assert rec["hdr_rel"] <= G.HDR_REL, (name, rec, worst, got[worst].tolist(), ref.rgba[worst].tolist())
    assert rec["sky_rel"] <= G.HDR_REL, (name, rec)
    return rec


@pytest.mark.parametrize("assignment", ASSIGNMENTS)
def test_against_the_float64_pixel(pkg, hip, oracle, assignment):
    I = HM.inputs(pkg, assignment)
    c = I.c
    never = handle(pkg, hip, c)                                                  # a handle that never sets the option
    never.pass_shadow_map(c.desc)
    base = never.shade_hits(c.desc, c.rays, c.hits)
    r = handle(pkg, hip, c)
    r.pass_shadow_map(c.desc)
    attrs, mat = r.hit_attributes(c.desc, c.hits)                                # inputs
    lit = HS.sun_lit(oracle, r.read_shadow_map(), attrs, mat)
    HS.check_conditions(c, attrs, mat)
    for bad in (2, -1, 7):
        with pytest.raises(hip.ArcticError) as e:
            r.set_option("hit_model", bad)
        assert e.value.code == INVALID
    assert r.shade_hits(c.desc, c.rays, c.hits).tobytes() == base.tobytes()      # a refused value changes nothing
    r.set_hit_model(1)
    # P1: none of the four features on the handle -- the base model's bytes, host and device forms
    p1 = r.shade_hits(c.desc, c.rays, c.hits)
    assert p1.tobytes() == base.tobytes(), int((p1 != base).any(1).sum())
    d_rays, d_hits, d_out = device_form(r, c)
    r.shade_hits_device(c.desc, d_rays.data_ptr(), d_hits.data_ptr(), len(c.rays), d_out.data_ptr())
    r.flush()
    host = d_out.cpu().numpy()
    assert host[:len(c.rays)].tobytes() == base.tobytes() and (host[len(c.rays):] == -7.0).all()
    # each feature alone and all four together against float64
    refs, env, got = {"none": HM.reference(I, attrs, mat, lit, ())}, None, {}
    for name, on in HM.SETS.items():
        configure(r, I, on)
        if "env" in on and env is None:
            env = r.read_env_lighting()                                          # inputs: the tables as the handle built them
        got[name] = r.shade_hits(c.desc, c.rays, c.hits)
        assert got[name].shape == (len(c.rays), 4) and got[name].dtype == np.float32
        refs[name] = HM.reference(I, attrs, mat, lit, on, env=env)
        rec = judge(f"{assignment}, {name}", got[name], refs[name])
        assert rec["left_out"] <= HS.LEFT_OUT_CAP * rec["covered"], rec
        moved = (got[name][:, :3] != base[:, :3]).any(1)
        assert moved[refs[name].covered].sum() >= 200 and not moved[~refs[name].covered].any(), (name, int(moved.sum()))
    print(assignment, TR.conditions(I, attrs, mat, lit, refs))                   # the cap and the terms, as the CPU test asserts them
    print(assignment, TR.defects_told_apart(I, attrs, mat, lit, env, refs))      # ... and every defect against the truth, on what was read back
    # the device form of all four
    d_rays, d_hits, d_out = device_form(r, c)
    r.shade_hits_device(c.desc, d_rays.data_ptr(), d_hits.data_ptr(), len(c.rays), d_out.data_ptr())
    r.flush()
    host = d_out.cpu().numpy()
    assert host[:len(c.rays)].tobytes() == got["all"].tobytes() and (host[len(c.rays):] == -7.0).all()
    # in tiles of 4 x 4 texels (forced on before the materials are created): the same bytes
    t = handle(pkg, hip, c, tiling=1)
    t.pass_shadow_map(c.desc)
    t.set_hit_model(1)
    configure(t, I, HM.FEATURES)
    tiled = t.shade_hits(c.desc, c.rays, c.hits)
    assert tiled.tobytes() == got["all"].tobytes(), int((tiled != got["all"]).any(1).sum())
    t.close()
    # the option back to 0 with everything still on the handle: the bytes of a handle that never set it
    r.set_hit_model(0)
    assert r.shade_hits(c.desc, c.rays, c.hits).tobytes() == base.tobytes()
    assert never.shade_hits(c.desc, c.rays, c.hits).tobytes() == base.tobytes()
    r.close()
    never.close()


def test_cube_faces_drawn_by_the_handle(pkg, hip, oracle):
    """arctic_pass_point_shadows draws the faces; read back, they are inputs like the traced ones"""
    from types import SimpleNamespace
    I = SimpleNamespace(**dict(vars(HM.inputs(pkg, ASSIGNMENTS[0])), cubes=HM.cubes_above(pkg), faces=None))
    c = I.c
    r = handle(pkg, hip, c)
    r.pass_shadow_map(c.desc)
    r.set_hit_model(1)
    configure(r, I, ("cube",), write_faces=False)
    r.pass_point_shadows(c.desc)
    faces = [r.read_point_shadow(i) for i in range(len(I.cubes))]
    assert all(f.shape == (6, HM.FACE, HM.FACE) and (f < 1).any() and (f == 1).any() for f in faces)   # (the pass culls front faces: the floor seen from above is not in them)
    attrs, mat = r.hit_attributes(c.desc, c.hits)
    lit = HS.sun_lit(oracle, r.read_shadow_map(), attrs, mat)
    ref = HM.reference(I, attrs, mat, lit, ("cube",), faces=faces)
    some, hidden = HM.cube_terms(I, attrs, mat, lit, faces)
    got = r.shade_hits(c.desc, c.rays, c.hits)
    rec = judge("faces drawn by the handle", got, ref)
    rec.update({"cube, 0 < v": int((some & ref.judged).sum()), "cube, v = 0": int((hidden & ref.judged).sum())})
    print(rec)
    assert rec["cube, 0 < v"] >= 200 and rec["cube, v = 0"] >= 50, rec
    assert rec["left_out"] <= HS.LEFT_OUT_CAP * rec["covered"], rec
    r.close()


def test_cube_lights_whose_faces_were_never_filled_are_refused(pkg, hip):
    import torch
    I = HM.inputs(pkg, ASSIGNMENTS[0])
    c = I.c
    r = handle(pkg, hip, c, width=64, height=48)
    desc = pkg.scenes.SceneDesc(camera=dict(c.desc.camera, aspect=64 / 48), ambient=HS.AMBIENT, sun=c.desc.sun, objects=c.g.objects)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    r.update_point_shadow_lights(I.cubes)
    under0 = r.shade_hits(desc, c.rays[:64], c.hits[:64])                        # option 0 never asks
    r.set_hit_model(1)
    d_rays, d_hits, d_out = device_form(r, c, 64)
    plane = torch.full((48 * 64 + 4, 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def refused(call):
        with pytest.raises(hip.ArcticError) as e:
            call()
        assert e.value.code == STATE and "faces" in str(e.value), e.value
    dirs = GS.cosine_table(1, 2, 12)
    calls = [lambda: r.shade_hits(desc, c.rays[:64], c.hits[:64]),
             lambda: r.shade_hits_device(desc, d_rays.data_ptr(), d_hits.data_ptr(), 64, d_out.data_ptr()),
             lambda: r.trace_reflections(desc, BIAS),
             lambda: r.trace_reflections_device(desc, BIAS, plane.data_ptr()),
             lambda: r.trace_gi(desc, dirs, bias=BIAS),
             lambda: r.trace_gi_device(desc, dirs, plane.data_ptr(), bias=BIAS)]
    for call in calls:
        refused(call)
    r.flush()
    assert (d_out.cpu().numpy() == -7.0).all() and (plane.cpu().numpy() == -7.0).all()      # a refused call writes nothing
    r.write_point_shadow(0, I.faces[0])                                          # written: the list's faces count as filled
    assert (r.shade_hits(desc, c.rays[:64], c.hits[:64])[:, 3] == under0[:, 3]).all()
    r.update_point_shadow_lights(I.cubes)                                        # the list set again: cleared faces, refused again
    refused(calls[0])
    r.pass_point_shadows(desc)                                                   # drawn
    r.shade_hits(desc, c.rays[:64], c.hits[:64])
    r.set_option("point_shadow_size", 2 * HM.FACE)                               # another F: cleared faces
    refused(calls[0])
    r.set_hit_model(0)
    assert r.shade_hits(desc, c.rays[:64], c.hits[:64]).tobytes() == under0.tobytes()
    r.close()


def test_the_consumers_follow(pkg, hip):
    """the reflection plane and the indirect light go through the same choke point: under option 1 each is still the public calls by hand"""
    import torch
    I = HM.inputs(pkg, ASSIGNMENTS[0])
    c = I.c
    width, height = 64, 48
    desc = pkg.scenes.SceneDesc(camera=dict(c.desc.camera, aspect=width / height), ambient=HS.AMBIENT, sun=c.desc.sun, objects=c.g.objects)
    r = handle(pkg, hip, c, width=width, height=height)
    r.pass_shadow_map(desc)
    r.pass_gbuffer(desc)
    attrs, mat, _, _ = r.read_gbuffer(want=("attrs", "material"))
    configure(r, I, ("spot",))                                                   # the spot-lit scene
    plane0 = r.trace_reflections(desc, BIAS)
    gi0 = r.trace_gi(desc, GS.cosine_table(1, 2, 12), bias=BIAS, clamp_max=8.0)
    r.set_hit_model(1)
    plane1 = r.trace_reflections(desc, BIAS)
    differ = (plane1 != plane0).any(-1)
    assert differ.sum() >= 50 and (plane1[..., 3] == plane0[..., 3]).all(), int(differ.sum())
    rays, has = HR.reflection_rays(attrs, mat, desc.camera["eye"], BIAS)
    hits = r.trace_rays(desc, rays)
    d_rays = torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()
    d_hits = torch.from_numpy(hits.view(np.uint32).reshape(-1, 4).copy().view(np.int32)).cuda()
    d_out = torch.full((len(rays), 4), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r.shade_hits_device(desc, d_rays.data_ptr(), d_hits.data_ptr(), len(rays), d_out.data_ptr())
    r.flush()
    assert d_out.cpu().numpy().tobytes() == plane1.tobytes()
    assert (has & (hits["prim"] != HR.NO_PRIM)).sum() >= 300
    # the indirect light at n_rays = 1: the published rays, traced and shaded through the public calls on the same handle
    configure(r, I, HM.FEATURES)
    dirs = GS.cosine_table(1, 2, 12)
    kw = dict(bias=BIAS, clamp_max=8.0)
    g_rays = r.gi_rays(dirs, 0, **kw)[None]
    g_hits = r.trace_rays(desc, g_rays[0].ravel()).reshape(g_rays.shape)
    colors = r.shade_hits(desc, g_rays[0].ravel(), g_hits[0].ravel()).reshape(g_rays.shape + (4,))
    want = GI.estimate(GI.add(g_rays, colors, kw["clamp_max"]))
    got = r.trace_gi(desc, dirs, **kw)
    assert got.tobytes() == want.tobytes(), int((got != want).any(-1).sum())
    had, hit = g_rays["t_max"] > 0, g_hits["prim"] != HR.NO_PRIM
    assert (had & hit).sum() >= 150 and (got != gi0).any(-1).sum() >= 50       # rays that hit, and an estimate the extended model moved
    r.close()
