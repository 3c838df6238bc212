"""The hit attributes on a machine without a GPU: arctic_interpolate_hits -- the library's own per-vertex arithmetic and interpolation on the
host -- against the numpy reference (tests/hit_reference.py, written from the header alone) bit for bit on the scene of tests/hit_scenes.py,
hits taken from arctic_trace_triangles; the reference's deliberate defects, each of which that scene tells from the truth; the eye of the shading
(the ray's origin, not the camera); the share of the covered hits the grazing mask leaves out; and the arbiter under the address and
undefined-behaviour sanitizers in a program of its own (tests/cpp/hit_attributes_sanitize.cpp)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hit_reference as HR
import hit_scenes as HS
import test_gpu_extended_shading as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSIGNMENTS = list(HS.ASSIGNMENTS)


@pytest.fixture(scope="module")
def lib(pkg):
    from importlib import import_module
    b = import_module("arctic_renderer_amd.binding")
    if not os.path.exists(b.LIB_PATH):
        import __graft_entry__ as entry
        entry.build()
    return b


@pytest.fixture(scope="module")
def truth(pkg, lib):
    """per assignment: (scene, attrs, material) of the reference"""
    out = {}
    for a in ASSIGNMENTS:
        c = HS.scene(pkg, a)
        out[a] = (c,) + HR.hit_attributes(c.g.objects, c.g.meshes, c.mesh_materials, c.lpv, c.hits)
    return out


@pytest.mark.parametrize("assignment", ASSIGNMENTS)
def test_the_arbiter_equals_the_reference_bit_for_bit(pkg, lib, truth, assignment):
    c, want_a, want_m = truth[assignment]
    got_a, got_m = HS.arbiter_attributes(pkg, c.g.objects, c.g.meshes, c.mesh_materials, c.lpv, c.hits)
    assert got_m.tobytes() == want_m.tobytes(), np.nonzero(got_m != want_m)[0][:8].tolist()
    assert HR.same_bytes(got_a) == HR.same_bytes(want_a), np.nonzero((got_a.view(np.uint32) != want_a.view(np.uint32)).any(1))[0][:8].tolist()
    print(HS.check_conditions(c, want_a, want_m))
    # ... and with the box elsewhere (the refit's pose), where only the first object's hits move
    moved_a, moved_m = HS.arbiter_attributes(pkg, c.g.moved, c.g.meshes, c.mesh_materials, c.lpv, c.hits)
    ref_a, ref_m = HR.hit_attributes(c.g.moved, c.g.meshes, c.mesh_materials, c.lpv, c.hits)
    assert HR.same_bytes(moved_a) == HR.same_bytes(ref_a) and moved_m.tobytes() == ref_m.tobytes()
    obj, _, _ = HR.prim_sources(c.g.objects, c.g.meshes)
    cov = want_m != HR.NO_MATERIAL
    changed = (moved_a.view(np.uint32) != want_a.view(np.uint32)).any(1)
    assert changed[cov][obj[c.hits["prim"][cov]] == 0].mean() >= 0.9 and not changed[cov][obj[c.hits["prim"][cov]] != 0].any()


def test_the_edges_and_the_records_nobody_resolves(pkg, lib, truth):
    c, a, m = truth[ASSIGNMENTS[0]]
    v = HR.vertex_attributes(c.g.meshes[1][0], c.g.objects[3]["trs"], c.lpv)
    obj, idx, _ = HR.prim_sources(c.g.objects, c.g.meshes)
    floor = [k for k in c.edge[0] if obj[c.hits["prim"][k]] == 3]
    assert floor
    for k in floor:   # u = 0: the third vertex's weight is v, the first's 1 - v, the second's attribute times zero adds +-0
        i0, _, i2 = idx[c.hits["prim"][k]]
        w0 = (np.float32(1.0) - np.float32(0.0)) - c.hits["v"][k]
        assert np.allclose(a[k], w0 * v[i0] + c.hits["v"][k] * v[i2], rtol=1e-6, atol=1e-7)
    assert (m[c.handmade] == HR.NO_MATERIAL).all() and not a[c.handmade].any()
    assert c.hits["prim"][c.handmade].tolist() == [c.g.skipped, c.g.n_prims, c.g.n_prims + 5, 0xFFFFFFFE, c.g.n_prims, c.g.skipped]


@pytest.mark.parametrize("defect", HR.DEFECTS)
def test_the_scene_tells_each_defect_from_the_truth(pkg, lib, truth, defect):
    c, want_a, want_m = truth[ASSIGNMENTS[0]]
    a, m = HR.hit_attributes(c.g.objects, c.g.meshes, c.mesh_materials, c.lpv, c.hits, defect=defect)
    cov = want_m != HR.NO_MATERIAL
    moved = (a.view(np.uint32) != want_a.view(np.uint32)).any(1) | (m != want_m)
    assert (moved & cov).sum() >= 100, (defect, int((moved & cov).sum()))
    # not by a rounding: the attributes of the moved hits differ by more than 1e-3 of the scene somewhere
    far = np.nanmax(np.abs(a.astype(np.float64) - want_a.astype(np.float64)), axis=1) > 1e-3
    assert (far & cov).sum() >= 100, (defect, int((far & cov).sum()))


def _lit(pkg, oracle, c, attrs, mat):
    """1 - shadow per covered hit on the sun's map as the CPU oracle draws it (the device draws the same map: tests/test_gpu_parity.py)"""
    o = oracle.Oracle(64, 64, HS.SHADOW, HS.MAX_LIGHTS)
    for d, n, m in c.images:
        o.create_material(d, n, m)
    for (v, i), m in zip(c.g.meshes, c.mesh_materials):
        o.create_mesh(v, i, m)
    have = pkg.scene.make_objects([(ob["trs"], int(ob["mesh_idx"])) for ob in c.g.objects if int(ob["mesh_idx"]) < len(c.g.meshes)])
    o.pass_shadow_map(HS.description(pkg, have))
    shadow = o.read_shadow_map()
    o.close()
    return HS.sun_lit(oracle, shadow, attrs, mat)


@pytest.mark.parametrize("assignment", ASSIGNMENTS)
def test_the_shading_inputs(pkg, lib, oracle, truth, assignment):
    """the mask leaves out at most 5 % of the covered hits; the sun's map shadows some hits and not others; and the eye matters: with the camera's eye
    instead of each ray's origin at least half of the judged hits move by more than 10 x the gate"""
    c, attrs, mat = truth[assignment]
    lit = _lit(pkg, oracle, c, attrs, mat)
    ref = HS.shade_reference(c, c.rays, attrs, mat, lit)
    HS.check_conditions(c, attrs, mat, ref.judged)
    cov = ref.covered
    assert (lit[cov] == 0).mean() >= 0.02 and (lit[cov] == 1).mean() >= 0.3, ((lit[cov] == 0).mean(), (lit[cov] == 1).mean())
    assert ref.sky.sum() >= 200 and ref.invalid.sum() >= 8 * HS.N_ORIGINS
    assert (ref.rgba[ref.sky, :3] > 0).all() and not ref.rgba[ref.invalid].any() and (ref.rgba[ref.sky | ref.invalid, 3] == 0).all()
    wrong = HS.shade_reference(c, c.rays, attrs, mat, lit, eyes=[c.desc.camera["eye"]] * HS.N_ORIGINS)
    j = ref.judged               # every judged hit, the fully shadowed ones included (their point lights still have an eye)
    rel = (np.abs(wrong.rgba[:, :3] - ref.rgba[:, :3]) / (np.abs(ref.rgba[:, :3]) + 1e-3)).max(1)
    moved = rel > 10 * G.HDR_REL
    print(f"{assignment}: covered {int(cov.sum())}, left out {int((cov & ~ref.judged).sum())}, sky {int(ref.sky.sum())}, "
          f"fully shadowed {float((lit[cov] == 0).mean()):.3f}, moved by the eye {float(moved[j].mean()):.3f} of the judged hits, "
          f"{float(moved[j & (lit > 0)].mean()):.3f} of those the sun reaches")
    assert moved[j].mean() >= 0.5, moved[j].mean()


def test_reflection_rays_of_the_reference():
    """the ray rule by hand on four pixels: a mirror facing the eye, one facing away, a degenerate normal, no geometry"""
    attrs = np.zeros((1, 4, 18), np.float32)
    attrs[0, :, 11:14] = (0, 0, 0)
    attrs[0, 0, 8:11] = (0, 2, 0)            # not a unit vector: m = (0, 1, 0)
    attrs[0, 1, 8:11] = (0, -1, 0)
    attrs[0, 2, 8:11] = (0, 0, 0)
    attrs[0, 3, 8:11] = (0, 1, 0)
    mat = np.array([[0, 0, 0, HR.NO_MATERIAL]], np.uint32)
    rays, has = HR.reflection_rays(attrs, mat, (3, 4, 0), 0.5)
    assert has.tolist() == [True, False, False, False]
    assert rays["direction"][0].tolist() == [-3, 4, 0] and rays["origin"][0].tolist() == [0, 0.5, 0] and rays["t_min"][0] == 0 and np.isinf(rays["t_max"][0])
    assert rays[1:].tobytes() == bytes(3 * 32)


def test_arbiter_under_sanitizers(pkg, lib, truth, tmp_path):
    """tests/cpp/hit_attributes_sanitize.cpp: a program of its own (the sanitizers' runtime is never loaded into python), on its own cases and
    on the scene above"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "arctic-renderer_amd", "csrc")
    driver = os.path.join(ROOT, "tests", "cpp", "hit_attributes_sanitize")
    src = [os.path.join(ROOT, "tests", "cpp", "hit_attributes_sanitize.cpp"), os.path.join(csrc, "hit_attributes.cpp")]
    deps = src + [os.path.join(csrc, "ray_query.h"), os.path.join(csrc, "hit_attributes.h")]
    if not os.path.exists(driver) or any(os.path.getmtime(s) > os.path.getmtime(driver) for s in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", driver] + src)
    c, want_a, want_m = truth[ASSIGNMENTS[0]]
    have = [ob for ob in c.g.objects if int(ob["mesh_idx"]) < len(c.g.meshes)]
    blob = struct.pack("<Q", len(have))
    for ob in have:
        v, ix = c.g.meshes[int(ob["mesh_idx"])]
        blob += struct.pack("<QQ", len(v), len(ix)) + np.asarray(ob["trs"], np.float32).tobytes() + struct.pack("<I", c.mesh_materials[int(ob["mesh_idx"])])
        blob += np.ascontiguousarray(v).tobytes() + np.ascontiguousarray(ix, np.uint32).tobytes()
    blob += np.asarray(c.lpv, np.float32).tobytes() + struct.pack("<Q", len(c.hits)) + np.ascontiguousarray(c.hits).tobytes()
    (tmp_path / "scene.bin").write_bytes(blob)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver, str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = out.stdout.splitlines()
    assert len(lines) >= 15 and all(l.startswith("ok") for l in lines)
    for name in ("empty", "no-hits", "large-20000", "no-vertices", "indices-out-of-range", "nan-and-inf-vertices", "huge-1e30", "refusals", "nothing-to-do", "scene"):
        assert any(l.startswith("ok " + name) for l in lines), name
    raw = (tmp_path / "out.bin").read_bytes()
    n = len(c.hits)
    assert len(raw) == n * 76
    assert HR.same_bytes(np.frombuffer(raw[:n * 72], np.float32)) == HR.same_bytes(want_a.reshape(-1)) and raw[n * 72:] == want_m.tobytes()
