"""arctic_hit_attributes on the device (needs an MI355X): k_hit_attributes against tests/hit_reference.py -- numpy float32 written from the header
alone, pinned to the host arbiter by tests/test_hit_reference.py -- bit for bit, as bytes, on the scene of tests/hit_scenes.py: as built, with
the shared mesh posed, with morph weights set, after a refit and after a re-split.  What is read back from the handle are inputs: the vertices in
use (arctic_read_mesh_vertices).  (Bytes: with every NaN as one pattern -- hit_reference.same_bytes; two of the 4096 records carry a NaN u or v.)"""
import numpy as np
import pytest

import hit_reference as HR
import hit_scenes as HS

pytestmark = pytest.mark.gpu
F = np.float32
ASSIGNMENT = "packed 64 / unequal"


@pytest.fixture(scope="module")
def case(pkg):
    return HS.scene(pkg, ASSIGNMENT)


def handle(pkg, hip, c, refit=0):
    r = HS.upload(pkg, hip.Renderer(64, 64, HS.SHADOW, HS.MAX_LIGHTS), c)
    r.set_option("ray_refit", refit)
    return r


def check(pkg, r, c, desc, what):
    """the device against the reference on the vertices in use and the objects of `desc`; -> (attrs, material)"""
    meshes = [(r.read_mesh_vertices(k, len(v)), i) for k, (v, i) in enumerate(c.g.meshes)]
    want_a, want_m = HR.hit_attributes(desc.objects, meshes, c.mesh_materials, c.lpv, c.hits)
    got_a, got_m = r.hit_attributes(desc, c.hits)
    assert got_m.tobytes() == want_m.tobytes(), (what, np.nonzero(got_m != want_m)[0][:8].tolist())
    differ = np.nonzero(((got_a.view(np.uint32) != want_a.view(np.uint32)) & ~(np.isnan(got_a) & np.isnan(want_a))).any(1))[0]
    assert HR.same_bytes(got_a) == HR.same_bytes(want_a), (what, len(differ), differ[:8].tolist(), got_a[differ[:2]].tolist(), want_a[differ[:2]].tolist())
    return want_a, want_m


def test_the_scene_as_built(pkg, hip, case):
    c = case
    r = handle(pkg, hip, c)
    a, m = check(pkg, r, c, c.desc, "as built")
    print(HS.check_conditions(c, a, m))
    assert r.ray_scene_info()[2] == 1
    check(pkg, r, c, c.desc, "again")                                            # the table and the structure stay
    assert r.ray_scene_info()[2] == 1
    got_a, got_m = r.hit_attributes(c.desc, c.hits[:0])                          # nothing to do
    assert got_a.shape == (0, 18) and got_m.shape == (0,)
    one_a, one_m = r.hit_attributes(c.desc, c.hits[37:38])                       # a single lane
    assert HR.same_bytes(one_a) == HR.same_bytes(a[37:38]) and one_m.tobytes() == m[37:38].tobytes()
    r.close()


def test_posed(pkg, hip, case):
    """the mesh the two boxes share, posed (arctic_set_mesh_pose): both instances follow"""
    c = case
    r = handle(pkg, hip, c)
    base, _ = check(pkg, r, c, c.desc, "before the pose")
    v = c.g.meshes[0][0]
    s = np.zeros(len(v), pkg.scene.SKIN_VERTEX_DTYPE)
    s["joints"][:, 1] = 1
    w = ((v["position"][:, 0] + 0.8) / 1.6).astype(F)
    s["weights"][:, 0], s["weights"][:, 1] = F(1) - w, w
    r.set_mesh_skin(0, s, 2)
    lift = np.eye(4, dtype=F); lift[1, 3] = 0.4; lift[0, 1] = 0.25
    r.set_mesh_pose(0, np.stack([np.eye(4, dtype=F).T.reshape(16), lift.T.reshape(16)]))
    posed, m = check(pkg, r, c, c.desc, "posed")
    obj, _, _ = HR.prim_sources(c.g.objects, c.g.meshes)
    cov = m != HR.NO_MATERIAL
    on_box = obj[c.hits["prim"][cov]] != 3
    changed = (posed.view(np.uint32) != base.view(np.uint32)).any(1)[cov]
    assert changed[on_box].mean() >= 0.5 and not changed[~on_box].any()
    r.close()


def test_morphed(pkg, hip, case):
    c = case
    r = handle(pkg, hip, c)
    base, _ = check(pkg, r, c, c.desc, "before the weights")
    v = c.g.meshes[0][0]
    rng = np.random.default_rng(63)
    d = np.zeros((2, len(v)), pkg.scene.MORPH_DELTA_DTYPE)
    d["position"][0] = rng.uniform(-0.1, 0.1, (len(v), 3)).astype(F)
    d["normal"][0] = rng.uniform(-0.3, 0.3, (len(v), 3)).astype(F)
    d["tangent"][1] = rng.uniform(-0.3, 0.3, (len(v), 3)).astype(F)
    d["position"][1, :, 1] = 0.2
    r.set_mesh_morph_targets(0, d)
    r.set_mesh_morph_weights(0, [0.75, -0.5])
    morphed, m = check(pkg, r, c, c.desc, "morphed")
    cov = m != HR.NO_MATERIAL
    assert (morphed.view(np.uint32) != base.view(np.uint32)).any(1)[cov].mean() >= 0.3
    r.close()


def test_after_a_refit_and_after_a_resplit(pkg, hip, case):
    """ARCTIC_OPT_RAY_REFIT = 1: a changed trs is followed by a refit, not a build, and the table of sources made behind the build still stands;
    then arctic_ray_scene_resplit, which reorders the structure's slots but not the scene's prims"""
    c = case
    r = handle(pkg, hip, c, refit=1)
    # (a structure is refittable only when every object's mesh exists: the entry without a mesh is left out here; it has no prims, so the scene's
    # numbering and the hit records stay what they are)
    have = [k for k, ob in enumerate(c.g.objects) if int(ob["mesh_idx"]) < len(c.g.meshes)]
    here, moved = HS.description(pkg, c.g.objects[have]), HS.description(pkg, c.g.moved[have])
    base, _ = check(pkg, r, c, here, "built under the option")
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info()[:2] == (0, 1)
    whole, _ = HR.hit_attributes(c.g.objects, c.g.meshes, c.mesh_materials, c.lpv, c.hits)
    assert HR.same_bytes(base) == HR.same_bytes(whole)
    after, m = check(pkg, r, c, moved, "refitted")
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info()[0] == 1
    assert HR.same_bytes(after) != HR.same_bytes(base)
    # the structure the refit left is the moved scene's: its hits are the arbiter's for the moved triangles
    import ray_reference as R
    tris, prims = R.world_triangles(moved.objects, c.g.meshes)
    want = pkg.renderer.trace_triangles(tris, c.rays)
    found = want["prim"] != HR.NO_PRIM
    want["prim"][found] = prims[want["prim"][found]]
    assert r.trace_rays(moved, c.rays).tobytes() == want.tobytes()
    r.ray_scene_resplit(moved)
    assert r.ray_resplit_info()[0] == 1 and r.ray_resplit_info()[2] == 0
    again, _ = check(pkg, r, c, moved, "re-split")
    assert HR.same_bytes(again) == HR.same_bytes(after) and r.ray_scene_info()[2] == 1
    check(pkg, r, c, here, "and back")
    assert r.ray_scene_info()[2] == 1 and r.ray_refit_info()[0] == 2
    r.close()


def test_refusals_write_nothing(pkg, hip, case):
    c = case
    r = handle(pkg, hip, c)
    L, s = r.L, c.desc.fill(pkg.scene.CScene())
    import ctypes as C
    hits = np.ascontiguousarray(c.hits[:8])
    attrs, mat = np.full((8, 18), 77, F), np.full(8, 77, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.arctic_hit_attributes(None, C.byref(s), p(hits), 8, p(attrs), p(mat)) == -1
    assert L.arctic_hit_attributes(r.h, None, p(hits), 8, p(attrs), p(mat)) == -1
    assert L.arctic_hit_attributes(r.h, C.byref(s), None, 8, p(attrs), p(mat)) == -1
    assert L.arctic_hit_attributes(r.h, C.byref(s), p(hits), 8, None, p(mat)) == -1
    assert L.arctic_hit_attributes(r.h, C.byref(s), p(hits), 8, p(attrs), None) == -1
    assert L.arctic_hit_attributes(r.h, C.byref(s), p(hits), 1 << 32, p(attrs), p(mat)) == -5
    assert (attrs == 77).all() and (mat == 77).all()
    assert L.arctic_hit_attributes(r.h, C.byref(s), p(hits), 8, p(attrs), p(mat)) == 0 and (mat != 77).all()
    r.close()
