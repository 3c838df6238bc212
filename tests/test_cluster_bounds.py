"""The object-space boxes of ARCTIC_OPT_CLUSTER_CULL on the host (arctic_cluster_bounds = renderer.cpp's cluster_bounds, the function
arctic_create_mesh keeps a mesh's boxes from), without a device.

k_vertex may skip a vertex block only if k_setup skips every cluster that reads one of its vertices; box_outside makes that follow from ONE
property of the host's tables: a block's box contains the box of each of those clusters.  Here: the tables are their definition, bit for bit;
the property holds on every mesh; the rule the library had before (a block's box = the union of its TRIANGLES' boxes) breaks it on the very
meshes used here, so the meshes can tell the two apart; and the camera and sun sequences of the reused-handle GPU tests
(tests/test_gpu_cluster_cull.py) are not vacuous -- under the old rule, a float64 replay of box_outside finds hundreds of triangles of kept
clusters reading skipped blocks in each of them, under the library's tables none.
"""
import numpy as np
import pytest

import cluster_cull_cases as CC


@pytest.fixture(scope="module")
def R(pkg):
    from importlib import import_module
    return import_module("arctic_renderer_amd.renderer")


@pytest.fixture(scope="module")
def config3(pkg):
    return pkg.scenes.config3(scale=0.5)


@pytest.fixture(scope="module")
def meshes(pkg, config3):
    """{name: (vertices, indices)}: the quads, every mesh of config 3 at 0.5, and each of them with its triangles permuted"""
    S = pkg.scenes
    plain = {"quad24": CC.small_quad(S), "quad48": CC.big_quad(S)}
    plain.update({f"config3-mesh{k}": (v, i) for k, (v, i, _) in enumerate(config3.meshes)})
    out = dict(plain)
    out.update({name + "-permuted": (v, CC.permuted(i, 77 + k)) for k, (name, (v, i)) in enumerate(plain.items())})
    return out


def _same_bits(a, b):
    np.testing.assert_array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _edge_meshes(S):
    """meshes the host cannot bound everywhere, and ragged sizes"""
    v, i = S.quad((-1, -1, 0), (2, 0, 0), (0, 2, 0), 40, 40)            # 3200 triangles, 1681 vertices (7 blocks, the last of 145)
    out = {}
    out["ragged"] = (v, i[: 3 * 1000])                                   # 1000 triangles: the last cluster holds 232, and whole blocks go unused
    bad = i.copy()
    bad[5 * 3] = len(v) + 7                                              # indices out of range: those triangles bound nothing
    bad[300 * 3 + 1] = 0xFFFFFFFF
    bad[3 * 256 * 2: 3 * 256 * 3] = len(v)                               # ... a whole cluster of them: it has no valid triangle
    out["indices-out-of-range"] = (v, bad)
    nf = v.copy()
    nf["position"][len(v) // 2] = (np.nan, 0.0, np.inf)                  # a position that is not finite: its clusters, and the blocks they touch
    nf["position"][3] = (0.0, -np.inf, 0.0)
    out["not-finite"] = (nf, i)
    extra = np.concatenate([v, v[:600]])                                 # 600 vertices behind the mesh that no triangle uses: two whole blocks
    out["unused-blocks"] = (extra, i)
    out["no-indices"] = (v, i[:0])
    out["one-triangle"] = (v[:3], np.uint32([0, 1, 2]))
    return out


def test_tables_are_their_definition(pkg, R, meshes):
    """both tables, bit for bit, against the numpy restatement (tests/cluster_cull_cases.py), on every mesh and every edge"""
    everything = dict(meshes)
    everything.update(_edge_meshes(pkg.scenes))
    for name, (v, i) in everything.items():
        tb, vb = R.cluster_bounds(v, i)
        assert tb.shape == ((len(i) // 3 + 255) // 256, 6) and vb.shape == ((len(v) + 255) // 256, 6), name
        _same_bits(tb, CC.cluster_boxes(v, i))
        _same_bits(vb, CC.block_boxes(v, i, "clusters"))


def test_edges_are_what_the_header_says(pkg, R):
    E = _edge_meshes(pkg.scenes)
    inf = lambda box: bool((box == CC.INF_BOX).all())
    tb, vb = R.cluster_bounds(*E["ragged"])
    assert len(tb) == 4 and np.isfinite(tb).all()
    used = np.unique(E["ragged"][1] // 256)
    assert len(used) < len(vb)                                           # blocks no triangle uses ...
    assert all(inf(vb[b]) != (b in used) for b in range(len(vb)))        # ... are infinite, the others bounded
    tb, vb = R.cluster_bounds(*E["indices-out-of-range"])
    assert inf(tb[2]) and not inf(tb[0]) and not inf(tb[1]) and np.isfinite(tb[[0, 1, 3]]).all()
    tb, vb = R.cluster_bounds(*E["not-finite"])
    v, i = E["not-finite"]
    hit = np.unique(np.nonzero((~np.isfinite(v["position"][i.reshape(-1, 3)])).any((1, 2)))[0] // 256)
    assert len(hit) >= 2 and all(inf(tb[c]) for c in hit) and not all(inf(b) for b in tb)
    for c, b in CC.uses(v, i):                                           # "cannot bound" carries over: a block that touches such a cluster
        if c in hit:
            assert inf(vb[b])
    assert not np.isnan(tb).any() and not np.isnan(vb).any()
    tb, vb = R.cluster_bounds(*E["unused-blocks"])
    assert len(vb) == 9 and inf(vb[7]) and inf(vb[8]) and np.isfinite(vb[:6]).all()
    tb, vb = R.cluster_bounds(*E["no-indices"])
    assert tb.shape == (0, 6) and len(vb) == 7 and all(inf(b) for b in vb)
    tb, vb = R.cluster_bounds(*E["one-triangle"])
    _same_bits(tb, vb)


def test_refusals(pkg, R):
    import ctypes as C
    L = pkg.binding.lib()
    v, i = CC.small_quad(pkg.scenes)
    v = np.ascontiguousarray(v); i = np.ascontiguousarray(i, np.uint32)
    tb, vb = np.full((5, 6), 7.0, np.float32), np.full((3, 6), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    call = L.arctic_cluster_bounds
    assert call(p(v), len(v), p(i), len(i), p(tb), p(vb)) == 0
    good = (tb.copy(), vb.copy())
    tb[:], vb[:] = 7.0, 7.0
    for args in ((None, len(v), p(i), len(i), p(tb), p(vb)), (p(v), len(v), None, len(i), p(tb), p(vb)), (p(v), len(v), p(i), len(i) - 1, p(tb), p(vb)),
                 (p(v), len(v), p(i), len(i), None, p(vb)), (p(v), len(v), p(i), len(i), p(tb), None)):
        assert call(*args) == -1, args                                   # ARCTIC_E_INVALID
    for args in ((p(v), 1 << 31, p(i), len(i), p(tb), p(vb)), (p(v), len(v), p(i), 0xFFFFFFF0 + 3, p(tb), p(vb))):
        assert call(*args) == -5, args                                   # ARCTIC_E_CAPACITY, before anything is read
    assert (tb == 7.0).all() and (vb == 7.0).all()                       # a refused call writes nothing
    assert call(None, 0, None, 0, None, None) == 0                       # no vertices, no triangles: no tables
    assert call(p(v), len(v), None, 0, None, p(vb)) == 0 and (vb == CC.INF_BOX).all()
    _same_bits(good[0], R.cluster_bounds(v, i)[0])
    with pytest.raises(R.ArcticError):
        R.cluster_bounds(v, i[:-1])


def test_a_block_contains_its_clusters(pkg, R, meshes):
    """for every valid triangle and each block it touches, vbounds[b] contains tbounds[t // 256], component by component"""
    everything = dict(meshes)
    everything.update(_edge_meshes(pkg.scenes))
    pairs = 0
    for name, (v, i) in everything.items():
        tb, vb = R.cluster_bounds(v, i)
        assert CC.violations(tb, vb, v, i) == [], name
        pairs += len(CC.uses(v, i))
    assert pairs > 1000


def test_the_meshes_tell_the_rules_apart(pkg, R, meshes):
    """the rule the library had (a block's box = the union of its triangles' boxes) breaks the property on the 24 x 24 quad -- ADVICE.md's
    triangle 768, of cluster 3, reads vertices of block 1 alone, whose box then ends below the cluster's -- and on every permuted mesh of more than
    256 triangles"""
    v, i = meshes["quad24"]
    tb, _ = R.cluster_bounds(v, i)
    old = CC.block_boxes(v, i, "triangles")
    assert (i.reshape(-1, 3)[768] // 256 == 1).all()
    assert (3, 1) in CC.violations(tb, old, v, i)
    assert not CC.contains(old[1], tb[3]) and CC.contains(R.cluster_bounds(v, i)[1][1], tb[3])
    seen = 0
    for name, (v, i) in meshes.items():
        if name.endswith("-permuted") and len(i) // 3 > 256:
            tb, vb = R.cluster_bounds(v, i)
            bad = CC.violations(tb, CC.block_boxes(v, i, "triangles"), v, i)
            print(f"{name}: {len(i) // 3} triangles, {len(vb)} blocks: the old rule breaks {len(bad)} of {len(CC.uses(v, i))} (cluster, block) pairs")
            assert bad, name
            seen += 1
    assert seen >= 20


# ---- the GPU scenarios are not vacuous -----------------------------------------------------------------------------------------------
def _scenarios(pkg, R, config3):
    """name -> (meshes, [(objects, clip_from_world, vp_w, vp_h, scissor)] per step): the exact sequences of tests/test_gpu_cluster_cull.py"""
    S = pkg.scenes
    out = {}
    for tag, perm in (("as generated", False), ("permuted", True)):
        quad = [CC.big_quad(S)]
        quad = CC.permuted_meshes(quad) if perm else quad
        steps = []
        for cam in CC.QUAD_CAMERAS:
            desc = CC.quad_desc(S, cam)
            steps.append((desc.objects, R.frame_constants(desc)[0].ravel(), CC.QUAD_W, CC.QUAD_H, (0, 0, CC.QUAD_W, CC.QUAD_H)))
        out[f"quad, {tag}"] = (quad, steps)
        sc = CC.permuted_scene(config3) if perm else config3
        steps = []
        for rot in CC.FRAME_ROTATIONS:
            desc = CC.with_camera_rotation(sc.desc, rot)
            steps.append((desc.objects, R.frame_constants(desc)[0].ravel(), sc.width, sc.height, (0, 0, sc.width, sc.height)))
        out[f"frames, {tag}"] = (sc.meshes, steps)
        steps = []
        for rot in CC.SUN_ROTATIONS:
            desc = CC.with_sun_rotation(sc.desc, rot)
            n = sc.shadow_size
            steps.append((desc.objects, R.frame_constants(desc)[1].ravel(), n, n, (0, 0, n, n)))
        out[f"sun, {tag}"] = (sc.meshes, steps)
    return out


def test_the_gpu_scenarios_are_not_vacuous(pkg, R, config3):
    """box_outside in float64 with the kernel's E, margins and strict, the matrices of arctic_frame_constants, depth and facing ignored: under the
    old rule every sequence has triangles of kept clusters that read skipped vertex blocks (at least 50 as generated, 1000 permuted); with the
    library's own tables none, at any step"""
    assert np.array_equal(np.float32(config3.desc.camera["rotation"]), np.float32(CC.FRAME_ROTATIONS[0]))
    assert np.array_equal(np.float32(config3.desc.sun["rotation"]), np.float32(CC.SUN_ROTATIONS[0]))
    for name, (meshes, steps) in _scenarios(pkg, R, config3).items():
        new = [R.cluster_bounds(v, i) for v, i, *_ in meshes]
        old = [(tb, CC.block_boxes(v, i, "triangles")) for (tb, _), (v, i, *_) in zip(new, meshes)]
        total = 0
        for k, (objects, m, w, h, scissor) in enumerate(steps):
            n_b, skipped_old, holes_old = CC.holes(meshes, objects, m, w, h, scissor, old)
            _, skipped_new, holes_new = CC.holes(meshes, objects, m, w, h, scissor, new)
            print(f"{name}, step {k}: {n_b} blocks; old rule skips {skipped_old} with {holes_old} holes; clusters rule skips {skipped_new} with {holes_new} holes")
            assert holes_new == 0, (name, k)
            total += holes_old
        assert total >= (1000 if "permuted" in name else 50), (name, total)


def test_a_box_through_the_eye_plane(pkg, R):
    """one box, as a block (strict = 2) and as a cluster (strict = 1): with the same side planes for both, as the kernel has them, `block outside`
    implies `cluster outside` at every camera of the sweep; with the sides `strict` pixels out, as it had them, the sweep crosses cameras at which
    the block is skipped and the cluster kept (tests/test_gpu_cluster_cull.py renders them)"""
    S = pkg.scenes
    v, i = CC.wall(S)
    tb, vb = R.cluster_bounds(v, i)
    assert tb.shape == vb.shape == (1, 6) and (tb == vb).all()
    size = (CC.QUAD_W, CC.QUAD_H, (0, 0, CC.QUAD_W, CC.QUAD_H))
    states = {1.0: [], None: []}
    for rot in CC.WALL_SWEEP:
        desc = CC.quad_desc(S, CC.wall_camera(rot))
        m = R.frame_constants(desc)[0].ravel()
        for px in states:
            block = bool(CC.box_outside(vb, desc.objects[0]["trs"], m, *size, 2.0, side_pixels=2.0 if px is None else px)[0])
            cluster = bool(CC.box_outside(tb, desc.objects[0]["trs"], m, *size, 1.0, side_pixels=1.0)[0])
            states[px].append((block, cluster))
    print("sides 2 px for the block:", "".join("X" if b and not c else "s" if b else "." for b, c in states[None]))
    print("sides 1 px for both:     ", "".join("X" if b and not c else "s" if b else "." for b, c in states[1.0]))
    assert sum(b and not c for b, c in states[None]) >= 5
    assert not any(b and not c for b, c in states[1.0])
    assert any(b and c for b, c in states[1.0]) and any(not b and not c for b, c in states[1.0])      # the sweep crosses the planes
    desc = CC.quad_desc(S, CC.wall_camera(CC.WALL_VISIBLE))
    assert not CC.box_outside(tb, desc.objects[0]["trs"], R.frame_constants(desc)[0].ravel(), *size, 1.0)[0]
