"""The scene-loader stand-in (include/arctic_gltf.h) against glTF files this test writes itself: the real
SciFiHelmet / FlightHelmet / Sponza assets and assimp are not available offline, so what is checked is the restated
behaviour of App::load_scene (reference src/app.cpp:173-385, 540-564) -- parity with assimp's own output is unpinned."""
import base64
import json
import os
import struct
import zlib

import numpy as np
import pytest


def png_bytes(img, color_type=6, depth=8, palette=None, filters=(0, 1, 2, 3, 4)):
    """minimal PNG writer (all five filter types in rotation) for (h, w, C) uint8/uint16 arrays."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    bpp = max(1, img.shape[2] * depth // 8) if img.ndim == 3 else max(1, depth // 8)
    rows = []
    prev = np.zeros(0, np.uint8)
    for y in range(h):
        if depth == 16:
            line = img[y].astype(">u2").tobytes()
        elif depth == 8:
            line = img[y].astype(np.uint8).tobytes()
        else:   # packed 1/2/4 bit samples, one channel
            vals = img[y].reshape(-1).astype(np.uint8)
            per = 8 // depth
            vals = np.concatenate([vals, np.zeros((-len(vals)) % per, np.uint8)]).reshape(-1, per)
            line = bytes(int(sum(int(v) << (8 - depth * (k + 1)) for k, v in enumerate(r))) for r in vals)
        cur = np.frombuffer(line, np.uint8).astype(np.int32)
        pr = prev.astype(np.int32) if len(prev) else np.zeros_like(cur)
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if len(cur) > bpp else np.zeros_like(cur)
        c = np.concatenate([np.zeros(bpp, np.int32), pr[:-bpp]]) if len(cur) > bpp else np.zeros_like(cur)
        ft = filters[y % len(filters)]
        if ft == 0: f = cur
        elif ft == 1: f = cur - a
        elif ft == 2: f = cur - pr
        elif ft == 3: f = cur - ((a + pr) >> 1)
        else:
            pa, pb, pc = np.abs(pr - c), np.abs(a - c), np.abs(a + pr - 2 * c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, pr, c))
            f = cur - pred
        rows.append(bytes([ft]) + (f & 255).astype(np.uint8).tobytes())
        prev = cur.astype(np.uint8)

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))
    raw = zlib.compress(b"".join(rows), 6)
    mid = len(raw) // 2
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, 0))
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    return out + chunk(b"IDAT", raw[:mid]) + chunk(b"IDAT", raw[mid:]) + chunk(b"IEND", b"")   # two IDAT chunks on purpose


@pytest.fixture(scope="module")
def gltf(pkg):
    from importlib import import_module
    m = import_module("arctic_renderer_amd.gltf")
    m.build()
    return m


def test_png_decoder(gltf):
    rng = np.random.default_rng(3)
    rgba = rng.integers(0, 256, (13, 17, 4), dtype=np.uint8)
    np.testing.assert_array_equal(gltf.png_decode(png_bytes(rgba, 6)), rgba)
    rgb = rng.integers(0, 256, (9, 31, 3), dtype=np.uint8)
    out = gltf.png_decode(png_bytes(rgb, 2))
    np.testing.assert_array_equal(out[..., :3], rgb); assert (out[..., 3] == 255).all()
    grey = rng.integers(0, 256, (8, 8, 1), dtype=np.uint8)
    out = gltf.png_decode(png_bytes(grey, 0))
    np.testing.assert_array_equal(out[..., 0], grey[..., 0]); np.testing.assert_array_equal(out[..., 1], out[..., 2])
    ga = rng.integers(0, 256, (5, 7, 2), dtype=np.uint8)
    out = gltf.png_decode(png_bytes(ga, 4))
    np.testing.assert_array_equal(out[..., 0], ga[..., 0]); np.testing.assert_array_equal(out[..., 3], ga[..., 1])
    rgb16 = rng.integers(0, 65536, (6, 5, 3), dtype=np.uint16)
    np.testing.assert_array_equal(gltf.png_decode(png_bytes(rgb16, 2, depth=16))[..., :3], (rgb16 >> 8).astype(np.uint8))   # stb keeps the high byte
    pal = rng.integers(0, 256, (16, 3), dtype=np.uint8)
    idx = rng.integers(0, 16, (7, 9, 1), dtype=np.uint8)
    np.testing.assert_array_equal(gltf.png_decode(png_bytes(idx, 3, depth=4, palette=pal))[..., :3], pal[idx[..., 0]])
    bits = rng.integers(0, 2, (5, 19, 1), dtype=np.uint8)
    np.testing.assert_array_equal(gltf.png_decode(png_bytes(bits, 0, depth=1))[..., 0], bits[..., 0] * 255)
    with pytest.raises(ValueError):
        gltf.png_decode(b"\xff\xd8\xff\xe0 not a png")
    for name, want in (("white.png", (255, 255, 255)), ("normal.png", (128, 128, 255))):   # the reference's fallback textures (16 x 16, 4-bit palette)
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)
        img = gltf.png_decode(open(path, "rb").read())
        assert (img[..., :3] == want).all() and img.shape[2] == 4


def write_scene(tmp, embed=False):
    rng = np.random.default_rng(11)
    # mesh 0: two primitives (a quad with indices + TANGENT, a lone triangle without tangents, u16 / u8 indices); mesh 1: quad, no indices
    quad_p = np.array([(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)], np.float32)
    quad_n = np.tile(np.float32([0, 0, 1]), (4, 1))
    quad_uv = np.array([(0, 1), (1, 1), (1, 0), (0, 0)], np.float32)          # glTF convention: v down
    quad_t = np.tile(np.float32([1, 0, 0, -1]), (4, 1))                       # handedness -1
    quad_i = np.array([0, 1, 2, 0, 2, 3], np.uint16)
    tri_p = np.array([(0, 0, 0), (2, 0, 0), (0, 0, -2)], np.float32)
    tri_n = np.tile(np.float32([0, 1, 0]), (3, 1))
    tri_uv = np.array([(0.25, 0.75), (0.75, 0.75), (0.25, 0.25)], np.float32)
    tri_i = np.array([0, 1, 2], np.uint8)
    soup_p = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], np.float32)
    soup_n = np.tile(np.float32([0, 0, 1]), (6, 1))
    soup_uv = soup_p[:, :2].copy()
    blobs, views, accessors = [], [], []

    def add(arr, type_, ctype, target=None, stride=None):
        data = arr.tobytes()
        if stride:   # interleave with padding to exercise byteStride
            rec = arr.reshape(len(arr), -1)
            data = b"".join(r.tobytes() + b"\0" * (stride - r.nbytes) for r in rec)
        off = sum(len(b) for b in blobs)
        pad = (-off) % 4
        blobs.append(b"\0" * pad + data)
        v = {"buffer": 0, "byteOffset": off + pad, "byteLength": len(data)}
        if stride: v["byteStride"] = stride
        views.append(v)
        accessors.append({"bufferView": len(views) - 1, "componentType": ctype, "count": len(arr), "type": type_})
        return len(accessors) - 1
    a = {k: add(*v) for k, v in dict(qp=(quad_p, "VEC3", 5126, None, 16), qn=(quad_n, "VEC3", 5126), quv=(quad_uv, "VEC2", 5126), qt=(quad_t, "VEC4", 5126),
                                     qi=(quad_i, "SCALAR", 5123), tp=(tri_p, "VEC3", 5126), tn=(tri_n, "VEC3", 5126), tuv=(tri_uv, "VEC2", 5126),
                                     ti=(tri_i, "SCALAR", 5121), sp=(soup_p, "VEC3", 5126), sn=(soup_n, "VEC3", 5126), suv=(soup_uv, "VEC2", 5126)).items()}
    binary = b"".join(blobs)
    imgs = {"base.png": rng.integers(0, 256, (8, 8, 4), dtype=np.uint8), "nrm.png": rng.integers(0, 256, (4, 16, 3), dtype=np.uint8),
            "mr.png": rng.integers(0, 256, (16, 4, 3), dtype=np.uint8)}
    for name, im in imgs.items():
        open(os.path.join(tmp, name), "wb").write(png_bytes(im, 6 if im.shape[2] == 4 else 2))
    doc = {
        "asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0, 3]}],
        "nodes": [
            {"name": "a", "children": [1, 2], "translation": [1.0, 2.0, 3.0]},
            {"name": "b", "mesh": 0, "rotation": [0.0, 0.7071068, 0.0, 0.7071068], "scale": [2.0, 1.0, 0.5]},
            {"name": "c", "mesh": 1, "matrix": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, -4, 5, 6, 1]},
            {"name": "d", "mesh": 1},
        ],
        "meshes": [
            {"primitives": [{"attributes": {"POSITION": a["qp"], "NORMAL": a["qn"], "TEXCOORD_0": a["quv"], "TANGENT": a["qt"]}, "indices": a["qi"], "material": 0},
                            {"attributes": {"POSITION": a["tp"], "NORMAL": a["tn"], "TEXCOORD_0": a["tuv"]}, "indices": a["ti"], "material": 1}]},
            {"primitives": [{"attributes": {"POSITION": a["sp"], "NORMAL": a["sn"], "TEXCOORD_0": a["suv"]}, "material": 1}]},
        ],
        "materials": [
            {"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicRoughnessTexture": {"index": 2}}, "normalTexture": {"index": 1}},
            {"pbrMetallicRoughness": {"baseColorTexture": {"index": 0}}},     # normal + metal-rough fall back
        ],
        "textures": [{"source": 0}, {"source": 1}, {"source": 2}],
        "images": [{"uri": "base.png"}, {"uri": "nrm.png"}, {"uri": "mr%2Epng"}],
        "buffers": [{"byteLength": len(binary), "uri": "data:application/octet-stream;base64," + base64.b64encode(binary).decode() if embed else "scene.bin"}],
        "bufferViews": views, "accessors": accessors,
    }
    if not embed:
        open(os.path.join(tmp, "scene.bin"), "wb").write(binary)
    path = os.path.join(tmp, "embedded.gltf" if embed else "scene.gltf")
    json.dump(doc, open(path, "w"))
    return path, imgs, dict(quad_p=quad_p, quad_uv=quad_uv, quad_i=quad_i, tri_p=tri_p, tri_uv=tri_uv, soup_p=soup_p)


@pytest.mark.parametrize("embed", [False, True], ids=["external-bin", "base64"])
def test_load_scene_conventions(gltf, tmp_path, embed):
    path, imgs, geo = write_scene(str(tmp_path), embed)
    sc = gltf.load(path)
    # ---- materials: three RGBA8 images each, fallbacks for missing ones (app.cpp:195-294)
    assert len(sc.materials) == 2
    np.testing.assert_array_equal(sc.materials[0][0], imgs["base.png"])
    np.testing.assert_array_equal(sc.materials[0][1][..., :3], imgs["nrm.png"]); assert (sc.materials[0][1][..., 3] == 255).all()
    np.testing.assert_array_equal(sc.materials[0][2][..., :3], imgs["mr.png"])
    assert (sc.materials[1][1][..., :3] == (128, 128, 255)).all() and (sc.materials[1][2] == 255).all()
    # ---- meshes: one per primitive, FlipUVs, tangents (app.cpp:296-352)
    assert [m[2] for m in sc.meshes] == [0, 1, 1] and [len(m[1]) for m in sc.meshes] == [6, 3, 6]
    v, ix, _ = sc.meshes[0]
    np.testing.assert_array_equal(v["position"], geo["quad_p"])
    np.testing.assert_array_equal(v["tex_coords"], np.stack([geo["quad_uv"][:, 0], 1 - geo["quad_uv"][:, 1]], -1))
    np.testing.assert_array_equal(ix, geo["quad_i"].astype(np.uint32))
    np.testing.assert_array_equal(v["tangent"], np.tile(np.float32([1, 0, 0]), (4, 1)))
    np.testing.assert_array_equal(v["bitangent"], np.tile(np.float32([0, -1, 0]), (4, 1)))     # cross(n, t) * w = (0,1,0) * -1
    v, ix, _ = sc.meshes[1]   # no TANGENT: from the UV gradients of the FLIPPED uvs, orthonormal to the normal
    uvf = np.stack([geo["tri_uv"][:, 0], 1 - geo["tri_uv"][:, 1]], -1)
    np.testing.assert_array_equal(v["tex_coords"], uvf.astype(np.float32))
    e1, e2 = geo["tri_p"][1] - geo["tri_p"][0], geo["tri_p"][2] - geo["tri_p"][0]
    d1, d2 = uvf[1] - uvf[0], uvf[2] - uvf[0]
    det = d1[0] * d2[1] - d2[0] * d1[1]
    t_ref = (e1 * d2[1] - e2 * d1[1]) / det          # dP/du
    b_ref = (e2 * d1[0] - e1 * d2[0]) / det          # dP/dv
    for k in range(3):
        assert abs(np.dot(v["tangent"][k], v["normal"][k])) < 1e-6 and abs(np.linalg.norm(v["tangent"][k]) - 1) < 1e-6
        # assimp's dirCorrection flips BOTH vectors when the UV winding is mirrored: they are +-(dP/du, dP/dv) together
        s = np.sign(np.dot(v["tangent"][k], t_ref))
        np.testing.assert_allclose(v["tangent"][k], s * t_ref / np.linalg.norm(t_ref), atol=1e-6)
        np.testing.assert_allclose(v["bitangent"][k], s * b_ref / np.linalg.norm(b_ref), atol=1e-6)
    v, ix, _ = sc.meshes[2]   # no index accessor: 0..n-1
    np.testing.assert_array_equal(ix, np.arange(6, dtype=np.uint32))
    # ---- objects: stack order (children last-to-first), one per primitive, matrices through assimp_to_mat4 (transposed) as parent * child
    def local(n):
        if "matrix" in n:
            return np.float32(n["matrix"]).reshape(4, 4).T          # math matrix from the column-major array
        m = np.eye(4, dtype=np.float32)
        x, y, z, w = np.float32(n.get("rotation", [0, 0, 0, 1]))
        r = np.float32([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        m[:3, :3] = r * np.float32(n.get("scale", [1, 1, 1]))[None, :]
        m[:3, 3] = np.float32(n.get("translation", [0, 0, 0]))
        return m
    nodes = json.load(open(path))["nodes"]
    A, B, Cn = local(nodes[0]), local(nodes[1]), local(nodes[2])
    # two scene roots -> synthetic identity root; pop order: d (pushed last), then a; a's children: c popped before b
    want = [(np.eye(4, dtype=np.float32), 2), (A.T @ Cn.T, 2), (A.T @ B.T, 0), (A.T @ B.T, 1)]
    assert len(sc.objects) == len(want)
    for o, (m, mesh) in zip(sc.objects, want):
        assert int(o["mesh_idx"]) == mesh
        np.testing.assert_allclose(o["trs"].reshape(4, 4).T, m, atol=1e-6)      # trs is glm memory order (column-major)
    # the quirk, spelled out: a pure translation ends up in the bottom ROW of the math matrix, not in its last column
    assert np.allclose(sc.objects[1]["trs"].reshape(4, 4).T[3, :3], [1 - 4, 2 + 5, 3 + 6]) and np.allclose(sc.objects[1]["trs"].reshape(4, 4).T[:3, 3], 0)


def test_glb_container(gltf, tmp_path):
    """the binary container: JSON chunk + BIN chunk (buffer 0 without uri), images through bufferViews."""
    path, imgs, geo = write_scene(str(tmp_path))
    doc = json.load(open(path))
    binary = open(os.path.join(str(tmp_path), "scene.bin"), "rb").read()
    binary += b"\0" * ((-len(binary)) % 4)
    for k, name in enumerate(("base.png", "nrm.png", "mr.png")):       # move the images into the BIN chunk
        data = open(os.path.join(str(tmp_path), name), "rb").read()
        doc["bufferViews"].append({"buffer": 0, "byteOffset": len(binary), "byteLength": len(data)})
        doc["images"][k] = {"bufferView": len(doc["bufferViews"]) - 1, "mimeType": "image/png"}
        binary += data + b"\0" * ((-len(data)) % 4)
    doc["buffers"] = [{"byteLength": len(binary)}]
    js = json.dumps(doc).encode()
    js += b" " * ((-len(js)) % 4)
    glb = tmp_path / "scene.glb"
    glb.write_bytes(b"glTF" + struct.pack("<II", 2, 12 + 8 + len(js) + 8 + len(binary)) + struct.pack("<I", len(js)) + b"JSON" + js +
                    struct.pack("<I", len(binary)) + b"BIN\0" + binary)
    a, b = gltf.load(path), gltf.load(str(glb))
    assert len(a.materials) == len(b.materials) and len(a.meshes) == len(b.meshes)
    for ma, mb in zip(a.materials, b.materials):
        for x, y in zip(ma, mb):
            np.testing.assert_array_equal(x, y)
    for (va, ia, ka), (vb, ib, kb) in zip(a.meshes, b.meshes):
        assert va.tobytes() == vb.tobytes() and ia.tobytes() == ib.tobytes() and ka == kb
    assert a.objects.tobytes() == b.objects.tobytes()


def test_errors(gltf, tmp_path):
    with pytest.raises(ValueError, match="cannot open"):
        gltf.load(str(tmp_path / "missing.gltf"))
    p = tmp_path / "bad.gltf"
    p.write_text("{ not json")
    with pytest.raises(ValueError):
        gltf.load(str(p))
    p = tmp_path / "broken.glb"
    p.write_bytes(b"glTF\x02\x00\x00\x00\x10\x00\x00\x00")
    with pytest.raises(ValueError, match="glb"):
        gltf.load(str(p))
    path, _, _ = write_scene(str(tmp_path))
    doc = json.load(open(path))
    doc["images"][0]["uri"] = "photo.webp"
    (tmp_path / "photo.webp").write_bytes(b"RIFF\0\0\0\0WEBPVP8 " + b"\0" * 32)
    json.dump(doc, open(path, "w"))
    with pytest.raises(ValueError, match="PNG or baseline JPEG"):
        gltf.load(path)


def test_loaded_scene_renders_on_the_oracle(gltf, oracle, pkg, tmp_path):
    """end to end on the CPU: the loader's output drives the Renderer surface like App::load_scene does."""
    path, _, _ = write_scene(str(tmp_path))
    sc = gltf.load(path)
    o = sc.upload(oracle.Oracle(96, 64, 0, 16))
    # identity transforms for the picture (the transposed translations of the test scene distort it, as in the reference)
    objs = sc.objects.copy()
    objs["trs"] = np.eye(4, dtype=np.float32).reshape(16)
    desc = pkg.scene.SceneDesc(camera=dict(eye=(0.3, 0.4, 4.0), rotation=(0.0, -90.0), aspect=1.5, fov_y=60.0, z_near_far=(0.1, 100.0)),
                               ambient=0.2, sun=dict(position=(2, 10, 6), rotation=(-55.0, -110.0), color=(8, 8, 8)), objects=objs)
    img = o.render_frame(desc, (0, 2.2, 1.0))
    assert (img[..., :3].sum(-1) > 0).mean() > 0.1


@pytest.mark.gpu
def test_loaded_scene_renders_on_the_gpu_like_on_the_oracle(gltf, oracle, hip, pkg, tmp_path):
    """load_scene's replacement end to end: arctic_gltf_upload feeds the HIP renderer through the C-ABI; the frame matches
    the oracle fed with the same loader output."""
    import ctypes as C
    path, _, _ = write_scene(str(tmp_path))
    sc = gltf.load(path)
    objs = sc.objects.copy()
    objs["trs"] = np.eye(4, dtype=np.float32).reshape(16)
    desc = pkg.scene.SceneDesc(camera=dict(eye=(0.3, 0.4, 4.0), rotation=(0.0, -90.0), aspect=1.5, fov_y=60.0, z_near_far=(0.1, 100.0)),
                               ambient=0.2, sun=dict(position=(2, 10, 6), rotation=(-55.0, -110.0), color=(8, 8, 8)), objects=objs,
                               point_lights=pkg.scene.make_lights([(0.5, 0.5, 2.0)], [(3.0, 2.0, 1.0)]))
    o = sc.upload(oracle.Oracle(192, 128, 256, 16))
    o.update_lights(desc.point_lights)
    ref = o.render_frame(desc, (2, 2.2, 1.0))
    r = hip.Renderer(192, 128, 256, 16)
    L = gltf.lib()
    err = C.create_string_buffer(256)
    h = L.arctic_gltf_load(os.fsencode(path), err, 256)
    assert h and L.arctic_gltf_upload(h, r.h) == 0            # the C entry point a C++ host would call
    L.arctic_gltf_free(h)
    r.update_lights(desc.point_lights)
    img = r.render_frame(desc, (2, 2.2, 1.0))
    d = np.abs(img.astype(np.int16) - ref.astype(np.int16))
    assert d.max() <= 1 and (d != 0).mean() < 2e-3 and (img[..., :3].sum(-1) > 0).mean() > 0.1
    r.close(); o.close()


def test_library_exports_every_symbol_of_its_header(gltf):
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "arctic_gltf.h")).read()
    names = set(re.findall(r"\b(arctic_(?:gltf|png)_\w+)\s*\(", text))
    assert len(names) >= 10
    L = gltf.lib()
    for n in names:
        assert hasattr(L, n), n


# ------------------------------------------------------------------------------------------- baseline JPEG
ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
DCT = np.array([[(np.sqrt(0.5) if u == 0 else 1.0) * 0.5 * np.cos((2 * x + 1) * u * np.pi / 16) for u in range(8)] for x in range(8)])   # [x][u]


def jpeg_bytes(rgb, sub=(1, 1), quant=4, restart=0):
    """minimal baseline JPEG writer for the test: fixed-length Huffman codes (any prefix code is legal), one interleaved
    scan, luma sampled (sub x sub... ) relative to chroma.  Returns (bytes, reference decode) where the reference is the
    textbook decoder arithmetic in float64."""
    h, w = rgb.shape[:2]
    hs, vs = sub
    r, g, b = [rgb[..., k].astype(np.float64) for k in range(3)]
    ycc = [0.299 * r + 0.587 * g + 0.114 * b, -0.168736 * r - 0.331264 * g + 0.5 * b + 128, 0.5 * r - 0.418688 * g - 0.081312 * b + 128]
    mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
    planes = []
    for c, p in enumerate(ycc):
        fh, fv = (hs, vs) if c == 0 else (1, 1)
        full = np.pad(p, ((0, mh * 8 * vs - h), (0, mw * 8 * hs - w)), mode="edge")
        if c:   # chroma: average the hs x vs block
            full = full.reshape(mh * 8, vs, mw * 8, hs).mean((1, 3))
        planes.append(full)
    q = np.full(64, quant, np.int64)
    ac_syms = [0x00, 0xF0] + [(run << 4) | size for run in range(16) for size in range(1, 11)]
    ac_code = {s: i for i, s in enumerate(ac_syms)}          # 8-bit codes 0..161
    bits = []

    def put(v, n):
        for k in range(n - 1, -1, -1):
            bits.append((v >> k) & 1)

    def amp(v):
        if v == 0:
            return 0, 0
        n = int(abs(v)).bit_length()
        return n, (v if v > 0 else v + (1 << n) - 1)
    coeffs = [np.zeros((p.shape[0] // 8, p.shape[1] // 8, 64), np.int64) for p in planes]
    for c, p in enumerate(planes):
        for by in range(p.shape[0] // 8):
            for bx in range(p.shape[1] // 8):
                blk = p[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] - 128.0
                f = DCT.T @ blk @ DCT                                    # F[v][u]
                coeffs[c][by, bx] = np.rint(f.reshape(64) / q).astype(np.int64)
    pred = [0, 0, 0]
    out = bytearray()
    count = 0

    def flush():
        nonlocal bits
        while len(bits) % 8:
            bits.append(1)
        by = np.packbits(np.array(bits, np.uint8)).tobytes() if bits else b""
        for v in by:
            out.append(v)
            if v == 0xFF:
                out.append(0)
        bits = []
    for my in range(mh):
        for mx in range(mw):
            if restart and count and count % restart == 0:
                flush()
                out.extend(bytes([0xFF, 0xD0 + ((count // restart - 1) % 8)]))
                pred = [0, 0, 0]
            for c in range(3):
                fh, fv = (hs, vs) if c == 0 else (1, 1)
                for by in range(fv):
                    for bx in range(fh):
                        z = coeffs[c][my * fv + by, mx * fh + bx][ZZ]
                        n, a = amp(int(z[0]) - pred[c]); pred[c] = int(z[0])
                        put(n, 4); put(a, n)
                        run = 0
                        last = max([k for k in range(1, 64) if z[k] != 0], default=0)
                        for k in range(1, last + 1):
                            if z[k] == 0:
                                run += 1
                                if run == 16:
                                    put(ac_code[0xF0], 8); run = 0
                                continue
                            n, a = amp(int(z[k]))
                            put(ac_code[(run << 4) | n], 8); put(a, n); run = 0
                        if last < 63:
                            put(ac_code[0x00], 8)
            count += 1
    flush()

    def seg(m, body):
        return bytes([0xFF, m]) + struct.pack(">H", len(body) + 2) + body
    dht_dc = bytes([0x00]) + bytes([0, 0, 0, 12] + [0] * 12) + bytes(range(12))
    dht_ac = bytes([0x10]) + bytes([0] * 7 + [len(ac_syms)] + [0] * 8) + bytes(ac_syms)
    sof = struct.pack(">BHHB", 8, h, w, 3) + bytes([1, (hs << 4) | vs, 0, 2, 0x11, 0, 3, 0x11, 0])
    sos = bytes([3, 1, 0x00, 2, 0x00, 3, 0x00, 0, 63, 0])
    data = (b"\xff\xd8" + seg(0xE0, b"JFIF\0\1\1\0\0\1\0\1\0\0") + seg(0xDB, bytes([0]) + bytes([quant] * 64)) + seg(0xC0, sof) + seg(0xC4, dht_dc) + seg(0xC4, dht_ac)
            + (seg(0xDD, struct.pack(">H", restart)) if restart else b"") + seg(0xDA, sos) + bytes(out) + b"\xff\xd9")
    # reference decode (float64): dequantise, IDCT, +128, round, clamp; chroma replicated; JFIF conversion
    rec = []
    for c, p in enumerate(planes):
        o = np.zeros_like(p)
        for by in range(p.shape[0] // 8):
            for bx in range(p.shape[1] // 8):
                f = (coeffs[c][by, bx] * q).reshape(8, 8).astype(np.float64)
                o[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = DCT @ f @ DCT.T
        o = np.clip(np.rint(o + 128), 0, 255)
        if c:
            o = np.repeat(np.repeat(o, vs, 0), hs, 1)
        rec.append(o[:h, :w])
    Y, cb, cr = rec[0], rec[1] - 128, rec[2] - 128
    ref = np.stack([Y + 1.402 * cr, Y - 0.344136 * cb - 0.714136 * cr, Y + 1.772 * cb], -1)
    return data, np.clip(np.rint(ref), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("sub,restart,size", [((1, 1), 0, (24, 40)), ((2, 2), 0, (37, 53)), ((2, 1), 3, (16, 48)), ((2, 2), 2, (50, 33))],
                         ids=["444", "420-ragged", "422-restart", "420-restart-ragged"])
def test_baseline_jpeg_decoder(gltf, sub, restart, size):
    rng = np.random.default_rng(sum(size) + restart)
    h, w = size
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([127 + 100 * np.sin(xx / 7.0 + yy / 11.0), 127 + 90 * np.cos(xx / 5.0), 40 + 3.0 * yy + 20 * rng.random((h, w))], -1)
    img = np.clip(img, 0, 255).astype(np.uint8)
    data, ref = jpeg_bytes(img, sub=sub, quant=3, restart=restart)
    out = gltf.png_decode(data)                      # the image entry point picks the decoder by signature
    assert out.shape == (h, w, 4) and (out[..., 3] == 255).all()
    d = np.abs(out[..., :3].astype(np.int16) - ref.astype(np.int16))
    assert d.max() <= 1 and (d != 0).mean() < 0.02, (d.max(), (d != 0).mean())     # float32 vs float64 rounding
    assert np.abs(out[..., :3].astype(np.int16) - img.astype(np.int16)).mean() < 6  # and it is the picture that went in
    with pytest.raises(ValueError, match="progressive"):
        gltf.png_decode(data.replace(b"\xff\xc0", b"\xff\xc2", 1))
