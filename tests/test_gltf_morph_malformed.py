"""Hostile morph targets, sparse accessors and weights animations through a sanitizer build of the scene-loader stand-in
(host/gltf_loader.cpp), by the method of tests/test_gltf_skins_malformed.py: the loader is compiled with -fsanitize=address,undefined (CPU
only) into the stand-alone driver tests/cpp/morph_sanitize.cpp, which loads each file and evaluates every mesh's weights under every animation.
Every file must either be refused with a message -- when it is loaded or when its weights are evaluated -- or give finite deltas and weights:
no sanitizer report, no crash, no hang."""
import base64
import os
import subprocess

import numpy as np
import pytest

from gltf_morph_files import write_morphed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "cpp", "morph_sanitize")


@pytest.fixture(scope="module")
def driver():
    src = [os.path.join(ROOT, "tests", "cpp", "morph_sanitize.cpp"), os.path.join(ROOT, "arctic-renderer_amd", "host", "gltf_loader.cpp")]
    if not os.path.exists(DRIVER) or any(os.path.getmtime(s) > os.path.getmtime(DRIVER) for s in src):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-o", DRIVER] + src + ["-lz"])
    return DRIVER


def run(driver, paths):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([driver] + [str(p) for p in paths], capture_output=True, text=True, errors="replace", timeout=300, env=env)
    report = out.stdout + out.stderr
    assert out.returncode == 0 and "AddressSanitizer" not in report and "runtime error" not in report and "BAD" not in report, report[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith(("ok", "refused"))]
    assert len(lines) == len(paths)
    return lines


def target(doc, k, name):
    return doc["accessors"][doc["meshes"][0]["primitives"][0]["targets"][k][name]]


def set_(obj, key, val):
    obj[key] = val


def rewrite(doc, view, data, at=0):
    """overwrite bytes of a bufferView's data"""
    v = doc["bufferViews"][view]
    raw = bytearray(base64.b64decode(doc["buffers"][0]["uri"].split(",", 1)[1]))
    raw[v["byteOffset"] + at:v["byteOffset"] + at + len(data)] = data
    doc["buffers"][0]["uri"] = "data:application/octet-stream;base64," + base64.b64encode(bytes(raw)).decode()


def test_valid_files_evaluate(driver, tmp_path):
    paths = [write_morphed(tmp_path, "dense.gltf", animations=False)[0],
             write_morphed(tmp_path, "sparse8.gltf", storage="sparse", animations=False)[0],
             write_morphed(tmp_path, "sparse32.gltf", storage="sparse", index_type=5125, base_view=True, animations=False, two_nodes=True, tangent_attr=False)[0],
             write_morphed(tmp_path, "skin.gltf", skin=True, animations=False, mesh_weights=[0.5, 0.25])[0]]
    lines = run(driver, paths)
    assert all(l.startswith("ok") and " 0 morphed" not in l for l in lines), lines
    lines = run(driver, [write_morphed(tmp_path, "cubic.gltf")[0]])          # loads; the CUBICSPLINE / stray-weights animations refuse their evaluation
    assert lines[0].startswith("refused") and "(weights)" in lines[0]


def test_hostile_targets_and_weights(driver, tmp_path):
    def variant(name, edit, **kw):
        kw.setdefault("animations", True)
        def whole(d):
            d["animations"] = d["animations"][:2] if "animations" in d else []   # (without the two animations that refuse only themselves)
            edit(d)
        return write_morphed(tmp_path, name + ".gltf", edit=whole, **kw)[0]

    sparse = dict(storage="sparse", index_type=5123)
    f32 = lambda values: np.asarray(values, np.float32).tobytes()
    u16 = lambda values: np.asarray(values, np.uint16).tobytes()
    sp = lambda d: target(d, 0, "POSITION")["sparse"]

    def near_the_end(d, view):           # the view starts 8 bytes before the end of the buffer: too short for its accessor
        d["bufferViews"][view]["byteOffset"] = d["buffers"][0]["byteLength"] - 8

    def second_primitive(d):             # a second primitive of the same mesh with one target fewer
        p = dict(d["meshes"][0]["primitives"][0])
        p["targets"] = p["targets"][:1]
        d["meshes"][0]["primitives"].append(p)

    refused = [
        variant("sparse_index_out_of_range", lambda d: rewrite(d, sp(d)["indices"]["bufferView"], u16([6, 7, 8, 9, 18])), **sparse),
        variant("sparse_index_far_out_of_range", lambda d: rewrite(d, sp(d)["indices"]["bufferView"], u16([6, 7, 8, 9, 65535])), **sparse),
        variant("sparse_indices_not_increasing", lambda d: rewrite(d, sp(d)["indices"]["bufferView"], u16([6, 7, 7, 9, 11])), **sparse),
        variant("sparse_indices_decreasing", lambda d: rewrite(d, sp(d)["indices"]["bufferView"], u16([11, 9, 8, 7, 6])), **sparse),
        variant("sparse_count_above_accessor", lambda d: set_(sp(d), "count", 19), **sparse),
        variant("sparse_count_huge", lambda d: set_(sp(d), "count", 2 ** 40), **sparse),
        variant("sparse_and_accessor_count_huge", lambda d: (set_(sp(d), "count", 2 ** 40), set_(target(d, 0, "POSITION"), "count", 2 ** 40)), **sparse),
        variant("accessor_count_huge", lambda d: set_(target(d, 0, "POSITION"), "count", 2 ** 40), **sparse),
        variant("sparse_indices_view_short", lambda d: set_(sp(d), "count", 6), **sparse),
        variant("sparse_values_view_short", lambda d: set_(sp(d)["values"], "byteOffset", 8), **sparse),
        variant("sparse_indices_offset_huge", lambda d: set_(sp(d)["indices"], "byteOffset", 2 ** 50), **sparse),
        variant("sparse_indices_as_floats", lambda d: set_(sp(d)["indices"], "componentType", 5126), **sparse),
        variant("sparse_view_index_high", lambda d: set_(sp(d)["values"], "bufferView", 999), **sparse),
        variant("sparse_count_negative", lambda d: set_(sp(d), "count", -1), **sparse),
        variant("base_view_short", lambda d: near_the_end(d, target(d, 0, "POSITION")["bufferView"]), base_view=True, **sparse),
        variant("dense_view_short", lambda d: near_the_end(d, target(d, 1, "NORMAL")["bufferView"])),
        variant("target_vec4", lambda d: set_(target(d, 0, "POSITION"), "type", "VEC4")),
        variant("target_vec2", lambda d: set_(target(d, 1, "NORMAL"), "type", "VEC2")),
        variant("target_as_shorts", lambda d: set_(target(d, 0, "TANGENT"), "componentType", 5122)),
        variant("target_count_short", lambda d: set_(target(d, 0, "POSITION"), "count", 17)),
        variant("target_count_long", lambda d: set_(target(d, 1, "POSITION"), "count", 19), **sparse),
        variant("target_accessor_high", lambda d: set_(d["meshes"][0]["primitives"][0]["targets"][0], "POSITION", 999)),
        variant("target_accessor_negative", lambda d: set_(d["meshes"][0]["primitives"][0]["targets"][0], "NORMAL", -3)),
        variant("targets_not_an_array", lambda d: set_(d["meshes"][0]["primitives"][0], "targets", {"POSITION": 0})),
        variant("target_not_an_object", lambda d: set_(d["meshes"][0]["primitives"][0], "targets", [3, 4])),
        variant("unequal_target_counts", second_primitive),
        variant("mesh_weights_short", lambda d: set_(d["meshes"][0], "weights", [0.5])),
        variant("mesh_weights_long", lambda d: set_(d["meshes"][0], "weights", [0.5, 0.5, 0.5])),
        variant("node_weights_long", lambda d: set_(d["nodes"][1], "weights", [0.5, 0.5, 0.5])),
        variant("node_weights_not_numbers", lambda d: set_(d["nodes"][1], "weights", ["a", "b"])),
        variant("node_weights_not_finite", lambda d: set_(d["nodes"][1], "weights", [1e999, 0.0])),
        variant("mesh_weights_beyond_fp32", lambda d: set_(d["meshes"][0], "weights", [1e300, 0.0])),
        variant("node_weights_on_a_mesh_without_targets", lambda d: d["meshes"][0]["primitives"][0].pop("targets"), node_weights=[0.5, 0.5]),
        variant("output_count_not_keyframes_x_targets", lambda d: set_(d["accessors"][d["animations"][0]["samplers"][0]["output"]], "count", 5)),
        variant("output_count_huge", lambda d: set_(d["accessors"][d["animations"][0]["samplers"][0]["output"]], "count", 2 ** 40)),
        variant("output_vec3", lambda d: set_(d["accessors"][d["animations"][0]["samplers"][0]["output"]], "type", "VEC3")),
        variant("output_not_finite", lambda d: rewrite(d, d["accessors"][d["animations"][0]["samplers"][0]["output"]]["bufferView"], f32([np.nan]), at=8)),
        variant("input_not_increasing", lambda d: rewrite(d, d["accessors"][d["animations"][0]["samplers"][0]["input"]]["bufferView"], f32([0.5, 0.5, 2.0]))),
        variant("delta_not_finite", lambda d: rewrite(d, target(d, 1, "POSITION")["bufferView"], f32([np.inf]), at=40)),
        variant("delta_nan_in_sparse_values", lambda d: rewrite(d, sp(d)["values"]["bufferView"], f32([np.nan])), **sparse),
        variant("normal_delta_not_finite", lambda d: rewrite(d, target(d, 0, "NORMAL")["bufferView"], f32([-np.inf]), at=12)),
    ]
    lines = run(driver, refused)
    assert all(l.startswith("refused") and "(weights)" not in l for l in lines), [l for l in lines if not l.startswith("refused") or "(weights)" in l]
    # files that are odd but have a meaning: evaluated, with finite weights
    fine = [
        variant("sparse_count_zero", lambda d: set_(sp(d), "count", 0), **sparse),
        variant("no_target_attributes", lambda d: set_(d["meshes"][0]["primitives"][0], "targets", [{}, {}])),
        variant("huge_weights", lambda d: set_(d["nodes"][1], "weights", [1e30, -1e30])),
        variant("channel_without_node", lambda d: d["animations"][0]["channels"][0]["target"].pop("node")),
        variant("empty_mesh_weights_without_targets", lambda d: (d["meshes"][0]["primitives"][0].pop("targets"), set_(d["meshes"][0], "weights", []))),
    ]
    lines = run(driver, fine)
    assert all(l.startswith(("ok", "refused")) for l in lines) and all(l.startswith("ok") for l in lines[:4]), lines


def test_mutated_documents(driver, tmp_path):
    """150 random byte flips in the JSON of a morphed, skinned file with sparse targets: whatever it decodes to is refused or evaluated"""
    rng = np.random.default_rng(8)
    text = open(write_morphed(tmp_path, "base.gltf", storage="sparse", index_type=5123, base_view=True, skin=True, two_nodes=True, mesh_weights=[0.25, 0.5])[0], "rb").read()
    head = text.index(b'"buffers"') if b'"buffers"' in text else len(text)
    paths = []
    for k in range(150):
        b = bytearray(text)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, head))] = int(rng.integers(32, 127))
        p = tmp_path / f"m{k}.gltf"
        p.write_bytes(bytes(b))
        paths.append(p)
    assert head > 1000
    run(driver, paths)
