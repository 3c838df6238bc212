"""The edge anti-aliasing pass on the device (csrc/antialias.hip; ARCTIC_OPT_ANTIALIAS, arctic_antialias, arctic_antialias_device): bit for bit
against tests/antialias_reference.py -- through the host entry on the input set that tests/test_antialias_reference.py shows to catch every
entry of MUTATIONS, through the device entry, through every frame path of a handle with the option on, and on shards."""
import copy

import numpy as np
import pytest

import antialias_reference as AR

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 16          # the kernel's workgroup tile (csrc/common.h: ANTIALIAS_TILE_W / _H)
INPUTS = AR.make_inputs(TILE_W, TILE_H)


@pytest.fixture(scope="module")
def truth():
    return {k: AR.antialias(v) for k, v in INPUTS.items()}


@pytest.fixture(scope="module")
def handle(hip):
    r = hip.Renderer(64, 48, 0, 1)   # any handle filters any image
    yield r
    r.close()


@pytest.fixture(scope="module")
def scene(pkg):
    return pkg.scenes.config3(scale=0.1)


def _renderer(hip, sc, **kw):
    return sc.upload(hip.Renderer(sc.width, sc.height, sc.shadow_size, sc.max_lights, **kw))


@pytest.fixture(scope="module")
def plain(hip, scene):
    """config 3 at 384 x 216 (216 is no multiple of 16) with the option off, and the reference's filtered image of it"""
    r = _renderer(hip, scene)
    img = r.render_frame(scene.desc, scene.settings).copy()
    r.close()
    want, edge = AR.antialias(img, return_edges=True)
    assert (scene.width, scene.height) == (384, 216) and 0.005 < edge.mean() < 0.5 and (want != img).any()
    return img, want


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def test_input_set_covers_the_sizes():
    shapes = {v.shape[:2] for v in INPUTS.values()}
    assert {(1, 1), (1, 40), (40, 1), (2, 2), (33, 65), (70, 130)} <= shapes
    assert any(h % TILE_H == 0 and w % TILE_W == 0 for h, w in shapes)
    assert any(h > 3 * TILE_H and h % TILE_H and w > 3 * TILE_W and w % TILE_W for h, w in shapes)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_host_entry_bit_for_bit(handle, truth, name):
    img = INPUTS[name]
    got = handle.antialias(img)
    assert got.shape == img.shape and got.dtype == np.uint8
    np.testing.assert_array_equal(got, truth[name])


def test_host_entry_in_place_and_constant(handle, truth):
    img = INPUTS["polygons"].copy()
    import ctypes as C
    rc = handle.L.arctic_antialias(handle.h, img.ctypes.data_as(C.c_void_p), img.shape[1], img.shape[0], img.ctypes.data_as(C.c_void_p))
    assert rc == 0
    np.testing.assert_array_equal(img, truth["polygons"])           # the same host buffer for input and output
    np.testing.assert_array_equal(handle.antialias(INPUTS["constant"]), INPUTS["constant"])


@pytest.mark.parametrize("name", ["polygons", "palette_tiles", "random_65x33", "tile_multiple"])
def test_device_entry_into_a_callers_buffer(handle, truth, name):
    """16-byte aligned whole rows (the vector path) and an odd width / a misaligned base (the scalar path)"""
    import torch
    img = INPUTS[name]
    h, w = img.shape[:2]
    d_in = dev(img)
    d_out = torch.full((h * w * 4 + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    for shift in (0, 4):     # a destination that is only 4-byte aligned
        out = d_out[shift:shift + h * w * 4]
        handle.antialias_device(d_in.data_ptr(), out.data_ptr(), w, h)
        handle.flush()
        np.testing.assert_array_equal(out.cpu().numpy().reshape(h, w, 4), truth[name])
    assert int(d_out[h * w * 4 + 4]) == 0xAB and (d_in.cpu().numpy() == img).all()      # nothing beyond the image, nothing of the input written


def test_device_entry_refuses_bad_arguments(hip, handle):
    import torch
    buf = torch.zeros(2 * 64 * 64 * 4, dtype=torch.uint8, device="cuda")
    a, n = buf.data_ptr(), 64 * 64 * 4
    for args in ((0, a, 64, 64), (a, 0, 64, 64),               # a null pointer
                 (a, a + n, 0, 64), (a, a + n, 64, 0),         # a zero size
                 (a, a, 64, 64), (a, a + n - 4, 64, 64), (a + n - 4, a, 64, 64)):   # overlapping ranges
        with pytest.raises(hip.ArcticError) as e:
            handle.antialias_device(*args)
        assert e.value.code == -1
    handle.antialias_device(a, a + n, 64, 64)                  # adjacent ranges do not overlap
    handle.flush()
    with pytest.raises(hip.ArcticError) as e:
        handle.antialias(np.zeros((0, 4, 4), np.uint8))
    assert e.value.code == -1


@pytest.mark.parametrize("value", [2, -1])
def test_other_option_values_are_refused(hip, handle, value):
    with pytest.raises(hip.ArcticError) as e:
        handle.set_option("antialias", value)
    assert e.value.code == -1


def test_render_frame_with_the_option(hip, scene, plain):
    img, want = plain
    r = _renderer(hip, scene)
    r.set_option("antialias", 1)
    np.testing.assert_array_equal(r.render_frame(scene.desc, scene.settings), want)
    np.testing.assert_array_equal(r.read_output(want=("rgba8",))[2], want)
    r.set_option("antialias", 0)          # back to 0: the bytes of a fresh handle
    np.testing.assert_array_equal(r.render_frame(scene.desc, scene.settings), img)
    np.testing.assert_array_equal(r.read_output(want=("rgba8",))[2], img)
    r.close()


def test_render_frame_device_and_the_passes(hip, scene, plain):
    import torch
    img, want = plain
    r = _renderer(hip, scene)
    r.set_option("antialias", 1)
    out = torch.zeros((scene.height, scene.width, 4), dtype=torch.uint8, device="cuda")
    r.render_frame_device(scene.desc, scene.settings, out.data_ptr())
    r.flush()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    out.zero_()
    r.pass_gbuffer(scene.desc)
    r.pass_shade(scene.desc, scene.settings, out.data_ptr())       # into the caller's buffer ...
    r.flush()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    r.pass_shade(scene.desc, scene.settings)                       # ... and into the handle's own
    np.testing.assert_array_equal(r.read_output(want=("rgba8",))[2], want)
    r.time_shade(scene.desc, scene.settings, warmup=0, iters=1)    # the shading kernel alone: what it wrote
    np.testing.assert_array_equal(r.read_output(want=("rgba8",))[2], img)
    r.close()


def test_float_planes_are_not_filtered(hip, scene, plain):
    img, want = plain
    outs = []
    for on in (0, 1):
        r = _renderer(hip, scene)
        r.set_option("keep_float_output", 1)
        r.set_option("antialias", on)
        r.render_frame(scene.desc, scene.settings)
        outs.append(r.read_output())
        r.close()
    (ldr0, hdr0, rgba0), (ldr1, hdr1, rgba1) = outs
    assert ldr0.tobytes() == ldr1.tobytes() and hdr0.tobytes() == hdr1.tobytes()
    np.testing.assert_array_equal(rgba0, img)
    np.testing.assert_array_equal(rgba1, want)


@pytest.mark.parametrize("in_flight", [1, 2])
def test_moving_camera_frames_in_flight(hip, scene, in_flight):
    import torch
    descs = []
    for k in range(3):
        d = copy.deepcopy(scene.desc)
        d.camera["rotation"] = (-12.0 + 2.0 * k, 9.0 * k)
        descs.append(d)
    frames = []
    for on in (0, 1):
        r = _renderer(hip, scene)
        r.set_option("frames_in_flight", in_flight)
        r.set_option("antialias", on)
        outs = [torch.zeros((scene.height, scene.width, 4), dtype=torch.uint8, device="cuda") for _ in descs]
        for d, o in zip(descs, outs):
            r.render_frame_device(d, scene.settings, o.data_ptr())
        last = r.render_frame(descs[-1], scene.settings)             # and one into the handle's own buffers behind them
        r.flush()
        frames.append([o.cpu().numpy() for o in outs] + [last])
        r.close()
    assert (frames[0][0] != frames[0][2]).any()
    for off, on in zip(*frames):
        np.testing.assert_array_equal(on, AR.antialias(off))


def test_shards_accept_the_option_and_stay_unfiltered(hip, scene, plain):
    img, want = plain
    cut = 100                                                         # inside a tile row
    kinds = [dict(row_begin=0, row_end=cut), dict(row_begin=cut, row_end=scene.height), dict(band_rows=16, shard=(0, 3)),
             dict(band_rows=16, shard=(1, 3)), dict(band_rows=16, shard=(2, 3))]
    shards = []
    for kw in kinds:
        r = _renderer(hip, scene, **kw)
        off = r.render_frame(scene.desc, scene.settings).copy()
        r.set_option("antialias", 1)
        on = r.render_frame(scene.desc, scene.settings)
        np.testing.assert_array_equal(on, off)
        np.testing.assert_array_equal(r.read_output(want=("rgba8",))[2], off)
        shards.append(on.copy())
        r.close()
    np.testing.assert_array_equal(np.concatenate(shards[:2]), img)


def test_root_filters_the_assembled_frame(pkg, hip, scene, plain):
    import torch
    from importlib import import_module
    sharding = import_module("arctic_renderer_amd.sharding")
    img, want = plain
    cut = 100
    parts, handles = [], []
    for kw in (dict(row_begin=0, row_end=cut), dict(row_begin=cut, row_end=scene.height)):
        r = _renderer(hip, scene, **kw)
        r.set_option("antialias", 1)
        parts.append(dev(r.render_frame(scene.desc, scene.settings)))
        handles.append(r)
    frame = sharding.assemble(parts)
    np.testing.assert_array_equal(frame.cpu().numpy(), img)
    np.testing.assert_array_equal(sharding.assemble(parts, antialias=handles[0]).cpu().numpy(), want)
    out = torch.zeros_like(frame)
    handles[1].antialias_device(frame.data_ptr(), out.data_ptr(), scene.width, scene.height)
    handles[1].flush()
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    for r in handles:
        r.close()
