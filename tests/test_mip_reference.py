"""tests/mip_reference.py on its own terms (no device): the chain the GPU tests compare the device's with."""
import numpy as np

import mip_reference as MR


def test_level_sizes():
    assert MR.level_sizes(1, 1) == [(1, 1)]
    assert MR.level_sizes(5, 3) == [(5, 3), (2, 1), (1, 1)]
    assert MR.level_sizes(16, 16) == [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    s = MR.level_sizes(2048, 512)
    assert len(s) == 12 and s[0] == (2048, 512) and s[9] == (4, 1) and s[-1] == (1, 1)
    for w, h in ((1, 1), (5, 3), (16, 16), (2048, 512), (33, 17)):
        lv = MR.chain(np.zeros((h, w, 8), np.uint8))
        assert [(x.shape[1], x.shape[0]) for x in lv] == MR.level_sizes(w, h)


def test_table_is_the_srgb_decode():
    t = MR.srgb_table()
    assert t.dtype == np.float32 and t[0] == 0.0 and t[255] == 1.0 and np.all(np.diff(t) > 0)
    c = np.arange(256) / 255.0
    want = np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)
    assert np.abs(t - want).max() < 2e-7


def test_encode_inverts_the_table():
    t = MR.srgb_table().astype(np.float64)
    np.testing.assert_array_equal(MR.encode(t), np.arange(256))
    mid = (t[:-1] + t[1:]) / 2
    np.testing.assert_array_equal(MR.encode(mid), np.arange(255))                      # a tie: the lower code
    np.testing.assert_array_equal(MR.encode(np.nextafter(mid, 2.0)), np.arange(1, 256))


def test_constant_image_stays_constant():
    rng = np.random.default_rng(0)
    for w, h in ((16, 16), (5, 3), (37, 9)):
        texel = rng.integers(0, 256, 8, dtype=np.uint8)
        for lv in MR.chain(np.broadcast_to(texel, (h, w, 8)).copy()):
            assert np.all(lv == texel)


def test_checkerboard_reduces_to_the_code_nearest_one_half():
    img = np.zeros((2, 2, 8), np.uint8)
    img[0, 0] = img[1, 1] = 255
    lv = MR.chain(img)
    assert len(lv) == 2 and lv[1].shape == (1, 1, 8)
    t = MR.srgb_table().astype(np.float64)
    m = (t[0] + t[255] + t[255] + t[0]) / 4
    assert m == 0.5
    d = np.abs(t - m)
    want = int(np.argmin(d))                          # (argmin takes the lower code on a tie)
    assert np.all(lv[1][0, 0, :3] == want)
    assert abs(t[want] - 0.5) <= min(abs(t[want - 1] - 0.5), abs(t[want + 1] - 0.5))
    assert np.all(lv[1][0, 0, 3:] == (0 + 255 + 255 + 0 + 2) >> 2)


def test_trilinear_endpoints():
    rng = np.random.default_rng(2)
    lv = MR.chain(rng.integers(0, 256, (8, 8, 8), dtype=np.uint8))
    u, v = rng.random(20) * 3 - 1, rng.random(20) * 3 - 1
    for k in range(len(lv)):
        np.testing.assert_array_equal(MR.trilinear(lv, u, v, np.full(20, float(k))), MR.bilinear(lv[k], u, v))
    np.testing.assert_array_equal(MR.trilinear(lv, u, v, np.full(20, -3.0)), MR.bilinear(lv[0], u, v))
    np.testing.assert_array_equal(MR.trilinear(lv, u, v, np.full(20, np.nan)), MR.bilinear(lv[0], u, v))
    np.testing.assert_array_equal(MR.trilinear(lv, u, v, np.full(20, 99.0)), MR.bilinear(lv[-1], u, v))
