"""tests/antialias_reference.py pinned with known answers (no GPU): values worked out from the text of include/arctic_hip.h, and the proof that the
input set of tests/test_gpu_antialias.py tells every entry of MUTATIONS from the definition on at least one pixel."""
import numpy as np
import pytest

import antialias_reference as AR


def _levels(img):
    assert (img[..., 0] == img[..., 1]).all() and (img[..., 1] == img[..., 2]).all()
    return img[..., 0].astype(int)


def test_isolated_spike():
    """9x9 grey 30, centre 255: s1 = 256 -> s2 = 256 -> off_s = 192; off_e = 0 because both searches stop at 1;
    (255 * 64 + 30 * 192 + 128) >> 8 = 86.  The four neighbours pass the early exit but blend with offset 0."""
    img = AR.centre_image(9, 30, 255)
    out, edge = AR.antialias(img, return_edges=True)
    want = _levels(img)
    want[4, 4] = 86
    assert (_levels(out) == want).all() and (out[..., 3] == 255).all()
    assert edge.sum() == 5


@pytest.mark.parametrize("background,centre,changes", [(100, 116, True), (100, 115, False), (175, 200, True), (175, 199, False)])
def test_early_exit_thresholds(background, centre, changes):
    """16 grey steps are 16 * 256 = 4096 = T_MIN of luma; at 175 / 200 the range 25 * 256 = 6400 = 51200 >> 3"""
    img = AR.centre_image(5, background, centre)
    out, edge = AR.antialias(img, return_edges=True)
    assert bool(edge[2, 2]) == changes
    if changes:
        assert out[2, 2, 0] != centre and (np.delete(_levels(out).ravel(), 12) == background).all()
        if background == 100:
            assert out[2, 2, 0] == 104
    else:
        assert (out == img).all() and not edge.any()


def test_straight_edge_longer_than_the_image():
    """both searches saturate: span = 24, d = 12, off_e = 0; the sub-pixel term alone moves the two columns at the edge"""
    img = AR.straight_edge(9, 16, 8)
    out = AR.antialias(img)
    assert int((out != img).any(axis=-1).sum()) == 18
    want = _levels(img)
    want[:, 7], want[:, 8] = 9, 191
    assert (_levels(out) == want).all()


def test_staircase_ramps():
    img = AR.staircase_12x40()
    out = _levels(AR.antialias(img))
    assert list(out[6, 10:30]) == [191, 186, 180, 174, 167, 159, 150, 141, 129, 116, 84, 71, 59, 50, 41, 33, 26, 20, 14, 9]
    assert list(out[7, 10:30]) == [9] * 9 + [3] + [0] * 10


def test_flat_and_low_contrast_images_are_left_alone():
    rs = np.random.RandomState(0)
    noise = AR.grey(120 + rs.randint(0, 8, (40, 40)))      # 7 grey steps < 16
    assert (AR.antialias(noise) == noise).all()
    flat = np.full((17, 23, 4), 200, np.uint8)
    assert (AR.antialias(flat) == flat).all()


def test_alpha_is_copied_and_shape_kept():
    img = AR.polygons(37, 53)
    out, edge = AR.antialias(img, return_edges=True)
    assert out.shape == img.shape and out.dtype == np.uint8
    assert (out[..., 3] == img[..., 3]).all()
    assert 0.02 < edge.mean() < 0.2
    assert (out[~edge] == img[~edge]).all()


def test_transpose_symmetry_away_from_ties():
    """on an image without orientation ties the filter commutes with transposition (the definition treats the axes alike but for eh >= ev)"""
    img = AR.straight_edge(20, 31, 13)
    t = np.ascontiguousarray(img.transpose(1, 0, 2))
    assert (AR.antialias(t) == AR.antialias(img).transpose(1, 0, 2)).all()


@pytest.fixture(scope="module")
def gpu_inputs():
    # the tile of the kernel as built (csrc/antialias.hip: 64 x 16); any tile gives the same named images, only three sizes follow it
    inputs = AR.make_inputs(64, 16)
    return inputs, {k: AR.antialias(v) for k, v in inputs.items()}


@pytest.mark.parametrize("mutation", sorted(AR.MUTATIONS))
def test_gpu_input_set_catches_every_mutation(gpu_inputs, mutation):
    inputs, truth = gpu_inputs
    caught = [k for k, v in inputs.items() if (AR.antialias(v, mutation=mutation) != truth[k]).any()]
    assert caught, f"{mutation}: {AR.MUTATIONS[mutation]} changes no pixel of the GPU test's inputs"


def test_which_inputs_catch_which_mutation(gpu_inputs):
    """what the issue's CPU check found: uniformly random RGBA misses the two ties that the palette / grey-level images catch, and only the
    threshold images catch the early exit's >="""
    inputs, truth = gpu_inputs

    def catches(name, mutation):
        return bool((AR.antialias(inputs[name], mutation=mutation) != truth[name]).any())

    for m in ("orientation_gt", "search_k_plus_1", "no_subpixel", "no_rounding", "alpha_blended"):
        assert catches("random", m), m
    for m in ("side_gt", "search_stop_gt"):
        assert catches("palette", m) or catches("grey_levels", m), m
    assert catches("tmin_at", "early_exit_gt") and catches("eighth_at", "early_exit_gt")
    assert not any(catches(k, "early_exit_gt") for k in ("random", "polygons", "staircases"))
