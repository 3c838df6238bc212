"""The morph-target arbiter (tests/morph_reference.py) pinned against a hand-computed vertex and a float64 evaluation, and the properties
the definition in include/arctic_hip.h states: all-zero weights are the input bytes, a weight of either sign of zero is skipped, and skipping
is not the same as adding 0 * d."""
import numpy as np

import morph_reference as R

F = np.float32
VERTEX_DTYPE = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("tangent", "<f4", 3), ("bitangent", "<f4", 3), ("tex_coords", "<f4", 2)])


def test_vertex_dtype_is_the_package_s(pkg):
    assert VERTEX_DTYPE == pkg.scene.VERTEX_DTYPE and R.MORPH_DTYPE == pkg.scene.MORPH_DELTA_DTYPE


def test_hand_computed_vertex():
    u = 2.0 ** -23                                      # one ulp of 1.0
    v = np.zeros(1, VERTEX_DTYPE)
    v["position"] = (1.0, 2.0, -4.0)
    v["normal"] = (1.0, 1.0, 0.0)
    v["tangent"] = (0.5, 0.0, 0.0)
    v["bitangent"] = (0.0, 0.0, 8.0)
    v["tex_coords"] = (0.25, 0.75)
    d = np.zeros((3, 1), R.MORPH_DTYPE)
    d["position"][0, 0] = (0.25, -1.0, 0.5)
    d["position"][1, 0] = (100.0, 100.0, 100.0)         # weight 0: never seen
    d["position"][2, 0] = (1.0, 1.0, 1.0)
    # normal.x: 1 + 3 * (u/2) is a tie between 1 + u and 1 + 2u and rounds to the even 1 + 2u; then + 1 * (-u/2) is a tie again, between 1 + u
    # and 1 + 2u, and stays 1 + 2u.  Exact arithmetic gives 1 + u: the two roundings are visible.
    d["normal"][0, 0] = (u / 2, u / 2, 0.0)
    d["normal"][2, 0] = (-u / 2, 0.0, 0.0)
    d["tangent"][0, 0] = (0.1, 0.0, 0.0)                # 0.5 + fl(3 * fl(0.1))
    d["bitangent"][2, 0] = (0.0, 0.0, -8.0)
    w = np.array([3.0, 0.0, 1.0], F)
    got = R.morph_vertices(v, d, w)[0]
    np.testing.assert_array_equal(got["position"], np.array([1.0 + 0.75 + 1.0, 2.0 - 3.0 + 1.0, -4.0 + 1.5 + 1.0], F))
    assert got["normal"][0] == F(1.0 + 2 * u) and got["normal"][0] != F(1.0 + u)
    assert got["normal"][1] == F(1.0 + 2 * u) and got["normal"][2] == 0.0
    assert got["tangent"][0] == F(0.5) + F(3.0) * F(0.1)
    assert got["bitangent"][2] == 0.0
    np.testing.assert_array_equal(got["tex_coords"], v["tex_coords"][0])


def test_against_float64_within_the_rounding_it_must_show(pkg):
    rng = np.random.default_rng(11)
    v, d, w = R.random_case(rng, 200, 9, VERTEX_DTYPE)
    got = R.morph_vertices(v, d, w)
    differs = 0
    for name in R.VERTEX_FIELDS:
        m = v[name].astype(np.float64)
        bound = np.zeros_like(m)
        for k in range(len(w)):
            if w[k] == 0:
                continue
            p = np.float64(w[k]) * d[k][name].astype(np.float64)
            m = m + p
            bound += (np.abs(p) + np.abs(m)) * 2.0 ** -24          # half an ulp for the product, half an ulp for the sum
        err = np.abs(got[name].astype(np.float64) - m)
        assert (err <= bound * 1.001 + 1e-45).all()
        differs += int((got[name].astype(np.float64) != m).sum())
    assert differs > 100                                            # float32 rounding is there: this is not a float64 evaluation cast down
    assert got["tex_coords"].tobytes() == v["tex_coords"].tobytes()


def test_all_zero_weights_return_the_input_bytes():
    v, d, _ = R.random_case(np.random.default_rng(5), 50, 4, VERTEX_DTYPE)
    assert np.signbit(v["normal"][0, 1]) and v["normal"][0, 1] == 0          # a -0.0 in the base
    for w in (np.zeros(4, F), np.array([0.0, -0.0, 0.0, -0.0], F)):
        assert R.morph_vertices(v, d, w).tobytes() == v.tobytes()


def test_a_weight_of_minus_zero_is_skipped():
    v, d, _ = R.random_case(np.random.default_rng(6), 20, 3, VERTEX_DTYPE)
    w = np.array([0.5, -0.0, -1.25], F)
    two = R.morph_vertices(v, d[[0, 2]], w[[0, 2]])
    assert R.morph_vertices(v, d, w).tobytes() == two.tobytes()


def test_skipping_differs_from_adding_zero_times_d_exactly_at_a_minus_zero():
    v = np.zeros(1, VERTEX_DTYPE)
    v["position"] = (-0.0, 1.5, 0.0)
    d = np.zeros((1, 1), R.MORPH_DTYPE)
    d["position"] = (2.0, 2.0, 2.0)
    skipped = R.morph_vertices(v, d, np.zeros(1, F))
    added = v["position"] + F(0.0) * d[0]["position"]                # what "no skipping" would compute
    assert np.signbit(skipped["position"][0, 0]) and not np.signbit(added[0, 0])      # -0.0 + 0.0 = +0.0
    assert skipped["position"][0, 1:].tobytes() == added[0, 1:].tobytes()             # ... and nowhere else
    assert skipped.tobytes() == v.tobytes()
