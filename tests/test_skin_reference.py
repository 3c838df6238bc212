"""tests/skin_reference.py, the numpy arbiter of skeletal skinning, pinned by hand: the cases below are worked out here, not by the arbiter."""
import numpy as np

import skin_reference as R

F = np.float32
VERTEX = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("tangent", "<f4", 3), ("bitangent", "<f4", 3), ("tex_coords", "<f4", 2)])


def glm(m):
    """a math matrix M[row][col] as 16 floats in glm memory order"""
    return np.asarray(m, F).T.reshape(16)


def one_vertex(p, n=(0, 0, 1), t=(1, 0, 0), b=(0, 1, 0), uv=(0.25, 0.75)):
    v = np.zeros(1, VERTEX)
    v["position"], v["normal"], v["tangent"], v["bitangent"], v["tex_coords"] = p, n, t, b, uv
    return v


def one_skin(joints, weights):
    s = np.zeros(1, R.SKIN_DTYPE)
    s["joints"], s["weights"] = joints, weights
    return s


def test_identity_joints_return_the_input_bits():
    rng = np.random.default_rng(1)
    v, s, _ = R.random_case(rng, 97, 5, VERTEX)
    s["weights"] = 0
    s["weights"][:, 0] = 1                       # (weights that merely sum to 1 in fp32 need not give S = I exactly)
    J = np.tile(glm(np.eye(4)), (5, 1))
    out = R.skin_vertices(v, s, J)
    assert out.tobytes() == v.tobytes()


def test_one_joint_translation():
    T = np.eye(4); T[:3, 3] = (1.0, 2.0, -3.0)
    v = one_vertex((0.5, 0.25, 4.0))
    out = R.skin_vertices(v, one_skin((0, 0, 0, 0), (1, 0, 0, 0)), glm(T)[None])
    np.testing.assert_array_equal(out["position"][0], np.array([1.5, 2.25, 1.0], F))     # exact in fp32
    for name in ("normal", "tangent", "bitangent", "tex_coords"):                      # a translation moves no vector
        np.testing.assert_array_equal(out[name], v[name])


def test_two_joint_blend():
    """50 / 50 between the identity and a quarter turn about z with translation (2, 0, 0): S = [[.5, -.5, 0, 1], [.5, .5, 0, 0], [0, 0, 1, 0]]"""
    A = np.eye(4)
    B = np.array([[0, -1, 0, 2], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], float)
    v = one_vertex((1.0, 3.0, 5.0), n=(1, 0, 0))
    out = R.skin_vertices(v, one_skin((0, 1, 0, 0), (0.5, 0.5, 0, 0)), np.stack([glm(A), glm(B)]))
    np.testing.assert_array_equal(out["position"][0], np.array([0.5 * 1 - 0.5 * 3 + 1.0, 0.5 * 1 + 0.5 * 3, 5.0], F))
    np.testing.assert_array_equal(out["normal"][0], np.array([0.5, 0.5, 0.0], F))        # not normalised here
    np.testing.assert_array_equal(out["tex_coords"][0], np.array([0.25, 0.75], F))


def test_the_summation_order_is_the_headers():
    """w0 J0 + w1 J1 cancels to 0 first, then the small third term survives: ((a + b) + c) + d.  Summed from the other end the small term is
    absorbed by the large one before the cancellation, and the bits differ."""
    big, small = F(2.0 ** 26), F(1.0)
    mats = [np.eye(4) for _ in range(4)]
    mats[0][0, 3], mats[1][0, 3], mats[2][0, 3], mats[3][0, 3] = big, -big, small, 0.0
    J = np.stack([glm(m) for m in mats])
    s = one_skin((0, 1, 2, 3), (1, 1, 1, 1))
    S = R.blended(s, J)[0]
    assert S[12] == F(1.0)                                                        # ((2^26 - 2^26) + 1) + 0
    reordered = F(1) * J[0][12] + (F(1) * J[1][12] + (F(1) * J[2][12] + F(1) * J[3][12]))    # 2^26 + (-2^26 + 1) = 2^26 - 2^26
    assert reordered == F(0.0) and reordered.tobytes() != S[12].tobytes()
    # and the position's sum: ((S0 x + S4 y) + S8 z) + S12, with x chosen so that the order matters as well
    mats = [np.eye(4)]
    mats[0][0, :] = (1.0, 1.0, 1.0, 0.0)
    v = one_vertex((2.0 ** 26, -(2.0 ** 26), 1.0))
    out = R.skin_vertices(v, one_skin((0, 0, 0, 0), (1, 0, 0, 0)), glm(mats[0])[None])
    assert out["position"][0, 0] == F(1.0)
    assert F(2.0 ** 26) + (F(-(2.0 ** 26)) + F(1.0)) == F(0.0)
