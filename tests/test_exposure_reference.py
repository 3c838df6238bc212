"""Auto-exposure on a machine without a GPU: the numpy definition of tests/exposure_reference.py pinned on values worked by hand, the exact
properties (i) to (iv) of include/arctic_hip.h, the piecewise-linear logarithm's error on a log-normal plane, the host arbiters
(arctic_exposure_histogram, arctic_exposure_resolve, arctic_exposure_pixels -- the functions the kernels run) equal to numpy BY BYTES at every
size, record and window the GPU tests use, sequences of six calls, and ten deliberate defects in a copy of the reference, each of which must
change output bytes.  The cases, records and windows here are the GPU tests' too (tests/test_gpu_exposure.py)."""
import functools

import numpy as np
import pytest

import exposure_reference as E

F = np.float32
SMALL_SIZES = ((1, 1), (3, 5), (17, 9), (40, 24), (136, 72))            # (width, height)
RECORDS = (E.record(),
           E.record(flags=E.SKIP_BLACK, low_q16=6554, high_q16=65536, key_value=0.5, min_exposure=0.01, max_exposure=8.0, rate_up=0.25, rate_down=0.0625, fallback_exposure=2.0))


@functools.lru_cache(maxsize=None)
def second_trip_size():
    """the frame with the smallest pixel count above G * (pixels per workgroup per trip): every workgroup of k_exposure_meter makes one full
    trip and the first one a second, ragged one.  From arctic_exposure_layout, as square as the count's factors allow"""
    import __graft_entry__ as entry
    R = entry.load_package().renderer
    top = R.exposure_layout(16384, 16384)
    n = top["groups"] * top["pixels_per_trip"] + 1
    while True:
        for h in range(int(n ** 0.5), 0, -1):
            if n % h == 0 and n // h <= 16384:
                lay = R.exposure_layout(n // h, h)
                assert lay["groups"] == top["groups"] and n > lay["groups"] * lay["pixels_per_trip"]
                return n // h, h
        n += 1


def sizes():
    return SMALL_SIZES + (second_trip_size(),)


def windows(width, height):
    """whole, 1 x 1, one row, a ragged interior -- as far as the frame has room for them"""
    out = [(0, 0, 0, 0), (width // 2, height // 2, width // 2 + 1, height // 2 + 1), (0, height - 1, width, height)]
    out.append((1, 1, width - 1, height - 2) if width > 2 and height > 3 else (0, 0, max(width - 1, 1), height))
    return out


@functools.lru_cache(maxsize=None)
def case(width, height, seed=0):
    """a plane over 38 octaves, 2^-20 .. 2^18 (both ends of the histogram and beyond), coloured, with a NaN, both infinities, a negative, a -0 and
    1e30 where there is room; read only.  (The negative pixel is chosen so that no E a clamp or a fallback of RECORDS produces -- 1, 2, 8, 0.01 --
    puts a channel on -1, the pole of the Reinhard curve, where the float64 tonemapper the GPU tests judge against has no value itself)"""
    rng = np.random.default_rng(9000 + 131 * width + height + 7919 * seed)
    l = np.exp2(rng.uniform(-20.0, 18.0, (height, width, 1)))
    C = (l * rng.uniform(0.25, 1.75, (height, width, 3))).astype(F)
    flat = C.reshape(-1, 3)
    if len(flat) >= 12:
        at = rng.choice(len(flat), 8, replace=False)
        flat[at[0]] = (np.nan, 1.0, 2.0); flat[at[1]] = (np.inf, np.inf, np.inf); flat[at[2]] = (-np.inf, 0.5, 0.0); flat[at[3]] = (-3.0, -1.5, -0.75)
        flat[at[4]] = (-0.0, -0.0, -0.0); flat[at[5]] = (1e30, 1e30, 1e30); flat[at[6]] = (np.nan, np.nan, np.nan); flat[at[7]] = (0.0, 0.0, 0.0)
    C.setflags(write=False)
    return C


def constant_plane(width, height):
    """every lane of every wave on one bin"""
    C = np.full((height, width, 3), 0.37, F)
    C.setflags(write=False)
    return C


def cycle_plane(width, height):
    """all 256 bins in turn along a row: grey pixels whose luminance sits in the middle of bin x mod 256"""
    keys = (np.arange(width, dtype=np.uint32) % 256 + 888) << 20 | (1 << 19)
    l = keys.view(F).astype(np.float64)
    grey = (l / (float(F(0.2126)) + float(F(0.7152)) + float(F(0.0722)))).astype(F)
    C = np.ascontiguousarray(np.broadcast_to(grey[None, :, None], (height, width, 3)))
    C.setflags(write=False)
    return C


def state_bytes(s):
    return np.ascontiguousarray(s).tobytes()


def same_state(got, want, what):
    assert state_bytes(got) == state_bytes(want), (what, got, want)


def same_out(got, want, what):
    """the same bytes, no pixel left out -- where a value is a NaN, a NaN (its payload is no part of the definition)"""
    assert got.shape == want.shape and got.dtype == want.dtype == F, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (what, "NaNs elsewhere")
    assert np.where(nan, F(0.0), got).tobytes() == np.where(nan, F(0.0), want).tobytes(), (what, int((np.where(nan, F(0.0), got) != np.where(nan, F(0.0), want)).sum()))


def a_valid_state(adapted_key=1000.25, frames=3):
    s = E.invalid_state()
    s["adapted_key"], s["valid"], s["frames"] = adapted_key, 1, frames
    s["luminance"] = np.array([int(adapted_key * 1048576.0)], np.uint32).view(F)[0]
    s["exposure"] = F(0.18) / s["luminance"]
    return s


# ---- numpy pinned on values worked by hand -------------------------------------------------------------------------------------------------------------
def test_keys_and_bins_by_hand():
    # key = (biased exponent) * 8 + the mantissa's top three bits; 888 = (127 - 16) * 8
    for l, want in ((1.0, 128), (2.0 ** -16, 0), (1.126 * 2.0 ** -16, 1), (1.124 * 2.0 ** -16, 0), (65504.0, 255), (0.0, 0), (2.0 ** -17, 0), (1e-30, 0), (0.5, 120), (1.9, 135),
                    (2.0 ** 15 * 1.874, 254), (2.0 ** 15 * 1.876, 255)):
        assert int(E.bin_of(F(l))) == want, (l, int(E.bin_of(F(l))), want)
    assert ((127 - 16) * 8, 127 * 8 - 888, (127 + 15) * 8 + 7 - 888) == (888, 128, 255)
    # pixels, in scalar arithmetic: the sanitiser, then (0.2126 r + 0.7152 g) + 0.0722 b
    def by_hand(r, g, b):
        x = [F(min(v, 65504.0)) if v > 0 else F(0.0) for v in (r, g, b)]     # (nan > 0 is False)
        l = F(F(F(0.2126) * x[0]) + F(F(0.7152) * x[1])) + F(F(0.0722) * x[2])
        return F(l)
    pixels = [(np.nan, np.nan, np.nan), (np.inf, np.inf, np.inf), (-np.inf, -np.inf, -np.inf), (-1.0, -2.0, -3.0), (-0.0, -0.0, -0.0), (1e30, 1e30, 1e30), (np.nan, 1.0, -3.0),
              (0.18, 0.18, 0.18), (np.inf, 0.0, 0.0), (3.0, np.nan, 0.25)]
    want_bins = [0, 255, 0, 0, 0, 255, 123, None, None, None]
    got = E.bins(np.array(pixels, F))
    lum = E.luminance(np.array(pixels, F))
    for k, (px, want) in enumerate(zip(pixels, want_bins)):
        l = by_hand(*px)
        assert lum[k].tobytes() == l.tobytes(), (px, lum[k], l)
        assert int(got[k]) == int(E.bin_of(l)) and (want is None or int(got[k]) == want), (px, int(got[k]), want)
    assert float(by_hand(np.nan, 1.0, -3.0)) == float(F(0.7152)) and 0.7152 == pytest.approx(1.4304 * 2.0 ** -1) and 126 * 8 + 3 - 888 == 123
    assert float(by_hand(np.inf, np.inf, np.inf)) <= 65504.0 * 1.0000002                 # 65504 cannot exceed bin 255
    H = E.histogram(np.array(pixels, F).reshape(2, 5, 3), E.record())
    assert H.dtype == np.uint32 and int(H.sum()) == 10 and int(H[0]) == 4 and int(H[255]) >= 2


def test_the_band_and_the_tail_by_hand():
    H = np.zeros(256, np.uint32)
    H[10], H[20] = 10, 10
    rec = E.record(low_q16=16384, high_q16=49152)
    # N = 20, lo = 5, hi = 15: bin 10 holds ranks 0..9 -> 5 of them in [5, 15); bin 20 holds ranks 10..19 -> 5
    assert E.band(H, rec) == (10, 5 * 10 + 5 * 20)
    s = E.resolve(H, rec)
    assert float(s["adapted_key"][0]) == 15.0 + 888.5 and int(s["metered"][0]) == 10 and int(s["valid"][0]) == 1 and int(s["frames"][0]) == 1
    # key 903 = exponent 112, mantissa bits 111, and the half bin: 1.9375 * 2^-15
    assert s["luminance"][0].tobytes() == F(1.9375 * 2.0 ** -15).tobytes()
    assert s["exposure"][0].tobytes() == min(F(0.18) / F(1.9375 * 2.0 ** -15), F(1024.0)).tobytes()
    # a band that cuts one bin only
    H2 = np.zeros(256, np.uint32)
    H2[100] = 1000
    assert E.band(H2, E.record(low_q16=100, high_q16=200)) == ((1000 * 200 >> 16) - (1000 * 100 >> 16), 100 * ((1000 * 200 >> 16) - (1000 * 100 >> 16)))
    # lo == hi: nothing measured
    H3 = np.zeros(256, np.uint32)
    H3[50] = 1
    rec3 = E.record(low_q16=100, high_q16=200, fallback_exposure=3.0, max_exposure=2.5)
    assert E.band(H3, rec3) == (0, 0)
    s3 = E.resolve(H3, rec3)
    assert int(s3["valid"][0]) == 0 and float(s3["exposure"][0]) == 2.5 and float(s3["adapted_key"][0]) == 0.0 and int(s3["frames"][0]) == 0
    # all black under SKIP_BLACK: M == 0 -- a valid state is left, an invalid one stays invalid, E is the clamped fallback
    black = np.zeros(256, np.uint32)
    black[0] = 77
    recb = E.record(flags=E.SKIP_BLACK, fallback_exposure=0.0001, min_exposure=0.5)
    assert E.band(black, recb) == (0, 0) and E.band(black, E.record())[0] > 0
    held = a_valid_state()
    sb = E.resolve(black, recb, held)
    assert float(sb["exposure"][0]) == 0.5 and int(sb["metered"][0]) == 0
    for name in ("adapted_key", "luminance", "valid", "frames"):
        assert sb[name].tobytes() == held[name].tobytes(), name
    si = E.resolve(black, recb, None)
    assert int(si["valid"][0]) == 0 and float(si["exposure"][0]) == 0.5
    # the rates: 0 stays, 1 arrives, and each branch takes its own
    target = float(s["adapted_key"][0])                                           # 903.5
    for prev_key, up in ((800.0, True), (1000.0, False)):
        prev = a_valid_state(prev_key, frames=9)
        for ru, rd in ((0.0, 0.0), (1.0, 1.0), (0.25, 0.75)):
            got = E.resolve(H, E.record(low_q16=16384, high_q16=49152, rate_up=ru, rate_down=rd), prev)
            rate = ru if up else rd
            assert float(got["adapted_key"][0]) == prev_key + (target - prev_key) * rate and int(got["frames"][0]) == 10, (prev_key, ru, rd)
        got = E.resolve(H, E.record(flags=E.RESET, low_q16=16384, high_q16=49152, rate_up=0.0, rate_down=0.0), prev)
        assert float(got["adapted_key"][0]) == target and int(got["frames"][0]) == 1


# ---- the exact properties ----------------------------------------------------------------------------------------------------------------------------
def test_property_i_the_histogram_counts_every_pixel_of_the_window():
    for width, height in sizes():
        C = case(width, height)
        for w in windows(width, height):
            x0, y0, x1, y1 = E.window_of(E.record(window=w), width, height)
            assert int(E.histogram(C, E.record(window=w)).astype(np.uint64).sum()) == (x1 - x0) * (y1 - y0), (width, height, w)
    junk = np.array([np.nan, np.inf, -np.inf, -1.0, 1e38, -0.0], F)[np.random.default_rng(1).integers(0, 6, (9, 7, 3))]
    assert int(E.histogram(junk, E.record()).sum()) == 63


def inside_plane(width, height, seed):
    """a nearly grey plane whose bins lie in 24 .. 200"""
    rng = np.random.default_rng(seed)
    l = np.exp2(rng.uniform(-12.9, 8.9, (height, width, 1)))
    C = (l * rng.uniform(0.9, 1.1, (height, width, 3))).astype(F)
    b = E.bins(C)
    assert b.min() >= 24 and b.max() <= 200
    return C


@pytest.mark.parametrize("k", (-3, 1, 5))
def test_property_ii_a_power_of_two_shifts_the_keys(k):
    wide = dict(min_exposure=2.0 ** -20, max_exposure=65504.0)                   # (E stays inside its clamp before and after)
    for (width, height), rec, exact in (((64, 32), E.record(flags=E.RESET, low_q16=0, high_q16=65536, **wide), True),      # M = 2048: the division is exact
                                        ((40, 24), E.record(flags=E.RESET, **wide), False), ((17, 9), dict(RECORDS[1], flags=E.RESET, **wide), False)):
        C = inside_plane(width, height, 40 + width)
        scaled = (C * F(2.0 ** k)).astype(F)
        assert (E.bins(scaled) == E.bins(C) + 8 * k).all()
        H0, s0, out0 = E.exposure(C, rec)
        H1, s1, out1 = E.exposure(scaled, rec)
        assert (np.roll(H0, 8 * k) == H1).all()
        shift = float(s1["adapted_key"][0]) - float(s0["adapted_key"][0])
        print(f"k = {k}, {width} x {height}: a_t shifts by {shift!r}")
        assert shift == 8.0 * k if exact else abs(shift - 8.0 * k) <= 4 * np.spacing(float(s0["adapted_key"][0]))
        assert float(s1["luminance"][0]) == float(s0["luminance"][0]) * 2.0 ** k and float(s1["exposure"][0]) == float(s0["exposure"][0]) * 2.0 ** -k
        assert rec["min_exposure"] < float(s0["exposure"][0]) < rec["max_exposure"] and rec["min_exposure"] < float(s1["exposure"][0]) < rec["max_exposure"]
        assert out0.tobytes() == out1.tobytes()


def test_property_iii_a_constant_grey_lands_in_the_middle_of_its_bin():
    for l, ratio in ((1e-4, 1.030), (0.18, 0.998), (1.0, 1.0625), (3.3, 1.023), (1000.0, 0.992)):
        C = np.full((9, 17, 3), l, F)
        lum = float(E.luminance(C)[0, 0])
        s = E.resolve(E.histogram(C, E.record()), E.record())
        got = float(s["luminance"][0]) / l
        print(f"l = {l}: luminance {lum!r}, L = {float(s['luminance'][0])!r}, L / l = {got:.4f}")
        assert abs(float(s["luminance"][0]) / lum - 1.0) <= 1.0 / 16.0
        assert abs(got - ratio) <= 6e-4, (l, got, ratio)


def test_property_iv_n_calls_on_one_frame_move_monotonically():
    C = case(40, 24)
    for rec, start in ((E.record(rate_up=0.125, rate_down=0.5), 700.0), (E.record(rate_up=0.125, rate_down=0.5), 1200.0), (RECORDS[1], 950.0)):
        target = float(E.resolve(E.histogram(C, rec), dict(rec, flags=rec["flags"] | E.RESET))["adapted_key"][0])
        s = a_valid_state(start)
        gaps = [abs(target - start)]
        for n in range(12):
            s = E.resolve(E.histogram(C, rec), rec, s)
            a = float(s["adapted_key"][0])
            assert (start <= a <= target) or (target <= a <= start)
            gaps.append(abs(target - a))
            assert int(s["frames"][0]) == 3 + n + 1
        assert all(g1 <= g0 for g0, g1 in zip(gaps, gaps[1:])) and gaps[-1] < gaps[0] * 0.5, gaps


def test_the_logarithm_is_within_its_bound_on_a_log_normal_plane():
    """L against the float64 geometric mean of a log-normal plane's luminance, the whole histogram as the band.  The bound is derived, not
    measured: the piecewise-linear logarithm is at most 0.0861 octaves off log2 at either end (the mean of the keys, and the key's inverse), and
    L sits in the middle of a bin 1/8 octave wide: 2^(2 * 0.0861 + 1/16) = 1.177.  The measured ratio is printed (DESIGN.md 6w quotes it)"""
    rng = np.random.default_rng(77)
    grey = np.exp(rng.normal(np.log(0.4), 1.5, (72, 136))).astype(F)
    C = np.repeat(grey[..., None], 3, -1)
    rec = E.record(low_q16=0, high_q16=65536)
    s = E.resolve(E.histogram(C, rec), rec)
    lum = E.luminance(C).astype(np.float64)
    gm = float(np.exp(np.log(lum).mean()))
    ratio = float(s["luminance"][0]) / gm
    print(f"log-normal plane: L = {float(s['luminance'][0]):.6f}, geometric mean {gm:.6f}, ratio {ratio:.4f}")
    assert 2.0 ** (2 * 0.0861 + 1.0 / 16.0) == pytest.approx(1.177, abs=5e-4)
    assert 1.0 / 1.177 <= ratio <= 1.177, ratio


# ---- the arbiters against numpy, by bytes ------------------------------------------------------------------------------------------------------------
def arguments(R, rec):
    return R.exposure_arguments(**rec)


@pytest.mark.parametrize("size", SMALL_SIZES + ("second trip",), ids=str)
def test_arbiters_equal_numpy_by_bytes(pkg, size):
    R = pkg.renderer
    width, height = second_trip_size() if size == "second trip" else size
    C = case(width, height)
    for rec0 in RECORDS:
        for w in windows(width, height):
            rec = dict(rec0, window=w)
            what = (width, height, rec["flags"], w)
            H = R.exposure_histogram(C, exposure=arguments(R, rec))
            want_H = E.histogram(C, rec)
            assert H.dtype == np.uint32 and H.tobytes() == want_H.tobytes(), what
            for prev in (None, a_valid_state(700.0), a_valid_state(1100.0)):
                same_state(R.exposure_resolve(H, prev, exposure=arguments(R, rec)), E.resolve(want_H, rec, prev), what)
                same_state(R.exposure_resolve(H, prev, exposure=arguments(R, dict(rec, flags=rec["flags"] | E.RESET))), E.resolve(want_H, dict(rec, flags=rec["flags"] | E.RESET), prev), what)
            e = E.resolve(want_H, rec)["exposure"][0]
            same_out(R.exposure_pixels(C, e), E.apply(C, e), what)


def test_contention_planes_and_the_layout(pkg):
    R = pkg.renderer
    for width, height in ((136, 72), second_trip_size()):
        lay = R.exposure_layout(width, height)
        trip = lay["pixels_per_trip"]
        assert trip % 256 == 0 and lay["groups"] == min(-(-width * height // trip), R.exposure_layout(16384, 16384)["groups"]) and lay["table_bytes"] == lay["groups"] * 1024
        flat = R.exposure_histogram(constant_plane(width, height))
        assert int(flat.max()) == width * height and int((flat != 0).sum()) == 1 and flat.tobytes() == E.histogram(constant_plane(width, height), E.record()).tobytes()
        cyc = cycle_plane(width, height)
        H = R.exposure_histogram(cyc)
        assert H.tobytes() == E.histogram(cyc, E.record()).tobytes() and (H > 0).sum() == min(width, 256) and int(H.max()) - int(H[H > 0].min()) <= height
    w, h = second_trip_size()
    lay = R.exposure_layout(w, h)
    assert w * h > lay["groups"] * lay["pixels_per_trip"] and w * h - lay["groups"] * lay["pixels_per_trip"] < lay["pixels_per_trip"]       # one ragged second trip


def frames_of_a_sequence(width, height):
    """six frames: the plane, four stops down, all black, eight stops up, the plane with NaNs only, the plane"""
    C = case(width, height, seed=1)
    nan = np.full_like(C, np.nan)
    return [C, (C * F(2.0 ** -4)).astype(F), np.zeros_like(C), (C * F(2.0 ** 8)).astype(F), nan, C]


SEQUENCE_FLAGS = (0, 0, 0, E.RESET, 0, 0)


def sequence_reference(width, height, rec0):
    """[(H, state, out)] of the six calls, the state threaded through"""
    s, out = None, []
    for C, extra in zip(frames_of_a_sequence(width, height), SEQUENCE_FLAGS):
        rec = dict(rec0, flags=rec0["flags"] | extra)
        H, s, o = E.exposure(C, rec, s)
        out.append((H, s, o))
    return out


def test_sequences_of_six_calls_state_by_bits(pkg):
    R = pkg.renderer
    for width, height in ((17, 9), (40, 24)):
        for rec0 in RECORDS + (dict(RECORDS[1], window=(1, 1, width - 1, height - 2)),):
            want = sequence_reference(width, height, rec0)
            s = None
            for k, (C, extra) in enumerate(zip(frames_of_a_sequence(width, height), SEQUENCE_FLAGS)):
                rec = dict(rec0, flags=rec0["flags"] | extra)
                H = R.exposure_histogram(C, exposure=arguments(R, rec))
                s = R.exposure_resolve(H, s, exposure=arguments(R, rec))
                assert H.tobytes() == want[k][0].tobytes()
                same_state(s, want[k][1], (width, height, k))
            states = [w[1] for w in want]
            assert len({state_bytes(x) for x in states}) >= 4                    # the frames do move it
            if rec0["flags"] & E.SKIP_BLACK:                                       # the black and the NaN frame measure nothing: a stays, E is the fallback
                assert int(states[2]["metered"][0]) == 0 and states[2]["adapted_key"].tobytes() == states[1]["adapted_key"].tobytes()
                assert float(states[2]["exposure"][0]) == 2.0 and int(states[4]["metered"][0]) == 0


# ---- deliberate defects --------------------------------------------------------------------------------------------------------------------------------
def copy_of_the_reference(C, rec, prev, defect=None):
    """the three steps once more, with one switch per defect; defect=None is the definition (asserted below).  Returns the call's bytes"""
    height, width = C.shape[:2]
    x0, y0, x1, y1 = E.window_of(rec, width, height)
    if defect == "window":
        x1, y1 = min(x1 + 1, width), min(y1 + 1, height)
    W = C[y0:y1, x0:x1]
    with np.errstate(invalid="ignore"):
        keep = (W > 0) | np.isnan(W) if defect == "nan" else W > 0
        x = np.where(keep, np.minimum(W, F(65504.0)), F(0.0)).astype(F)
        if defect == "nan":
            x = np.where(np.isnan(W), W, x)
    if defect == "contracted":
        x64 = x.astype(np.float64)
        inner = (float(F(0.2126)) * x64[..., 0] + (F(0.7152) * x[..., 1]).astype(np.float64)).astype(F)        # fma(0.2126, r, 0.7152 g)
        l = (float(F(0.0722)) * x64[..., 2] + inner.astype(np.float64)).astype(F)                             # fma(0.0722, b, ...)
    else:
        l = (F(0.2126) * x[..., 0] + F(0.7152) * x[..., 1]) + F(0.0722) * x[..., 2]
    key = np.ascontiguousarray(l).view(np.uint32) >> (19 if defect == "shift" else 20)
    H = np.bincount(np.clip(key.astype(np.int64) - 888, 0, 255).ravel(), minlength=256)
    Hc = [int(h) for h in H]
    if rec["flags"] & E.SKIP_BLACK and defect != "black":
        Hc[0] = 0
    N = sum(Hc)
    half = 32768 if defect == "rounded" else 0
    lo, hi = (N * rec["low_q16"] + half) >> 16, (N * rec["high_q16"] + half) >> 16
    if defect == "inclusive":
        hi += 1
    P = M = S = 0
    for b in range(256):
        c = max(0, min(P + Hc[b], hi) - max(P, lo))
        M, S, P = M + c, S + b * c, P + Hc[b]
    was = prev is not None and bool(prev["valid"][0])
    s = E.invalid_state()
    clamp = lambda e: min(max(F(e), F(rec["min_exposure"])), F(rec["max_exposure"]))
    if M == 0:
        if was:
            for name in ("adapted_key", "luminance", "valid", "frames"):
                s[name] = prev[name]
        s["exposure"] = e = clamp(rec["fallback_exposure"])
    else:
        a_t = float(S) / float(M) + (888.0 if defect == "middle" else 888.5)
        if not was or rec["flags"] & E.RESET:
            a, frames = a_t, 1
        else:
            a_prev = float(prev["adapted_key"][0])
            up = a_t > a_prev
            if defect == "rates":
                up = not up
            a = a_prev + (a_t - a_prev) * float(F(rec["rate_up"]) if up else F(rec["rate_down"]))
            frames = int(prev["frames"][0]) + 1
        L = np.array([int(a * 1048576.0)], np.uint32).view(F)[0]
        e = F(rec["key_value"]) / L if defect == "unclamped" else clamp(F(rec["key_value"]) / L)
        s["adapted_key"], s["luminance"], s["exposure"], s["metered"], s["valid"], s["frames"] = a, L, clamp(F(rec["key_value"]) / L), M, 1, frames
    with np.errstate(invalid="ignore", over="ignore"):
        out = (C * F(e)).astype(F)
    return H.astype(np.uint32).tobytes() + state_bytes(s) + out.tobytes()


@functools.lru_cache(maxsize=None)
def an_edge_pixel():
    """a pixel whose luminance lands on a bin's edge when every operation rounds and under it when the sums are fused"""
    rng = np.random.default_rng(5)
    near = (1.0 + rng.integers(-40, 40, (200000, 3)) * 2.0 ** -23).astype(F)
    x64 = near.astype(np.float64)
    plain = E.bins(near)
    inner = (float(F(0.2126)) * x64[:, 0] + (F(0.7152) * near[:, 1]).astype(np.float64)).astype(F)
    fused = E.bin_of((float(F(0.0722)) * x64[:, 2] + inner.astype(np.float64)).astype(F))
    hit = np.flatnonzero(plain != fused)
    assert len(hit), "no pixel found on which contraction changes the bin"
    return near[hit[0]]


def defect_scenarios():
    """(C, record, previous state): planes with NaNs and black pixels, a dark one that drives E into its clamp, an interior window, both records,
    a state on either side of the target, and the pixel on a bin's edge"""
    out = []
    for width, height in ((17, 9), (40, 24)):
        C = case(width, height).copy()
        C[0, :3] = 0.0
        C[1, 1] = an_edge_pixel()
        dark = (case(width, height, seed=2) * F(2.0 ** -12)).astype(F)
        for rec0 in RECORDS:
            for w in ((0, 0, 0, 0), (1, 1, width - 1, height - 2)):
                rec = dict(rec0, window=w)
                out += [(C, rec, None), (C, rec, a_valid_state(700.0)), (C, rec, a_valid_state(1100.0)), (dark, rec, None)]
    edge = np.tile(an_edge_pixel(), (3, 5, 1)).astype(F)
    out.append((edge, E.record(), None))
    return out


def test_the_copy_is_the_reference():
    for C, rec, prev in defect_scenarios():
        H, s, o = E.exposure(C, rec, prev)
        assert copy_of_the_reference(C, rec, prev) == H.tobytes() + state_bytes(s) + o.tobytes()


@pytest.mark.parametrize("defect", ("shift", "middle", "black", "inclusive", "rounded", "rates", "contracted", "nan", "unclamped", "window"))
def test_a_defect_changes_output_bytes(defect):
    changed = sum(copy_of_the_reference(C, rec, prev, defect) != copy_of_the_reference(C, rec, prev) for C, rec, prev in defect_scenarios())
    print(f"{defect}: {changed} of {len(defect_scenarios())} scenarios change")
    assert changed >= 1, defect
