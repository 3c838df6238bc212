"""Auto-exposure in numpy, written from the definition in include/arctic_hip.h (in front of arctic_exposure_device), not from the C++: the
meter (a 256-bin histogram of the float's own bits), the resolve (a percentile band, the binary64 adaptation, the exposure E) and the apply
(one multiply).  fp32 operations are numpy float32 operations, one rounding each in the written order; the binary64 part is python's float; the
counts are python's integers."""
import numpy as np

F = np.float32
SOURCE_COMPOSED, SOURCE_TAA, SOURCE_MOTION_BLUR, SOURCE_DOF, SOURCE_BLOOM = 1, 2, 4, 8, 16
SKIP_BLACK, RESET, HOLD, METER_ONLY = 32, 64, 128, 256
STATE_DTYPE = np.dtype([("adapted_key", "<f8"), ("exposure", "<f4"), ("luminance", "<f4"), ("metered", "<u4"), ("valid", "<u4"), ("frames", "<u4"), ("reserved", "<u4")])
DEFAULTS = dict(flags=0, low_q16=32768, high_q16=62259, key_value=0.18, min_exposure=1.0 / 1024.0, max_exposure=1024.0, rate_up=1.0, rate_down=1.0, fallback_exposure=1.0,
                window=(0, 0, 0, 0))


def record(**kw):
    """the parameters of one call, every field present"""
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def luminance(C):
    """step 1's l of every pixel of C (..., 3)"""
    C = np.asarray(C, F)
    with np.errstate(invalid="ignore"):
        x = np.where(C > 0, np.minimum(C, F(65504.0)), F(0.0)).astype(F)      # a NaN fails the test
    return (F(0.2126) * x[..., 0] + F(0.7152) * x[..., 1]) + F(0.0722) * x[..., 2]


def bin_of(l):
    """the bin of a luminance (float32, sign 0)"""
    l = np.asarray(l, F)
    key = np.ascontiguousarray(l).view(np.uint32).reshape(l.shape) >> 20
    return np.clip(key.astype(np.int64) - 888, 0, 255)


def bins(C):
    """step 1's bin of every pixel"""
    return bin_of(luminance(C))


def window_of(rec, width, height):
    x0, y0, x1, y1 = (int(v) for v in rec["window"])
    return (0, 0, width, height) if (x0, y0, x1, y1) == (0, 0, 0, 0) else (x0, y0, x1, y1)


def histogram(C, rec):
    """H of the frame C (height, width, 3) under the record's window: (256,) uint32"""
    height, width = C.shape[:2]
    x0, y0, x1, y1 = window_of(rec, width, height)
    return np.bincount(bins(C[y0:y1, x0:x1]).ravel(), minlength=256).astype(np.uint32)


def invalid_state():
    return np.zeros(1, STATE_DTYPE)


def clamp_exposure(rec, e):
    return min(max(F(e), F(rec["min_exposure"])), F(rec["max_exposure"]))


def band(H, rec):
    """(M, S) of step 2"""
    Hc = [int(h) for h in H]
    if rec["flags"] & SKIP_BLACK:
        Hc[0] = 0
    N = sum(Hc)
    lo, hi = (N * int(rec["low_q16"])) >> 16, (N * int(rec["high_q16"])) >> 16
    P, M, S = 0, 0, 0
    for b in range(256):
        c = max(0, min(P + Hc[b], hi) - max(P, lo))
        M += c
        S += b * c
        P += Hc[b]
    return M, S


def resolve(H, rec, prev=None):
    """the state behind a metering call: H (256,), the record, the state in front of the call (None: invalid)"""
    prev = invalid_state() if prev is None else prev
    was = bool(prev["valid"][0])
    out = invalid_state()
    M, S = band(H, rec)
    if M == 0:
        if was:
            for name in ("adapted_key", "luminance", "valid", "frames"):
                out[name] = prev[name]
        out["exposure"] = clamp_exposure(rec, rec["fallback_exposure"])
        return out
    a_t = float(S) / float(M) + 888.5
    if not was or rec["flags"] & RESET:
        a, frames = a_t, 1
    else:
        a_prev = float(prev["adapted_key"][0])
        rate = F(rec["rate_up"]) if a_t > a_prev else F(rec["rate_down"])
        step = (a_t - a_prev) * float(rate)
        a = a_prev + step
        frames = (int(prev["frames"][0]) + 1) & 0xFFFFFFFF
    L = np.array([int(a * 1048576.0)], np.uint32).view(F)[0]
    out["adapted_key"], out["luminance"], out["exposure"] = a, L, clamp_exposure(rec, F(rec["key_value"]) / L)
    out["metered"], out["valid"], out["frames"] = min(M, 0xFFFFFFFF), 1, frames
    return out


def apply(C, e):
    """step 3's out"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(C, F) * F(e)).astype(F)


def exposure(C, rec, prev=None):
    """one call on the frame C: (H, state, out).  HOLD: (None, prev, out under prev's E); METER_ONLY: out is None"""
    if rec["flags"] & HOLD:
        return None, prev, apply(C, prev["exposure"][0])
    H = histogram(C, rec)
    state = resolve(H, rec, prev)
    return H, state, (None if rec["flags"] & METER_ONLY else apply(C, state["exposure"][0]))
