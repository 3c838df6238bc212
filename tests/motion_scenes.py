"""Analytic frames for the accumulation's motion form: ao_history_scenes' floor, wall and box, with the BOX translated a step further along +z in
every call -- its front face moves along its own normal towards the camera by more than the history's plane_dist per call -- and the prev_world4
plane that belongs to every frame, made in numpy: a box pixel's surface point lay one step back at the previous call, every other surface stood
still.  A few entries of every plane are flags 0 and 1 and positions that are not finite, so that every rule of the definition is met.  The CPU
tests (numpy against the host arbiter) and the device tests (against k_ao_accumulate_motion, the G-buffers injected with arctic_write_gbuffer and
the planes uploaded) judge the same inputs."""
import numpy as np

import ao_history_reference as HR
import ao_history_scenes as HS

F = np.float32
STEP = 0.08                   # the box's step per call along +z: above HR.HIST's plane_dist of 0.05
CAMERAS = ["still", "translated"]
N_CALLS = 5
_cache = {}


def gbuffer(pkg, cam, W, H, shift):
    """ao_history_scenes.gbuffer with the box `shift` further along +z"""
    lo, hi = HS.BOX
    kept = HS.BOX
    HS.BOX = ((lo[0], lo[1], lo[2] + shift), (hi[0], hi[1], hi[2] + shift))   # (the module's constant for the duration of one call; its own cases are cached by name)
    try:
        return HS.gbuffer(pkg, cam, W, H)
    finally:
        HS.BOX = kept


def on_box(attrs):
    """the pixels of the box: its stored normals are the only ones of length 3"""
    n = attrs[..., 8:11]
    return np.abs(n).sum(-1) == F(3.0)


def on_front_face(attrs):
    return attrs[..., 10] == F(3.0)


def motion_plane(attrs, material, k, seed, odd=True):
    """prev_world4 of call k: zeros at the first call (M is empty) and where there is no geometry; else {w - the box's step, 2} on the box and
    {w, 2} elsewhere; then the odd entries"""
    H, W = material.shape
    pw4 = np.zeros((H, W, 4), F)
    if k == 0:
        return pw4
    geometry = material != HR.NO_MATERIAL
    w = attrs[..., 11:14].copy()
    w[on_box(attrs), 2] -= F(STEP)
    pw4[geometry, :3], pw4[geometry, 3] = w[geometry], F(2.0)
    if not odd:
        return pw4
    rng = np.random.default_rng([seed, W, H, k])
    px = rng.choice(np.nonzero(geometry.reshape(-1))[0], 60, replace=False)
    flat = pw4.reshape(-1, 4)
    flat[px[:15], 3] = F(1.0)                                                    # the point alone: as good as 2 for the accumulation
    flat[px[15:25], 3] = F(0.0)                                                  # a flag below 1, whatever the point: reject everything
    flat[px[25:30]] = 0.0                                                        # no previous, as k_motion writes it
    flat[px[30:40], 3] = np.nan                                                  # not "at least 1"
    flat[px[40:50], 0] = np.nan                                                  # a point that projects to nothing
    flat[px[50:], 1] = np.inf
    return pw4


def case(pkg, camera, W, H, n=N_CALLS, odd=True):
    """-> dict(frames [(attrs, material, P)], motions [prev_world4], descs, planes): the inputs of n calls; odd=False: planes without the odd entries"""
    key = (camera, W, H, n, odd)
    if key not in _cache:
        cams = HS.cameras(camera, n, W / H)
        frames = [gbuffer(pkg, c, W, H, STEP * k) for k, c in enumerate(cams)]
        motions = [motion_plane(a, m, k, CAMERAS.index(camera), odd) for k, (a, m, _) in enumerate(frames)]
        _cache[key] = dict(frames=frames, motions=motions, descs=[HS.desc_of(pkg, c) for c in cams], planes=HS.current_planes(W, H, n, 11 + CAMERAS.index(camera)))
    return _cache[key]


def taps_on_front_face(c, k):
    """the front-face pixels of call k (k >= 1) whose four taps, through call k - 1's matrix, lay on the front face in call k - 1"""
    attrs, material, _ = c["frames"][k]
    prev_attrs, _, prev_P = c["frames"][k - 1]
    H, W = material.shape
    pw = c["motions"][k].reshape(-1, 4)
    inside, _, ix, iy, _, _ = HR.reproject(prev_P, pw[:, :3], W, H)
    face_now, face_then = on_front_face(attrs).reshape(-1), on_front_face(prev_attrs)
    ok = face_now & inside & (pw[:, 3] >= 1)
    with np.errstate(invalid="ignore"):
        x0, y0 = np.where(ok, ix, 0).astype(np.int32), np.where(ok, iy, 0).astype(np.int32)
    for t in range(4):
        qx, qy = x0 + (t & 1), y0 + (t >> 1)
        inb = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
        ok &= inb & face_then[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)]
    return ok.reshape(H, W)
