"""The edge anti-aliasing filter of include/arctic_hip.h (ARCTIC_OPT_ANTIALIAS, arctic_antialias*) restated in numpy int64, written from the
header's text, not from the kernel.  Every quantity is an integer, so the library is held to it bit for bit.

antialias(img) is the definition.  antialias(img, mutation=name) is the definition with ONE deliberate defect (MUTATIONS): the tests show that
the inputs they feed the GPU tell every such defect from the truth, so a kernel with that defect could not pass them.  make_inputs() is the
input set the CPU and the GPU tests share."""
import numpy as np

K = 12
T_MIN = 4096

# name -> what the defect is (the code below asks `mutation == name` where it applies)
MUTATIONS = {
    "early_exit_gt": "early exit: the pixel goes on only when rng > the threshold (the text: rng >= it)",
    "orientation_gt": "orientation: horizontal iff eh > ev (the text: eh >= ev)",
    "side_gt": "side: a iff ga > gb (the text: ga >= gb)",
    "search_stop_gt": "search: stops when 2 |e| > g (the text: >=)",
    "search_k_plus_1": "search: K + 1 steps",
    "no_subpixel": "no sub-pixel term (off_s = 0)",
    "no_rounding": "blend without the + 128",
    "alpha_blended": "alpha blended like the colours instead of copied",
}


def luma(img):
    c = np.asarray(img).astype(np.int64)
    return 77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2]


def antialias(img, mutation=None, return_edges=False):
    """img: (H, W, 4) uint8 -> (H, W, 4) uint8.  return_edges: also the mask of the pixels past the early exit."""
    assert mutation is None or mutation in MUTATIONS, mutation
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape[:2]
    assert img.shape == (H, W, 4) and H > 0 and W > 0
    C = img.astype(np.int64)
    Y = luma(img)
    ys, xs = np.mgrid[0:H, 0:W]

    def at(a, x, y):   # addressing: clamped per axis
        return a[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]

    M = Y
    N, S, Wl, E = at(Y, xs, ys - 1), at(Y, xs, ys + 1), at(Y, xs - 1, ys), at(Y, xs + 1, ys)
    NW, NE, SW, SE = at(Y, xs - 1, ys - 1), at(Y, xs + 1, ys - 1), at(Y, xs - 1, ys + 1), at(Y, xs + 1, ys + 1)
    # 1. early exit
    hi = np.maximum.reduce([M, N, S, Wl, E])
    lo = np.minimum.reduce([M, N, S, Wl, E])
    rng = hi - lo
    thr = np.maximum(T_MIN, hi >> 3)
    edge = (rng > thr) if mutation == "early_exit_gt" else (rng >= thr)
    # 2. orientation
    eh = np.abs(NW + SW - 2 * Wl) + 2 * np.abs(N + S - 2 * M) + np.abs(NE + SE - 2 * E)
    ev = np.abs(NW + NE - 2 * N) + 2 * np.abs(Wl + E - 2 * M) + np.abs(SW + SE - 2 * S)
    horiz = (eh > ev) if mutation == "orientation_gt" else (eh >= ev)
    # 3. side
    a, b = np.where(horiz, N, Wl), np.where(horiz, S, E)
    ga, gb = np.abs(a - M), np.abs(b - M)
    g = np.maximum(ga, gb)
    side_a = (ga > gb) if mutation == "side_gt" else (ga >= gb)
    step = np.where(side_a, -1, 1)
    nx, ny = np.where(horiz, 0, step), np.where(horiz, step, 0)
    tx, ty = np.where(horiz, 1, 0), np.where(horiz, 0, 1)
    Ls = np.where(side_a, a, b)
    avg2 = M + Ls
    # 4. search
    k = K + 1 if mutation == "search_k_plus_1" else K
    d, e_end = {}, {}
    for s in (-1, 1):
        ds = np.full((H, W), k, np.int64)
        es = np.zeros((H, W), np.int64)
        done = np.zeros((H, W), bool)
        for i in range(1, k + 1):
            qx, qy = np.clip(xs + s * i * tx, 0, W - 1), np.clip(ys + s * i * ty, 0, H - 1)
            e = at(Y, qx, qy) + at(Y, qx + nx, qy + ny) - avg2
            stop = (2 * np.abs(e) > g) if mutation == "search_stop_gt" else (2 * np.abs(e) >= g)
            es = np.where(done, es, e)           # the e of the stopping step, or of step K when none stops
            ds = np.where(~done & stop, i, ds)
            done = done | stop
        d[s], e_end[s] = ds, es
    # 5. edge offset
    span = d[-1] + d[1]
    dmin = np.minimum(d[-1], d[1])
    ee = np.where(d[-1] < d[1], e_end[-1], e_end[1])
    good = (ee < 0) != (M < Ls)
    off_e = np.where(good, (128 * (span - 2 * dmin)) // span, 0)
    # 6. sub-pixel offset
    A = np.abs(2 * (N + S + E + Wl) + NW + NE + SW + SE - 12 * M)
    s1 = np.minimum(256, (256 * A) // np.maximum(12 * rng, 1))   # (rng >= T_MIN wherever the value is used)
    s2 = (s1 * s1 * (768 - 2 * s1)) >> 16
    off_s = (s2 * s2 * 3) >> 10
    if mutation == "no_subpixel":
        off_s = np.zeros_like(off_s)
    # 7. blend
    off = np.minimum(np.maximum(off_e, off_s), 192)[..., None]
    Cn = at(C, xs + nx, ys + ny)
    out = (C * (256 - off) + Cn * off + (0 if mutation == "no_rounding" else 128)) >> 8
    if mutation != "alpha_blended":
        out[..., 3] = C[..., 3]
    out = np.where(edge[..., None], out, C).astype(np.uint8)
    return (out, edge) if return_edges else out


# ---- the inputs the tests share -----------------------------------------------------------------------------------------------------------

def grey(levels, alpha=255):
    """(H, W) grey levels -> RGBA8"""
    l = np.asarray(levels, dtype=np.uint8)
    return np.ascontiguousarray(np.stack([l, l, l, np.full_like(l, alpha)], axis=-1))


def centre_image(side, background, centre):
    l = np.full((side, side), background, np.uint8)
    l[side // 2, side // 2] = centre
    return grey(l)


def threshold_images():
    """rng exactly at / one grey step below T_MIN, and exactly at / one step below hi >> 3"""
    return {"tmin_at": centre_image(5, 100, 116), "tmin_below": centre_image(5, 100, 115),
            "eighth_at": centre_image(5, 175, 200), "eighth_below": centre_image(5, 175, 199)}


def straight_edge(h, w, at, vertical=True, lo=0, hi=200):
    l = np.full((h, w), lo, np.uint8)
    if vertical:
        l[:, at:] = hi
    else:
        l[at:, :] = hi
    return grey(l)


def staircase_12x40():
    l = np.zeros((12, 40), np.uint8)
    l[:6] = 200
    l[6, :20] = 200
    return grey(l)


def staircases(h, w, transpose=False):
    """a boundary that climbs one pixel after runs of 1, 2, ... 30 pixels, bright above it"""
    edge_y, y, run, left = np.empty(w, np.int64), h - 3, 1, 1
    for x in range(w):
        edge_y[x] = max(y, 2)
        left -= 1
        if left == 0:
            y -= 1
            run = run % 30 + 1
            left = run
    l = np.where(np.arange(h)[:, None] < edge_y[None, :], 210, 25).astype(np.uint8)
    img = grey(l)
    img[..., 2] = 255 - img[..., 2]   # not grey: the channels blend separately
    return np.ascontiguousarray(img.transpose(1, 0, 2)) if transpose else img


def polygons(h, w, seed=5):
    """half-planes of slope 2/7 and 9/4 and a disc over a dim gradient, with varied alpha"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 0] = 20 + (x * 20) // max(w - 1, 1)
    img[..., 1] = 30
    img[..., 2] = 25 + (y * 20) // max(h - 1, 1)
    img[7 * (y - h // 3) > 2 * x] = (200, 180, 40, 0)                 # slope 2/7
    img[4 * (y - h) > -9 * (x - w // 4)] = (30, 90, 220, 0)           # slope 9/4
    r = min(h, w) // 4
    img[(x - (2 * w) // 3) ** 2 + (y - h // 2) ** 2 <= r * r] = (250, 250, 245, 0)
    img[..., 3] = rs.randint(0, 256, (h, w))
    return img


def stripes(h, w, vertical=True):
    l = np.zeros((h, w), np.uint8)
    if vertical:
        l[:, ::2] = 220
    else:
        l[::2, :] = 220
    return grey(l, alpha=7)


def random_images(h=70, w=130, seed=11):
    rs = np.random.RandomState(seed)
    uniform = rs.randint(0, 256, (h, w, 4)).astype(np.uint8)
    palette = np.array([0, 64, 128, 255], np.uint8)[rs.randint(0, 4, (h, w, 4))]
    levels = grey(np.array([0, 16, 32, 48], np.uint8)[rs.randint(0, 4, (h, w))])
    levels[..., 3] = rs.randint(0, 256, (h, w))
    return {"random": uniform, "palette": palette, "grey_levels": levels}


def make_inputs(tile_w, tile_h):
    """name -> image: the input set of the GPU test (tests/test_gpu_antialias.py), for a kernel whose workgroup covers tile_w x tile_h pixels"""
    rs = np.random.RandomState(3)
    inputs = dict(random_images())
    inputs.update(threshold_images())
    for h, w in ((1, 1), (1, 40), (40, 1), (2, 2), (33, 65)):
        inputs[f"random_{w}x{h}"] = rs.randint(0, 256, (h, w, 4)).astype(np.uint8)
        inputs[f"palette_{w}x{h}"] = np.array([0, 64, 128, 255], np.uint8)[rs.randint(0, 4, (h, w, 4))]
    inputs["constant"] = np.full((33, 65, 4), 137, np.uint8)
    inputs["stripes_v"], inputs["stripes_h"] = stripes(33, 65), stripes(33, 65, vertical=False)
    inputs["spike_9x9"] = centre_image(9, 30, 255)
    inputs["edge_9x16"] = straight_edge(9, 16, 8)
    inputs["staircase_12x40"] = staircase_12x40()
    # one exact multiple of the tile; three tiles and a ragged remainder per axis (searches cross tile borders both ways)
    inputs["tile_multiple"] = np.array([0, 64, 128, 255], np.uint8)[rs.randint(0, 4, (2 * tile_h, 2 * tile_w, 4))]
    inputs["polygons"] = polygons(3 * tile_h + 5, 3 * tile_w + 7)
    inputs["palette_tiles"] = np.array([0, 64, 128, 255], np.uint8)[rs.randint(0, 4, (3 * tile_h + 3, 3 * tile_w + 1, 4))]
    inputs["edge_300_v"] = straight_edge(300, 9, 4)
    inputs["edge_300_h"] = straight_edge(9, 300, 4, vertical=False, lo=180, hi=10)
    inputs["staircases"] = staircases(40, 500)
    inputs["staircases_t"] = staircases(40, 500, transpose=True)
    return inputs
