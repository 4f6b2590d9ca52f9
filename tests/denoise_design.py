"""The per-pixel design the denoiser's tests share (a helper, like taa_reference.py's `design`): illumination, G-buffer and
velocity of frame `k` at a given extent, built so that the rule of prosper_amd/denoise.py takes every one of its paths.

    two planes at a depth step (x < 0.45 w: a curved, slanted near plane; beyond: a far plane slanted in y)
    a crease in the normal only (far plane, y >= 0.6 h: same depth, a normal 70 degrees away)
    a sky block (top right), seeded noise, a noiseless dark / bright texture edge on the far plane
    planted NaN / Inf texels that move with the frame, one NaN velocity
    velocity bands: zero, sub-pixel, a whole pixel, out of the image at the left edge, across the depth step, across the crease

tests/test_denoise_cpu.py proves from the statement that every path is reached at 101 x 71."""
import numpy as np

F = np.float32
NEAR, FAR = 0.1, 100.0
C22, C32 = F(NEAR / (FAR - NEAR)), F(FAR * NEAR / (FAR - NEAR))  # cameraToClip[2][2], [3][2] of a reverse-Z projection
FRAMES = 5
EXTENTS = ((1, 1), (3, 2), (17, 9), (101, 71), (130, 33), (33, 130))
FULL = (101, 71)  # the extent at which every path must be reached


def encode_normal(n):
    """signedOctEncode: the inverse of the decode the pass uses, to (x, y, sign) in [0, 1]"""
    o = n / np.abs(n).sum(-1, keepdims=True)
    # the decode forms o.x = ex - ey, o.y = ex + ey - 1
    ex, ey = (o[..., 0] + o[..., 1] + 1.0) * 0.5, (o[..., 1] - o[..., 0] + 1.0) * 0.5
    return ex.astype(np.float32), ey.astype(np.float32), (n[..., 2] >= 0).astype(np.float32)


def design(w, h, k):
    """-> dict of float32 arrays: illumination [h, w, 4], albedo [h, w, 4], normal_metallic [h, w, 4], depth [h, w],
    velocity [h, w, 2]"""
    rng = np.random.default_rng(7000 + 31 * k + w * 1000 + h)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    split, crease = int(0.45 * w), int(0.6 * h)
    near = xs < split
    sky = (xs > 0.8 * w) & (ys < 0.3 * h) & (w > 3)

    z = np.where(near, 2.0 + 0.01 * xs + 0.0005 * xs * xs + 0.003 * ys, 5.0 + 0.02 * ys)
    depth = (float(C32) / z - float(C22)).astype(np.float32)
    depth[sky] = 0.0

    # normals: the near plane's vary smoothly (dot slightly below 1), the far plane faces the camera, beyond the crease it
    # is tilted by 70 degrees (dot 0.34: w_n underflows to 0, and the reprojection's 0.9 rejects it)
    n = np.zeros((h, w, 3))
    n[..., 2] = 1.0
    n[..., 0] = np.where(near, 0.3 * np.sin(xs * 0.31) + 0.002 * ys, 0.0)
    tilt = ~near & (ys >= crease)
    n[tilt] = (np.sin(np.radians(70.0)), 0.0, np.cos(np.radians(70.0)))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    ex, ey, sign = encode_normal(n)
    normal_metallic = np.stack([ex, ey, rng.random((h, w)).astype(np.float32), sign], -1).astype(np.float32)

    # (the albedo belongs to the surface: the same in every frame)
    albedo = (0.2 + 0.6 * np.random.default_rng(w * 1000 + h).random((h, w, 4))).astype(np.float32)
    albedo[((xs + ys) % 7 == 3), 1] = 0.001  # below 1/64: the max

    base = np.where(near, 0.25, np.where(xs < 0.7 * w, 0.05, 1.5))[..., None] * np.array([1.0, 0.8, 0.6])
    noisy = near | (ys < 0.35 * h)  # the far plane's lower part is a noiseless texture edge
    noise = rng.gamma(0.7, 1.0, (h, w, 1)) * np.where(noisy, 1.0, 0.0)[..., None]
    illumination = np.concatenate([base * (np.where(noisy, 0.3, 1.0)[..., None] + noise), rng.random((h, w, 1))], -1).astype(np.float32)
    illumination[sky] = np.concatenate([rng.random((int(sky.sum()), 3)) * 4.0, np.ones((int(sky.sum()), 1))], -1).astype(np.float32)

    def px(shift_x, shift_y):  # the velocity that fetches the history shift texels away: c = px - shift
        return np.array([2.0 * shift_x / w, -2.0 * shift_y / h])

    velocity = np.zeros((h, w, 2))
    velocity[(ys >= 0.75 * h) & near] = px(0.37, -0.21)                   # between four texels
    velocity[(ys >= 0.55 * h) & (ys < 0.75 * h) & near] = px(1.0, 0.0)    # a whole pixel
    velocity[xs < 3] = px(5.0, 0.0)                                       # leaves the image on the left
    velocity[(xs >= split) & (xs < split + 3) & (ys > 0.3 * h)] = px(4.0, 0.0)  # across the depth step
    velocity[~near & (ys >= crease) & (ys < crease + 3) & (xs >= split + 3)] = px(0.0, 4.0)  # across the crease
    velocity = velocity.astype(np.float32)

    if w >= 17 and h >= 9:
        # outliers that move with the frame: a pixel sees them with and without a history
        spots = [(h // 2, w // 4 + k, np.nan), (h // 3, w // 2 + 3 + k, np.inf), (h // 2 + 1, w // 5 + 2 * k, -np.inf), (h - 2, 4 + k, np.nan)]
        for c, (y, x, v) in enumerate(spots):
            illumination[y % h, x % w, c % 3] = v
        velocity[h // 2 + 2, w // 3] = np.nan
    return {"illumination": illumination, "albedo": albedo, "normal_metallic": normal_metallic, "depth": depth, "velocity": velocity}


def inputs(d):
    """the design's arrays in the order of prosper_amd.denoise's stage functions"""
    return d["illumination"], d["albedo"], d["normal_metallic"], d["depth"], d["velocity"]
