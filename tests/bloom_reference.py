"""NumPy restatement of prosper's bloom, the multi-resolution blur (not a test module), for tests/test_bloom*.py:

  streak_weights(h)                         the streak's weights, float32 (rg, b)
  separate, reduce_level, blur_pass,        res/shader/bloom/{separate,reduce,blur,compose}.comp stage by stage over
  compose                                   arrays
  design(w, h, seed), coverage(...)         the test image and what of the passes it reaches

Everything is float64 and goes through the normalised uv as the GLSL does: a bilinear lookup of an image at uv has the
texel coordinate c = uv * size - 0.5, i = floor(c), f = c - i.  A stage returns its unrounded value `v` and the texel's
sum of absolute terms `s`; the allowance is REL * s (dof_reference.REL, the 2e-4 of tests/test_deferred_shading.py).
"""
import math

import numpy as np

from dof_reference import REL, half, within_half  # noqa: F401  (re-exported for the tests)

# blur.comp:20-25
OFFSETS = (-2.089779143016758, -0.38698196063011614, 1.2004365440663936, 3.0)
WEIGHTS = (0.0666055522709221, 0.6249460483713625, 0.3024686099546741, 0.005979789403041253)
HALF, QUARTER = 0, 1
LEVELS = 4
DEFAULT_BLEND = (0.9, 0.04, 0.04)


def scale_of(resolution_scale):
    return 2 if resolution_scale == HALF else 4


def first_level(resolution_scale):
    return 0 if resolution_scale == HALF else 1


def working_extent(w, h, resolution_scale):
    s = scale_of(resolution_scale)
    return w // s, h // s


def level_extent(ww, wh, l):
    return max(ww >> l, 1), max(wh >> l, 1)


def streak_half_width(ww):
    return max(ww >> 1, 1) // 2


def streak_weights(h):
    """w(i) for i = -h .. h - 1: float32 (rg, b) of the double-precision value from the integer i."""
    rg, b = np.empty(2 * h, np.float32), np.empty(2 * h, np.float32)
    for k in range(2 * h):
        i = float(k - h)
        a = abs(i)
        c = 0.05 if a < 10.0 else 0.01
        wave = abs(math.sin(i * 0.5)) + abs(math.cos(i * 0.95)) + abs(math.sin(i * 0.75))
        fall = 150.0 / max(0.015 * i * i + a, 1.0)
        rg[k] = ((c * 4.0) * wave) * fall
        b[k] = (4.0 * wave) * fall
    return rg, b


def bilinear(img, u, v, edge):
    """The lookup of img [h, w, 3] (float64) at uv arrays: border (0, 0, 0) sampler, or clamp to edge.  Every term is
    non-negative for a non-negative image, so the value is also the sum of absolute terms."""
    h, w = img.shape[:2]
    cx, cy = u * w - 0.5, v * h - 0.5
    ix, iy = np.floor(cx), np.floor(cy)
    fx, fy = cx - ix, cy - iy
    ix, iy = ix.astype(np.int64), iy.astype(np.int64)

    def tex(x, y):
        if edge:
            return img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(inside[..., None], img[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0.0)

    w00, w10 = ((1 - fx) * (1 - fy))[..., None], (fx * (1 - fy))[..., None]
    w01, w11 = ((1 - fx) * fy)[..., None], (fx * fy)[..., None]
    return w00 * tex(ix, iy) + w10 * tex(ix + 1, iy) + w01 * tex(ix, iy + 1) + w11 * tex(ix + 1, iy + 1)


def _grid(w, h):
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return xs, ys


def separate(illum, threshold, resolution_scale):
    """(v, s) of level 0 of the highlights, [wh, ww, 3]."""
    h, w = illum.shape[:2]
    rgb = illum[..., :3].astype(np.float64)
    ww, wh = working_extent(w, h, resolution_scale)
    xs, ys = _grid(ww, wh)
    inv_w, inv_h = 1.0 / w, 1.0 / h
    if resolution_scale == HALF:
        mean = bilinear(rgb, (2 * xs) * inv_w, (2 * ys) * inv_h, edge=False)
    else:
        mean = sum(bilinear(rgb, (4 * xs + dx) * inv_w, (4 * ys + dy) * inv_h, edge=False)
                   for dx, dy in ((-1, -1), (-1, 1), (1, -1), (1, 1))) / 4.0
    t = float(np.float32(threshold))
    return np.maximum(mean - t, 0.0), np.abs(mean) + t


def reduce_level(k, level0_16):
    """Level k (1-3) from the stored level 0: means of four unrounded texels of the level below over virtual texels, the
    source clamped to its edge; cropped to the level's extent.  (v, s)."""
    src = np.asarray(level0_16, np.float16)[..., :3].astype(np.float64)
    wh, ww = src.shape[:2]
    vh, vw = -(-wh // 8) * 8, -(-ww // 8) * 8
    cur = src[np.minimum(np.arange(vh), wh - 1)][:, np.minimum(np.arange(vw), ww - 1)]
    for _ in range(k):
        cur = (((cur[0::2, 0::2] + cur[0::2, 1::2]) + cur[1::2, 0::2]) + cur[1::2, 1::2]) * 0.25
    lw, lh = level_extent(ww, wh, k)
    v = cur[:lh, :lw]
    return v, np.abs(v)


def blur_pass(src16, vertical, streak_level0_16=None):
    """One blur pass over a stored level: (v, s), plus (taps, streak) for the coverage conditions.  With
    `streak_level0_16` (the stored level 0 of the highlights) the horizontal pass of level 1."""
    src = np.asarray(src16, np.float16)[..., :3].astype(np.float64)
    h, w = src.shape[:2]
    xs, ys = _grid(w, h)
    inv_w, inv_h = 1.0 / w, 1.0 / h
    u, v = (xs + 0.5) * inv_w, (ys + 0.5) * inv_h
    taps = np.zeros_like(src)
    for o, wt in zip(OFFSETS, WEIGHTS):
        taps = taps + bilinear(src, u + (0.0 if vertical else o * inv_w), v + (o * inv_h if vertical else 0.0), edge=False) * wt
    streak = np.zeros_like(src)
    if streak_level0_16 is not None:
        assert not vertical
        level0 = np.asarray(streak_level0_16, np.float16)[..., :3].astype(np.float64)
        hw = w // 2
        rg, b = streak_weights(hw)
        for i in range(-hw, hw):
            wt = np.array([rg[i + hw], rg[i + hw], b[i + hw]], np.float64)
            streak = streak + wt * bilinear(level0, u + i * inv_w, v, edge=False)
        streak = streak / (w * 2.0)
    total = taps + streak
    return total, np.abs(total), taps, streak


def compose(illum, levels16, blend, resolution_scale, biquadratic):
    """(v, s) of the output's rgb; levels16: the three images compose reads, levels 0, 1, 2."""
    h, w = illum.shape[:2]
    rgb = illum[..., :3].astype(np.float64)
    xs, ys = _grid(w, h)
    u, v = (xs + 0.5) * (1.0 / w), (ys + 0.5) * (1.0 / h)
    s = scale_of(resolution_scale)
    parts = []
    for l in range(3):
        img = np.asarray(levels16[l], np.float16)[..., :3].astype(np.float64)
        if biquadratic:
            rx, ry = w / (s * 2.0 ** l), h / (s * 2.0 ** l)
            qx, qy = (u * rx) % 1.0, (v * ry) % 1.0
            cx, cy = (qx * (qx - 1.0) + 0.5) / rx, (qy * (qy - 1.0) + 0.5) / ry
            val = (bilinear(img, u - cx, v - cy, True) + bilinear(img, u - cx, v + cy, True) + bilinear(img, u + cx, v + cy, True) +
                   bilinear(img, u + cx, v - cy, True)) / 4.0
        else:
            val = bilinear(img, u, v, True)
        parts.append(val * float(np.float32(blend[l])))
    added = parts[0] + parts[1] + parts[2]
    return rgb + added, np.abs(rgb) + np.abs(added), parts


def chain(illum, threshold, blend, resolution_scale, biquadratic):
    """Every stage one after another with each store rounded to fp16: dict of the working images and the output."""
    first = first_level(resolution_scale)
    hl = [half(separate(illum, threshold, resolution_scale)[0])]
    for k in range(1, LEVELS):
        hl.append(half(reduce_level(k, hl[0])[0]))
    horizontal, blurred, taps, streak = {}, {}, None, None
    for l in range(first, first + 3):
        r = blur_pass(hl[l], False, hl[0] if l == 1 else None)
        if l == 1:
            taps, streak = r[2], r[3]
        horizontal[l] = half(r[0])
        blurred[l] = half(blur_pass(horizontal[l], True)[0])
    read = [blurred[l] if l in blurred else hl[l] for l in range(3)]
    out, _, parts = compose(illum, read, blend, resolution_scale, biquadratic)
    return {"highlights": hl, "horizontal": horizontal, "blurred": blurred, "out": out, "parts": parts,
            "level1_taps": taps, "level1_streak": streak}


# ---- the test image ----

THRESHOLD = 1.0
BRIGHT = 40.0
BAR = 6.0


def design(w, h, seed=11):
    """RGBA32F [h, w, 4], alpha 0.25: a smooth diagonal gradient crossing the threshold, multiplicative noise, single
    bright texels (one well inside, one in each corner, one mid-edge on each side) and a bright vertical bar three
    texels wide."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ramp = 0.35 + 1.5 * (0.65 * xs / max(w - 1, 1) + 0.35 * ys / max(h - 1, 1))
    rgb = ramp[..., None] * np.array([1.0, 0.92, 0.8]) * rng.uniform(0.85, 1.15, (h, w, 3))
    spots = [(h // 3, w // 4), (0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)]
    for y, x in spots:
        rgb[y, x] = BRIGHT * np.array([1.0, 0.5, 0.25])
    bar = (3 * w) // 5
    rgb[:, bar:bar + 3] = BAR * np.array([0.5, 1.0, 0.75])
    out = np.empty((h, w, 4), np.float32)
    out[..., :3] = rgb
    out[..., 3] = 0.25
    return out


def coverage(illum, resolution_scale, biquadratic=True, threshold=THRESHOLD, blend=DEFAULT_BLEND):
    """What the design reaches, from the restatement alone."""
    c = chain(illum, threshold, blend, resolution_scale, biquadratic)
    hl0 = c["highlights"][0][..., :3].astype(np.float64)
    lit = hl0.any(axis=-1)
    beside = np.zeros_like(lit)
    beside[:, 1:] |= lit[:, :-1]
    beside[:, :-1] |= lit[:, 1:]
    beside[1:] |= lit[:-1]
    beside[:-1] |= lit[1:]
    added = sum(c["parts"])
    some = added.sum(axis=-1) > 0
    per_level = [int(((p.sum(axis=-1) >= 0.01 * added.sum(axis=-1)) & some).sum()) for p in c["parts"]]
    return {
        "lit_share": float(lit.mean()),
        "zero_beside_lit": int((~lit & beside).sum()),
        "streak_dominant": int((c["level1_streak"].sum(axis=-1) > c["level1_taps"].sum(axis=-1)).sum()),
        "level1_texels": int(c["level1_taps"].shape[0] * c["level1_taps"].shape[1]),
        "compose_level_pixels": per_level,
    }
