"""NumPy restatement of prosper's temporal anti-aliasing resolve (not a test module), for tests/test_taa*.py:

  halton23(), jitter(index, w, h)            the jitter cycle and Camera::perspective's jitter, float32
  specialization_index(...)                  TemporalAntiAliasing.cpp:50-65
  resolve(illum, velocity, depth, history16, variant)
                                             res/shader/taa_resolve.comp over arrays: per texel the
                                             unrounded value, its allowance and what the texel went through
  design(w, h, frame), coverage(...)         the per-pixel test inputs and what of the pass they reach

Coordinates and every discrete choice - the sampled velocity, the reprojected uv and its range test, the footprint i and
the fraction f, the Catmull-Rom weights - are computed in np.float32, operation for operation as the header states them,
so the restatement and the kernel pick the same texels, fractions and branches.  Colour arithmetic is float64.

The allowance is REL (dof_reference.REL, the 2e-4 of tests/test_deferred_shading.py) of the sum of absolute terms of
each stage, carried on:
  history lookup   a_P = REL * sum |weight| |texel| (over |sum of the weights| for Catmull-Rom)
  clamp            clamp(x, lo, hi) moves by at most the largest move of its three arguments: a_C = max(a_P, a_lo, a_hi).
                   MinMax: the bounds are input texels, a_lo = a_hi = 0.  Variance: mu has REL * sum |c| / 9; the variance
                   m2 / 9 - mu mu has a_var = REL * (m2 / 9 + (sum |c| / 9)^2), and sigma is carried as the interval
                   sqrt(max(var -/+ a_var, 0)), so a_lo = a_hi = REL * (sum |c| / 9 + sigma) + the interval's half width
  blend            r = (I cw + C hw) / W: REL * (|I| cw + |C| hw) / W, plus what a_C does to r to first order:
                   (hw / W) a_C and, with luminance weighting where hw = .9 / (1 + L(C)),
                   cw hw / ((1 + L) W^2) |C - I| a_L with a_L = .299 a_Cr + .587 a_Cg + .114 a_Cb
A texel that falls back to the illumination (history ignored, or reprojected outside) has allowance 0.
"""
import numpy as np

from dof_reference import REL, half, within_half  # noqa: F401  (re-exported for the tests)

F = np.float32
NONE, MIN_MAX, VARIANCE = 0, 1, 2
CENTER, LARGEST, CLOSEST = 0, 1, 2
DEFAULT = (1, VARIANCE, CLOSEST, 1)  # catmullRom, colorClipping, velocitySampling, luminanceWeighting
CHEAPEST = (0, NONE, CENTER, 0)
VARIANTS = [(cr, clip, vel, lw) for cr in (0, 1) for clip in (NONE, MIN_MAX, VARIANCE) for vel in (CENTER, LARGEST, CLOSEST)
            for lw in (0, 1)]
LUMA = (0.299, 0.587, 0.114)


def halton(index, base):
    f, r = 1.0, 0.0
    while index > 0:
        f /= base
        r += f * (index % base)
        index //= base
    return r


def halton23():
    """The 8-sample cycle: samples 1 .. 8 of the base-2 and base-3 radical inverses, float32 [8, 2]."""
    return np.array([[halton(i, 2), halton(i, 3)] for i in range(1, 9)], np.float32)


def jitter(index, w, h):
    s = halton23()[index % 8]
    return (s * F(2) - F(1)) / np.array([w, h], np.float32)


def specialization_index(ignore_history, catmull_rom, clipping, sampling, luminance_weighting):
    return ignore_history | (catmull_rom << 1) | (clipping << 2) | (sampling << 4) | (luminance_weighting << 6)


def _grid(w, h):
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return xs, ys


def _at(img, xs, ys):
    h, w = img.shape[:2]
    return img[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)]


OFFSETS = [(ox, oy) for ox in (-1, 0, 1) for oy in (-1, 0, 1)]  # x outer, y inner


def sample_velocity(velocity, depth, sampling):
    """float32 [h, w, 2], and per texel how many neighbours share the winning length / depth (ties)."""
    vel = np.asarray(velocity, F)
    h, w = vel.shape[:2]
    xs, ys = _grid(w, h)
    if sampling == CENTER:
        return vel.copy(), np.ones((h, w), np.int64)
    if sampling == LARGEST:
        best, ret = np.zeros((h, w), F), np.zeros((h, w, 2), F)
        lens = []
        for ox, oy in OFFSETS:
            v = _at(vel, xs + ox, ys + oy)
            length = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]
            lens.append(length)
            take = best < length
            ret = np.where(take[..., None], v, ret)
            best = np.where(take, length, best)
        return ret, sum((l == best).astype(np.int64) for l in lens)
    dep = np.asarray(depth, F)
    closest, cx, cy = np.zeros((h, w), F), np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    deps = []
    for ox, oy in OFFSETS:
        d = _at(dep, xs + ox, ys + oy)
        deps.append(d)
        take = d > closest
        closest = np.where(take, d, closest)
        cx, cy = np.where(take, ox, cx), np.where(take, oy, cy)
    return _at(vel, xs + cx, ys + cy), sum((d == closest).astype(np.int64) for d in deps)


def saturate32(x):
    return np.fmin(np.fmax(np.asarray(x, F), F(0)), F(1))


def reproject(vel, w, h):
    """float32: (ru, rv), inside, (ix, iy) int64, (fx, fy)."""
    xs, ys = _grid(w, h)
    rx, ry = F(w), F(h)
    u, v = (xs.astype(F) + F(0.5)) / rx, (ys.astype(F) + F(0.5)) / ry
    ru, rv = u - vel[..., 0] * F(0.5), v - vel[..., 1] * F(-0.5)
    with np.errstate(invalid="ignore"):
        inside = (ru == saturate32(ru)) & (rv == saturate32(rv))
    sru, srv = np.where(inside, ru, F(0.5)), np.where(inside, rv, F(0.5))
    cx, cy = sru * rx - F(0.5), srv * ry - F(0.5)
    wx, wy = np.floor(cx), np.floor(cy)
    return (ru, rv), inside, (wx.astype(np.int64), wy.astype(np.int64)), (cx - wx, cy - wy)


def catmull_axis(f):
    """(w0, w12, w3, t) in float32, taa_resolve.comp:95-107 with c = 70 / 100."""
    f = np.asarray(f, F)
    c = F(70.0) / F(100.0)
    k2c, k2mc, k3mc, k3m2c = F(2) * c, F(2) - c, F(3) - c, F(3) - F(2) * c
    f2 = f * f
    f3 = f * f2
    w0 = (-c * f3 + k2c * f2) - c * f
    w1 = (k2mc * f3 - k3mc * f2) + F(1)
    w2 = (-k2mc * f3 + k3m2c * f2) + c * f
    w3 = c * f3 - c * f2
    w12 = w1 + w2
    return w0, w12, w3, w2 / w12


def _mix(a, b, t):
    """(value, sum of absolute terms) of (1 - t) a + t b."""
    t = t.astype(np.float64)[..., None]
    return (1 - t) * a + t * b, np.abs(1 - t) * np.abs(a) + np.abs(t) * np.abs(b)


def _bilinear(hist, ix, iy, fx, fy):
    fx, fy = fx.astype(np.float64)[..., None], fy.astype(np.float64)[..., None]
    t = [_at(hist, ix + dx, iy + dy) for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1))]
    wts = [(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy]
    return sum(wt * x for wt, x in zip(wts, t)), sum(np.abs(wt) * np.abs(x) for wt, x in zip(wts, t))


def history_lookup(history16, ix, iy, fx, fy, catmull_rom):
    """(P, S): the previous resolve at the footprint and its sum of absolute terms, float64 [h, w, 3]."""
    hist = np.asarray(history16, np.float16)[..., :3].astype(np.float64)
    if not catmull_rom:
        return _bilinear(hist, ix, iy, fx, fy)
    x0, x12, x3, tx = catmull_axis(fx)
    y0, y12, y3, ty = catmull_axis(fy)
    taps = [_mix(_at(hist, ix, iy - 1), _at(hist, ix + 1, iy - 1), tx), _mix(_at(hist, ix - 1, iy), _at(hist, ix - 1, iy + 1), ty),
            _bilinear(hist, ix, iy, tx, ty), _mix(_at(hist, ix + 2, iy), _at(hist, ix + 2, iy + 1), ty),
            _mix(_at(hist, ix, iy + 2), _at(hist, ix + 1, iy + 2), tx)]
    ks = [(a * b).astype(np.float64)[..., None] for a, b in ((x12, y0), (x0, y12), (x12, y12), (x3, y12), (x12, y3))]
    total = sum(ks)
    return sum(k * t[0] for k, t in zip(ks, taps)) / total, sum(np.abs(k) * t[1] for k, t in zip(ks, taps)) / np.abs(total)


def neighbourhood(illum):
    """The nine clamped neighbours of every texel, float64 [9, h, w, 3]."""
    rgb = np.asarray(illum, F)[..., :3].astype(np.float64)
    h, w = rgb.shape[:2]
    xs, ys = _grid(w, h)
    return np.stack([_at(rgb, xs + ox, ys + oy) for ox, oy in OFFSETS])


def clip_bounds(illum, clipping):
    """(lo, hi, a): the bounds of clipColor and their allowance."""
    n = neighbourhood(illum)
    if clipping == MIN_MAX:
        return np.minimum(n.min(axis=0), 9999.0), np.maximum(n.max(axis=0), -9999.0), np.zeros(n.shape[1:])
    m2, s_mu = (n * n).sum(axis=0) / 9.0, np.abs(n).sum(axis=0) / 9.0
    mu = n.sum(axis=0) / 9.0
    var = m2 - mu * mu
    a_var = REL * (m2 + s_mu * s_mu)
    sigma = np.sqrt(np.maximum(var, 0.0))
    s_lo, s_hi = np.sqrt(np.maximum(var - a_var, 0.0)), np.sqrt(np.maximum(var + a_var, 0.0))
    a = REL * (s_mu + sigma) + np.maximum(s_hi - sigma, sigma - s_lo)
    return mu - sigma, mu + sigma, a


def luminance(c):
    return LUMA[0] * c[..., 0] + LUMA[1] * c[..., 1] + LUMA[2] * c[..., 2]


def resolve(illum, velocity, depth, history16, variant):
    """taa_resolve.comp over [h, w] arrays; history16 None: IGNORE_HISTORY.  A dict: `v`, `a` (float64 [h, w, 3]), and
    for the coverage `inside`, `velocity`, `ties`, `ru`, `rv`, `previous`, `lo`, `hi`, `history_luminance`."""
    catmull_rom, clipping, sampling, luminance_weighting = variant
    rgb = np.asarray(illum, F)[..., :3].astype(np.float64)
    h, w = rgb.shape[:2]
    if history16 is None:
        return {"v": rgb, "a": np.zeros_like(rgb), "inside": np.zeros((h, w), bool)}
    vel, ties = sample_velocity(velocity, depth, sampling)
    (ru, rv), inside, (ix, iy), (fx, fy) = reproject(vel, w, h)
    P, S = history_lookup(history16, ix, iy, fx, fy, catmull_rom)
    a_P = REL * S
    out = {"inside": inside, "velocity": vel, "ties": ties, "ru": ru, "rv": rv, "previous": P}
    if clipping == NONE:
        C, a_C = P, a_P
    else:
        lo, hi, a_b = clip_bounds(illum, clipping)
        C, a_C = np.minimum(np.maximum(P, lo), hi), np.maximum(a_P, a_b)
        out.update(lo=lo, hi=hi)
    cw = np.full((h, w), float(F(0.1)))
    hw = np.full((h, w), float(F(1) - F(0.1)))
    sensitivity = np.zeros_like(rgb)
    if luminance_weighting:
        lh = luminance(C)
        cw = cw * (1.0 / (1.0 + luminance(rgb)))
        hw = hw * (1.0 / (1.0 + lh))
        a_L = luminance(a_C)
        out["history_luminance"] = lh
    W = np.maximum(cw + hw, float(F(0.00001)))
    if luminance_weighting:
        sensitivity = (np.abs(cw * hw / ((1.0 + lh) * W * W)) * a_L)[..., None] * np.abs(C - rgb)
    cw, hw, W = cw[..., None], hw[..., None], W[..., None]
    r = (rgb * cw + C * hw) / W
    a_r = REL * (np.abs(rgb) * np.abs(cw) + np.abs(C) * np.abs(hw)) / W + np.abs(hw / W) * a_C + sensitivity
    keep = inside[..., None]
    out.update(v=np.where(keep, r, rgb), a=np.where(keep, a_r, 0.0))
    return out


# ---- the test inputs ----

SEED = 23
VELOCITY_BLOCK, DEPTH_BLOCK, FACTOR_BLOCK = 4, 5, 6
(V_ZERO, V_SUB_PIXEL, V_WHOLE_PIXELS, V_LANDS_ON_EDGE_X, V_LANDS_ON_EDGE_Y, V_STEP_OUTSIDE_X, V_STEP_OUTSIDE_Y, V_PLUS_ONE, V_MINUS_ONE,
 V_EQUAL_LENGTHS) = range(10)
VELOCITY_KINDS = 10
D_ZERO, D_EQUAL, D_RANDOM, D_MIXED = range(4)
# per block and frame; None: a flat block.  (Neighbouring blocks differ by a factor of 6 at the most: Catmull-Rom's negative
# lobes, about -0.2 of the neighbours in all, then leave the history's luminance well above -1, the pole of the
# luminance weight 1 / (1 + L), under every variant: tests/test_taa_cpu.py asserts it.)
FACTORS = (1.0, 3.0, 1.0, 0.5, None, 1.0)


def _kinds(w, h, block, step, count, frame):
    xs, ys = _grid(w, h)
    return (xs // block + step * (ys // block) + frame) % count


def velocity_kinds(w, h, frame):
    return _kinds(w, h, VELOCITY_BLOCK, 3, VELOCITY_KINDS, frame)


def depth_kinds(w, h, frame):
    return _kinds(w, h, DEPTH_BLOCK, 2, 4, frame)


def factor_kinds(w, h, frame):
    return _kinds(w, h, FACTOR_BLOCK, 2, len(FACTORS), frame)


def design(w, h, frame=0, seed=SEED):
    """(illumination RGBA32F [h, w, 4], velocity float32 [h, w, 2], depth float32 [h, w]) of one frame.

    Velocity, in blocks of 4 x 4 texels whose kind moves on with the frame: zero; a sub-pixel shift; whole pixels; landing
    exactly on uv.x (or uv.y) = 0 from the lower half of the axis and = 1 from the upper half; the same one float32 step
    further, outside; (1, 1); (-1, -1); and texels of equal length and different direction.  Depth, in blocks of 5 x 5:
    all zero, all equal, random, and random with zeros.  Illumination: a ramp with multiplicative noise, drawn afresh
    every frame, times a factor per 6 x 6 block that moves on with the frame (1, 3, 1, 0.5, a flat block, 1), so the
    previous frame's block is an outlier above or below this frame's neighbourhood; alpha 0.25."""
    rng = np.random.default_rng(seed + 1000 * frame)
    xs, ys = _grid(w, h)
    rx, ry = F(w), F(h)
    u, v = (xs.astype(F) + F(0.5)) / rx, (ys.astype(F) + F(0.5)) / ry
    kinds = velocity_kinds(w, h, frame)
    vel = np.zeros((h, w, 2), F)

    def put(kind, vx, vy):
        m = kinds == kind
        vel[..., 0] = np.where(m, np.asarray(vx, F), vel[..., 0])
        vel[..., 1] = np.where(m, np.asarray(vy, F), vel[..., 1])

    # reprojectedUv = uv - velocity * (.5, -.5): x lands on 0 with 2 u and on 1 with -2 (1 - u), y with the signs swapped
    low_x, low_y = u <= F(0.5), v <= F(0.5)
    edge_x = np.where(low_x, F(2) * u, -(F(2) * (F(1) - u)))
    edge_y = np.where(low_y, -(F(2) * v), F(2) * (F(1) - v))
    out_x = np.where(low_x, np.nextafter(edge_x, F(np.inf)), np.nextafter(edge_x, F(-np.inf)))
    out_y = np.where(low_y, np.nextafter(edge_y, F(-np.inf)), np.nextafter(edge_y, F(np.inf)))
    put(V_SUB_PIXEL, F(2 * 0.37) / rx, F(-2 * 0.41) / ry)
    put(V_WHOLE_PIXELS, F(2 * 2) / rx, F(-2 * 1) / ry)
    put(V_LANDS_ON_EDGE_X, edge_x, 0)
    put(V_LANDS_ON_EDGE_Y, 0, edge_y)
    put(V_STEP_OUTSIDE_X, out_x, 0)
    put(V_STEP_OUTSIDE_Y, 0, out_y)
    put(V_PLUS_ONE, 1, 1)
    put(V_MINUS_ONE, -1, -1)
    a, b = F(2 * 0.45) / rx, F(2 * 0.2) / rx
    which = (xs + ys) % 3
    put(V_EQUAL_LENGTHS, np.where(which == 0, a, np.where(which == 1, b, -a)), np.where(which == 0, b, np.where(which == 1, a, b)))

    dk = depth_kinds(w, h, frame)
    random_depth = rng.uniform(0.05, 0.95, (h, w)).astype(F)
    depth = np.where(dk == D_ZERO, F(0), np.where(dk == D_EQUAL, F(0.5), random_depth)).astype(F)
    depth = np.where((dk == D_MIXED) & ((xs + 2 * ys) % 3 != 0), F(0), depth).astype(F)

    ramp = 0.4 + 1.6 * (0.6 * xs / max(w - 1, 1) + 0.4 * ys / max(h - 1, 1))
    rgb = ramp[..., None] * np.array([1.0, 0.9, 0.75]) * rng.uniform(0.8, 1.2, (h, w, 3))
    fk = factor_kinds(w, h, frame)
    for k, factor in enumerate(FACTORS):
        if factor is None:
            rgb = np.where((fk == k)[..., None], np.array([0.7, 1.1, 0.9]) * (1.0 + 0.5 * frame), rgb)
        else:
            rgb = np.where((fk == k)[..., None], rgb * factor, rgb)
    illum = np.empty((h, w, 4), F)
    illum[..., :3] = rgb
    illum[..., 3] = 0.25
    return illum, vel, depth


def coverage(w, h, frame, history16, variant):
    """How many texels of each kind frame `frame` of the design holds under `variant`, from the restatement alone."""
    illum, vel, depth = design(w, h, frame)
    r = resolve(illum, vel, depth, history16, variant)
    kinds = velocity_kinds(w, h, frame)
    centre = resolve(illum, vel, depth, history16, (variant[0], variant[1], CENTER, variant[3]))
    inside, ru, rv = centre["inside"], centre["ru"], centre["rv"]
    n = neighbourhood(illum)
    flat = (n.min(axis=0) == n.max(axis=0)).all(axis=-1)
    xs, ys = _grid(w, h)
    dn = np.stack([_at(depth, xs + ox, ys + oy) for ox, oy in OFFSETS])
    lo, hi, _ = clip_bounds(illum, MIN_MAX)
    largest = sample_velocity(vel, depth, LARGEST)
    P = r["previous"]
    on_edge = ((ru == 0) | (ru == 1) | (rv == 0) | (rv == 1)) & inside
    return {
        "zero": int((inside & (kinds == V_ZERO)).sum()),
        "sub_pixel": int((inside & (kinds == V_SUB_PIXEL)).sum()),
        "whole_pixels": int((inside & (kinds == V_WHOLE_PIXELS)).sum()),
        "lands_on_edge": int((on_edge & ((kinds == V_LANDS_ON_EDGE_X) | (kinds == V_LANDS_ON_EDGE_Y))).sum()),
        "step_outside": int((~inside & ((kinds == V_STEP_OUTSIDE_X) | (kinds == V_STEP_OUTSIDE_Y))).sum()),
        "plus_minus_one": int(((kinds == V_PLUS_ONE) | (kinds == V_MINUS_ONE)).sum()),
        "largest_ties": int(((largest[1] > 1) & largest[0].any(axis=-1)).sum()),
        "closest_ties": int(((sample_velocity(vel, depth, CLOSEST)[1] > 1) & (dn.max(axis=0) > 0)).sum()),
        "all_zero_depths": int((dn.max(axis=0) == 0).sum()),
        "history_above": int((r["inside"][..., None] & (P > hi)).any(axis=-1).sum()),
        "history_below": int((r["inside"][..., None] & (P < lo)).any(axis=-1).sum()),
        "flat": int(flat.sum()),
        "resolved": int(r["inside"].sum()),
        "fallback": int((~r["inside"]).sum()),
    }
