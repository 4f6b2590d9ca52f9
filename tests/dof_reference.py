"""NumPy restatement of prosper's depth of field and skybox fill (not a test module), for tests/test_depth_of_field*.py:

  sample_offsets()                          the octaweb's 121 unit offsets, float32 [121, 2]
  setup, reduce_level, flatten, dilate,     res/shader/dof/*.comp stage by stage over arrays
  gather, median_filter, combine
  chain(illum, depth, pc, cam)              the seven stages one after another, every store rounded to fp16
  sky_directions(cam, w, h)                 the G-buffer tracer's pixel-centre primary rays (unnormalised), float64
  design(cam, w, h), coverage(...)          the banded test design and what of the passes it reaches

Every decision (early-outs, bucket sorting, nearest texels, the median's compares) is taken in float32 in the order the
kernels take it: np.float32 operations round as the kernels' uncontracted arithmetic does.  Sums and filtered lookups
are float64.  A stage returns its unrounded value `v` and the allowance `a` (REL times the texel's sum of absolute
terms); `half_bounds` gives the fp16 codes between which a stored texel must lie.
"""
import math

import numpy as np

import deferred_shading_reference as D

F = np.float32
REL = 2e-4  # tests/test_deferred_shading.py's allowance, relative to a texel's sum of absolute terms
PI32 = F(3.14159265)  # common/math.glsl, which only sampleAlpha uses
SINGLE_PIXEL_RADIUS = F(0.7071)
RING_COUNTS = (1, 8, 16, 24, 32, 40)
RING_FIRST = (0, 1, 9, 25, 49, 81)
TAPS = 121


def sample_offsets():
    out = np.zeros((TAPS, 2), np.float32)
    k = 0
    for ring, count in enumerate(RING_COUNTS):
        for s in range(count):
            phi = (float(s) + (0.5 if ring % 2 == 0 else 0.0)) * (2.0 * math.pi) / float(count)
            out[k] = (math.cos(phi), math.sin(phi))
            k += 1
    return out


def extents(w, h):
    """(hw, hh, tw, th, levels) of a w x h image."""
    hw, hh = (w + 1) // 2, (h + 1) // 2
    return hw, hh, (hw + 7) // 8, (hh + 7) // 8, max(hw, hh).bit_length()


def level_extent(hw, hh, l):
    return max(hw >> l, 1), max(hh >> l, 1)


def half(x):
    """Round to fp16 as the library does (nearest even)."""
    return np.asarray(x).astype(np.float16)


def half_bounds(v, a):
    """The fp16 values between which a stored texel of unrounded value v and allowance a lies (inclusive)."""
    with np.errstate(over="ignore"):
        return half(v - a).astype(np.float64), half(v + a).astype(np.float64)


def within_half(got16, v, a):
    """Per texel: the stored fp16 `got16` lies between the roundings of v - a and v + a."""
    lo, hi = half_bounds(np.asarray(v, np.float64), np.asarray(a, np.float64))
    g = np.asarray(got16, np.float64)
    return (g >= lo) & (g <= hi)


def camera_terms(cam):
    """(cameraToClip22, cameraToClip32) as float32: the terms of linearizeDepth."""
    c2c = D.mat(cam.cameraToClip)
    return F(c2c[2, 2]), F(c2c[2, 3])


def saturate32(x):
    """fminf(fmaxf(x, 0), 1) in float32: NaN becomes 0."""
    return np.fmin(np.fmax(np.asarray(x, F), F(0)), F(1))


def circle_of_confusion(depth, pc, cam):
    """float32 [h, w]: max((1 - focus / -viewZ) * maxBackgroundCoC, -maxCoC), mirrored operation by operation."""
    c22, c32 = camera_terms(cam)
    d = np.asarray(depth, F)
    with np.errstate(all="ignore"):
        view_z = (-c32) / (d + c22)
        return np.fmax((F(1) - F(pc.focusDistance) / (-view_z)) * F(pc.maxBackgroundCoC), -F(pc.maxCoC))


def _four(img, hw, hh):
    """The four full-resolution texels of every half-resolution texel in the order 01, 11, 10, 00 (dx, dy)."""
    h, w = img.shape[:2]
    ys, xs = np.arange(hh)[:, None] * 2, np.arange(hw)[None, :] * 2
    return [img[np.minimum(ys + dy, h - 1), np.minimum(xs + dx, w - 1)] for dx, dy in ((0, 1), (1, 1), (1, 0), (0, 0))]


def _bilateral(vals, cocs):
    """bilateralFilter: (weighted mean float64 [..., c], sum of absolute terms over the weight, cocOut float32)."""
    coc_out = np.fmin(np.fmin(cocs[0], cocs[1]), np.fmin(cocs[2], cocs[3]))
    w = [saturate32(F(1) - (coc_out - c)).astype(np.float64) for c in cocs]
    norm = w[0] + w[1] + w[2] + w[3]
    with np.errstate(all="ignore"):
        v = sum(wi[..., None] * np.asarray(x, np.float64) for wi, x in zip(w, vals)) / norm[..., None]
        s = sum(wi[..., None] * np.abs(np.asarray(x, np.float64)) for wi, x in zip(w, vals)) / norm[..., None]
    return v, s, coc_out


def setup(illum, depth, pc, cam):
    """setup.comp: dict with colour v / a [hh, hw, 3] and coc v / a [hh, hw] (the stored CoC is the minimum of the four)."""
    h, w = depth.shape
    hw, hh = extents(w, h)[:2]
    coc = circle_of_confusion(depth, pc, cam)
    cocs = _four(coc, hw, hh)
    v, s, coc_out = _bilateral([x[..., :3] for x in _four(np.asarray(illum, F), hw, hh)], cocs)
    # the CoC's terms: 1 * maxBackgroundCoC and (focus / -viewZ) * maxBackgroundCoC
    terms = np.abs(coc_out.astype(np.float64)) + 2.0 * float(pc.maxBackgroundCoC)
    return {"colour": v, "colour_a": REL * s, "coc": coc_out.astype(np.float64), "coc_a": REL * terms}


def _mean4(x):
    return 0.25 * (x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2])


def reduce_level(k, level0, below=None):
    """reduce.comp level k >= 1, unrounded float64 [h_k, w_k, 3].  k <= 6: from `level0` (stored fp16 [hh, hw, 4]) over
    virtual texels, the source clamped to its edge, every level below unrounded.  k >= 7: from `below`, the stored level
    k - 1, clamped to its own extent."""
    hh, hw = level0.shape[:2]
    wk, hk = level_extent(hw, hh, k)
    if k <= 6:
        x = np.asarray(level0, np.float64)[..., :3]
        x = np.pad(x, ((0, -hh % 64), (0, -hw % 64), (0, 0)), mode="edge")
        for _ in range(k):
            x = _mean4(x)
        return x[:hk, :wk]
    x = np.asarray(below, np.float64)[..., :3]
    x = np.pad(x, ((0, x.shape[0] % 2), (0, x.shape[1] % 2), (0, 0)), mode="edge")
    return _mean4(x)[:hk, :wk]


def flatten(coc16):
    """flatten.comp: fp16 [th, tw, 2] (min, max) of the stored CoC over 8 x 8 tiles clamped at the edge: exact."""
    hh, hw = coc16.shape
    x = np.pad(np.asarray(coc16, np.float16), ((0, -hh % 8), (0, -hw % 8)), mode="edge")
    t = x.reshape(x.shape[0] // 8, 8, x.shape[1] // 8, 8)
    return np.stack([t.min(axis=(1, 3)), t.max(axis=(1, 3))], axis=-1)


def dilate(tiles16, gather_radius):
    """dilate.comp over the in-image tiles within gather_radius: fp16 [th, tw, 2], exact."""
    th, tw = tiles16.shape[:2]
    lo_in, hi_in = tiles16[..., 0].astype(F), tiles16[..., 1].astype(F)
    lo, hi = np.full((th, tw), np.inf, F), np.full((th, tw), -np.inf, F)
    r = int(min(gather_radius, max(th, tw) - 1))
    for j in range(-r, r + 1):
        for i in range(-r, r + 1):
            # destination tiles (y, x) whose neighbour (y + j, x + i) lies in the image
            y0, y1, x0, x1 = max(0, -j), min(th, th - j), max(0, -i), min(tw, tw - i)
            if y0 >= y1 or x0 >= x1:
                continue
            dist = F(8) * np.sqrt(F(i * i + j * j))
            a, b = lo_in[y0 + j:y1 + j, x0 + i:x1 + i], hi_in[y0 + j:y1 + j, x0 + i:x1 + i]
            dl, dh = lo[y0:y1, x0:x1], hi[y0:y1, x0:x1]
            dl[...] = np.where(dist <= np.abs(a) + F(4), np.fmin(dl, a), dl)
            dh[...] = np.where(dist <= np.abs(b) + F(4), np.fmax(dh, b), dh)
    return np.stack([lo, hi], axis=-1).astype(np.float16)


def _bilinear(level, sx, sy, px, py):
    h, w = level.shape[:2]
    qx, qy = px * sx - 0.5, py * sy - 0.5
    fx, fy = np.floor(qx), np.floor(qy)
    a, b = (qx - fx)[:, None], (qy - fy)[:, None]
    x0, x1 = np.clip(fx, 0, w - 1).astype(np.int64), np.clip(fx + 1, 0, w - 1).astype(np.int64)
    y0, y1 = np.clip(fy, 0, h - 1).astype(np.int64), np.clip(fy + 1, 0, h - 1).astype(np.int64)
    return ((1 - a) * (1 - b) * level[y0, x0] + a * (1 - b) * level[y0, x1] + (1 - a) * b * level[y1, x0]
            + a * b * level[y1, x1])


def trilinear(mips, px, py, mip):
    """textureLod over the stored mips (float64 [h_l, w_l, 3] each) at half-resolution texel positions (px, py)."""
    n = len(mips)
    hh, hw = mips[0].shape[:2]
    lod = np.clip(mip, 0.0, n - 1.0)
    l0 = np.floor(lod).astype(np.int64)
    t = (lod - l0)[:, None]
    l1 = np.minimum(l0 + 1, n - 1)
    out = np.zeros((len(px), 3))
    for l, level in enumerate(mips):
        sx = float(F(level.shape[1]) / F(hw))
        sy = float(F(level.shape[0]) / F(hh))
        m = l0 == l
        if m.any():
            out[m] += (1 - t[m]) * _bilinear(level, sx, sy, px[m], py[m])
        m = (l1 == l) & (t[:, 0] > 0)
        if m.any():
            out[m] += t[m] * _bilinear(level, sx, sy, px[m], py[m])
    # (a texel with t == 0 took (1 - 0) of level l0 above)
    return out


def sample_alpha(c):
    """sampleAlpha of gather.comp, float64 over the GLSL's float32 constants."""
    c = np.asarray(c, np.float64)
    with np.errstate(all="ignore"):
        return np.minimum(1.0 / (float(PI32) * c * c), 1.0 / (float(PI32) * float(SINGLE_PIXEL_RADIUS) ** 2))


def _sat64(x):
    return np.where(np.isnan(x), 0.0, np.clip(x, 0.0, 1.0))


def gather(mips16, coc16, dilated16, background, stats=None):
    """gather.comp over every half-resolution texel: (v float64 [hh, hw, 4], a [hh, hw, 4]).  mips16: the stored levels
    (fp16 [h_l, w_l, 4]); coc16 fp16 [hh, hw]; dilated16 fp16 [th, tw, 2].  `stats` (a dict) receives, for the
    background, taps[ring][0 = inner (current), 1 = outer (previous)]: how many taps each bucket of each ring took."""
    hh, hw = coc16.shape
    mips = [np.asarray(m, np.float64)[..., :3] for m in mips16]
    coc = np.asarray(coc16, F)
    off = sample_offsets()
    ys, xs = np.meshgrid(np.arange(hh), np.arange(hw), indexing="ij")
    ys, xs = ys.ravel(), xs.ravel()
    tile_min = np.asarray(dilated16, F)[ys // 8, xs // 8, 0]
    tile_max = np.asarray(dilated16, F)[ys // 8, xs // 8, 1]
    out = np.zeros((hh * hw, 4))
    active = (tile_max >= F(1)) if background else (tile_min <= F(-0.5))
    # (the early-outs are tileMaxCoC < 1 and tileMinCoC > -0.5: a NaN tile would go on, and no design has one)
    idx = np.nonzero(active)[0]
    if stats is not None:
        stats["active_texels"] = int(active.sum())
        stats["taps"] = [[0, 0] for _ in RING_COUNTS]
    if idx.size == 0:
        return out.reshape(hh, hw, 4), np.zeros((hh, hw, 4))
    cx, cy = xs[idx].astype(F) + F(0.5), ys[idx].astype(F) + F(0.5)
    n = idx.size

    def tap(ring_radius, k):
        px, py = cx + ring_radius * off[k, 0], cy + ring_radius * off[k, 1]
        ix = np.clip(np.floor(px), 0, hw - 1).astype(np.int64)
        iy = np.clip(np.floor(py), 0, hh - 1).astype(np.int64)
        return px, py, coc[iy, ix]

    if background:
        kernel_radius = tile_max[idx]
        spacing = kernel_radius / F(5)
        prev = np.zeros((n, 6))  # r, g, b, w, cocSum, sampleCount
        for ring in range(5, -1, -1):
            count = RING_COUNTS[ring]
            bordering = ((F(ring) + F(0.5)) + F(1)) * spacing
            ring_radius = F(ring) * spacing
            cur = np.zeros((n, 6))
            for s in range(count):
                px, py, c = tap(ring_radius, RING_FIRST[ring] + s)
                inside = c >= ring_radius
                to_cur = inside & (c < bordering)
                to_prev = inside & ~to_cur
                if stats is not None:
                    stats["taps"][ring][0] += int(to_cur.sum())
                    stats["taps"][ring][1] += int(to_prev.sum())
                m = np.nonzero(inside)[0]
                if m.size == 0:
                    continue
                c64 = c[m].astype(np.float64)
                with np.errstate(all="ignore"):
                    mip = np.where(c64 > 0, np.maximum(np.log2(np.where(c64 > 0, c64, 1.0)) - 1.0, 0.0), 0.0)
                wgt = sample_alpha(c64)
                col = trilinear(mips, px[m].astype(np.float64), py[m].astype(np.float64), mip)
                add = np.concatenate([col * wgt[:, None], wgt[:, None], c64[:, None], np.ones((m.size, 1))], axis=1)
                sel = to_cur[m]
                cur[m[sel]] += add[sel]
                prev[m[~sel]] += add[~sel]
            with np.errstate(all="ignore"):
                opacity = _sat64(cur[:, 5] / count)
                occluding = _sat64(prev[:, 4] / prev[:, 5] - cur[:, 4] / cur[:, 5])
            blend = np.where(prev[:, 3] == 0.0, 0.0, 1.0 - opacity * occluding)
            prev = prev * blend[:, None] + cur
        colour = prev[:, :3] / np.maximum(prev[:, 3], float(F(0.00001)))[:, None]
        out[idx, :3] = colour
    else:
        kernel_radius = -tile_min[idx]
        spacing = kernel_radius / F(5)
        acc = np.zeros((n, 5))  # r, g, b, alphaSum, totalWeight
        for ring in range(6):
            ring_radius = F(ring) * spacing
            for s in range(RING_COUNTS[ring]):
                k = RING_FIRST[ring] + s
                px, py, c = tap(ring_radius, k)
                c = -c
                sx, sy = ring_radius * off[k, 0], ring_radius * off[k, 1]
                dist = np.sqrt(sx * sx + sy * sy)
                take = ~(c < F(0.5)) & (c >= dist - spacing)
                m = np.nonzero(take)[0]
                if m.size == 0:
                    continue
                c64 = c[m].astype(np.float64)
                mip = np.maximum((np.frexp(c[m])[1] - 1).astype(np.float64) - 1.0, 0.0)
                wgt = kernel_radius[m].astype(np.float64) / c64
                col = trilinear(mips, px[m].astype(np.float64), py[m].astype(np.float64), mip)
                acc[m, :3] += col * wgt[:, None]
                acc[m, 3] += sample_alpha(c64) * _sat64(c64 - 0.5)
                acc[m, 4] += wgt
        out[idx, :3] = acc[:, :3] / np.maximum(acc[:, 4], float(F(0.001)))[:, None]
        kr = kernel_radius.astype(np.float64)
        out[idx, 3] = _sat64(2.0 * (1.0 / TAPS) * (1.0 / sample_alpha(kr)) * acc[:, 3])
    # every term is a product of non-negative factors: the sum of absolute terms over the weight is the value itself
    return out.reshape(hh, hw, 4), REL * np.abs(out).reshape(hh, hw, 4)


def median_filter(layer16):
    """filter.comp: the 3 x 3 median by luminance as written, fp16 [hh, hw, 4]: one of the nine inputs, exact.  The second
    compare-swap round's pairs are (0, 2), (1, 3), (6, 8); its fourth pair (7, 9) reaches past the nine elements."""
    hh, hw = layer16.shape[:2]
    ys, xs = np.meshgrid(np.arange(hh), np.arange(hw), indexing="ij")
    texels = np.asarray(layer16, np.float16)
    lum, sy, sx = [], [], []
    for i in (-1, 0, 1):  # i outer, j inner
        for j in (-1, 0, 1):
            yy, xx = np.clip(ys + j, 0, hh - 1), np.clip(xs + i, 0, hw - 1)
            c = texels[yy, xx].astype(F)
            lum.append((F(0.299) * c[..., 0] + F(0.587) * c[..., 1]) + F(0.114) * c[..., 2])
            sy.append(yy)
            sx.append(xx)
    lum = np.stack(lum)  # [9, hh, hw]
    max_lum, max_i = np.zeros((hh, hw), F), np.zeros((hh, hw), np.int64)
    for k in range(9):
        better = max_lum < lum[k]
        max_lum = np.where(better, lum[k], max_lum)
        max_i = np.where(better, k, max_i)
    idx = np.tile(np.arange(9)[:, None, None], (1, hh, hw))
    move = max_i < 8
    yy, xx = np.nonzero(move)
    idx[8, yy, xx] = max_i[yy, xx]
    idx[max_i[yy, xx], yy, xx] = 8

    def lum_of(slot):
        return np.take_along_axis(lum, idx[slot][None], axis=0)[0]

    def compare_swap(first, second):
        swap = lum_of(first) < lum_of(second)
        a, b = idx[first].copy(), idx[second].copy()
        idx[first], idx[second] = np.where(swap, b, a), np.where(swap, a, b)

    for i in range(4):
        compare_swap(i, i + 4)
    for first, second in ((0, 2), (1, 3), (6, 8)):
        compare_swap(first, second)
    for i in range(4):
        compare_swap(2 * i, 2 * i + 1)
    m = idx[4]
    my = np.take_along_axis(np.stack(sy), m[None], axis=0)[0]
    mx = np.take_along_axis(np.stack(sx), m[None], axis=0)[0]
    return texels[my, mx]


def combine(illum, coc16, fg16, bg16):
    """combine.comp: (v float64 [h, w, 3], a [h, w, 3]); the output alpha is the input's."""
    h, w = illum.shape[:2]
    hh, hw = coc16.shape
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    coc = np.asarray(coc16, F)[ys // 2, xs // 2]
    hx0, hx1 = xs // 2, np.minimum((xs + 1) // 2, hw - 1)
    hy0, hy1 = ys // 2, np.minimum((ys + 1) // 2, hh - 1)
    out = np.asarray(illum, np.float64)[..., :3].copy()
    mag = np.abs(out)
    bg = np.asarray(bg16, np.float64)
    c00, c10, c11 = bg[hy0, hx0, :3], bg[hy0, hx1, :3], bg[hy1, hx1, :3]
    bg_colour = 0.5 * (0.5 * c00 + 0.5 * c10) + 0.5 * (0.5 * c10 + 0.5 * c11)
    bg_factor = saturate32(coc - F(1)).astype(np.float64)[..., None]
    out = np.where(bg_factor > 0, out * (1 - bg_factor) + bg_colour * bg_factor, out)
    mag = np.where(bg_factor > 0, mag * (1 - bg_factor) + np.abs(bg_colour) * bg_factor, mag)
    fg = np.asarray(fg16, F)
    texels = [fg[hy0, hx0], fg[hy1, hx0], fg[hy1, hx1], fg[hy0, hx1]]  # the bilateral's 01, 11, 10, 00
    v, s, _ = _bilateral(texels, [t[..., 3] for t in texels])
    fg_weight = v[..., 3:4]
    take = fg_weight > 0
    out = np.where(take, out * (1 - fg_weight) + v[..., :3] * fg_weight, out)
    mag = np.where(take, mag * (1 - fg_weight) + s[..., :3] * fg_weight, mag)
    return out, REL * mag


def foreground_footprint(h, w, fg16):
    """The four filtered foreground texels combine.comp reads for every full-resolution pixel, fp16 [h, w, 4, 4]."""
    hh, hw = fg16.shape[:2]
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    hx0, hx1 = xs // 2, np.minimum((xs + 1) // 2, hw - 1)
    hy0, hy1 = ys // 2, np.minimum((ys + 1) // 2, hh - 1)
    fg = np.asarray(fg16)
    return np.stack([fg[hy0, hx0], fg[hy1, hx0], fg[hy1, hx1], fg[hy0, hx1]], axis=2)


def constant_colour_bounds(colour, h, w, fg16):
    """What a constant `colour` may become, (lo, hi) float64 [h, w, 3].  Every lookup and mean of a constant is that
    constant, so both layers hold it wherever they hold anything, and the image keeps it, with one exception the GLSL
    has as written: a foreground texel that took no tap is (0, 0, 0, 0), and where the foreground's bilateral upscale
    meets such a texel beside one with a weight it averages the black in (every bilateral weight is 1 when the smallest
    alpha is 0).  The pixel then darkens by at most the largest of the four alphas."""
    f = foreground_footprint(h, w, fg16).astype(np.float64)
    empty = ~f[..., :3].any(axis=-1)
    mixes = empty.any(axis=-1) & (f[..., 3] > 0).any(axis=-1)
    colour = np.broadcast_to(np.asarray(colour, np.float64), (h, w, 3))
    tol = 1e-6 * colour
    lo = np.where(mixes[..., None], colour * (1.0 - f[..., 3].max(axis=-1))[..., None], colour) - tol
    return lo, colour + tol


def chain(illum, depth, pc, cam):
    """The seven stages one after another, every store rounded to fp16: dict of the stored intermediates and `out`
    (float64 [h, w, 4]) with its allowance `out_a` for the last stage alone."""
    h, w = depth.shape
    hw, hh, tw, th, levels = extents(w, h)
    s = setup(illum, depth, pc, cam)
    level0 = np.concatenate([half(s["colour"]), np.ones((hh, hw, 1), np.float16)], axis=-1)
    coc16 = half(s["coc"])
    mips = [level0]
    for k in range(1, levels):
        v = reduce_level(k, level0, mips[-1])
        mips.append(np.concatenate([half(v), np.ones(v.shape[:2] + (1,), np.float16)], axis=-1))
    tiles = flatten(coc16)
    dilated = dilate(tiles, pc.gatherRadius)
    fg = half(gather(mips, coc16, dilated, False)[0])
    bg = half(gather(mips, coc16, dilated, True)[0])
    fgf, bgf = median_filter(fg), median_filter(bg)
    v, a = combine(illum, coc16, fgf, bgf)
    out = np.concatenate([v, np.asarray(illum, np.float64)[..., 3:4]], axis=-1)
    return {"mips": mips, "coc": coc16, "tiles": tiles, "dilated": dilated, "fg": fg, "bg": bg, "fg_filtered": fgf,
            "bg_filtered": bgf, "out": out, "out_a": a}


def sky_directions(cam, w, h):
    """The G-buffer tracer's primary rays through the pixel centres (px + 0.5, py + 0.5), unnormalised, float64 [h, w, 3]."""
    w2c, c2c = D.mat(cam.worldToCamera), D.mat(cam.cameraToClip)
    right, up, fwd = w2c[0, :3], w2c[1, :3], -w2c[2, :3]
    aspect, tan_half = c2c[1, 1] / c2c[0, 0], 1.0 / c2c[1, 1]
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    ndx, ndy = (xs + 0.5) / w * 2.0 - 1.0, (ys + 0.5) / h * 2.0 - 1.0
    return (right * (ndx * tan_half * aspect)[..., None] + up * (ndy * tan_half)[..., None]) + fwd


# ---- the test design ----

BAND_DEPTHS = (0.6, 1.0, 2.0, 2.2, 4.0, 12.0, None, 1.6, 3.0)  # None: a miss
FOCUS = 2.0
FAR = 50.0


def nonlinear_depth(cam, lin):
    """Non-linear depth float32 of positive distances `lin` along the view direction (NaN: a miss, 0)."""
    c2c = D.mat(cam.cameraToClip)
    lin = np.asarray(lin, np.float64)
    with np.errstate(all="ignore"):
        return np.where(np.isnan(lin), 0.0, c2c[2, 3] / lin - c2c[2, 2]).astype(np.float32)


def design(cam, w, h, seed=7, depths=BAND_DEPTHS, constant=None, band=10, shift=5):
    """(illumination float32 [h, w, 4], nonLinearDepth float32 [h, w]): vertical `band`-pixel bands of linear depth
    cycling through `depths`, the lower half of the image shifted by `shift` pixels; the colour is a per-band level
    between 0.2 and 5 times a smooth gradient times per-texel noise (or `constant`), the alpha varies."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    band = ((xs + np.where(ys >= h // 2, shift, 0)) // band) % len(depths)
    lin = np.array([np.nan if d is None else d for d in depths])[band]
    levels = rng.uniform(0.2, 5.0, (len(depths), 3))
    gradient = 0.6 + 0.4 * np.sin(xs / max(w, 1) * 3.0 + ys / max(h, 1) * 2.0)
    colour = levels[band] * gradient[..., None] * rng.uniform(0.7, 1.3, (h, w, 3))
    if constant is not None:
        colour = np.broadcast_to(np.asarray(constant, np.float64), (h, w, 3))
    alpha = rng.uniform(0.5, 1.0, (h, w, 1))
    return np.concatenate([colour, alpha], axis=-1).astype(np.float32), nonlinear_depth(cam, lin)


# The dilation spreads a tile's maximum over every tile its circle can reach, so within gatherRadius no tap's CoC exceeds
# the kernel radius and the outer buckets of rings 4 and 5 (CoC >= 1.1 and 1.3 kernel radii) stay empty.  They fill only
# where the dilation stops short: this variant has bands three tiles wide, circles of 14 and 19 texels beside each other
# and a gatherRadius of one tile.
REACH_DEPTHS = (6.67, 40.0, 1.0, 2.0)
REACH_BAND = 48
REACH_MAX_BACKGROUND_COC = 20.0
REACH_GATHER_RADIUS = 1


def reach_design(cam, w, h, seed=9):
    return design(cam, w, h, seed=seed, depths=REACH_DEPTHS, band=REACH_BAND, shift=0)


def coverage(illum, depth, pc, cam):
    """What of the passes the design reaches, from the restatement alone: shares of tiles and texels, and the taps each
    ring / bucket pair of the background takes."""
    c = chain(illum, depth, pc, cam)
    tiles, dilated = c["tiles"].astype(F), c["dilated"].astype(F)
    coc = c["coc"].astype(F)
    stats = {}
    gather(c["mips"], c["coc"], c["dilated"], True, stats)
    return {
        "bg_active_tiles": float((dilated[..., 1] >= 1).mean()),
        "bg_skipped_tiles": float((dilated[..., 1] < 1).mean()),
        "fg_skipped_tiles": float((dilated[..., 0] > -0.5).mean()),
        "coc_ge_4": float((coc >= 4).mean()),
        "coc_le_m8": float((coc <= -8).mean()),
        "dilation_changed_tiles": float((tiles.view(np.uint32) != dilated.view(np.uint32)).any(axis=-1).mean()),
        "bg_taps": stats["taps"],
    }
