"""The rule of prosper_pt_denoise, stated in NumPy: float32, operation for operation.

prosper has no denoiser, so this file is the contract: the kernels of csrc/pt_denoise.hip compute these values bit for
bit.  The rule uses only + - * / sqrt min max floor abs and comparisons, each correctly rounded in float32, in the order
written here (min and max: a NaN operand loses, np.fmin / np.fmax).  Nothing is stored narrower than float32.

Images are [h, w, 4] float32 records as prosper_pt_read_denoise_stage returns them:
    guide_a   z, dz/dx, dz/dy, the geometry flag (uint32 bits)
    guide_b   n.x, n.y, n.z, 0
    moments   m1, m2, the history length (uint32 bits), 0
    colour images   r, g, b, variance
A history is the dict {"colour", "moments", "guide_a", "guide_b"} a frame hands to the next one.

Every stage is a function of its own, so that a test can feed each with what the GPU's previous stage wrote."""
import numpy as np

F = np.float32
MIN_ALBEDO = F(1.0 / 64.0)
B3 = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))


class PC:
    """prosper_pt_denoise_pc; the defaults are prosper_pt_denoise_pc_default's"""

    def __init__(self, iterations=5, demodulate=1, max_history_length=32, feedback_iteration=1, normal_power_log2=7,
                 reset_history=0, min_alpha=0.05, depth_tolerance=0.1, normal_threshold=0.9, sigma_depth=1.0,
                 sigma_luminance=4.0):
        self.iterations, self.demodulate, self.max_history_length = iterations, demodulate, max_history_length
        self.feedback_iteration, self.normal_power_log2, self.reset_history = feedback_iteration, normal_power_log2, reset_history
        self.min_alpha, self.depth_tolerance, self.normal_threshold = F(min_alpha), F(depth_tolerance), F(normal_threshold)
        self.sigma_depth, self.sigma_luminance = F(sigma_depth), F(sigma_luminance)


def _quiet(fn):
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    wrapped.__doc__ = fn.__doc__
    wrapped.__name__ = fn.__name__
    return wrapped


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def from_bits(a):
    return np.ascontiguousarray(a, np.uint32).view(np.float32)


def luminance(rgb):
    return (F(0.299) * rgb[..., 0] + F(0.587) * rgb[..., 1]) + F(0.114) * rgb[..., 2]


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


@_quiet
def decode_normal(nm):
    """signedOctDecode of normalMetallic's (x, y, w)"""
    ox = nm[..., 0] - nm[..., 1]
    oy = (nm[..., 0] + nm[..., 1]) - F(1)
    oz = nm[..., 3] * F(2) - F(1)
    oz = oz * ((F(1) - np.abs(ox)) - np.abs(oy))
    o = np.stack([ox, oy, oz], -1)
    inv = F(1) / np.sqrt(dot3(o, o))
    return o * inv[..., None]


@_quiet
def view_depth(depth, c22, c32):
    """linearize_depth's distance along the view direction (-viewZ: positive in front of the camera)"""
    return F(c32) / (depth + F(c22))


def falloff(x):
    """F(x) = max(0, 1 - x / 8) ^ 8 by three squarings"""
    t = np.fmax(F(0), F(1) - x * F(0.125))
    t2 = t * t
    t4 = t2 * t2
    return t4 * t4


def normal_weight(d, power_log2):
    wn = np.fmax(F(0), d)
    for _ in range(power_log2):
        wn = wn * wn
    return wn


def tap(a, ox, oy):
    """(a[y + oy, x + ox] where that lies inside, 0 elsewhere; the mask of inside)"""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    inside = np.zeros((h, w), bool)
    x0, x1, y0, y1 = max(0, -ox), min(w, w - ox), max(0, -oy), min(h, h - oy)
    if x0 < x1 and y0 < y1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return out, inside


def flag_of(guide_a):
    return bits(guide_a[..., 3]) != 0


def _gradient(z, geometry, axis):
    ox, oy = (1, 0) if axis == 0 else (0, 1)
    zf, inf_ = tap(z, ox, oy)
    gf, _ = tap(geometry, ox, oy)
    zb, inb = tap(z, -ox, -oy)
    gb, _ = tap(geometry, -ox, -oy)
    has_f, has_b = inf_ & gf, inb & gb
    f, k = zf - z, z - zb
    both = np.where(np.abs(k) < np.abs(f), k, f)
    return np.where(has_f & has_b, both, np.where(has_f, f, np.where(has_b, k, F(0)))).astype(np.float32)


@_quiet
def edge_weight(pc, zp, gx, gy, np_, zq, nq, ox, oy, xl):
    """w_n F(x_z + xl) of the tap at the offset (ox, oy) texels"""
    tx, ty = gx * F(ox), gy * F(oy)
    xz = np.abs(zq - ((zp + tx) + ty)) / (pc.sigma_depth * (np.abs(tx) + np.abs(ty)) + F(1e-3) * zp)
    return normal_weight(dot3(np_, nq), pc.normal_power_log2) * falloff(xz + xl)


@_quiet
def temporal_stage(pc, c22, c32, illumination, albedo, normal_metallic, depth, velocity, history):
    """The guide of this frame and the blended colour, moments and length.  `history`: None to ignore it.
    -> dict: guide_a, guide_b, moments, temporal (the variance is the temporal one), counts (with, without history) and
    the masks `has_history`, `rejected_depth`, `rejected_normal`, `left_image` (of geometry pixels) for a test's design."""
    illumination = np.ascontiguousarray(illumination, np.float32)
    depth = np.ascontiguousarray(depth, np.float32)
    velocity = np.ascontiguousarray(velocity, np.float32)
    h, w = depth.shape
    geometry = depth != 0
    z = np.where(geometry, view_depth(depth, c22, c32), F(0)).astype(np.float32)
    zn = view_depth(depth, c22, c32).astype(np.float32)  # (a neighbour's z is computed whether it is geometry or not)
    gx, gy = _gradient(zn, geometry, 0), _gradient(zn, geometry, 1)
    n = decode_normal(np.ascontiguousarray(normal_metallic, np.float32))
    c = illumination[..., :3]
    if pc.demodulate:
        c = c / np.fmax(np.ascontiguousarray(albedo, np.float32)[..., :3], MIN_ALBEDO)
    sample = np.isfinite(c).all(-1)
    l = luminance(c)

    sw = np.zeros((h, w), np.float32)
    prev = np.zeros((h, w, 3), np.float32)
    m1 = np.zeros((h, w), np.float32)
    m2 = np.zeros((h, w), np.float32)
    length = np.zeros((h, w), np.uint32)
    rejected_depth = np.zeros((h, w), bool)
    rejected_normal = np.zeros((h, w), bool)
    left_image = np.zeros((h, w), bool)
    if history is not None:
        res_x, res_y = F(w), F(h)
        xs, ys = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
        u, v = (xs + F(0.5)) / res_x, (ys + F(0.5)) / res_y
        ru, rv = u - velocity[..., 0] * F(0.5), v - velocity[..., 1] * F(-0.5)
        cx, cy = ru * res_x - F(0.5), rv * res_y - F(0.5)
        in_range = (cx >= F(-1)) & (cx <= res_x) & (cy >= F(-1)) & (cy <= res_y)
        wx, wy = np.floor(np.where(in_range, cx, F(0))), np.floor(np.where(in_range, cy, F(0)))
        fx, fy = np.where(in_range, cx, F(0)) - wx, np.where(in_range, cy, F(0)) - wy
        ix, iy = wx.astype(np.int32), wy.astype(np.int32)
        weights = [(F(1) - fx) * (F(1) - fy), fx * (F(1) - fy), (F(1) - fx) * fy, fx * fy]
        pa, pb = history["guide_a"], history["guide_b"]
        left_image |= geometry & ~in_range
        for k in range(4):
            qx, qy = ix + (k & 1), iy + (k >> 1)
            inside = in_range & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
            left_image |= geometry & in_range & ~inside
            gx_, gy_ = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            qa, qb = pa[gy_, gx_], pb[gy_, gx_]
            ok = inside & flag_of(qa)
            depth_ok = np.abs(qa[..., 0] - z) <= pc.depth_tolerance * np.fmax(z, qa[..., 0])
            rejected_depth |= geometry & ok & ~depth_ok
            ok = ok & depth_ok
            normal_ok = dot3(qb[..., :3], n) >= pc.normal_threshold
            rejected_normal |= geometry & ok & ~normal_ok
            ok = ok & normal_ok & geometry
            qc, qm = history["colour"][gy_, gx_], history["moments"][gy_, gx_]
            wk = weights[k]
            sw = np.where(ok, sw + wk, sw)
            prev = np.where(ok[..., None], prev + wk[..., None] * qc[..., :3], prev)
            m1 = np.where(ok, m1 + wk * qm[..., 0], m1)
            m2 = np.where(ok, m2 + wk * qm[..., 1], m2)
            length = np.where(ok, np.maximum(length, bits(qm[..., 2])), length)
    has_history = geometry & (sw > 0)
    prev = prev / sw[..., None]
    m1p, m2p = m1 / sw, m2 / sw
    cap = np.uint32(pc.max_history_length)
    grown = np.minimum(length + np.uint32(1), cap)
    alpha = np.fmax(F(1) / grown.astype(np.float32), pc.min_alpha)
    keep = F(1) - alpha
    blended = keep[..., None] * prev + alpha[..., None] * c
    colour = np.where((has_history & sample)[..., None], blended,
                      np.where(has_history[..., None], prev, np.where(sample[..., None], c, F(0))))
    m1n = np.where(has_history & sample, keep * m1p + alpha * l, np.where(has_history, m1p, np.where(sample, l, F(0))))
    m2n = np.where(has_history & sample, keep * m2p + alpha * (l * l), np.where(has_history, m2p, np.where(sample, l * l, F(0))))
    newlen = np.where(has_history & sample, grown, np.where(has_history, np.minimum(length, cap), np.where(sample, 1, 0))).astype(np.uint32)
    variance = np.fmax(m2n - m1n * m1n, F(0))

    g3, g = geometry[..., None], geometry
    zero = np.zeros((h, w), np.float32)
    temporal = np.where(g3, np.concatenate([colour, variance[..., None]], -1), F(0)).astype(np.float32)
    moments = np.stack([np.where(g, m1n, F(0)), np.where(g, m2n, F(0)), from_bits(np.where(g, newlen, 0).astype(np.uint32)), zero], -1)
    guide_a = np.stack([z, np.where(g, gx, F(0)), np.where(g, gy, F(0)), from_bits(g.astype(np.uint32))], -1)
    guide_b = np.where(g3, np.concatenate([n, zero[..., None]], -1), F(0))
    return {"guide_a": guide_a.astype(np.float32), "guide_b": guide_b.astype(np.float32), "moments": moments.astype(np.float32),
            "temporal": temporal, "counts": (int(has_history.sum()), int((geometry & ~has_history).sum())),
            "has_history": has_history, "rejected_depth": rejected_depth & ~has_history, "rejected_normal": rejected_normal & ~has_history,
            "left_image": left_image & ~has_history}


@_quiet
def temporal_variance(moments):
    return np.fmax(moments[..., 1] - moments[..., 0] * moments[..., 0], F(0))


@_quiet
def variance_stage(pc, guide_a, guide_b, moments, temporal):
    """`temporal` with the variance after the estimate: re-estimated over 7 x 7 where the length is below 4"""
    h, w = guide_a.shape[:2]
    geometry = flag_of(guide_a)
    length = bits(moments[..., 2])
    zp, gx, gy, np_ = guide_a[..., 0], guide_a[..., 1], guide_a[..., 2], guide_b[..., :3]
    sw = np.zeros((h, w), np.float32)
    s1 = np.zeros((h, w), np.float32)
    s2 = np.zeros((h, w), np.float32)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            if dx == 0 and dy == 0:
                wk, ok, qm = np.ones((h, w), np.float32), np.ones((h, w), bool), moments
            else:
                qa, inside = tap(guide_a, dx, dy)
                qb, _ = tap(guide_b, dx, dy)
                qm, _ = tap(moments, dx, dy)
                ok = inside & flag_of(qa)
                wk = edge_weight(pc, zp, gx, gy, np_, qa[..., 0], qb[..., :3], dx, dy, F(0))
            sw = np.where(ok, sw + wk, sw)
            s1 = np.where(ok, s1 + wk * qm[..., 0], s1)
            s2 = np.where(ok, s2 + wk * qm[..., 1], s2)
    m1, m2 = s1 / sw, s2 / sw
    spatial = np.fmax(m2 - m1 * m1, F(0)) * (F(4) / np.maximum(length, 1).astype(np.float32))
    out = np.array(temporal, np.float32)
    out[..., 3] = np.where(geometry, np.where(length < 4, spatial, temporal_variance(moments)), temporal[..., 3])
    return out


@_quiet
def atrous_taps(pc, i, guide_a, guide_b, image):
    """The 25 taps of pass i in the rule's order, each (dx, dy, counted, w, c_q, terms); terms = (w_n, F(x_z), F(x_l)) each
    alone, for a test's design (None for the centre)"""
    h, w = guide_a.shape[:2]
    s = 1 << i
    geometry = flag_of(guide_a)
    zp, gx, gy, np_ = guide_a[..., 0], guide_a[..., 1], guide_a[..., 2], guide_b[..., :3]
    gw = np.zeros((h, w), np.float32)
    gv = np.zeros((h, w), np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qa, inside = tap(guide_a, dx, dy)
            qv, _ = tap(image[..., 3], dx, dy)
            ok = inside & flag_of(qa)
            k = (F(0.5) if dx == 0 else F(0.25)) * (F(0.5) if dy == 0 else F(0.25))
            gw = np.where(ok, gw + k, gw)
            gv = np.where(ok, gv + k * qv, gv)
    denom_l = pc.sigma_luminance * np.sqrt(gv / gw) + F(1e-4)
    lp = luminance(image[..., :3])
    taps = []
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            hh = B3[dx + 2] * B3[dy + 2]
            if dx == 0 and dy == 0:
                taps.append((dx, dy, geometry, np.full((h, w), hh, np.float32), image, None))
                continue
            ox, oy = s * dx, s * dy
            qa, inside = tap(guide_a, ox, oy)
            qb, _ = tap(guide_b, ox, oy)
            qc, _ = tap(image, ox, oy)
            ok = geometry & inside & flag_of(qa)
            xl = np.abs(luminance(qc[..., :3]) - lp) / denom_l
            wk = hh * edge_weight(pc, zp, gx, gy, np_, qa[..., 0], qb[..., :3], ox, oy, xl)
            tx, ty = gx * F(ox), gy * F(oy)
            xz = np.abs(qa[..., 0] - ((zp + tx) + ty)) / (pc.sigma_depth * (np.abs(tx) + np.abs(ty)) + F(1e-3) * zp)
            terms = (normal_weight(dot3(np_, qb[..., :3]), pc.normal_power_log2), falloff(xz), falloff(xl))
            taps.append((dx, dy, ok, wk.astype(np.float32), qc, terms))
    return taps


@_quiet
def atrous_pass(pc, i, guide_a, guide_b, image):
    """One edge-avoiding a-trous pass, step 1 << i, over `image` (rgb + variance)"""
    h, w = guide_a.shape[:2]
    geometry = flag_of(guide_a)
    sw = np.zeros((h, w), np.float32)
    sv = np.zeros((h, w), np.float32)
    sc = np.zeros((h, w, 3), np.float32)
    for _, _, ok, wk, qc, _ in atrous_taps(pc, i, guide_a, guide_b, image):
        sw = np.where(ok, sw + wk, sw)
        sc = np.where(ok[..., None], sc + wk[..., None] * qc[..., :3], sc)
        sv = np.where(ok, sv + (wk * wk) * qc[..., 3], sv)
    out = np.concatenate([sc / sw[..., None], (sv / (sw * sw))[..., None]], -1)
    return np.where(geometry[..., None], out, image).astype(np.float32)


@_quiet
def finish(pc, illumination, albedo, guide_a, image):
    """The HDR image: the filtered colour times the albedo it was divided by, the input's alpha; sky as it came in"""
    illumination = np.ascontiguousarray(illumination, np.float32)
    rgb = image[..., :3]
    if pc.demodulate:
        rgb = rgb * np.fmax(np.ascontiguousarray(albedo, np.float32)[..., :3], MIN_ALBEDO)
    out = np.concatenate([rgb, illumination[..., 3:]], -1).astype(np.float32)
    return np.where(flag_of(guide_a)[..., None], out, illumination)


def denoise(pc, c22, c32, illumination, albedo, normal_metallic, depth, velocity, history=None):
    """One whole call.  -> dict: the temporal stage's entries, `temporal` after the variance estimate, `atrous` (a list,
    one image per pass), `out` (the HDR image) and `history` (what the next call reads)."""
    if pc.reset_history:
        history = None
    r = temporal_stage(pc, c22, c32, illumination, albedo, normal_metallic, depth, velocity, history)
    feedback = r["temporal"]
    r["temporal"] = variance_stage(pc, r["guide_a"], r["guide_b"], r["moments"], r["temporal"])
    image, r["atrous"] = r["temporal"], []
    for i in range(pc.iterations):
        image = atrous_pass(pc, i, r["guide_a"], r["guide_b"], image)
        r["atrous"].append(image)
        if i == pc.feedback_iteration:
            feedback = image
    r["out"] = finish(pc, illumination, albedo, r["guide_a"], image)
    r["history"] = {"colour": feedback, "moments": r["moments"], "guide_a": r["guide_a"], "guide_b": r["guide_b"]}
    return r
