"""NumPy float32 restatement of the material textures' mip chains and of sample_texture_lod.

Generation (pt_texture_mips.hip generate_mip_kernel), level selection and the trilinear sample (pt_device.hpp
texture_lambda / lod_levels / lod_taps / filter_lod_taps) in the written-down operation order, with the single-rounding
fmaf of particles_reference.py.  The device's log2_, exp2_, pow_ and srgb_to_linear (pt_math.hpp, pt_device.hpp) are
restated too: every operation is one IEEE float32 operation, so the results are compared bit for bit."""
import numpy as np

from particles_reference import fma

F = np.float32
NEAREST, LINEAR = 0, 1
REPEAT, MIRRORED_REPEAT, CLAMP_TO_EDGE = 0, 1, 2


# ---- the device's math (pt_math.hpp) ----
def log2_(x):
    x = np.asarray(x, F)
    bits = x.view(np.uint32)
    e = (bits >> 23).astype(np.int32) - 127
    m = ((bits & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(F)
    fold = m > F(1.41421354)
    m = np.where(fold, m * F(0.5), m).astype(F)
    e = e + fold.astype(np.int32)
    s = ((m - F(1.0)) / (m + F(1.0))).astype(F)
    z = (s * s).astype(F)
    p = fma(F(0.222222222), z, F(0.285714286))
    p = fma(p, z, F(0.4))
    p = fma(p, z, F(0.666666667))
    p = fma(p, z, F(2.0))
    ln = (p * s).astype(F)
    return fma(ln, F(1.44269504), e.astype(F))


def exp2_(x):
    x = np.clip(np.asarray(x, F), F(-126.0), F(127.0)).astype(F)
    n = np.rint(x).astype(F)
    f = (x - n).astype(F)
    p = fma(F(1.52527338e-5), f, F(1.54035304e-4))
    for c in (1.33335581e-3, 9.61812911e-3, 5.55041087e-2, 2.40226507e-1, 6.93147181e-1, 1.0):
        p = fma(p, f, F(c))
    scale = ((n.astype(np.int32) + 127).astype(np.uint32) << 23).view(F)
    return (p * scale).astype(F)


def pow_(x, y):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        r = exp2_((F(y) * log2_(np.where(x > 0, x, F(1.0)).astype(F))).astype(F))
    return np.where(x > 0, r, F(0.0)).astype(F)


def srgb_to_linear(x):
    """materials.glsl:26-29 as the device evaluates it."""
    x = np.asarray(x, F)
    lo = (x * (F(1.0) / F(12.92))).astype(F)
    hi = pow_(((x + F(0.055)).astype(F) * (F(1.0) / F(1.055))).astype(F), F(2.4))
    return np.where(x <= F(0.04045), lo, hi).astype(F)


K255 = F(1.0) / F(255.0)


def srgb_lut():
    """lut[c] = srgb_to_linear(c * (1 / 255)): what sample_material decodes from code c."""
    return srgb_to_linear((np.arange(256, dtype=F) * K255).astype(F))


# ---- chains ----
def mip_level_count(width, height):
    """max(floor(log2(max(w, h))) + 1 - 2, 1) (src/scene/Texture.cpp:217-225)."""
    return max(int(max(width, height)).bit_length() - 2, 1)


def level_extent(width, height, level):
    return max(width >> level, 1), max(height >> level, 1)


def generate_level(parent, srgb):
    """Child (i, j) = mean of parent (2i, min(2i + 1, pw - 1)) x (2j, min(2j + 1, ph - 1)).  uint8 [ph, pw, 4] ->
    uint8 [max(ph >> 1, 1), max(pw >> 1, 1), 4]."""
    ph, pw = parent.shape[:2]
    ch, cw = max(ph >> 1, 1), max(pw >> 1, 1)
    x0 = 2 * np.arange(cw)
    y0 = 2 * np.arange(ch)
    x1 = np.minimum(x0 + 1, pw - 1)
    y1 = np.minimum(y0 + 1, ph - 1)
    p00 = parent[y0][:, x0]
    p10 = parent[y0][:, x1]
    p01 = parent[y1][:, x0]
    p11 = parent[y1][:, x1]
    out = ((p00.astype(np.uint32) + p10 + p01 + p11 + 2) >> 2).astype(np.uint8)
    if srgb:
        lut = srgb_lut()
        mean = (((lut[p00[..., :3]] + lut[p10[..., :3]]).astype(F) + (lut[p01[..., :3]] + lut[p11[..., :3]]).astype(F)).astype(F) * F(0.25)).astype(F)
        # the first code with the smallest |lut[c] - mean| (float32): ties go to the lower code
        dist = np.abs((lut[None, None, None, :] - mean[..., None]).astype(F))
        out[..., :3] = np.argmin(dist, axis=-1).astype(np.uint8)
    return out


def generate_chain(level0, srgb, levels=None):
    """The whole chain of a texture: [level0, level1, ...], prosper's level count unless `levels` says otherwise."""
    level0 = np.ascontiguousarray(level0, np.uint8)
    n = mip_level_count(level0.shape[1], level0.shape[0]) if levels is None else levels
    chain = [level0]
    for _ in range(1, n):
        chain.append(generate_level(chain[-1], srgb))
    return chain


# ---- one level's sample (pt_device.hpp texel_taps / filter_taps) ----
def f2i(x):
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        r = np.where(np.isnan(x), 0, np.clip(np.nan_to_num(x.astype(np.float64), nan=0.0), -2147483648.0, 2147483647.0)).astype(np.int64)
    return r


def floor_mod(i, period):
    return np.mod(i, period)


def wrap_coord(i, size, mode):
    if mode == REPEAT:
        return floor_mod(i, size)
    if mode == MIRRORED_REPEAT:
        m = floor_mod(i, 2 * size)
        return np.where(m < size, m, 2 * size - 1 - m)
    return np.clip(i, 0, size - 1)


def wrap_pair(i, size, mode):
    if mode in (REPEAT, MIRRORED_REPEAT):
        period = size if mode == REPEAT else 2 * size
        m = floor_mod(i, period)
        n = np.where(m + 1 == period, 0, m + 1)
        return np.where(m < size, m, period - 1 - m), np.where(n < size, n, period - 1 - n)
    return np.clip(i, 0, size - 1), np.where(i < -1, 0, np.where(i >= size - 1, size - 1, i + 1))


def unpack(texels):
    return (texels.astype(F) * K255).astype(F)


def sample_level(level, filt, wrap_s, wrap_t, uv):
    """One level through filter `filt` (NEAREST, anything else is linear) and the wrap modes: float32 [n, 4]."""
    h, w = level.shape[:2]
    uv = np.asarray(uv, F).reshape(-1, 2)
    if filt == NEAREST:
        i = wrap_coord(f2i(np.floor((uv[:, 0] * F(w)).astype(F))), w, wrap_s)
        j = wrap_coord(f2i(np.floor((uv[:, 1] * F(h)).astype(F))), h, wrap_t)
        return unpack(level[j, i])
    u = fma(uv[:, 0], F(w), F(-0.5))
    v = fma(uv[:, 1], F(h), F(-0.5))
    fu, fv = np.floor(u).astype(F), np.floor(v).astype(F)
    a, b = (u - fu).astype(F), (v - fv).astype(F)
    i0, i1 = wrap_pair(f2i(fu), w, wrap_s)
    j0, j1 = wrap_pair(f2i(fv), h, wrap_t)
    t00, t10, t01, t11 = unpack(level[j0, i0]), unpack(level[j0, i1]), unpack(level[j1, i0]), unpack(level[j1, i1])
    one = F(1.0)
    w00 = ((one - a) * (one - b)).astype(F)[:, None]
    w10 = (a * (one - b)).astype(F)[:, None]
    w01 = ((one - a) * b).astype(F)[:, None]
    w11 = (a * b).astype(F)[:, None]
    return fma(w11, t11, fma(w01, t01, fma(w10, t10, (w00 * t00).astype(F))))


# ---- level selection and the trilinear sample ----
def texture_lambda(width, height, derivatives, bias):
    """lambda per record: derivatives float32 [n, 4] = (du/dx, dv/dx, du/dy, dv/dy)."""
    d = np.asarray(derivatives, F).reshape(-1, 4)
    w, h = F(width), F(height)
    with np.errstate(all="ignore"):
        ax, ay = (d[:, 0] * w).astype(F), (d[:, 1] * h).astype(F)
        bx, by = (d[:, 2] * w).astype(F), (d[:, 3] * h).astype(F)
        rho_x = np.sqrt(fma(ay, ay, (ax * ax).astype(F))).astype(F)
        rho_y = np.sqrt(fma(by, by, (bx * bx).astype(F))).astype(F)
        rho = np.maximum(rho_x, rho_y).astype(F)
        bad = ~np.isfinite(d).all(axis=1) | ~np.isfinite(rho)
        zero = rho == 0
        lam = (log2_(np.where(bad | zero, F(1.0), rho).astype(F)) + F(bias)).astype(F)
    lam = np.where(zero, F(-np.inf), lam)
    return np.where(bad, F(np.inf), lam).astype(F)


def lod_levels(lam, level_count):
    """-> (lo, hi, fraction) of every lambda > 0."""
    lam = np.asarray(lam, F)
    last = level_count - 1
    clamped = lam >= F(last)
    with np.errstate(all="ignore"):
        fl = np.floor(np.where(clamped, F(last), lam)).astype(F)
        lo = np.where(clamped, last, fl.astype(np.int64))
        frac = np.where(clamped, F(0.0), (lam - fl).astype(F)).astype(F)
    return lo, np.where(clamped, last, lo + 1), frac


def sample_texture_lod(chain, sampler, uv, derivatives, bias):
    """texture(sampler2D, uv) with explicit derivatives over a chain [level0, level1, ...]; sampler = (magFilter,
    minFilter, wrapS, wrapT).  -> (float32 [n, 4] RGBA, float32 [n] lambda)."""
    mag, min_, ws, wt = sampler
    uv = np.asarray(uv, F).reshape(-1, 2)
    h, w = chain[0].shape[:2]
    lam = texture_lambda(w, h, derivatives, bias)
    out = sample_level(chain[0], mag, ws, wt, uv)  # lambda <= 0: the LOD-0 sample
    minified = lam > 0
    if minified.any():
        idx = np.nonzero(minified)[0]
        lo, hi, frac = lod_levels(lam[idx], len(chain))
        a = np.zeros((idx.size, 4), F)
        b = np.zeros((idx.size, 4), F)
        for l in range(len(chain)):
            for which, dst in ((lo, a), (hi, b)):
                sel = which == l
                if sel.any():
                    dst[sel] = sample_level(chain[l], min_, ws, wt, uv[idx[sel]])
        f = frac[:, None]
        g = (F(1.0) - f).astype(F)
        out[idx] = fma(f, b, (g * a).astype(F))
    return out, lam


def sample_material_lod(chains, samplers, factors, uv, derivatives, bias, normal_chain=None, normal_sampler=None, alpha_factor=1.0):
    """sample_material_lod (pt_device.hpp): chains = (base colour chain, metallic-roughness chain), samplers likewise,
    factors = (baseColorFactor rgb, roughnessFactor, metallicFactor).  -> (albedo float32 [n, 3], roughness [n],
    metallic [n], [with `normal_chain`: the tangent-space normal fmaf(sample, 2, -1) [n, 3],] base.a * alpha_factor [n]).
    Each texture takes its own lambda from the same derivatives; a packed material's level 0 holds the same texels and
    goes through the same arithmetic."""
    base, _ = sample_texture_lod(chains[0], samplers[0], uv, derivatives, bias)
    mr, _ = sample_texture_lod(chains[1], samplers[1], uv, derivatives, bias)
    rgb, rf, mf = factors
    albedo = (srgb_to_linear(base[:, :3]) * np.asarray(rgb, F)[None, :]).astype(F)
    roughness = np.maximum((mr[:, 1] * F(rf)).astype(F), F(0.05)).astype(F)
    metallic = (mr[:, 2] * F(mf)).astype(F)
    out = (albedo, roughness, metallic)
    if normal_chain is not None:
        n, _ = sample_texture_lod(normal_chain, normal_sampler, uv, derivatives, bias)
        out = out + (fma(n[:, :3], F(2.0), F(-1.0)),)
    return out + ((base[:, 3] * F(1.0 if alpha_factor is None else alpha_factor)).astype(F),)


def normalize3(v):
    """pt_math.hpp normalize: a * (1 / sqrt(dot(a, a))), dot = fmaf(z, z, fmaf(y, y, x * x))."""
    v = np.asarray(v, F)
    d = fma(v[..., 2], v[..., 2], fma(v[..., 1], v[..., 1], (v[..., 0] * v[..., 0]).astype(F)))
    inv = (F(1.0) / np.sqrt(d).astype(F)).astype(F)
    return (v * inv[..., None]).astype(F)


def mapped_normal_axis_frame(tsn, sign=1.0):
    """mapped_normal (pt_device.hpp) for the frame normal (0, 0, 1), tangent (1, 0, 0, sign): the bitangent is
    cross(n, t) * sign = (0, sign, 0) and every other term of the sum is an exact zero, so the result is
    normalize((tsn.x, sign * tsn.y, tsn.z))."""
    tsn = np.asarray(tsn, F)
    return normalize3(np.stack([tsn[..., 0], (tsn[..., 1] * F(sign)).astype(F), tsn[..., 2]], axis=-1))


def signed_oct_encode(n):
    """gbuffer.frag:41-58 as pt_gbuffer_kernels.hip evaluates it (no contraction: a product, then a sum)."""
    n = np.asarray(n, F)
    s = ((np.abs(n[..., 0]) + np.abs(n[..., 1])).astype(F) + np.abs(n[..., 2])).astype(F)
    x, y, z = (n[..., 0] / s).astype(F), (n[..., 1] / s).astype(F), (n[..., 2] / s).astype(F)
    oy = ((y * F(0.5)).astype(F) + F(0.5)).astype(F)
    ox = ((x * F(0.5)).astype(F) + oy).astype(F)
    oy = ((x * F(-0.5)).astype(F) + oy).astype(F)
    with np.errstate(all="ignore"):
        oz = np.clip((z * F(3.40282e+38)).astype(F), F(0.0), F(1.0)).astype(F)
    return np.stack([ox, oy, oz], axis=-1)


# ---- the float64 side of the primary ray's uv differences ----
def camera_ray_terms(cam):
    """eye, right, up, fwd, aspect, tanHalfFovY as the G-buffer's pinhole ray takes them from CameraUniforms."""
    c = cam.worldToCamera.col
    right = np.array([c[0].x, c[1].x, c[2].x], np.float64)
    up = np.array([c[0].y, c[1].y, c[2].y], np.float64)
    fwd = -np.array([c[0].z, c[1].z, c[2].z], np.float64)
    c00, c11 = float(cam.cameraToClip.col[0].x), float(cam.cameraToClip.col[1].y)
    eye = np.array([cam.eye.x, cam.eye.y, cam.eye.z], np.float64)
    return eye, right, up, fwd, c11 / c00, 1.0 / c11


def analytic_derivatives(cam, width, height, plane_point, plane_normal, uv_of_point):
    """Float64: per pixel, the uv at the pixel centre's ray and the forward differences towards (px + 1, py) and
    (px, py + 1) on the plane - uv_of_point maps world points [..., 3] to uv [..., 2].  -> (uv [h, w, 2], d [h, w, 4])."""
    eye, right, up, fwd, aspect, tan_half = camera_ray_terms(cam)
    n = np.asarray(plane_normal, np.float64)

    def uv_at(dx, dy):
        x = (np.arange(width)[None, :] + 0.5 + dx) / width * 2.0 - 1.0
        y = (np.arange(height)[:, None] + 0.5 + dy) / height * 2.0 - 1.0
        d = (x[..., None] * right * tan_half * aspect) + (y[..., None] * up * tan_half) + fwd
        t = np.dot(np.asarray(plane_point, np.float64) - eye, n) / np.dot(d, n)
        assert (t > 0).all()
        return uv_of_point(eye + d * t[..., None])

    uv0, uvx, uvy = uv_at(0, 0), uv_at(1, 0), uv_at(0, 1)
    return uv0, np.concatenate([uvx - uv0, uvy - uv0], axis=-1)


def lambda64(width, height, d, bias=0.0):
    d = np.asarray(d, np.float64)
    rx = np.hypot(d[..., 0] * width, d[..., 1] * height)
    ry = np.hypot(d[..., 2] * width, d[..., 3] * height)
    return np.log2(np.maximum(rx, ry)) + bias


# ---- a running forward error analysis of the derivative sequence ("the derivative bound") ----
U32 = 2.0 ** -24  # unit roundoff of float32


class Err:
    """A quantity of the float32 sequence: `v`, its value in exact (float64) arithmetic, and `e`, a bound on
    |computed - v|.  Every operation adds its own rounding, U32 * (|result| + propagated error), to the first-order
    propagation of its operands' bounds (products of two bounds included)."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    @staticmethod
    def _round(v, prop):
        return Err(v, prop + U32 * (np.abs(v) + prop))

    def __add__(self, o):
        o = Err.of(o)
        return Err._round(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = Err.of(o)
        return Err._round(self.v - o.v, self.e + o.e)

    def __neg__(self):
        return Err(-self.v, self.e)

    def __mul__(self, o):
        o = Err.of(o)
        return Err._round(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = Err.of(o)
        lo = np.abs(o.v) - o.e
        assert (lo > 0).all(), "a divisor's bound reaches zero"
        q = self.v / o.v
        return Err._round(q, (self.e + np.abs(q) * o.e) / lo)

    def sqrt(self):
        lo = self.v - self.e
        assert (lo > 0).all()
        r = np.sqrt(self.v)
        return Err._round(r, self.e / (2.0 * np.sqrt(lo)))


def efma(a, b, c):
    """fmaf(a, b, c): one rounding."""
    a, b, c = Err.of(a), Err.of(b), Err.of(c)
    return Err._round(a.v * b.v + c.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e + c.e)


def edot(a, b):
    return efma(a[2], b[2], efma(a[1], b[1], a[0] * b[0]))


def ecross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def esub3(a, b):
    return [Err.of(a[k]) - Err.of(b[k]) for k in range(3)]


def epinhole(cam, width, height, dx, dy):
    """pinhole_camera_ray through (px + 0.5 + dx, py + 0.5 + dy) for every pixel: the direction's three components."""
    eye, right, up, fwd, aspect, tan_half = camera_ray_terms(cam)
    x = Err(np.broadcast_to(np.arange(width)[None, :] + 0.5 + dx, (height, width))) / Err(float(width))
    y = Err(np.broadcast_to(np.arange(height)[:, None] + 0.5 + dy, (height, width))) / Err(float(height))
    ndx, ndy = efma(x, 2.0, -1.0), efma(y, 2.0, -1.0)
    d = []
    for k in range(3):
        tx = ((Err(right[k]) * ndx) * Err(tan_half)) * Err(aspect)
        ty = (Err(up[k]) * ndy) * Err(tan_half)
        d.append((tx + ty) + Err(fwd[k]))
    inv = Err(1.0) / edot(d, d).sqrt()
    return [c * inv for c in d], [Err(np.full((height, width), e)) for e in eye]


def lambda_error_bound(cam, width, height, triangle, corner_uvs, extent, log2_error=2.0 ** -18, readout_error=4e-6):
    """A bound on |lambda_gpu - lambda_exact| per pixel for one world-space triangle (three corners and their uvs, exact
    float32 inputs: binary16 values under an identity transform) extended over the whole image: the hit's uv through
    edge_functions / finish_triangle / interpolate, the neighbours' through ray_uv_difference, texture_lambda with log2_
    taken within `log2_error` (tests/test_texture_lod_cpu.py measures that over the range), and `readout_error` for
    reading lambda off the blended roughness (a value below 0.47 with at most ten roundings, times 255 / 20).
    -> (bound [h, w], lambda in exact arithmetic [h, w], the bounds of the four uv differences [h, w, 4])."""
    P = [[Err(float(c)) for c in p] for p in triangle]
    T = [[Err(float(c)) for c in t] for t in corner_uvs]
    d0, o = epinhole(cam, width, height, 0.0, 0.0)
    # the hit: edge_functions, finish_triangle's barycentrics, interpolate's uv
    A, B, C_ = esub3(P[0], o), esub3(P[1], o), esub3(P[2], o)
    Uf, Vf, Wf = edot(d0, ecross(C_, B)), edot(d0, ecross(A, C_)), edot(d0, ecross(B, A))
    inv = Err(1.0) / ((Uf + Vf) + Wf)
    bu, bv = Vf * inv, Wf * inv
    a = (Err(1.0) - bu) - bv
    uv = [efma(T[2][k], bv, efma(T[1][k], bu, T[0][k] * a)) for k in range(2)]
    # the neighbours: ray_uv_difference
    e1, e2 = esub3(P[1], P[0]), esub3(P[2], P[0])
    n = ecross(e1, e2)
    d00, d01, d11 = edot(e1, e1), edot(e1, e2), edot(e2, e2)
    den = efma(d00, d11, -(d01 * d01))
    diffs = []
    for dx, dy in ((1.0, 0.0), (0.0, 1.0)):
        dn, _ = epinhole(cam, width, height, dx, dy)
        t = edot(n, esub3(P[0], o)) / edot(n, dn)
        q = esub3([efma(dn[k], t, o[k]) for k in range(3)], P[0])
        d20, d21 = edot(q, e1), edot(q, e2)
        b1 = efma(d11, d20, -(d01 * d21)) / den
        b2 = efma(d00, d21, -(d01 * d20)) / den
        for k in range(2):
            diffs.append(efma(b2, T[2][k] - T[0][k], efma(b1, T[1][k] - T[0][k], T[0][k])) - uv[k])
    # texture_lambda
    w, h = Err(float(extent[0])), Err(float(extent[1]))
    ax, ay, bx, by = diffs[0] * w, diffs[1] * h, diffs[2] * w, diffs[3] * h
    rx, ry = efma(ay, ay, ax * ax).sqrt(), efma(by, by, bx * bx).sqrt()
    rho_v = np.maximum(rx.v, ry.v)
    rho_e = np.maximum(rx.e, ry.e)  # |max(a', b') - max(a, b)| <= max(|a' - a|, |b' - b|)
    assert (rho_v - rho_e > 0).all()
    lam_e = rho_e / ((rho_v - rho_e) * np.log(2.0)) + log2_error
    lam_e = lam_e + U32 * (np.abs(np.log2(rho_v)) + lam_e) + readout_error
    return lam_e, np.log2(rho_v), np.stack([x.e for x in diffs], axis=-1)


def quad_error_bounds(cam, width, height, corners, corner_uvs, extent):
    """lambda_error_bound over both triangles of a quad, (0, 1, 2) and (0, 2, 3), the larger bound at every pixel (either
    triangle's formulas hold on the whole plane, so no pixel has to be assigned to one)."""
    out = [lambda_error_bound(cam, width, height, [corners[i] for i in tri], [corner_uvs[i] for i in tri], extent)
           for tri in ((0, 1, 2), (0, 2, 3))]
    return np.maximum(out[0][0], out[1][0]), np.maximum(out[0][2], out[1][2])
