"""NumPy restatement of prosper's two ReSTIR-DI resampling passes (not a test module), for
tests/test_restir_di_resampling.py:

  initial(...)   res/shader/restir_di/initial_reservoirs.comp:31-60  RIS over 5 uniformly drawn lights
  spatial(...)   res/shader/restir_di/spatial_reuse.comp:33-134      resampling of 5 neighbour reservoirs

Both return (light index int32 [h, w], unbiasedContributionWeight float64 [h, w], margin float64 [h, w]); spatial also
returns its neighbour lookups (which pixel looked at which, and whether the pair reached the normal test).

Arithmetic.  The random numbers (pcg3d, rngTo01: common/random.glsl) and everything computed from them alone are
restated bit for bit in uint32 / float32: the candidate index min(int(rnd01 * lightCount), lightCount - 1), the disc
offsets (sqrt and the products in float32, sin / cos from the oracle's PROSPER_PT_FN_SINCOS hook, the function the
device's sincos_ is pinned to), the bounds, and the 10 % depth test (linearizeDepth and the ratio are two float32
operations each).  Those decisions are exact and carry no margin.  The surface, sampleLight, evalBRDFTimesNoL and pHat
are computed in float64, so every decision that depends on them records how far it was from going the other way:
  - each accept test rnd01() < w / sum(w): |u - w / sum| / max(u, w / sum);
  - the normal test dot(n_q, n) < 0.9: |dot - 0.9| / 0.9;
  - where pHat is zero or not: |n.l| (NoL's saturate), |1 - (d / r)^4| (a point light's range), |cos * scale + offset|
    (a spot light's cone), each for every light pHat was evaluated for.
`margin` is the smallest of these per pixel (inf when every decision was exact).  A pixel whose sum of weights is 0 or
NaN selects nothing under either arithmetic (the comparison with NaN is false): index -1, decided.
"""
import numpy as np

from test_restir_di import make_gbuffer, signed_oct_encode  # noqa: F401  (the G-buffer of these tests)

F32 = np.float32
K_TWO_PI = F32(6.2831853)  # pt_math.hpp kTwoPi: the GLSL front end folds 2 * PI
SAMPLE_COUNT = 5


# ---- common/random.glsl ----

def pcg3d(x, y, z):
    """random.glsl:17-28 on uint32 arrays (wrapping arithmetic)."""
    x = x * np.uint32(1664525) + np.uint32(1013904223)
    y = y * np.uint32(1664525) + np.uint32(1013904223)
    z = z * np.uint32(1664525) + np.uint32(1013904223)
    x = x + y * z
    y = y + z * x
    z = z + x * y
    x = x ^ (x >> np.uint32(16))
    y = y ^ (y >> np.uint32(16))
    z = z ^ (z >> np.uint32(16))
    x = x + y * z
    y = y + z * x
    z = z + x * y
    return x, y, z


def rng_to_01(u):
    """random.glsl:42: float(u) / float(0xFFFFFFFF), the divisor rounding to 2^32 (a power of two: exact)."""
    return u.astype(F32) / F32(4294967296.0)


class Rng:
    """pcg_state = uvec3(px, py, frameIndex) per pixel; `mask` steps only the lanes that draw."""

    def __init__(self, px, py, frame):
        self.s = [np.asarray(px, np.uint32).copy(), np.asarray(py, np.uint32).copy(),
                  np.full(np.shape(px), frame, np.uint32)]

    def _step(self, mask):
        n = pcg3d(*self.s)
        if mask is None:
            self.s = list(n)
        else:
            for k in range(3):
                self.s[k] = np.where(mask, n[k], self.s[k])

    def rnd01(self, mask=None):
        self._step(mask)
        return rng_to_01(self.s[0])

    def rnd2d01(self, mask=None):
        self._step(mask)
        return rng_to_01(self.s[0]), rng_to_01(self.s[1])


# ---- the scene's lights (scene/lighting.glsl:58-89) as a table indexed by light index ----

class Lights:
    def __init__(self, world):
        world.freeze()  # "honor scene lighting": no sun in a scene with punctual lights only
        d = world.directional
        npt, nsp = world.point_lights.count, world.spot_lights.count
        self.count = 1 + npt + nsp
        n = self.count + 1  # + one "no light" entry for indices past the end
        self.kind = np.full(n, 3, np.int32)  # 0 sun, 1 point, 2 spot, 3 none
        self.pos = np.zeros((n, 3))
        self.rad = np.zeros((n, 3))
        self.w0 = np.ones(n)
        self.off = np.zeros(n)
        self.dir = np.zeros((n, 3))
        self.kind[0] = 0
        sd = np.array([d.direction.x, d.direction.y, d.direction.z], np.float64)
        self.sun_l = -sd / np.linalg.norm(sd)
        self.rad[0] = [d.irradiance.x, d.irradiance.y, d.irradiance.z]
        for i in range(npt):
            L = world.point_lights.lights[i]
            self.kind[1 + i] = 1
            self.pos[1 + i] = [L.position.x, L.position.y, L.position.z]
            self.rad[1 + i] = [L.radianceAndRadius.x, L.radianceAndRadius.y, L.radianceAndRadius.z]
            self.w0[1 + i] = L.radianceAndRadius.w
        for i in range(nsp):
            L = world.spot_lights.lights[i]
            j = 1 + npt + i
            self.kind[j] = 2
            self.pos[j] = [L.positionAndAngleOffset.x, L.positionAndAngleOffset.y, L.positionAndAngleOffset.z]
            self.off[j] = L.positionAndAngleOffset.w
            self.rad[j] = [L.radianceAndAngleScale.x, L.radianceAndAngleScale.y, L.radianceAndAngleScale.z]
            self.w0[j] = L.radianceAndAngleScale.w
            self.dir[j] = [L.direction.x, L.direction.y, L.direction.z]

    def sample(self, index, p):
        """sampleLight for light `index` (int array) at positions p [n, 3] -> l, irradiance, zero-margin."""
        j = np.where((index >= 0) & (index < self.count), index, self.count)
        kind = self.kind[j]
        to = self.pos[j] - p
        d2 = (to * to).sum(-1)
        d = np.sqrt(d2)
        with np.errstate(all="ignore"):
            l_punct = to / d[:, None]
            rr = (d / self.w0[j]) ** 4
            att_point = np.clip(1.0 - rr, 0.0, 1.0)
            cone = (-self.dir[j] * l_punct).sum(-1) * self.w0[j] + self.off[j]
            att_spot = np.clip(cone, 0.0, 1.0) ** 2
            att = np.where(kind == 1, att_point, att_spot)
            irr = self.rad[j] * (att / d2)[:, None]
        sun = kind == 0
        none = kind == 3
        l = np.where(sun[:, None], self.sun_l, l_punct)
        l = np.where(none[:, None], np.array([0.0, 1.0, 0.0]), l)
        irr = np.where(sun[:, None], self.rad[j], irr)
        irr = np.where(none[:, None], 0.0, irr)
        margin = np.where(kind == 1, np.abs(1.0 - rr), np.where(kind == 2, np.abs(cone), np.inf))
        return l, irr, margin


# ---- surface and BRDF (brdf.glsl:9-87) in float64 ----

def signed_oct_decode(n):
    """material.glsl:20-32, float64, n = (x, y, z) [..., 3]."""
    o = np.empty(n.shape)
    o[..., 0] = n[..., 0] - n[..., 1]
    o[..., 1] = n[..., 0] + n[..., 1] - 1.0
    o[..., 2] = (n[..., 2] * 2.0 - 1.0) * (1.0 - np.abs(o[..., 0]) - np.abs(o[..., 1]))
    with np.errstate(all="ignore"):
        return o / np.linalg.norm(o, axis=-1, keepdims=True)


class Surfaces:
    """VisibleSurface of every pixel (initial_reservoirs.comp:70-87): uv = px / size, worldPos through clipToWorld,
    the signed-octahedral normal; also the float32 linear depth the spatial pass compares."""

    def __init__(self, cam, ar, nm, depth):
        h, w = depth.shape
        self.h, self.w = h, w
        py, px = np.mgrid[0:h, 0:w]
        self.px, self.py = px.ravel().astype(np.uint32), py.ravel().astype(np.uint32)
        c2w = np.frombuffer(bytes(cam.clipToWorld), np.float32).reshape(4, 4).T.astype(np.float64)
        clip = np.stack([px.ravel() / w * 2.0 - 1.0, py.ravel() / h * 2.0 - 1.0, depth.ravel().astype(np.float64),
                         np.ones(h * w)], axis=-1)
        v = clip @ c2w.T
        with np.errstate(all="ignore"):
            self.pos = v[:, :3] / v[:, 3:4]
            eye = np.array([cam.eye.x, cam.eye.y, cam.eye.z], np.float64)
            iv = eye - self.pos
            self.v = iv / np.linalg.norm(iv, axis=-1, keepdims=True)
        nmv = nm.reshape(-1, 4).astype(np.float64)
        self.n = signed_oct_decode(nmv[:, [0, 1, 3]])
        self.metal = nmv[:, 2]
        arv = ar.reshape(-1, 4).astype(np.float64)
        self.albedo, self.rough = arv[:, :3], arv[:, 3]
        with np.errstate(all="ignore"):
            self.NoV = np.clip((self.n * self.v).sum(-1), 0.0, 1.0)
        c2c = np.frombuffer(bytes(cam.cameraToClip), np.float32).reshape(4, 4).T  # [row, col]
        with np.errstate(all="ignore"):
            self.lin_depth = (-c2c[2, 3]) / (depth.ravel() + c2c[2, 2])  # float32, scene/camera.glsl:11-22


def brdf_parts(sf, l, idx=slice(None)):
    """The terms of evalBRDFTimesNoL (brdf.glsl:67-87) for the pixels `idx` of `sf` and directions l [n, 3]: the diffuse
    and the specular term (each times NoL) [n, 3], n.l [n], and trowbridgeReitz's denominator NoH^2 (a2 - 1) + 1 [n]."""
    n, v, albedo, rough, metal, NoV = sf.n[idx], sf.v[idx], sf.albedo[idx], sf.rough[idx], sf.metal[idx], sf.NoV[idx]
    with np.errstate(all="ignore"):
        hv = v + l
        hv = hv / np.linalg.norm(hv, axis=-1, keepdims=True)
        nl = (n * l).sum(-1)
        NoL = np.clip(nl, 0.0, 1.0)
        NoH = np.clip((n * hv).sum(-1), 0.0, 1.0)
        VoH = np.clip((v * hv).sum(-1), 0.0, 1.0)
        m = metal[:, None]
        f0 = 0.04 * (1.0 - m) + albedo * m
        cdiff = albedo * 0.96 * (1.0 - m)
        alpha = rough * rough
        a2 = alpha * alpha
        den = NoH * NoH * (a2 - 1.0) + 1.0
        D = a2 / (np.pi * den * den)
        F = f0 + (1.0 - f0) * ((1.0 - VoH) ** 5)[:, None]
        k = np.maximum(alpha * 0.5, 0.0001)
        G = NoL / (NoL * (1.0 - k) + k) * (NoV / (NoV * (1.0 - k) + k))
        spec = F * (D * G / (4.0 * NoL * NoV + 0.0001))[:, None]
        return (cdiff / np.pi) * NoL[:, None], spec * NoL[:, None], nl, den


def brdf_times_nol(sf, l, idx=slice(None)):
    """evalBRDFTimesNoL (brdf.glsl:67-87) for the pixels `idx` of `sf` and directions l [n, 3]."""
    with np.errstate(all="ignore"):
        diffuse, spec, nl, _ = brdf_parts(sf, l, idx)
        return diffuse + spec, np.abs(nl)


def light_contribution(sf, lights, index, idx=slice(None)):
    """irradiance * evalBRDFTimesNoL per channel (float64) and the zero-margin of that evaluation."""
    l, irr, m_light = lights.sample(index, sf.pos[idx])
    b, m_nol = brdf_times_nol(sf, l, idx)
    return irr * b, np.minimum(m_light, m_nol)


def p_hat(sf, lights, index, idx=slice(None)):
    """pHatLight (resampling_phat.glsl): luminance (math.glsl:15) of light_contribution."""
    f, m = light_contribution(sf, lights, index, idx)
    return f @ np.array([0.299, 0.587, 0.114]), m


def _accept_margin(u, ratio, exact):
    with np.errstate(all="ignore"):
        m = np.abs(u - ratio) / np.maximum(u, ratio)
    return np.where(exact | np.isnan(ratio) | (ratio == 0.0), np.inf, m)


def initial(world, cam, ar, nm, depth, frame):
    """initial_reservoirs.comp for every pixel -> (index, W, margin)."""
    sf = Surfaces(cam, ar, nm, depth)
    lights = Lights(world)
    lc = lights.count
    rng = Rng(sf.px, sf.py, frame)
    npx = sf.px.size
    chosen = np.full(npx, -1, np.int32)
    chosen_ph = np.zeros(npx)
    total = np.zeros(npx)
    margin = np.full(npx, np.inf)
    for _ in range(SAMPLE_COUNT):
        cand = np.minimum((rng.rnd01() * F32(lc)).astype(np.int32), lc - 1)  # float32 product, truncation: exact
        ph, mz = p_hat(sf, lights, cand)
        w = (0.2 * ph) * lc
        total = total + w
        with np.errstate(all="ignore"):
            ratio = w / total
        u = rng.rnd01().astype(np.float64)
        take = u < ratio
        margin = np.minimum(margin, np.minimum(mz, _accept_margin(u, ratio, (w == total) & (w > 0))))
        chosen = np.where(take, cand, chosen)
        chosen_ph = np.where(take, ph, chosen_ph)
    with np.errstate(all="ignore"):
        W = np.where(chosen >= 0, total / chosen_ph, 0.0)
    undecidable_sum = ~(total > 0)  # 0 or NaN: nothing selected in either arithmetic
    margin = np.where(undecidable_sum & (chosen < 0), np.inf, margin)
    return chosen.reshape(sf.h, sf.w), W.reshape(sf.h, sf.w), margin.reshape(sf.h, sf.w)


def disc_offset(u0, u1, oracle):
    """ivec2(uniformSampleDisk(u) * 30 * 2 - 30) (sampling.glsl:8-13, spatial_reuse.comp:45-47) in float32."""
    r = np.sqrt(u0)
    sc = oracle.eval_fn("SINCOS", (K_TWO_PI * u1).reshape(-1, 1))
    sn, cs = sc[:, 0], sc[:, 1]
    ox = ((r * cs) * F32(30.0)) * F32(2.0) - F32(30.0)
    oy = ((r * sn) * F32(30.0)) * F32(2.0) - F32(30.0)
    return np.trunc(ox).astype(np.int64), np.trunc(oy).astype(np.int64)


def spatial(world, cam, ar, nm, depth, reservoirs, frame, oracle, lookups=False):
    """spatial_reuse.comp for every pixel over the input `reservoirs` [h, w, 2] -> (index, W, margin, lookups).
    The fourth value is None unless `lookups` is set; then it is (p, q, tested): for every neighbour lookup inside the
    image the flat indices of the pixel and of the neighbour, and whether the pair passed the depth test (`tested`: the
    normal test was evaluated on it)."""
    sf = Surfaces(cam, ar, nm, depth)
    lights = Lights(world)
    rng = Rng(sf.px, sf.py, frame)
    h, w, npx = sf.h, sf.w, sf.px.size
    px, py = sf.px.astype(np.int64), sf.py.astype(np.int64)
    in_idx = np.ascontiguousarray(reservoirs[..., 0]).view(np.int32).ravel()
    in_w = reservoirs[..., 1].astype(np.float64).ravel()
    margin = np.full(npx, np.inf)
    slots_idx, slots_w = [], []
    valid = np.zeros(npx, np.int64)
    look_p, look_q, look_t = [], [], []
    for _ in range(SAMPLE_COUNT):
        searching = np.ones(npx, bool)
        s_idx = np.full(npx, -1, np.int32)
        s_w = np.zeros(npx)
        for _ in range(5):  # while (kill++ < 5)
            u0, u1 = rng.rnd2d01(searching)
            ox, oy = disc_offset(u0, u1, oracle)
            qx, qy = px + ox, py + oy
            inside = searching & (qx > 0) & (qy > 0) & (qx < w) & (qy < h)
            q = np.where(inside, qy * w + qx, 0)
            with np.errstate(all="ignore"):
                depth_ok = ~(np.abs(F32(1.0) - sf.lin_depth[q] / sf.lin_depth) > F32(0.1))  # float32; NaN passes
                ndot = (sf.n[q] * sf.n).sum(-1)
            tested = inside & depth_ok
            if lookups:
                look_p.append(np.nonzero(inside)[0])
                look_q.append(q[inside])
                look_t.append(tested[inside])
            margin = np.where(tested, np.minimum(margin, np.abs(ndot - 0.9) / 0.9), margin)
            found = tested & ~(ndot < 0.9)
            s_idx = np.where(found, in_idx[q], s_idx)
            s_w = np.where(found, in_w[q], s_w)
            valid += found
            searching &= ~found
        slots_idx.append(s_idx)
        slots_w.append(s_w)
    chosen = np.full(npx, -1, np.int32)
    chosen_ph = np.zeros(npx)
    total = np.zeros(npx)
    for s_idx, s_w in zip(slots_idx, slots_w):
        live = s_idx >= 0
        ph, mz = p_hat(sf, lights, s_idx)
        wgt = np.where(live, ph * s_w, 0.0)
        total = np.where(live, total + wgt, total)
        with np.errstate(all="ignore"):
            ratio = wgt / total
        u = rng.rnd01(live).astype(np.float64)
        take = live & (u < ratio)
        m = np.minimum(mz, _accept_margin(u, ratio, (wgt == total) & (wgt > 0)))
        margin = np.where(live, np.minimum(margin, m), margin)
        chosen = np.where(take, s_idx, chosen)
        chosen_ph = np.where(take, ph, chosen_ph)
    with np.errstate(all="ignore"):
        W = np.where(chosen >= 0, (1.0 / np.maximum(valid, 1)) * total / chosen_ph, 0.0)
    margin = np.where(~(total > 0) & (chosen < 0), np.inf, margin)
    looked = (np.concatenate(look_p), np.concatenate(look_q), np.concatenate(look_t)) if lookups else None
    return chosen.reshape(h, w), W.reshape(h, w), margin.reshape(h, w), looked
