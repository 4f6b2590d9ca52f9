"""NumPy restatement of prosper's image-based lighting (not a test module), for tests/test_image_based_lighting.py:

  sample_cube(cube, d)              seamless bilinear lookup of a [6, n, n, 4] cube (the path tracer's sample_skybox rule)
  irradiance(sky, face, i, j)       res/shader/ibl/sample_irradiance.comp at texels of the 64^2 cube
  prefilter(sky, mip, face, i, j)   res/shader/ibl/prefilter_radiance.comp at texels of mip `mip` (roughness mip / 10)
  brdf_lut(rows)                    res/shader/ibl/integrate_specular_brdf.comp, whole rows of the 512^2 LUT
  eval_ibl(sf, idx, maps)           scene/skybox.glsl evalIBL over read-back maps (Vulkan's trilinear rule)
  switch_margin(d)                  how far a direction is from the cube's face switch (float32 may pick the other face)

Everything is float64.  Two frame switches can go either way between float32 and float64 (the irradiance frame's
|n.y| < 0.99 and the sampler's |N.z| < 0.999); for a texel direction within FLIP_EPS of one, the branch is the one
float32 takes, and `near_switch` counts those texels.  One term is rounded as float32 rounds it: alpha^2 - 1 of the
importance sampling, exactly -1 in float32 at small roughness (tangent_half_vectors).
"""
import numpy as np

PI = 3.14159265  # common/math.glsl
IRR, RAD, MIPS, LUT, SAMPLES = 64, 512, 10, 512, 1024
FLIP_EPS = 1e-6


def texel_dirs(face, i, j, n):
    """The texel-centre direction of both cube passes (unnormalised), float64 [k, 3]."""
    face, i, j = np.broadcast_arrays(np.asarray(face), np.asarray(i), np.asarray(j))
    cx, cy = i + 0.5, j + 0.5
    res, h = float(n), n * 0.5
    one = np.full(cx.shape, h)
    table = [
        (one, (res - cy) - h, (res - cx) - h),
        (-one, (res - cy) - h, cx - h),
        (cx - h, one, cy - h),
        (cx - h, -one, (res - cy) - h),
        (cx - h, (res - cy) - h, one),
        ((res - cx) - h, (res - cy) - h, -one),
    ]
    out = np.zeros(cx.shape + (3,))
    for f, comps in enumerate(table):
        m = face == f
        out[m] = np.stack([c[m] for c in comps], -1)
    return out


def normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def normalize32(v):
    """normalize in float32 as the kernels do: v * (1 / sqrt(dot(v, v)))."""
    v = np.asarray(v, np.float32)
    d = v[..., 2] * v[..., 2] + (v[..., 1] * v[..., 1] + v[..., 0] * v[..., 0])
    return v * (np.float32(1.0) / np.sqrt(d))[..., None]


def face_coords(d):
    """Vulkan cube face selection: (face, sc, tc, ma) of directions d [k, 3]."""
    ax, ay, az = np.abs(d[..., 0]), np.abs(d[..., 1]), np.abs(d[..., 2])
    zsel = (az >= ax) & (az >= ay)
    ysel = ~zsel & (ay >= ax)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    face = np.where(zsel, np.where(z < 0, 5, 4), np.where(ysel, np.where(y < 0, 3, 2), np.where(x < 0, 1, 0)))
    sc = np.where(zsel, np.where(z < 0, -x, x), np.where(ysel, x, np.where(x < 0, z, -z)))
    tc = np.where(zsel, -y, np.where(ysel, np.where(y < 0, -z, z), -y))
    ma = np.where(zsel, az, np.where(ysel, ay, ax))
    return face, sc, tc, ma


def switch_margin(d):
    """The relative difference of the two largest |components| of directions d [k, 3]: below ~1e-5 float32 and float64
    may select different faces (the lookup is continuous there only as far as the two faces' texels agree)."""
    a = np.sort(np.abs(d), axis=-1)
    with np.errstate(all="ignore"):
        return (a[..., 2] - a[..., 1]) / a[..., 2]


def face_dir(face, sc, tc):
    one = np.ones_like(sc)
    table = [(one, -tc, -sc), (-one, -tc, sc), (sc, one, tc), (sc, -one, -tc), (sc, -tc, one), (-sc, -tc, -one)]
    out = np.zeros(sc.shape + (3,))
    for f, comps in enumerate(table):
        m = face == f
        out[m] = np.stack([c[m] for c in comps], -1)
    return out


def texel(cube, face, i, j):
    """Texels (i, j) in [-1, n] of faces: outside the face, the seamless-edge rule's texel of the neighbouring face."""
    n = cube.shape[1]
    out = (i < 0) | (j < 0) | (i >= n) | (j >= n)
    face, i, j = face.copy(), i.copy(), j.copy()
    if out.any():
        sc = 2.0 * (i[out] + 0.5) / n - 1.0
        tc = 2.0 * (j[out] + 0.5) / n - 1.0
        f2, sc2, tc2, ma2 = face_coords(face_dir(face[out], sc, tc))
        face[out] = f2
        i[out] = np.clip(np.floor((0.5 * sc2 / ma2 + 0.5) * n), 0, n - 1).astype(np.int64)
        j[out] = np.clip(np.floor((0.5 * tc2 / ma2 + 0.5) * n), 0, n - 1).astype(np.int64)
    return cube[face, j, i, :3]


def sample_cube(cube, d):
    """Seamless bilinear lookup (float weights) of cube float64 [6, n, n, 4] (or None: zero) in directions d [k, 3]."""
    if cube is None:
        return np.zeros(d.shape[:-1] + (3,))
    n = cube.shape[1]
    face, sc, tc, ma = face_coords(d)
    with np.errstate(all="ignore"):
        u = (0.5 * sc / ma + 0.5) * n - 0.5
        v = (0.5 * tc / ma + 0.5) * n - 0.5
    fu, fv = np.floor(u), np.floor(v)
    a, b = (u - fu)[..., None], (v - fv)[..., None]
    i0 = np.clip(np.nan_to_num(fu), -1, n - 1).astype(np.int64)
    j0 = np.clip(np.nan_to_num(fv), -1, n - 1).astype(np.int64)
    return ((1 - a) * (1 - b) * texel(cube, face, i0, j0) + a * (1 - b) * texel(cube, face, i0 + 1, j0)
            + (1 - a) * b * texel(cube, face, i0, j0 + 1) + a * b * texel(cube, face, i0 + 1, j0 + 1))


def sky64(world):
    return None if world.skybox is None else np.asarray(world.skybox, np.float64)


def irradiance(sky, face, i, j, chunk=16):
    """sample_irradiance.comp at texels (face, i, j) of the 64^2 cube: float64 [k, 3], and the texels near the switch."""
    d = texel_dirs(face, i, j, IRR)
    n = normalize(d)
    n32 = normalize32(d)
    near_switch = int((np.abs(np.abs(n[:, 1]) - 0.99) < FLIP_EPS).sum())
    up = np.where((np.abs(n32[:, 1]) < np.float32(0.99))[:, None], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0])
    right = normalize(np.cross(up, n))
    up = normalize(np.cross(n, right))
    theta = 0.5 * PI * np.arange(64) / 64.0
    phi = 2.0 * PI * np.arange(128) / 128.0
    st, ct = np.repeat(np.sin(theta), 128), np.repeat(np.cos(theta), 128)
    sp, cp = np.tile(np.sin(phi), 64), np.tile(np.cos(phi), 64)
    t = np.stack([st * cp, st * sp, ct], -1)  # [8192, 3]
    w = (ct * st)[None, :, None]
    out = np.empty((len(n), 3))
    for a in range(0, len(n), chunk):
        b = slice(a, a + chunk)
        vec = (t[None, :, 0:1] * right[b, None] + t[None, :, 1:2] * up[b, None] + t[None, :, 2:3] * n[b, None])
        s = np.minimum(sample_cube(sky, vec), 10.0)
        out[b] = PI * (s * w).sum(1) / 8192.0
    return out, near_switch


def bitreverse32(i):
    return np.array([int("{:032b}".format(int(k))[::-1], 2) for k in np.atleast_1d(i)], np.float64)


def tangent_half_vectors(alpha):
    """importanceSampleIBLTrowbridgeReitz's H of hammersley(i, 1024) around +Z: [1024, 3]."""
    i = np.arange(SAMPLES)
    xi0, xi1 = i / SAMPLES, bitreverse32(i) * 2.32830643653896e-10
    p = 2.0 * PI * xi0
    # alpha^2 - 1 as float32 rounds it: below alpha^2 = 2^-25 (roughness < 0.02) it is exactly -1 there and every
    # cos theta 1 (row 1 of the LUT is then row 0's)
    cos_t = np.sqrt((1.0 - xi1) / (1.0 + float(np.float32(alpha * alpha - 1.0)) * xi1))
    sin_t = np.sqrt(1.0 - cos_t * cos_t)
    return np.stack([sin_t * np.cos(p), sin_t * np.sin(p), cos_t], -1)


def tangent_frame(n, n32):
    up = np.where((np.abs(n32[..., 2]) < np.float32(0.999))[..., None], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0])
    tx = normalize(np.cross(up, n))
    return tx, normalize(np.cross(n, tx))


def prefilter(sky, mip, face, i, j, chunk=64):
    """prefilter_radiance.comp at texels of mip `mip`: float64 [k, 3], and the texels near the sampler's switch."""
    size = RAD >> mip
    d = texel_dirs(face, i, j, size)
    n, n32 = normalize(d), normalize32(d)
    near_switch = int((np.abs(np.abs(n[:, 2]) - 0.999) < FLIP_EPS).sum())
    tx, ty = tangent_frame(n, n32)
    alpha = (mip / MIPS) ** 2
    h = tangent_half_vectors(alpha)
    if mip == 0:
        h = h[:1]  # every half vector is N: the weighted mean of equal samples
    out = np.empty((len(n), 3))
    for a in range(0, len(n), chunk):
        b = slice(a, a + chunk)
        N = n[b, None]
        H = normalize(h[None, :, 0:1] * tx[b, None] + h[None, :, 1:2] * ty[b, None] + h[None, :, 2:3] * N)
        L = 2.0 * (N * H).sum(-1, keepdims=True) * H - N
        NoL = np.clip((N * L).sum(-1), 0.0, 1.0)
        s = np.minimum(sample_cube(sky, L), 10.0)
        wgt = np.where(NoL > 0, NoL, 0.0)[..., None]
        out[b] = (s * wgt).sum(1) / wgt.sum(1)
    return out, near_switch


def brdf_lut(rows):
    """integrate_specular_brdf.comp for whole rows: float64 [len(rows), 512, 2] after saturate (NaN -> 0)."""
    out = np.empty((len(rows), LUT, 2))
    NoV = np.arange(LUT) / LUT
    V = np.stack([np.sqrt(1.0 - NoV * NoV), np.zeros(LUT), NoV], -1)
    N = np.array([0.0, 0.0, 1.0])
    tx, ty = tangent_frame(N, N.astype(np.float32))
    for r, y in enumerate(rows):
        alpha = (y / LUT) ** 2
        h = tangent_half_vectors(alpha)
        H = normalize(h[:, 0:1] * tx + h[:, 1:2] * ty + h[:, 2:3] * N)  # [1024, 3]
        VdH = V @ H.T  # [512, 1024]
        Lz = 2.0 * VdH * H[None, :, 2] - V[:, 2:3]
        NoL, NoH, VoH = np.clip(Lz, 0, 1), np.clip(H[None, :, 2], 0, 1), np.clip(VdH, 0, 1)
        k = max(alpha * 0.5, 0.0001)
        nv = NoV[:, None]
        with np.errstate(all="ignore"):
            G = (NoL / (NoL * (1 - k) + k)) * (nv / (nv * (1 - k) + k))
            gvis = G * VoH / (NoH * nv)
        fc = (1.0 - VoH) ** 5
        m = NoL > 0
        A = np.where(m, (1 - fc) * gvis, 0.0).sum(1) / SAMPLES
        B = np.where(m, fc * gvis, 0.0).sum(1) / SAMPLES
        ab = np.stack([A, B], -1)
        out[r] = np.where(np.isnan(ab), 0.0, np.clip(ab, 0.0, 1.0))
    return out


def lut_codes(v):
    return np.rint(np.clip(v, 0.0, 1.0) * 65535.0).astype(np.int64)


def half_ulps(got_f16, want):
    """Distance in units in the last place between float16 results and float64 values rounded to float16 (both >= 0)."""
    g = np.asarray(got_f16, np.float16).view(np.uint16).astype(np.int64)
    w = np.asarray(want, np.float64).astype(np.float16).view(np.uint16).astype(np.int64)
    return np.abs(g - w)


# ---- evalIBL over read-back maps ----

def sample_radiance(levels, r, rough):
    """textureLod(skyboxRadiance, r, roughness * 10): the level clamped to [0, 9], floor and floor + 1 blended."""
    lod = np.clip(np.nan_to_num(rough * 10.0), 0.0, MIPS - 1.0)
    l0 = np.floor(lod).astype(np.int64)
    t = (lod - l0)[:, None]
    l1 = np.minimum(l0 + 1, MIPS - 1)
    c0, c1 = np.zeros(r.shape), np.zeros(r.shape)
    for m in range(MIPS):
        cube = np.asarray(levels[m], np.float64)
        for sel, c in ((l0 == m, c0), (l1 == m, c1)):
            if sel.any():
                c[sel] = sample_cube(cube, r[sel])
    return (1.0 - t) * c0 + t * c1


def sample_lut(lut, NoV, rough):
    """texture(specularBrdfLut, (NoV, roughness)).rg: bilinear, clamp-to-edge, codes / 65535."""
    tab = lut.astype(np.float64) / 65535.0
    u, v = NoV * LUT - 0.5, rough * LUT - 0.5
    fu, fv = np.floor(u), np.floor(v)
    a, b = (u - fu)[:, None], (v - fv)[:, None]
    i0, j0 = fu.astype(np.int64), fv.astype(np.int64)
    ia, ib = np.clip(i0, 0, LUT - 1), np.clip(i0 + 1, 0, LUT - 1)
    ja, jb = np.clip(j0, 0, LUT - 1), np.clip(j0 + 1, 0, LUT - 1)
    return ((1 - a) * (1 - b) * tab[ja, ia] + a * (1 - b) * tab[ja, ib] + (1 - a) * b * tab[jb, ia] + a * b * tab[jb, ib])


def eval_ibl(sf, idx, maps):
    """evalIBL for the pixels idx of restir_resampling_reference.Surfaces sf: float64 [k, 3], |terms| summed [k], and
    the smaller switch_margin of the two cube directions (the normal and the reflection vector) [k]."""
    n, v, albedo, rough, metal = sf.n[idx], sf.v[idx], sf.albedo[idx], sf.rough[idx], sf.metal[idx]
    m = metal[:, None]
    f0 = 0.04 * (1.0 - m) + albedo * m
    NoV = np.clip((n * v).sum(-1), 0.0, 1.0)
    F = f0 + (np.maximum(1.0 - rough[:, None], f0) - f0) * ((1.0 - NoV) ** 5)[:, None]
    kD = (1.0 - F) * (1.0 - m)
    diffuse = sample_cube(np.asarray(maps["irradiance"], np.float64), n) * albedo
    R = -v - 2.0 * (n * -v).sum(-1, keepdims=True) * n
    pref = sample_radiance(maps["radiance"], R, rough)
    env = sample_lut(maps["lut"], NoV, rough)
    spec = pref * (F * env[:, 0:1] + env[:, 1:2])
    margin = np.minimum(switch_margin(n), switch_margin(R))
    return kD * diffuse + spec, np.abs(kD * diffuse).sum(-1) + np.abs(spec).sum(-1), margin
