"""NumPy restatement of the forward transparent pass (not a test module), for tests/test_transparent.py and
tests/test_transparent_cpu.py: forward.frag's shading of a layer and prosper's blend state over a pixel's sorted layers,
in float64, over the layers the GPU's own debug read-back reports (as the restatements of (f8)-(f11) work over the
GPU's intermediate stages).

  composite_back_to_front / composite_front_to_back   the blend state over one pixel's stack, both arrangements
  LayerSurfaces(cam, layers)                           the VisibleSurface of every layer record
  shade(world, cam, sf, lists, maps)                   forward.frag:69-81 over given cluster lists (and IBL maps)
  composite(...)                                       the whole pass over (counts, layers, the input image)

The surface and BRDF code is tests/restir_resampling_reference.py's, the cluster lookup
tests/deferred_shading_reference.py's, evalIBL tests/ibl_reference.py's.
"""
import numpy as np

import deferred_shading_reference as D
import ibl_reference as I
import restir_resampling_reference as R


def composite_back_to_front(src, a, dst):
    """VkUtils.hpp:93-106 applied farthest layer first: rgb = src * a + dst * (1 - a).  src [k, 3], a [k], both front to
    back; dst [3].  Returns (rgb [3], alpha): alpha = a (1 - a) of the nearest layer, dst's alpha without layers."""
    rgb = np.asarray(dst, np.float64)[:3].copy()
    for k in range(len(a) - 1, -1, -1):
        rgb = np.asarray(src[k], np.float64) * a[k] + rgb * (1.0 - a[k])
    return rgb, (a[0] * (1.0 - a[0]) if len(a) else None)


def composite_front_to_back(src, a, dst):
    """The same as the pass evaluates it: C += T a src, T *= 1 - a, the end C + T dst; stops at T == 0."""
    c, t = np.zeros(3), 1.0
    for k in range(len(a)):
        if t == 0.0:
            break
        c = c + np.asarray(src[k], np.float64) * (t * a[k])
        t = t * (1.0 - a[k])
    return c + t * np.asarray(dst, np.float64)[:3], (a[0] * (1.0 - a[0]) if len(a) else None)


class LayerSurfaces:
    """forward.frag:50-67 for a flat array of layer records (the dtype of structs.TransparentLayer): what
    restir_resampling_reference.brdf_times_nol / light_contribution and ibl_reference.eval_ibl read of a Surfaces."""

    def __init__(self, cam, layers, px, py):
        self.pos = layers["positionWS"].astype(np.float64).reshape(-1, 3)
        eye = np.array([cam.eye.x, cam.eye.y, cam.eye.z], np.float64)
        iv = eye - self.pos
        self.v = iv / np.linalg.norm(iv, axis=-1, keepdims=True)
        self.n = layers["normal"].astype(np.float64).reshape(-1, 3)
        self.albedo = layers["albedo"].astype(np.float64).reshape(-1, 3)
        self.rough = layers["roughness"].astype(np.float64).ravel()
        self.metal = layers["metallic"].astype(np.float64).ravel()
        self.NoV = np.clip((self.n * self.v).sum(-1), 0.0, 1.0)
        self.px, self.py = np.asarray(px, np.int64), np.asarray(py, np.int64)
        # forward.mesh:75
        p1 = np.concatenate([self.pos, np.ones((len(self.pos), 1))], axis=-1)
        self.z_cam = (p1 @ D.mat(cam.worldToCamera).T)[:, 2]


def shade(world, cam, sf, lists=None, maps=None):
    """forward.frag:69-81 in float64 for every layer of `sf`: the sun, the point and the spot lights of the layer's
    cluster (`lists` as deferred_shading_reference.membership gives them; None: every light), then evalIBL over `maps`.
    Returns (rgb [n, 3], the sum of the absolute terms [n], slice margin [n])."""
    L = R.Lights(world)
    n_point, n_spot = world.point_lights.count, world.spot_lights.count
    n = len(sf.pos)
    b, _ = R.brdf_times_nol(sf, np.broadcast_to(L.sun_l, (n, 3)))
    color = L.rad[0] * b
    total = np.abs(color).sum(-1)
    s, beyond, margin = D.slices(cam, sf.z_cam)
    tx, ty = sf.px // D.DIM, sf.py // D.DIM
    for kind, count, offset in ((1, n_point, 1), (2, n_spot, 1 + n_point)):
        part = np.zeros((n, 3))
        for i in range(count):
            if lists is None:
                member = ~beyond & (kind == 1 or i < D.MAX_SPOTS)
            else:
                member = ~beyond & lists[kind - 1][s, ty, tx, i]
            if not member.any():
                continue
            c, _ = R.light_contribution(sf, L, np.full(n, offset + i))
            c = np.where(member[:, None], c, 0.0)
            part += c
            total += np.abs(c).sum(-1)
        color = color + part
    if maps is not None:
        ibl, ibl_total, _ = I.eval_ibl(sf, np.arange(n), maps)
        color = color + ibl
        total = total + ibl_total
    return color, total, margin


def composite(world, cam, counts, layers, hdr_in, lists=None, maps=None, sources=None):
    """The pass over the read-back (counts [h, w], layers [h, w, N]) and the input image [h, w, 4], float64.  `sources`
    [h, w, N, 3]: the layers' colours given (a debug draw type: alpha 1) instead of shaded.  Returns (rgb [h, w, 3],
    alpha [h, w] - NaN where there is no layer -, tolerance scale [h, w]: the pixel's sum of absolute terms, slice margin
    [h, w])."""
    h, w = counts.shape
    n_layers = layers.shape[2]
    assert counts.max(initial=0) <= n_layers, "the read-back holds fewer layers than a pixel has"
    py, px = np.mgrid[0:h, 0:w]
    k = np.arange(n_layers)
    live = k[None, None, :] < counts[..., None]
    flat = layers[live]
    sf = LayerSurfaces(cam, flat, np.broadcast_to(px[..., None], live.shape)[live], np.broadcast_to(py[..., None], live.shape)[live])
    if sources is None:
        color, total, margin = shade(world, cam, sf, lists, maps)
        alpha = flat["alpha"].astype(np.float64)
        alpha = np.where(alpha > 0.0, alpha, 1.0)  # forward.frag:83
    else:
        color = sources[live].astype(np.float64)
        total, margin, alpha = np.abs(color).sum(-1), np.full(len(flat), np.inf), np.ones(len(flat))
    src = np.zeros((h, w, n_layers, 3))
    a = np.zeros((h, w, n_layers))
    tot = np.zeros((h, w, n_layers))
    mar = np.full((h, w, n_layers), np.inf)
    src[live], a[live], tot[live], mar[live] = color, alpha, total, margin
    dst = hdr_in[..., :3].astype(np.float64)
    c, t, scale = np.zeros((h, w, 3)), np.ones((h, w)), np.zeros((h, w))
    for j in range(n_layers):  # a dead layer has a = 0: it changes nothing
        wgt = t * a[..., j]
        c = c + src[..., j, :] * wgt[..., None]
        scale = scale + tot[..., j] * np.abs(wgt)
        t = t * (1.0 - a[..., j])
    rgb = c + t[..., None] * dst
    scale = scale + np.abs(t) * np.abs(dst).sum(-1)
    out_alpha = np.where(counts > 0, a[..., 0] * (1.0 - a[..., 0]), np.nan)
    return rgb, out_alpha, scale, mar.min(axis=-1)
