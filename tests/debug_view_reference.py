"""NumPy restatement of the inspection passes (pt_debug_view.hip): float32, one operation per rounding,
the matrix rows as chains of fused multiply-adds, so that the kernels' images can be compared bit for bit.

The debug lines' fragment rule is the library's own (Vulkan leaves non-strict lines to the implementation), so this file
IS its contract:
  * clip = cameraToClip * (worldToCamera * (p, 1));
  * a Liang-Barsky parameter interval against -w <= x, y <= w, 0 <= z <= w; a non-finite clip coordinate or an empty
    interval: the line is clipped away;
  * framebuffer coordinates of the clipped endpoints, clamped to the viewport; along the major axis one fragment per
    pixel centre in [start, end) (half-open); minor coordinate and z / w linear in screen space;
  * depth test strictly greater against the stored depth; per pixel the greatest (depth, line index) wins."""
import numpy as np

from particles_reference import fma

F = np.float32
LINE_FLOATS = 9
MAX_LINES = 100000


def mat4(m):
    """a S.Mat4 (column-major) -> [4, 4] float32, m[row, col]"""
    return np.array([[getattr(m.col[c], "xyzw"[r]) for c in range(4)] for r in range(4)], F)


def row_point(m, r, p):
    return fma(m[r, 2], p[2], fma(m[r, 1], p[1], fma(m[r, 0], p[0], m[r, 3])))


def row_vec(m, r, v):
    with np.errstate(all="ignore"):
        return fma(m[r, 3], v[3], fma(m[r, 2], v[2], fma(m[r, 1], v[1], m[r, 0] * v[0])))


def to_clip(world_to_camera, camera_to_clip, p):
    """cameraToClip * (worldToCamera * (p, 1)) -> [4] float32"""
    p = np.asarray(p, F)
    v = np.array([row_point(world_to_camera, r, p) for r in range(4)], F)
    return np.array([row_vec(camera_to_clip, r, v) for r in range(4)], F)


def plane_distances(c):
    with np.errstate(all="ignore"):
        return [c[3] + c[0], c[3] - c[0], c[3] + c[1], c[3] - c[1], c[2], c[3] - c[2]]


def clip_interval(c0, c1):
    """-> (t0, t1) float32, or None when the segment is clipped away"""
    if not (np.isfinite(c0).all() and np.isfinite(c1).all()):
        return None
    t0, t1 = F(0.0), F(1.0)
    with np.errstate(all="ignore"):
        for d0, d1 in zip(plane_distances(c0), plane_distances(c1)):
            if d0 < 0 and d1 < 0:
                return None
            if d0 < 0:
                t0 = np.fmax(t0, d0 / (d0 - d1))
            elif d1 < 0:
                t1 = np.fmin(t1, d0 / (d0 - d1))
    if not t0 <= t1:
        return None
    return t0, t1


def to_screen(c, width, height):
    """clip point -> (x, y, depth) in framebuffer coordinates clamped to the viewport, or None"""
    w = c[3]
    if not w > 0:
        return None
    with np.errstate(all="ignore"):
        sx = ((c[0] / w) * F(0.5) + F(0.5)) * F(width)
        sy = ((c[1] / w) * F(0.5) + F(0.5)) * F(height)
        sz = c[2] / w
    if not (np.isfinite(sx) and np.isfinite(sy) and np.isfinite(sz)):
        return None
    clamp = lambda v, hi: np.fmin(np.fmax(v, F(0.0)), F(hi))
    return clamp(sx, width), clamp(sy, height), clamp(sz, 1.0)


def screen_segment(line, world_to_camera, camera_to_clip, width, height):
    """-> ((ax, ay, az), (bx, by, bz)) of the clipped segment in framebuffer coordinates, or None: clipped away"""
    line = np.asarray(line, F)
    c0 = to_clip(world_to_camera, camera_to_clip, line[0:3])
    c1 = to_clip(world_to_camera, camera_to_clip, line[3:6])
    t = clip_interval(c0, c1)
    if t is None:
        return None
    t0, t1 = t
    with np.errstate(all="ignore"):
        d = c1 - c0
        a = c0 + t0 * d if t0 > 0 else c0
        b = c0 + t1 * d if t1 < 1 else c1
    a, b = to_screen(a, width, height), to_screen(b, width, height)
    if a is None or b is None:
        return None
    return a, b


def walk(a, b, width, height):
    """The fragments of the screen segment a -> b: (x int64 [n], y int64 [n], depth float32 [n]), in walking order."""
    (ax, ay, az), (bx, by, bz) = a, b
    dx, dy = bx - ax, by - ay
    x_major = abs(dx) >= abs(dy)
    m0, m1, dm = (ax, bx, dx) if x_major else (ay, by, dy)
    n0, dn = (ay, dy) if x_major else (ax, dx)
    major_extent, minor_extent = (width, height) if x_major else (height, width)
    if m1 > m0:
        first = int(np.ceil(m0 - F(0.5)))
        steps, step = int(np.ceil(m1 - F(0.5))) - first, 1
    elif m1 < m0:
        first = int(np.floor(m0 - F(0.5)))
        steps, step = first - int(np.floor(m1 - F(0.5))), -1
    else:
        steps, first, step = 0, 0, 1
    steps = min(max(steps, 0), max(width, height))
    k = first + step * np.arange(steps, dtype=np.int64)
    k = k[(k >= 0) & (k < major_extent)]
    t = ((k.astype(F) + F(0.5)) - m0) / dm if len(k) else np.zeros(0, F)
    q = np.clip(np.floor(n0 + t * dn).astype(np.int64), 0, minor_extent - 1)
    depth = np.fmin(np.fmax(az + t * (bz - az), F(0.0)), F(1.0)).astype(F)
    return (k, q, depth) if x_major else (q, k, depth)


def line_fragments(line, camera, width, height):
    """-> (x, y, depth) of one line's fragments before the depth test, or None when it is clipped away"""
    seg = screen_segment(line, mat4(camera.worldToCamera), mat4(camera.cameraToClip), width, height)
    if seg is None:
        return None
    return walk(seg[0], seg[1], width, height)


def debug_lines(lines, camera, width, height, hdr, depth):
    """prosper_pt_debug_lines -> (hdr, depth, info): info = dict(fragmentsWritten, linesClippedAway, winner int64 [h, w]:
    the line that wrote the pixel, -1 where none did)."""
    lines = np.asarray(lines, F).reshape(-1, LINE_FLOATS)
    assert len(lines) <= MAX_LINES
    w2c, c2c = mat4(camera.worldToCamera), mat4(camera.cameraToClip)
    keys = np.zeros((height, width), np.uint64)
    clipped = 0
    for i, line in enumerate(lines):
        seg = screen_segment(line, w2c, c2c, width, height)
        if seg is None:
            clipped += 1
            continue
        x, y, d = walk(seg[0], seg[1], width, height)
        with np.errstate(invalid="ignore"):
            passed = d > depth[y, x]
        x, y, d = x[passed], y[passed], d[passed]
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(i)
        np.maximum.at(keys, (y, x), key)
    wrote = keys != 0
    winner = np.where(wrote, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    out_hdr, out_depth = hdr.copy(), depth.copy()
    out_hdr[wrote, :3] = lines[winner[wrote], 6:9]
    out_hdr[wrote, 3] = F(1.0)
    out_depth[wrote] = (keys[wrote] >> np.uint64(32)).astype(np.uint32).view(F)
    return out_hdr, out_depth, {"fragmentsWritten": int(wrote.sum()), "linesClippedAway": clipped, "winner": winner}


# ---- the registry's formats and the one-texel readback (prosper_pt_texture_readback) ----

# bytes per texel of PROSPER_PT_DEBUG_FORMAT_* 0-7: RGBA32F, RG32F, R32F, RGBA16F, RG16F, R16F, RG16_UNORM, RGBA8_UNORM
FORMAT_BYTES = (16, 8, 4, 8, 4, 2, 4, 4)


def expand_texels(image):
    """A read-back image -> float32 [h, w, 4] as Vulkan returns its texels: float32 and float16 as they are (fp16 decodes
    exactly), uint16 codes / 65535, uint8 codes / 255; missing components read (0, 0, 1)."""
    a = np.asarray(image)
    if a.ndim == 2:
        a = a[..., None]
    if a.dtype == np.uint16:
        v = a.astype(F) / F(65535.0)
    elif a.dtype == np.uint8:
        v = a.astype(F) / F(255.0)
    else:
        v = a.astype(F)
    out = np.zeros(a.shape[:2] + (4,), F)
    out[..., 3] = F(1.0)
    out[..., :a.shape[2]] = v
    return out


def nearest_texel(px, extent):
    """clamp(floor(u * extent), 0, extent - 1) of u = px / extent, in float32"""
    e = F(extent)
    with np.errstate(all="ignore"):
        t = np.floor((F(px) / e) * e)
    if not t >= 0:
        return 0
    return extent - 1 if t >= e else int(t)


def texture_readback(image, px_x, px_y):
    """texture_readback.comp over a read-back image: float32 [4]"""
    texels = expand_texels(image)
    h, w = texels.shape[:2]
    return texels[nearest_texel(px_y, h), nearest_texel(px_x, w)]


# ---- the texture viewer (prosper_pt_texture_debug; texture_debug.comp as it is compiled) ----

CHANNEL_RGB, ABS_BEFORE_RANGE, ZOOM, MAGNIFIER = 4, 1 << 3, 1 << 4, 1 << 5


def in_res(res, lod):
    """inRes() = max(inRes / (1 << lod), 1)"""
    return max(res[0] >> lod, 1), max(res[1] >> lod, 1)


def aspect_corrected_uv(u, v, in_wh, out_wh, undo=False):
    """aspectCorrectedUv / unAspectCorrectedUv on float32 arrays (or scalars) u, v"""
    (iw, ih), (ow, oh) = in_wh, out_wh
    u, v = np.asarray(u, F), np.asarray(v, F)
    if (iw, ih) == (ow, oh):
        return u, v
    in_aspect, out_aspect = F(iw) / F(ih), F(ow) / F(oh)
    tall = in_aspect > out_aspect
    scale = in_aspect / out_aspect if tall else out_aspect / in_aspect
    shift = (scale - F(1.0)) * F(0.5)
    with np.errstate(all="ignore"):
        fix = (lambda c: (c + shift) / scale) if undo else (lambda c: c * scale - shift)
        return (u, fix(v)) if tall else (fix(u), v)


def zoom4x_uv(u, v):
    return u * F(0.25) + F(0.375), v * F(0.25) + F(0.375)


def unzoom4x_uv(u, v):
    return (u - F(0.375)) * F(4.0), (v - F(0.375)) * F(4.0)


def _clampi(i, n):
    return np.clip(i, 0, n - 1)


def _floor_int(x):
    """floor of a float32 array as int64, saturating like the kernel's float -> int (NaN -> 0)"""
    with np.errstate(all="ignore"):
        f = np.floor(x)
    return np.where(np.isnan(f), 0, np.clip(f, -2147483648.0, 2147483647.0)).astype(np.int64)


def sample_level(texels, u, v, bilinear):
    """textureLod with clamp-to-edge over one decoded level texels [h, w, 4]; u, v float32 arrays -> [..., 4]"""
    h, w = texels.shape[:2]
    u, v = np.asarray(u, F), np.asarray(v, F)
    with np.errstate(all="ignore"):
        if not bilinear:
            return texels[_clampi(_floor_int(v * F(h)), h), _clampi(_floor_int(u * F(w)), w)]
        cu, cv = u * F(w) - F(0.5), v * F(h) - F(0.5)
        fu, fv = np.floor(cu), np.floor(cv)
        a, b = cu - fu, cv - fv
        i0, j0 = _floor_int(cu), _floor_int(cv)
        ia, ib, ja, jb = _clampi(i0, w), _clampi(i0 + 1, w), _clampi(j0, h), _clampi(j0 + 1, h)
        w00, w10, w01, w11 = (F(1.0) - a) * (F(1.0) - b), a * (F(1.0) - b), (F(1.0) - a) * b, a * b
        t00, t10, t01, t11 = texels[ja, ia], texels[ja, ib], texels[jb, ia], texels[jb, ib]
        e = lambda x: x[..., None]
        return fma(e(w11), t11, fma(e(w01), t01, fma(e(w10), t10, e(w00) * t00)))


def to_unorm8(x):
    """tone_map_kernel's conversion: rint(clamp(x, 0, 1) * 255), NaN -> 0"""
    with np.errstate(all="ignore"):
        c = np.fmin(np.fmax(np.asarray(x, F), F(0.0)), F(1.0))
        return np.rint(c * F(255.0)).astype(np.uint8)


def snapped_cursor(cursor_uv, in_wh, out_wh, zoom):
    """the magnifier's sample uv, snapped to the nearest input texel centre: (su, sv) float32"""
    su, sv = aspect_corrected_uv(F(cursor_uv[0]), F(cursor_uv[1]), in_wh, out_wh)
    if zoom:
        su, sv = zoom4x_uv(su, sv)
    with np.errstate(all="ignore"):
        su = (np.floor(su * F(in_wh[0])) + F(0.5)) / F(in_wh[0])
        sv = (np.floor(sv * F(in_wh[1])) + F(0.5)) / F(in_wh[1])
    return F(su), F(sv)


def texture_debug(level_image, out_res, value_range=(0.0, 1.0), flags=CHANNEL_RGB, cursor_uv=(0.0, 0.0), bilinear=False):
    """prosper_pt_texture_debug over the read-back level the call views (its extent is inRes()) ->
    (rgba8 uint8 [outH, outW, 4], peek float32 [4] or None without the magnifier flag)"""
    texels = expand_texels(level_image)
    in_wh = (texels.shape[1], texels.shape[0])
    ow, oh = out_res
    zoom = bool(flags & ZOOM)
    oy, ox = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    u, v = (ox.astype(F) + F(0.5)) / F(ow), (oy.astype(F) + F(0.5)) / F(oh)
    u, v = aspect_corrected_uv(u, v, in_wh, (ow, oh))
    if zoom:
        u, v = zoom4x_uv(u, v)
    inside = (u >= 0) & (v >= 0) & (u <= 1) & (v <= 1)
    s = sample_level(texels, u, v, bilinear)
    channel = flags & 7
    colour = s[..., :3] if channel > 3 else np.repeat(s[..., channel:channel + 1], 3, axis=-1)
    colour = np.where(inside[..., None], colour, F(0.0)).astype(F)
    if flags & ABS_BEFORE_RANGE:
        colour = np.abs(colour)
    lo, hi = F(value_range[0]), F(value_range[1])
    with np.errstate(all="ignore"):
        scaled = (colour - lo) / (hi - lo)
    peek = None
    if flags & MAGNIFIER:
        su, sv = snapped_cursor(cursor_uv, in_wh, (ow, oh), zoom)
        if su >= 0 and sv >= 0 and su < 1 and sv < 1:
            peek = sample_level(texels, su, sv, False).astype(F)
        else:
            peek = np.full(4, np.inf, F)
        cu, cv = (su, sv)
        if zoom:
            cu, cv = unzoom4x_uv(cu, cv)
        cu, cv = aspect_corrected_uv(cu, cv, in_wh, (ow, oh), undo=True)
        with np.errstate(all="ignore"):
            dx, dy = np.abs(F(cu) * F(ow) - ox.astype(F)), np.abs(F(cv) * F(oh) - oy.astype(F))
        scaled = np.where(((dx < 3) & (dy < 3))[..., None], F(0.0), scaled)
        scaled = np.where(((dx < 2) & (dy < 2))[..., None], F(1.0), scaled).astype(F)
    out = np.empty((oh, ow, 4), np.uint8)
    out[..., :3] = to_unorm8(scaled)
    out[..., 3] = 255
    return out, peek
