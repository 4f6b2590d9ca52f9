"""NumPy restatement of prosper's bloom, the FFT technique (not a test module), for tests/test_bloom_fft*.py:

  plan(w, h, resolution_scale)              dim, kernelDim and the convolution's scale
  separate(illum, threshold, scale, dim)    separate.comp over the padded dim x dim image, or its lit rectangle: (v, s)
  kernel_image(kd), kernel_margins(kd)      generate_kernel.comp in float64, and how close a sub-sample comes to a branch;
                                            both over the whole image or, in bands, over the texel rows asked for
  prepare(kernel, dim)                      prepare_kernel.comp
  dft(x, inverse), convolve(...)            the transform (np.fft, float64) with prosper's normalisations, the convolution
  compose(illum, convolved, ...)            compose.comp with MULTI_RESOLUTION = false: (v, s)
  prosper_schedule(x, inverse)              Fft.cpp's radix sequence over fft.comp's butterflies, in float32: the
                                            yardstick for the accuracy of a float32 transform
  schedule_convolve(...)                    the convolution through prosper_schedule

An image is [dim, dim, 4]; a texel holds the complex numbers r + i g and b + i a.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import bloom_reference as B

HALF, QUARTER = B.HALF, B.QUARTER
REL = B.REL
MIN_DIM, MAX_DIM = 256, 4096
# math.glsl's PI, and the constant sdStar writes out
PI = 3.14159265
STAR_PI = 3.1415927


def bit_ceil(v):
    return 1 << max(int(v) - 1, 0).bit_length()


def plan(w, h, resolution_scale):
    """(dim, kernelDim, scale) of Separate.cpp:98-101, GenerateKernel.cpp:81-85 and Bloom.cpp:95-98; None where the
    technique refuses the extent."""
    s = B.scale_of(resolution_scale)
    if w <= 0 or h <= 0 or w // s == 0 or h // s == 0 or max(w, h) > 2 * MAX_DIM:
        return None
    dim = max(bit_ceil(max(w, h)) // s, MIN_DIM)
    kd = h // s
    scale = np.float32(2.0) / np.float32(kd)
    if resolution_scale == QUARTER:
        scale = scale * np.float32(2.0)
    return dim, kd, np.float32(scale)


# ---- separate ----

def outside_from(w, h, resolution_scale):
    """The first column and row of the highlights whose lookups all fall outside the w x h input."""
    if resolution_scale == HALF:
        return (w + 2) // 2, (h + 2) // 2  # the texels 2 c - 1 and 2 c: outside from 2 c - 1 >= size on
    return (w + 5) // 4, (h + 5) // 4  # the texels 4 c - 2 .. 4 c + 1: outside from 4 c - 2 >= size on


def separate(illum, threshold, resolution_scale, dim, crop=False):
    """(v, s) of the dim x dim highlights, and the first column and row whose lookups all fall outside the input.  With
    `crop`, (v, s) of the rectangle [:y_out, :x_out] alone (cut to dim): what a dim of 4096 leaves affordable."""
    h, w = illum.shape[:2]
    rgb = illum[..., :3].astype(np.float64)
    outside = outside_from(w, h, resolution_scale)
    nx, ny = (min(outside[0], dim), min(outside[1], dim)) if crop else (dim, dim)
    ys, xs = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    inv_w, inv_h = 1.0 / w, 1.0 / h
    if resolution_scale == HALF:
        mean = B.bilinear(rgb, (2 * xs) * inv_w, (2 * ys) * inv_h, edge=False)
    else:
        mean = sum(B.bilinear(rgb, (4 * xs + dx) * inv_w, (4 * ys + dy) * inv_h, edge=False)
                   for dx, dy in ((-1, -1), (-1, 1), (1, -1), (1, 1))) / 4.0
    t = float(np.float32(threshold))
    return np.maximum(mean - t, 0.0), np.abs(mean) + t, outside


# ---- the kernel image ----

def _gaussian(x, a, b, c):
    return a * np.exp(-(x - b * b) / (2.0 * c * c))


def _sd_star(px, py, r, n, w):
    m = n + w * (2.0 - n)
    an, en = STAR_PI / n, STAR_PI / m
    racs_x, racs_y = r * np.cos(an), r * np.sin(an)
    ecs_x, ecs_y = np.cos(en), np.sin(en)
    px = np.abs(px)
    at, period = np.arctan2(px, py), 2.0 * an
    bn = (at - period * np.floor(at / period)) - an
    ln = np.sqrt(px * px + py * py)
    qx, qy = ln * np.cos(bn), ln * np.abs(np.sin(bn))
    qx, qy = qx - racs_x, qy - racs_y
    t = np.clip(-(qx * ecs_x + qy * ecs_y), 0.0, racs_y / ecs_y)
    qx, qy = qx + ecs_x * t, qy + ecs_y * t
    return np.sqrt(qx * qx + qy * qy) * np.sign(qx)


def _filter_value(px, py):
    """filterValue of generate_kernel.comp as written, float64: (.r = .g, .b = .a, dStar)."""
    a, c = 1.5, 0.055
    g = _gaussian(np.sqrt(px * px + py * py), a, 0.0, c)
    d = _sd_star(px, py, 0.5, 4.0, 0.075)
    angle = PI / 4.0
    rx, ry = np.cos(angle) * px + np.sin(angle) * py, np.cos(angle) * py - np.sin(angle) * px
    d = np.minimum(d, _sd_star(rx, ry, 0.35, 4.0, 0.05))
    rg = np.where(d < 0.0, g + g, g)
    ba = rg.copy()
    t = np.clip(np.abs(px) * 6.0, 0.0, 1.0)
    mix_rg, mix_ba = 0.05 * (1.0 - t) + 0.01 * t, 1.0 * (1.0 - t) + 1.0 * t
    wave = (np.abs(np.sin(px * 50.0)) + np.abs(np.cos(px * 95.0))) + np.abs(np.sin(px * 75.0))
    streak = _gaussian(np.abs(px) * 10.0, 0.5, 1.0, 1.0)
    on = np.abs(py) < 0.005
    rg = np.where(on, rg + ((0.5 * mix_rg) * wave) * streak, rg)
    ba = np.where(on, ba + ((0.5 * mix_ba) * wave) * streak, ba)
    return rg, ba, d


def _sub_samples(kd, texel_rows=None):
    """(px, py) of the 8 kd sub-sample columns over every sub-sample row, or over the eight of each texel row given."""
    c = ((np.arange(8 * kd, dtype=np.float64) + 0.5) / (8.0 * kd)) * 2.0 - 1.0
    cy = c if texel_rows is None else c[(8 * np.asarray(texel_rows, np.int64)[:, None] + np.arange(8)).ravel()]
    py, px = np.meshgrid(cy, c, indexing="ij")
    return px, py


KERNEL_BAND = 16  # texel rows evaluated at once where rows are given: 128 sub-sample rows of 8 kd values per temporary


def _bands(kd, rows, of_band):
    """of_band over `rows` (sorted texel rows) in bands of at most KERNEL_BAND, a few bands at a time."""
    rows = [int(r) for r in rows]
    assert rows == sorted(set(rows)) and (not rows or (0 <= rows[0] and rows[-1] < kd))
    bands = [rows[i:i + KERNEL_BAND] for i in range(0, len(rows), KERNEL_BAND)]
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return list(pool.map(of_band, bands))


def kernel_image(kd, rows=None):
    """[kd, kd, 4] float64: the mean of filterValue over the 8 x 8 sub-samples of each texel (round it once to float32).
    With `rows`, a sorted list of texel rows, only their 8 len(rows) sub-sample rows are evaluated, in bands, and the
    result is [len(rows), kd, 4]: the same arithmetic, so the same bytes as those rows of the whole image."""
    def mean(px, py):
        n = px.shape[0] // 8
        rg, ba, _ = _filter_value(px, py)
        rg = rg.reshape(n, 8, kd, 8).sum(axis=(1, 3)) / 64.0
        ba = ba.reshape(n, 8, kd, 8).sum(axis=(1, 3)) / 64.0
        return np.stack([rg, rg, ba, ba], axis=-1)

    if rows is None:
        return mean(*_sub_samples(kd))
    return np.concatenate(_bands(kd, rows, lambda band: mean(*_sub_samples(kd, band))) or [np.empty((0, kd, 4))], axis=0)


def kernel_margins(kd, rows=None):
    """How close a sub-sample comes to a branch of filterValue: (min |dStar|, min ||p.y| - .005|); with `rows`, over the
    sub-samples of those texel rows, in bands."""
    def margins(px, py):
        d = _filter_value(px, py)[2]
        return float(np.abs(d).min()), float(np.abs(np.abs(py) - 0.005).min())

    if rows is None:
        return margins(*_sub_samples(kd))
    found = _bands(kd, rows, lambda band: margins(*_sub_samples(kd, band)))
    return min(f[0] for f in found), min(f[1] for f in found)


def prepare_indices(kd, dim):
    """For each output coordinate the input one, or -1: pIn = pOut + kd / 2 below dim / 2 and pOut + (kd - 2 dim) / 2
    from there on, as the GLSL's floats (exact in float64), inside while 0 <= pIn < kd, truncated."""
    p_out = np.arange(dim, dtype=np.float64)
    p_in = np.where(p_out >= dim / 2.0, p_out + (kd - 2.0 * dim) / 2.0, p_out + kd / 2.0)
    inside = (p_in >= 0.0) & (p_in < kd)
    return np.where(inside, np.trunc(p_in), -1).astype(np.int64)


def prepare(kernel, dim):
    """prepare_kernel.comp: the centred kernel [kd, kd, 4] wrapped round the corners of [dim, dim, 4], .g = .a = 0."""
    kd = kernel.shape[0]
    idx = prepare_indices(kd, dim)
    inside = (idx >= 0)[:, None] & (idx >= 0)[None, :]
    src = kernel[np.clip(idx, 0, kd - 1)][:, np.clip(idx, 0, kd - 1)]
    out = np.where(inside[..., None], src, 0).astype(kernel.dtype)
    out[..., 1] = 0
    out[..., 3] = 0
    return out


# ---- the transform ----

def to_complex(img):
    img = np.asarray(img)
    return img[..., 0::2] + 1j * img[..., 1::2].astype(np.float64)


def from_complex(z):
    out = np.empty(z.shape[:2] + (4,), np.float64)
    out[..., 0::2] = z.real
    out[..., 1::2] = z.imag
    return out


def dft(img, inverse=False):
    """Float64.  Forward: X[ky][kx] = (1 / dim) sum x[y][x] e^{-2 pi i (kx x + ky y) / dim}; inverse: the unnormalised
    inverse DFT."""
    z = to_complex(np.asarray(img, np.float64))
    dim = z.shape[0]
    if inverse:
        return from_complex(np.fft.ifft2(z, axes=(0, 1)) * (dim * dim))
    return from_complex(np.fft.fft2(z, axes=(0, 1)) / dim)


def multiply(a, k, scale):
    """convolution.comp in float64"""
    return from_complex(to_complex(np.asarray(a, np.float64)) * to_complex(np.asarray(k, np.float64)) * float(scale))


def convolve(highlights, kernel_dft, scale):
    """The inverse of DFT(highlights) * kernel_dft * scale, float64."""
    return dft(multiply(dft(highlights), kernel_dft, scale), inverse=True)


# ---- prosper's own schedule, float32 ----

def radix_sequence(n):
    """Fft.cpp:157-247: the first radix is what the later ones, all min(n / 32, 16), leave over."""
    max_radix = min(n // 32, 16)
    v = n
    while v > max_radix:
        v //= max_radix
    seq, ns = [v], v
    while ns < n:
        seq.append(max_radix)
        ns *= max_radix
    assert ns == n
    return seq


_F = np.float32
_W8 = (np.complex64(complex(_F(0.707106781187), _F(-0.707106781187))), np.complex64(complex(_F(-0.707106781187), _F(-0.707106781187))))
_W16 = [np.complex64(complex(_F(re), _F(im))) for re, im in (
    (1, 0), (1, 0), (1, 0), (1, 0), (1, 0), (0.92387953251, -0.38268343237), (0.707106781187, -0.707106781187),
    (0.38268343237, -0.92387953251), (1, 0), (0.707106781187, -0.707106781187), (0, -1), (-0.707106781187, -0.707106781187),
    (1, 0), (0.38268343237, -0.92387953251), (-0.707106781187, -0.707106781187), (-0.92387953251, 0.38268343237))]


def _minus_i(c):
    """-mulI(c) = (c.y, -c.x)"""
    out = np.empty_like(c)
    out.real = c.imag
    out.imag = -c.real
    return out


def _r2(a, b):
    return a + b, a - b


def _r4(i0, i1, i2, i3):
    t0, t2 = _r2(i0, i2)
    t1, t3 = _r2(i1, i3)
    t3 = _minus_i(t3)
    o0, o2 = _r2(t0, t1)
    o1, o3 = _r2(t2, t3)
    return o0, o1, o2, o3


def _r8(v):
    t = [None] * 8
    for k in range(4):
        t[k], t[k + 4] = _r2(v[k], v[k + 4])
    t[5] = t[5] * _W8[0]
    t[6] = _minus_i(t[6])
    t[7] = t[7] * _W8[1]
    o = [None] * 8
    o[0], o[2], o[4], o[6] = _r4(t[0], t[1], t[2], t[3])
    o[1], o[3], o[5], o[7] = _r4(t[4], t[5], t[6], t[7])
    return o


def _swap(c):
    out = np.empty_like(c)
    out.real = c.imag
    out.imag = c.real
    return out


def _pass(a, radix, ns, inverse):
    """One iteration of fft.comp along axis 0 of the complex64 array a [n, ...]."""
    n = a.shape[0]
    count = n // radix
    j = np.arange(count)
    shape = (count,) + (1,) * (a.ndim - 1)
    angle = (_F(-2.0) * _F(PI) * (j % ns).astype(_F) / _F(ns * radix)).astype(_F)
    c = [a[r * count:(r + 1) * count] for r in range(radix)]
    if inverse:
        c = [_swap(x) for x in c]
    else:
        root = np.sqrt(_F(radix))
        c = [(x.view(_F) / root).view(np.complex64) for x in c]

    def twiddle(r):
        x = (_F(r) * angle).astype(_F)
        return (np.cos(x).astype(_F) + 1j * np.sin(x).astype(_F)).astype(np.complex64).reshape(shape)

    if radix == 16:
        # four lanes q per butterfly: lane q takes the inputs q + 4 m, and after its first radix-4 the lanes trade
        first = [_r4(*[c[q + 4 * m] * twiddle(q + 4 * m) for m in range(4)]) for q in range(4)]
        d = [None] * 16
        for q in range(4):
            t = [first[m][q] for m in range(4)]
            t = [t[0]] + [t[m] * _W16[4 * q + m] for m in range(1, 4)]
            o = _r4(*t)
            for m in range(4):
                d[4 * m + q] = o[m]
    else:
        v = [c[0]] + [c[r] * twiddle(r) for r in range(1, radix)]
        d = {2: lambda x: list(_r2(*x)), 4: lambda x: list(_r4(*x)), 8: _r8}[radix](v)
    if inverse:
        d = [_swap(x) for x in d]
    out = np.empty_like(a)
    view = out.reshape((count // ns, radix, ns) + a.shape[1:])
    for r in range(radix):
        view[:, r] = d[r].reshape((count // ns, ns) + a.shape[1:])
    return out


def _lines(a, inverse):
    """Every pass of one dimension along axis 0 of a [n, lines, 2]."""
    ns = 1
    for radix in radix_sequence(a.shape[0]):
        a = _pass(a, radix, ns, inverse)
        ns *= radix
    return a


def prosper_schedule(img, inverse=False):
    """Fft::record in float32 over a [dim, dim, 4] image: rows, then columns, every pass divided by sqrt(R) when forward."""
    z = np.ascontiguousarray(img, np.float32).view(np.complex64)  # [y, x, pair]
    dim = z.shape[0]
    out = np.empty_like(z)
    step = min(dim, max(16, 262144 // dim))  # lines of one piece of work
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        def rows(y0):
            out[y0:y0 + step] = _lines(np.ascontiguousarray(z[y0:y0 + step].transpose(1, 0, 2)), inverse).transpose(1, 0, 2)

        def columns(x0):
            out[:, x0:x0 + step] = _lines(np.ascontiguousarray(out[:, x0:x0 + step]), inverse)

        list(pool.map(rows, range(0, dim, step)))
        list(pool.map(columns, range(0, dim, step)))
    return out.view(np.float32).reshape(dim, dim, 4)


def schedule_convolve(highlights, kernel_dft, scale):
    """prosper's chain in float32: the schedule forward, convolution.comp, the schedule inverse."""
    a = prosper_schedule(np.asarray(highlights, np.float32)).view(np.complex64)
    k = np.ascontiguousarray(kernel_dft, np.float32).view(np.complex64)
    prod = ((a * k).view(np.float32) * np.float32(scale)).astype(np.float32)
    return prosper_schedule(prod.reshape(np.asarray(highlights).shape), inverse=True)


# ---- compose ----

def compose(illum, convolved, resolution_scale, biquadratic):
    """(v, s) of the output's rgb: illumination + the lookup of the convolved [dim, dim, 4] image at
    highlightUV = (coord + .5) / (dim s), clamped to the edge."""
    h, w = illum.shape[:2]
    dim = convolved.shape[0]
    s = B.scale_of(resolution_scale)
    rgb = illum[..., :3].astype(np.float64)
    img = np.asarray(convolved, np.float32)[..., :3].astype(np.float64)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    u, v = (xs + 0.5) / (dim * s), (ys + 0.5) / (dim * s)

    def lookups(image):
        if not biquadratic:
            return B.bilinear(image, u, v, True)
        res = float(dim)
        qx, qy = (u * res) % 1.0, (v * res) % 1.0
        cx, cy = (qx * (qx - 1.0) + 0.5) / res, (qy * (qy - 1.0) + 0.5) / res
        return (B.bilinear(image, u - cx, v - cy, True) + B.bilinear(image, u - cx, v + cy, True) +
                B.bilinear(image, u + cx, v + cy, True) + B.bilinear(image, u + cx, v - cy, True)) / 4.0

    return rgb + lookups(img), np.abs(rgb) + lookups(np.abs(img))
