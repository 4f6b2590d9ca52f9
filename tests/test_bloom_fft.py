"""Bloom's FFT technique on the GPU (prosper_pt_bloom_fft, prosper_pt_bloom_fft_transform).

The transform alone, at every dim it takes, against the DFT in float64 (np.fft): with E the largest absolute error of
prosper's own schedule in float32 (bloom_fft_reference.prosper_schedule) on the same input, the GPU's largest absolute
error is at most 2 E.  E comes from the reference's schedule, never from the code under test; the factor 2 is room for
a different but equally careful summation order, and a wrong twiddle, index or normalisation is off by the signal's
own magnitude, five to six orders above E.  Forward then inverse returns dim times the input ((1 / dim) dim^2) under the
same rule.  No texel is left out.  The cases of dim 4096 move 268 MB images and take ten seconds or so each.

The whole pass, each stage against the restatement (tests/bloom_fft_reference.py) over the GPU's own read-back of that
stage's inputs, as tests/test_bloom.py does.  The extents (tests/test_bloom_fft_cpu.py): CASES have dim 256 or 512;
EDGE_CASES a kernelDim of dim itself and of 1; LARGE_CASES reach dim 1024, 2048 and 4096, landscape and portrait, under the
same rules, with the kernel image compared on KERNEL_ROWS(kernelDim) (every row up to 600) and separate restated over
the rectangle it can light, the rest of the read-back being exactly zero.  The two cases of dim 4096 read back 134 +
268 + 268 MB, run the schedule and the float64 DFT over them on the CPU and, like the transform's, take ten seconds or
so each; their read-backs are not kept.
"""
import ctypes as C

import numpy as np
import pytest

import bloom_fft_reference as F
import bloom_reference as B
from prosper_amd import capi, structs as S
from test_bloom_fft_cpu import CASES, EDGE_CASES, KERNEL_ROWS, LARGE_CASES, SEED
from test_depth_of_field import DeviceCopy, check_half, share

pytestmark = pytest.mark.gpu

DIMS = (256, 512, 1024, 2048, 4096)
INPUTS = ("random", "impulse", "frequency")
ALL_CASES = CASES + EDGE_CASES + LARGE_CASES
IDS = ["%dx%d-%s-%s" % (w, h, "half" if s == F.HALF else "quarter", "biquadratic" if b else "bilinear") for w, h, s, b in ALL_CASES]
STAGES = ((S.BLOOM_FFT_HIGHLIGHTS, "highlights"), (S.BLOOM_FFT_KERNEL, "kernel"), (S.BLOOM_FFT_KERNEL_DFT, "kernel_dft"),
          (S.BLOOM_FFT_CONVOLVED, "convolved"))
_runs = {}


# ---- the transform alone ----

def transform_input(kind, dim):
    if kind == "random":
        return np.random.default_rng(SEED + dim).standard_normal((dim, dim, 4)).astype(np.float32)
    x = np.zeros((dim, dim, 4), np.float32)
    if kind == "impulse":  # a single texel off the origin
        x[dim // 3 + 1, dim // 5 + 2] = (1.5, -2.0, 0.75, 3.0)
        return x
    # a single frequency per channel pair: e^{2 pi i (fx x + fy y) / dim}, and half of another one
    ys, xs = np.meshgrid(np.arange(dim), np.arange(dim), indexing="ij")
    for pair, (fx, fy, amp) in enumerate(((5, dim // 2 - 3, 1.0), (dim - 7, 11, 0.5))):
        phase = 2.0 * np.pi * ((fx * xs + fy * ys) % dim) / dim
        x[..., 2 * pair] = amp * np.cos(phase)
        x[..., 2 * pair + 1] = amp * np.sin(phase)
    return x


def within_twice_the_schedule(label, got, schedule, exact):
    """The rule of every transform check: largest absolute errors against float64, the GPU's within twice the schedule's."""
    assert got.shape == exact.shape and np.isfinite(got).all()
    e = float(np.abs(schedule.astype(np.float64) - exact).max())
    err = float(np.abs(got.astype(np.float64) - exact).max())
    print("%s: GPU error %.3e, prosper's schedule E %.3e, largest magnitude %.3e" % (label, err, e, np.abs(exact).max()))
    assert err <= 2.0 * e, label


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("dim", DIMS)
def test_the_transform_alone_against_the_dft(gpu_ctx, dim, kind):
    x = transform_input(kind, dim)
    forward = scheduled = None
    for inverse in (False, True):
        got = gpu_ctx.bloom_fft_transform(x, inverse)
        schedule = F.prosper_schedule(x, inverse)
        within_twice_the_schedule("dim %d %s %s" % (dim, kind, "inverse" if inverse else "forward"), got, schedule, F.dft(x, inverse))
        if not inverse:
            forward, scheduled = got, schedule
    back = gpu_ctx.bloom_fft_transform(forward, inverse=True)
    within_twice_the_schedule("dim %d %s forward then inverse" % (dim, kind), back, F.prosper_schedule(scheduled, inverse=True),
                              x.astype(np.float64) * dim)


def test_the_transform_on_device_images_and_in_place_equals_the_host_call(gpu_ctx):
    dim = 512
    x = transform_input("random", dim)
    want = gpu_ctx.bloom_fft_transform(x)
    got = np.empty_like(x)
    lib = capi.lib()
    with DeviceCopy(x) as src, DeviceCopy(np.zeros_like(x)) as dst:
        assert lib.prosper_pt_bloom_fft_transform(gpu_ctx._h, dim, 0, src, dst, 1, None) == 0
        assert DeviceCopy.hip.hipMemcpy(C.c_void_p(got.ctypes.data), C.c_void_p(dst), C.c_size_t(got.nbytes), 2) == 0
        assert got.tobytes() == want.tobytes()
        assert lib.prosper_pt_bloom_fft_transform(gpu_ctx._h, dim, 0, src, src, 1, None) == 0  # in place
        assert DeviceCopy.hip.hipMemcpy(C.c_void_p(got.ctypes.data), C.c_void_p(src), C.c_size_t(got.nbytes), 2) == 0
        assert got.tobytes() == want.tobytes()


# ---- the whole pass ----

def read_back(ctx):
    info = ctx.bloom_fft_info()
    assert info.valid == 1
    rb = {name: ctx.read_bloom_fft_stage(stage) for stage, name in STAGES}
    rb.update(info=info, out=ctx.read_hdr())
    return rb


def run(ctx, w, h, scale, biquadratic):
    """One call per case and session, with everything it left behind; a large case's images are its caller's alone."""
    key = (w, h, scale, biquadratic)
    if key in _runs:
        return _runs[key]
    illum, pc = B.design(w, h, SEED), S.BloomFftPC.default(B.THRESHOLD, scale, biquadratic)
    ctx.bloom_fft(pc, w, h, illum)
    rb = read_back(ctx)
    rb.update(pc=pc, illum=illum)
    if key not in LARGE_CASES:
        _runs[key] = rb
    return rb


def same_bytes(a, b):
    return all(a[name].tobytes() == b[name].tobytes() for name in ("highlights", "kernel", "kernel_dft", "convolved", "out"))


def one_ulp(got32, want64):
    """got is the float32 rounding of want, or one of its two neighbours"""
    w = want64.astype(np.float32)
    return (got32 == w) | (got32 == np.nextafter(w, np.float32(np.inf))) | (got32 == np.nextafter(w, np.float32(-np.inf)))


def worst_ulps(got32, want64):
    """The largest distance of got from want in units of the float32 spacing at want."""
    w = want64.astype(np.float32)
    spacing = np.maximum(np.spacing(np.abs(w)), np.float32(np.finfo(np.float32).smallest_subnormal)).astype(np.float64)
    return float((np.abs(got32.astype(np.float64) - want64) / spacing).max()) if w.size else 0.0


def check_stages(rb, illum, pc, label):
    h, w = illum.shape[:2]
    scale = pc.resolutionScale
    dim, kd, conv_scale = F.plan(w, h, scale)
    info = rb["info"]
    assert (info.width, info.height, info.dim, info.kernelDim, info.fused) == (w, h, dim, kd, 0x70)  # the fused middle
    assert np.float32(info.convolutionScale) == conv_scale
    times = [info.separateMs, info.generateMs, info.prepareMs, info.kernelFftMs, info.forwardFftMs, info.convolutionMs,
             info.inverseFftMs, info.composeMs]
    assert all(np.isfinite(t) and t >= 0 for t in times)
    hl, kernel, kdft, conv = rb["highlights"], rb["kernel"], rb["kernel_dft"], rb["convolved"]
    assert hl.shape == kdft.shape == conv.shape == (dim, dim, 4) and kernel.shape == (kd, kd, 4)
    # separate, and the zero padding; above dim 512 the restatement covers the rectangle separate can light and no more
    large = dim > 512
    v, s, (x_out, y_out) = F.separate(illum, pc.threshold, scale, dim, crop=large)
    check_half(label + " separate", hl[:y_out, :x_out, :3] if large else hl[..., :3], v, F.REL * s)
    assert not hl[..., 3].any()
    # (where the input fills the image, 512 x 512 at Half for one, there is no padding on that side)
    assert not hl[:, x_out:].any() if x_out < dim else hl[:, x_out:].size == 0
    assert not hl[y_out:].any() if y_out < dim else hl[y_out:].size == 0
    assert hl[:y_out, :x_out, :3].any()
    # the kernel image: the float64 value rounded once, give or take the last bits of the device's exp, atan, sin and cos
    rows = KERNEL_ROWS(kd)
    restated = F.kernel_image(kd, rows=rows)
    ok = one_ulp(kernel[rows], restated)
    print("%s kernel, %d of %d rows: %d of %d values off the float32 rounding of the restatement by more than one ulp, the worst %.2f ulp from it" % (
        label, len(rows), kd, (~ok).sum(), ok.size, worst_ulps(kernel[rows], restated)))
    assert ok.all(), label + " kernel"
    if len(rows) < kd:
        # sampled rows: what every texel has to satisfy whatever its row
        assert np.isfinite(kernel).all() and (kernel >= 0).all()
        assert (kernel[..., 0] == kernel[..., 1]).all() and (kernel[..., 2] == kernel[..., 3]).all()
        assert kd // 2 - 1 <= np.unravel_index(np.argmax(kernel[..., 0]), (kd, kd))[0] <= kd // 2 + 1
    if kd == dim:
        # the edge: every texel of the wrapped image comes from the kernel image, so where one of its rows or columns
        # is empty, that row or column of the kernel image is (float32 has no value for exp(-|p| / .00605) beyond
        # |p| = .63, so the outer rows are zero by definition), and the streak leaves no column empty
        idx = F.prepare_indices(kd, dim)
        wrapped = F.prepare(kernel, dim)[..., 0]
        assert (idx >= 0).all() and sorted(idx.tolist()) == list(range(kd))
        assert (wrapped.any(axis=1) == kernel[..., 0].any(axis=1)[idx]).all()
        assert (wrapped.any(axis=0) == kernel[..., 0].any(axis=0)[idx]).all() and wrapped.any(axis=0).all()
        assert (wrapped == np.roll(kernel[..., 0], (dim // 2, dim // 2), axis=(0, 1))).all()
    # the kernel's DFT, from the read-back kernel
    prepared = F.prepare(kernel, dim)
    within_twice_the_schedule(label + " kernel DFT", kdft, F.prosper_schedule(prepared), F.dft(prepared))
    # the convolution, from the read-back highlights and kernel DFT
    hl32 = hl.astype(np.float32)
    within_twice_the_schedule(label + " convolved", conv, F.schedule_convolve(hl32, kdft, conv_scale), F.convolve(hl32, kdft, conv_scale))
    # compose, from the read-back convolved image
    v, s = F.compose(illum, conv, scale, pc.biquadratic)
    a = F.REL * s
    print("%s compose: worst error %.3f of the allowance" % (label, share(rb["out"][..., :3], v, a)))
    assert (np.abs(rb["out"][..., :3].astype(np.float64) - v) <= a).all(), label + " compose"
    assert (rb["out"][..., 3] == 1).all()
    added = rb["out"][..., :3].astype(np.float64) - illum[..., :3]
    # highlights and kernel are non-negative and neither is empty: some pixel gains.  (A kernelDim of 1 is the exception:
    # its one texel is 4e-14, so what the restatement adds nowhere exceeds the allowance and float32 cannot hold the sum.)
    gains = (v - illum[..., :3] > a).any()
    assert gains or kd == 1
    assert added.max() > 0 or not gains


@pytest.mark.parametrize("w,h,scale,biquadratic", ALL_CASES, ids=IDS)
def test_every_stage_equals_the_restatement_over_its_read_back_inputs(gpu_ctx, w, h, scale, biquadratic):
    rb = run(gpu_ctx, w, h, scale, biquadratic)
    check_stages(rb, rb["illum"], rb["pc"], IDS[ALL_CASES.index((w, h, scale, biquadratic))])


def one_bright_texel(ctx, w, h, x, y):
    """Input texel (2 x - 1, 2 y - 1), one of the four of highlight (x, y), a quarter of it each, is the only lit one."""
    illum = np.zeros((h, w, 4), np.float32)
    illum[..., 3] = 0.25
    illum[2 * y - 1, 2 * x - 1, :3] = (40.0, 20.0, 10.0)
    ctx.bloom_fft(S.BloomFftPC.default(threshold=0.0), w, h, illum)
    rb = read_back(ctx)
    dim, kd, scale = F.plan(w, h, F.HALF)
    hl = rb["highlights"].astype(np.float64)
    lit = np.argwhere(hl[..., :3].any(axis=-1))
    assert lit.tolist() == [[y, x]] and hl[y, x].tolist() == [10.0, 5.0, 2.5, 0.0]
    wrapped = F.prepare(rb["kernel"], dim)
    shifted = np.roll(wrapped.astype(np.float64), (y, x), axis=(0, 1))
    want = np.stack([shifted[..., 0] * 10.0, shifted[..., 0] * 5.0, shifted[..., 2] * 2.5, np.zeros((dim, dim))], axis=-1) * float(scale)
    # prosper's chain in float32 from the same two images
    schedule = F.schedule_convolve(rb["highlights"].astype(np.float32), F.prosper_schedule(wrapped), scale)
    within_twice_the_schedule("one bright texel, dim %d" % dim, rb["convolved"], schedule, want)
    # the kernel is brightest at its centre (tests/test_bloom_fft_cpu.py), which lands on the lit texel; an even kernelDim
    # has four equal central texels, kd / 2 - 1 and kd / 2 a side, which the wrap puts on the lit texel and the one before
    peak = np.unravel_index(np.argmax(rb["convolved"][..., 0]), (dim, dim))
    if kd % 2:
        assert peak == (y, x)
    else:
        centre, others = rb["kernel"][kd // 2 - 1:kd // 2 + 1, kd // 2 - 1:kd // 2 + 1, 0], rb["kernel"][..., 0].copy()
        others[kd // 2 - 1:kd // 2 + 1, kd // 2 - 1:kd // 2 + 1] = 0
        assert centre.min() > 2 * others.max()
        assert peak[0] in (y - 1, y) and peak[1] in (x - 1, x)


def test_one_bright_texel_convolves_to_the_wrapped_shifted_kernel(gpu_ctx):
    one_bright_texel(gpu_ctx, 75, 55, 21, 16)


def test_one_bright_texel_off_the_column_tiles_of_dim_1024(gpu_ctx):
    """The middle kernel's tile is four columns wide at 1024: column 303 is the last of its tile, row 117 no multiple of a
    power of two."""
    assert F.plan(1030, 300, F.HALF)[0] == 1024 and 303 % 4 == 3
    one_bright_texel(gpu_ctx, 1030, 300, 303, 117)


def test_a_small_case_after_the_largest_gives_the_bytes_it_gave_before(gpu_ctx):
    """The context's images only grow and the twiddle tables are kept per dim: 4100 x 64 leaves the largest images it
    will own and the table of 4096 behind, and 75 x 55 after it must read neither with their strides or sizes."""
    first = run(gpu_ctx, 75, 55, F.HALF, 1)
    w, h = 4100, 64
    gpu_ctx.bloom_fft(S.BloomFftPC.default(B.THRESHOLD, F.HALF, 1), w, h, B.design(w, h, SEED))
    info = gpu_ctx.bloom_fft_info()
    assert (info.dim, info.kernelDim, info.kernelRemade) == (4096, 32, 1)
    gpu_ctx.bloom_fft(first["pc"], 75, 55, first["illum"])
    assert gpu_ctx.bloom_fft_info().kernelRemade == 1  # dim changed
    assert same_bytes(first, read_back(gpu_ctx))


@pytest.mark.parametrize("scale", [F.HALF, F.QUARTER])
def test_nothing_above_the_threshold_returns_the_input(gpu_ctx, scale):
    w, h = 100, 70
    illum = B.design(w, h, SEED)
    want = illum.copy()
    want[..., 3] = 1.0
    gpu_ctx.bloom_fft(S.BloomFftPC.default(float(illum[..., :3].max()) + 1.0, scale), w, h, illum)
    assert gpu_ctx.read_hdr().tobytes() == want.tobytes()
    assert not gpu_ctx.read_bloom_fft_stage(S.BLOOM_FFT_HIGHLIGHTS).any()
    assert not gpu_ctx.read_bloom_fft_stage(S.BLOOM_FFT_CONVOLVED).any()


def test_the_kernel_is_kept_until_the_extent_changes_or_the_caller_asks(gpu_ctx):
    w, h = 75, 55
    first = run(gpu_ctx, w, h, F.HALF, 1)
    pc, illum = first["pc"], first["illum"]
    gpu_ctx.bloom_fft_release_kernel()
    gpu_ctx.bloom_fft(pc, w, h, illum)
    assert gpu_ctx.bloom_fft_info().kernelRemade == 1 and same_bytes(first, read_back(gpu_ctx))
    gpu_ctx.bloom_fft(pc, w, h, illum)
    info = gpu_ctx.bloom_fft_info()
    assert info.kernelRemade == 0 and (info.generateMs, info.prepareMs, info.kernelFftMs) == (0, 0, 0)
    assert same_bytes(first, read_back(gpu_ctx))
    again = S.BloomFftPC.default(B.THRESHOLD, F.HALF, 1, regenerate_kernel=1)
    gpu_ctx.bloom_fft(again, w, h, illum)
    assert gpu_ctx.bloom_fft_info().kernelRemade == 1 and same_bytes(first, read_back(gpu_ctx))
    # another kernelDim with the same dim, and back
    other = run(gpu_ctx, 64, 48, F.HALF, 1)
    gpu_ctx.bloom_fft(other["pc"], 64, 48, other["illum"])
    assert gpu_ctx.bloom_fft_info().kernelRemade == 1 and same_bytes(other, read_back(gpu_ctx))
    gpu_ctx.bloom_fft(pc, w, h, illum)
    assert gpu_ctx.bloom_fft_info().kernelRemade == 1 and same_bytes(first, read_back(gpu_ctx))


def test_in_place_and_device_inputs_equal_the_host_call(gpu_ctx):
    w, h = 75, 55
    want = run(gpu_ctx, w, h, F.HALF, 1)
    pc, illum = want["pc"], want["illum"]
    above = S.BloomFftPC.default(float(illum[..., :3].max()) + 1.0)
    with DeviceCopy(illum) as il:
        gpu_ctx.bloom_fft(pc, w, h, illumination_ptr=il)
        assert same_bytes(want, read_back(gpu_ctx))
    # in place: a threshold above everything first puts the input's rgb into the HDR image (alpha 1, which bloom does not read)
    gpu_ctx.bloom_fft(above, w, h, illum)
    gpu_ctx.bloom_fft(pc, w, h)
    assert same_bytes(want, read_back(gpu_ctx))
    # ... and with the HDR image passed explicitly
    gpu_ctx.bloom_fft(above, w, h, illum)
    gpu_ctx.bloom_fft(pc, w, h, illumination_ptr=gpu_ctx.hdr_device_ptr()[0])
    assert same_bytes(want, read_back(gpu_ctx))


def test_bad_arguments_are_refused_and_change_nothing(gpu_ctx):
    w, h = 75, 55
    want = run(gpu_ctx, w, h, F.HALF, 1)
    pc, illum = want["pc"], want["illum"]
    gpu_ctx.bloom_fft(pc, w, h, illum)
    before, info_before = read_back(gpu_ctx), bytes(gpu_ctx.bloom_fft_info())
    lib = capi.lib()

    def refused(words, call):
        with pytest.raises(capi.ProsperPtError) as e:
            call()
        assert e.value.code == -1 and words in str(e.value), str(e.value)

    assert lib.prosper_pt_bloom_fft(gpu_ctx._h, None, w, h, illum.ctypes.data, 0, None) == -1
    reserved = S.BloomFftPC.default()
    reserved.reserved[3] = 7
    for bad, words in ((S.BloomFftPC.default(threshold=np.nan), "non-finite"), (S.BloomFftPC.default(threshold=-np.inf), "non-finite"),
                       (S.BloomFftPC.default(threshold=-0.5), "negative"), (S.BloomFftPC.default(resolution_scale=2), "unknown resolution scale"),
                       (S.BloomFftPC.default(biquadratic=2), "biquadratic"), (S.BloomFftPC.default(regenerate_kernel=2), "regenerateKernel"),
                       (reserved, "reserved")):
        refused(words, lambda: gpu_ctx.bloom_fft(bad, w, h, illum))
    hdr = gpu_ctx.hdr_device_ptr()[0]
    refused("empty extent", lambda: gpu_ctx.bloom_fft(pc, 0, h, illumination_ptr=hdr))
    refused("empty extent", lambda: gpu_ctx.bloom_fft(pc, w, 0, illumination_ptr=hdr))
    refused("working image empty", lambda: gpu_ctx.bloom_fft(pc, 1, h, illumination_ptr=hdr))
    refused("working image empty", lambda: gpu_ctx.bloom_fft(S.BloomFftPC.default(resolution_scale=1), w, 3, illumination_ptr=hdr))
    refused("above 8192", lambda: gpu_ctx.bloom_fft(pc, 8193, 2, illumination_ptr=hdr))
    refused("another extent", lambda: gpu_ctx.bloom_fft(pc, 64, 48))
    x = np.zeros((256, 256, 4), np.float32)
    for dim in (128, 384, 8192):
        assert lib.prosper_pt_bloom_fft_transform(gpu_ctx._h, dim, 0, x.ctypes.data, x.ctypes.data, 0, None) == -1
    assert lib.prosper_pt_bloom_fft_transform(gpu_ctx._h, 256, 0, None, x.ctypes.data, 0, None) == -1
    buf = np.zeros(16, np.uint8)
    assert lib.prosper_pt_read_bloom_fft_stage(gpu_ctx._h, S.BLOOM_FFT_HIGHLIGHTS, buf.ctypes.data, 16, None) == -1  # not its size
    assert lib.prosper_pt_read_bloom_fft_stage(gpu_ctx._h, 4, buf.ctypes.data, 16, None) == -1
    assert same_bytes(before, read_back(gpu_ctx)) and bytes(gpu_ctx.bloom_fft_info()) == info_before


def test_the_mirror_with_the_fft_technique_equals_a_direct_call(gpu_ctx):
    from prosper_amd.rt_reference import Bloom
    want = run(gpu_ctx, 75, 55, F.HALF, 1)
    quarter = run(gpu_ctx, 100, 70, F.QUARTER, 0)
    bloom = Bloom(gpu_ctx, technique=S.BLOOM_FFT)
    try:
        got = bloom.record(75, 55, want["illum"])
        assert isinstance(got, S.BloomFftPC) and bytes(got) == bytes(want["pc"]) and same_bytes(want, read_back(gpu_ctx))
        bloom.draw_ui(threshold=B.THRESHOLD, biquadratic=False, resolution_scale=S.BLOOM_QUARTER)
        got = bloom.record(100, 70, quarter["illum"])
        assert (got.resolutionScale, got.biquadratic, got.regenerateKernel) == (1, 0, 0) and same_bytes(quarter, read_back(gpu_ctx))
        # the checkbox, and releasePreserved
        bloom.record(100, 70, quarter["illum"])
        assert gpu_ctx.bloom_fft_info().kernelRemade == 0
        bloom.set_technique(S.BLOOM_FFT, regenerate_kernel=True)
        assert bloom.record(100, 70, quarter["illum"]).regenerateKernel == 1 and gpu_ctx.bloom_fft_info().kernelRemade == 1
        bloom.set_technique(S.BLOOM_FFT)
        bloom.record(100, 70, quarter["illum"])
        assert gpu_ctx.bloom_fft_info().kernelRemade == 0
        bloom.release_preserved()
        bloom.record(100, 70, quarter["illum"])
        assert gpu_ctx.bloom_fft_info().kernelRemade == 1 and same_bytes(quarter, read_back(gpu_ctx))
        # the default technique drops the kernel as Bloom.cpp:117 does, and returns its own push constants
        bloom.set_technique(S.BLOOM_MULTI_RESOLUTION_BLUR)
        assert isinstance(bloom.record(100, 70, quarter["illum"]), S.BloomPC)
        bloom.set_technique(S.BLOOM_FFT)
        bloom.record(100, 70, quarter["illum"])
        assert gpu_ctx.bloom_fft_info().kernelRemade == 1 and same_bytes(quarter, read_back(gpu_ctx))
    finally:
        bloom.close()


def test_the_blur_gives_the_bytes_it_gave_before(gpu_ctx):
    """The two techniques share no image that the other reads."""
    w, h = 101, 71
    illum, pc = B.design(w, h, SEED), S.BloomPC.default()

    def blur():
        gpu_ctx.bloom(pc, w, h, illum)
        info = gpu_ctx.bloom_info()
        images = [gpu_ctx.read_bloom_stage(S.BLOOM_HIGHLIGHTS, l).tobytes() for l in range(S.BLOOM_LEVELS)]
        for stage in (S.BLOOM_HORIZONTAL, S.BLOOM_BLURRED):
            images += [gpu_ctx.read_bloom_stage(stage, l).tobytes() for l in range(info.firstLevel, info.firstLevel + 3)]
        return images + [gpu_ctx.read_hdr().tobytes()]

    before = blur()
    fft = run(gpu_ctx, 75, 55, F.HALF, 1)
    gpu_ctx.bloom_fft(fft["pc"], 75, 55, fft["illum"])
    stages = read_back(gpu_ctx)
    assert blur() == before
    # ... and the blur left the FFT technique's images alone
    assert all(gpu_ctx.read_bloom_fft_stage(stage).tobytes() == stages[name].tobytes() for stage, name in STAGES)
