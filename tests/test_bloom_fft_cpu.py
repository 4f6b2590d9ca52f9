"""Bloom's FFT technique without a GPU: the host-only plan, the struct sizes, the refusals that need no
context, and the numpy restatement (tests/bloom_fft_reference.py) checking itself.  The GPU side: tests/test_bloom_fft.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bloom_fft_reference as F
import bloom_reference as B
from prosper_amd import capi, structs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("prosper_pt_bloom_fft", "prosper_pt_bloom_fft_plan", "prosper_pt_bloom_fft_transform", "prosper_pt_bloom_fft_release_kernel",
               "prosper_pt_read_bloom_fft_stage", "prosper_pt_get_bloom_fft_info", "prosper_host_bloom_set_technique",
               "prosper_host_bloom_release_preserved", "prosper_host_bloom_fft_push_constants")
SEED = 11
# (w, h, resolution scale) of the whole pass on the GPU with a whole kernel image evaluated here; every dim is 256 or 512
# (LARGE_CASES reach the others).  75 x 55 is the odd one (kernelDim 27,
# compose fractions .25 / .75): at 75 x 51 the kernelDim is 25, and with 200 sub-samples a side one of them has
# |p.y| = 1 / 200, the streak's threshold itself (test_no_sub_sample_of_the_kernel_image_lies_on_a_branch).
HALF_EXTENTS = ((64, 48), (75, 55), (48, 100), (512, 288), (520, 8))
QUARTER_EXTENTS = ((100, 70), (1030, 40))
EXTENTS = [(w, h, F.HALF) for w, h in HALF_EXTENTS] + [(w, h, F.QUARTER) for w, h in QUARTER_EXTENTS]
# (w, h, resolution scale, biquadratic): biquadratic on all, bilinear on two
CASES = [(w, h, s, 1) for w, h, s in EXTENTS] + [(75, 55, F.HALF, 0), (100, 70, F.QUARTER, 0)]
# The smallest inputs that reach the instantiations of dim 1024, 2048 and 4096, each dim landscape and portrait: separate
# lights only the rows below H / s, so the rows of a landscape image's highlights are mostly exact zeros and a middle
# kernel that took one zero row for another would pass; a portrait one lights them all, and its kernelDim = H / s is large.
LARGE_CASES = [(1030, 300, F.HALF, 1), (300, 1030, F.HALF, 1), (2100, 64, F.HALF, 0), (64, 2100, F.HALF, 1), (4100, 64, F.HALF, 1),
               (64, 4100, F.HALF, 0)]
# kernelDim == dim (the wrapped kernel image leaves no zero texel between its halves), twice, and kernelDim 1
EDGE_CASES = [(512, 512, F.HALF, 1), (512, 1024, F.QUARTER, 1), (300, 2, F.HALF, 1)]
NEW_CASES = EDGE_CASES + LARGE_CASES
PLAN_EXTENTS = [(1920, 1080), (64, 48), (75, 51), (48, 100), (512, 288), (520, 8), (100, 70), (1030, 40), (8192, 2)] + sorted(
    {(w, h) for w, h, _, _ in NEW_CASES})
FULL_KERNEL_ROWS = 600


def KERNEL_ROWS(kd):
    """The sorted texel rows on which a kernel image of kernelDim kd is checked: every row up to kernelDim 600, and above
    it the first two, the last two, the three about kd // 2 and 17 seeded ones, 24 in all.  The sampling caps the time of
    the restatement (64 kd^2 evaluations in float64) and is no tolerance: the kernel computes a texel per wave and rows
    do not depend on each other, a wrong texel index shifts every row, and the rows that differ in kind, those of the
    streak |p.y| < .005, include the three about kd // 2."""
    if kd <= FULL_KERNEL_ROWS:
        return list(range(kd))
    fixed = [0, 1, kd // 2 - 1, kd // 2, kd // 2 + 1, kd - 2, kd - 1]
    rest = np.setdiff1d(np.arange(kd), fixed)
    rows = sorted(fixed + np.random.default_rng(SEED + kd).choice(rest, 17, replace=False).tolist())
    assert len(rows) == 24
    return rows


def test_new_symbols_are_exported_and_the_abi_version_is_unchanged():
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4


def header_struct_size(name):
    """The size of a header struct whose fields are 4-byte scalars and arrays of them."""
    text = open(os.path.join(ROOT, "include", "prosper_pt", "prosper_pt.h")).read()
    start = text.index("struct " + name)
    body = text[start:text.index("}", start)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    words = 0
    for decl in re.findall(r"\b(?:uint32_t|int32_t|float)\s+([^;]+);", body):
        for field in decl.split(","):
            m = re.search(r"\[(\d+)\]", field)
            words += int(m.group(1)) if m else 1
    return 4 * words


def test_struct_sizes_equal_the_headers():
    assert C.sizeof(S.BloomFftPC) == header_struct_size("prosper_pt_bloom_fft_pc") == 32
    assert C.sizeof(S.BloomFftPlan) == header_struct_size("prosper_pt_bloom_fft_plan") == 12
    assert C.sizeof(S.BloomFftInfo) == header_struct_size("prosper_pt_bloom_fft_info") == 64
    pc = S.BloomFftPC.default()
    assert (pc.threshold, pc.resolutionScale, pc.biquadratic, pc.regenerateKernel, list(pc.reserved)) == (1.0, 0, 1, 0, [0, 0, 0, 0])
    # prosper_pt_bloom's own push constants are as they were
    assert C.sizeof(S.BloomPC) == 32


@pytest.mark.parametrize("w,h", PLAN_EXTENTS)
@pytest.mark.parametrize("scale", [F.HALF, F.QUARTER])
def test_the_plan_equals_the_restatement(w, h, scale):
    want = F.plan(w, h, scale)
    plan = S.BloomFftPlan()
    rc = capi.lib().prosper_pt_bloom_fft_plan(w, h, scale, C.byref(plan))
    if want is None:
        assert rc == -1
        return
    assert rc == 0
    assert (plan.dim, plan.kernelDim) == want[:2]
    assert np.float32(plan.convolutionScale).view(np.uint32) == want[2].view(np.uint32)
    assert plan.dim & (plan.dim - 1) == 0 and 256 <= plan.dim <= 4096 and plan.kernelDim <= plan.dim


def test_every_dim_has_a_whole_pass_case_and_the_large_ones_both_orientations():
    planned = {}
    for w, h, scale, _ in CASES + LARGE_CASES + EDGE_CASES:
        planned.setdefault(F.plan(w, h, scale)[0], []).append((w, h))
    assert set(planned) == {256, 512, 1024, 2048, 4096}
    for dim in (1024, 2048, 4096):
        assert any(w > h for w, h in planned[dim]) and any(h > w for w, h in planned[dim]), dim
    assert not set(CASES) & set(NEW_CASES) and len(set(NEW_CASES)) == len(NEW_CASES)
    # the edges: kernelDim == dim at both scales, and kernelDim 1 with a convolution scale of 2
    assert [F.plan(w, h, s)[:2] for w, h, s, _ in EDGE_CASES] == [(256, 256), (256, 256), (256, 1)]
    assert float(F.plan(300, 2, F.HALF)[2]) == 2.0
    assert [F.plan(w, h, s)[:2] for w, h, s, _ in LARGE_CASES] == [(1024, 150), (1024, 515), (2048, 32), (2048, 1050), (4096, 32), (4096, 2050)]


def test_known_plans_and_the_largest_extent():
    assert F.plan(1920, 1080, F.HALF)[:2] == (1024, 540) and F.plan(1920, 1080, F.QUARTER)[:2] == (512, 270)
    assert F.plan(1030, 40, F.QUARTER)[:2] == (512, 10) and F.plan(520, 8, F.HALF)[:2] == (512, 4)
    assert float(F.plan(1920, 1080, F.QUARTER)[2]) == float(np.float32(2.0) / np.float32(270) * np.float32(2.0))
    p = capi.bloom_fft_plan(8192, 2, S.BLOOM_HALF)  # accepted
    assert (p.dim, p.kernelDim, p.convolutionScale) == (4096, 1, 2.0)
    lib = capi.lib()
    plan = S.BloomFftPlan()
    for w, h, s in ((8193, 2, 0), (2, 8193, 0), (0, 8, 0), (8, 0, 0), (1, 8, 0), (8, 1, 0), (8, 3, 1), (3, 8, 1), (64, 48, 2)):
        assert lib.prosper_pt_bloom_fft_plan(w, h, s, C.byref(plan)) == -1, (w, h, s)
    assert lib.prosper_pt_bloom_fft_plan(64, 48, 0, None) == -1


def test_bad_arguments_are_rejected_before_touching_the_gpu():
    lib = capi.lib()
    il = np.zeros((48, 64, 4), np.float32)

    def refused(rc, words):
        return rc == -1 and words in lib.prosper_pt_last_error().decode()

    def bloom(pc=S.BloomFftPC.default(), w=64, h=48):
        return lib.prosper_pt_bloom_fft(None, None if pc is None else C.byref(pc), w, h, il.ctypes.data, 0, None)

    assert refused(bloom(), "null argument")  # only the context is missing
    assert refused(bloom(pc=None), "null argument")
    assert refused(bloom(pc=S.BloomFftPC.default(threshold=np.nan)), "non-finite")
    assert refused(bloom(pc=S.BloomFftPC.default(threshold=np.inf)), "non-finite")
    assert refused(bloom(pc=S.BloomFftPC.default(threshold=-1.0)), "negative")
    assert refused(bloom(pc=S.BloomFftPC.default(resolution_scale=2)), "unknown resolution scale")
    assert refused(bloom(pc=S.BloomFftPC.default(biquadratic=2)), "biquadratic")
    assert refused(bloom(pc=S.BloomFftPC.default(regenerate_kernel=2)), "regenerateKernel")
    for k in range(4):
        reserved = S.BloomFftPC.default()
        reserved.reserved[k] = 1
        assert refused(bloom(pc=reserved), "reserved")
    assert refused(bloom(w=0), "empty extent") and refused(bloom(h=0), "empty extent")
    assert refused(bloom(w=1), "working image empty") and refused(bloom(h=1), "working image empty")
    assert refused(bloom(pc=S.BloomFftPC.default(resolution_scale=1), w=64, h=3), "working image empty")
    assert refused(bloom(w=8193, h=2), "above 8192") and refused(bloom(w=2, h=8193), "above 8192")
    assert refused(bloom(w=8192, h=2), "null argument")  # the extent passes
    # the transform
    x = np.zeros((256, 256, 4), np.float32)
    for dim in (0, 128, 255, 384, 8192):
        assert refused(lib.prosper_pt_bloom_fft_transform(None, dim, 0, x.ctypes.data, x.ctypes.data, 0, None), "power of two")
    assert refused(lib.prosper_pt_bloom_fft_transform(None, 256, 2, x.ctypes.data, x.ctypes.data, 0, None), "inverse is 0 or 1")
    assert refused(lib.prosper_pt_bloom_fft_transform(None, 256, 0, x.ctypes.data, x.ctypes.data, 0, None), "null argument")
    buf = np.zeros(16, np.uint8)
    assert lib.prosper_pt_read_bloom_fft_stage(None, S.BLOOM_FFT_HIGHLIGHTS, buf.ctypes.data, 16, None) == -1
    assert lib.prosper_pt_read_bloom_fft_stage(None, 4, buf.ctypes.data, 16, None) == -1
    assert lib.prosper_pt_get_bloom_fft_info(None, None) == -1
    lib.prosper_pt_bloom_fft_release_kernel(None)  # (nothing to drop)
    # prosper_pt_bloom still refuses its reserved words
    old = S.BloomPC.default()
    old.reserved[0] = 1
    assert refused(lib.prosper_pt_bloom(None, C.byref(old), 8, 8, il.ctypes.data, 0, None), "reserved")


def test_prepare_at_an_odd_and_an_even_kernel_extent():
    # kernelDim 5: pIn = pOut + 2.5 below 128 (2.5, 3.5, 4.5, then outside) and pOut - 253.5 from 128 on (0.5 at 254)
    want = np.full(256, -1)
    want[[0, 1, 2, 254, 255]] = [2, 3, 4, 0, 1]
    assert (F.prepare_indices(5, 256) == want).all()
    # kernelDim 4: pIn = pOut + 2 and pOut - 254
    want = np.full(256, -1)
    want[[0, 1, 254, 255]] = [2, 3, 0, 1]
    assert (F.prepare_indices(4, 256) == want).all()
    # kernelDim 1: only pOut = 0 reads the texel (0.5 truncates to 0; -0.5 at 255 is outside)
    want = np.full(256, -1)
    want[0] = 0
    assert (F.prepare_indices(1, 256) == want).all()
    # the whole kernel when it fills the image: a shift by half
    assert (F.prepare_indices(256, 256) == (np.arange(256) + 128) % 256).all()
    k = np.arange(5 * 5 * 4, dtype=np.float32).reshape(5, 5, 4) + 1
    p = F.prepare(k, 256)
    assert p[0, 0, 0] == k[2, 2, 0] and p[255, 254, 2] == k[1, 0, 2] and p[1, 255, 0] == k[3, 1, 0]
    assert not p[..., 1].any() and not p[..., 3].any() and np.count_nonzero(p[..., 0]) == 25


@pytest.mark.parametrize("dim", [256, 512, 1024, 2048])
def test_the_schedule_agrees_with_the_dft(dim):
    """prosper's own passes in float32 against np.fft in float64.  A transform of log2(dim^2) radix-2 levels rounds a
    value at most about four times per level (twiddle, product, sum), each within eps of the largest magnitude; a wrong
    twiddle, index or normalisation is off by that magnitude itself."""
    assert F.radix_sequence(256) == [4, 8, 8] and F.radix_sequence(512) == [2, 16, 16] and F.radix_sequence(1024) == [4, 16, 16]
    assert F.radix_sequence(2048) == [8, 16, 16] and F.radix_sequence(4096) == [16, 16, 16]
    rng = np.random.default_rng(5)
    x = rng.standard_normal((dim, dim, 4)).astype(np.float32)
    eps = float(np.finfo(np.float32).eps)
    for inverse in (False, True):
        want = F.dft(x, inverse)
        got = F.prosper_schedule(x, inverse)
        bound = 4 * eps * 2 * np.log2(dim) * np.abs(want).max()
        err = np.abs(got - want).max()
        print("dim %d %s: error %.3e, bound %.3e, largest magnitude %.3e" % (dim, "inverse" if inverse else "forward", err, bound, np.abs(want).max()))
        assert err <= bound
    # forward, then inverse: dim times the input ((1 / dim) dim^2)
    back = F.dft(F.dft(x), inverse=True)
    assert np.abs(back - dim * x.astype(np.float64)).max() < 1e-9 * dim


def test_an_impulse_convolves_to_the_wrapped_kernel_shifted_there():
    dim, kd, scale = 256, 25, np.float32(0.08)
    kernel = F.kernel_image(kd).astype(np.float32)
    wrapped = F.prepare(kernel, dim)
    x0, y0, value = 37, 201, 3.5
    hl = np.zeros((dim, dim, 4), np.float64)
    hl[y0, x0, :3] = (value, 2 * value, 3 * value)
    got = F.convolve(hl, F.dft(wrapped), scale)
    shifted = np.roll(wrapped.astype(np.float64), (y0, x0), axis=(0, 1))
    want = np.stack([shifted[..., 0] * value, shifted[..., 0] * 2 * value, shifted[..., 2] * 3 * value], axis=-1) * float(scale)
    assert np.abs(got[..., :3] - want).max() < 1e-12 * np.abs(want).max() * dim
    assert np.abs(got[..., 3]).max() < 1e-12 * np.abs(want).max() * dim
    # the kernel is brightest at its centre, which prepare moves to the origin
    assert wrapped[0, 0, 0] == wrapped[..., 0].max() > 0 and (wrapped[..., 0] >= 0).all()


@pytest.mark.parametrize("kd", sorted({F.plan(w, h, s)[1] for w, h, s in EXTENTS} | {F.plan(w, h, s)[1] for w, h, s, _ in NEW_CASES}))
def test_no_sub_sample_of_the_kernel_image_lies_on_a_branch(kd):
    """A condition on the inputs of the GPU test: float64 on the device and here may differ in the last bits, which must
    not decide a branch of filterValue (dStar < 0, |p.y| < .005).  Over KERNEL_ROWS(kd), the rows the GPU test compares."""
    assert F.kernel_margins(25)[1] < 1e-15  # what the condition is there to keep out
    rows = KERNEL_ROWS(kd)
    star, streak = F.kernel_margins(kd, rows=rows)
    print("kernelDim %d, %d rows: |dStar| >= %.3e, ||p.y| - .005| >= %.3e" % (kd, len(rows), star, streak))
    assert star > 1e-9 and streak > 1e-9
    k = F.kernel_image(kd, rows=rows)
    assert k.shape == (len(rows), kd, 4) and np.isfinite(k).all() and (k >= 0).all()
    assert (k[..., 0] == k[..., 1]).all() and (k[..., 2] == k[..., 3]).all()


def test_the_rows_of_a_kernel_image_are_sampled_only_above_600():
    assert KERNEL_ROWS(1) == [0] and KERNEL_ROWS(600) == list(range(600))
    for kd in (601, 1050, 2050):
        rows = KERNEL_ROWS(kd)
        assert len(rows) == 24 and rows == sorted(set(rows)) and rows == KERNEL_ROWS(kd)
        assert {0, 1, kd // 2 - 1, kd // 2, kd // 2 + 1, kd - 2, kd - 1} <= set(rows) and 0 <= rows[0] and rows[-1] < kd
    # a kernelDim of 25 modulo 50 puts a row of sub-samples on |p.y| = .005 itself: why the portrait extents are 2100 and 4100
    assert F.kernel_margins(1025, rows=[515])[1] < 1e-15


def test_a_kernel_image_in_bands_equals_the_whole_one():
    for kd in (27, 150):
        whole = F.kernel_image(kd)
        assert F.kernel_image(kd, rows=list(range(kd))).tobytes() == whole.tobytes()
        assert F.kernel_margins(kd, rows=list(range(kd))) == F.kernel_margins(kd)
    some = [0, 74, 75, 149]
    assert F.kernel_image(150, rows=some).tobytes() == whole[some].tobytes()
    assert F.kernel_image(150, rows=[]).shape == (0, 150, 4)


@pytest.mark.parametrize("w,h,scale,biquadratic", LARGE_CASES)
def test_the_design_lights_the_rows_of_a_portrait_and_the_columns_of_a_landscape_extent(w, h, scale, biquadratic):
    """From the restatement alone, over the rectangle separate can light (the rest of a 4096^2 image is never formed): a
    portrait case lights every row below y_out, so the middle kernel's column tiles hold no empty row there; a landscape
    one lights at least 400 columns."""
    dim = F.plan(w, h, scale)[0]
    v, _, (x_out, y_out) = F.separate(B.design(w, h, SEED), B.THRESHOLD, scale, dim, crop=True)
    assert v.shape == (y_out, x_out, 3) and x_out <= dim and y_out <= dim
    lit = v.any(axis=-1)
    rows, columns = int(lit.any(axis=1).sum()), int(lit.any(axis=0).sum())
    print("%d x %d: %d of %d rows and %d of %d columns lit" % (w, h, rows, y_out, columns, x_out))
    if h > w:
        assert rows == y_out
    else:
        assert columns >= 400


def test_separate_over_the_rectangle_equals_the_whole_image_there():
    for w, h, scale in ((75, 55, F.HALF), (100, 70, F.QUARTER), (512, 512, F.HALF)):
        illum = B.design(w, h, SEED)
        v, s, outside = F.separate(illum, B.THRESHOLD, scale, 256)
        cv, cs, c_outside = F.separate(illum, B.THRESHOLD, scale, 256, crop=True)
        assert outside == c_outside == F.outside_from(w, h, scale)
        ny, nx = min(outside[1], 256), min(outside[0], 256)
        assert cv.shape == (ny, nx, 3) and (cv == v[:ny, :nx]).all() and (cs == s[:ny, :nx]).all()
        assert not v[ny:].any() and not v[:, nx:].any()
