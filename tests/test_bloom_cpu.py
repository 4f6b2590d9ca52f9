"""Bloom without a GPU: the host-only entry, the struct sizes, the refusals that need no context, the numpy
restatement's known answers and what the test design (tests/bloom_reference.py) reaches of the passes.  The GPU side:
tests/test_bloom.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bloom_reference as R
from prosper_amd import capi, structs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("prosper_pt_bloom", "prosper_pt_bloom_streak_weights", "prosper_pt_read_bloom_stage", "prosper_pt_get_bloom_info",
               "prosper_host_bloom_create", "prosper_host_bloom_destroy", "prosper_host_bloom_draw_ui", "prosper_host_bloom_record")
# (w, h, resolution scale): the smallest extents at which each rule can go wrong (see tests/test_bloom.py)
HALF_EXTENTS = ((8, 8), (17, 9), (101, 71), (130, 33), (258, 20), (2100, 8))
QUARTER_EXTENTS = ((32, 32), (100, 70), (258, 36))
EXTENTS = [(w, h, R.HALF) for w, h in HALF_EXTENTS] + [(w, h, R.QUARTER) for w, h in QUARTER_EXTENTS]
# (w, h, resolution scale, biquadratic): every extent with prosper's default sampling, two also with the bilinear one
CASES = [(w, h, s, 1) for w, h, s in EXTENTS] + [(101, 71, R.HALF, 0), (100, 70, R.QUARTER, 0)]
SEED = 11


def test_new_symbols_are_exported_and_the_abi_version_is_unchanged():
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4


def header_struct_size(name):
    """The size of a header struct whose fields are 4-byte scalars and arrays of them."""
    text = open(os.path.join(ROOT, "include", "prosper_pt", "prosper_pt.h")).read()
    body = text[text.index("typedef struct " + name):text.index("} " + name + ";")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    words = 0
    for decl in re.findall(r"\b(?:uint32_t|int32_t|float)\s+([^;]+);", body):
        for field in decl.split(","):
            m = re.search(r"\[(\d+)\]", field)
            words += int(m.group(1)) if m else 1
    return 4 * words


def test_struct_sizes_equal_the_headers():
    assert C.sizeof(S.BloomPC) == header_struct_size("prosper_pt_bloom_pc") == 32
    assert C.sizeof(S.BloomInfo) == header_struct_size("prosper_pt_bloom_info") == 64
    pc = S.BloomPC.default()
    assert (pc.threshold, list(pc.blendFactors), pc.resolutionScale, pc.biquadratic, list(pc.reserved)) == (
        1.0, [np.float32(0.9), np.float32(0.04), np.float32(0.04)], 0, 1, [0, 0])


@pytest.mark.parametrize("h", [1, 2, 9, 10, 11, 32, 262])
def test_streak_weights_equal_the_formula_to_the_last_bit(h):
    rg, b = capi.bloom_streak_weights(h)
    want_rg, want_b = R.streak_weights(h)
    assert rg.shape == b.shape == (2 * h,)
    assert (rg.view(np.uint32) == want_rg.view(np.uint32)).all() and (b.view(np.uint32) == want_b.view(np.uint32)).all()
    i = np.arange(-h, h)
    ratio = rg.astype(np.float64) / b.astype(np.float64)
    assert np.allclose(ratio[np.abs(i) < 10], 0.05, rtol=2e-7, atol=0) and np.allclose(ratio[np.abs(i) >= 10], 0.01, rtol=2e-7, atol=0)
    assert b[h] == 600.0 and (b > 0).all()  # i = 0: 4 * (0 + 1 + 0) * 150


def test_bad_arguments_are_rejected_before_touching_the_gpu():
    lib = capi.lib()
    il = np.zeros((8, 8, 4), np.float32)

    def refused(rc, words):
        return rc == -1 and words in lib.prosper_pt_last_error().decode()

    def bloom(pc=S.BloomPC.default(), w=8, h=8):
        return lib.prosper_pt_bloom(None, None if pc is None else C.byref(pc), w, h, il.ctypes.data, 0, None)

    assert refused(bloom(), "null argument")  # only the context is missing
    assert refused(bloom(pc=None), "null argument")
    assert refused(bloom(pc=S.BloomPC.default(threshold=np.nan)), "non-finite")
    assert refused(bloom(pc=S.BloomPC.default(blend_factors=(0.9, np.inf, 0.04))), "non-finite")
    assert refused(bloom(pc=S.BloomPC.default(threshold=-1.0)), "negative")
    assert refused(bloom(pc=S.BloomPC.default(blend_factors=(0.9, 0.04, -0.04))), "negative")
    assert refused(bloom(pc=S.BloomPC.default(resolution_scale=2)), "unknown resolution scale")
    assert refused(bloom(pc=S.BloomPC.default(biquadratic=2)), "biquadratic")
    reserved = S.BloomPC.default()
    reserved.reserved[1] = 1
    assert refused(bloom(pc=reserved), "reserved")
    assert refused(bloom(w=0), "empty extent") and refused(bloom(h=0), "empty extent")
    assert refused(bloom(w=7), "blurred level empty") and refused(bloom(h=7), "blurred level empty")
    assert refused(bloom(pc=S.BloomPC.default(resolution_scale=1), w=31, h=32), "blurred level empty")
    assert refused(bloom(pc=S.BloomPC.default(resolution_scale=1), w=32, h=32), "null argument")  # the extent passes
    buf = np.zeros(16, np.uint8)
    assert lib.prosper_pt_read_bloom_stage(None, S.BLOOM_HIGHLIGHTS, 0, buf.ctypes.data, 16, None) == -1
    assert lib.prosper_pt_read_bloom_stage(None, 3, 0, buf.ctypes.data, 16, None) == -1
    assert lib.prosper_pt_get_bloom_info(None, None) == -1


def test_the_blur_weights_sum_to_one_and_a_constant_image_stays_constant():
    assert abs(sum(R.WEIGHTS) - 1.0) < 1e-12
    src = np.full((20, 24, 4), 0.75, np.float16)
    for vertical in (False, True):
        v = R.blur_pass(src, vertical)[0]
        assert np.abs(v[4:-4, 4:-4] - 0.75).max() < 1e-12
        assert (v[:, 0] < 0.75).all() if not vertical else (v[0] < 0.75).all()  # the border darkens the edge


def test_known_answers_of_the_restatement():
    # separate at Half is the mean of 2 x 2 input texels, with the border at coord 0; at Quarter the mean of 4 x 4 texel
    # corners, i.e. of the texels 4c-2 .. 4c+1 with weights 1, 2 (the two middle ones shared by two lookups) ...
    il = np.zeros((8, 8, 4), np.float32)
    il[..., :3] = 3.0
    v, s = R.separate(il, 1.0, R.HALF)
    assert v.shape == (4, 4, 3) and np.allclose(v[1:, 1:], 2.0) and np.allclose(v[0, 0], 0.0)
    assert np.allclose(v[0, 1:], 0.5) and np.allclose(s[1:, 1:], 4.0)
    il = np.zeros((32, 32, 4), np.float32)
    il[..., :3] = 5.0
    v, _ = R.separate(il, 1.0, R.QUARTER)
    assert v.shape == (8, 8, 3) and np.allclose(v[1:, 1:], 4.0) and np.allclose(v[0, 1:], 1.5)
    # reduce: a level-0 image of 5 x 3 texels: level 1 is 2 x 1, levels 2 and 3 are 1 x 1 and take in virtual texels
    l0 = np.zeros((3, 5, 4), np.float16)
    l0[..., 0] = np.arange(5, dtype=np.float16)[None, :]
    assert np.allclose(R.reduce_level(1, l0)[0][..., 0], [[0.5, 2.5]])
    assert np.allclose(R.reduce_level(2, l0)[0][..., 0], [[1.5]])
    assert np.allclose(R.reduce_level(3, l0)[0][..., 0], [[(1.5 + 4.0) / 2]])  # the virtual texels 4 .. 7 are the edge texel 4
    # compose with the bilinear sampling on a constant level adds blend * constant everywhere (edge sampler)
    il = R.design(16, 16)
    lv = [np.full((8 >> l, 8 >> l, 4), 2.0, np.float16) for l in range(3)]
    for biquadratic in (False, True):
        v, _, _ = R.compose(il, lv, (0.5, 0.25, 0.125), R.HALF, biquadratic)
        assert np.allclose(v, il[..., :3].astype(np.float64) + 2.0 * 0.875, rtol=1e-12)
    # the streak of a single lit level-0 texel pair lands on every texel of the level-1 row, blue 20 (rg) / 100 (rg far) times red
    l0 = np.zeros((8, 64, 4), np.float16)
    l0[2:4, 30:32, :3] = 1.0
    l1 = R.half(np.concatenate([R.reduce_level(1, l0)[0], np.zeros((4, 32, 1))], axis=-1))
    total, _, taps, streak = R.blur_pass(l1, False, l0)
    assert (streak[1, :, 2] > 0).all() and not streak[0].any() and not streak[2:].any()
    ratio = streak[1, :, 0] / streak[1, :, 2]
    assert np.allclose(ratio[np.abs(np.arange(32) - 15) < 10], 0.05) and np.allclose(ratio[np.abs(np.arange(32) - 15) >= 10], 0.01)
    assert np.allclose(total, taps + streak)


@pytest.mark.parametrize("w,h,scale", EXTENTS, ids=["%dx%d-%s" % (w, h, "half" if s == 0 else "quarter") for w, h, s in EXTENTS])
def test_the_design_reaches_every_rule(w, h, scale):
    """The coverage conditions, from the restatement alone."""
    il = R.design(w, h, SEED)
    assert il.dtype == np.float32 and (il[..., 3] == 0.25).all()
    c = R.coverage(il, scale)
    print("%dx%d scale %d: %s" % (w, h, scale, c))
    assert 0.20 <= c["lit_share"] <= 0.80
    assert c["zero_beside_lit"] >= 1
    if c["level1_texels"] >= 100:
        assert c["streak_dominant"] >= 100
    if w * h >= 1000:
        assert all(n >= 100 for n in c["compose_level_pixels"])
