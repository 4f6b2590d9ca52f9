"""The rule of the spatiotemporal denoiser (prosper_amd/denoise.py) without a GPU: hand-computed cases of the
statement, the properties that need no restatement, the proof that the shared design (tests/denoise_design.py) reaches
every path, and the binding (symbols, struct layouts against the header, defaults, refusals).  The GPU side:
tests/test_denoise.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_design as D
from prosper_amd import capi, denoise as R, structs as S

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "prosper_pt", "prosper_pt.h")).read()
FACING = (0.5, 0.5, 0.0, 1.0)  # normalMetallic of the normal (0, 0, 1): the decode gives it exactly


def flat(w, h, colour=1.0, z=2.0):
    """a facing plane at distance z: (illumination, albedo, normal_metallic, depth, velocity)"""
    il = np.zeros((h, w, 4), np.float32)
    il[..., :3] = colour
    il[..., 3] = 0.75
    depth = np.full((h, w), D.C32 / F(z) - D.C22, np.float32)
    return il, np.full((h, w, 4), 0.5, np.float32), np.tile(np.array(FACING, np.float32), (h, w, 1)), depth, np.zeros((h, w, 2), np.float32)


def run(pc, frames, history=None):
    out = None
    for f in frames:
        out = R.denoise(pc, D.C22, D.C32, *f, history=history)
        history = out["history"]
    return out


def same(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


# ---- the statement itself ----

def test_the_falloff_is_compact_and_exact():
    x = np.array([0.0, 4.0, 8.0, 9.0, 1e30, np.inf, np.nan], np.float32)
    assert R.falloff(x).tolist() == [1.0, 1.0 / 256.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert R.falloff(F(1.0)) == F(0.875) ** 8  # three exact squarings of 7/8


def test_the_normal_weight_squares_the_clamped_cosine():
    d = np.array([-0.5, 0.0, 0.5, 0.99, 1.0], np.float32)
    assert R.normal_weight(d, 0).tolist() == [0.0, 0.0, 0.5, float(F(0.99)), 1.0]
    assert R.normal_weight(d, 1).tolist() == [0.0, 0.0, 0.25, float(F(0.99) * F(0.99)), 1.0]
    by_hand = F(0.99)
    for _ in range(8):
        by_hand = by_hand * by_hand
    got = R.normal_weight(d, 8)
    assert got[3] == by_hand and 0.0 < got[3] < 0.08 and got[4] == 1.0
    assert got[2] == 0.0  # 2^-256 underflows: the weight is exactly 0


def test_the_facing_normal_decodes_exactly():
    assert R.decode_normal(np.array(FACING, np.float32)).tolist() == [0.0, 0.0, 1.0]


def test_a_one_by_one_image():
    il, al, nm, depth, vel = flat(1, 1, 0.3)
    r = run(R.PC(iterations=1, demodulate=0), [(il, al, nm, depth, vel)])
    assert R.bits(r["guide_a"][0, 0, 3]) == 1 and r["guide_a"][0, 0, 1:3].tolist() == [0.0, 0.0]
    assert r["guide_a"][0, 0, 0] == D.C32 / (depth[0, 0] + D.C22)
    l = (F(0.299) * F(0.3) + F(0.587) * F(0.3)) + F(0.114) * F(0.3)
    assert r["moments"][0, 0, :2].tolist() == [float(l), float(l * l)] and R.bits(r["moments"][0, 0, 2]) == 1
    assert r["temporal"][0, 0].tolist() == [float(F(0.3))] * 3 + [0.0]  # max(l l - l l, 0) * 4
    k = F(0.375) * F(0.375)  # the one tap: the centre
    want = (k * F(0.3)) / k
    assert r["atrous"][0][0, 0].tolist() == [float(want)] * 3 + [0.0]
    assert r["out"][0, 0].tolist() == [float(want)] * 3 + [0.75]
    assert r["counts"] == (0, 1)


def scalar_atrous(pc, step, ga, gb, img):
    """one a-trous pass written out per pixel with float32 scalars, for small images"""
    h, w = ga.shape[:2]
    out = np.array(img, np.float32)
    b3 = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))
    lum = lambda c: (F(0.299) * c[0] + F(0.587) * c[1]) + F(0.114) * c[2]
    geo = lambda y, x: 0 <= x < w and 0 <= y < h and R.bits(ga[y, x, 3]) != 0
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                if not geo(y, x):
                    continue
                gw = gv = F(0)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if geo(y + dy, x + dx):
                            k = (F(0.5) if dx == 0 else F(0.25)) * (F(0.5) if dy == 0 else F(0.25))
                            gw, gv = gw + k, gv + k * img[y + dy, x + dx, 3]
                denom = pc.sigma_luminance * np.sqrt(gv / gw) + F(1e-4)
                zp, gx, gy = ga[y, x, :3]
                sw = sv = F(0)
                sc = [F(0)] * 3
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        wk, qy, qx = b3[dx + 2] * b3[dy + 2], y + step * dy, x + step * dx
                        if (dx, dy) != (0, 0):
                            if not geo(qy, qx):
                                continue
                            xl = abs(lum(img[qy, qx]) - lum(img[y, x])) / denom
                            tx, ty = gx * F(step * dx), gy * F(step * dy)
                            xz = abs(ga[qy, qx, 0] - ((zp + tx) + ty)) / (pc.sigma_depth * (abs(tx) + abs(ty)) + F(1e-3) * zp)
                            wn = max(F(0), (gb[y, x, 0] * gb[qy, qx, 0] + gb[y, x, 1] * gb[qy, qx, 1]) + gb[y, x, 2] * gb[qy, qx, 2])
                            for _ in range(pc.normal_power_log2):
                                wn = wn * wn
                            t = max(F(0), F(1) - (xz + xl) * F(0.125))
                            t2 = t * t
                            t4 = t2 * t2
                            wk = wk * (wn * (t4 * t4))
                        sw = sw + wk
                        sc = [sc[c] + wk * img[qy, qx, c] for c in range(3)]
                        sv = sv + (wk * wk) * img[qy, qx, 3]
                out[y, x] = [sc[0] / sw, sc[1] / sw, sc[2] / sw, sv / (sw * sw)]
    return out


def test_a_three_by_three_image_with_one_pass_written_out_by_hand():
    # uniform: every weight is h(dx) h(dy), and sum(w 1) / sum(w) is exactly 1
    pc = R.PC(iterations=1, demodulate=0)
    r = run(pc, [flat(3, 3)])
    assert (r["atrous"][0][..., :3] == 1).all() and (r["atrous"][0][..., 3] == 0).all()
    # a black column beside two white ones, every variance 1/4, derived by hand in float64: vbar = 1/4, so the luminance
    # denominator is 4 * 1/2 + 1e-4; across the edge x_l = l(white) / 2.0001 and F = (1 - x_l / 8)^8, along it w = h h.
    # The rows' weights cancel.  Column 1 sees the black column at h = 1/4, column 2 at 1/16, column 0 sees the white ones.
    il, al, nm, depth, vel = flat(3, 3)
    t = R.temporal_stage(pc, D.C22, D.C32, il, al, nm, depth, vel, None)
    image = np.ones((3, 3, 4), np.float32)
    image[:, 0, :3] = 0.0
    image[..., 3] = 0.25
    got = R.atrous_pass(pc, 0, t["guide_a"], t["guide_b"], image).astype(np.float64)
    f = (1.0 - ((0.299 + 0.587 + 0.114) / 2.0001) / 8.0) ** 8
    assert abs(f - 0.59673) < 1e-5  # (15/16)^8 = 0.596719, a little more for the 1e-4
    want = [0.25 * f * 1.0 + 0.0625 * f * 1.0, 0.375 + 0.25, 0.375 + 0.25]
    norm = [0.375 + 0.25 * f + 0.0625 * f, 0.25 * f + 0.375 + 0.25, 0.0625 * f + 0.25 + 0.375]
    for x in range(3):
        assert np.allclose(got[:, x, :3], want[x] / norm[x], rtol=0, atol=2e-6), x
    # the variance: sum(w^2 v) / sum(w)^2 over the centre row's weights times the rows' (which do not cancel here)
    rows = {0: [0.375, 0.25, 0.0625], 1: [0.25, 0.375, 0.25], 2: [0.0625, 0.25, 0.375]}
    cols = {0: [0.375, 0.25 * f, 0.0625 * f], 1: [0.25 * f, 0.375, 0.25], 2: [0.0625 * f, 0.25, 0.375]}
    for y in range(3):
        for x in range(3):
            w2 = sum((a * b) ** 2 for a in rows[y] for b in cols[x])
            w1 = sum(a * b for a in rows[y] for b in cols[x])
            assert abs(got[y, x, 3] - 0.25 * w2 / w1 ** 2) < 2e-6, (y, x)
    # varied colours, depths and normals against the scalar loop
    d = D.design(3, 3, 0)
    d["depth"][0, 2] = 0
    r = run(R.PC(iterations=1), [D.inputs(d)])
    for step in (1, 2):
        want = scalar_atrous(pc, step, r["guide_a"], r["guide_b"], r["temporal"])
        assert same(R.atrous_pass(pc, step.bit_length() - 1, r["guide_a"], r["guide_b"], r["temporal"]), want)
    assert not same(r["atrous"][0], r["temporal"])


def test_the_history_length_counts_to_the_cap_under_zero_velocity():
    pc = R.PC(max_history_length=3)
    history, lengths = None, []
    for k in range(5):
        r = R.denoise(pc, D.C22, D.C32, *flat(4, 4, 0.25 * (k + 1)), history=history)
        history = r["history"]
        lengths.append(sorted(set(R.bits(r["moments"][..., 2]).ravel().tolist())))
    assert lengths == [[1], [2], [3], [3], [3]]


def dyadic_frames(w, h, vel):
    a, b = flat(w, h), flat(w, h)
    a[0][..., :3] = (np.arange(w * h).reshape(h, w, 1) % 16) / 8.0
    b[0][..., :3] = ((np.arange(w * h).reshape(h, w, 1) * 5) % 16) / 4.0
    b[4][...] = vel
    return a, b


def test_a_reprojection_that_lands_on_an_exact_texel():
    w, h = 8, 4
    a, b = dyadic_frames(w, h, (2.0 / w, 0.0))  # fetches the texel one to the left
    r = run(R.PC(iterations=0, demodulate=0), [a, b])
    want = 0.5 * a[0][:, :-1, :3] + 0.5 * b[0][:, 1:, :3]  # N' = 2: alpha 1/2; exact in float32
    assert same(r["temporal"][:, 1:, :3], want)
    assert (R.bits(r["moments"][:, 1:, 2]) == 2).all()
    # column 0 fetches column -1: the tap beside it lies inside with weight 0, which is no history
    assert same(r["temporal"][:, 0, :3], b[0][:, 0, :3]) and (R.bits(r["moments"][:, 0, 2]) == 1).all()
    assert r["counts"] == ((w - 1) * h, h)


def test_a_reprojection_between_four_texels():
    w, h = 8, 8
    a, b = dyadic_frames(w, h, (1.0 / w, -1.0 / h))  # half a texel left and up
    r = run(R.PC(iterations=0, demodulate=0), [a, b])
    p = a[0][..., :3]
    prev = ((0.25 * p[:-1, :-1] + 0.25 * p[:-1, 1:]) + 0.25 * p[1:, :-1]) + 0.25 * p[1:, 1:]
    assert same(r["temporal"][1:, 1:, :3], 0.5 * prev + 0.5 * b[0][1:, 1:, :3])
    # the first row and column keep the taps that lie inside, renormalised
    edge = (0.25 * p[0, :-1] + 0.25 * p[0, 1:]) / 0.5
    assert same(r["temporal"][0, 1:, :3], 0.5 * edge + 0.5 * b[0][0, 1:, :3])
    assert (R.bits(r["moments"][..., 2]) == 2).all()


# ---- properties that need no restatement ----

def check_passthrough(denoise):
    d = D.design(33, 17, 0)
    out = denoise(R.PC(iterations=0, demodulate=0), [d])
    valid = np.isfinite(d["illumination"][..., :3]).all(-1)
    assert (~valid).sum() >= 3
    assert same(out[valid], d["illumination"][valid])
    assert np.isfinite(out[..., :3]).all()


def half_planes(w=40, h=24):
    il, al, nm, depth, vel = flat(w, h, 0.0)
    il[:, w // 2:, :3] = 1.0
    depth[:, w // 2:] = D.C32 / F(9.0) - D.C22  # 2 against 9: beyond every tolerance
    return {"illumination": il, "albedo": al, "normal_metallic": nm, "depth": depth, "velocity": vel}


def check_half_planes(denoise):
    d = half_planes()
    out = denoise(R.PC(demodulate=0), [d, d, d])
    w = out.shape[1]
    assert (out[:, :w // 2, :3] == 0).all() and (out[:, w // 2:, :3] == 1).all()
    assert same(out[..., 3], d["illumination"][..., 3])


def check_sky(denoise):
    frames = [D.design(33, 17, k) for k in range(3)]
    out = denoise(R.PC(), frames)
    sky = frames[-1]["depth"] == 0
    assert sky.sum() >= 8 and same(out[sky], frames[-1]["illumination"][sky])


def check_outliers(denoise):
    """planted NaN / Inf texels (no history: it is 0) against the same input with those texels set to 0"""
    d = D.design(33, 17, 0)
    bad = ~np.isfinite(d["illumination"][..., :3]).all(-1)
    assert bad.sum() >= 3
    clean = dict(d, illumination=np.array(d["illumination"]))
    clean["illumination"][bad, :3] = 0.0
    for pc in (R.PC(), R.PC(demodulate=0, iterations=2)):
        got, want = denoise(pc, [d]), denoise(pc, [clean])
        assert np.isfinite(got[..., :3]).all()
        assert same(got[~bad], want[~bad]) and same(got[bad][:, :3], want[bad][:, :3])
    # with a history too every output stays finite
    frames = [D.design(33, 17, k) for k in range(4)]
    assert np.isfinite(denoise(R.PC(), frames)[..., :3]).all()
    # With a history the texel keeps its reprojected history unchanged: at 32 x 16 (uv and back is exact) and zero velocity
    # that is the texel's own value of the frame before, which the pass alone (no a-trous pass, no demodulation) hands on.
    frames = [D.design(32, 16, k) for k in range(3)]
    bad = ~np.isfinite(frames[2]["illumination"][..., :3]).all(-1)
    still = bad & (frames[2]["velocity"] == 0).all(-1) & (frames[2]["depth"] != 0)
    assert still.sum() >= 2
    pc = R.PC(iterations=0, demodulate=0)
    before, got = denoise(pc, frames[:2]), denoise(pc, frames)
    assert same(got[still][:, :3], before[still][:, :3])
    # ... and no neighbour beyond the filters' reach (one a-trous pass: 2 texels; the 7 x 7 variance window feeds the 3 x 3
    # Gaussian of a tap: 3 + 1 + 2) differs from the run over the same frame with those texels finite
    clean = dict(frames[2], illumination=np.array(frames[2]["illumination"]))
    clean["illumination"][bad, :3] = 0.0
    ys, xs = np.nonzero(bad)
    gy, gx = np.mgrid[0:16, 0:32]
    far = (np.maximum(abs(gy[..., None] - ys), abs(gx[..., None] - xs)) > 6).all(-1)
    assert far.sum() >= 8
    pc = R.PC(iterations=1, feedback_iteration=9)
    got, want = denoise(pc, frames), denoise(pc, frames[:2] + [clean])
    assert same(got[far], want[far]) and np.isfinite(got[..., :3]).all()


def statement(pc, frames):
    return run(pc, [D.inputs(f) for f in frames])["out"]


@pytest.mark.parametrize("check", [check_passthrough, check_half_planes, check_sky, check_outliers])
def test_properties_of_the_statement(check):
    check(statement)


# ---- the design reaches every path ----

@pytest.fixture(scope="module")
def full_design():
    w, h = D.FULL
    pc, history, frames = R.PC(max_history_length=4), None, []
    for k in range(D.FRAMES):
        r = R.denoise(pc, D.C22, D.C32, *D.inputs(D.design(w, h, k)), history=history)
        history = r["history"]
        frames.append(r)
    return pc, frames


def test_the_design_reaches_every_path(full_design):
    pc, frames = full_design
    w, h = D.FULL
    geometry = R.flag_of(frames[0]["guide_a"])
    assert (~geometry).sum() >= 8
    for r in frames[1:]:
        assert r["rejected_depth"].sum() >= 8 and r["rejected_normal"].sum() >= 8 and r["left_image"].sum() >= 8
        assert r["counts"][0] >= 8 and r["counts"][1] >= 8
    assert frames[0]["counts"][0] == 0
    length = [R.bits(r["moments"][..., 2]) for r in frames]
    assert ((length[2] < 4) & (length[2] > 0) & geometry).sum() >= 8        # the re-estimated variance in frame 2
    assert ((length[3] >= 4) & geometry).sum() >= 8                         # the temporal variance stands
    assert ((length[4] == pc.max_history_length) & (length[3] == pc.max_history_length)).sum() >= 8  # at the cap
    assert ((length[4] == 0) & geometry).sum() + ((length[0] == 0) & geometry).sum() >= 1  # an invalid sample without history
    invalid = ~np.isfinite(D.design(w, h, 2)["illumination"][..., :3]).all(-1)
    assert (invalid & (length[2] == length[1]) & (length[1] > 0)).sum() >= 1  # ... and with: the length not incremented
    # every tap of step 16 inside the image
    reach = np.ones((h, w), bool)
    for dy in (-32, 32):
        for dx in (-32, 32):
            reach &= R.tap(np.ones((h, w), np.float32), dx, dy)[1]
    assert (reach & geometry).sum() >= 8
    # each of the three terms alone: exactly 0, and strictly between 0 and 1
    r = frames[3]
    taps = [t for t in R.atrous_taps(pc, 0, r["guide_a"], r["guide_b"], r["temporal"]) if t[5] is not None]
    for term in range(3):
        zero = np.zeros((h, w), bool)
        between = np.zeros((h, w), bool)
        for _, _, ok, _, _, terms in taps:
            zero |= ok & (terms[term] == 0)
            between |= ok & (terms[term] > 0) & (terms[term] < 1)
        assert zero.sum() >= 8 and between.sum() >= 8, term


# ---- the binding ----

def struct_fields(name):
    body = HEADER[HEADER.index("typedef struct %s\n" % name):HEADER.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for kind, decl in re.findall(r"\b(const void \*|const float \*|uint32_t|float)\s*([^;]+);", body):
        names += [re.sub(r"\[.*", "", n.strip()) for n in decl.split(",")]
    return names


def test_the_symbols_are_exported():
    lib = capi.lib()
    for name in ("prosper_pt_denoise", "prosper_pt_denoise_pc_default", "prosper_pt_denoise_release_history",
                 "prosper_pt_read_denoise_stage", "prosper_pt_get_denoise_info"):
        assert hasattr(lib, name), name
    assert lib.prosper_pt_abi_version() == 4


def test_struct_layouts_match_the_header():
    assert struct_fields("prosper_pt_denoise_pc") == [n for n, _ in S.DenoisePC._fields_]
    assert struct_fields("prosper_pt_denoise_inputs") == [n for n, _ in S.DenoiseInputs._fields_]
    assert struct_fields("prosper_pt_denoise_info") == [n for n, _ in S.DenoiseInfo._fields_]
    assert C.sizeof(S.DenoisePC) == 44 and C.sizeof(S.DenoiseInputs) == 48 and C.sizeof(S.DenoiseInfo) == 8 * 4 + 9 * 4
    assert S.DenoiseInfo.atrousMs.size == 5 * 4
    stages = dict(re.findall(r"PROSPER_PT_DENOISE_([A-Z_0-9]+) = (\d+)", HEADER))
    assert {k: int(v) for k, v in stages.items()} == {
        "GUIDE_A": S.DENOISE_GUIDE_A, "GUIDE_B": S.DENOISE_GUIDE_B, "MOMENTS": S.DENOISE_MOMENTS, "TEMPORAL": S.DENOISE_TEMPORAL,
        "ATROUS_0": S.DENOISE_ATROUS_0, "HISTORY_COLOUR": S.DENOISE_HISTORY_COLOUR, "STAGE_COUNT": S.DENOISE_STAGE_COUNT}


def test_the_defaults_are_the_documented_ones():
    pc = S.DenoisePC()
    capi.lib().prosper_pt_denoise_pc_default(C.byref(pc))
    body = HEADER[HEADER.index("typedef struct prosper_pt_denoise_pc\n"):HEADER.index("} prosper_pt_denoise_pc;")]
    documented = re.findall(r"(?:uint32_t|float)\s+(\w+);\s*/\*.*?default ([0-9.]+) \*/", body, flags=re.S)
    assert [n for n, _ in documented] == [n for n, _ in S.DenoisePC._fields_]
    for (name, value), (_, kind) in zip(documented, S.DenoisePC._fields_):
        assert getattr(pc, name) == kind(float(value) if kind is C.c_float else int(value)).value, name
        assert getattr(S.DenoisePC.default(), name) == getattr(pc, name), name
    ref = R.PC()
    assert (ref.iterations, ref.demodulate, ref.max_history_length, ref.feedback_iteration, ref.normal_power_log2, ref.reset_history) == (
        pc.iterations, pc.demodulate, pc.maxHistoryLength, pc.feedbackIteration, pc.normalPowerLog2, pc.resetHistory)
    assert [float(v) for v in (ref.min_alpha, ref.depth_tolerance, ref.normal_threshold, ref.sigma_depth, ref.sigma_luminance)] == [
        pc.minAlpha, pc.depthTolerance, pc.normalThreshold, pc.sigmaDepth, pc.sigmaLuminance]
    capi.lib().prosper_pt_denoise_pc_default(None)  # tolerated


def refused(pc=None, inputs=None, camera=True, w=8, h=8, text=None):
    pc = S.DenoisePC.default() if pc is None else pc
    inputs = S.DenoiseInputs() if inputs is None else inputs
    cam = S.CameraUniforms()
    rc = capi.lib().prosper_pt_denoise(None, C.byref(pc) if pc else None, C.byref(cam) if camera else None, w, h,
                                       C.byref(inputs) if inputs else None, None)
    assert rc == -1
    if text:
        assert text in capi.lib().prosper_pt_last_error().decode()


def test_refusals_that_need_no_device():
    refused(pc=False, text="null argument")
    refused(inputs=False, text="null argument")
    refused(camera=False, text="null argument")
    refused(text="null argument")  # everything valid but the context
    for field, value, text in (("iterations", 6, "iterations"), ("demodulate", 2, "0 or 1"), ("resetHistory", 2, "0 or 1"),
                               ("maxHistoryLength", 0, "maxHistoryLength"), ("maxHistoryLength", 256, "maxHistoryLength"),
                               ("normalPowerLog2", 9, "normalPowerLog2"), ("minAlpha", 1.5, "minAlpha")):
        pc = S.DenoisePC.default()
        setattr(pc, field, value)
        refused(pc=pc, text=text)
    for field in ("minAlpha", "depthTolerance", "normalThreshold", "sigmaDepth", "sigmaLuminance"):
        for value, text in ((float("nan"), "non-finite"), (float("inf"), "non-finite"), (0.0, "positive"), (-1.0, "positive")):
            pc = S.DenoisePC.default()
            setattr(pc, field, value)
            refused(pc=pc, text=text)
    refused(w=0, text="empty extent")
    refused(h=0, text="empty extent")
    refused(w=32769, text="32768")
    refused(h=32769, text="32768")
    for given in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        refused(inputs=S.DenoiseInputs(None, *[4096 if g else None for g in given], None, 0), text="together")
    refused(inputs=S.DenoiseInputs(4096 + 8, None, None, None, None, 1), text="16-byte")
    refused(inputs=S.DenoiseInputs(None, 4096 + 4, 4096, 4096, None, 1), text="16-byte")
    refused(inputs=S.DenoiseInputs(None, 4096, 4096 + 8, 4096, None, 1), text="16-byte")
    refused(inputs=S.DenoiseInputs(None, 4096, 4096, 4096 + 2, None, 1), text="4-byte")
    refused(inputs=S.DenoiseInputs(None, None, None, None, 4096 + 4, 1), text="8-byte")
    lib = capi.lib()
    assert lib.prosper_pt_read_denoise_stage(None, S.DENOISE_STAGE_COUNT, None, 0, None) == -1
    assert lib.prosper_pt_read_denoise_stage(None, 0, None, 0, None) == -1
    assert lib.prosper_pt_get_denoise_info(None, None) == -1
    lib.prosper_pt_denoise_release_history(None)  # tolerated
