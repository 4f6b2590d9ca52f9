"""The G-buffer passes (deferred shading with and without IBL, the ReSTIR-DI resampling passes) over synthetic G-buffers
that sweep their inputs (tests/gbuffer_sweep.py), where the rendered scenes of the other tests leave them unexercised:
the radiance mip blend, the border texels of every IBL cube level, the BRDF LUT's clamp rows and first interval,
roughness below 0.05, the cluster lookup at extents that are no whole number of tiles, images of fewer than 8 tiles,
and neighbour pairs on either side of the spatial pass's two thresholds.  On the CPU: the builder and the shares every
GPU check relies on, from the references alone."""
import functools

import numpy as np
import pytest

import deferred_shading_reference as D
import gbuffer_sweep as G
import ibl_reference as I
import restir_resampling_reference as R
from conftest import same_bits
from prosper_amd import scenes, structs as S
from test_deferred_shading import ABS, REL, _cluster_check
from test_restir_di_resampling import _check_against_reference, pack

IBL_W, IBL_H = 160, 96
DIRECT_CASES = {"100x70": (100, 70, 1), "130x33": (130, 33, 1), "17x9": (17, 9, 1), "1x1": (1, 1, 1),
                "100x70_resolution_x2": (100, 70, 2)}
BAND_EXTENTS = {"100x70": (100, 70), "17x9": (17, 9)}


# ---- the builder ----

def _cornell_camera(oracle, w, h, resolution=None):
    c = scenes.cornell().camera
    rw, rh = resolution or (w, h)
    return oracle.camera_uniforms(c["eye"], c["target"], c["up"], c["fov"], c["zN"], c["zF"], rw, rh)[0]


@pytest.mark.parametrize("scale", [1, 2])
def test_builder_round_trips_through_the_reference_surface(oracle, scale):
    w, h = 100, 70
    cam = _cornell_camera(oracle, w, h, (w * scale, h * scale))
    rng = np.random.default_rng(1)
    lin = -np.exp(rng.uniform(np.log(0.05), np.log(150.0), (h, w)))
    lin[rng.uniform(size=(h, w)) < 0.1] = 0.0
    normal = rng.standard_normal((h, w, 3)) * rng.uniform(0.1, 3.0, (h, w, 1))
    albedo, rough, metal = rng.uniform(size=(h, w, 3)), rng.uniform(size=(h, w)), rng.uniform(size=(h, w))
    ar, nm, depth = G.build(cam, lin, normal, albedo, rough, metal)
    assert ar.dtype == nm.dtype == depth.dtype == np.float32
    sf = R.Surfaces(cam, ar, nm, depth)
    hit = lin.ravel() != 0.0
    assert (depth.ravel()[~hit] == 0.0).all() and (depth.ravel()[hit] != 0.0).all()
    assert np.abs(sf.lin_depth[hit] / lin.ravel()[hit] - 1.0).max() <= 1e-6
    unit = (normal / np.linalg.norm(normal, axis=-1, keepdims=True)).reshape(-1, 3)
    assert np.abs(sf.n - unit).max() <= 1e-6
    assert np.abs(sf.albedo - albedo.reshape(-1, 3)).max() <= 1e-7 and np.abs(sf.rough - rough.ravel()).max() <= 1e-7
    assert np.abs(sf.metal - metal.ravel()).max() <= 1e-7
    # the designed view vector and position are the surface's
    px, py = sf.px.astype(np.float64), sf.py.astype(np.float64)
    assert np.abs(G.view_vectors(cam, px, py, (w, h)) - sf.v)[hit].max() <= 1e-6
    pos = G.positions(cam, px, py, lin.ravel(), (w, h))
    assert (np.abs(pos - sf.pos)[hit].max(-1) <= 1e-5 * np.abs(lin.ravel()[hit])).all()


def test_aimed_normals_reflect_the_view_ray_onto_the_target(oracle):
    w, h = 100, 70
    cam = _cornell_camera(oracle, w, h)
    rng = np.random.default_rng(2)
    py, px = [a.ravel() for a in np.mgrid[0:h, 0:w]]
    v = G.view_vectors(cam, px, py)
    target = I.normalize(rng.standard_normal((w * h, 3)))
    target = np.where(((target * v).sum(-1) < -0.9)[:, None], -target, target)  # (v + target would all but cancel)
    lin = -rng.uniform(0.5, 20.0, w * h)
    n = G.aim_reflection(cam, px, py, lin, target)
    ar, nm, depth = G.build(cam, lin.reshape(h, w), n.reshape(h, w, 3), np.ones((h, w, 3)), np.ones((h, w)), np.zeros((h, w)))
    sf = R.Surfaces(cam, ar, nm, depth)
    reflected = -sf.v - 2.0 * (sf.n * -sf.v).sum(-1, keepdims=True) * sf.n
    assert np.abs(reflected - target).max() <= 1e-5


@pytest.mark.parametrize("n", [512, 64, 2, 1])
def test_edge_band_directions_touch_every_edge_and_corner(n):
    d = G.edge_band_directions(n)
    assert np.abs(np.linalg.norm(d, axis=-1) - 1.0).max() < 1e-12 and (I.switch_margin(d) >= 1e-5).all()
    face, i0, j0, holds_border = G.footprint(d, n)
    assert (i0 >= -1).all() and (i0 <= n - 1).all() and (j0 >= -1).all() and (j0 <= n - 1).all()
    edges, corners = set(), set()
    outside = np.zeros(len(d), bool)
    for di in (0, 1):
        for dj in (0, 1):
            i, j = i0 + di, j0 + dj
            out_i, out_j = (i < 0) | (i >= n), (j < 0) | (j >= n)
            outside |= out_i | out_j
            # where the border texel's centre lies: on the face across the edge, or past the corner
            c = I.face_dir(face, 2.0 * (i + 0.5) / n - 1.0, 2.0 * (j + 0.5) / n - 1.0)
            across = I.face_coords(c)[0]
            for k in np.nonzero(out_i ^ out_j)[0]:
                edges.add(frozenset((int(face[k]), int(across[k]))))
            for k in np.nonzero(out_i & out_j)[0]:
                corners.add(tuple(np.sign(c[k]).astype(int)))
    assert outside.all() and holds_border.all(), "%d directions read no border texel" % (~outside).sum()
    assert len(edges) == 12 and all(len(e) == 2 for e in edges), sorted(map(sorted, edges))
    assert len(corners) == 8, sorted(corners)


# ---- the IBL evaluation sweep ----

@functools.lru_cache(maxsize=None)
def _ibl_design(oracle):
    world = G.ibl_world()
    fov = world.camera["fov"]
    cams = [oracle.camera_uniforms((0.0, 0.0, 0.0), (0.0, 0.0, z), (0.0, 1.0, 0.0), fov, 0.1, 100.0, IBL_W, IBL_H)[0]
            for z in (-1.0, 1.0)]
    gbuffers, view, pixel, entries = G.ibl_sweep(cams, IBL_W, IBL_H)
    surfaces = [R.Surfaces(cam, *gb) for cam, gb in zip(cams, gbuffers)]
    return world, cams, gbuffers, view, pixel, entries, surfaces


def _ibl_bookkeeping(sf, idx):
    """Of the pixels idx: (left out: a cube direction within 1e-5 of a face switch; grazing; weight [k, 10]: what the
    trilinear lookup gives each radiance level; border [k, 10]: the levels that have at least 0.2 of it and whose
    footprint holds a border texel; the blend fraction; whether the irradiance cube's footprint holds a border texel).
    The level comes from the stored float32 roughness: (m + 0) / 10 may round to just below level m, which then has
    all but 1e-7 of the weight as the upper level of the blend."""
    n, v, rough = sf.n[idx], sf.v[idx], sf.rough[idx]
    refl = -v - 2.0 * (n * -v).sum(-1, keepdims=True) * n
    left_out = np.minimum(I.switch_margin(n), I.switch_margin(refl)) < 1e-5
    grazing = np.clip((n * v).sum(-1), 0.0, 1.0) < 1.5 / 512
    lod = np.clip(rough * 10.0, 0.0, I.MIPS - 1.0)
    l0 = np.floor(lod).astype(np.int64)
    t = lod - l0
    k = np.arange(len(idx))
    weight = np.zeros((len(idx), I.MIPS))
    weight[k, l0] = 1.0 - t
    weight[k, np.minimum(l0 + 1, I.MIPS - 1)] += t
    border = np.zeros((len(idx), I.MIPS), bool)
    for m in range(I.MIPS):
        sel = weight[:, m] >= 0.2
        border[sel, m] = G.footprint(refl[sel], I.RAD >> m)[3]
    return left_out, grazing, weight, border, t, G.footprint(n, I.IRR)[3]


def test_ibl_sweep_design_keeps_its_shares(oracle):
    """From the reference alone: at most 1 % of the designed pixels are left out or grazing; per radiance level at least
    200 read a border texel and (below level 9) at least 200 blend with a fraction in [0.2, 0.8]; the irradiance group
    reads the 64^2 cube's borders; every LUT clamp is met."""
    world, cams, gbuffers, view, pixel, e, surfaces = _ibl_design(oracle)
    k = len(view)
    assert k <= 15000 and len(set(zip(view.tolist(), pixel.tolist()))) == k, "every entry has a pixel of its own"
    weak, per_level_border, per_level_blend = 0, np.zeros(10, int), np.zeros(10, int)
    irr_border, rows, cols = 0, [], []
    for a, sf in enumerate(surfaces):
        sel = view == a
        idx = pixel[sel]
        left_out, grazing, weight, border, t, iborder = _ibl_bookkeeping(sf, idx)
        weak += int((left_out | grazing).sum())
        ok = ~left_out & ~grazing
        rad = e["group"][sel] == G.RADIANCE
        assert (weight[rad, e["level"][sel][rad]] > 0.0).all(), "the designed roughness reads the level aimed at"
        NoV = (sf.n[idx] * sf.v[idx]).sum(-1)
        assert NoV[rad].min() >= 0.3 and NoV[e["group"][sel] == G.IRRADIANCE].min() >= 0.3
        for m in range(10):
            per_level_border[m] += int((ok & rad & border[:, m]).sum())
            per_level_blend[m] += int((ok & rad & (weight[:, m] >= 0.2) & (t >= 0.2) & (t <= 0.8)).sum())
        irr_border += int((ok & (e["group"][sel] == G.IRRADIANCE) & iborder).sum())
        lut = e["group"][sel] == G.LUT_GRID
        assert np.abs(NoV[lut] - e["nov"][sel][lut]).max() <= 1e-6
        rows.append(np.floor(sf.rough[idx][lut] * 512 - 0.5))
        cols.append(np.floor(NoV[lut] * 512 - 0.5))
    assert weak <= 0.01 * k, "%d of %d designed pixels left out or grazing" % (weak, k)
    assert (per_level_border >= 200).all(), per_level_border
    assert (per_level_blend[:9] >= 200).all(), per_level_blend
    assert irr_border >= 1000, irr_border
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    assert rows.min() == -1 and rows.max() == 511 and cols.min() == 1 and cols.max() == 511
    assert (e["rough"] == 0.0).sum() >= 50 and (e["rough"] == 1.0).sum() >= 50


def test_sweep_sky_has_contrast_across_the_face_edges():
    """From the reference's generation of seeded edge texels: the irradiance cube and radiance levels 1, 4 and 8 under
    sweep_sky differ across the face edges by at least EDGE_CONTRAST at the median, so a border that held the wrong
    texel shows."""
    sky = I.sky64(G.ibl_world())
    for name, n, generate in (("irradiance", I.IRR, lambda f, i, j: I.irradiance(sky, f, i, j)[0]),
                              ("radiance 1", I.RAD >> 1, lambda f, i, j: I.prefilter(sky, 1, f, i, j)[0]),
                              ("radiance 4", I.RAD >> 4, lambda f, i, j: I.prefilter(sky, 4, f, i, j)[0]),
                              ("radiance 8", I.RAD >> 8, lambda f, i, j: I.prefilter(sky, 8, f, i, j)[0])):
        inside, across = G.edge_pairs(n, per_edge=6)
        contrast = G.edge_contrast(generate(*inside), generate(*across))
        print("sweep sky %s: median contrast across the face edges %.4f" % (name, contrast))
        assert contrast >= G.EDGE_CONTRAST, (name, contrast)


def _map_edge_contrast(cube):
    cube = np.asarray(cube, np.float64)
    (f, i, j), (f2, i2, j2) = G.edge_pairs(cube.shape[1])
    return G.edge_contrast(cube[f, j, i, :3], cube[f2, j2, i2, :3])


@pytest.mark.gpu
def test_gpu_ibl_sweep_matches_the_reference(gpu_ctx, oracle):
    """deferred shading with ibl = 1 over the two designed views against ibl_reference.eval_ibl over the maps read back
    from the same context: test_image_based_lighting's rule (REL of the summed absolute terms + ABS; 1e-2 where
    NoV < 1.5 / 512), pixels within 1e-5 of a face switch left out."""
    world, cams, gbuffers, view, pixel, e, surfaces = _ibl_design(oracle)
    gpu_ctx.upload_scene(world)
    gpu_ctx.generate_ibl()
    maps = gpu_ctx.read_ibl()
    # the generated maps differ across every cube's face edges: a wrong border texel moves the lookups that read it
    for name, cube in [("irradiance", maps["irradiance"])] + [("radiance %d" % m, maps["radiance"][m]) for m in range(10)]:
        contrast = _map_edge_contrast(cube)
        print("ibl sweep %-18s median contrast across the face edges %.4f" % (name, contrast))
        assert contrast >= G.EDGE_CONTRAST, (name, contrast)
    worst = {}
    per_level_border, per_level_blend, weak = np.zeros(10, int), np.zeros(10, int), 0
    failures = []
    for a, (cam, gb, sf) in enumerate(zip(cams, gbuffers, surfaces)):
        gpu_ctx.deferred_shading(cam, *gb, ibl=1)
        got = gpu_ctx.read_hdr()
        assert (got[..., 3] == 1.0).all()
        sel = view == a
        idx, group = pixel[sel], e["group"][sel]
        want, total, margin = I.eval_ibl(sf, idx, maps)
        left_out, grazing, weight, border, t, _ = _ibl_bookkeeping(sf, idx)
        assert ((margin < 1e-5) == left_out).all()
        g = got[..., :3].reshape(-1, 3)[idx].astype(np.float64)
        assert np.isfinite(g).all()
        ratio = np.abs(g - want).max(-1) / (np.where(grazing, 1e-2, REL) * total + ABS)
        checked = ~left_out
        weak += int((left_out | grazing).sum())
        rad = group == G.RADIANCE
        for m in range(10):
            per_level_border[m] += int((checked & ~grazing & rad & border[:, m]).sum())
            per_level_blend[m] += int((checked & ~grazing & rad & (weight[:, m] >= 0.2) & (t >= 0.2) & (t <= 0.8)).sum())
        labels = [(G.GROUP_NAMES[G.RADIANCE] + " level %d" % m, rad & (e["level"][sel] == m)) for m in range(10)]
        labels += [(G.GROUP_NAMES[k], group == k) for k in (G.IRRADIANCE, G.LUT_GRID, G.INTERIOR)]
        for name, s in labels:
            s = s & checked
            count, w = worst.get(name, (0, 0.0))
            worst[name] = (count + int(s.sum()), max(w, float(ratio[s].max()) if s.any() else 0.0))
        for j in np.nonzero(checked & (ratio > 1.0))[0]:
            failures.append((a, int(idx[j]), G.GROUP_NAMES[group[j]], float(ratio[j]), float(sf.rough[idx[j]])))
        assert (want.sum(-1) > 0).mean() > 0.9, "the IBL term lights the designed pixels"
    for name, (count, w) in worst.items():
        print("ibl sweep %-18s %5d pixels, worst error %.3f of the allowance" % (name, count, w))
    assert not failures, "%d pixels off (view, pixel, group, error / allowance, roughness): %s" % (len(failures), failures[:10])
    assert weak <= 0.01 * len(view)
    assert (per_level_border >= 200).all(), per_level_border
    assert (per_level_blend[:9] >= 200).all(), per_level_blend


# ---- the direct-lighting sweep ----

@functools.lru_cache(maxsize=None)
def _sweep_world(oracle):
    return G.sweep_world(oracle)


@functools.lru_cache(maxsize=None)
def _direct_design(oracle, case):
    w, h, scale = DIRECT_CASES[case]
    world = _sweep_world(oracle)
    cam = G.sweep_camera(oracle, world, w, h, (w * scale, h * scale))
    gb, low = G.direct_design(cam, w, h)
    return world, cam, gb, low


def _conditioning_limited(extra, total, low):
    """How many of the low-roughness pixels carry a conditioning term above REL * total, and the group's size."""
    return int((low & (extra > REL * total)).sum()), int(low.sum())


@pytest.mark.parametrize("case", sorted(DIRECT_CASES))
def test_direct_sweep_design_keeps_its_shares(oracle, case):
    """From the reference alone (the lists are the reference's own clustering): nearly every hit's slice is decided,
    the depths reach from before the near plane to past slice 16, at most 10 % of the low-roughness group is limited by
    the conditioning of trowbridgeReitz's denominator, and the short-range point lights make the lists matter: a
    pixel's own cluster misses lights that others list.  17 x 9 and 1 x 1 hold too few pixels for the spreads: there
    the slice margins and the conditioning share are established (17 x 9 has 26 low-roughness pixels; the one pixel of
    1 x 1 is a hit of the main group, so that case checks no low-roughness pixel)."""
    world, cam, (ar, nm, depth), low = _direct_design(oracle, case)
    h, w = depth.shape
    visible, _ = D.clusters(world, cam, w, h)
    lists = (visible, np.ones(visible.shape[:3] + (world.spot_lights.count,), bool))
    want, total, margin = D.shade(world, cam, ar, nm, depth, lists=lists)
    hit = depth != 0.0
    assert hit.any() and (margin > 1e-4)[hit].mean() > 0.99
    assert np.isfinite(want).all()
    extra = G.shade_conditioning(world, cam, ar, nm, depth, lists)
    limited, size = _conditioning_limited(extra, total, low)
    assert limited <= 0.1 * size, (limited, size)
    if w * h <= 17 * 9:
        assert size >= 20 if case == "17x9" else (size == 0 and hit.all())
        return
    assert 0.85 < hit.mean() < 0.95
    sf = R.Surfaces(cam, ar, nm, depth)
    s, beyond, _ = D.slices(cam, sf.lin_depth.astype(np.float64))
    assert (beyond & hit.ravel()).sum() >= 20 and (-sf.lin_depth[hit.ravel()] < cam.near_).sum() >= 20
    assert set(s[hit.ravel() & ~beyond].tolist()) == set(range(17))
    assert size >= 0.1 * w * h
    assert 5 < visible.sum(-1).mean() < 35 and len({tuple(c) for c in visible.reshape(-1, visible.shape[-1])}) > 30
    if case == "100x70_resolution_x2":
        # the lookup's px / 32 names the cluster of another part of the image (its frusta are camera.resolution's): the
        # lists it finds are not the pixel's own, and with lights of this range the brute force is another image
        brute, btotal, _ = D.shade(world, cam, ar, nm, depth, lists=None)
        assert (np.abs(brute - want).max(-1) > REL * btotal + ABS).mean() > 0.01


def _sweep_shade_check(got, want, total, margin, depth, extra, low, what):
    """test_deferred_shading._shade_check with `extra` added to the allowance of the low-roughness group; prints each
    group's pixel count and worst error relative to its allowance."""
    assert (got[..., 3] == 1.0).all(), what
    assert (margin > 1e-4)[depth != 0.0].mean() > 0.99, what
    g = got[..., :3].astype(np.float64)
    finite = np.isfinite(want).all(-1)
    assert (np.isfinite(g).all(-1) == finite).all(), what
    err = np.abs(g - want).max(-1)
    allow = REL * total + ABS + np.where(low, extra, 0.0)
    with np.errstate(all="ignore"):
        ratio = np.where(finite, err / allow, 0.0)
    for name, sel in (("roughness >= 0.05", ~low), ("roughness < 0.05", low)):
        if sel.any():
            print("direct sweep %s %-18s %5d pixels, worst error %.3f of the allowance" % (what, name, sel.sum(), ratio[sel].max()))
    bad = finite & (err > allow)
    assert not bad.any(), "%s: %d pixels off (%d of them roughness >= 0.05), worst %.3g of %.3g" % (
        what, bad.sum(), (bad & ~low).sum(), err[bad].max(), total[bad][np.argmax(err[bad])])


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(DIRECT_CASES))
def test_gpu_direct_sweep_matches_the_reference(gpu_ctx, oracle, case):
    """As test_deferred_shading.test_gpu_shading_matches_the_reference: against the reference over the read-back lists
    and against the brute force.  Only the low-roughness group's allowance gains the conditioning term."""
    world, cam, (ar, nm, depth), low = _direct_design(oracle, case)
    h, w = depth.shape
    gpu_ctx.upload_scene(world)
    gpu_ctx.deferred_shading(cam, ar, nm, depth)
    got = gpu_ctx.read_hdr()
    assert got.shape == (h, w, 4)
    lists = _cluster_check(gpu_ctx.read_light_clusters(), world, cam, w, h)
    want, total, margin = D.shade(world, cam, ar, nm, depth, lists=lists)
    extra = G.shade_conditioning(world, cam, ar, nm, depth, lists)
    limited, size = _conditioning_limited(extra, total, low)
    assert limited <= 0.1 * size, (limited, size)
    _sweep_shade_check(got, want, total, margin, depth, extra, low, case)
    if DIRECT_CASES[case][2] == 1:
        # culling is conservative: the clustered image is the brute force over every light.  (With a resolution of
        # twice the extent the lookup names another part of the image's cluster: see the design's CPU test.)
        brute, btotal, _ = D.shade(world, cam, ar, nm, depth, lists=None)
        every = tuple(np.ones(l.shape, bool) for l in lists)
        _sweep_shade_check(got, brute, btotal, margin, depth, G.shade_conditioning(world, cam, ar, nm, depth, every), low,
                           case + " brute force")
    if w * h <= 17 * 9:
        # every pixel of an image smaller than a tile round (8 tiles) is written
        gpu_ctx.deferred_shading(cam, ar, nm, depth, draw_type=S.DrawType["Position"])
        pos = gpu_ctx.read_hdr()
        wantp = R.Surfaces(cam, ar, nm, depth).pos.reshape(h, w, 3)
        assert (pos[..., 3] == 1.0).all() and np.abs(pos[..., :3] - wantp).max() <= 1e-5 * np.abs(wantp).max()


# ---- the resampling sweep ----

@functools.lru_cache(maxsize=None)
def _band_reference(oracle, extent):
    w, h = BAND_EXTENTS[extent]
    world = _sweep_world(oracle)
    cam = G.sweep_camera(oracle, world, w, h)
    gb, band = G.band_design(cam, w, h)
    frames = {}
    for frame in (1, 2, 3):
        initial = R.initial(world, cam, *gb, frame)
        res = pack(initial[0], initial[1])
        frames[frame] = (initial, res, R.spatial(world, cam, *gb, res, frame, oracle, lookups=True))
    return world, cam, gb, band, frames


@pytest.mark.parametrize("extent", sorted(BAND_EXTENTS))
def test_band_design_decides_and_meets_both_thresholds(oracle, extent):
    """From the reference alone: at least 99 % of the pixels are decided and at least 8 % hold a light in both passes
    of frames 1 - 3 (the GPU check wants 5 %, and at 17 x 9 few neighbour lookups stay inside the image), and
    (100 x 70) each of the eight band pairs is looked up at least 100 times: the pairs 5 and 9 % apart in depth always pass on to
    the normal test, the pair 20 % apart never, the pair 11 % apart only from its farther band (1 - 1 / 1.11 < 0.1 <
    0.11); of the pairs turned against each other, 0.99 and 0.92 are accepted and 0.88 and 0.80 refused."""
    world, cam, (ar, nm, depth), band, frames = _band_reference(oracle, extent)
    for frame, (initial, _, spatial) in frames.items():
        assert (initial[2] >= 1e-4).mean() >= 0.99 and (spatial[2] >= 1e-4).mean() >= 0.99, frame
        # _check_against_reference wants a light in more than 5 % of the reservoirs; the decided ones hold the reference's
        assert (initial[0] >= 0).mean() >= 0.08 and (spatial[0] >= 0).mean() >= 0.08, frame
    assert ar[..., 3].min() >= 0.05
    sf = R.Surfaces(cam, ar, nm, depth)
    lin, b = sf.lin_depth.astype(np.float64), band.ravel()
    p, q, tested = [np.concatenate([frames[f][2][3][k] for f in frames]) for k in range(3)]
    with np.errstate(all="ignore"):
        diff = np.abs(1.0 - lin[q] / lin[p])
        dot = (sf.n[p] * sf.n[q]).sum(-1)
    assert np.abs(diff - 0.1).min() >= 5e-4 and np.abs(dot[tested] - 0.9).min() >= 0.9e-4 * 0.9
    if extent != "100x70":
        return
    for k, step in enumerate(G.DEPTH_STEPS):
        up = (b[p] == 2 * k) & (b[q] == 2 * k + 1)
        down = (b[p] == 2 * k + 1) & (b[q] == 2 * k)
        assert up.sum() >= 100 and down.sum() >= 100, (step, up.sum(), down.sum())
        assert np.abs(diff[up] - (step - 1.0)).max() < 1e-5 and np.abs(diff[down] - (1.0 - 1.0 / step)).max() < 1e-5
        assert tested[up].all() == (step - 1.0 < 0.1) and tested[up].any() == (step - 1.0 < 0.1)
        assert tested[down].all() == (1.0 - 1.0 / step < 0.1) and tested[down].any() == (1.0 - 1.0 / step < 0.1)
    for k, want in enumerate(G.NORMAL_DOTS):
        pair = (((b[p] == 2 * k + 1) & (b[q] == 2 * k + 2)) | ((b[p] == 2 * k + 2) & (b[q] == 2 * k + 1))) & tested
        assert pair.sum() >= 100, (want, pair.sum())
        assert np.abs(dot[pair] - want).max() <= 0.004
        if want == 0.88:  # on both sides of a threshold of 0.88, all below 0.9
            assert (dot[pair] < 0.88).sum() >= 20 and (dot[pair] > 0.88).sum() >= 20


@pytest.mark.gpu
@pytest.mark.parametrize("extent", sorted(BAND_EXTENTS))
def test_gpu_resampling_sweep_matches_the_reference(gpu_ctx, oracle, extent):
    """Both passes for frames 1 - 3 under test_restir_di_resampling's rules; the spatial pass is fed the reference's
    reservoirs.  17 x 9 is narrower than two tiles and has fewer tiles (2) than the 8 the blocks are dealt over."""
    world, cam, (ar, nm, depth), band, frames = _band_reference(oracle, extent)
    gpu_ctx.upload_scene(world)
    lights = R.Lights(world).count
    for frame, (initial, res, spatial) in frames.items():
        got = gpu_ctx.restir_di_resample(S.RESTIR_INITIAL, frame, cam, ar, nm, depth)
        _check_against_reference(got, *initial, lights)
        got = gpu_ctx.restir_di_resample(S.RESTIR_SPATIAL, frame, cam, ar, nm, depth, res)
        _check_against_reference(got, *spatial[:3], lights)


# ---- evalBRDFTimesNoL below roughness 0.05 ----

def test_oracle_brdf_below_roughness_005_matches_float64(oracle):
    """The oracle's evalBRDFTimesNoL against the float64 restatement's arithmetic where max(alpha / 2, 1e-4) switches
    and a2 - 1 rounds to -1: test_oracle_kat.test_brdf_lights_offset's tolerance plus the conditioning of
    trowbridgeReitz's denominator."""
    x = G.low_roughness_brdf_inputs()
    assert len(x) == 20000 and x[:, 12].min() >= 0.001 and x[:, 12].max() <= 0.05
    assert 0.3 < (x[:, 12].astype(np.float64) ** 2 * 0.5 < 1e-4).mean() < 0.4
    want, conditioning = G.brdf_reference(x)
    got = oracle.eval_fn("EVAL_BRDF", x).astype(np.float64)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    allow = 1e-6 + 3e-4 * np.abs(want) + conditioning
    ratio = np.abs(got - want) / allow
    print("oracle evalBRDFTimesNoL below 0.05: worst error %.3f of the allowance, %d of %d values lit" % (
        ratio.max(), (want > 0).sum(), want.size))
    assert (ratio <= 1.0).all(), "%d values off, worst %.3g of the allowance" % ((ratio > 1).sum(), ratio.max())
    assert (want.max(-1) > 0).mean() > 0.5
    assert (conditioning.max(-1) > 3e-4 * np.abs(want).max(-1)).mean() < 0.1


@pytest.mark.gpu
def test_gpu_brdf_below_roughness_005_matches_the_oracle_bitwise(gpu_ctx, oracle):
    x = G.low_roughness_brdf_inputs()
    want = oracle.eval_fn("EVAL_BRDF", x)
    got = gpu_ctx.eval_device_fn(9, x, 14, 3)
    bad = np.argwhere(~same_bits(got, want))
    assert bad.size == 0, "%d mismatches, first at %s: gpu=%r oracle=%r in=%r" % (
        len(bad), bad[0], got[bad[0][0]], want[bad[0][0]], x[bad[0][0]])
