"""The rasteriser's kernels (pt_raster.hip) over the sweep's scenes of tests/raster_scenes.py: the record
loop of raster_large_kernel past its first 64 records, the queue append with a wave's every lane queuing, clipped polygons of
4 to 7 vertices and fans that skip a triangle, the kMask instantiations with queued records, meshes whose triangles fall into
every size class, and raster_scan_blocks_kernel's carry.  tests/test_raster_sweep_cpu.py shows that the scenes reach those
paths.  Everything is compared with the restatement bit for bit: ids, depth bits, counters, fragment lists."""
import ctypes as C

import numpy as np
import pytest

import culling_reference as CR
import raster_reference as R
import raster_scenes as RS
import raster_transparent_reference as RT
from prosper_amd import structs as S
from test_raster_gbuffer import assert_is_the_restatement, counts_of, draw_unculled
from test_raster_sweep_cpu import FLOOR_EXTENTS, QUEUE_SIZES, SCAN_EXTENTS, SOUP_EXTENTS, SOUP_SEEDS, camera
from test_raster_transparent import check_lists, opaque_frame

pytestmark = pytest.mark.gpu


def is_the_restatement_twice(ctx, world, extent):
    """uploads and draws the unculled list: the restatement's image and counters; the same list again without a clear leaves
    every byte as it is and counts the same"""
    ctx.upload_scene(world)
    cam = camera(extent)
    ids, depth = draw_unculled(ctx, cam)
    want = assert_is_the_restatement(ctx, world, cam, ids, depth)
    ctx.raster_meshlets(cam, S.DRAW_LIST_GENERATED, clear=False)
    ids2, depth2 = ctx.read_raster_visibility(*extent)
    assert ids2.tobytes() == ids.tobytes() and depth2.tobytes() == depth.tobytes()
    info = ctx.raster_info()
    assert counts_of(info.draw[1]) == want["counts"] and counts_of(info.draw[0]) == want["counts"]
    return want, ids


@pytest.mark.parametrize("n,grouped", [(n, False) for n in QUEUE_SIZES] + [(n, True) for n in QUEUE_SIZES[-3:]])
def test_queue_worlds(gpu_ctx, n, grouped):
    want, _ = is_the_restatement_twice(gpu_ctx, RS.queue_world(n, grouped), RS.SWEEP_EXTENT)
    assert want["counts"]["queued"] == n


def test_clip_zoo(gpu_ctx):
    want, _ = is_the_restatement_twice(gpu_ctx, RS.clip_zoo_world(), RS.SWEEP_EXTENT)
    assert want["counts"]["clipped"] >= 12


@pytest.mark.parametrize("extent", SOUP_EXTENTS, ids=lambda e: "%dx%d" % e)
@pytest.mark.parametrize("seed", SOUP_SEEDS)
def test_soups(gpu_ctx, seed, extent):
    is_the_restatement_twice(gpu_ctx, RS.soup_world(seed)[0], extent)


@pytest.mark.parametrize("extent", FLOOR_EXTENTS, ids=lambda e: "%dx%d" % e)
def test_graded_floor_is_watertight_on_the_device(gpu_ctx, extent):
    want, ids = is_the_restatement_twice(gpu_ctx, RS.graded_floor_world(), extent)
    covered = int((ids[..., 0] != R.NO_ID).sum())
    assert gpu_ctx.raster_info().draw[0].fragments == covered > 0  # every pixel of the floor exactly once


@pytest.mark.parametrize("scene", ["queue", "soup"])
def test_mask_variants(gpu_ctx, scene):
    """the <true, false> instantiations of both kernels: more than 64 records, and small triangles walked by the wave"""
    world = RS.mask_variant(RS.queue_world(129, True) if scene == "queue" else RS.soup_world(SOUP_SEEDS[0])[0])
    want, ids = is_the_restatement_twice(gpu_ctx, world, RS.SWEEP_EXTENT)
    assert want["counts"]["queued"] > (64 if scene == "queue" else 20) and (ids[..., 0] != R.NO_ID).any()


def test_a_shuffled_list_draws_the_same_image(gpu_ctx):
    world = RS.soup_world(SOUP_SEEDS[1])[0]
    gpu_ctx.upload_scene(world)
    cam = camera(SOUP_EXTENTS[-1])
    ids, depth = draw_unculled(gpu_ctx, cam)
    pairs, _ = gpu_ctx.read_draw_list(S.DRAW_LIST_GENERATED)  # (synchronises: the generator has written the list)
    list_ptr, _, capacity = gpu_ctx.draw_list_device_ptr(S.DRAW_LIST_GENERATED)
    shuffled = np.ascontiguousarray(pairs[np.random.default_rng(9).permutation(len(pairs))])
    assert len(pairs) <= capacity and not np.array_equal(shuffled, pairs)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(list_ptr + 4, shuffled.ctypes.data, shuffled.nbytes, 1) == 0
    gpu_ctx.raster_meshlets(cam, S.DRAW_LIST_GENERATED, clear=True)
    ids2, depth2 = gpu_ctx.read_raster_visibility(*SOUP_EXTENTS[-1])
    assert ids2.tobytes() == ids.tobytes() and depth2.tobytes() == depth.tobytes()  # the draw order decides nothing
    got, _ = gpu_ctx.read_draw_list(S.DRAW_LIST_GENERATED)
    assert np.array_equal(got, shuffled)


def lists_are_the_restatement(ctx, monkeypatch, world, extent, what):
    """the opaque frame, the transparent pass, and its per-pixel lists against the restatement -> (counts, fragments)"""
    ctx.upload_scene(world)
    cam = camera(extent)
    _, stored, _ = opaque_frame(ctx, cam)
    ctx.raster_forward_transparent(cam)
    counts, fragments = ctx.read_raster_fragments()
    sure, maybe = RT.lists(world, cam, CR.generate(world, CR.MODE_TRANSPARENT), stored)
    assert not any(m for row in maybe for m in row), "no BLEND material here carries a texture: nothing is undecided"
    monkeypatch.setattr(RT, "lists", lambda *a, **k: (sure, maybe))  # (check_lists asks for the same lists: made once)
    check_lists(world, cam, stored, counts, fragments, what)
    assert counts.sum() == len(fragments) == ctx.raster_transparent_info().fragments
    return counts, fragments


@pytest.mark.parametrize("scene", ["queue", "soup"])
def test_layer_modes(gpu_ctx, monkeypatch, scene):
    world = RS.blend_variant(RS.queue_world(129, True) if scene == "queue" else RS.soup_world(SOUP_SEEDS[0])[0])
    counts, _ = lists_are_the_restatement(gpu_ctx, monkeypatch, world, RS.SWEEP_EXTENT, "blend %s" % scene)
    assert counts.max() >= 4


@pytest.mark.parametrize("extent", SCAN_EXTENTS, ids=lambda e: "%dx%d" % e)
def test_the_scan_carries_past_64_blocks(gpu_ctx, monkeypatch, extent):
    counts, _ = lists_are_the_restatement(gpu_ctx, monkeypatch, RS.scan_world(), extent, "scan %dx%d" % extent)
    assert set(np.unique(counts).tolist()) == set(range(5))
