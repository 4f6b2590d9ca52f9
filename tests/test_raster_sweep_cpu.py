"""The sweep's scenes (tests/raster_scenes.py) through the restatement alone: every scene reaches the path of the kernels it
was made for, so that tests/test_raster_sweep.py is not vacuous, and the properties it relies on hold for the restatement by
itself.  Every condition is computed from raster_reference and raster_transparent_reference only."""
import functools

import numpy as np
import pytest

import culling_reference as CR
import culling_scenes as CS
import raster_reference as R
import raster_scenes as RS
import raster_transparent_reference as RT
from prosper_amd import meshlets as M

F = np.float32
I = np.int64
TILE, SCAN_BLOCK = 32, 1024  # pt_raster.hpp's kRasterTile and kRasterScanBlock
QUEUE_SIZES = (63, 64, 65, 129, 200)
SOUP_SEEDS = (16, 17, 22)
SOUP_EXTENTS = ((33, 17), (96, 80), (130, 70))
FLOOR_EXTENTS = ((96, 80), (130, 70))
SCAN_EXTENTS = ((260, 253), (364, 363))  # 65 and 130 blocks: raster_scan_blocks_kernel carries once and twice


def camera(extent):
    return CS.camera_at(width=extent[0], height=extent[1])


def census(world, cam):
    """What rasterise does with every triangle of the unculled opaque list, decided by raster_reference's own functions
    -> [dict(id=(drawInstance, meshlet, triangle), kind, polygon=its clipped size, skipped / drawn = fan triangles, box)]
    kind: back, zero, outside, small, medium, queued (unclipped), clipped, nothing_left"""
    view = R.View(cam)
    f = world.freeze()
    dis = CR.draw_instances_of(world)
    m2w = CR.transforms_of(world)
    out = []
    for di, mi in CR.generate(world, CR.MODE_OPAQUE).tolist():
        inst, mesh, _ = dis[di]
        md, info = world.metadatas[mesh], world.mesh_infos[mesh]
        built = M.read_meshlets(f["geometry_buffers"][md.bufferIndex], md, info)
        vo, to, vc, tc = (int(v) for v in built["meshlets"][mi])
        clip = R.to_clip(view, m2w[inst], world.mesh_geometry(mesh)[0][built["vertices"][vo:vo + vc].astype(I)])
        X, Y, _, ok = R.snap(view, clip)
        fast = R.is_fast(clip, ok)
        outcode = ~(R.plane_distances(view, clip) >= 0)
        for t, v in enumerate(built["triangles"][to:to + 3 * tc].reshape(-1, 3).astype(I).tolist()):
            row = dict(id=(di, mi, t), polygon=0, skipped=0, drawn=0, box=None)
            if fast[v].all():
                a2 = R.area2(X[v], Y[v])
                bx = R.box(X[v], Y[v], view.width, view.height)
                if a2 >= 0:
                    row["kind"] = "zero" if a2 == 0 else "back"
                elif bx[0] > bx[2] or bx[1] > bx[3]:
                    row["kind"] = "outside"
                else:
                    bw, bh = bx[2] - bx[0] + 1, bx[3] - bx[1] + 1
                    row["kind"] = "small" if bw * bh <= R.SMALL_PIXELS else "medium" if max(bw, bh) <= R.MEDIUM_SIDE else "queued"
                    row["box"] = bx
            elif outcode[v].all(axis=0).any():
                row["kind"] = "outside"
            else:
                poly = R.clip_polygon(view, clip[v])
                PX, PY, _, pok = R.snap(view, poly) if len(poly) else (None, None, None, np.zeros(1, bool))
                if not len(poly) or not pok.all():
                    row["kind"] = "nothing_left"
                else:
                    areas = [R.area2(PX[[0, k, k + 1]], PY[[0, k, k + 1]]) for k in range(1, len(poly) - 1)]
                    row.update(kind="clipped", polygon=len(poly), skipped=sum(a >= 0 for a in areas), drawn=sum(a < 0 for a in areas),
                               box=(max((int(PX.min()) + 127) >> 8, 0), max((int(PY.min()) + 127) >> 8, 0),
                                    min((int(PX.max()) - 128) >> 8, view.width - 1), min((int(PY.max()) - 128) >> 8, view.height - 1)))
            out.append(row)
    return out


def kinds(rows):
    out = {}
    for r in rows:
        out[r["kind"]] = out.get(r["kind"], 0) + 1
    return out


def drawn(world, cam):
    """-> (counts, ids [h, w, 3], covered bool [h, w]) of the unculled opaque list in the restatement"""
    out = R.rasterise(world, cam, CR.generate(world, CR.MODE_OPAQUE))
    ids, _ = R.decode(world, out["keys"])
    return out["counts"], ids, ids[..., 0] != R.NO_ID


def winners(ids, covered):
    return {tuple(v) for v in ids[covered].tolist()}


# ---- the queue ----

@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("n", QUEUE_SIZES)
def test_queue_world_queues_every_triangle(n, grouped):
    world, cam = RS.queue_world(n, grouped), camera(RS.SWEEP_EXTENT)
    counts, ids, covered = drawn(world, cam)
    rows = census(world, cam)
    k = kinds(rows)
    print("queue_world(%d, %s): %s, %s, %d winners" % (n, grouped, counts, k, len(winners(ids, covered))))
    assert counts["triangles"] == n and counts["queued"] == n
    assert counts["clipped"] >= n // 4 and k.get("clipped", 0) == counts["clipped"]
    assert k.get("queued", 0) >= n // 4
    meshlets = sum(info.meshletCount for info in world.mesh_infos)
    assert meshlets == (-(-n // M.MAX_TRIANGLES) if grouped else n)
    # many different triangles win pixels, from every third of the order the queue is filled in
    order = {r["id"]: i for i, r in enumerate(rows)}
    won = sorted(order[w] for w in winners(ids, covered))
    assert len(won) >= min(20, n // 3)
    assert all(any(third * n <= 3 * i < (third + 1) * n for i in won) for third in range(3))
    # every tile of the image is reached by a queued triangle
    tiles = np.zeros((-(-cam.resolution[1] // TILE), -(-cam.resolution[0] // TILE)), bool)
    for r in rows:
        if r["box"] is not None and r["box"][0] <= r["box"][2] and r["box"][1] <= r["box"][3]:
            x0, y0, x1, y1 = r["box"]
            tiles[y0 // TILE:y1 // TILE + 1, x0 // TILE:x1 // TILE + 1] = True
    assert tiles.shape == (3, 3) and tiles.all()


# ---- the clipper ----

def test_clip_zoo_has_every_polygon_size_and_skipped_fan_triangles():
    world, cam = RS.clip_zoo_world(), camera(RS.SWEEP_EXTENT)
    rows = census(world, cam)
    sizes = {}
    for r in rows:
        assert r["kind"] == "clipped" and r["drawn"] >= 1
        sizes[r["polygon"]] = sizes.get(r["polygon"], 0) + 1
    skipping = [r for r in rows if r["skipped"]]
    print("clip_zoo_world: polygon sizes %s, %d triangles skip a fan triangle" % (sorted(sizes.items()), len(skipping)))
    assert all(sizes.get(s, 0) >= 3 for s in (4, 5, 6, 7))
    assert len(skipping) >= 3
    counts, ids, covered = drawn(world, cam)
    assert counts["clipped"] == counts["queued"] == len(rows)
    assert len({w for w in winners(ids, covered)} & {r["id"] for r in skipping}) >= 1  # what is left of such a fan is drawn


# ---- the soup ----

@functools.lru_cache(maxsize=None)
def soup_at(seed, extent):
    world, names = RS.soup_world(seed)
    cam = camera(extent)
    return (world, names, cam) + drawn(world, cam)


@pytest.mark.parametrize("seed", SOUP_SEEDS)
def test_soup_world_has_every_class(seed):
    world, names, cam, counts, ids, covered = soup_at(seed, SOUP_EXTENTS[-1])
    k = kinds(census(world, cam))
    won = winners(ids, covered)
    print("soup_world(%d) at %dx%d: %s, %s, %d winners" % ((seed,) + SOUP_EXTENTS[-1] + (counts, k, len(won))))
    assert 300 <= counts["triangles"] <= 600
    assert k.get("small", 0) >= 50 and k.get("medium", 0) >= 30 and k.get("queued", 0) >= 10 and k.get("clipped", 0) >= 20
    assert k.get("back", 0) >= 20 and k.get("zero", 0) >= 3 and k.get("outside", 0) + k.get("nothing_left", 0) >= 10
    assert (k.get("back", 0), k.get("zero", 0), k.get("clipped", 0)) == (counts["culledBackface"], counts["culledZeroArea"], counts["clipped"])
    assert len(won) >= 30
    # equal depths across draw instances: the later instance never wins, the earlier one does
    by_instance = {}
    for di, mi, t in won:
        by_instance.setdefault(di, set()).add((mi, t))
    assert names["duplicate"] not in by_instance and len(by_instance[names["plain"]]) >= 5
    info = [world.mesh_infos[mesh] for _, mesh, _ in CR.draw_instances_of(world)]
    assert {world.metadatas[mesh].usesShortIndices for _, mesh, _ in CR.draw_instances_of(world)} == {0, 1}
    assert max(i.meshletCount for i in info) > 1


@pytest.mark.parametrize("extent", SOUP_EXTENTS[:2], ids=lambda e: "%dx%d" % e)
def test_soup_world_draws_something_at_the_smaller_extents(extent):
    for seed in SOUP_SEEDS:
        world, names, cam, counts, ids, covered = soup_at(seed, extent)
        assert counts["fragments"] >= covered.sum() > 0.2 * covered.size and counts["clipped"] >= 10


# ---- the floor ----

@pytest.mark.parametrize("extent", FLOOR_EXTENTS, ids=lambda e: "%dx%d" % e)
def test_graded_floor_is_watertight_and_has_every_class(extent):
    world, cam = RS.graded_floor_world(), camera(extent)
    counts, ids, covered = drawn(world, cam)
    rows = census(world, cam)
    k = kinds(rows)
    print("graded_floor_world at %dx%d: %s, %s, %d pixels covered" % (extent + (counts, k, covered.sum())))
    assert counts["culledBackface"] == 0 and counts["culledZeroArea"] == 0
    assert all(k.get(kind, 0) >= 10 for kind in ("small", "medium", "queued", "clipped"))
    assert counts["fragments"] == covered.sum() > 0  # no pixel is hit twice, and none of the floor's is missed
    kind_of = {r["id"]: r["kind"] for r in rows}
    owner = np.full(covered.shape, "", dtype=object)
    for y, x in zip(*np.nonzero(covered)):
        owner[y, x] = kind_of[tuple(ids[y, x])]
    assert any({"clipped", "queued", "medium"} <= set(row) for row in owner), "no image row crosses three classes"
    # the floor's image has no hole: every covered row is covered from its first pixel of the floor to its last
    for row in covered:
        at = np.nonzero(row)[0]
        assert len(at) == 0 or row[at[0]:at[-1] + 1].all()


# ---- the layer modes ----

@pytest.mark.parametrize("extent", SCAN_EXTENTS, ids=lambda e: "%dx%d" % e)
def test_scan_world_fills_the_scan_s_last_blocks(extent):
    world, cam = RS.scan_world(), camera(extent)
    sure, maybe = RT.lists(world, cam, CR.generate(world, CR.MODE_TRANSPARENT))
    assert not any(m for row in maybe for m in row)
    counts = np.array([[len(keys) for keys in row] for row in sure])
    blocks = -(-counts.size // SCAN_BLOCK)
    print("scan_world at %dx%d: %d fragments, %d blocks, pixels per count %s" % (extent + (counts.sum(), blocks, np.bincount(counts.ravel()).tolist())))
    assert blocks == (65 if extent == SCAN_EXTENTS[0] else 130)
    assert set(np.unique(counts).tolist()) == set(range(5))  # 0 to the number of BLEND triangles
    last = np.nonzero(counts.ravel())[0].max() // SCAN_BLOCK
    assert last >= (64 if extent == SCAN_EXTENTS[0] else 128) and last == blocks - 1
    per_block = np.add.reduceat(counts.ravel(), np.arange(0, counts.size, SCAN_BLOCK))
    assert (per_block[:64] > 0).all() and len(set(per_block.tolist())) > blocks // 2  # a lost carry moves real offsets
    # no two neighbouring pixels hold the same keys: a fragment in another pixel's slot is seen
    for y in range(counts.shape[0]):
        for x in range(counts.shape[1]):
            if sure[y][x]:
                assert (x + 1 == counts.shape[1] or sure[y][x] != sure[y][x + 1]) and (y + 1 == counts.shape[0] or sure[y][x] != sure[y + 1][x])


@pytest.mark.parametrize("scene", ["queue", "soup"])
def test_blend_variants_have_deep_pixels_and_queue_records(scene):
    world = RS.blend_variant(RS.queue_world(129, True) if scene == "queue" else RS.soup_world(SOUP_SEEDS[0])[0])
    cam = camera(RS.SWEEP_EXTENT)
    pairs = CR.generate(world, CR.MODE_TRANSPARENT)
    sure, maybe = RT.lists(world, cam, pairs)
    assert not any(m for row in maybe for m in row)  # no BLEND material carries a texture
    counts = np.array([[len(keys) for keys in row] for row in sure])
    # the records the layer modes queue are the visibility pass's of the same geometry
    opaque = RS.queue_world(129, True) if scene == "queue" else RS.soup_world(SOUP_SEEDS[0])[0]
    queued = R.rasterise(opaque, cam, CR.generate(opaque, CR.MODE_OPAQUE))["counts"]["queued"]
    print("blend %s: %d fragments, deepest pixel %d, %d queue records" % (scene, counts.sum(), counts.max(), queued))
    assert queued > (128 if scene == "queue" else 20) and counts.max() >= 4


def test_mask_variants_keep_and_discard():
    for world in (RS.mask_variant(RS.queue_world(129, True)), RS.mask_variant(RS.soup_world(SOUP_SEEDS[0])[0])):
        cam = camera(RS.SWEEP_EXTENT)
        counts, ids, covered = drawn(world, cam)
        dis = CR.draw_instances_of(world)
        kept = {di for di, (_, _, mat) in enumerate(dis) if world.materials[mat].baseColorFactor.w >= 0.5}
        assert 0 < len(kept) < len(dis)
        assert covered.any() and {int(d) for d in np.unique(ids[covered][:, 0])} <= kept
        assert counts["queued"] > (64 if len(dis) == 2 else 20)
