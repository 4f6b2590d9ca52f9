"""Texture mip chains and sample_texture_lod on the GPU, bit for bit against tests/texture_lod_reference.py:
generated chains of linear and base-colour textures, supplied RGBA8 and BC7 chains, chains replaced by
prosper_pt_update_textures, and prosper_pt_debug_sample_texture_lod over seeded and hand-placed records."""
import numpy as np
import pytest

import texture_lod_reference as R
from prosper_amd import bc7, capi, scenes, structs as S
from prosper_amd.world import Bc7Texture, TextureChain, World

pytestmark = pytest.mark.gpu
F = np.float32

SIZES = [(64, 64), (16, 4), (36, 20), (5, 3)]  # (width, height): square, thin, odd parents (9 x 5 -> 4 x 2), one level
WRAPS = [S.WRAP_REPEAT, S.WRAP_MIRRORED_REPEAT, S.WRAP_CLAMP_TO_EDGE]


class MipScene:
    """One quad per material; what each texture slot holds, for the comparisons."""

    def __init__(self):
        rng = np.random.default_rng(0x4D495053)
        w = World()
        self.world = w
        self.linear, self.base = {}, {}  # size -> (texture index, texels)

        def rand(size):
            return rng.integers(0, 256, (size[1], size[0], 4), dtype=np.uint8)

        def quad(material):
            q = scenes._add(w, scenes.quad((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)), material)
            w.add_instance(w.add_model([(q, material)]))

        # (mag, min, wrapS, wrapT): both filters under every wrap mode (S and T differ), and the two mixed pairs
        self.samplers = []
        for flt in (S.FILTER_NEAREST, S.FILTER_LINEAR):
            for k, ws in enumerate(WRAPS):
                self.samplers.append((flt, flt, ws, WRAPS[(k + 1) % 3]))
        self.samplers += [(S.FILTER_NEAREST, S.FILTER_LINEAR, S.WRAP_REPEAT, S.WRAP_REPEAT),
                          (S.FILTER_LINEAR, S.FILTER_NEAREST, S.WRAP_REPEAT, S.WRAP_REPEAT)]
        self.sampler_index = [w.add_sampler(*s) for s in self.samplers]
        for size in SIZES:
            lin, base = rand(size), rand(size)
            self.linear[size] = (w.add_texture(lin), lin)
            self.base[size] = (w.add_texture(base), base)
            # no normal texture: not packable, both keep their level 0
            quad(w.add_material(base_tex=(self.base[size][0], 0), mr_tex=(self.linear[size][0], 0)))
        # a packed material: its three textures lose their own level 0 and keep the levels above
        self.packed = [(w.add_texture(t), t) for t in (rand((64, 64)), rand((64, 64)), rand((64, 64)))]
        quad(w.add_material(base_tex=(self.packed[0][0], 0), mr_tex=(self.packed[1][0], 0), normal_tex=(self.packed[2][0], 0)))
        # supplied chains: a whole RGBA8 one (random levels, nothing like a reduction), the first two levels of a 64 x 64
        # one, and a BC7 16 x 16 one (16, 8, 4: 16 + 4 + 1 blocks)
        self.supplied = [rand(R.level_extent(36, 20, l)) for l in range(4)]
        self.supplied_index = w.add_texture_chain(self.supplied)
        self.partial = [rand((64, 64)), rand((32, 32))]
        self.partial_index = w.add_texture_chain(self.partial)
        self.blocks = rng.integers(0, 256, (21, 16), dtype=np.uint8)
        self.bc7_index = w.add_texture_bc7(self.blocks, 16, 16, levels=3)
        quad(w.add_material(base_tex=(self.supplied_index, 0), mr_tex=(self.partial_index, 0)))
        quad(w.add_material(mr_tex=(self.bc7_index, 0)))


@pytest.fixture(scope="module")
def mip_scene():
    return MipScene()


@pytest.fixture(scope="module")
def mip_ctx(mip_scene):
    ctx = capi.Context(device=0, flags=S.CREATE_TEXTURE_MIPS)
    ctx.set_debug(widePacks=1)
    ctx.upload_scene(mip_scene.world)
    yield ctx
    ctx.close()


def read_chain(ctx, texture, first=0):
    info = ctx.texture_mips_info(texture)
    return [ctx.read_texture_level(texture, l, info.width, info.height) for l in range(first, info.levelCount)], info


def assert_same(got, want):
    assert len(got) == len(want)
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, l
        assert (g == w).all(), "level %d: %d texels differ" % (l, (g != w).any(axis=-1).sum())


@pytest.mark.parametrize("size", SIZES)
def test_generated_chains_are_the_restatement_bit_for_bit(mip_ctx, mip_scene, size):
    for (index, texels), srgb in ((mip_scene.linear[size], False), (mip_scene.base[size], True)):
        got, info = read_chain(mip_ctx, index)
        assert (info.width, info.height) == size and info.levelCount == R.mip_level_count(*size) and info.srgbAveraged == int(srgb)
        assert_same(got, R.generate_chain(texels, srgb))
    if size == (36, 20):
        assert [g.shape[:2] for g in got] == [(20, 36), (10, 18), (5, 9), (2, 4)]
    if size == (5, 3):
        assert len(got) == 1


def test_a_packed_materials_textures_keep_their_chains_beside_the_pack(mip_ctx, mip_scene):
    stats = mip_ctx.scene_stats()
    assert stats.variantFlags & S.VARIANT_TEXTURE_PACKS
    for k, (index, texels) in enumerate(mip_scene.packed):
        with pytest.raises(capi.ProsperPtError) as e:
            mip_ctx.read_texture_level(index, 0, 64, 64)
        assert e.value.code == -6
        got, info = read_chain(mip_ctx, index, first=1)
        assert info.levelCount == 5 and info.srgbAveraged == int(k == 0)
        assert_same(got, R.generate_chain(texels, k == 0)[1:])


def test_supplied_chains_come_back_as_given(mip_ctx, mip_scene):
    got, info = read_chain(mip_ctx, mip_scene.supplied_index)
    assert info.levelCount == 4 and info.srgbAveraged == 0  # (a base-colour texture, but nothing was averaged)
    assert_same(got, mip_scene.supplied)
    got, info = read_chain(mip_ctx, mip_scene.partial_index)
    assert info.levelCount == 2
    assert_same(got, mip_scene.partial)
    got, info = read_chain(mip_ctx, mip_scene.bc7_index)
    assert info.levelCount == 3
    blob, want, offset = mip_scene.blocks.tobytes(), [], 0
    for l in range(3):
        n = 16 >> l
        want.append(bc7.decode_image(blob[offset:offset + (n // 4) ** 2 * 16], n, n))
        offset += (n // 4) ** 2 * 16
    assert_same(got, want)


def test_the_mip_texel_bytes_are_reported_and_levels_out_of_range_refused(mip_ctx, mip_scene):
    w = mip_scene.world
    total = 0
    for i, t in enumerate(w.textures):
        if isinstance(t, TextureChain):
            width, height, levels = t.width, t.height, len(t.levels)
        elif isinstance(t, Bc7Texture):
            width, height, levels = t.width, t.height, t.levels
        else:
            width, height, levels = t.shape[1], t.shape[0], R.mip_level_count(t.shape[1], t.shape[0])
        total += sum(4 * a * b for a, b in (R.level_extent(width, height, l) for l in range(1, levels)))
        assert mip_ctx.texture_mips_info(i).levelCount == levels
    assert mip_ctx.texture_mips_info(1).mipTexelBytes == total
    index = mip_scene.linear[(16, 4)][0]
    with pytest.raises(capi.ProsperPtError) as e:
        mip_ctx.read_texture_level(index, 3, 16, 4)
    assert e.value.code == -1
    with pytest.raises(capi.ProsperPtError):
        mip_ctx.read_texture_level(len(w.textures), 0, 1, 1)


def test_a_context_without_the_flag_keeps_no_chains(gpu_ctx, mip_scene):
    gpu_ctx.upload_scene(mip_scene.world)
    with pytest.raises(capi.ProsperPtError) as e:
        gpu_ctx.texture_mips_info(1)
    assert e.value.code == -6
    with pytest.raises(capi.ProsperPtError) as e:
        gpu_ctx.debug_sample_texture_lod(1, 0, np.zeros((1, 6), F))
    assert e.value.code == -6
    index, texels = mip_scene.linear[(36, 20)]
    assert (gpu_ctx.read_texture_level(index, 0, 36, 20) == texels).all()
    with pytest.raises(capi.ProsperPtError):
        gpu_ctx.read_texture_level(index, 1, 36, 20)
    # mipLevelCount is not read: level 0 of the supplied chain is the texture
    assert (gpu_ctx.read_texture_level(mip_scene.supplied_index, 0, 36, 20) == mip_scene.supplied[0]).all()


def records(rng, size, levels, n):
    """Seeded records: uv over several periods on both sides of 0, every derivative of either sign with a magnitude
    between an eighth of a texel and four times the last level's texel."""
    rec = np.zeros((n, 6), F)
    rec[:, :2] = rng.uniform(-2.0, 3.0, (n, 2))
    mag = np.exp2(rng.uniform(-3.0, levels + 1.0, (n, 4))) * rng.choice([-1.0, 1.0], (n, 4))
    rec[:, 2:] = mag / np.array([size[0], size[1], size[0], size[1]], np.float64)
    rec[rng.random(n) < 0.2, 3:5] = 0.0  # axis-aligned footprints
    return rec


def hand_placed(size):
    w, h = size
    inf, nan = np.inf, np.nan
    rows = [
        (0.3, 0.7, 0.25 / w, 0, 0, 0.5 / h),     # lambda < 0
        (0.3, 0.7, 1.0 / w, 0, 0, 1.0 / h),      # rho = 1 (where 1 / extent is exact): lambda = 0 + bias
        (0.3, 0.7, 2.0 / w, 0, 0, 1.0 / h),      # integer lambda: 1
        (0.3, 0.7, 0, 4.0 / h, 1.0 / w, 0),      # 2
        (0.3, 0.7, 3.0 / w, 0, 0, 0.1 / h),      # between 1 and 2
        (-1.6, 2.2, 1024.0 / w, 0, 0, 0),        # far beyond the last level
        (0.3, 0.7, 0, 0, 0, 0),                  # rho = 0
        (0.3, 0.7, inf, 0, 0, 0), (0.3, 0.7, 0, -inf, 0, 0), (0.3, 0.7, 0, 0, nan, 0), (0.3, 0.7, 1.0 / w, 0, 0, nan),
        (0.3, 0.7, 3e38, 3e38, 0, 0),            # rho overflows
        (0.0, 1.0, 1.5 / w, 0, 0, 1.5 / h), (-0.0, -1.0, 1.5 / w, 0, 0, 1.5 / h),  # texel borders
        (0.999999, 1e-7, 2.5 / w, 0, 0, 2.5 / h),
    ]
    return np.array(rows, F)


@pytest.mark.parametrize("size", [(64, 64), (36, 20)])
@pytest.mark.parametrize("sampler", range(8))
def test_sample_texture_lod_is_the_restatement_bit_for_bit(mip_ctx, mip_scene, size, sampler):
    index, texels = mip_scene.linear[size]
    chain = R.generate_chain(texels, False)
    rng = np.random.default_rng(1000 * sampler + size[0])
    rec = np.concatenate([hand_placed(size), records(rng, size, len(chain), 3000)])
    desc = mip_scene.samplers[sampler]
    zero = rec.copy()
    zero[:, 2:] = 0.0
    lod0 = mip_ctx.debug_sample_texture_lod(index, mip_scene.sampler_index[sampler], zero)  # the LOD-0 sample itself
    assert np.isneginf(lod0[:, 4]).all()
    seen = set()
    for bias in (0.0, -1.0, 1.0):
        got = mip_ctx.debug_sample_texture_lod(index, mip_scene.sampler_index[sampler], rec, bias)
        rgba, lam = R.sample_texture_lod(chain, desc, rec[:, :2], rec[:, 2:], bias)
        assert (got[:, 4].view(np.uint32) == lam.view(np.uint32)).all(), bias
        bad = (got[:, :4].view(np.uint32) != rgba.view(np.uint32)).any(axis=1)
        assert not bad.any(), "bias %g: %d records differ, first %s" % (bias, bad.sum(), rec[np.nonzero(bad)[0][:1]])
        # lambda <= 0 is the existing LOD-0 sample, exactly
        low = ~(lam > 0)
        assert (got[low, :4].view(np.uint32) == lod0[low, :4].view(np.uint32)).all()
        last = len(chain) - 1
        seen |= {"below" if (lam < 0).any() else "", "zero" if (lam == 0).any() else "", "last" if (lam > last).any() else "",
                 "whole" if ((lam > 0) & (lam < last) & (lam == np.floor(lam))).any() else "",
                 "inside" if ((lam > 0) & (lam < last) & (lam != np.floor(lam))).any() else ""}
        # the non-finite derivatives, the overflow and the far-away record sample the last level alone
        for k in (5, 7, 8, 9, 10, 11):
            assert got[k, 4] == np.inf or got[k, 4] > last
            want = R.sample_level(chain[last], desc[1], desc[2], desc[3], rec[k:k + 1, :2])
            assert (got[k:k + 1, :4].view(np.uint32) == want.view(np.uint32)).all()
    # (1 / 36 and 1 / 20 are not floats: whether rho lands on a power of two there is the rounding's business)
    assert {"below", "last", "inside"} <= seen and (size != (64, 64) or {"zero", "whole"} <= seen)


def test_update_textures_replaces_a_chain(mip_scene):
    ctx = capi.Context(device=0, flags=S.CREATE_TEXTURE_MIPS)
    try:
        ctx.upload_scene(mip_scene.world)
        before = ctx.texture_mips_info(1).mipTexelBytes
        rng = np.random.default_rng(77)
        lin_index = mip_scene.linear[(16, 4)][0]   # 3 levels, 16 x 4
        base_index = mip_scene.base[(36, 20)][0]   # 4 levels, 36 x 20
        assert lin_index + 1 != base_index and mip_scene.base[(16, 4)][0] == lin_index + 1
        new_lin = rng.integers(0, 256, (8, 32, 4), dtype=np.uint8)     # 32 x 8: 4 levels
        new_base16 = rng.integers(0, 256, (4, 16, 4), dtype=np.uint8)  # stays 16 x 4, a base colour
        ctx.update_textures([new_lin, new_base16], lin_index)
        got, info = read_chain(ctx, lin_index)
        assert (info.width, info.height, info.levelCount, info.srgbAveraged) == (32, 8, 4, 0)
        assert_same(got, R.generate_chain(new_lin, False))
        got, info = read_chain(ctx, lin_index + 1)
        assert (info.levelCount, info.srgbAveraged) == (3, 1)
        assert_same(got, R.generate_chain(new_base16, True))
        grown = 4 * (16 * 4 + 8 * 2 + 4 * 1) - 4 * (8 * 2 + 4 * 1)
        assert ctx.texture_mips_info(1).mipTexelBytes == before + grown
        # a supplied chain in place of a generated one, and the sampler sees the new chain
        chain = [rng.integers(0, 256, (max(20 >> l, 1), max(36 >> l, 1), 4), dtype=np.uint8) for l in range(3)]
        ctx.update_textures([TextureChain(chain)], base_index)
        got, info = read_chain(ctx, base_index)
        assert (info.levelCount, info.srgbAveraged) == (3, 0)
        assert_same(got, chain)
        rec = records(np.random.default_rng(5), (36, 20), 3, 500)
        got = ctx.debug_sample_texture_lod(base_index, 0, rec, 0.0)
        rgba, lam = R.sample_texture_lod(chain, (1, 1, 0, 0), rec[:, :2], rec[:, 2:], 0.0)
        assert (got[:, 4].view(np.uint32) == lam.view(np.uint32)).all()
        assert (got[:, :4].view(np.uint32) == rgba.view(np.uint32)).all()
        # a count above prosper's is refused and changes nothing
        with pytest.raises(capi.ProsperPtError) as e:
            ctx.update_textures([TextureChain(R.generate_chain(new_lin, False, levels=5))], lin_index)
        assert e.value.code == -5
        assert ctx.texture_mips_info(lin_index).levelCount == 4
    finally:
        ctx.close()
