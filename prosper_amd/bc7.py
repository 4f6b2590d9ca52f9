"""BC7 (BPTC UNORM) block decoder and encoder, numpy; the decoder bit-exact per the format definition (Khronos Data Format Specification,
"BPTC compressed texture image formats"; the same rules D3D11's BC7_UNORM and VK_FORMAT_BC7_UNORM_BLOCK decode by).

Why it is here: prosper does not sample the PNG texels of a glTF - it compresses every texture whose
mip chain divides by 4 to BC7 with a third-party encoder and caches the result as `prosper_cache/<name>.dds`
(src/scene/Texture.cpp:213-296, 377-415); the GPU then decodes those blocks in hardware.  Texel parity with prosper
on real assets therefore means reading that cache and decoding it exactly; the encoder itself (lossy heuristics of
the ISPC texture compressor) is not part of the path.  Where no cache exists yet the library writes one with an encoder
of its own rule: `encode_blocks` below states that rule, the HIP kernel reproduces it.

Pinned against an independent implementation: tests/test_bc7.py decodes random blocks of all eight modes (and the
reserved one) with Pillow's "bcn" decoder and compares every byte; the partition / anchor tables below were
recovered from that decoder by tests/golden/make_bc7_tables.py (the reference holds neither tables nor test data).
"""
import numpy as np

# subset of each of the 16 pixels (row-major) for the 64 two-subset and 64 three-subset partitions
PARTITION2 = (
    '0011001100110011', '0001000100010001', '0111011101110111', '0001001100110111',
    '0000000100010011', '0011011101111111', '0001001101111111', '0000000100110111',
    '0000000000010011', '0011011111111111', '0000000101111111', '0000000000010111',
    '0001011111111111', '0000000011111111', '0000111111111111', '0000000000001111',
    '0000100011101111', '0111000100000000', '0000000010001110', '0111001100010000',
    '0011000100000000', '0000100011001110', '0000000010001100', '0111001100110001',
    '0011000100010000', '0000100010001100', '0110011001100110', '0011011001101100',
    '0001011111101000', '0000111111110000', '0111000110001110', '0011100110011100',
    '0101010101010101', '0000111100001111', '0101101001011010', '0011001111001100',
    '0011110000111100', '0101010110101010', '0110100101101001', '0101101010100101',
    '0111001111001110', '0001001111001000', '0011001001001100', '0011101111011100',
    '0110100110010110', '0011110011000011', '0110011010011001', '0000011001100000',
    '0100111001000000', '0010011100100000', '0000001001110010', '0000010011100100',
    '0110110010010011', '0011011011001001', '0110001110011100', '0011100111000110',
    '0110110011001001', '0110001100111001', '0111111010000001', '0001100011100111',
    '0000111100110011', '0011001111110000', '0010001011101110', '0100010001110111',
)
PARTITION3 = (
    '0011001102212222', '0001001122112221', '0000200122112211', '0222002200110111',
    '0000000011221122', '0011001100220022', '0022002211111111', '0011001122112211',
    '0000000011112222', '0000111111112222', '0000111122222222', '0012001200120012',
    '0112011201120112', '0122012201220122', '0011011211221222', '0011200122002220',
    '0001001101121122', '0111001120012200', '0000112211221122', '0022002200221111',
    '0111011102220222', '0001000122212221', '0000001101220122', '0000110022102210',
    '0122012200110000', '0012001211222222', '0110122112210110', '0000011012211221',
    '0022110211020022', '0110011020022222', '0011012201220011', '0000200022112221',
    '0000000211221222', '0222002200120011', '0011001200220222', '0120012001200120',
    '0000111122220000', '0120120120120120', '0120201212010120', '0011220011220011',
    '0011112222000011', '0101010122222222', '0000000021212121', '0022112200221122',
    '0022001100220011', '0220122102201221', '0101222222220101', '0000212121212121',
    '0101010101012222', '0222011102220111', '0002111200021112', '0000211221122112',
    '0222011101110222', '0002111211120002', '0110011001102222', '0000000021122112',
    '0110011022222222', '0022001100110022', '0022112211220022', '0000000000002112',
    '0002000100020001', '0222122202221222', '0101222222222222', '0111201122012220',
)
# anchor pixel (its index drops the top bit) of subset 1 of a two-subset partition, of subsets 1 and 2 of a
# three-subset one; the anchor of subset 0 is always pixel 0
ANCHOR2 = (
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
    15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
    15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6,
    6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15,
)
ANCHOR3A = (
    3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3,
    3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15,
    8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15,
    3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3,
)
ANCHOR3B = (
    15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8,
    15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8,
    15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8,
    15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8,
)

# mode: subsets, partition bits, rotation bits, index-selection bits, colour bits, alpha bits,
#       per-endpoint p-bits, shared (per-subset) p-bits, index bits, secondary index bits
MODES = (
    (3, 4, 0, 0, 4, 0, 1, 0, 3, 0),
    (2, 6, 0, 0, 6, 0, 0, 1, 3, 0),
    (3, 6, 0, 0, 5, 0, 0, 0, 2, 0),
    (2, 6, 0, 0, 7, 0, 1, 0, 2, 0),
    (1, 0, 2, 1, 5, 6, 0, 0, 2, 3),
    (1, 0, 2, 0, 7, 8, 0, 0, 2, 2),
    (1, 0, 0, 0, 7, 7, 1, 0, 4, 0),
    (2, 6, 0, 0, 5, 5, 1, 0, 2, 0),
)
WEIGHTS = {2: (0, 21, 43, 64), 3: (0, 9, 18, 27, 37, 46, 55, 64),
           4: (0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64)}

_P2 = np.array([[int(c) for c in row] for row in PARTITION2], np.int64)
_P3 = np.array([[int(c) for c in row] for row in PARTITION3], np.int64)
_A2 = np.array(ANCHOR2, np.int64)
_A3A = np.array(ANCHOR3A, np.int64)
_A3B = np.array(ANCHOR3B, np.int64)


def _field(bits, pos, n):
    """bits [N, 128] (bit k of the block in column k) -> the n-bit little-endian field at fixed position pos."""
    w = (1 << np.arange(n, dtype=np.int64))
    return bits[:, pos:pos + n].astype(np.int64) @ w


def _indices(bits, start, width, anchors):
    """16 indices of `width` bits starting at bit `start`, pixel order; pixels listed in anchors [N, k] store
    width - 1 bits.  -> [N, 16]"""
    n = bits.shape[0]
    pixel = np.arange(16, dtype=np.int64)[None, :]
    is_anchor = (pixel[:, :, None] == anchors[:, None, :]).any(axis=2)            # [N, 16]
    before = (anchors[:, None, :] < pixel[:, :, None]).sum(axis=2)                 # anchors strictly before the pixel
    pos = start + pixel * width - before                                           # [N, 16]
    out = np.zeros((n, 16), np.int64)
    for k in range(width):
        have = ~is_anchor | (k < width - 1)
        at = np.minimum(pos + k, 127)
        out |= (np.take_along_axis(bits, at, axis=1).astype(np.int64) & have) << k
    return out


def _interpolate(e0, e1, idx, width):
    w = np.array(WEIGHTS[width], np.int64)[idx]
    return ((64 - w) * e0 + w * e1 + 32) >> 6


def _decode_mode(bits, mode):
    ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2 = MODES[mode]
    n = bits.shape[0]
    pos = mode + 1
    partition = _field(bits, pos, pb) if pb else np.zeros(n, np.int64)
    pos += pb
    rotation = _field(bits, pos, rb) if rb else np.zeros(n, np.int64)
    pos += rb
    index_selection = _field(bits, pos, isb) if isb else np.zeros(n, np.int64)
    pos += isb
    # endpoints: channel-major, then endpoint (subset 0 e0, subset 0 e1, subset 1 e0, ...)
    ends = np.zeros((n, 2 * ns, 4), np.int64)
    for channel in range(3):
        for e in range(2 * ns):
            ends[:, e, channel] = _field(bits, pos, cb)
            pos += cb
    if ab:
        for e in range(2 * ns):
            ends[:, e, 3] = _field(bits, pos, ab)
            pos += ab
    channels = 4 if ab else 3
    cbits = np.array([cb, cb, cb, ab], np.int64)
    if epb:
        for e in range(2 * ns):
            p = _field(bits, pos, 1)
            pos += 1
            ends[:, e, :channels] = (ends[:, e, :channels] << 1) | p[:, None]
        cbits = cbits + 1
    if spb:
        for s in range(ns):
            p = _field(bits, pos, 1)
            pos += 1
            for e in (2 * s, 2 * s + 1):
                ends[:, e, :channels] = (ends[:, e, :channels] << 1) | p[:, None]
        cbits = cbits + 1
    for channel in range(channels):
        b = int(cbits[channel])
        v = ends[:, :, channel] << (8 - b)
        ends[:, :, channel] = v | (v >> b)
    if not ab:
        ends[:, :, 3] = 255

    if ns == 1:
        subset = np.zeros((n, 16), np.int64)
        anchors = np.zeros((n, 1), np.int64)
    elif ns == 2:
        subset = _P2[partition]
        anchors = np.stack([np.zeros(n, np.int64), _A2[partition]], axis=1)
    else:
        subset = _P3[partition]
        anchors = np.stack([np.zeros(n, np.int64), _A3A[partition], _A3B[partition]], axis=1)
    idx = _indices(bits, pos, ib, anchors)
    pos += 16 * ib - ns
    e0 = np.take_along_axis(ends, (2 * subset)[:, :, None].repeat(4, axis=2), axis=1)       # [N, 16, 4]
    e1 = np.take_along_axis(ends, (2 * subset + 1)[:, :, None].repeat(4, axis=2), axis=1)
    out = np.empty((n, 16, 4), np.int64)
    if ib2:
        # two index sets (modes 4, 5): colour from the primary and alpha from the secondary set, swapped when the
        # index-selection bit of mode 4 is set
        idx2 = _indices(bits, pos, ib2, anchors)
        swap = (index_selection == 1)[:, None]
        colour_a = _interpolate(e0[:, :, :3], e1[:, :, :3], idx[:, :, None], ib)
        colour_b = _interpolate(e0[:, :, :3], e1[:, :, :3], idx2[:, :, None], ib2)
        alpha_a = _interpolate(e0[:, :, 3], e1[:, :, 3], idx, ib)
        alpha_b = _interpolate(e0[:, :, 3], e1[:, :, 3], idx2, ib2)
        out[:, :, :3] = np.where(swap[:, :, None], colour_b, colour_a)
        out[:, :, 3] = np.where(swap, alpha_a, alpha_b)
    else:
        out[:] = _interpolate(e0, e1, idx[:, :, None], ib)
    if rb:
        for r, channel in ((1, 0), (2, 1), (3, 2)):
            m = rotation == r
            if m.any():
                a = out[m, :, 3].copy()
                out[m, :, 3] = out[m, :, channel]
                out[m, :, channel] = a
    return out.astype(np.uint8)


def decode_blocks(blocks):
    """uint8 [N, 16] BC7 blocks -> uint8 [N, 16, 4] RGBA texels (pixel order row-major inside the 4x4 block).
    A block whose mode byte is 0 (reserved) decodes to transparent black, as the format specifies."""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 16)
    n = blocks.shape[0]
    out = np.zeros((n, 16, 4), np.uint8)
    first = blocks[:, 0].astype(np.int64)
    low = first & -first                                  # lowest set bit of the mode byte
    mode = np.where(first == 0, 8, np.log2(np.maximum(low, 1)).astype(np.int64))
    for m in range(8):
        sel = np.nonzero(mode == m)[0]
        for c0 in range(0, len(sel), 1 << 16):            # bounded working set
            chunk = sel[c0:c0 + (1 << 16)]
            bits = np.unpackbits(blocks[chunk], axis=1, bitorder="little")
            out[chunk] = _decode_mode(bits, m)
    return out


def decode_image(data, width, height):
    """BC7 payload of one mip level (blocks row-major, 16 B each) -> uint8 [height, width, 4]."""
    if width % 4 or height % 4:
        raise ValueError("BC7 levels are whole 4x4 blocks (the reference falls back to RGBA8 otherwise)")
    bx, by = width // 4, height // 4
    blocks = np.frombuffer(data, np.uint8, count=bx * by * 16).reshape(-1, 16)
    texels = decode_blocks(blocks).reshape(by, bx, 4, 4, 4)
    return np.ascontiguousarray(texels.transpose(0, 2, 1, 3, 4).reshape(height, width, 4))


# ---- the encoder ----
# prosper compresses with a third-party encoder whose source is not part of its tree, so no byte-for-byte pin against
# it exists.  The rule below is this library's own: integer arithmetic only, stated here in numpy, and the HIP kernel
# (csrc/pt_bc7_encode.hip) has to reproduce it bit for bit (tests/test_bc7_encode.py).  Candidates are the three
# single-subset modes with alpha - 6, 5 and 4, the latter with both values of its index-selection bit - with rotation 0.
ENCODE_CANDIDATES = ((6, 0), (5, 0), (4, 0), (4, 1))   # (mode, index selection), in tie order
_COLOUR, _ALPHA, _ALL = (0, 1, 2), (3,), (0, 1, 2, 3)
_CHUNK = 1 << 14


def _index_sets(mode, selection):
    """(channels, index bits) of every index set of a candidate, the colour set first."""
    if mode == 6:
        return ((_ALL, 4),)
    if mode == 5:
        return ((_COLOUR, 2), (_ALPHA, 2))
    return ((_COLOUR, 3), (_ALPHA, 2)) if selection else ((_COLOUR, 2), (_ALPHA, 3))


def _expand(code, bits):
    """The decoder's bit replication of a `bits`-bit endpoint code to 8 bits."""
    v = code << (8 - bits)
    return v | (v >> bits)


def _nearest(values):
    """[256] table: of the ascending 8-bit `values`, the one nearest to v; a tie goes to the lower one."""
    values = np.asarray(values, np.int64)
    return values[np.argmin(np.abs(values[None, :] - np.arange(256, dtype=np.int64)[:, None]), axis=1)]


_NEAREST = {bits: _nearest(_expand(np.arange(1 << bits, dtype=np.int64), bits)) for bits in (5, 6, 7, 8)}
_NEAREST_PARITY = (_nearest(np.arange(0, 256, 2)), _nearest(np.arange(1, 256, 2)))


def _endpoint_line(x):
    """x [N, 16, C] -> (e0, e1) [N, C]: the corners of the channels' bounding box that the block's line runs between.
    The reference channel is the first with the largest range; a channel whose covariance with it is negative runs
    from its maximum to its minimum."""
    lo, hi = x.min(axis=1), x.max(axis=1)
    ref = np.argmax(hi - lo, axis=1)
    xr = np.take_along_axis(x, ref[:, None, None], axis=2)                       # [N, 16, 1]
    cov = 16 * (xr * x).sum(axis=1) - xr.sum(axis=1) * x.sum(axis=1)             # [N, C]
    return np.where(cov < 0, hi, lo), np.where(cov < 0, lo, hi)


def _quantise(mode, e, opaque):
    """8-bit endpoint e [N, 4] -> the value the decoder dequantises the nearest code of the mode's precision to."""
    if mode == 6:
        # 7 bits and a p-bit: both p tried, the channels take the nearest value of that parity; the smaller squared
        # error wins, p = 0 on a tie; an opaque block takes p = 1, so that alpha stays 255
        q = [table[e] for table in _NEAREST_PARITY]
        err = [((v - e) ** 2).sum(axis=1) for v in q]
        p = (err[1] < err[0]) | opaque
        return np.where(p[:, None], q[1], q[0])
    colour, alpha = (7, 8) if mode == 5 else (5, 6)
    return np.concatenate([_NEAREST[colour][e[:, :3]], _NEAREST[alpha][e[:, 3:]]], axis=1)


def _assign(x, e0, e1, bits):
    """Per texel the index (lowest on a tie) whose decoded value is nearest over the set's channels.
    x [N, 16, C], e0 / e1 [N, C] -> (indices [N, 16], squared error [N, 16])"""
    best = idx = None
    for k, w in enumerate(WEIGHTS[bits]):
        value = ((64 - w) * e0 + w * e1 + 32) >> 6
        d = ((x - value[:, None, :]) ** 2).sum(axis=2)
        if best is None:
            best, idx = d, np.zeros(d.shape, np.int64)
        else:
            better = d < best
            best = np.where(better, d, best)
            idx = np.where(better, k, idx)
    return idx, best


def _refine(x, idx, bits, e0, e1):
    """Least-squares endpoints for the given indices: with a = 64 - w, b = w the model is (a e0 + b e1) / 64, whose
    normal equations are solved per channel in integers; the quotient is rounded as floor((2 n + d) / (2 d)) and
    clamped to 0..255.  A zero determinant (every texel on one index) keeps the endpoints."""
    w = np.array(WEIGHTS[bits], np.int64)[idx]
    a, b = 64 - w, w
    saa, sab, sbb = (a * a).sum(axis=1), (a * b).sum(axis=1), (b * b).sum(axis=1)
    det = saa * sbb - sab * sab
    sax, sbx = (a[:, :, None] * x).sum(axis=1), (b[:, :, None] * x).sum(axis=1)
    n0 = 64 * (sbb[:, None] * sax - sab[:, None] * sbx)
    n1 = 64 * (saa[:, None] * sbx - sab[:, None] * sax)
    d = np.maximum(det, 1)[:, None]
    keep = (det == 0)[:, None]
    r0 = np.where(keep, e0, np.clip((2 * n0 + d) // (2 * d), 0, 255))
    r1 = np.where(keep, e1, np.clip((2 * n1 + d) // (2 * d), 0, 255))
    return r0, r1


def _candidate(x, opaque, mode, selection):
    """One candidate over x [N, 16, 4] -> (e0, e1 [N, 4] dequantised, [indices [N, 16] per set], sse [N])."""
    sets = _index_sets(mode, selection)

    def fit(e0, e1):
        e0, e1 = _quantise(mode, e0, opaque), _quantise(mode, e1, opaque)
        indices, sse = [], 0
        for channels, bits in sets:
            c = list(channels)
            idx, err = _assign(x[:, :, c], e0[:, c], e1[:, c], bits)
            indices.append(idx)
            sse = sse + err.sum(axis=1)
        return e0, e1, indices, sse

    e0, e1 = np.empty((x.shape[0], 4), np.int64), np.empty((x.shape[0], 4), np.int64)
    for channels, _ in sets:
        c = list(channels)
        e0[:, c], e1[:, c] = _endpoint_line(x[:, :, c])
    e0, e1, indices, sse = fit(e0, e1)
    r0, r1 = e0.copy(), e1.copy()
    for (channels, bits), idx in zip(sets, indices):
        c = list(channels)
        r0[:, c], r1[:, c] = _refine(x[:, :, c], idx, bits, e0[:, c], e1[:, c])
    r0, r1, refined, refined_sse = fit(r0, r1)
    use = refined_sse < sse                                    # the refinement stays only where strictly better
    e0, e1 = np.where(use[:, None], r0, e0), np.where(use[:, None], r1, e1)
    indices = [np.where(use[:, None], r, i) for r, i in zip(refined, indices)]
    return e0, e1, indices, np.where(use, refined_sse, sse)


class _Bits:
    """128 bits per block, written least significant first at fixed positions."""

    def __init__(self, n):
        self.lo, self.hi, self.pos = np.zeros(n, np.uint64), np.zeros(n, np.uint64), 0

    def put(self, value, n):
        v = np.asarray(value).astype(np.uint64) & np.uint64((1 << n) - 1)
        if self.pos < 64:
            self.lo |= v << np.uint64(self.pos)
            if self.pos + n > 64:
                self.hi |= v >> np.uint64(64 - self.pos)
        else:
            self.hi |= v << np.uint64(self.pos - 64)
        self.pos += n

    def indices(self, idx, bits):
        self.put(idx[:, 0], bits - 1)                         # the anchor's top bit is implied 0
        for i in range(1, 16):
            self.put(idx[:, i], bits)


def _pack(mode, selection, e0, e1, indices):
    sets = _index_sets(mode, selection)
    e0, e1, indices = e0.copy(), e1.copy(), list(indices)
    for s, (channels, bits) in enumerate(sets):
        # an anchor index with its top bit set: the set's endpoints (p-bits with them) swap, its indices complement
        swap = (indices[s][:, 0] >> (bits - 1)) == 1
        c = list(channels)
        e0[:, c], e1[:, c] = np.where(swap[:, None], e1[:, c], e0[:, c]), np.where(swap[:, None], e0[:, c], e1[:, c])
        indices[s] = np.where(swap[:, None], (1 << bits) - 1 - indices[s], indices[s])
    out = _Bits(e0.shape[0])
    out.put(1 << mode, mode + 1)
    if mode == 6:
        for c in range(4):
            out.put(e0[:, c] >> 1, 7)
            out.put(e1[:, c] >> 1, 7)
        out.put(e0[:, 0] & 1, 1)
        out.put(e1[:, 0] & 1, 1)
        out.indices(indices[0], 4)
    else:
        colour, alpha = (7, 8) if mode == 5 else (5, 6)
        out.put(0, 2)                                          # rotation
        if mode == 4:
            out.put(selection, 1)
        for c in range(3):
            out.put(e0[:, c] >> (8 - colour), colour)
            out.put(e1[:, c] >> (8 - colour), colour)
        out.put(e0[:, 3] >> (8 - alpha), alpha)
        out.put(e1[:, 3] >> (8 - alpha), alpha)
        # the primary (2-bit) set first; with the selection bit it is alpha's
        first, second = (1, 0) if selection else (0, 1)
        out.indices(indices[first], sets[first][1])
        out.indices(indices[second], sets[second][1])
    assert out.pos == 128
    return np.stack([out.lo, out.hi], axis=1).astype("<u8").view(np.uint8).reshape(-1, 16)


def encode_blocks(texels, mode_mask=0):
    """uint8 [N, 16, 4] RGBA texels (row-major inside the 4x4 block) -> (blocks uint8 [N, 16], sse int64 [N] of the
    decoded block against the source over all four channels, mode int64 [N]).  mode_mask: bits 4, 5 and 6 enable
    that mode; 0 enables all three.  The block takes the candidate with the least SSE, ties in the order 6, 5, 4
    (index selection 0 before 1)."""
    texels = np.ascontiguousarray(texels, np.uint8).reshape(-1, 16, 4)
    n = texels.shape[0]
    mode_mask = int(mode_mask) & 0x70 or 0x70
    blocks, sse, mode = np.zeros((n, 16), np.uint8), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for c0 in range(0, n, _CHUNK):
        x = texels[c0:c0 + _CHUNK].astype(np.int64)
        opaque = (x[:, :, 3] == 255).all(axis=1)
        best = None
        for m, selection in ENCODE_CANDIDATES:
            if not mode_mask >> m & 1:
                continue
            e0, e1, indices, err = _candidate(x, opaque, m, selection)
            packed = _pack(m, selection, e0, e1, indices)
            if best is None:
                best = [packed, err, np.full(len(x), m, np.int64)]
            else:
                better = err < best[1]
                best = [np.where(better[:, None], packed, best[0]), np.where(better, err, best[1]), np.where(better, m, best[2])]
        blocks[c0:c0 + _CHUNK], sse[c0:c0 + _CHUNK], mode[c0:c0 + _CHUNK] = best
    return blocks, sse, mode


def image_blocks(rgba):
    """uint8 [height, width, 4] -> uint8 [(height / 4) * (width / 4), 16, 4]: the image's 4x4 blocks, row-major."""
    rgba = np.ascontiguousarray(rgba, np.uint8)
    height, width = rgba.shape[:2]
    if width % 4 or height % 4 or rgba.shape[2] != 4:
        raise ValueError("BC7 levels are whole 4x4 blocks of RGBA8 texels")
    return np.ascontiguousarray(rgba.reshape(height // 4, 4, width // 4, 4, 4).transpose(0, 2, 1, 3, 4)).reshape(-1, 16, 4)


def encode_image(rgba, mode_mask=0):
    """uint8 [height, width, 4] -> the BC7 payload of the level (bytes; blocks row-major, 16 B each)."""
    return encode_blocks(image_blocks(rgba), mode_mask)[0].tobytes()
