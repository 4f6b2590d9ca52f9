// pt_bc7_encode.hip — gfx950 kernels of the BC7 encoder.
//
//   bc7_encode_level_kernel    one lane per 4 x 4 block of a level in the DeviceTexture tiling: a block is half of an
//                              8 x 4 tile, its four rows are four 16-byte loads (two neighbouring lanes share a tile's
//                              128-byte line), the result one 16-byte store.  No LDS.
//   bc7_encode_blocks_kernel   the same device function over a list of loose blocks, with the squared error of each
//                              (prosper_pt_debug_bc7_encode_blocks: tests)
//
// The rule is the library's own and prosper_amd/bc7.py (encode_blocks) states it in numpy; everything is integer
// arithmetic and this file has to reproduce it bit for bit.  Candidates are evaluated one after another and only the
// best packed block is kept; every loop over a block's texels is unrolled so that the texels, the per-texel errors and
// the packed indices stay in registers (no scratch).
#include "pt_bc7_encode.hpp"

#include "pt_bc7.hpp"
#include "pt_scene.hpp"

namespace ppt
{

namespace
{

constexpr uint32_t kAll = 0xFu, kColour = 0x7u, kAlpha = 0x8u; // channel sets: bit c = channel c of R G B A

__device__ __forceinline__ uint32_t channel(uint32_t texel, uint32_t c) { return (texel >> (8u * c)) & 0xFFu; }

// The corners of the set's bounding box the block's line runs between, into the set's bytes of e0 / e1: the reference
// channel is the first with the largest range; a channel whose covariance with it is negative runs from its maximum
// to its minimum.
template <uint32_t SET> __device__ __forceinline__ void endpoint_line(const uint32_t (&t)[16], uint32_t &e0, uint32_t &e1)
{
    uint32_t lo[4], hi[4], sum[4];
    uint32_t ref = 0, range = 0;
    bool first = true;
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c)
    {
        if (!(SET >> c & 1u)) continue;
        lo[c] = 255u, hi[c] = 0u, sum[c] = 0u;
#pragma unroll
        for (uint32_t i = 0; i < 16u; ++i)
        {
            const uint32_t v = channel(t[i], c);
            lo[c] = v < lo[c] ? v : lo[c];
            hi[c] = v > hi[c] ? v : hi[c];
            sum[c] += v;
        }
        if (first || hi[c] - lo[c] > range)
        {
            ref = c;
            range = hi[c] - lo[c];
        }
        first = false;
    }
    uint32_t refSum = 0, product[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i)
    {
        const uint32_t r = (t[i] >> (8u * ref)) & 0xFFu;
        refSum += r;
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c)
            if (SET >> c & 1u) product[c] += r * channel(t[i], c);
    }
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c)
    {
        if (!(SET >> c & 1u)) continue;
        const bool negative = (int32_t)(16u * product[c]) - (int32_t)(refSum * sum[c]) < 0;
        e0 |= (negative ? hi[c] : lo[c]) << (8u * c);
        e1 |= (negative ? lo[c] : hi[c]) << (8u * c);
    }
}

// the value the decoder expands the nearest BITS-bit code to; a tie goes to the lower code.  The code that shares v's
// top bits is less than one step away, so the nearest is that one or a neighbour.
template <uint32_t BITS> __device__ __forceinline__ uint32_t nearest_code_value(uint32_t v)
{
    if constexpr (BITS == 8u)
        return v;
    else
    {
        const uint32_t q = v >> (8u - BITS), last = (1u << BITS) - 1u;
        auto expand = [](uint32_t code) {
            const uint32_t x = code << (8u - BITS);
            return x | (x >> BITS);
        };
        auto distance = [v](uint32_t x) { return x > v ? x - v : v - x; };
        uint32_t best = expand(q > 0u ? q - 1u : 0u);
        const uint32_t mid = expand(q), up = expand(q < last ? q + 1u : last);
        if (distance(mid) < distance(best)) best = mid;
        if (distance(up) < distance(best)) best = up;
        return best;
    }
}

// an endpoint at the mode's precision, as the decoder dequantises it
template <uint32_t MODE> __device__ __forceinline__ uint32_t quantise(uint32_t e, bool opaque)
{
    if constexpr (MODE == 6u)
    {
        // 7 bits and a p-bit: with p = 0 every odd channel is off by one, with p = 1 every even one; the smaller error
        // wins and a tie goes to p = 0.  An opaque block takes p = 1, so that alpha stays 255.
        const uint32_t odd = (uint32_t)__builtin_popcount(e & 0x01010101u);
        if (!(odd >= 3u || opaque)) return e & 0xFEFEFEFEu;
        uint32_t out = 0;
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c)
        {
            const uint32_t v = channel(e, c);
            out |= ((v & 1u) ? v : (v == 0u ? 1u : v - 1u)) << (8u * c); // the nearest odd value, the lower on a tie
        }
        return out;
    }
    else
    {
        constexpr uint32_t CB = MODE == 5u ? 7u : 5u, AB = MODE == 5u ? 8u : 6u;
        return nearest_code_value<CB>(channel(e, 0)) | (nearest_code_value<CB>(channel(e, 1)) << 8) |
               (nearest_code_value<CB>(channel(e, 2)) << 16) | (nearest_code_value<AB>(channel(e, 3)) << 24);
    }
}

// Per texel the index (lowest on a tie) whose decoded value is nearest over the set's channels; the indices four bits
// apiece in `idx`.  -> the set's squared error over the block
template <uint32_t SET, uint32_t BITS> __device__ __forceinline__ uint32_t assign(const uint32_t (&t)[16], uint32_t e0, uint32_t e1, uint64_t &idx)
{
    uint32_t best[16];
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i) best[i] = 0xFFFFFFFFu;
    idx = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < (1u << BITS); ++k)
    {
        const uint32_t w = bc7_weight(BITS, k);
        uint32_t value[4];
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c)
            if (SET >> c & 1u) value[c] = bc7_interpolate(channel(e0, c), channel(e1, c), w);
#pragma unroll
        for (uint32_t i = 0; i < 16u; ++i)
        {
            uint32_t d = 0;
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c)
                if (SET >> c & 1u)
                {
                    const int32_t x = (int32_t)channel(t[i], c) - (int32_t)value[c];
                    d += (uint32_t)(x * x);
                }
            if (d < best[i])
            {
                best[i] = d;
                idx = (idx & ~(0xFull << (4u * i))) | ((uint64_t)k << (4u * i));
            }
        }
    }
    uint32_t sse = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i) sse += best[i];
    return sse;
}

// Least-squares endpoints of the set for the given indices, into the set's bytes of e0 / e1: with a = 64 - w, b = w the
// model is (a e0 + b e1) / 64; the 2 x 2 normal equations per channel in integers, the quotient rounded as
// floor((2 n + d) / (2 d)) and clamped to 0..255.  A zero determinant keeps the endpoints.
template <uint32_t SET, uint32_t BITS> __device__ __forceinline__ void refine(const uint32_t (&t)[16], uint64_t idx, uint32_t &e0, uint32_t &e1)
{
    uint32_t saa = 0, sab = 0, sbb = 0, sax[4] = {0u, 0u, 0u, 0u}, sbx[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i)
    {
        const uint32_t b = bc7_weight(BITS, (uint32_t)(idx >> (4u * i)) & 0xFu), a = 64u - b;
        saa += a * a;
        sab += a * b;
        sbb += b * b;
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c)
            if (SET >> c & 1u)
            {
                sax[c] += a * channel(t[i], c);
                sbx[c] += b * channel(t[i], c);
            }
    }
    const int64_t det = (int64_t)saa * sbb - (int64_t)sab * sab;
    if (det == 0) return;
    auto solve = [det](int64_t n) -> uint32_t {
        const int64_t rounded = 2 * n + det;
        if (rounded < 0) return 0u;
        const uint64_t q = (uint64_t)rounded / (uint64_t)(2 * det);
        return q > 255u ? 255u : (uint32_t)q;
    };
#pragma unroll
    for (uint32_t c = 0; c < 4u; ++c)
    {
        if (!(SET >> c & 1u)) continue;
        const uint32_t r0 = solve(64 * ((int64_t)sbb * sax[c] - (int64_t)sab * sbx[c]));
        const uint32_t r1 = solve(64 * ((int64_t)saa * sbx[c] - (int64_t)sab * sax[c]));
        e0 = (e0 & ~(0xFFu << (8u * c))) | (r0 << (8u * c));
        e1 = (e1 & ~(0xFFu << (8u * c))) | (r1 << (8u * c));
    }
}

// 128 bits, written least significant first
struct Bc7Writer
{
    uint64_t lo = 0, hi = 0;
    uint32_t pos = 0;
    __device__ __forceinline__ void put(uint64_t v, uint32_t n)
    {
        v &= (1ull << n) - 1ull;
        if (pos < 64u)
        {
            lo |= v << pos;
            if (pos + n > 64u) hi |= v >> (64u - pos);
        }
        else
            hi |= v << (pos - 64u);
        pos += n;
    }
    // sixteen BITS-bit indices; the anchor's top bit is implied 0
    template <uint32_t BITS> __device__ __forceinline__ void indices(uint64_t idx)
    {
        put(idx & 0xFu, BITS - 1u);
#pragma unroll
        for (uint32_t i = 1; i < 16u; ++i) put((idx >> (4u * i)) & 0xFu, BITS);
    }
};

// An anchor index with its top bit set: the set's endpoints (p-bits with them) swap and its indices complement.
template <uint32_t SET, uint32_t BITS> __device__ __forceinline__ void fix_anchor(uint32_t &e0, uint32_t &e1, uint64_t &idx)
{
    if (!((idx >> (BITS - 1u)) & 1u)) return;
    constexpr uint32_t bytes = (SET & 1u ? 0xFFu : 0u) | (SET & 2u ? 0xFF00u : 0u) | (SET & 4u ? 0xFF0000u : 0u) | (SET & 8u ? 0xFF000000u : 0u);
    const uint32_t x = (e0 ^ e1) & bytes;
    e0 ^= x;
    e1 ^= x;
    constexpr uint64_t last = (1ull << BITS) - 1ull;
    idx = last * 0x1111111111111111ull - idx; // every nibble: last - index
}

// One candidate - MODE with index selection SEL - against the best block so far.
template <uint32_t MODE, uint32_t SEL>
__device__ __forceinline__ void try_candidate(const uint32_t (&t)[16], bool opaque, uint32_t &bestSse, uint64_t &bestLo, uint64_t &bestHi)
{
    // index bits of the colour set (mode 6: of the one set) and of the alpha set
    constexpr uint32_t CB = MODE == 6u ? 4u : (MODE == 4u && SEL == 1u ? 3u : 2u), AB = MODE == 4u && SEL == 0u ? 3u : 2u;
    uint32_t e0 = 0, e1 = 0;
    if constexpr (MODE == 6u)
        endpoint_line<kAll>(t, e0, e1);
    else
    {
        endpoint_line<kColour>(t, e0, e1);
        endpoint_line<kAlpha>(t, e0, e1);
    }
    uint32_t keptE0 = 0, keptE1 = 0, sse = 0xFFFFFFFFu;
    uint64_t keptC = 0, keptA = 0;
#pragma unroll 1
    for (uint32_t pass = 0; pass < 2u; ++pass)
    {
        if (pass == 1u)
        {
            // one refinement from the first pass's indices; it stays only where strictly better
            e0 = keptE0, e1 = keptE1;
            if constexpr (MODE == 6u)
                refine<kAll, CB>(t, keptC, e0, e1);
            else
            {
                refine<kColour, CB>(t, keptC, e0, e1);
                refine<kAlpha, AB>(t, keptA, e0, e1);
            }
        }
        e0 = quantise<MODE>(e0, opaque);
        e1 = quantise<MODE>(e1, opaque);
        uint64_t idxC, idxA = 0;
        uint32_t s;
        if constexpr (MODE == 6u)
            s = assign<kAll, CB>(t, e0, e1, idxC);
        else
            s = assign<kColour, CB>(t, e0, e1, idxC) + assign<kAlpha, AB>(t, e0, e1, idxA);
        if (s < sse)
        {
            sse = s;
            keptE0 = e0, keptE1 = e1, keptC = idxC, keptA = idxA;
        }
    }
    if (sse >= bestSse) return;
    bestSse = sse;
    Bc7Writer out;
    out.put(1u << MODE, MODE + 1u);
    if constexpr (MODE == 6u)
    {
        fix_anchor<kAll, CB>(keptE0, keptE1, keptC);
#pragma unroll
        for (uint32_t c = 0; c < 4u; ++c)
        {
            out.put(channel(keptE0, c) >> 1, 7u);
            out.put(channel(keptE1, c) >> 1, 7u);
        }
        out.put(keptE0 & 1u, 1u);
        out.put(keptE1 & 1u, 1u);
        out.indices<CB>(keptC);
    }
    else
    {
        constexpr uint32_t colourBits = MODE == 5u ? 7u : 5u, alphaBits = MODE == 5u ? 8u : 6u;
        fix_anchor<kColour, CB>(keptE0, keptE1, keptC);
        fix_anchor<kAlpha, AB>(keptE0, keptE1, keptA);
        out.put(0u, 2u); // rotation
        if constexpr (MODE == 4u) out.put(SEL, 1u);
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c)
        {
            out.put(channel(keptE0, c) >> (8u - colourBits), colourBits);
            out.put(channel(keptE1, c) >> (8u - colourBits), colourBits);
        }
        out.put(channel(keptE0, 3) >> (8u - alphaBits), alphaBits);
        out.put(channel(keptE1, 3) >> (8u - alphaBits), alphaBits);
        // the primary (2-bit) set first; with the selection bit it is alpha's
        if constexpr (SEL == 1u)
        {
            out.indices<AB>(keptA);
            out.indices<CB>(keptC);
        }
        else
        {
            out.indices<CB>(keptC);
            out.indices<AB>(keptA);
        }
    }
    bestLo = out.lo;
    bestHi = out.hi;
}

// texel[i] = R | G << 8 | B << 16 | A << 24 of pixel i, row-major in the block -> the block's four words and its squared
// error.  Ties between candidates resolve in the order 6, 5, 4 (index selection 0 before 1).
__device__ __forceinline__ uint4 bc7_encode_block(const uint32_t (&t)[16], uint32_t modeMask, uint32_t &sse)
{
    if ((modeMask & kBc7EncodeModes) == 0u) modeMask = kBc7EncodeModes;
    uint32_t alpha = 0xFF000000u;
#pragma unroll
    for (uint32_t i = 0; i < 16u; ++i) alpha &= t[i];
    const bool opaque = alpha == 0xFF000000u;
    uint64_t lo = 0, hi = 0;
    sse = 0xFFFFFFFFu;
    if (modeMask & (1u << 6)) try_candidate<6, 0>(t, opaque, sse, lo, hi);
    if (modeMask & (1u << 5)) try_candidate<5, 0>(t, opaque, sse, lo, hi);
    if (modeMask & (1u << 4))
    {
        try_candidate<4, 0>(t, opaque, sse, lo, hi);
        try_candidate<4, 1>(t, opaque, sse, lo, hi);
    }
    return uint4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
}

} // namespace

__global__ __launch_bounds__(256) void bc7_encode_level_kernel(
    const uint32_t *__restrict__ tiled, uint32_t blocksX, uint32_t blockCount, uint32_t tilesPerRow, uint32_t modeMask, uint4 *__restrict__ blocks)
{
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= blockCount) return;
    const uint32_t bx = id % blocksX, by = id / blocksX;
    // the block is the left or the right half of tile (bx / 2, by): row r at words 8 r + 4 (bx & 1) of the tile
    const uint4 *rows = reinterpret_cast<const uint4 *>(tiled + ((size_t)by * tilesPerRow + (bx >> 1)) * (kTexTileW * kTexTileH)) + (bx & 1u);
    uint32_t t[16];
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r)
    {
        const uint4 q = rows[2u * r];
        t[4u * r] = q.x, t[4u * r + 1u] = q.y, t[4u * r + 2u] = q.z, t[4u * r + 3u] = q.w;
    }
    uint32_t sse;
    blocks[id] = bc7_encode_block(t, modeMask, sse);
}

__global__ __launch_bounds__(256) void bc7_encode_blocks_kernel(
    const uint4 *__restrict__ texels, uint32_t n, uint32_t modeMask, uint4 *__restrict__ blocks, uint32_t *__restrict__ sse)
{
    const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n) return;
    uint32_t t[16];
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r)
    {
        const uint4 q = texels[(size_t)id * 4u + r];
        t[4u * r] = q.x, t[4u * r + 1u] = q.y, t[4u * r + 2u] = q.z, t[4u * r + 3u] = q.w;
    }
    uint32_t error;
    blocks[id] = bc7_encode_block(t, modeMask, error);
    sse[id] = error;
}

void launch_bc7_encode_level(const void *tiled, uint32_t width, uint32_t height, uint32_t modeMask, void *blocks, hipStream_t stream)
{
    const uint32_t blocksX = width / 4u, blockCount = blocksX * (height / 4u);
    if (blockCount == 0) return;
    hipLaunchKernelGGL(
        bc7_encode_level_kernel, dim3((blockCount + 255u) / 256u), dim3(256), 0, stream, static_cast<const uint32_t *>(tiled), blocksX,
        blockCount, (width + kTexTileW - 1u) / kTexTileW, modeMask, static_cast<uint4 *>(blocks));
}

void launch_bc7_encode_blocks(const uint32_t *texels, uint32_t n, uint32_t modeMask, uint32_t *blocks, uint32_t *sse, hipStream_t stream)
{
    if (n == 0) return;
    hipLaunchKernelGGL(
        bc7_encode_blocks_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, reinterpret_cast<const uint4 *>(texels), n, modeMask,
        reinterpret_cast<uint4 *>(blocks), sse);
}

} // namespace ppt
