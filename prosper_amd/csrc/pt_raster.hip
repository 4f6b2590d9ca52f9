// pt_raster.hip — gfx950 kernels of the compute rasteriser over the meshlet draw lists.
//
//   raster_meshlets_kernel  one WAVE per draw-list entry, launched over the list's capacity (the count is the list's first
//                           word; waves past it leave, so the kernel has no block barrier).  A lane per meshlet vertex
//                           takes it to clip space and snaps it; a lane per triangle (two rounds for up to 124) fetches its
//                           three vertices from their lanes, sets up, culls and sorts it by its box of pixel centres:
//                             small    the lane walks its own box
//                             medium   compacted by ballot; the whole wave walks the box as 8 x 8 pixel blocks
//                             large    and every triangle the clipper has to see: one 8-byte record appended to a queue
//                                      through one atomic per wave
//   raster_large_kernel     a fixed grid of 32 x 32 pixel tiles, one wave each; every wave reads the queue's count, sets the
//                           records up 64 at a time (a lane per record: its vertices again, the clipper - Sutherland-Hodgman
//                           in float32 over a polygon in the lane's slice of LDS -, the box against the tile) and walks the
//                           part of each record that reaches its tile; the fan's triangles take the common rule.
//   raster_depth_kernel     key -> depth, for the pyramid between the culling phases
//   raster_layers_*_kernel  the two kernels above instantiated for the transparent pass's per-pixel lists:
//                           a fragment that is a layer candidate is counted (kFill false) or its key stored (kFill true)
//   raster_scan_*_kernel    the exclusive scan of the per-pixel counts between the two: a wave per 1024 counters, the wave's
//                           scan by DPP row shifts and row broadcasts
//
// A fragment is one 64-bit atomicMax on (depth bits, ~(ordinal * 128 + triangle)): the greatest depth wins (reverse Z),
// among equal depths the lowest ordinal, whatever order the waves ran in.
#include "pt_raster.hpp"

#include <type_traits>

#include "pt_math.hpp"
#include "pt_raster_surface.hpp"

namespace ppt
{

namespace
{

#define PPT_RS __device__ __forceinline__

// The size classes (scripts/build_variant.sh can set others; DESIGN.md f18 has what was measured).  They decide who walks
// a box, never a bit of the image; tests/raster_reference.py restates them for the `queued` count.
#ifndef PPT_RASTER_SMALL_PIXELS
#define PPT_RASTER_SMALL_PIXELS 32
#endif
#ifndef PPT_RASTER_MEDIUM_SIDE
#define PPT_RASTER_MEDIUM_SIDE 64
#endif
constexpr int32_t kSmallPixels = PPT_RASTER_SMALL_PIXELS; // a box of at most this many pixel centres is walked by its own lane
constexpr int32_t kMediumSide = PPT_RASTER_MEDIUM_SIDE;   // a box of at most this side by the wave; beyond it the tiles take it
constexpr uint32_t kPolyMax = 10;     // a triangle against six planes: at most nine vertices

struct ClipV
{
    float x, y, z, w;
};

// modelToWorld (its three rows as vec4s), then worldToCamera, then cameraToClip: project_ndc's chains, the translation first
PPT_RS ClipV to_clip(const RasterView &v, const prosper_mat3x4 &m, f3 p)
{
    const float wx = __builtin_fmaf(p.z, m.col[0].z, __builtin_fmaf(p.y, m.col[0].y, __builtin_fmaf(p.x, m.col[0].x, m.col[0].w)));
    const float wy = __builtin_fmaf(p.z, m.col[1].z, __builtin_fmaf(p.y, m.col[1].y, __builtin_fmaf(p.x, m.col[1].x, m.col[1].w)));
    const float wz = __builtin_fmaf(p.z, m.col[2].z, __builtin_fmaf(p.y, m.col[2].y, __builtin_fmaf(p.x, m.col[2].x, m.col[2].w)));
    const float *w = v.worldToCamera, *c = v.cameraToClip;
    float cam[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cam[k] = __builtin_fmaf(w[8 + k], wz, __builtin_fmaf(w[4 + k], wy, __builtin_fmaf(w[k], wx, w[12 + k])));
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
        o[r] = __builtin_fmaf(c[12 + r], cam[3], __builtin_fmaf(c[8 + r], cam[2], __builtin_fmaf(c[4 + r], cam[1], c[r] * cam[0])));
    return ClipV{o[0], o[1], o[2], o[3]};
}

// the signed distance of plane k: near (z <= w), far (z >= 0), x <= G w, x >= -G w, y <= G w, y >= -G w; inside is >= 0
PPT_RS float plane_distance(uint32_t k, ClipV c, float G)
{
    switch (k)
    {
    case 0: return c.w - c.z;
    case 1: return c.z;
    case 2: return __builtin_fmaf(G, c.w, -c.x);
    case 3: return __builtin_fmaf(G, c.w, c.x);
    case 4: return __builtin_fmaf(G, c.w, -c.y);
    default: return __builtin_fmaf(G, c.w, c.y);
    }
}

struct SnapV
{
    int32_t X, Y; // 1/256 pixel
    float d;      // z / w
    bool ok;      // both coordinates within 2^23
};

PPT_RS SnapV snap_vertex(const RasterView &v, ClipV c)
{
    const float fx = ((c.x / c.w) * 0.5f + 0.5f) * (float)v.width;
    const float fy = ((c.y / c.w) * 0.5f + 0.5f) * (float)v.height;
    const float sx = __builtin_rintf(fx * 256.0f), sy = __builtin_rintf(fy * 256.0f);
    SnapV s;
    s.ok = fabs_(sx) <= 8388608.0f && fabs_(sy) <= 8388608.0f; // (false for a NaN)
    s.X = s.ok ? (int32_t)sx : 0;
    s.Y = s.ok ? (int32_t)sy : 0;
    s.d = c.z / c.w;
    return s;
}

// vertex flags: bit 0 the index is the mesh's, bit 1 the fast path's conditions hold, bits 2-7 outside plane k
constexpr uint32_t kVertexValid = 1u, kVertexFast = 2u;
PPT_RS uint32_t vertex_flags(ClipV c, const SnapV &s, float G)
{
    uint32_t f = kVertexValid;
    if (c.w > 0.0f && c.z >= 0.0f && c.z <= c.w && s.ok) f |= kVertexFast;
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k)
        if (!(plane_distance(k, c, G) >= 0.0f)) f |= 4u << k;
    return f;
}

// One triangle ready to be walked: snapped vertices, z / w at each, and the pixel centres its box holds inside the image
struct Tri
{
    int32_t X0, Y0, X1, Y1, X2, Y2;
    float d0, d1, d2;
    int32_t px0, py0, px1, py1;
};

// twice the area in framebuffer coordinates, y down: negative is the front
PPT_RS int64_t area2_of(const Tri &t)
{
    return (int64_t)(t.X1 - t.X0) * (int64_t)(t.Y2 - t.Y0) - (int64_t)(t.Y1 - t.Y0) * (int64_t)(t.X2 - t.X0);
}

// the pixels whose centres (256 p + 128) lie in the vertices' box, clamped to the image; false: none
PPT_RS bool set_box(Tri &t, uint32_t width, uint32_t height)
{
    const int32_t minX = min(t.X0, min(t.X1, t.X2)), maxX = max(t.X0, max(t.X1, t.X2));
    const int32_t minY = min(t.Y0, min(t.Y1, t.Y2)), maxY = max(t.Y0, max(t.Y1, t.Y2));
    t.px0 = max((minX + 127) >> 8, 0);
    t.py0 = max((minY + 127) >> 8, 0);
    t.px1 = min((maxX - 128) >> 8, (int32_t)width - 1);
    t.py1 = min((maxY - 128) >> 8, (int32_t)height - 1);
    return t.px0 <= t.px1 && t.py0 <= t.py1;
}

// Coverage of pixel (px, py) by a FRONT-facing triangle (area2 < 0) under the top-left rule, and its depth
PPT_RS bool covers(const Tri &t, int64_t area2, int32_t px, int32_t py, float *depth)
{
    const int64_t sx = (int64_t)px * 256 + 128, sy = (int64_t)py * 256 + 128;
    // edges 0 -> 1, 1 -> 2, 2 -> 0: positive inside a front-facing triangle
    const int64_t ex0 = t.X1 - t.X0, ey0 = t.Y1 - t.Y0;
    const int64_t ex1 = t.X2 - t.X1, ey1 = t.Y2 - t.Y1;
    const int64_t ex2 = t.X0 - t.X2, ey2 = t.Y0 - t.Y2;
    const int64_t f0 = ey0 * (sx - t.X0) - ex0 * (sy - t.Y0);
    const int64_t f1 = ey1 * (sx - t.X1) - ex1 * (sy - t.Y1);
    const int64_t f2 = ey2 * (sx - t.X2) - ex2 * (sy - t.Y2);
    const bool in0 = f0 > 0 || (f0 == 0 && (ey0 > 0 || (ey0 == 0 && ex0 < 0)));
    const bool in1 = f1 > 0 || (f1 == 0 && (ey1 > 0 || (ey1 == 0 && ex1 < 0)));
    const bool in2 = f2 > 0 || (f2 == 0 && (ey2 > 0 || (ey2 == 0 && ex2 < 0)));
    if (!(in0 && in1 && in2)) return false;
    // f2 belongs to vertex 1 (the edge opposite it), f0 to vertex 2; f0 + f1 + f2 = -area2
    const float twoA = (float)(-area2);
    const float l1 = (float)f2 / twoA, l2 = (float)f0 / twoA;
    const float d = __builtin_fmaf(l2, t.d2 - t.d0, __builtin_fmaf(l1, t.d1 - t.d0, t.d0));
    *depth = d;
    return d > 0.0f && d <= 1.0f;
}

PPT_RS void emit(unsigned long long *keys, size_t pixel, float depth, uint32_t low)
{
    const uint32_t hi = f2u(depth);
    // the stored depth only grows: a fragment below it can never win (an equal one still may, by its low word)
    const unsigned long long stored = __hip_atomic_load(keys + pixel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (hi < (uint32_t)(stored >> 32)) return;
    atomicMax(keys + pixel, ((unsigned long long)hi << 32) | (unsigned long long)low);
}

PPT_RS uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

PPT_RS void count_ballot(uint32_t *counter, bool flag, uint32_t lane)
{
    const unsigned long long mask = __ballot(flag);
    if (lane == 0u && mask != 0ull) atomicAdd(counter, (uint32_t)__popcll(mask));
}

// A draw-list entry's meshlet, every read checked against the mesh's guard
struct Meshlet
{
    const uint32_t *words;
    prosper_GeometryMetadata md;
    RasterMeshGuard guard;
    const prosper_ModelInstanceTransforms *transform;
    uint32_t vertexOffset, triangleOffset, vertexCount, triangleCount;
    uint32_t ordinal;
    uint32_t drawInstance;
    uint32_t mask;                  // its material is MASK: fragments are tested (p.anyMask)
    uint32_t mapStart, mapCount;    // its geometry triangles: triMap[mapStart .. mapStart + mapCount)
};

// gbuffer.frag:61-63: sampleMaterial's alpha of the fragment's pixel is 0.  The resolve's own functions, so that the
// resolve never meets it.
template <bool kLod> PPT_RS bool alpha_discards(const RasterParams &p, int32_t px, int32_t py, uint32_t di, uint32_t prim)
{
    const Ray ray = raster_pixel_ray(p.ray, p.currentJitter, (uint32_t)px, (uint32_t)py);
    const Hit hit = raster_hit(p.scene, ray, di, prim);
    const Surface sf = raster_pixel_surface<kLod>(p.scene, p.ray, p.currentJitter, p.mips, p.lodBias, (uint32_t)px, (uint32_t)py, ray, hit, nullptr);
    return sf.material.alpha == 0.0f;
}

// What a raster pass does with its fragments: the visibility image's atomicMax, or the transparent lists' two passes
// (plain ints, not an unnamed enum: the mode is part of the kernels' mangled names, which host and device must agree on)
constexpr int kModeVisibility = 0, kModeLayerCount = 1, kModeLayerFill = 2;

// A fragment of the transparent lists: eGreater against the stored depth (a coplanar fragment fails, a stored 0 passes
// everything, a NaN nothing), then forward.frag:57's discard, then the count or the key.  One function for both passes.
template <int kMode, bool kLod>
PPT_RS void layer_fragment(const RasterParams &p, const RasterLayerTargets &L, int32_t px, int32_t py, float depth, uint32_t low, uint32_t di, uint32_t prim)
{
    const size_t pixel = (size_t)py * p.view.width + (size_t)px;
    if (!(depth > L.depth[pixel])) return;
    if (alpha_discards<kLod>(p, px, py, di, prim)) return;
    if constexpr (kMode == kModeLayerCount)
        atomicAdd(L.counts + pixel, 1u);
    else
    {
        const uint32_t at = L.offsets[pixel] + atomicAdd(L.cursor + pixel, 1u);
        if (at < L.capacity) L.fragments[at] = ((unsigned long long)f2u(depth) << 32) | (unsigned long long)low;
    }
}

// kAll: every meshlet's fragments are tested against the material (the transparent lists), not only a MASK meshlet's
template <bool kAll = false> PPT_RS bool load_meshlet(const RasterParams &p, uint32_t entry, Meshlet *out)
{
    const uint32_t di = p.list[1u + 2u * entry], mi = p.list[2u + 2u * entry];
    if (di >= p.drawInstanceCount) return false;
    const prosper_DrawInstance inst = p.drawInstances[di];
    if (inst.meshIndex >= p.meshCount || inst.modelInstanceIndex >= p.modelInstanceCount) return false;
    Meshlet m;
    m.md = p.metadatas[inst.meshIndex];
    m.guard = p.guards[inst.meshIndex];
    if (mi >= m.guard.meshletCount || m.md.bufferIndex >= PROSPER_PT_MAX_GEOMETRY_BUFFERS || m.guard.bufferWords == 0u) return false;
    if ((uint64_t)m.md.meshletsOffset + 4ull * mi + 3ull >= (uint64_t)m.guard.bufferWords) return false;
    m.words = static_cast<const uint32_t *>(p.geometryBuffers[m.md.bufferIndex]);
    const uint32_t *h = m.words + m.md.meshletsOffset + 4u * mi;
    m.vertexOffset = h[0];
    m.triangleOffset = h[1];
    m.vertexCount = h[2] < kRasterMaxVertices ? h[2] : kRasterMaxVertices;
    m.triangleCount = h[3] < kRasterMaxTriangles ? h[3] : kRasterMaxTriangles;
    m.transform = p.transforms + inst.modelInstanceIndex;
    m.ordinal = p.meshletBase[di] + mi;
    m.drawInstance = di;
    m.mask = 0u, m.mapStart = 0u, m.mapCount = 0u;
    bool tested = true;
    if constexpr (!kAll)
        tested = p.anyMask && inst.materialIndex < p.scene.materialCount && p.scene.materials[inst.materialIndex].alphaMode == PROSPER_ALPHA_MODE_MASK;
    if (tested)
    {
        const uint32_t gm = p.meshMeshletBase[inst.meshIndex] + mi; // (mi is below the mesh's meshlet count: the map has it)
        m.mask = 1u;
        m.mapStart = p.meshletTriStart[gm];
        m.mapCount = p.meshletTriStart[gm + 1u] - m.mapStart;
    }
    *out = m;
    return true;
}

// loadMeshletVertexIndex, loadVertex's position (fp16) and the way to clip space; false: an index that is not the mesh's
PPT_RS bool load_clip_vertex(const RasterParams &p, const Meshlet &m, uint32_t k, ClipV *out)
{
    const uint64_t at = (uint64_t)m.md.meshletVerticesOffset + m.vertexOffset + k;
    uint32_t vi;
    if (m.md.usesShortIndices == 1u)
    {
        if (at / 2u >= (uint64_t)m.guard.bufferWords) return false;
        vi = reinterpret_cast<const uint16_t *>(m.words)[at];
    }
    else
    {
        if (at >= (uint64_t)m.guard.bufferWords) return false;
        vi = m.words[at];
    }
    if (vi >= m.guard.vertexCount) return false;
    const uint64_t pos = (uint64_t)m.md.positionsOffset + 2ull * vi;
    if (pos + 1ull >= (uint64_t)m.guard.bufferWords) return false;
    const uint32_t xy = m.words[pos], zw = m.words[pos + 1ull];
    const f3 position = {half_to_float(xy & 0xFFFFu), half_to_float(xy >> 16), half_to_float(zw & 0xFFFFu)};
    *out = to_clip(p.view, m.transform->modelToWorld, position);
    return true;
}

// the three meshlet-local vertex indices of triangle t; false: bytes outside the buffer or an index past the meshlet's vertices
PPT_RS bool load_triangle(const Meshlet &m, uint32_t t, uint32_t *i0, uint32_t *i1, uint32_t *i2)
{
    const uint64_t at = (uint64_t)m.md.meshletTrianglesByteOffset + m.triangleOffset + 3ull * t;
    if (at + 2ull >= (uint64_t)m.guard.bufferWords * 4ull) return false;
    const uint8_t *b = reinterpret_cast<const uint8_t *>(m.words) + at;
    *i0 = b[0], *i1 = b[1], *i2 = b[2];
    return *i0 < m.vertexCount && *i1 < m.vertexCount && *i2 < m.vertexCount;
}

enum : uint32_t
{
    kClassNone = 0,
    kClassSmall = 1,
    kClassMedium = 2,
    kClassQueue = 3,
};

// kMode: what becomes of a fragment.  The layer modes test every meshlet's fragments against the material (kMask), in the
// wave's walk, and count nothing.
struct RasterNoLayers
{
};
template <int kMode> using LayerTargetsOf = std::conditional_t<kMode != kModeVisibility, RasterLayerTargets, RasterNoLayers>;

template <bool kMask, bool kLod, int kMode = kModeVisibility>
__global__ __launch_bounds__(256) void raster_meshlets_kernel(const RasterParams p, const LayerTargetsOf<kMode> L)
{
    constexpr bool kLayers = kMode != kModeVisibility;
    static_assert(kMask || !kLayers, "the layer modes test every fragment");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t entry = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t count = p.list[0] < p.capacity ? p.list[0] : p.capacity;
    if (entry >= count) return; // (the whole wave)
    Meshlet m;
    if (!load_meshlet<kLayers>(p, entry, &m)) return; // (the whole wave: every lane reads the same entry)

    // ---- a lane per vertex ----
    int32_t vX = 0, vY = 0;
    float vD = 0.0f;
    uint32_t vFlags = 0u;
    if (lane < m.vertexCount)
    {
        ClipV c;
        if (load_clip_vertex(p, m, lane, &c))
        {
            const SnapV s = snap_vertex(p.view, c);
            vX = s.X, vY = s.Y, vD = s.d;
            vFlags = vertex_flags(c, s, p.view.guardBand);
        }
    }

    uint32_t fragments = 0u;
    const uint32_t lowBase = m.ordinal * 128u;
    // ---- a lane per triangle ----
    for (uint32_t round = 0; round * 64u < m.triangleCount; ++round) // (the same in every lane)
    {
        const uint32_t t = round * 64u + lane;
        const bool live = t < m.triangleCount;
        uint32_t i0 = 0, i1 = 0, i2 = 0;
        const bool indexed = live && load_triangle(m, t, &i0, &i1, &i2);
        if (!indexed) i0 = i1 = i2 = 0u;
        // (every lane takes part in the exchanges; a lane without a triangle reads vertex 0 and drops it)
        Tri tri;
        tri.X0 = __shfl(vX, (int)i0, 64), tri.Y0 = __shfl(vY, (int)i0, 64), tri.d0 = __shfl(vD, (int)i0, 64);
        tri.X1 = __shfl(vX, (int)i1, 64), tri.Y1 = __shfl(vY, (int)i1, 64), tri.d1 = __shfl(vD, (int)i1, 64);
        tri.X2 = __shfl(vX, (int)i2, 64), tri.Y2 = __shfl(vY, (int)i2, 64), tri.d2 = __shfl(vD, (int)i2, 64);
        const uint32_t fl0 = (uint32_t)__shfl((int)vFlags, (int)i0, 64), fl1 = (uint32_t)__shfl((int)vFlags, (int)i1, 64);
        const uint32_t fl2 = (uint32_t)__shfl((int)vFlags, (int)i2, 64);
        tri.px0 = tri.py0 = 0, tri.px1 = tri.py1 = -1;

        // a MASK meshlet's fragments are tested against the material: the lane needs its geometry triangle
        uint32_t prim = 0u;
        bool mapped = true;
        if constexpr (kMask)
            if (m.mask && live)
            {
                mapped = t < m.mapCount;
                if (mapped) prim = p.triMap[m.mapStart + t];
            }
        uint32_t cls = kClassNone;
        bool back = false, zero = false, outside = false;
        int64_t area2 = 0;
        if (live)
        {
            const uint32_t all = fl0 & fl1 & fl2;
            if (!indexed || !mapped || !(all & kVertexValid)) outside = true;
            else if (all & kVertexFast)
            {
                area2 = area2_of(tri);
                if (area2 == 0) zero = true;
                else if (area2 > 0) back = true;
                else if (!set_box(tri, p.view.width, p.view.height)) outside = true;
                else
                {
                    const int32_t bw = tri.px1 - tri.px0 + 1, bh = tri.py1 - tri.py0 + 1;
                    cls = bw * bh <= kSmallPixels ? kClassSmall : (bw <= kMediumSide && bh <= kMediumSide) ? kClassMedium : kClassQueue;
                }
            }
            else if (all >> 2) outside = true; // all three vertices beyond one plane
            else cls = kClassQueue;            // the clipper's
        }
        if constexpr (kMask)
            if (m.mask && cls == kClassSmall) cls = kClassMedium; // (one place tests the material: the wave's walk)
        if constexpr (!kLayers)
        {
            count_ballot(&p.counters->triangles, live, lane);
            count_ballot(&p.counters->culledBackface, back, lane);
            count_ballot(&p.counters->culledZeroArea, zero, lane);
            count_ballot(&p.counters->culledOutside, outside, lane);
        }

        if constexpr (!kLayers) // (a layer mode has no small class: m.mask)
            if (cls == kClassSmall)
            {
                const uint32_t low = ~(lowBase + t);
                for (int32_t py = tri.py0; py <= tri.py1; ++py)
                    for (int32_t px = tri.px0; px <= tri.px1; ++px)
                    {
                        float depth;
                        if (!covers(tri, area2, px, py, &depth)) continue;
                        ++fragments;
                        emit(p.keys, (size_t)py * p.view.width + (size_t)px, depth, low);
                    }
            }
        // medium: one triangle at a time, the wave over its box in blocks of 8 x 8 pixels
        unsigned long long medium = __ballot(cls == kClassMedium);
        while (medium != 0ull) // (the same in every lane)
        {
            const int src = __ffsll((long long)medium) - 1;
            medium &= medium - 1ull;
            Tri w;
            w.X0 = __shfl(tri.X0, src, 64), w.Y0 = __shfl(tri.Y0, src, 64), w.d0 = __shfl(tri.d0, src, 64);
            w.X1 = __shfl(tri.X1, src, 64), w.Y1 = __shfl(tri.Y1, src, 64), w.d1 = __shfl(tri.d1, src, 64);
            w.X2 = __shfl(tri.X2, src, 64), w.Y2 = __shfl(tri.Y2, src, 64), w.d2 = __shfl(tri.d2, src, 64);
            w.px0 = __shfl(tri.px0, src, 64), w.py0 = __shfl(tri.py0, src, 64);
            w.px1 = __shfl(tri.px1, src, 64), w.py1 = __shfl(tri.py1, src, 64);
            const int64_t a2 = area2_of(w);
            const uint32_t wprim = (uint32_t)__shfl((int)prim, src, 64);
            const uint32_t low = ~(lowBase + round * 64u + (uint32_t)src);
            for (int32_t by = w.py0; by <= w.py1; by += 8)
                for (int32_t bx = w.px0; bx <= w.px1; bx += 8)
                {
                    const int32_t px = bx + (int32_t)(lane & 7u), py = by + (int32_t)(lane >> 3);
                    float depth;
                    if (px > w.px1 || py > w.py1 || !covers(w, a2, px, py, &depth)) continue;
                    if constexpr (kLayers)
                        layer_fragment<kMode, kLod>(p, L, px, py, depth, low, m.drawInstance, wprim);
                    else
                    {
                        if constexpr (kMask)
                            if (m.mask && alpha_discards<kLod>(p, px, py, m.drawInstance, wprim)) continue;
                        ++fragments;
                        emit(p.keys, (size_t)py * p.view.width + (size_t)px, depth, low);
                    }
                }
        }
        // large, and what has to be clipped: the queue
        {
            const bool queued = cls == kClassQueue;
            const unsigned long long mask = __ballot(queued);
            if (mask != 0ull)
            {
                const uint32_t n = (uint32_t)__popcll(mask);
                uint32_t start = 0;
                if (lane == 0u) start = atomicAdd(p.queue, n);
                start = (uint32_t)__builtin_amdgcn_readfirstlane((int)start);
                const uint32_t at = start + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                const bool room = at < p.queueCapacity;
                if (queued && room)
                {
                    p.queue[2u + 2u * at] = entry;
                    p.queue[3u + 2u * at] = t;
                }
                if constexpr (!kLayers)
                {
                    count_ballot(&p.counters->queued, queued && room, lane);
                    count_ballot(&p.counters->queueOverflow, queued && !room, lane);
                }
            }
        }
    }
    if constexpr (!kLayers)
    {
        fragments = wave_sum(fragments);
        if (lane == 0u && fragments != 0u) atomicAdd(&p.counters->fragments, fragments);
    }
}


// Sutherland-Hodgman over the six planes, in float32, by the record's lane: the polygon ping-pongs between poly[0] and poly[1]
// (LDS, so that the running index costs no private memory).  A crossing is cut from the inside vertex towards the outside
// one, t = d_in / (d_in - d_out), every component fma(t, out - in, in): the same point whichever way the edge is walked.
// -> the vertex count, the polygon in poly[0]
PPT_RS uint32_t clip_polygon(ClipV (*poly)[kPolyMax], float G)
{
    uint32_t n = 3u, from = 0u;
    for (uint32_t k = 0; k < 6u && n != 0u; ++k)
    {
        const ClipV *in = poly[from];
        ClipV *out = poly[1u - from];
        uint32_t m = 0u;
        for (uint32_t i = 0; i < n; ++i)
        {
            const ClipV a = in[i], b = in[i + 1u < n ? i + 1u : 0u];
            const float da = plane_distance(k, a, G), db = plane_distance(k, b, G);
            const bool ina = da >= 0.0f, inb = db >= 0.0f;
            if (ina && m < kPolyMax) out[m++] = a;
            if (ina != inb && m < kPolyMax)
            {
                const ClipV s = ina ? a : b, e = ina ? b : a;
                const float ds = ina ? da : db, de = ina ? db : da;
                const float t = ds / (ds - de);
                out[m++] = ClipV{__builtin_fmaf(t, e.x - s.x, s.x), __builtin_fmaf(t, e.y - s.y, s.y),
                                 __builtin_fmaf(t, e.z - s.z, s.z), __builtin_fmaf(t, e.w - s.w, s.w)};
            }
        }
        n = m < 3u ? 0u : m;
        from = 1u - from;
    }
    if (from == 1u)
        for (uint32_t i = 0; i < n; ++i) poly[0][i] = poly[1][i];
    return n;
}

// One WAVE per 32 x 32 pixel tile.  The queue is taken 64 records at a time: every lane sets one record up - its three
// vertices again, the clipper where it is needed, the snapped polygon into the lane's slice of LDS - and tests the
// polygon's box against the tile; the records that reach the tile are then walked one after the other by the whole wave.
// (A workgroup is one wave: the barriers order the wave's own LDS traffic and cost nothing.)
template <bool kMask, bool kLod, int kMode = kModeVisibility>
__global__ __launch_bounds__(64) void raster_large_kernel(const RasterParams p, const LayerTargetsOf<kMode> L)
{
    constexpr bool kLayers = kMode != kModeVisibility;
    __shared__ ClipV poly[64][2][kPolyMax];
    __shared__ int32_t sX[64][kPolyMax], sY[64][kPolyMax];
    __shared__ float sD[64][kPolyMax];
    const uint32_t records = p.queue[0] < p.queueCapacity ? p.queue[0] : p.queueCapacity; // the one load of an empty queue
    if (records == 0u) return;
    const uint32_t lane = threadIdx.x;
    const bool first = blockIdx.x == 0u && blockIdx.y == 0u; // the tile that counts what happens once per triangle
    const int32_t tx0 = (int32_t)(blockIdx.x * kRasterTile), ty0 = (int32_t)(blockIdx.y * kRasterTile);
    const int32_t tx1 = min(tx0 + (int32_t)kRasterTile, (int32_t)p.view.width) - 1;
    const int32_t ty1 = min(ty0 + (int32_t)kRasterTile, (int32_t)p.view.height) - 1;
    const float G = p.view.guardBand;
    uint32_t fragments = 0u;
    for (uint32_t base = 0; base < records; base += 64u) // (the same in every lane: the barriers below are reached by all)
    {
        const uint32_t r = base + lane;
        uint32_t n = 0u, low = 0u, recMask = 0u, recPrim = 0u, recDi = 0u;
        bool hit = false, clipped = false, nothingLeft = false;
        if (r < records)
        {
            const uint32_t entry = p.queue[2u + 2u * r], t = p.queue[3u + 2u * r];
            Meshlet m;
            uint32_t i0, i1, i2;
            ClipV c0, c1, c2;
            if (entry < p.capacity && load_meshlet<kLayers>(p, entry, &m) && t < m.triangleCount && load_triangle(m, t, &i0, &i1, &i2) &&
                load_clip_vertex(p, m, i0, &c0) && load_clip_vertex(p, m, i1, &c1) && load_clip_vertex(p, m, i2, &c2))
            {
                const SnapV s0 = snap_vertex(p.view, c0), s1 = snap_vertex(p.view, c1), s2 = snap_vertex(p.view, c2);
                if ((vertex_flags(c0, s0, G) & vertex_flags(c1, s1, G) & vertex_flags(c2, s2, G) & kVertexFast) != 0u)
                {
                    sX[lane][0] = s0.X, sY[lane][0] = s0.Y, sD[lane][0] = s0.d;
                    sX[lane][1] = s1.X, sY[lane][1] = s1.Y, sD[lane][1] = s1.d;
                    sX[lane][2] = s2.X, sY[lane][2] = s2.Y, sD[lane][2] = s2.d;
                    n = 3u;
                }
                else
                {
                    poly[lane][0][0] = c0, poly[lane][0][1] = c1, poly[lane][0][2] = c2;
                    n = clip_polygon(poly[lane], G);
                    for (uint32_t i = 0; i < n; ++i)
                    {
                        const SnapV s = snap_vertex(p.view, poly[lane][0][i]);
                        if (!s.ok)
                        {
                            n = 0u; // (the guard band's margin keeps a clipped vertex inside 2^23: never taken)
                            break;
                        }
                        sX[lane][i] = s.X, sY[lane][i] = s.Y, sD[lane][i] = s.d;
                    }
                    clipped = n != 0u;
                    nothingLeft = n == 0u;
                }
                low = ~(m.ordinal * 128u + t);
                if constexpr (kMask)
                    if (m.mask)
                    {
                        recMask = 1u, recDi = m.drawInstance;
                        if (t < m.mapCount)
                            recPrim = p.triMap[m.mapStart + t];
                        else
                            n = 0u; // (the meshlet kernel drops such a triangle: never queued)
                    }
                if (n != 0u)
                {
                    // the pixel centres in the polygon's box, against the tile
                    int32_t minX = sX[lane][0], maxX = minX, minY = sY[lane][0], maxY = minY;
                    for (uint32_t i = 1; i < n; ++i)
                    {
                        minX = min(minX, sX[lane][i]), maxX = max(maxX, sX[lane][i]);
                        minY = min(minY, sY[lane][i]), maxY = max(maxY, sY[lane][i]);
                    }
                    hit = max((minX + 127) >> 8, tx0) <= min((maxX - 128) >> 8, tx1) &&
                          max((minY + 127) >> 8, ty0) <= min((maxY - 128) >> 8, ty1);
                }
            }
        }
        if constexpr (!kLayers)
            if (first)
            {
                count_ballot(&p.counters->clipped, clipped, lane);
                count_ballot(&p.counters->culledOutside, nothingLeft, lane);
            }
        __syncthreads(); // the lanes' polygons are in LDS
        unsigned long long todo = __ballot(hit);
        while (todo != 0ull) // (the same in every lane)
        {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const uint32_t count = (uint32_t)__shfl((int)n, src, 64), key = (uint32_t)__shfl((int)low, src, 64);
            const uint32_t smask = (uint32_t)__shfl((int)recMask, src, 64), sprim = (uint32_t)__shfl((int)recPrim, src, 64);
            const uint32_t sdi = (uint32_t)__shfl((int)recDi, src, 64);
            for (uint32_t k = 1; k + 1u < count; ++k) // the fan from the polygon's first vertex
            {
                Tri tri;
                tri.X0 = sX[src][0], tri.Y0 = sY[src][0], tri.d0 = sD[src][0];
                tri.X1 = sX[src][k], tri.Y1 = sY[src][k], tri.d1 = sD[src][k];
                tri.X2 = sX[src][k + 1u], tri.Y2 = sY[src][k + 1u], tri.d2 = sD[src][k + 1u];
                const int64_t area2 = area2_of(tri);
                if (area2 >= 0 || !set_box(tri, p.view.width, p.view.height)) continue;
                const int32_t x0 = max(tri.px0, tx0), x1 = min(tri.px1, tx1), y0 = max(tri.py0, ty0), y1 = min(tri.py1, ty1);
                if (x0 > x1 || y0 > y1) continue;
                const uint32_t bw = (uint32_t)(x1 - x0 + 1), total = bw * (uint32_t)(y1 - y0 + 1);
                for (uint32_t i = lane; i < total; i += 64u)
                {
                    const int32_t px = x0 + (int32_t)(i % bw), py = y0 + (int32_t)(i / bw);
                    float depth;
                    if (!covers(tri, area2, px, py, &depth)) continue;
                    if constexpr (kLayers)
                        layer_fragment<kMode, kLod>(p, L, px, py, depth, key, sdi, sprim);
                    else
                    {
                        if constexpr (kMask)
                            if (smask && alpha_discards<kLod>(p, px, py, sdi, sprim)) continue;
                        ++fragments;
                        emit(p.keys, (size_t)py * p.view.width + (size_t)px, depth, key);
                    }
                }
            }
        }
        __syncthreads(); // ... and have been read before the next 64 records replace them
    }
    if constexpr (!kLayers)
    {
        fragments = wave_sum(fragments);
        if (lane == 0u && fragments != 0u) atomicAdd(&p.counters->fragments, fragments);
    }
}


// ---- the exclusive scan of the per-pixel counts ----

// The inclusive scan of a wave's 64 values: Hillis-Steele inside each row of 16 lanes by DPP row_shr 1, 2, 4, 8 (a lane
// whose source lies outside its row adds 0), then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3.
// Every lane of the wave is active where it is called.
template <int Ctrl, int RowMask> PPT_RS uint32_t dpp_or_zero(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, Ctrl, RowMask, 0xF, false);
}
PPT_RS uint32_t wave_inclusive_scan(uint32_t v)
{
    v += dpp_or_zero<0x111, 0xF>(v);
    v += dpp_or_zero<0x112, 0xF>(v);
    v += dpp_or_zero<0x114, 0xF>(v);
    v += dpp_or_zero<0x118, 0xF>(v);
    v += dpp_or_zero<0x142, 0xA>(v);
    v += dpp_or_zero<0x143, 0xC>(v);
    return v;
}

constexpr uint32_t kScanPerLane = kRasterScanBlock / 64u; // consecutive counters of one lane

// blockSums[b] = the sum of the block's counters
__global__ __launch_bounds__(64) void raster_scan_sums_kernel(const uint32_t *__restrict__ counts, uint32_t *__restrict__ blockSums, size_t pixels)
{
    const size_t base = (size_t)blockIdx.x * kRasterScanBlock + (size_t)threadIdx.x * kScanPerLane;
    uint32_t sum = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kScanPerLane; ++k)
        if (base + k < pixels) sum += counts[base + k];
    sum = wave_inclusive_scan(sum);
    if (threadIdx.x == 63u) blockSums[blockIdx.x] = sum;
}

// One wave: blockSums -> their exclusive scan in place, 64 at a time with a carry; *total = the sum of all
__global__ __launch_bounds__(64) void raster_scan_blocks_kernel(uint32_t *__restrict__ blockSums, uint32_t blocks, uint32_t *__restrict__ total)
{
    uint32_t carry = 0u;
    for (uint32_t b = 0; b < blocks; b += 64u) // (the same in every lane)
    {
        const uint32_t i = b + threadIdx.x;
        const uint32_t v = i < blocks ? blockSums[i] : 0u;
        const uint32_t inclusive = wave_inclusive_scan(v);
        if (i < blocks) blockSums[i] = carry + (inclusive - v);
        carry += (uint32_t)__builtin_amdgcn_readlane((int)inclusive, 63);
    }
    if (threadIdx.x == 0u) *total = carry;
}

// offsets[i] = the block's offset + the counters before i in the block
__global__ __launch_bounds__(64) void raster_scan_offsets_kernel(
    const uint32_t *__restrict__ counts, const uint32_t *__restrict__ blockOffsets, uint32_t *__restrict__ offsets, size_t pixels)
{
    const size_t base = (size_t)blockIdx.x * kRasterScanBlock + (size_t)threadIdx.x * kScanPerLane;
    uint32_t c[kScanPerLane];
    uint32_t sum = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kScanPerLane; ++k)
    {
        c[k] = base + k < pixels ? counts[base + k] : 0u;
        sum += c[k];
    }
    uint32_t run = blockOffsets[blockIdx.x] + (wave_inclusive_scan(sum) - sum);
#pragma unroll
    for (uint32_t k = 0; k < kScanPerLane; ++k)
    {
        if (base + k < pixels) offsets[base + k] = run;
        run += c[k];
    }
}

__global__ __launch_bounds__(256) void raster_depth_kernel(const unsigned long long *keys, float *depth, size_t pixels)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i < pixels) depth[i] = u2f((uint32_t)(keys[i] >> 32));
}

} // namespace

float raster_guard_band(uint32_t width, uint32_t height)
{
    const uint32_t side = width > height ? width : height;
    return 65536.0f / (float)(side ? side : 1u) - 2.0f;
}

void launch_raster_meshlets(const RasterParams &p, hipStream_t stream)
{
    if (p.capacity == 0u) return;
    // the instantiations that test MASK fragments run only where the scene has such a material on meshlets
    const auto kernel = !p.anyMask ? raster_meshlets_kernel<false, false> : p.lod ? raster_meshlets_kernel<true, true> : raster_meshlets_kernel<true, false>;
    hipLaunchKernelGGL(kernel, dim3((p.capacity + 3u) / 4u), dim3(256), 0, stream, p, RasterNoLayers{});
}

void launch_raster_large(const RasterParams &p, hipStream_t stream)
{
    const dim3 grid((p.view.width + kRasterTile - 1u) / kRasterTile, (p.view.height + kRasterTile - 1u) / kRasterTile);
    const auto kernel = !p.anyMask ? raster_large_kernel<false, false> : p.lod ? raster_large_kernel<true, true> : raster_large_kernel<true, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(64), 0, stream, p, RasterNoLayers{});
}

void launch_raster_layers(const RasterParams &p, const RasterLayerTargets &t, bool fill, hipStream_t stream)
{
    if (p.capacity == 0u) return;
    const auto meshlets = p.lod ? (fill ? raster_meshlets_kernel<true, true, kModeLayerFill> : raster_meshlets_kernel<true, true, kModeLayerCount>)
                                : (fill ? raster_meshlets_kernel<true, false, kModeLayerFill> : raster_meshlets_kernel<true, false, kModeLayerCount>);
    hipLaunchKernelGGL(meshlets, dim3((p.capacity + 3u) / 4u), dim3(256), 0, stream, p, t);
    const dim3 grid((p.view.width + kRasterTile - 1u) / kRasterTile, (p.view.height + kRasterTile - 1u) / kRasterTile);
    const auto large = p.lod ? (fill ? raster_large_kernel<true, true, kModeLayerFill> : raster_large_kernel<true, true, kModeLayerCount>)
                             : (fill ? raster_large_kernel<true, false, kModeLayerFill> : raster_large_kernel<true, false, kModeLayerCount>);
    hipLaunchKernelGGL(large, grid, dim3(64), 0, stream, p, t);
}

void launch_raster_layer_scan(const uint32_t *counts, uint32_t *offsets, uint32_t *blockSums, uint32_t *total, size_t pixels, hipStream_t stream)
{
    const uint32_t blocks = raster_scan_blocks(pixels);
    if (blocks == 0u) return;
    hipLaunchKernelGGL(raster_scan_sums_kernel, dim3(blocks), dim3(64), 0, stream, counts, blockSums, pixels);
    hipLaunchKernelGGL(raster_scan_blocks_kernel, dim3(1), dim3(64), 0, stream, blockSums, blocks, total);
    hipLaunchKernelGGL(raster_scan_offsets_kernel, dim3(blocks), dim3(64), 0, stream, counts, blockSums, offsets, pixels);
}

void launch_raster_depth(const unsigned long long *keys, float *depth, uint32_t width, uint32_t height, hipStream_t stream)
{
    const size_t pixels = (size_t)width * height;
    if (pixels == 0u) return;
    hipLaunchKernelGGL(raster_depth_kernel, dim3((uint32_t)((pixels + 255u) / 256u)), dim3(256), 0, stream, keys, depth, pixels);
}

} // namespace ppt
