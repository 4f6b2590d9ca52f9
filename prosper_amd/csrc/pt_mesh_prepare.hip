// pt_mesh_prepare.hip — the kernels of prosper_pt_prepare_mesh: tangents for a primitive without any,
// packMeshData, and the bounds of the meshlets the host partitioned.  Each follows a statement in NumPy operation by
// operation and meets it bit for bit: prosper_amd/tangents.py, world.pack_mesh_data, meshlets.meshlet_bounds
// (ordered=True).  That needs one rounding per operation (-ffp-contract=off, the Makefile's) and the correctly rounded
// division and square root hipcc gives by default.
#include "pt_mesh_prepare.hpp"

#include "bvh_encode.hpp"
#include "meshlet_build.hpp"

namespace ppt
{

namespace
{

template <class T> struct V3
{
    T x, y, z;
};
using F3 = V3<float>;
using D3 = V3<double>;

template <class T> __device__ inline V3<T> sub(V3<T> a, V3<T> b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
template <class T> __device__ inline V3<T> div(V3<T> a, T s) { return {a.x / s, a.y / s, a.z / s}; }
template <class T> __device__ inline T dot(V3<T> a, V3<T> b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
template <class T> __device__ inline V3<T> cross(V3<T> a, V3<T> b)
{
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ inline float length(F3 a) { return __builtin_sqrtf(dot(a, a)); }
__device__ inline double length(D3 a) { return __builtin_sqrt(dot(a, a)); }
__device__ inline bool finite(float f) { return (enc_bits(f) & 0x7F800000u) != 0x7F800000u; }
__device__ inline bool finite(double d) { return (__builtin_bit_cast(uint64_t, d) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }
__device__ inline F3 load3(const float *p, uint32_t i) { return {p[3u * (size_t)i], p[3u * (size_t)i + 1u], p[3u * (size_t)i + 2u]}; }

constexpr double kFixedOne = 4294967296.0; // 2^32

// one corner's share of a unit direction, added to three of its vertex's sums
__device__ inline void add_fixed(long long *sums, F3 unit, float weight)
{
    const float v[3] = {unit.x * weight, unit.y * weight, unit.z * weight};
    for (int k = 0; k < 3; ++k)
    {
        const long long fixed = (long long)rint((double)v[k] * kFixedOne);
        if (fixed != 0) atomicAdd(reinterpret_cast<unsigned long long *>(sums + k), (unsigned long long)fixed);
    }
}

__global__ __launch_bounds__(256) void tangent_sums_kernel(
    const float *__restrict__ positions, const float *__restrict__ uvs, const uint32_t *__restrict__ indices, uint32_t triangleCount,
    long long *__restrict__ sums)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= triangleCount) return;
    const uint32_t i[3] = {indices[3u * (size_t)t], indices[3u * (size_t)t + 1u], indices[3u * (size_t)t + 2u]};
    const F3 p0 = load3(positions, i[0]), p1 = load3(positions, i[1]), p2 = load3(positions, i[2]);
    const F3 e1 = sub(p1, p0), e2 = sub(p2, p0);
    const float u0 = uvs[2u * (size_t)i[0]], v0 = uvs[2u * (size_t)i[0] + 1u];
    const float s1 = uvs[2u * (size_t)i[1]] - u0, t1 = uvs[2u * (size_t)i[1] + 1u] - v0;
    const float s2 = uvs[2u * (size_t)i[2]] - u0, t2 = uvs[2u * (size_t)i[2] + 1u] - v0;
    const float det = s1 * t2 - s2 * t1;
    const float sign = det < 0.0f ? -1.0f : 1.0f;
    const F3 sdir = {(e1.x * t2 - e2.x * t1) * sign, (e1.y * t2 - e2.y * t1) * sign, (e1.z * t2 - e2.z * t1) * sign};
    const F3 tdir = {(e2.x * s1 - e1.x * s2) * sign, (e2.y * s1 - e1.y * s2) * sign, (e2.z * s1 - e1.z * s2) * sign};
    const float slen = length(sdir), tlen = length(tdir);
    if (!(finite(det) && det != 0.0f && finite(slen) && slen > 0.0f && finite(tlen) && tlen > 0.0f)) return;
    const F3 su = div(sdir, slen), tu = div(tdir, tlen);
    const F3 a[3] = {e1, sub(p2, p1), sub(p0, p2)}, b[3] = {e2, sub(p0, p1), sub(p1, p2)};
    for (int c = 0; c < 3; ++c)
    {
        const float la = length(a[c]), lb = length(b[c]);
        const float sine = length(cross(div(a[c], la), div(b[c], lb)));
        const float weight = sine > 1.0f ? 1.0f : sine; // (a NaN stays one)
        if (!(finite(la) && la > 0.0f && finite(lb) && lb > 0.0f && finite(weight))) continue;
        add_fixed(sums + 6u * (size_t)i[c], su, weight);
        add_fixed(sums + 6u * (size_t)i[c] + 3u, tu, weight);
    }
}

// glm::packSnorm3x10_1x2 as world.pack_snorm3x10_1x2 states it: round half away from zero of the clamped value
__device__ inline uint32_t snorm_bits(float v, float scale, uint32_t mask)
{
    if (v != v) return 0u;
    const float c = (v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v)) * scale;
    return (uint32_t)(int32_t)__builtin_truncf(c + __builtin_copysignf(0.5f, c)) & mask;
}
__device__ inline uint32_t pack_snorm3x10_1x2(float x, float y, float z, float w)
{
    return snorm_bits(x, 511.0f, 0x3FFu) | (snorm_bits(y, 511.0f, 0x3FFu) << 10) | (snorm_bits(z, 511.0f, 0x3FFu) << 20) |
           (snorm_bits(w, 1.0f, 0x3u) << 30);
}

// tangents.py finish for one vertex
__device__ inline void finish_tangent(const long long *sums, F3 normal, float out[4])
{
    const D3 n = {(double)normal.x, (double)normal.y, (double)normal.z};
    const double inv = 1.0 / kFixedOne;
    const D3 T = {(double)sums[0] * inv, (double)sums[1] * inv, (double)sums[2] * inv};
    const D3 B = {(double)sums[3] * inv, (double)sums[4] * inv, (double)sums[5] * inv};
    const double d = dot(n, T);
    D3 t = {T.x - n.x * d, T.y - n.y * d, T.z - n.z * d};
    const double len = length(t);
    if (finite(len) && len > 0.0)
    {
        t = div(t, len);
        const double hand = dot(cross(n, t), B);
        out[0] = (float)t.x;
        out[1] = (float)t.y;
        out[2] = (float)t.z;
        out[3] = hand < 0.0 ? -1.0f : 1.0f;
        return;
    }
    // the fallback: across the axis of the normal's smallest component, the first of equal ones
    const double ax = __builtin_fabs(n.x), ay = __builtin_fabs(n.y), az = __builtin_fabs(n.z);
    int axis = 0;
    double smallest = ax;
    if (ay < smallest)
    {
        axis = 1;
        smallest = ay;
    }
    if (az < smallest) axis = 2;
    D3 f = axis == 0 ? D3{0.0, n.z, -n.y} : (axis == 1 ? D3{-n.z, 0.0, n.x} : D3{n.y, -n.x, 0.0});
    const double flen = length(f);
    f = div(f, flen);
    const bool ok = finite(n.x) && finite(n.y) && finite(n.z) && finite(flen) && flen > 0.0;
    out[0] = ok ? (float)f.x : 1.0f;
    out[1] = ok ? (float)f.y : 0.0f;
    out[2] = ok ? (float)f.z : 0.0f;
    out[3] = 1.0f;
}

__global__ __launch_bounds__(256) void pack_mesh_kernel(PackMeshArgs a)
{
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= a.vertexCount) return;
    const F3 p = load3(a.positions, v);
    // half4 (x, y, z, 1)
    a.blob[a.positionsOffset + 2u * (size_t)v] = (uint32_t)half_rne(p.x) | ((uint32_t)half_rne(p.y) << 16);
    a.blob[a.positionsOffset + 2u * (size_t)v + 1u] = (uint32_t)half_rne(p.z) | (0x3C00u << 16);
    F3 n = {0.0f, 0.0f, 0.0f};
    if (a.normals)
    {
        n = load3(a.normals, v);
        a.blob[a.normalsOffset + v] = pack_snorm3x10_1x2(n.x, n.y, n.z, 0.0f);
    }
    if (a.mode == PrepareTangents::Supplied)
    {
        const float *t = a.tangents + 4u * (size_t)v;
        a.blob[a.tangentsOffset + v] = pack_snorm3x10_1x2(t[0], t[1], t[2], t[3]);
    }
    else if (a.mode == PrepareTangents::Generated)
    {
        float t[4];
        finish_tangent(a.sums + 6u * (size_t)v, n, t);
        for (int k = 0; k < 4; ++k) a.tangentsOut[4u * (size_t)v + k] = t[k];
        a.blob[a.tangentsOffset + v] = pack_snorm3x10_1x2(t[0], t[1], t[2], t[3]);
    }
    if (a.uvs)
        a.blob[a.texCoord0sOffset + v] = (uint32_t)half_rne(a.uvs[2u * (size_t)v]) | ((uint32_t)half_rne(a.uvs[2u * (size_t)v + 1u]) << 16);
}

__device__ inline double wave_min(double v)
{
    for (int o = 32; o > 0; o >>= 1)
    {
        const double other = __shfl_xor(v, o, 64);
        v = other < v ? other : v;
    }
    return v;
}
__device__ inline double wave_max(double v)
{
    for (int o = 32; o > 0; o >>= 1)
    {
        const double other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
    }
    return v;
}

__device__ inline int32_t s8_of(double v)
{
    const double r = rint(v * 127.0);
    return (int32_t)(r < -127.0 ? -127.0 : (r > 127.0 ? 127.0 : r));
}

// One wave per meshlet: lane l holds vertex l, and triangles l and l + 64.
__global__ __launch_bounds__(64) void meshlet_bounds_kernel(MeshletBoundsArgs a)
{
    static_assert(kMeshletMaxVertices == 64 && kMeshletMaxTriangles <= 128, "a lane per vertex, two triangles per lane");
    __shared__ double points[kMeshletMaxVertices][3];
    __shared__ double normals[kMeshletMaxTriangles][3];
    __shared__ uint32_t faces[kMeshletMaxTriangles]; // 1: the triangle has a normal
    const uint32_t m = blockIdx.x, lane = threadIdx.x;
    const uint32_t *meshlet = a.blob + a.meshletsOffset + 4u * (size_t)m;
    const uint32_t vertexOffset = meshlet[0], triangleOffset = meshlet[1], vertexCount = meshlet[2], triangleCount = meshlet[3];
    const double inf = __builtin_inf();

    D3 p = {0.0, 0.0, 0.0};
    const bool hasVertex = lane < vertexCount;
    if (hasVertex)
    {
        const size_t entry = (size_t)a.meshletVerticesOffset + vertexOffset + lane;
        const uint32_t v = a.usesShortIndices ? reinterpret_cast<const uint16_t *>(a.blob)[entry] : a.blob[entry];
        const uint32_t w0 = a.blob[a.positionsOffset + 2u * (size_t)v], w1 = a.blob[a.positionsOffset + 2u * (size_t)v + 1u];
        p = {(double)half_value((uint16_t)(w0 & 0xFFFFu)), (double)half_value((uint16_t)(w0 >> 16)), (double)half_value((uint16_t)(w1 & 0xFFFFu))};
        points[lane][0] = p.x;
        points[lane][1] = p.y;
        points[lane][2] = p.z;
    }
    // the sphere: the middle of the box in float32, the largest distance from it rounded up
    const D3 lo = {wave_min(hasVertex ? p.x : inf), wave_min(hasVertex ? p.y : inf), wave_min(hasVertex ? p.z : inf)};
    const D3 hi = {wave_max(hasVertex ? p.x : -inf), wave_max(hasVertex ? p.y : -inf), wave_max(hasVertex ? p.z : -inf)};
    const float centre[3] = {(float)((lo.x + hi.x) * 0.5), (float)((lo.y + hi.y) * 0.5), (float)((lo.z + hi.z) * 0.5)};
    const D3 offset = sub(p, D3{(double)centre[0], (double)centre[1], (double)centre[2]});
    const double farthest = wave_max(hasVertex ? length(offset) : -1.0);
    float radius = (float)farthest;
    if ((double)radius < farthest) radius = enc_next_up(radius);
    __syncthreads();

    const uint8_t *corners = reinterpret_cast<const uint8_t *>(a.blob) + a.meshletTrianglesByteOffset + triangleOffset;
    for (uint32_t t = lane; t < triangleCount; t += 64u)
    {
        const uint32_t i0 = corners[3u * t], i1 = corners[3u * t + 1u], i2 = corners[3u * t + 2u];
        const D3 p0 = {points[i0][0], points[i0][1], points[i0][2]};
        const D3 p1 = {points[i1][0], points[i1][1], points[i1][2]};
        const D3 p2 = {points[i2][0], points[i2][1], points[i2][2]};
        const D3 n = cross(sub(p1, p0), sub(p2, p0));
        const double len = length(n);
        const bool faced = len > 0.0; // (a degenerate triangle faces nowhere)
        faces[t] = faced ? 1u : 0u;
        normals[t][0] = faced ? n.x / len : 0.0;
        normals[t][1] = faced ? n.y / len : 0.0;
        normals[t][2] = faced ? n.z / len : 0.0;
    }
    __syncthreads();

    // the sum of the normals is order-sensitive: row by row, every lane the same
    D3 sum = {0.0, 0.0, 0.0};
    bool any = false;
    for (uint32_t t = 0; t < triangleCount; ++t)
    {
        if (!faces[t]) continue;
        const D3 n = {normals[t][0], normals[t][1], normals[t][2]};
        sum = any ? D3{sum.x + n.x, sum.y + n.y, sum.z + n.z} : n;
        any = true;
    }
    int32_t axis[3] = {0, 0, 0}, cutoff = 127;
    const double sumLength = any ? length(sum) : 0.0;
    if (sumLength > 0.0)
    {
        // quantised first: the cutoff is taken against the axis the shader will see
        const int32_t q[3] = {s8_of(sum.x / sumLength), s8_of(sum.y / sumLength), s8_of(sum.z / sumLength)};
        D3 seen = {(double)q[0], (double)q[1], (double)q[2]};
        const double seenSquared = dot(seen, seen);
        if (seenSquared > 0.0)
        {
            seen = div(seen, __builtin_sqrt(seenSquared));
            double least = inf;
            for (uint32_t t = lane; t < triangleCount; t += 64u)
                if (faces[t])
                {
                    const double dp = (normals[t][0] * seen.x + normals[t][1] * seen.y) + normals[t][2] * seen.z;
                    least = dp < least ? dp : least;
                }
            least = wave_min(least);
            if (least > 0.1)
            {
                const double rest = 1.0 - least * least;
                const int32_t c = (int32_t)__builtin_ceil(__builtin_sqrt(rest > 0.0 ? rest : 0.0) * 127.0) + 1;
                if (c < 127)
                {
                    axis[0] = q[0];
                    axis[1] = q[1];
                    axis[2] = q[2];
                    cutoff = c;
                }
            }
        }
    }
    if (lane == 0)
    {
        uint32_t *words = a.blob + a.meshletBoundsOffset + 5u * (size_t)m;
        words[0] = enc_bits(centre[0]);
        words[1] = enc_bits(centre[1]);
        words[2] = enc_bits(centre[2]);
        words[3] = enc_bits(radius);
        words[4] = ((uint32_t)axis[0] & 0xFFu) | (((uint32_t)axis[1] & 0xFFu) << 8) | (((uint32_t)axis[2] & 0xFFu) << 16) | (((uint32_t)cutoff & 0xFFu) << 24);
    }
}

} // namespace

void launch_tangent_sums(const float *positions, const float *uvs, const uint32_t *indices, uint32_t triangleCount, long long *sums, hipStream_t stream)
{
    if (triangleCount == 0) return;
    hipLaunchKernelGGL(tangent_sums_kernel, dim3((triangleCount + 255u) / 256u), dim3(256), 0, stream, positions, uvs, indices, triangleCount, sums);
}

void launch_pack_mesh(const PackMeshArgs &args, hipStream_t stream)
{
    if (args.vertexCount == 0) return;
    hipLaunchKernelGGL(pack_mesh_kernel, dim3((args.vertexCount + 255u) / 256u), dim3(256), 0, stream, args);
}

void launch_meshlet_bounds(const MeshletBoundsArgs &args, hipStream_t stream)
{
    if (args.meshletCount == 0) return;
    hipLaunchKernelGGL(meshlet_bounds_kernel, dim3(args.meshletCount), dim3(64), 0, stream, args);
}

} // namespace ppt
