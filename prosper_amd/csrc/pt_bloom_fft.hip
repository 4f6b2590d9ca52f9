// pt_bloom_fft.hip — gfx950 kernels of bloom's FFT technique (src/render/bloom/{GenerateKernel,Fft,Convolution}.cpp,
// res/shader/bloom/{generate_kernel,prepare_kernel,fft,convolution}.comp).
//
//   bloom_fft_generate_kernel   generate_kernel.comp: the 8 x 8 supersampled filter, in double precision
//   bloom_fft_prepare_kernel    prepare_kernel.comp: the centred kernel wrapped round the corners of the dim x dim image
//   bloom_fft_rows_kernel       every radix stage of whole rows between registers and LDS: one read, one write
//   bloom_fft_columns_kernel    the same over a tile of adjacent columns
//   bloom_fft_middle_kernel     forward columns, the convolution and inverse columns of a tile in one launch
//
// prosper's fft.comp is a Stockham schedule whose every radix pass goes through global memory.  Here a workgroup holds
// kTileTexels texels (64 KB) of whole lines in LDS - 16 rows of 256 texels ... one row of 4096, or as many adjacent
// columns - and runs radix-4 Stockham stages (and a last radix-2 one where log2(dim) is odd) over them: a stage reads
// its butterflies' inputs into registers, the workgroup meets, the stage writes them back where the next one reads.
// The twiddles come from a table of e^{-2 pi i k / dim} made on the host in double precision.
#include "pt_bloom_fft.hpp"

#include <cmath>
#include <vector>

#include "pt_device.hpp"

namespace ppt
{

namespace bloom_fft
{

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTileTexels = 4096;                     // of one workgroup: 64 KB of float4
constexpr uint32_t kLoads = kTileTexels / kThreads;        // texels a lane loads and stores
constexpr uint32_t kRadix4 = kTileTexels / 4u / kThreads;  // radix-4 butterflies of a lane per stage
constexpr uint32_t kRadix2 = kTileTexels / 2u / kThreads;  // radix-2 butterflies of a lane

// ---- generate_kernel ----

// The constants of generate_kernel.comp as written: math.glsl's PI, and sdStar's own
constexpr double kPi = 3.14159265;
constexpr double kStarPi = 3.1415927;

PPT_D double gaussian(double x, double a, double b, double c) { return a * exp(-(x - b * b) / (2.0 * c * c)); }

// iq's signed distance to an n-star polygon (generate_kernel.comp:22-45)
PPT_D double sd_star(double px, double py, double r, double n, double w)
{
    const double m = n + w * (2.0 - n);
    const double an = kStarPi / n, en = kStarPi / m;
    const double racsX = r * cos(an), racsY = r * sin(an);
    const double ecsX = cos(en), ecsY = sin(en);
    px = fabs(px);
    const double at = atan2(px, py), period = 2.0 * an;
    const double bn = (at - period * floor(at / period)) - an;
    const double len = sqrt(px * px + py * py);
    double qx = len * cos(bn), qy = len * fabs(sin(bn));
    qx -= racsX;
    qy -= racsY;
    double t = -(qx * ecsX + qy * ecsY);
    const double hi = racsY / ecsY;
    t = t < 0.0 ? 0.0 : (t > hi ? hi : t);
    qx += ecsX * t;
    qy += ecsY * t;
    const double sign = qx > 0.0 ? 1.0 : (qx < 0.0 ? -1.0 : 0.0);
    return sqrt(qx * qx + qy * qy) * sign;
}

// filterValue: .r = .g is `rg`, .b = .a is `ba`
PPT_D void filter_value(double px, double py, double &rg, double &ba)
{
    const double a = 1.5, c = 0.055;
    const double len = sqrt(px * px + py * py);
    const double g = gaussian(len, a, 0.0, c);
    rg = ba = g;
    double d = sd_star(px, py, 0.5, 4.0, 0.075);
    const double angle = kPi / 4.0;
    const double rx = cos(angle) * px + sin(angle) * py, ry = cos(angle) * py - sin(angle) * px; // pR
    const double d2 = sd_star(rx, ry, 0.35, 4.0, 0.05);
    d = d2 < d ? d2 : d;
    if (d < 0.0)
    {
        rg += g;
        ba += g;
    }
    if (fabs(py) < 0.005)
    {
        double t = fabs(px) * 6.0;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const double mixRg = 0.05 * (1.0 - t) + 0.01 * t, mixBa = 1.0 * (1.0 - t) + 1.0 * t;
        const double wave = (fabs(sin(px * 50.0)) + fabs(cos(px * 95.0))) + fabs(sin(px * 75.0));
        const double streak = gaussian(fabs(px) * 10.0, 0.5, 1.0, 1.0);
        rg += ((0.5 * mixRg) * wave) * streak;
        ba += ((0.5 * mixBa) * wave) * streak;
    }
}

// One wave per texel, one lane per sub-sample (i, j) = (lane & 7, lane >> 3); the 64 values are summed over the lanes in a
// fixed tree.  p = ((8 xy + (i, j) + .5) / (8 kernelDim)) 2 - 1.
__global__ __launch_bounds__(256) void bloom_fft_generate_kernel(uint32_t kernelDim, float4 *__restrict__ kernelImage)
{
    const uint32_t texels = kernelDim * kernelDim;
    const uint32_t texel = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t t = texel < texels ? texel : texels - 1u; // (every lane takes part in the sum)
    const uint32_t x = t % kernelDim, y = t / kernelDim;
    const double size = 8.0 * (double)kernelDim;
    const double px = (((double)(8u * x + (lane & 7u)) + 0.5) / size) * 2.0 - 1.0;
    const double py = (((double)(8u * y + (lane >> 3)) + 0.5) / size) * 2.0 - 1.0;
    double rg, ba;
    filter_value(px, py, rg, ba);
#pragma unroll
    for (int32_t step = 1; step < 64; step <<= 1)
    {
        rg += __shfl_xor(rg, step);
        ba += __shfl_xor(ba, step);
    }
    if (lane == 0u && texel < texels)
    {
        const float r = (float)(rg / 64.0), b = (float)(ba / 64.0);
        kernelImage[texel] = make_float4(r, r, b, b);
    }
}

// ---- prepare_kernel ----

// pIn = pOut + kernelDim / 2 below dim / 2 and pOut + (kernelDim - 2 dim) / 2 from there on, in halves: twice pIn is an
// integer.  Inside while 0 <= pIn < kernelDim; ivec2(pIn) truncates.
PPT_D bool prepare_source(uint32_t pOut, uint32_t kernelDim, uint32_t dim, uint32_t &pIn)
{
    const int32_t twice = 2 * (int32_t)pOut + (int32_t)kernelDim - (2u * pOut >= dim ? 2 * (int32_t)dim : 0);
    if (twice < 0 || twice >= 2 * (int32_t)kernelDim) return false;
    pIn = (uint32_t)twice >> 1;
    return true;
}

__global__ __launch_bounds__(256) void bloom_fft_prepare_kernel(
    uint32_t kernelDim, uint32_t dim, const float4 *__restrict__ kernelImage, float4 *__restrict__ out)
{
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= dim || y >= dim) return;
    uint32_t sx, sy;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (prepare_source(x, kernelDim, dim, sx) && prepare_source(y, kernelDim, dim, sy))
    {
        const float4 k = kernelImage[(size_t)sy * kernelDim + sx];
        v = make_float4(k.x, 0.0f, k.z, 0.0f);
    }
    out[(size_t)y * dim + x] = v;
}

// ---- the transform ----

PPT_D float4 mul_complex(float4 a, float2 w)
{
    return make_float4(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x, a.z * w.x - a.w * w.y, a.z * w.y + a.w * w.x);
}
PPT_D float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
PPT_D float4 sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
PPT_D float4 swap_re_im(float4 a) { return make_float4(a.y, a.x, a.w, a.z); }

// Where texel `idx` of line `line` lives in LDS.  A stage reads consecutive texels on consecutive lanes, which is
// conflict-free as it stands (ds_read_b128: 16 lanes over the 16 slots of a 256-byte bank row), but the first stages
// write with a stride of 4 and 16 texels: 8 lanes of a ds_write_b128 group would share 2 of its 8 slots.  XOR-ing the
// low two bits with the next two spreads them over 4 and permutes texels only inside aligned groups of 4, which the
// reads do not notice.  The column kernel moves line l by l * kRotate slots so that the 8 lanes of a transposed store,
// which hold the same rows of adjacent columns, do not meet on one slot either.
template <uint32_t N, uint32_t kRotate>
PPT_D uint32_t lds_at(uint32_t line, uint32_t idx)
{
    const uint32_t s = idx ^ ((idx >> 2) & 3u);
    return line * N + ((s + line * kRotate) & (N - 1u));
}

// The forward DFT of the kTileTexels / N lines of N texels in `lds`, unnormalised, in place and in natural order.
// fft.comp's iteration: butterfly j of a stage with Ns done reads j + r N / R, multiplies by w^(r (j % Ns)) with
// w = e^{-2 pi i / (Ns R)}, and writes (j / Ns) Ns R + j % Ns + r Ns.  Ends with the workgroup met.
template <uint32_t N, uint32_t kRotate>
PPT_D void fft_lines(float4 *lds, const float2 *__restrict__ twiddles, uint32_t tid)
{
    constexpr uint32_t kQuarter = N / 4u, kHalf = N / 2u;
    uint32_t ns = 1u;
    for (; ns * 4u <= N; ns *= 4u)
    {
        float4 v[kRadix4][4];
#pragma unroll
        for (uint32_t k = 0; k < kRadix4; ++k)
        {
            const uint32_t b = tid + k * kThreads, line = b / kQuarter, j = b & (kQuarter - 1u);
#pragma unroll
            for (uint32_t r = 0; r < 4u; ++r) v[k][r] = lds[lds_at<N, kRotate>(line, j + r * kQuarter)];
            if (ns > 1u)
            {
                const uint32_t m = (j & (ns - 1u)) * (kQuarter / ns); // below N / 4
                v[k][1] = mul_complex(v[k][1], twiddles[m]);
                v[k][2] = mul_complex(v[k][2], twiddles[2u * m]);
                v[k][3] = mul_complex(v[k][3], twiddles[3u * m]);
            }
            // fftButterflyRadix4
            const float4 t0 = add4(v[k][0], v[k][2]), t2 = sub4(v[k][0], v[k][2]), t1 = add4(v[k][1], v[k][3]);
            const float4 d = sub4(v[k][1], v[k][3]);
            const float4 t3 = make_float4(d.y, -d.x, d.w, -d.z); // -i d
            v[k][0] = add4(t0, t1);
            v[k][2] = sub4(t0, t1);
            v[k][1] = add4(t2, t3);
            v[k][3] = sub4(t2, t3);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kRadix4; ++k)
        {
            const uint32_t b = tid + k * kThreads, line = b / kQuarter, j = b & (kQuarter - 1u);
            const uint32_t dst = ((j & ~(ns - 1u)) << 2) | (j & (ns - 1u));
#pragma unroll
            for (uint32_t r = 0; r < 4u; ++r) lds[lds_at<N, kRotate>(line, dst + r * ns)] = v[k][r];
        }
        __syncthreads();
    }
    if (ns < N)
    {
        // the last stage, radix 2 with Ns = N / 2: butterfly j reads and writes j and j + N / 2, so no lane waits for another
#pragma unroll
        for (uint32_t k = 0; k < kRadix2; ++k)
        {
            const uint32_t b = tid + k * kThreads, line = b / kHalf, j = b & (kHalf - 1u);
            const uint32_t i0 = lds_at<N, kRotate>(line, j), i1 = lds_at<N, kRotate>(line, j + kHalf);
            const float4 a = lds[i0], c = mul_complex(lds[i1], twiddles[j]);
            lds[i0] = add4(a, c);
            lds[i1] = sub4(a, c);
        }
        __syncthreads();
    }
}

PPT_D float4 load_texel(const float4 *in, size_t i) { return in[i]; }
PPT_D float4 load_texel(const uint2 *in, size_t i)
{
    const uint2 p = in[i];
    return make_float4(half_to_float(p.x & 0xFFFFu), half_to_float(p.x >> 16), half_to_float(p.y & 0xFFFFu), half_to_float(p.y >> 16));
}
PPT_D float4 scaled(float4 v, float s) { return make_float4(v.x * s, v.y * s, v.z * s, v.w * s); }
// convolution.comp: mulComplex(h, f) * scale per channel pair
PPT_D float4 multiply_scaled(float4 h, float4 f, float scale)
{
    return make_float4((h.x * f.x - h.y * f.y) * scale, (h.x * f.y + h.y * f.x) * scale, (h.z * f.z - h.w * f.w) * scale,
                       (h.z * f.w + h.w * f.z) * scale);
}

// kTileTexels / N whole rows per workgroup: the tile is kTileTexels consecutive texels of the image.  The inverse swaps
// re and im on the way in and out (fft.comp's INVERSE).  `in` may be `out`: a workgroup reads all it writes first.
template <uint32_t N, bool kInverse, class In>
__global__ __launch_bounds__(256) void bloom_fft_rows_kernel(const In *in, float4 *out, const float2 *__restrict__ twiddles, float scale)
{
    __shared__ float4 lds[kTileTexels];
    const uint32_t tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * kTileTexels;
#pragma unroll
    for (uint32_t k = 0; k < kLoads; ++k)
    {
        const uint32_t e = tid + k * kThreads;
        const float4 v = load_texel(in, base + e);
        lds[lds_at<N, 0u>(e / N, e & (N - 1u))] = kInverse ? swap_re_im(v) : v;
    }
    __syncthreads();
    fft_lines<N, 0u>(lds, twiddles, tid);
#pragma unroll
    for (uint32_t k = 0; k < kLoads; ++k)
    {
        const uint32_t e = tid + k * kThreads;
        const float4 v = scaled(lds[lds_at<N, 0u>(e / N, e & (N - 1u))], scale);
        out[base + e] = kInverse ? swap_re_im(v) : v;
    }
}

// kTileTexels / N adjacent columns per workgroup, so a row of the tile is one contiguous segment of that many texels.
template <uint32_t N, bool kInverse>
__global__ __launch_bounds__(256) void bloom_fft_columns_kernel(const float4 *in, float4 *out, const float2 *__restrict__ twiddles, float scale)
{
    constexpr uint32_t kColumns = kTileTexels / N;
    constexpr uint32_t kRotate = kColumns >= 8u ? 1u : 8u / kColumns;
    __shared__ float4 lds[kTileTexels];
    const uint32_t tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * kColumns;
#pragma unroll
    for (uint32_t k = 0; k < kLoads; ++k)
    {
        const uint32_t e = tid + k * kThreads, row = e / kColumns, column = e & (kColumns - 1u);
        const float4 v = in[base + (size_t)row * N + column];
        lds[lds_at<N, kRotate>(column, row)] = kInverse ? swap_re_im(v) : v;
    }
    __syncthreads();
    fft_lines<N, kRotate>(lds, twiddles, tid);
#pragma unroll
    for (uint32_t k = 0; k < kLoads; ++k)
    {
        const uint32_t e = tid + k * kThreads, row = e / kColumns, column = e & (kColumns - 1u);
        const float4 v = scaled(lds[lds_at<N, kRotate>(column, row)], scale);
        out[base + (size_t)row * N + column] = kInverse ? swap_re_im(v) : v;
    }
}

// The middle of the pass in one launch: the forward columns, convolution.comp and the inverse columns over a tile of
// adjacent columns, with the same operations in the same order as the three launches, so the bytes are theirs.
template <uint32_t N>
__global__ __launch_bounds__(256) void bloom_fft_middle_kernel(
    float4 *image, const float4 *__restrict__ kernelDft, const float2 *__restrict__ twiddles, float convolutionScale)
{
    constexpr uint32_t kColumns = kTileTexels / N;
    constexpr uint32_t kRotate = kColumns >= 8u ? 1u : 8u / kColumns;
    __shared__ float4 lds[kTileTexels];
    const uint32_t tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * kColumns;
#pragma unroll
    for (uint32_t k = 0; k < kLoads; ++k)
    {
        const uint32_t e = tid + k * kThreads, row = e / kColumns, column = e & (kColumns - 1u);
        lds[lds_at<N, kRotate>(column, row)] = image[base + (size_t)row * N + column];
    }
    __syncthreads();
    fft_lines<N, kRotate>(lds, twiddles, tid);
#pragma unroll
    for (uint32_t k = 0; k < kLoads; ++k)
    {
        const uint32_t e = tid + k * kThreads, row = e / kColumns, column = e & (kColumns - 1u);
        const uint32_t at = lds_at<N, kRotate>(column, row);
        const float4 h = scaled(lds[at], 1.0f / (float)N), f = kernelDft[base + (size_t)row * N + column];
        lds[at] = swap_re_im(multiply_scaled(h, f, convolutionScale)); // (each lane rewrites the texels it read)
    }
    __syncthreads();
    fft_lines<N, kRotate>(lds, twiddles, tid);
#pragma unroll
    for (uint32_t k = 0; k < kLoads; ++k)
    {
        const uint32_t e = tid + k * kThreads, row = e / kColumns, column = e & (kColumns - 1u);
        image[base + (size_t)row * N + column] = swap_re_im(lds[lds_at<N, kRotate>(column, row)]);
    }
}

template <uint32_t N>
void launch_rows(bool inverse, const void *in, bool inHalf, float4 *out, const float2 *tw, hipStream_t s)
{
    const dim3 grid(N * N / kTileTexels), block(kThreads);
    if (inverse)
        hipLaunchKernelGGL((bloom_fft_rows_kernel<N, true, float4>), grid, block, 0, s, static_cast<const float4 *>(in), out, tw, 1.0f);
    else if (inHalf)
        hipLaunchKernelGGL((bloom_fft_rows_kernel<N, false, uint2>), grid, block, 0, s, static_cast<const uint2 *>(in), out, tw, 1.0f);
    else
        hipLaunchKernelGGL((bloom_fft_rows_kernel<N, false, float4>), grid, block, 0, s, static_cast<const float4 *>(in), out, tw, 1.0f);
}

template <uint32_t N>
void launch_columns(bool inverse, const float4 *in, float4 *out, const float2 *tw, hipStream_t s)
{
    const dim3 grid(N * N / kTileTexels), block(kThreads);
    if (inverse)
        hipLaunchKernelGGL((bloom_fft_columns_kernel<N, true>), grid, block, 0, s, in, out, tw, 1.0f);
    else
        hipLaunchKernelGGL((bloom_fft_columns_kernel<N, false>), grid, block, 0, s, in, out, tw, 1.0f / (float)N);
}

template <uint32_t N>
void launch_middle(float4 *image, const float4 *kernelDft, const float2 *tw, float convolutionScale, hipStream_t s)
{
    hipLaunchKernelGGL((bloom_fft_middle_kernel<N>), dim3(N * N / kTileTexels), dim3(kThreads), 0, s, image, kernelDft, tw, convolutionScale);
}

} // namespace bloom_fft

using namespace bloom_fft;

bool bloom_fft_plan(uint32_t width, uint32_t height, uint32_t resolutionScale, BloomFftPlan &plan)
{
    if (resolutionScale > 1u || width == 0u || height == 0u) return false;
    const uint32_t scale = resolutionScale == 0u ? 2u : 4u;
    const uint32_t largest = width > height ? width : height;
    if (width / scale == 0u || height / scale == 0u || largest > 2u * kBloomFftMaxDim) return false;
    uint32_t ceil = 1u;
    while (ceil < largest) ceil <<= 1;
    plan.scale = scale;
    plan.dim = ceil / scale > kBloomFftMinDim ? ceil / scale : kBloomFftMinDim; // Separate.cpp:98-101
    plan.kernelDim = height / scale;                                           // GenerateKernel.cpp:81
    plan.convolutionScale = 2.0f / (float)plan.kernelDim;                      // GenerateKernel::convolutionScale
    if (resolutionScale == 1u) plan.convolutionScale *= 2.0f;                  // Bloom.cpp:95-98
    return true;
}

void bloom_fft_twiddles(uint32_t dim, float *out)
{
    for (uint32_t k = 0; k < dim; ++k)
    {
        const double angle = -2.0 * M_PI * (double)k / (double)dim;
        out[2u * k] = (float)std::cos(angle);
        out[2u * k + 1u] = (float)std::sin(angle);
    }
}

void launch_bloom_fft_generate_kernel(uint32_t kernelDim, float4 *kernelImage, hipStream_t stream)
{
    hipLaunchKernelGGL(bloom_fft_generate_kernel, dim3((kernelDim * kernelDim + 3u) / 4u), dim3(256), 0, stream, kernelDim, kernelImage);
}

void launch_bloom_fft_prepare_kernel(uint32_t kernelDim, uint32_t dim, const float4 *kernelImage, float4 *out, hipStream_t stream)
{
    hipLaunchKernelGGL(bloom_fft_prepare_kernel, dim3(dim / 64u, dim / 4u), dim3(256), 0, stream, kernelDim, dim, kernelImage, out);
}

void launch_bloom_fft_rows(uint32_t dim, bool inverse, const void *in, bool inHalf, float4 *out, const float2 *twiddles, hipStream_t stream)
{
    switch (dim)
    {
    case 256u: return launch_rows<256u>(inverse, in, inHalf, out, twiddles, stream);
    case 512u: return launch_rows<512u>(inverse, in, inHalf, out, twiddles, stream);
    case 1024u: return launch_rows<1024u>(inverse, in, inHalf, out, twiddles, stream);
    case 2048u: return launch_rows<2048u>(inverse, in, inHalf, out, twiddles, stream);
    case 4096u: return launch_rows<4096u>(inverse, in, inHalf, out, twiddles, stream);
    }
}

void launch_bloom_fft_columns(uint32_t dim, bool inverse, const float4 *in, float4 *out, const float2 *twiddles, hipStream_t stream)
{
    switch (dim)
    {
    case 256u: return launch_columns<256u>(inverse, in, out, twiddles, stream);
    case 512u: return launch_columns<512u>(inverse, in, out, twiddles, stream);
    case 1024u: return launch_columns<1024u>(inverse, in, out, twiddles, stream);
    case 2048u: return launch_columns<2048u>(inverse, in, out, twiddles, stream);
    case 4096u: return launch_columns<4096u>(inverse, in, out, twiddles, stream);
    }
}

void launch_bloom_fft_middle(uint32_t dim, float4 *image, const float4 *kernelDft, const float2 *twiddles, float scale, hipStream_t stream)
{
    switch (dim)
    {
    case 256u: return launch_middle<256u>(image, kernelDft, twiddles, scale, stream);
    case 512u: return launch_middle<512u>(image, kernelDft, twiddles, scale, stream);
    case 1024u: return launch_middle<1024u>(image, kernelDft, twiddles, scale, stream);
    case 2048u: return launch_middle<2048u>(image, kernelDft, twiddles, scale, stream);
    case 4096u: return launch_middle<4096u>(image, kernelDft, twiddles, scale, stream);
    }
}

} // namespace ppt
