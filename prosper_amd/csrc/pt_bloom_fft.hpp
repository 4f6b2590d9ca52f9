// pt_bloom_fft.hpp — host-callable launchers of the gfx950 kernels of bloom's FFT technique (pt_bloom_fft.hip;
// src/render/bloom/{GenerateKernel,Fft,Convolution}.cpp, res/shader/bloom/{generate_kernel,prepare_kernel,fft,
// convolution}.comp).  Separate and compose: pt_bloom.hpp.  C entry points: pt_bloom_passes.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace ppt
{

constexpr uint32_t kBloomFftMinDim = 256;  // Fft::sMinResolution
constexpr uint32_t kBloomFftMaxDim = 4096; // a line of 4096 texels is the 64 KB of LDS a workgroup holds
constexpr uint32_t kBloomFftStages = 8;    // separate, generate, prepare, the kernel's FFT, forward FFT, convolution, inverse FFT, compose

// What one call works on: the transform is dim x dim, the kernel image kernelDim x kernelDim.
struct BloomFftPlan
{
    uint32_t scale;     // 2 (Half) or 4 (Quarter)
    uint32_t dim;       // max(bit_ceil(max(width, height)) / scale, 256)
    uint32_t kernelDim; // height / scale
    float convolutionScale;
};
// false for an extent the technique does not take: empty, width / scale or height / scale 0, max(width, height) above 8192
bool bloom_fft_plan(uint32_t width, uint32_t height, uint32_t resolutionScale, BloomFftPlan &plan);
inline bool bloom_fft_is_dim(uint32_t dim) { return dim >= kBloomFftMinDim && dim <= kBloomFftMaxDim && (dim & (dim - 1u)) == 0u; }

// e^{-2 pi i k / dim}, k = 0 .. dim - 1, as (cos, sin) pairs: made in double precision and rounded once to float32
void bloom_fft_twiddles(uint32_t dim, float *out);

// generate_kernel.comp over kernelDim x kernelDim RGBA32F, evaluated in double precision and stored as float32
void launch_bloom_fft_generate_kernel(uint32_t kernelDim, float4 *kernelImage, hipStream_t stream);
// prepare_kernel.comp: the centred kernel image wrapped round the corners of a dim x dim RGBA32F image, .g = .a = 0
void launch_bloom_fft_prepare_kernel(uint32_t kernelDim, uint32_t dim, const float4 *kernelImage, float4 *out, hipStream_t stream);
// One dimension of a transform of a dim x dim image whose texel holds the complex numbers r + i g and b + i a.  `in` is
// RGBA16F when `inHalf` (forward rows only) and RGBA32F otherwise; `in` may be `out`.  The forward rows are unscaled and
// the forward columns divide by dim, so rows then columns is the DFT divided by dim; the inverse is unnormalised.
void launch_bloom_fft_rows(uint32_t dim, bool inverse, const void *in, bool inHalf, float4 *out, const float2 *twiddles, hipStream_t stream);
void launch_bloom_fft_columns(uint32_t dim, bool inverse, const float4 *in, float4 *out, const float2 *twiddles, hipStream_t stream);
// The forward columns, the convolution with `kernelDft` and the inverse columns of `image` in one launch
// (convolution.comp: mulComplex(a, k) * scale per channel pair): the bytes of the forward columns, a multiply pass and
// the inverse columns, with one read and one write of the image instead of three
void launch_bloom_fft_middle(uint32_t dim, float4 *image, const float4 *kernelDft, const float2 *twiddles, float scale, hipStream_t stream);

} // namespace ppt
