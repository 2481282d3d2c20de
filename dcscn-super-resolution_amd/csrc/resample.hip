// Bicubic resize bit-compatible with Pillow: single-channel float images (mode "F", below) and uint8 images of 1 or 3
// interleaved channels (modes "L" / "RGB", the 8-bpc section at the end of this file).
//
// Mode "F" (Image.resize(..., BICUBIC), libImaging/Resample.c: precompute_coeffs + ImagingResampleHorizontal_32bpc /
// ImagingResampleVertical_32bpc) is what the reference uses for the bicubic residual input x2 and for
// building LR images (helper/utilty.py:211-239 resize_image_by_pil, DCSCN.py:552-554, 682-683).
//
// Pillow: per output index a window [xmin, xmin + n) of input pixels and n <= ksize normalised float64 weights
// (a = -0.5 cubic, support 2 * max(1, in/out): antialiased when shrinking); horizontal pass into a float32
// image, then the vertical pass; each output is a float64 sum  ss += (double)pixel * k[i]  in window order,
// rounded once to float32.  The tables are built on the host with the same expressions; the kernels keep the
// summation order, and this translation unit is compiled with FP contraction OFF: hipcc's device default
// (-ffp-contract=fast) would fuse `ss + p * k` into an FMA -- HIP's __dmul_rn / __dadd_rn are plain * and + and
// do not prevent it -- while Pillow's x86-64 builds have no FMA; the difference is one float32 ulp on ~0.1 % of
// the pixels for non-dyadic scales (x3), none for x2 / x4.
#include <hip/hip_runtime.h>
#pragma clang fp contract(off)

#include <cmath>
#include <vector>

#include "kernels.h"

namespace dcscn {

namespace {

inline double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

}  // namespace

// precompute_coeffs(inSize, 0, inSize, outSize, BICUBIC): bounds[2 * xx] = first input index, [2 * xx + 1] = count
int resample_coeffs(int in_size, int out_size, std::vector<int>* bounds, std::vector<double>* kk) {
    const double in0 = 0.0, in1 = (double)in_size;
    double scale, filterscale;
    filterscale = scale = (in1 - in0) / out_size;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = 2.0 * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    bounds->assign((size_t)out_size * 2, 0);
    kk->assign((size_t)out_size * ksize, 0.0);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;
        double ww = 0.0;
        const double ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double* k = &(*kk)[(size_t)xx * ksize];
        for (int x = 0; x < xmax; ++x) {
            const double w = bicubic_filter((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x)
            if (ww != 0.0) k[x] /= ww;
        (*bounds)[(size_t)xx * 2] = xmin;
        (*bounds)[(size_t)xx * 2 + 1] = xmax;
    }
    return ksize;
}

// out[img][y][xx] = (float) sum_i (double) in[img][y][xmin + i] * k[xx][i]
__global__ __launch_bounds__(256) void resample_h_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                           const int* __restrict__ bounds, const double* __restrict__ kk,
                                                           int ksize, long long rows, int w, int ow) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * ow) return;
    const int xx = (int)(idx % ow);
    const long long row = idx / ow;
    const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
    const float* p = in + row * w + xmin;
    const double* k = kk + (size_t)xx * ksize;
    double ss = 0.0;
    for (int i = 0; i < n; ++i) ss += (double)p[i] * k[i];
    out[idx] = (float)ss;
}

// out[img][yy][x] = (float) sum_i (double) in[img][ymin + i][x] * k[yy][i]
__global__ __launch_bounds__(256) void resample_v_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                           const int* __restrict__ bounds, const double* __restrict__ kk,
                                                           int ksize, int n_img, int h, int oh, int w) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)n_img * oh * w) return;
    const int x = (int)(idx % w);
    const long long t = idx / w;
    const int yy = (int)(t % oh);
    const long long img = t / oh;
    const int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
    const float* p = in + (img * h + ymin) * w + x;
    const double* k = kk + (size_t)yy * ksize;
    double ss = 0.0;
    for (int i = 0; i < n; ++i) ss += (double)p[(size_t)i * w] * k[i];
    out[idx] = (float)ss;
}

hipError_t resample_h_launch(const float* in, float* out, const int* bounds, const double* kk, int ksize,
                             long long rows, int w, int ow, hipStream_t stream) {
    const long long total = rows * ow;
    hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, out, bounds, kk, ksize, rows, w, ow);
    return hipGetLastError();
}

hipError_t resample_v_launch(const float* in, float* out, const int* bounds, const double* kk, int ksize,
                             int n_img, int h, int oh, int w, hipStream_t stream) {
    const long long total = (long long)n_img * oh * w;
    hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, in, out, bounds, kk, ksize, n_img, h, oh, w);
    return hipGetLastError();
}

// ---- 8 bits per channel (Resample.c: normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc) -------
// Modes "L" and "RGB": the float64 weights become int32 fixed point with PRECISION_BITS = 32 - 8 - 2 = 22 fraction bits, each
// output byte is clip8((1 << 21 + sum_i in[i] * k8[i]) >> 22) in int32, and the horizontal pass writes a uint8 image that the
// vertical pass reads -- that rounding and clipping is part of the result.  Pillow's RGB resize is its "L" resize of each
// channel, so an image is handled as rows of W * C bytes: a lane produces the four consecutive bytes of one dword of the
// output, each byte with its own (row, pixel, channel), and stores the dword; the bytes in front of the first aligned address
// and behind the last one are stored one by one.

namespace {

constexpr int kPrecisionBits = 22;

__device__ __forceinline__ uint8_t clip8(int ss) {
    const int v = ss >> kPrecisionBits;
    return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// Byte `idx` of the horizontal pass: in [rows][w][c], out [rows][ow][c]
__device__ __forceinline__ uint8_t h8_byte(const uint8_t* __restrict__ in, const int* __restrict__ bounds, const int* __restrict__ kk,
                                           int ksize, int w, int ow, int c, long long idx) {
    const long long pix = idx / c;
    const int ch = (int)(idx - pix * c);
    const long long row = pix / ow;
    const int xx = (int)(pix - row * ow);
    const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
    const uint8_t* p = in + (row * w + xmin) * c + ch;
    const int* k = kk + (size_t)xx * ksize;
    int ss = 1 << (kPrecisionBits - 1);
    for (int i = 0; i < n; ++i) ss += (int)p[(size_t)i * c] * k[i];
    return clip8(ss);
}

// Byte `idx` of the vertical pass: in [n_img][h][wc], out [n_img][oh][wc] (wc = bytes of a row)
__device__ __forceinline__ uint8_t v8_byte(const uint8_t* __restrict__ in, const int* __restrict__ bounds, const int* __restrict__ kk,
                                           int ksize, int h, int oh, int wc, long long idx) {
    const long long t = idx / wc;
    const int x = (int)(idx - t * wc);
    const long long img = t / oh;
    const int yy = (int)(t - img * oh);
    const int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
    const uint8_t* p = in + (img * h + ymin) * wc + x;
    const int* k = kk + (size_t)yy * ksize;
    int ss = 1 << (kPrecisionBits - 1);
    for (int i = 0; i < n; ++i) ss += (int)p[(size_t)i * wc] * k[i];
    return clip8(ss);
}

// Lane g owns the bytes [4 g - head, 4 g - head + 4) of the output, head = out & 3: a dword at an aligned address, or -- in
// the first and the last lane -- the part of it inside [0, total), stored bytewise.
template <class Byte>
__device__ __forceinline__ void store_quad(uint8_t* __restrict__ out, long long total, const Byte& byte) {
    const int head = (int)(reinterpret_cast<uintptr_t>(out) & 3);
    const long long first = ((long long)blockIdx.x * 256 + threadIdx.x) * 4 - head;
    if (first >= total) return;
    if (first >= 0 && first + 4 <= total) {
        const uint32_t b0 = byte(first), b1 = byte(first + 1), b2 = byte(first + 2), b3 = byte(first + 3);
        *reinterpret_cast<uint32_t*>(out + first) = b0 | b1 << 8 | b2 << 16 | b3 << 24;
        return;
    }
    for (long long i = first < 0 ? 0 : first; i < first + 4 && i < total; ++i) out[i] = byte(i);
}

__global__ __launch_bounds__(256) void resample_h8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                          const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                          long long rows, int w, int ow, int c) {
    store_quad(out, rows * ow * c, [&](long long idx) { return h8_byte(in, bounds, kk, ksize, w, ow, c, idx); });
}

__global__ __launch_bounds__(256) void resample_v8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                          const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                          int n_img, int h, int oh, int wc) {
    store_quad(out, (long long)n_img * oh * wc, [&](long long idx) { return v8_byte(in, bounds, kk, ksize, h, oh, wc, idx); });
}

// one lane per dword the output touches (one more than total / 4 when it starts or ends inside a dword)
inline unsigned quad_blocks(const uint8_t* out, long long total) {
    const long long lanes = (total + (long long)(reinterpret_cast<uintptr_t>(out) & 3) + 3) / 4;
    return (unsigned)((lanes + 255) / 256);
}

}  // namespace

// normalize_coeffs_8bpc: round half away from zero at 22 fraction bits
int resample_coeffs8(int in_size, int out_size, std::vector<int>* bounds, std::vector<int>* k8) {
    std::vector<double> kk;
    const int ksize = resample_coeffs(in_size, out_size, bounds, &kk);
    k8->resize(kk.size());
    for (size_t i = 0; i < kk.size(); ++i)
        (*k8)[i] = kk[i] < 0 ? (int)(-0.5 + kk[i] * (1 << kPrecisionBits)) : (int)(0.5 + kk[i] * (1 << kPrecisionBits));
    return ksize;
}

hipError_t resample_h8_launch(const uint8_t* in, uint8_t* out, const int* bounds, const int* k8, int ksize, long long rows, int w, int ow,
                              int c, hipStream_t stream) {
    const long long total = rows * ow * c;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(resample_h8_kernel, dim3(quad_blocks(out, total)), dim3(256), 0, stream, in, out, bounds, k8, ksize, rows, w, ow, c);
    return hipGetLastError();
}

hipError_t resample_v8_launch(const uint8_t* in, uint8_t* out, const int* bounds, const int* k8, int ksize, int n_img, int h, int oh,
                              int wc, hipStream_t stream) {
    const long long total = (long long)n_img * oh * wc;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(resample_v8_kernel, dim3(quad_blocks(out, total)), dim3(256), 0, stream, in, out, bounds, k8, ksize, n_img, h, oh, wc);
    return hipGetLastError();
}

}  // namespace dcscn
