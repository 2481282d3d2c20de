// Option "train_split16" (include/dcscn.h): the forward and data-gradient convs of the training plan on v_mfma_f32_16x16x32_f16 at f32
// accuracy -- split16.hpp's three products wh*xh + wh*xl + wl*xh per k-chunk of 32, accumulated in f32.  Unlike the inference split, EVERY
// operand is scaled by a power of two before it is split: the layer's input slice (forward), dz (data gradient) and the filter.  The scale
// 2^e puts the tensor's max-abs into [2^13, 2^14), so the lo pieces of all but vanishing elements are normal f16 numbers whatever the
// tensor's magnitude (dz of an MSE loss is 1e-4 and below: unscaled, its lo pieces would all be subnormal) and no operand can leave the f16
// range: the mode has no redo flags and no float32 fallback.  e is computed on the device (tabsmax_part + texp_final: a max is
// order-independent, no atomics) and read from device memory by the consumers; the epilogue multiplies by 2^-(e_a + e_w) with ldexpf
// (exact).  A non-finite input gives a non-finite result, as on the f32 path.
//
// The contract is tconv_gemm's (train_kernels.hpp): SAME padding, stride 1, k order tap-major then channel-minor in chunks of 32 (a tap's channels
// are padded to a multiple of 32 with zeros), bias added after the chain (ACCUM = 0) or out += result (ACCUM = 1), arbitrary in_stride /
// out_stride slices, ragged pixel and channel counts masked to zero.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace dcscn_impl {

struct TConvHArgs {
    const float* in; int in_stride; int cin;
    int n, H, W, ks;
    const void* w16;           // tpack_h image of the filter: [tap][k-chunk][16-column tile][hi | lo][64 lanes][8 halves]
    int cout;
    const float* bias;
    float* out; int out_stride;
    const int* e_in;           // exponent of the input's scale (device memory)
    const int* e_w;            // ... of the filter's
};

constexpr int kAbsMaxBlocks = 256;   // partial maxima of one tensor (texp_final reads them all)

// shape alone, and symmetric: the data gradient is the same conv with cin and cout swapped
inline bool tconv_h_eligible(int cin, int cout) { return (cin < cout ? cin : cout) >= 16; }
// bytes of one filter image with K = cin (forward) or cout (data gradient) contraction channels and N columns
inline size_t tpack_h_bytes(int taps, int k, int n) { return (size_t)taps * ((k + 31) / 32) * ((n + 15) / 16) * 2048; }

// e[0] = the exponent that puts max|v| over `rows` rows of `width` floats, `stride` apart, into [2^13, 2^14); part: kAbsMaxBlocks words
void launch_texp(const float* v, int stride, int width, int64_t rows, unsigned* part, int* e, hipStream_t st);
// the scaled (hi | lo) images of w [taps][cin][cout]: fwd (K = cin, N = cout) and, unless null, dgrad (flipped in space, K = cout, N = cin)
void launch_tpack_h(const float* w, int taps, int cin, int cout, const int* e, void* fwd, void* dgrad, hipStream_t st);
void launch_tconv_gemm_h(const TConvHArgs& a, int accumulate, hipStream_t st);

}  // namespace dcscn_impl
