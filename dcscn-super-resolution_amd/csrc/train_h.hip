// tconv_gemm_h, tpack_h and the exponent reduction of option "train_split16": see train_h.hpp for the arithmetic and the contract.
//
// tconv_gemm_h: workgroup = 4 waves x (32 pixels x 64 output channels) = 128 pixels x 64 channels; a wave holds 2 x 4 accumulator tiles
// and issues 2 x 4 x 3 MFMAs per k-chunk of 32.  Operand layout of v_mfma_f32_16x16x32_f16 (conv3_h.hpp, tools/gen_pipe_probe.py): lane l
// of A holds row l & 15, k = 8 (l >> 4) .. + 7; of B column l & 15, the same k; of C / D column l & 15, rows 4 (l >> 4) .. + 3.
//   A (pixels): every lane reads its 8 consecutive channels straight from the f32 tensor (two 16-byte loads where the slice is 16-byte
//     aligned, element loads otherwise), multiplies them by 2^e_a and splits them in registers (split16.hpp: 3 VALU per two values).  No
//     pre-split copy: it would be written and read once per step for a tensor that the f32 kernels (wgrad, activator) still read in f32.
//   B (filter): tpack_h's image is in fragment order, so a lane's operand is one contiguous 16-byte read, coalesced over the wave; the
//     four waves of a workgroup read the same fragments (L1 / L2 hits).
//   No LDS: with 64 output channels per workgroup an activation element is fetched from memory ceil(cout / 64) times (4 for the widest
//     layer), each fetch feeding 4 x 3 MFMAs; the k loop has no barrier and the waves of a SIMD hide each other's load latency.
#include "train_h.hpp"

#include "split16.hpp"

#pragma clang fp contract(off)

namespace dcscn_impl {
using namespace dcscn;

// 2^e for e in [-126, 126]: a normal f32
__device__ __forceinline__ float exp2i(int e) { return __uint_as_float((unsigned)(127 + e) << 23); }

// ---------------------------------------------------------------------------------------------
// exponent of a tensor: block b -> part[b] = max over its chunk of the bits of |v| (as integers: the order of non-negative floats; a NaN
// sorts above infinity); then e = 13 - floor(log2 max), clamped to [-126, 126] so that 2^e and 2^-e are normal; 0 for an all-zero tensor
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tabsmax_part(const float* v, int stride, int width, int64_t count, int64_t chunk, unsigned* part) {
    __shared__ unsigned red[256];
    const int64_t p0 = (int64_t)blockIdx.x * chunk;
    const int64_t p1 = p0 + chunk < count ? p0 + chunk : count;
    unsigned m = 0;
    // (row, column) of the thread's element, advanced by 256 elements per step without a division: 256 = dr * width + dc
    const int64_t e0 = p0 + threadIdx.x;
    int64_t row = e0 / width;
    int col = (int)(e0 - row * width);
    const int dr = 256 / width, dc = 256 - dr * width;
    for (int64_t e = e0; e < p1; e += 256) {
        const unsigned b = __float_as_uint(v[row * stride + col]) & 0x7fffffffu;
        m = b > m ? b : m;
        row += dr;
        col += dc;
        if (col >= width) { col -= width; ++row; }
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x + o] > red[threadIdx.x] ? red[threadIdx.x + o] : red[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void texp_final(const unsigned* part, int blocks, int* e) {
    __shared__ unsigned red[256];
    red[threadIdx.x] = (int)threadIdx.x < blocks ? part[threadIdx.x] : 0u;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x + o] > red[threadIdx.x] ? red[threadIdx.x + o] : red[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const unsigned m = red[0];
    int ex = 13 - ((int)(m >> 23) - 127);          // (a subnormal maximum has exponent field 0: clamped below)
    ex = ex > 126 ? 126 : ex < -126 ? -126 : ex;
    e[0] = m == 0u ? 0 : ex;
}

void launch_texp(const float* v, int stride, int width, int64_t rows, unsigned* part, int* e, hipStream_t st) {
    const int64_t count = rows * width;
    int64_t blocks = (count + 2047) / 2048;
    blocks = blocks < 1 ? 1 : blocks > kAbsMaxBlocks ? kAbsMaxBlocks : blocks;
    const int64_t chunk = (count + blocks - 1) / blocks;
    hipLaunchKernelGGL(tabsmax_part, dim3((unsigned)blocks), dim3(256), 0, st, v, stride, width, count, chunk, part);
    hipLaunchKernelGGL(texp_final, dim3(1), dim3(256), 0, st, (const unsigned*)part, (int)blocks, e);
}

// ---------------------------------------------------------------------------------------------
// filter images: one thread per (tap, k-chunk, column tile, lane) writes the lane's hi and lo fragments (8 halves each) of
//   blockIdx.y = 0: forward         B[k = ci][col = co] = w[tap][ci][co]
//   blockIdx.y = 1: data gradient   B[k = co][col = ci] = w[taps - 1 - tap][ci][co]
// times 2^e; zeros past the last channel / column
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tpack_h(const float* w, int taps, int cin, int cout, const int* e, h8* fwd, h8* dgrad) {
    const bool dg = blockIdx.y == 1;
    const int K = dg ? cout : cin, N = dg ? cin : cout;
    const int nkc = (K + 31) / 32, ntl = (N + 15) / 16;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= (int64_t)taps * nkc * ntl * 64) return;
    const int lane = (int)(u & 63);
    int64_t q = u >> 6;
    const int nt = (int)(q % ntl); q /= ntl;
    const int kc = (int)(q % nkc);
    const int tap = (int)(q / nkc);
    const int col = nt * 16 + (lane & 15), k0 = kc * 32 + 8 * (lane >> 4);
    const float scale = exp2i(e[0]);
    const int t = dg ? taps - 1 - tap : tap;
    h8 hi, lo;
    for (int j = 0; j < 8; ++j) {
        const int k = k0 + j;
        float v = 0.0f;
        if (k < K && col < N) {
            const int ci = dg ? col : k, co = dg ? k : col;
            v = w[((int64_t)t * cin + ci) * cout + co] * scale;
        }
        const _Float16 hj = (_Float16)v;
        hi[j] = hj;
        lo[j] = (_Float16)(v - (float)hj);
    }
    h8* img = dg ? dgrad : fwd;
    const int64_t base = (((int64_t)tap * nkc + kc) * ntl + nt) * 128 + lane;
    img[base] = hi;
    img[base + 64] = lo;
}

void launch_tpack_h(const float* w, int taps, int cin, int cout, const int* e, void* fwd, void* dgrad, hipStream_t st) {
    const int64_t units = (int64_t)taps * ((cin + 31) / 32) * ((cout + 15) / 16) * 64;
    const int64_t units_d = (int64_t)taps * ((cout + 31) / 32) * ((cin + 15) / 16) * 64;
    const int64_t most = dgrad && units_d > units ? units_d : units;
    hipLaunchKernelGGL(tpack_h, dim3((unsigned)((most + 255) / 256), dgrad ? 2 : 1), dim3(256), 0, st, w, taps, cin, cout, e, (h8*)fwd, (h8*)dgrad);
}

// ---------------------------------------------------------------------------------------------
// the conv
// ---------------------------------------------------------------------------------------------
template <int ACCUM>
__global__ __launch_bounds__(256) void tconv_gemm_h(const TConvHArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int64_t P = (int64_t)a.n * a.H * a.W;
    const int64_t r0 = (int64_t)blockIdx.x * 128 + wave * 32;
    const int nt0 = blockIdx.y * 4, c0 = nt0 * 16;
    const int nkc = (a.cin + 31) / 32, ntl = (a.cout + 15) / 16;
    const int pad = a.ks / 2;
    const int e_sum = a.e_in[0] + a.e_w[0];
    const float sa = exp2i(a.e_in[0]);
    const float m1 = opaque_minus_one();
    // 16-byte loads of a lane's 8 channels: the slice starts on a 16-byte boundary and every pixel does
    const bool vec = ((uintptr_t)a.in & 15) == 0 && (a.in_stride & 3) == 0;
    int py[2], px[2]; int64_t pimg[2]; bool pv[2];
    for (int mi = 0; mi < 2; ++mi) {
        const int64_t p = r0 + mi * 16 + lr;
        pv[mi] = p < P;
        const int64_t q = pv[mi] ? p : 0;
        px[mi] = (int)(q % a.W);
        py[mi] = (int)((q / a.W) % a.H);
        pimg[mi] = q / ((int64_t)a.W * a.H);
    }
    f32x4 acc[2][4];
    for (int mi = 0; mi < 2; ++mi)
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const h8* wimg = static_cast<const h8*>(a.w16) + (int64_t)nt0 * 128 + lane;
    for (int tap = 0; tap < a.ks * a.ks; ++tap) {
        const int kh = tap / a.ks, kw = tap - kh * a.ks;
        const float* src[2]; bool sv[2];
        for (int mi = 0; mi < 2; ++mi) {
            const int y = py[mi] + kh - pad, x = px[mi] + kw - pad;
            sv[mi] = pv[mi] && y >= 0 && y < a.H && x >= 0 && x < a.W;
            src[mi] = a.in + (sv[mi] ? ((pimg[mi] * a.H + y) * a.W + x) * a.in_stride : 0);
        }
        for (int kc = 0; kc < nkc; ++kc) {
            const int ci = kc * 32 + lk * 8;
            h8 xh[2], xl[2];
            for (int mi = 0; mi < 2; ++mi) {
                f32x4 v0 = {0.0f, 0.0f, 0.0f, 0.0f}, v1 = v0;
                if (sv[mi]) {
                    const float* s = src[mi] + ci;
                    if (vec && ci + 8 <= a.cin) {
                        v0 = *reinterpret_cast<const f32x4*>(s);
                        v1 = *reinterpret_cast<const f32x4*>(s + 4);
                    } else {
                        for (int j = 0; j < 4; ++j) {
                            if (ci + j < a.cin) v0[j] = s[j];
                            if (ci + 4 + j < a.cin) v1[j] = s[4 + j];
                        }
                    }
                }
                for (int j = 0; j < 4; ++j) { v0[j] = v0[j] * sa; v1[j] = v1[j] * sa; }
                split8(v0, v1, m1, xh[mi], xl[mi]);
            }
            const h8* wp = wimg + ((int64_t)tap * nkc + kc) * ntl * 128;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                if (nt0 + ni >= ntl) break;              // (uniform over the workgroup) no such column tile: the image ends here
                const h8 wh = wp[ni * 128], wl = wp[ni * 128 + 64];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl[mi], wh, acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[mi], wl, acc[mi][ni], 0, 0, 0);
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[mi], wh, acc[mi][ni], 0, 0, 0);
                }
            }
        }
    }
    for (int mi = 0; mi < 2; ++mi)
        for (int ni = 0; ni < 4; ++ni) {
            const int co = c0 + ni * 16 + lr;
            if (co >= a.cout) continue;
            const float b = a.bias ? a.bias[co] : 0.0f;
            for (int i = 0; i < 4; ++i) {
                const int64_t p = r0 + mi * 16 + lk * 4 + i;
                if (p >= P) continue;
                float* o = a.out + p * a.out_stride + co;
                const float v = ldexpf(acc[mi][ni][i], -e_sum) + b;
                *o = ACCUM ? *o + v : v;
            }
        }
}

void launch_tconv_gemm_h(const TConvHArgs& a, int accumulate, hipStream_t st) {
    const int64_t P = (int64_t)a.n * a.H * a.W;
    dim3 grid((unsigned)((P + 127) / 128), (unsigned)((a.cout + 63) / 64));
    if (accumulate) hipLaunchKernelGGL(tconv_gemm_h<1>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(tconv_gemm_h<0>, grid, dim3(256), 0, st, a);
}

}  // namespace dcscn_impl
