// tconv_wgrad_h of option "train_split16_wgrad": see train_wgrad_h.hpp for the arithmetic, the contract and the partition.
//
// The contraction index of a weight gradient is the pixel, and both tensors are pixel-major, channel-minor: a lane's 8 k-values of
// v_mfma_f32_16x16x32_f16 are 8 pixels of ONE channel.  So both operands go through LDS as [position][channel] f16 images, written once per
// tile with coalesced loads (scaled and split into hi | lo there), and are read back with ds_read_b64_tr_b16, which hands lane i of a
// 16-lane group column i of a block of 4 positions x 16 channels.
//
// A tile is tr rows x tc columns of one image.  Its LDS positions are laid out with the SAME row pitch tcp = tc + ks - 1 for both images:
//   input   position (r, c), r < tr + ks - 1, c < tcp   = pixel (y0 - pad + r, x0 - pad + c), zero outside the image
//   dz      position (r, c), r < tr,          c < tcp   = pixel (y0 + r, x0 + c), zero for c >= tc, outside the image, and up to kpad
// so that the input pixel of dz position q under tap (kh, kw) is input position q + kh * tcp + kw: a tap is a different row address and
// nothing else, borders and ragged tiles are zeros of the staged images, and the k loop has no mask and no branch.  (A dz position in the
// halo columns meets an input position of the neighbouring row: dz is zero there.)  Every LDS address is in bounds by construction: the dz
// image has kpad positions, the input image in_cap >= kpad + (ks - 1) * (tcp + 1), and reads go up to q = kpad - 1.
//
// Workgroup = 4 waves = a block of 64 input channels x 64 columns x TG taps of the gradient over the tiles of one split; wave w holds
// channels 16 w .. + 15 against all 64 columns: TG x 4 accumulator tiles (144 VGPRs for a 3x3).  Per k-chunk of 32 positions a wave reads
// the 4 dz fragments once and, per tap, one input fragment that feeds 4 x 3 MFMAs.  The staged input tile serves every tap and the dz
// tile every wave.  Waves and column tiles past the layer's channels skip the chunk (wave-uniform: EXEC stays all ones at the reads).
//
// k order within a chunk: the MFMA's k = 8 g + j (g = lane >> 4) is position 4 g + j for j < 4 and 16 + 4 g + (j - 4) for j >= 4 -- the
// same permutation for both operands, so the sum is over the same 32 positions; it makes the 8 rows that a 32-lane half reads in one
// instruction consecutive, which with the 288-byte pitch (72 dwords = 8 mod 64) puts them on 8 disjoint sets of banks.
#include "train_wgrad_h.hpp"

#include "split16.hpp"

#pragma clang fp contract(off)

namespace dcscn_impl {
using namespace dcscn;

typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));     // the builtin's own element type
typedef __attribute__((address_space(3))) fp16x4 lds_h4;

__device__ __forceinline__ float wg_exp2i(int e) { return __uint_as_float((unsigned)(127 + e) << 23); }   // e in [-126, 126]

// the 8 k-values of one operand: two transposed reads, 16 positions apart
__device__ __forceinline__ h8 tr_read8(const unsigned char* p) {
    const h4 a = __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4*)p));
    const h4 b = __builtin_bit_cast(h4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h4*)(p + 16 * kWgHPitch)));
    return h8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// 4 consecutive channels of one pixel (zeros past `count` channels or when !valid: no load is issued), scaled and split, to one position
__device__ __forceinline__ void stage4(const float* src, bool valid, int count, bool vec, float scale, float m1, unsigned char* dst) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
        if (vec && count >= 4) v = *reinterpret_cast<const f32x4*>(src);
        else
            for (int j = 0; j < 4; ++j)
                if (j < count) v[j] = src[j];
    }
    for (int j = 0; j < 4; ++j) v[j] = v[j] * scale;
    h4 hi, lo;
    split4(v, m1, hi, lo);
    *reinterpret_cast<h4*>(dst) = hi;
    *reinterpret_cast<h4*>(dst + 2 * kWgHBlock) = lo;
}

template <int TG>
__global__ __launch_bounds__(256) void tconv_wgrad_h(const TWgradHArgs a, const TWgradHPlan p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int group = blockIdx.x % p.groups, ci0 = (blockIdx.x / p.groups) * kWgHBlock, co0 = blockIdx.y * kWgHBlock;
    const int pad = a.ks / 2, taps = a.ks * a.ks;
    unsigned char* const in_img = lds;
    unsigned char* const dz_img = lds + (size_t)p.in_cap * kWgHPitch;
    const int e_sum = a.e_in[0] + a.e_dz[0];
    const float s_in = wg_exp2i(a.e_in[0]), s_dz = wg_exp2i(a.e_dz[0]);
    const float m1 = opaque_minus_one();
    // staging: thread = (position tid >> 4 of a pass of 16, channel quad tid & 15)
    const int sq = tid & 15, sp = tid >> 4;
    const int in_ch = ci0 + 4 * sq, dz_ch = co0 + 4 * sq;
    const int in_count = a.cin - in_ch, dz_count = a.cout - dz_ch;       // (<= 0: nothing to load)
    const bool in_vec = ((uintptr_t)a.in & 15) == 0 && (a.in_stride & 3) == 0;
    const bool dz_vec = ((uintptr_t)a.dz & 15) == 0 && (a.cout & 3) == 0;
    // operand reads: lane 4 q + c4 of group g supplies the address of position 4 g + q, channels 4 c4 .. + 3 of the 16-channel block
    const int g = lane >> 4, rq = (lane & 15) >> 2, c4 = lane & 3;
    const unsigned char* const a_rd = in_img + (4 * g + rq) * kWgHPitch + (wave * 16 + 4 * c4) * 2;
    const unsigned char* const b_rd = dz_img + (4 * g + rq) * kWgHPitch + (4 * c4) * 2;
    const bool wave_on = ci0 + wave * 16 < a.cin;
    int toff[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        const int tap = group * TG + t, kh = tap / a.ks;
        toff[t] = (kh * p.tcp + (tap - kh * a.ks)) * kWgHPitch;
    }
    f32x4 acc[TG][4];
#pragma unroll
    for (int t = 0; t < TG; ++t)
        for (int ni = 0; ni < 4; ++ni) acc[t][ni] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int64_t t0 = (int64_t)blockIdx.z * p.tps;
    const int64_t t1 = t0 + p.tps < p.tiles ? t0 + p.tps : p.tiles;
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int tx = (int)(tile % p.tiles_x);
        const int ty = (int)((tile / p.tiles_x) % p.tiles_y);
        const int64_t img = tile / ((int64_t)p.tiles_x * p.tiles_y);
        const int y0 = ty * p.tr, x0 = tx * p.tc;
        __syncthreads();                                   // the previous tile's reads are done
        for (int i = sp; i < p.in_cap; i += 16) {
            const int r = i / p.tcp, c = i - r * p.tcp;
            const int y = y0 - pad + r, x = x0 - pad + c;
            const bool v = r < p.tr + a.ks - 1 && y >= 0 && y < a.H && x >= 0 && x < a.W && in_count > 0;
            const float* src = a.in + (v ? ((img * a.H + y) * a.W + x) * a.in_stride + in_ch : 0);
            stage4(src, v, in_count, in_vec, s_in, m1, in_img + i * kWgHPitch + sq * 8);
        }
        for (int q = sp; q < p.kpad; q += 16) {
            const int r = q / p.tcp, c = q - r * p.tcp;
            const int y = y0 + r, x = x0 + c;
            const bool v = r < p.tr && c < p.tc && y < a.H && x < a.W && dz_count > 0;
            const float* src = a.dz + (v ? ((img * a.H + y) * a.W + x) * a.cout + dz_ch : 0);
            stage4(src, v, dz_count, dz_vec, s_dz, m1, dz_img + q * kWgHPitch + sq * 8);
        }
        __syncthreads();
        if (!wave_on) continue;                            // (wave-uniform; the barriers are above)
        for (int kc = 0; kc < p.kpad; kc += 32) {
            const unsigned char* const bp = b_rd + kc * kWgHPitch;
            const unsigned char* const ap = a_rd + kc * kWgHPitch;
            h8 bh[4], bl[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                if (co0 + ni * 16 >= a.cout) break;        // (uniform over the workgroup)
                bh[ni] = tr_read8(bp + ni * 32);
                bl[ni] = tr_read8(bp + ni * 32 + 2 * kWgHBlock);
            }
#pragma unroll
            for (int t = 0; t < TG; ++t) {
                const h8 ah = tr_read8(ap + toff[t]);
                const h8 al = tr_read8(ap + toff[t] + 2 * kWgHBlock);
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    if (co0 + ni * 16 >= a.cout) break;
                    acc[t][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[ni], acc[t][ni], 0, 0, 0);
                    acc[t][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[ni], acc[t][ni], 0, 0, 0);
                    acc[t][ni] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[ni], acc[t][ni], 0, 0, 0);
                }
            }
        }
    }
    // D: lane holds column lane & 15, rows 4 (lane >> 4) .. + 3
    float* part = a.part + (size_t)blockIdx.z * taps * a.cin * a.cout;
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        const int tap = group * TG + t;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int co = co0 + ni * 16 + (lane & 15);
            if (co >= a.cout) continue;
            for (int i = 0; i < 4; ++i) {
                const int ci = ci0 + wave * 16 + 4 * g + i;
                if (ci < a.cin) part[((size_t)tap * a.cin + ci) * a.cout + co] = ldexpf(acc[t][ni][i], -e_sum);
            }
        }
    }
}

template <int TG>
static hipError_t launch_tg(const TWgradHArgs& a, const TWgradHPlan& p, hipStream_t st) {
    static const hipError_t attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(&tconv_wgrad_h<TG>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWgHLdsMax);
    if (attr != hipSuccess) return attr;
    const dim3 grid((unsigned)((a.cin + kWgHBlock - 1) / kWgHBlock * p.groups), (unsigned)((a.cout + kWgHBlock - 1) / kWgHBlock), (unsigned)p.splits);
    hipLaunchKernelGGL(tconv_wgrad_h<TG>, grid, dim3(256), p.lds_bytes, st, a, p);
    return hipGetLastError();
}

hipError_t launch_tconv_wgrad_h(const TWgradHArgs& a, const TWgradHPlan& p, hipStream_t st) {
    if (p.lds_bytes > kWgHLdsMax || p.lds_bytes != (size_t)(p.kpad + p.in_cap) * kWgHPitch) return hipErrorInvalidValue;
    switch (p.tg) {
        case 1: return launch_tg<1>(a, p, st);
        case 9: return launch_tg<9>(a, p, st);
        case 5: return launch_tg<5>(a, p, st);
        case 7: return launch_tg<7>(a, p, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace dcscn_impl
