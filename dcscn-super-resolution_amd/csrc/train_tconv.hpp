// The transposed-conv upsampler in training (option "train_transposed"; build_transposed_conv, tf_graph.py:219-236): layer Up-TCNN is
//   hr = tf.nn.conv2d_transpose(x, W[k][k][oc][ic], stride s, SAME),  k = 2s - s % 2,  C -> C channels, no bias, no activator,
// the only layer that changes resolution by a strided scatter.  With pt = (k - s) / 2:
//   hr[n, s h + ky - pt, s w + kx - pt, oc] += x[n, h, w, ic] * W[ky][kx][oc][ic].
// Three f32 GEMMs on v_mfma_f32_16x16x4_f32 with the conventions of train_kernels.hpp (4 waves per workgroup, 32 x 32 per wave tile, every
// lane loads its own operands, every sum a fixed partition in a fixed order, no atomics), none of which multiplies a structural zero: the
// work is k^2 C^2 MACs per LR pixel in each direction (the derived 3x3 filter of the inference plan, graph.hip: add_tconv, has 9 s^2 C^2).
//
//   tup_fwd    one GEMM per output phase (a, b) = (Y % s, X % s): rows = LR pixels, columns = oc, k = (valid tap, ic).  HR pixel
//              (s h + a, s w + b) reads LR pixel (h + dy, w + dx), dy, dx in {-1, 0, 1}, through tap ky = a + pt - s dy where that lies
//              in [0, k).  Valid dy per phase a:    x2 (k 4): a0 {-1, 0}  a1 {0, 1}
//                                                   x3 (k 5): a0 {-1, 0}  a1 {0}  a2 {0, 1}
//                                                   x4 (k 8): a0, a1 {-1, 0}  a2, a3 {0, 1}
//              Written straight into the HR activation buffer.  The [ic][oc] operand is read from the per-step image that tpack_dgrad
//              makes of every filter (wd[t'][ic][oc] = W[k k - 1 - t'][oc][ic]), so the loads along oc are contiguous.
//   tup_dgrad  a stride-s conv over the HR gradient: rows = LR pixels, columns = ic, k = (tap, oc); W as stored is the [k][column]
//              operand; HR positions outside the image are masked; accumulates into the gradient of the layer's input.
//   tup_wgrad  rows = (tap, oc), columns = ic, k = the LR pixels of one split; the partials are summed by treduce_wgrad.
// Pixel and HR offsets are 64-bit as in tconv_gemm / tconv_wgrad.  Included by train.hip behind train_kernels.hpp: fp contract(off).
#pragma once
#include "train_kernels.hpp"

namespace dcscn_impl {

struct TUpArgs {
    float* lr; int lr_stride;   // the LR side, a channel slice of a concat buffer: the layer's input (read), or its gradient (tup_dgrad: +=)
    int C;
    int n, H, W;                // the LR shape; the HR side is [n][s H][s W][C], dense
    int s, k;
    const float* w;             // tup_fwd: tpack_dgrad's image of the filter; tup_dgrad: the filter [k][k][oc][ic]
    float* hr;                  // tup_fwd: written; tup_dgrad, tup_wgrad: the HR gradient (read)
    int64_t chunk;              // tup_wgrad: LR pixels per split (multiple of 16)
    float* part;                // tup_wgrad: [splits][k*k*C][C]
};

__global__ __launch_bounds__(256) void tup_fwd(const TUpArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int64_t P = (int64_t)a.n * a.H * a.W;
    const int64_t r0 = (int64_t)blockIdx.x * 128 + wave * 32;
    const int c0 = blockIdx.y * 32;
    const int pa = blockIdx.z / a.s, pb = blockIdx.z % a.s;      // the output phase
    const int pt = (a.k - a.s) / 2;
    int py[2], px[2]; int64_t pimg[2]; bool pv[2];
    for (int mi = 0; mi < 2; ++mi) {
        const int64_t p = r0 + mi * 16 + lr;
        pv[mi] = p < P;
        const int64_t q = pv[mi] ? p : 0;
        px[mi] = (int)(q % a.W);
        py[mi] = (int)((q / a.W) % a.H);
        pimg[mi] = q / ((int64_t)a.W * a.H);
    }
    bool cv[2];
    for (int ni = 0; ni < 2; ++ni) cv[ni] = c0 + ni * 16 + lr < a.C;
    tf32x4 acc[2][2];
    for (int mi = 0; mi < 2; ++mi)
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = tf32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int dy = -1; dy <= 1; ++dy) {
        const int ky = pa + pt - a.s * dy;
        if (ky < 0 || ky >= a.k) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int kx = pb + pt - a.s * dx;
            if (kx < 0 || kx >= a.k) continue;
            const float* src[2]; bool sv[2];
            for (int mi = 0; mi < 2; ++mi) {
                const int y = py[mi] + dy, x = px[mi] + dx;
                sv[mi] = pv[mi] && y >= 0 && y < a.H && x >= 0 && x < a.W;
                src[mi] = a.lr + (sv[mi] ? ((pimg[mi] * a.H + y) * a.W + x) * a.lr_stride : 0);
            }
            const float* wt = a.w + (size_t)(a.k * a.k - 1 - (ky * a.k + kx)) * a.C * a.C + c0 + lr;
            for (int ci0 = 0; ci0 < a.C; ci0 += 4) {
                const int ci = ci0 + lk;
                const bool kv = ci < a.C;
                float av[2], bv[2];
                for (int mi = 0; mi < 2; ++mi) av[mi] = (kv && sv[mi]) ? src[mi][ci] : 0.0f;
                for (int ni = 0; ni < 2; ++ni) bv[ni] = (kv && cv[ni]) ? wt[(size_t)ci * a.C + ni * 16] : 0.0f;
                for (int mi = 0; mi < 2; ++mi)
                    for (int ni = 0; ni < 2; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
            }
        }
    }
    const int64_t Hs = (int64_t)a.H * a.s, Ws = (int64_t)a.W * a.s;
    for (int mi = 0; mi < 2; ++mi)
        for (int i = 0; i < 4; ++i) {
            const int64_t p = r0 + mi * 16 + lk * 4 + i;
            if (p >= P) continue;
            const int x = (int)(p % a.W), y = (int)((p / a.W) % a.H);
            const int64_t img = p / ((int64_t)a.W * a.H);
            float* o = a.hr + ((img * Hs + (int64_t)y * a.s + pa) * Ws + (int64_t)x * a.s + pb) * a.C;
            for (int ni = 0; ni < 2; ++ni) {
                const int co = c0 + ni * 16 + lr;
                if (co < a.C) o[co] = acc[mi][ni][i];
            }
        }
}

__global__ __launch_bounds__(256) void tup_dgrad(const TUpArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int64_t P = (int64_t)a.n * a.H * a.W;
    const int64_t r0 = (int64_t)blockIdx.x * 128 + wave * 32;
    const int c0 = blockIdx.y * 32;
    const int pt = (a.k - a.s) / 2;
    const int Hs = a.H * a.s, Ws = a.W * a.s;
    int py[2], px[2]; int64_t pimg[2]; bool pv[2];
    for (int mi = 0; mi < 2; ++mi) {
        const int64_t p = r0 + mi * 16 + lr;
        pv[mi] = p < P;
        const int64_t q = pv[mi] ? p : 0;
        px[mi] = (int)(q % a.W) * a.s - pt;                      // the HR position of tap (0, 0)
        py[mi] = (int)((q / a.W) % a.H) * a.s - pt;
        pimg[mi] = q / ((int64_t)a.W * a.H);
    }
    bool cv[2];
    for (int ni = 0; ni < 2; ++ni) cv[ni] = c0 + ni * 16 + lr < a.C;
    tf32x4 acc[2][2];
    for (int mi = 0; mi < 2; ++mi)
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = tf32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int ky = 0; ky < a.k; ++ky)
        for (int kx = 0; kx < a.k; ++kx) {
            const float* src[2]; bool sv[2];
            for (int mi = 0; mi < 2; ++mi) {
                const int y = py[mi] + ky, x = px[mi] + kx;
                sv[mi] = pv[mi] && y >= 0 && y < Hs && x >= 0 && x < Ws;
                src[mi] = a.hr + (sv[mi] ? ((pimg[mi] * Hs + y) * Ws + x) * a.C : 0);
            }
            const float* wt = a.w + (size_t)(ky * a.k + kx) * a.C * a.C + c0 + lr;
            for (int co0 = 0; co0 < a.C; co0 += 4) {
                const int co = co0 + lk;
                const bool kv = co < a.C;
                float av[2], bv[2];
                for (int mi = 0; mi < 2; ++mi) av[mi] = (kv && sv[mi]) ? src[mi][co] : 0.0f;
                for (int ni = 0; ni < 2; ++ni) bv[ni] = (kv && cv[ni]) ? wt[(size_t)co * a.C + ni * 16] : 0.0f;
                for (int mi = 0; mi < 2; ++mi)
                    for (int ni = 0; ni < 2; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
            }
        }
    for (int mi = 0; mi < 2; ++mi)
        for (int ni = 0; ni < 2; ++ni) {
            const int ci = c0 + ni * 16 + lr;
            if (ci >= a.C) continue;
            for (int i = 0; i < 4; ++i) {
                const int64_t p = r0 + mi * 16 + lk * 4 + i;
                if (p >= P) continue;
                float* o = a.lr + p * a.lr_stride + ci;
                *o = *o + acc[mi][ni][i];
            }
        }
}

// Workgroup = one 32 x 32 tile of ((tap, oc), ic) and one split; its 4 waves take interleaved 4-pixel k-steps and their tiles are summed in
// wave order through LDS, as in tconv_wgrad.
__global__ __launch_bounds__(256) void tup_wgrad(const TUpArgs a) {
    __shared__ float red[4][32 * 32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int M = a.k * a.k * a.C;
    const int m0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int64_t P = (int64_t)a.n * a.H * a.W;
    const int64_t p0 = (int64_t)blockIdx.z * a.chunk;
    const int64_t p1 = p0 + a.chunk < P ? p0 + a.chunk : P;
    const int pt = (a.k - a.s) / 2;
    const int Hs = a.H * a.s, Ws = a.W * a.s;
    int oy[2], ox[2], ch[2]; bool mv[2];
    for (int mi = 0; mi < 2; ++mi) {
        const int m = m0 + mi * 16 + lr;
        mv[mi] = m < M;
        const int mm = mv[mi] ? m : 0;
        const int tap = mm / a.C;
        ch[mi] = mm - tap * a.C;
        oy[mi] = tap / a.k - pt;
        ox[mi] = tap % a.k - pt;
    }
    bool cv[2];
    for (int ni = 0; ni < 2; ++ni) cv[ni] = c0 + ni * 16 + lr < a.C;
    tf32x4 acc[2][2];
    for (int mi = 0; mi < 2; ++mi)
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = tf32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t pb = p0 + wave * 4; pb < p1; pb += 16) {
        const int64_t p = pb + lk;
        const bool pv = p < p1;
        const int64_t q = pv ? p : p0;
        const int x = (int)(q % a.W), y = (int)((q / a.W) % a.H);
        const int64_t img = q / ((int64_t)a.W * a.H);
        float av[2], bv[2];
        for (int mi = 0; mi < 2; ++mi) {
            const int yy = y * a.s + oy[mi], xx = x * a.s + ox[mi];
            const bool v = pv && mv[mi] && yy >= 0 && yy < Hs && xx >= 0 && xx < Ws;
            av[mi] = v ? a.hr[((img * Hs + yy) * Ws + xx) * a.C + ch[mi]] : 0.0f;
        }
        for (int ni = 0; ni < 2; ++ni) bv[ni] = (pv && cv[ni]) ? a.lr[q * a.lr_stride + c0 + ni * 16 + lr] : 0.0f;
        for (int mi = 0; mi < 2; ++mi)
            for (int ni = 0; ni < 2; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
    }
    for (int mi = 0; mi < 2; ++mi)
        for (int ni = 0; ni < 2; ++ni)
            for (int i = 0; i < 4; ++i) red[wave][(mi * 16 + lk * 4 + i) * 32 + ni * 16 + lr] = acc[mi][ni][i];
    __syncthreads();
    float* part = a.part + (size_t)blockIdx.z * M * a.C;
    for (int e = threadIdx.x; e < 32 * 32; e += 256) {
        const int m = m0 + e / 32, ci = c0 + e % 32;
        if (m < M && ci < a.C) part[(size_t)m * a.C + ci] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    }
}

}  // namespace dcscn_impl
