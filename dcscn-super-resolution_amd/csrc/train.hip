// Single-GPU f32 training of the non-separable pixel-shuffler DCSCN nets (DCSCN.py:334-425, tf_graph.py:117-153).
//
// The training plan is its own list of layers over its own arena (TrainState); it shares only the variables with the inference
// plan.  Every conv runs as one launch of tconv_gemm (implicit GEMM on v_mfma_f32_16x16x4_f32, rows = output pixels, columns =
// output channels, k = (tap, input channel)); the data gradient is the same kernel on the filter flipped in space with Cin <-> Cout
// transposed (tpack_dgrad, repacked on the device every step) accumulating into the gradient of the layer's input; the weight
// gradient is tconv_wgrad (rows = (tap, cin), columns = cout, k = pixels) over a fixed split of the pixels, reduced in a fixed order
// by treduce_wgrad.  Concat (H_concat, Concat2 = [B2 | A1]) is a strided slice of one tensor and its gradient one of the same
// layout, so neither direction copies.  Every reduction is a fixed partition summed in a fixed order: no atomics anywhere, two
// identical runs give identical bits.
//
// Variables, their gradients and the optimizer slots live in flat f32 buffers in the checkpoint (HWIO) layout, in the order of
// the graph's variable list (dcscn_tensor_info), so the update is one elementwise launch.
#include "plan.h"
#include "train_h.hpp"
#include "train_wgrad_h.hpp"

#pragma clang fp contract(off)

namespace dcscn_impl {

typedef float tf32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// dropout mask: the counter-based hash documented in include/dcscn.h (dcscn_train_step)
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ inline bool dropout_keep(uint64_t layer_key, uint64_t idx, uint32_t thresh) {
    return (uint32_t)(splitmix64(layer_key ^ idx) >> 40) < thresh;
}
inline uint64_t dropout_layer_key(uint64_t key, int layer) { return splitmix64(key + 0x9E3779B97F4A7C15ull * (uint64_t)(layer + 1)); }

// activator (helper/tf_graph.py:77-102) and its derivative from the pre-activation z; ACT_ALPHA = prelu / relu / leaky_relu
__device__ inline float tact(float z, float alpha, int act) {
    switch (act) {
        case ACT_ALPHA:   return z > 0.0f ? z : alpha * z;
        case ACT_SIGMOID: return 1.0f / (1.0f + expf(-z));
        case ACT_TANH:    return tanhf(z);
        case ACT_SELU:    return 1.0507009873554805f * (z > 0.0f ? z : 1.6732632423543772f * (expf(z) - 1.0f));
        default:          return z;
    }
}
// At z == 0 the derivative is the one the reference's graph takes under TensorFlow 1.x's registered gradients (include/dcscn.h,
// "ties"): prelu = relu(z) + a (z - |z|) / 2 gives a / 2, leaky_relu = maximum(z, 0.1 z) gives 1, selu gives the scale, relu gives 0.
// prelu: the layer has a slope tensor; otherwise alpha is the constant slope, 0.1 (leaky_relu) or 0 (relu).
__device__ inline float tact_grad(float z, float alpha, int act, bool prelu) {
    switch (act) {
        case ACT_ALPHA:   return z == 0.0f ? (prelu ? 0.5f * alpha : alpha > 0.0f ? 1.0f : 0.0f) : z > 0.0f ? 1.0f : alpha;
        case ACT_SIGMOID: { const float s = 1.0f / (1.0f + expf(-z)); return s * (1.0f - s); }
        case ACT_TANH:    { const float t = tanhf(z); return 1.0f - t * t; }
        case ACT_SELU:    return z >= 0.0f ? 1.0507009873554805f : 1.0507009873554805f * 1.6732632423543772f * expf(z);
        default:          return 1.0f;
    }
}

// ---------------------------------------------------------------------------------------------
// implicit-GEMM conv, SAME padding, stride 1:  out[p][co] (+)= bias[co] + sum_{tap, ci} in[p + tap][ci] * w[tap][ci][co]
// Workgroup = 4 waves x (32 pixels x 32 channels); per k-step of 4 a wave issues 2 x 2 MFMAs whose operands every lane loads
// itself (A: lane = (pixel l & 15, channel l >> 4), B: lane = (channel l >> 4, output channel l & 15)).  The k order is tap-major,
// channel-minor, so the result is the fmaf chain over (tap, ci) in that order; the bias is added after the chain.
// ---------------------------------------------------------------------------------------------
struct TConvArgs {
    const float* in; int in_stride; int cin;
    int n, H, W, ks;
    const float* w; int cout;
    const float* bias;
    float* out; int out_stride;
};

// ACCUM = 0: the forward conv (z = ...); 1: the data gradient (out += ...) -- two instantiations, so profiles tell them apart
template <int ACCUM>
__global__ __launch_bounds__(256) void tconv_gemm(const TConvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int64_t P = (int64_t)a.n * a.H * a.W;
    const int64_t r0 = (int64_t)blockIdx.x * 128 + wave * 32;
    const int c0 = blockIdx.y * 32;
    const int pad = a.ks / 2;
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
    for (int ni = 0; ni < 2; ++ni) cv[ni] = c0 + ni * 16 + lr < a.cout;
    tf32x4 acc[2][2];
    for (int mi = 0; mi < 2; ++mi)
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = tf32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int kh = 0; kh < a.ks; ++kh)
        for (int kw = 0; kw < a.ks; ++kw) {
            const float* src[2]; bool sv[2];
            for (int mi = 0; mi < 2; ++mi) {
                const int y = py[mi] + kh - pad, x = px[mi] + kw - pad;
                sv[mi] = pv[mi] && y >= 0 && y < a.H && x >= 0 && x < a.W;
                src[mi] = a.in + (sv[mi] ? ((pimg[mi] * a.H + y) * a.W + x) * a.in_stride : 0);
            }
            const float* wt = a.w + (size_t)(kh * a.ks + kw) * a.cin * a.cout + c0 + lr;
            for (int ci0 = 0; ci0 < a.cin; ci0 += 4) {
                const int ci = ci0 + lk;
                const bool kv = ci < a.cin;
                float av[2], bv[2];
                for (int mi = 0; mi < 2; ++mi) av[mi] = (kv && sv[mi]) ? src[mi][ci] : 0.0f;
                for (int ni = 0; ni < 2; ++ni) bv[ni] = (kv && cv[ni]) ? wt[(size_t)ci * a.cout + ni * 16] : 0.0f;
                for (int mi = 0; mi < 2; ++mi)
                    for (int ni = 0; ni < 2; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
            }
        }
    for (int mi = 0; mi < 2; ++mi)
        for (int ni = 0; ni < 2; ++ni) {
            const int co = c0 + ni * 16 + lr;
            if (co >= a.cout) continue;
            const float b = a.bias ? a.bias[co] : 0.0f;
            for (int i = 0; i < 4; ++i) {
                const int64_t p = r0 + mi * 16 + lk * 4 + i;
                if (p >= P) continue;
                float* o = a.out + p * a.out_stride + co;
                const float v = acc[mi][ni][i] + b;
                *o = ACCUM ? *o + v : v;
            }
        }
}

// ---------------------------------------------------------------------------------------------
// weight gradient: part[s][tap][ci][co] = sum over the pixels of split s of in[p + tap][ci] * dz[p][co]
// Workgroup = one 32 x 32 tile of (tap*cin + ci, co) and one split; its 4 waves take interleaved 4-pixel k-steps and their tiles
// are summed in wave order through LDS.
// ---------------------------------------------------------------------------------------------
struct TWgradArgs {
    const float* in; int in_stride; int cin;
    int n, H, W, ks;
    const float* dz; int cout;
    int64_t chunk;          // pixels per split (multiple of 16)
    float* part;            // [splits][ks*ks*cin][cout]
};

__global__ __launch_bounds__(256) void tconv_wgrad(const TWgradArgs a) {
    __shared__ float red[4][32 * 32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    const int M = a.ks * a.ks * a.cin;
    const int m0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int64_t P = (int64_t)a.n * a.H * a.W;
    const int64_t p0 = (int64_t)blockIdx.z * a.chunk;
    const int64_t p1 = p0 + a.chunk < P ? p0 + a.chunk : P;
    const int pad = a.ks / 2;
    int dy[2], dx[2], ch[2]; bool mv[2];
    for (int mi = 0; mi < 2; ++mi) {
        const int m = m0 + mi * 16 + lr;
        mv[mi] = m < M;
        const int mm = mv[mi] ? m : 0;
        const int tap = mm / a.cin;
        ch[mi] = mm - tap * a.cin;
        dy[mi] = tap / a.ks - pad;
        dx[mi] = tap % a.ks - pad;
    }
    bool cv[2];
    for (int ni = 0; ni < 2; ++ni) cv[ni] = c0 + ni * 16 + lr < a.cout;
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
            const int yy = y + dy[mi], xx = x + dx[mi];
            const bool v = pv && mv[mi] && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
            av[mi] = v ? a.in[((img * a.H + yy) * a.W + xx) * a.in_stride + ch[mi]] : 0.0f;
        }
        for (int ni = 0; ni < 2; ++ni) bv[ni] = (pv && cv[ni]) ? a.dz[q * a.cout + c0 + ni * 16 + lr] : 0.0f;
        for (int mi = 0; mi < 2; ++mi)
            for (int ni = 0; ni < 2; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
    }
    for (int mi = 0; mi < 2; ++mi)
        for (int ni = 0; ni < 2; ++ni)
            for (int i = 0; i < 4; ++i) red[wave][(mi * 16 + lk * 4 + i) * 32 + ni * 16 + lr] = acc[mi][ni][i];
    __syncthreads();
    float* part = a.part + (size_t)blockIdx.z * M * a.cout;
    for (int e = threadIdx.x; e < 32 * 32; e += 256) {
        const int m = m0 + e / 32, co = c0 + e % 32;
        if (m < M && co < a.cout) part[(size_t)m * a.cout + co] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
    }
}

// grad[e] = sum_s part[s][e] (in split order) + l2_decay * w[e]
__global__ void treduce_wgrad(const float* part, int splits, int64_t count, const float* w, float l2, float* grad) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    float s = 0.0f;
    for (int k = 0; k < splits; ++k) s += part[(size_t)k * count + e];
    grad[e] = s + l2 * w[e];
}

// per-channel sums over the pixels (bias gradient, PReLU-alpha gradient): block (co, split) -> part[split][co]; LDS tree in fixed order
__global__ __launch_bounds__(256) void tcol_partial(const float* v, int cout, int64_t P, int64_t chunk, float* part) {
    __shared__ float red[256];
    const int co = blockIdx.x;
    const int64_t p0 = (int64_t)blockIdx.y * chunk;
    const int64_t p1 = p0 + chunk < P ? p0 + chunk : P;
    float s = 0.0f;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) s += v[p * cout + co];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * cout + co] = red[0];
}
__global__ void tcol_final(const float* part, int cout, int splits, float* grad) {
    const int co = blockIdx.x * blockDim.x + threadIdx.x;
    if (co >= cout) return;
    float s = 0.0f;
    for (int k = 0; k < splits; ++k) s += part[(size_t)k * cout + co];
    grad[co] = s;
}

// forward epilogue of a conv with an activator: h = act(z), then dropout (mask / keep), into a strided slice.  idx0 = the index of
// the batch's first element within the global batch (a shard of a data-parallel step; 0 otherwise): the mask is the whole batch's
__global__ void tact_fwd(const float* z, int cout, int64_t P, const float* alpha, float calpha, int act, float* h, int h_stride,
                         uint64_t lkey, uint64_t idx0, uint32_t thresh, float keep, int dropout) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P * cout) return;
    const int64_t p = e / cout;
    const int co = (int)(e - p * cout);
    float v = tact(z[e], alpha ? alpha[co] : calpha, act);
    if (dropout) v = dropout_keep(lkey, idx0 + (uint64_t)e, thresh) ? v / keep : 0.0f;
    h[p * h_stride + co] = v;
}

// backward through dropout and the activator: dA = dh * mask / keep; dz = dA * act'(z); at = dA * min(z, 0) (PReLU alpha term)
__global__ void tact_bwd(const float* dh, int dh_stride, const float* z, int cout, int64_t P, const float* alpha, float calpha, int act,
                         uint64_t lkey, uint64_t idx0, uint32_t thresh, float keep, int dropout, float* dz, float* at) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P * cout) return;
    const int64_t p = e / cout;
    const int co = (int)(e - p * cout);
    float g = dh[p * dh_stride + co];
    if (dropout) g = dropout_keep(lkey, idx0 + (uint64_t)e, thresh) ? g / keep : 0.0f;
    const float zz = z[e];
    dz[e] = g * tact_grad(zz, alpha ? alpha[co] : calpha, act, alpha != nullptr);
    if (at) at[e] = g * (zz < 0.0f ? zz : 0.0f);
}

// depth_to_space (TF order: LR channel (i*s + j)*C + c -> HR pixel (s*y + i, s*x + j), channel c) and its inverse
__global__ void td2s(const float* lr, float* hr, int n, int H, int W, int s, int C, int inverse) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)n * H * W * s * s * C;
    if (e >= total) return;
    int64_t q = e;
    const int c = (int)(q % C); q /= C;
    const int X = (int)(q % (W * s)); q /= W * s;
    const int Y = (int)(q % (H * s));
    const int64_t img = q / (H * s);
    const int y = Y / s, i = Y - y * s, x = X / s, j = X - x * s;
    const int64_t li = (((img * H + y) * W + x) * s * s + (i * s + j)) * C + c;
    if (inverse) const_cast<float*>(lr)[li] = hr[e];
    else hr[e] = lr[li];
}

// dgrad filter: wd[tap'][co][ci] = w[taps - 1 - tap'][ci][co]
__global__ void tpack_dgrad(const float* w, int taps, int cin, int cout, float* wd) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)taps * cin * cout;
    if (e >= total) return;
    const int ci = (int)(e % cin);
    const int64_t q = e / cin;
    const int co = (int)(q % cout);
    const int t = (int)(q / cout);
    wd[e] = w[((int64_t)(taps - 1 - t) * cin + ci) * cout + co];
}

// loss: y_ = z + x2, diff = y_ - y_true over the whole HR patch (DCSCN.py:334-365); dz = d image_loss / d y_; per-block partial
// sums (float64) of diff^2 and |diff|
__global__ __launch_bounds__(256) void tloss(const float* z, const float* x2, const float* yt, int64_t count, int64_t chunk, int l1,
                                             float* dz, double* part) {
    __shared__ double r2[256], r1[256];
    const int64_t p0 = (int64_t)blockIdx.x * chunk;
    const int64_t p1 = p0 + chunk < count ? p0 + chunk : count;
    const float inv = 1.0f / (float)count;
    double s2 = 0.0, s1 = 0.0;
    for (int64_t e = p0 + threadIdx.x; e < p1; e += 256) {
        const float d = (z[e] + x2[e]) - yt[e];
        s2 += (double)d * d;
        s1 += fabs((double)d);
        dz[e] = l1 ? (d > 0.0f ? inv : d < 0.0f ? -inv : 0.0f) : (2.0f * d) * inv;
    }
    r2[threadIdx.x] = s2; r1[threadIdx.x] = s1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { r2[threadIdx.x] += r2[threadIdx.x + o]; r1[threadIdx.x] += r1[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = r2[0]; part[2 * blockIdx.x + 1] = r1[0]; }
}

// sum of squares of v[0, count) per block (float64, fixed order) into part[slot0 + block]
__global__ __launch_bounds__(256) void tsumsq(const float* v, int64_t count, int64_t chunk, double* part) {
    __shared__ double r[256];
    const int64_t p0 = (int64_t)blockIdx.x * chunk;
    const int64_t p1 = p0 + chunk < count ? p0 + chunk : count;
    double s = 0.0;
    for (int64_t e = p0 + threadIdx.x; e < p1; e += 256) s += (double)v[e] * v[e];
    r[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) r[threadIdx.x] += r[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = r[0];
}

// stats[0] image_loss, [1] mse, [2] global gradient norm (before clipping), [3] total loss; clip[0] = clip_by_global_norm factor.
// One workgroup: thread t sums partials t, t + 256, ... in order, then an LDS tree of fixed shape -- deterministic.
__global__ __launch_bounds__(256) void tstats(const double* loss_part, int loss_blocks, const double* w2_part, int w2_blocks, const double* g2_part,
                                              int g2_blocks, int64_t count, int l1, double l2_decay, double clip_norm, double* stats, float* clip) {
    __shared__ double r[4][256];
    const int t = threadIdx.x;
    double s2 = 0.0, s1 = 0.0, w2 = 0.0, g2 = 0.0;
    for (int b = t; b < loss_blocks; b += 256) { s2 += loss_part[2 * b]; s1 += loss_part[2 * b + 1]; }
    for (int b = t; b < w2_blocks; b += 256) w2 += w2_part[b];
    for (int b = t; b < g2_blocks; b += 256) g2 += g2_part[b];
    r[0][t] = s2; r[1][t] = s1; r[2][t] = w2; r[3][t] = g2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o)
            for (int k = 0; k < 4; ++k) r[k][t] += r[k][t + o];
        __syncthreads();
    }
    if (t != 0) return;
    const double mse = r[0][0] / (double)count, image = l1 ? r[1][0] / (double)count : mse;
    const float norm = (float)sqrt(r[3][0]);
    stats[0] = image; stats[1] = mse; stats[2] = norm; stats[3] = image + l2_decay * 0.5 * r[2][0];
    const float c = (float)clip_norm;
    clip[0] = clip_norm > 0.0 ? c / fmaxf(norm, c) : 1.0f;
}

// one optimizer step over the flat buffers (TF's ApplyAdam / ApplyGradientDescent / ApplyMomentum), g scaled by the clip factor
__device__ inline void opt_update(int kind, float* w, const float* g, float* m, float* v, int64_t e, const float* clip, const float* pw,
                                  float lr, float b1, float b2, float eps, float mu) {
    const float gg = g[e] * clip[0];
    if (kind == DCSCN_OPTIMIZER_ADAM) {
        const float lr_t = lr * sqrtf(1.0f - pw[1]) / (1.0f - pw[0]);
        const float mm = b1 * m[e] + (1.0f - b1) * gg;
        const float vv = b2 * v[e] + (1.0f - b2) * (gg * gg);
        m[e] = mm; v[e] = vv;
        w[e] = w[e] - lr_t * mm / (sqrtf(vv) + eps);
    } else if (kind == DCSCN_OPTIMIZER_MOMENTUM) {
        const float a = mu * m[e] + gg;
        m[e] = a;
        w[e] = w[e] - lr * a;
    } else {
        w[e] = w[e] - lr * gg;
    }
}
__global__ void topt(int kind, float* w, const float* g, float* m, float* v, int64_t count, const float* clip, const float* pw,
                     float lr, float b1, float b2, float eps, float mu) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    opt_update(kind, w, g, m, v, e, clip, pw, lr, b1, b2, eps, mu);
}
__global__ void tpowers(float* pw, float b1, float b2) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { pw[0] = pw[0] * b1; pw[1] = pw[1] * b2; }
}

// ---------------------------------------------------------------------------------------------
// data-parallel step (dcscn_train_local_gradients_* / dcscn_train_apply_records): every rank writes a record
//   [count gradient floats | zeros up to a multiple of 4 | 4 doubles: image_loss, mse, n_local, total loss]
// and every rank reduces all of them in rank order, so the replicas never differ by a bit.
// ---------------------------------------------------------------------------------------------
static constexpr int kRecordTrailer = 8;   // floats: 4 doubles
__host__ __device__ inline int64_t record_pad(int64_t count) { return (count + 3) / 4 * 4; }

// padding and trailer of a record behind the gradient copy; stats = tstats' four doubles of the local batch
__global__ void trecord_tail(float* rec, int64_t count, const double* stats, double n_local) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t pad = record_pad(count);
    for (int64_t e = count; e < pad; ++e) rec[e] = 0.0f;
    double* tr = reinterpret_cast<double*>(rec + pad);
    tr[0] = stats[0]; tr[1] = stats[1]; tr[2] = n_local; tr[3] = stats[3];
}

// w[r] = n_r / sum n_r (double, summed in rank order); ok[0] = every n_r is > 0 and the sum is finite (else every weight is 0)
__global__ void trank_weights(const float* records, int world, int64_t rf, int64_t pad, double* w, int* ok) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double sum = 0.0;
    bool good = true;
    for (int r = 0; r < world; ++r) {
        const double n = reinterpret_cast<const double*>(records + (size_t)r * rf + pad)[2];
        good = good && n > 0.0;              // (false for a NaN too)
        sum += n;
    }
    good = good && sum <= 1.7976931348623157e308;
    for (int r = 0; r < world; ++r) w[r] = good ? reinterpret_cast<const double*>(records + (size_t)r * rf + pad)[2] / sum : 0.0;
    ok[0] = good ? 1 : 0;
}

// g[e] = (float) sum_{r = 0 .. world-1, in that order} w[r] * (double) records[r][e]; one thread per 4 floats, 16-byte loads over the
// padded records and 16-byte stores (the ragged last quad of g is stored by element: g holds `count` floats, not the padding)
__global__ __launch_bounds__(256) void treduce_ranks(const float* records, int world, int64_t rf, int64_t count, const double* w, float* g) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e = q * 4;
    if (e >= count) return;
    tf32x4 v = *reinterpret_cast<const tf32x4*>(records + e);
    double wr = w[0];
    double a0 = wr * (double)v[0], a1 = wr * (double)v[1], a2 = wr * (double)v[2], a3 = wr * (double)v[3];
    for (int r = 1; r < world; ++r) {
        v = *reinterpret_cast<const tf32x4*>(records + (size_t)r * rf + e);
        wr = w[r];
        a0 += wr * (double)v[0]; a1 += wr * (double)v[1]; a2 += wr * (double)v[2]; a3 += wr * (double)v[3];
    }
    const tf32x4 out = {(float)a0, (float)a1, (float)a2, (float)a3};
    if (e + 4 <= count) *reinterpret_cast<tf32x4*>(g + e) = out;
    else
        for (int i = 0; e + i < count; ++i) g[e + i] = out[i];
}

// tstats of the reduced step: stats[0] image_loss, [1] mse, [3] total loss = the weighted sums, in rank order, of the trailers;
// [2] = the norm of the reduced gradient from tsumsq's partials, summed as tstats sums them; clip[0] by tstats' formula
__global__ __launch_bounds__(256) void tstats_ranks(const float* records, int world, int64_t rf, int64_t pad, const double* w, const double* g2_part,
                                                    int g2_blocks, double clip_norm, double* stats, float* clip) {
    __shared__ double r[256];
    const int t = threadIdx.x;
    double g2 = 0.0;
    for (int b = t; b < g2_blocks; b += 256) g2 += g2_part[b];
    r[t] = g2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) r[t] += r[t + o];
        __syncthreads();
    }
    if (t != 0) return;
    const double* tr = reinterpret_cast<const double*>(records + pad);
    double image = w[0] * tr[0], mse = w[0] * tr[1], total = w[0] * tr[3];
    for (int k = 1; k < world; ++k) {
        tr = reinterpret_cast<const double*>(records + (size_t)k * rf + pad);
        image += w[k] * tr[0]; mse += w[k] * tr[1]; total += w[k] * tr[3];
    }
    const float norm = (float)sqrt(r[0]);
    stats[0] = image; stats[1] = mse; stats[2] = norm; stats[3] = total;
    const float c = (float)clip_norm;
    clip[0] = clip_norm > 0.0 ? c / fmaxf(norm, c) : 1.0f;
}

// topt / tpowers behind a reduction: nothing moves when the records' patch counts did not form a batch (ok[0] = 0)
__global__ void topt_ranks(const int* ok, int kind, float* w, const float* g, float* m, float* v, int64_t count, const float* clip, const float* pw,
                           float lr, float b1, float b2, float eps, float mu) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count || !ok[0]) return;
    opt_update(kind, w, g, m, v, e, clip, pw, lr, b1, b2, eps, mu);
}
__global__ void tpowers_ranks(const int* ok, float* pw, float b1, float b2) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && ok[0]) { pw[0] = pw[0] * b1; pw[1] = pw[1] * b2; }
}

// ---------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------
struct TBuf { int stride = 0; int res = 1; float* h = nullptr; float* g = nullptr; };

struct TLayer {
    std::string name;
    int index = 0;                 // position in the graph's layer list (dcscn_layer_info order): the dropout layer number
    int ks = 3, cin = 0, cout = 0, res = 1;
    int act = ACT_NONE; float calpha = 0.0f;
    bool dropout = false;          // has an activator (DCSCN.py: dropout follows exactly those convs)
    int in_buf = -1, in_off = 0;   // -1: the network input x
    int out_buf = -1, out_off = 0; // activation destination (act layers) / depth_to_space destination (ps > 0); -1: y_ (last layer)
    int ps = 0;                    // > 0: Up-PS conv followed by depth_to_space with this factor
    int w_t = -1, b_t = -1, a_t = -1;
    float* z = nullptr;            // pre-activation, dense [P res^2, cout]
    // option "train_split16" (train_h.hpp), in the current carve: h16 = the layer's forward and data-gradient convs run on tconv_gemm_h
    bool h16 = false;
    void *w16 = nullptr, *wd16 = nullptr;   // tpack_h images: forward, data gradient (null for a layer on the network input)
    int* e = nullptr;                       // exponents of the scales: [0] filter, [1] input slice, [2] dz
    // option "train_split16_wgrad" (train_wgrad_h.hpp), in the current carve: the layer's weight gradient runs on tconv_wgrad_h; it reads
    // e[1] and e[2], which the forward and the data gradient have found already when h16 is set as well
    bool wg16 = false;
};

// the variables the l2 term sums over: the filters, not biases or prelu slopes
static bool is_conv_w(const std::string& name) { return name.size() >= 7 && name.compare(name.size() - 7, 7, "/conv_W") == 0; }

static constexpr int kLossBlocks = 256, kNormBlocks = 256, kW2Blocks = 32;   // (kW2Blocks: per conv_W tensor, for the l2 term)

struct TrainState {
    dcscn_train_config tc{};
    std::vector<TBuf> bufs;
    std::vector<TLayer> layers;
    std::vector<int64_t> off;      // flat offset of every variable (h->tensors order)
    int64_t count = 0;
    float *d_w = nullptr, *d_g = nullptr, *d_m = nullptr, *d_v = nullptr, *d_wd = nullptr, *d_pw = nullptr;
    float h_pw[2] = {0.0f, 0.0f};
    // arena for the current batch shape
    void* arena = nullptr; size_t arena_bytes = 0;
    int n = 0, H = 0, W = 0;
    bool h16 = false;              // the carve holds the filter images and exponents of option "train_split16"
    bool wg16 = false;             // ... the exponents and the partial sums of option "train_split16_wgrad"
    unsigned* absmax = nullptr;    // kAbsMaxBlocks partial maxima (launch_texp)
    float *dz = nullptr, *at = nullptr, *part = nullptr, *col = nullptr, *zlast = nullptr, *dzlast = nullptr, *clip = nullptr;
    float *io_x = nullptr, *io_x2 = nullptr, *io_y = nullptr;
    double *dpart = nullptr, *d_stats = nullptr;
    int w2_blocks = 0;
    std::vector<double> stats_host;
    bool stepped = false;          // a step has changed the variables since the inference plan was last packed
    // dcscn_train_apply_records: [kNormBlocks] norm partials | 4 stats | clip (float) | ok (int) | [world] rank weights, as doubles
    double* d_red = nullptr; size_t red_cap = 0;
    hipEvent_t join_ev = nullptr;  // join_stream's event, made on first use
};

static int grid1(int64_t n) { return (int)((n + 255) / 256); }

static int tensor_of(dcscn_ctx* h, const std::string& name) {
    auto it = h->tensor_index.find(name);
    return it == h->tensor_index.end() ? -1 : it->second;
}

// the training graph of build_graph (graph.hip), without the launch-level rewrites
static int build_train_plan(dcscn_ctx* h, TrainState* t) {
    const dcscn_config& c = h->cfg;
    float ca = 0.0f;
    const int act = kernel_act(c.activator, &ca);
    auto add_buf = [&](int stride, int res) { TBuf b; b.stride = stride; b.res = res; t->bufs.push_back(b); return (int)t->bufs.size() - 1; };
    auto add_layer = [&](const std::string& var, const std::string& short_name, int in_buf, int in_off, int cin, int ks, int cout, bool has_act,
                         int out_buf, int out_off, int ps, int res) -> int {
        TLayer L;
        L.name = var; L.index = (int)t->layers.size(); L.ks = ks; L.cin = cin; L.cout = cout; L.res = res;
        L.act = has_act ? act : ACT_NONE; L.calpha = has_act ? ca : 0.0f; L.dropout = has_act;
        L.in_buf = in_buf; L.in_off = in_off; L.out_buf = out_buf; L.out_off = out_off; L.ps = ps;
        L.w_t = tensor_of(h, var + "/conv_W");
        L.b_t = tensor_of(h, var + "/conv_B");
        if (has_act && c.activator == DCSCN_ACT_PRELU) L.a_t = tensor_of(h, var + "/prelu/" + short_name + "_prelu");
        if (L.w_t < 0 || (has_act && c.activator == DCSCN_ACT_PRELU && L.a_t < 0))
            return fail(h, DCSCN_ERR_UNSUPPORTED, "training: layer %s has no conv_W / prelu variable", var.c_str());
        t->layers.push_back(L);
        return DCSCN_OK;
    };
    int rc;
    int total = 0;
    std::vector<int> off(c.layers);
    for (int i = 0; i < c.layers; ++i) { off[i] = total; total += h->sched[i]; }
    const int cat = add_buf(total, 1);
    int in_buf = -1, in_off = 0, cin = c.channels;
    for (int i = 0; i < c.layers; ++i) {
        const std::string nm = "CNN" + std::to_string(i + 1);
        if ((rc = add_layer(nm, nm, in_buf, in_off, cin, c.cnn_size, h->sched[i], true, cat, off[i], 0, 1))) return rc;
        in_buf = cat; in_off = off[i]; cin = h->sched[i];
    }
    if (c.use_nin) {
        const int na = c.nin_filters, nb = c.nin_filters2;
        const int t1 = add_buf(nb, 1), t2 = add_buf(nb + na, 1);
        if ((rc = add_layer("A1", "A1", cat, 0, total, 1, na, true, t2, nb, 0, 1))) return rc;
        if ((rc = add_layer("B1", "B1", cat, 0, total, 1, nb, true, t1, 0, 0, 1))) return rc;
        if ((rc = add_layer("B2", "B2", t1, 0, nb, 3, nb, true, t2, 0, 0, 1))) return rc;           // (3x3 whatever cnn_size); Concat2 = [B2 | A1]
        in_buf = t2; in_off = 0; cin = nb + na;
    } else if (c.legacy_no_c) {
        in_buf = cat; in_off = 0; cin = total;
    } else {
        const int tc = add_buf(c.filters, 1);
        if ((rc = add_layer("C", "C", cat, 0, total, 1, c.filters, true, tc, 0, 0, 1))) return rc;
        in_buf = tc; in_off = 0; cin = c.filters;
    }
    const int ps_out = c.pixel_shuffler_filters != 0 ? c.pixel_shuffler_filters : cin;
    struct Stage { const char* name; int s; int cout; };
    std::vector<Stage> stages;
    if (c.scale == 4) { stages.push_back({"Up-PS", 2, cin}); stages.push_back({"Up-PS2", 2, ps_out}); }
    else stages.push_back({"Up-PS", c.scale, ps_out});
    int res = 1;
    for (const Stage& st : stages) {
        const int ub = add_buf(st.cout, res * st.s);
        const std::string var = std::string(st.name) + "/" + st.name + "_CNN";
        if ((rc = add_layer(var, std::string(st.name) + "_CNN", in_buf, in_off, cin, c.cnn_size, st.s * st.s * st.cout, false, ub, 0, st.s, res))) return rc;
        in_buf = ub; in_off = 0; cin = st.cout; res *= st.s;
    }
    const int rl = std::max(c.reconstruct_layers, 1);
    for (int i = 0; i < rl - 1; ++i) {
        const std::string nm = "R-CNN" + std::to_string(i + 1);
        const int rb = add_buf(c.reconstruct_filters, res);
        if ((rc = add_layer(nm, nm, in_buf, in_off, cin, c.cnn_size, c.reconstruct_filters, true, rb, 0, 0, res))) return rc;
        in_buf = rb; in_off = 0; cin = c.reconstruct_filters;
    }
    const std::string nm = "R-CNN" + std::to_string(rl);
    if ((rc = add_layer(nm, nm, in_buf, in_off, cin, c.cnn_size, 1, false, -1, 0, 0, res))) return rc;
    if (t->layers.size() != h->layers.size()) return fail(h, DCSCN_ERR_UNSUPPORTED, "training: internal layer count mismatch");
    return DCSCN_OK;
}

// wgrad split of a layer: fixed by the shape alone
static int wgrad_splits(const TLayer& L, int64_t P, int64_t* chunk) {
    const int64_t tiles = (int64_t)((L.ks * L.ks * L.cin + 31) / 32) * ((L.cout + 31) / 32);
    int64_t s = std::max<int64_t>(1, std::min<int64_t>((2048 + tiles - 1) / tiles, (P + 1023) / 1024));
    int64_t ch = ((P + s - 1) / s + 15) / 16 * 16;
    s = (P + ch - 1) / ch;
    *chunk = ch;
    return (int)s;
}
static int col_splits(int64_t P, int64_t* chunk) {
    int64_t s = std::max<int64_t>(1, std::min<int64_t>(64, (P + 4095) / 4096));
    *chunk = (P + s - 1) / s;
    return (int)s;
}

static int carve(dcscn_ctx* h, TrainState* t, int n, int H, int W) {
    const bool h16 = h->train_split16, wg16 = h->train_split16_wgrad;
    if (t->arena && t->n == n && t->H == H && t->W == W && t->h16 == h16 && t->wg16 == wg16) return DCSCN_OK;
    const int64_t P = (int64_t)n * H * W;
    size_t bytes = 0;
    auto take = [&](size_t floats) { size_t o = bytes; bytes += (floats * 4 + 255) / 256 * 256; return o; };
    std::vector<size_t> oh(t->bufs.size()), og(t->bufs.size()), oz(t->layers.size());
    for (size_t b = 0; b < t->bufs.size(); ++b) {
        const int64_t px = P * t->bufs[b].res * t->bufs[b].res;
        oh[b] = take((size_t)px * t->bufs[b].stride);
        og[b] = take((size_t)px * t->bufs[b].stride);
    }
    size_t dz_max = 0, part_max = 0, col_max = 0;
    for (size_t l = 0; l < t->layers.size(); ++l) {
        const TLayer& L = t->layers[l];
        const int64_t px = P * L.res * L.res;
        oz[l] = take((size_t)px * L.cout);
        dz_max = std::max(dz_max, (size_t)px * L.cout);
        int64_t ch;
        const int s = wg16 && tconv_h_eligible(L.cin, L.cout) ? twgrad_h_plan(L.ks, L.cin, L.cout, n, H * L.res, W * L.res).splits
                                                              : wgrad_splits(L, px, &ch);
        part_max = std::max(part_max, (size_t)s * L.ks * L.ks * L.cin * L.cout);
        const int cs = col_splits(px, &ch);
        col_max = std::max(col_max, (size_t)cs * L.cout);
    }
    const int s = h->cfg.scale;
    const size_t hr = (size_t)P * s * s;
    const size_t o_dz = take(dz_max), o_at = take(dz_max), o_part = take(part_max), o_col = take(col_max);
    const size_t o_x = take((size_t)P), o_x2 = take(hr), o_y = take(hr), o_clip = take(4);
    const size_t o_dpart = take(2 * (2 * kLossBlocks + (size_t)t->w2_blocks + kNormBlocks) + 16);
    // option "train_split16": both filter images of every eligible layer, three exponents per layer, the partial maxima
    std::vector<size_t> ow(t->layers.size(), 0), owd(t->layers.size(), 0);
    size_t o_exp = 0, o_absmax = 0;
    if (h16) {
        for (size_t l = 0; l < t->layers.size(); ++l) {
            const TLayer& L = t->layers[l];
            if (!tconv_h_eligible(L.cin, L.cout)) continue;
            ow[l] = take(tpack_h_bytes(L.ks * L.ks, L.cin, L.cout) / 4);
            if (L.in_buf >= 0) owd[l] = take(tpack_h_bytes(L.ks * L.ks, L.cout, L.cin) / 4);
        }
    }
    if (h16 || wg16) {      // either option reads exponents
        o_exp = take(3 * t->layers.size());
        o_absmax = take(kAbsMaxBlocks);
    }
    if ((int64_t)bytes > h->workspace_budget)
        return fail(h, DCSCN_ERR_NOMEM, "training batch %d x %d x %d needs %zu bytes of workspace, over the budget of %lld (training does not tile)",
                    n, H, W, bytes, (long long)h->workspace_budget);
    if (t->arena) { (void)hipStreamSynchronize(h->stream); HIP_TRY(h, hipFree(t->arena)); t->arena = nullptr; }
    hipError_t e = hipMalloc(&t->arena, bytes);
    if (e != hipSuccess) { t->arena = nullptr; return fail(h, DCSCN_ERR_NOMEM, "training workspace of %zu bytes: %s", bytes, hipGetErrorString(e)); }
    t->arena_bytes = bytes;
    char* base = static_cast<char*>(t->arena);
    for (size_t b = 0; b < t->bufs.size(); ++b) { t->bufs[b].h = (float*)(base + oh[b]); t->bufs[b].g = (float*)(base + og[b]); }
    for (size_t l = 0; l < t->layers.size(); ++l) {
        TLayer& L = t->layers[l];
        L.z = (float*)(base + oz[l]);
        L.h16 = h16 && tconv_h_eligible(L.cin, L.cout);
        L.w16 = L.h16 ? base + ow[l] : nullptr;
        L.wd16 = L.h16 && L.in_buf >= 0 ? base + owd[l] : nullptr;
        L.wg16 = wg16 && tconv_h_eligible(L.cin, L.cout);
        L.e = L.h16 || L.wg16 ? (int*)(base + o_exp) + 3 * l : nullptr;
    }
    t->h16 = h16; t->wg16 = wg16;
    t->absmax = h16 || wg16 ? (unsigned*)(base + o_absmax) : nullptr;
    t->dz = (float*)(base + o_dz); t->at = (float*)(base + o_at); t->part = (float*)(base + o_part); t->col = (float*)(base + o_col);
    t->io_x = (float*)(base + o_x); t->io_x2 = (float*)(base + o_x2); t->io_y = (float*)(base + o_y); t->clip = (float*)(base + o_clip);
    t->dpart = (double*)(base + o_dpart);
    t->d_stats = t->dpart + 2 * kLossBlocks + t->w2_blocks + kNormBlocks;
    t->zlast = t->layers.back().z;
    t->n = n; t->H = H; t->W = W;
    return DCSCN_OK;
}

#define KTRY(h, launch)                                                                                \
    do {                                                                                               \
        launch;                                                                                        \
        hipError_t e_ = hipGetLastError();                                                             \
        if (e_ != hipSuccess) return fail(h, DCSCN_ERR_HIP, "%s: %s", #launch, hipGetErrorString(e_)); \
    } while (0)

static int launch_conv(dcscn_ctx* h, hipStream_t st, const float* in, int in_stride, int cin, int n, int H, int W, int ks, const float* w, int cout,
                       const float* bias, float* out, int out_stride, int accumulate) {
    TConvArgs a{in, in_stride, cin, n, H, W, ks, w, cout, bias, out, out_stride};
    const int64_t P = (int64_t)n * H * W;
    dim3 grid((unsigned)((P + 127) / 128), (unsigned)((cout + 31) / 32));
    if (accumulate) KTRY(h, hipLaunchKernelGGL(tconv_gemm<1>, grid, dim3(256), 0, st, a));
    else KTRY(h, hipLaunchKernelGGL(tconv_gemm<0>, grid, dim3(256), 0, st, a));
    return DCSCN_OK;
}

// the same conv on tconv_gemm_h (option "train_split16"): the exponent of the input's scale first (unless the caller has found it
// already: find_e = false), then the launch that reads it
static int launch_conv_h(dcscn_ctx* h, TrainState* t, hipStream_t st, const float* in, int in_stride, int cin, int n, int H, int W, int ks, const void* w16,
                         const int* e_w, int* e_in, int cout, const float* bias, float* out, int out_stride, int accumulate, bool find_e = true) {
    if (find_e) KTRY(h, launch_texp(in, in_stride, cin, (int64_t)n * H * W, t->absmax, e_in, st));
    TConvHArgs a{in, in_stride, cin, n, H, W, ks, w16, cout, bias, out, out_stride, e_in, e_w};
    KTRY(h, launch_tconv_gemm_h(a, accumulate, st));
    return DCSCN_OK;
}

// forward + backward of one step (gradients into d_g, stats into d_stats); no host synchronisation
static int run_gradients(dcscn_ctx* h, TrainState* t, const float* x, const float* x2, const float* yt, uint64_t key, hipStream_t st,
                         int64_t first_index = 0) {
    const dcscn_train_config& tc = t->tc;
    const int n = t->n, H = t->H, W = t->W;
    const int64_t P = (int64_t)n * H * W;
    const bool drop = tc.keep_prob < 1.0;
    const float keep = (float)tc.keep_prob;
    const uint32_t thresh = drop ? (uint32_t)std::min(16777216.0, std::floor(tc.keep_prob * 16777216.0)) : 0u;
    auto in_ptr = [&](const TLayer& L, float** g) -> const float* {
        if (L.in_buf < 0) { *g = nullptr; return x; }
        const TBuf& b = t->bufs[L.in_buf];
        *g = b.g + L.in_off;
        return b.h + L.in_off;
    };
    auto in_stride = [&](const TLayer& L) { return L.in_buf < 0 ? 1 : t->bufs[L.in_buf].stride; };

    // dgrad filters of the current weights
    for (const TLayer& L : t->layers) {
        const int64_t cnt = (int64_t)L.ks * L.ks * L.cin * L.cout;
        if (L.h16) {   // the scaled f16 images of both directions instead
            KTRY(h, launch_texp(t->d_w + t->off[L.w_t], 1, 1, cnt, t->absmax, L.e, st));
            KTRY(h, launch_tpack_h(t->d_w + t->off[L.w_t], L.ks * L.ks, L.cin, L.cout, L.e, L.w16, L.wd16, st));
            continue;
        }
        KTRY(h, hipLaunchKernelGGL(tpack_dgrad, dim3(grid1(cnt)), dim3(256), 0, st, t->d_w + t->off[L.w_t], L.ks * L.ks, L.cin, L.cout, t->d_wd + t->off[L.w_t]));
    }
    // ---- forward ----
    for (const TLayer& L : t->layers) {
        const int r = L.res;
        const int64_t px = P * r * r;
        float* gdummy;
        const float* in = in_ptr(L, &gdummy);
        const float* bias = L.b_t >= 0 ? t->d_w + t->off[L.b_t] : nullptr;
        int rc = L.h16 ? launch_conv_h(h, t, st, in, in_stride(L), L.cin, n, H * r, W * r, L.ks, L.w16, L.e, L.e + 1, L.cout, bias, L.z, L.cout, 0)
                       : launch_conv(h, st, in, in_stride(L), L.cin, n, H * r, W * r, L.ks, t->d_w + t->off[L.w_t], L.cout, bias, L.z, L.cout, 0);
        if (rc) return rc;
        if (L.dropout) {
            const TBuf& ob = t->bufs[L.out_buf];
            KTRY(h, hipLaunchKernelGGL(tact_fwd, dim3(grid1(px * L.cout)), dim3(256), 0, st, L.z, L.cout, px, L.a_t >= 0 ? t->d_w + t->off[L.a_t] : nullptr,
                                       L.calpha, L.act, ob.h + L.out_off, ob.stride, dropout_layer_key(key, L.index), (uint64_t)first_index * (uint64_t)(px / n * L.cout),
                                       thresh, keep, drop ? 1 : 0));
        } else if (L.ps > 0) {
            const TBuf& ob = t->bufs[L.out_buf];
            const int C = L.cout / (L.ps * L.ps);
            KTRY(h, hipLaunchKernelGGL(td2s, dim3(grid1(px * L.cout)), dim3(256), 0, st, (const float*)L.z, ob.h, n, H * r, W * r, L.ps, C, 0));
        }
    }
    // ---- loss ----
    const int64_t cnt = P * h->cfg.scale * h->cfg.scale;
    for (const TBuf& b : t->bufs) HIP_TRY(h, hipMemsetAsync(b.g, 0, (size_t)P * b.res * b.res * b.stride * 4, st));
    const int64_t lchunk = (cnt + kLossBlocks - 1) / kLossBlocks;
    KTRY(h, hipLaunchKernelGGL(tloss, dim3(kLossBlocks), dim3(256), 0, st, (const float*)t->zlast, x2, yt, cnt, lchunk, tc.use_l1_loss, t->dz, t->dpart));
    // ---- backward, layers in reverse ----
    for (int l = (int)t->layers.size() - 1; l >= 0; --l) {
        const TLayer& L = t->layers[l];
        const int r = L.res, Hr = H * r, Wr = W * r;
        const int64_t px = P * r * r;
        float* gin;
        const float* in = in_ptr(L, &gin);
        const bool prelu = L.a_t >= 0;
        if (L.dropout) {
            const TBuf& ob = t->bufs[L.out_buf];
            KTRY(h, hipLaunchKernelGGL(tact_bwd, dim3(grid1(px * L.cout)), dim3(256), 0, st, (const float*)(ob.g + L.out_off), ob.stride, (const float*)L.z, L.cout, px,
                                       prelu ? t->d_w + t->off[L.a_t] : nullptr, L.calpha, L.act, dropout_layer_key(key, L.index),
                                       (uint64_t)first_index * (uint64_t)(px / n * L.cout), thresh, keep, drop ? 1 : 0,
                                       t->dz, prelu ? t->at : nullptr));
        } else if (L.ps > 0) {
            const TBuf& ob = t->bufs[L.out_buf];
            const int C = L.cout / (L.ps * L.ps);
            KTRY(h, hipLaunchKernelGGL(td2s, dim3(grid1(px * L.cout)), dim3(256), 0, st, (const float*)t->dz, (float*)ob.g, n, Hr, Wr, L.ps, C, 1));
        }   // (the last layer: dz is the loss gradient already)
        // weight gradient (+ l2_decay * W)
        const int M = L.ks * L.ks * L.cin;
        int splits;
        if (L.wg16) {
            // e[1] is the forward's when the layer's convs run on tconv_gemm_h; e[2] is found here, once, for this launch and the data gradient's
            if (!L.h16) KTRY(h, launch_texp(in, in_stride(L), L.cin, px, t->absmax, L.e + 1, st));
            KTRY(h, launch_texp(t->dz, L.cout, L.cout, px, t->absmax, L.e + 2, st));
            const TWgradHPlan wp = twgrad_h_plan(L.ks, L.cin, L.cout, n, Hr, Wr);
            const TWgradHArgs wa{in, in_stride(L), L.cin, n, Hr, Wr, L.ks, t->dz, L.cout, L.e + 1, L.e + 2, t->part};
            const hipError_t we = launch_tconv_wgrad_h(wa, wp, st);
            if (we != hipSuccess) return fail(h, DCSCN_ERR_HIP, "tconv_wgrad_h (%s, %zu bytes of LDS): %s", L.name.c_str(), wp.lds_bytes, hipGetErrorString(we));
            splits = wp.splits;
        } else {
            int64_t chunk;
            splits = wgrad_splits(L, px, &chunk);
            TWgradArgs wa{in, in_stride(L), L.cin, n, Hr, Wr, L.ks, t->dz, L.cout, chunk, t->part};
            KTRY(h, hipLaunchKernelGGL(tconv_wgrad, dim3((M + 31) / 32, (L.cout + 31) / 32, splits), dim3(256), 0, st, wa));
        }
        const int64_t wc = (int64_t)M * L.cout;
        KTRY(h, hipLaunchKernelGGL(treduce_wgrad, dim3(grid1(wc)), dim3(256), 0, st, (const float*)t->part, splits, wc, (const float*)(t->d_w + t->off[L.w_t]),
                                   (float)tc.l2_decay, t->d_g + t->off[L.w_t]));
        // bias and PReLU-alpha gradients
        int64_t cchunk;
        const int cs = col_splits(px, &cchunk);
        if (L.b_t >= 0) {
            KTRY(h, hipLaunchKernelGGL(tcol_partial, dim3(L.cout, cs), dim3(256), 0, st, (const float*)t->dz, L.cout, px, cchunk, t->col));
            KTRY(h, hipLaunchKernelGGL(tcol_final, dim3(grid1(L.cout)), dim3(256), 0, st, (const float*)t->col, L.cout, cs, t->d_g + t->off[L.b_t]));
        }
        if (prelu) {
            KTRY(h, hipLaunchKernelGGL(tcol_partial, dim3(L.cout, cs), dim3(256), 0, st, (const float*)t->at, L.cout, px, cchunk, t->col));
            KTRY(h, hipLaunchKernelGGL(tcol_final, dim3(grid1(L.cout)), dim3(256), 0, st, (const float*)t->col, L.cout, cs, t->d_g + t->off[L.a_t]));
        }
        // data gradient, accumulated into the input's gradient (none for the network input)
        if (gin) {
            int rc = L.h16 ? launch_conv_h(h, t, st, t->dz, L.cout, L.cout, n, Hr, Wr, L.ks, L.wd16, L.e, L.e + 2, L.cin, nullptr, gin, in_stride(L), 1, !L.wg16)
                           : launch_conv(h, st, t->dz, L.cout, L.cout, n, Hr, Wr, L.ks, t->d_wd + t->off[L.w_t], L.cin, nullptr, gin, in_stride(L), 1);
            if (rc) return rc;
        }
    }
    // ---- l2 term, global norm, stats ----
    double* w2p = t->dpart + 2 * kLossBlocks;
    int slot = 0;
    for (size_t i = 0; i < h->tensors.size(); ++i) {
        if (!is_conv_w(h->tensors[i].name)) continue;
        const int64_t c = (int64_t)h->tensors[i].data.size();
        KTRY(h, hipLaunchKernelGGL(tsumsq, dim3(kW2Blocks), dim3(256), 0, st, (const float*)(t->d_w + t->off[i]), c, (c + kW2Blocks - 1) / kW2Blocks,
                                   w2p + slot));
        slot += kW2Blocks;
    }
    double* g2p = w2p + t->w2_blocks;
    const int64_t gchunk = (t->count + kNormBlocks - 1) / kNormBlocks;
    KTRY(h, hipLaunchKernelGGL(tsumsq, dim3(kNormBlocks), dim3(256), 0, st, (const float*)t->d_g, t->count, gchunk, g2p));
    KTRY(h, hipLaunchKernelGGL(tstats, dim3(1), dim3(256), 0, st, (const double*)t->dpart, kLossBlocks, (const double*)w2p, slot, (const double*)g2p, kNormBlocks,
                               cnt, tc.use_l1_loss, tc.l2_decay, tc.clipping_norm, t->d_stats, t->clip));
    return DCSCN_OK;
}

static int apply_update(dcscn_ctx* h, TrainState* t, double lr, hipStream_t st) {
    const dcscn_train_config& tc = t->tc;
    KTRY(h, hipLaunchKernelGGL(topt, dim3(grid1(t->count)), dim3(256), 0, st, tc.optimizer, t->d_w, (const float*)t->d_g, t->d_m, t->d_v, t->count,
                               (const float*)t->clip, (const float*)t->d_pw, (float)lr, (float)tc.beta1, (float)tc.beta2, (float)tc.epsilon, (float)tc.momentum));
    if (tc.optimizer == DCSCN_OPTIMIZER_ADAM) KTRY(h, hipLaunchKernelGGL(tpowers, dim3(1), dim3(1), 0, st, t->d_pw, (float)tc.beta1, (float)tc.beta2));
    t->stepped = true;
    return DCSCN_OK;
}

static int check_step(dcscn_ctx* h, const void* x, const void* x2, const void* y, int n, int H, int W) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!h->finalized) return fail(h, DCSCN_ERR_STATE, "training step before dcscn_finalize");
    if (!h->train) return fail(h, DCSCN_ERR_STATE, "training step before dcscn_train_begin");
    if (!x || !x2 || !y) return fail(h, DCSCN_ERR_INVALID_ARG, "training step: null buffer");
    if (n < 1 || H < 1 || W < 1) return fail(h, DCSCN_ERR_INVALID_ARG, "training step: bad shape %d x %d x %d", n, H, W);
    return DCSCN_OK;
}

// the four doubles of a step's stats (tstats) to the caller, who asked for them: synchronises `st`; stats == nullptr: nothing, the step stays enqueued
static int read_stats(dcscn_ctx* h, TrainState* t, double* stats, hipStream_t st) {
    if (!stats) return DCSCN_OK;
    HIP_TRY(h, hipMemcpyAsync(stats, t->d_stats, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    return DCSCN_OK;
}

// steps in host memory: upload, step, read the stats back
static int host_step(dcscn_ctx* h, const float* x, const float* x2, const float* y, int n, int H, int W, double lr, uint64_t key, double* stats, bool update) {
    int rc = check_step(h, x, x2, y, n, H, W);
    if (rc) return rc;
    TrainState* t = h->train;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = carve(h, t, n, H, W))) return rc;
    const int s = h->cfg.scale;
    const size_t lr_b = (size_t)n * H * W * 4, hr_b = lr_b * s * s;
    hipStream_t st = h->stream;
    HIP_TRY(h, hipMemcpyAsync(t->io_x, x, lr_b, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(t->io_x2, x2, hr_b, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(t->io_y, y, hr_b, hipMemcpyHostToDevice, st));
    if ((rc = run_gradients(h, t, t->io_x, t->io_x2, t->io_y, key, st))) return rc;
    if (update && (rc = apply_update(h, t, lr, st))) return rc;
    if (!stats) HIP_TRY(h, hipStreamSynchronize(st));     // (the uploads read the caller's buffers: done with them on return, stats or not)
    return read_stats(h, t, stats, st);
}

// later host-buffer steps, forwards and tensor reads run on the handle's stream: order it behind the caller's
static int join_stream(dcscn_ctx* h, hipStream_t st) {
    if (st == h->stream) return DCSCN_OK;
    TrainState* t = h->train;
    if (!t->join_ev) HIP_TRY(h, hipEventCreateWithFlags(&t->join_ev, hipEventDisableTiming));
    HIP_TRY(h, hipEventRecord(t->join_ev, st));
    HIP_TRY(h, hipStreamWaitEvent(h->stream, t->join_ev, 0));
    return DCSCN_OK;
}

static int check_record(dcscn_ctx* h, const void* rec, int64_t first_index, const char* what) {
    if (!rec) return fail(h, DCSCN_ERR_INVALID_ARG, "%s: null record buffer", what);
    if ((uintptr_t)rec % 16 != 0) return fail(h, DCSCN_ERR_INVALID_ARG, "%s: the record buffer is not 16-byte aligned", what);
    if (first_index < 0) return fail(h, DCSCN_ERR_INVALID_ARG, "%s: first_index %lld < 0", what, (long long)first_index);
    return DCSCN_OK;
}

// the gradient of the batch just run (d_g) and its stats as a record at `rec`, on `st`
static int write_record(dcscn_ctx* h, TrainState* t, int n, float* rec, hipStream_t st) {
    HIP_TRY(h, hipMemcpyAsync(rec, t->d_g, (size_t)t->count * 4, hipMemcpyDeviceToDevice, st));
    KTRY(h, hipLaunchKernelGGL(trecord_tail, dim3(1), dim3(1), 0, st, rec, t->count, (const double*)t->d_stats, (double)n));
    return join_stream(h, st);
}

void train_free(dcscn_ctx* h) {
    TrainState* t = h->train;
    if (!t) return;
    for (float* p : {t->d_w, t->d_g, t->d_m, t->d_v, t->d_wd, t->d_pw})
        if (p) (void)hipFree(p);
    if (t->d_red) (void)hipFree(t->d_red);
    if (t->join_ev) (void)hipEventDestroy(t->join_ev);
    if (t->arena) (void)hipFree(t->arena);
    delete t;
    h->train = nullptr;
}

// Before a forward on a handle whose variables a training step changed: bring them to the host copies and repack the inference plan.
int train_sync_inference(dcscn_ctx* h) {
    TrainState* t = h->train;
    if (!t || !t->stepped) return DCSCN_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<float> host((size_t)t->count);
    HIP_TRY(h, hipMemcpy(host.data(), t->d_w, host.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h->tensors.size(); ++i) {
        TensorSpec& ts = h->tensors[i];
        std::copy(host.begin() + t->off[i], host.begin() + t->off[i] + ts.data.size(), ts.data.begin());
    }
    int rc = repack_weights(h);
    if (rc) return rc;
    t->stepped = false;
    return DCSCN_OK;
}

}  // namespace dcscn_impl

extern "C" {

int dcscn_train_begin(dcscn_handle h, const dcscn_train_config* tc) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!tc) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_train_begin: null config");
    if (tc->struct_size != (int32_t)sizeof(dcscn_train_config))
        return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_train_begin: struct_size %d != %zu", tc->struct_size, sizeof(dcscn_train_config));
    if (!h->finalized) return fail(h, DCSCN_ERR_STATE, "dcscn_train_begin before dcscn_finalize");
    if (h->train) return fail(h, DCSCN_ERR_STATE, "dcscn_train_begin called twice on one handle");
    const dcscn_config& c = h->cfg;
    if (c.depthwise_separable) return fail(h, DCSCN_ERR_UNSUPPORTED, "training of depthwise separable nets is not implemented");
    if (!c.pixel_shuffler) return fail(h, DCSCN_ERR_UNSUPPORTED, "training of the transposed-conv upsampler (pixel_shuffler = false) is not implemented");
    if (c.batch_norm) return fail(h, DCSCN_ERR_UNSUPPORTED, "batch_norm is not implemented");
    switch (tc->optimizer) {
        case DCSCN_OPTIMIZER_ADAM: case DCSCN_OPTIMIZER_GD: case DCSCN_OPTIMIZER_MOMENTUM: break;
        case DCSCN_OPTIMIZER_ADADELTA: return fail(h, DCSCN_ERR_UNSUPPORTED, "optimizer adadelta is not implemented (supported: adam, gd, momentum)");
        case DCSCN_OPTIMIZER_ADAGRAD: return fail(h, DCSCN_ERR_UNSUPPORTED, "optimizer adagrad is not implemented (supported: adam, gd, momentum)");
        case DCSCN_OPTIMIZER_RMSPROP: return fail(h, DCSCN_ERR_UNSUPPORTED, "optimizer rmsprop is not implemented (supported: adam, gd, momentum)");
        default: return fail(h, DCSCN_ERR_INVALID_ARG, "unknown optimizer %d", tc->optimizer);
    }
    if (!(tc->keep_prob > 0.0 && tc->keep_prob <= 1.0)) return fail(h, DCSCN_ERR_INVALID_ARG, "keep_prob must be in (0, 1]");
    if (tc->l2_decay < 0.0 || tc->clipping_norm < 0.0) return fail(h, DCSCN_ERR_INVALID_ARG, "l2_decay and clipping_norm must be >= 0");
    TrainState* t = new (std::nothrow) TrainState();
    if (!t) return fail(h, DCSCN_ERR_NOMEM, "out of host memory");
    t->tc = *tc;
    h->train = t;
    int rc = build_train_plan(h, t);
    if (rc) { train_free(h); return rc; }
    for (const TensorSpec& ts : h->tensors) {
        t->off.push_back(t->count);
        t->count += (int64_t)ts.data.size();
        if (is_conv_w(ts.name)) t->w2_blocks += kW2Blocks;
    }
    std::vector<float> flat((size_t)t->count);
    for (size_t i = 0; i < h->tensors.size(); ++i) std::copy(h->tensors[i].data.begin(), h->tensors[i].data.end(), flat.begin() + t->off[i]);
    const size_t bytes = (size_t)t->count * 4;
    hipError_t e = hipSetDevice(h->device);
    for (float** p : {&t->d_w, &t->d_g, &t->d_m, &t->d_v, &t->d_wd})
        if (e == hipSuccess) e = hipMalloc(p, bytes);
    if (e == hipSuccess) e = hipMalloc(&t->d_pw, 2 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(t->d_w, flat.data(), bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(t->d_g, 0, bytes);
    if (e == hipSuccess) e = hipMemset(t->d_m, 0, bytes);
    if (e == hipSuccess) e = hipMemset(t->d_v, 0, bytes);
    t->h_pw[0] = (float)tc->beta1; t->h_pw[1] = (float)tc->beta2;      // TF: beta1_power / beta2_power start at beta1 / beta2
    if (e == hipSuccess) e = hipMemcpy(t->d_pw, t->h_pw, sizeof t->h_pw, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        train_free(h);
        return fail(h, DCSCN_ERR_HIP, "dcscn_train_begin: %s", hipGetErrorString(e));
    }
    return DCSCN_OK;
}

int dcscn_train_step(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width, double lr,
                     uint64_t dropout_key, double* stats) {
    return host_step(h, x, x2, y_true, n, height, width, lr, dropout_key, stats, true);
}

int dcscn_train_gradients(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width,
                          uint64_t dropout_key, double* stats) {
    return host_step(h, x, x2, y_true, n, height, width, 0.0, dropout_key, stats, false);
}

int dcscn_train_step_device(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width, double lr,
                            uint64_t dropout_key, double* stats, void* stream) {
    int rc = check_step(h, x, x2, y_true, n, height, width);
    if (rc) return rc;
    TrainState* t = h->train;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = carve(h, t, n, height, width))) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = run_gradients(h, t, x, x2, y_true, dropout_key, st))) return rc;
    if ((rc = apply_update(h, t, lr, st))) return rc;
    if ((rc = read_stats(h, t, stats, st))) return rc;
    return join_stream(h, st);
}

int dcscn_train_step_patches(dcscn_handle h, const dcscn_patch* patches, int n, int lr_size, double max_value, double lr, uint64_t dropout_key,
                             double* stats) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    int rc = check_patches(h, patches, n, lr_size, max_value);
    if (rc) return rc;
    TrainState* t = h->train;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = carve(h, t, n, lr_size, lr_size))) return rc;
    hipStream_t st = h->stream;
    if ((rc = build_batch_device(h, patches, n, lr_size, max_value, t->io_x, t->io_x2, t->io_y, st))) return rc;   // train_data.hip
    if ((rc = run_gradients(h, t, t->io_x, t->io_x2, t->io_y, dropout_key, st))) return rc;
    if ((rc = apply_update(h, t, lr, st))) return rc;
    return read_stats(h, t, stats, st);
}

int64_t dcscn_train_record_floats(dcscn_handle h) {
    if (!h) return 0;
    int64_t count = 0;
    for (const TensorSpec& ts : h->tensors) count += (int64_t)ts.data.size();
    return record_pad(count) + kRecordTrailer;
}

int dcscn_train_local_gradients_device(dcscn_handle h, const float* x, const float* x2, const float* y_true, int n, int height, int width,
                                       uint64_t dropout_key, int64_t first_index, float* record_out, void* stream) {
    int rc = check_step(h, x, x2, y_true, n, height, width);
    if (rc) return rc;
    if ((rc = check_record(h, record_out, first_index, "dcscn_train_local_gradients_device"))) return rc;
    TrainState* t = h->train;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = carve(h, t, n, height, width))) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = run_gradients(h, t, x, x2, y_true, dropout_key, st, first_index))) return rc;
    return write_record(h, t, n, record_out, st);
}

int dcscn_train_local_gradients_patches(dcscn_handle h, const dcscn_patch* patches, int n, int lr_size, double max_value, uint64_t dropout_key,
                                        int64_t first_index, float* record_out, void* stream) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    int rc = check_patches(h, patches, n, lr_size, max_value);
    if (rc) return rc;
    if ((rc = check_record(h, record_out, first_index, "dcscn_train_local_gradients_patches"))) return rc;
    TrainState* t = h->train;
    HIP_TRY(h, hipSetDevice(h->device));
    if ((rc = carve(h, t, n, lr_size, lr_size))) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = build_batch_device(h, patches, n, lr_size, max_value, t->io_x, t->io_x2, t->io_y, st))) return rc;   // train_data.hip
    if ((rc = run_gradients(h, t, t->io_x, t->io_x2, t->io_y, dropout_key, st, first_index))) return rc;
    return write_record(h, t, n, record_out, st);
}

int dcscn_train_apply_records(dcscn_handle h, const float* records, int world, double lr, double* stats, void* stream) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!h->finalized) return fail(h, DCSCN_ERR_STATE, "dcscn_train_apply_records before dcscn_finalize");
    if (!h->train) return fail(h, DCSCN_ERR_STATE, "dcscn_train_apply_records before dcscn_train_begin");
    if (world < 1) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_train_apply_records: world %d < 1", world);
    int rc = check_record(h, records, 0, "dcscn_train_apply_records");
    if (rc) return rc;
    TrainState* t = h->train;
    const dcscn_train_config& tc = t->tc;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    if ((rc = grow(h, &t->d_red, &t->red_cap, (size_t)kNormBlocks + 8 + (size_t)world, st))) return rc;
    double *g2p = t->d_red, *d_stats = g2p + kNormBlocks, *w = d_stats + 8;
    float* clip = reinterpret_cast<float*>(d_stats + 4);
    int* ok = reinterpret_cast<int*>(d_stats + 5);
    const int64_t pad = record_pad(t->count), rf = pad + kRecordTrailer;
    KTRY(h, hipLaunchKernelGGL(trank_weights, dim3(1), dim3(1), 0, st, records, world, rf, pad, w, ok));
    KTRY(h, hipLaunchKernelGGL(treduce_ranks, dim3(grid1(pad / 4)), dim3(256), 0, st, records, world, rf, t->count, (const double*)w, t->d_g));
    const int64_t gchunk = (t->count + kNormBlocks - 1) / kNormBlocks;
    KTRY(h, hipLaunchKernelGGL(tsumsq, dim3(kNormBlocks), dim3(256), 0, st, (const float*)t->d_g, t->count, gchunk, g2p));
    KTRY(h, hipLaunchKernelGGL(tstats_ranks, dim3(1), dim3(256), 0, st, records, world, rf, pad, (const double*)w, (const double*)g2p, kNormBlocks,
                               tc.clipping_norm, d_stats, clip));
    KTRY(h, hipLaunchKernelGGL(topt_ranks, dim3(grid1(t->count)), dim3(256), 0, st, (const int*)ok, tc.optimizer, t->d_w, (const float*)t->d_g, t->d_m,
                               t->d_v, t->count, (const float*)clip, (const float*)t->d_pw, (float)lr, (float)tc.beta1, (float)tc.beta2,
                               (float)tc.epsilon, (float)tc.momentum));
    if (tc.optimizer == DCSCN_OPTIMIZER_ADAM)
        KTRY(h, hipLaunchKernelGGL(tpowers_ranks, dim3(1), dim3(1), 0, st, (const int*)ok, t->d_pw, (float)tc.beta1, (float)tc.beta2));
    t->stepped = true;
    if ((rc = join_stream(h, st))) return rc;
    if (!stats) return DCSCN_OK;
    double host[6];
    HIP_TRY(h, hipMemcpyAsync(host, d_stats, sizeof host, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    int good;
    memcpy(&good, &host[5], sizeof good);
    if (!good) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_train_apply_records: a patch count of the %d records is not > 0, or their sum is not finite; nothing was updated", world);
    std::copy(host, host + 4, stats);
    return DCSCN_OK;
}

// "<var>", "<var>/grad", "<var>/Adam", "<var>/Adam_1", "<var>/Momentum", "beta1_power", "beta2_power"
static int train_tensor(dcscn_ctx* h, const char* name, float** dev, int64_t* count, bool* is_var) {
    TrainState* t = h->train;
    *is_var = false;
    if (!strcmp(name, "beta1_power") || !strcmp(name, "beta2_power")) {
        if (!t || t->tc.optimizer != DCSCN_OPTIMIZER_ADAM) return fail(h, DCSCN_ERR_SHAPE, "'%s' exists only while training with adam", name);
        *dev = t->d_pw + (name[4] == '1' ? 0 : 1);
        *count = 1;
        return DCSCN_OK;
    }
    std::string nm = name, suffix;
    auto it = h->tensor_index.find(nm);
    if (it == h->tensor_index.end()) {
        const size_t slash = nm.rfind('/');
        if (slash == std::string::npos) return fail(h, DCSCN_ERR_SHAPE, "unknown tensor '%s'", name);
        suffix = nm.substr(slash + 1);
        it = h->tensor_index.find(nm.substr(0, slash));
        if (it == h->tensor_index.end()) return fail(h, DCSCN_ERR_SHAPE, "unknown tensor '%s'", name);
    }
    const int i = it->second;
    *count = (int64_t)h->tensors[i].data.size();
    if (suffix.empty()) {
        *is_var = true;
        *dev = t ? t->d_w + t->off[i] : nullptr;
        return DCSCN_OK;
    }
    if (!t) return fail(h, DCSCN_ERR_STATE, "'%s' exists only after dcscn_train_begin", name);
    const int opt = t->tc.optimizer;
    if (suffix == "grad") *dev = t->d_g + t->off[i];
    else if (suffix == "Adam" && opt == DCSCN_OPTIMIZER_ADAM) *dev = t->d_m + t->off[i];
    else if (suffix == "Adam_1" && opt == DCSCN_OPTIMIZER_ADAM) *dev = t->d_v + t->off[i];
    else if (suffix == "Momentum" && opt == DCSCN_OPTIMIZER_MOMENTUM) *dev = t->d_m + t->off[i];
    else return fail(h, DCSCN_ERR_SHAPE, "unknown tensor '%s' for this optimizer", name);
    return DCSCN_OK;
}

int dcscn_get_tensor(dcscn_handle h, const char* name, float* out, int64_t count) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!name || !out) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_get_tensor: null argument");
    float* dev = nullptr;
    int64_t n = 0;
    bool is_var;
    int rc = train_tensor(h, name, &dev, &n, &is_var);
    if (rc) return rc;
    if (count != n) return fail(h, DCSCN_ERR_SHAPE, "tensor '%s' has %lld values, not %lld", name, (long long)n, (long long)count);
    if (!dev) {   // a variable of a handle that is not training: the host copy
        const TensorSpec& ts = h->tensors[h->tensor_index[name]];
        if (!ts.set) return fail(h, DCSCN_ERR_MISSING_TENSOR, "variable '%s' was never set", name);
        std::copy(ts.data.begin(), ts.data.end(), out);
        return DCSCN_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(out, dev, (size_t)n * 4, hipMemcpyDeviceToHost));
    return DCSCN_OK;
}

int dcscn_set_train_tensor(dcscn_handle h, const char* name, const float* data, int64_t count) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!name || !data) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_set_train_tensor: null argument");
    if (!h->train) return fail(h, DCSCN_ERR_STATE, "dcscn_set_train_tensor before dcscn_train_begin");
    if (strlen(name) > 5 && !strcmp(name + strlen(name) - 5, "/grad")) return fail(h, DCSCN_ERR_SHAPE, "gradients are not settable");
    float* dev = nullptr;
    int64_t n = 0;
    bool is_var;
    int rc = train_tensor(h, name, &dev, &n, &is_var);
    if (rc) return rc;
    if (count != n) return fail(h, DCSCN_ERR_SHAPE, "tensor '%s' has %lld values, not %lld", name, (long long)n, (long long)count);
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(data[i])) return fail(h, DCSCN_ERR_INVALID_ARG, "tensor '%s' holds a non-finite value", name);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(dev, data, (size_t)n * 4, hipMemcpyHostToDevice));
    if (is_var) h->train->stepped = true;
    return DCSCN_OK;
}

}  // extern "C"
