// The kernels and device helpers of train.hip, which is the only source that includes this file (one translation unit).  Everything here and
// in train.hip behind the include is compiled with fp contract(off): every multiply, add, divide and sqrt is one IEEE operation with one rounding
// (tests/train_ref.py restates them with no tolerance).
#pragma once
#include "plan.h"

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

// The sums over a 256-thread workgroup of the N values every thread holds, left in red[k][0]: an LDS tree of fixed shape (thread t adds slot
// t + o, o = 128 ... 1, a barrier per level), so the order of the additions never depends on the run.
template <class T, int N>
__device__ inline void block_sum(T (&red)[N][256], const T (&v)[N]) {
    const int t = threadIdx.x;
    for (int k = 0; k < N; ++k) red[k][t] = v[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o)
            for (int k = 0; k < N; ++k) red[k][t] += red[k][t + o];
        __syncthreads();
    }
}

// tf.clip_by_global_norm's factor; clip_norm = 0: no clipping.  norm <= clip_norm gives c / c = 1 exactly.
__device__ inline float clip_factor(float norm, double clip_norm) {
    const float c = (float)clip_norm;
    return clip_norm > 0.0 ? c / fmaxf(norm, c) : 1.0f;
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
    __shared__ float red[1][256];
    const int co = blockIdx.x;
    const int64_t p0 = (int64_t)blockIdx.y * chunk;
    const int64_t p1 = p0 + chunk < P ? p0 + chunk : P;
    float s = 0.0f;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) s += v[p * cout + co];
    block_sum(red, {s});
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * cout + co] = red[0][0];
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
    __shared__ double r[2][256];
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
    block_sum(r, {s2, s1});
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = r[0][0]; part[2 * blockIdx.x + 1] = r[1][0]; }
}

// sum of squares of v[0, count) per block (float64, fixed order) into part[slot0 + block]
__global__ __launch_bounds__(256) void tsumsq(const float* v, int64_t count, int64_t chunk, double* part) {
    __shared__ double r[1][256];
    const int64_t p0 = (int64_t)blockIdx.x * chunk;
    const int64_t p1 = p0 + chunk < count ? p0 + chunk : count;
    double s = 0.0;
    for (int64_t e = p0 + threadIdx.x; e < p1; e += 256) s += (double)v[e] * v[e];
    block_sum(r, {s});
    if (threadIdx.x == 0) part[blockIdx.x] = r[0][0];
}

// stats[0] image_loss, [1] mse, [2] global gradient norm (before clipping), [3] total loss; clip[0] = clip_by_global_norm factor.
// One workgroup: thread t sums partials t, t + 256, ... in order, then block_sum -- deterministic.
__global__ __launch_bounds__(256) void tstats(const double* loss_part, int loss_blocks, const double* w2_part, int w2_blocks, const double* g2_part,
                                              int g2_blocks, int64_t count, int l1, double l2_decay, double clip_norm, double* stats, float* clip) {
    __shared__ double r[4][256];
    const int t = threadIdx.x;
    double s2 = 0.0, s1 = 0.0, w2 = 0.0, g2 = 0.0;
    for (int b = t; b < loss_blocks; b += 256) { s2 += loss_part[2 * b]; s1 += loss_part[2 * b + 1]; }
    for (int b = t; b < w2_blocks; b += 256) w2 += w2_part[b];
    for (int b = t; b < g2_blocks; b += 256) g2 += g2_part[b];
    block_sum(r, {s2, s1, w2, g2});
    if (t != 0) return;
    const double mse = r[0][0] / (double)count, image = l1 ? r[1][0] / (double)count : mse;
    const float norm = (float)sqrt(r[3][0]);
    stats[0] = image; stats[1] = mse; stats[2] = norm; stats[3] = image + l2_decay * 0.5 * r[2][0];
    clip[0] = clip_factor(norm, clip_norm);
}

// one optimizer step over the flat buffers (TF's ApplyAdam / ApplyGradientDescent / ApplyMomentum), g scaled by the clip factor.  ok: null,
// or the device flag of a reduction (trank_weights): nothing moves when the records' patch counts did not form a batch (ok[0] = 0)
__global__ void topt(const int* ok, int kind, float* w, const float* g, float* m, float* v, int64_t count, const float* clip, const float* pw,
                     float lr, float b1, float b2, float eps, float mu) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count || (ok && !ok[0])) return;
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
// The three rules behind option "train_optimizers" (adagrad, adadelta, rmsprop), which topt does not know: same ok gate, clip scaling, flat
// buffers and grid.  The reference constructs the optimizers with TF 1.x's defaults (DCSCN.py:383-392), so the constants are fixed here:
// AdadeltaOptimizer rho 0.95, epsilon 1e-8; AdagradOptimizer initial_accumulator_value 0.1 (filled by dcscn_train_begin);
// RMSPropOptimizer decay 0.9, epsilon 1e-10, not centred, momentum = --momentum (mu).  Each rule takes its operations in the order of TF's
// ApplyAdagrad / ApplyAdadelta / ApplyRMSProp functors, one float32 rounding per operation (train.hip: fp contract(off)).
static constexpr float kAdadeltaRho = 0.95f, kAdadeltaEps = 1e-8f, kAdagradInitialAccumulator = 0.1f;
static constexpr float kRmsPropDecay = 0.9f, kRmsPropEps = 1e-10f, kRmsPropInitialMs = 1.0f;
__global__ void topt_more(const int* ok, int kind, float* w, const float* g, float* m, float* v, int64_t count, const float* clip, float lr, float mu) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count || (ok && !ok[0])) return;
    const float gg = g[e] * clip[0];
    if (kind == DCSCN_OPTIMIZER_ADAGRAD) {            // m: <var>/Adagrad
        const float a = m[e] + gg * gg;
        m[e] = a;
        w[e] = w[e] - lr * gg * (1.0f / sqrtf(a));
    } else if (kind == DCSCN_OPTIMIZER_ADADELTA) {    // m: <var>/Adadelta (accum), v: <var>/Adadelta_1 (accum_update)
        const float rho = kAdadeltaRho, eps = kAdadeltaEps;
        const float a = m[e] * rho + gg * gg * (1.0f - rho);
        const float u = sqrtf(v[e] + eps) * (1.0f / sqrtf(a + eps)) * gg;
        w[e] = w[e] - u * lr;
        v[e] = v[e] * rho + u * u * (1.0f - rho);
        m[e] = a;
    } else {                                          // DCSCN_OPTIMIZER_RMSPROP; m: <var>/RMSProp (ms), v: <var>/RMSProp_1 (mom)
        const float s = m[e] + (gg * gg - m[e]) * (1.0f - kRmsPropDecay);
        const float q = v[e] * mu + (gg * lr) / sqrtf(s + kRmsPropEps);
        w[e] = w[e] - q;
        m[e] = s;
        v[e] = q;
    }
}
// beta1_power / beta2_power behind an adam step; ok as topt's
__global__ void tpowers(const int* ok, float* pw, float b1, float b2) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && (!ok || ok[0])) { pw[0] = pw[0] * b1; pw[1] = pw[1] * b2; }
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
    __shared__ double r[1][256];
    const int t = threadIdx.x;
    double g2 = 0.0;
    for (int b = t; b < g2_blocks; b += 256) g2 += g2_part[b];
    block_sum(r, {g2});
    if (t != 0) return;
    const double* tr = reinterpret_cast<const double*>(records + pad);
    double image = w[0] * tr[0], mse = w[0] * tr[1], total = w[0] * tr[3];
    for (int k = 1; k < world; ++k) {
        tr = reinterpret_cast<const double*>(records + (size_t)k * rf + pad);
        image += w[k] * tr[0]; mse += w[k] * tr[1]; total += w[k] * tr[3];
    }
    const float norm = (float)sqrt(r[0][0]);
    stats[0] = image; stats[1] = mse; stats[2] = norm; stats[3] = total;
    clip[0] = clip_factor(norm, clip_norm);
}

}  // namespace dcscn_impl
