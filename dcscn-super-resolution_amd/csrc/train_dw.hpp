// The depthwise stage of a separable conv layer in training (option "train_separable"; tf.nn.separable_conv2d, tf_graph.py:155-177):
//   d = depthwise k x k SAME (in; dw[k][k][cin][1]),  z = d . pointwise[cin][cout] + bias.
// The pointwise stage is train.hip's conv machinery with ks = 1 on d; here are the depthwise forward and its two gradients.  All three are
// memory-bound f32 VALU kernels over NHWC tensors.  `in` is a channel slice of a concat buffer (stride in_stride, any offset: nothing about
// its alignment is assumed), d and dd are dense [pixels][cin].  Element e = pixel * cin + channel is the thread index, so a wave reads
// consecutive channels of a pixel and, with cin = 1 (CNN1, and R-CNN1 at HR), consecutive pixels.  Every product-sum is an explicit fmaf
// chain from 0 in tap order (taps outside the image are skipped: they would add an exact 0); included by train.hip behind train_kernels.hpp,
// so fp contract(off) holds here too.
#pragma once
#include "train_kernels.hpp"

namespace dcscn_impl {

struct TDwArgs {
    const float* in; int in_stride; int cin;
    int n, H, W, ks;
    const float* dw;        // [ks*ks][cin]
};

// pixel q = (img, y, x) of an [n][H][W] tensor; 32-bit divisions where q allows (64-bit ones cost several times as much, and these
// kernels have little else to do)
__device__ inline void tdw_pixel(int64_t q, int H, int W, int* x, int* y, int64_t* img) {
    if (q <= 0x7fffffff) {
        const unsigned u = (unsigned)q, r = u / (unsigned)W, i = r / (unsigned)H;
        *x = (int)(u - r * (unsigned)W); *y = (int)(r - i * (unsigned)H); *img = i;
    } else {
        *x = (int)(q % W); *y = (int)((q / W) % H); *img = q / ((int64_t)W * H);
    }
}
// element e = (pixel q, channel c) of a dense [pixels][cin] tensor
__device__ inline void tdw_element(int64_t e, int cin, int64_t* q, int* c) {
    if (e <= 0x7fffffff) {
        const unsigned u = (unsigned)e, p = u / (unsigned)cin;
        *q = p; *c = (int)(u - p * (unsigned)cin);
    } else {
        *q = e / cin; *c = (int)(e % cin);
    }
}

// d[p][c] = sum_t in[p + t][c] * dw[t][c]
__global__ __launch_bounds__(256) void tdw_fwd(const TDwArgs a, float* d) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)a.n * a.H * a.W * a.cin) return;
    int c, x, y;
    int64_t q, img;
    tdw_element(e, a.cin, &q, &c);
    tdw_pixel(q, a.H, a.W, &x, &y, &img);
    const int pad = a.ks / 2;
    float acc = 0.0f;
    for (int kh = 0; kh < a.ks; ++kh) {
        const int yy = y + kh - pad;
        if (yy < 0 || yy >= a.H) continue;
        for (int kw = 0; kw < a.ks; ++kw) {
            const int xx = x + kw - pad;
            if (xx < 0 || xx >= a.W) continue;
            acc = fmaf(a.in[((img * a.H + yy) * a.W + xx) * a.in_stride + c], a.dw[(kh * a.ks + kw) * a.cin + c], acc);
        }
    }
    d[e] = acc;
}

// gin[p][c] += sum_t dd[p - t][c] * dw[t][c]: the data gradient, accumulated into the input's gradient slice (a.in = gin, written); one thread
// owns an element
__global__ __launch_bounds__(256) void tdw_dgrad(const TDwArgs a, const float* dd) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)a.n * a.H * a.W * a.cin) return;
    int c, x, y;
    int64_t q, img;
    tdw_element(e, a.cin, &q, &c);
    tdw_pixel(q, a.H, a.W, &x, &y, &img);
    const int pad = a.ks / 2;
    float acc = 0.0f;
    for (int kh = 0; kh < a.ks; ++kh) {
        const int yy = y - (kh - pad);
        if (yy < 0 || yy >= a.H) continue;
        for (int kw = 0; kw < a.ks; ++kw) {
            const int xx = x - (kw - pad);
            if (xx < 0 || xx >= a.W) continue;
            acc = fmaf(dd[((img * a.H + yy) * a.W + xx) * a.cin + c], a.dw[(kh * a.ks + kw) * a.cin + c], acc);
        }
    }
    float* g = const_cast<float*>(a.in) + q * a.in_stride + c;
    *g = *g + acc;
}

// The pixel split of the depthwise weight gradient, fixed by the shape alone: a workgroup is cw channels (a power of two <= 64) by 256 / cw
// pixel rows; a split is about 32 pixels per row, at most 128 splits.
inline int dw_splits(int cin, int64_t P, int* cw, int64_t* chunk) {
    int w = 1;
    while (w < cin && w < 64) w <<= 1;
    const int64_t per = (int64_t)(256 / w) * 32;
    int64_t s = std::max<int64_t>(1, std::min<int64_t>(128, (P + per - 1) / per));
    const int64_t ch = (P + s - 1) / s;
    s = (P + ch - 1) / ch;
    *cw = w; *chunk = ch;
    return (int)s;
}

// part[s][t][c] = sum over the pixels p of split s of in[p + t][c] * dd[p][c].  Workgroup (tap, channel group, split): thread (row, channel)
// takes the split's pixels row, row + rows, ... in order (an fmaf chain), then the rows of a channel are summed by an LDS tree of fixed shape.
// treduce_wgrad sums the splits in order.
__global__ __launch_bounds__(256) void tdw_wgrad(const TDwArgs a, const float* dd, int cw, int64_t chunk, float* part) {
    __shared__ float red[256];
    const int t = threadIdx.x, rows = 256 / cw, row = t / cw;
    const int tap = blockIdx.x, c = blockIdx.y * cw + (t & (cw - 1));
    const int pad = a.ks / 2, dy = tap / a.ks - pad, dx = tap % a.ks - pad;
    const int64_t P = (int64_t)a.n * a.H * a.W;
    const int64_t p0 = (int64_t)blockIdx.z * chunk;
    const int64_t p1 = p0 + chunk < P ? p0 + chunk : P;
    float acc = 0.0f;
    if (c < a.cin)
        for (int64_t p = p0 + row; p < p1; p += rows) {
            int xx, yy;
            int64_t img;
            tdw_pixel(p, a.H, a.W, &xx, &yy, &img);
            xx += dx; yy += dy;
            if (xx < 0 || xx >= a.W || yy < 0 || yy >= a.H) continue;
            acc = fmaf(a.in[((img * a.H + yy) * a.W + xx) * a.in_stride + c], dd[p * a.cin + c], acc);
        }
    red[t] = acc;
    __syncthreads();
    for (int o = 128; o >= cw; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t < cw && c < a.cin) part[((size_t)blockIdx.z * a.ks * a.ks + tap) * a.cin + c] = red[t];
}

}  // namespace dcscn_impl
