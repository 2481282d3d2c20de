// PSNR and SSIM of an evaluated image on the device (helper/utilty.py:509-536 of the reference; imaging.compute_psnr_and_ssim
// is the host restatement).  Both images are trimmed on load -- min(max(rint(v), 0), 255), round-half-to-even in double, an
// integer 0..255 -- and shaved by `border` pixels on every side.
//   squared error   exact: the int64 sum of squared integer differences over every shaved pixel; the PSNR is formed from it
//                   and the pixel count on the host, so it has the host's bits.
//   SSIM            the reference hands 2-D arrays to scikit-image with multichannel=True, so its "SSIM" is the mean over
//                   image columns of a 1-D SSIM down each column (imaging._ssim_last_axis_channels): an 11-tap Gaussian
//                   (sigma 1.5, truncated at 3.5 sigma) of a, b, a^2, b^2, ab, sample covariance with 11/10, and only rows
//                   whose window lies wholly inside the image enter the mean -- rows [5, h - 5).  No border handling exists.
// Order of the sums (fixed, no atomics, so two runs give the same bits): each filtered value is the in-order sum of its 11
// products; a thread adds the S of its segment's rows top to bottom; the final workgroup adds a column's segments top to
// bottom, divides by the row count, and thread t adds the means of columns t, t + 256, ... in order, then an LDS tree.
// This file is compiled with -ffp-contract=off: every product and sum rounds once, as numpy's do.
// a, b, a^2, b^2 and ab are integers below 2^16 and exact in double; everything else is float64 arithmetic.
#include "kernels.h"

namespace dcscn {

namespace {

constexpr int kWin = kMetricTaps, kPad = kWin / 2;
constexpr int kSegRows = 16;       // output rows per thread: a thread reads kSegRows + 10 rows of both images

__device__ __forceinline__ int trim_load(const double* p64, const float* p32, long long i) {
    const double v = p32 ? (double)p32[i] : p64[i];
    return (int)fmin(fmax(rint(v), 0.0), 255.0);
}

// One thread = one shaved column x one segment of kSegRows SSIM rows; lanes of a wave own adjacent columns (coalesced rows).
// part_s[seg * w + col] = sum of S over the segment's rows; part_e[seg * w + col] = squared error of the segment's pixel
// rows, where the first segment also takes the 5 rows above the first SSIM row and the last one the 5 rows below the last.
__global__ __launch_bounds__(64) void metric_columns(const double* __restrict__ a64, const float* __restrict__ a32,
                                                     const double* __restrict__ b64, const float* __restrict__ b32, int stride,
                                                     int border, int h, int w, MetricWeights wt, double* __restrict__ part_s,
                                                     long long* __restrict__ part_e) {
    const int col = blockIdx.x * 64 + threadIdx.x;
    if (col >= w) return;
    const int seg = blockIdx.y, nseg = gridDim.y;
    const int r0 = kPad + seg * kSegRows;                         // SSIM rows [r0, r1) of the shaved image
    const int r1 = min(r0 + kSegRows, h - kPad);
    const bool first = seg == 0, last = seg == nseg - 1;
    const double cov_norm = (double)kWin / (kWin - 1.0);
    const double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
    double wa[kWin] = {}, wb[kWin] = {};
    double sum_s = 0.0;
    long long sum_e = 0;
    const long long base = (long long)border * stride + border + col;
    for (int i = r0 - kPad; i < r1 + kPad; ++i) {                 // rows [0, h): r0 >= 5 and r1 <= h - 5
        const long long at = base + (long long)i * stride;
        const int ia = trim_load(a64, a32, at), ib = trim_load(b64, b32, at);
        if ((i >= r0 && i < r1) || (first && i < r0) || (last && i >= r1)) sum_e += (long long)((ia - ib) * (ia - ib));
#pragma unroll
        for (int k = 0; k < kWin - 1; ++k) { wa[k] = wa[k + 1]; wb[k] = wb[k + 1]; }
        wa[kWin - 1] = (double)ia;
        wb[kWin - 1] = (double)ib;
        if (i < r0 + kPad) continue;                              // the window [i - 10, i] is not full yet
        double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            ux += wt.w[k] * wa[k];
            uy += wt.w[k] * wb[k];
            uxx += wt.w[k] * (wa[k] * wa[k]);
            uyy += wt.w[k] * (wb[k] * wb[k]);
            uxy += wt.w[k] * (wa[k] * wb[k]);
        }
        const double vx = cov_norm * (uxx - ux * ux);
        const double vy = cov_norm * (uyy - uy * uy);
        const double vxy = cov_norm * (uxy - ux * uy);
        sum_s += ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
    }
    part_s[(long long)seg * w + col] = sum_s;
    part_e[(long long)seg * w + col] = sum_e;
}

// One workgroup.  out[0] = int64 squared-error total, out[1] = int64 pixel count, out[2] = the SSIM as a double's bits.
__global__ __launch_bounds__(256) void metric_final(const double* __restrict__ part_s, const long long* __restrict__ part_e, int nseg, int h,
                                                    int w, long long* __restrict__ out) {
    __shared__ double rs[256];
    __shared__ long long re[256];
    const int t = threadIdx.x;
    const double rows = (double)(h - 2 * kPad);
    double s = 0.0;
    long long e = 0;
    for (int col = t; col < w; col += 256) {
        double cs = 0.0;
#pragma unroll 8
        for (int seg = 0; seg < nseg; ++seg) {                     // (unrolled: the loads of eight segments are in flight together)
            cs += part_s[(long long)seg * w + col];
            e += part_e[(long long)seg * w + col];
        }
        s += cs / rows;
    }
    rs[t] = s;
    re[t] = e;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { rs[t] += rs[t + o]; re[t] += re[t + o]; }
        __syncthreads();
    }
    if (t != 0) return;
    out[0] = re[0];
    out[1] = (long long)h * w;
    out[2] = __double_as_longlong(rs[0] / (double)w);
}

}  // namespace

int metric_segments(int h) { return (h - 2 * kPad + kSegRows - 1) / kSegRows; }

hipError_t metrics_launch(const double* a64, const float* a32, const double* b64, const float* b32, int stride, int border, int h, int w,
                          const MetricWeights& wt, double* part_s, long long* part_e, long long* out, hipStream_t stream) {
    if (h < kWin || w < 1) return hipErrorInvalidValue;
    const int nseg = metric_segments(h);
    hipLaunchKernelGGL(metric_columns, dim3((unsigned)((w + 63) / 64), (unsigned)nseg), dim3(64), 0, stream, a64, a32, b64, b32, stride, border, h,
                       w, wt, part_s, part_e);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(metric_final, dim3(1), dim3(256), 0, stream, (const double*)part_s, (const long long*)part_e, nseg, h, w, out);
    return hipGetLastError();
}

}  // namespace dcscn
