// TensorBoard summary records reduced on the device: what util.add_summaries (helper/utilty.py:427-443) asks TensorFlow for -- mean, stddev and
// the histogram of a tensor -- as one record per tensor (include/dcscn.h: dcscn_summary), so that a log pass downloads 12 KiB per tensor
// instead of the tensor.
//
// Three launches per tensor, all over the same fixed partition of the values into at most kSummaryMaxBlocks contiguous chunks (a function of
// the count alone), one workgroup per chunk:
//   tsummary_pass1   per chunk: num, nonfinite, min, max, the double sums of v and v^2; the bucket of every finite value by a binary search of
//                    the limit table in LDS (the exact upper_bound: no logarithm, no guess), counted in an LDS histogram with integer atomics
//                    and added to the tensor's int64 counts with integer atomics, which commute exactly
//   tsummary_pass2   every workgroup adds the chunks' partial results in chunk order (all get the same bits), forms mean = sum / num, and sums
//                    (v - mean)^2 in double over its chunk; workgroup 0 writes the first pass's fields of the record
//   tsummary_final   the chunks' sums in chunk order; stddev = sqrt(total / num)
// A thread adds its values in index order, the lanes of a wave combine in a fixed shuffle tree and the waves in wave order: no floating-point
// atomic, two runs give the same bits.  Values are read one float at a time: the pointer needs float alignment only.
#include "summary.hpp"

#include <cfloat>
#include <mutex>

namespace dcscn_impl {

#pragma clang fp contract(off)

struct SumPart {
    double sum, sumsq;
    float mn, mx;
    long long num, nonfinite;
};

__device__ double g_summary_limits[kSummaryBuckets];

const double* summary_limits() {
    static std::vector<double> limits;
    static std::once_flag once;
    std::call_once(once, [] {
        std::vector<double> pos;
        double v = 1e-12;
        while (v < 1e20) {
            pos.push_back(v);
            v *= 1.1;
        }
        std::vector<double> l;
        l.push_back(-DBL_MAX);
        for (size_t i = pos.size(); i-- > 0;) l.push_back(-pos[i]);
        l.push_back(0.0);
        for (double p : pos) l.push_back(p);
        l.push_back(DBL_MAX);
        limits.swap(l);
    });
    return limits.data();
}

hipError_t summary_prepare_device(int device) {
    static std::mutex mu;
    static std::vector<char> done;
    std::lock_guard<std::mutex> lock(mu);
    if (device >= 0 && (size_t)device < done.size() && done[device]) return hipSuccess;
    // (blocking copy to the symbol of the current device: the table is in place before any later launch on any stream)
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_summary_limits), summary_limits(), sizeof(double) * kSummaryBuckets);
    if (e != hipSuccess) return e;
    if (device >= 0) {
        if ((size_t)device >= done.size()) done.resize(device + 1, 0);
        done[device] = 1;
    }
    return hipSuccess;
}

size_t summary_scratch_bytes() { return kSummaryMaxBlocks * (sizeof(SumPart) + sizeof(double)); }

__device__ __forceinline__ float view_load(const SummaryView& v, int64_t i) {
    if (v.C == v.stride) return v.p[i];
    if (v.count <= 0x7fffffff) {   // (32-bit division where it suffices)
        const uint32_t r = (uint32_t)i / (uint32_t)v.C;
        return v.p[(int64_t)r * v.stride + ((uint32_t)i - r * (uint32_t)v.C)];
    }
    const int64_t r = i / v.C;
    return v.p[r * v.stride + (i - r * v.C)];
}

// sum over the workgroup (256 threads = 4 waves) in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double x, double* lds) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    return threadIdx.x == 0 ? ((lds[0] + lds[1]) + lds[2]) + lds[3] : 0.0;
}

__global__ __launch_bounds__(256) void tsummary_pass1(SummaryView v, int64_t chunk, SumPart* parts, unsigned long long* buckets) {
    __shared__ double lim[kSummaryBuckets];
    __shared__ unsigned hist[kSummaryBuckets];
    __shared__ double red[4];
    __shared__ float redf[8];
    __shared__ long long redi[8];
    for (int i = threadIdx.x; i < kSummaryBuckets; i += 256) {
        lim[i] = g_summary_limits[i];
        hist[i] = 0u;
    }
    __syncthreads();
    const int64_t begin = (int64_t)blockIdx.x * chunk, end = begin + chunk < v.count ? begin + chunk : v.count;
    double sum = 0.0, sumsq = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    long long num = 0, bad = 0;
    int cur = -1;
    unsigned run = 0;   // values in a row that fell into bucket `cur`: one LDS atomic per run (an all-zero tensor is one run per thread)
    for (int64_t i = begin + threadIdx.x; i < end; i += 256) {
        const float f = view_load(v, i);
        if (!(fabsf(f) <= FLT_MAX)) { ++bad; continue; }   // NaN, +Inf, -Inf
        const double d = (double)f;
        ++num;
        sum += d;
        sumsq += d * d;
        mn = fminf(mn, f);
        mx = fmaxf(mx, f);
        int lo = 0, hi = kSummaryBuckets;   // upper_bound: the first limit > d
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (lim[mid] <= d) lo = mid + 1; else hi = mid;
        }
        if (lo > kSummaryBuckets - 1) lo = kSummaryBuckets - 1;   // (unreachable: every finite float is below DBL_MAX)
        if (lo == cur) ++run;
        else {
            if (run) atomicAdd(&hist[cur], run);
            cur = lo;
            run = 1;
        }
    }
    if (run) atomicAdd(&hist[cur], run);
    // min, max and the integer counts: order does not matter for them
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_down(mn, o, 64));
        mx = fmaxf(mx, __shfl_down(mx, o, 64));
        num += __shfl_down(num, o, 64);
        bad += __shfl_down(bad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        redf[w] = mn; redf[4 + w] = mx; redi[w] = num; redi[4 + w] = bad;
    }
    const double s1 = block_sum(sum, red);      // (its barriers publish redf / redi and the histogram as well)
    const double s2 = block_sum(sumsq, red);
    if (threadIdx.x == 0) {
        SumPart p;
        p.sum = s1; p.sumsq = s2;
        p.mn = fminf(fminf(redf[0], redf[1]), fminf(redf[2], redf[3]));
        p.mx = fmaxf(fmaxf(redf[4], redf[5]), fmaxf(redf[6], redf[7]));
        p.num = redi[0] + redi[1] + redi[2] + redi[3];
        p.nonfinite = redi[4] + redi[5] + redi[6] + redi[7];
        parts[blockIdx.x] = p;
    }
    for (int i = threadIdx.x; i < kSummaryBuckets; i += 256)
        if (hist[i]) atomicAdd(&buckets[i], (unsigned long long)hist[i]);
}

__global__ __launch_bounds__(256) void tsummary_pass2(SummaryView v, int64_t chunk, const SumPart* parts, double* ss_parts, dcscn_summary* rec) {
    __shared__ double red[4];
    __shared__ double s_mean;
    if (threadIdx.x == 0) {
        double sum = 0.0, sumsq = 0.0;
        float mn = INFINITY, mx = -INFINITY;
        long long num = 0, bad = 0;
        for (unsigned b = 0; b < gridDim.x; ++b) {
            const SumPart p = parts[b];
            sum += p.sum; sumsq += p.sumsq;
            mn = fminf(mn, p.mn); mx = fmaxf(mx, p.mx);
            num += p.num; bad += p.nonfinite;
        }
        const double mean = num > 0 ? sum / (double)num : 0.0;
        s_mean = mean;
        if (blockIdx.x == 0) {
            rec->num = num; rec->nonfinite = bad;
            rec->min = num > 0 ? (double)mn : 0.0; rec->max = num > 0 ? (double)mx : 0.0;
            rec->sum = sum; rec->sum_squares = sumsq; rec->mean = mean;
        }
    }
    __syncthreads();
    const double mean = s_mean;
    const int64_t begin = (int64_t)blockIdx.x * chunk, end = begin + chunk < v.count ? begin + chunk : v.count;
    double ss = 0.0;
    for (int64_t i = begin + threadIdx.x; i < end; i += 256) {
        const float f = view_load(v, i);
        if (!(fabsf(f) <= FLT_MAX)) continue;
        const double d = (double)f - mean;
        ss += d * d;
    }
    const double s = block_sum(ss, red);
    if (threadIdx.x == 0) ss_parts[blockIdx.x] = s;
}

__global__ void tsummary_final(const double* ss_parts, int nblocks, dcscn_summary* rec) {
    double total = 0.0;
    for (int b = 0; b < nblocks; ++b) total += ss_parts[b];
    rec->stddev = rec->num > 0 ? sqrt(total / (double)rec->num) : 0.0;
}

hipError_t launch_summary(const SummaryView& v, void* scratch, dcscn_summary* rec, int64_t* buckets, hipStream_t st) {
    if (v.count < 1) return hipSuccess;   // the zeroed record stands
    int64_t blocks = (v.count + kSummaryBlockValues - 1) / kSummaryBlockValues;
    if (blocks > kSummaryMaxBlocks) blocks = kSummaryMaxBlocks;
    const int64_t chunk = (v.count + blocks - 1) / blocks;
    blocks = (v.count + chunk - 1) / chunk;   // (no empty chunk)
    SumPart* parts = static_cast<SumPart*>(scratch);
    double* ss_parts = reinterpret_cast<double*>(parts + kSummaryMaxBlocks);
    hipLaunchKernelGGL(tsummary_pass1, dim3((unsigned)blocks), dim3(256), 0, st, v, chunk, parts, reinterpret_cast<unsigned long long*>(buckets));
    hipLaunchKernelGGL(tsummary_pass2, dim3((unsigned)blocks), dim3(256), 0, st, v, chunk, (const SumPart*)parts, ss_parts, rec);
    hipLaunchKernelGGL(tsummary_final, dim3(1), dim3(1), 0, st, (const double*)ss_parts, (int)blocks, rec);
    return hipGetLastError();
}

}  // namespace dcscn_impl

using namespace dcscn_impl;

extern "C" {

int dcscn_summary_bucket_limits(double* out, int capacity) {
    if (out && capacity > 0) std::copy(summary_limits(), summary_limits() + std::min(capacity, kSummaryBuckets), out);
    return kSummaryBuckets;
}

int dcscn_summarize_device(dcscn_handle h, const float* data, int64_t count, dcscn_summary* out, int64_t* buckets, int capacity, void* stream) {
    if (!h) return DCSCN_ERR_INVALID_ARG;
    if (!data || !out) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_summarize_device: null pointer");
    if (count < 1) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_summarize_device: count %lld < 1", (long long)count);
    if ((uintptr_t)data % alignof(float) != 0) return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_summarize_device: the data pointer is not float-aligned");
    if (buckets && capacity < kSummaryBuckets)
        return fail(h, DCSCN_ERR_INVALID_ARG, "dcscn_summarize_device: room for %d bucket counts, %d needed", capacity, kSummaryBuckets);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, summary_prepare_device(h->device));
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    // one allocation: the record, the counts, the scratch
    const size_t head = sizeof(dcscn_summary) + sizeof(int64_t) * kSummaryBuckets, bytes = head + summary_scratch_bytes();
    char* dev = nullptr;
    hipError_t e = hipMalloc((void**)&dev, bytes);
    if (e != hipSuccess) return fail(h, DCSCN_ERR_NOMEM, "dcscn_summarize_device: %zu bytes: %s", bytes, hipGetErrorString(e));
    std::vector<char> host(head);
    dcscn_summary* d_rec = reinterpret_cast<dcscn_summary*>(dev);
    int64_t* d_buckets = reinterpret_cast<int64_t*>(dev + sizeof(dcscn_summary));
    e = hipMemsetAsync(dev, 0, head, st);
    if (e == hipSuccess) e = launch_summary(flat_view(data, count), dev + head, d_rec, d_buckets, st);
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), dev, head, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(dev);
    if (e != hipSuccess) return fail(h, DCSCN_ERR_HIP, "dcscn_summarize_device: %s", hipGetErrorString(e));
    memcpy(out, host.data(), sizeof(dcscn_summary));
    if (buckets) memcpy(buckets, host.data() + sizeof(dcscn_summary), sizeof(int64_t) * kSummaryBuckets);
    return DCSCN_OK;
}

}  // extern "C"
