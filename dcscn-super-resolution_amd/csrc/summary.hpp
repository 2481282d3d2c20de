// TensorBoard summary records reduced on the device (summary.hip; include/dcscn.h: "TensorBoard summaries").
#pragma once
#include "plan.h"

namespace dcscn_impl {

constexpr int kSummaryBuckets = DCSCN_SUMMARY_BUCKETS;
constexpr int kSummaryMaxBlocks = 256;        // chunks a tensor is cut into at the most
constexpr int64_t kSummaryBlockValues = 4096; // ... and the values a chunk holds at the least (but for the last)

// `count` values in rows of C at a distance of `stride` floats: value i is p[(i / C) * stride + i % C].  C == stride: a flat buffer.
// A layer's slice of a concat tensor is such a view.
struct SummaryView {
    const float* p;
    int64_t count;
    int C, stride;
};
inline SummaryView flat_view(const float* p, int64_t count) { return SummaryView{p, count, 1, 1}; }

// The bucket limits, built once on the host (kSummaryBuckets doubles).
const double* summary_limits();
// Uploads the limits to the current device's copy of the table the kernels search, once per device.
hipError_t summary_prepare_device(int device);
// Bytes of scratch one reduction needs (the chunks' partial results); reductions on one stream may share it.
size_t summary_scratch_bytes();
// Enqueues the reduction of `v` into *rec and buckets[kSummaryBuckets], both device memory and ZEROED by the caller beforehand.
hipError_t launch_summary(const SummaryView& v, void* scratch, dcscn_summary* rec, int64_t* buckets, hipStream_t st);

}  // namespace dcscn_impl
