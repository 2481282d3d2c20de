// feat_stream / tail_stream with ONE product per MAC (feat_stream.hpp: NP = 1; option "fast16_separable"), one translation unit to
// parallelise the build and to keep the three-product kernels' code apart from it.
#include "tail_stream.hpp"

namespace dcscn {

void stream_fast16_init_kernels() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&feat_stream<true, false, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tail_stream<true, false, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

hipError_t tail_fast16_launch(const TailArgs& a, int grid, hipStream_t stream) {
    const size_t lds = (size_t)a.ring_bytes + a.ldsw_bytes;
    hipLaunchKernelGGL((tail_stream<true, false, 1>), dim3(grid), dim3(640), lds, stream, a);
    return hipGetLastError();
}

hipError_t stream_fast16_launch(const StreamArgs& a, int grid, hipStream_t stream) {
    const int threads = (1 + a.n_conv + a.L) * 64;
    const size_t lds = (size_t)a.ring_bytes + a.ldsw_bytes;
    hipLaunchKernelGGL((feat_stream<true, false, 1>), dim3(grid), dim3(threads), lds, stream, a);
    return hipGetLastError();
}

}  // namespace dcscn
