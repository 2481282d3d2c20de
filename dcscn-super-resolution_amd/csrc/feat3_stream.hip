// feat3_stream (feat3_stream.hpp): CNN1 .. CNNL of the non-separable narrow nets as one row-streamed launch.
#include "feat3_stream.hpp"

namespace dcscn {

hipError_t stream3_launch(const Stream3Args& a, int grid, hipStream_t stream, bool fast16) {
    if (fast16) return stream3_fast16_launch(a, grid, stream);
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&feat3_stream<3>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (attr != hipSuccess) return attr;
    if (a.n_waves < 2 || a.n_waves > kS3MaxWaves || a.ring_bytes > 160 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(feat3_stream<3>, dim3(grid), dim3(a.n_waves * 64), (size_t)a.ring_bytes + 256, stream, a);
    return hipGetLastError();
}

}  // namespace dcscn
