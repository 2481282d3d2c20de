// conv5_h and fold_border with ONE product per MAC (conv5_h.hpp: NP = 1; option "fast16"), one translation unit.
#include "conv5_h.hpp"

namespace dcscn {

template <int NT>
static hipError_t c5h1_set_attr() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv5_h<NT, true, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, C5HGeom<NT>::LDS_BYTES);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv5_h<NT, false, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, C5HGeom<NT>::LDS_BYTES);
}

hipError_t c5h1_init_kernels() {
    hipError_t e = c5h1_set_attr<1>();
    if (e == hipSuccess) e = c5h1_set_attr<3>();
    return e != hipSuccess ? e : c5h1_set_attr<4>();
}

template <int NT>
static hipError_t c5h1_launch_one(const ConvArgs& a, hipStream_t stream) {
    const long long tiles = (long long)a.N * a.tiles_y * a.tiles_x;
    if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    if (a.in16.base) {
        if ((long long)a.N * a.H * a.W > kP16MaxPixels) return hipErrorInvalidValue;
        hipLaunchKernelGGL((conv5_h<NT, true, 1>), dim3((unsigned)tiles), dim3(256), C5HGeom<NT>::LDS_BYTES, stream, a);
    } else
        hipLaunchKernelGGL((conv5_h<NT, false, 1>), dim3((unsigned)tiles), dim3(256), C5HGeom<NT>::LDS_BYTES, stream, a);
    return hipGetLastError();
}

// (arguments checked by c5h_launch)
hipError_t c5h1_launch(int nt, const ConvArgs& a, hipStream_t stream) {
    switch (nt) {
        case 1: return c5h1_launch_one<1>(a, stream);
        case 3: return c5h1_launch_one<3>(a, stream);
        case 4: return c5h1_launch_one<4>(a, stream);
        default: return hipErrorInvalidValue;
    }
}

// (arguments checked by c5h_border_launch)
hipError_t c5h1_border_launch(const ConvArgs& a, unsigned grid, hipStream_t stream) {
    if (a.in16.base) {
        if ((long long)a.N * a.H * a.W > kP16MaxPixels) return hipErrorInvalidValue;
        hipLaunchKernelGGL((fold_border<true, 1>), dim3(grid), dim3(256), 4 * kFbWinBytes, stream, a);
    } else
        hipLaunchKernelGGL((fold_border<false, 1>), dim3(grid), dim3(256), 4 * kFbWinBytes, stream, a);
    return hipGetLastError();
}

}  // namespace dcscn
