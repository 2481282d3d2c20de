// conv3_h with ONE product per MAC (conv3_h.hpp: NP = 1; option "fast16"), both input forms, one translation unit to parallelise the build.
#include "conv3_h.hpp"

namespace dcscn {

template <int NT, bool IN16>
static hipError_t c3h1_set_attr() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_h<NT, 2, IN16, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, C3HGeom<NT>::LDS_BYTES);
}

template <int NT>
static hipError_t c3h1_set_attrs() {
    const hipError_t e = c3h1_set_attr<NT, false>();
    return e != hipSuccess ? e : c3h1_set_attr<NT, true>();
}

hipError_t c3h1_init_kernels() {
    hipError_t e = c3h1_set_attrs<1>();
    if (e == hipSuccess) e = c3h1_set_attrs<2>();
    if (e == hipSuccess) e = c3h1_set_attrs<3>();
    if (e == hipSuccess) e = c3h1_set_attrs<4>();
    if (e == hipSuccess) e = c3h1_set_attrs<5>();
    return e != hipSuccess ? e : c3h1_set_attrs<6>();
}

// 1-D grid as c3h_launch_one's (conv3_h.hip)
template <int NT>
static hipError_t c3h1_launch_one(ConvArgs a, int n_groups, hipStream_t stream) {
    a.n_groups = n_groups;
    a.group_span = n_groups < 3 ? n_groups : 3;
    const long long tiles = (long long)a.N * a.tiles_y * a.tiles_x;
    const int phases = (n_groups + a.group_span - 1) / a.group_span;
    const long long ids = ((tiles + 7) / 8) * 8 * a.group_span * phases;
    if (ids > 0x7fffffffLL) return hipErrorInvalidValue;
    if (a.in16.base) {
        if ((long long)a.N * a.H * a.W > kP16MaxPixels) return hipErrorInvalidValue;
        hipLaunchKernelGGL((conv3_h<NT, 2, true, 1>), dim3((unsigned)ids), dim3(256), C3HGeom<NT>::LDS_BYTES, stream, a);
    } else
        hipLaunchKernelGGL((conv3_h<NT, 2, false, 1>), dim3((unsigned)ids), dim3(256), C3HGeom<NT>::LDS_BYTES, stream, a);
    return hipGetLastError();
}

// (arguments checked by c3h_launch)
hipError_t c3h1_launch(int nt, const ConvArgs& a, int n_groups, hipStream_t stream) {
    switch (nt) {
        case 1: return c3h1_launch_one<1>(a, n_groups, stream);
        case 2: return c3h1_launch_one<2>(a, n_groups, stream);
        case 3: return c3h1_launch_one<3>(a, n_groups, stream);
        case 4: return c3h1_launch_one<4>(a, n_groups, stream);
        case 5: return c3h1_launch_one<5>(a, n_groups, stream);
        case 6: return c3h1_launch_one<6>(a, n_groups, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace dcscn
