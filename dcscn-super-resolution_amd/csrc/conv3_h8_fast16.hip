// conv3_h8 with ONE product per MAC (conv3_h8.hpp: NP = 1; option "fast16"), float32 and P16 tensors, one translation unit.
#include "conv3_h8.hpp"

namespace dcscn {

template <int NT, int C1, bool P16>
static hipError_t c3e1_set_attr() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3_h8<NT, C1, NT, P16, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, C3EGeom<NT>::LDS_BYTES);
}

template <int NT, int C1>
static hipError_t c3e1_set_attrs() {
    const hipError_t e = c3e1_set_attr<NT, C1, false>();
    return e != hipSuccess ? e : c3e1_set_attr<NT, C1, true>();
}

hipError_t c3e1_init_kernels() {
    hipError_t e = c3e1_set_attrs<6, 6>();
    if (e == hipSuccess) e = c3e1_set_attrs<6, 5>();
    if (e == hipSuccess) e = c3e1_set_attrs<5, 5>();
    if (e == hipSuccess) e = c3e1_set_attrs<5, 4>();
    if (e == hipSuccess) e = c3e1_set_attrs<4, 4>();
    return e != hipSuccess ? e : c3e1_set_attrs<4, 3>();
}

template <int NT, int C1>
static hipError_t c3e1_launch_one(const ConvArgs& a, int wgs, bool p16, hipStream_t stream) {
    if (p16) hipLaunchKernelGGL((conv3_h8<NT, C1, NT, true, 1>), dim3((unsigned)wgs), dim3(512), C3EGeom<NT>::LDS_BYTES, stream, a);
    else hipLaunchKernelGGL((conv3_h8<NT, C1, NT, false, 1>), dim3((unsigned)wgs), dim3(512), C3EGeom<NT>::LDS_BYTES, stream, a);
    return hipGetLastError();
}

// (a: eligible and completed by c3e_launch, which also decides p16: P16 tensors in and out, or float32 in and out)
hipError_t c3e1_launch(int nt, const ConvArgs& a, int wgs, bool p16, hipStream_t stream) {
    if (p16 && (long long)a.N * a.H * a.W > kP16MaxPixels) return hipErrorInvalidValue;
    const bool eq = a.n_full == 2;
    switch (nt) {
        case 6: return eq ? c3e1_launch_one<6, 6>(a, wgs, p16, stream) : c3e1_launch_one<6, 5>(a, wgs, p16, stream);
        case 5: return eq ? c3e1_launch_one<5, 5>(a, wgs, p16, stream) : c3e1_launch_one<5, 4>(a, wgs, p16, stream);
        case 4: return eq ? c3e1_launch_one<4, 4>(a, wgs, p16, stream) : c3e1_launch_one<4, 3>(a, wgs, p16, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace dcscn
