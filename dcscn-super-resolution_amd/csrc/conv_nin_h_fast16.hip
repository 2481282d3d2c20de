// conv_nin_h with ONE product per MAC (conv_nin_h.hpp: NP = 1; option "fast16"): the three source forms on 128-pixel workgroups and the
// 256-pixel workgroup of conv_nin_h_w8.hip, one translation unit.
#include "conv_nin_h.hpp"

namespace dcscn {

constexpr int kNinH1Stages = 3;                  // as conv_nin_h.hip / conv_nin_h_w8.hip
constexpr int kNinH1MaxTable = 16 * 1024;
constexpr int kNinH1W8Waves = 8, kNinH1W8Tiles = 2;

template <int NT>
static hipError_t nin_h1_set_attr() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_nin_h<NT, 0, kNinH1Stages, 2, 4, 2, 1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       NinHGeom<NT, kNinH1Stages>::LDS_BYTES);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_nin_h<NT, 2, kNinH1Stages, 2, 4, 2, 1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            NinHGeom<NT, kNinH1Stages>::LDS_BYTES + kNinH1MaxTable);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_nin_h<NT, 1, kNinH1Stages, 2, 4, 2, 1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               NinHGeom<NT, kNinH1Stages>::LDS_BYTES + kNinH1MaxTable);
}

hipError_t nin_h1_init_kernels() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_nin_h<6, 2, kNinH1Stages, 2, kNinH1W8Waves, kNinH1W8Tiles, 1>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, NinHGeom<6, kNinH1Stages, kNinH1W8Waves, kNinH1W8Tiles>::LDS_BYTES + kNinH1MaxTable);
    if (e == hipSuccess) e = nin_h1_set_attr<1>();
    if (e == hipSuccess) e = nin_h1_set_attr<2>();
    if (e == hipSuccess) e = nin_h1_set_attr<3>();
    if (e == hipSuccess) e = nin_h1_set_attr<4>();
    if (e == hipSuccess) e = nin_h1_set_attr<5>();
    return e != hipSuccess ? e : nin_h1_set_attr<6>();
}

template <int NT>
static hipError_t nin_h1_launch_one(const ConvArgs& a, int n_groups, hipStream_t stream) {
    using G = NinHGeom<NT, kNinH1Stages>;
    const long long npix = (long long)a.N * a.H * a.W;
    const dim3 grid((unsigned)((npix + G::PIX - 1) / G::PIX), (unsigned)n_groups);
    if (a.in16.base) {                                           // P16 sources: a.srctab holds one entry per channel OCTET (4 per chunk)
        const size_t table = (size_t)a.n_chunks * 64;
        if (!a.srctab || table > (size_t)kNinH1MaxTable || npix > kP16MaxPixels) return hipErrorInvalidValue;
        hipLaunchKernelGGL((conv_nin_h<NT, 2, kNinH1Stages, 2, 4, 2, 1>), grid, dim3(G::THREADS), G::LDS_BYTES + table, stream, a);
    } else if (a.srctab) {
        const size_t table = (size_t)a.n_chunks * 128;           // 8 quads of 16 bytes per 32-channel chunk
        if (table > (size_t)kNinH1MaxTable) return hipErrorInvalidValue;
        hipLaunchKernelGGL((conv_nin_h<NT, 1, kNinH1Stages, 2, 4, 2, 1>), grid, dim3(G::THREADS), G::LDS_BYTES + table, stream, a);
    } else {
        hipLaunchKernelGGL((conv_nin_h<NT, 0, kNinH1Stages, 2, 4, 2, 1>), grid, dim3(G::THREADS), G::LDS_BYTES, stream, a);
    }
    return hipGetLastError();
}

static hipError_t nin_h1_launch_w8(const ConvArgs& a, int n_groups, hipStream_t stream) {
    using G = NinHGeom<6, kNinH1Stages, kNinH1W8Waves, kNinH1W8Tiles>;
    const long long npix = (long long)a.N * a.H * a.W;
    const size_t table = (size_t)a.n_chunks * 64;
    if (!a.in16.base || !a.srctab || table > (size_t)kNinH1MaxTable || npix > kP16MaxPixels) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((npix + G::PIX - 1) / G::PIX), (unsigned)n_groups);
    hipLaunchKernelGGL((conv_nin_h<6, 2, kNinH1Stages, 2, kNinH1W8Waves, kNinH1W8Tiles, 1>), grid, dim3(G::THREADS), G::LDS_BYTES + table, stream, a);
    return hipGetLastError();
}

// (arguments checked by nin_h_launch, which also decides w8: the 256-pixel workgroups)
hipError_t nin_h1_launch(int nt, const ConvArgs& a, int n_groups, bool w8, hipStream_t stream) {
    if (w8) return nin_h1_launch_w8(a, n_groups, stream);
    switch (nt) {
        case 1: return nin_h1_launch_one<1>(a, n_groups, stream);
        case 2: return nin_h1_launch_one<2>(a, n_groups, stream);
        case 3: return nin_h1_launch_one<3>(a, n_groups, stream);
        case 4: return nin_h1_launch_one<4>(a, n_groups, stream);
        case 5: return nin_h1_launch_one<5>(a, n_groups, stream);
        case 6: return nin_h1_launch_one<6>(a, n_groups, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace dcscn
