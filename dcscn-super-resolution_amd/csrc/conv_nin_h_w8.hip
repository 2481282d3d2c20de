// conv_nin_h with 8 waves x two 16-pixel tiles = 256 pixels per workgroup, ONE workgroup per CU: half the filter traffic per pixel.
// Same products in the same order per pixel: bit-identical to the 128-pixel workgroups.  Its own translation unit, for build
// parallelism and the no-spill gate.
// Measured same-box in r05 (profiles/r05_ninh_ablation.txt): -3 % on the 1301-channel GEMM of the L12 nets, +7 ... +9 % on 540 / 131 channels --
// so only the wide K axes take it (conv_nin_h.hip: nin_h_launch), P16 sources, six output tiles.
#include "conv_nin_h.hpp"

namespace dcscn {

constexpr int kNinH8Stages = 3;
constexpr int kNinH8MaxTable = 16 * 1024;
constexpr int kNinH8Waves = 8, kNinH8Tiles = 2;

hipError_t nin_h8_init_kernels() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_nin_h<6, 2, kNinH8Stages, 2, kNinH8Waves, kNinH8Tiles>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, NinHGeom<6, kNinH8Stages, kNinH8Waves, kNinH8Tiles>::LDS_BYTES + kNinH8MaxTable);
}

hipError_t nin_h8_launch(const ConvArgs& a, int n_groups, hipStream_t stream) {
    using G = NinHGeom<6, kNinH8Stages, kNinH8Waves, kNinH8Tiles>;
    const long long npix = (long long)a.N * a.H * a.W;
    const size_t table = (size_t)a.n_chunks * 64;
    if (!a.in16.base || !a.srctab || table > (size_t)kNinH8MaxTable || npix > kP16MaxPixels) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((npix + G::PIX - 1) / G::PIX), (unsigned)n_groups);
    hipLaunchKernelGGL((conv_nin_h<6, 2, kNinH8Stages, 2, kNinH8Waves, kNinH8Tiles>), grid, dim3(G::THREADS), G::LDS_BYTES + table, stream, a);
    return hipGetLastError();
}

}  // namespace dcscn
