// conv_nin_h with ONE product per MAC (conv_nin_h.hpp: NP = 1; option "fast16"): the three source forms on 128-pixel workgroups and the
// 256-pixel workgroup of conv_nin_h_w8.hip, one translation unit.
#include "conv_nin_h.hpp"

namespace dcscn {

using List = decltype(NinHNarrow<1>{} + NinHWide<1>{});

hipError_t nin_h1_init_kernels() { return List::set_attrs(); }
hipError_t nin_h1_launch(int key, const ConvArgs& a, int n_groups, hipStream_t stream) { return List::launch(key, a, n_groups, stream); }

}  // namespace dcscn
