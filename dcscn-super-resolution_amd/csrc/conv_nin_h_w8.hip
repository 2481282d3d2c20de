// conv_nin_h with 256 pixels per workgroup (conv_nin_h.hpp: NinHWide), for the wide K axes.  Its own translation unit, for build
// parallelism and the no-spill gate.
#include "conv_nin_h.hpp"

namespace dcscn {

using List = NinHWide<3>;

hipError_t nin_h8_init_kernels() { return List::set_attrs(); }
hipError_t nin_h8_launch(int key, const ConvArgs& a, int n_groups, hipStream_t stream) { return List::launch(key, a, n_groups, stream); }

}  // namespace dcscn
