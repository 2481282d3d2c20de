// conv3_h variants that read a P16 tensor (conv3_h.hpp: IN16; p16.hpp), one translation unit to parallelise the build.
#include "conv3_h.hpp"

namespace dcscn {

using List = C3HVariants<true, 3>;

hipError_t c3h16_init_kernels() { return List::set_attrs(); }
hipError_t c3h16_launch(int key, const ConvArgs& a, int n_groups, hipStream_t stream) { return List::launch(key, a, n_groups, stream); }

}  // namespace dcscn
