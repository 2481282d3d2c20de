// conv3_h with ONE product per MAC (conv3_h.hpp: NP = 1; option "fast16"), both input forms, one translation unit to parallelise the build.
#include "conv3_h.hpp"

namespace dcscn {

using List = decltype(C3HVariants<false, 1>{} + C3HVariants<true, 1>{});

hipError_t c3h1_init_kernels() { return List::set_attrs(); }
hipError_t c3h1_launch(int key, const ConvArgs& a, int n_groups, hipStream_t stream) { return List::launch(key, a, n_groups, stream); }

}  // namespace dcscn
