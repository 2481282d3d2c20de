// conv3_h8 with ONE product per MAC (conv3_h8.hpp: NP = 1; option "fast16"), float32 and P16 tensors, one translation unit.
#include "conv3_h8.hpp"

namespace dcscn {

using List = decltype(C3EVariants<false, 1>{} + C3EVariants<true, 1>{});

hipError_t c3e1_init_kernels() { return List::set_attrs(); }
hipError_t c3e1_launch(int key, const ConvArgs& a, int wgs, hipStream_t stream) { return List::launch(key, a, wgs, stream); }

}  // namespace dcscn
