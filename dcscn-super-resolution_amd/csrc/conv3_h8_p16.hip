// conv3_h8 variants with P16 tensors in and out (conv3_h8.hpp: P16; p16.hpp), one translation unit to parallelise the build.
#include "conv3_h8.hpp"

namespace dcscn {

using List = C3EVariants<true, 3>;

hipError_t c3e16_init_kernels() { return List::set_attrs(); }
hipError_t c3e16_launch(int key, const ConvArgs& a, int wgs, hipStream_t stream) { return List::launch(key, a, wgs, stream); }

}  // namespace dcscn
