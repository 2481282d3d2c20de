// conv5_h and fold_border with ONE product per MAC (conv5_h.hpp: NP = 1; option "fast16"), one translation unit.
#include "conv5_h.hpp"

namespace dcscn {

using List = C5HVariants<1>;
using BorderList = FoldBorderVariants<1>;

hipError_t c5h1_init_kernels() {
    const hipError_t e = List::set_attrs();
    return e != hipSuccess ? e : BorderList::set_attrs();
}
hipError_t c5h1_launch(int key, const ConvArgs& a, hipStream_t stream) { return List::launch(key, a, stream); }
hipError_t c5h1_border_launch(int key, const ConvArgs& a, hipStream_t stream) { return BorderList::launch(key, a, stream); }

}  // namespace dcscn
