// conv5_h variants (conv5_h.hpp): the folded tail of x2 / x3 / x4 models.
#include "conv5_h.hpp"

namespace dcscn {

using List = C5HVariants<3>;
using BorderList = FoldBorderVariants<3>;

hipError_t c5h_init_kernels() {
    hipError_t e = c5h1_init_kernels();
    if (e == hipSuccess) e = List::set_attrs();
    return e != hipSuccess ? e : BorderList::set_attrs();
}

hipError_t c5h_launch(int nt, const ConvArgs& a, hipStream_t stream, bool fast16) {
    if (!a.fold || (a.fold == 2 && nt != 1) || !a.wpack16 || a.tiles_x != (a.W + 15) / 16 || a.tiles_y != (a.H + 15) / 16 || a.n_chunks < 1) return hipErrorInvalidValue;
    const int key = c5h_key(nt, a.in16.base != nullptr);
    return fast16 ? c5h1_launch(key, a, stream) : List::launch(key, a, stream);
}

hipError_t c5h_border_launch(const ConvArgs& a, hipStream_t stream, bool fast16) {
    if (a.fold != 2 || !a.wpack16 || !a.bias || a.n_chunks < 1 || a.ps < 2 || a.ps * a.ps > 16 || a.N < 1) return hipErrorInvalidValue;
    const int key = a.in16.base != nullptr;
    return fast16 ? c5h1_border_launch(key, a, stream) : BorderList::launch(key, a, stream);
}

}  // namespace dcscn
