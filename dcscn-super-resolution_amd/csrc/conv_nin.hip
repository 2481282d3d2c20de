// conv_nin variants (conv_nin.hpp), one translation unit to parallelise the build.
#include "conv_nin.hpp"

namespace dcscn {

using List = decltype(NinVariants<false>{} + NinVariants<true>{});

hipError_t nin_init_kernels() { return List::set_attrs(); }

hipError_t nin_launch(int nt, const ConvArgs& a, int n_groups, hipStream_t stream) {
    if (a.n_full < 1 || a.n_full > n_groups || (nt == 1 && a.n_full != n_groups)) return hipErrorInvalidValue;
    return List::launch(nin_key(nt, a.srctab != nullptr), a, n_groups, stream);
}

}  // namespace dcscn
