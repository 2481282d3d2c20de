// conv_nin_h variants (conv_nin_h.hpp), one translation unit to parallelise the build.
#include "conv_nin_h.hpp"

namespace dcscn {

using List = NinHNarrow<3>;

hipError_t nin_h_init_kernels() {
    hipError_t e = nin_h8_init_kernels();
    if (e == hipSuccess) e = nin_h1_init_kernels();
    return e != hipSuccess ? e : List::set_attrs();
}

hipError_t nin_h_launch(int nt, const ConvArgs& a, int n_groups, bool w8, hipStream_t stream, bool fast16) {
    if (a.n_full < 1 || a.n_full > n_groups || (nt == 1 && a.n_full != n_groups) || !a.wpack16) return hipErrorInvalidValue;
    const bool wide = w8 && nt == 6 && a.in16.base && a.n_chunks >= kNinH8MinChunks && a.n_full == n_groups;
    const int key = nin_h_key(nt, a.in16.base ? 2 : a.srctab ? 1 : 0, wide);
    if (fast16) return nin_h1_launch(key, a, n_groups, stream);
    if (wide) return nin_h8_launch(key, a, n_groups, stream);
    return List::launch(key, a, n_groups, stream);
}

}  // namespace dcscn
