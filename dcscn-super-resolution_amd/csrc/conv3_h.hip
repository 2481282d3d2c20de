// conv3_h variants (conv3_h.hpp), one translation unit to parallelise the build.
#include "conv3_h.hpp"

namespace dcscn {

using List = C3HVariants<false, 3>;

hipError_t c3h_init_kernels() {
    hipError_t e = c3h16_init_kernels();
    if (e == hipSuccess) e = c3h1_init_kernels();
    return e != hipSuccess ? e : List::set_attrs();
}

hipError_t c3h_launch(int nt, const ConvArgs& a, int n_groups, hipStream_t stream, bool fast16) {
    if (a.n_full < 1 || a.n_full > n_groups || (nt == 1 && a.n_full != n_groups) || !a.wpack16 || a.tiles_x != (a.W + 15) / 16 ||
        a.tiles_y != (a.H + 15) / 16 || a.n_chunks < 1)
        return hipErrorInvalidValue;
    const int key = c3h_key(nt, a.in16.base != nullptr);
    if (fast16) return c3h1_launch(key, a, n_groups, stream);
    if (a.in16.base) return c3h16_launch(key, a, n_groups, stream);
    return List::launch(key, a, n_groups, stream);
}

}  // namespace dcscn
