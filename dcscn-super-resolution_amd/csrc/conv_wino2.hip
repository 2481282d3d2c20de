// Winograd F(2x2,3x3) variants (conv_wino2.hpp), one translation unit to parallelise the build.
// Built with -fno-slp-vectorize: hipcc would otherwise pair the input transform's adds into v_pk_add_f32, which costs
// v_mov shuffles and issues worse beside MFMAs (tools/wino2_tune: 36.1 vs 35.6 ms over the 3x3 layers of the bench model).
#include "conv_wino2.hpp"

namespace dcscn {

hipError_t wino_init_kernels() { return WinoVariants::set_attrs(); }

hipError_t wino_launch(int nt, const ConvArgs& a, int n_groups, hipStream_t stream) {
    if (a.n_full < 1 || a.n_full > n_groups || (nt == 1 && a.n_full != n_groups)) return hipErrorInvalidValue;
    return WinoVariants::launch(nt, a, n_groups, stream);
}

}  // namespace dcscn
