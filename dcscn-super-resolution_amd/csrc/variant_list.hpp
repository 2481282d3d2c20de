// The variants of a kernel family as ONE type list per translation unit: the list raises the dynamic-LDS limit of every variant (init) and
// launches the one whose KEY equals a runtime key (dispatch), so nothing can be launched that init did not cover.  A variant is a
// host-only struct next to its kernel (conv3_h.hpp: C3HVariant, ...), modelled on Variant<> of conv_variants.hpp:
//     static constexpr int KEY;   static hipError_t set_attr();   static hipError_t launch(args...);
#pragma once
#include <hip/hip_runtime.h>

namespace dcscn {

template <class K>
hipError_t allow_lds(K kernel, int bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

template <class... V>
struct Variants {
    static hipError_t set_attrs() {                              // stops at the first error
        hipError_t e = hipSuccess;
        (void)(((e = V::set_attr()) == hipSuccess) && ...);
        return e;
    }
    template <class... A>
    static hipError_t launch(int key, const A&... args) {        // hipErrorInvalidValue: no such variant in this list
        hipError_t e = hipErrorInvalidValue;
        (void)((V::KEY == key && ((e = V::launch(args...)), true)) || ...);
        return e;
    }
};
template <class... A, class... B>
constexpr Variants<A..., B...> operator+(Variants<A...>, Variants<B...>) { return {}; }     // decltype(X{} + Y{}): both lists as one

}  // namespace dcscn
