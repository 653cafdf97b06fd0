// Host-side dispatch on the storage type of an activation tensor.
//
// The ReID kernels are templates over T = _Float16 or float, and every extern "C" launcher takes
// `int half`.  by_storage(half, f) calls the generic lambda f once, with a tag whose ::type is the
// storage type, so a launcher names its kernel and its argument list once:
//
//     by_storage(half, [&](auto tag) {
//         using T = typename decltype(tag)::type;
//         hipLaunchKernelGGL(k<T>, grid, block, lds, st, (const T *)x, ..., (T *)y);
//     });
//
// Both instantiations are compiled, as with the if / else it replaces; f's result is returned
// (both instantiations must agree on its type; void is fine).
#pragma once

namespace yta {

template <typename T>
struct storage_tag {
    using type = T;
};

template <typename F>
inline auto by_storage(int half, F &&f) {
    if (half) return f(storage_tag<_Float16>{});
    return f(storage_tag<float>{});
}

}  // namespace yta
