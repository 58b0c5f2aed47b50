// atc_kernarg.h — where a kernel's by-value arguments lie in its kernarg segment, computed from the kernel's own parameter list.
//   The kernarg segment holds the parameters in order, each at its natural alignment (the explicit arguments come first: offset 0 is
//   the first parameter's).  KernArgs<decltype(kernel<...>)> lays the list out by that rule at compile time, so a kernel that re-reads
//   an argument by its byte offset (kernarg_reread, atc_step.hip) and a static_assert that holds one list to another both read the
//   offsets from the one description there is: the parameter list.  decltype of a kernel is an unevaluated operand — no address of a
//   __global__ function is taken — and top-level qualifiers of a parameter (__restrict__, const) are not part of the function type.
#pragma once
#include <stddef.h>
#include <type_traits>

template <typename F>
struct KernArgs;
template <typename... A>
struct KernArgs<void(A...)> {
    static constexpr size_t count = sizeof...(A);
    // offset of parameter I
    template <size_t I>
    static constexpr size_t at() {
        static_assert(I < count, "the kernel has no parameter of that index");
        return offset(I);
    }
    // offset of the first parameter of type T
    template <typename T>
    static constexpr size_t of() {
        static_assert((std::is_same<T, A>::value || ...), "the kernel has no parameter of that type");
        const bool is[] = {std::is_same<T, A>::value...};
        size_t i = 0;
        while (!is[i]) ++i;
        return offset(i);
    }
    // offset of the last parameter
    static constexpr size_t last() { return at<count - 1>(); }

private:
    static constexpr size_t offset(size_t i) {
        const size_t size[] = {sizeof(A)...}, align[] = {alignof(A)...};
        size_t off = 0;
        for (size_t k = 0;; ++k) {
            off = (off + align[k] - 1) / align[k] * align[k];
            if (k == i) return off;
            off += size[k];
        }
    }
};
