// Reading an id stream that is aligned to its element size only (idstats.hip, batch.hip): the
// stream is read as 16-byte vectors on the 16-byte grid of the address space; a vector that lies
// partly outside [0, n) is loaded element by element, every other one with one 16-byte load.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace bpe {

// The values of vector j of the 16-byte grid (sh: elements of vector 0 that lie before ids[0]);
// returns the mask of the slots inside [0, n).
template <class E>
__device__ __forceinline__ unsigned load_ids(const E* __restrict__ ids, size_t n, unsigned sh, size_t j,
                                             E (&v)[16 / sizeof(E)]) {
    constexpr unsigned V = 16 / sizeof(E);
    const long long e0 = (long long)(j * V) - (long long)sh;   // element index of slot 0
    if (e0 >= 0 && (size_t)e0 + V <= n) {
        union { uint4 w; E e[V]; } u;
        u.w = *reinterpret_cast<const uint4*>(ids + e0);
#pragma unroll
        for (unsigned k = 0; k < V; ++k) v[k] = u.e[k];
        return (1u << V) - 1u;
    }
    unsigned m = 0;
#pragma unroll
    for (unsigned k = 0; k < V; ++k) {
        const long long e = e0 + (long long)k;
        const bool in = e >= 0 && (size_t)e < n;
        v[k] = in ? ids[e] : E(0);
        m |= in ? (1u << k) : 0u;
    }
    return m;
}

}  // namespace bpe
