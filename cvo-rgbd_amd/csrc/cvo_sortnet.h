// cvo_sortnet.h -- sorting N 32-bit keys in registers by a fixed network, and the lower median of the valid ones among
// them: what the median stage (cvo_median.hip) and the input bin (cvo_bin.hip) share.  Every index is a compile-time
// constant: nothing is indexed by a runtime value and nothing goes to scratch.
// The sort key is value - 1 in 32 bits: a cell without a value (0) becomes 0xFFFFFFFF and sorts behind every depth,
// 65535 (key 65534) included; no 16-bit sentinel.  The network is Batcher's odd-even merge sort for any N, made at
// compile time; the comparators that only order the upper half never reach an output and the compiler drops them.
#ifndef CVO_SORTNET_H
#define CVO_SORTNET_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

namespace {

// Batcher's odd-even merge sort on N keys, N any number: the comparators (a < b: the smaller key goes to a) in order
template <int N> struct MdNet {
    int a[N * N], b[N * N];
    int n;
};

template <int N> constexpr MdNet<N> md_make_net()
{
    MdNet<N> t{};
    for (int p = 1; p < N; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j <= N - 1 - k; j += 2 * k)
                for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        t.a[t.n] = i + j;
                        t.b[t.n] = i + j + k;
                        ++t.n;
                    }
    return t;
}

template <int N> struct MdNetOf {
    static constexpr MdNet<N> net = md_make_net<N>();
};

template <int N, int I> __host__ __device__ __forceinline__ void md_exchange(uint32_t (&v)[N])
{
    constexpr int ia = MdNetOf<N>::net.a[I], ib = MdNetOf<N>::net.b[I];
    static_assert(ia >= 0 && ia < ib && ib < N, "a comparator of the network");
    const uint32_t lo = v[ia] < v[ib] ? v[ia] : v[ib], hi = v[ia] < v[ib] ? v[ib] : v[ia];
    v[ia] = lo;
    v[ib] = hi;
}

template <int N, int... I> __host__ __device__ __forceinline__ void md_sort_seq(uint32_t (&v)[N], std::integer_sequence<int, I...>)
{
    (md_exchange<N, I>(v), ...);
}

template <int N> __host__ __device__ __forceinline__ void md_sort(uint32_t (&v)[N])
{
    md_sort_seq<N>(v, std::make_integer_sequence<int, MdNetOf<N>::net.n>{});
}

// the lower median of the valid cells among N (0 = none), and 0 where there is none; *count = n
template <int N> __host__ __device__ __forceinline__ uint32_t md_lower_median(const uint32_t (&cells)[N], int *count)
{
    uint32_t key[N];
    int n = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        key[i] = cells[i] - 1u;   // (none: 0xFFFFFFFF, behind every depth)
        n += cells[i] != 0u ? 1 : 0;
    }
    md_sort<N>(key);
    const int pick = (n - 1) >> 1;   // (n == 0: -1, and the chain below keeps key[0], which is "none" then)
    uint32_t m = key[0];
#pragma unroll
    for (int j = 1; j <= (N - 1) / 2; ++j) m = pick == j ? key[j] : m;
    *count = n;
    return m + 1u;
}

}   // namespace

#endif
