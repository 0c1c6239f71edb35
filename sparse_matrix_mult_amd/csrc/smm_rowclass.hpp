// smm_rowclass.hpp -- pieces shared by the row-class kernels of the sparse triple product (smm_triple_sparse.hpp), the
// masked SpGEMM (smm_masked.hpp) and sparse x dense (smm_spmm.hpp): the class-list append of their bin kernels, the
// shapes of the two LDS hash classes and the open-addressing hash itself.  Host driver: smm_api.hip.
#pragma once
#include "smm_kernels.hpp"

namespace smm {

// Appends `row` to lists[cls * m ..] and counts it in counts[cls] for the lanes with cls in [0, ncls) (others: no
// class); one atomic per wave and class.  All lanes of the wave call it.
__device__ __forceinline__ void class_list_append(int cls, int ncls, int64_t m, int row, int *lists, int *counts)
{
    for (int c = 0; c < ncls; ++c) {
        const unsigned long long mask = __ballot(cls == c);
        if (!mask) continue;
        const int leader = __ffsll((long long)mask) - 1;
        int base = 0;
        if (lane_id() == leader) base = atomicAdd(&counts[c], __popcll(mask));
        base = __shfl(base, leader);
        if (cls == c) lists[(int64_t)c * m + base + mbcnt(mask)] = row;
    }
}

// An LDS hash class: HS = 2^BITS slots per row, TPR threads per row, RPB rows per workgroup of 256 threads.  A row of
// the class holds at most MAX = HS / 2 keys (longer rows go to the next class).
template <int HS_, int BITS_, int TPR_, int RPB_> struct HashClass {
    static_assert((1 << BITS_) == HS_ && TPR_ * RPB_ == 256, "hash class");
    static constexpr int HS = HS_, BITS = BITS_, TPR = TPR_, RPB = RPB_, MAX = HS_ / 2;
};
using WaveHash = HashClass<512, 9, 64, 4>;        // one wave per row, four rows per workgroup
using WgHash = HashClass<8192, 13, 256, 1>;       // one workgroup per row

// Open-addressing hash of int keys in LDS: HS = 2^BITS slots of `key` (-1: empty), multiplicative hashing, linear
// probing over at most HS slots.  Callers keep their values in arrays of their own, indexed by slot.
template <int HS, int BITS> struct LdsHash {
    static_assert((1 << BITS) == HS, "hash size");
    int *key;
    __device__ __forceinline__ static unsigned start(int k) { return ((unsigned)k * 2654435761u) >> (32 - BITS); }
    // Slots t, t + nt, ... emptied; slot(s) clears the caller's arrays alongside.
    template <typename Slot> __device__ __forceinline__ void clear(int t, int nt, Slot slot) const
    {
        for (int s = t; s < HS; s += nt) { key[s] = -1; slot(s); }
    }
    __device__ __forceinline__ void clear(int t, int nt) const { clear(t, nt, [](int) {}); }
    // Slot of k, claimed when absent (lanes inserting one key meet in one slot); -1 when the table is full.
    __device__ __forceinline__ int insert(int k) const
    {
        unsigned s = start(k);
        for (int probe = 0; probe < HS; ++probe, s = (s + 1) & (HS - 1)) {
            const int prev = atomicCAS(&key[s], -1, k);
            if (prev == -1 || prev == k) return (int)s;
        }
        return -1;
    }
    // at(slot of k), or `absent` when k is not in the table.  (A value read at the hit inside the probe loop costs
    // the hash kernels some 25 SGPRs less than one read through the returned slot.)
    template <typename T, typename At> __device__ __forceinline__ T find(int k, T absent, At at) const
    {
        unsigned s = start(k);
        for (int probe = 0; probe < HS; ++probe, s = (s + 1) & (HS - 1)) {
            const int kk = key[s];
            if (kk == k) return at((int)s);
            if (kk == -1) break;
        }
        return absent;
    }
    // Slot of k, -1 when absent.
    __device__ __forceinline__ int find(int k) const { return find(k, -1, [](int s) { return s; }); }
};

}  // namespace smm
