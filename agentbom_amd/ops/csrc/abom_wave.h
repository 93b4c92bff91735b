// Wave- and block-level device helpers shared by the graph kernels (gfx950).
// wave64 only.  A helper that shuffles or ballots must be reached by all
// lanes of the wave; lanes without work pass 0 / false.
#pragma once

#include "abom_common.h"

namespace abom {

// Where a thread sits in a one-wave-per-item kernel: the wave takes items
// wave, wave + n_waves, ...  `waves_per_block` is blockDim.x >> 6, read by
// the kernel, or the constant the kernel is always launched with (blockDim.x
// read in a helper misses the compiler's uniform-block-size folding).
struct WaveId {
    int lane;           // lane of the wave
    int wid;            // wave of the block
    long long wave;     // wave of the grid
    long long n_waves;  // waves in the grid
};

__device__ __forceinline__ WaveId wave_id(unsigned waves_per_block) {
    WaveId w;
    w.lane = threadIdx.x & 63;
    w.wid = threadIdx.x >> 6;
    w.wave = (long long)blockIdx.x * waves_per_block + w.wid;
    w.n_waves = (long long)gridDim.x * waves_per_block;
    return w;
}

// Fixed-tree wave sum, total in lane 0.  T: int, unsigned, long long, double;
// the order off = 32, 16, ... 1 is what keeps the fp64 results bit-identical.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// One atomic per wave: lanes accumulate locally, reduce, lane 0 adds.
__device__ __forceinline__ void wave_add(unsigned int* dst, unsigned v) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

// Exclusive prefix sum of v over the lanes; *total = the sum, in every lane.
__device__ __forceinline__ int wave_exclusive_scan(int v, int lane, int* total) {
    int incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    *total = __shfl(incl, 63, 64);
    return incl - v;
}

// Append `value` of every lane with `want` to the queue: one atomic per wave
// reserves the slots, a lane's slot is its rank among the wanting lanes.  The
// caller sizes the queue; no bound is checked here.
__device__ __forceinline__ void wave_queue_push(bool want, uint32_t value,
                                                uint32_t* __restrict__ queue,
                                                unsigned int* __restrict__ count, int lane) {
    const unsigned long long mask = __ballot(want);
    if (mask) {
        const int leader = __ffsll((long long)mask) - 1;
        unsigned int base = 0;
        if (lane == leader) base = atomicAdd(count, (unsigned int)__popcll(mask));
        base = __shfl(base, leader, 64);
        if (want) queue[base + __popcll(mask & ((1ull << lane) - 1))] = value;
    }
}

// *counter += number of lanes with `flag`: one atomic per wave.
__device__ __forceinline__ void wave_count_flag(bool flag, unsigned int* __restrict__ counter,
                                                int lane) {
    const unsigned long long mask = __ballot(flag);
    if (mask && lane == __ffsll((long long)mask) - 1)
        atomicAdd(counter, (unsigned int)__popcll(mask));
}

// Per-block LDS stage in front of a global queue: the block reserves its
// slots with ONE atomic per flush.  `n` counts the pushes since the last flush
// and may pass N: the pushes past it went straight to the global queue.  The
// caller sets n = 0 and passes a barrier before the first push of a round.
template <unsigned N>
struct BlockStage {
    uint32_t e[N];
    unsigned n;
    unsigned base;  // the block's first slot of the global queue, set by the flush
};

// Any lane.  The slot comes from an LDS atomic; only a push that finds the
// stage full pays the global one.  Past `capacity`: counted, not stored.
template <unsigned N>
__device__ __forceinline__ void stage_push(uint32_t entry, BlockStage<N>& st,
                                           uint32_t* __restrict__ queue,
                                           unsigned int* __restrict__ count,
                                           long long capacity) {
    const unsigned slot = atomicAdd(&st.n, 1u);
    if (slot < N) {
        st.e[slot] = entry;
    } else {
        const unsigned idx = atomicAdd(count, 1u);
        if ((long long)idx < capacity) queue[idx] = entry;
    }
}

// Whole block, block-uniform call (two barriers inside): one global atomic
// for the staged entries, then a coalesced copy.
template <unsigned N>
__device__ __forceinline__ void stage_flush(BlockStage<N>& st, uint32_t* __restrict__ queue,
                                            unsigned int* __restrict__ count,
                                            long long capacity) {
    __syncthreads();
    const unsigned n = st.n < N ? st.n : N;
    if (threadIdx.x == 0 && n) st.base = atomicAdd(count, n);
    __syncthreads();
    if (n) {
        const unsigned base = st.base;
        for (unsigned k = threadIdx.x; k < n; k += blockDim.x) {
            const unsigned idx = base + k;
            if ((long long)idx < capacity) queue[idx] = st.e[k];
        }
    }
}

// Segments laid end to end, pref = exclusive prefix of their lengths: entry i
// is element i - pref[s] of segment s, the last one with pref[s] <= i.
__device__ __forceinline__ int segment_of(const int* pref, int n_items, int i) {
    int lo = 0, hi = n_items;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pref[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace abom
