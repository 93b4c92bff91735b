// Distinct unions over the installs of an item (a remediation item, an
// advisory): the servers that hold an install and, through the per-server
// reach index, what those servers reach.  Both tiers, their launch and the
// slot / cursor words of an item's `state` row live here; remediation.hip and
// toxic.hip bring their caps as a traits struct and the kernels around them.
//
// Tier 1 (union_wave_kernel), one wave per matched item: distinct servers,
//   then agents (PLANES == 1) or agents, creds and tools (PLANES == 3) as
//   capped LDS sets (abom_sets.h).  An item past a cap, or with more than
//   T1_INSTALLS installs, goes to the tier-2 queue.
// Tier 2 (union_block_kernel), one block per slice of the bitmap pool: a
//   slice holds one bit per reach-index row and PLANES planes of one bit per
//   node id below `node_span`; atomicOr sets a bit and the old word says
//   whether it was new.  A block walks its item twice, the second time
//   clearing what the first set, so a slice is all-zero whenever a block
//   leaves an item, and block b takes the queued items b, b + slices, ...
#pragma once

#include "abom_sets.h"

namespace abom {

constexpr int UNION_WAVES = 4;      // waves per block of both tiers
constexpr int UNION_T2_LIST = 1024; // servers a tier-2 block lists per chunk

// `state` holds one row of UNION_ROW u32 words per item; the first six are
// the user's, the last two carry a matched item from its gather to its union
constexpr int UNION_ROW = 8;
constexpr int UW_SLOT = 6;    // 1 + the item's position among the matched ones
constexpr int UW_CURSOR = 7;  // installs claimed so far in the item's csr span
// words of `counters` the tiers write; the others are the user's
constexpr int UC_QUEUED = 1;  // items tier 1 left to tier 2
constexpr int UC_ROUNDS = 2;  // queued items per pool slice, rounded up

// gather: the row's item is the m-th matched one
__device__ __forceinline__ void slot_set(uint32_t* row, long long m) {
    row[UW_SLOT] = (uint32_t)m + 1;
}

// m = the position of the row's item among the M matched ones, if it has one
__device__ __forceinline__ bool slot_get(const uint32_t* row, long long M, long long& m) {
    m = (long long)row[UW_SLOT] - 1;
    return m >= 0 && m < M;
}

// scatter: `value` goes to the next place in the span of the row's item,
// off[m] onwards, of a csr of n entries.  Nowhere without a slot or past the
// end; neither is reached with the gather's slots and offsets.
__device__ __forceinline__ void slot_claim(uint32_t* row, const int* __restrict__ off,
                                           long long M, long long n, int* __restrict__ csr,
                                           int value) {
    long long m;
    if (!slot_get(row, M, m)) return;
    const long long at = (long long)off[m] + atomicAdd(&row[UW_CURSOR], 1u);
    if (at < n) csr[at] = value;
}

__device__ __forceinline__ void slot_clear(uint32_t* row) {
    row[UW_SLOT] = 0;
    row[UW_CURSOR] = 0;
}

struct UnionGraph {
    const uint64_t* rev_off;
    const uint32_t* rev_col;
    const uint8_t* rev_et;
    uint8_t et_contains;
    long long pkg_base;
    const int* items_off;   // [M + 1]
    const int* csr_pkgs;    // package indices, grouped by matched item
};

// Tier 1, whole wave: srv ∪= the distinct sources of CONTAINS edges into the
// installs csr_pkgs[beg .. beg + n_inst), one install per lane, the k-th edge
// of every lane's reverse row at a time.  False once the set would pass `cap`.
__device__ __forceinline__ bool collect_servers(const UnionGraph& g, int beg, int n_inst,
                                                uint32_t* srv, int& n_srv, int cap,
                                                uint32_t* stage, int lane) {
    bool ok = true;
    for (int base = 0; base < n_inst && ok; base += 64) {
        uint64_t e = 0, e_end = 0;
        if (base + lane < n_inst) {
            const long long node = g.pkg_base + g.csr_pkgs[beg + base + lane];
            e = g.rev_off[node];
            e_end = g.rev_off[node + 1];
        }
        for (; ok && __ballot(e < e_end); ++e) {
            const bool valid = e < e_end && g.rev_et[e] == g.et_contains;
            const uint32_t v = valid ? g.rev_col[e] : 0u;
            ok = append_distinct(srv, n_srv, cap, v, valid, stage, lane);
        }
    }
    return ok;
}

struct UnionSlice {
    uint32_t* srv;        // one bit per reach-index row
    uint32_t* planes;     // PLANES planes of plane_words each, one bit per node id
    long long plane_words;
    uint32_t node_span;
};

// The index row `r`, entries start, start + step, ... of its first PLANES
// segments (1: agents; 3: agents, creds, tools): set and count new bits
// (CLEAR = false) or return their words to zero.
template <bool CLEAR, int PLANES>
__device__ __forceinline__ void visit_row(const HopIndex& ix, const UnionSlice& sl, uint32_t r,
                                          int start, int step, int3& fresh) {
    const int4 off = ix.reach_off[r];
    static_assert(PLANES == 1 || PLANES == 3, "agents alone, or agents, creds and tools");
    const int end = PLANES == 3 ? off.w : off.y;
    for (int t = off.x + start; t < end; t += step) {
        const uint32_t v = ix.reach_col[t];
        if (v >= sl.node_span) continue;  // not reached: node_span covers reach_col
        const int kind = t < off.y ? 0 : t < off.z ? 1 : 2;
        uint32_t* word = sl.planes + kind * sl.plane_words + (v >> 5);
        if (CLEAR) {
            *word = 0;
        } else if (!(atomicOr(word, 1u << (v & 31)) & (1u << (v & 31)))) {
            fresh.x += kind == 0;
            fresh.y += kind == 1;
            fresh.z += kind == 2;
        }
    }
}

// One walk of an item by the block (256 threads): per chunk of 256 installs,
// a thread marks the servers of its install, the servers whose bit changed
// go to an LDS list, and the waves then visit the listed servers' index rows.
template <bool CLEAR, int PLANES>
__device__ __forceinline__ void walk_item(const UnionGraph& g, const HopIndex& ix,
                                          const UnionSlice& sl, int beg, int n_inst,
                                          uint32_t* list, unsigned* n_list, int& n_srv,
                                          int3& fresh) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int base = 0; base < n_inst; base += 256) {
        if (threadIdx.x == 0) *n_list = 0;
        __syncthreads();
        if (base + (int)threadIdx.x < n_inst) {
            const long long node = g.pkg_base + g.csr_pkgs[beg + base + threadIdx.x];
            for (uint64_t e = g.rev_off[node]; e < g.rev_off[node + 1]; ++e) {
                if (g.rev_et[e] != g.et_contains) continue;
                const uint32_t r = g.rev_col[e] - ix.row_base;
                if (r >= ix.num_rows) continue;  // not reached: see the preconditions
                const uint32_t bit = 1u << (r & 31);
                const uint32_t old = CLEAR ? atomicAnd(sl.srv + (r >> 5), ~bit)
                                           : atomicOr(sl.srv + (r >> 5), bit);
                if (((old & bit) != 0) != CLEAR) continue;  // another install had it
                ++n_srv;
                const unsigned slot = atomicAdd(n_list, 1u);
                if (slot < UNION_T2_LIST) list[slot] = r;
                else visit_row<CLEAR, PLANES>(ix, sl, r, 0, 1, fresh);  // list full: alone
            }
        }
        __syncthreads();
        const unsigned n = *n_list < UNION_T2_LIST ? *n_list : UNION_T2_LIST;
        for (unsigned j = wid; j < n; j += UNION_WAVES)
            visit_row<CLEAR, PLANES>(ix, sl, list[j], lane, 64, fresh);
        __syncthreads();
    }
}

// per matched item: servers, agents and, with PLANES == 3, creds and tools
struct UnionOut {
    int* n[4];
};

// Tier 1.  T gives SRV_CAP, AG_CAP and, with PLANES == 3, CR_CAP and TL_CAP;
// T1_INSTALLS, above which an item skips the tier; and ZERO_SLOT, whether
// lane 0 returns the slot and cursor of row items[m] of `state` to 0 (a user
// whose later passes still read the slot says no, and may pass both null).
template <class T>
__global__ void __launch_bounds__(256) union_wave_kernel(
    const int* __restrict__ items, long long M, UnionGraph g, HopIndex ix,
    uint32_t* __restrict__ state, uint32_t* __restrict__ queue,
    unsigned int* __restrict__ counters, UnionOut out) {
    static_assert(T::PLANES == 1 || T::PLANES == 3, "agents alone, or agents, creds and tools");
    __shared__ uint32_t lds_srv[UNION_WAVES][T::SRV_CAP];
    __shared__ uint32_t lds_ag[UNION_WAVES][T::AG_CAP];
    __shared__ uint32_t lds_stage[UNION_WAVES][64];
    __shared__ int lds_beg[UNION_WAVES][64];
    __shared__ int lds_pref[UNION_WAVES][64];

    const WaveId w = wave_id(UNION_WAVES);
    const int lane = w.lane, wid = w.wid;
    uint32_t* srv = lds_srv[wid];
    uint32_t* stage = lds_stage[wid];
    int* t_beg = lds_beg[wid];
    int* t_pref = lds_pref[wid];

    for (long long m = w.wave; m < M; m += w.n_waves) {
        if (T::ZERO_SLOT && lane == 0) slot_clear(state + (size_t)items[m] * UNION_ROW);
        const int beg = g.items_off[m];
        const int n_inst = g.items_off[m + 1] - beg;
        int n_srv = 0, n_ag = 0, n_cr = 0, n_tl = 0;
        bool ok = n_inst <= T::T1_INSTALLS;
        ok = ok && collect_servers(g, beg, n_inst, srv, n_srv, T::SRV_CAP, stage, lane);
        ok = ok && expand_append<AGENTS_OF_SERVER>(ix, srv, 0, n_srv, lds_ag[wid], n_ag,
                                                  T::AG_CAP, t_beg, t_pref, stage, lane);
        if constexpr (T::PLANES == 3) {
            // only this instance pays LDS for the two sets
            __shared__ uint32_t lds_cr[UNION_WAVES][T::CR_CAP];
            __shared__ uint32_t lds_tl[UNION_WAVES][T::TL_CAP];
            ok = ok && expand_append<CREDS_OF_SERVER>(ix, srv, 0, n_srv, lds_cr[wid], n_cr,
                                                     T::CR_CAP, t_beg, t_pref, stage, lane);
            ok = ok && expand_append<TOOLS_OF_SERVER>(ix, srv, 0, n_srv, lds_tl[wid], n_tl,
                                                     T::TL_CAP, t_beg, t_pref, stage, lane);
        }
        if (ok && lane == 0) {
            out.n[0][m] = n_srv;
            out.n[1][m] = n_ag;
            if constexpr (T::PLANES == 3) {
                out.n[2][m] = n_cr;
                out.n[3][m] = n_tl;
            }
        }
        wave_queue_push(!ok && lane == 0, (uint32_t)m, queue, &counters[UC_QUEUED], lane);
        __builtin_amdgcn_wave_barrier();
    }
}

// Tier 2: block b owns slice b of the pool and takes the queued items b,
// b + gridDim.x, ...
template <int PLANES>
__global__ void __launch_bounds__(256) union_block_kernel(
    UnionGraph g, HopIndex ix, const uint32_t* __restrict__ queue,
    unsigned int* __restrict__ counters, uint32_t* __restrict__ pool,
    long long srv_words, long long plane_words, uint32_t node_span, UnionOut out) {
    __shared__ uint32_t list[UNION_T2_LIST];
    __shared__ unsigned n_list;
    __shared__ int totals[1 + PLANES];
    const unsigned n_queued = counters[UC_QUEUED];
    UnionSlice sl;
    sl.srv = pool + (size_t)blockIdx.x * (size_t)(srv_words + PLANES * plane_words);
    sl.planes = sl.srv + srv_words;
    sl.plane_words = plane_words;
    sl.node_span = node_span;
    if (blockIdx.x == 0 && threadIdx.x == 0)
        counters[UC_ROUNDS] = (n_queued + gridDim.x - 1) / gridDim.x;
    for (unsigned q = blockIdx.x; q < n_queued; q += gridDim.x) {
        const long long m = queue[q];
        const int beg = g.items_off[m];
        const int n_inst = g.items_off[m + 1] - beg;
        if (threadIdx.x < 1 + PLANES) totals[threadIdx.x] = 0;
        int n_srv = 0, unused_srv = 0;
        int3 fresh = make_int3(0, 0, 0), unused = make_int3(0, 0, 0);
        walk_item<false, PLANES>(g, ix, sl, beg, n_inst, list, &n_list, n_srv, fresh);
        walk_item<true, PLANES>(g, ix, sl, beg, n_inst, list, &n_list, unused_srv, unused);
        n_srv = wave_sum(n_srv);
        fresh.x = wave_sum(fresh.x);
        if constexpr (PLANES == 3) {
            fresh.y = wave_sum(fresh.y);
            fresh.z = wave_sum(fresh.z);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&totals[0], n_srv);
            atomicAdd(&totals[1], fresh.x);
            if constexpr (PLANES == 3) {
                atomicAdd(&totals[2], fresh.y);
                atomicAdd(&totals[3], fresh.z);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < 1 + PLANES; ++k) out.n[k][m] = totals[k];
        __syncthreads();
    }
}

// Both tiers for the M matched items `items` (ascending; read only with
// T::ZERO_SLOT) whose installs are csr_pkgs[items_off[m] .. items_off[m + 1]).
// `queue` holds M words, `pool` pool_slices slices, all-zero before and after;
// `counters` as above.  Returns the first error.
template <class T>
inline int launch_union_tiers(
    const void* items, long long M, const void* items_off, const void* csr_pkgs,
    long long pkg_base,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    const void* reach_off, const void* reach_col, long long row_base, long long num_rows,
    long long node_span, void* state, void* queue, void* pool, long long pool_slices,
    void* counters, const UnionOut& out, hipStream_t s) {
    if (pool_slices < 1 || node_span < 0 || node_span >= (1ll << 32)) return (int)hipErrorInvalidValue;
    if (M <= 0) return 0;
    UnionGraph g;
    g.rev_off = (const uint64_t*)rev_off;
    g.rev_col = (const uint32_t*)rev_col;
    g.rev_et = (const uint8_t*)rev_et;
    g.et_contains = (uint8_t)et_contains;
    g.pkg_base = pkg_base;
    g.items_off = (const int*)items_off;
    g.csr_pkgs = (const int*)csr_pkgs;
    const HopIndex ix = make_hop_index(reach_off, reach_col, row_base, num_rows, nullptr, nullptr, 0);
    hipLaunchKernelGGL(union_wave_kernel<T>, dim3(grid_for(M, UNION_WAVES)), dim3(256), 0, s,
                       (const int*)items, M, g, ix, (uint32_t*)state, (uint32_t*)queue,
                       (unsigned int*)counters, out);
    ABOM_CHECK(hipGetLastError());
    // the queue length is known on the device only: one block per slice, a
    // block without a queued item leaves at once
    const long long blocks = pool_slices < M ? pool_slices : M;
    hipLaunchKernelGGL(union_block_kernel<T::PLANES>, dim3((unsigned)blocks), dim3(256), 0, s,
                       g, ix, (const uint32_t*)queue, (unsigned int*)counters, (uint32_t*)pool,
                       (num_rows + 31) / 32, (node_span + 31) / 32, (uint32_t)node_span, out);
    return (int)hipGetLastError();
}

}  // namespace abom
