// Distinct unions over the installs of an item (a remediation item, an
// advisory): the servers that hold an install and, through the per-server
// reach index, what those servers reach.  Shared by remediation.hip and
// toxic.hip.  Tier 1 is a capped LDS set per wave (abom_sets.h); tier 2 a
// slice of a bitmap pool per block, set in one walk and cleared in a second,
// so a slice is all-zero whenever a block leaves an item.
#pragma once

#include "abom_sets.h"

namespace abom {

constexpr int UNION_WAVES = 4;      // waves per block of both tiers
constexpr int UNION_T2_LIST = 1024; // servers a tier-2 block lists per chunk

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

}  // namespace abom
