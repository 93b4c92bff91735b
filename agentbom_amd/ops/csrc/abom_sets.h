// Capped distinct sets in LDS, one per wave, over the per-server reach index
// and the per-agent server index (gfx950, wave64).  Shared by the multi-hop
// expansion (blast_hops.hip) and, through abom_union.h, the remediation and
// toxic-combination unions (remediation.hip, toxic.hip).
// Every helper here must be reached by all lanes of the wave.
#pragma once

#include "abom_wave.h"

namespace abom {

constexpr uint32_t HOPS_NONE = 0xFFFFFFFFu;

struct HopIndex {
    const int4* reach_off;      // [num_rows] (agents, creds, tools, end)
    const uint32_t* reach_col;
    uint32_t row_base, num_rows;
    const int* agent_off;       // [num_agents + 1]
    const uint32_t* agent_srv;
    uint32_t num_agents;
};

// host: the agent fields are null / 0 for a user of the server rows alone
inline HopIndex make_hop_index(const void* reach_off, const void* reach_col, long long row_base,
                               long long num_rows, const void* agent_off, const void* agent_srv,
                               long long num_agents) {
    HopIndex ix;
    ix.reach_off = (const int4*)reach_off;
    ix.reach_col = (const uint32_t*)reach_col;
    ix.row_base = (uint32_t)row_base;
    ix.num_rows = (uint32_t)num_rows;
    ix.agent_off = (const int*)agent_off;
    ix.agent_srv = (const uint32_t*)agent_srv;
    ix.num_agents = (uint32_t)num_agents;
    return ix;
}

enum HopSegment { AGENTS_OF_SERVER, CREDS_OF_SERVER, TOOLS_OF_SERVER, SERVERS_OF_AGENT };

// (begin, length) of the node's segment; empty for a node without a row
template <HopSegment KIND>
__device__ __forceinline__ int2 hop_segment(const HopIndex& ix, uint32_t node) {
    if (KIND == SERVERS_OF_AGENT) {
        if (node >= ix.num_agents) return make_int2(0, 0);
        const int beg = ix.agent_off[node];
        return make_int2(beg, ix.agent_off[node + 1] - beg);
    }
    const uint32_t row = node - ix.row_base;
    if (row >= ix.num_rows) return make_int2(0, 0);
    const int4 off = ix.reach_off[row];
    if (KIND == TOOLS_OF_SERVER) return make_int2(off.z, off.w - off.z);
    return KIND == AGENTS_OF_SERVER ? make_int2(off.x, off.y - off.x)
                                    : make_int2(off.y, off.z - off.y);
}

// Append this wave's candidates (one per lane with `valid`) that are neither
// in list[0..n) nor held by an earlier lane.  False, with nothing stored, when
// the list would pass `cap`: the bound is checked before any store.
__device__ __forceinline__ bool append_distinct(
    uint32_t* list, int& n, int cap, uint32_t v, bool valid, uint32_t* stage, int lane) {
    stage[lane] = valid ? v : HOPS_NONE;
    __builtin_amdgcn_wave_barrier();
    bool fresh = valid;
    if (valid) {
        int dup = 0, j = 0;
        for (; j + 4 <= n; j += 4)
            dup |= (list[j] == v) | (list[j + 1] == v) | (list[j + 2] == v) | (list[j + 3] == v);
        for (; j < n; ++j) dup |= list[j] == v;
        for (j = 0; j < lane; ++j) dup |= stage[j] == v;
        fresh = !dup;
    }
    const unsigned long long fmask = __ballot(fresh);
    const int total = n + __popcll(fmask);
    if (total > cap) return false;
    if (fresh) list[n + __popcll(fmask & ((1ull << lane) - 1))] = v;
    __builtin_amdgcn_wave_barrier();
    n = total;
    return true;
}

// dst ∪= the KIND segments of items[i_beg..i_end), 64 items at a time: their
// segments are laid end to end (t_pref = exclusive prefix of the lengths) and
// entry j belongs to the last item with t_pref <= j.  False on overflow.
template <HopSegment KIND>
__device__ __forceinline__ bool expand_append(
    const HopIndex& ix, const uint32_t* items, int i_beg, int i_end,
    uint32_t* dst, int& n_dst, int cap, int* t_beg, int* t_pref, uint32_t* stage, int lane) {
    const uint32_t* __restrict__ col = KIND == SERVERS_OF_AGENT ? ix.agent_srv : ix.reach_col;
    for (int base = i_beg; base < i_end; base += 64) {
        const int i = base + lane;
        int2 seg = make_int2(0, 0);
        if (i < i_end) seg = hop_segment<KIND>(ix, items[i]);
        int total;
        const int pref = wave_exclusive_scan(seg.y, lane, &total);
        t_beg[lane] = seg.x;
        t_pref[lane] = pref;
        __builtin_amdgcn_wave_barrier();
        const int n_items = i_end - base < 64 ? i_end - base : 64;
        for (int k = 0; k < total; k += 64) {
            const int j = k + lane;
            const bool valid = j < total;
            uint32_t v = 0;
            if (valid) {
                const int s = segment_of(t_pref, n_items, j);
                v = col[t_beg[s] + (j - t_pref[s])];
            }
            if (!append_distinct(dst, n_dst, cap, v, valid, stage, lane)) return false;
        }
        __builtin_amdgcn_wave_barrier();  // the tables are rewritten next round
    }
    return true;
}

}  // namespace abom
