// Batched bounded blast-radius query (impact_of / traverse_subgraph).
//
// One BLOCK per query: a small BFS bounded by max_hops (<=4 default, matching
// container.impact_of) and max_nodes per query.  The visited set is an
// open-addressed hash table in LDS (8K slots), the per-level frontier also
// lives in LDS.  Collected (node, hop) pairs stream to the query's output
// slab.  Used for p50 blast-radius query latency and the /v1/graph read path.

#include "abom_api.h"
#include "abom_common.h"

namespace abom {

constexpr int IQ_HASH = 8192;       // LDS hash slots (32 KB)
constexpr int IQ_FRONTIER = 2048;   // per-level frontier cap in LDS

__global__ void impact_query_kernel(
    const uint64_t* __restrict__ row_off,
    const uint32_t* __restrict__ col,
    const uint8_t* __restrict__ etype,
    uint32_t allowed_mask,
    const uint32_t* __restrict__ query_sources,   // [Q]
    int num_queries,
    int max_hops,
    int max_nodes_per_query,                      // slab stride
    uint32_t* __restrict__ out_nodes,             // [Q * stride]
    uint8_t* __restrict__ out_hops,               // [Q * stride]
    uint32_t* __restrict__ out_counts,            // [Q] (clamped to stride)
    uint8_t* __restrict__ out_truncated) {        // [Q]
    __shared__ uint32_t h_table[IQ_HASH];
    __shared__ uint32_t fr[2][IQ_FRONTIER];
    __shared__ unsigned fr_size[2];
    __shared__ unsigned out_cursor;
    __shared__ unsigned truncated;

    for (int q = blockIdx.x; q < num_queries; q += gridDim.x) {
        // reset LDS state
        for (int i = threadIdx.x; i < IQ_HASH; i += blockDim.x) h_table[i] = ABOM_UNVISITED;
        // the seed below lands in a slot that another wave clears: without
        // this barrier a late clear wipes it, and a cycle back to the source
        // reports the source a second time
        __syncthreads();
        if (threadIdx.x == 0) {
            fr_size[0] = 1;
            fr_size[1] = 0;
            out_cursor = 0;
            truncated = 0;
            fr[0][0] = query_sources[q];
            // seed visited
            uint32_t s = query_sources[q];
            uint32_t h = (s * 2654435761u) & (IQ_HASH - 1);
            h_table[h] = s;
        }
        __syncthreads();

        uint32_t* slab_nodes = out_nodes + (long long)q * max_nodes_per_query;
        uint8_t* slab_hops = out_hops + (long long)q * max_nodes_per_query;
        if (threadIdx.x == 0 && max_nodes_per_query > 0) {
            slab_nodes[0] = fr[0][0];
            slab_hops[0] = 0;
            out_cursor = 1;
        }
        __syncthreads();

        int cur = 0;
        for (int hop = 1; hop <= max_hops; ++hop) {
            const int nxt = cur ^ 1;
            const unsigned fsz = fr_size[cur];
            if (fsz == 0) break;
            __syncthreads();
            // Threads stride the (frontier x neighbor) work by frontier entry.
            for (unsigned i = threadIdx.x; i < fsz; i += blockDim.x) {
                const uint32_t u = fr[cur][i];
                const uint64_t beg = row_off[u];
                const uint64_t end = row_off[u + 1];
                for (uint64_t e = beg; e < end; ++e) {
                    if (edge_filtered(etype, allowed_mask, e)) continue;
                    const uint32_t v = col[e];
                    // LDS open-addressing insert; full table => truncate.
                    uint32_t h = (v * 2654435761u) & (IQ_HASH - 1);
                    bool inserted = false, seen = false;
                    for (int probe = 0; probe < 64; ++probe) {
                        uint32_t prev = atomicCAS(&h_table[h], ABOM_UNVISITED, v);
                        if (prev == ABOM_UNVISITED) { inserted = true; break; }
                        if (prev == v) { seen = true; break; }
                        h = (h + 1) & (IQ_HASH - 1);
                    }
                    if (seen) continue;
                    if (!inserted) { truncated = 1; continue; }
                    const unsigned oi = atomicAdd(&out_cursor, 1u);
                    if ((int)oi < max_nodes_per_query) {
                        slab_nodes[oi] = v;
                        slab_hops[oi] = (uint8_t)hop;
                    } else {
                        truncated = 1;
                    }
                    const unsigned fi = atomicAdd(&fr_size[nxt], 1u);
                    if ((int)fi < IQ_FRONTIER) fr[nxt][fi] = v;
                    else truncated = 1;
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                if (fr_size[nxt] > IQ_FRONTIER) fr_size[nxt] = IQ_FRONTIER;
                fr_size[cur] = 0;
            }
            cur = nxt;
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            out_counts[q] = out_cursor < (unsigned)max_nodes_per_query ? out_cursor
                                                                       : (unsigned)max_nodes_per_query;
            out_truncated[q] = (uint8_t)truncated;
        }
        __syncthreads();
    }
}

}  // namespace abom

extern "C" int abom_impact_query(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* query_sources, int num_queries, int max_hops, int max_nodes_per_query,
    void* out_nodes, void* out_hops, void* out_counts, void* out_truncated, void* stream) {
    const int block = 256;
    const int grid = num_queries < 2048 ? (num_queries > 0 ? num_queries : 1) : 2048;
    hipLaunchKernelGGL(abom::impact_query_kernel, dim3(grid), dim3(block), 0,
                       (hipStream_t)stream, (const uint64_t*)row_off, (const uint32_t*)col,
                       (const uint8_t*)etype, allowed_mask, (const uint32_t*)query_sources,
                       num_queries, max_hops, max_nodes_per_query, (uint32_t*)out_nodes,
                       (uint8_t*)out_hops, (uint32_t*)out_counts, (uint8_t*)out_truncated);
    return (int)hipGetLastError();
}
