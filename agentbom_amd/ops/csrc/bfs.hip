// Dependency-reach BFS: level-synchronous multi-source BFS over CSR in HBM.
//
// Replaces the reference's Python adjacency-dict walks
// (reference: src/agent_bom/graph/dependency_reach.py:109-198 per-agent BFS,
// src/agent_bom/graph/container.py:613-683 BFS/impact_of/traverse_subgraph)
// with frontier kernels over a CSR whose 10M-100M nodes stay resident in
// 288 GB of HBM3E.
//
// BFS design (CDNA4):
// - one thread per frontier vertex, grid-stride; dist claims via atomicCAS
//   from UNVISITED so each vertex is pushed exactly once (level-synchronous
//   => first touch is the minimal hop).
// - edge-type filtering via a 32-bit allowed-mask over per-edge type bytes
//   (the reference traverses only USES/DEPENDS_ON/CONTAINS/PROVIDES_TOOL
//   classes for dependency reach — types are a closed enum).
// - high-degree frontier vertices (skewed estates: ~1% of agents fan out
//   18-32x) are handled wave-cooperatively: degree >= 64 vertices are
//   expanded by whole waves from a secondary queue filled in pass 1.
// - dense levels (frontier edges > 1/8 of all edges) switch to a pass over
//   all edges or, with a reverse CSR, a bottom-up pass over all vertices.
//
// The host-side level loop is abom_bfs_run at the end of this file (C++, one
// sync per level).

#include "abom_api.h"
#include "abom_common.h"

namespace abom {

// Slots of the device counter array shared by the kernels and the level loop
// (mirrored in ops/native.py).
enum { CTR_NEXT = 0, CTR_HEAVY = 1, CTR_DEGREE = 2, CTR_SLOTS = 3 };

// One atomic per wave: lanes accumulate locally, reduce, lane 0 adds.
__device__ __forceinline__ void wave_add_degree(unsigned int* dst, unsigned v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, v);
}

// Claim v for `level` and append it to the next frontier.  Returns v's
// out-degree when this thread won the claim, 0 otherwise.  The relaxed
// pre-check keeps atomics off already-visited vertices.
__device__ __forceinline__ unsigned claim_and_append(
    uint32_t v, uint32_t level, uint32_t* __restrict__ dist,
    const uint64_t* __restrict__ row_off, uint32_t* __restrict__ next_frontier,
    unsigned int* __restrict__ next_count, long long capacity) {
    if (dist[v] != ABOM_UNVISITED ||
        atomicCAS(&dist[v], ABOM_UNVISITED, level) != ABOM_UNVISITED)
        return 0;
    const unsigned idx = atomicAdd(next_count, 1u);
    if ((long long)idx < capacity) next_frontier[idx] = v;
    return (unsigned)(row_off[v + 1] - row_off[v]);
}

// Pass over the frontier: expand vertices with degree < WAVE_DEG inline;
// defer heavy vertices to the heavy queue.
__global__ void bfs_expand_kernel(
    const uint64_t* __restrict__ row_off,   // [N+1]
    const uint32_t* __restrict__ col,       // [E]
    const uint8_t* __restrict__ etype,      // [E] or nullptr
    uint32_t allowed_mask,
    const uint32_t* __restrict__ frontier,
    long long frontier_size,
    uint32_t* __restrict__ dist,
    uint32_t next_level,
    uint32_t* __restrict__ next_frontier,
    unsigned int* __restrict__ next_count,
    uint32_t* __restrict__ heavy_queue,
    unsigned int* __restrict__ heavy_count,
    unsigned int* __restrict__ next_degree_sum,
    long long capacity) {
    constexpr uint64_t WAVE_DEG = 64;
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned my_deg = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < frontier_size;
         i += stride) {
        const uint32_t u = frontier[i];
        const uint64_t beg = row_off[u];
        const uint64_t end = row_off[u + 1];
        if (end - beg >= WAVE_DEG) {
            heavy_queue[atomicAdd(heavy_count, 1u)] = u;
            continue;
        }
        for (uint64_t e = beg; e < end; ++e) {
            if (edge_filtered(etype, allowed_mask, e)) continue;
            my_deg += claim_and_append(col[e], next_level, dist, row_off, next_frontier,
                                       next_count, capacity);
        }
    }
    wave_add_degree(next_degree_sum, my_deg);
}

// Wave-cooperative expansion of heavy vertices: one wave (64 lanes) walks one
// vertex's adjacency with coalesced col[] reads.
__global__ void bfs_expand_heavy_kernel(
    const uint64_t* __restrict__ row_off,
    const uint32_t* __restrict__ col,
    const uint8_t* __restrict__ etype,
    uint32_t allowed_mask,
    const uint32_t* __restrict__ heavy_queue,
    const unsigned int* __restrict__ heavy_size_ptr,
    uint32_t* __restrict__ dist,
    uint32_t next_level,
    uint32_t* __restrict__ next_frontier,
    unsigned int* __restrict__ next_count,
    unsigned int* __restrict__ next_degree_sum,
    long long capacity) {
    const unsigned heavy_size = *heavy_size_ptr;
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    unsigned my_deg = 0;
    for (long long q = wave; q < heavy_size; q += nwaves) {
        const uint32_t u = heavy_queue[q];
        const uint64_t beg = row_off[u];
        const uint64_t end = row_off[u + 1];
        for (uint64_t e = beg + lane; e < end; e += 64) {
            if (edge_filtered(etype, allowed_mask, e)) continue;
            my_deg += claim_and_append(col[e], next_level, dist, row_off, next_frontier,
                                       next_count, capacity);
        }
    }
    wave_add_degree(next_degree_sum, my_deg);
}

// Edge-centric expansion for DENSE frontiers: one thread per edge, fully
// coalesced src/col streams.  Used when the frontier would touch a large
// share of all edges (the agent->server->everything levels of estate
// graphs), where per-vertex serial neighbor loops are latency-bound.
// Requires the per-edge source array (edge_src, same order as col).
// build_frontier == 0: dist-driven mode for subsequent edge-centric levels —
// claims are only counted (one wave-reduced atomic per wave), no frontier
// append, no degree accumulation.  Removes the single-counter atomic storm
// on claim-heavy levels (~10M returning atomicAdds on one word otherwise).
__global__ void bfs_expand_edges_kernel(
    const uint32_t* __restrict__ edge_src,   // [E]
    const uint32_t* __restrict__ col,        // [E]
    const uint8_t* __restrict__ etype,       // [E] or nullptr
    uint32_t allowed_mask,
    long long num_edges,
    const uint64_t* __restrict__ row_off,
    uint32_t* __restrict__ dist,
    uint32_t cur_level,                      // frontier's level (claimed at cur_level)
    uint32_t* __restrict__ next_frontier,
    unsigned int* __restrict__ next_count,
    unsigned int* __restrict__ next_degree_sum,
    int build_frontier,
    long long capacity) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned my_deg = 0;
    unsigned my_claims = 0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < num_edges;
         e += stride) {
        if (edge_filtered(etype, allowed_mask, e)) continue;
        if (dist[edge_src[e]] != cur_level) continue;
        const uint32_t v = col[e];
        if (build_frontier) {
            my_deg += claim_and_append(v, cur_level + 1, dist, row_off, next_frontier,
                                       next_count, capacity);
        } else if (dist[v] == ABOM_UNVISITED) {
            // dist-driven mode: every racer writes the SAME value, so a plain
            // store is exact (level-synchronous); the claim count may double-
            // count racers but is only used for termination (>0) and the
            // hand-back threshold — both tolerant of overcounting.
            dist[v] = cur_level + 1;
            ++my_claims;
        }
    }
    wave_add_degree(next_degree_sum, my_deg);
    if (!build_frontier) wave_add_degree(next_count, my_claims);
}

// Direction-optimized bottom-up step: every UNVISITED vertex probes its
// REVERSE edges for a parent in the current frontier and claims itself.
// dist[v] reads/writes are coalesced (v is the loop index), the per-vertex
// probe loop EARLY-EXITS on the first frontier parent, and no frontier is
// materialized — the dense-level complement of the edge-centric push pass.
__global__ void bfs_bottom_up_kernel(
    const uint64_t* __restrict__ rev_off,
    const uint32_t* __restrict__ rev_col,
    const uint8_t* __restrict__ rev_et,   // type of edge (parent -> v)
    uint32_t allowed_mask,
    long long num_nodes,
    uint32_t* __restrict__ dist,
    uint32_t cur_level,
    unsigned int* __restrict__ next_count) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned my_claims = 0;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < num_nodes;
         v += stride) {
        if (dist[v] != ABOM_UNVISITED) continue;
        const uint64_t beg = rev_off[v];
        const uint64_t end = rev_off[v + 1];
        for (uint64_t e = beg; e < end; ++e) {
            if (edge_filtered(rev_et, allowed_mask, e)) continue;
            if (dist[rev_col[e]] == cur_level) {
                dist[v] = cur_level + 1;
                ++my_claims;
                break;
            }
        }
    }
    wave_add_degree(next_count, my_claims);
}

// Rebuild a frontier from dist (nodes claimed at `level`): used when
// dist-driven dense mode hands back to vertex-frontier mode after the
// claim rate drops.  Claim counts are small here, so appends are cheap.
__global__ void collect_frontier_kernel(
    const uint32_t* __restrict__ dist, long long num_nodes, uint32_t level,
    const uint64_t* __restrict__ row_off,
    uint32_t* __restrict__ frontier, unsigned int* __restrict__ count,
    unsigned int* __restrict__ degree_sum, long long capacity) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned my_deg = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < num_nodes;
         i += stride) {
        if (dist[i] == level) {
            const unsigned idx = atomicAdd(count, 1u);
            if ((long long)idx < capacity) frontier[idx] = (uint32_t)i;
            my_deg += (unsigned)(row_off[i + 1] - row_off[i]);
        }
    }
    wave_add_degree(degree_sum, my_deg);
}

__global__ void seed_sources_kernel(
    const uint32_t* __restrict__ sources, long long n_sources,
    const uint64_t* __restrict__ row_off,
    uint32_t* __restrict__ dist, uint32_t* __restrict__ frontier,
    unsigned int* __restrict__ degree_sum) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned my_deg = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_sources;
         i += stride) {
        const uint32_t s = sources[i];
        dist[s] = 0;
        frontier[i] = s;
        my_deg += (unsigned)(row_off[s + 1] - row_off[s]);
    }
    wave_add_degree(degree_sum, my_deg);
}

// ── Host helpers of the level loop ─────────────────────────────────────────

static int bfs_init(void* dist, long long n, hipStream_t s) {
    // ABOM_UNVISITED is 0xFFFFFFFF — a byte-uniform pattern, so the DMA
    // memset path beats a grid-stride store kernel (and frees the CUs for
    // the match kernel running concurrently on the side stream).
    return (int)hipMemsetAsync(dist, 0xFF, (size_t)n * sizeof(uint32_t), s);
}

static int bfs_seed(const void* sources, long long n_sources, const void* row_off, void* dist,
                    void* frontier, unsigned int* degree_sum, hipStream_t s) {
    const int block = 256;
    hipLaunchKernelGGL(seed_sources_kernel, dim3(grid_for(n_sources, block)), dim3(block), 0, s,
                       (const uint32_t*)sources, n_sources, (const uint64_t*)row_off,
                       (uint32_t*)dist, (uint32_t*)frontier, degree_sum);
    return (int)hipGetLastError();
}

static int reset_counters(unsigned int* ctr, hipStream_t s) {
    return (int)hipMemsetAsync(ctr, 0, CTR_SLOTS * sizeof(unsigned int), s);
}

// Device -> host read of `n` counters; the one sync point of a level.
static int read_counters(unsigned int* host, const unsigned int* dev, int n, hipStream_t s) {
    ABOM_CHECK(hipMemcpyAsync(host, dev, n * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    return (int)hipStreamSynchronize(s);
}

// One sparse level: per-vertex expansion, then the heavy queue it filled.
static int expand_level(const void* row_off, const void* col, const void* etype,
                        unsigned int allowed_mask, const void* frontier,
                        long long frontier_size, void* dist, unsigned int next_level,
                        void* next_frontier, unsigned int* ctr, void* heavy_queue,
                        long long capacity, void* stream) {
    int rc = abom_bfs_expand(row_off, col, etype, allowed_mask, frontier, frontier_size, dist,
                             next_level, next_frontier, ctr + CTR_NEXT, heavy_queue,
                             ctr + CTR_HEAVY, ctr + CTR_DEGREE, capacity, stream);
    if (rc) return rc;
    return abom_bfs_expand_heavy(row_off, col, etype, allowed_mask, heavy_queue,
                                 ctr + CTR_HEAVY, dist, next_level, next_frontier,
                                 ctr + CTR_NEXT, ctr + CTR_DEGREE, capacity, stream);
}

}  // namespace abom

// ── C ABI: single-level launches ───────────────────────────────────────────

extern "C" int abom_bfs_expand(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* frontier, long long frontier_size, void* dist, unsigned int next_level,
    void* next_frontier, void* next_count, void* heavy_queue, void* heavy_count,
    void* next_degree_sum, long long capacity, void* stream) {
    const int block = 256;
    hipLaunchKernelGGL(abom::bfs_expand_kernel, dim3(abom::grid_for(frontier_size, block)),
                       dim3(block), 0, (hipStream_t)stream, (const uint64_t*)row_off,
                       (const uint32_t*)col, (const uint8_t*)etype, allowed_mask,
                       (const uint32_t*)frontier, frontier_size, (uint32_t*)dist, next_level,
                       (uint32_t*)next_frontier, (unsigned int*)next_count,
                       (uint32_t*)heavy_queue, (unsigned int*)heavy_count,
                       (unsigned int*)next_degree_sum, capacity);
    return (int)hipGetLastError();
}

extern "C" int abom_bfs_expand_heavy(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* heavy_queue, const void* heavy_size_ptr, void* dist, unsigned int next_level,
    void* next_frontier, void* next_count, void* next_degree_sum, long long capacity,
    void* stream) {
    const int block = 256;  // 4 waves per block; kernel grid-strides by wave
    hipLaunchKernelGGL(abom::bfs_expand_heavy_kernel, dim3(2048), dim3(block), 0,
                       (hipStream_t)stream, (const uint64_t*)row_off, (const uint32_t*)col,
                       (const uint8_t*)etype, allowed_mask, (const uint32_t*)heavy_queue,
                       (const unsigned int*)heavy_size_ptr, (uint32_t*)dist, next_level,
                       (uint32_t*)next_frontier, (unsigned int*)next_count,
                       (unsigned int*)next_degree_sum, capacity);
    return (int)hipGetLastError();
}

extern "C" int abom_bfs_expand_edges(
    const void* edge_src, const void* col, const void* etype, unsigned int allowed_mask,
    long long num_edges, const void* row_off, void* dist, unsigned int cur_level,
    void* next_frontier, void* next_count, void* next_degree_sum, int build_frontier,
    long long capacity, void* stream) {
    const int block = 256;
    hipLaunchKernelGGL(abom::bfs_expand_edges_kernel, dim3(abom::grid_for(num_edges, block)),
                       dim3(block), 0, (hipStream_t)stream, (const uint32_t*)edge_src,
                       (const uint32_t*)col, (const uint8_t*)etype, allowed_mask, num_edges,
                       (const uint64_t*)row_off, (uint32_t*)dist, cur_level,
                       (uint32_t*)next_frontier, (unsigned int*)next_count,
                       (unsigned int*)next_degree_sum, build_frontier, capacity);
    return (int)hipGetLastError();
}

// ── C ABI: the level loop ──────────────────────────────────────────────────

// Full multi-source BFS: host-side level loop, one device->host count read
// per level.  dist must be u32[N]; frontier_a/b u32[N]; heavy_queue u32[N];
// counters = device u32[CTR_SLOTS].  ``edge_src`` (the per-edge source
// array, col-aligned) may be null; when present, levels whose frontier would
// touch > ~1/8 of all edges go dense: bottom-up over the reverse CSR when
// rev_off/rev_col are given, else the edge-centric kernel (coalesced
// streams), instead of per-vertex expansion.
// Returns negative hip error or the number of levels run.
extern "C" int abom_bfs_run(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* sources, long long n_sources, void* dist, long long num_nodes,
    void* frontier_a, void* frontier_b, void* heavy_queue, void* counters,
    int max_levels, const void* edge_src, long long num_edges, double avg_degree,
    const void* rev_off, const void* rev_col, const void* rev_et,
    void* stream) {
    using namespace abom;
    (void)avg_degree;  // part of ABI v1; the mode switches use exact degree sums
    hipStream_t s = (hipStream_t)stream;
    unsigned int* ctr = (unsigned int*)counters;
    int rc = bfs_init(dist, num_nodes, s);
    if (rc) return -rc;
    if ((rc = reset_counters(ctr, s))) return -rc;
    rc = bfs_seed(sources, n_sources, row_off, dist, frontier_a, ctr + CTR_DEGREE, s);
    if (rc) return -rc;
    unsigned int frontier_degree = 0;
    if ((rc = read_counters(&frontier_degree, ctr + CTR_DEGREE, 1, s))) return -rc;

    uint32_t* cur = (uint32_t*)frontier_a;
    uint32_t* nxt = (uint32_t*)frontier_b;
    long long frontier_size = n_sources;  // < 0: rebuild the frontier from dist
    int level = 0;
    bool stay_dense = false;
    while (frontier_size != 0 && level < max_levels) {
        ++level;
        if ((rc = reset_counters(ctr, s))) return -rc;
        // Dense frontier (its edges are a big share of ALL edges): a pass
        // over all edges / all unvisited vertices with coalesced streams
        // beats per-vertex serial neighbor loops.  Once dense mode fires,
        // stay dist-driven: dense levels never materialize a frontier,
        // claims are wave-counted only.
        const bool dense = stay_dense ||
                           (edge_src != nullptr && num_edges > 0 &&
                            (double)frontier_degree > (double)num_edges / 8.0);
        if (dense) {
            stay_dense = true;
            if (rev_off && rev_col) {
                hipLaunchKernelGGL(bfs_bottom_up_kernel,
                                   dim3(abom::grid_for(num_nodes, 256)), dim3(256), 0, s,
                                   (const uint64_t*)rev_off, (const uint32_t*)rev_col,
                                   (const uint8_t*)rev_et, allowed_mask, num_nodes,
                                   (uint32_t*)dist, (unsigned int)(level - 1), ctr + CTR_NEXT);
                rc = (int)hipGetLastError();
            } else {
                rc = abom_bfs_expand_edges(edge_src, col, etype, allowed_mask, num_edges,
                                           row_off, dist, (unsigned int)(level - 1), nxt,
                                           ctr + CTR_NEXT, ctr + CTR_DEGREE,
                                           /*build_frontier=*/0, num_nodes, stream);
            }
            if (rc) return -rc;
        } else {
            if (frontier_size < 0) {
                // dense mode handed back: rebuild the frontier from dist
                hipLaunchKernelGGL(collect_frontier_kernel,
                                   dim3(abom::grid_for(num_nodes, 256)), dim3(256), 0, s,
                                   (const uint32_t*)dist, num_nodes,
                                   (unsigned int)(level - 1), (const uint64_t*)row_off,
                                   cur, ctr + CTR_NEXT, ctr + CTR_DEGREE, num_nodes);
                rc = (int)hipGetLastError();
                if (rc) return -rc;
                unsigned int rebuilt = 0;
                if ((rc = read_counters(&rebuilt, ctr + CTR_NEXT, 1, s))) return -rc;
                frontier_size = rebuilt;
                // reset all counters: the rebuilt frontier's degree sum is
                // the CURRENT level's, while the dense decision needs the
                // NEXT frontier's (accumulated by the expand below)
                if ((rc = reset_counters(ctr, s))) return -rc;
            }
            rc = expand_level(row_off, col, etype, allowed_mask, cur, frontier_size, dist,
                              (unsigned int)level, nxt, ctr, heavy_queue, num_nodes, stream);
            if (rc) return -rc;
        }
        unsigned int host_ctr[CTR_SLOTS] = {0, 0, 0};
        if ((rc = read_counters(host_ctr, ctr, CTR_SLOTS, s))) return -rc;
        frontier_size = host_ctr[CTR_NEXT];
        frontier_degree = host_ctr[CTR_DEGREE];
        if (stay_dense && frontier_size > 0 &&
            (double)frontier_size < (double)num_edges / 4096.0) {
            // dense claims have trickled out: hand back to vertex mode next
            // level (frontier rebuilt from dist — signalled by negative size)
            stay_dense = false;
            frontier_size = -1;
        }
        uint32_t* t = cur; cur = nxt; nxt = t;
    }
    return level;
}
