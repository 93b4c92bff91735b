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
// - with a parent index (abom_bfs_parent_index: per vertex the first allowed
//   in-edge of its reverse row, built once per reverse CSR and mask) the
//   bottom-up pass reads dist and one index word per vertex, four vertices
//   per thread with 16-byte loads, and gathers dist[parent]; the reverse row
//   is walked only when that parent is outside the frontier and the row has
//   another allowed in-edge.  The row walk alone is a chain of four
//   dependent loads per vertex over 64-bit offsets, type bytes and columns.
// - a block of bfs_expand_kernel or bfs_expand_heavy_kernel stages its claims
//   in an LDS queue and reserves their slots of the next frontier with ONE
//   atomic per flush: the frontier counter is a single word, and a returning
//   atomic per wave and edge-loop iteration ran both kernels at that word's
//   atomic rate (208 -> 52 us and 40 -> 22 us at 550k edges).
// - a bottom-up pass also counts the vertices it leaves unvisited that have
//   an allowed in-edge; when there is none, no later level can claim
//   anything and the loop ends without a pass that only finds that out.
// - dist is initialised by a 16-byte-store fill kernel that also zeroes the
//   counters.  abom_bfs_begin enqueues fill + seed without a sync, so a
//   caller that overlaps the BFS with other work can put the 4N-byte fill
//   ahead of that work instead of beside it.
//
// The host-side level loop is abom_bfs_run_indexed at the end of this file
// (abom_bfs_run_ex and abom_bfs_run are that loop without an index; C++,
// one sync per level, counts read into pinned host memory when the caller
// passes some; the degree sum of the sources is read only when the caller
// does not know it).

#include "abom_api.h"
#include "abom_wave.h"

namespace abom {

// Slots of the device counter array shared by the kernels and the level loop
// (mirrored in ops/native.py).
// CTR_OPEN: vertices a bottom-up pass left unvisited that have an allowed
// in-edge (zero => the BFS is over).
enum { CTR_NEXT = 0, CTR_HEAVY = 1, CTR_DEGREE = 2, CTR_OPEN = 3, CTR_SLOTS = 4 };

// Entries of the per-block LDS claim queue of bfs_expand_kernel and
// bfs_expand_heavy_kernel (16 KiB).
constexpr unsigned BFS_STAGE = 4096;

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

// claim_and_append with the append staged (stage_push): only a claim that
// finds the LDS queue full pays the global atomic.
__device__ __forceinline__ unsigned claim_and_stage(
    uint32_t v, uint32_t level, uint32_t* __restrict__ dist,
    const uint64_t* __restrict__ row_off, BlockStage<BFS_STAGE>& st,
    uint32_t* __restrict__ next_frontier, unsigned int* __restrict__ next_count,
    long long capacity) {
    if (dist[v] != ABOM_UNVISITED ||
        atomicCAS(&dist[v], ABOM_UNVISITED, level) != ABOM_UNVISITED)
        return 0;
    stage_push(v, st, next_frontier, next_count, capacity);
    return (unsigned)(row_off[v + 1] - row_off[v]);
}

// Pass over the frontier: expand vertices with degree < WAVE_DEG inline;
// defer heavy vertices to the heavy queue.  Claims are staged in the LDS
// queue and flushed at the end of each grid-stride round; the round count is
// block-uniform (from frontier_size), so the barriers are legal.
__global__ __launch_bounds__(256) void bfs_expand_kernel(
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
    __shared__ BlockStage<BFS_STAGE> st;
    __shared__ unsigned block_deg;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long rounds = (frontier_size + stride - 1) / stride;
    if (threadIdx.x == 0) block_deg = 0;
    unsigned my_deg = 0;
    for (long long r = 0; r < rounds; ++r) {
        if (threadIdx.x == 0) st.n = 0;
        __syncthreads();
        const long long i = r * stride + (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (i < frontier_size) {
            const uint32_t u = frontier[i];
            const uint64_t beg = row_off[u];
            const uint64_t end = row_off[u + 1];
            if (end - beg >= WAVE_DEG) {
                heavy_queue[atomicAdd(heavy_count, 1u)] = u;
            } else {
                for (uint64_t e = beg; e < end; ++e) {
                    if (edge_filtered(etype, allowed_mask, e)) continue;
                    my_deg += claim_and_stage(col[e], next_level, dist, row_off, st,
                                              next_frontier, next_count, capacity);
                }
            }
        }
        stage_flush(st, next_frontier, next_count, capacity);
    }
    // degree sum: wave reduce, one LDS atomic per wave, one global per block
    my_deg = wave_sum(my_deg);
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && my_deg) atomicAdd(&block_deg, my_deg);
    __syncthreads();
    if (threadIdx.x == 0 && block_deg) atomicAdd(next_degree_sum, block_deg);
}

// Wave-cooperative expansion of heavy vertices: one wave (64 lanes) walks one
// vertex's adjacency with coalesced col[] reads.  The block's claims share
// one LDS queue, flushed once when all its waves are done.
__global__ __launch_bounds__(256) void bfs_expand_heavy_kernel(
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
    __shared__ BlockStage<BFS_STAGE> st;
    const unsigned heavy_size = *heavy_size_ptr;
    // the block's first wave id: no wave of the block has work past the queue
    if (((long long)blockIdx.x * blockDim.x >> 6) >= heavy_size) return;
    const WaveId w = wave_id(blockDim.x >> 6);
    if (threadIdx.x == 0) st.n = 0;
    __syncthreads();
    unsigned my_deg = 0;
    for (long long q = w.wave; q < heavy_size; q += w.n_waves) {
        const uint32_t u = heavy_queue[q];
        const uint64_t beg = row_off[u];
        const uint64_t end = row_off[u + 1];
        for (uint64_t e = beg + w.lane; e < end; e += 64) {
            if (edge_filtered(etype, allowed_mask, e)) continue;
            my_deg += claim_and_stage(col[e], next_level, dist, row_off, st, next_frontier,
                                      next_count, capacity);
        }
    }
    stage_flush(st, next_frontier, next_count, capacity);
    wave_add(next_degree_sum, my_deg);
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
    wave_add(next_degree_sum, my_deg);
    if (!build_frontier) wave_add(next_count, my_claims);
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
    unsigned int* __restrict__ next_count,
    unsigned int* __restrict__ open_count) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned my_claims = 0;
    unsigned my_open = 0;  // left unvisited, yet with an allowed in-edge
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < num_nodes;
         v += stride) {
        if (dist[v] != ABOM_UNVISITED) continue;
        const uint64_t beg = rev_off[v];
        const uint64_t end = rev_off[v + 1];
        bool allowed_edge = false, claimed = false;
        for (uint64_t e = beg; e < end; ++e) {
            if (edge_filtered(rev_et, allowed_mask, e)) continue;
            allowed_edge = true;
            if (dist[rev_col[e]] == cur_level) {
                dist[v] = cur_level + 1;
                claimed = true;
                break;
            }
        }
        my_claims += claimed;
        my_open += allowed_edge && !claimed;
    }
    wave_add(next_count, my_claims);
    wave_add(open_count, my_open);
}

// The parent index of the bottom-up pass: which vertex has which allowed
// parent is a property of the reverse CSR and the edge mask, not of a
// traversal.  first_parent[v] = PARENT_NONE when v has no allowed in-edge;
// else bits 0-30 = the source of the first allowed in-edge in reverse-row
// order, PARENT_MORE set when the row holds a second allowed in-edge (from
// the same parent or another).
constexpr uint32_t PARENT_NONE = 0xFFFFFFFFu;
constexpr uint32_t PARENT_MORE = 0x80000000u;

__global__ void bfs_parent_index_kernel(
    const uint64_t* __restrict__ rev_off,
    const uint32_t* __restrict__ rev_col,
    const uint8_t* __restrict__ rev_et,
    uint32_t allowed_mask,
    long long num_nodes,
    uint32_t* __restrict__ first_parent) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < num_nodes;
         v += stride) {
        const uint64_t end = rev_off[v + 1];
        uint32_t entry = PARENT_NONE;
        for (uint64_t e = rev_off[v]; e < end; ++e) {
            if (edge_filtered(rev_et, allowed_mask, e)) continue;
            if (entry != PARENT_NONE) {
                entry |= PARENT_MORE;
                break;
            }
            entry = rev_col[e];
        }
        first_parent[v] = entry;
    }
}

// One vertex of the indexed bottom-up pass, after its first parent missed:
// walk the reverse row with the mask, as bfs_bottom_up_kernel does.
__device__ __forceinline__ bool bottom_up_walk_row(
    long long v, const uint64_t* __restrict__ rev_off, const uint32_t* __restrict__ rev_col,
    const uint8_t* __restrict__ rev_et, uint32_t allowed_mask,
    const uint32_t* dist, uint32_t cur_level) {
    const uint64_t end = rev_off[v + 1];
    for (uint64_t e = rev_off[v]; e < end; ++e) {
        if (edge_filtered(rev_et, allowed_mask, e)) continue;
        if (dist[rev_col[e]] == cur_level) return true;
    }
    return false;
}

// A single vertex of the indexed pass: the words of dist before and after
// its 16-byte body; counts like the body does.
__device__ __forceinline__ void bottom_up_indexed_one(
    long long v, const uint32_t* __restrict__ first_parent,
    const uint64_t* __restrict__ rev_off, const uint32_t* __restrict__ rev_col,
    const uint8_t* __restrict__ rev_et, uint32_t allowed_mask,
    uint32_t* dist, uint32_t cur_level, unsigned& claims, unsigned& open) {
    const uint32_t d = dist[v];
    const uint32_t fp = first_parent[v];
    if (d != ABOM_UNVISITED || fp == PARENT_NONE) return;
    bool hit = dist[fp & ~PARENT_MORE] == cur_level;
    if (!hit && (fp & PARENT_MORE))
        hit = bottom_up_walk_row(v, rev_off, rev_col, rev_et, allowed_mask, dist, cur_level);
    if (hit) dist[v] = cur_level + 1;
    claims += hit;
    open += !hit;
}

// The bottom-up pass over the parent index.  A thread takes four consecutive
// vertices of the 16-byte-aligned body of dist (`head` words come before it,
// `n4` uint4 make it up, as in bfs_fill_kernel): it loads their dist and
// first_parent words together, then gathers the four dist[parent] together,
// then stores the four words back at once when it claimed any.  Only the
// thread of v writes dist[v], so writing back an unclaimed word as read is
// exact.  A vertex that needs no gather reads its own dist word in its place.
// The reverse row is walked only when the first parent missed and the entry
// says there is another allowed in-edge.  `fp_vec`: first_parent + head is
// 16-byte aligned too.
__global__ __launch_bounds__(256) void bfs_bottom_up_indexed_kernel(
    const uint32_t* __restrict__ first_parent,
    const uint64_t* __restrict__ rev_off,
    const uint32_t* __restrict__ rev_col,
    const uint8_t* __restrict__ rev_et,
    uint32_t allowed_mask,
    long long num_nodes, long long head, long long n4, int fp_vec,
    uint32_t* dist,  // read at the parents, written at the thread's own vertices
    uint32_t cur_level,
    unsigned int* __restrict__ next_count,
    unsigned int* __restrict__ open_count) {
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned my_claims = 0;
    unsigned my_open = 0;  // left unvisited, yet with an index entry
    uint4* body = reinterpret_cast<uint4*>(dist + head);
    const uint32_t* __restrict__ fp_body = first_parent + head;
    for (long long i = tid; i < n4; i += stride) {
        const long long v0 = head + 4 * i;
        const uint4 d4 = body[i];
        uint4 f4;
        if (fp_vec) {
            f4 = reinterpret_cast<const uint4*>(fp_body)[i];
        } else {
            f4 = make_uint4(fp_body[4 * i], fp_body[4 * i + 1], fp_body[4 * i + 2],
                            fp_body[4 * i + 3]);
        }
        uint32_t d[4] = {d4.x, d4.y, d4.z, d4.w};
        const uint32_t f[4] = {f4.x, f4.y, f4.z, f4.w};
        bool want[4];
        uint32_t g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // & not &&: no branch between the loads
            want[k] = (d[k] == ABOM_UNVISITED) & (f[k] != PARENT_NONE);
            g[k] = dist[want[k] ? (long long)(f[k] & ~PARENT_MORE) : v0 + k];
        }
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!want[k]) continue;
            bool hit = g[k] == cur_level;
            if (!hit && (f[k] & PARENT_MORE))
                hit = bottom_up_walk_row(v0 + k, rev_off, rev_col, rev_et, allowed_mask, dist,
                                         cur_level);
            if (hit) d[k] = cur_level + 1;
            any |= hit;
            my_claims += hit;
            my_open += !hit;
        }
        if (any) body[i] = make_uint4(d[0], d[1], d[2], d[3]);
    }
    const long long tail = head + 4 * n4;  // first vertex after the body
    if (tid < head)
        bottom_up_indexed_one(tid, first_parent, rev_off, rev_col, rev_et, allowed_mask, dist,
                              cur_level, my_claims, my_open);
    if (tid < num_nodes - tail)
        bottom_up_indexed_one(tail + tid, first_parent, rev_off, rev_col, rev_et, allowed_mask,
                              dist, cur_level, my_claims, my_open);
    wave_add(next_count, my_claims);
    wave_add(open_count, my_open);
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
    wave_add(degree_sum, my_deg);
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
    wave_add(degree_sum, my_deg);
}

// dist[0..n) = UNVISITED with 16-byte stores, counters = 0.  `head` elements
// come before the first 16-byte boundary of dist and `n4` whole uint4 follow
// it; the elements before and after those go out as single words.
__global__ void bfs_fill_kernel(uint32_t* __restrict__ dist, long long n, long long head,
                                long long n4, unsigned int* __restrict__ counters) {
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    uint4* __restrict__ body = reinterpret_cast<uint4*>(dist + head);
    const uint4 fill = make_uint4(ABOM_UNVISITED, ABOM_UNVISITED, ABOM_UNVISITED,
                                  ABOM_UNVISITED);
    for (long long i = tid; i < n4; i += stride) body[i] = fill;
    const long long tail = head + 4 * n4;  // first element after the body
    if (tid < head) dist[tid] = ABOM_UNVISITED;
    if (tid < n - tail) dist[tail + tid] = ABOM_UNVISITED;
    if (tid < CTR_SLOTS) counters[tid] = 0;
}

// ── Host helpers of the level loop ─────────────────────────────────────────

// Fill dist and zero the counters in one launch.  The fill used to be a
// hipMemsetAsync, which the runtime ran as a 256-block kernel at 3 % of the
// achievable store bandwidth beside the match kernel.
static int bfs_init(void* dist, long long n, unsigned int* ctr, hipStream_t s) {
    long long head = (long long)(((16 - ((uintptr_t)dist & 15)) & 15) / sizeof(uint32_t));
    if (head > n) head = n;
    const long long n4 = (n - head) / 4;
    const int block = 256;
    // head, tail and counters take at most CTR_SLOTS threads: one block has them
    hipLaunchKernelGGL(bfs_fill_kernel, dim3(grid_for(n4, block)), dim3(block), 0, s,
                       (uint32_t*)dist, n, head, n4, ctr);
    return (int)hipGetLastError();
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

// One bottom-up level: over the parent index when the caller has one, else
// over the reverse rows.
static int bottom_up_level(const void* rev_off, const void* rev_col, const void* rev_et,
                           unsigned int allowed_mask, long long num_nodes, void* dist,
                           unsigned int cur_level, const void* first_parent,
                           unsigned int* next_count, unsigned int* open_count, hipStream_t s) {
    const int block = 256;
    if (first_parent) {
        // the 16-byte body of dist, as bfs_init lays it out
        long long head = (long long)(((16 - ((uintptr_t)dist & 15)) & 15) / sizeof(uint32_t));
        if (head > num_nodes) head = num_nodes;
        const long long n4 = (num_nodes - head) / 4;
        const int fp_vec = (((uintptr_t)first_parent + head * sizeof(uint32_t)) & 15) == 0;
        hipLaunchKernelGGL(bfs_bottom_up_indexed_kernel, dim3(grid_for(n4, block)), dim3(block),
                           0, s, (const uint32_t*)first_parent, (const uint64_t*)rev_off,
                           (const uint32_t*)rev_col, (const uint8_t*)rev_et, allowed_mask,
                           num_nodes, head, n4, fp_vec, (uint32_t*)dist, cur_level, next_count,
                           open_count);
    } else {
        hipLaunchKernelGGL(bfs_bottom_up_kernel, dim3(grid_for(num_nodes, block)), dim3(block),
                           0, s, (const uint64_t*)rev_off, (const uint32_t*)rev_col,
                           (const uint8_t*)rev_et, allowed_mask, num_nodes, (uint32_t*)dist,
                           cur_level, next_count, open_count);
    }
    return (int)hipGetLastError();
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

// first_parent u32 [num_nodes] of (reverse CSR, allowed_mask): see
// bfs_parent_index_kernel.  num_nodes must stay below 2^31 - 1, so that a
// vertex id fits bits 0-30 and never reads as "none".
extern "C" int abom_bfs_parent_index(
    const void* rev_off, const void* rev_col, const void* rev_et, unsigned int allowed_mask,
    long long num_nodes, void* first_parent, void* stream) {
    if (num_nodes < 0 || num_nodes >= 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
    const int block = 256;
    hipLaunchKernelGGL(abom::bfs_parent_index_kernel, dim3(abom::grid_for(num_nodes, block)),
                       dim3(block), 0, (hipStream_t)stream, (const uint64_t*)rev_off,
                       (const uint32_t*)rev_col, (const uint8_t*)rev_et, allowed_mask, num_nodes,
                       (uint32_t*)first_parent);
    return (int)hipGetLastError();
}

// One bottom-up pass: every unvisited vertex with a parent at cur_level gets
// cur_level + 1; *next_count += the claims, *open_count += the vertices left
// unvisited that have an allowed in-edge.
extern "C" int abom_bfs_bottom_up(
    const void* rev_off, const void* rev_col, const void* rev_et, unsigned int allowed_mask,
    long long num_nodes, void* dist, unsigned int cur_level,
    void* next_count, void* open_count, void* stream) {
    return abom::bottom_up_level(rev_off, rev_col, rev_et, allowed_mask, num_nodes, dist,
                                 cur_level, nullptr, (unsigned int*)next_count,
                                 (unsigned int*)open_count, (hipStream_t)stream);
}

// The same pass over the parent index of (rev, allowed_mask).
extern "C" int abom_bfs_bottom_up_indexed(
    const void* rev_off, const void* rev_col, const void* rev_et, unsigned int allowed_mask,
    long long num_nodes, void* dist, unsigned int cur_level, const void* first_parent,
    void* next_count, void* open_count, void* stream) {
    if (!first_parent) return (int)hipErrorInvalidValue;
    return abom::bottom_up_level(rev_off, rev_col, rev_et, allowed_mask, num_nodes, dist,
                                 cur_level, first_parent, (unsigned int*)next_count,
                                 (unsigned int*)open_count, (hipStream_t)stream);
}

// ── C ABI: the level loop ──────────────────────────────────────────────────

// First part of a BFS, enqueued without a sync: dist = UNVISITED, counters
// = 0, sources seeded into frontier_a (their degree sum lands in the
// counters).  abom_bfs_run_ex(..., begun = 1, ...) on the same buffers and
// stream runs the levels.
extern "C" int abom_bfs_begin(
    const void* row_off, const void* sources, long long n_sources, void* dist,
    long long num_nodes, void* frontier_a, void* counters, void* stream) {
    using namespace abom;
    hipStream_t s = (hipStream_t)stream;
    unsigned int* ctr = (unsigned int*)counters;
    int rc = bfs_init(dist, num_nodes, ctr, s);
    if (rc) return rc;
    return bfs_seed(sources, n_sources, row_off, dist, frontier_a, ctr + CTR_DEGREE, s);
}

// Full multi-source BFS: host-side level loop, one device->host count read
// per level.  dist must be u32[N]; frontier_a/b u32[N]; heavy_queue u32[N];
// counters = device u32[CTR_SLOTS].  ``edge_src`` (the per-edge source
// array, col-aligned) may be null; when present, levels whose frontier would
// touch > ~1/8 of all edges go dense: bottom-up over the reverse CSR when
// rev_off/rev_col are given, else the edge-centric kernel (coalesced
// streams), instead of per-vertex expansion.  A bottom-up level that leaves
// no unvisited vertex with an allowed in-edge ends the loop.
// ``begun`` != 0: abom_bfs_begin has been enqueued on this stream.
// ``sources_degree``: the degree sum of the sources (duplicates counted), or
// -1 to read it from the device.  ``host_counters``: pinned host u32
// [CTR_SLOTS] for the count reads, or null to read into the stack.
// Returns negative hip error or the number of levels run.
// ``first_parent``: the parent index of (rev, allowed_mask) from
// abom_bfs_parent_index, or null; with it the bottom-up levels run
// bfs_bottom_up_indexed_kernel.
extern "C" int abom_bfs_run_indexed(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* sources, long long n_sources, void* dist, long long num_nodes,
    void* frontier_a, void* frontier_b, void* heavy_queue, void* counters,
    int max_levels, const void* edge_src, long long num_edges,
    const void* rev_off, const void* rev_col, const void* rev_et, const void* first_parent,
    int begun, long long sources_degree, void* host_counters, void* stream) {
    using namespace abom;
    hipStream_t s = (hipStream_t)stream;
    unsigned int* ctr = (unsigned int*)counters;
    unsigned int stack_ctr[CTR_SLOTS] = {0, 0, 0, 0};
    unsigned int* host_ctr = host_counters ? (unsigned int*)host_counters : stack_ctr;
    int rc;
    if (!begun) {
        rc = abom_bfs_begin(row_off, sources, n_sources, dist, num_nodes, frontier_a, counters,
                            stream);
        if (rc) return -rc;
    }
    unsigned int frontier_degree = 0;
    if (sources_degree < 0) {
        if ((rc = read_counters(host_ctr, ctr + CTR_DEGREE, 1, s))) return -rc;
        frontier_degree = host_ctr[0];
    } else {
        frontier_degree = sources_degree > 0xFFFFFFFFll ? 0xFFFFFFFFu
                                                        : (unsigned int)sources_degree;
    }

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
        const bool bottom_up = dense && rev_off && rev_col;
        if (dense) {
            stay_dense = true;
            if (bottom_up) {
                rc = bottom_up_level(rev_off, rev_col, rev_et, allowed_mask, num_nodes, dist,
                                     (unsigned int)(level - 1), first_parent, ctr + CTR_NEXT,
                                     ctr + CTR_OPEN, s);
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
                if ((rc = read_counters(host_ctr, ctr + CTR_NEXT, 1, s))) return -rc;
                frontier_size = host_ctr[0];
                // reset all counters: the rebuilt frontier's degree sum is
                // the CURRENT level's, while the dense decision needs the
                // NEXT frontier's (accumulated by the expand below)
                if ((rc = reset_counters(ctr, s))) return -rc;
            }
            rc = expand_level(row_off, col, etype, allowed_mask, cur, frontier_size, dist,
                              (unsigned int)level, nxt, ctr, heavy_queue, num_nodes, stream);
            if (rc) return -rc;
        }
        if ((rc = read_counters(host_ctr, ctr, CTR_SLOTS, s))) return -rc;
        frontier_size = host_ctr[CTR_NEXT];
        frontier_degree = host_ctr[CTR_DEGREE];
        // a claim needs an unvisited vertex with an allowed in-edge: when the
        // bottom-up pass left none, every later level would claim nothing
        if (bottom_up && host_ctr[CTR_OPEN] == 0) frontier_size = 0;
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

// The level loop without a parent index.
extern "C" int abom_bfs_run_ex(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* sources, long long n_sources, void* dist, long long num_nodes,
    void* frontier_a, void* frontier_b, void* heavy_queue, void* counters,
    int max_levels, const void* edge_src, long long num_edges,
    const void* rev_off, const void* rev_col, const void* rev_et,
    int begun, long long sources_degree, void* host_counters, void* stream) {
    return abom_bfs_run_indexed(row_off, col, etype, allowed_mask, sources, n_sources, dist,
                                num_nodes, frontier_a, frontier_b, heavy_queue, counters,
                                max_levels, edge_src, num_edges, rev_off, rev_col, rev_et,
                                /*first_parent=*/nullptr, begun, sources_degree, host_counters,
                                stream);
}

// The one-shot form of ABI v1: begin + levels, degree sum read from the device.
extern "C" int abom_bfs_run(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* sources, long long n_sources, void* dist, long long num_nodes,
    void* frontier_a, void* frontier_b, void* heavy_queue, void* counters,
    int max_levels, const void* edge_src, long long num_edges, double avg_degree,
    const void* rev_off, const void* rev_col, const void* rev_et,
    void* stream) {
    (void)avg_degree;  // part of ABI v1; the mode switches use exact degree sums
    return abom_bfs_run_ex(row_off, col, etype, allowed_mask, sources, n_sources, dist, num_nodes,
                           frontier_a, frontier_b, heavy_queue, counters, max_levels, edge_src,
                           num_edges, rev_off, rev_col, rev_et, /*begun=*/0,
                           /*sources_degree=*/-1, /*host_counters=*/nullptr, stream);
}
