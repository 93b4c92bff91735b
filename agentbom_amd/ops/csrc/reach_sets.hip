// Per-source dependency reach: bit-parallel multi-source BFS over the forward
// CSR.  Where bfs.hip keeps one dist label per node ("some source reaches v at
// hop d"), this keeps one BIT per (node, source), 64 sources to a 64-bit word,
// so every source of a pass shares one walk of the adjacency and the result
// says which source reaches which target in how many hops.
//
// State per (node, word), W words of 64 sources per node, entry e = v*W + k:
//   seen[e]  sources that have reached v at an earlier level
//   cur[e]   sources whose frontier holds v at this level
//   nxt[e]   sources that reach v at the next level, ORed in by the expand
// The frontier is a queue of entries e; no kernel scans all N nodes.
//
// One level is two phases:
// - expand (reach_expand_kernel, one lane per queue entry; rows of degree >=
//   REACH_HEAVY_DEG go to reach_expand_heavy_kernel, one wave per entry):
//   bits = cur[e], cur[e] = 0; for each allowed edge v->w,
//   nb = bits & ~seen[w*W+k]; if nb, old = atomicOr(&nxt[w*W+k], nb), and the
//   lane that saw old == 0 appends the entry to the next queue.  seen is
//   read-only here, nxt[e] is zero between levels, so an entry is appended
//   exactly once per level.  Appends are staged in a per-block LDS queue and
//   reserved with one atomic per flush, as in bfs.hip.
// - commit (reach_commit_kernel, one lane per entry of the next queue):
//   fresh = nxt[e] & ~seen[e]; seen[e] |= fresh; cur[e] = fresh; nxt[e] = 0;
//   when v is a target, hops[slot, column of bit b] = level for every bit b of
//   fresh.  A (target, source) cell is written at most once, by one lane, so
//   the output does not depend on the order of the queue.
// Seeding ORs each source's bit into nxt and queues the entry; the commit of
// level 0 then does the rest.  A commit at level == max_depth leaves cur
// alone (that frontier is recorded but not expanded), so cur and nxt are
// all-zero again when the call returns; seen is cleared at the start.
//
// The host level loop is abom_reach_hops at the end of this file: one sync
// per level, the frontier count read through pinned host memory.

#include "abom_api.h"
#include "abom_wave.h"

namespace abom {

enum { RCTR_NEXT = 0, RCTR_HEAVY = 1, RCTR_SLOTS = 2 };

// Rows with at least this many edges are expanded by a whole wave.  A lane
// that walks a row alone pays a returning 64-bit atomic per edge, one after
// the other, so the threshold is lower than the 64 of bfs.hip's heavy queue:
// at 16 the estate's ~30-edge server rows go to a wave and a pass is 21-23 %
// shorter than at 64 (profiles/reach_sets.md; -DABOM_REACH_HEAVY_DEG=...
// builds an A/B variant).
#ifndef ABOM_REACH_HEAVY_DEG
#define ABOM_REACH_HEAVY_DEG 16
#endif
constexpr uint64_t REACH_HEAVY_DEG = ABOM_REACH_HEAVY_DEG;
// Entries of the per-block LDS append queue (16 KiB).
constexpr unsigned REACH_STAGE = 4096;

// Offer `bits` of word k to neighbour w.
__device__ __forceinline__ void reach_offer(
    uint32_t w, uint32_t k, uint32_t W, uint64_t bits,
    const uint64_t* __restrict__ seen, uint64_t* __restrict__ nxt,
    BlockStage<REACH_STAGE>& st, uint32_t* __restrict__ next_queue,
    unsigned int* __restrict__ next_count, long long capacity) {
    const uint32_t idx = w * W + k;
    const uint64_t nb = bits & ~seen[idx];
    if (!nb) return;
    const uint64_t old = atomicOr((unsigned long long*)&nxt[idx], (unsigned long long)nb);
    if (old == 0) stage_push(idx, st, next_queue, next_count, capacity);
}

// nxt[s*W + j/64] |= 1 << (j%64) for source j of the pass; the lane that set
// the entry's first bit queues it.  Sources outside [0, N) are skipped.
__global__ void reach_seed_kernel(
    const uint32_t* __restrict__ sources, int n_sources, uint32_t W, long long num_nodes,
    uint64_t* __restrict__ nxt, uint32_t* __restrict__ queue,
    unsigned int* __restrict__ count, long long capacity) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_sources) return;
    const uint32_t s = sources[j];
    if ((long long)s >= num_nodes) return;
    const uint32_t idx = s * W + (uint32_t)(j >> 6);
    const uint64_t bit = 1ull << (j & 63);
    const uint64_t old = atomicOr((unsigned long long*)&nxt[idx], (unsigned long long)bit);
    if (old == 0) {
        const unsigned slot = atomicAdd(count, 1u);
        if ((long long)slot < capacity) queue[slot] = idx;
    }
}

// The round count is block-uniform (from queue_size), so the barriers of the
// flush are legal.
__global__ __launch_bounds__(256) void reach_expand_kernel(
    const uint64_t* __restrict__ row_off, const uint32_t* __restrict__ col,
    const uint8_t* __restrict__ etype, uint32_t allowed_mask, uint32_t W,
    const uint32_t* __restrict__ queue, long long queue_size,
    const uint64_t* __restrict__ seen, uint64_t* __restrict__ cur, uint64_t* __restrict__ nxt,
    uint32_t* __restrict__ next_queue, unsigned int* __restrict__ next_count,
    uint32_t* __restrict__ heavy_queue, unsigned int* __restrict__ heavy_count,
    long long capacity) {
    __shared__ BlockStage<REACH_STAGE> st;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long rounds = (queue_size + stride - 1) / stride;
    for (long long r = 0; r < rounds; ++r) {
        if (threadIdx.x == 0) st.n = 0;
        __syncthreads();
        const long long i = r * stride + (long long)blockIdx.x * blockDim.x + threadIdx.x;
        if (i < queue_size) {
            const uint32_t e = queue[i];
            const uint32_t v = e / W;
            const uint32_t k = e - v * W;
            const uint64_t beg = row_off[v];
            const uint64_t end = row_off[v + 1];
            if (end - beg >= REACH_HEAVY_DEG) {
                // cur[e] stays for the wave that expands the row
                const unsigned slot = atomicAdd(heavy_count, 1u);
                if ((long long)slot < capacity) heavy_queue[slot] = e;
            } else {
                const uint64_t bits = cur[e];
                cur[e] = 0;
                for (uint64_t x = beg; x < end; ++x) {
                    if (edge_filtered(etype, allowed_mask, x)) continue;
                    reach_offer(col[x], k, W, bits, seen, nxt, st, next_queue, next_count,
                                capacity);
                }
            }
        }
        stage_flush(st, next_queue, next_count, capacity);
    }
}

// One wave per heavy entry: the lanes share the entry's bits and stride over
// its row with coalesced col[] reads.
__global__ __launch_bounds__(256) void reach_expand_heavy_kernel(
    const uint64_t* __restrict__ row_off, const uint32_t* __restrict__ col,
    const uint8_t* __restrict__ etype, uint32_t allowed_mask, uint32_t W,
    const uint32_t* __restrict__ heavy_queue, const unsigned int* __restrict__ heavy_size_ptr,
    const uint64_t* __restrict__ seen, uint64_t* __restrict__ cur, uint64_t* __restrict__ nxt,
    uint32_t* __restrict__ next_queue, unsigned int* __restrict__ next_count,
    long long capacity) {
    __shared__ BlockStage<REACH_STAGE> st;
    long long heavy_size = *heavy_size_ptr;
    if (heavy_size > capacity) heavy_size = capacity;
    const WaveId w = wave_id(blockDim.x >> 6);
    // the block's first wave id: no wave of the block has work past the queue
    if (((long long)blockIdx.x * blockDim.x >> 6) >= heavy_size) return;
    if (threadIdx.x == 0) st.n = 0;
    __syncthreads();
    for (long long q = w.wave; q < heavy_size; q += w.n_waves) {
        const uint32_t e = heavy_queue[q];
        const uint32_t v = e / W;
        const uint32_t k = e - v * W;
        const uint64_t bits = cur[e];
        if (w.lane == 0) cur[e] = 0;
        const uint64_t beg = row_off[v];
        const uint64_t end = row_off[v + 1];
        for (uint64_t x = beg + w.lane; x < end; x += 64) {
            if (edge_filtered(etype, allowed_mask, x)) continue;
            reach_offer(col[x], k, W, bits, seen, nxt, st, next_queue, next_count, capacity);
        }
    }
    stage_flush(st, next_queue, next_count, capacity);
}

// The queue size is read from the device, so the launch need not wait for the
// host to learn it.  hops is row-major [T, hops_stride]; bit b of word k is
// column col_base + 64k + b.
__global__ void reach_commit_kernel(
    const uint32_t* __restrict__ queue, const unsigned int* __restrict__ queue_size_ptr,
    long long capacity, uint32_t W,
    uint64_t* __restrict__ seen, uint64_t* __restrict__ cur, uint64_t* __restrict__ nxt,
    const int32_t* __restrict__ target_slot, uint8_t* __restrict__ hops,
    long long hops_stride, long long col_base, uint32_t level, int keep_cur) {
    long long n = *queue_size_ptr;
    if (n > capacity) n = capacity;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t e = queue[i];
        const uint64_t old_seen = seen[e];
        uint64_t fresh = nxt[e] & ~old_seen;
        nxt[e] = 0;
        seen[e] = old_seen | fresh;
        if (keep_cur) cur[e] = fresh;
        const uint32_t v = e / W;
        const int32_t slot = target_slot[v];
        if (slot < 0) continue;
        uint8_t* __restrict__ row = hops + (long long)slot * hops_stride + col_base +
                                    64ll * (e - v * W);
        while (fresh) {
            const int b = __ffsll((unsigned long long)fresh) - 1;
            row[b] = (uint8_t)level;
            fresh &= fresh - 1;
        }
    }
}

}  // namespace abom

// One pass of per-source reach: n_sources <= 64 * words sources (int32 node
// ids, duplicates allowed) walk the CSR together for at most max_depth levels
// (clamped to [0, 254]; a node at distance max_depth is recorded, not
// expanded).  hops[target_slot[v], col_base + j] = distance from sources[j]
// to v for every target v that source reaches; the other cells are not
// touched (the caller fills hops with 255).  seen, cur, nxt: u64 [N * words]
// (cur and nxt all-zero on entry and again on return; seen is cleared here);
// queue_a, queue_b, heavy_queue: u32 [N * words]; counters: device u32 [2];
// host_counters: pinned host u32 [2], or null to read into the stack.
// Returns the number of levels expanded or a negated hipError_t.
extern "C" int abom_reach_hops(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* sources, int n_sources, int words, long long num_nodes,
    const void* target_slot, void* hops, long long hops_stride, long long col_base,
    int max_depth,
    void* seen, void* cur, void* nxt, void* queue_a, void* queue_b, void* heavy_queue,
    void* counters, void* host_counters, void* stream) {
    using namespace abom;
    hipStream_t s = (hipStream_t)stream;
    if (words < 1 || words > 4 || n_sources < 0 || n_sources > 64 * words || num_nodes < 0 ||
        num_nodes * words > 0xFFFFFFFFll || col_base < 0 ||
        col_base + n_sources > hops_stride)
        return -(int)hipErrorInvalidValue;
    if (n_sources == 0 || num_nodes == 0) return 0;
    if (max_depth < 0) max_depth = 0;
    if (max_depth > 254) max_depth = 254;
    const uint32_t W = (uint32_t)words;
    const long long capacity = num_nodes * words;
    unsigned int* ctr = (unsigned int*)counters;
    unsigned int stack_ctr[RCTR_SLOTS] = {0, 0};
    unsigned int* host_ctr = host_counters ? (unsigned int*)host_counters : stack_ctr;
    uint32_t* curq = (uint32_t*)queue_a;
    uint32_t* nxtq = (uint32_t*)queue_b;
    const int block = 256;
    hipError_t rc;

    auto fail = [](hipError_t e) { return -(int)e; };
    auto commit = [&](const uint32_t* queue, long long at_most, int level) {
        hipLaunchKernelGGL(reach_commit_kernel, dim3(grid_for(at_most, block)), dim3(block), 0, s,
                           queue, (const unsigned int*)(ctr + RCTR_NEXT), capacity, W,
                           (uint64_t*)seen, (uint64_t*)cur, (uint64_t*)nxt,
                           (const int32_t*)target_slot, (uint8_t*)hops, hops_stride, col_base,
                           (uint32_t)level, level < max_depth ? 1 : 0);
        return hipGetLastError();
    };
    // {next, heavy} -> host; the one sync point of a level
    auto read_counts = [&]() {
        hipError_t e = hipMemcpyAsync(host_ctr, ctr, RCTR_SLOTS * sizeof(unsigned int),
                                      hipMemcpyDeviceToHost, s);
        return e != hipSuccess ? e : hipStreamSynchronize(s);
    };

    if ((rc = hipMemsetAsync(seen, 0, (size_t)capacity * sizeof(uint64_t), s))) return fail(rc);
    if ((rc = hipMemsetAsync(ctr, 0, RCTR_SLOTS * sizeof(unsigned int), s))) return fail(rc);
    hipLaunchKernelGGL(reach_seed_kernel, dim3(grid_for(n_sources, block)), dim3(block), 0, s,
                       (const uint32_t*)sources, n_sources, W, num_nodes, (uint64_t*)nxt, curq,
                       ctr + RCTR_NEXT, capacity);
    if ((rc = hipGetLastError())) return fail(rc);
    if ((rc = commit(curq, n_sources, 0))) return fail(rc);
    if ((rc = read_counts())) return fail(rc);
    long long frontier = host_ctr[RCTR_NEXT];

    int level = 0;
    while (frontier > 0 && level < max_depth) {
        ++level;
        if (frontier > capacity) frontier = capacity;
        if ((rc = hipMemsetAsync(ctr, 0, RCTR_SLOTS * sizeof(unsigned int), s))) return fail(rc);
        hipLaunchKernelGGL(reach_expand_kernel, dim3(grid_for(frontier, block)), dim3(block), 0,
                           s, (const uint64_t*)row_off, (const uint32_t*)col,
                           (const uint8_t*)etype, allowed_mask, W, (const uint32_t*)curq,
                           frontier, (const uint64_t*)seen, (uint64_t*)cur, (uint64_t*)nxt, nxtq,
                           ctr + RCTR_NEXT, (uint32_t*)heavy_queue, ctr + RCTR_HEAVY, capacity);
        if ((rc = hipGetLastError())) return fail(rc);
        // at most one heavy entry per frontier entry, one wave each
        hipLaunchKernelGGL(reach_expand_heavy_kernel, dim3(grid_for(frontier * 64, block)),
                           dim3(block), 0, s, (const uint64_t*)row_off, (const uint32_t*)col,
                           (const uint8_t*)etype, allowed_mask, W,
                           (const uint32_t*)heavy_queue,
                           (const unsigned int*)(ctr + RCTR_HEAVY), (const uint64_t*)seen,
                           (uint64_t*)cur, (uint64_t*)nxt, nxtq, ctr + RCTR_NEXT, capacity);
        if ((rc = hipGetLastError())) return fail(rc);
        if ((rc = commit(nxtq, capacity, level))) return fail(rc);
        if ((rc = read_counts())) return fail(rc);
        frontier = host_ctr[RCTR_NEXT];
        uint32_t* t = curq; curq = nxtq; nxtq = t;
    }
    return level;
}
