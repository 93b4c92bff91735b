// Weakly connected components over an edge list, and the per-component
// roll-up: the kernels behind graph/backend.py::HipBackend.components and
// EstateEngine.components / lateral_domains.
//
// Labelling contract: on return labels[v] is the smallest node id of v's
// component (an isolated or fully masked node labels itself).  That fixed
// point is unique, so the result is bit-identical from run to run whatever
// the schedule.
//
// Algorithm: iterated rounds of min-label hooking on union-find parents.
// labels[] is the parent array.  One round is
//   hook      thread per edge (grid-stride): walk both endpoints to their
//             roots; if the roots differ, atomicMin(&parent[hi], lo) and raise
//             the round's flag;
//   compress  thread per node: pointer jumping until parent[v] is a root.
// The host loop (abom_components_run, at the end of this file) reads the flag
// once per round and stops after the first round that hooked nothing.
//
// Why this is correct, lost unions included.  Every store to parent[x] is
// either an atomicMin or a jump to an ancestor, and each writes a value
// that is <= the id of x and belongs to x's component, so
//   (a) parent[x] <= x always, with equality only at roots: no cycles, and
//       the root of a tree is its smallest member;
//   (b) a node that stopped being a root never becomes one again.
// A bare atomicMin(&parent[hi], lo) can hit a `hi` that another thread has
// just hooked elsewhere and overwrite that link: the union it carried is
// lost from the forest.  It is not lost from the input: no edge is ever
// retired.  Every round re-examines every edge, and the loop only stops
// after a round in which no edge found two different roots.  In that round
// nothing was stored by the hook kernel, so each walk read a static forest;
// both endpoints of every edge then share a root, hence every component has
// exactly one root, and by (a) it is the component's smallest id.  The loop
// does stop: a hooking round turns at least one root into a non-root (the
// `hi` of its first atomicMin was read as a root and is below itself
// afterwards), and by (b) that can happen at most N-1 times, so at most N
// rounds run, the confirming one included.  ops/native.py derives its
// default max_rounds from that bound.  No thread waits for another.
//
// Walks read parent[] with plain loads.  A stale value is an earlier parent
// of the same node, which by the invariants is still a smaller id of the
// same component; it can cost a step or a round, never an answer.
//
// abom_component_stats (per-component node-class counts, weight sums and
// worst severity) uses integer atomicAdd / atomicMin only, which commute:
// bit-reproducible as well.  Runs of adjacent lanes that share a component
// are folded inside the wave first, so one lane per run issues the atomics.

#include "abom_api.h"
#include "abom_common.h"

namespace abom {

constexpr int CC_BLOCK = 256;
// component_stats packs one 8-bit counter per node class into a 64-bit word
// (a wave holds at most 64 nodes of a class; mirrored in ops/native.py)
constexpr int CC_MAX_KINDS = 8;

__global__ __launch_bounds__(CC_BLOCK) void components_init_kernel(
    uint32_t* __restrict__ parent, long long num_nodes) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < num_nodes;
         v += stride)
        parent[v] = (uint32_t)v;
}

// Root of x in the current forest, halving the path on the way up.  The
// halving store is an atomicMin as well: parent[] only ever decreases.
__device__ __forceinline__ uint32_t components_find(uint32_t* parent, uint32_t x) {
    uint32_t p = parent[x];
    while (p != x) {
        const uint32_t gp = parent[p];
        if (gp != p) atomicMin(&parent[x], gp);
        x = p;
        p = gp;
    }
    return x;
}

__global__ __launch_bounds__(CC_BLOCK) void components_hook_kernel(
    const uint32_t* __restrict__ edge_src, const uint32_t* __restrict__ col,
    const uint8_t* __restrict__ etype, uint32_t allowed_mask, long long num_edges,
    uint32_t num_nodes, uint32_t* parent, unsigned int* __restrict__ hooked_flag) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    bool hooked = false;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < num_edges;
         e += stride) {
        if (edge_filtered(etype, allowed_mask, (uint64_t)e)) continue;
        const uint32_t u = edge_src[e];
        const uint32_t v = col[e];
        if (u == v || u >= num_nodes || v >= num_nodes) continue;  // ids outside [0, N) are skipped
        const uint32_t ru = components_find(parent, u);
        const uint32_t rv = components_find(parent, v);
        if (ru == rv) continue;
        atomicMin(&parent[ru > rv ? ru : rv], ru > rv ? rv : ru);
        hooked = true;
    }
    // all 64 lanes of every wave arrive here: one flag store per wave
    if (__ballot(hooked) != 0ull && (threadIdx.x & 63) == 0) atomicOr(hooked_flag, 1u);
}

// Pointer jumping until parent[v] is a root.  Every thread shortens its own
// pointer while it climbs, so the waves in flight double each other's reach.
__global__ __launch_bounds__(CC_BLOCK) void components_compress_kernel(
    uint32_t* parent, long long num_nodes) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < num_nodes;
         v += stride) {
        uint32_t p = parent[v];
        for (;;) {
            const uint32_t gp = parent[p];
            if (gp == p) break;
            parent[v] = gp;
            p = gp;
        }
    }
}

// Fold (packed class counters, weight, worst) over each run of adjacent
// lanes that share a component; the head lane of a run issues the atomics.
__global__ __launch_bounds__(CC_BLOCK) void component_stats_kernel(
    const uint32_t* __restrict__ comp, const uint8_t* __restrict__ kind,
    const int32_t* __restrict__ weight, const uint8_t* __restrict__ worst,
    long long num_nodes, uint32_t num_components, int num_kinds,
    unsigned int* __restrict__ kind_counts, unsigned long long* __restrict__ weight_sum,
    unsigned int* __restrict__ worst_min) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    // the loop bound is the wave's first index, so a wave stays whole
    for (long long base = (long long)blockIdx.x * blockDim.x + (threadIdx.x - lane);
         base < num_nodes; base += stride) {
        const long long v = base + lane;
        uint32_t c = 0xFFFFFFFFu;  // lanes past the end or with a bad index: no component
        if (v < num_nodes) c = comp[v];
        const bool valid = c < num_components;
        unsigned long long classes = 0;
        long long w = 0;
        uint32_t m = 0xFFFFFFFFu;
        if (valid) {
            const int k = kind[v];
            if (k < num_kinds) classes = 1ull << (8 * k);
            if (weight) w = weight[v];
            if (worst) m = worst[v];
        }
        const uint32_t prev = __shfl_up(c, 1, 64);
        const bool head = lane == 0 || prev != c;
        const unsigned long long heads = __ballot(head);
        // run id = number of heads at or below this lane
        const int run = __popcll(heads & (~0ull >> (63 - lane)));
        for (int off = 1; off < 64; off <<= 1) {
            const int o_run = __shfl_down(run, off, 64);
            const unsigned long long o_classes = __shfl_down(classes, off, 64);
            const long long o_w = __shfl_down(w, off, 64);
            const uint32_t o_m = __shfl_down(m, off, 64);
            if (lane + off < 64 && o_run == run) {
                classes += o_classes;
                w += o_w;
                m = o_m < m ? o_m : m;
            }
        }
        if (!head || !valid) continue;
        for (int k = 0; k < num_kinds; ++k) {
            const unsigned int cnt = (unsigned int)(classes >> (8 * k)) & 0xFFu;
            if (cnt) atomicAdd(&kind_counts[(size_t)c * num_kinds + k], cnt);
        }
        // two's complement: the unsigned add is the signed add
        if (weight && w) atomicAdd(&weight_sum[c], (unsigned long long)w);
        if (worst && m != 0xFFFFFFFFu) atomicMin(&worst_min[c], m);
    }
}

}  // namespace abom

// ── C ABI ──────────────────────────────────────────────────────────────────

// Component labels of the undirected graph of the unfiltered edges
// (edge_src[e], col[e]): labels is u32[N] and receives the smallest node id
// of each node's component.  Direction is ignored; self-loops, parallel
// edges and edges with an endpoint outside [0, N) change nothing.  counters
// is one device u32 (the round's hooked-anything flag).  Returns the number
// of rounds run, the last of which hooked nothing; max_rounds + 1 if
// max_rounds rounds ran and every one of them hooked (labels are then not
// final); 0 without launching the hook kernel when there are no nodes or no
// edges; or a negated hipError_t.
extern "C" int abom_components_run(
    const void* edge_src, const void* col, const void* etype, unsigned int allowed_mask,
    long long num_edges, long long num_nodes, void* labels, void* counters,
    int max_rounds, void* stream) {
    using namespace abom;
    if (num_nodes <= 0) return 0;
    if (num_nodes >= (1ll << 31)) return -(int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const int ngrid = grid_for(num_nodes, CC_BLOCK);
    uint32_t* parent = (uint32_t*)labels;
    unsigned int* flag = (unsigned int*)counters;
    int rc;

    hipLaunchKernelGGL(components_init_kernel, dim3(ngrid), dim3(CC_BLOCK), 0, s,
                       parent, num_nodes);
    if ((rc = (int)hipGetLastError())) return -rc;
    if (num_edges <= 0) return 0;

    const int egrid = grid_for(num_edges, CC_BLOCK);
    for (int round = 1; round <= max_rounds; ++round) {
        if ((rc = (int)hipMemsetAsync(flag, 0, sizeof(unsigned int), s))) return -rc;
        hipLaunchKernelGGL(components_hook_kernel, dim3(egrid), dim3(CC_BLOCK), 0, s,
                           (const uint32_t*)edge_src, (const uint32_t*)col,
                           (const uint8_t*)etype, allowed_mask, num_edges,
                           (uint32_t)num_nodes, parent, flag);
        if ((rc = (int)hipGetLastError())) return -rc;
        unsigned int hooked = 0;
        // the one sync point of a round
        if ((rc = (int)hipMemcpyAsync(&hooked, flag, sizeof(hooked), hipMemcpyDeviceToHost, s)))
            return -rc;
        if ((rc = (int)hipStreamSynchronize(s))) return -rc;
        if (!hooked) return round;  // parents untouched since the last compress
        hipLaunchKernelGGL(components_compress_kernel, dim3(ngrid), dim3(CC_BLOCK), 0, s,
                           parent, num_nodes);
        if ((rc = (int)hipGetLastError())) return -rc;
    }
    return max_rounds + 1;
}

// Per-component roll-up over N nodes: comp is u32[N] (dense component index,
// entries >= num_components are skipped), kind u8[N] (node class; values >=
// num_kinds are not counted), weight i32[N] and worst u8[N] are nullable.
// Adds into kind_counts u32[C * num_kinds] and weight_sum i64[C] and folds
// worst_min u32[C] with min: the caller zero-fills the first two and fills
// worst_min with 0xFFFFFFFF.  num_kinds is at most 8.
extern "C" int abom_component_stats(
    const void* comp, const void* kind, const void* weight, const void* worst,
    long long num_nodes, long long num_components, int num_kinds,
    void* kind_counts, void* weight_sum, void* worst_min, void* stream) {
    using namespace abom;
    if (num_kinds < 1 || num_kinds > CC_MAX_KINDS) return (int)hipErrorInvalidValue;
    if (num_components < 0 || num_components >= (1ll << 31)) return (int)hipErrorInvalidValue;
    if (num_nodes <= 0 || num_components == 0) return 0;
    hipLaunchKernelGGL(component_stats_kernel, dim3(grid_for(num_nodes, CC_BLOCK)),
                       dim3(CC_BLOCK), 0, (hipStream_t)stream,
                       (const uint32_t*)comp, (const uint8_t*)kind, (const int32_t*)weight,
                       (const uint8_t*)worst, num_nodes, (uint32_t)num_components, num_kinds,
                       (unsigned int*)kind_counts, (unsigned long long*)weight_sum,
                       (unsigned int*)worst_min);
    return (int)hipGetLastError();
}
