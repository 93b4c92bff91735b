// Graph centrality on the device-resident CSR: PageRank and Brandes
// betweenness (unweighted), the kernels behind graph/backend.py::HipBackend
// and EstateEngine.pagerank / betweenness / choke_points.
//
// Determinism contract: two runs on the same input give bit-identical
// outputs.  No floating-point atomic touches a value.  Both algorithms are
// PULLS over a CSR, so every output element has exactly one owner:
// - a row below CENTRALITY_HEAVY_DEGREE edges is owned by one thread, which
//   sums its edges in CSR order;
// - a row at or above it is owned by one wave: lane l sums edges l, l+64, ...
//   in CSR order, then a fixed shuffle tree folds the 64 lane sums
//   (the zipf hubs of an estate: same split as bfs_expand_heavy_kernel);
// - sums across blocks (PageRank's L1 change and dangling mass) go through
//   per-block partials that one wave folds in index order.
// The heavy rows arrive as a precomputed id list (ops/native.py builds it
// once per call), so the heavy kernels touch only those rows.
// All accumulation is fp64.  The only atomics are the integer discovery
// counters of the Brandes forward pass, one per wave.
//
// Per-source Brandes arrays are [B][N] (dist u32, sigma/delta fp64) and are
// indexed with 64-bit arithmetic: B*N exceeds 2^32 at estate scale.  The
// batch index is blockIdx.y, so no kernel divides by N.
//
// The host-side loops (abom_pagerank_run, abom_brandes_run) are at the end
// of this file: C++, one device->host scalar read per iteration / level.

#include "abom_api.h"
#include "abom_wave.h"

namespace abom {

// Rows whose scanned degree is >= this are handled by one wave per row
// (mirrored as ops/native.py::CENTRALITY_HEAVY_DEGREE).
constexpr uint64_t CENTRALITY_HEAVY_DEGREE = 64;

constexpr int CEN_BLOCK = 256;                 // 4 waves
constexpr int CEN_WAVES = CEN_BLOCK / 64;

// Grid for one-wave-per-row kernels over `rows` heavy rows.
inline int heavy_grid(long long rows) { return grid_for(rows * 64, CEN_BLOCK); }

// ── PageRank ───────────────────────────────────────────────────────────────
//
// new[v] = (1-d)/n + d * sum_{u in in(v)} contrib[u] + d * dangling / n,
// contrib[u] = rank[u] / outdeg[u] (0 for dangling u), dangling = sum of rank
// over out-degree-0 nodes of the previous iterate.  The pass that writes
// new[v] also writes the next contrib[v] and feeds |new-rank| and the next
// dangling mass into the block partials.

// Fold (a, b) over the block in a fixed order and store them as this block's
// partial pair.  Every thread of the block must call it.
__device__ __forceinline__ void block_store_partials(double a, double b,
                                                     double* __restrict__ partial_pair) {
    __shared__ double sh[2 * CEN_WAVES];
    a = wave_sum(a);
    b = wave_sum(b);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[2 * wave] = a;
        sh[2 * wave + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sa = 0.0, sb = 0.0;
        for (int w = 0; w < CEN_WAVES; ++w) {
            sa += sh[2 * w];
            sb += sh[2 * w + 1];
        }
        partial_pair[0] = sa;
        partial_pair[1] = sb;
    }
}

__device__ __forceinline__ void pagerank_store(
    long long v, double pulled, double teleport, double damping, double dangling_share,
    const uint32_t* __restrict__ out_degree, const double* __restrict__ rank,
    double* __restrict__ new_rank, double* __restrict__ new_contrib,
    double& l1, double& dangling) {
    const double nv = teleport + damping * pulled + dangling_share;
    const uint32_t od = out_degree[v];
    new_rank[v] = nv;
    new_contrib[v] = od ? nv / (double)od : 0.0;
    l1 += fabs(nv - rank[v]);
    if (od == 0) dangling += nv;
}

__global__ __launch_bounds__(CEN_BLOCK) void pagerank_init_kernel(
    const uint32_t* __restrict__ out_degree, long long num_nodes,
    double* __restrict__ rank, double* __restrict__ contrib, double* __restrict__ partials) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const double r0 = 1.0 / (double)num_nodes;
    double dangling = 0.0;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < num_nodes;
         v += stride) {
        const uint32_t od = out_degree[v];
        rank[v] = r0;
        contrib[v] = od ? r0 / (double)od : 0.0;
        if (od == 0) dangling += r0;
    }
    block_store_partials(0.0, dangling, partials + 2 * (size_t)blockIdx.x);
}

// Thread per light row (in-degree < CENTRALITY_HEAVY_DEGREE).
__global__ __launch_bounds__(CEN_BLOCK) void pagerank_pull_kernel(
    const uint64_t* __restrict__ rev_off, const uint32_t* __restrict__ rev_col,
    const uint32_t* __restrict__ out_degree, long long num_nodes,
    double damping, const double* __restrict__ scalars,
    const double* __restrict__ rank, const double* __restrict__ contrib,
    double* __restrict__ new_rank, double* __restrict__ new_contrib,
    double* __restrict__ partials) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const double teleport = (1.0 - damping) / (double)num_nodes;
    const double dangling_share = damping * scalars[1] / (double)num_nodes;
    double l1 = 0.0, dangling = 0.0;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < num_nodes;
         v += stride) {
        const uint64_t beg = rev_off[v];
        const uint64_t end = rev_off[v + 1];
        if (end - beg >= CENTRALITY_HEAVY_DEGREE) continue;  // a wave owns it
        double pulled = 0.0;
        for (uint64_t e = beg; e < end; ++e) pulled += contrib[rev_col[e]];
        pagerank_store(v, pulled, teleport, damping, dangling_share, out_degree, rank,
                       new_rank, new_contrib, l1, dangling);
    }
    block_store_partials(l1, dangling, partials + 2 * (size_t)blockIdx.x);
}

// Wave per heavy row.
__global__ __launch_bounds__(CEN_BLOCK) void pagerank_pull_heavy_kernel(
    const uint64_t* __restrict__ rev_off, const uint32_t* __restrict__ rev_col,
    const uint32_t* __restrict__ heavy_rows, long long num_heavy,
    const uint32_t* __restrict__ out_degree, long long num_nodes,
    double damping, const double* __restrict__ scalars,
    const double* __restrict__ rank, const double* __restrict__ contrib,
    double* __restrict__ new_rank, double* __restrict__ new_contrib,
    double* __restrict__ partials) {
    const WaveId w = wave_id(blockDim.x >> 6);
    const int lane = w.lane;
    const double teleport = (1.0 - damping) / (double)num_nodes;
    const double dangling_share = damping * scalars[1] / (double)num_nodes;
    double l1 = 0.0, dangling = 0.0;  // carried by lane 0 only
    for (long long q = w.wave; q < num_heavy; q += w.n_waves) {
        const long long v = heavy_rows[q];
        const uint64_t beg = rev_off[v];
        const uint64_t end = rev_off[v + 1];
        double pulled = 0.0;
        for (uint64_t e = beg + lane; e < end; e += 64) pulled += contrib[rev_col[e]];
        pulled = wave_sum(pulled);
        if (lane == 0)
            pagerank_store(v, pulled, teleport, damping, dangling_share, out_degree, rank,
                           new_rank, new_contrib, l1, dangling);
    }
    block_store_partials(l1, dangling, partials + 2 * (size_t)blockIdx.x);
}

// One wave folds the partial pairs in index order: lane l takes pairs l,
// l+64, ... ascending, then the fixed tree.  scalars[0] = L1 change,
// scalars[1] = dangling mass of the iterate just written.
__global__ __launch_bounds__(64) void pagerank_finalize_kernel(
    const double* __restrict__ partials, int num_partials, double* __restrict__ scalars) {
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < num_partials; i += 64) {
        a += partials[2 * (size_t)i];
        b += partials[2 * (size_t)i + 1];
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (threadIdx.x == 0) {
        scalars[0] = a;
        scalars[1] = b;
    }
}

// ── Brandes betweenness, batched over B sources (blockIdx.y = b) ───────────

__global__ void brandes_seed_kernel(
    const uint32_t* __restrict__ sources, int batch, long long num_nodes,
    uint32_t* __restrict__ dist, double* __restrict__ sigma) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const uint64_t i = (uint64_t)b * (uint64_t)num_nodes + sources[b];
    dist[i] = 0;
    sigma[i] = 1.0;
}

// Forward level L, thread per light row: an undiscovered v pulls over its
// in-edges; if any in-neighbour sits at level L-1, v joins level L with
// sigma[v] = sum of their sigma (parallel edges count once each).
//
// Another thread may store L into dist[b][u] while this one reads it.  That
// is harmless: the reader only tests for == L-1, a 32-bit store is
// indivisible (the value read is UNVISITED or L, never a mix), and sigma of
// level L-1 was completed by the previous launch.
__global__ __launch_bounds__(CEN_BLOCK) void brandes_forward_kernel(
    const uint64_t* __restrict__ rev_off, const uint32_t* __restrict__ rev_col,
    const uint8_t* __restrict__ rev_et, uint32_t allowed_mask, long long num_nodes,
    uint32_t level, uint32_t* __restrict__ dist, double* __restrict__ sigma,
    unsigned int* __restrict__ discovered) {
    const uint64_t base = (uint64_t)blockIdx.y * (uint64_t)num_nodes;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const uint32_t prev = level - 1;
    unsigned claims = 0;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < num_nodes;
         v += stride) {
        if (dist[base + v] != ABOM_UNVISITED) continue;
        const uint64_t beg = rev_off[v];
        const uint64_t end = rev_off[v + 1];
        if (end - beg >= CENTRALITY_HEAVY_DEGREE) continue;  // a wave owns it
        double paths = 0.0;
        bool found = false;
        for (uint64_t e = beg; e < end; ++e) {
            if (edge_filtered(rev_et, allowed_mask, e)) continue;
            const uint64_t u = base + rev_col[e];
            if (dist[u] == prev) {
                paths += sigma[u];
                found = true;
            }
        }
        if (found) {
            dist[base + v] = level;
            sigma[base + v] = paths;
            ++claims;
        }
    }
    wave_add(discovered, claims);
}

// Forward level L, wave per heavy row (same race argument as above).
__global__ __launch_bounds__(CEN_BLOCK) void brandes_forward_heavy_kernel(
    const uint64_t* __restrict__ rev_off, const uint32_t* __restrict__ rev_col,
    const uint8_t* __restrict__ rev_et, uint32_t allowed_mask,
    const uint32_t* __restrict__ heavy_rows, long long num_heavy, long long num_nodes,
    uint32_t level, uint32_t* __restrict__ dist, double* __restrict__ sigma,
    unsigned int* __restrict__ discovered) {
    const uint64_t base = (uint64_t)blockIdx.y * (uint64_t)num_nodes;
    const WaveId w = wave_id(blockDim.x >> 6);
    const int lane = w.lane;
    const uint32_t prev = level - 1;
    unsigned claims = 0;  // lane 0 only
    for (long long q = w.wave; q < num_heavy; q += w.n_waves) {
        const uint64_t v = heavy_rows[q];
        if (dist[base + v] != ABOM_UNVISITED) continue;  // wave-uniform
        const uint64_t beg = rev_off[v];
        const uint64_t end = rev_off[v + 1];
        double paths = 0.0;
        bool found = false;
        for (uint64_t e = beg + lane; e < end; e += 64) {
            if (edge_filtered(rev_et, allowed_mask, e)) continue;
            const uint64_t u = base + rev_col[e];
            if (dist[u] == prev) {
                paths += sigma[u];
                found = true;
            }
        }
        paths = wave_sum(paths);
        const bool any_found = __ballot(found) != 0ull;
        if (lane == 0 && any_found) {
            dist[base + v] = level;
            sigma[base + v] = paths;
            ++claims;
        }
    }
    if (lane == 0 && claims) atomicAdd(discovered, claims);
}

// Backward level L, thread per light row: v at level L pulls over its
// out-edges from the successors at level L+1, whose delta is final.
__global__ __launch_bounds__(CEN_BLOCK) void brandes_backward_kernel(
    const uint64_t* __restrict__ fwd_off, const uint32_t* __restrict__ fwd_col,
    const uint8_t* __restrict__ fwd_et, uint32_t allowed_mask, long long num_nodes,
    uint32_t level, const uint32_t* __restrict__ dist, const double* __restrict__ sigma,
    double* __restrict__ delta) {
    const uint64_t base = (uint64_t)blockIdx.y * (uint64_t)num_nodes;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const uint32_t next = level + 1;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < num_nodes;
         v += stride) {
        if (dist[base + v] != level) continue;
        const uint64_t beg = fwd_off[v];
        const uint64_t end = fwd_off[v + 1];
        if (end - beg >= CENTRALITY_HEAVY_DEGREE) continue;  // a wave owns it
        const double sv = sigma[base + v];
        double dep = 0.0;
        for (uint64_t e = beg; e < end; ++e) {
            if (edge_filtered(fwd_et, allowed_mask, e)) continue;
            const uint64_t w = base + fwd_col[e];
            if (dist[w] == next) dep += sv / sigma[w] * (1.0 + delta[w]);
        }
        delta[base + v] = dep;
    }
}

// Backward level L, wave per heavy row.
__global__ __launch_bounds__(CEN_BLOCK) void brandes_backward_heavy_kernel(
    const uint64_t* __restrict__ fwd_off, const uint32_t* __restrict__ fwd_col,
    const uint8_t* __restrict__ fwd_et, uint32_t allowed_mask,
    const uint32_t* __restrict__ heavy_rows, long long num_heavy, long long num_nodes,
    uint32_t level, const uint32_t* __restrict__ dist, const double* __restrict__ sigma,
    double* __restrict__ delta) {
    const uint64_t base = (uint64_t)blockIdx.y * (uint64_t)num_nodes;
    const WaveId w = wave_id(blockDim.x >> 6);
    const int lane = w.lane;
    const uint32_t next = level + 1;
    for (long long q = w.wave; q < num_heavy; q += w.n_waves) {
        const uint64_t v = heavy_rows[q];
        if (dist[base + v] != level) continue;  // wave-uniform
        const uint64_t beg = fwd_off[v];
        const uint64_t end = fwd_off[v + 1];
        const double sv = sigma[base + v];
        double dep = 0.0;
        for (uint64_t e = beg + lane; e < end; e += 64) {
            if (edge_filtered(fwd_et, allowed_mask, e)) continue;
            const uint64_t w = base + fwd_col[e];
            if (dist[w] == next) dep += sv / sigma[w] * (1.0 + delta[w]);
        }
        dep = wave_sum(dep);
        if (lane == 0) delta[base + v] = dep;
    }
}

// bc[v] += sum_b delta[b][v], ascending b, skipping each batch member's own
// source and the nodes it did not reach.  One thread owns v: plain stores.
__global__ __launch_bounds__(CEN_BLOCK) void brandes_accumulate_kernel(
    const uint32_t* __restrict__ sources, int batch, long long num_nodes,
    const uint32_t* __restrict__ dist, const double* __restrict__ delta,
    double* __restrict__ bc) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < num_nodes;
         v += stride) {
        double acc = bc[v];
        for (int b = 0; b < batch; ++b) {
            const uint64_t i = (uint64_t)b * (uint64_t)num_nodes + (uint64_t)v;
            if ((long long)sources[b] == v || dist[i] == ABOM_UNVISITED) continue;
            acc += delta[i];
        }
        bc[v] = acc;
    }
}

// Device -> host read of one value; the one sync point of an iteration/level.
template <typename T>
static int read_scalar(T* host, const T* dev, hipStream_t s) {
    ABOM_CHECK(hipMemcpyAsync(host, dev, sizeof(T), hipMemcpyDeviceToHost, s));
    return (int)hipStreamSynchronize(s);
}

}  // namespace abom

// ── C ABI: the iteration / level loops ─────────────────────────────────────

// PageRank power iteration over the reverse CSR.  rank_a/rank_b and
// contrib_a/contrib_b are fp64[N] ping-pong buffers, partials is
// fp64[2 * (grid_for(N) + heavy grid)] (4096 pairs always suffice), scalars
// is fp64[2].  Stops after `iterations` passes or after the first pass whose
// L1 change is below `tolerance`.  Returns the number of passes run (the
// result is in rank_a when that is even, rank_b when odd) or a negated
// hipError_t.
extern "C" int abom_pagerank_run(
    const void* rev_off, const void* rev_col, const void* rev_heavy, long long num_rev_heavy,
    const void* out_degree, long long num_nodes, double damping, double tolerance,
    int iterations, void* rank_a, void* rank_b, void* contrib_a, void* contrib_b,
    void* partials, void* scalars, void* stream) {
    using namespace abom;
    if (num_nodes <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int grid = grid_for(num_nodes, CEN_BLOCK);
    const int hgrid = num_rev_heavy > 0 ? heavy_grid(num_rev_heavy) : 0;
    double* part = (double*)partials;
    double* sc = (double*)scalars;
    double* rank = (double*)rank_a;
    double* next_rank = (double*)rank_b;
    double* contrib = (double*)contrib_a;
    double* next_contrib = (double*)contrib_b;
    int rc;

    hipLaunchKernelGGL(pagerank_init_kernel, dim3(grid), dim3(CEN_BLOCK), 0, s,
                       (const uint32_t*)out_degree, num_nodes, rank, contrib, part);
    if ((rc = (int)hipGetLastError())) return -rc;
    hipLaunchKernelGGL(pagerank_finalize_kernel, dim3(1), dim3(64), 0, s,
                       (const double*)part, grid, sc);
    if ((rc = (int)hipGetLastError())) return -rc;

    int done = 0;
    while (done < iterations) {
        hipLaunchKernelGGL(pagerank_pull_kernel, dim3(grid), dim3(CEN_BLOCK), 0, s,
                           (const uint64_t*)rev_off, (const uint32_t*)rev_col,
                           (const uint32_t*)out_degree, num_nodes, damping,
                           (const double*)sc, (const double*)rank, (const double*)contrib,
                           next_rank, next_contrib, part);
        if ((rc = (int)hipGetLastError())) return -rc;
        if (hgrid) {
            hipLaunchKernelGGL(pagerank_pull_heavy_kernel, dim3(hgrid), dim3(CEN_BLOCK), 0, s,
                               (const uint64_t*)rev_off, (const uint32_t*)rev_col,
                               (const uint32_t*)rev_heavy, num_rev_heavy,
                               (const uint32_t*)out_degree, num_nodes, damping,
                               (const double*)sc, (const double*)rank,
                               (const double*)contrib, next_rank, next_contrib,
                               part + 2 * (size_t)grid);
            if ((rc = (int)hipGetLastError())) return -rc;
        }
        // stream order: both pulls read scalars[1] before this overwrites it
        hipLaunchKernelGGL(pagerank_finalize_kernel, dim3(1), dim3(64), 0, s,
                           (const double*)part, grid + hgrid, sc);
        if ((rc = (int)hipGetLastError())) return -rc;
        double l1 = 0.0;
        if ((rc = read_scalar(&l1, (const double*)sc, s))) return -rc;
        ++done;
        double* t = rank; rank = next_rank; next_rank = t;
        t = contrib; contrib = next_contrib; next_contrib = t;
        if (l1 < tolerance) break;
    }
    return done;
}

// One batch of Brandes sources: forward levels until no batch member
// discovers anything (no cap on levels), backward levels from the deepest
// down to 0, then bc[v] += sum_b delta[b][v].  dist is u32[B*N], sigma and
// delta are fp64[B*N], bc is fp64[N] (accumulated into, not cleared),
// counter is one device u32.  Edge types and the heavy-row lists are
// nullable (num_*_heavy == 0).  Returns the deepest level reached or a
// negated hipError_t.
extern "C" int abom_brandes_run(
    const void* fwd_off, const void* fwd_col, const void* fwd_et,
    const void* rev_off, const void* rev_col, const void* rev_et, unsigned int allowed_mask,
    const void* fwd_heavy, long long num_fwd_heavy,
    const void* rev_heavy, long long num_rev_heavy,
    const void* sources, int batch, long long num_nodes,
    void* dist, void* sigma, void* delta, void* bc, void* counter, void* stream) {
    using namespace abom;
    if (num_nodes <= 0 || batch <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const size_t cells = (size_t)batch * (size_t)num_nodes;
    const dim3 block(CEN_BLOCK);
    const dim3 grid(grid_for(num_nodes, CEN_BLOCK), batch);
    const dim3 rev_hgrid(num_rev_heavy > 0 ? heavy_grid(num_rev_heavy) : 0, batch);
    const dim3 fwd_hgrid(num_fwd_heavy > 0 ? heavy_grid(num_fwd_heavy) : 0, batch);
    unsigned int* ctr = (unsigned int*)counter;
    int rc;

    // 0xFF bytes = ABOM_UNVISITED; delta of the deepest level stays 0
    if ((rc = (int)hipMemsetAsync(dist, 0xFF, cells * sizeof(uint32_t), s))) return -rc;
    if ((rc = (int)hipMemsetAsync(delta, 0, cells * sizeof(double), s))) return -rc;
    hipLaunchKernelGGL(brandes_seed_kernel, dim3((batch + 63) / 64), dim3(64), 0, s,
                       (const uint32_t*)sources, batch, num_nodes, (uint32_t*)dist,
                       (double*)sigma);
    if ((rc = (int)hipGetLastError())) return -rc;

    unsigned int level = 0;
    for (;;) {
        ++level;
        if ((rc = (int)hipMemsetAsync(ctr, 0, sizeof(unsigned int), s))) return -rc;
        hipLaunchKernelGGL(brandes_forward_kernel, grid, block, 0, s,
                           (const uint64_t*)rev_off, (const uint32_t*)rev_col,
                           (const uint8_t*)rev_et, allowed_mask, num_nodes, level,
                           (uint32_t*)dist, (double*)sigma, ctr);
        if ((rc = (int)hipGetLastError())) return -rc;
        if (rev_hgrid.x) {
            hipLaunchKernelGGL(brandes_forward_heavy_kernel, rev_hgrid, block, 0, s,
                               (const uint64_t*)rev_off, (const uint32_t*)rev_col,
                               (const uint8_t*)rev_et, allowed_mask,
                               (const uint32_t*)rev_heavy, num_rev_heavy, num_nodes, level,
                               (uint32_t*)dist, (double*)sigma, ctr);
            if ((rc = (int)hipGetLastError())) return -rc;
        }
        unsigned int discovered = 0;
        if ((rc = read_scalar(&discovered, (const unsigned int*)ctr, s))) return -rc;
        if (discovered == 0) break;
    }
    const unsigned int deepest = level - 1;  // last level that discovered a node

    for (unsigned int l = deepest; l-- > 0;) {
        hipLaunchKernelGGL(brandes_backward_kernel, grid, block, 0, s,
                           (const uint64_t*)fwd_off, (const uint32_t*)fwd_col,
                           (const uint8_t*)fwd_et, allowed_mask, num_nodes, l,
                           (const uint32_t*)dist, (const double*)sigma, (double*)delta);
        if ((rc = (int)hipGetLastError())) return -rc;
        if (fwd_hgrid.x) {
            hipLaunchKernelGGL(brandes_backward_heavy_kernel, fwd_hgrid, block, 0, s,
                               (const uint64_t*)fwd_off, (const uint32_t*)fwd_col,
                               (const uint8_t*)fwd_et, allowed_mask,
                               (const uint32_t*)fwd_heavy, num_fwd_heavy, num_nodes, l,
                               (const uint32_t*)dist, (const double*)sigma, (double*)delta);
            if ((rc = (int)hipGetLastError())) return -rc;
        }
    }

    hipLaunchKernelGGL(brandes_accumulate_kernel, dim3(grid.x), block, 0, s,
                       (const uint32_t*)sources, batch, num_nodes, (const uint32_t*)dist,
                       (const double*)delta, (double*)bc);
    if ((rc = (int)hipGetLastError())) return -rc;
    return (int)deepest;
}
