// Fused blast-radius reach counting on gfx950.
//
// Three entry points, same outputs (six counts and an overflow flag per
// package):
//
// abom_blast_counts_indexed — the engine's path.  A server's distinct
// agents, creds and tools depend on the graph alone, so the engine lays them
// out once per server (the reach index, built next to the CSR).  Pass A
// (blast_index_fast_kernel, one thread per package, no LDS) finishes every
// package with at most one distinct containing server straight from that
// server's index row -- ~89 % of the matched packages of the benchmark
// estate -- and queues the rest.  Pass B (blast_index_wave_kernel, one wave
// per queued package) copies the index segments of the package's servers
// into LDS and distinct-counts the unions.  The queue length stays on the
// device; the kernels count the overflowed rows into one word, the only
// thing the host reads.
//
// abom_blast_counts_indexed_sized — the same two passes when the host knows
// only a bound on the package count: the count is a device word that an
// earlier kernel of the stream writes, the grids are sized for the bound, and
// the two counters reach pinned host memory through a copy on the stream.
//
// abom_blast_counts — for callers without an index (and the A/B knob
// AGENT_BOM_BLAST_INDEX=0).  It replaced the torch sort/unique/bincount join
// pipeline (gpu_engine.py _blast_counts_join — ~20 kernel launches per step)
// with ONE wave-cooperative
// kernel: each 64-lane wave owns one finding package and walks
// package -> servers (reverse CONTAINS) -> {agents (reverse USES),
// creds (forward EXPOSES_CRED), tools (forward PROVIDES_TOOL)} collecting
// candidates into per-wave LDS arrays, then distinct-counts them in LDS
// (O(m^2/64) first-occurrence scan — m is capped, LDS reads are 2 cycles).
//
// Zipf-head packages that overflow the LDS caps are flagged; the host
// resolves just those with the sort-based path (hybrid, exact either way);
// all entry points share the caps.
// CDNA4 notes: one workgroup = 4 waves = 4 packages; LDS slice per wave =
// (SRV_CAP + AG_CAP + CR_CAP + TL_CAP) * 4 B = 4.25 KiB -> 17 KiB/block,
// sized so LDS is not the occupancy limiter (see cap comment below); the
// indexed wave kernel adds a 64-entry server chunk and the per-server
// segment tables, 6 KiB per wave -> 24 KiB/block.

#include "abom_api.h"
#include "abom_wave.h"

namespace abom {

// Caps sized for occupancy: 4.1 KiB LDS per wave -> 16.5 KiB per 4-wave
// block -> 9 blocks/CU (full 32-wave occupancy; the previous 8.5 KiB/wave
// layout measured 11.1/32).  Zipf-head packages beyond a cap overflow to
// the exact sort-based join, so caps trade fallback rate for occupancy.
constexpr int SRV_CAP = 64;
constexpr int AG_CAP = 256;
constexpr int CR_CAP = 256;
constexpr int TL_CAP = 512;
constexpr int WAVES_PER_BLOCK = 4;

// Collect neighbors of `node` with edge type `want` into lds[cap]; returns
// new count or -1 on overflow (count accumulated across calls).
__device__ __forceinline__ int collect(
    const uint64_t* __restrict__ row_off, const uint32_t* __restrict__ col,
    const uint8_t* __restrict__ etype, uint32_t node, uint8_t want,
    uint32_t* lds, int count, int cap, int lane, bool* overflow) {
    const uint64_t beg = row_off[node];
    const uint64_t end = row_off[node + 1];
    for (uint64_t base = beg; base < end; base += 64) {
        const uint64_t e = base + lane;
        const bool valid = e < end && etype[e] == want;
        const unsigned long long mask = __ballot(valid);
        const int my_rank = __popcll(mask & ((1ull << lane) - 1));
        const int n_new = __popcll(mask);
        if (valid) {
            const int idx = count + my_rank;
            if (idx < cap) lds[idx] = col[e];
        }
        count += n_new;
        if (count > cap) { *overflow = true; return cap; }
    }
    return count;
}

// One pass over `node`'s FORWARD edge row appending creds and tools into
// their LDS arrays simultaneously — the fwd row of a server is dominated by
// CONTAINS->package edges, so scanning it once instead of once per type
// saves the bulk of this kernel's edge traffic.
__device__ __forceinline__ void collect_fwd2(
    const uint64_t* __restrict__ row_off, const uint32_t* __restrict__ col,
    const uint8_t* __restrict__ etype, uint32_t node,
    uint8_t want_a, uint32_t* lds_a, int* count_a, int cap_a,
    uint8_t want_b, uint32_t* lds_b, int* count_b, int cap_b,
    int lane, bool* overflow) {
    const uint64_t beg = row_off[node];
    const uint64_t end = row_off[node + 1];
    for (uint64_t base = beg; base < end; base += 64) {
        const uint64_t e = base + lane;
        const bool in = e < end;
        const uint8_t et = in ? etype[e] : (uint8_t)0xFF;
        const uint32_t v = in ? col[e] : 0u;
        const bool va = in && et == want_a;
        const bool vb = in && et == want_b;
        const unsigned long long ma = __ballot(va);
        const unsigned long long mb = __ballot(vb);
        if (va) {
            const int idx = *count_a + __popcll(ma & ((1ull << lane) - 1));
            if (idx < cap_a) lds_a[idx] = v;
        }
        if (vb) {
            const int idx = *count_b + __popcll(mb & ((1ull << lane) - 1));
            if (idx < cap_b) lds_b[idx] = v;
        }
        *count_a += __popcll(ma);
        *count_b += __popcll(mb);
        if (*count_a > cap_a || *count_b > cap_b) { *overflow = true; return; }
    }
}

// Distinct count of lds[0..m): lane-strided first-occurrence scan.
// Also counts distinct elements whose db_flag[node] is set.
// FULL_SCAN compares an entry with every earlier one, four per iteration,
// instead of leaving the loop at the first hit: with the exit every LDS read
// waits for the compare before it, and the heavy packages of the indexed
// wave kernel (hundreds of entries) were its tail.  Same counts either way.
// blast_count_kernel keeps the exit: the wider loop costs it a wave per
// SIMD, and nothing measured that path.
template <bool FULL_SCAN>
__device__ __forceinline__ void distinct_count(
    const uint32_t* lds, int m, const uint8_t* __restrict__ db_flag,
    int lane, int* out_all, int* out_db) {
    int cnt = 0, cnt_db = 0;
    for (int i = lane; i < m; i += 64) {
        const uint32_t v = lds[i];
        bool first = true;
        if (FULL_SCAN) {
            int dup = 0, j = 0;
            for (; j + 4 <= i; j += 4)
                dup |= (lds[j] == v) | (lds[j + 1] == v) | (lds[j + 2] == v) | (lds[j + 3] == v);
            for (; j < i; ++j) dup |= lds[j] == v;
            first = !dup;
        } else {
            for (int j = 0; j < i; ++j) {
                if (lds[j] == v) { first = false; break; }
            }
        }
        if (first) {
            ++cnt;
            if (db_flag && db_flag[v]) ++cnt_db;
        }
    }
    *out_all = wave_sum(cnt);
    *out_db = wave_sum(cnt_db);
}

__global__ void __launch_bounds__(256) blast_count_kernel(
    const uint32_t* __restrict__ pkgs,          // [n] package node ids
    long long n,
    const uint64_t* __restrict__ rev_off, const uint32_t* __restrict__ rev_col,
    const uint8_t* __restrict__ rev_et,
    const uint64_t* __restrict__ fwd_off, const uint32_t* __restrict__ fwd_col,
    const uint8_t* __restrict__ fwd_et,
    uint8_t et_contains, uint8_t et_uses, uint8_t et_cred, uint8_t et_tool,
    const uint8_t* __restrict__ node_is_db_cred,  // [N]
    const uint8_t* __restrict__ node_is_db_tool,  // [N]
    uint32_t* __restrict__ out_counts,            // [n*6]
    uint8_t* __restrict__ out_overflow) {         // [n]
    __shared__ uint32_t lds_srv[WAVES_PER_BLOCK][SRV_CAP];
    __shared__ uint32_t lds_ag[WAVES_PER_BLOCK][AG_CAP];
    __shared__ uint32_t lds_cr[WAVES_PER_BLOCK][CR_CAP];
    __shared__ uint32_t lds_tl[WAVES_PER_BLOCK][TL_CAP];

    const WaveId w = wave_id(WAVES_PER_BLOCK);
    const int lane = w.lane, wid = w.wid;

    for (long long p = w.wave; p < n; p += w.n_waves) {
        const uint32_t pkg = pkgs[p];
        bool overflow = false;

        int n_srv = collect(rev_off, rev_col, rev_et, pkg, et_contains,
                            lds_srv[wid], 0, SRV_CAP, lane, &overflow);
        int n_ag = 0, n_cr = 0, n_tl = 0;
        if (!overflow) {
            for (int s = 0; s < n_srv && !overflow; ++s) {
                const uint32_t srv = lds_srv[wid][s];
                n_ag = collect(rev_off, rev_col, rev_et, srv, et_uses,
                               lds_ag[wid], n_ag, AG_CAP, lane, &overflow);
                if (overflow) break;
                collect_fwd2(fwd_off, fwd_col, fwd_et, srv,
                             et_cred, lds_cr[wid], &n_cr, CR_CAP,
                             et_tool, lds_tl[wid], &n_tl, TL_CAP,
                             lane, &overflow);
            }
        }

        if (overflow) {
            if (lane == 0) {
                out_overflow[p] = 1;
                for (int k = 0; k < 6; ++k) out_counts[p * 6 + k] = 0;
            }
            continue;
        }

        int srv_all, srv_db, ag_all, ag_db, cr_all, cr_db, tl_all, tl_db;
        distinct_count<false>(lds_srv[wid], n_srv, nullptr, lane, &srv_all, &srv_db);
        distinct_count<false>(lds_ag[wid], n_ag, nullptr, lane, &ag_all, &ag_db);
        distinct_count<false>(lds_cr[wid], n_cr, node_is_db_cred, lane, &cr_all, &cr_db);
        distinct_count<false>(lds_tl[wid], n_tl, node_is_db_tool, lane, &tl_all, &tl_db);

        if (lane == 0) {
            out_overflow[p] = 0;
            out_counts[p * 6 + 0] = (uint32_t)srv_all;
            out_counts[p * 6 + 1] = (uint32_t)ag_all;
            out_counts[p * 6 + 2] = (uint32_t)cr_all;
            out_counts[p * 6 + 3] = (uint32_t)cr_db;
            out_counts[p * 6 + 4] = (uint32_t)tl_all;
            out_counts[p * 6 + 5] = (uint32_t)tl_db;
        }
    }
}

// ── indexed path ───────────────────────────────────────────────────────────
//
// reach_off / reach_col / reach_db are the per-server reach index that
// EstateEngine builds once next to the CSR (graph/gpu_engine.py
// build_reach_index): row r = server node id - row_base, reach_off[r] =
// (agents begin, creds begin, tools begin, end) into reach_col, every segment
// ascending and duplicate-free, reach_db[r] = (db creds, db tools).

constexpr uint32_t NO_SERVER = 0xFFFFFFFFu;

__device__ __forceinline__ void write_counts(
    uint32_t* __restrict__ out_counts, long long p, uint32_t srv, uint32_t ag,
    uint32_t cr, uint32_t cr_db, uint32_t tl, uint32_t tl_db) {
    uint2* row = reinterpret_cast<uint2*>(out_counts + p * 6);  // 24 B rows
    row[0] = make_uint2(srv, ag);
    row[1] = make_uint2(cr, cr_db);
    row[2] = make_uint2(tl, tl_db);
}

// Pass A: one thread per package.  Packages with no or one distinct
// containing server are finished here from the index row alone (no LDS, no
// set operation); the rest are queued for the wave kernel.  counters[0] is
// the queue length, counters[1] the number of overflowed rows.
// `n_dev`, when given, holds the package count (the sized entry point: the
// host knows only a bound); otherwise the count is `n`.
__global__ void __launch_bounds__(256) blast_index_fast_kernel(
    const uint32_t* __restrict__ pkgs, long long n, const long long* __restrict__ n_dev,
    const uint64_t* __restrict__ rev_off, const uint32_t* __restrict__ rev_col,
    const uint8_t* __restrict__ rev_et, uint8_t et_contains,
    const int4* __restrict__ reach_off, const int2* __restrict__ reach_db,
    uint32_t row_base, uint32_t num_rows,
    uint32_t* __restrict__ queue, unsigned int* __restrict__ counters,
    uint32_t* __restrict__ out_counts, uint8_t* __restrict__ out_overflow) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long start = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n_dev) n = *n_dev;
    // wave-uniform trip count: every lane reaches the ballots below
    for (long long base = start - lane; base < n; base += stride) {
        const long long p = base + lane;
        const bool active = p < n;
        uint32_t first = NO_SERVER;
        bool multi = false;
        if (active) {
            const uint32_t pkg = pkgs[p];
            const uint64_t beg = rev_off[pkg];
            const uint64_t end = rev_off[pkg + 1];
            for (uint64_t e = beg; e < end; ++e) {
                if (rev_et[e] != et_contains) continue;
                const uint32_t s = rev_col[e];
                if (first == NO_SERVER) {
                    first = s;
                } else if (s != first) {
                    multi = true;
                    break;
                }
            }
        }
        // a server outside the index cannot be answered here: flag the row,
        // the caller's exact join takes it
        const bool outside = active && !multi && first != NO_SERVER &&
                             first - row_base >= num_rows;
        if (active && !multi && !outside) {
            if (first == NO_SERVER) {
                write_counts(out_counts, p, 0, 0, 0, 0, 0, 0);
            } else {
                const int4 off = reach_off[first - row_base];
                const int2 db = reach_db[first - row_base];
                write_counts(out_counts, p, 1, (uint32_t)(off.y - off.x),
                             (uint32_t)(off.z - off.y), (uint32_t)db.x,
                             (uint32_t)(off.w - off.z), (uint32_t)db.y);
            }
            out_overflow[p] = 0;
        }
        if (outside) {
            write_counts(out_counts, p, 0, 0, 0, 0, 0, 0);
            out_overflow[p] = 1;
        }
        // one atomic per wave and counter
        wave_queue_push(multi, (uint32_t)p, queue, &counters[0], lane);
        wave_count_flag(outside, &counters[1], lane);
    }
}

// Copy the index segments of the wave's servers into dst[0..total): entry i
// belongs to the last server s with pref[s] <= i (pref = exclusive prefix of
// the segment lengths), at reach_col[beg[s] + i - pref[s]].
__device__ __forceinline__ void gather_segments(
    const int* beg, const int* pref, int n_srv, int total,
    const uint32_t* __restrict__ reach_col, uint32_t* dst, int lane) {
    for (int i = lane; i < total; i += 64) {
        const int s = segment_of(pref, n_srv, i);
        dst[i] = reach_col[beg[s] + (i - pref[s])];
    }
}

// Pass B: one wave per queued package (two or more containing servers).
// The grid reads the queue length from device memory, so no host read sits
// between the passes.
__global__ void __launch_bounds__(256) blast_index_wave_kernel(
    const uint32_t* __restrict__ pkgs,
    const uint64_t* __restrict__ rev_off, const uint32_t* __restrict__ rev_col,
    const uint8_t* __restrict__ rev_et, uint8_t et_contains,
    const int4* __restrict__ reach_off, const uint32_t* __restrict__ reach_col,
    uint32_t row_base, uint32_t num_rows,
    const uint8_t* __restrict__ node_is_db_cred,
    const uint8_t* __restrict__ node_is_db_tool,
    const uint32_t* __restrict__ queue, unsigned int* __restrict__ counters,
    uint32_t* __restrict__ out_counts, uint8_t* __restrict__ out_overflow) {
    // servers: SRV_CAP distinct ones plus one 64-edge chunk being deduplicated
    __shared__ uint32_t lds_srv[WAVES_PER_BLOCK][SRV_CAP + 64];
    __shared__ int lds_beg[WAVES_PER_BLOCK][3][SRV_CAP];
    __shared__ int lds_pref[WAVES_PER_BLOCK][3][SRV_CAP];
    __shared__ uint32_t lds_ag[WAVES_PER_BLOCK][AG_CAP];
    __shared__ uint32_t lds_cr[WAVES_PER_BLOCK][CR_CAP];
    __shared__ uint32_t lds_tl[WAVES_PER_BLOCK][TL_CAP];

    const WaveId w = wave_id(WAVES_PER_BLOCK);
    const int lane = w.lane, wid = w.wid;
    const long long n_queued = counters[0];
    uint32_t* srv = lds_srv[wid];

    for (long long q = w.wave; q < n_queued; q += w.n_waves) {
        const long long p = queue[q];
        const uint32_t pkg = pkgs[p];
        bool overflow = false;

        // distinct containing servers, in first-seen order
        int n_srv = 0;
        const uint64_t beg = rev_off[pkg];
        const uint64_t end = rev_off[pkg + 1];
        for (uint64_t base = beg; base < end && !overflow; base += 64) {
            const uint64_t e = base + lane;
            const bool valid = e < end && rev_et[e] == et_contains;
            const uint32_t v = valid ? rev_col[e] : 0u;
            const unsigned long long mask = __ballot(valid);
            const int rank = __popcll(mask & ((1ull << lane) - 1));
            if (valid) srv[n_srv + rank] = v;  // n_srv <= SRV_CAP: inside the chunk area
            __builtin_amdgcn_wave_barrier();
            bool first = valid;
            if (valid) {
                for (int j = 0; j < n_srv + rank; ++j) {
                    if (srv[j] == v) { first = false; break; }
                }
            }
            // out-of-index servers cannot be joined here
            if (first && v - row_base >= num_rows) overflow = true;
            const unsigned long long fmask = __ballot(first);
            __builtin_amdgcn_wave_barrier();  // all reads above precede the compaction
            if (first) srv[n_srv + __popcll(fmask & ((1ull << lane) - 1))] = v;
            __builtin_amdgcn_wave_barrier();
            n_srv += __popcll(fmask);
            if (n_srv > SRV_CAP) overflow = true;
            overflow = __ballot(overflow) != 0;
        }

        int n_ag = 0, n_cr = 0, n_tl = 0;
        if (!overflow) {
            // one lane per server: its index row, then the three prefix sums
            int4 off = make_int4(0, 0, 0, 0);
            if (lane < n_srv) off = reach_off[srv[lane] - row_base];
            const int p_ag = wave_exclusive_scan(off.y - off.x, lane, &n_ag);
            const int p_cr = wave_exclusive_scan(off.z - off.y, lane, &n_cr);
            const int p_tl = wave_exclusive_scan(off.w - off.z, lane, &n_tl);
            overflow = n_ag > AG_CAP || n_cr > CR_CAP || n_tl > TL_CAP;
            if (!overflow) {
                lds_beg[wid][0][lane] = off.x; lds_pref[wid][0][lane] = p_ag;
                lds_beg[wid][1][lane] = off.y; lds_pref[wid][1][lane] = p_cr;
                lds_beg[wid][2][lane] = off.z; lds_pref[wid][2][lane] = p_tl;
                __builtin_amdgcn_wave_barrier();
                gather_segments(lds_beg[wid][0], lds_pref[wid][0], n_srv, n_ag,
                                reach_col, lds_ag[wid], lane);
                gather_segments(lds_beg[wid][1], lds_pref[wid][1], n_srv, n_cr,
                                reach_col, lds_cr[wid], lane);
                gather_segments(lds_beg[wid][2], lds_pref[wid][2], n_srv, n_tl,
                                reach_col, lds_tl[wid], lane);
                __builtin_amdgcn_wave_barrier();
            }
        }

        if (overflow) {
            if (lane == 0) {
                out_overflow[p] = 1;
                write_counts(out_counts, p, 0, 0, 0, 0, 0, 0);
                atomicAdd(&counters[1], 1u);
            }
            continue;
        }

        int ag_all, ag_db, cr_all, cr_db, tl_all, tl_db;
        distinct_count<true>(lds_ag[wid], n_ag, nullptr, lane, &ag_all, &ag_db);
        distinct_count<true>(lds_cr[wid], n_cr, node_is_db_cred, lane, &cr_all, &cr_db);
        distinct_count<true>(lds_tl[wid], n_tl, node_is_db_tool, lane, &tl_all, &tl_db);

        if (lane == 0) {
            out_overflow[p] = 0;
            write_counts(out_counts, p, (uint32_t)n_srv, (uint32_t)ag_all,
                         (uint32_t)cr_all, (uint32_t)cr_db, (uint32_t)tl_all,
                         (uint32_t)tl_db);
        }
    }
}

// Both passes over `n` packages, or, with n_dev, over at most `n` packages of
// which the device word says how many count: the grids are sized for `n` and
// stride.
static int launch_blast_index(
    const void* pkgs, long long n, const void* n_dev,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    const void* reach_off, const void* reach_col, const void* reach_db,
    long long row_base, long long num_rows,
    const void* node_is_db_cred, const void* node_is_db_tool,
    void* queue, void* counters, void* out_counts, void* out_overflow, hipStream_t s) {
    const int block = 256;
    hipLaunchKernelGGL(blast_index_fast_kernel, dim3(grid_for(n, block)), dim3(block), 0, s,
                       (const uint32_t*)pkgs, n_dev ? 0ll : n, (const long long*)n_dev,
                       (const uint64_t*)rev_off, (const uint32_t*)rev_col,
                       (const uint8_t*)rev_et, (uint8_t)et_contains,
                       (const int4*)reach_off, (const int2*)reach_db,
                       (uint32_t)row_base, (uint32_t)num_rows,
                       (uint32_t*)queue, (unsigned int*)counters,
                       (uint32_t*)out_counts, (uint8_t*)out_overflow);
    ABOM_CHECK(hipGetLastError());
    // the queue length is known on the device only: size the grid for the
    // worst case (every package queued) and let the waves stride over it
    hipLaunchKernelGGL(blast_index_wave_kernel, dim3(grid_for(n, WAVES_PER_BLOCK)), dim3(block),
                       0, s, (const uint32_t*)pkgs,
                       (const uint64_t*)rev_off, (const uint32_t*)rev_col,
                       (const uint8_t*)rev_et, (uint8_t)et_contains,
                       (const int4*)reach_off, (const uint32_t*)reach_col,
                       (uint32_t)row_base, (uint32_t)num_rows,
                       (const uint8_t*)node_is_db_cred, (const uint8_t*)node_is_db_tool,
                       (const uint32_t*)queue, (unsigned int*)counters,
                       (uint32_t*)out_counts, (uint8_t*)out_overflow);
    return (int)hipGetLastError();
}

}  // namespace abom

extern "C" int abom_blast_counts_indexed(
    const void* pkgs, long long n,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    const void* reach_off, const void* reach_col, const void* reach_db,
    long long row_base, long long num_rows,
    const void* node_is_db_cred, const void* node_is_db_tool,
    void* queue, void* counters, void* out_counts, void* out_overflow, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    ABOM_CHECK(hipMemsetAsync(counters, 0, 2 * sizeof(unsigned int), s));
    if (n <= 0) return 0;
    return abom::launch_blast_index(pkgs, n, nullptr, rev_off, rev_col, rev_et, et_contains,
                                    reach_off, reach_col, reach_db, row_base, num_rows,
                                    node_is_db_cred, node_is_db_tool, queue, counters,
                                    out_counts, out_overflow, s);
}

// The same two passes over at most `n_cap` packages; the count itself is the
// device word `n_dev`, which an earlier kernel of the stream writes.  The
// counters reach `host_counters` (pinned, two u32) through a copy on the
// stream; the caller waits for it.
extern "C" int abom_blast_counts_indexed_sized(
    const void* pkgs, const void* n_dev, long long n_cap,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    const void* reach_off, const void* reach_col, const void* reach_db,
    long long row_base, long long num_rows,
    const void* node_is_db_cred, const void* node_is_db_tool,
    void* queue, void* counters, void* host_counters,
    void* out_counts, void* out_overflow, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    ABOM_CHECK(hipMemsetAsync(counters, 0, 2 * sizeof(unsigned int), s));
    if (n_cap > 0) {
        const int rc = abom::launch_blast_index(
            pkgs, n_cap, n_dev, rev_off, rev_col, rev_et, et_contains, reach_off, reach_col,
            reach_db, row_base, num_rows, node_is_db_cred, node_is_db_tool, queue, counters,
            out_counts, out_overflow, s);
        if (rc != 0) return rc;
    }
    ABOM_CHECK(hipMemcpyAsync(host_counters, counters, 2 * sizeof(unsigned int),
                              hipMemcpyDeviceToHost, s));
    return 0;
}

extern "C" int abom_blast_counts(
    const void* pkgs, long long n,
    const void* rev_off, const void* rev_col, const void* rev_et,
    const void* fwd_off, const void* fwd_col, const void* fwd_et,
    int et_contains, int et_uses, int et_cred, int et_tool,
    const void* node_is_db_cred, const void* node_is_db_tool,
    void* out_counts, void* out_overflow, void* stream) {
    const int block = 256;
    hipLaunchKernelGGL(abom::blast_count_kernel,
                       dim3(abom::grid_for(n, abom::WAVES_PER_BLOCK)), dim3(block), 0,
                       (hipStream_t)stream,
                       (const uint32_t*)pkgs, n,
                       (const uint64_t*)rev_off, (const uint32_t*)rev_col,
                       (const uint8_t*)rev_et,
                       (const uint64_t*)fwd_off, (const uint32_t*)fwd_col,
                       (const uint8_t*)fwd_et,
                       (uint8_t)et_contains, (uint8_t)et_uses, (uint8_t)et_cred,
                       (uint8_t)et_tool,
                       (const uint8_t*)node_is_db_cred, (const uint8_t*)node_is_db_tool,
                       (uint32_t*)out_counts, (uint8_t*)out_overflow);
    return (int)hipGetLastError();
}
