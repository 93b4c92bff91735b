// findings.hip — assemble the canonical finding stream from dedup-match pairs.
//
// The match kernel emits UNSORTED (row << 32 | win) pairs over the DISTINCT
// (name, version) rows.  The engine needs them fanned out to package rows and
// sorted by (pkg << 32 | win), plus the per-step unique-package list and each
// finding's position in it.  Nothing here is a sort: package order comes from
// a P-bit bitmap walked in ascending order, window order from a per-pair rank
// counted along the row's (tiny) match chain.
//
//   1. findings_mark:   per pair, count it on its row and push it on the
//                       row's chain (atomicExch on the tail); the row's first
//                       arrival sets the bitmap bits of the row's packages.
//   2. findings_rank:   per pair, rank = pairs of the same row with a smaller
//                       window (ties by pair index) — independent of the
//                       order in which the atomics arrived.
//   3. findings_count:  per bitmap word, findings under it; per block, sums
//                       of (packages, findings).
//   4. findings_scan:   exclusive scan of the block sums; totals for the host.
//   5. findings_emit:   per word, block-scan to the word's output offsets,
//                       walk the set bits ascending and scatter each
//                       package's windows by rank; the word is zeroed.
//   6. findings_reset:  per pair, zero its row's count and tail.
//
// Steps 5 and 6 leave the workspace all-zero again by revisiting only what
// this call touched, so the steady state never writes U- or P-sized arrays.
// wave64; plain stores and atomics only.
#include "abom_api.h"
#include "abom_common.h"

namespace {

constexpr int FA_BLOCK = 256;      // threads per block; emit/count: one word each
constexpr int FA_WAVES = FA_BLOCK / 64;
constexpr int FA_RUN_LANE_MAX = 16;  // longer runs are walked by the whole wave
constexpr uint64_t WIN_MASK = 0xFFFFFFFFull;

// number of valid pairs: the device match counter clamped to the buffer
__device__ __forceinline__ long long pair_count(const int* __restrict__ count,
                                                long long cap) {
    const long long c = *count;
    return c < 0 ? 0 : (c < cap ? c : cap);
}

// Calls f(k) for every k in [beg, end) of each lane with `has` set.  Short
// runs stay on their lane; a longer run is walked by all 64 lanes in turn, so
// no lane loops alone over thousands of packages.  Every lane of the wave
// must reach this call.
template <class F>
__device__ __forceinline__ void visit_runs(bool has, long long beg, long long end, F f) {
    const int lane = threadIdx.x & 63;
    const long long len = has ? end - beg : 0;
    if (len > 0 && len <= FA_RUN_LANE_MAX)
        for (long long k = beg; k < end; ++k) f(k);
    uint64_t heavy = __ballot(len > FA_RUN_LANE_MAX);
    while (heavy) {
        const int src = __ffsll((unsigned long long)heavy) - 1;
        heavy &= heavy - 1;
        const long long b = __shfl(beg, src);
        const long long e = __shfl(end, src);
        for (long long k = b + lane; k < e; k += 64) f(k);
    }
}

__global__ __launch_bounds__(FA_BLOCK) void findings_mark_kernel(
        const uint64_t* __restrict__ pairs, const int* __restrict__ count, long long cap,
        const long long* __restrict__ run_off, const long long* __restrict__ perm2,
        long long U, long long P,
        unsigned long long* __restrict__ bitmap, int* __restrict__ row_cnt,
        int* __restrict__ row_tail, int* __restrict__ chain_prev) {
    const long long n = pair_count(count, cap);
    // block-uniform trip count: visit_runs needs whole waves
    for (long long base = (long long)blockIdx.x * FA_BLOCK; base < n;
         base += (long long)gridDim.x * FA_BLOCK) {
        const long long i = base + threadIdx.x;
        bool first = false;
        long long beg = 0, end = 0;
        if (i < n) {
            const long long u = (long long)(pairs[i] >> 32);
            if (u < U) {
                first = atomicAdd(&row_cnt[u], 1) == 0;
                // chain links are pair index + 1; 0 ends the chain
                chain_prev[i] = atomicExch(&row_tail[u], (int)(i + 1));
                if (first) {
                    beg = run_off[u];
                    end = run_off[u + 1];
                }
            } else {
                chain_prev[i] = 0;
            }
        }
        visit_runs(first, beg, end, [&](long long k) {
            const unsigned long long p = (unsigned long long)perm2[k];
            if (p < (unsigned long long)P)
                atomicOr(&bitmap[p >> 6], 1ull << (p & 63));
        });
    }
}

__global__ __launch_bounds__(FA_BLOCK) void findings_rank_kernel(
        const uint64_t* __restrict__ pairs, const int* __restrict__ count, long long cap,
        long long U, const int* __restrict__ row_cnt, const int* __restrict__ row_tail,
        const int* __restrict__ chain_prev, int* __restrict__ rank_of) {
    const long long n = pair_count(count, cap);
    for (long long i = (long long)blockIdx.x * FA_BLOCK + threadIdx.x; i < n;
         i += (long long)gridDim.x * FA_BLOCK) {
        const uint64_t pr = pairs[i];
        const long long u = (long long)(pr >> 32);
        int r = 0;
        const int c = u < U ? row_cnt[u] : 0;
        if (c > 1) {
            const uint64_t wi = pr & WIN_MASK;
            // a chain holds exactly c pairs; the step bound only keeps a
            // corrupted workspace from looping
            int j = row_tail[u];
            for (int step = 0; j != 0 && step < c; ++step, j = chain_prev[j - 1]) {
                const uint64_t wj = pairs[j - 1] & WIN_MASK;
                r += (wj < wi) | ((wj == wi) & (j - 1 < i));
            }
        }
        rank_of[i] = r;
    }
}

// block-wide sums of two counters; the result is valid in thread 0
__device__ __forceinline__ void block_sum2(long long& a, long long& b, long long* lds) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off);
        b += __shfl_down(b, off);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        lds[2 * wave] = a;
        lds[2 * wave + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = b = 0;
        for (int w = 0; w < FA_WAVES; ++w) {
            a += lds[2 * w];
            b += lds[2 * w + 1];
        }
    }
}

// block-wide exclusive scan of two counters (shfl_up ladder per wave, wave
// totals through LDS); `ta`/`tb` return the block totals in every thread
__device__ __forceinline__ void block_exscan2(long long& a, long long& b,
                                              long long& ta, long long& tb,
                                              long long* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long xa = a, xb = b;
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long ya = __shfl_up(xa, off);
        const long long yb = __shfl_up(xb, off);
        if (lane >= off) {
            xa += ya;
            xb += yb;
        }
    }
    if (lane == 63) {
        lds[2 * wave] = xa;
        lds[2 * wave + 1] = xb;
    }
    __syncthreads();
    long long ca = 0, cb = 0;
    ta = tb = 0;
    for (int w = 0; w < FA_WAVES; ++w) {
        if (w < wave) {
            ca += lds[2 * w];
            cb += lds[2 * w + 1];
        }
        ta += lds[2 * w];
        tb += lds[2 * w + 1];
    }
    a = xa - a + ca;
    b = xb - b + cb;
    __syncthreads();  // lds is reused by the caller's next tile
}

__global__ __launch_bounds__(FA_BLOCK) void findings_count_kernel(
        const unsigned long long* __restrict__ bitmap, long long W,
        const int* __restrict__ row_of, const int* __restrict__ row_cnt,
        unsigned int* __restrict__ word_f, long long* __restrict__ block_sums) {
    __shared__ long long lds[2 * FA_WAVES];
    const long long w = (long long)blockIdx.x * FA_BLOCK + threadIdx.x;
    unsigned long long bits = w < W ? bitmap[w] : 0ull;
    long long pc = __popcll(bits), fs = 0;
    while (bits) {
        const int b = __ffsll(bits) - 1;
        bits &= bits - 1;
        fs += row_cnt[row_of[w * 64 + b]];
    }
    if (w < W) word_f[w] = (unsigned int)fs;
    block_sum2(pc, fs, lds);
    if (threadIdx.x == 0) {
        block_sums[2 * (long long)blockIdx.x] = pc;
        block_sums[2 * (long long)blockIdx.x + 1] = fs;
    }
}

// One block: block_sums [nblocks][2] -> exclusive offsets in place;
// totals = {findings, unique packages, raw device match count}.
__global__ __launch_bounds__(FA_BLOCK) void findings_scan_kernel(
        long long* __restrict__ block_sums, long long nblocks,
        const int* __restrict__ count, long long* __restrict__ totals) {
    __shared__ long long lds[2 * FA_WAVES];
    long long carry_p = 0, carry_f = 0;
    for (long long t = 0; t < nblocks; t += FA_BLOCK) {
        const long long idx = t + threadIdx.x;
        long long p = idx < nblocks ? block_sums[2 * idx] : 0;
        long long f = idx < nblocks ? block_sums[2 * idx + 1] : 0;
        long long tp, tf;
        block_exscan2(p, f, tp, tf, lds);
        if (idx < nblocks) {
            block_sums[2 * idx] = p + carry_p;
            block_sums[2 * idx + 1] = f + carry_f;
        }
        carry_p += tp;
        carry_f += tf;
    }
    if (threadIdx.x == 0) {
        totals[0] = carry_f;
        totals[1] = carry_p;
        totals[2] = *count;
    }
}

// The emit step for the block's 256 bitmap words; every thread of the block
// must reach the call.
__device__ __forceinline__ void emit_words(
        const uint64_t* __restrict__ pairs, unsigned long long* __restrict__ bitmap,
        long long W, const int* __restrict__ row_of, const int* __restrict__ row_cnt,
        const int* __restrict__ row_tail, const int* __restrict__ chain_prev,
        const int* __restrict__ rank_of, const unsigned int* __restrict__ word_f,
        const long long* __restrict__ block_off, long long pkg_base,
        long long F, long long NU,
        long long* __restrict__ out_pkg_idx, long long* __restrict__ out_win_idx,
        long long* __restrict__ out_pkg_nodes, long long* __restrict__ out_pos,
        long long* __restrict__ out_uniq64, int* __restrict__ out_uniq32,
        long long* lds) {
    const long long w = (long long)blockIdx.x * FA_BLOCK + threadIdx.x;
    unsigned long long bits = w < W ? bitmap[w] : 0ull;
    long long uo = __popcll(bits), fo = w < W ? word_f[w] : 0;
    long long tp, tf;
    block_exscan2(uo, fo, tp, tf, lds);
    if (!bits) return;
    uo += block_off[2 * (long long)blockIdx.x];
    fo += block_off[2 * (long long)blockIdx.x + 1];
    bitmap[w] = 0ull;  // only this thread reads or writes word w here
    while (bits) {
        const int b = __ffsll(bits) - 1;
        bits &= bits - 1;
        const long long p = w * 64 + b;
        const int u = row_of[p];
        const int c = row_cnt[u];
        const long long node = p + pkg_base;
        if (uo < NU) {
            out_uniq64[uo] = node;
            out_uniq32[uo] = (int)node;
        }
        int j = row_tail[u];
        for (int step = 0; j != 0 && step < c; ++step, j = chain_prev[j - 1]) {
            const int r = rank_of[j - 1];
            const long long at = fo + r;
            if (r < c && at < F) {
                out_pkg_idx[at] = p;
                out_win_idx[at] = (long long)(pairs[j - 1] & WIN_MASK);
                out_pkg_nodes[at] = node;
                out_pos[at] = uo;
            }
        }
        fo += c;
        ++uo;
    }
}

__global__ __launch_bounds__(FA_BLOCK) void findings_emit_kernel(
        const uint64_t* __restrict__ pairs, unsigned long long* __restrict__ bitmap,
        long long W, const int* __restrict__ row_of, const int* __restrict__ row_cnt,
        const int* __restrict__ row_tail, const int* __restrict__ chain_prev,
        const int* __restrict__ rank_of, const unsigned int* __restrict__ word_f,
        const long long* __restrict__ block_off, long long pkg_base,
        long long F, long long NU,
        long long* __restrict__ out_pkg_idx, long long* __restrict__ out_win_idx,
        long long* __restrict__ out_pkg_nodes, long long* __restrict__ out_pos,
        long long* __restrict__ out_uniq64, int* __restrict__ out_uniq32) {
    __shared__ long long lds[2 * FA_WAVES];
    emit_words(pairs, bitmap, W, row_of, row_cnt, row_tail, chain_prev, rank_of, word_f,
               block_off, pkg_base, F, NU, out_pkg_idx, out_win_idx, out_pkg_nodes,
               out_pos, out_uniq64, out_uniq32, lds);
}

// The grid-uniform condition of the sized variants: the totals of
// findings_scan_kernel fit the capacities the host chose before it knew them.
__device__ __forceinline__ bool sized_ok(const long long* __restrict__ totals,
                                         long long F_cap, long long NU_cap, long long cap) {
    const long long n = totals[2];
    return totals[0] <= F_cap && totals[1] <= NU_cap && n >= 0 && n <= cap;
}

// findings_emit_kernel with F and NU read from `totals`.  When they do not
// fit the capacities nothing is read or written beyond `num_sized`, which
// tells the kernels behind this one how many packages were emitted: NU, or 0.
__global__ __launch_bounds__(FA_BLOCK) void findings_emit_sized_kernel(
        const uint64_t* __restrict__ pairs, unsigned long long* __restrict__ bitmap,
        long long W, const int* __restrict__ row_of, const int* __restrict__ row_cnt,
        const int* __restrict__ row_tail, const int* __restrict__ chain_prev,
        const int* __restrict__ rank_of, const unsigned int* __restrict__ word_f,
        const long long* __restrict__ block_off, long long pkg_base,
        const long long* __restrict__ totals, long long F_cap, long long NU_cap,
        long long cap, long long* __restrict__ num_sized,
        long long* __restrict__ out_pkg_idx, long long* __restrict__ out_win_idx,
        long long* __restrict__ out_pkg_nodes, long long* __restrict__ out_pos,
        long long* __restrict__ out_uniq64, int* __restrict__ out_uniq32) {
    __shared__ long long lds[2 * FA_WAVES];
    const bool ok = sized_ok(totals, F_cap, NU_cap, cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) *num_sized = ok ? totals[1] : 0;
    if (!ok) return;
    emit_words(pairs, bitmap, W, row_of, row_cnt, row_tail, chain_prev, rank_of, word_f,
               block_off, pkg_base, totals[0], totals[1], out_pkg_idx, out_win_idx,
               out_pkg_nodes, out_pos, out_uniq64, out_uniq32, lds);
}

__global__ __launch_bounds__(FA_BLOCK) void findings_reset_kernel(
        const uint64_t* __restrict__ pairs, const int* __restrict__ count, long long cap,
        long long U, int* __restrict__ row_cnt, int* __restrict__ row_tail) {
    const long long n = pair_count(count, cap);
    for (long long i = (long long)blockIdx.x * FA_BLOCK + threadIdx.x; i < n;
         i += (long long)gridDim.x * FA_BLOCK) {
        const long long u = (long long)(pairs[i] >> 32);
        if (u < U) {
            row_cnt[u] = 0;
            row_tail[u] = 0;
        }
    }
}

// findings_reset_kernel under the same condition as the sized emit
__global__ __launch_bounds__(FA_BLOCK) void findings_reset_sized_kernel(
        const uint64_t* __restrict__ pairs, const int* __restrict__ count, long long cap,
        long long U, const long long* __restrict__ totals, long long F_cap, long long NU_cap,
        int* __restrict__ row_cnt, int* __restrict__ row_tail) {
    if (!sized_ok(totals, F_cap, NU_cap, cap)) return;
    const long long n = pair_count(count, cap);
    for (long long i = (long long)blockIdx.x * FA_BLOCK + threadIdx.x; i < n;
         i += (long long)gridDim.x * FA_BLOCK) {
        const long long u = (long long)(pairs[i] >> 32);
        if (u < U) {
            row_cnt[u] = 0;
            row_tail[u] = 0;
        }
    }
}

inline long long word_blocks(long long num_packages) {
    const long long W = (num_packages + 63) / 64;
    return (W + FA_BLOCK - 1) / FA_BLOCK;
}

}  // namespace

extern "C" int abom_findings_count(
        const void* pairs, const void* count, long long capacity,
        const void* run_off, const void* perm2, const void* row_of,
        long long num_rows, long long num_packages,
        void* bitmap, void* row_cnt, void* row_tail, void* chain_prev,
        void* rank_of, void* word_f, void* block_sums, void* totals, void* stream) {
    if (num_packages <= 0 || capacity <= 0 || capacity >= (1ll << 31)) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const long long W = (num_packages + 63) / 64;
    const long long nblocks = word_blocks(num_packages);
    if (nblocks >= (1ll << 31)) return (int)hipErrorInvalidValue;
    const int pair_grid = abom::grid_for(capacity, FA_BLOCK);
    hipLaunchKernelGGL(findings_mark_kernel, dim3(pair_grid), dim3(FA_BLOCK), 0, s,
                       (const uint64_t*)pairs, (const int*)count, capacity,
                       (const long long*)run_off, (const long long*)perm2,
                       num_rows, num_packages, (unsigned long long*)bitmap,
                       (int*)row_cnt, (int*)row_tail, (int*)chain_prev);
    hipLaunchKernelGGL(findings_rank_kernel, dim3(pair_grid), dim3(FA_BLOCK), 0, s,
                       (const uint64_t*)pairs, (const int*)count, capacity, num_rows,
                       (const int*)row_cnt, (const int*)row_tail,
                       (const int*)chain_prev, (int*)rank_of);
    hipLaunchKernelGGL(findings_count_kernel, dim3((unsigned)nblocks), dim3(FA_BLOCK), 0, s,
                       (const unsigned long long*)bitmap, W, (const int*)row_of,
                       (const int*)row_cnt, (unsigned int*)word_f, (long long*)block_sums);
    hipLaunchKernelGGL(findings_scan_kernel, dim3(1), dim3(FA_BLOCK), 0, s,
                       (long long*)block_sums, nblocks, (const int*)count,
                       (long long*)totals);
    return (int)hipGetLastError();
}

extern "C" int abom_findings_emit(
        const void* pairs, const void* count, long long capacity,
        const void* row_of, long long num_rows, long long num_packages,
        void* bitmap, void* row_cnt, void* row_tail, const void* chain_prev,
        const void* rank_of, const void* word_f, const void* block_off,
        long long pkg_base, long long num_findings, long long num_unique,
        void* out_pkg_idx, void* out_win_idx, void* out_pkg_nodes, void* out_pos,
        void* out_uniq64, void* out_uniq32, void* stream) {
    if (num_packages <= 0 || capacity <= 0) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const long long W = (num_packages + 63) / 64;
    const long long nblocks = word_blocks(num_packages);
    if (num_findings > 0)
        hipLaunchKernelGGL(findings_emit_kernel, dim3((unsigned)nblocks), dim3(FA_BLOCK), 0, s,
                           (const uint64_t*)pairs, (unsigned long long*)bitmap, W,
                           (const int*)row_of, (const int*)row_cnt, (const int*)row_tail,
                           (const int*)chain_prev, (const int*)rank_of,
                           (const unsigned int*)word_f, (const long long*)block_off,
                           pkg_base, num_findings, num_unique,
                           (long long*)out_pkg_idx, (long long*)out_win_idx,
                           (long long*)out_pkg_nodes, (long long*)out_pos,
                           (long long*)out_uniq64, (int*)out_uniq32);
    hipLaunchKernelGGL(findings_reset_kernel, dim3(abom::grid_for(capacity, FA_BLOCK)),
                       dim3(FA_BLOCK), 0, s,
                       (const uint64_t*)pairs, (const int*)count, capacity, num_rows,
                       (int*)row_cnt, (int*)row_tail);
    return (int)hipGetLastError();
}

extern "C" int abom_findings_emit_sized(
        const void* pairs, const void* count, long long capacity,
        const void* row_of, long long num_rows, long long num_packages,
        void* bitmap, void* row_cnt, void* row_tail, const void* chain_prev,
        const void* rank_of, const void* word_f, const void* block_off,
        long long pkg_base, const void* totals, long long findings_cap, long long unique_cap,
        void* num_sized,
        void* out_pkg_idx, void* out_win_idx, void* out_pkg_nodes, void* out_pos,
        void* out_uniq64, void* out_uniq32, void* stream) {
    if (num_packages <= 0 || capacity <= 0 || findings_cap < 0 || unique_cap < 0)
        return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const long long W = (num_packages + 63) / 64;
    const long long nblocks = word_blocks(num_packages);
    // F is not known here: the kernel always runs, block 0 writes num_sized
    hipLaunchKernelGGL(findings_emit_sized_kernel, dim3((unsigned)nblocks), dim3(FA_BLOCK), 0, s,
                       (const uint64_t*)pairs, (unsigned long long*)bitmap, W,
                       (const int*)row_of, (const int*)row_cnt, (const int*)row_tail,
                       (const int*)chain_prev, (const int*)rank_of,
                       (const unsigned int*)word_f, (const long long*)block_off,
                       pkg_base, (const long long*)totals, findings_cap, unique_cap,
                       capacity, (long long*)num_sized,
                       (long long*)out_pkg_idx, (long long*)out_win_idx,
                       (long long*)out_pkg_nodes, (long long*)out_pos,
                       (long long*)out_uniq64, (int*)out_uniq32);
    hipLaunchKernelGGL(findings_reset_sized_kernel, dim3(abom::grid_for(capacity, FA_BLOCK)),
                       dim3(FA_BLOCK), 0, s,
                       (const uint64_t*)pairs, (const int*)count, capacity, num_rows,
                       (const long long*)totals, findings_cap, unique_cap,
                       (int*)row_cnt, (int*)row_tail);
    return (int)hipGetLastError();
}

// The whole side arm of the step in one call: count phase, totals to the
// host, sized emit and reset, then the blast counts of the emitted packages
// with their two counters to the host.  Nothing here waits for the device.
extern "C" int abom_findings_ahead(
        const void* pairs, const void* count, long long capacity,
        const void* run_off, const void* perm2, const void* row_of,
        long long num_rows, long long num_packages,
        void* bitmap, void* row_cnt, void* row_tail, void* chain_prev,
        void* rank_of, void* word_f, void* block_sums, void* totals, void* host_totals,
        long long pkg_base, long long findings_cap, long long unique_cap, void* num_sized,
        void* out_pkg_idx, void* out_win_idx, void* out_pkg_nodes, void* out_pos,
        void* out_uniq64, void* out_uniq32,
        const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
        const void* reach_off, const void* reach_col, const void* reach_db,
        long long row_base, long long reach_rows,
        const void* node_is_db_cred, const void* node_is_db_tool,
        void* queue, void* counters, void* host_counters,
        void* out_counts, void* out_overflow, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int rc = abom_findings_count(pairs, count, capacity, run_off, perm2, row_of, num_rows,
                                 num_packages, bitmap, row_cnt, row_tail, chain_prev,
                                 rank_of, word_f, block_sums, totals, stream);
    if (rc) return rc;
    ABOM_CHECK(hipMemcpyAsync(host_totals, totals, 3 * sizeof(long long),
                              hipMemcpyDeviceToHost, s));
    rc = abom_findings_emit_sized(pairs, count, capacity, row_of, num_rows, num_packages,
                                  bitmap, row_cnt, row_tail, chain_prev, rank_of, word_f,
                                  block_sums, pkg_base, totals, findings_cap, unique_cap,
                                  num_sized, out_pkg_idx, out_win_idx, out_pkg_nodes,
                                  out_pos, out_uniq64, out_uniq32, stream);
    if (rc) return rc;
    return abom_blast_counts_indexed_sized(
        out_uniq32, num_sized, unique_cap, rev_off, rev_col, rev_et, et_contains,
        reach_off, reach_col, reach_db, row_base, reach_rows, node_is_db_cred,
        node_is_db_tool, queue, counters, host_counters, out_counts, out_overflow, stream);
}
