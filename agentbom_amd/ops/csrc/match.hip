// Bulk OSV/GHSA version-range matching on gfx950.
//
// Replaces the reference's per-(package, advisory-window) Python hot loop
// (reference: src/agent_bom/scanners/package_scan.py:694-803 window walk,
// src/agent_bom/db/lookup.py:549 batch lookup + Python version filtering)
// with one kernel over the whole package batch against a GPU-resident
// columnar advisory arena.
//
// Arena model: advisory windows for all ecosystems live in
// HBM as sorted columnar arrays grouped by group_key = hash64(ecosystem,
// normalized_name).  One row per window — multi-branch advisories keep one
// row per (introduced, fixed, last_affected) triple, never collapsed.
//
// Matching semantics (fail-closed):
// - introduced "0"/missing  -> window has no lower bound (WF_HAS_INTRO off)
// - fixed is exclusive, last_affected inclusive
// - commit-SHA / unencodable bounds  -> WF_CPU_FALLBACK, never matched here;
//   the host resolves those windows with the exact CPU comparator
// - packages with unencodable versions are skipped (PF_ENCODABLE off) and
//   resolved on the host the same way.
//
// Three kernels answer the same question, which (row, window) pairs match:
//
// match_kernel: each thread owns one package row: binary-search the sorted
// group_key array (top of the tree stays L2/L3-resident; skipped when the
// caller hands in precomputed window ranges), then walk that group's
// windows testing the row's u128 key against each window's bounds.  It needs
// nothing but the rows and the arena, so it serves native.match, the
// non-dedup and distributed engines and every caller without a search table;
// on the dedup path of EstateEngine.step it runs when
// AGENT_BOM_MATCH_BY_WINDOW=0.
//
// match_by_window_kernel: each thread owns one WINDOW.  The distinct rows of
// a group, sorted by unsigned (hi, lo) key in a search table built once with
// the engine (graph/gpu_engine.py::build_match_search_table), make a
// window's match set a contiguous run of rows: two or three binary searches
// find its ends, where the row kernel tests every (row, window) pair of the
// group.  Every key-against-bound comparison still happens in the kernel,
// every step; the table only joins rows to groups by name.  Selected by
// AGENT_BOM_MATCH_TILED=0.
//
// match_by_window_tiled_kernel: the same searches, one block per tile of 256
// consecutive windows.  Windows are stored group by group and the table's
// runs follow the groups, so the rows a tile searches are one short
// contiguous slice of s_key: the block copies up to MT_CAP rows of it into
// LDS with coalesced 16-byte loads and the searches probe LDS, not global
// memory (a probe outside the staged slice reads global memory, so nothing
// rests on the order of the runs).  All of a window's columns are loaded
// ahead of the flag tests, and a block reserves its pairs with one atomic.
// The default of EstateEngine.step whenever the estate has a dedup layout.
//
// All append matches through a device atomic cursor as
// (row_idx << 32 | window_idx), in no particular order; the caller sorts the
// pairs, or hands them to the finding assembly, which needs no order.

#include "abom_api.h"
#include "abom_common.h"

namespace abom {

__global__ void match_kernel(
    const uint64_t* __restrict__ pkg_group_key,   // [P] hash64(eco, name)
    const uint64_t* __restrict__ pkg_key_hi,      // [P]
    const uint64_t* __restrict__ pkg_key_lo,      // [P]
    const uint8_t* __restrict__ pkg_flags,        // [P]
    long long num_packages,
    const uint64_t* __restrict__ group_keys,      // [G] sorted ascending
    const uint32_t* __restrict__ group_off,       // [G+1] -> window ranges
    long long num_groups,
    const uint64_t* __restrict__ w_intro_hi,      // [W]
    const uint64_t* __restrict__ w_intro_lo,
    const uint64_t* __restrict__ w_fixed_hi,
    const uint64_t* __restrict__ w_fixed_lo,
    const uint64_t* __restrict__ w_last_hi,
    const uint64_t* __restrict__ w_last_lo,
    const uint8_t* __restrict__ w_flags,
    const uint64_t* __restrict__ w_packed,        // [W*8] AoS 64B/window (nullable)
    const uint32_t* __restrict__ pkg_wbeg,        // [P] precomputed ranges
    const uint32_t* __restrict__ pkg_wend,        //     (nullable)
    const int* __restrict__ p_order,              // [P] heavy-first schedule
    uint64_t* __restrict__ out_pairs,             // [capacity]
    unsigned int* __restrict__ out_count,
    long long capacity) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < num_packages;
         i += stride) {
        // Heavy-first schedule: rows are visited in window-count-descending
        // order (stable, so same-group rows stay wave-adjacent and the
        // cooperative walk still fires).  The zipf-head walks start FIRST
        // and the tail of the grid is all tiny rows — without this the
        // kernel ends with a handful of live waves grinding the head
        // groups (PMC: 17.8% achieved occupancy, stall-free VALU idle).
        const long long p = p_order ? (long long)p_order[i] : i;
        const bool enc = (pkg_flags[p] & PF_ENCODABLE) != 0;
        uint32_t wbeg, wend;
        if (pkg_wbeg) {
            // resident-estate serving mode: the engine precomputes each
            // package's window range once at build (the estate and arena
            // are static between steps) — two coalesced u32 loads replace
            // the per-leader binary search over the (L1-spilling at 2M
            // windows / 482k groups) group-key tree.
            if (!enc) continue;
            wbeg = pkg_wbeg[p];
            wend = pkg_wend[p];
            if (wbeg >= wend) continue;
        } else {
            const uint64_t gkey = enc ? pkg_group_key[p] : 0;

            // Packages are laid out sorted by group key (engine build), so
            // most lanes in a wave share their key with a predecessor: only
            // segment LEADERS run the binary search; followers copy the
            // result via a leader-index max-scan + shuffle (wave64
            // segmented broadcast).
            const uint64_t prev_key = __shfl_up(gkey, 1, 64);
            const bool leader = (lane == 0) || (gkey != prev_key) || !enc;
            long long found = -1;
            if (leader && enc) {
                long long lo = 0, hi = num_groups;
                while (lo < hi) {
                    long long mid = (lo + hi) >> 1;
                    if (group_keys[mid] < gkey) lo = mid + 1; else hi = mid;
                }
                found = (lo < num_groups && group_keys[lo] == gkey) ? lo : -1;
            }
            // inclusive max-scan of leader lane indices -> my segment leader
            int leader_lane = leader ? lane : -1;
            #pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                int up = __shfl_up(leader_lane, off, 64);
                if (lane >= off && up > leader_lane) leader_lane = up;
            }
            found = __shfl(found, leader_lane, 64);
            if (!enc || found < 0) continue;
            wbeg = group_off[found];
            wend = group_off[found + 1];
        }
        const uint64_t khi = pkg_key_hi[p];
        const uint64_t klo = pkg_key_lo[p];

        // Cooperative wave walk: when the whole wave shares one window
        // range (zipf-head groups under the sorted/dedup layouts, where
        // the walk cost concentrates), each WINDOW is loaded once by one
        // lane (coalesced across lanes) and broadcast by shuffle — 64x
        // less L1 traffic than every lane re-walking the same run.
        const uint32_t wbeg0 = (uint32_t)__shfl((int)wbeg, 0, 64);
        const uint32_t wend0 = (uint32_t)__shfl((int)wend, 0, 64);
        const unsigned long long same =
            __ballot(wbeg == wbeg0 && wend == wend0);
        if (same == ~0ull && wend - wbeg >= 16) {
            for (uint32_t base = wbeg; base < wend; base += 64) {
                const uint32_t w = base + lane;
                uint8_t f = 0;
                uint64_t ihi = 0, ilo = 0, fhi = 0, flo = 0, lhi = 0, llo = 0;
                if (w < wend) {
                    f = w_flags[w];
                    ihi = w_intro_hi[w]; ilo = w_intro_lo[w];
                    fhi = w_fixed_hi[w]; flo = w_fixed_lo[w];
                    lhi = w_last_hi[w];  llo = w_last_lo[w];
                }
                const int nwin = (int)min((uint32_t)64, wend - base);
                for (int j = 0; j < nwin; ++j) {
                    const uint8_t fj = (uint8_t)__shfl((int)f, j, 64);
                    if (fj & (WF_CPU_FALLBACK | WF_UNFIXED_SUPPRESSED)) continue;
                    const uint64_t jihi = __shfl(ihi, j, 64), jilo = __shfl(ilo, j, 64);
                    const uint64_t jfhi = __shfl(fhi, j, 64), jflo = __shfl(flo, j, 64);
                    const uint64_t jlhi = __shfl(lhi, j, 64), jllo = __shfl(llo, j, 64);
                    if ((fj & WF_HAS_INTRO) && key_lt(khi, klo, jihi, jilo)) continue;
                    if ((fj & WF_HAS_FIXED) && key_ge(khi, klo, jfhi, jflo)) continue;
                    if ((fj & WF_HAS_LAST) && key_gt(khi, klo, jlhi, jllo)) continue;
                    const unsigned idx = atomicAdd(out_count, 1u);
                    if ((long long)idx < capacity) {
                        out_pairs[idx] = ((uint64_t)p << 32) | (uint64_t)(base + j);
                    }
                }
            }
            continue;
        }

        if (w_packed) {
            // AoS walk: one 64-byte line per window
            for (uint32_t w = wbeg; w < wend; ++w) {
                const uint64_t* rec = w_packed + (uint64_t)w * 8;
                const uint8_t f = (uint8_t)rec[6];
                if (f & (WF_CPU_FALLBACK | WF_UNFIXED_SUPPRESSED)) continue;
                if ((f & WF_HAS_INTRO) && key_lt(khi, klo, rec[0], rec[1])) continue;
                if ((f & WF_HAS_FIXED) && key_ge(khi, klo, rec[2], rec[3])) continue;
                if ((f & WF_HAS_LAST) && key_gt(khi, klo, rec[4], rec[5])) continue;
                const unsigned idx = atomicAdd(out_count, 1u);
                if ((long long)idx < capacity) {
                    out_pairs[idx] = ((uint64_t)p << 32) | (uint64_t)w;
                }
            }
            continue;
        }
        for (uint32_t w = wbeg; w < wend; ++w) {
            const uint8_t f = w_flags[w];
            if (f & (WF_CPU_FALLBACK | WF_UNFIXED_SUPPRESSED)) continue;
            if ((f & WF_HAS_INTRO) && key_lt(khi, klo, w_intro_hi[w], w_intro_lo[w])) continue;
            if ((f & WF_HAS_FIXED) && key_ge(khi, klo, w_fixed_hi[w], w_fixed_lo[w])) continue;
            if ((f & WF_HAS_LAST) && key_gt(khi, klo, w_last_hi[w], w_last_lo[w])) continue;
            const unsigned idx = atomicAdd(out_count, 1u);
            if ((long long)idx < capacity) {
                out_pairs[idx] = ((uint64_t)p << 32) | (uint64_t)w;
            }
        }
    }
}

// First row in [lo, hi) whose key is >= (bhi, blo), or > it when `after`.
// Probes are one 16-byte load each; the rows of the run ascend by key.
__device__ __forceinline__ uint32_t row_bound(const ulonglong2* __restrict__ s_key,
                                              uint32_t lo, uint32_t hi,
                                              uint64_t bhi, uint64_t blo, bool after) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const ulonglong2 k = s_key[mid];  // x = hi word, y = lo word
        const bool before = after ? !key_lt(bhi, blo, k.x, k.y) : key_lt(k.x, k.y, bhi, blo);
        if (before) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One thread per advisory window.  [w_rbeg[w], w_rend[w]) is the run of the
// window's group in the search table (s_key ascending within the run,
// s_row the row's index in the dedup layout); an empty run means that no
// encodable estate row carries the group's name.
__global__ void match_by_window_kernel(
    const uint64_t* __restrict__ w_intro_hi,      // [W]
    const uint64_t* __restrict__ w_intro_lo,
    const uint64_t* __restrict__ w_fixed_hi,
    const uint64_t* __restrict__ w_fixed_lo,
    const uint64_t* __restrict__ w_last_hi,
    const uint64_t* __restrict__ w_last_lo,
    const uint8_t* __restrict__ w_flags,
    const uint32_t* __restrict__ w_rbeg,          // [W]
    const uint32_t* __restrict__ w_rend,          // [W]
    long long num_windows,
    const ulonglong2* __restrict__ s_key,         // [R] (hi, lo)
    const int* __restrict__ s_row,                // [R]
    uint64_t* __restrict__ out_pairs,             // [capacity]
    unsigned int* __restrict__ out_count,
    long long capacity) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < num_windows;
         w += stride) {
        const uint8_t f = w_flags[w];
        if (f & (WF_CPU_FALLBACK | WF_UNFIXED_SUPPRESSED)) continue;
        const uint32_t rbeg = w_rbeg[w], rend = w_rend[w];
        if (rbeg >= rend) continue;
        // intro inclusive, fixed exclusive, last inclusive.  The end searches
        // start at `begin`: a bound below it gives end == begin, the same
        // empty result as its true position further left.
        uint32_t begin = rbeg, end = rend;
        if (f & WF_HAS_INTRO)
            begin = row_bound(s_key, rbeg, rend, w_intro_hi[w], w_intro_lo[w], false);
        if (f & WF_HAS_FIXED)
            end = row_bound(s_key, begin, end, w_fixed_hi[w], w_fixed_lo[w], false);
        if (f & WF_HAS_LAST)
            end = row_bound(s_key, begin, end, w_last_hi[w], w_last_lo[w], true);
        if (begin >= end) continue;
        // one reservation for the whole run; the count keeps growing past
        // capacity (the caller relaunches), the stores do not
        const uint32_t n = end - begin;
        const unsigned base = atomicAdd(out_count, n);
        for (uint32_t j = 0; j < n; ++j) {
            if ((long long)base + j < capacity) {
                out_pairs[(long long)base + j] =
                    ((uint64_t)(uint32_t)s_row[begin + j] << 32) | (uint64_t)w;
            }
        }
    }
}

constexpr int MT_TILE = 256;   // windows per block, one per thread
constexpr int MT_CAP = 1024;   // rows staged per tile: 16 KiB of LDS, ten blocks per CU

// row_bound over a run of which rows [slo, slo + nst) are staged in `tile`;
// a probe outside them reads s_key.  The unsigned difference also sends a
// probe below slo to global memory.
__device__ __forceinline__ uint32_t row_bound_staged(
    const ulonglong2* tile, uint32_t slo, uint32_t nst,
    const ulonglong2* __restrict__ s_key, uint32_t lo, uint32_t hi,
    uint64_t bhi, uint64_t blo, bool after) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const uint32_t at = mid - slo;
        const ulonglong2 k = at < nst ? tile[at] : s_key[mid];
        const bool before = after ? !key_lt(bhi, blo, k.x, k.y) : key_lt(k.x, k.y, bhi, blo);
        if (before) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One block per tile of MT_TILE consecutive windows, thread t owns window
// tile * MT_TILE + t.  Same arguments and same pairs as
// match_by_window_kernel.
__global__ __launch_bounds__(MT_TILE) void match_by_window_tiled_kernel(
    const uint64_t* __restrict__ w_intro_hi,      // [W]
    const uint64_t* __restrict__ w_intro_lo,
    const uint64_t* __restrict__ w_fixed_hi,
    const uint64_t* __restrict__ w_fixed_lo,
    const uint64_t* __restrict__ w_last_hi,
    const uint64_t* __restrict__ w_last_lo,
    const uint8_t* __restrict__ w_flags,
    const uint32_t* __restrict__ w_rbeg,          // [W]
    const uint32_t* __restrict__ w_rend,          // [W]
    long long num_windows,
    const ulonglong2* __restrict__ s_key,         // [R] (hi, lo)
    const int* __restrict__ s_row,                // [R]
    uint64_t* __restrict__ out_pairs,             // [capacity]
    unsigned int* __restrict__ out_count,
    long long capacity) {
    __shared__ ulonglong2 tile[MT_CAP];
    __shared__ uint32_t wave_lo[MT_TILE / 64], wave_hi[MT_TILE / 64], wave_n[MT_TILE / 64];
    __shared__ unsigned block_base;
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * MT_TILE + threadIdx.x;

    // every column of the window at once: nine independent loads, none
    // behind a flag test
    uint8_t f = WF_CPU_FALLBACK;
    uint32_t rbeg = 0, rend = 0;
    uint64_t ihi = 0, ilo = 0, fhi = 0, flo = 0, lhi = 0, llo = 0;
    if (w < num_windows) {
        f = w_flags[w];
        rbeg = w_rbeg[w]; rend = w_rend[w];
        ihi = w_intro_hi[w]; ilo = w_intro_lo[w];
        fhi = w_fixed_hi[w]; flo = w_fixed_lo[w];
        lhi = w_last_hi[w];  llo = w_last_lo[w];
    }
    const bool searches = !(f & (WF_CPU_FALLBACK | WF_UNFIXED_SUPPRESSED)) && rbeg < rend;

    // the tile's row slice: min rbeg .. max rend over the lanes that search
    uint32_t slo = searches ? rbeg : 0xFFFFFFFFu;
    uint32_t shi = searches ? rend : 0u;
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        slo = min(slo, (uint32_t)__shfl_xor((int)slo, off, 64));
        shi = max(shi, (uint32_t)__shfl_xor((int)shi, off, 64));
    }
    if (lane == 0) {
        wave_lo[threadIdx.x >> 6] = slo;
        wave_hi[threadIdx.x >> 6] = shi;
    }
    __syncthreads();
    #pragma unroll
    for (int i = 0; i < MT_TILE / 64; ++i) {
        slo = min(slo, wave_lo[i]);
        shi = max(shi, wave_hi[i]);
    }
    const uint32_t nst = slo < shi ? min(shi - slo, (uint32_t)MT_CAP) : 0u;
    for (uint32_t i = threadIdx.x; i < nst; i += MT_TILE) tile[i] = s_key[slo + i];
    __syncthreads();

    // intro inclusive, fixed exclusive, last inclusive; the end searches
    // start at `begin`, as in match_by_window_kernel
    uint32_t n = 0, begin = rbeg;
    if (searches) {
        uint32_t end = rend;
        if (f & WF_HAS_INTRO)
            begin = row_bound_staged(tile, slo, nst, s_key, rbeg, rend, ihi, ilo, false);
        if (f & WF_HAS_FIXED)
            end = row_bound_staged(tile, slo, nst, s_key, begin, end, fhi, flo, false);
        if (f & WF_HAS_LAST)
            end = row_bound_staged(tile, slo, nst, s_key, begin, end, lhi, llo, true);
        if (begin < end) n = end - begin;
    }

    // one reservation per block: every atomic on out_count is a request to
    // one address, and those are served one after the other whatever number
    // of lanes each carries.  Inclusive prefix sum of the run lengths per
    // wave, the waves' totals through LDS, thread 0 adds the block's total
    // and hands the base to the others.  The count keeps growing past
    // capacity (the caller relaunches), the stores do not.
    uint32_t incl = n;
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, off, 64);
        if (lane >= off) incl += up;
    }
    if (lane == 63) wave_n[threadIdx.x >> 6] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        #pragma unroll
        for (int i = 0; i < MT_TILE / 64; ++i) total += wave_n[i];
        block_base = total ? atomicAdd(out_count, total) : 0u;
    }
    __syncthreads();
    uint32_t before = incl - n;
    for (int i = 0; i < (int)(threadIdx.x >> 6); ++i) before += wave_n[i];
    const long long base = (long long)block_base + before;
    for (uint32_t j = 0; j < n; ++j) {
        if (base + j < capacity) {
            out_pairs[base + j] = ((uint64_t)(uint32_t)s_row[begin + j] << 32) | (uint64_t)w;
        }
    }
}

}  // namespace abom

namespace abom {
// Match-specific grid: zipf-head advisory groups make per-package work
// highly variable, so give the scheduler FINE work units (many more
// workgroups than resident waves) instead of the default 2048-block
// grid-stride — the hardware queue load-balances the long walks.
inline int match_grid_for(long long work, int block) {
    long long blocks = (work + block - 1) / block;
    if (blocks > 16384) blocks = 16384;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}
}  // namespace abom

extern "C" int abom_match(
    const void* pkg_group_key, const void* pkg_key_hi, const void* pkg_key_lo,
    const void* pkg_flags, long long num_packages,
    const void* group_keys, const void* group_off, long long num_groups,
    const void* w_intro_hi, const void* w_intro_lo,
    const void* w_fixed_hi, const void* w_fixed_lo,
    const void* w_last_hi, const void* w_last_lo,
    const void* w_flags,
    const void* w_packed,                        // nullable AoS windows
    const void* pkg_wbeg, const void* pkg_wend,  // nullable precomputed ranges
    const void* p_order,                         // nullable heavy-first order
    void* out_pairs, void* out_count, long long capacity, void* stream) {
    const int block = 256;
    const int grid = abom::match_grid_for(num_packages, block);
    hipLaunchKernelGGL(abom::match_kernel, dim3(grid), dim3(block), 0, (hipStream_t)stream,
                       (const uint64_t*)pkg_group_key, (const uint64_t*)pkg_key_hi,
                       (const uint64_t*)pkg_key_lo, (const uint8_t*)pkg_flags, num_packages,
                       (const uint64_t*)group_keys, (const uint32_t*)group_off, num_groups,
                       (const uint64_t*)w_intro_hi, (const uint64_t*)w_intro_lo,
                       (const uint64_t*)w_fixed_hi, (const uint64_t*)w_fixed_lo,
                       (const uint64_t*)w_last_hi, (const uint64_t*)w_last_lo,
                       (const uint8_t*)w_flags,
                       (const uint64_t*)w_packed,
                       (const uint32_t*)pkg_wbeg, (const uint32_t*)pkg_wend,
                       (const int*)p_order,
                       (uint64_t*)out_pairs,
                       (unsigned int*)out_count, capacity);
    return (int)hipGetLastError();
}

extern "C" int abom_match_by_window(
    const void* w_intro_hi, const void* w_intro_lo,
    const void* w_fixed_hi, const void* w_fixed_lo,
    const void* w_last_hi, const void* w_last_lo,
    const void* w_flags,
    const void* w_rbeg, const void* w_rend, long long num_windows,
    const void* s_key, const void* s_row,
    void* out_pairs, void* out_count, long long capacity, void* stream) {
    const int block = 256;
    const int grid = abom::grid_for(num_windows, block);
    hipLaunchKernelGGL(abom::match_by_window_kernel, dim3(grid), dim3(block), 0,
                       (hipStream_t)stream,
                       (const uint64_t*)w_intro_hi, (const uint64_t*)w_intro_lo,
                       (const uint64_t*)w_fixed_hi, (const uint64_t*)w_fixed_lo,
                       (const uint64_t*)w_last_hi, (const uint64_t*)w_last_lo,
                       (const uint8_t*)w_flags,
                       (const uint32_t*)w_rbeg, (const uint32_t*)w_rend, num_windows,
                       (const ulonglong2*)s_key, (const int*)s_row,
                       (uint64_t*)out_pairs, (unsigned int*)out_count, capacity);
    return (int)hipGetLastError();
}

extern "C" int abom_match_by_window_tiled(
    const void* w_intro_hi, const void* w_intro_lo,
    const void* w_fixed_hi, const void* w_fixed_lo,
    const void* w_last_hi, const void* w_last_lo,
    const void* w_flags,
    const void* w_rbeg, const void* w_rend, long long num_windows,
    const void* s_key, const void* s_row,
    void* out_pairs, void* out_count, long long capacity, void* stream) {
    if (num_windows <= 0) return 0;
    // one tile per block: the blocks are short and retire as they finish, so
    // work queued on other streams finds wave slots while the match runs
    const long long tiles = (num_windows + abom::MT_TILE - 1) / abom::MT_TILE;
    hipLaunchKernelGGL(abom::match_by_window_tiled_kernel, dim3((unsigned)tiles),
                       dim3(abom::MT_TILE), 0, (hipStream_t)stream,
                       (const uint64_t*)w_intro_hi, (const uint64_t*)w_intro_lo,
                       (const uint64_t*)w_fixed_hi, (const uint64_t*)w_fixed_lo,
                       (const uint64_t*)w_last_hi, (const uint64_t*)w_last_lo,
                       (const uint8_t*)w_flags,
                       (const uint32_t*)w_rbeg, (const uint32_t*)w_rend, num_windows,
                       (const ulonglong2*)s_key, (const int*)s_row,
                       (uint64_t*)out_pairs, (unsigned int*)out_count, capacity);
    return (int)hipGetLastError();
}
