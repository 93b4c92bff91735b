// Fix-first remediation plan on gfx950: the findings of a step folded per
// (name, version) item, and per matched item the distinct servers that hold
// an install and the distinct union of their agents, creds and tools.
// Semantics: cpu_ref.remediation_plan.  Every output is a count, a max of
// integers or an index, so no order of lanes, waves or atomics can show.
//
// Four entry points, enqueued in this order on one stream:
//
// abom_remediation_fold     one thread per finding into `state`, u32 [I, 8],
//   one 32-byte row per item: {findings, installs, score bits, severity, kev,
//   F - first head finding, slot, cursor}.  Lanes next to each other that hold
//   the same item (the findings of one package are a run) are combined in the
//   wave first; the run's first lane does the atomics.  The wave that finds
//   `findings` at 0 appends the item to `matched`.  counters = {matched
//   items, tier-2 items, pool rounds, matched installs}, copied to pinned
//   host memory: the caller reads them once, sorts `matched` and sizes the
//   outputs.
// abom_remediation_gather   one wave per matched item, ascending: the folded
//   fields move to the outputs and their words of `state` return to 0; the
//   wave then walks the finding run of the item's first package for the
//   distinct windows, the unfixed ones and the largest fixed key.  slot =
//   position + 1 stays for the scatter.
// abom_remediation_scatter  one thread per finding; the head of a package run
//   claims a place in its item's span of `csr_pkgs` through the cursor.
// abom_remediation_union    the two union tiers of abom_union.h (shared with
//   toxic.hip) with three planes: distinct servers, agents, creds and tools
//   per matched item.  Tier 1 also returns slot and cursor to 0: `state`,
//   `pool` and `counters` are all-zero on return.
//
// Preconditions, as EstateEngine.step and build_reach_index give them:
// pkg_idx ascending; the installs of one item carry the same windows; every
// source of a CONTAINS edge has a reach-index row; fewer than 2^31 findings.
//
// CDNA4 notes: tier 1 runs 4 waves per block; LDS per wave = the four caps
// (256 + 256 + 256 + 512 words), a 64-word candidate stage and two 64-word
// segment tables = 1472 words = 5.75 KiB -> 23 KiB per block -> 6 blocks per
// CU fit the 160 KiB LDS (24 of 32 wave slots).  Tier 2 holds a 1024-entry
// server list, 4 KiB per block.

#include "abom_api.h"
#include "abom_union.h"

namespace abom {

constexpr int REMED_SRV_CAP = 256;
constexpr int REMED_AG_CAP = 256;
constexpr int REMED_CR_CAP = 256;
constexpr int REMED_TL_CAP = 512;
// an item with more installs than this skips tier 1: on an estate that
// spreads installs over its servers it would pass the server cap anyway
constexpr int REMED_T1_INSTALLS = 4 * REMED_SRV_CAP;

struct RemedUnion {
    static constexpr int SRV_CAP = REMED_SRV_CAP, AG_CAP = REMED_AG_CAP;
    static constexpr int CR_CAP = REMED_CR_CAP, TL_CAP = REMED_TL_CAP;
    static constexpr int PLANES = 3, T1_INSTALLS = REMED_T1_INSTALLS;
    static constexpr bool ZERO_SLOT = true;
};

enum RemedWord { RW_FINDINGS, RW_INSTALLS, RW_SCORE, RW_SEV, RW_KEV, RW_HEAD,
                 RW_SLOT = UW_SLOT, RW_CURSOR = UW_CURSOR };
enum RemedCounter { RC_MATCHED, RC_QUEUED = UC_QUEUED, RC_ROUNDS = UC_ROUNDS, RC_INSTALLS };
static_assert(RW_HEAD < RW_SLOT && RC_MATCHED < RC_QUEUED && RC_ROUNDS < RC_INSTALLS);

__global__ void __launch_bounds__(256) remed_fold_kernel(
    const long long* __restrict__ pkg_idx, const long long* __restrict__ win_idx,
    const uint32_t* __restrict__ score_bits, long long F,
    const int* __restrict__ item_of, const uint8_t* __restrict__ a_sev,
    const uint8_t* __restrict__ a_kev,
    uint32_t* __restrict__ state, uint32_t* __restrict__ matched,
    unsigned int* __restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long start = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    // wave-uniform trip count: every lane reaches the ballots and shuffles
    for (long long base = start - lane; base < F; base += stride) {
        const long long f = base + lane;
        const bool active = f < F;
        long long pkg = -1;
        bool head = false;
        uint32_t item = 0xFFFFFFFFu, bits = 0, sevkev = 0;
        if (active) {
            pkg = pkg_idx[f];
            head = f == 0 || pkg_idx[f - 1] != pkg;
            item = (uint32_t)item_of[pkg];
            const long long w = win_idx[f];
            // scores are >= 0: the order of the bit patterns is the order of the values
            bits = score_bits[f];
            sevkev = (uint32_t)a_sev[w] | (a_kev[w] ? 0x100u : 0u);
        }
        // runs of neighbouring lanes with one item: [lane, end) for a run's first lane
        const uint32_t left = __shfl_up(item, 1, 64);
        const bool first = active && (lane == 0 || left != item);
        const unsigned long long firsts = __ballot(first);
        const unsigned long long heads = __ballot(head);
        const int n_active = __popcll(__ballot(active));  // the active lanes are a prefix
        const unsigned long long above = firsts & ~((2ull << lane) - 1);
        const int end = above ? __ffsll((long long)above) - 1 : n_active;
        uint32_t mx = bits, sv = sevkev & 0xFFu, kv = sevkev >> 8;
        for (int k = 1; __ballot(first && lane + k < end); ++k) {
            const uint32_t b2 = __shfl_down(bits, k, 64);
            const uint32_t s2 = __shfl_down(sevkev, k, 64);
            if (first && lane + k < end) {
                mx = b2 > mx ? b2 : mx;
                sv = (s2 & 0xFFu) > sv ? (s2 & 0xFFu) : sv;
                kv |= s2 >> 8;
            }
        }
        bool fresh = false;
        if (first) {
            uint32_t* row = state + (size_t)item * UNION_ROW;
            const unsigned long long below_end = end >= 64 ? ~0ull : (1ull << end) - 1;
            const unsigned long long run_heads = heads & below_end & ~((1ull << lane) - 1);
            fresh = atomicAdd(&row[RW_FINDINGS], (uint32_t)(end - lane)) == 0;
            if (run_heads) {
                // pkg_idx ascends: the first head of the run is its smallest package
                const long long f_head = base + __ffsll((long long)run_heads) - 1;
                atomicAdd(&row[RW_INSTALLS], (uint32_t)__popcll(run_heads));
                atomicMax(&row[RW_HEAD], (uint32_t)(F - f_head));
            }
            if (mx) atomicMax(&row[RW_SCORE], mx);
            if (sv) atomicMax(&row[RW_SEV], sv);
            if (kv) atomicOr(&row[RW_KEV], 1u);
        }
        wave_queue_push(fresh, item, matched, &counters[RC_MATCHED], lane);
        wave_count_flag(head, &counters[RC_INSTALLS], lane);
    }
}

__global__ void __launch_bounds__(256) remed_gather_kernel(
    const int* __restrict__ items, long long M,
    const long long* __restrict__ pkg_idx, const long long* __restrict__ win_idx, long long F,
    const uint8_t* __restrict__ w_flags, const long long* __restrict__ w_fixed_hi,
    const long long* __restrict__ w_fixed_lo, uint32_t* __restrict__ state,
    int* __restrict__ out_rep_pkg, int* __restrict__ out_installs, int* __restrict__ out_findings,
    int* __restrict__ out_vulns, uint32_t* __restrict__ out_score, uint8_t* __restrict__ out_sev,
    uint8_t* __restrict__ out_kev, long long* __restrict__ out_fix_hi,
    long long* __restrict__ out_fix_lo, int* __restrict__ out_unfixed) {
    const WaveId w = wave_id(UNION_WAVES);
    const int lane = w.lane;
    for (long long m = w.wave; m < M; m += w.n_waves) {
        uint32_t* row = state + (size_t)items[m] * UNION_ROW;
        const uint32_t n_find = row[RW_FINDINGS], n_inst = row[RW_INSTALLS];
        const uint32_t score = row[RW_SCORE], sev = row[RW_SEV], kev = row[RW_KEV];
        // a matched item has a head finding, so 1 <= row[RW_HEAD] <= F
        long long head = F - (long long)row[RW_HEAD];
        if (head >= F) head = F - 1;
        const long long rep = pkg_idx[head];
        // the finding run of the first package: distinct windows, the unfixed
        // ones, and the largest fixed key as unsigned 128 bits
        int n_vulns = 0, n_unfixed = 0;
        uint64_t fhi = 0, flo = 0;
        for (long long base = head;; base += 64) {
            const long long f = base + lane;
            const bool in = f < F && pkg_idx[f] == rep;
            if (in) {
                const long long win = win_idx[f];
                bool dup = false;
                for (long long g = head; g < f; ++g) dup |= win_idx[g] == win;
                if (!dup) {
                    ++n_vulns;
                    if (w_flags[win] & WF_HAS_FIXED) {
                        const uint64_t hi = (uint64_t)w_fixed_hi[win], lo = (uint64_t)w_fixed_lo[win];
                        if (key_gt(hi, lo, fhi, flo)) { fhi = hi; flo = lo; }
                    } else {
                        ++n_unfixed;
                    }
                }
            }
            if (__ballot(in) != ~0ull) break;
        }
        n_vulns = wave_sum(n_vulns);
        n_unfixed = wave_sum(n_unfixed);
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t hi = (uint64_t)__shfl_down((long long)fhi, off, 64);
            const uint64_t lo = (uint64_t)__shfl_down((long long)flo, off, 64);
            if (key_gt(hi, lo, fhi, flo)) { fhi = hi; flo = lo; }
        }
        if (lane == 0) {
            out_rep_pkg[m] = (int)rep;
            out_installs[m] = (int)n_inst;
            out_findings[m] = (int)n_find;
            out_vulns[m] = n_vulns;
            out_score[m] = score;
            out_sev[m] = (uint8_t)sev;
            out_kev[m] = (uint8_t)kev;
            out_fix_hi[m] = (long long)fhi;
            out_fix_lo[m] = (long long)flo;
            out_unfixed[m] = n_unfixed;
            row[RW_FINDINGS] = 0; row[RW_INSTALLS] = 0; row[RW_SCORE] = 0;
            row[RW_SEV] = 0; row[RW_KEV] = 0; row[RW_HEAD] = 0;
            slot_set(row, m);
        }
    }
}

__global__ void __launch_bounds__(256) remed_scatter_kernel(
    const long long* __restrict__ pkg_idx, long long F, const int* __restrict__ item_of,
    uint32_t* __restrict__ state, const int* __restrict__ items_off, long long M,
    long long n_installs, int* __restrict__ csr_pkgs) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += stride) {
        const long long pkg = pkg_idx[f];
        if (f != 0 && pkg_idx[f - 1] == pkg) continue;
        uint32_t* row = state + (size_t)(uint32_t)item_of[pkg] * UNION_ROW;
        slot_claim(row, items_off, M, n_installs, csr_pkgs, (int)pkg);
    }
}

}  // namespace abom

extern "C" int abom_remediation_cap(int which) {
    switch (which) {
        case 0: return abom::REMED_SRV_CAP;
        case 1: return abom::REMED_AG_CAP;
        case 2: return abom::REMED_CR_CAP;
        case 3: return abom::REMED_TL_CAP;
        case 4: return abom::REMED_T1_INSTALLS;
        default: return -1;
    }
}

extern "C" int abom_remediation_fold(
    const void* pkg_idx, const void* win_idx, const void* scores, long long num_findings,
    const void* item_of, const void* a_severity, const void* a_kev,
    void* state, void* matched, void* counters, void* host_counters, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (num_findings >= (1ll << 31)) return (int)hipErrorInvalidValue;
    if (num_findings > 0) {
        const int block = 256;
        hipLaunchKernelGGL(abom::remed_fold_kernel, dim3(abom::grid_for(num_findings, block)),
                           dim3(block), 0, s,
                           (const long long*)pkg_idx, (const long long*)win_idx,
                           (const uint32_t*)scores, num_findings, (const int*)item_of,
                           (const uint8_t*)a_severity, (const uint8_t*)a_kev,
                           (uint32_t*)state, (uint32_t*)matched, (unsigned int*)counters);
        ABOM_CHECK(hipGetLastError());
    }
    ABOM_CHECK(hipMemcpyAsync(host_counters, counters, 4 * sizeof(unsigned int),
                              hipMemcpyDeviceToHost, s));
    return 0;
}

extern "C" int abom_remediation_gather(
    const void* items, long long num_items,
    const void* pkg_idx, const void* win_idx, long long num_findings,
    const void* w_flags, const void* w_fixed_hi, const void* w_fixed_lo, void* state,
    void* out_rep_pkg, void* out_installs, void* out_findings, void* out_vulns,
    void* out_score, void* out_sev, void* out_kev, void* out_fix_hi, void* out_fix_lo,
    void* out_unfixed, void* stream) {
    if (num_items <= 0) return 0;
    hipLaunchKernelGGL(abom::remed_gather_kernel,
                       dim3(abom::grid_for(num_items, abom::UNION_WAVES)), dim3(256), 0,
                       (hipStream_t)stream,
                       (const int*)items, num_items, (const long long*)pkg_idx,
                       (const long long*)win_idx, num_findings, (const uint8_t*)w_flags,
                       (const long long*)w_fixed_hi, (const long long*)w_fixed_lo,
                       (uint32_t*)state, (int*)out_rep_pkg, (int*)out_installs,
                       (int*)out_findings, (int*)out_vulns, (uint32_t*)out_score,
                       (uint8_t*)out_sev, (uint8_t*)out_kev, (long long*)out_fix_hi,
                       (long long*)out_fix_lo, (int*)out_unfixed);
    return (int)hipGetLastError();
}

extern "C" int abom_remediation_scatter(
    const void* pkg_idx, long long num_findings, const void* item_of, void* state,
    const void* items_off, long long num_items, long long num_installs, void* csr_pkgs,
    void* stream) {
    if (num_findings <= 0 || num_items <= 0) return 0;
    const int block = 256;
    hipLaunchKernelGGL(abom::remed_scatter_kernel, dim3(abom::grid_for(num_findings, block)),
                       dim3(block), 0, (hipStream_t)stream,
                       (const long long*)pkg_idx, num_findings, (const int*)item_of,
                       (uint32_t*)state, (const int*)items_off, num_items, num_installs,
                       (int*)csr_pkgs);
    return (int)hipGetLastError();
}

// The counters reach `host_counters` (pinned, four u32) through a copy on the
// stream, and are zeroed behind it; the caller waits for the copy.
extern "C" int abom_remediation_union(
    const void* items, long long num_items, const void* items_off, const void* csr_pkgs,
    long long pkg_base,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    const void* reach_off, const void* reach_col, long long row_base, long long num_rows,
    long long node_span, void* state, void* queue, void* pool, long long pool_slices,
    void* counters, void* host_counters,
    void* out_servers, void* out_agents, void* out_creds, void* out_tools, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const abom::UnionOut out = {{(int*)out_servers, (int*)out_agents, (int*)out_creds,
                                 (int*)out_tools}};
    const int rc = abom::launch_union_tiers<abom::RemedUnion>(
        items, num_items, items_off, csr_pkgs, pkg_base, rev_off, rev_col, rev_et, et_contains,
        reach_off, reach_col, row_base, num_rows, node_span, state, queue, pool, pool_slices,
        counters, out, s);
    if (rc != 0) return rc;
    ABOM_CHECK(hipMemcpyAsync(host_counters, counters, 4 * sizeof(unsigned int),
                              hipMemcpyDeviceToHost, s));
    ABOM_CHECK(hipMemsetAsync(counters, 0, 4 * sizeof(unsigned int), s));
    return 0;
}
