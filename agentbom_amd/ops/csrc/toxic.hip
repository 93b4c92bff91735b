// Toxic combinations on gfx950: per finding of a step the pattern bits that
// turn a vulnerable package into an incident (creds, KEV, dangerous or
// retrieval tools, a shared server, an advisory across agents) and their
// score, and per matched advisory its findings, packages and the distinct
// servers and agents over all of them.  Semantics: cpu_ref.toxic_combinations.
// Every output is a count, an OR, a max of integers or an index, so no order
// of lanes, waves or atomics can show.
//
// abom_toxic_server_table  one thread per reach-index row, once per caps
//   tensor: table[r] = caps_all | caps_db << 8 | shared << 16, the OR of
//   tool_caps over the row's tools, over its db tools, and whether the row
//   has two or more agents.
// Then five calls per step result, enqueued in this order on one stream:
// abom_toxic_fold     one thread per finding.  The first lane of a package
//   run in the wave walks the package's reverse CONTAINS row once and ORs the
//   server words; the lanes of the run take the result by shuffle.  Writes
//   the finding's bits (all but the multi-agent one) and folds into `state`,
//   u32 [V, 8], one row per advisory: {findings, packages, score bits,
//   severity, kev, patterns, slot, cursor}.  A finding counts a package when
//   no earlier finding of its package run has the same advisory.  The thread
//   that finds `findings` at 0 appends the advisory to `matched`.  counters
//   u32 [16] = {matched advisories, tier-2 advisories, pool rounds, (package,
//   advisory) heads, findings per pattern x 6, multi-agent advisories,
//   findings with a pattern}; the first four are copied to pinned host
//   memory: the caller reads them once, sorts `matched` and sizes the outputs.
// abom_toxic_gather   one thread per matched advisory, ascending: the folded
//   fields move to the outputs, their words return to 0, slot = position + 1.
// abom_toxic_scatter  one thread per finding; a (package, advisory) head
//   claims a place in its advisory's span of `csr_pkgs` through the cursor.
// abom_toxic_union    the two union tiers of abom_union.h (shared with
//   remediation.hip) with one plane: distinct servers and agents per matched
//   advisory.  Tier 1 leaves the slot for the finish.
// abom_toxic_finish   one thread per finding: the multi-agent bit from the
//   advisory's agents, combo_score, and the histogram, reduced in the wave
//   over the thread's whole stride before the atomics; then one thread per
//   matched advisory returns slot and cursor to 0.  All of `counters` goes to
//   the host and is zeroed behind the copy: `state`, `pool` and `counters`
//   are all-zero on return.
//
// Preconditions, as EstateEngine.step and build_reach_index give them:
// pkg_idx ascending; every source of a CONTAINS edge has a reach-index row;
// scores >= 0; fewer than 2^31 findings.  A finding whose window or advisory
// is out of range is left without bits and folded nowhere.
//
// CDNA4 notes: tier 1 runs 4 waves per block; LDS per wave = 256 + 256 set
// words, a 64-word candidate stage and two 64-word segment tables = 704 words
// = 2.75 KiB -> 11 KiB per block.  Tier 2 holds a 1024-entry server list.

#include "abom_api.h"
#include "abom_union.h"

namespace abom {

constexpr int TOXIC_SRV_CAP = 256;
constexpr int TOXIC_AG_CAP = 256;
// an advisory with more packages than this skips tier 1
constexpr int TOXIC_T1_PKGS = 4 * TOXIC_SRV_CAP;
constexpr int TOXIC_COUNTERS = 16;

struct ToxicUnion {
    static constexpr int SRV_CAP = TOXIC_SRV_CAP, AG_CAP = TOXIC_AG_CAP;
    static constexpr int PLANES = 1, T1_INSTALLS = TOXIC_T1_PKGS;
    static constexpr bool ZERO_SLOT = false;  // toxic_finish_kernel reads the slot
};

// mirrors of cpu_ref.TC_* and cpu_ref.TP_*
constexpr uint32_t TC_EXEC = 1, TC_WRITE = 2, TC_DELETE = 4, TC_RETRIEVAL = 16;
constexpr uint32_t TC_DANGEROUS = TC_EXEC | TC_WRITE | TC_DELETE;
constexpr uint32_t TP_CRED_BLAST = 1, TP_KEV_WITH_CREDS = 2, TP_EXECUTE_EXPLOIT = 4;
constexpr uint32_t TP_CACHE_POISON = 8, TP_LATERAL_CHAIN = 16, TP_MULTI_AGENT_CVE = 32;
constexpr uint32_t TOXIC_HOT_SEVERITY = 4;
constexpr int TOXIC_MULTI_AGENTS = 3;

enum ToxicWord { TW_FINDINGS, TW_PKGS, TW_SCORE, TW_SEV, TW_KEV, TW_PAT,
                 TW_SLOT = UW_SLOT, TW_CURSOR = UW_CURSOR };
enum ToxicCounter { XC_MATCHED, XC_QUEUED = UC_QUEUED, XC_ROUNDS = UC_ROUNDS, XC_HEADS, XC_HIST,
                    XC_MULTI = XC_HIST + 6, XC_ANY };
static_assert(TW_PAT < TW_SLOT && XC_MATCHED < XC_QUEUED && XC_ROUNDS < XC_HEADS);

__global__ void __launch_bounds__(256) toxic_server_table_kernel(
    const int4* __restrict__ reach_off, const uint32_t* __restrict__ reach_col, long long num_rows,
    const uint8_t* __restrict__ tool_caps, const uint8_t* __restrict__ tool_is_db,
    long long tool_base, long long n_tools, uint32_t* __restrict__ table) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < num_rows; r += stride) {
        const int4 off = reach_off[r];
        uint32_t all = 0, db = 0;
        for (int t = off.z; t < off.w; ++t) {
            const long long k = (long long)reach_col[t] - tool_base;
            if (k < 0 || k >= n_tools) continue;  // not a tool of the caps table
            const uint32_t c = tool_caps[k];
            all |= c;
            if (tool_is_db[k]) db |= c;
        }
        table[r] = all | db << 8 | (off.y - off.x >= 2 ? 1u << 16 : 0u);
    }
}

struct ToxicFindings {
    const long long* pkg_idx;
    const long long* win_idx;
    long long F;
    const int* vuln_of;  // nullable: the identity map
    long long W, V;      // windows, advisories
};

// the advisory of finding f, or -1 when its window or advisory is out of range
__device__ __forceinline__ long long toxic_vuln(const ToxicFindings& fs, long long f) {
    const long long w = fs.win_idx[f];
    if (w < 0 || w >= fs.W) return -1;
    const long long v = fs.vuln_of ? (long long)fs.vuln_of[w] : w;
    return v >= 0 && v < fs.V ? v : -1;
}

// no earlier finding of the package run of f has advisory v: runs are short
__device__ __forceinline__ bool toxic_head(const ToxicFindings& fs, long long f, long long pkg,
                                           long long v) {
    for (long long g = f - 1; g >= 0 && fs.pkg_idx[g] == pkg; --g)
        if (toxic_vuln(fs, g) == v) return false;
    return true;
}

__global__ void __launch_bounds__(256) toxic_fold_kernel(
    ToxicFindings fs, const uint32_t* __restrict__ score_bits, const int* __restrict__ n_creds,
    const uint8_t* __restrict__ a_sev, const uint8_t* __restrict__ a_kev,
    const uint8_t* __restrict__ a_impact, const uint8_t* __restrict__ tool_lut,
    const uint64_t* __restrict__ rev_off, const uint32_t* __restrict__ rev_col,
    const uint8_t* __restrict__ rev_et, uint8_t et_contains, long long pkg_base,
    const uint32_t* __restrict__ table, uint32_t row_base, uint32_t num_rows,
    uint32_t* __restrict__ state, uint32_t* __restrict__ matched,
    unsigned int* __restrict__ counters, uint8_t* __restrict__ out_patterns) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long start = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    // wave-uniform trip count: every lane reaches the ballots and shuffles
    for (long long base = start - lane; base < fs.F; base += stride) {
        const long long f = base + lane;
        const bool active = f < fs.F;
        const long long pkg = active ? fs.pkg_idx[f] : -1;
        // the package run inside the wave: its first lane walks the servers
        const long long left = __shfl_up(pkg, 1, 64);
        const bool first = active && (lane == 0 || left != pkg);
        uint32_t word = 0;
        if (first) {
            const long long node = pkg_base + pkg;
            for (uint64_t e = rev_off[node]; e < rev_off[node + 1]; ++e) {
                if (rev_et[e] != et_contains) continue;
                const uint32_t r = rev_col[e] - row_base;
                if (r < num_rows) word |= table[r];
            }
        }
        const unsigned long long firsts = __ballot(first) & ((2ull << lane) - 1);
        word = __shfl(word, firsts ? 63 - __clzll((long long)firsts) : 0, 64);

        const long long v = active ? toxic_vuln(fs, f) : -1;
        uint32_t bits = 0;
        bool fresh = false, head = false;
        if (v >= 0) {
            const long long w = fs.win_idx[f];
            const uint32_t sev = a_sev[w];
            const bool kev = a_kev[w] != 0, hot = sev >= TOXIC_HOT_SEVERITY;
            const bool creds = n_creds[f] > 0;
            const uint32_t cls = tool_lut[a_impact[w]];
            const uint32_t exposed = cls == 2 ? word & 0xFFu : cls == 1 ? (word >> 8) & 0xFFu : 0u;
            if (hot && creds) bits |= TP_CRED_BLAST;
            if (kev && creds) bits |= TP_KEV_WITH_CREDS;
            if (hot && (exposed & TC_DANGEROUS)) bits |= TP_EXECUTE_EXPLOIT;
            if (hot && (exposed & TC_RETRIEVAL)) bits |= TP_CACHE_POISON;
            if (hot && (word >> 16 & 1u)) bits |= TP_LATERAL_CHAIN;
            head = toxic_head(fs, f, pkg, v);
            uint32_t* row = state + (size_t)v * UNION_ROW;
            fresh = atomicAdd(&row[TW_FINDINGS], 1u) == 0;
            if (head) atomicAdd(&row[TW_PKGS], 1u);
            // scores are >= 0: the order of the bit patterns is the order of the values
            const uint32_t sb = score_bits[f];
            if (sb) atomicMax(&row[TW_SCORE], sb);
            if (sev) atomicMax(&row[TW_SEV], sev);
            if (kev) atomicOr(&row[TW_KEV], 1u);
            if (bits) atomicOr(&row[TW_PAT], bits);
        }
        if (active) out_patterns[f] = (uint8_t)bits;
        wave_queue_push(fresh, (uint32_t)v, matched, &counters[XC_MATCHED], lane);
        wave_count_flag(head, &counters[XC_HEADS], lane);
    }
}

__global__ void __launch_bounds__(256) toxic_gather_kernel(
    const int* __restrict__ vulns, long long M, uint32_t* __restrict__ state,
    int* __restrict__ out_findings, int* __restrict__ out_packages,
    uint32_t* __restrict__ out_score, uint8_t* __restrict__ out_sev, uint8_t* __restrict__ out_kev,
    uint8_t* __restrict__ out_patterns) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += stride) {
        uint32_t* row = state + (size_t)vulns[m] * UNION_ROW;
        out_findings[m] = (int)row[TW_FINDINGS];
        out_packages[m] = (int)row[TW_PKGS];
        out_score[m] = row[TW_SCORE];
        out_sev[m] = (uint8_t)row[TW_SEV];
        out_kev[m] = (uint8_t)row[TW_KEV];
        out_patterns[m] = (uint8_t)row[TW_PAT];
        row[TW_FINDINGS] = 0; row[TW_PKGS] = 0; row[TW_SCORE] = 0;
        row[TW_SEV] = 0; row[TW_KEV] = 0; row[TW_PAT] = 0;
        slot_set(row, m);
    }
}

__global__ void __launch_bounds__(256) toxic_scatter_kernel(
    ToxicFindings fs, uint32_t* __restrict__ state, const int* __restrict__ vulns_off,
    long long M, long long n_heads, int* __restrict__ csr_pkgs) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < fs.F; f += stride) {
        const long long v = toxic_vuln(fs, f);
        if (v < 0) continue;
        const long long pkg = fs.pkg_idx[f];
        if (!toxic_head(fs, f, pkg, v)) continue;
        uint32_t* row = state + (size_t)v * UNION_ROW;
        slot_claim(row, vulns_off, M, n_heads, csr_pkgs, (int)pkg);
    }
}

// min(s * mult, 10) for a score > 0, else the pattern's default: one fp32
// multiply and a min, nothing to contract
__device__ __forceinline__ float toxic_score(float s, float mult, float dflt) {
    return s > 0.0f ? fminf(s * mult, 10.0f) : dflt;
}

__global__ void __launch_bounds__(256) toxic_finish_kernel(
    ToxicFindings fs, const uint32_t* __restrict__ score_bits,
    const uint32_t* __restrict__ state, long long M, const int* __restrict__ v_agents,
    const uint32_t* __restrict__ v_score, uint8_t* __restrict__ patterns,
    float* __restrict__ combo_score, unsigned int* __restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long start = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned hist[6] = {0, 0, 0, 0, 0, 0}, any = 0;  // wave-uniform
    for (long long base = start - lane; base < fs.F; base += stride) {
        const long long f = base + lane;
        uint32_t bits = 0;
        if (f < fs.F) {
            bits = patterns[f];
            float m_score = 0.0f;
            const long long v = toxic_vuln(fs, f);
            if (v >= 0) {
                long long m;
                if (slot_get(state + (size_t)v * UNION_ROW, M, m) &&
                    v_agents[m] >= TOXIC_MULTI_AGENTS) {
                    bits |= TP_MULTI_AGENT_CVE;
                    m_score = __uint_as_float(v_score[m]);
                }
            }
            const float s = __uint_as_float(score_bits[f]);
            float best = 0.0f;
            if (bits & TP_CRED_BLAST) best = fmaxf(best, toxic_score(s, 1.5f, 9.0f));
            if (bits & TP_KEV_WITH_CREDS) best = fmaxf(best, 10.0f);
            if (bits & TP_EXECUTE_EXPLOIT) best = fmaxf(best, toxic_score(s, 1.3f, 8.5f));
            if (bits & TP_CACHE_POISON) best = fmaxf(best, toxic_score(s, 1.5f, 9.5f));
            if (bits & TP_LATERAL_CHAIN) best = fmaxf(best, toxic_score(s, 1.4f, 9.0f));
            if (bits & TP_MULTI_AGENT_CVE) best = fmaxf(best, toxic_score(m_score, 1.2f, 7.5f));
            patterns[f] = (uint8_t)bits;
            combo_score[f] = best;
        }
        for (int b = 0; b < 6; ++b) hist[b] += (unsigned)__popcll(__ballot(bits >> b & 1u));
        any += (unsigned)__popcll(__ballot(bits != 0));
    }
    if (lane == 0) {
        for (int b = 0; b < 6; ++b)
            if (hist[b]) atomicAdd(&counters[XC_HIST + b], hist[b]);
        if (any) atomicAdd(&counters[XC_ANY], any);
    }
}

__global__ void __launch_bounds__(256) toxic_close_kernel(
    const int* __restrict__ vulns, long long M, uint32_t* __restrict__ state,
    const int* __restrict__ v_agents, uint8_t* __restrict__ v_patterns,
    unsigned int* __restrict__ counters) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long start = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long base = start - lane; base < M; base += stride) {
        const long long m = base + lane;
        bool multi = false;
        if (m < M) {
            uint32_t* row = state + (size_t)vulns[m] * UNION_ROW;
            slot_clear(row);
            multi = v_agents[m] >= TOXIC_MULTI_AGENTS;
            if (multi) v_patterns[m] |= (uint8_t)TP_MULTI_AGENT_CVE;
        }
        wave_count_flag(multi, &counters[XC_MULTI], lane);
    }
}

static ToxicFindings toxic_findings(const void* pkg_idx, const void* win_idx, long long F,
                                    const void* vuln_of, long long W, long long V) {
    ToxicFindings fs;
    fs.pkg_idx = (const long long*)pkg_idx;
    fs.win_idx = (const long long*)win_idx;
    fs.F = F;
    fs.vuln_of = (const int*)vuln_of;
    fs.W = W;
    fs.V = V;
    return fs;
}

}  // namespace abom

extern "C" int abom_toxic_cap(int which) {
    switch (which) {
        case 0: return abom::TOXIC_SRV_CAP;
        case 1: return abom::TOXIC_AG_CAP;
        case 2: return abom::TOXIC_T1_PKGS;
        default: return -1;
    }
}

extern "C" int abom_toxic_server_table(
    const void* reach_off, const void* reach_col, long long num_rows,
    const void* tool_caps, const void* tool_is_db, long long tool_base, long long num_tools,
    void* table, void* stream) {
    if (num_rows <= 0) return 0;
    const int block = 256;
    hipLaunchKernelGGL(abom::toxic_server_table_kernel, dim3(abom::grid_for(num_rows, block)),
                       dim3(block), 0, (hipStream_t)stream,
                       (const int4*)reach_off, (const uint32_t*)reach_col, num_rows,
                       (const uint8_t*)tool_caps, (const uint8_t*)tool_is_db, tool_base,
                       num_tools, (uint32_t*)table);
    return (int)hipGetLastError();
}

extern "C" int abom_toxic_fold(
    const void* pkg_idx, const void* win_idx, const void* scores, const void* n_creds,
    long long num_findings, const void* vuln_of, long long num_windows, long long num_vulns,
    const void* a_severity, const void* a_kev, const void* a_impact, const void* tool_lut,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    long long pkg_base, const void* table, long long row_base, long long num_rows,
    void* state, void* matched, void* counters, void* host_counters, void* out_patterns,
    void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (num_findings >= (1ll << 31) || num_vulns >= (1ll << 31)) return (int)hipErrorInvalidValue;
    if (num_findings > 0) {
        const int block = 256;
        hipLaunchKernelGGL(abom::toxic_fold_kernel, dim3(abom::grid_for(num_findings, block)),
                           dim3(block), 0, s,
                           abom::toxic_findings(pkg_idx, win_idx, num_findings, vuln_of,
                                                num_windows, num_vulns),
                           (const uint32_t*)scores, (const int*)n_creds,
                           (const uint8_t*)a_severity, (const uint8_t*)a_kev,
                           (const uint8_t*)a_impact, (const uint8_t*)tool_lut,
                           (const uint64_t*)rev_off, (const uint32_t*)rev_col,
                           (const uint8_t*)rev_et, (uint8_t)et_contains, pkg_base,
                           (const uint32_t*)table, (uint32_t)row_base, (uint32_t)num_rows,
                           (uint32_t*)state, (uint32_t*)matched, (unsigned int*)counters,
                           (uint8_t*)out_patterns);
        ABOM_CHECK(hipGetLastError());
    }
    ABOM_CHECK(hipMemcpyAsync(host_counters, counters, 4 * sizeof(unsigned int),
                              hipMemcpyDeviceToHost, s));
    return 0;
}

extern "C" int abom_toxic_gather(
    const void* vulns, long long num_matched, void* state,
    void* out_findings, void* out_packages, void* out_score, void* out_sev, void* out_kev,
    void* out_patterns, void* stream) {
    if (num_matched <= 0) return 0;
    const int block = 256;
    hipLaunchKernelGGL(abom::toxic_gather_kernel, dim3(abom::grid_for(num_matched, block)),
                       dim3(block), 0, (hipStream_t)stream,
                       (const int*)vulns, num_matched, (uint32_t*)state, (int*)out_findings,
                       (int*)out_packages, (uint32_t*)out_score, (uint8_t*)out_sev,
                       (uint8_t*)out_kev, (uint8_t*)out_patterns);
    return (int)hipGetLastError();
}

extern "C" int abom_toxic_scatter(
    const void* pkg_idx, const void* win_idx, long long num_findings,
    const void* vuln_of, long long num_windows, long long num_vulns, void* state,
    const void* vulns_off, long long num_matched, long long num_heads, void* csr_pkgs,
    void* stream) {
    if (num_findings <= 0 || num_matched <= 0) return 0;
    const int block = 256;
    hipLaunchKernelGGL(abom::toxic_scatter_kernel, dim3(abom::grid_for(num_findings, block)),
                       dim3(block), 0, (hipStream_t)stream,
                       abom::toxic_findings(pkg_idx, win_idx, num_findings, vuln_of, num_windows,
                                            num_vulns),
                       (uint32_t*)state, (const int*)vulns_off, num_matched, num_heads,
                       (int*)csr_pkgs);
    return (int)hipGetLastError();
}

extern "C" int abom_toxic_union(
    long long num_matched, const void* vulns_off, const void* csr_pkgs, long long pkg_base,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    const void* reach_off, const void* reach_col, long long row_base, long long num_rows,
    long long node_span, void* queue, void* pool, long long pool_slices, void* counters,
    void* out_servers, void* out_agents, void* stream) {
    const abom::UnionOut out = {{(int*)out_servers, (int*)out_agents, nullptr, nullptr}};
    // tier 1 leaves the slots alone: no items, no state
    return abom::launch_union_tiers<abom::ToxicUnion>(
        nullptr, num_matched, vulns_off, csr_pkgs, pkg_base, rev_off, rev_col, rev_et,
        et_contains, reach_off, reach_col, row_base, num_rows, node_span, nullptr, queue, pool,
        pool_slices, counters, out, (hipStream_t)stream);
}

// All sixteen counters reach `host_counters` (pinned) through a copy on the
// stream, and are zeroed behind it; the caller waits for the copy.
extern "C" int abom_toxic_finish(
    const void* pkg_idx, const void* win_idx, const void* scores, long long num_findings,
    const void* vuln_of, long long num_windows, long long num_vulns,
    const void* vulns, long long num_matched, void* state,
    const void* v_agents, const void* v_score, void* v_patterns,
    void* patterns, void* combo_score, void* counters, void* host_counters, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int block = 256;
    if (num_findings > 0) {
        hipLaunchKernelGGL(abom::toxic_finish_kernel, dim3(abom::grid_for(num_findings, block)),
                           dim3(block), 0, s,
                           abom::toxic_findings(pkg_idx, win_idx, num_findings, vuln_of,
                                                num_windows, num_vulns),
                           (const uint32_t*)scores, (const uint32_t*)state, num_matched,
                           (const int*)v_agents, (const uint32_t*)v_score, (uint8_t*)patterns,
                           (float*)combo_score, (unsigned int*)counters);
        ABOM_CHECK(hipGetLastError());
    }
    if (num_matched > 0) {
        hipLaunchKernelGGL(abom::toxic_close_kernel, dim3(abom::grid_for(num_matched, block)),
                           dim3(block), 0, s,
                           (const int*)vulns, num_matched, (uint32_t*)state, (const int*)v_agents,
                           (uint8_t*)v_patterns, (unsigned int*)counters);
        ABOM_CHECK(hipGetLastError());
    }
    ABOM_CHECK(hipMemcpyAsync(host_counters, counters,
                              abom::TOXIC_COUNTERS * sizeof(unsigned int),
                              hipMemcpyDeviceToHost, s));
    ABOM_CHECK(hipMemsetAsync(counters, 0, abom::TOXIC_COUNTERS * sizeof(unsigned int), s));
    return 0;
}
