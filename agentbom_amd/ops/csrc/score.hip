// Risk scoring and rollup reductions: the risk-score formula (plain and
// fused with the per-finding gathers) and the per-container severity
// histogram.

#include <string.h>

#include "abom_api.h"
#include "abom_common.h"

namespace abom {

// ── Risk-score kernel ──────────────────────────────────────────────────────
// Implements models/blast.py risk_score_from_counts exactly (f32): the CPU
// formula is the specification; parity is asserted in tests/test_ops_gpu.py.

struct RiskWeights {
    float base_critical, base_high, base_medium, base_low;
    float agent_w, agent_cap, cred_w, cred_cap, tool_w, tool_cap;
    float ai_boost, kev_boost, epss_boost, epss_threshold;
    float sc_t1, sc_b1, sc_t2, sc_b2, sc_t3, sc_b3;
    float reach_boost, unreach_penalty;
};

// weights22 is the host float vector of native.risk_weights_array(), in the
// field order above.
static RiskWeights load_weights(const float* weights22) {
    static_assert(sizeof(RiskWeights) == 22 * sizeof(float), "RiskWeights is 22 packed floats");
    RiskWeights w;
    memcpy(&w, weights22, sizeof(w));
    return w;
}

__device__ __forceinline__ float score_one(
    uint8_t sev, uint32_t n_agents, uint32_t n_creds, uint32_t n_tools,
    uint8_t f, float epss, float scorecard, int8_t reach, const RiskWeights& w) {
    if (f & 4u) return 0.0f;  // suppressed / VEX
    float base = 0.0f;
    switch (sev) {
        case 5: base = w.base_critical; break;
        case 4: base = w.base_high; break;
        case 3: base = w.base_medium; break;
        case 2: base = w.base_low; break;
        default: base = 0.0f;
    }
    const float af = fminf((float)n_agents * w.agent_w, w.agent_cap);
    const float cf = fminf((float)n_creds * w.cred_w, w.cred_cap);
    const float tf = fminf((float)n_tools * w.tool_w, w.tool_cap);
    const int ai_signals = (int)(f & 1u) + (n_creds > 0) + (n_tools > 0);
    const float ai = ai_signals >= 2 ? w.ai_boost : 0.0f;
    const float kev = (f & 2u) ? w.kev_boost : 0.0f;
    const float ep = (epss >= w.epss_threshold) ? w.epss_boost : 0.0f;
    float sc = 0.0f;
    if (scorecard >= 0.0f) {
        if (scorecard < w.sc_t1) sc = w.sc_b1;
        else if (scorecard < w.sc_t2) sc = w.sc_b2;
        else if (scorecard < w.sc_t3) sc = w.sc_b3;
    }
    float ra = 0.0f;
    if (reach == 1) ra = w.reach_boost;
    else if (reach == 0) ra = -w.unreach_penalty;
    return fmaxf(0.0f, fminf(base + af + cf + tf + ai + kev + ep + sc + ra, 10.0f));
}

// Fused per-finding gather + score: replaces the ~14-op torch chain
// (arena gathers, CWE-impact LUT classification, count selection,
// reachability compare, score) with one pass.
__global__ void score_gather_kernel(
    const long long* __restrict__ win_idx,    // [n] -> arena window rows
    const long long* __restrict__ pkg_nodes,  // [n] -> global node ids
    const long long* __restrict__ pos,        // [n] -> rows into counts2d
    const uint8_t* __restrict__ a_sev,        // [W]
    const uint8_t* __restrict__ a_kev,        // [W]
    const float* __restrict__ a_epss,         // [W]
    const uint8_t* __restrict__ a_impact,     // [W]
    const uint8_t* __restrict__ cred_lut,     // [9]
    const uint8_t* __restrict__ tool_lut,     // [9]
    const int* __restrict__ counts2d,         // [U*6]
    const uint32_t* __restrict__ dist,        // [N]
    float* __restrict__ out_scores,
    int* __restrict__ out_agents,
    int* __restrict__ out_creds,
    int* __restrict__ out_tools,
    long long n, RiskWeights w) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const long long wrow = win_idx[i];
        const long long crow = pos[i] * 6;
        const uint8_t impact = a_impact[wrow];
        const uint8_t ccls = cred_lut[impact];
        const uint8_t tcls = tool_lut[impact];
        const int n_creds = ccls == 2 ? counts2d[crow + 2]
                          : ccls == 1 ? counts2d[crow + 3] : 0;
        const int n_tools = tcls == 2 ? counts2d[crow + 4]
                          : tcls == 1 ? counts2d[crow + 5] : 0;
        const int n_agents = counts2d[crow + 1];
        const uint8_t flags = (uint8_t)(a_kev[wrow] ? 2u : 0u);
        const int8_t reach = dist[pkg_nodes[i]] != ABOM_UNVISITED ? 1 : 0;
        out_scores[i] = score_one(a_sev[wrow], (uint32_t)n_agents,
                                  (uint32_t)n_creds, (uint32_t)n_tools, flags,
                                  a_epss[wrow], -1.0f, reach, w);
        out_agents[i] = n_agents;
        out_creds[i] = n_creds;
        out_tools[i] = n_tools;
    }
}

__global__ void risk_score_kernel(
    const uint8_t* __restrict__ severity,     // SEVERITY_CODE (5=crit..2=low)
    const uint32_t* __restrict__ n_agents,
    const uint32_t* __restrict__ n_creds,
    const uint32_t* __restrict__ n_tools,
    const uint8_t* __restrict__ flags,        // bit0 ai_ctx, bit1 kev, bit2 suppressed
    const float* __restrict__ epss,           // <0 => none
    const float* __restrict__ scorecard,      // <0 => none
    const int8_t* __restrict__ reach,         // -1 unknown / 0 unreachable / 1 reachable
    float* __restrict__ out,
    long long n, RiskWeights w) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        out[i] = score_one(severity[i], n_agents[i], n_creds[i], n_tools[i],
                           flags[i], epss[i], scorecard[i], reach[i], w);
    }
}

// ── Segmented reductions for rollup ────────────────────────────────────────
// Per-finding severity scatter into per-container histograms (6 severity
// buckets) — container.rollup's descendant aggregates.
__global__ void severity_histogram_kernel(
    const uint32_t* __restrict__ owner,       // [F] container index per finding
    const uint8_t* __restrict__ severity,     // [F] SEVERITY_CODE
    unsigned int* __restrict__ hist,          // [C * 6]
    long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        atomicAdd(&hist[(long long)owner[i] * 6 + severity[i]], 1u);
    }
}

}  // namespace abom

extern "C" int abom_risk_score(
    const void* severity, const void* n_agents, const void* n_creds, const void* n_tools,
    const void* flags, const void* epss, const void* scorecard, const void* reach,
    void* out, long long n, const float* weights22, void* stream) {
    const int block = 256;
    hipLaunchKernelGGL(abom::risk_score_kernel, dim3(abom::grid_for(n, block)), dim3(block), 0,
                       (hipStream_t)stream, (const uint8_t*)severity, (const uint32_t*)n_agents,
                       (const uint32_t*)n_creds, (const uint32_t*)n_tools, (const uint8_t*)flags,
                       (const float*)epss, (const float*)scorecard, (const int8_t*)reach,
                       (float*)out, n, abom::load_weights(weights22));
    return (int)hipGetLastError();
}

extern "C" int abom_score_gather(
    const void* win_idx, const void* pkg_nodes, const void* pos,
    const void* a_sev, const void* a_kev, const void* a_epss, const void* a_impact,
    const void* cred_lut, const void* tool_lut, const void* counts2d,
    const void* dist, void* out_scores, void* out_agents, void* out_creds,
    void* out_tools, long long n, const float* weights22, void* stream) {
    const int block = 256;
    hipLaunchKernelGGL(abom::score_gather_kernel, dim3(abom::grid_for(n, block)),
                       dim3(block), 0, (hipStream_t)stream,
                       (const long long*)win_idx, (const long long*)pkg_nodes,
                       (const long long*)pos, (const uint8_t*)a_sev,
                       (const uint8_t*)a_kev, (const float*)a_epss,
                       (const uint8_t*)a_impact, (const uint8_t*)cred_lut,
                       (const uint8_t*)tool_lut, (const int*)counts2d,
                       (const uint32_t*)dist, (float*)out_scores,
                       (int*)out_agents, (int*)out_creds, (int*)out_tools, n,
                       abom::load_weights(weights22));
    return (int)hipGetLastError();
}

extern "C" int abom_severity_histogram(
    const void* owner, const void* severity, void* hist, long long n, void* stream) {
    const int block = 256;
    hipLaunchKernelGGL(abom::severity_histogram_kernel, dim3(abom::grid_for(n, block)),
                       dim3(block), 0, (hipStream_t)stream, (const uint32_t*)owner,
                       (const uint8_t*)severity, (unsigned int*)hist, n);
    return (int)hipGetLastError();
}
