// The C ABI of _abom_gpu.so: every exported entry point, declared once.
// Every csrc/*.hip file includes this header, so a definition that drifts
// from its prototype stops compiling (C linkage cannot overload).
// ops/native.py::_SIGNATURES mirrors it line for line for ctypes;
// tests/test_native_abi.py parses this file to hold the two together.
//
// Device buffers travel as void* / const void*, counts as long long, `stream`
// is a hipStream_t, and unless noted the int result is a hipError_t.  Only
// void*, const void*, long long, unsigned int, int, double and const float*
// appear as parameter types.
#pragma once

#ifdef __cplusplus
extern "C" {
#endif

// abom_api.hip
int abom_abi_version();
int abom_device_count();
const char* abom_error_string(int code);

// match.hip (w_packed, pkg_wbeg/pkg_wend and p_order are nullable)
int abom_match(
    const void* pkg_group_key, const void* pkg_key_hi, const void* pkg_key_lo,
    const void* pkg_flags, long long num_packages,
    const void* group_keys, const void* group_off, long long num_groups,
    const void* w_intro_hi, const void* w_intro_lo, const void* w_fixed_hi, const void* w_fixed_lo,
    const void* w_last_hi, const void* w_last_lo, const void* w_flags, const void* w_packed,
    const void* pkg_wbeg, const void* pkg_wend, const void* p_order,
    void* out_pairs, void* out_count, long long capacity, void* stream);
// one thread per window over the row search table (s_key int64 [R,2], s_row
// int32 [R]; [w_rbeg, w_rend) is a window's run of rows); same pair output
int abom_match_by_window(
    const void* w_intro_hi, const void* w_intro_lo, const void* w_fixed_hi, const void* w_fixed_lo,
    const void* w_last_hi, const void* w_last_lo, const void* w_flags,
    const void* w_rbeg, const void* w_rend, long long num_windows,
    const void* s_key, const void* s_row,
    void* out_pairs, void* out_count, long long capacity, void* stream);
// the same match, one block per tile of 256 windows with the tile's slice of
// s_key staged in LDS; same arguments, same pair output
int abom_match_by_window_tiled(
    const void* w_intro_hi, const void* w_intro_lo, const void* w_fixed_hi, const void* w_fixed_lo,
    const void* w_last_hi, const void* w_last_lo, const void* w_flags,
    const void* w_rbeg, const void* w_rend, long long num_windows,
    const void* s_key, const void* s_row,
    void* out_pairs, void* out_count, long long capacity, void* stream);

// bfs.hip (abom_bfs_run, abom_bfs_run_ex and abom_bfs_run_indexed return the
// number of levels run or a negated hipError_t)
int abom_bfs_expand(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* frontier, long long frontier_size, void* dist, unsigned int next_level,
    void* next_frontier, void* next_count, void* heavy_queue, void* heavy_count,
    void* next_degree_sum, long long capacity, void* stream);
int abom_bfs_expand_heavy(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* heavy_queue, const void* heavy_size_ptr, void* dist, unsigned int next_level,
    void* next_frontier, void* next_count, void* next_degree_sum, long long capacity,
    void* stream);
int abom_bfs_expand_edges(
    const void* edge_src, const void* col, const void* etype, unsigned int allowed_mask,
    long long num_edges, const void* row_off, void* dist, unsigned int cur_level,
    void* next_frontier, void* next_count, void* next_degree_sum, int build_frontier,
    long long capacity, void* stream);
int abom_bfs_run(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* sources, long long n_sources, void* dist, long long num_nodes,
    void* frontier_a, void* frontier_b, void* heavy_queue, void* counters,
    int max_levels, const void* edge_src, long long num_edges, double avg_degree,
    const void* rev_off, const void* rev_col, const void* rev_et, void* stream);
// abom_bfs_begin enqueues the dist fill, the counter zeroing and the seeding
// without a sync; abom_bfs_run_ex runs the levels (and the begin part unless
// begun != 0).  sources_degree < 0: read the sources' degree sum from the
// device; host_counters: pinned host u32[4] for the count reads, nullable
int abom_bfs_begin(
    const void* row_off, const void* sources, long long n_sources, void* dist,
    long long num_nodes, void* frontier_a, void* counters, void* stream);
int abom_bfs_run_ex(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* sources, long long n_sources, void* dist, long long num_nodes,
    void* frontier_a, void* frontier_b, void* heavy_queue, void* counters,
    int max_levels, const void* edge_src, long long num_edges,
    const void* rev_off, const void* rev_col, const void* rev_et,
    int begun, long long sources_degree, void* host_counters, void* stream);
// the parent index of the bottom-up pass, built once per (reverse CSR,
// allowed_mask): first_parent u32 [num_nodes] = 0xFFFFFFFF for a vertex
// without an allowed in-edge, else the source of the first allowed in-edge of
// its reverse row in bits 0-30 and bit 31 set when the row holds another
// allowed in-edge; num_nodes >= 2^31 - 1 is refused (hipErrorInvalidValue)
int abom_bfs_parent_index(
    const void* rev_off, const void* rev_col, const void* rev_et, unsigned int allowed_mask,
    long long num_nodes, void* first_parent, void* stream);
// one bottom-up pass at cur_level over the reverse rows, or over the parent
// index with the rows behind it: *next_count += vertices claimed, *open_count
// += vertices left unvisited that have an allowed in-edge
int abom_bfs_bottom_up(
    const void* rev_off, const void* rev_col, const void* rev_et, unsigned int allowed_mask,
    long long num_nodes, void* dist, unsigned int cur_level,
    void* next_count, void* open_count, void* stream);
int abom_bfs_bottom_up_indexed(
    const void* rev_off, const void* rev_col, const void* rev_et, unsigned int allowed_mask,
    long long num_nodes, void* dist, unsigned int cur_level, const void* first_parent,
    void* next_count, void* open_count, void* stream);
// abom_bfs_run_ex with the parent index of (rev, allowed_mask) for its
// bottom-up levels; first_parent is nullable (then it is abom_bfs_run_ex)
int abom_bfs_run_indexed(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* sources, long long n_sources, void* dist, long long num_nodes,
    void* frontier_a, void* frontier_b, void* heavy_queue, void* counters,
    int max_levels, const void* edge_src, long long num_edges,
    const void* rev_off, const void* rev_col, const void* rev_et, const void* first_parent,
    int begun, long long sources_degree, void* host_counters, void* stream);

// reach_sets.hip (one pass of per-source reach for n_sources <= 64 * words
// sources, words in 1..4: hops u8 [T, hops_stride] gets the hop count of
// source j at column col_base + j of every target row it reaches within
// max_depth, clamped to [0, 254], and is otherwise left as the caller filled
// it; seen, cur and nxt are u64 [num_nodes * words], cur and nxt all-zero on
// entry and on return; the three queues are u32 [num_nodes * words];
// counters is device u32 [2]; host_counters is pinned host u32 [2], nullable.
// Returns the number of levels run or a negated hipError_t)
int abom_reach_hops(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* sources, int n_sources, int words, long long num_nodes,
    const void* target_slot, void* hops, long long hops_stride, long long col_base,
    int max_depth,
    void* seen, void* cur, void* nxt, void* queue_a, void* queue_b, void* heavy_queue,
    void* counters, void* host_counters, void* stream);

// query.hip
int abom_impact_query(
    const void* row_off, const void* col, const void* etype, unsigned int allowed_mask,
    const void* query_sources, int num_queries, int max_hops, int max_nodes_per_query,
    void* out_nodes, void* out_hops, void* out_counts, void* out_truncated, void* stream);

// score.hip
int abom_risk_score(
    const void* severity, const void* n_agents, const void* n_creds, const void* n_tools,
    const void* flags, const void* epss, const void* scorecard, const void* reach,
    void* out, long long n, const float* weights22, void* stream);
int abom_score_gather(
    const void* win_idx, const void* pkg_nodes, const void* pos,
    const void* a_sev, const void* a_kev, const void* a_epss, const void* a_impact,
    const void* cred_lut, const void* tool_lut, const void* counts2d,
    const void* dist, void* out_scores, void* out_agents, void* out_creds,
    void* out_tools, long long n, const float* weights22, void* stream);
int abom_severity_histogram(
    const void* owner, const void* severity, void* hist, long long n, void* stream);

// blast.hip (the indexed entry point reads the per-server reach index and
// leaves {queued packages, overflowed rows} in counters)
int abom_blast_counts(
    const void* pkgs, long long n,
    const void* rev_off, const void* rev_col, const void* rev_et,
    const void* fwd_off, const void* fwd_col, const void* fwd_et,
    int et_contains, int et_uses, int et_cred, int et_tool,
    const void* node_is_db_cred, const void* node_is_db_tool,
    void* out_counts, void* out_overflow, void* stream);
int abom_blast_counts_indexed(
    const void* pkgs, long long n,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    const void* reach_off, const void* reach_col, const void* reach_db,
    long long row_base, long long num_rows,
    const void* node_is_db_cred, const void* node_is_db_tool,
    void* queue, void* counters, void* out_counts, void* out_overflow, void* stream);
// the indexed passes over at most n_cap packages: the count is the device
// long long n_dev; the counters are also copied to host_counters (pinned u32[2])
int abom_blast_counts_indexed_sized(
    const void* pkgs, const void* n_dev, long long n_cap,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    const void* reach_off, const void* reach_col, const void* reach_db,
    long long row_base, long long num_rows,
    const void* node_is_db_cred, const void* node_is_db_tool,
    void* queue, void* counters, void* host_counters,
    void* out_counts, void* out_overflow, void* stream);

// blast_hops.hip (multi-hop delegation expansion per package from the reach
// index and the agent index: out_hop_agents int32 [n,4] = |A_h| for h = 2..5,
// out_creds int32 [n], out_depth u8 [n], out_overflow u8 [n]; counters is
// {queued packages, overflowed rows}; max_depth is clamped to [1, 5].
// abom_blast_hops_cap returns a cap of the wave kernel, not a hipError_t:
// 0 = visited servers, 1 = visited agents, 2 = credentials, else -1)
int abom_blast_hops_cap(int which);
int abom_blast_hops(
    const void* pkgs, long long n,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    const void* reach_off, const void* reach_col, long long row_base, long long num_rows,
    const void* agent_off, const void* agent_srv, long long num_agents, int max_depth,
    void* queue, void* counters,
    void* out_hop_agents, void* out_creds, void* out_depth, void* out_overflow, void* stream);
// the same over at most n_cap packages: the count is the device long long
// n_dev; the counters are also copied to host_counters (pinned u32[2])
int abom_blast_hops_sized(
    const void* pkgs, const void* n_dev, long long n_cap,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    const void* reach_off, const void* reach_col, long long row_base, long long num_rows,
    const void* agent_off, const void* agent_srv, long long num_agents, int max_depth,
    void* queue, void* counters, void* host_counters,
    void* out_hop_agents, void* out_creds, void* out_depth, void* out_overflow, void* stream);

// remediation.hip (the remediation plan per (name, version) item, four calls
// on one stream: state is u32 [items, 8], pool u32 [pool_slices *
// ((num_rows + 31) / 32 + 3 * ((node_span + 31) / 32))], counters u32 [4] =
// {matched items, tier-2 items, pool rounds, matched installs}, all three
// all-zero on entry and after abom_remediation_union; host_counters is pinned
// host u32 [4], written by the fold and again by the union.  pkg_idx and
// win_idx are int64 [num_findings], pkg_idx ascending; items is the sorted
// `matched` list, items_off the exclusive prefix of out_installs with the
// total at [num_items].  abom_remediation_cap returns a cap of the wave
// kernel, not a hipError_t: 0 = servers, 1 = agents, 2 = creds, 3 = tools,
// 4 = the install count above which an item skips the wave kernel, else -1)
int abom_remediation_cap(int which);
int abom_remediation_fold(
    const void* pkg_idx, const void* win_idx, const void* scores, long long num_findings,
    const void* item_of, const void* a_severity, const void* a_kev,
    void* state, void* matched, void* counters, void* host_counters, void* stream);
int abom_remediation_gather(
    const void* items, long long num_items,
    const void* pkg_idx, const void* win_idx, long long num_findings,
    const void* w_flags, const void* w_fixed_hi, const void* w_fixed_lo, void* state,
    void* out_rep_pkg, void* out_installs, void* out_findings, void* out_vulns,
    void* out_score, void* out_sev, void* out_kev, void* out_fix_hi, void* out_fix_lo,
    void* out_unfixed, void* stream);
int abom_remediation_scatter(
    const void* pkg_idx, long long num_findings, const void* item_of, void* state,
    const void* items_off, long long num_items, long long num_installs, void* csr_pkgs,
    void* stream);
int abom_remediation_union(
    const void* items, long long num_items, const void* items_off, const void* csr_pkgs,
    long long pkg_base,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    const void* reach_off, const void* reach_col, long long row_base, long long num_rows,
    long long node_span, void* state, void* queue, void* pool, long long pool_slices,
    void* counters, void* host_counters,
    void* out_servers, void* out_agents, void* out_creds, void* out_tools, void* stream);

// toxic.hip (toxic combinations per finding and per advisory.
// abom_toxic_server_table fills table u32 [num_rows] = caps_all | caps_db << 8
// | shared << 16 per reach-index row from tool_caps and tool_is_db, u8
// [num_tools] indexed by node id - tool_base.  Then five calls on one stream:
// state is u32 [num_vulns, 8], pool u32 [pool_slices * ((num_rows + 31) / 32
// + (node_span + 31) / 32)], counters u32 [16] = {matched advisories, tier-2
// advisories, pool rounds, (package, advisory) heads, findings per pattern x
// 6, multi-agent advisories, findings with a pattern, 0...}, all three
// all-zero on entry and after abom_toxic_finish; host_counters is pinned host
// u32 [16]: the fold writes its first four words, the finish all.  pkg_idx
// and win_idx are int64 [num_findings], pkg_idx ascending, scores fp32,
// n_creds int32; vuln_of is int32 [num_windows] or null for the identity map;
// vulns is the sorted `matched` list, vulns_off the exclusive prefix of
// out_packages with the total at [num_matched].  abom_toxic_cap returns a cap
// of the wave kernel, not a hipError_t: 0 = servers, 1 = agents, 2 = the
// package count above which an advisory skips the wave kernel, else -1)
int abom_toxic_cap(int which);
int abom_toxic_server_table(
    const void* reach_off, const void* reach_col, long long num_rows,
    const void* tool_caps, const void* tool_is_db, long long tool_base, long long num_tools,
    void* table, void* stream);
int abom_toxic_fold(
    const void* pkg_idx, const void* win_idx, const void* scores, const void* n_creds,
    long long num_findings, const void* vuln_of, long long num_windows, long long num_vulns,
    const void* a_severity, const void* a_kev, const void* a_impact, const void* tool_lut,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    long long pkg_base, const void* table, long long row_base, long long num_rows,
    void* state, void* matched, void* counters, void* host_counters, void* out_patterns,
    void* stream);
int abom_toxic_gather(
    const void* vulns, long long num_matched, void* state,
    void* out_findings, void* out_packages, void* out_score, void* out_sev, void* out_kev,
    void* out_patterns, void* stream);
int abom_toxic_scatter(
    const void* pkg_idx, const void* win_idx, long long num_findings,
    const void* vuln_of, long long num_windows, long long num_vulns, void* state,
    const void* vulns_off, long long num_matched, long long num_heads, void* csr_pkgs,
    void* stream);
int abom_toxic_union(
    long long num_matched, const void* vulns_off, const void* csr_pkgs, long long pkg_base,
    const void* rev_off, const void* rev_col, const void* rev_et, int et_contains,
    const void* reach_off, const void* reach_col, long long row_base, long long num_rows,
    long long node_span, void* queue, void* pool, long long pool_slices, void* counters,
    void* out_servers, void* out_agents, void* stream);
int abom_toxic_finish(
    const void* pkg_idx, const void* win_idx, const void* scores, long long num_findings,
    const void* vuln_of, long long num_windows, long long num_vulns,
    const void* vulns, long long num_matched, void* state,
    const void* v_agents, const void* v_score, void* v_patterns,
    void* patterns, void* combo_score, void* counters, void* host_counters, void* stream);

// paths.hip (edge_weight and node_gate are nullable)
int abom_path_relax(
    const void* edge_src, const void* col, const void* etype, const void* edge_weight,
    const void* cur, void* nxt, const void* node_boost, const void* etype_boost,
    const void* etype_trav, const void* etype_gate, const void* node_gate,
    long long num_edges, void* stream);

// rank.hip
int abom_rank_order(
    const void* scores, long long n, void* hist, void* bin_scratch, int nblocks,
    void* order, void* stream);

// findings.hip (abom_findings_count leaves {findings, unique packages, match
// count} in totals; the caller reads them, sizes the outputs and calls
// abom_findings_emit, which also returns the workspace to all-zero)
int abom_findings_count(
    const void* pairs, const void* count, long long capacity,
    const void* run_off, const void* perm2, const void* row_of,
    long long num_rows, long long num_packages,
    void* bitmap, void* row_cnt, void* row_tail, void* chain_prev,
    void* rank_of, void* word_f, void* block_sums, void* totals, void* stream);
int abom_findings_emit(
    const void* pairs, const void* count, long long capacity,
    const void* row_of, long long num_rows, long long num_packages,
    void* bitmap, void* row_cnt, void* row_tail, const void* chain_prev,
    const void* rank_of, const void* word_f, const void* block_off,
    long long pkg_base, long long num_findings, long long num_unique,
    void* out_pkg_idx, void* out_win_idx, void* out_pkg_nodes, void* out_pos,
    void* out_uniq64, void* out_uniq32, void* stream);
// abom_findings_emit with the sizes read from totals on the device: it emits
// and resets only if findings <= findings_cap, unique packages <= unique_cap
// and match count <= capacity, and otherwise leaves workspace and outputs as
// they are; num_sized (device long long) receives the packages emitted, or 0
int abom_findings_emit_sized(
    const void* pairs, const void* count, long long capacity,
    const void* row_of, long long num_rows, long long num_packages,
    void* bitmap, void* row_cnt, void* row_tail, const void* chain_prev,
    const void* rank_of, const void* word_f, const void* block_off,
    long long pkg_base, const void* totals, long long findings_cap, long long unique_cap,
    void* num_sized,
    void* out_pkg_idx, void* out_win_idx, void* out_pkg_nodes, void* out_pos,
    void* out_uniq64, void* out_uniq32, void* stream);
// abom_findings_count, totals -> host_totals (pinned i64[3]),
// abom_findings_emit_sized and abom_blast_counts_indexed_sized over
// out_uniq32, enqueued by one call
int abom_findings_ahead(
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
    void* out_counts, void* out_overflow, void* stream);

// centrality.hip (abom_pagerank_run returns the number of passes run,
// abom_brandes_run the deepest BFS level, or a negated hipError_t; the edge
// types and the heavy-row lists are nullable)
int abom_pagerank_run(
    const void* rev_off, const void* rev_col, const void* rev_heavy, long long num_rev_heavy,
    const void* out_degree, long long num_nodes, double damping, double tolerance,
    int iterations, void* rank_a, void* rank_b, void* contrib_a, void* contrib_b,
    void* partials, void* scalars, void* stream);
int abom_brandes_run(
    const void* fwd_off, const void* fwd_col, const void* fwd_et,
    const void* rev_off, const void* rev_col, const void* rev_et, unsigned int allowed_mask,
    const void* fwd_heavy, long long num_fwd_heavy,
    const void* rev_heavy, long long num_rev_heavy,
    const void* sources, int batch, long long num_nodes,
    void* dist, void* sigma, void* delta, void* bc, void* counter, void* stream);

// components.hip (abom_components_run returns the number of rounds run,
// max_rounds + 1 when that cap was hit before a round hooked nothing, or a
// negated hipError_t; etype, weight and worst are nullable)
int abom_components_run(
    const void* edge_src, const void* col, const void* etype, unsigned int allowed_mask,
    long long num_edges, long long num_nodes, void* labels, void* counters,
    int max_rounds, void* stream);
int abom_component_stats(
    const void* comp, const void* kind, const void* weight, const void* worst,
    long long num_nodes, long long num_components, int num_kinds,
    void* kind_counts, void* weight_sum, void* worst_min, void* stream);

#ifdef __cplusplus
}
#endif
