// Internal state of libpclean_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pclean_hip.h"

#define PCLEAN_MAX_TABLES 64
#define PCLEAN_MAX_BLOCKS 16

// RAII-less device buffer: freed by ctx destroy / reassign.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  int alloc(size_t count) {
    if (count <= n && p) return 0;
    release();
    if (count == 0) return 0;
    if (hipMalloc((void**)&p, count * sizeof(T)) != hipSuccess) {
      p = nullptr;
      n = 0;
      return -1;
    }
    n = count;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

// Page-locked staging area owned by the library (grow-only).  Host arrays of the caller are copied through it instead
// of being handed to hipMemcpy[Async]: the runtime page-locks a caller's pageable pages for the DMA and keeps that
// registration; when the caller later frees them (NumPy returns large arrays to the OS) the kernel driver's MMU
// notifier evicts the process's GPU queues to drop the mapping and restores them lazily — measured as 5-27 ms on
// the next GPU operation, whatever its size (a 48-byte table upload after a latent sweep had uploaded 16 MB of evidence).
struct HostStage {
  unsigned char* p = nullptr;
  size_t n = 0, used = 0;
  void rewind() { used = 0; }
  void* take(size_t bytes) {  // null when the area cannot hold it (grow() first)
    const size_t at = (used + 255) & ~(size_t)255;
    if (at + bytes > n) return nullptr;
    used = at + bytes;
    return p + at;
  }
  int grow(size_t bytes) {  // only between uses (nothing in flight reads the old area)
    if (bytes <= n) return 0;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    if (hipHostMalloc((void**)&p, want, hipHostMallocDefault) != hipSuccess) {
      p = nullptr;
      return -1;
    }
    n = want;
    return 0;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = used = 0;
  }
};

extern uint64_t g_pclean_version;  // bumped whenever a table is (re)uploaded; keys the leaf caches

struct PairTable {
  bool valid = false;
  uint64_t version = 0;
  int32_t n_obs = 0, n_lat = 0;
  int32_t elem_bytes = 1;     // 1: uint8 distances, 2: uint16
  DevBuf<uint8_t> d;          // [n_obs][n_lat] * elem_bytes
  DevBuf<uint16_t> lat_len;   // word length (characters) of each latent value
  DevBuf<int32_t> obs_ids;    // AddTypos tables built on the device: pool string of every observed value
  int32_t dist_mode = PCLEAN_DIST_DL;  // flavour the table was built with (dummy_dev.h scores drawn strings with it)
  int32_t max_lat_len = 0, max_obs_len = 0;
  double mean_lat_len = 0.0;  // AddTypos tables built on the device: mean length of the latent strings
  DevBuf<int32_t> same_obs_ids, same_lat_ids;  // host-set 0/1 "same string" tables: pool string of every observed / latent
                                               // value (pclean_set_pair_strings; forgotten by pclean_set_pair_table)
  DevBuf<double> cls;         // [n_lat][4] class densities of a PCLEAN_DENS_TABULATED term (pclean_set_class_density)
  bool cls_valid = false;     // ... uploaded since the table was last built
};

struct CandTable {
  bool valid = false;
  uint64_t version = 0;       // any re-upload (counts / priors)
  uint64_t cols_version = 0;  // re-upload of the value columns
  bool is_options = false;
  int32_t n_rows = 0, n_cols = 0;
  // option tables whose first two value columns form a full grid (a product leaf: option a * |B| + b holds (a, b); or the
  // keyed form of an indexed parameter: option key * |B| + b holds (b, key)): the column that holds k / grid_inner,
  // -1: no grid (pclean_set_options_cols looks at the values it uploads)
  int32_t grid_outer_col = -1, grid_inner = 0;
  // rows [n_used, n_rows) have never held a row (the spare capacity of the device-resident commit: count 0, weight
  // exactly 0): a scan need not look at them.  0: unknown (every row may be in use)
  int32_t n_used = 0;
  DevBuf<int32_t> cols;       // column-major [n_cols][n_rows]
  DevBuf<int64_t> counts;     // FK tables
  DevBuf<double> logc_full;   // FK: log(count-discount); options: logp
  DevBuf<double> logc_m1;     // FK only
  double scal[4] = {0, 0, 0, 0};  // logden_full, logden_m1, lognew_n, lognew_nm1
  std::vector<int32_t> h_vals;   // option tables: the values as last uploaded (pclean_set_options)
  bool is_options_1col = false;
  std::vector<int64_t> h_counts;
  std::vector<double> h_logc_full, h_logc_m1;
  DevBuf<int64_t> stats;      // delta reference counts of last sweep
  double strength = 1.0, discount = 0.0;  // Pitman-Yor parameters of the last upload
  double logc_max = 0.0;      // FK tables: max over rows of log(count - discount) (-inf for an empty table)
  // the last change of the value columns, when a device commit made it: rows [cols_delta_rows[0 .. cols_delta_n)) are what
  // differs between cols_version and cols_delta_base (-1: unknown, e.g. a re-upload)
  uint64_t cols_delta_base = 0;
  int32_t cols_delta_n = -1;
  const int32_t* cols_delta_rows = nullptr;
  // ... or a re-upload of the same shape that differs from the previous one in a few rows (pclean_set_table compares with
  // h_cols, the columns as last uploaded: a latent sub-batch's host commit creates / collects a handful of rows)
  std::vector<int32_t> h_cols;
  DevBuf<int32_t> upload_delta_rows;
  bool h_mirror_stale = false;  // the device arrays moved on without the host mirrors (pclean_commit_device)
  bool h_cols_stale = false;    // ... the value columns among them (a commit that created rows; pclean_commit_pull_table
                                // brings h_cols up to date again)
  // The chain of the host re-uploads' deltas: entry i leads from cols_version `base` to `next` by rewriting `rows`, entry
  // i + 1 starts where entry i ends, the last one ends at cols_version.  A consumer built from ANY version on the chain (the
  // observed class's compact byte tables, last refreshed before the 32 sub-batch uploads of a latent class sweep) refreshes
  // the union of the rows since then instead of rebuilding (cols_union, eval.hip: try_fast_root).
  // the device commit's own delta (rows it wrote, a device list that lives until the table's next commit): the chain's link
  // before the first host re-upload that follows it
  uint64_t commit_delta_base = 0, commit_delta_next = 0;
  int32_t commit_delta_n = -1;
  const int32_t* commit_delta_rows = nullptr;
  struct DeltaEntry {
    uint64_t base, next;
    std::vector<int32_t> rows;
    std::vector<uint64_t> masks;  // bit min(c, 63): column c of the row changed (a Place that moved to another of a hundred
                                  // identical County rows rewrites a reference column that no byte table is built from)
  };
  std::vector<DeltaEntry> delta_log;
  DevBuf<int32_t> union_rows;  // memo of the last union asked for: rows differing between union_base and union_head
  uint64_t union_base = 0, union_head = 0, union_mask = 0;
  int32_t union_n = -1;
  double h_lse = 0.0;         // options: log-sum of logp (+1e-9), valid for version h_lse_ver (eval.hip: subtree_ub)
  uint64_t h_lse_ver = 0;
};

struct FnTable {
  bool valid = false;
  int32_t n_a = 0, n_b = 0;
  DevBuf<int32_t> fn;
  uint64_t version = 0;  // bumped by every pclean_set_fn_table of this id (keys the memo of option-list marginals)
};

struct MeanTable {
  bool valid = false;
  int32_t n = 0;
  DevBuf<double> v;
};

struct ScoreTerm {
  int32_t obs_col, pair_table, val_block, val_col, key_block, key_col, nopt_fn, other_val;
};

// What a PCLEAN_DENS_NAME3 term reads besides its pclean_term (pclean_set_term_name3): where the three values come from,
// the suffix table, and per value of the four domains where its string lies in the pool (start and folded length)
struct Name3Term {
  int32_t term = -1;  // index into Block::terms
  int32_t src_kind[3] = {0, 0, 0}, src_col[3] = {0, 0, 0};
  int32_t suffix_table = -1, n_obs = 0, n_first = 0, n_mid = 0, n_last = 0;
  double log_three = 0.0, log_two = 0.0;
  DevBuf<int64_t> obs_lo, mid_lo;
  DevBuf<int32_t> obs_len, first_len, mid_len, last_len;
  void release() {
    obs_lo.release();
    mid_lo.release();
    obs_len.release();
    first_len.release();
    mid_len.release();
    last_len.release();
  }
};

struct Block {
  bool valid = false;
  uint64_t version = 0;              // bumped by every pclean_load_block of this block
  int32_t group = -1;                // pclean_set_block_group (-1: its own group)
  bool is_score = false;             // no reference slot: only scores observed choices (flights Obs block 3)
  std::vector<ScoreTerm> score_terms;
  int32_t prob_fn = -1, prob_a_block = -1, prob_a_col = -1, prob_b_block = -1, prob_b_col = -1;
  std::vector<pclean_gauss> gauss;   // Gaussian terms of this block's nodes
  std::vector<int32_t> node_gauss;   // per node: index into gauss of its first term, -1 none
  std::vector<std::vector<int32_t>> node_gauss_more;  // per node: its further terms (pclean_add_node_gauss), in order
  std::vector<pclean_node> nodes;
  std::vector<pclean_term> terms;
  std::vector<Name3Term> name3;      // the block's PCLEAN_DENS_NAME3 terms (few: looked up by term index)
  std::vector<int32_t> children;
  std::vector<int32_t> colmap;
  int32_t n_ctx = 0;
  int32_t ctx_src_block[PCLEAN_MAX_CTX] = {-1, -1};
  int32_t ctx_src_col[PCLEAN_MAX_CTX] = {-1, -1};
  DevBuf<pclean_term> d_terms;
  // per-sweep work buffers live in Sweep state (sweep.hip)
  std::vector<DevBuf<double>> leaf_cache;  // per node: marginal per unique observed value
  // cacheable option lists (enum_kernels.hip: leaf_coarse_*): per unique observed value the maximum, the fixed-point
  // total and the inclusive prefix at every 256th option
  std::vector<DevBuf<double>> leaf_m;
  std::vector<DevBuf<uint64_t>> leaf_U, leaf_coarse;
  std::vector<DevBuf<uint64_t>> leaf_udummy;  // fixed-point weight of the ProposalDummyValue option per observed value
  std::vector<int> leaf_drawable;  // per node: -1 unknown, 0 the dummy cannot be drawn for any loaded row, 1 it can
  std::vector<int32_t> new_rows_host, new_vals_host, locals_host;
  DevBuf<int32_t> cur_locals;  // [n_rows][2] current own choices of every observed row (pclean_set_cur_locals), null: none
  int cur_locals_rows = 0;
  std::vector<int32_t> moved_rows_host, moved_choice_host;  // rows whose referent changed in the last sweep
};

struct pclean_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  // string pool
  int32_t n_strings = 0;
  DevBuf<uint16_t> sym;
  DevBuf<int64_t> off;
  std::vector<int64_t> h_off;
  int32_t n_symbols = 0;
  DevBuf<uint16_t> fold;  // case-folding map over the symbols (pclean_set_fold_table)
  int32_t n_fold = 0;

  // observed columns
  int32_t n_rows = 0, n_cols = 0;
  DevBuf<int32_t> obs;  // [n_cols][n_rows]
  uint64_t obs_version = 0;  // bumped by every pclean_load_columns (keys the static per-row tuple ids, eval.hip)
  std::vector<char> col_has_missing;  // per observed column: some row holds an explicitly missing value (-1)
  DevBuf<int32_t> iota; // identity column for per-unique-value leaf caches
  int32_t n_xcols = 0;
  DevBuf<double> xnum;  // numeric observed columns [n_xcols][n_rows]
  MeanTable mean[PCLEAN_MAX_TABLES];
  int32_t n_prob = 0;
  DevBuf<double> prob_same, prob_diff, logn;  // log1p(-p), log(p), log(n)
  std::vector<double> h_prob_same, h_prob_diff, h_logn;

  // density tables
  int32_t max_r = -1, max_d = -1, max_len = -1;
  std::vector<double> h_nb, h_logl;
  DevBuf<double> nb, logl;
  // letter model of random(StringPrior) + pool symbol of every letter (pclean_set_lm_tables)
  bool lm_valid = false;
  DevBuf<double> lm_init, lm_trans;
  DevBuf<uint16_t> letter_sym;
  DevBuf<double> atd;  // [max_len + 1][max_d + 1]: nb[(L+4)/5][d] - logl[L] d - log(26)/2 d in that fp64 order (add_typos.jl:61-63)

  PairTable pair[PCLEAN_MAX_TABLES];
  CandTable cand[PCLEAN_MAX_TABLES];
  FnTable fn[PCLEAN_MAX_TABLES];
  Block block[PCLEAN_MAX_BLOCKS];

  pclean_timing timing = {};
  pclean_root_stats root_stats = {};
  int64_t cur_stride = 0;  // pclean_set_cur_stride
  // device-resident current referents [n_blocks][n_rows] (pclean_set_cur; kept up to date by pclean_commit_device)
  DevBuf<int32_t> dev_cur;
  int32_t dev_cur_blocks = 0;
  bool dev_cur_valid = false;
  // evidence CSR of a latent class built on the device (pclean_build_evidence): the observed rows ordered by the latent row
  // they refer to and their per-row context values, kept for the sub-batches of the class sweep (pclean_sweep_latent_resident)
  DevBuf<int32_t> ev_res_rows, ev_res_ctx;
  int32_t ev_res_n = 0;         // rows held (0: nothing resident)
  bool ev_res_has_ctx = false;
  bool defer_outputs = false;   // pclean_set_sweep_mode bit 0
  // pclean_set_latent_dummy_correction: latent sweeps weigh the particles whose served option lists chose (or hold a value
  // that stands for) the ProposalDummyValue (latent.hip); lat_w = the log-weight corrections [lat_w_items][lat_w_P] of the
  // last such sweep (pclean_get_latent_weights), lat_dp / lat_flag = its distance matrices and "string too long" mark
  bool latent_dummy = false;
  DevBuf<double> lat_w;
  int32_t lat_w_items = 0, lat_w_P = 0;
  DevBuf<int16_t> lat_dp;
  DevBuf<unsigned int> lat_flag;
  // ... its keyed roots: lat_dk[r * lat_dk_items + t] = the dummy option of row t's key in root r's option table, for the next
  // pclean_sweep_latent call alone (pclean_set_latent_dummy_options); time_sym = the pool symbols of a rendered TimePrior draw
  DevBuf<int32_t> lat_dk;
  int32_t lat_dk_roots = 0, lat_dk_items = 0;
  bool lat_dk_valid = false;
  DevBuf<uint16_t> time_sym;
  bool time_sym_valid = false;
  void* commit_state = nullptr;  // owned by commit.hip
  HostStage stage;               // page-locked staging of caller arrays (table uploads, latent-sweep inputs / outputs)
  HostStage ustage;              // ... of the row unions of CandTable::delta_log (asked for in the middle of a sweep call,
                                 // while `stage` holds the call's inputs and outputs)
  const int32_t* obs_override = nullptr;  // eval.hip: ensure_leaf_cache scores "item t observes value t"
  int32_t active_begin = 0, active_count = -1;  // pclean_set_active_rows window (-1 = all rows)
  int32_t timed_block = 0;  // the block whose root launch group pclean_timing / pclean_root_stats describe (pclean_set_timed_block)
  bool prior_mode = false;     // sweep.hip / latent.hip: the running sweep proposes from the priors (use_dd_proposals = false)
  bool force_generic = false;  // debug: never take the compact-table root kernel
  bool no_item_agg = false;    // debug: aggregate evidence with the global sort + run-length encoding only
  // debug (pclean_debug_enum_launches): kernel launches of pclean_launch_enum per instantiation, counted on the host.
  // [0..8) enum_node_kernel / enum_node_big_kernel: 4 * big + 2 * (BT == 1024) + EV; [8..10) enum_scores_kernel<EV>;
  // [10..14) enum_product_kernel: 10 + 2 * (BT == 1024) + !LDSP
  int64_t enum_launches[PCLEAN_ENUM_LAUNCH_SLOTS] = {};
  // debug (pclean_debug_root_launches): what pclean_launch_root_fast / pclean_launch_overflow_fast launched, counted on the
  // host.  [0..5) fk_root_wave_kernel<2|4|8|12|16>, 5 group_settle_kernel, 6 worklist_pack_kernel, 7 a scan launch that was
  // given the lazy-draw lists, 8 overflow_lds_kernel, 9 resolved_draws_kernel
  int64_t root_launches[PCLEAN_ROOT_LAUNCH_SLOTS] = {};
  // debug (pclean_debug_dist_launches): the table-building kernel pclean_launch_dist / launch_dl_seg launched, counted on the
  // host.  [0..16) osa_bitpar_kernel: 8 * (OutT 16-bit) + 4 * (SymT 16-bit) + W - 1; [16..18) osa_tile_kernel<u8 | u16>;
  // [18..26) dl_seg_kernel: 18 + 4 * (SymT 16-bit) + log2(NSEG); [26..32) dl_wave_kernel<16,1 | 32,1 | 64,1..4>; 32
  // dl_lds_kernel; [33..35) dl_pair_kernel<u8 | u16>
  int64_t dist_launches[PCLEAN_DIST_LAUNCH_SLOTS] = {};
  void* sweep_state = nullptr;  // owned by sweep.hip
  void* rccl_comm = nullptr;    // ncclComm_t of pclean_comm_init (comm.hip)
  void* recon_state = nullptr;  // owned by recon.hip
  void* own_state = nullptr;    // owned by own_block.hip
  DevBuf<int64_t> stats_pack;   // pclean_allreduce_stats_fused: the tables' delta counts as one vector
  int32_t comm_ranks = 0, comm_rank = 0;
  // what the collectives of this context moved (pclean_comm_get_stats): HIP events around the last all-gather / all-reduce on
  // the library's stream, folded into the totals when the next one is queued or the statistics are read
  struct CommStats {
    uint64_t ag_calls = 0, ag_bytes_last = 0, ar_calls = 0, ar_elems_last = 0;
    double ag_us = 0.0, ar_us = 0.0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // all-gather begin / end, all-reduce begin / end
    bool ag_pending = false, ar_pending = false;
  } comm_stats;
};

inline int pclean_fail(pclean_ctx* ctx, int code, const char* fmt, ...) {
  if (ctx) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    ctx->err = buf;
  }
  return code;
}

#define HIPCHK(ctx, call)                                                                      \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return pclean_fail(ctx, PCLEAN_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                         __FILE__, __LINE__);                                                  \
  } while (0)

// dist_kernels.hip
int pclean_launch_dist(pclean_ctx* ctx, PairTable& pt, const int32_t* d_obs_ids, const int32_t* d_lat_ids,
                       int dist_mode, const int32_t* h_lat_ids);  // h_lat_ids: the latent string ids on the host
// class_kernels.hip
int pclean_launch_class_table(pclean_ctx* ctx, PairTable& pt, const int32_t* d_obs_ids, const int32_t* d_lat_ids, int rule,
                              int dot_symbol);
int pclean_launch_short_count(pclean_ctx* ctx, int n_opt, const int32_t* d_opt_ids, int n_lat, const int32_t* d_lat_ids,
                              int32_t* d_out);
// density tables (api.hip)
int pclean_ensure_density(pclean_ctx* ctx, int max_len);
// sweep.hip
void pclean_sweep_state_free(pclean_ctx* ctx);
// commit.hip
void pclean_commit_state_free(pclean_ctx* ctx);
void pclean_commit_table_reuploaded(pclean_ctx* ctx, int table_id);
// recon.hip
void pclean_recon_state_free(pclean_ctx* ctx);
// own_block.hip
void pclean_own_state_free(pclean_ctx* ctx);
// comm.hip: collectives queued on the library's stream (no synchronisation)
int pclean_comm_allreduce_stats_queue(pclean_ctx* ctx, int32_t n_tables, const int32_t* table_ids, int32_t local_is_zero);
int pclean_comm_allgather_i32(pclean_ctx* ctx, const int32_t* send, int32_t* recv, size_t words_per_rank);
