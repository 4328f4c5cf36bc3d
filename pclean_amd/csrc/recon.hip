// The cleaned table where the sweeps leave their state: reconstruction of the queried columns from the device-resident
// referents and latent tables, the five counters of evaluate_accuracy (analysis.jl:36-88), a ring of the last
// reconstructions and its per-cell consensus (most frequent value + support).  Everything here streams [columns][rows]
// int32 arrays; nothing touches the sweep, commit or enumeration state.  Own enumerated choices of the observed class and
// numeric columns reported through a Gaussian term are two further column kinds (PCLEAN_RECON_OWN / _NUM): they read a copy
// of the rows' own choices that this state owns, a numeric column's cells are Transformation option indices and its fp64
// values are materialised by a second small kernel; the counters take a row bound (evaluate_accuracy_up_to).
#include <algorithm>

#include "ctx.h"

#define RECON_CHUNK 16  // columns per launch: their descriptors travel as kernel arguments

struct ReconState {
  std::vector<pclean_recon_col> cols;
  DevBuf<int32_t> id_map;  // the columns' value id -> pool id maps, concatenated
  int32_t n_map = 0;
  DevBuf<int32_t> out;     // [n_cols][n_rows]: the last pclean_recon_run
  bool out_valid = false;
  DevBuf<int32_t> dirty, clean;  // [n_cols][n_rows] pool ids of the dirty / clean table (pclean_recon_set_truth)
  bool truth_valid = false;
  DevBuf<unsigned long long> counts;  // [n_cols][6]
  // own enumerated choices of the observed rows per block, [n_rows][2] (pclean_recon_set_locals): what OWN / NUM columns read
  DevBuf<int32_t> locals[PCLEAN_MAX_BLOCKS];
  int32_t locals_rows[PCLEAN_MAX_BLOCKS] = {};
  std::vector<int32_t> num_cols;   // plan positions of the NUM columns
  DevBuf<double> vals;             // [n_numeric][n_rows]: the last pclean_recon_values
  DevBuf<double> dirty_num, clean_num;  // [n_numeric][n_rows] (pclean_recon_set_truth_num)
  bool truth_num_valid = false;
};

struct pclean_ring {
  int device = 0;
  int32_t keep = 0, n_cols = 0, n_rows = 0;
  int64_t adds = 0;
  std::vector<char> is_num;       // per column: its cells are option indices of a NUM column (pclean_ring_remap skips them)
  DevBuf<int32_t> data;           // [keep][n_cols][n_rows]
  DevBuf<int32_t> mode, support;  // [n_cols][n_rows]: the last pclean_ring_consensus
  bool consensus_valid = false;
};

static ReconState* rst(pclean_ctx* ctx) {
  if (!ctx->recon_state) ctx->recon_state = new ReconState();
  return (ReconState*)ctx->recon_state;
}

void pclean_recon_state_free(pclean_ctx* ctx) {
  ReconState* r = (ReconState*)ctx->recon_state;
  if (!r) return;
  r->id_map.release();
  r->out.release();
  r->dirty.release();
  r->clean.release();
  r->counts.release();
  for (auto& l : r->locals) l.release();
  r->vals.release();
  r->dirty_num.release();
  r->clean_num.release();
  delete r;
  ctx->recon_state = nullptr;
}

static inline dim3 recon_grid(size_t n) { return dim3((unsigned)std::max<size_t>((n + 255) / 256, 1)); }
// memory-bound passes over many cells: a bounded grid, the rest by grid stride
static inline dim3 stream_grid(size_t n) { return dim3((unsigned)std::min<size_t>(std::max<size_t>((n + 255) / 256, 1), 8192)); }

// ---- reconstruction ---------------------------------------------------------------------------------------------------
struct ReconColDev {
  const int32_t* cur_a;  // referents of the observed rows in the column's block
  const int32_t* col_a;  // the value column of that block's root table
  const int32_t* cur_b;  // function-table columns: the second argument's block / column
  const int32_t* col_b;
  const int32_t* fn;     // [fn_na][fn_nb]
  const int32_t* map;    // value id -> pool id
  int32_t rows_a, rows_b, fn_na, fn_nb, map_len, kind;
  // OWN / NUM: cur_a = the block's own choices [n_rows][2] (null: a term without a Transformation, option 0),
  // rows_a = which of the two
};
struct ReconArgs {
  int32_t n_cols;
  ReconColDev c[RECON_CHUNK];
};

// One thread per observed row; the columns of one block follow each other in the plan, so the row's referent in that block
// is read once.  A row without a referent (or any index outside its table: nothing is read out of bounds) yields -1.
__global__ __launch_bounds__(256) void recon_kernel(int n_rows, ReconArgs a, int32_t* __restrict__ out) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  const int32_t* held = nullptr;
  int k = -1;
  for (int c = 0; c < a.n_cols; ++c) {
    const ReconColDev& d = a.c[c];
    if (d.kind == PCLEAN_RECON_OWN || d.kind == PCLEAN_RECON_NUM) {
      const int32_t l = d.cur_a ? max(d.cur_a[(size_t)row * 2 + d.rows_a], 0) : 0;
      out[(size_t)c * n_rows + row] = d.kind == PCLEAN_RECON_NUM ? l : (l < d.map_len ? d.map[l] : -1);
      continue;
    }
    if (d.cur_a != held) {
      k = d.cur_a[row];
      held = d.cur_a;
    }
    int32_t v = -1;
    if (k >= 0 && k < d.rows_a) {
      int32_t x = d.col_a[k];
      if (d.kind == PCLEAN_RECON_FN) {
        const int kb = d.cur_b[row];
        int32_t y = -1;
        if (kb >= 0 && kb < d.rows_b) y = d.col_b[kb];
        x = (x >= 0 && x < d.fn_na && y >= 0 && y < d.fn_nb) ? d.fn[(size_t)x * d.fn_nb + y] : -1;
      }
      if (x >= 0 && x < d.map_len) v = d.map[x];
    }
    out[(size_t)c * n_rows + row] = v;
  }
}

// The Gaussian term a NUM column names (block, node = q.table, position on the node = q.col) as it is loaded now; null:
// none, or one whose Transformation is not picked by an own choice of the block.
static const pclean_gauss* recon_gauss_of(const pclean_ctx* ctx, const pclean_recon_col& q) {
  if (q.block < 0 || q.block >= PCLEAN_MAX_BLOCKS || q.table < 0 || q.col < 0) return nullptr;
  const Block& b = ctx->block[q.block];
  if (!b.valid || (size_t)q.table >= b.node_gauss.size() || b.node_gauss[q.table] < 0) return nullptr;
  int32_t gi = b.node_gauss[q.table];
  if (q.col > 0) {
    if ((size_t)q.table >= b.node_gauss_more.size() || (size_t)(q.col - 1) >= b.node_gauss_more[q.table].size()) return nullptr;
    gi = b.node_gauss_more[q.table][q.col - 1];
  }
  if (gi < 0 || (size_t)gi >= b.gauss.size()) return nullptr;
  const pclean_gauss* g = &b.gauss[gi];
  if (g->transform_src_kind == PCLEAN_GSRC_LOCAL ? (g->transform_src < 0 || g->transform_src > 1) : g->transform_src_kind != -1)
    return nullptr;
  return g;
}

// Values of one NUM column: the option index of every row -> rint(backward_u(x)).  One multiply, then round-half-even
// (no addition follows the product: nothing to contract), as np.round(x * t_scale[u]) on the host.
struct NumColDev {
  const double* x;      // the term's numeric column
  const double* tx[4];  // per option: the derived column holding backward_u(x) (non-linear), null: x * scale[u]
  double scale[4];
  int32_t n_opt;
};
__global__ __launch_bounds__(256) void recon_values_kernel(int n_rows, NumColDev d, const int32_t* __restrict__ idx,
                                                           double* __restrict__ out) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n_rows) return;
  const int32_t u = idx[row];
  double v = __longlong_as_double(0x7ff8000000000000LL);
  if (u >= 0 && u < d.n_opt) {
    const double* t = u == 0 ? d.tx[0] : u == 1 ? d.tx[1] : u == 2 ? d.tx[2] : d.tx[3];
    const double s = u == 0 ? d.scale[0] : u == 1 ? d.scale[1] : u == 2 ? d.scale[2] : d.scale[3];
    v = rint(t ? t[row] : d.x[row] * s);
  }
  out[row] = v;
}

extern "C" int pclean_recon_set_plan(pclean_ctx* ctx, int32_t n_cols, const pclean_recon_col* cols, int32_t n_map,
                                     const int32_t* id_map) {
  if (!ctx || n_cols < 0 || (n_cols > 0 && !cols) || n_map < 0 || (n_map > 0 && !id_map))
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_recon_set_plan: bad arguments");
  for (int c = 0; c < n_cols; ++c) {
    const pclean_recon_col& q = cols[c];
    if (q.kind == PCLEAN_RECON_OWN) {
      if (q.block < 0 || q.block >= PCLEAN_MAX_BLOCKS || (q.col != 0 && q.col != 1) || q.map_off < 0 || q.map_len < 0 ||
          (int64_t)q.map_off + q.map_len > n_map)
        return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_recon_set_plan: bad column %d (an own choice is 0 or 1)", c);
      continue;
    }
    if (q.kind == PCLEAN_RECON_NUM) {
      if (!recon_gauss_of(ctx, q))
        return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_recon_set_plan: bad column %d (block %d, node %d holds no Gaussian term %d "
                                                "whose Transformation an own choice picks)", c, q.block, q.table, q.col);
      continue;
    }
    const bool fn = q.kind == PCLEAN_RECON_FN;
    if ((q.kind != PCLEAN_RECON_PATH && !fn) || q.block < 0 || q.block >= PCLEAN_MAX_BLOCKS || q.table < 0 ||
        q.table >= PCLEAN_MAX_TABLES || q.col < 0 || q.map_off < 0 || q.map_len < 0 || (int64_t)q.map_off + q.map_len > n_map ||
        (fn && (q.block_b < 0 || q.block_b >= PCLEAN_MAX_BLOCKS || q.table_b < 0 || q.table_b >= PCLEAN_MAX_TABLES || q.col_b < 0 ||
                q.fn_table < 0 || q.fn_table >= PCLEAN_MAX_TABLES)))
      return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_recon_set_plan: bad column %d", c);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ReconState* r = rst(ctx);
  r->out_valid = r->truth_valid = r->truth_num_valid = false;
  r->cols.assign(cols, cols + n_cols);
  r->num_cols.clear();
  for (int c = 0; c < n_cols; ++c)
    if (cols[c].kind == PCLEAN_RECON_NUM) r->num_cols.push_back(c);
  if (r->id_map.alloc((size_t)std::max(n_map, 1))) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  if (n_map) HIPCHK(ctx, hipMemcpy(r->id_map.p, id_map, (size_t)n_map * 4, hipMemcpyHostToDevice));
  r->n_map = n_map;
  return PCLEAN_OK;
}

// the plan's columns against the tables as they are NOW (a re-upload may have moved them) into out [n_cols][n_rows]
static int recon_launch(pclean_ctx* ctx, ReconState* r, int32_t* out) {
  const int n_cols = (int)r->cols.size();
  if (!ctx->dev_cur_valid || !ctx->dev_cur.p || ctx->n_rows <= 0)
    return pclean_fail(ctx, PCLEAN_ERR_STATE, "reconstruction needs the device-resident referents (pclean_set_cur)");
  const size_t n = (size_t)ctx->n_rows;
  for (int c0 = 0; c0 < n_cols; c0 += RECON_CHUNK) {
    ReconArgs a{};
    a.n_cols = std::min(RECON_CHUNK, n_cols - c0);
    for (int c = 0; c < a.n_cols; ++c) {
      const pclean_recon_col& q = r->cols[c0 + c];
      ReconColDev& d = a.c[c];
      if (q.kind == PCLEAN_RECON_OWN || q.kind == PCLEAN_RECON_NUM) {
        int32_t li = q.col;
        if (q.kind == PCLEAN_RECON_NUM) {
          const pclean_gauss* g = recon_gauss_of(ctx, q);
          if (!g) return pclean_fail(ctx, PCLEAN_ERR_STATE, "reconstruction: column %d names a Gaussian term that is not loaded", c0 + c);
          li = g->transform_src_kind == PCLEAN_GSRC_LOCAL ? g->transform_src : -1;
        }
        d.kind = q.kind;
        d.cur_a = nullptr;
        d.rows_a = 0;
        if (li >= 0) {
          if (!r->locals[q.block].p || r->locals_rows[q.block] != ctx->n_rows)
            return pclean_fail(ctx, PCLEAN_ERR_STATE, "reconstruction: column %d needs the own choices of block %d "
                                                      "(pclean_recon_set_locals)", c0 + c, q.block);
          d.cur_a = r->locals[q.block].p;
          d.rows_a = li;
        }
        d.map = q.kind == PCLEAN_RECON_OWN ? r->id_map.p + q.map_off : nullptr;
        d.map_len = q.kind == PCLEAN_RECON_OWN ? q.map_len : 0;
        continue;
      }
      const CandTable& ta = ctx->cand[q.table];
      if (q.block >= ctx->dev_cur_blocks || !ta.valid || ta.is_options || q.col >= ta.n_cols || !ta.cols.p)
        return pclean_fail(ctx, PCLEAN_ERR_STATE, "reconstruction: column %d names a block / table that is not loaded", c0 + c);
      d.kind = q.kind;
      d.cur_a = ctx->dev_cur.p + (size_t)q.block * n;
      d.col_a = ta.cols.p + (size_t)q.col * ta.n_rows;
      d.rows_a = ta.n_rows;
      d.map = r->id_map.p + q.map_off;
      d.map_len = q.map_len;
      if (q.kind == PCLEAN_RECON_FN) {
        const CandTable& tb = ctx->cand[q.table_b];
        const FnTable& f = ctx->fn[q.fn_table];
        if (q.block_b >= ctx->dev_cur_blocks || !tb.valid || tb.is_options || q.col_b >= tb.n_cols || !tb.cols.p || !f.valid)
          return pclean_fail(ctx, PCLEAN_ERR_STATE, "reconstruction: column %d names a table that is not loaded", c0 + c);
        d.cur_b = ctx->dev_cur.p + (size_t)q.block_b * n;
        d.col_b = tb.cols.p + (size_t)q.col_b * tb.n_rows;
        d.rows_b = tb.n_rows;
        d.fn = f.fn.p;
        d.fn_na = f.n_a;
        d.fn_nb = f.n_b;
      }
    }
    hipLaunchKernelGGL(recon_kernel, recon_grid(n), dim3(256), 0, ctx->stream, ctx->n_rows, a, out + (size_t)c0 * n);
  }
  HIPCHK(ctx, hipGetLastError());
  return PCLEAN_OK;
}

extern "C" int pclean_recon_run(pclean_ctx* ctx, int32_t* out) {
  if (!ctx) return PCLEAN_ERR_ARG;
  ReconState* r = rst(ctx);
  if (r->cols.empty()) return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_recon_run: no plan (pclean_recon_set_plan)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t cells = r->cols.size() * (size_t)std::max(ctx->n_rows, 0);
  if (r->out.alloc(std::max<size_t>(cells, 1))) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  r->out_valid = false;
  const int rc = recon_launch(ctx, r, r->out.p);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  r->out_valid = true;
  if (out) HIPCHK(ctx, hipMemcpy(out, r->out.p, cells * 4, hipMemcpyDeviceToHost));
  return PCLEAN_OK;
}

extern "C" int pclean_recon_set_locals(pclean_ctx* ctx, int32_t block, int32_t n_rows, const int32_t* locals) {
  if (!ctx || block < 0 || block >= PCLEAN_MAX_BLOCKS || !locals || n_rows <= 0)
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_recon_set_locals: bad arguments");
  if (n_rows != ctx->n_rows)
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_recon_set_locals: %d rows, the context holds %d", n_rows, ctx->n_rows);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ReconState* r = rst(ctx);
  r->locals_rows[block] = 0;
  r->out_valid = false;
  if (r->locals[block].alloc((size_t)n_rows * 2)) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  HIPCHK(ctx, hipMemcpy(r->locals[block].p, locals, (size_t)n_rows * 8, hipMemcpyHostToDevice));
  r->locals_rows[block] = n_rows;
  return PCLEAN_OK;
}

// option indices of the source (the last reconstruction or a ring's consensus), or null with the error set
static const int32_t* recon_source(pclean_ctx* ctx, ReconState* r, const pclean_ring* ring, const char* who) {
  if (ring) {
    if (!ring->consensus_valid || ring->n_cols != (int32_t)r->cols.size() || ring->n_rows != ctx->n_rows || ring->device != ctx->device) {
      pclean_fail(ctx, PCLEAN_ERR_STATE, "%s: the ring holds no consensus of this plan's shape", who);
      return nullptr;
    }
    return ring->mode.p;
  }
  if (!r->out_valid) {
    pclean_fail(ctx, PCLEAN_ERR_STATE, "%s: no reconstruction (pclean_recon_run)", who);
    return nullptr;
  }
  return r->out.p;
}

// the NUM columns' values of `ours` [n_cols][n_rows] into r->vals [n_numeric][n_rows] (queued on the stream)
static int recon_values_launch(pclean_ctx* ctx, ReconState* r, const int32_t* ours) {
  const size_t n = (size_t)ctx->n_rows;
  if (r->vals.alloc(std::max<size_t>(r->num_cols.size() * n, 1))) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  for (size_t k = 0; k < r->num_cols.size(); ++k) {
    const int c = r->num_cols[k];
    const pclean_gauss* g = recon_gauss_of(ctx, r->cols[c]);
    if (!g) return pclean_fail(ctx, PCLEAN_ERR_STATE, "reconstruction: column %d names a Gaussian term that is not loaded", c);
    if (!ctx->xnum.p || g->x_col < 0 || g->x_col >= ctx->n_xcols || ctx->xnum.n < (size_t)ctx->n_xcols * n)
      return pclean_fail(ctx, PCLEAN_ERR_STATE, "reconstruction: column %d reads a numeric column that is not loaded", c);
    NumColDev d{};
    d.x = ctx->xnum.p + (size_t)g->x_col * n;
    d.n_opt = g->transform_src_kind == PCLEAN_GSRC_LOCAL ? std::min(std::max(g->local_n[g->transform_src], 0), 4) : 1;
    for (int u = 0; u < 4; ++u) {
      d.scale[u] = g->t_scale[u];
      d.tx[u] = nullptr;
      if (g->t_x_col[u] >= 0) {
        if (g->t_x_col[u] >= ctx->n_xcols)
          return pclean_fail(ctx, PCLEAN_ERR_STATE, "reconstruction: column %d reads a numeric column that is not loaded", c);
        d.tx[u] = ctx->xnum.p + (size_t)g->t_x_col[u] * n;
      }
    }
    hipLaunchKernelGGL(recon_values_kernel, recon_grid(n), dim3(256), 0, ctx->stream, ctx->n_rows, d, ours + (size_t)c * n,
                       r->vals.p + k * n);
  }
  HIPCHK(ctx, hipGetLastError());
  return PCLEAN_OK;
}

extern "C" int pclean_recon_values(pclean_ctx* ctx, const pclean_ring* ring, double* out) {
  if (!ctx) return PCLEAN_ERR_ARG;
  ReconState* r = rst(ctx);
  if (r->num_cols.empty() || ctx->n_rows <= 0)
    return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_recon_values: the plan has no numeric column");
  const int32_t* ours = recon_source(ctx, r, ring, "pclean_recon_values");
  if (!ours) return PCLEAN_ERR_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int rc = recon_values_launch(ctx, r, ours);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (out) HIPCHK(ctx, hipMemcpy(out, r->vals.p, r->num_cols.size() * (size_t)ctx->n_rows * 8, hipMemcpyDeviceToHost));
  return PCLEAN_OK;
}

// ---- accuracy counters ------------------------------------------------------------------------------------------------
// per thread six integer sums over its rows, per workgroup one 64-bit atomic per counter: {errors, changed, cleaned,
// imputed, correctly imputed, missing}.  Rows >= n_up_to have not been cleaned (analysis.jl:99, `ours === nothing`): they
// add to errors and missing only.
__device__ __forceinline__ void recon_counts_reduce(const unsigned int (&s)[6], unsigned long long* __restrict__ counts) {
  __shared__ unsigned int part[4][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    unsigned int v = s[q];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) part[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const unsigned long long v = (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] +
                                 part[3][threadIdx.x];
    if (v) atomicAdd(&counts[threadIdx.x], v);
  }
}

// blockIdx.y = column
__global__ __launch_bounds__(256) void recon_counts_kernel(int n_rows, int n_up_to, const int32_t* __restrict__ ours,
                                                           const int32_t* __restrict__ dirty, const int32_t* __restrict__ clean,
                                                           unsigned long long* __restrict__ counts) {
  const size_t base = (size_t)blockIdx.y * n_rows;
  unsigned int s[6] = {0, 0, 0, 0, 0, 0};
  for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += gridDim.x * blockDim.x) {
    const int32_t o = ours[base + row], d = dirty[base + row], c = clean[base + row];
    const bool in = row < n_up_to;
    const bool dmiss = d == -4, cmiss = c == -6;
    const bool ch = in && !dmiss && o != d;
    s[0] += (!dmiss && d != c);
    s[1] += ch;
    s[2] += (ch && o == c);
    s[3] += (in && dmiss && !cmiss);
    s[4] += (in && dmiss && !cmiss && o == c);
    s[5] += (dmiss && !cmiss);
  }
  recon_counts_reduce(s, counts + (size_t)blockIdx.y * 6);
}

// one NUM column: the rules of the host's numeric branch on fp64 values, dmiss = the dirty value is NaN; comparisons as
// IEEE has them (NaN equals nothing, differs from everything)
__global__ __launch_bounds__(256) void recon_counts_num_kernel(int n_rows, int n_up_to, const double* __restrict__ ours,
                                                               const double* __restrict__ dirty, const double* __restrict__ clean,
                                                               unsigned long long* __restrict__ counts) {
  unsigned int s[6] = {0, 0, 0, 0, 0, 0};
  for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += gridDim.x * blockDim.x) {
    const double o = ours[row], d = dirty[row], c = clean[row];
    const bool in = row < n_up_to;
    const bool dmiss = d != d, cmiss = c != c;
    const bool ch = in && !dmiss && o != d;
    s[0] += (!dmiss && d != c);
    s[1] += ch;
    s[2] += (ch && o == c);
    s[3] += (in && dmiss && !cmiss);
    s[4] += (in && dmiss && o == c);
    s[5] += (dmiss && !cmiss);
  }
  recon_counts_reduce(s, counts);
}

extern "C" int pclean_recon_set_truth(pclean_ctx* ctx, const int32_t* dirty, const int32_t* clean) {
  if (!ctx || !dirty || !clean) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_recon_set_truth: bad arguments");
  ReconState* r = rst(ctx);
  if (r->cols.empty() || ctx->n_rows <= 0)
    return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_recon_set_truth: no plan (pclean_recon_set_plan) or no observed rows");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t cells = r->cols.size() * (size_t)ctx->n_rows;
  r->truth_valid = false;
  if (r->dirty.alloc(cells) || r->clean.alloc(cells)) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  HIPCHK(ctx, hipMemcpy(r->dirty.p, dirty, cells * 4, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(r->clean.p, clean, cells * 4, hipMemcpyHostToDevice));
  r->truth_valid = true;
  return PCLEAN_OK;
}

extern "C" int pclean_recon_set_truth_num(pclean_ctx* ctx, const double* dirty, const double* clean) {
  if (!ctx || !dirty || !clean) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_recon_set_truth_num: bad arguments");
  ReconState* r = rst(ctx);
  if (r->num_cols.empty() || ctx->n_rows <= 0)
    return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_recon_set_truth_num: the plan has no numeric column, or no observed rows");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t cells = r->num_cols.size() * (size_t)ctx->n_rows;
  r->truth_num_valid = false;
  if (r->dirty_num.alloc(cells) || r->clean_num.alloc(cells)) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  HIPCHK(ctx, hipMemcpy(r->dirty_num.p, dirty, cells * 8, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(r->clean_num.p, clean, cells * 8, hipMemcpyHostToDevice));
  r->truth_num_valid = true;
  return PCLEAN_OK;
}

// six counters per column into r->counts (device) over the first n_up_to cleaned rows; a NUM column's int32 counters are
// replaced by those of its fp64 values
static int recon_counts_run(pclean_ctx* ctx, const pclean_ring* ring, int32_t n_up_to, const char* who) {
  ReconState* r = rst(ctx);
  if (!r->truth_valid) return pclean_fail(ctx, PCLEAN_ERR_STATE, "%s: no dirty / clean columns (pclean_recon_set_truth)", who);
  if (!r->num_cols.empty() && !r->truth_num_valid)
    return pclean_fail(ctx, PCLEAN_ERR_STATE, "%s: no dirty / clean values of the numeric columns (pclean_recon_set_truth_num)", who);
  const int n_cols = (int)r->cols.size();
  const int32_t* ours = recon_source(ctx, r, ring, who);
  if (!ours) return PCLEAN_ERR_STATE;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (r->counts.alloc((size_t)n_cols * 6)) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  HIPCHK(ctx, hipMemsetAsync(r->counts.p, 0, (size_t)n_cols * 6 * 8, ctx->stream));
  const size_t n = (size_t)ctx->n_rows;
  const unsigned gx = (unsigned)std::min<size_t>(std::max<size_t>((n + 255) / 256, 1), 1024);
  hipLaunchKernelGGL(recon_counts_kernel, dim3(gx, (unsigned)n_cols), dim3(256), 0, ctx->stream, ctx->n_rows, n_up_to, ours,
                     r->dirty.p, r->clean.p, r->counts.p);
  HIPCHK(ctx, hipGetLastError());
  if (!r->num_cols.empty()) {
    const int rc = recon_values_launch(ctx, r, ours);
    if (rc) return rc;
    for (size_t k = 0; k < r->num_cols.size(); ++k) {
      unsigned long long* cnt = r->counts.p + (size_t)r->num_cols[k] * 6;
      HIPCHK(ctx, hipMemsetAsync(cnt, 0, 6 * 8, ctx->stream));
      hipLaunchKernelGGL(recon_counts_num_kernel, dim3(gx), dim3(256), 0, ctx->stream, ctx->n_rows, n_up_to, r->vals.p + k * n,
                         r->dirty_num.p + k * n, r->clean_num.p + k * n, cnt);
    }
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return PCLEAN_OK;
}

extern "C" int pclean_recon_counts(pclean_ctx* ctx, const pclean_ring* ring, int64_t* out) {
  if (!ctx || !out) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_recon_counts: bad arguments");
  const int rc = recon_counts_run(ctx, ring, ctx->n_rows, "pclean_recon_counts");
  if (rc) return rc;
  ReconState* r = rst(ctx);
  std::vector<int64_t> six(r->cols.size() * 6);  // [n_cols][6] on the device -> the first five of every column
  HIPCHK(ctx, hipMemcpy(six.data(), r->counts.p, six.size() * 8, hipMemcpyDeviceToHost));
  for (size_t c = 0; c < r->cols.size(); ++c) std::copy(six.begin() + c * 6, six.begin() + c * 6 + 5, out + c * 5);
  return PCLEAN_OK;
}

extern "C" int pclean_recon_counts_up_to(pclean_ctx* ctx, const pclean_ring* ring, int32_t n_up_to, int64_t* out) {
  if (!ctx || !out || n_up_to < 0) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_recon_counts_up_to: bad arguments");
  const int rc = recon_counts_run(ctx, ring, n_up_to, "pclean_recon_counts_up_to");
  if (rc) return rc;
  ReconState* r = rst(ctx);
  HIPCHK(ctx, hipMemcpy(out, r->counts.p, r->cols.size() * 6 * 8, hipMemcpyDeviceToHost));
  return PCLEAN_OK;
}

// ---- per-cell consensus -----------------------------------------------------------------------------------------------
// One thread per cell: its S kept values sit in registers (K = the compiled capacity, S <= K), oldest first.  Walking from
// the newest value down, the occurrences of v[s] at or before s are counted: at a value's LATEST occurrence that is its
// total, at earlier ones less — so the first strict maximum met is the most frequent value and, among equally frequent
// ones, the one seen most recently.  Slot of snapshot s: (first + s) mod keep.
template <int K>
__global__ __launch_bounds__(256) void cell_mode_kernel(size_t n_cells, int S, const int32_t* __restrict__ base, size_t slot_stride,
                                                        int first, int keep, int32_t* __restrict__ mode,
                                                        int32_t* __restrict__ support) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (size_t)gridDim.x * blockDim.x) {
    int32_t v[K];
#pragma unroll
    for (int s = 0; s < K; ++s) {
      v[s] = 0;
      if (s < S) {
        int slot = first + s;
        if (slot >= keep) slot -= keep;
        v[s] = base[(size_t)slot * slot_stride + i];
      }
    }
    int32_t best = 0;
    int best_n = 0;
#pragma unroll
    for (int s = K - 1; s >= 0; --s) {
      if (s < S) {
        int c = 0;
#pragma unroll
        for (int t = 0; t <= s; ++t) c += (v[t] == v[s]);
        if (c > best_n) {
          best_n = c;
          best = v[s];
        }
      }
    }
    mode[i] = best;
    support[i] = best_n;
  }
}

static int launch_cell_mode(pclean_ctx* ctx, size_t n_cells, int S, const int32_t* base, size_t slot_stride, int first, int keep,
                            int32_t* mode, int32_t* support) {
  const dim3 g = stream_grid(n_cells), b(256);
  if (S <= 4)
    hipLaunchKernelGGL(cell_mode_kernel<4>, g, b, 0, ctx->stream, n_cells, S, base, slot_stride, first, keep, mode, support);
  else if (S <= 8)
    hipLaunchKernelGGL(cell_mode_kernel<8>, g, b, 0, ctx->stream, n_cells, S, base, slot_stride, first, keep, mode, support);
  else if (S <= 16)
    hipLaunchKernelGGL(cell_mode_kernel<16>, g, b, 0, ctx->stream, n_cells, S, base, slot_stride, first, keep, mode, support);
  else
    hipLaunchKernelGGL(cell_mode_kernel<32>, g, b, 0, ctx->stream, n_cells, S, base, slot_stride, first, keep, mode, support);
  HIPCHK(ctx, hipGetLastError());
  return PCLEAN_OK;
}

extern "C" int pclean_cell_mode(pclean_ctx* ctx, int32_t n_snapshots, int64_t n_cells, const int32_t* snapshots, int32_t* mode,
                                int32_t* support) {
  if (!ctx || n_snapshots < 1 || n_snapshots > PCLEAN_RING_MAX_KEEP || n_cells < 0 || (n_cells > 0 && (!snapshots || !mode || !support)))
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_cell_mode: 1 <= n_snapshots <= %d, non-null arrays", PCLEAN_RING_MAX_KEEP);
  if (n_cells == 0) return PCLEAN_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf<int32_t> in, out;
  const size_t m = (size_t)n_cells;
  int rc = PCLEAN_OK;
  if (in.alloc(m * n_snapshots) || out.alloc(2 * m)) rc = pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemcpy(in.p, snapshots, m * n_snapshots * 4, hipMemcpyHostToDevice);
  if (!rc && e == hipSuccess) rc = launch_cell_mode(ctx, m, n_snapshots, in.p, m, 0, n_snapshots, out.p, out.p + m);
  if (!rc && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (!rc && e == hipSuccess) e = hipMemcpy(mode, out.p, m * 4, hipMemcpyDeviceToHost);
  if (!rc && e == hipSuccess) e = hipMemcpy(support, out.p + m, m * 4, hipMemcpyDeviceToHost);
  in.release();
  out.release();
  if (!rc && e != hipSuccess) rc = pclean_fail(ctx, PCLEAN_ERR_HIP, "pclean_cell_mode: %s", hipGetErrorString(e));
  return rc;
}

// ---- the ring of the last reconstructions -----------------------------------------------------------------------------
extern "C" int pclean_ring_create(pclean_ctx* ctx, int32_t keep, pclean_ring** out) {
  if (!ctx || !out) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_ring_create: bad arguments");
  *out = nullptr;
  if (keep < 1 || keep > PCLEAN_RING_MAX_KEEP)
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_ring_create: 1 <= keep <= %d", PCLEAN_RING_MAX_KEEP);
  ReconState* r = rst(ctx);
  if (r->cols.empty() || ctx->n_rows <= 0)
    return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_ring_create: no plan (pclean_recon_set_plan) or no observed rows");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  pclean_ring* g = new pclean_ring();
  g->device = ctx->device;
  g->keep = keep;
  g->n_cols = (int32_t)r->cols.size();
  g->n_rows = ctx->n_rows;
  g->is_num.assign(r->cols.size(), 0);
  for (int32_t c : r->num_cols) g->is_num[c] = 1;
  const size_t cells = (size_t)g->n_cols * g->n_rows;
  if (g->data.alloc(cells * keep) || g->mode.alloc(cells) || g->support.alloc(cells)) {
    g->data.release();
    g->mode.release();
    g->support.release();
    delete g;
    return pclean_fail(ctx, PCLEAN_ERR_HIP, "pclean_ring_create: device alloc of %zu bytes failed", cells * (keep + 2) * 4);
  }
  *out = g;
  return PCLEAN_OK;
}

extern "C" int pclean_ring_destroy(pclean_ring* ring) {
  if (!ring) return PCLEAN_ERR_ARG;
  (void)hipSetDevice(ring->device);
  (void)hipDeviceSynchronize();
  ring->data.release();
  ring->mode.release();
  ring->support.release();
  delete ring;
  return PCLEAN_OK;
}

extern "C" int pclean_ring_info(const pclean_ring* ring, int64_t out[4]) {
  if (!ring || !out) return PCLEAN_ERR_ARG;
  out[0] = ring->keep;
  out[1] = ring->n_cols;
  out[2] = ring->n_rows;
  out[3] = ring->adds;
  return PCLEAN_OK;
}

static int ring_matches(pclean_ctx* ctx, const pclean_ring* g, const char* who) {
  if (!ctx || !g) return pclean_fail(ctx, PCLEAN_ERR_ARG, "%s: bad arguments", who);
  if (g->device != ctx->device) return pclean_fail(ctx, PCLEAN_ERR_ARG, "%s: the ring lives on another device", who);
  return PCLEAN_OK;
}

extern "C" int pclean_ring_add(pclean_ctx* ctx, pclean_ring* ring) {
  int rc = ring_matches(ctx, ring, "pclean_ring_add");
  if (rc) return rc;
  ReconState* r = rst(ctx);
  if ((int32_t)r->cols.size() != ring->n_cols || ctx->n_rows != ring->n_rows)
    return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_ring_add: the plan's shape is not the ring's");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t cells = (size_t)ring->n_cols * ring->n_rows;
  const int slot = (int)(ring->adds % ring->keep);
  rc = recon_launch(ctx, r, ring->data.p + (size_t)slot * cells);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ring->adds += 1;
  ring->consensus_valid = false;
  return PCLEAN_OK;
}

extern "C" int pclean_ring_consensus(pclean_ctx* ctx, pclean_ring* ring, int32_t* mode, int32_t* support) {
  int rc = ring_matches(ctx, ring, "pclean_ring_consensus");
  if (rc) return rc;
  if (ring->adds < 1) return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_ring_consensus: the ring is empty");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t cells = (size_t)ring->n_cols * ring->n_rows;
  const int kept = (int)std::min<int64_t>(ring->adds, ring->keep);
  const int first = (int)((ring->adds - kept) % ring->keep);
  rc = launch_cell_mode(ctx, cells, kept, ring->data.p, cells, first, ring->keep, ring->mode.p, ring->support.p);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ring->consensus_valid = true;
  if (mode) HIPCHK(ctx, hipMemcpy(mode, ring->mode.p, cells * 4, hipMemcpyDeviceToHost));
  if (support) HIPCHK(ctx, hipMemcpy(support, ring->support.p, cells * 4, hipMemcpyDeviceToHost));
  return PCLEAN_OK;
}

// kept pool ids through an old -> new id map (the string pool was rebuilt); negative ids stand for themselves, an id the
// map does not cover becomes -2 ("a string outside the pool")
__global__ __launch_bounds__(256) void ring_remap_kernel(size_t n, int32_t* __restrict__ data, int n_old,
                                                         const int32_t* __restrict__ old_to_new) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int32_t v = data[i];
    if (v >= 0) data[i] = v < n_old ? old_to_new[v] : -2;
  }
}

extern "C" int pclean_ring_remap(pclean_ctx* ctx, pclean_ring* ring, int32_t n_old, const int32_t* old_to_new) {
  int rc = ring_matches(ctx, ring, "pclean_ring_remap");
  if (rc) return rc;
  if (n_old < 0 || (n_old > 0 && !old_to_new)) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_ring_remap: bad arguments");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DevBuf<int32_t> map;
  if (map.alloc((size_t)std::max(n_old, 1))) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  hipError_t e = n_old ? hipMemcpy(map.p, old_to_new, (size_t)n_old * 4, hipMemcpyHostToDevice) : hipSuccess;
  if (e == hipSuccess) {
    const size_t n = (size_t)ring->n_cols * ring->n_rows * (size_t)std::min<int64_t>(ring->adds, ring->keep);
    // (before the ring has wrapped its kept snapshots are slots [0, adds))
    const bool any_num = std::find(ring->is_num.begin(), ring->is_num.end(), (char)1) != ring->is_num.end();
    if (n && !any_num)
      hipLaunchKernelGGL(ring_remap_kernel, stream_grid(n), dim3(256), 0, ctx->stream, n, ring->data.p, n_old, map.p);
    else if (n) {  // column by column in every kept slot; the option indices of NUM columns stay
      const size_t rows = (size_t)ring->n_rows, slots = n / ((size_t)ring->n_cols * rows);
      for (size_t s = 0; s < slots; ++s)
        for (int32_t c = 0; c < ring->n_cols; ++c)
          if (!ring->is_num[c])
            hipLaunchKernelGGL(ring_remap_kernel, stream_grid(rows), dim3(256), 0, ctx->stream, rows,
                               ring->data.p + (s * ring->n_cols + c) * rows, n_old, map.p);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  }
  map.release();
  ring->consensus_valid = false;
  if (e != hipSuccess) return pclean_fail(ctx, PCLEAN_ERR_HIP, "pclean_ring_remap: %s", hipGetErrorString(e));
  return PCLEAN_OK;
}
