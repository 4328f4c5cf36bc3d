// The cleaned table where the sweeps leave their state: reconstruction of the queried columns from the device-resident
// referents and latent tables, the five counters of evaluate_accuracy (analysis.jl:36-88), a ring of the last
// reconstructions and its per-cell consensus (most frequent value + support).  Everything here streams [columns][rows]
// int32 arrays; nothing touches the sweep, commit or enumeration state.
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
  DevBuf<unsigned long long> counts;  // [n_cols][5]
};

struct pclean_ring {
  int device = 0;
  int32_t keep = 0, n_cols = 0, n_rows = 0;
  int64_t adds = 0;
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

extern "C" int pclean_recon_set_plan(pclean_ctx* ctx, int32_t n_cols, const pclean_recon_col* cols, int32_t n_map,
                                     const int32_t* id_map) {
  if (!ctx || n_cols < 0 || (n_cols > 0 && !cols) || n_map < 0 || (n_map > 0 && !id_map))
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_recon_set_plan: bad arguments");
  for (int c = 0; c < n_cols; ++c) {
    const pclean_recon_col& q = cols[c];
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
  r->out_valid = r->truth_valid = false;
  r->cols.assign(cols, cols + n_cols);
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

// ---- accuracy counters ------------------------------------------------------------------------------------------------
// blockIdx.y = column; per thread five integer sums over its rows, per workgroup one 64-bit atomic per counter
__global__ __launch_bounds__(256) void recon_counts_kernel(int n_rows, const int32_t* __restrict__ ours,
                                                           const int32_t* __restrict__ dirty, const int32_t* __restrict__ clean,
                                                           unsigned long long* __restrict__ counts) {
  const size_t base = (size_t)blockIdx.y * n_rows;
  unsigned int s[5] = {0, 0, 0, 0, 0};
  for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += gridDim.x * blockDim.x) {
    const int32_t o = ours[base + row], d = dirty[base + row], c = clean[base + row];
    const bool dmiss = d == -4, cmiss = c == -6;
    const bool ch = !dmiss && o != d;
    s[0] += (!dmiss && d != c);
    s[1] += ch;
    s[2] += (ch && o == c);
    s[3] += (dmiss && !cmiss);
    s[4] += (dmiss && !cmiss && o == c);
  }
  __shared__ unsigned int part[4][5];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    unsigned int v = s[q];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) part[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const unsigned long long v = (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] +
                                 part[3][threadIdx.x];
    if (v) atomicAdd(&counts[(size_t)blockIdx.y * 5 + threadIdx.x], v);
  }
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

extern "C" int pclean_recon_counts(pclean_ctx* ctx, const pclean_ring* ring, int64_t* out) {
  if (!ctx || !out) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_recon_counts: bad arguments");
  ReconState* r = rst(ctx);
  if (!r->truth_valid) return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_recon_counts: no dirty / clean columns (pclean_recon_set_truth)");
  const int n_cols = (int)r->cols.size();
  const int32_t* ours = nullptr;
  if (ring) {
    if (!ring->consensus_valid || ring->n_cols != n_cols || ring->n_rows != ctx->n_rows || ring->device != ctx->device)
      return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_recon_counts: the ring holds no consensus of this plan's shape");
    ours = ring->mode.p;
  } else {
    if (!r->out_valid) return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_recon_counts: no reconstruction (pclean_recon_run)");
    ours = r->out.p;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (r->counts.alloc((size_t)n_cols * 5)) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  HIPCHK(ctx, hipMemsetAsync(r->counts.p, 0, (size_t)n_cols * 5 * 8, ctx->stream));
  const unsigned gx = (unsigned)std::min<size_t>(std::max<size_t>(((size_t)ctx->n_rows + 255) / 256, 1), 1024);
  hipLaunchKernelGGL(recon_counts_kernel, dim3(gx, (unsigned)n_cols), dim3(256), 0, ctx->stream, ctx->n_rows, ours, r->dirty.p,
                     r->clean.p, r->counts.p);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  HIPCHK(ctx, hipMemcpy(out, r->counts.p, (size_t)n_cols * 5 * 8, hipMemcpyDeviceToHost));
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
    if (n) hipLaunchKernelGGL(ring_remap_kernel, stream_grid(n), dim3(256), 0, ctx->stream, n, ring->data.p, n_old, map.p);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  }
  map.release();
  ring->consensus_valid = false;
  if (e != hipSuccess) return pclean_fail(ctx, PCLEAN_ERR_HIP, "pclean_ring_remap: %s", hipGetErrorString(e));
  return PCLEAN_OK;
}
