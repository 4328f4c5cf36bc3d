// Own blocks: a flat observed class (pclean_load_own_block / pclean_sweep_own and their probes).
//
// A block of the observed class without a reference slot whose own discrete choices are enumerated from their observations
// (src/inference/proposal_compiler.jl:55-129; the retained value is forced at 100-101).  Every choice is one option list
// (values, logp) with its likelihood terms.  When ALL blocks of the class are of this kind every particle of run_smc!
// (row_inference.jl:108-187) carries the same weight after every block — the weight of a block is its option lists'
// marginals, which do not depend on the particle — so maybe_resample never fires, the final choice is made on equal
// weights and the return value is the sum of the log-marginals.  The sweep is then, per row: choose the particle, and
// unless that is the retained one, draw every choice from its conditional.
//
// With the parameters frozen during a sweep the scores of a list's K options depend on a row only through the tuple of
// its observed values over the list's terms, and that tuple is static: the host orders the rows by it once per loaded plan
// (ensure_groups) and own_leaf_kernel scores every distinct tuple ONCE per sweep —
//   one workgroup (4 wavefronts) per tuple run (a long run is cut into pieces of OWN_RUN_SPLIT rows):
//   pass 1  lane-strided over the options: fp64 score (candidate_score's operations in candidate_score's order), maximum
//   pass 2  u_k = floor(exp(s_k - m) 2^40); per 64 options one sum by a wave reduction; inclusive prefix of those sums
//           RESIDENT (K <= OWN_LDS_OPTIONS): the u_k stay in LDS; otherwise they are recomputed where they are needed
//   draws   one row of the run per lane: Philox threshold x = mulhi64(R, U), binary search over the chunk prefix, then a
//           walk inside the chunk — the sequential scan's  min{k : u_0 + .. + u_k > x}  in two steps
// Integer sums: maximum, U, lse and every draw are the generic enumeration kernels' (enum_kernels.hip), bit for bit,
// whatever the variant, the grouping or the window.
//
// own_product_kernel serves a leaf whose option list is a full grid over two value columns (an own choice indexed by a
// sibling own choice, enumerated jointly): every term once per value of the factor it reads, then the grid from the cached
// values — the same doubles in the same order, so the same bits (see the kernel).
//
// own_marginal_kernel (pclean_own_marginals) reports what the sweep holds before it draws: passes 1 and 2 as above, then
// instead of the draws the `top` options of largest u_k (ties: the smaller index) with u_k / U, and u_cur / U of every row's
// current value.  It writes no value.
#include "sweep_internal.h"

#define OWN_BT 256
#define OWN_LDS_OPTIONS 4096                   // options whose fixed-point weights stay in LDS (32 KiB of a workgroup)
#define OWN_MAX_OPTIONS (64 * OWN_LDS_OPTIONS)  // the chunked variant keeps one sum per 64 options in the same array
#define OWN_RUN_SPLIT 2048                      // rows a workgroup draws for; a longer tuple run is cut (same results)
#define OWN_HALF_LOG26 1.629048269010741
#define OWN_ADD_TYPOS_IMPOSSIBLE (-1e5)

namespace {

struct OwnLeaf {
  pclean_node node;
  std::vector<pclean_term> terms;
  // the static grouping: pieces of tuple runs, rows ascending within a run
  bool grouped = false;
  uint64_t obs_version = 0;
  int n_runs = 0, longest = 0, n_pieces = 0;
  DevBuf<int32_t> piece_off, piece_rows;
  std::vector<int32_t> h_piece_of_row, h_run_of_piece, h_run_len;
};

struct OwnBlock {
  bool valid = false;
  std::vector<OwnLeaf> leaves;
  DevBuf<int32_t> vals;  // [n_leaves][vals_rows]
  int vals_rows = 0;
};

struct OwnState {
  OwnBlock block[PCLEAN_MAX_BLOCKS];
  pclean_own_stats stats = {0, 0, 0, 0, 0, -1, OWN_LDS_OPTIONS, 0};
  DevBuf<double> zero;       // one 0.0: the equal weights of the final choice
  DevBuf<int32_t> bad;       // {rows with logml == -inf, the smallest of them}
  DevBuf<unsigned long long> hist;
  hipEvent_t ev[2] = {nullptr, nullptr};  // around the launches of the last pclean_sweep_own (pclean_timing.total_ms)
  bool product_attr_set = false;          // own_product_kernel's dynamic-LDS limit is raised on this context's device
};

OwnState* own(pclean_ctx* ctx) {
  if (!ctx->own_state) ctx->own_state = new OwnState();
  return static_cast<OwnState*>(ctx->own_state);
}

// ---- device side -------------------------------------------------------------------------------------------------
struct OwnNodeDev {
  int32_t n_cand, n_terms;
  const double* logp;
  TermDev terms[PCLEAN_MAX_TERMS];
};

struct OwnLaunch {
  const int32_t* piece_off;  // [pieces + 1] into members
  const int32_t* members;    // sweep: rows (index into the loaded rows); probe: item ids
  const int32_t* item_row;   // probe: row of every item
  int32_t win_lo, win_hi;    // sweep: the active window (rows outside are left alone)
  int32_t probe, n_draws;
  const int32_t* chosen;     // sweep, indexed by row - win_lo
  const int32_t* keep;
  double* logml;
  int32_t* vals;             // sweep: the leaf's current values, indexed by row
  double* lse_out;           // probe, indexed by item
  double* scores_out;
  int32_t* draws_out;
  int64_t row_offset;        // global id of loaded row 0
  uint64_t seed;
  uint32_t sweep, site;
};

__device__ __forceinline__ double own_wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ unsigned long long own_wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ unsigned long long own_wave_scan(unsigned long long v, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long x = __shfl_up(v, o, 64);
    if (lane >= o) v += x;
  }
  return v;
}

// enum_kernels.hip: term_density — the same operations on the same values
__device__ __forceinline__ double own_term_density(const TermDev& tm, const DensDev& dn, int d, int val) {
  if (tm.dens_kind == PCLEAN_DENS_EQUAL) return d == 0 ? 0.0 : -__builtin_inf();
  if (tm.max_typos >= 0 && d > tm.max_typos) return OWN_ADD_TYPOS_IMPOSSIBLE;
  const int L = tm.lat_len[val];
  const int r = (L + 4) / 5;
  double l = dn.nb[(size_t)r * dn.nb_stride + d];
  l -= dn.logl[L] * (double)d;
  l -= OWN_HALF_LOG26 * (double)d;
  return l;
}

// score of option k for the run's observed tuple obs[0 .. n_terms): enum_kernels.hip's candidate_score for an option list
// (prior first, then the terms in declaration order; a tabulated term counts a missing observation, the others skip it)
__device__ __forceinline__ double own_score(const OwnNodeDev& nd, const DensDev& dn, const int* obs, int k) {
  double sk = nd.logp[k];
  for (int ti = 0; ti < nd.n_terms; ++ti) {
    const TermDev& tm = nd.terms[ti];
    const int o = obs[ti];
    if (tm.dens_kind == PCLEAN_DENS_TABULATED) {
      const int val = tm.cand_col[k];
      const int c = o < 0 ? 3 : ((int)tm.pair[(size_t)o * tm.n_lat + val] & 3);
      sk += tm.cls[(size_t)val * 4 + c];
      continue;
    }
    if (o < 0) continue;
    const int val = tm.cand_col[k];
    const size_t idx = (size_t)o * tm.n_lat + val;
    const int d = tm.elem_bytes == 1 ? (int)tm.pair[idx] : (int)((const uint16_t*)tm.pair)[idx];
    sk += own_term_density(tm, dn, d, val);
  }
  return sk;
}

template <bool RESIDENT>
__global__ __launch_bounds__(OWN_BT) void own_leaf_kernel(const OwnNodeDev nd, const DensDev dn, const OwnLaunch L) {
  // RESIDENT: the scores (as doubles), then the fixed-point weights; otherwise the chunk sums, then their inclusive prefix
  __shared__ unsigned long long s_u[OWN_LDS_OPTIONS];
  __shared__ unsigned long long s_cs[OWN_LDS_OPTIONS / 64];  // RESIDENT: inclusive prefix of the chunk sums
  __shared__ double s_red[OWN_BT / 64];
  __shared__ int s_obs[PCLEAN_MAX_TERMS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  const int m_lo = L.piece_off[g], m_hi = L.piece_off[g + 1];
  const int n = nd.n_cand;
  if (!L.probe) {  // a run none of whose rows lies in the window has nothing to do
    int any = 0;
    for (int q = m_lo + tid; q < m_hi; q += OWN_BT) {
      const int r = L.members[q];
      any |= (r >= L.win_lo && r < L.win_hi) ? 1 : 0;
    }
    if (!__syncthreads_or(any)) return;
  }
  {
    const int row0 = L.probe ? L.item_row[L.members[m_lo]] : L.members[m_lo];
    for (int ti = 0; ti < nd.n_terms; ++ti)
      if (tid == ti) s_obs[ti] = nd.terms[ti].obs_col[row0];
  }
  __syncthreads();

  // ---- pass 1: scores and their maximum
  double* s = reinterpret_cast<double*>(s_u);
  double lmax = -__builtin_inf();
  for (int k = tid; k < n; k += OWN_BT) {
    const double sk = own_score(nd, dn, s_obs, k);
    if (RESIDENT) s[k] = sk;
    if (L.probe && L.scores_out)
      for (int mi = m_lo; mi < m_hi; ++mi) L.scores_out[(size_t)L.members[mi] * n + k] = sk;
    lmax = fmax(lmax, sk);
  }
  lmax = own_wave_max(lmax);
  if (lane == 0) s_red[wave] = lmax;
  __syncthreads();
  double m = s_red[0];
  for (int w = 1; w < OWN_BT / 64; ++w) m = fmax(m, s_red[w]);
  const bool dead = m == -__builtin_inf();

  // ---- pass 2: fixed-point weights, one sum per 64 options, inclusive prefix of the sums
  const int nch = (n + 63) >> 6;
  unsigned long long* pre = RESIDENT ? s_cs : s_u;
  if (RESIDENT) {
    for (int k = tid; k < n; k += OWN_BT) {
      const double sk = s[k];
      s_u[k] = dead ? 0ull : pclean_fixw(sk - m);
    }
    __syncthreads();
  }
  for (int c = wave; c < nch; c += OWN_BT / 64) {
    const int k = (c << 6) + lane;
    unsigned long long v = 0ull;
    if (k < n) v = RESIDENT ? s_u[k] : (dead ? 0ull : pclean_fixw(own_score(nd, dn, s_obs, k) - m));
    v = own_wave_sum(v);
    if (lane == 0) pre[c] = v;
  }
  __syncthreads();
  if (wave == 0) {
    unsigned long long carry = 0ull;
    for (int base = 0; base < nch; base += 64) {
      const int i = base + lane;
      unsigned long long v = own_wave_scan(i < nch ? pre[i] : 0ull, lane) + carry;
      if (i < nch) pre[i] = v;
      carry = __shfl(v, 63, 64);
    }
  }
  __syncthreads();
  const unsigned long long U = pre[nch - 1];
  const double lse = pclean_lse_from_fix(m, U);

  // ---- the run's rows: one member per lane
  const int nd_eff = L.probe ? max(L.n_draws, 1) : 1;
  const int n_out = (m_hi - m_lo) * nd_eff;
  for (int q = tid; q < n_out; q += OWN_BT) {
    const int mem = L.members[m_lo + q / nd_eff], j = q % nd_eff;
    int row, pid;
    if (L.probe) {
      row = L.item_row[mem];
      pid = j;
      if (j == 0 && L.lse_out) L.lse_out[mem] = lse;
      if (L.n_draws <= 0) continue;
    } else {
      row = mem;
      if (row < L.win_lo || row >= L.win_hi) continue;
      const int i = row - L.win_lo;
      L.logml[i] += lse;  // (a row lies in exactly one run of the leaf; the leaves are launched one after the other)
      if (L.keep[i]) continue;
      pid = L.chosen[i];
    }
    int res = n - 1;
    if (U != 0ull) {
      const uint32_t rng_row = (uint32_t)((int64_t)row + L.row_offset);
      const unsigned long long x = pclean_mulhi64(pclean_rand64(L.seed, rng_row, L.site, (uint32_t)pid, L.sweep), U);
      int a = 0, b = nch - 1;
      while (a < b) {  // the first chunk whose inclusive prefix exceeds x
        const int mid = (a + b) >> 1;
        if (pre[mid] > x)
          b = mid;
        else
          a = mid + 1;
      }
      unsigned long long acc = a ? pre[a - 1] : 0ull;
      int k = a << 6;
      const int k_end = min(n, k + 64) - 1;  // (the chunk's total exceeds x - acc: the walk stops inside it)
      for (; k < k_end; ++k) {
        acc += RESIDENT ? s_u[k] : pclean_fixw(own_score(nd, dn, s_obs, k) - m);
        if (acc > x) break;
      }
      res = k;
    }
    if (L.probe)
      L.draws_out[(size_t)mem * L.n_draws + j] = res;
    else
      L.vals[row] = res;
  }
}

// ---- product leaf: an option list that is a full grid a * n_inner + b over two value columns ------------------------------
// (an own choice indexed by a sibling own choice: model.py, _lower_own_block).  Every term reads ONE of the two factors, so
// per tuple run its density takes n_outer or n_inner values, not n_outer x n_inner:
//   phase 1  each term once per value of the factor it reads (own_score's rules: a tabulated term scores a missing
//            observation, the others skip it), the doubles into LDS; the gathers of a term are independent, in flight together
//   phase 2  the grid, OWN_SUPER chunks of 64 options per wave at a time (one division per lane and group: (a, b) of option
//            k + 64 follows from that of k): s_k = logp[k], then += the cached value of every non-skipped term in plan
//            order — own_score's doubles in own_score's order, so m, u_k = fixw(s_k - m), U, lse and every draw are
//            own_leaf_kernel's (and enum_product_kernel's on the latent twin), bit for bit.  The pass that finds m
//            keeps the maximum of every group; the weight pass skips a group whose maximum lies more than
//            OWN_SKIP_BELOW under m: pclean_fixw is 0 below -28.5, and fp64 subtraction is monotone, so every weight of such
//            a group is the 0 it would have computed.  One sum per chunk and their inclusive prefix in LDS; draws by
//            own_leaf_kernel's binary search and a walk that recomputes the weights from the cached values.
// Dynamic LDS: [total] cached term values, [n_chunks] chunk sums, [n_super] group maxima (left out, with the skip, when
// they do not fit) — 8 bytes each, at most OWN_PRODUCT_LDS_MAX; a plan beyond that takes own_leaf_kernel<false>.
#define OWN_PRODUCT_LDS_MAX ((size_t)160 * 1024 - 512)  // (the static arrays of the kernel take the rest of the 160 KiB)
#define OWN_PRODUCT_WIDE 16384                          // options from which a workgroup has 1024 threads (16 chunks per wave)
#define OWN_SKIP_BELOW 30.0
#define OWN_SUPER 8  // chunks of 64 options a wavefront takes together: one division per lane and one maximum per 512 options

struct OwnProductDev {
  int32_t n_outer, n_inner, total, n_chunks;  // total: cached doubles
  int32_t use_cmax, n_super;                  // n_super: groups of OWN_SUPER chunks (one maximum each)
  int32_t q64, r64;                           // 64 / n_inner, 64 % n_inner: the step of (a, b) from option k to k + 64
  int32_t inner[PCLEAN_MAX_TERMS];  // 1: the term reads the inner factor (k % n_inner), 0: the outer (k / n_inner)
  int32_t off[PCLEAN_MAX_TERMS];
};

template <int BT>
__global__ __launch_bounds__(BT) void own_product_kernel(const OwnNodeDev nd, const DensDev dn, const OwnLaunch L,
                                                          const OwnProductDev pr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char own_smem[];
  __shared__ double s_red[BT / 64];
  __shared__ int s_obs[PCLEAN_MAX_TERMS];
  double* tv = reinterpret_cast<double*>(own_smem);                                // [pr.total]
  unsigned long long* pre = reinterpret_cast<unsigned long long*>(tv + pr.total);  // [pr.n_chunks]
  double* cmax = reinterpret_cast<double*>(pre + pr.n_chunks);                     // [pr.n_super] when pr.use_cmax
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  const int m_lo = L.piece_off[g], m_hi = L.piece_off[g + 1];
  const int n = nd.n_cand, n_inner = pr.n_inner, nch = pr.n_chunks;
  if (!L.probe) {  // a run none of whose rows lies in the window has nothing to do
    int any = 0;
    for (int q = m_lo + tid; q < m_hi; q += BT) {
      const int r = L.members[q];
      any |= (r >= L.win_lo && r < L.win_hi) ? 1 : 0;
    }
    if (!__syncthreads_or(any)) return;
  }
  {
    const int row0 = L.probe ? L.item_row[L.members[m_lo]] : L.members[m_lo];
    for (int ti = 0; ti < nd.n_terms; ++ti)
      if (tid == ti) s_obs[ti] = nd.terms[ti].obs_col[row0];
  }
  __syncthreads();

  // ---- phase 1: the terms, once per factor value
  unsigned int skip = 0;
  for (int ti = 0; ti < nd.n_terms; ++ti) {
    const TermDev& tm = nd.terms[ti];
    const int o = s_obs[ti];
    const bool tab = tm.dens_kind == PCLEAN_DENS_TABULATED;
    if (!tab && o < 0) {  // a missing observation: the term adds nothing
      skip |= 1u << ti;
      continue;
    }
    const int nf = pr.inner[ti] ? n_inner : pr.n_outer;
    const size_t stride = pr.inner[ti] ? 1 : (size_t)n_inner;
    double* dst = tv + pr.off[ti];
    for (int j = tid; j < nf; j += BT) {
      const int val = tm.cand_col[(size_t)j * stride];
      double x;
      if (tab) {
        const int c = o < 0 ? 3 : ((int)tm.pair[(size_t)o * tm.n_lat + val] & 3);
        x = tm.cls[(size_t)val * 4 + c];
      } else {
        const size_t idx = (size_t)o * tm.n_lat + val;
        const int d = tm.elem_bytes == 1 ? (int)tm.pair[idx] : (int)((const uint16_t*)tm.pair)[idx];
        x = own_term_density(tm, dn, d, val);
      }
      dst[j] = x;
    }
  }
  __syncthreads();
  // score of option k = a * n_inner + b with (a, b) at hand (a wavefront steps from k to k + 64 without dividing again):
  // the ONE place where the plan-order sum that the bit parity rests on is written
  auto score_ab = [&](int k, int a, int b) -> double {
    double sk = nd.logp[k];
    for (int ti = 0; ti < nd.n_terms; ++ti)
      if (!((skip >> ti) & 1u)) sk += tv[pr.off[ti] + (pr.inner[ti] ? b : a)];
    return sk;
  };
  auto score = [&](int k) -> double {  // (the walk of a draw: one option, its (a, b) by division)
    const int a = k / n_inner;
    return score_ab(k, a, k - a * n_inner);
  };

  // ---- phase 2, pass 1: scores (the loads of a group of chunks in flight together), the maximum of every group, the maximum
  const int nsup = pr.n_super;
  double lmax = -__builtin_inf();
  for (int sc = wave; sc < nsup; sc += BT / 64) {
    const int k0 = sc * (64 * OWN_SUPER) + lane;
    int a = k0 / n_inner, b = k0 - a * n_inner;
    double mx = -__builtin_inf();
#pragma unroll
    for (int j = 0; j < OWN_SUPER; ++j) {
      const int k = k0 + (j << 6);
      if (k < n) {
        const double sk = score_ab(k, a, b);
        if (L.probe && L.scores_out)
          for (int mi = m_lo; mi < m_hi; ++mi) L.scores_out[(size_t)L.members[mi] * n + k] = sk;
        mx = fmax(mx, sk);
      }
      a += pr.q64;
      b += pr.r64;
      if (b >= n_inner) {
        b -= n_inner;
        ++a;
      }
    }
    const double cm = own_wave_max(mx);  // (one reduction per group: a maximum per 64 options measured slower)
    if (pr.use_cmax && lane == 0) cmax[sc] = cm;
    lmax = fmax(lmax, cm);
  }
  if (lane == 0) s_red[wave] = lmax;
  __syncthreads();
  double m = s_red[0];
  for (int w = 1; w < BT / 64; ++w) m = fmax(m, s_red[w]);
  const bool dead = m == -__builtin_inf();

  // ---- pass 2: fixed-point weights, one sum per chunk (the chunks of a group far below the maximum sum to 0), inclusive prefix
  for (int sc = wave; sc < nsup; sc += BT / 64) {
    const bool weigh = !dead && (!pr.use_cmax || cmax[sc] - m >= -OWN_SKIP_BELOW);  // (the same for every lane of the wave)
    const int k0 = sc * (64 * OWN_SUPER) + lane;
    if (!weigh) {
      for (int j = lane; j < OWN_SUPER && sc * OWN_SUPER + j < nch; j += 64) pre[sc * OWN_SUPER + j] = 0ull;
      continue;
    }
    int a = k0 / n_inner, b = k0 - a * n_inner;
    unsigned long long v[OWN_SUPER];
#pragma unroll
    for (int j = 0; j < OWN_SUPER; ++j) {
      const int k = k0 + (j << 6);
      v[j] = k < n ? pclean_fixw(score_ab(k, a, b) - m) : 0ull;
      a += pr.q64;
      b += pr.r64;
      if (b >= n_inner) {
        b -= n_inner;
        ++a;
      }
    }
#pragma unroll
    for (int j = 0; j < OWN_SUPER; ++j) {
      const int c = sc * OWN_SUPER + j;
      if (c >= nch) break;  // (the same for every lane of the wave)
      const unsigned long long t = own_wave_sum(v[j]);
      if (lane == 0) pre[c] = t;
    }
  }
  __syncthreads();
  if (wave == 0) {
    unsigned long long carry = 0ull;
    for (int base = 0; base < nch; base += 64) {
      const int i = base + lane;
      unsigned long long v = own_wave_scan(i < nch ? pre[i] : 0ull, lane) + carry;
      if (i < nch) pre[i] = v;
      carry = __shfl(v, 63, 64);
    }
  }
  __syncthreads();
  const unsigned long long U = pre[nch - 1];
  const double lse = pclean_lse_from_fix(m, U);

  // ---- the run's rows: one member per lane (own_leaf_kernel's draws)
  const int nd_eff = L.probe ? max(L.n_draws, 1) : 1;
  const int n_out = (m_hi - m_lo) * nd_eff;
  for (int q = tid; q < n_out; q += BT) {
    const int mem = L.members[m_lo + q / nd_eff], j = q % nd_eff;
    int row, pid;
    if (L.probe) {
      row = L.item_row[mem];
      pid = j;
      if (j == 0 && L.lse_out) L.lse_out[mem] = lse;
      if (L.n_draws <= 0) continue;
    } else {
      row = mem;
      if (row < L.win_lo || row >= L.win_hi) continue;
      const int i = row - L.win_lo;
      L.logml[i] += lse;
      if (L.keep[i]) continue;
      pid = L.chosen[i];
    }
    int res = n - 1;
    if (U != 0ull) {
      const uint32_t rng_row = (uint32_t)((int64_t)row + L.row_offset);
      const unsigned long long x = pclean_mulhi64(pclean_rand64(L.seed, rng_row, L.site, (uint32_t)pid, L.sweep), U);
      int a = 0, b = nch - 1;
      while (a < b) {  // the first chunk whose inclusive prefix exceeds x
        const int mid = (a + b) >> 1;
        if (pre[mid] > x)
          b = mid;
        else
          a = mid + 1;
      }
      unsigned long long acc = a ? pre[a - 1] : 0ull;
      int k = a << 6;
      const int k_end = min(n, k + 64) - 1;  // (the chunk's total exceeds x - acc: the walk stops inside it)
      for (; k < k_end; ++k) {
        acc += pclean_fixw(score(k) - m);
        if (acc > x) break;
      }
      res = k;
    }
    if (L.probe)
      L.draws_out[(size_t)mem * L.n_draws + j] = res;
    else
      L.vals[row] = res;
  }
}

// ---- exact marginals: the top options of every tuple run and the probability of every row's current value ----------------
#define OWN_MAX_TOP 8

struct OwnMarginal {
  const int32_t* piece_off;  // [pieces + 1] into members
  const int32_t* members;    // rows (index into the loaded rows)
  int32_t win_lo, win_hi;    // the active window (rows outside are left alone)
  int32_t top;               // 1 .. OWN_MAX_TOP
  const int32_t* vals;       // the leaf's current values, indexed by row (read when cur_prob is set)
  int32_t* top_option;       // [top][win_hi - win_lo]
  double* top_prob;          // [top][win_hi - win_lo]
  double* cur_prob;          // [win_hi - win_lo] or null
  int32_t* bad;              // {rows of the window with U == 0, the smallest of them}
};

// the order of the selection: the larger weight first, equal weights by the smaller option index (a free slot is (0, -1))
__device__ __forceinline__ bool own_before(unsigned long long ua, int ka, unsigned long long ub, int kb) {
  return ua > ub || (ua == ub && ka < kb);
}

// Passes 1 and 2 are own_leaf_kernel's, operation for operation (without the probe's outputs): m, every u_k and U are the
// sweep's.  Selection: in pass 2 every lane keeps the CAP first of ITS options (they reach it by ascending index) in
// registers; then `top` rounds of a workgroup-wide arg-max over the lanes' first entries, the winning lane moving on to its
// next.  CAP >= top; the result does not depend on it.
template <bool RESIDENT, int CAP>
__global__ __launch_bounds__(OWN_BT) void own_marginal_kernel(const OwnNodeDev nd, const DensDev dn, const OwnMarginal L) {
  __shared__ unsigned long long s_u[OWN_LDS_OPTIONS];
  __shared__ unsigned long long s_cs[OWN_LDS_OPTIONS / 64];
  __shared__ double s_red[OWN_BT / 64];
  __shared__ int s_obs[PCLEAN_MAX_TERMS];
  __shared__ unsigned long long s_wu[2][OWN_BT / 64];  // the waves' winners of a round (two rounds in flight)
  __shared__ int s_wk[2][OWN_BT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x;
  const int m_lo = L.piece_off[g], m_hi = L.piece_off[g + 1];
  const int n = nd.n_cand;
  {
    int any = 0;
    for (int q = m_lo + tid; q < m_hi; q += OWN_BT) {
      const int r = L.members[q];
      any |= (r >= L.win_lo && r < L.win_hi) ? 1 : 0;
    }
    if (!__syncthreads_or(any)) return;
  }
  {
    const int row0 = L.members[m_lo];
    for (int ti = 0; ti < nd.n_terms; ++ti)
      if (tid == ti) s_obs[ti] = nd.terms[ti].obs_col[row0];
  }
  __syncthreads();

  // ---- pass 1: scores and their maximum
  double* s = reinterpret_cast<double*>(s_u);
  double lmax = -__builtin_inf();
  for (int k = tid; k < n; k += OWN_BT) {
    const double sk = own_score(nd, dn, s_obs, k);
    if (RESIDENT) s[k] = sk;
    lmax = fmax(lmax, sk);
  }
  lmax = own_wave_max(lmax);
  if (lane == 0) s_red[wave] = lmax;
  __syncthreads();
  double m = s_red[0];
  for (int w = 1; w < OWN_BT / 64; ++w) m = fmax(m, s_red[w]);
  const bool dead = m == -__builtin_inf();

  // ---- pass 2: fixed-point weights, one sum per 64 options, inclusive prefix of the sums; the lane's best options
  unsigned long long lu[CAP];
  int lk[CAP];
#pragma unroll
  for (int j = 0; j < CAP; ++j) {
    lu[j] = 0ull;
    lk[j] = -1;
  }
  const int nch = (n + 63) >> 6;
  unsigned long long* pre = RESIDENT ? s_cs : s_u;
  if (RESIDENT) {
    for (int k = tid; k < n; k += OWN_BT) {
      const double sk = s[k];
      s_u[k] = dead ? 0ull : pclean_fixw(sk - m);
    }
    __syncthreads();
  }
  for (int c = wave; c < nch; c += OWN_BT / 64) {
    const int k = (c << 6) + lane;
    unsigned long long v = 0ull;
    if (k < n) v = RESIDENT ? s_u[k] : (dead ? 0ull : pclean_fixw(own_score(nd, dn, s_obs, k) - m));
    if (v > lu[CAP - 1]) {  // (k ascends: an equal weight seen earlier stays in front)
      lu[CAP - 1] = v;
      lk[CAP - 1] = k;
#pragma unroll
      for (int j = CAP - 1; j > 0; --j)
        if (lu[j] > lu[j - 1]) {
          const unsigned long long tu = lu[j];
          const int tk = lk[j];
          lu[j] = lu[j - 1];
          lk[j] = lk[j - 1];
          lu[j - 1] = tu;
          lk[j - 1] = tk;
        }
    }
    v = own_wave_sum(v);
    if (lane == 0) pre[c] = v;
  }
  __syncthreads();
  if (wave == 0) {
    unsigned long long carry = 0ull;
    for (int base = 0; base < nch; base += 64) {
      const int i = base + lane;
      unsigned long long v = own_wave_scan(i < nch ? pre[i] : 0ull, lane) + carry;
      if (i < nch) pre[i] = v;
      carry = __shfl(v, 63, 64);
    }
  }
  __syncthreads();
  const unsigned long long U = pre[nch - 1];
  const double Ud = (double)U;

  // ---- selection: round t takes the first of all lanes' entries
  int top_k[CAP];
  double top_p[CAP];
#pragma unroll
  for (int t = 0; t < CAP; ++t) {
    top_k[t] = -1;
    top_p[t] = 0.0;
    if (t >= L.top) continue;  // (uniform)
    unsigned long long u = lu[0];
    int k = lk[0];
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long uo = __shfl_xor(u, o, 64);
      const int ko = __shfl_xor(k, o, 64);
      if (own_before(uo, ko, u, k)) {
        u = uo;
        k = ko;
      }
    }
    if (lane == 0) {
      s_wu[t & 1][wave] = u;
      s_wk[t & 1][wave] = k;
    }
    __syncthreads();
    u = s_wu[t & 1][0];
    k = s_wk[t & 1][0];
    for (int w = 1; w < OWN_BT / 64; ++w)
      if (own_before(s_wu[t & 1][w], s_wk[t & 1][w], u, k)) {
        u = s_wu[t & 1][w];
        k = s_wk[t & 1][w];
      }
    if (u != 0ull) {
      top_k[t] = k;
      top_p[t] = (double)u / Ud;
      if (lk[0] == k) {
#pragma unroll
        for (int j = 0; j + 1 < CAP; ++j) {
          lu[j] = lu[j + 1];
          lk[j] = lk[j + 1];
        }
        lu[CAP - 1] = 0ull;
        lk[CAP - 1] = -1;
      }
    }
  }

  // ---- the run's rows: one member per lane
  const size_t nw = (size_t)(L.win_hi - L.win_lo);
  for (int q = m_lo + tid; q < m_hi; q += OWN_BT) {
    const int row = L.members[q];
    if (row < L.win_lo || row >= L.win_hi) continue;
    const size_t i = (size_t)(row - L.win_lo);
#pragma unroll
    for (int t = 0; t < CAP; ++t)
      if (t < L.top) {
        L.top_option[(size_t)t * nw + i] = top_k[t];
        L.top_prob[(size_t)t * nw + i] = top_p[t];
      }
    if (L.cur_prob) {
      const int cur = L.vals[row];
      double p = 0.0;
      if (U != 0ull && cur >= 0 && cur < n) {
        const unsigned long long uc = RESIDENT ? s_u[cur] : pclean_fixw(own_score(nd, dn, s_obs, cur) - m);
        p = (double)uc / Ud;
      }
      L.cur_prob[i] = p;
    }
    if (U == 0ull) {
      atomicAdd(&L.bad[0], 1);
      atomicMin(&L.bad[1], row);
    }
  }
}

// row_inference.jl:158-165 on equal weights — final_choice_kernel's operations (sweep.hip) with every weight 0.0
template <int PMAX>
__global__ void own_choice_kernel(int N, int P, int use_mh, const double* __restrict__ zero, const int32_t* __restrict__ vals0,
                                  uint64_t seed, uint32_t sweep, int64_t row_offset, int32_t* __restrict__ chosen,
                                  int32_t* __restrict__ keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  FixW<PMAX> f;
  fix_weights<PMAX>(zero, (size_t)0, P, f);
  const uint32_t rr = (uint32_t)((int64_t)i + row_offset);
  const bool csmc = vals0[i] >= 0;
  int c;
  if (use_mh && csmc && P >= 2) {
    const double Ud = (double)f.U;
    const double w0 = (double)f.u[0] / Ud, w1 = (double)f.u[PMAX > 1 ? 1 : 0] / Ud;
    double ratio = w1 / (1e-10 + w0);
    if (ratio > 1.0) ratio = 1.0;
    const double x = pclean_u01(pclean_rand64(seed, rr, PCLEAN_SITE_MH, 0u, sweep));
    c = (f.U != 0 && x < ratio) ? 1 : 0;
  } else {
    c = fix_pick<PMAX>(f, P, pclean_rand64(seed, rr, PCLEAN_SITE_FINAL, 0u, sweep));
  }
  chosen[i] = c;
  keep[i] = (csmc && c == 0) ? 1 : 0;
}

__global__ void own_fill_kernel(int32_t* __restrict__ p, size_t n, int32_t v) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

// bad[0] = rows of the window with logml == -inf, bad[1] = the smallest of them (preset to INT_MAX)
__global__ void own_bad_rows_kernel(int N, int win_lo, const double* __restrict__ logml, int32_t* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (logml[i] == -__builtin_inf()) {
    atomicAdd(&bad[0], 1);
    atomicMin(&bad[1], i + win_lo);
  }
}

// histogram of the current values: a workgroup counts in LDS (K <= OWN_LDS_OPTIONS) and adds its non-zero bins once
__global__ __launch_bounds__(256) void own_counts_kernel(int n_rows, int K, const int32_t* __restrict__ vals,
                                                         unsigned long long* __restrict__ hist) {
  __shared__ unsigned int s_h[OWN_LDS_OPTIONS];
  const bool lds = K <= OWN_LDS_OPTIONS;
  if (lds) {
    for (int k = threadIdx.x; k < K; k += blockDim.x) s_h[k] = 0u;
    __syncthreads();
  }
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n_rows; i += stride) {
    const int v = vals[i];
    if (v < 0 || v >= K) continue;
    if (lds)
      atomicAdd(&s_h[v], 1u);
    else
      atomicAdd(&hist[v], 1ull);
  }
  if (lds) {
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += blockDim.x)
      if (s_h[k]) atomicAdd(&hist[k], (unsigned long long)s_h[k]);
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
int check_plan(pclean_ctx* ctx, int32_t n_nodes, const pclean_node* nodes, int32_t n_terms, const pclean_term* terms) {
  for (int i = 0; i < n_nodes; ++i) {
    const pclean_node& n = nodes[i];
    if (n.kind != PCLEAN_NODE_LEAF || n.n_children != 0 || n.parent != -1)
      return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_load_own_block: node %d is not a leaf without a parent (an own block holds "
                                              "option lists only)", i);
    if (n.dummy_value != 0)
      return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_load_own_block: node %d has a dummy value (StringPrior / TimePrior own "
                                              "choices are not served)", i);
    if (n.table < 0 || n.table >= PCLEAN_MAX_TABLES) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_load_own_block: node %d: bad table", i);
    if (n.n_terms < 0 || n.term_begin < 0 || n.term_begin + n.n_terms > n_terms)
      return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_load_own_block: node %d: terms out of range", i);
    if (n.n_terms > PCLEAN_MAX_TERMS) return pclean_fail(ctx, PCLEAN_ERR_CAPACITY, "pclean_load_own_block: node %d: too many terms", i);
    for (int t = n.term_begin; t < n.term_begin + n.n_terms; ++t) {
      const pclean_term& tm = terms[t];
      if (tm.ctx_slot >= 0)
        return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_load_own_block: term %d has a ctx slot (an own block has no earlier "
                                                "slot to read)", t);
      if (tm.dens_kind == PCLEAN_DENS_NAME3)
        return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_load_own_block: term %d is a name3 term (three values of one candidate)", t);
      if (tm.dens_kind != PCLEAN_DENS_ADD_TYPOS && tm.dens_kind != PCLEAN_DENS_EQUAL && tm.dens_kind != PCLEAN_DENS_TABULATED)
        return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_load_own_block: term %d: density kind %d is not served", t, tm.dens_kind);
      if (tm.pair_table < 0 || tm.pair_table >= PCLEAN_MAX_TABLES || tm.obs_col < 0 || tm.cand_col < 0)
        return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_load_own_block: term %d: bad table or column", t);
    }
  }
  return PCLEAN_OK;
}

int ensure_vals(pclean_ctx* ctx, OwnBlock& b) {
  if (b.vals_rows == ctx->n_rows && (b.vals.p || ctx->n_rows == 0)) return PCLEAN_OK;
  const size_t n = b.leaves.size() * (size_t)ctx->n_rows;
  if (b.vals.alloc(n)) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  b.vals_rows = ctx->n_rows;
  if (n) {
    hipLaunchKernelGGL(own_fill_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, ctx->stream, b.vals.p, n, -1);
    HIPCHK(ctx, hipGetLastError());
  }
  return PCLEAN_OK;
}

// The leaf's device view: build_node_dev's (eval.hip) pointers, with the observed columns addressed by loaded row
int leaf_dev(pclean_ctx* ctx, const OwnLeaf& lf, OwnNodeDev& od) {
  Block tmp;
  tmp.nodes.push_back(lf.node);
  tmp.nodes[0].term_begin = 0;
  tmp.terms = lf.terms;
  NodeDev nd;
  ctx->prior_mode = false;
  const int rc = build_node_dev(ctx, tmp, 0, nd);
  if (rc) return rc;
  if (nd.n_cand < 1 || nd.n_cand > OWN_MAX_OPTIONS)
    return pclean_fail(ctx, PCLEAN_ERR_CAPACITY, "own block: an option list of %d options (1 .. %d are served)", nd.n_cand, OWN_MAX_OPTIONS);
  od.n_cand = nd.n_cand;
  od.n_terms = nd.n_terms;
  od.logp = nd.logc_full;
  for (int i = 0; i < nd.n_terms; ++i) {
    od.terms[i] = nd.terms[i];
    od.terms[i].obs_col -= ctx->active_begin;
  }
  return PCLEAN_OK;
}

// Rows ordered by their tuple of observed values over the leaf's terms (stable: ascending row within a tuple), cut into
// pieces of at most OWN_RUN_SPLIT rows; rebuilt when the observations were reloaded.
int ensure_groups(pclean_ctx* ctx, OwnLeaf& lf) {
  if (lf.grouped && lf.obs_version == ctx->obs_version) return PCLEAN_OK;
  const int N = ctx->n_rows, T = (int)lf.terms.size();
  std::vector<int32_t> cols((size_t)T * N);
  for (int t = 0; t < T; ++t) {
    if (lf.terms[t].obs_col >= ctx->n_cols) return pclean_fail(ctx, PCLEAN_ERR_ARG, "own block: observed column out of range");
    if (N) HIPCHK(ctx, hipMemcpyAsync(cols.data() + (size_t)t * N, ctx->obs.p + (size_t)lf.terms[t].obs_col * ctx->n_rows, (size_t)N * 4,
                                      hipMemcpyDeviceToHost, ctx->stream));
  }
  PCLEAN_SYNC(ctx);
  std::vector<int32_t> order(N);
  for (int i = 0; i < N; ++i) order[i] = i;
  auto less = [&](int32_t a, int32_t b) {
    for (int t = 0; t < T; ++t) {
      const int32_t x = cols[(size_t)t * N + a], y = cols[(size_t)t * N + b];
      if (x != y) return x < y;
    }
    return false;
  };
  if (T) std::stable_sort(order.begin(), order.end(), less);
  std::vector<int32_t> poff;
  lf.h_piece_of_row.assign(N, 0);
  lf.h_run_of_piece.clear();
  lf.h_run_len.clear();
  lf.n_runs = 0;
  lf.longest = 0;
  int i = 0;
  while (i < N) {
    int j = i + 1;
    while (j < N && !less(order[i], order[j])) ++j;  // (sorted: not less = same tuple)
    const int run = lf.n_runs++;
    lf.h_run_len.push_back(j - i);
    lf.longest = std::max(lf.longest, j - i);
    for (int p = i; p < j; p += OWN_RUN_SPLIT) {
      const int piece = (int)poff.size();
      poff.push_back(p);
      lf.h_run_of_piece.push_back(run);
      for (int q = p; q < std::min(j, p + OWN_RUN_SPLIT); ++q) lf.h_piece_of_row[order[q]] = piece;
    }
    i = j;
  }
  lf.n_pieces = (int)poff.size();
  poff.push_back(N);
  if (lf.piece_off.alloc(poff.size()) || lf.piece_rows.alloc(std::max(N, 1))) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  HIPCHK(ctx, hipMemcpy(lf.piece_off.p, poff.data(), poff.size() * 4, hipMemcpyHostToDevice));
  if (N) HIPCHK(ctx, hipMemcpy(lf.piece_rows.p, order.data(), (size_t)N * 4, hipMemcpyHostToDevice));
  lf.grouped = true;
  lf.obs_version = ctx->obs_version;
  return PCLEAN_OK;
}

// The leaf's option table is a full grid over its two value columns (pclean_set_options_cols: grid_outer_col, grid_inner) and
// every term reads one of them: the plan of own_product_kernel and its dynamic LDS.  False: the generic kernels — no grid,
// PCLEAN_NO_OWN_PRODUCT (the benchmark's baseline), or cached values and chunk sums beyond OWN_PRODUCT_LDS_MAX.
// PCLEAN_NO_OWN_SKIP (read once per process, for the benchmark alone) keeps the product kernel and leaves out the group maxima
// with the skip, as a plan does whose maxima do not fit: the same bits, every group weighed.
bool own_product_plan(pclean_ctx* ctx, const OwnLeaf& lf, const OwnNodeDev& od, OwnProductDev* pr, size_t* lds) {
  static const bool off = getenv("PCLEAN_NO_OWN_PRODUCT") != nullptr;
  static const bool no_skip = getenv("PCLEAN_NO_OWN_SKIP") != nullptr;  // (the benchmark's ablation: every group is weighed)
  const CandTable& t = ctx->cand[lf.node.table];
  if (off || od.n_terms < 1 || od.n_terms > PCLEAN_MAX_TERMS) return false;
  if (!t.valid || !t.is_options || t.logc_full.p != od.logp || t.grid_outer_col < 0 || t.n_cols != 2 || t.n_rows != od.n_cand ||
      t.grid_inner < 1 || t.n_rows % t.grid_inner)
    return false;
  pr->n_inner = t.grid_inner;
  pr->n_outer = t.n_rows / t.grid_inner;
  pr->n_chunks = (od.n_cand + 63) >> 6;
  pr->n_super = (pr->n_chunks + OWN_SUPER - 1) / OWN_SUPER;
  pr->q64 = 64 / pr->n_inner;
  pr->r64 = 64 % pr->n_inner;
  pr->total = 0;
  for (int ti = 0; ti < od.n_terms; ++ti) {
    int col = -1;
    for (int c = 0; c < 2; ++c)
      if (od.terms[ti].cand_col == t.cols.p + (size_t)c * t.n_rows) col = c;
    if (col < 0) return false;
    pr->inner[ti] = col != t.grid_outer_col;
    pr->off[ti] = pr->total;
    pr->total += pr->inner[ti] ? pr->n_inner : pr->n_outer;
  }
  for (int ti = od.n_terms; ti < PCLEAN_MAX_TERMS; ++ti) pr->inner[ti] = pr->off[ti] = 0;
  const size_t need = ((size_t)pr->total + (size_t)pr->n_chunks) * 8;
  if (need > OWN_PRODUCT_LDS_MAX) return false;  // the cached term values do not fit the LDS of a workgroup
  pr->use_cmax = !no_skip && need + (size_t)pr->n_super * 8 <= OWN_PRODUCT_LDS_MAX ? 1 : 0;
  *lds = need + (pr->use_cmax ? (size_t)pr->n_super * 8 : 0);
  return true;
}

int launch_leaf(pclean_ctx* ctx, const OwnLeaf& lf, const OwnNodeDev& od, const OwnLaunch& L, int n_pieces, OwnState* s) {
  if (n_pieces <= 0) return PCLEAN_OK;
  const DensDev dn{ctx->nb.p, ctx->logl.p, ctx->max_d + 1, 0, ctx->prob_same.p, ctx->prob_diff.p, ctx->logn.p};
  OwnProductDev pr;
  size_t lds = 0;
  if (own_product_plan(ctx, lf, od, &pr, &lds)) {
    if (!s->product_attr_set) {  // (a function attribute belongs to the device: once per context, not per process)
      HIPCHK(ctx, hipFuncSetAttribute((const void*)own_product_kernel<256>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)OWN_PRODUCT_LDS_MAX));
      HIPCHK(ctx, hipFuncSetAttribute((const void*)own_product_kernel<1024>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)OWN_PRODUCT_LDS_MAX));
      s->product_attr_set = true;
    }
    // a long grid: 16 wavefronts per workgroup — the LDS of such a plan leaves room for one or two workgroups on a CU, and
    // every wavefront still has 16 chunks and more to go through
    if (od.n_cand >= OWN_PRODUCT_WIDE)
      hipLaunchKernelGGL(own_product_kernel<1024>, dim3(n_pieces), dim3(1024), lds, ctx->stream, od, dn, L, pr);
    else
      hipLaunchKernelGGL(own_product_kernel<256>, dim3(n_pieces), dim3(256), lds, ctx->stream, od, dn, L, pr);
    s->stats.variants |= 4;
  } else if (od.n_cand <= OWN_LDS_OPTIONS) {
    hipLaunchKernelGGL(own_leaf_kernel<true>, dim3(n_pieces), dim3(OWN_BT), 0, ctx->stream, od, dn, L);
    s->stats.variants |= 1;
  } else {
    hipLaunchKernelGGL(own_leaf_kernel<false>, dim3(n_pieces), dim3(OWN_BT), 0, ctx->stream, od, dn, L);
    s->stats.variants |= 2;
  }
  HIPCHK(ctx, hipGetLastError());
  s->stats.n_workgroups += n_pieces;
  return PCLEAN_OK;
}

// the constant, the counters of impossible rows and the events around a call's launches
int ensure_aux(pclean_ctx* ctx, OwnState* s) {
  if (s->zero.p) return PCLEAN_OK;
  if (s->zero.alloc(1) || s->bad.alloc(2)) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  const double z = 0.0;
  HIPCHK(ctx, hipMemcpy(s->zero.p, &z, 8, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipEventCreate(&s->ev[0]));
  HIPCHK(ctx, hipEventCreate(&s->ev[1]));
  return PCLEAN_OK;
}

OwnBlock* find_block(pclean_ctx* ctx, int32_t block_id) {
  if (!ctx || block_id < 0 || block_id >= PCLEAN_MAX_BLOCKS || !ctx->own_state) return nullptr;
  OwnBlock& b = own(ctx)->block[block_id];
  return b.valid ? &b : nullptr;
}

void reset_stats(OwnState* s) {
  s->stats = pclean_own_stats{0, 0, 0, 0, 0, -1, OWN_LDS_OPTIONS, 0};
}

}  // namespace

void pclean_own_state_free(pclean_ctx* ctx) {
  if (!ctx || !ctx->own_state) return;
  OwnState* s = static_cast<OwnState*>(ctx->own_state);
  for (OwnBlock& b : s->block) {
    b.vals.release();
    for (OwnLeaf& lf : b.leaves) {
      lf.piece_off.release();
      lf.piece_rows.release();
    }
  }
  s->zero.release();
  s->bad.release();
  s->hist.release();
  for (hipEvent_t e : s->ev)
    if (e) (void)hipEventDestroy(e);
  delete s;
  ctx->own_state = nullptr;
}

extern "C" int pclean_load_own_block(pclean_ctx* ctx, int32_t block_id, int32_t n_nodes, const pclean_node* nodes, int32_t n_terms,
                                     const pclean_term* terms) {
  if (!ctx || block_id < 0 || block_id >= PCLEAN_MAX_BLOCKS || n_nodes <= 0 || n_nodes > 65535 || !nodes || n_terms < 0 ||
      (n_terms > 0 && !terms))
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_load_own_block: bad arguments");
  if (ctx->block[block_id].valid)
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_load_own_block: block %d is loaded as a block with a reference slot (a class "
                                            "that mixes the two kinds is not served)", block_id);
  const int rc = check_plan(ctx, n_nodes, nodes, n_terms, terms);
  if (rc) return rc;  // (nothing modified)
  HIPCHK(ctx, hipSetDevice(ctx->device));
  OwnBlock& b = own(ctx)->block[block_id];
  for (OwnLeaf& lf : b.leaves) {
    lf.piece_off.release();
    lf.piece_rows.release();
  }
  b.leaves.clear();
  b.leaves.resize(n_nodes);
  for (int i = 0; i < n_nodes; ++i) {
    b.leaves[i].node = nodes[i];
    b.leaves[i].terms.assign(terms + nodes[i].term_begin, terms + nodes[i].term_begin + nodes[i].n_terms);
  }
  b.vals.release();
  b.vals_rows = -1;
  b.valid = true;
  return PCLEAN_OK;
}

extern "C" int pclean_set_own(pclean_ctx* ctx, int32_t block_id, const int32_t* vals, int32_t n_rows) {
  OwnBlock* b = find_block(ctx, block_id);
  if (!b) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_set_own: block %d is not a loaded own block", block_id);
  if (vals && n_rows != ctx->n_rows) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_set_own: %d rows given, %d loaded", n_rows, ctx->n_rows);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  b->vals_rows = -1;  // (re-allocated and cleared)
  const int rc = ensure_vals(ctx, *b);
  if (rc) return rc;
  const size_t n = b->leaves.size() * (size_t)ctx->n_rows;
  if (vals && n) HIPCHK(ctx, hipMemcpyAsync(b->vals.p, vals, n * 4, hipMemcpyHostToDevice, ctx->stream));
  PCLEAN_SYNC(ctx);
  return PCLEAN_OK;
}

extern "C" int pclean_get_own(pclean_ctx* ctx, int32_t block_id, int32_t* vals_out) {
  OwnBlock* b = find_block(ctx, block_id);
  if (!b || !vals_out) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_get_own: block %d is not a loaded own block", block_id);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int rc = ensure_vals(ctx, *b);
  if (rc) return rc;
  const size_t n = b->leaves.size() * (size_t)ctx->n_rows;
  if (n) HIPCHK(ctx, hipMemcpyAsync(vals_out, b->vals.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCLEAN_SYNC(ctx);
  return PCLEAN_OK;
}

extern "C" int pclean_sweep_own(pclean_ctx* ctx, const pclean_infer_config* cfg, uint64_t seed, uint32_t sweep_idx,
                                int32_t* chosen_particle, double* logml) {
  if (!ctx || !cfg) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_sweep_own: bad arguments");
  if (!cfg->use_dd_proposals)
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_sweep_own: use_dd_proposals = 0 (prior proposals) is not served for own blocks");
  if (ctx->comm_ranks > 1) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_sweep_own: more than one rank is not served");
  const int use_mh = cfg->use_mh_instead_of_pg ? 1 : 0;
  const int P = use_mh ? 2 : cfg->num_particles;
  if (P < 1 || P > MAXP) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_sweep_own: num_particles must be 1 .. %d", MAXP);
  OwnState* s = ctx->own_state ? own(ctx) : nullptr;
  int first = -1;
  for (int bi = 0; s && bi < PCLEAN_MAX_BLOCKS; ++bi)
    if (s->block[bi].valid && first < 0) first = bi;
  if (first < 0) return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_sweep_own: no own block is loaded");
  const int win_lo = ctx->active_begin;
  const int N = ctx->active_count < 0 ? ctx->n_rows - win_lo : ctx->active_count;
  if (win_lo < 0 || N < 0 || win_lo + N > ctx->n_rows) return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_sweep_own: the active window lies outside the loaded rows");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  {
    const int rcb = begin_call(ctx);
    if (rcb) return rcb;
  }
  reset_stats(s);
  if (N == 0) return PCLEAN_OK;
  // everything that can fail for want of a table comes before the first write: a refused sweep changes nothing
  std::vector<OwnNodeDev> ods;
  for (int bi = 0; bi < PCLEAN_MAX_BLOCKS; ++bi) {
    OwnBlock& b = s->block[bi];
    if (!b.valid) continue;
    int rc = ensure_vals(ctx, b);
    if (rc) return rc;
    for (OwnLeaf& lf : b.leaves) {
      ods.emplace_back();
      rc = leaf_dev(ctx, lf, ods.back());
      if (!rc) rc = ensure_groups(ctx, lf);
      if (rc) return rc;
    }
  }
  {
    const int rc = ensure_aux(ctx, s);
    if (rc) return rc;
  }
  int32_t* d_chosen = scratch<int32_t>(ctx, N);
  int32_t* d_keep = scratch<int32_t>(ctx, N);
  double* d_logml = scratch<double>(ctx, N);
  if (!d_chosen || !d_keep || !d_logml) return pclean_fail(ctx, PCLEAN_ERR_HIP, "scratch alloc failed");
  const int64_t row_offset = st(ctx)->row_offset;
  {
    const int rc = dev_zero(ctx, d_logml, (size_t)N * 8);
    if (rc) return rc;
  }
  const int32_t bad0[2] = {0, 0x7fffffff};
  HIPCHK(ctx, hipMemcpyAsync(s->bad.p, bad0, 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipEventRecord(s->ev[0], ctx->stream));
  DISPATCH_PMAX(P, hipLaunchKernelGGL(own_choice_kernel<PMAX>, grid1(N), dim3(256), 0, ctx->stream, N, P, use_mh,
                                      (const double*)s->zero.p, (const int32_t*)(s->block[first].vals.p + win_lo), seed, sweep_idx,
                                      row_offset + win_lo, d_chosen, d_keep));
  HIPCHK(ctx, hipGetLastError());
  size_t li = 0;
  for (int bi = 0; bi < PCLEAN_MAX_BLOCKS; ++bi) {
    OwnBlock& b = s->block[bi];
    if (!b.valid) continue;
    for (size_t ni = 0; ni < b.leaves.size(); ++ni, ++li) {
      OwnLeaf& lf = b.leaves[ni];
      OwnLaunch L{};
      L.piece_off = lf.piece_off.p;
      L.members = lf.piece_rows.p;
      L.win_lo = win_lo;
      L.win_hi = win_lo + N;
      L.chosen = d_chosen;
      L.keep = d_keep;
      L.logml = d_logml;
      L.vals = b.vals.p + ni * (size_t)ctx->n_rows;
      L.row_offset = row_offset;
      L.seed = seed;
      L.sweep = sweep_idx;
      L.site = PCLEAN_SITE_NODE(bi, ni);
      const int rc = launch_leaf(ctx, lf, ods[li], L, lf.n_pieces, s);
      if (rc) return rc;
      s->stats.n_runs += lf.n_runs;
      s->stats.longest_run = std::max(s->stats.longest_run, lf.longest);
    }
  }
  hipLaunchKernelGGL(own_bad_rows_kernel, grid1(N), dim3(256), 0, ctx->stream, N, win_lo, (const double*)d_logml, s->bad.p);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(s->ev[1], ctx->stream));
  int32_t bad[2] = {0, 0};
  HIPCHK(ctx, hipMemcpyAsync(bad, s->bad.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (chosen_particle) HIPCHK(ctx, hipMemcpyAsync(chosen_particle, d_chosen, (size_t)N * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (logml) HIPCHK(ctx, hipMemcpyAsync(logml, d_logml, (size_t)N * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCLEAN_SYNC(ctx);
  ctx->timing = pclean_timing{};
  (void)hipEventElapsedTime(&ctx->timing.total_ms, s->ev[0], s->ev[1]);
  s->stats.impossible_rows = bad[0];
  s->stats.first_impossible_row = bad[0] ? bad[1] : -1;
  return finish_call(ctx);
}

extern "C" int pclean_score_own(pclean_ctx* ctx, int32_t block_id, int32_t node_id, int32_t n_items, const int32_t* rows,
                                uint64_t seed, uint32_t sweep, int32_t n_draws, double* lse, double* scores, int32_t* draws) {
  OwnBlock* b = find_block(ctx, block_id);
  if (!b) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_score_own: block %d is not a loaded own block", block_id);
  if (node_id < 0 || node_id >= (int)b->leaves.size() || n_items <= 0 || !rows || n_draws < 0 || (n_draws > 0 && !draws))
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_score_own: bad arguments");
  const int win_lo = ctx->active_begin;
  const int N = ctx->active_count < 0 ? ctx->n_rows - win_lo : ctx->active_count;
  for (int t = 0; t < n_items; ++t)
    if (rows[t] < 0 || rows[t] >= N) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_score_own: row %d lies outside the active window", rows[t]);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  {
    const int rcb = begin_call(ctx);
    if (rcb) return rcb;
  }
  OwnState* s = own(ctx);
  reset_stats(s);
  OwnLeaf& lf = b->leaves[node_id];
  OwnNodeDev od;
  int rc = leaf_dev(ctx, lf, od);
  if (!rc) rc = ensure_groups(ctx, lf);
  if (rc) return rc;
  // the items grouped by the piece of a tuple run their row lies in (stable): the sweep's grouping, restricted to the items
  std::vector<int32_t> h_row(n_items), order(n_items), poff;
  for (int t = 0; t < n_items; ++t) {
    h_row[t] = rows[t] + win_lo;
    order[t] = t;
  }
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t c) { return lf.h_piece_of_row[h_row[a]] < lf.h_piece_of_row[h_row[c]]; });
  std::set<int32_t> runs;
  for (int q = 0; q < n_items; ++q) {
    const int piece = lf.h_piece_of_row[h_row[order[q]]];
    if (q == 0 || piece != lf.h_piece_of_row[h_row[order[q - 1]]]) poff.push_back(q);
    if (runs.insert(lf.h_run_of_piece[piece]).second) s->stats.longest_run = std::max(s->stats.longest_run, lf.h_run_len[lf.h_run_of_piece[piece]]);
  }
  const int n_pieces = (int)poff.size();
  poff.push_back(n_items);
  s->stats.n_runs = (int)runs.size();
  const int K = od.n_cand;
  int32_t* d_row = scratch<int32_t>(ctx, n_items);
  int32_t* d_order = scratch<int32_t>(ctx, n_items);
  int32_t* d_poff = scratch<int32_t>(ctx, poff.size());
  double* d_lse = scratch<double>(ctx, n_items);
  double* d_scores = scores ? scratch<double>(ctx, (size_t)n_items * K) : nullptr;
  int32_t* d_draws = n_draws ? scratch<int32_t>(ctx, (size_t)n_items * n_draws) : nullptr;
  if (!d_row || !d_order || !d_poff || !d_lse || (scores && !d_scores) || (n_draws && !d_draws))
    return pclean_fail(ctx, PCLEAN_ERR_HIP, "scratch alloc failed");
  HIPCHK(ctx, hipMemcpyAsync(d_row, h_row.data(), (size_t)n_items * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_order, order.data(), (size_t)n_items * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(d_poff, poff.data(), poff.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  OwnLaunch L{};
  L.piece_off = d_poff;
  L.members = d_order;
  L.item_row = d_row;
  L.probe = 1;
  L.n_draws = n_draws;
  L.lse_out = d_lse;
  L.scores_out = d_scores;
  L.draws_out = d_draws;
  L.row_offset = st(ctx)->row_offset;
  L.seed = seed;
  L.sweep = sweep;
  L.site = PCLEAN_SITE_NODE(block_id, node_id);
  rc = launch_leaf(ctx, lf, od, L, n_pieces, s);
  if (rc) return rc;
  if (lse) HIPCHK(ctx, hipMemcpyAsync(lse, d_lse, (size_t)n_items * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (scores) HIPCHK(ctx, hipMemcpyAsync(scores, d_scores, (size_t)n_items * K * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (n_draws) HIPCHK(ctx, hipMemcpyAsync(draws, d_draws, (size_t)n_items * n_draws * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCLEAN_SYNC(ctx);  // (h_row / order / poff are read by the copies queued above)
  return finish_call(ctx);
}

extern "C" int pclean_own_marginals(pclean_ctx* ctx, int32_t block_id, int32_t node_id, int32_t top, int32_t* top_option,
                                    double* top_prob, double* cur_prob) {
  OwnBlock* b = find_block(ctx, block_id);
  if (!b) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_own_marginals: block %d is not a loaded own block", block_id);
  if (node_id < 0 || node_id >= (int)b->leaves.size())
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_own_marginals: block %d has no node %d", block_id, node_id);
  if (top < 1 || top > OWN_MAX_TOP) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_own_marginals: top must be 1 .. %d", OWN_MAX_TOP);
  if (!top_option || !top_prob) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_own_marginals: null outputs");
  const int win_lo = ctx->active_begin;
  const int N = ctx->active_count < 0 ? ctx->n_rows - win_lo : ctx->active_count;
  if (win_lo < 0 || N < 0 || win_lo + N > ctx->n_rows) return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_own_marginals: the active window lies outside the loaded rows");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  {
    const int rcb = begin_call(ctx);
    if (rcb) return rcb;
  }
  OwnState* s = own(ctx);
  reset_stats(s);
  if (N == 0) return PCLEAN_OK;
  OwnLeaf& lf = b->leaves[node_id];
  OwnNodeDev od;
  int rc = leaf_dev(ctx, lf, od);
  if (!rc) rc = ensure_groups(ctx, lf);
  if (!rc && cur_prob) rc = ensure_vals(ctx, *b);
  if (!rc) rc = ensure_aux(ctx, s);
  if (rc) return rc;
  int32_t* d_opt = scratch<int32_t>(ctx, (size_t)top * N);
  double* d_prob = scratch<double>(ctx, (size_t)top * N);
  double* d_cur = cur_prob ? scratch<double>(ctx, N) : nullptr;
  if (!d_opt || !d_prob || (cur_prob && !d_cur)) return pclean_fail(ctx, PCLEAN_ERR_HIP, "scratch alloc failed");
  const int32_t bad0[2] = {0, 0x7fffffff};
  HIPCHK(ctx, hipMemcpyAsync(s->bad.p, bad0, 8, hipMemcpyHostToDevice, ctx->stream));
  OwnMarginal L{};
  L.piece_off = lf.piece_off.p;
  L.members = lf.piece_rows.p;
  L.win_lo = win_lo;
  L.win_hi = win_lo + N;
  L.top = top;
  L.vals = cur_prob ? b->vals.p + (size_t)node_id * ctx->n_rows : nullptr;
  L.top_option = d_opt;
  L.top_prob = d_prob;
  L.cur_prob = d_cur;
  L.bad = s->bad.p;
  const DensDev dn{ctx->nb.p, ctx->logl.p, ctx->max_d + 1, 0, ctx->prob_same.p, ctx->prob_diff.p, ctx->logn.p};
  const bool resident = od.n_cand <= OWN_LDS_OPTIONS;
  HIPCHK(ctx, hipEventRecord(s->ev[0], ctx->stream));
  if (lf.n_pieces > 0) {  // (a lane keeps 1 entry for top == 1, OWN_MAX_TOP otherwise)
    const dim3 grid(lf.n_pieces), block(OWN_BT);
    if (resident && top == 1)
      hipLaunchKernelGGL((own_marginal_kernel<true, 1>), grid, block, 0, ctx->stream, od, dn, L);
    else if (resident)
      hipLaunchKernelGGL((own_marginal_kernel<true, OWN_MAX_TOP>), grid, block, 0, ctx->stream, od, dn, L);
    else if (top == 1)
      hipLaunchKernelGGL((own_marginal_kernel<false, 1>), grid, block, 0, ctx->stream, od, dn, L);
    else
      hipLaunchKernelGGL((own_marginal_kernel<false, OWN_MAX_TOP>), grid, block, 0, ctx->stream, od, dn, L);
    HIPCHK(ctx, hipGetLastError());
    s->stats.variants |= resident ? 1 : 2;
    s->stats.n_workgroups += lf.n_pieces;
  }
  HIPCHK(ctx, hipEventRecord(s->ev[1], ctx->stream));
  s->stats.n_runs = lf.n_runs;
  s->stats.longest_run = lf.longest;
  int32_t bad[2] = {0, 0};
  HIPCHK(ctx, hipMemcpyAsync(bad, s->bad.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(top_option, d_opt, (size_t)top * N * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(top_prob, d_prob, (size_t)top * N * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (cur_prob) HIPCHK(ctx, hipMemcpyAsync(cur_prob, d_cur, (size_t)N * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCLEAN_SYNC(ctx);
  ctx->timing = pclean_timing{};
  (void)hipEventElapsedTime(&ctx->timing.total_ms, s->ev[0], s->ev[1]);
  s->stats.impossible_rows = bad[0];
  s->stats.first_impossible_row = bad[0] ? bad[1] : -1;
  return finish_call(ctx);
}

extern "C" int pclean_own_counts(pclean_ctx* ctx, int32_t block_id, int32_t node_id, int64_t* counts) {
  OwnBlock* b = find_block(ctx, block_id);
  if (!b || node_id < 0 || node_id >= (int)b->leaves.size() || !counts)
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_own_counts: block %d node %d is not a node of a loaded own block", block_id, node_id);
  const CandTable& t = ctx->cand[b->leaves[node_id].node.table];
  if (!t.valid || !t.is_options) return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_own_counts: the node's option table is not set");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int rc = ensure_vals(ctx, *b);
  if (rc) return rc;
  OwnState* s = own(ctx);
  const int K = t.n_rows;
  if (s->hist.alloc(K)) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  HIPCHK(ctx, hipMemsetAsync(s->hist.p, 0, (size_t)K * 8, ctx->stream));
  if (ctx->n_rows) {
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)ctx->n_rows + 255) / 256, 1024);
    hipLaunchKernelGGL(own_counts_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->n_rows, K,
                       (const int32_t*)(b->vals.p + (size_t)node_id * ctx->n_rows), s->hist.p);
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, hipMemcpyAsync(counts, s->hist.p, (size_t)K * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCLEAN_SYNC(ctx);
  return PCLEAN_OK;
}

extern "C" int pclean_get_own_stats(pclean_ctx* ctx, pclean_own_stats* out) {
  if (!ctx || !out) return PCLEAN_ERR_ARG;
  if (ctx->own_state)
    *out = own(ctx)->stats;
  else
    *out = pclean_own_stats{0, 0, 0, 0, 0, -1, OWN_LDS_OPTIONS, 0};
  return PCLEAN_OK;
}
