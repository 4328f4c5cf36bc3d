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
// own_star_kernel serves a star (pclean_link_own_star): an index and two to four choices indexed by it, as a head node and one
// arm node per dependent.  The dependents are independent given the index: every one is summed out per index value in fixed
// point, the index is drawn, then every dependent given it (see the kernel).
//
// own_marginal_kernel (pclean_own_marginals) reports what the sweep holds before it draws: passes 1 and 2 as above, then
// instead of the draws the `top` options of largest u_k (ties: the smaller index) with u_k / U, and u_cur / U of every row's
// current value.  It writes no value.
#include "sweep_internal.h"
#include "../../include/pclean_ownq.h"
#include "own_star_check.h"

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
  // Gaussian terms (pclean_add_own_gauss) in attach order, and the exponent of each one's fixed-point statistics
  std::vector<pclean_gauss> gauss;
  std::vector<int32_t> gauss_e;
};

// a star (pclean_link_own_star): the head's node, its arms' nodes, and the grouping over the terms of all of them
struct OwnStar {
  int head = -1;
  std::vector<int> arms;
  OwnLeaf grp;                          // (terms: the head's, then every arm's; node unused)
  std::vector<uint64_t> cols_version;   // of the nodes' option tables when the grid was last checked
  std::vector<int32_t> kj;
  DevBuf<double> cmax;                  // [n_arms][ka]: the bound of every arm's prior row, as of the last launch
};

struct OwnBlock {
  bool valid = false;
  std::vector<OwnLeaf> leaves;
  std::vector<OwnStar> stars;
  std::vector<int> star_of;  // per leaf: its star, -1: none
  DevBuf<int32_t> vals;  // [n_leaves][vals_rows]
  int vals_rows = 0;
};

struct OwnState {
  OwnBlock block[PCLEAN_MAX_BLOCKS];
  pclean_own_stats stats = {0, 0, 0, 0, 0, -1, OWN_LDS_OPTIONS, 0};
  DevBuf<double> zero;       // one 0.0: the equal weights of the final choice
  DevBuf<int32_t> bad;       // {rows with logml == -inf, the smallest of them}
  DevBuf<unsigned long long> hist;
  DevBuf<unsigned long long> gstat;  // pclean_own_gauss_stats: [count | qsum]
  DevBuf<unsigned long long> star_ctr;  // own_star_kernel: {index values weighed, skipped}
  bool star_attr_set = false;
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

// ---- Gaussian leaf: numeric observations make every row its own tuple -------------------------------------------------------
// (pclean_add_own_gauss; model.py, _lower_own_block.)  The static grouping stays that of the STRING terms' observations (a leaf
// without string terms is one run cut into pieces); a workgroup takes a piece:
//   phase 1  every string term once per latent value of the column it reads (own_score's rules), the doubles into LDS —
//            indexed by the VALUE cand_col[k], so nothing rests on the table being recognised as a grid (1 x n, n x 1).  A
//            plan whose values exceed OWN_GAUSS_LDS_MAX evaluates the terms per option instead (the same doubles).
//   phase 2  the rows of the piece are dealt to groups of W = min(64, next power of two >= K) lanes, 64 / W rows per
//            wavefront at a time; the lanes of a group run over the options, step c covers options c W .. c W + W - 1 (only
//            W = 64 has more than one step, at most 64 of them).  Per row three passes, nothing in LDS:
//              1  s_k = logp[k] + string terms in plan order + per present number gauss_add_term, in attach order; maximum
//              2  u_k = fixw(s_k - m), one group sum per step, lane c keeps step c's total; one inclusive scan: U, lse
//              3  x = mulhi64(R, U): the step by ballot on the prefix, its W weights again, scanned, the option by ballot —
//                 min{k : u_0 + .. + u_k > x}, as own_leaf_kernel finds it
//            (the scores of step 0 stay in a register; further steps are recomputed from the cached values.)
// MARG: instead of pass 3, `top` rounds of a group arg-max over u_k (equal weights: the smaller index), each round taking
// only what comes after the last winner in that order; u_k / U; cur_prob by own_marginal_kernel's rule.
// Every shuffle and ballot is executed by all 64 lanes: rows past the piece's end or outside the window compute on the
// piece's first row and write nothing.
#define OWN_GAUSS_MAX_OPTIONS 4096
#define OWN_GAUSS_LDS_MAX ((size_t)60 * 1024)  // cached term values (within the default dynamic-LDS limit of a launch)

struct OwnGaussDev {
  int32_t n_gauss, n_cols, lw, cached;  // lw: log2 of the lanes per row
  int32_t local_n[2];
  const int32_t* col[2];  // the option table's value columns (col[1] null: one column)
  int32_t off[PCLEAN_MAX_TERMS];  // cached values of string term ti: tv[off[ti] + latent value]
  GaussDev g[PCLEAN_MAX_GAUSS];
};

// one string term for observed value o and latent value val (own_score's body; the caller skips a non-tabulated term of a
// missing observation)
__device__ __forceinline__ double own_term_value(const TermDev& tm, const DensDev& dn, int o, int val) {
  if (tm.dens_kind == PCLEAN_DENS_TABULATED) {
    const int c = o < 0 ? 3 : ((int)tm.pair[(size_t)o * tm.n_lat + val] & 3);
    return tm.cls[(size_t)val * 4 + c];
  }
  const size_t idx = (size_t)o * tm.n_lat + val;
  const int d = tm.elem_bytes == 1 ? (int)tm.pair[idx] : (int)((const uint16_t*)tm.pair)[idx];
  return own_term_density(tm, dn, d, val);
}

__device__ __forceinline__ int own_gauss_no_val(const GaussDev&, int) { return 0; }  // (every index dimension is an option column)

// the ONE place where the score of option k for `row` is written: own_score's sum, then gauss_add_term per present number
__device__ __forceinline__ double own_gauss_score(const OwnNodeDev& nd, const DensDev& dn, const OwnGaussDev& gd, const double* tv,
                                                  const int* obs, unsigned int skip, int row, const double* xv, int k) {
  double sk = nd.logp[k];
  for (int ti = 0; ti < nd.n_terms; ++ti) {
    if ((skip >> ti) & 1u) continue;
    const TermDev& tm = nd.terms[ti];
    const int val = tm.cand_col[k];
    sk += gd.cached ? tv[gd.off[ti] + val] : own_term_value(tm, dn, obs[ti], val);
  }
  const int l0 = gd.col[0][k], l1 = gd.n_cols > 1 ? gd.col[1][k] : 0;
  if ((unsigned)l0 >= (unsigned)gd.local_n[0] || (unsigned)l1 >= (unsigned)gd.local_n[1]) return -__builtin_inf();
#pragma unroll
  for (int gi = 0; gi < PCLEAN_MAX_GAUSS; ++gi) {
    if (gi >= gd.n_gauss) break;
    const double x = xv[gi];
    if (x != x) continue;  // (a missing number: the term is skipped)
    int ls[2];
    const int base = gauss_index_base(gd.g[gi], own_gauss_no_val, ls);
    sk = gauss_add_term(gd.g[gi], sk, x, row, nullptr, base, ls, l0, l1);
  }
  return sk;
}

// the lanes of this lane's group (W = 1 << lw of them) for which pred holds, bit 0 = the group's first lane
__device__ __forceinline__ unsigned long long own_group_ballot(int pred, int lane, int lw) {
  const unsigned long long b = __ballot(pred);
  if (lw == 6) return b;
  const int W = 1 << lw;
  return (b >> (lane & ~(W - 1))) & ((1ull << W) - 1ull);
}

template <bool MARG>
__global__ __launch_bounds__(OWN_BT) void own_gauss_kernel(const OwnNodeDev nd, const DensDev dn, const OwnGaussDev gd,
                                                           const OwnLaunch L, const OwnMarginal M) {
  extern __shared__ __attribute__((aligned(16))) unsigned char own_smem[];
  __shared__ int s_obs[PCLEAN_MAX_TERMS];
  double* tv = reinterpret_cast<double*>(own_smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* piece_off = MARG ? M.piece_off : L.piece_off;
  const int32_t* members = MARG ? M.members : L.members;
  const int win_lo = MARG ? M.win_lo : L.win_lo, win_hi = MARG ? M.win_hi : L.win_hi;
  const bool probe = !MARG && L.probe;
  const int m_lo = piece_off[blockIdx.x], m_hi = piece_off[blockIdx.x + 1];
  const int n = nd.n_cand;
  if (!probe) {  // a run none of whose rows lies in the window has nothing to do
    int any = 0;
    for (int q = m_lo + tid; q < m_hi; q += OWN_BT) {
      const int r = members[q];
      any |= (r >= win_lo && r < win_hi) ? 1 : 0;
    }
    if (!__syncthreads_or(any)) return;
  }
  {
    const int row0 = probe ? L.item_row[members[m_lo]] : members[m_lo];
    for (int ti = 0; ti < nd.n_terms; ++ti)
      if (tid == ti) s_obs[ti] = nd.terms[ti].obs_col[row0];
  }
  __syncthreads();

  // ---- phase 1: the string terms, once per latent value
  unsigned int skip = 0;
  for (int ti = 0; ti < nd.n_terms; ++ti) {
    const TermDev& tm = nd.terms[ti];
    const int o = s_obs[ti];
    if (tm.dens_kind != PCLEAN_DENS_TABULATED && o < 0) {  // a missing observation: the term adds nothing
      skip |= 1u << ti;
      continue;
    }
    if (!gd.cached) continue;
    double* dst = tv + gd.off[ti];
    for (int val = tid; val < tm.n_lat; val += OWN_BT) dst[val] = own_term_value(tm, dn, o, val);
  }
  __syncthreads();

  // ---- phase 2: a group of W lanes per row
  const int lw = gd.lw, W = 1 << lw, rpw = 64 >> lw;
  const int gl = lane & (W - 1), sub = lane >> lw;
  const int steps = (n + W - 1) >> lw;  // (W < 64: one)
  const int n_mem = m_hi - m_lo;
  const size_t nw = (size_t)(win_hi - win_lo);
  for (int base = 0; base < n_mem; base += (OWN_BT / 64) * rpw) {
    const int qi = base + wave * rpw + sub;
    const bool valid = qi < n_mem;
    const int mem = members[m_lo + (valid ? qi : 0)];
    const int row = probe ? L.item_row[mem] : mem;
    const bool live = valid && (probe || (row >= win_lo && row < win_hi));
    double xv[PCLEAN_MAX_GAUSS];
#pragma unroll
    for (int gi = 0; gi < PCLEAN_MAX_GAUSS; ++gi) xv[gi] = gi < gd.n_gauss ? gd.g[gi].x[row] : 0.0;
    auto score = [&](int k) -> double { return own_gauss_score(nd, dn, gd, tv, s_obs, skip, row, xv, k); };

    // pass 1: scores and their maximum
    const double s0 = gl < n ? score(gl) : -__builtin_inf();
    double m = s0;
    if (!MARG && probe && L.scores_out && live && gl < n) L.scores_out[(size_t)mem * n + gl] = s0;
    for (int c = 1; c < steps; ++c) {
      const int k = (c << lw) + gl;
      if (k < n) {
        const double sk = score(k);
        if (!MARG && probe && L.scores_out && live) L.scores_out[(size_t)mem * n + k] = sk;
        m = fmax(m, sk);
      }
    }
    for (int o = W >> 1; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));  // (o < W: the partner lies in the group)
    const bool dead = m == -__builtin_inf();

    // pass 2: fixed-point weights, one sum per step (lane c keeps step c's), their inclusive prefix
    unsigned long long pre = 0ull;
    for (int c = 0; c < steps; ++c) {
      const int k = (c << lw) + gl;
      unsigned long long v = (k < n && !dead) ? pclean_fixw((c == 0 ? s0 : score(k)) - m) : 0ull;
      for (int o = W >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (gl == c) pre = v;
    }
    for (int o = 1; o < W; o <<= 1) {
      const unsigned long long t = __shfl_up(pre, o, 64);
      if (gl >= o) pre += t;
    }
    const unsigned long long U = __shfl(pre, (lane & ~(W - 1)) + W - 1, 64);
    const double lse = pclean_lse_from_fix(m, U);

    if (!MARG) {
      // pass 3: the draws
      int n_dr = 1, pid0 = 0;
      bool draw = live;
      if (probe) {
        if (live && gl == 0 && L.lse_out) L.lse_out[mem] = lse;
        n_dr = L.n_draws;
      } else if (live) {
        const int i = row - win_lo;
        if (gl == 0) L.logml[i] += lse;  // (a row lies in exactly one run of the leaf; the leaves are launched one after the other)
        draw = !L.keep[i];
        pid0 = L.chosen[i];
      }
      for (int j = 0; j < n_dr; ++j) {  // (uniform: the probe's n_draws, the sweep's one)
        const int pid = probe ? j : pid0;
        const uint32_t rng_row = (uint32_t)((int64_t)row + L.row_offset);
        const unsigned long long x = pclean_mulhi64(pclean_rand64(L.seed, rng_row, L.site, (uint32_t)pid, L.sweep), U);
        int chunk = 0;
        unsigned long long acc0 = 0ull;
        if (steps > 1) {  // (W == 64: one row per wavefront, so this is uniform) the first step whose inclusive prefix exceeds x
          const unsigned long long cm = __ballot(lane < steps && pre > x);
          chunk = cm ? __builtin_ctzll(cm) : steps - 1;
          acc0 = __shfl(pre, chunk ? chunk - 1 : 0, 64);
          if (!chunk) acc0 = 0ull;
        }
        const int k = (chunk << lw) + gl;
        unsigned long long v = (k < n && !dead) ? pclean_fixw((chunk == 0 ? s0 : score(k)) - m) : 0ull;
        for (int o = 1; o < W; o <<= 1) {
          const unsigned long long t = __shfl_up(v, o, 64);
          if (gl >= o) v += t;
        }
        const unsigned long long hit = own_group_ballot(k < n && acc0 + v > x, lane, lw);
        int res = n - 1;
        if (U != 0ull) res = hit ? (chunk << lw) + __builtin_ctzll(hit) : min(n, (chunk + 1) << lw) - 1;
        if (draw && gl == 0) {
          if (probe)
            L.draws_out[(size_t)mem * L.n_draws + j] = res;
          else
            L.vals[row] = res;
        }
      }
    } else {
      // the `top` options of largest weight, then the probability of the current value
      const double Ud = (double)U;
      unsigned long long last_u = 0ull;
      int last_k = -1;
      bool open = true;  // (a round that finds nothing: every later one finds nothing either)
      for (int t = 0; t < M.top; ++t) {
        unsigned long long bu = 0ull;
        int bk = -1;
        for (int c = 0; c < steps && open; ++c) {
          const int k = (c << lw) + gl;
          if (k >= n || dead) continue;
          const unsigned long long u = pclean_fixw((c == 0 ? s0 : score(k)) - m);
          if (u != 0ull && (last_k < 0 || own_before(last_u, last_k, u, k)) && own_before(u, k, bu, bk)) {
            bu = u;
            bk = k;
          }
        }
        for (int o = W >> 1; o > 0; o >>= 1) {
          const unsigned long long uo = __shfl_xor(bu, o, 64);
          const int ko = __shfl_xor(bk, o, 64);
          if (own_before(uo, ko, bu, bk)) {
            bu = uo;
            bk = ko;
          }
        }
        if (bu != 0ull) {
          last_u = bu;
          last_k = bk;
        } else {
          open = false;
        }
        if (live && gl == 0) {
          const size_t i = (size_t)(row - win_lo);
          M.top_option[(size_t)t * nw + i] = bu != 0ull ? bk : -1;
          M.top_prob[(size_t)t * nw + i] = bu != 0ull ? (double)bu / Ud : 0.0;
        }
      }
      if (live && gl == 0) {
        const size_t i = (size_t)(row - win_lo);
        if (M.cur_prob) {
          const int cur = M.vals[row];
          double p = 0.0;
          if (U != 0ull && cur >= 0 && cur < n) p = (double)pclean_fixw(score(cur) - m) / Ud;
          M.cur_prob[i] = p;
        }
        if (U == 0ull) {
          atomicAdd(&M.bad[0], 1);
          atomicMin(&M.bad[1], row);
        }
      }
    }
  }
}

// pclean_own_gauss_stats: count and fixed-point sum of the backward values per mean index, over the rows' current options.
// The unit and bx are gauss_add_term's (u from the option column the term names; the derived column if the unit has one,
// else x * t_scale[u]).  n_mean <= OWN_GAUSS_STAT_LDS: a workgroup adds up in LDS and flushes its non-zero entries once.
#define OWN_GAUSS_STAT_LDS 1024
__global__ __launch_bounds__(256) void own_gauss_stats_kernel(int n_rows, int K, const int32_t* __restrict__ vals, const OwnGaussDev gd,
                                                              int gi, int n_mean, double scale, unsigned long long* __restrict__ count,
                                                              unsigned long long* __restrict__ qsum) {
  __shared__ unsigned long long s_q[OWN_GAUSS_STAT_LDS];
  __shared__ unsigned int s_c[OWN_GAUSS_STAT_LDS];
  const bool lds = n_mean <= OWN_GAUSS_STAT_LDS;
  if (lds) {
    for (int j = threadIdx.x; j < n_mean; j += blockDim.x) {
      s_q[j] = 0ull;
      s_c[j] = 0u;
    }
    __syncthreads();
  }
  const GaussDev& g = gd.g[gi];
  int ls[2];
  const int base = gauss_index_base(g, own_gauss_no_val, ls);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n_rows; i += stride) {
    const int v = vals[i];
    if (v < 0 || v >= K) continue;
    const double x = g.x[i];
    if (x != x) continue;
    const int l0 = gd.col[0][v], l1 = gd.n_cols > 1 ? gd.col[1][v] : 0;
    if ((unsigned)l0 >= (unsigned)gd.local_n[0] || (unsigned)l1 >= (unsigned)gd.local_n[1]) continue;
    const int idx = base + ls[0] * l0 + ls[1] * l1;
    if (idx < 0 || idx >= n_mean) continue;
    const int u = g.t_kind == PCLEAN_GSRC_LOCAL ? (g.t_src == 0 ? l0 : l1) : 0;
    const double bx = g.tx[u] ? g.tx[u][i] : x * g.t_scale[u];
    if (!(fabs(bx) <= 1.7976931348623157e308)) continue;  // (NaN or infinite)
    const unsigned long long q = (unsigned long long)pclean_ownq(bx, scale);  // (two's complement: the sum is the signed one)
    if (lds) {
      atomicAdd(&s_c[idx], 1u);
      atomicAdd(&s_q[idx], q);
    } else {
      atomicAdd(&count[idx], 1ull);
      atomicAdd(&qsum[idx], q);
    }
  }
  if (lds) {
    __syncthreads();
    for (int j = threadIdx.x; j < n_mean; j += blockDim.x)
      if (s_c[j]) {
        atomicAdd(&count[j], (unsigned long long)s_c[j]);
        atomicAdd(&qsum[j], s_q[j]);
      }
  }
}

// ---- star: several dependents on one index, enumerated collapsed ------------------------------------------------------------
// (pclean_link_own_star; model.py, _lower_own_star.)  The head node holds the index a with its terms, arm j holds dependent
// b_j on the grid a * K_j + b with prior log theta_j[a][b] alone.  The dependents are independent given the index, so
//   t_j(a, b) = log theta_j[a K_j + b] + arm j's terms at b (plan order)      M_j(a) = max_b t_j    v_j = fixw(t_j - M_j(a))
//   V_j(a) = sum_b v_j      L_j(a) = lse_from_fix(M_j(a), V_j(a))
//   S(a) = logp[a] + the head's terms at a + L_1(a) + .. + L_D(a)             m = max_a S   u_a = fixw(S(a) - m)   U = sum u_a
// and the row draws a from u, then every b_j from v_j(a, .).  One workgroup per piece of a tuple run over the terms of ALL nodes:
//   phase 1  every term once per value of the factor it reads, into LDS (own_product_kernel's phase 1)
//   phase 2  H(a) = logp[a] + head terms into S[a];  per arm the maximum of its cached term sums
//   skip     B(a) = H(a) + sum_j (taumax_j + cmax_j[a]) >= S(a), cmax_j[a] = max_b log theta_j[a][b] + log K_j (own_star_cmax_kernel,
//            from the table as it is at the call).  S is evaluated exactly at a* = argmax B; an a with B(a) < S(a*) - OWN_SKIP_BELOW
//            has S(a) - m < -30 + (the rounding of a dozen additions), far below the -28.5 under which pclean_fixw is 0: its u_a
//            is the 0 it would have computed and its arms are never touched.  PCLEAN_NO_OWN_SKIP and a probe that asks for the
//            head's scores weigh every a.
//   arms     the surviving a dealt to the wavefronts, lanes over b: M, V by wave reductions, S[a] += L_j(a) in arm order
//   head     m, u_a, one sum per 64 values, their prefix; one row per lane draws a (own_leaf_kernel's search) and stores it
//   draws    one (row, particle) per wavefront at a time: M_j(a), the chunk sums of v_j(a, .) (lane c keeps chunk c: K_j <= 4096)
//            and V_j(a) again — kept while the next row drew the same a — then the chunk by ballot and the option by ballot
// MARG: instead of the draws the top values of the head (u_a / U), or for an arm the top b at the head's first value a*
// (v_j(a*, b) / V_j(a*): P(b | a*, obs), neither a per-column marginal nor the joint).
struct OwnStarDev {
  int32_t n_arms, ka, total, use_skip;
  int32_t target;                          // -1: the sweep (every node); probe / marginals: 0 the head, 1 + j arm j
  int32_t kj[OWN_STAR_MAX_ARMS];
  const double* alogp[OWN_STAR_MAX_ARMS];  // log theta_j, [ka * kj]
  const double* cmax[OWN_STAR_MAX_ARMS];   // [ka]
  int32_t tbeg[1 + OWN_STAR_MAX_ARMS], tend[1 + OWN_STAR_MAX_ARMS];  // the terms of node n in nd.terms (head first, arms in order)
  int32_t off[PCLEAN_MAX_TERMS];           // cached values of term ti: tv[off[ti] + option of its node's factor]
  uint32_t site[1 + OWN_STAR_MAX_ARMS];
  int32_t* vals[1 + OWN_STAR_MAX_ARMS];    // sweep: the nodes' current values, indexed by row
  int32_t* abuf;                           // probe: the head's draw of every (item, particle)
  unsigned long long* ctr;                 // {index values weighed, skipped} over the call's workgroups
};

__global__ __launch_bounds__(256) void own_star_cmax_kernel(int ka, int kj, const double* __restrict__ logt, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int a = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (a >= ka) return;  // (a whole wavefront)
  double m = -__builtin_inf();
  for (int b = lane; b < kj; b += 64) m = fmax(m, logt[(size_t)a * kj + b]);
  m = own_wave_max(m);
  if (lane == 0) out[a] = m + log((double)kj);
}

// joint histogram of (head value, arm value) over the loaded rows; a row unset in either node is skipped
__global__ __launch_bounds__(256) void own_star_counts_kernel(int n_rows, int ka, int kj, const int32_t* __restrict__ va,
                                                              const int32_t* __restrict__ vb, unsigned long long* __restrict__ hist) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)n_rows; i += stride) {
    const int a = va[i], b = vb[i];
    if (a < 0 || a >= ka || b < 0 || b >= kj) continue;
    atomicAdd(&hist[(size_t)a * kj + b], 1ull);
  }
}

// t_j(a, b): own_score's sum on arm j — the ONE place where it is written
__device__ __forceinline__ double own_star_arm_score(const OwnStarDev& sd, const double* tv, unsigned int skip, int j, int a, int b) {
  double t = sd.alogp[j][(size_t)a * sd.kj[j] + b];
  for (int ti = sd.tbeg[1 + j]; ti < sd.tend[1 + j]; ++ti)
    if (!((skip >> ti) & 1u)) t += tv[sd.off[ti] + b];
  return t;
}

struct OwnStarArm {
  double M, t0;              // the maximum; this lane's score of chunk 0
  unsigned long long pre, V;  // lane c: inclusive prefix of the chunk sums; their total
};

// M_j(a), the chunk sums and V_j(a) on one wavefront (every lane takes part; j and a are the same for all of them)
__device__ __forceinline__ void own_star_arm_eval(const OwnStarDev& sd, const double* tv, unsigned int skip, int j, int a, int lane,
                                                  OwnStarArm& r) {
  const int K = sd.kj[j], steps = (K + 63) >> 6;
  r.t0 = lane < K ? own_star_arm_score(sd, tv, skip, j, a, lane) : -__builtin_inf();
  double m = r.t0;
  for (int c = 1; c < steps; ++c) {
    const int k = (c << 6) + lane;
    if (k < K) m = fmax(m, own_star_arm_score(sd, tv, skip, j, a, k));
  }
  m = own_wave_max(m);
  r.M = m;
  const bool dead = m == -__builtin_inf();
  unsigned long long pre = 0ull;
  for (int c = 0; c < steps; ++c) {
    const int k = (c << 6) + lane;
    unsigned long long v = (k < K && !dead) ? pclean_fixw((c == 0 ? r.t0 : own_star_arm_score(sd, tv, skip, j, a, k)) - m) : 0ull;
    v = own_wave_sum(v);
    if (lane == c) pre = v;
  }
  pre = own_wave_scan(pre, lane);
  r.pre = pre;
  r.V = __shfl(pre, 63, 64);
}

// min{b : v_j(a, 0) + .. + v_j(a, b) > x} from the arm as own_star_arm_eval left it (V != 0, x < V)
__device__ __forceinline__ int own_star_arm_pick(const OwnStarDev& sd, const double* tv, unsigned int skip, int j, int a, int lane,
                                                 const OwnStarArm& r, unsigned long long x) {
  const int K = sd.kj[j], steps = (K + 63) >> 6;
  const unsigned long long cm = __ballot(lane < steps && r.pre > x);
  const int chunk = cm ? __builtin_ctzll(cm) : steps - 1;
  unsigned long long acc0 = __shfl(r.pre, chunk ? chunk - 1 : 0, 64);
  if (!chunk) acc0 = 0ull;
  const int k = (chunk << 6) + lane;
  unsigned long long v = k < K ? pclean_fixw((chunk == 0 ? r.t0 : own_star_arm_score(sd, tv, skip, j, a, k)) - r.M) : 0ull;
  v = own_wave_scan(v, lane);
  const unsigned long long hit = __ballot(k < K && acc0 + v > x);
  return hit ? (chunk << 6) + __builtin_ctzll(hit) : min(K, (chunk + 1) << 6) - 1;
}

template <bool MARG>
__global__ __launch_bounds__(OWN_BT) void own_star_kernel(const OwnNodeDev nd, const DensDev dn, const OwnStarDev sd, const OwnLaunch L,
                                                          const OwnMarginal M) {
  extern __shared__ __attribute__((aligned(16))) unsigned char own_smem[];
  constexpr int NW = OWN_BT / 64;
  __shared__ double s_red[NW];
  __shared__ double s_thr;
  __shared__ int s_obs[PCLEAN_MAX_TERMS];
  // one small array used twice (the static LDS has to stay within the 512 bytes that OWN_PRODUCT_LDS_MAX leaves): the arms'
  // largest term sums and the argmax of the bound before the head's pass, the marginals' top values after it
  __shared__ unsigned long long s_misc[OWN_STAR_MAX_ARMS * NW + NW / 2];
  static_assert(OWN_STAR_MAX_ARMS * NW + NW / 2 >= OWN_MAX_TOP + OWN_MAX_TOP / 2 + 2, "s_misc holds the marginals' top values");
  double(*s_tau)[NW] = reinterpret_cast<double(*)[NW]>(s_misc);                 // [OWN_STAR_MAX_ARMS][NW]
  int* s_redk = reinterpret_cast<int*>(s_misc + OWN_STAR_MAX_ARMS * NW);        // [NW]
  unsigned long long* s_topu = s_misc;                                          // [OWN_MAX_TOP]
  int* s_topk = reinterpret_cast<int*>(s_misc + OWN_MAX_TOP);                   // [OWN_MAX_TOP]
  double& s_am = *reinterpret_cast<double*>(s_misc + OWN_MAX_TOP + OWN_MAX_TOP / 2);
  unsigned long long& s_av = s_misc[OWN_MAX_TOP + OWN_MAX_TOP / 2 + 1];
  const int ka = sd.ka, nchA = (ka + 63) >> 6;
  double* tv = reinterpret_cast<double*>(own_smem);                             // [sd.total]
  double* S = tv + sd.total;                                                    // [ka]
  unsigned long long* pre = reinterpret_cast<unsigned long long*>(S + ka);      // [nchA]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int32_t* piece_off = MARG ? M.piece_off : L.piece_off;
  const int32_t* members = MARG ? M.members : L.members;
  const int win_lo = MARG ? M.win_lo : L.win_lo, win_hi = MARG ? M.win_hi : L.win_hi;
  const bool probe = !MARG && L.probe;
  const int m_lo = piece_off[blockIdx.x], m_hi = piece_off[blockIdx.x + 1];
  if (!probe) {  // a run none of whose rows lies in the window has nothing to do
    int any = 0;
    for (int q = m_lo + tid; q < m_hi; q += OWN_BT) {
      const int r = members[q];
      any |= (r >= win_lo && r < win_hi) ? 1 : 0;
    }
    if (!__syncthreads_or(any)) return;
  }
  {
    const int row0 = probe ? L.item_row[members[m_lo]] : members[m_lo];
    for (int ti = 0; ti < nd.n_terms; ++ti)
      if (tid == ti) s_obs[ti] = nd.terms[ti].obs_col[row0];
  }
  __syncthreads();

  // ---- phase 1: the terms, once per value of the factor they read
  unsigned int skip = 0;
  for (int n = 0; n <= sd.n_arms; ++n) {
    const int nf = n == 0 ? ka : sd.kj[n - 1];
    for (int ti = sd.tbeg[n]; ti < sd.tend[n]; ++ti) {
      const TermDev& tm = nd.terms[ti];
      const int o = s_obs[ti];
      if (tm.dens_kind != PCLEAN_DENS_TABULATED && o < 0) {  // a missing observation: the term adds nothing
        skip |= 1u << ti;
        continue;
      }
      double* dst = tv + sd.off[ti];
      for (int j = tid; j < nf; j += OWN_BT) {  // (the head's column, or the first K_j entries of the arm's column 1: b's value)
        const int val = tm.cand_col[j];
        dst[j] = (unsigned)val < (unsigned)tm.n_lat ? own_term_value(tm, dn, o, val) : -__builtin_inf();
      }
    }
  }
  __syncthreads();
  if (probe && L.scores_out && sd.target > 0) {  // an arm's probe: t_j(a, b) of the whole grid
    const int j = sd.target - 1, K = sd.kj[j], n = ka * K;
    for (int k = tid; k < n; k += OWN_BT) {
      const int a = k / K;
      const double t = own_star_arm_score(sd, tv, skip, j, a, k - a * K);
      for (int mi = m_lo; mi < m_hi; ++mi) L.scores_out[(size_t)members[mi] * n + k] = t;
    }
  }

  // ---- phase 2: the head's own part of S, and the largest cached term sum of every arm
  for (int a = tid; a < ka; a += OWN_BT) {
    double h = nd.logp[a];
    for (int ti = sd.tbeg[0]; ti < sd.tend[0]; ++ti)
      if (!((skip >> ti) & 1u)) h += tv[sd.off[ti] + a];
    S[a] = h;
  }
  for (int j = 0; j < sd.n_arms; ++j) {
    double tm = -__builtin_inf();
    for (int b = tid; b < sd.kj[j]; b += OWN_BT) {
      double t = 0.0;
      for (int ti = sd.tbeg[1 + j]; ti < sd.tend[1 + j]; ++ti)
        if (!((skip >> ti) & 1u)) t += tv[sd.off[ti] + b];
      tm = fmax(tm, t);
    }
    tm = own_wave_max(tm);
    if (lane == 0) s_tau[j][wave] = tm;
  }
  __syncthreads();
  double add_tau[OWN_STAR_MAX_ARMS];
#pragma unroll
  for (int j = 0; j < OWN_STAR_MAX_ARMS; ++j) {
    double t = -__builtin_inf();
    if (j < sd.n_arms)
      for (int w = 0; w < NW; ++w) t = fmax(t, s_tau[j][w]);
    add_tau[j] = t;
  }
  auto bound = [&](int a) -> double {  // B(a) >= S(a)
    double b = S[a];
#pragma unroll
    for (int j = 0; j < OWN_STAR_MAX_ARMS; ++j)
      if (j < sd.n_arms) b += add_tau[j] + sd.cmax[j][a];
    return b;
  };
  auto exact = [&](int a) -> double {  // S(a), on one wavefront: the arms in arm order
    double acc = S[a];
    for (int j = 0; j < sd.n_arms; ++j) {
      OwnStarArm r;
      own_star_arm_eval(sd, tv, skip, j, a, lane, r);
      acc += pclean_lse_from_fix(r.M, r.V);
    }
    return acc;
  };

  // ---- the exact skip: S at argmax B
  const bool skipping = sd.use_skip && !(probe && L.scores_out && sd.target == 0);
  double thr = -__builtin_inf();
  if (skipping) {
    double bb = -__builtin_inf();
    int bk = 0x7fffffff;
    for (int a = tid; a < ka; a += OWN_BT) {
      const double b = bound(a);
      if (b > bb || (b == bb && a < bk)) {
        bb = b;
        bk = a;
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double bo = __shfl_xor(bb, o, 64);
      const int ko = __shfl_xor(bk, o, 64);
      if (bo > bb || (bo == bb && ko < bk)) {
        bb = bo;
        bk = ko;
      }
    }
    if (lane == 0) {
      s_red[wave] = bb;
      s_redk[wave] = bk;
    }
    __syncthreads();
    if (wave == 0) {  // (uniform per wavefront)
      bb = s_red[0];
      bk = s_redk[0];
      for (int w = 1; w < NW; ++w)
        if (s_red[w] > bb || (s_red[w] == bb && s_redk[w] < bk)) {
          bb = s_red[w];
          bk = s_redk[w];
        }
      if (bk >= ka) bk = 0;  // (every bound NaN: nothing is skipped below, whatever a)
      const double sx = exact(bk);
      if (lane == 0) s_thr = sx - OWN_SKIP_BELOW;
    }
    __syncthreads();
    thr = s_thr;
  }

  // ---- the arms of every surviving a
  {
    unsigned long long n_w = 0ull, n_s = 0ull;
    for (int a = wave; a < ka; a += NW) {
      if (skipping && bound(a) < thr) {  // (the same for every lane of the wavefront)
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) S[a] = -__builtin_inf();
        ++n_s;
        continue;
      }
      const double sx = exact(a);
      if (lane == 0) S[a] = sx;
      ++n_w;
    }
    if (lane == 0 && sd.ctr) {
      atomicAdd(&sd.ctr[0], n_w);
      atomicAdd(&sd.ctr[1], n_s);
    }
  }
  __syncthreads();
  if (probe && L.scores_out && sd.target == 0)
    for (int a = tid; a < ka; a += OWN_BT) {
      const double sa = S[a];
      for (int mi = m_lo; mi < m_hi; ++mi) L.scores_out[(size_t)members[mi] * ka + a] = sa;
    }

  // ---- the head: m, u_a, one sum per 64 values, their inclusive prefix
  double lmax = -__builtin_inf();
  for (int a = tid; a < ka; a += OWN_BT) lmax = fmax(lmax, S[a]);
  lmax = own_wave_max(lmax);
  if (lane == 0) s_red[wave] = lmax;
  __syncthreads();
  double m = s_red[0];
  for (int w = 1; w < NW; ++w) m = fmax(m, s_red[w]);
  const bool dead = m == -__builtin_inf();
  auto weight = [&](int a) -> unsigned long long { return dead ? 0ull : pclean_fixw(S[a] - m); };
  for (int c = wave; c < nchA; c += NW) {
    const int a = (c << 6) + lane;
    const unsigned long long v = own_wave_sum(a < ka ? weight(a) : 0ull);
    if (lane == 0) pre[c] = v;
  }
  __syncthreads();
  if (wave == 0) {  // (nchA <= 64)
    const unsigned long long v = own_wave_scan(lane < nchA ? pre[lane] : 0ull, lane);
    if (lane < nchA) pre[lane] = v;
  }
  __syncthreads();
  const unsigned long long U = pre[nchA - 1];
  const double lse = pclean_lse_from_fix(m, U);

  if (!MARG) {
    // ---- stage A: one (row, particle) per lane draws a
    const int nd_eff = probe ? max(L.n_draws, 1) : 1;
    const int n_out = (m_hi - m_lo) * nd_eff;
    for (int q = tid; q < n_out; q += OWN_BT) {
      const int mem = members[m_lo + q / nd_eff], j = q % nd_eff;
      int row, pid;
      if (probe) {
        row = L.item_row[mem];
        pid = j;
        if (j == 0 && L.lse_out && sd.target == 0) L.lse_out[mem] = lse;
      } else {
        row = mem;
        if (row < win_lo || row >= win_hi) continue;
        const int i = row - win_lo;
        L.logml[i] += lse;  // (once: the arms add nothing)
        if (L.keep[i]) continue;
        pid = L.chosen[i];
      }
      int res = ka - 1;
      if (U != 0ull) {
        const uint32_t rng_row = (uint32_t)((int64_t)row + L.row_offset);
        const unsigned long long x = pclean_mulhi64(pclean_rand64(L.seed, rng_row, sd.site[0], (uint32_t)pid, L.sweep), U);
        int a = 0, b = nchA - 1;
        while (a < b) {  // the first chunk whose inclusive prefix exceeds x
          const int mid = (a + b) >> 1;
          if (pre[mid] > x)
            b = mid;
          else
            a = mid + 1;
        }
        unsigned long long acc = a ? pre[a - 1] : 0ull;
        int k = a << 6;
        const int k_end = min(ka, k + 64) - 1;  // (the chunk's total exceeds x - acc: the walk stops inside it)
        for (; k < k_end; ++k) {
          acc += weight(k);
          if (acc > x) break;
        }
        res = k;
      }
      if (!probe)
        sd.vals[0][row] = res;
      else if (sd.target == 0) {
        if (L.n_draws > 0) L.draws_out[(size_t)mem * L.n_draws + j] = res;
      } else
        sd.abuf[(size_t)mem * nd_eff + j] = res;
    }
    if (probe && sd.target == 0) return;  // (uniform)
    __syncthreads();  // (the head's draws, written by other wavefronts of this workgroup, are read below)

    // ---- stage B: one (row, particle) per wavefront at a time draws the arms at its a
    const int j_lo = probe ? sd.target - 1 : 0, j_hi = probe ? sd.target : sd.n_arms;
    OwnStarArm arm[OWN_STAR_MAX_ARMS];
    int arm_a[OWN_STAR_MAX_ARMS];
#pragma unroll
    for (int j = 0; j < OWN_STAR_MAX_ARMS; ++j) arm_a[j] = -1;
    for (int q = wave; q < n_out; q += NW) {  // (everything below is the same for every lane of the wavefront)
      const int mem = members[m_lo + q / nd_eff], dj = q % nd_eff;
      int row, pid, a;
      if (probe) {
        row = L.item_row[mem];
        pid = dj;
        a = sd.abuf[(size_t)mem * nd_eff + dj];
      } else {
        row = mem;
        if (row < win_lo || row >= win_hi) continue;
        const int i = row - win_lo;
        if (L.keep[i]) continue;
        pid = L.chosen[i];
        a = sd.vals[0][row];
      }
      if (a < 0 || a >= ka) continue;  // (never: stage A wrote it)
      const uint32_t rng_row = (uint32_t)((int64_t)row + L.row_offset);
#pragma unroll
      for (int j = 0; j < OWN_STAR_MAX_ARMS; ++j) {
        if (j < j_lo || j >= j_hi) continue;
        if (arm_a[j] != a) {
          own_star_arm_eval(sd, tv, skip, j, a, lane, arm[j]);
          arm_a[j] = a;
        }
        int res = sd.kj[j] - 1;
        if (U != 0ull && arm[j].V != 0ull) {
          const unsigned long long x =
              pclean_mulhi64(pclean_rand64(L.seed, rng_row, sd.site[1 + j], (uint32_t)pid, L.sweep), arm[j].V);
          res = own_star_arm_pick(sd, tv, skip, j, a, lane, arm[j], x);
        }
        if (lane == 0) {
          if (!probe)
            sd.vals[1 + j][row] = res;
          else {
            if (L.n_draws > 0) L.draws_out[(size_t)mem * L.n_draws + dj] = res;
            if (dj == 0 && L.lse_out) L.lse_out[mem] = pclean_lse_from_fix(arm[j].M, arm[j].V);
          }
        }
      }
    }
  } else {
    // ---- marginals: the head's top values (every lane of wavefront 0 scans its share of a, `top` rounds)
    const double Ud = (double)U;
    if (wave == 0) {
      unsigned long long last_u = 0ull;
      int last_k = -1;
      bool open = true;
      for (int t = 0; t < M.top; ++t) {
        unsigned long long bu = 0ull;
        int bk = -1;
        for (int a = lane; a < ka && open; a += 64) {
          const unsigned long long u = weight(a);
          if (u != 0ull && (last_k < 0 || own_before(last_u, last_k, u, a)) && own_before(u, a, bu, bk)) {
            bu = u;
            bk = a;
          }
        }
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long uo = __shfl_xor(bu, o, 64);
          const int ko = __shfl_xor(bk, o, 64);
          if (own_before(uo, ko, bu, bk)) {
            bu = uo;
            bk = ko;
          }
        }
        if (bu != 0ull) {
          last_u = bu;
          last_k = bk;
        } else {
          open = false;
          bk = -1;
        }
        if (lane == 0) {
          s_topk[t] = bk;
          s_topu[t] = bu;
        }
      }
    }
    __syncthreads();
    const int a_star = s_topk[0];
    const int j = sd.target - 1;
    if (sd.target > 0) {  // an arm: the top b at a*
      __syncthreads();
      if (wave == 0) {
        OwnStarArm r;
        r.M = -__builtin_inf();
        r.V = 0ull;
        if (a_star >= 0) own_star_arm_eval(sd, tv, skip, j, a_star, lane, r);
        unsigned long long last_u = 0ull;
        int last_k = -1;
        bool open = a_star >= 0 && r.V != 0ull;
        for (int t = 0; t < M.top; ++t) {
          unsigned long long bu = 0ull;
          int bk = -1;
          for (int b = lane; b < sd.kj[j] && open; b += 64) {
            const unsigned long long u = pclean_fixw(own_star_arm_score(sd, tv, skip, j, a_star, b) - r.M);
            if (u != 0ull && (last_k < 0 || own_before(last_u, last_k, u, b)) && own_before(u, b, bu, bk)) {
              bu = u;
              bk = b;
            }
          }
          for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long uo = __shfl_xor(bu, o, 64);
            const int ko = __shfl_xor(bk, o, 64);
            if (own_before(uo, ko, bu, bk)) {
              bu = uo;
              bk = ko;
            }
          }
          if (bu != 0ull) {
            last_u = bu;
            last_k = bk;
          } else {
            open = false;
            bk = -1;
          }
          if (lane == 0) {
            s_topk[t] = bk;
            s_topu[t] = bu;
          }
        }
        if (lane == 0) {
          s_am = r.M;
          s_av = r.V;
        }
      }
      __syncthreads();
    }
    const double den = sd.target > 0 ? (double)s_av : Ud;
    const size_t nw = (size_t)(win_hi - win_lo);
    for (int q = m_lo + tid; q < m_hi; q += OWN_BT) {
      const int row = members[q];
      if (row < win_lo || row >= win_hi) continue;
      const size_t i = (size_t)(row - win_lo);
      for (int t = 0; t < M.top; ++t) {
        const bool has = s_topk[t] >= 0;
        M.top_option[(size_t)t * nw + i] = has ? s_topk[t] : -1;
        M.top_prob[(size_t)t * nw + i] = has ? (double)s_topu[t] / den : 0.0;
      }
      if (M.cur_prob) {
        const int cur = M.vals[row];
        double p = 0.0;
        if (sd.target == 0) {
          if (U != 0ull && cur >= 0 && cur < ka) p = (double)weight(cur) / Ud;
        } else if (a_star >= 0 && s_av != 0ull && cur >= 0 && cur < sd.kj[j]) {
          p = (double)pclean_fixw(own_star_arm_score(sd, tv, skip, j, a_star, cur) - s_am) / den;
        }
        M.cur_prob[i] = p;
      }
      if (U == 0ull) {
        atomicAdd(&M.bad[0], 1);
        atomicMin(&M.bad[1], row);
      }
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

// What pclean_add_own_gauss checks of a term against the node's option table and the numeric columns as they are now (the
// launches check again: either may have been set anew since)
int check_own_gauss(pclean_ctx* ctx, const OwnLeaf& lf, const pclean_gauss& g, int status, const char* who) {
  if (g.n_locals < 1 || g.n_locals > 2 || g.n_dims < 0 || g.n_dims > 4 || g.fixed_locals != 0)
    return pclean_fail(ctx, status, "%s: n_locals (the option table's value columns) must be 1 or 2, n_dims 0 .. 4, fixed_locals 0", who);
  int64_t K = 1, top = 0;
  for (int c = 0; c < g.n_locals; ++c) {
    if (g.local_n[c] < 1 || g.local_n[c] > OWN_GAUSS_MAX_OPTIONS) return pclean_fail(ctx, status, "%s: local_n[%d] = %d", who, c, g.local_n[c]);
    K *= g.local_n[c];
  }
  if (K > OWN_GAUSS_MAX_OPTIONS)
    return pclean_fail(ctx, status, "%s: a grid of %lld options (at most %d are served)", who, (long long)K, OWN_GAUSS_MAX_OPTIONS);
  for (int d = 0; d < g.n_dims; ++d) {
    if (g.src_kind[d] != PCLEAN_GSRC_LOCAL)
      return pclean_fail(ctx, status, "%s: index source %d is of kind %d; an own leaf's term reads option columns alone "
                                      "(PCLEAN_GSRC_LOCAL), no candidate, observed, ctx or evidence value", who, d, g.src_kind[d]);
    if (g.src[d] < 0 || g.src[d] >= g.n_locals || g.stride[d] < 0) return pclean_fail(ctx, status, "%s: index source %d: bad column or stride", who, d);
    top += (int64_t)g.stride[d] * (g.local_n[g.src[d]] - 1);
  }
  if (top > 0x7fffffff) return pclean_fail(ctx, status, "%s: mean index out of range", who);
  if (g.transform_src_kind != -1) {
    if (g.transform_src_kind != PCLEAN_GSRC_LOCAL)
      return pclean_fail(ctx, status, "%s: transformation source of kind %d; an option column (PCLEAN_GSRC_LOCAL) or none (-1)", who,
                         g.transform_src_kind);
    if (g.transform_src < 0 || g.transform_src >= g.n_locals || g.local_n[g.transform_src] > 4)
      return pclean_fail(ctx, status, "%s: the transformation column must be an option column with at most 4 values", who);
  }
  if (!(g.sigma > 0.0) || g.mean_table < 0 || g.mean_table >= PCLEAN_MAX_TABLES) return pclean_fail(ctx, status, "%s: bad sigma or mean table", who);
  const CandTable& t = ctx->cand[lf.node.table];
  if (!t.valid || !t.is_options) return pclean_fail(ctx, status, "%s: the node's option table is not set", who);
  if (t.n_cols != g.n_locals || (int64_t)t.n_rows != K)
    return pclean_fail(ctx, status, "%s: the option table holds %d options in %d columns, the term names %lld in %d", who, t.n_rows, t.n_cols,
                       (long long)K, g.n_locals);
  if (!ctx->xnum.p || ctx->n_xcols <= 0 || g.x_col < 0 || g.x_col >= ctx->n_xcols)
    return pclean_fail(ctx, status, "%s: numeric column %d is not loaded (pclean_load_numeric_columns)", who, g.x_col);
  for (int u = 0; u < 4; ++u)
    if (g.t_x_col[u] >= 0 || g.t_lad_col[u] >= 0)
      if (g.t_x_col[u] < 0 || g.t_x_col[u] >= ctx->n_xcols || g.t_lad_col[u] < 0 || g.t_lad_col[u] >= ctx->n_xcols)
        return pclean_fail(ctx, status, "%s: transformation column out of range", who);
  return PCLEAN_OK;
}

// The device view of a Gaussian leaf: its terms resolved (build_gauss_dev, rows addressed by loaded row), the option columns,
// the lanes per row and the layout of the cached string-term values
int own_gauss_plan(pclean_ctx* ctx, const OwnLeaf& lf, const OwnNodeDev& od, OwnGaussDev& gd, size_t* lds) {
  memset(&gd, 0, sizeof gd);
  const CandTable& t = ctx->cand[lf.node.table];
  if (od.n_cand > OWN_GAUSS_MAX_OPTIONS)
    return pclean_fail(ctx, PCLEAN_ERR_CAPACITY, "own block: a Gaussian leaf of %d options (at most %d)", od.n_cand, OWN_GAUSS_MAX_OPTIONS);
  gd.n_gauss = (int)lf.gauss.size();
  for (int gi = 0; gi < gd.n_gauss; ++gi) {
    pclean_gauss g = lf.gauss[gi];
    int rc = check_own_gauss(ctx, lf, g, PCLEAN_ERR_STATE, "own block (Gaussian term)");
    if (rc) return rc;
    g.local_obs_col[0] = g.local_obs_col[1] = -1;  // (not read: the choices' observations are the leaf's string terms)
    rc = build_gauss_dev(ctx, g, nullptr, gd.g[gi]);
    if (rc) return rc;
    GaussDev& d = gd.g[gi];
    d.x -= ctx->active_begin;  // (the own kernels address rows by loaded row)
    for (int u = 0; u < 4; ++u)
      if (d.tx[u]) {
        d.tx[u] -= ctx->active_begin;
        d.tl[u] -= ctx->active_begin;
      }
    int64_t top = 0;
    for (int dd = 0; dd < g.n_dims; ++dd) top += (int64_t)g.stride[dd] * (g.local_n[g.src[dd]] - 1);
    if (top >= ctx->mean[g.mean_table].n)
      return pclean_fail(ctx, PCLEAN_ERR_ARG, "own block: mean table %d holds %d values, the term's largest index is %lld", g.mean_table,
                         ctx->mean[g.mean_table].n, (long long)top);
    gd.n_cols = g.n_locals;
    gd.local_n[0] = g.local_n[0];
    gd.local_n[1] = g.n_locals > 1 ? g.local_n[1] : 1;
  }
  gd.col[0] = t.cols.p;
  gd.col[1] = gd.n_cols > 1 ? t.cols.p + (size_t)t.n_rows : nullptr;
  gd.lw = 0;
  while (gd.lw < 6 && (1 << gd.lw) < od.n_cand) ++gd.lw;
  size_t total = 0;
  for (int ti = 0; ti < od.n_terms; ++ti) {
    gd.off[ti] = (int32_t)total;
    total += (size_t)std::max(od.terms[ti].n_lat, 0);
  }
  gd.cached = total * 8 <= OWN_GAUSS_LDS_MAX ? 1 : 0;
  *lds = gd.cached ? total * 8 : 0;
  return PCLEAN_OK;
}

int launch_leaf(pclean_ctx* ctx, const OwnLeaf& lf, const OwnNodeDev& od, const OwnLaunch& L, int n_pieces, OwnState* s) {
  if (n_pieces <= 0) return PCLEAN_OK;
  const DensDev dn{ctx->nb.p, ctx->logl.p, ctx->max_d + 1, 0, ctx->prob_same.p, ctx->prob_diff.p, ctx->logn.p};
  if (!lf.gauss.empty()) {
    OwnGaussDev gd;
    size_t glds = 0;
    const int rc = own_gauss_plan(ctx, lf, od, gd, &glds);
    if (rc) return rc;
    hipLaunchKernelGGL(own_gauss_kernel<false>, dim3(n_pieces), dim3(OWN_BT), glds, ctx->stream, od, dn, gd, L, OwnMarginal{});
    HIPCHK(ctx, hipGetLastError());
    s->stats.variants |= 8;
    s->stats.n_workgroups += n_pieces;
    return PCLEAN_OK;
  }
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

// ---- star ---------------------------------------------------------------------------------------------------------------------
void release_stars(OwnBlock& b) {
  for (OwnStar& st : b.stars) {
    st.grp.piece_off.release();
    st.grp.piece_rows.release();
    st.cmax.release();
  }
  b.stars.clear();
  b.star_of.clear();
}

// The grid rule of a star on the tables as they are now (own_star_check.h): the head's values, every arm a key-major grid over
// them, and every value a term reads inside the term's latent domain.  Fills kj and cols_version; `status` for a refusal.
int check_star_tables(pclean_ctx* ctx, const OwnBlock& b, int head, const std::vector<int>& arms, int status, const char* who,
                      std::vector<int32_t>* kj_out, std::vector<uint64_t>* ver_out) {
  const OwnLeaf& hl = b.leaves[head];
  const CandTable& ht = ctx->cand[hl.node.table];
  if (!ht.valid || !ht.is_options || ht.n_cols != 1 || (int)ht.h_vals.size() != ht.n_rows)
    return pclean_fail(ctx, status, "%s: the head's option table %d is not set as a one-column option table", who, hl.node.table);
  const int ka = ht.n_rows;
  if (ka > OWN_STAR_MAX_K) return pclean_fail(ctx, status, "%s: the head holds %d options (at most %d)", who, ka, OWN_STAR_MAX_K);
  auto values_ok = [&](const OwnLeaf& lf, int64_t n, const int32_t* vals, int col) -> int {
    for (const pclean_term& tm : lf.terms) {
      if (tm.cand_col != col) return pclean_fail(ctx, status, "%s: a term reads column %d, a star's terms read column %d", who, tm.cand_col, col);
      const PairTable& pt = ctx->pair[tm.pair_table];
      if (!pt.valid) return pclean_fail(ctx, PCLEAN_ERR_STATE, "%s: pair table %d not built", who, tm.pair_table);
      const int64_t bad = own_star_check_values(n, vals, pt.n_lat);
      if (bad) return pclean_fail(ctx, status, "%s: option %lld holds value %d outside pair table %d's %d latent values", who,
                                  (long long)(bad - 1), vals[bad - 1], tm.pair_table, pt.n_lat);
    }
    return PCLEAN_OK;
  };
  int rc = values_ok(hl, ka, ht.h_vals.data(), 0);
  if (rc) return rc;
  kj_out->clear();
  ver_out->assign(1, ht.cols_version);
  std::vector<int32_t> cols;
  for (int an : arms) {
    const OwnLeaf& al = b.leaves[an];
    const CandTable& at = ctx->cand[al.node.table];
    if (!at.valid || !at.is_options || at.n_cols != 2)
      return pclean_fail(ctx, status, "%s: the option table %d of arm node %d is not set with two value columns", who, al.node.table, an);
    cols.resize((size_t)2 * at.n_rows);
    HIPCHK(ctx, hipMemcpy(cols.data(), at.cols.p, cols.size() * 4, hipMemcpyDeviceToHost));
    char msg[200];
    int32_t kj = 0;
    if (own_star_check_grid(ka, ht.h_vals.data(), at.n_rows, cols.data(), cols.data() + at.n_rows, &kj, msg, sizeof msg))
      return pclean_fail(ctx, status, "%s: arm node %d: %s", who, an, msg);
    rc = values_ok(al, kj, cols.data() + at.n_rows, 1);
    if (rc) return rc;
    kj_out->push_back(kj);
    ver_out->push_back(at.cols_version);
  }
  return PCLEAN_OK;
}

// The device view of a star: the nodes' views (leaf_dev) with their terms in one list, the layout of the cached values, and
// room for the bound of every arm's prior rows (launch_star fills it).  target: see OwnStarDev.
int star_dev(pclean_ctx* ctx, OwnBlock& b, OwnStar& st, int block_id, int target, OwnNodeDev& od, OwnStarDev& sd, size_t* lds) {
  static const bool no_skip = getenv("PCLEAN_NO_OWN_SKIP") != nullptr;
  const int D = (int)st.arms.size();
  bool moved = (int)st.cols_version.size() != 1 + D;
  for (int n = 0; n <= D && !moved; ++n)
    moved = ctx->cand[b.leaves[n == 0 ? st.head : st.arms[n - 1]].node.table].cols_version != st.cols_version[n];
  if (moved) {  // an option table was set anew since the star was linked: its lengths and values are checked again
    const int rc = check_star_tables(ctx, b, st.head, st.arms, PCLEAN_ERR_STATE, "own block (star)", &st.kj, &st.cols_version);
    if (rc) {
      st.cols_version.clear();
      return rc;
    }
  }
  memset(&sd, 0, sizeof sd);
  int rc = leaf_dev(ctx, b.leaves[st.head], od);
  if (rc) return rc;
  sd.n_arms = D;
  sd.ka = od.n_cand;
  sd.target = target;
  sd.use_skip = no_skip ? 0 : 1;
  sd.tbeg[0] = 0;
  sd.tend[0] = od.n_terms;
  sd.site[0] = PCLEAN_SITE_NODE(block_id, st.head);
  int32_t tpn[1 + OWN_STAR_MAX_ARMS] = {od.n_terms, 0, 0, 0, 0};
  int total = 0;
  for (int ti = 0; ti < od.n_terms; ++ti, total += sd.ka) sd.off[ti] = total;
  if (st.cmax.alloc((size_t)D * sd.ka)) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  for (int j = 0; j < D; ++j) {
    OwnNodeDev ad;
    rc = leaf_dev(ctx, b.leaves[st.arms[j]], ad);
    if (rc) return rc;
    if (ad.n_cand != sd.ka * st.kj[j]) return pclean_fail(ctx, PCLEAN_ERR_STATE, "own block (star): arm %d holds %d options, not %d x %d", j, ad.n_cand, sd.ka, st.kj[j]);
    if (od.n_terms + ad.n_terms > PCLEAN_MAX_TERMS)
      return pclean_fail(ctx, PCLEAN_ERR_CAPACITY, "own block (star): more than %d terms over the star", PCLEAN_MAX_TERMS);
    sd.kj[j] = st.kj[j];
    sd.alogp[j] = ad.logp;
    sd.cmax[j] = st.cmax.p + (size_t)j * sd.ka;
    sd.tbeg[1 + j] = od.n_terms;
    for (int ti = 0; ti < ad.n_terms; ++ti, total += sd.kj[j]) {
      sd.off[od.n_terms] = total;
      od.terms[od.n_terms++] = ad.terms[ti];
    }
    sd.tend[1 + j] = od.n_terms;
    tpn[1 + j] = ad.n_terms;
    sd.site[1 + j] = PCLEAN_SITE_NODE(block_id, st.arms[j]);
  }
  sd.total = total;
  *lds = own_star_lds_bytes(sd.ka, D, sd.kj, tpn);
  if (*lds > OWN_PRODUCT_LDS_MAX)
    return pclean_fail(ctx, PCLEAN_ERR_CAPACITY, "own block (star): %zu bytes of cached values, more than the %zu of a workgroup's LDS", *lds,
                       (size_t)OWN_PRODUCT_LDS_MAX);
  return PCLEAN_OK;
}

struct StarPlan {
  OwnNodeDev od;
  OwnStarDev sd;
  size_t lds = 0;
};

int launch_star(pclean_ctx* ctx, OwnState* s, const OwnNodeDev& od, const OwnStarDev& sd, size_t lds, const OwnLaunch& L, const OwnMarginal* M,
                int n_pieces) {
  if (n_pieces <= 0) return PCLEAN_OK;
  if (!s->star_attr_set) {
    HIPCHK(ctx, hipFuncSetAttribute((const void*)own_star_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)OWN_PRODUCT_LDS_MAX));
    HIPCHK(ctx, hipFuncSetAttribute((const void*)own_star_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)OWN_PRODUCT_LDS_MAX));
    s->star_attr_set = true;
  }
  const DensDev dn{ctx->nb.p, ctx->logl.p, ctx->max_d + 1, 0, ctx->prob_same.p, ctx->prob_diff.p, ctx->logn.p};
  for (int j = 0; j < sd.n_arms; ++j) {  // the bound of every arm's prior rows, from the priors as they are at this call
    hipLaunchKernelGGL(own_star_cmax_kernel, dim3((sd.ka + 3) / 4), dim3(256), 0, ctx->stream, sd.ka, sd.kj[j], sd.alogp[j],
                       const_cast<double*>(sd.cmax[j]));
    HIPCHK(ctx, hipGetLastError());
  }
  if (M)
    hipLaunchKernelGGL(own_star_kernel<true>, dim3(n_pieces), dim3(OWN_BT), lds, ctx->stream, od, dn, sd, OwnLaunch{}, *M);
  else
    hipLaunchKernelGGL(own_star_kernel<false>, dim3(n_pieces), dim3(OWN_BT), lds, ctx->stream, od, dn, sd, L, OwnMarginal{});
  HIPCHK(ctx, hipGetLastError());
  s->stats.variants |= 16;
  s->stats.n_workgroups += n_pieces;
  return PCLEAN_OK;
}

// the constant, the counters of impossible rows and the events around a call's launches
int ensure_aux(pclean_ctx* ctx, OwnState* s) {
  if (s->zero.p) return PCLEAN_OK;
  if (s->zero.alloc(1) || s->bad.alloc(2) || s->star_ctr.alloc(2)) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
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
    release_stars(b);
    for (OwnLeaf& lf : b.leaves) {
      lf.piece_off.release();
      lf.piece_rows.release();
    }
  }
  s->zero.release();
  s->bad.release();
  s->hist.release();
  s->gstat.release();
  s->star_ctr.release();
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
  release_stars(b);  // (pclean_link_own_star comes after the load)
  b.star_of.assign(n_nodes, -1);
  for (int i = 0; i < n_nodes; ++i) {
    b.leaves[i].node = nodes[i];
    b.leaves[i].terms.assign(terms + nodes[i].term_begin, terms + nodes[i].term_begin + nodes[i].n_terms);
  }
  b.vals.release();
  b.vals_rows = -1;
  b.valid = true;
  return PCLEAN_OK;
}

extern "C" int pclean_link_own_star(pclean_ctx* ctx, int32_t block_id, int32_t head_node, int32_t n_arms, const int32_t* arm_nodes) {
  OwnBlock* b = find_block(ctx, block_id);
  if (!b) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_link_own_star: block %d is not a loaded own block", block_id);
  const int nn = (int)b->leaves.size();
  if (n_arms < 2 || n_arms > OWN_STAR_MAX_ARMS || !arm_nodes)
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_link_own_star: %d arms (2 .. %d are served; one dependent is a product leaf)", n_arms,
                       OWN_STAR_MAX_ARMS);
  if (head_node < 0 || head_node >= nn || b->star_of[head_node] >= 0 || !b->leaves[head_node].gauss.empty())
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_link_own_star: head node %d is no free node of block %d without Gaussian terms", head_node,
                       block_id);
  std::vector<int> arms(arm_nodes, arm_nodes + n_arms);
  size_t n_terms = b->leaves[head_node].terms.size();
  for (int j = 0; j < n_arms; ++j) {
    const int an = arms[j];
    if (an != head_node + 1 + j || an >= nn || b->star_of[an] >= 0 || !b->leaves[an].gauss.empty())
      return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_link_own_star: arm %d is node %d; the arms are the free nodes that follow the head "
                                              "(%d), in order, without Gaussian terms", j, an, head_node);
    n_terms += b->leaves[an].terms.size();
  }
  if (n_terms > PCLEAN_MAX_TERMS)
    return pclean_fail(ctx, PCLEAN_ERR_CAPACITY, "pclean_link_own_star: %zu terms over the star (at most %d)", n_terms, PCLEAN_MAX_TERMS);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  OwnStar st;
  st.head = head_node;
  st.arms = arms;
  int rc = check_star_tables(ctx, *b, head_node, arms, PCLEAN_ERR_ARG, "pclean_link_own_star", &st.kj, &st.cols_version);
  if (rc) return rc;  // (nothing modified)
  {
    int32_t tpn[1 + OWN_STAR_MAX_ARMS] = {0, 0, 0, 0, 0};
    tpn[0] = (int32_t)b->leaves[head_node].terms.size();
    for (int j = 0; j < n_arms; ++j) tpn[1 + j] = (int32_t)b->leaves[arms[j]].terms.size();
    const size_t lds = own_star_lds_bytes(ctx->cand[b->leaves[head_node].node.table].n_rows, n_arms, st.kj.data(), tpn);
    if (lds > OWN_PRODUCT_LDS_MAX)
      return pclean_fail(ctx, PCLEAN_ERR_CAPACITY, "pclean_link_own_star: %zu bytes of cached values, more than the %zu of a workgroup's LDS", lds,
                         (size_t)OWN_PRODUCT_LDS_MAX);
  }
  st.grp.terms = b->leaves[head_node].terms;
  for (int an : arms) st.grp.terms.insert(st.grp.terms.end(), b->leaves[an].terms.begin(), b->leaves[an].terms.end());
  const int si = (int)b->stars.size();
  b->stars.push_back(st);
  b->star_of[head_node] = si;
  for (int an : arms) b->star_of[an] = si;
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
  std::vector<StarPlan> stars;  // (in block order, a block's in link order)
  for (int bi = 0; bi < PCLEAN_MAX_BLOCKS; ++bi) {
    OwnBlock& b = s->block[bi];
    if (!b.valid) continue;
    int rc = ensure_vals(ctx, b);
    if (rc) return rc;
    for (OwnLeaf& lf : b.leaves) {
      ods.emplace_back();
      rc = leaf_dev(ctx, lf, ods.back());
      if (!rc) rc = ensure_groups(ctx, lf);
      if (!rc && !lf.gauss.empty()) {  // (a missing mean table, an option table set anew in another shape)
        OwnGaussDev gd;
        size_t glds = 0;
        rc = own_gauss_plan(ctx, lf, ods.back(), gd, &glds);
      }
      if (rc) return rc;
    }
    for (OwnStar& st : b.stars) {
      stars.emplace_back();
      StarPlan& sp = stars.back();
      rc = ensure_groups(ctx, st.grp);
      if (!rc) rc = star_dev(ctx, b, st, bi, -1, sp.od, sp.sd, &sp.lds);
      if (rc) return rc;
      for (int n = 0; n <= sp.sd.n_arms; ++n) sp.sd.vals[n] = b.vals.p + (size_t)(n == 0 ? st.head : st.arms[n - 1]) * ctx->n_rows;
    }
  }
  {
    const int rc = ensure_aux(ctx, s);
    if (rc) return rc;
  }
  if (!stars.empty()) HIPCHK(ctx, hipMemsetAsync(s->star_ctr.p, 0, 16, ctx->stream));
  for (StarPlan& sp : stars) sp.sd.ctr = s->star_ctr.p;
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
  size_t li = 0, star0 = 0;
  for (int bi = 0; bi < PCLEAN_MAX_BLOCKS; ++bi) {
    OwnBlock& b = s->block[bi];
    if (!b.valid) continue;
    for (size_t ni = 0; ni < b.leaves.size(); ++ni, ++li) {
      const int si = b.star_of[ni];
      if (si >= 0 && b.stars[si].head != (int)ni) continue;  // (an arm: drawn in its head's launch)
      OwnLeaf& lf = si >= 0 ? b.stars[si].grp : b.leaves[ni];
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
      const StarPlan* sp = si >= 0 ? &stars[star0 + si] : nullptr;
      const int rc = sp ? launch_star(ctx, s, sp->od, sp->sd, sp->lds, L, nullptr, lf.n_pieces) : launch_leaf(ctx, lf, ods[li], L, lf.n_pieces, s);
      if (rc) return rc;
      s->stats.n_runs += lf.n_runs;
      s->stats.longest_run = std::max(s->stats.longest_run, lf.longest);
    }
    star0 += b.stars.size();
  }
  hipLaunchKernelGGL(own_bad_rows_kernel, grid1(N), dim3(256), 0, ctx->stream, N, win_lo, (const double*)d_logml, s->bad.p);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(s->ev[1], ctx->stream));
  int32_t bad[2] = {0, 0};
  unsigned long long ctr[2] = {0ull, 0ull};
  HIPCHK(ctx, hipMemcpyAsync(bad, s->bad.p, 8, hipMemcpyDeviceToHost, ctx->stream));
  if (!stars.empty()) HIPCHK(ctx, hipMemcpyAsync(ctr, s->star_ctr.p, 16, hipMemcpyDeviceToHost, ctx->stream));
  if (chosen_particle) HIPCHK(ctx, hipMemcpyAsync(chosen_particle, d_chosen, (size_t)N * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (logml) HIPCHK(ctx, hipMemcpyAsync(logml, d_logml, (size_t)N * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCLEAN_SYNC(ctx);
  ctx->timing = pclean_timing{};
  (void)hipEventElapsedTime(&ctx->timing.total_ms, s->ev[0], s->ev[1]);
  s->stats.impossible_rows = bad[0];
  s->stats.first_impossible_row = bad[0] ? bad[1] : -1;
  s->stats.star_weighed = (int64_t)ctr[0];
  s->stats.star_skipped = (int64_t)ctr[1];
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
  OwnStar* star = b->star_of[node_id] >= 0 ? &b->stars[b->star_of[node_id]] : nullptr;
  OwnLeaf& lf = star ? star->grp : b->leaves[node_id];  // (a star: the grouping over the terms of all its nodes)
  OwnNodeDev od;
  OwnStarDev sd;
  size_t star_lds = 0;
  int rc;
  if (star) {
    rc = ensure_groups(ctx, lf);
    if (!rc) rc = ensure_aux(ctx, s);
    if (!rc) rc = star_dev(ctx, *b, *star, block_id, node_id - star->head, od, sd, &star_lds);
  } else {
    rc = leaf_dev(ctx, lf, od);
    if (!rc) rc = ensure_groups(ctx, lf);
  }
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
  const int K = !star ? od.n_cand : sd.target == 0 ? sd.ka : sd.ka * sd.kj[sd.target - 1];
  int32_t* d_row = scratch<int32_t>(ctx, n_items);
  int32_t* d_order = scratch<int32_t>(ctx, n_items);
  int32_t* d_poff = scratch<int32_t>(ctx, poff.size());
  double* d_lse = scratch<double>(ctx, n_items);
  double* d_scores = scores ? scratch<double>(ctx, (size_t)n_items * K) : nullptr;
  int32_t* d_draws = n_draws ? scratch<int32_t>(ctx, (size_t)n_items * n_draws) : nullptr;
  if (!d_row || !d_order || !d_poff || !d_lse || (scores && !d_scores) || (n_draws && !d_draws))
    return pclean_fail(ctx, PCLEAN_ERR_HIP, "scratch alloc failed");
  if (star) {
    sd.abuf = scratch<int32_t>(ctx, (size_t)n_items * std::max(n_draws, 1));
    if (!sd.abuf) return pclean_fail(ctx, PCLEAN_ERR_HIP, "scratch alloc failed");
    sd.ctr = s->star_ctr.p;
    HIPCHK(ctx, hipMemsetAsync(s->star_ctr.p, 0, 16, ctx->stream));
  }
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
  rc = star ? launch_star(ctx, s, od, sd, star_lds, L, nullptr, n_pieces) : launch_leaf(ctx, lf, od, L, n_pieces, s);
  if (rc) return rc;
  unsigned long long ctr[2] = {0ull, 0ull};
  if (star) HIPCHK(ctx, hipMemcpyAsync(ctr, s->star_ctr.p, 16, hipMemcpyDeviceToHost, ctx->stream));
  if (lse) HIPCHK(ctx, hipMemcpyAsync(lse, d_lse, (size_t)n_items * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (scores) HIPCHK(ctx, hipMemcpyAsync(scores, d_scores, (size_t)n_items * K * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (n_draws) HIPCHK(ctx, hipMemcpyAsync(draws, d_draws, (size_t)n_items * n_draws * 4, hipMemcpyDeviceToHost, ctx->stream));
  PCLEAN_SYNC(ctx);  // (h_row / order / poff are read by the copies queued above)
  s->stats.star_weighed = (int64_t)ctr[0];
  s->stats.star_skipped = (int64_t)ctr[1];
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
  OwnStar* star = b->star_of[node_id] >= 0 ? &b->stars[b->star_of[node_id]] : nullptr;
  OwnLeaf& lf = star ? star->grp : b->leaves[node_id];
  OwnNodeDev od;
  OwnStarDev sd;
  size_t star_lds = 0;
  int rc = star ? PCLEAN_OK : leaf_dev(ctx, lf, od);
  if (!rc) rc = ensure_groups(ctx, lf);
  if (!rc && cur_prob) rc = ensure_vals(ctx, *b);
  if (!rc) rc = ensure_aux(ctx, s);
  if (!rc && star) rc = star_dev(ctx, *b, *star, block_id, node_id - star->head, od, sd, &star_lds);
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
  OwnGaussDev gd;
  size_t glds = 0;
  if (!lf.gauss.empty()) {
    rc = own_gauss_plan(ctx, lf, od, gd, &glds);
    if (rc) return rc;
  }
  HIPCHK(ctx, hipEventRecord(s->ev[0], ctx->stream));
  if (star) {  // the head's exact marginal, or an arm's conditional at the head's first value
    rc = launch_star(ctx, s, od, sd, star_lds, OwnLaunch{}, &L, lf.n_pieces);
    if (rc) return rc;
  } else if (lf.n_pieces > 0 && !lf.gauss.empty()) {
    hipLaunchKernelGGL(own_gauss_kernel<true>, dim3(lf.n_pieces), dim3(OWN_BT), glds, ctx->stream, od, dn, gd, OwnLaunch{}, L);
    HIPCHK(ctx, hipGetLastError());
    s->stats.variants |= 8;
    s->stats.n_workgroups += lf.n_pieces;
  } else if (lf.n_pieces > 0) {  // (a lane keeps 1 entry for top == 1, OWN_MAX_TOP otherwise)
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
  const OwnStar* star = b->star_of[node_id] >= 0 ? &b->stars[b->star_of[node_id]] : nullptr;
  if (star && node_id != star->head) {  // an arm: the joint histogram of (head value, arm value)
    const int ka = ctx->cand[b->leaves[star->head].node.table].n_rows;
    if (ka < 1 || K % ka) return pclean_fail(ctx, PCLEAN_ERR_STATE, "pclean_own_counts: the arm's table is no grid over the head's %d options", ka);
    if (ctx->n_rows) {
      const unsigned blocks = (unsigned)std::min<size_t>(((size_t)ctx->n_rows + 255) / 256, 1024);
      hipLaunchKernelGGL(own_star_counts_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->n_rows, ka, K / ka,
                         (const int32_t*)(b->vals.p + (size_t)star->head * ctx->n_rows),
                         (const int32_t*)(b->vals.p + (size_t)node_id * ctx->n_rows), s->hist.p);
      HIPCHK(ctx, hipGetLastError());
    }
  } else if (ctx->n_rows) {
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)ctx->n_rows + 255) / 256, 1024);
    hipLaunchKernelGGL(own_counts_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->n_rows, K,
                       (const int32_t*)(b->vals.p + (size_t)node_id * ctx->n_rows), s->hist.p);
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, hipMemcpyAsync(counts, s->hist.p, (size_t)K * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCLEAN_SYNC(ctx);
  return PCLEAN_OK;
}

extern "C" int pclean_add_own_gauss(pclean_ctx* ctx, int32_t block_id, int32_t node_id, const pclean_gauss* g) {
  OwnBlock* b = find_block(ctx, block_id);
  if (!b) return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_add_own_gauss: block %d is not a loaded own block", block_id);
  if (node_id < 0 || node_id >= (int)b->leaves.size() || !g)
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_add_own_gauss: block %d has no node %d", block_id, node_id);
  OwnLeaf& lf = b->leaves[node_id];
  int rc = check_own_gauss(ctx, lf, *g, PCLEAN_ERR_ARG, "pclean_add_own_gauss");
  if (rc) return rc;
  if (!lf.gauss.empty() && (lf.gauss[0].n_locals != g->n_locals || lf.gauss[0].local_n[0] != g->local_n[0] ||
                            (g->n_locals > 1 && lf.gauss[0].local_n[1] != g->local_n[1])))
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_add_own_gauss: the terms of a node share its option columns (n_locals, local_n)");
  if ((int)lf.gauss.size() >= PCLEAN_MAX_GAUSS)
    return pclean_fail(ctx, PCLEAN_ERR_CAPACITY, "pclean_add_own_gauss: more than %d Gaussian terms on node %d", PCLEAN_MAX_GAUSS, node_id);
  // the exponent of the term's fixed-point statistics: the largest finite |bx| over its units and the present rows
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int N = ctx->n_rows;
  const int n_units = g->transform_src_kind == PCLEAN_GSRC_LOCAL ? g->local_n[g->transform_src] : 1;
  double M = 0.0;
  if (N > 0) {
    std::vector<double> x(N), tx(N);
    HIPCHK(ctx, hipMemcpy(x.data(), ctx->xnum.p + (size_t)g->x_col * N, (size_t)N * 8, hipMemcpyDeviceToHost));
    for (int u = 0; u < n_units; ++u) {
      if (g->t_x_col[u] >= 0) HIPCHK(ctx, hipMemcpy(tx.data(), ctx->xnum.p + (size_t)g->t_x_col[u] * N, (size_t)N * 8, hipMemcpyDeviceToHost));
      for (int i = 0; i < N; ++i) {
        if (x[i] != x[i]) continue;
        const double bx = std::fabs(g->t_x_col[u] >= 0 ? tx[i] : x[i] * g->t_scale[u]);
        if (bx <= 1.7976931348623157e308 && bx > M) M = bx;
      }
    }
  }
  lf.gauss.push_back(*g);
  lf.gauss_e.push_back(pclean_ownq_exponent(M, N));
  return PCLEAN_OK;
}

extern "C" int pclean_own_gauss_stats(pclean_ctx* ctx, int32_t block_id, int32_t node_id, int32_t term, int64_t* count, int64_t* qsum,
                                      int32_t* exponent) {
  OwnBlock* b = find_block(ctx, block_id);
  if (!b || node_id < 0 || node_id >= (int)b->leaves.size())
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_own_gauss_stats: block %d node %d is not a node of a loaded own block", block_id, node_id);
  OwnLeaf& lf = b->leaves[node_id];
  if (term < 0 || term >= (int)lf.gauss.size() || (!count) != (!qsum))
    return pclean_fail(ctx, PCLEAN_ERR_ARG, "pclean_own_gauss_stats: node %d has no Gaussian term %d (or only one of count / qsum is given)",
                       node_id, term);
  if (exponent) *exponent = lf.gauss_e[term];
  if (!count) return PCLEAN_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  OwnNodeDev od;
  OwnGaussDev gd;
  size_t glds = 0;
  int rc = leaf_dev(ctx, lf, od);
  if (!rc) rc = own_gauss_plan(ctx, lf, od, gd, &glds);
  if (!rc) rc = ensure_vals(ctx, *b);
  OwnState* s = own(ctx);
  if (!rc) rc = ensure_aux(ctx, s);
  if (rc) return rc;
  const int n_mean = ctx->mean[lf.gauss[term].mean_table].n;
  if (s->gstat.alloc((size_t)2 * n_mean)) return pclean_fail(ctx, PCLEAN_ERR_HIP, "device alloc failed");
  HIPCHK(ctx, hipEventRecord(s->ev[0], ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(s->gstat.p, 0, (size_t)2 * n_mean * 8, ctx->stream));
  if (ctx->n_rows) {
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)ctx->n_rows + 255) / 256, 1024);
    hipLaunchKernelGGL(own_gauss_stats_kernel, dim3(blocks), dim3(256), 0, ctx->stream, ctx->n_rows, od.n_cand,
                       (const int32_t*)(b->vals.p + (size_t)node_id * ctx->n_rows), gd, term, n_mean, pclean_ownq_scale(lf.gauss_e[term]),
                       s->gstat.p, s->gstat.p + n_mean);
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, hipEventRecord(s->ev[1], ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(count, s->gstat.p, (size_t)n_mean * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(qsum, s->gstat.p + n_mean, (size_t)n_mean * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCLEAN_SYNC(ctx);
  ctx->timing = pclean_timing{};
  (void)hipEventElapsedTime(&ctx->timing.total_ms, s->ev[0], s->ev[1]);  // (the clearing and the kernel: pclean_get_timing)
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
