// Device/host-shared evaluation of the Gaussian term (pclean_gauss): marginal over the
// enumerated locals of  logp(locals) + logpdf(Normal(mean, sigma), backward(x)) - log|g'|
// (src/distributions/transformed_gaussian.jl:15-16, add_noise.jl:7, choose_uniformly.jl:7-10).
// The oracle (oracle/enumerate.h) restates the same operation order.
#pragma once
#include "../../include/pclean_detmath.h"
#include "enum.h"

#define PCLEAN_LOG_SQRT_2PI 0.91893853320467274178

__device__ __forceinline__ double gauss_normal_logpdf(double x, double mu, double sigma, double log_sigma) {
  const double z = (x - mu) / sigma;
  return -0.5 * z * z - log_sigma - PCLEAN_LOG_SQRT_2PI;
}

// Index of term g's mean for the non-local dimensions (base) and the strides of the own choices it indexes; val(g, d) gives
// the value of index dimension d for the non-local kinds.
template <typename ValFn>
__device__ __forceinline__ int gauss_index_base(const GaussDev& g, ValFn val, int* lstride) {
  int base = 0;
  lstride[0] = lstride[1] = 0;
  for (int d = 0; d < g.n_dims; ++d) {
    if (g.src_kind[d] == PCLEAN_GSRC_LOCAL)
      lstride[g.src_slot[d]] = g.stride[d];
    else
      base += g.stride[d] * val(g, d);
  }
  return base;
}

// s += logpdf;  s -= log|deriv|  of term g (its number xv is present) for the own choices (l0, l1)
__device__ __forceinline__ double gauss_add_term(const GaussDev& g, double s, double xv, int row, const int32_t* evctx, int base,
                                                 const int* lstride, int l0, int l1) {
  const int idx = base + lstride[0] * l0 + lstride[1] * l1;
  int u = 0;
  if (g.t_kind == PCLEAN_GSRC_LOCAL)
    u = g.t_src == 0 ? l0 : l1;
  else if (g.t_kind == PCLEAN_GSRC_EVCTX)
    u = evctx[g.t_src];
  s += gauss_normal_logpdf(g.tx[u] ? g.tx[u][row] : xv * g.t_scale[u], g.mu[idx], g.sigma, g.log_sigma);
  s -= g.tl[u] ? g.tl[u][row] : g.t_lad[u];
  return s;
}

// Scores of the (l0, l1) combinations of the node's Gaussian terms — `g0`, then more[0 .. n_more) in declaration order — for
// one candidate; returns the number of combinations written to sc[] / codes[] (code = l0 * 16 + l1), 0 when every term's
// number is missing for this row.  The terms share the block's own choices (pclean_add_node_gauss), so the bounds and prior
// densities of the locals are those of g0, computed once; each term has its own index base, strides, x, mean table, sigma
// and transformation columns.  Per combination the fp64 order is  s = lp[0] + lp[1];  then per present term  s += logpdf;
// s -= log|deriv|.  The enumeration itself scores the first term, as it always did: a one-term node makes one pass and
// writes sc[n] once.  Only the further terms walk sc[] again and add in place (no second array).
template <typename ValFn>
__device__ __forceinline__ int gauss_combo_scores(const GaussDev& g0, const GaussDev* more, int n_more, int row,
                                                  const int32_t* evctx, ValFn val, double* sc, int* codes) {
  const double x0 = g0.x[row];
  bool any = x0 == x0;  // (a missing numeric observation: the term is skipped)
  if (!any && n_more == 0) return 0;
  int lo[2] = {0, 0}, hi[2] = {1, 1};
  double lp[2] = {0.0, 0.0};
  for (int l = 0; l < g0.n_locals; ++l) {
    lo[l] = 0;
    hi[l] = g0.local_n[l];
    lp[l] = g0.local_logp[l];
    if (g0.local_obs[l]) {
      const int v = g0.local_obs[l][row];
      if (v >= 0) {
        lo[l] = v;
        hi[l] = v + 1;
      }
    }
  }
  int lstride[2] = {0, 0};  // strides of the first term (read only when its number is present)
  const int base0 = any ? gauss_index_base(g0, val, lstride) : 0;
  int n = 0;
  for (int l0 = lo[0]; l0 < hi[0]; ++l0)
    for (int l1 = lo[1]; l1 < hi[1]; ++l1) {
      double s = lp[0] + lp[1];
      if (any) s = gauss_add_term(g0, s, x0, row, evctx, base0, lstride, l0, l1);
      sc[n] = s;
      codes[n] = l0 * 16 + l1;
      ++n;
    }
  for (int t = 0; t < n_more; ++t) {
    const GaussDev& g = more[t];
    const double xv = g.x[row];
    if (xv != xv) continue;
    any = true;
    int ls[2];  // (this term's own strides)
    const int base = gauss_index_base(g, val, ls);
    for (int c = 0; c < n; ++c) sc[c] = gauss_add_term(g, sc[c], xv, row, evctx, base, ls, codes[c] >> 4, codes[c] & 15);
  }
  return any ? n : 0;
}

// marginal (fixed-point log-sum-exp) of the combination scores; a single combination is returned as is
__device__ __forceinline__ double gauss_lse(const double* sc, int n) {
  if (n == 1) return sc[0];
  double m = -__builtin_inf();
  for (int i = 0; i < n; ++i) m = fmax(m, sc[i]);
  if (m == -__builtin_inf()) return m;
  uint64_t U = 0;
  for (int i = 0; i < n; ++i) U += pclean_fixw(sc[i] - m);
  return pclean_lse_from_fix(m, U);
}
