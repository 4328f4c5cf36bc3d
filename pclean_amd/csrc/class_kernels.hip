// Class tables of the tabulated likelihood terms (PCLEAN_DENS_TABULATED): C[u][v] = class of the pair (observed string u,
// latent string v) under ExpandOnShortVersion's or FormatName's rule (expand_on_short_version.jl:6-19,30-41 /
// format_name.jl:33-55), one byte per pair in the layout of the distance tables, and the per-latent-value count of the
// options a latent string is a short version of.
//
// class_table_kernel<RULE> — 256 lanes along the LATENT values (byte stores coalesced along n_lat), blockIdx.y walks chunks
// of CLS_OBS_PER_BLOCK observed strings.  An observed string's folded symbols are staged in LDS once per workgroup, in
// pieces of CLS_PIECE symbols, so strings of any length take the same path; every lane walks the piece with its own
// two-pointer state (O(length of the observed string) per pair) and reads its latent string's next symbol only when its
// pointer advances.
// The rules PCLEAN_CLASS_NAME_PREFIX / _SUFFIX (the byte tables of the three-name FormatName term) take the same kernel:
// a lane's walk is decided at the first mismatch and reads its latent string only at the positions the affix covers.
// short_count_kernel — the same walk against the option strings; a lane sums over its workgroup's options in a register
// and adds the partial count with one integer atomic per latent value (sums of integers: order independent).
#include <algorithm>

#include "class_rules.h"
#include "ctx.h"

#define CLS_T 256
#define CLS_PIECE 64           // observed symbols staged in LDS at a time
#define CLS_OBS_PER_BLOCK 16   // observed strings (options) one workgroup walks
#define CLS_MAX_GRID_Y 65535

// class of (long / observed string at sym[llo .. llo + l), lane's latent string at sym[slo .. slo + s)); every thread of the
// workgroup calls it (it synchronises), `live` lanes compute.  s_long: CLS_PIECE words of LDS.
template <int RULE>
__device__ __forceinline__ int pair_class(const uint16_t* __restrict__ sym, const uint16_t* __restrict__ fold, int64_t llo,
                                          int l, int64_t slo, int s, bool live, uint16_t dotf, uint16_t* s_long) {
  const uint16_t first = (live && s > 0) ? fold[sym[slo]] : (uint16_t)0;
  ShortWalk w{0, first};
  bool eq = true, init = false;
  bool affix = name_affix_start(s, l);  // (the two name rules: dotf is the folded separator)
  for (int p0 = 0; p0 < l; p0 += CLS_PIECE) {
    const int np = min(CLS_PIECE, l - p0);
    __syncthreads();  // (the previous piece, or the previous string, is consumed)
    if ((int)threadIdx.x < np) s_long[threadIdx.x] = fold[sym[llo + p0 + threadIdx.x]];
    __syncthreads();
    if (!live) continue;
    if (RULE == PCLEAN_CLASS_SHORT_VERSION) {
      if (w.a >= s) continue;  // (matched: nothing left to look for)
      for (int b = 0; b < np; ++b) short_walk_step(w, s, s_long[b], [&](int a) { return fold[sym[slo + a]]; });
    } else if (RULE == PCLEAN_CLASS_NAME_PREFIX) {
      if (!affix || p0 > s) continue;  // (decided, or past the separator)
      for (int b = 0; b < np; ++b)
        affix = name_prefix_step(affix, p0 + b, s, s_long[b], dotf, [&](int a) { return fold[sym[slo + a]]; });
    } else if (RULE == PCLEAN_CLASS_NAME_SUFFIX) {
      if (!affix || p0 + np <= l - s - 1) continue;  // (decided, or the piece ends before the separator)
      for (int b = 0; b < np; ++b)
        affix = name_suffix_step(affix, p0 + b, s, l, s_long[b], dotf, [&](int a) { return fold[sym[slo + a]]; });
    } else {
      if (p0 == 0 && l == 2 && s >= 1) init = s_long[0] == first && s_long[1] == dotf;
      const int nb = min(np, s - p0);  // (symbols of the piece that the name has a counterpart for)
      for (int b = 0; b < nb && eq; ++b) eq = fold[sym[slo + p0 + b]] == s_long[b];
    }
  }
  if (RULE == PCLEAN_CLASS_SHORT_VERSION) return short_walk_class(w, s);
  if (RULE == PCLEAN_CLASS_NAME_PREFIX || RULE == PCLEAN_CLASS_NAME_SUFFIX) return affix ? 1 : 0;
  return format_name_class_of(eq, init, s, l);
}

template <int RULE>
__global__ __launch_bounds__(CLS_T) void class_table_kernel(const uint16_t* __restrict__ sym, const int64_t* __restrict__ off,
                                                            const uint16_t* __restrict__ fold,
                                                            const int32_t* __restrict__ obs_ids,
                                                            const int32_t* __restrict__ lat_ids, int obs_begin, int n_obs,
                                                            int n_lat, uint16_t dotf, uint8_t* __restrict__ out) {
  __shared__ uint16_t s_long[CLS_PIECE];
  const int v = blockIdx.x * CLS_T + threadIdx.x;
  const bool live = v < n_lat;
  int64_t slo = 0;
  int s = 0;
  if (live) {
    const int id = lat_ids[v];
    slo = off[id];
    s = (int)(off[id + 1] - slo);
  }
  const int u0 = obs_begin + blockIdx.y * CLS_OBS_PER_BLOCK, u1 = min(u0 + CLS_OBS_PER_BLOCK, n_obs);
  for (int u = u0; u < u1; ++u) {  // (uniform over the workgroup)
    const int id = obs_ids[u];
    const int64_t llo = off[id];
    const int l = (int)(off[id + 1] - llo);
    const int c = pair_class<RULE>(sym, fold, llo, l, slo, s, live, dotf, s_long);
    if (live) out[(size_t)u * n_lat + v] = (uint8_t)c;
  }
}

__global__ __launch_bounds__(CLS_T) void short_count_kernel(const uint16_t* __restrict__ sym, const int64_t* __restrict__ off,
                                                            const uint16_t* __restrict__ fold,
                                                            const int32_t* __restrict__ opt_ids,
                                                            const int32_t* __restrict__ lat_ids, int opt_begin, int n_opt,
                                                            int n_lat, int32_t* __restrict__ out) {
  __shared__ uint16_t s_long[CLS_PIECE];
  const int v = blockIdx.x * CLS_T + threadIdx.x;
  const bool live = v < n_lat;
  int64_t slo = 0;
  int s = 0;
  if (live) {
    const int id = lat_ids[v];
    slo = off[id];
    s = (int)(off[id + 1] - slo);
  }
  const int u0 = opt_begin + blockIdx.y * CLS_OBS_PER_BLOCK, u1 = min(u0 + CLS_OBS_PER_BLOCK, n_opt);
  int cnt = 0;
  for (int u = u0; u < u1; ++u) {
    const int id = opt_ids[u];
    const int64_t llo = off[id];
    const int l = (int)(off[id + 1] - llo);
    cnt += pair_class<PCLEAN_CLASS_SHORT_VERSION>(sym, fold, llo, l, slo, s, live, 0, s_long) == 0 ? 1 : 0;
  }
  if (live && cnt) atomicAdd(out + v, cnt);
}

// grid.y walks the chunks of observed strings; the host loops so that gridDim.y <= 65535
template <typename Launch>
static void for_chunks(int n, Launch launch) {
  const int per_launch = CLS_MAX_GRID_Y * CLS_OBS_PER_BLOCK;
  for (int begin = 0; begin < n; begin += per_launch) {
    const int cnt = std::min(per_launch, n - begin);
    launch(begin, (cnt + CLS_OBS_PER_BLOCK - 1) / CLS_OBS_PER_BLOCK);
  }
}

int pclean_launch_class_table(pclean_ctx* ctx, PairTable& pt, const int32_t* d_obs_ids, const int32_t* d_lat_ids, int rule,
                              int dot_symbol) {
  if (pt.n_obs <= 0) return PCLEAN_OK;
  // the dot in folded symbols; 0xFFFF (no pool symbol: pclean_load_strings keeps them below 0xfffe) matches nothing
  uint16_t dotf = 0xFFFF;
  if (dot_symbol != 0xFFFF)
    HIPCHK(ctx, hipMemcpy(&dotf, ctx->fold.p + dot_symbol, sizeof(uint16_t), hipMemcpyDeviceToHost));
  const unsigned gx = (unsigned)((pt.n_lat + CLS_T - 1) / CLS_T);
  for_chunks(pt.n_obs, [&](int begin, int gy) {
    if (rule == PCLEAN_CLASS_SHORT_VERSION)
      hipLaunchKernelGGL(class_table_kernel<PCLEAN_CLASS_SHORT_VERSION>, dim3(gx, gy), dim3(CLS_T), 0, ctx->stream, ctx->sym.p,
                         ctx->off.p, ctx->fold.p, d_obs_ids, d_lat_ids, begin, pt.n_obs, pt.n_lat, dotf, pt.d.p);
    else if (rule == PCLEAN_CLASS_NAME_PREFIX)
      hipLaunchKernelGGL(class_table_kernel<PCLEAN_CLASS_NAME_PREFIX>, dim3(gx, gy), dim3(CLS_T), 0, ctx->stream, ctx->sym.p,
                         ctx->off.p, ctx->fold.p, d_obs_ids, d_lat_ids, begin, pt.n_obs, pt.n_lat, dotf, pt.d.p);
    else if (rule == PCLEAN_CLASS_NAME_SUFFIX)
      hipLaunchKernelGGL(class_table_kernel<PCLEAN_CLASS_NAME_SUFFIX>, dim3(gx, gy), dim3(CLS_T), 0, ctx->stream, ctx->sym.p,
                         ctx->off.p, ctx->fold.p, d_obs_ids, d_lat_ids, begin, pt.n_obs, pt.n_lat, dotf, pt.d.p);
    else
      hipLaunchKernelGGL(class_table_kernel<PCLEAN_CLASS_FORMAT_NAME>, dim3(gx, gy), dim3(CLS_T), 0, ctx->stream, ctx->sym.p,
                         ctx->off.p, ctx->fold.p, d_obs_ids, d_lat_ids, begin, pt.n_obs, pt.n_lat, dotf, pt.d.p);
  });
  HIPCHK(ctx, hipGetLastError());
  return PCLEAN_OK;
}

int pclean_launch_short_count(pclean_ctx* ctx, int n_opt, const int32_t* d_opt_ids, int n_lat, const int32_t* d_lat_ids,
                              int32_t* d_out) {
  if (n_opt <= 0) return PCLEAN_OK;
  const unsigned gx = (unsigned)((n_lat + CLS_T - 1) / CLS_T);
  for_chunks(n_opt, [&](int begin, int gy) {
    hipLaunchKernelGGL(short_count_kernel, dim3(gx, gy), dim3(CLS_T), 0, ctx->stream, ctx->sym.p, ctx->off.p, ctx->fold.p,
                       d_opt_ids, d_lat_ids, begin, n_opt, n_lat, d_out);
  });
  HIPCHK(ctx, hipGetLastError());
  return PCLEAN_OK;
}
