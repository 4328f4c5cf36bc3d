// The grid rule of pclean_link_own_star (own_block.hip), host C++ alone so that it can be run under sanitizers from a program
// of its own (tests/own_star_host).  An arm's option table holds n_cand = K_a * K_j options, key-major: column 0 of option
// a * K_j + b is the head's value of option a, column 1 is the arm's value of option b (the same for every a).  Unlike the
// grid test of pclean_set_options_cols this one is told K_a, so 1 x n, n x 1 and grids below 4 options are grids too.
#ifndef PCLEAN_OWN_STAR_CHECK_H
#define PCLEAN_OWN_STAR_CHECK_H
#include <cstddef>
#include <cstdint>
#include <cstdio>

#define OWN_STAR_MAX_ARMS 4
#define OWN_STAR_MAX_K 4096            // values of the index or of a dependent: an arm's chunk sums fit the lanes of a wavefront
#define OWN_STAR_MAX_GRID (64 * 4096)  // K_a * K_j (OWN_MAX_OPTIONS)

// 0: the table is the grid, *kj_out = K_j.  Otherwise a negative number and a message in msg.
inline int own_star_check_grid(int32_t ka, const int32_t* head_vals, int64_t n_cand, const int32_t* col0, const int32_t* col1,
                               int32_t* kj_out, char* msg, size_t msg_len) {
  if (ka < 1 || ka > OWN_STAR_MAX_K || !head_vals) {
    snprintf(msg, msg_len, "the head holds %d options (1 .. %d are served)", ka, OWN_STAR_MAX_K);
    return -1;
  }
  if (n_cand < 1 || !col0 || !col1 || n_cand % ka) {
    snprintf(msg, msg_len, "an arm of %lld options is no grid over the head's %d", (long long)n_cand, ka);
    return -2;
  }
  const int64_t kj = n_cand / ka;
  if (kj > OWN_STAR_MAX_K) {
    snprintf(msg, msg_len, "an arm with %lld values (at most %d are served)", (long long)kj, OWN_STAR_MAX_K);
    return -3;
  }
  if (n_cand > OWN_STAR_MAX_GRID) {
    snprintf(msg, msg_len, "an arm's grid of %lld options (at most %d)", (long long)n_cand, OWN_STAR_MAX_GRID);
    return -4;
  }
  for (int64_t a = 0; a < ka; ++a)
    for (int64_t b = 0; b < kj; ++b) {
      const int64_t k = a * kj + b;
      if (col0[k] != head_vals[a]) {
        snprintf(msg, msg_len, "option %lld: column 0 holds %d, the head's option %lld holds %d", (long long)k, col0[k], (long long)a,
                 head_vals[a]);
        return -5;
      }
      if (col1[k] != col1[b]) {
        snprintf(msg, msg_len, "option %lld: column 1 holds %d, option %lld holds %d (the grid is key-major)", (long long)k, col1[k],
                 (long long)b, col1[b]);
        return -6;
      }
    }
  *kj_out = (int32_t)kj;
  return 0;
}

// every value a term reads lies inside the term's latent domain: 0, or the index of the first value that does not
inline int64_t own_star_check_values(int64_t n, const int32_t* vals, int32_t n_lat) {
  for (int64_t i = 0; i < n; ++i)
    if (vals[i] < 0 || vals[i] >= n_lat) return i + 1;
  return 0;
}

// dynamic LDS of own_star_kernel in bytes: the cached term values, S(a), the head's chunk sums
inline size_t own_star_lds_bytes(int32_t ka, int32_t n_arms, const int32_t* kj, const int32_t* terms_per_node) {
  size_t total = (size_t)terms_per_node[0] * (size_t)ka;
  for (int j = 0; j < n_arms; ++j) total += (size_t)terms_per_node[1 + j] * (size_t)kj[j];
  return (total + (size_t)ka + (size_t)((ka + 63) / 64)) * 8;
}
#endif
