// TEST INFRASTRUCTURE: commit_host.cpp plus one entry for leaves with several value columns (a product leaf): the option
// values of leaf `node` of plan p as a column-major [value columns][stride] array, the way pclean_amd/csrc/commit.hip hands
// the device build of commit_core.h an option table and its number of options.
#include "commit_host.cpp"

extern "C" int pcch_set_leaf_columns(void* hv, int p, int node, const int32_t* vals, int stride) {
  Harness* h = (Harness*)hv;
  if (!h->built || p < 0 || p >= h->sc.n_plans || node < 0 || node >= h->sc.plans[p].n_nodes || h->sc.plans[p].kind[node] != 1)
    return -1;
  h->sc.plans[p].opt_vals[node] = vals;
  h->sc.plans[p].opt_stride[node] = stride;
  return 0;
}
