"""enum_product_kernel (a product leaf scored one factor at a time) against the generic enumeration kernels, bit for bit:
the same program swept in two fresh processes, with and without PCLEAN_NO_PRODUCT_LEAF=1 (the switch is read once per
process, as PCLEAN_SORT_GROUPS is) — log-marginals and scores of the leaf, draws, referents, chosen particles, log-weights
and new-row records at P = 2 (MH), 5 and 20 over 64 rows that all start without a referent.  Shapes: 3 x 5; 7 x 300 =
2 100 options (the generic LDS kernel); 51 x 500 = 25 500 (the generic recomputing kernel; the product kernel keeps its
prefix in global recomputation too); 2 x 21 000, whose cached term values (21 000 doubles = 164 KB) exceed the LDS of a
workgroup: the profile must show that it fell back.  The profile's phase names say which path a leaf's launch took, and
pclean_debug_enum_launches which of enum_product_kernel's four instantiations ran: <256, prefix in LDS> at 3 x 5 and
7 x 300, <1024, not in LDS> at 51 x 500, <1024, in LDS> at 10 x 500 = 5 000 options, and <256, not in LDS> at 51 x 500 over
1 100 rows (more items than the 1024-thread kernels take).  The two children of a case run one after the other."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r'''
import hashlib, sys
import numpy as np
sys.path[:0] = [ROOT, ROOT + "/tests"]
import indexed_program as ip
from pclean_amd.engine import Engine, InferenceConfig
S = ip.product_shape_program(NA, NB, NR)
lw, obs, tr = S["lw"], S["obs"], S["trace"]
eng = Engine(lw, obs, dist_mode=1)
h = hashlib.sha256()
try:
    eng.upload_trace(tr)
    eng.hip.set_profiling(True)
    n = obs.shape[1]
    lse, scores, draws = eng.hip.score_node(0, 1, np.arange(n, dtype=np.int32), n_cand=NA * NB, want_scores=True, n_draws=3, seed=5)
    assert np.isfinite(lse).all()
    for a in (lse, scores, draws):
        h.update(np.ascontiguousarray(a).tobytes())
    for P, mh in ((2, True), (5, False), (20, False)):
        for sweep in range(2):
            choice, chosen, logml, new_rows = eng.sweep(tr, InferenceConfig(1, P, use_mh_instead_of_pg=mh), 31, sweep)
            assert (choice[0] == -1).all() and len(new_rows[0][0]) == n  # every row takes the new-row branch
            for a in (choice, chosen, logml, new_rows[0][0], new_rows[0][1]):
                h.update(np.ascontiguousarray(a).tobytes())
    print("DIGEST", h.hexdigest(), "PHASES", ",".join(sorted(eng.hip.get_profile())),
          "LAUNCHES", ",".join(k for k, v in eng.hip.enum_launches().items() if v > 0))
finally:
    eng.close()
'''


def _run(na, nb, nr, env_extra):
    env = dict(os.environ)
    env.pop("PCLEAN_NO_PRODUCT_LEAF", None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nNA, NB, NR = {na}, {nb}, {nr}\n" + SCRIPT], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("DIGEST")][-1].split()
    return line[1], set(line[3].split(",")), set(line[5].split(",") if len(line) > 5 else ())


@pytest.mark.parametrize("na,nb,nr,slot", [(3, 5, 64, "product_256_lds"), (7, 300, 64, "product_256_lds"),
                                           (51, 500, 64, "product_1024"), (2, 21000, 64, None),
                                           (10, 500, 64, "product_1024_lds"), (51, 500, 1100, "product_256")],
                         ids=["3x5", "7x300", "51x500", "2x21000-beyond-LDS", "10x500", "51x500-1100-rows"])
def test_product_kernel_equals_generic_kernels(na, nb, nr, slot, capsys):
    fits = slot is not None
    d_prod, ph_prod, ran_prod = _run(na, nb, nr, {})
    d_gen, ph_gen, ran_gen = _run(na, nb, nr, {"PCLEAN_NO_PRODUCT_LEAF": "1"})
    with capsys.disabled():
        print(f"\n[product kernel {na}x{nb}] default: {sorted(p for p in ph_prod if p.startswith('enum_leaf'))}; "
              f"switch: {sorted(p for p in ph_gen if p.startswith('enum_leaf'))}; launches: {sorted(ran_prod)}; "
              f"switch: {sorted(ran_gen)}")
    assert "enum_leaf_generic" in ph_gen and "enum_leaf_product" not in ph_gen
    if fits:
        assert "enum_leaf_product" in ph_prod and "enum_leaf_generic" not in ph_prod
    else:  # cached term values beyond LDS: the generic kernels, and the statistics say so
        assert "enum_leaf_generic" in ph_prod and "enum_leaf_product" not in ph_prod
    assert not any(k.startswith("product") for k in ran_gen)
    if fits:
        assert slot in ran_prod, (f"ran {sorted(ran_prod)}: a threshold of pclean_launch_product moved — move this shape to "
                                  f"the new threshold, do not loosen the assertion")
    else:
        assert not any(k.startswith("product") for k in ran_prod)
    assert d_prod == d_gen
