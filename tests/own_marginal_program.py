"""Exact marginals of a flat class (pclean_own_marginals): the definition restated in NumPy, a program with exact ties and
the bound against the literal conditional (TEST INFRASTRUCTURE; the programs are own_choice_program's).

  marginal_twin   from fp64 scores [rows][K] and a fixw function: m = max, u_k = fixw(s_k - m), U = sum of the u_k as
                  Python integers, the options with u_k > 0 in (-u_k, k) order, float64(u_k) / float64(U).  The fixw is the
                  device's (pclean_debug_detmath) in the GPU tests and the oracle library's pco_fixw on the CPU.
  TIES            state ~ ChooseUniformly(K words); y ~ AddTypos(state).  Rows without an observation tie all K options;
                  rows whose observation is one substitution away from two options of the same length tie those two: the
                  same operations on the same values, so the scores are equal to the bit.
  bound(K)        |u_k / U - pi_k| <= K 2^-40 + 1e-12: u_k 2^-40 lies within 2^-40 below e^(s_k - m), U 2^-40 within K 2^-40
                  below the sum of those, which is >= 1; 1e-12 covers the fp64 summation order of the two scorers."""
import math

import numpy as np

import own_choice_program as ocp
import posterior_exact as pe
from pclean_amd.model import AddTypos, ChooseUniformly, Model, Query

MAX_TOP = 8
TIE_PAIRS = (("qrstuva", "qrstuvb", "qrstuvc"), ("wxyzwxyza", "wxyzwxyzb", "wxyzwxyzc"))  # (option, option, observation)


def bound(K):
    return K * 2.0 ** -40 + 1e-12


def marginal_twin(scores, fixw, top):
    """(options int32 [top][n], probabilities float64 [top][n], u uint64 [n][K], U [n] Python integers)"""
    scores = np.asarray(scores, dtype=np.float64)
    n, K = scores.shape
    m = scores.max(axis=1)
    live = m > -math.inf
    u = np.zeros((n, K), dtype=np.uint64)
    if live.any():
        d = scores[live] - m[live, None]
        u[live] = np.asarray(fixw(np.ascontiguousarray(d).ravel()), dtype=np.uint64).reshape(-1, K)
    opt = np.full((top, n), -1, dtype=np.int32)
    prob = np.zeros((top, n), dtype=np.float64)
    U = []
    idx = np.arange(K)
    for i in range(n):
        U.append(sum(u[i].tolist()))
        order = np.lexsort((idx, np.uint64(2 ** 63) - u[i]))  # (-u, index); u <= 2^40
        order = order[u[i][order] > 0][:top]
        opt[:len(order), i] = order
        if U[i]:
            prob[:len(order), i] = u[i][order].astype(np.float64) / np.float64(U[i])
    return opt, prob, u, U


def current_twin(u, U, cur):
    """float64(u_cur) / float64(U) per row, 0.0 without a current value or with U == 0"""
    return np.array([np.float64(u[i, c]) / np.float64(U[i]) if c >= 0 and U[i] else 0.0 for i, c in enumerate(cur)])


def ties(K=70, seed=0, n_free=40):
    """TIES: the members of the first tie pair lie in different chunks of 64 options (different wavefronts hold them), those
    of the second in one chunk with the smaller index on the member named second; 66 rows share the second pair's
    observation (more than one wavefront of rows)"""
    rng = np.random.default_rng(seed)
    words = pe._words(rng, K - 4, 6, 10)
    (a0, a1, ao), (b0, b1, bo) = TIE_PAIRS
    words.insert(3, a0)
    words.insert(10, b1)
    words.insert(40, b0)
    words.insert(68, a1)
    assert len(words) == K and words.index(a1) - words.index(a0) > 64
    col = [None] * 5 + [ao] * 3 + [bo] * 66
    for _ in range(n_free):
        w = words[int(rng.integers(K))]
        col.append(w if rng.random() < 0.5 else pe._typo(rng, w))
    dirty = ocp._shuffled(rng, {"Y": col})
    m = Model()
    o = m.add_class("Obs")
    with o.block():
        o.choice("state", ChooseUniformly(words))
        o.choice("y", AddTypos("state"))
    q = Query(m, "Obs", {"Y": ("state", "y")})
    return ocp._spec(m, q, dirty, {"state": words}, {"state": [("Y", "typos", None)]})


def exact_rows(S, params, choice, mutate=None):
    """[(scores in option order float64 [K], {option: pi})] per row from the literal densities, one evaluation per distinct
    tuple of the row's observations; mutate(S, params) -> (S, params) changes what is scored (the power self-test)"""
    T, par = mutate(S, params) if mutate else (S, params)
    cols = [c for c, _, _ in S["terms"][choice]] + ([S["direct"][choice]] if choice in S["direct"] else [])
    memo, out = {}, []
    for i in range(S["n_rows"]):
        key = tuple(S["dirty"][c][i] for c in cols)
        if key not in memo:
            sc = ocp.exact_scores(T, par, choice, i)
            arr = np.array([sc[o] for o in S["choices"][choice]], dtype=np.float64)
            memo[key] = (arr, pe.normalise(sc) if np.isfinite(arr).any() else {})
        out.append(memo[key])
    return out


def compared_rows(S, pis, choice):
    """rows whose MAP option the literal decides: its two largest probabilities differ by more than twice the bound"""
    K = len(S["choices"][choice])
    out = []
    for i, pi in enumerate(pis):
        p = sorted(pi.values(), reverse=True) + [0.0, 0.0]
        if pi and p[0] - p[1] > 2 * bound(K):
            out.append(i)
    return out


# the two programs of the literal comparison with their parameters (the seeds satisfy compared_share >= 0.9 on the literal
# alone: tests/test_own_marginal_cpu.py)
def literal_cases():
    S3 = ocp.flat3()
    p3 = np.random.default_rng(31).dirichlet(np.ones(len(S3["choices"]["name"])))
    S2 = ocp.flat2b()
    rng = np.random.default_rng(32)
    p2 = {"city_p": rng.dirichlet(np.ones(len(S2["choices"]["city"]))), "cond_p": rng.dirichlet(np.ones(len(S2["choices"]["cond"])))}
    return {"flat3": (S3, {"p": p3}), "flat2b": (S2, p2)}


def compared_share(S, params):
    """share of (row, own choice) cells whose MAP option the literal decides"""
    hit = total = 0
    for choice in S["choices"]:
        pis = [pi for _, pi in exact_rows(S, params, choice)]
        hit += len(compared_rows(S, pis, choice))
        total += len(pis)
    return hit / float(total)
