"""The gkm table scorer (kmg_gkm_scorer_*, kmg_score.hip (4)): f(q) = sum_t beta_t K(q, x_t) + b
from one table of 4^l l-mer weights, against a brute-force restatement on strings summed in
np.longdouble:  K(q, x) = sum_{a,b} u_a w_b sum_strands c[ham(q_a, x_b)].

Tolerance (derived, not measured), with A_q = sum_t |beta_t| sum_{a,b} u_a w_b sum_strands |c[ham]|
(divided by sqrt(K_qq), and beta_t = coef_t / sqrt(K_tt), under normalisation):
  tol_q = (4 l + 2 (d + 1) + P_q + 16) 2^-52 A_q + 2^-79 max_t |beta_t| B_q
the (chain depth) u bound, doubled, of a sum whose elementary terms beta_t w_b c[m] enter with
the multiplicities u_a: the table entry V[v] is an exact integer sum rounded once (1), the
butterfly adds 4 l times, the filter takes d + 1 products and d sums, a query adds its P_q
words (product and sum a word are inside P_q + 16 with the lane tree, the two roundings of
beta_t = coef_t / sqrt(K_tt) and the final division and bias).  The second term is the fixed
point: beta_t is cut to 80 fraction bits below 2^E, max |beta| >= 2^(E - 1), so each beta_t is
off by less than 2^(E - 80) <= 2^-79 max |beta|, times B_q = A_q with every |beta_t| = 1.
Against the Gram route the float64 block and its product with coef add (N + 4) 2^-53 A_q.
Under normalisation the training row without a word carries coef 0: its kernel row is 0 / 0.
"""
import functools
import math

import numpy as np
import pytest

from kmgram import _lib as L

pytestmark = pytest.mark.gpu
LD = np.longdouble
RC = str.maketrans("ACGT", "TGCA")
FILTER = (1.5, -0.75, 0.5, -0.25)


@functools.lru_cache(maxsize=None)
def _data(l):
    """24 training rows (row 3 shorter than l, row 5 with an N, row 7 of 300 letters), their
    weights and coef; 9 queries: 3 words (fewer than the 8 lanes of the narrowest form), 40
    and 150 words (16 and 64 lanes), 1100 words (the workgroup-wide form), one without a valid
    word, one with an N, one cut out of training row 7; and the queries' weights."""
    rng = np.random.default_rng([20150, l])
    seq = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))  # noqa: E731
    T = [seq(l + 20 + 3 * i) for i in range(24)]
    T[3], T[7] = T[3][:l - 1], seq(300)
    T[5] = T[5][:l + 3] + "N" + T[5][l + 4:]
    Q = [seq(l + 2), seq(l + 39), seq(l + 149), seq(l + 1099), "N" * (l + 5),
         seq(l + 60), T[7][40:l + 90], seq(l + 7), T[2][::-1].translate(RC)]
    Q[5] = Q[5][:30] + "N" + Q[5][31:]
    wts = lambda S: [rng.integers(0, 256, max(0, len(s) - l + 1)).astype(np.uint8) for s in S]  # noqa: E731
    return T, wts(T), rng.standard_normal(24), Q, wts(Q)


@functools.lru_cache(maxsize=None)
def _ham(x, y, l):
    """int [words of x, words of y]: Hamming distances, l + 1 where a word holds a non-ACGT."""
    def words(s):
        n = max(0, len(s) - l + 1)
        ok = np.array([set(s[a:a + l]) <= set("ACGT") for a in range(n)], dtype=bool)
        return np.frombuffer("".join(s[a:a + l] for a in range(n)).encode(), np.uint8).reshape(n, l), ok
    (u, uo), (v, vo) = words(x), words(y)
    return np.where(np.outer(uo, vo), (u[:, None, :] != v[None, :, :]).sum(-1), l + 1)


def _K(x, u, y, v, l, c, both):
    """longdouble sum_{a,b} u_a v_b sum_strands c[ham]; u, v None: ones."""
    cp = np.zeros(l + 2, dtype=LD)
    cp[:len(c)] = c
    H = cp[_ham(x, y, l)]
    if both:  # word b of y reverse-complemented is word (last - b) of rc(y)
        H = H + cp[_ham(x, y[::-1].translate(RC), l)[:, ::-1]]
    u = np.ones(H.shape[0], LD) if u is None else u.astype(LD)
    v = np.ones(H.shape[1], LD) if v is None else v.astype(LD)
    return u @ H @ v


def _reference(Q, uq, T, wt, coef, l, c, both, normalize):
    """(f_ref, tol_q, A_q) in longdouble for the queries Q against the model (T, wt, coef)."""
    uq, wt = uq or [None] * len(Q), wt or [None] * len(T)
    ca = np.abs(np.asarray(c, dtype=np.float64))
    K = np.array([[_K(q, u, t, w, l, c, both) for t, w in zip(T, wt)] for q, u in zip(Q, uq)])
    Ka = np.array([[_K(q, u, t, w, l, ca, both) for t, w in zip(T, wt)] for q, u in zip(Q, uq)])
    beta, dq = coef.astype(LD), np.ones(len(Q), LD)
    if normalize:
        dt = np.sqrt(np.array([_K(t, w, t, w, l, c, both) for t, w in zip(T, wt)]))
        beta = np.where(coef != 0, beta / np.where(coef != 0, dt, 1), 0)
        dq = np.sqrt(np.array([_K(q, u, q, u, l, c, both) for q, u in zip(Q, uq)]))
    Pq = np.array([max(0, len(q) - l + 1) for q in Q])
    with np.errstate(invalid="ignore", divide="ignore"):
        A = (Ka @ np.abs(beta)) / dq
        tol = ((4 * l + 2 * len(c) + Pq + 16) * LD(2.0) ** -52 * A
               + LD(2.0) ** -79 * np.abs(beta).max() * Ka.sum(axis=1) / dq)
        return (K @ beta) / dq, tol, A


def _close(f, ref, tol, what):
    err = np.abs(f.astype(LD) - ref)
    ok = np.isfinite(ref)
    print(what, "max err / tol", float(np.max(err[ok] / np.maximum(tol[ok], np.finfo(LD).tiny), initial=0)))
    assert np.array_equal(np.isnan(f), ~ok)  # 0 / 0 exactly where the reference has it
    assert (err[ok] <= tol[ok]).all()


def _check(engine, l, k, c, both, normalize, weighted):
    T, wt, coef, Q, uq = _data(l)
    wt, uq = (wt, uq) if weighted else (None, None)
    if normalize:
        coef = np.where(np.arange(24) == 3, 0.0, coef)
    sc = engine.gkm_scorer(T, coef, l, k, len(c) - 1, both_strands=both, weights=wt,
                           filter=None if k else c, normalize=normalize)
    ref, tol, _ = _reference(Q, uq, T, wt, coef, l, c, both, normalize)
    f = sc.score(Q, weights=uq)
    _close(f, ref, tol, "all")
    assert np.isnan(f[4]) if normalize else f[4] == 0.0  # no valid word
    alone = np.array([sc.score([q], weights=None if uq is None else [uq[i]])[0] for i, q in enumerate(Q)])
    _close(alone, ref, tol, "alone")  # every row at the lanes of its own length
    sc.close()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("l,k,d", [(1, 1, 0), (4, 2, 1), (5, 2, 3), (7, 3, 4), (9, 5, 3), (12, 6, 4)])
def test_values(engine, l, k, d, both, normalize, weighted):
    _check(engine, l, k, [math.comb(l - m, k) for m in range(d + 1)], both, normalize, weighted)


@pytest.mark.parametrize("l,both,normalize,weighted", [(7, True, False, False), (9, False, False, True),
                                                        (5, True, True, False)])
def test_filter(engine, l, both, normalize, weighted):
    """A real filter with mixed signs; with position weights too (raw), which no block serves;
    normalised with a positive filter of five bins (the diagonals through the stored profile)."""
    _check(engine, l, None, [2.0, 1.0, 0.5, 0.25, 0.125] if normalize else FILTER, both, normalize, weighted)


@pytest.mark.parametrize("both", [False, True])
def test_lmer_weights(engine, both):
    """All 256 entries at l = 4: the table entry of z is the raw score of the one-word row z."""
    T, wt, coef, _, _ = _data(4)
    sc = engine.gkm_scorer(T, coef, 4, 2, 2, both_strands=both, weights=wt, normalize=False)
    U = sc.lmer_weights()
    sc.close()
    Z = ["".join("ACGT"[(z >> (2 * (3 - i))) & 3] for i in range(4)) for z in range(256)]
    ref, tol, _ = _reference(Z, None, T, wt, coef, 4, [6, 3, 1], both, False)
    _close(U, ref, tol, "table")
    if both:
        rcz = [Z.index(z[::-1].translate(RC)) for z in Z]
        assert U.tobytes() == U[rcz].tobytes()


@pytest.mark.parametrize("both,weighted", [(False, False), (True, True)])
def test_agrees_with_the_gram_route(engine, both, weighted):
    T, wt, coef, Q, uq = _data(9)
    T, wt, coef, Q, uq = T[4:], wt[4:], coef[4:], Q[:3] + Q[5:], uq[:3] + uq[5:]  # rows with a word
    wt, uq = (wt, uq) if weighted else (None, None)
    sc = engine.gkm_scorer(T, coef, 9, 5, 3, both_strands=both, weights=wt)
    f = sc.score(Q, weights=uq)
    sc.close()
    g = engine.gkm_cross(Q, T, 9, 5, 3, both_strands=both, weights_a=uq, weights_b=wt) @ coef
    _, tol, A = _reference(Q, uq, T, wt, coef, 9, [126, 56, 21, 6], both, True)
    assert (np.abs(f.astype(LD) - g) <= tol + (len(T) + 4) * LD(2.0) ** -53 * A).all()


@pytest.mark.parametrize("l,train", [(9, None), (3, ["A" * 40] * 30), (6, ["A" * 130] * 300)])
def test_reproducible_and_bias_once(engine, l, train):
    """Two builds from the same inputs: the same bytes.  Rows of A...A put every training word
    on one key of the workgroup-private table (l = 6: several workgroups flush it)."""
    T, _, coef, Q, _ = _data(l)
    if train:
        T, coef = train, np.random.default_rng(7).standard_normal(len(train))
        Q = Q + ["A" * 20]
    out = []
    for _ in range(2):
        sc = engine.gkm_scorer(T, coef, l, (l + 1) // 2, 1, both_strands=True, normalize=False)
        out.append((sc.lmer_weights(), sc.score(Q), sc.score(Q, bias=0.75)))
        sc.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(out[0][2], out[0][1] + 0.75) and out[0][1].any()
    if train:
        ref, tol, _ = _reference(Q, None, T, None, coef, l, [math.comb(l - m, (l + 1) // 2) for m in (0, 1)],
                                 True, False)
        _close(out[0][1], ref, tol, "one key")


@pytest.mark.parametrize("case", ["l13", "d5", "filter6", "norm_w_f", "coef"])
def test_refusals(engine, case):
    T = ["ACGTTGCAAGCTTAGGCATC" * 2] * 3
    w = [np.ones(40, dtype=np.uint8)] * 3
    args, kw = {"l13": ((13, 7, 3), {}), "d5": ((12, 6, 5), {}),
                "filter6": ((8,), dict(filter=[1.0] * 6)),
                "norm_w_f": ((8,), dict(filter=[1.0, 0.5], weights=w, normalize=True)),
                "coef": ((8, 4, 2), {})}[case]
    coef = np.array([1.0, np.inf if case == "coef" else 2.0, 3.0])
    with pytest.raises(L.KmgError) as e:
        engine.gkm_scorer(T, coef, *args, **kw)
    assert e.value.status == (L.KMG_EINVAL if case == "coef" else L.KMG_EUNSUPPORTED)
    assert isinstance(e.value, L.KmgUnsupported) == (case != "coef")
