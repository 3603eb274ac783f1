"""The gkm substitution map (kmg_gkm_scorer_mutate*, kmg_score.hip (5)):
out[q, i, b] = f_raw(q with letter b at i) - f_raw(q), bit for bit against the definition
restated on the host from the exported table, and in value against a brute force on strings
that never sees the table (the helpers of test_gpu_gkm_score.py).
"""
import math

import numpy as np
import pytest

from kmgram import _lib as L
from kmgram import encode as E
from test_gpu_gkm_score import LD, _data, _K

pytestmark = pytest.mark.gpu
KD = {1: (1, 0), 4: (2, 1), 5: (2, 3), 9: (5, 3), 12: (6, 4)}  # (k, d) of test_values


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _put(s, i, ch="N"):
    return s[:i] + ch + s[i + 1:]


def _scorer(engine, l, both, weighted, normalize=False):
    T, wt, coef, _, _ = _data(l)
    if normalize:
        coef = np.where(np.arange(24) == 3, 0.0, coef)  # the row without a word: K_tt = 0
    k, d = KD[l]
    return engine.gkm_scorer(T, coef, l, k, d, both_strands=both, weights=wt if weighted else None,
                             normalize=normalize), T, wt if weighted else [None] * 24, coef


def _definition(s, U, l, u):
    """The header's definition in plain float64: ascending a, one rounded product and one
    rounded add a word."""
    n, P = len(s), len(s) - l + 1
    out = np.zeros((n, 4))
    if P <= 0:
        return out
    let = np.array(["ACGT".find(c) for c in s])
    bad, let = let < 0, np.maximum(let, 0)
    code = sum(let[o:o + P].astype(np.int64) << (2 * (l - 1 - o)) for o in range(l))
    nbad = sum(bad[o:o + P].astype(int) for o in range(l))
    i = np.arange(n)
    for j in range(l):  # the word a = i - (l - 1) + j holds position i in its code bits 2j, 2j + 1
        a = i - (l - 1) + j
        ac = np.clip(a, 0, P - 1)
        ok = (a >= 0) & (a < P) & (nbad[ac] - bad == 0)
        for b in range(4):
            term = U[(code[ac] & ~(3 << (2 * j))) | (b << (2 * j))]
            if u is not None:
                term = u[ac].astype(np.float64) * term
            out[:, b] = np.where(ok, out[:, b] + term, out[:, b])
    return out - np.where(bad, 0.0, out[i, let])[:, None]


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("l", [1, 5, 12])
def test_bits_against_the_table(engine, l, weighted, both):
    """Rows without a word, of one word, of deltaSVM's 2l - 1 letters, on each side of the item
    sizes 8 / 16 / 32 (ldc 8 | 12, 16 | 20, 32 | 36) and of one item (64 | 65), and one of 2100
    letters; each alone (its own item size), all together, and the short ones together (item
    size 16, four items a workgroup, a count that is no multiple of four)."""
    rng = np.random.default_rng([77, l])
    Q = [_seq(rng, n) for n in (l - 1, l, 2 * l - 1, 8, 9, 16, 17, 32, 33, 64, 65, 2100)]
    Q[2] = _put(Q[2], l - 1)                          # all four values are sums there
    Q[8] = _put(_put(Q[8], 10), 10 + min(l - 1, 3))   # two Ns less than l apart
    Q[11] = _put(_put(Q[11], 318), 640)               # within l of a seam of the 64-letter items
    u = None
    if weighted:
        u = [rng.integers(1, 256, max(0, len(s) - l + 1)).astype(np.uint8) for s in Q]
        for w in u:
            w[1::5] = 0
    sc, _, _, _ = _scorer(engine, l, both, weighted)
    U = sc.lmer_weights()
    ref = [_definition(s, U, l, None if u is None else u[q]) for q, s in enumerate(Q)]
    short = [q for q, s in enumerate(Q) if len(s) <= 16]
    assert len(short) % 4
    for rows in [list(range(len(Q))), short] + [[q] for q in range(len(Q))]:
        out = sc.mutation_map([Q[q] for q in rows], None if u is None else [u[q] for q in rows])
        assert out.shape == (len(rows), max(len(Q[q]) for q in rows), 4)
        for r, q in enumerate(rows):
            n = len(Q[q])
            assert out[r, :n].tobytes() == ref[q].tobytes(), (rows, q)
            assert not out[r, n:].view(np.int64).any()  # +0.0, bit for bit
            own = [(i, "ACGT".find(c)) for i, c in enumerate(Q[q]) if c != "N"]
            assert not any(out[r, i, b] for i, b in own)
    assert ref[2][l - 1].all() and ref[11].any()
    sc.close()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("l", [4, 9])
def test_values_against_strings(engine, l, both, weighted, normalize):
    """Delta_ref = sum_t beta_t (K(q', x_t) - K(q, x_t)) in longdouble over the words that cover
    i (the others cancel), beta_t = coef_t / sqrt(K_tt) under normalisation, no query diagonal.
    tol = (4 l + 2 (d + 1) + l + 16) 2^-52 (A_mut + A_ref) + 2^-79 max |beta| (B_mut + B_ref):
    test_gpu_gkm_score.py's bound with at most l words a sum and two sums, A and B its
    absolute-value sums over the covering words of the mutant and of the original."""
    k, d = KD[l]
    c = [math.comb(l - m, k) for m in range(d + 1)]
    rng = np.random.default_rng([78, l])
    Q = [_seq(rng, 2 * l - 1), _put(_seq(rng, l + 20), l + 3), _seq(rng, l)]
    u = [rng.integers(0, 256, len(s) - l + 1).astype(np.uint8) if weighted else None for s in Q]
    sc, T, wt, coef = _scorer(engine, l, both, weighted, normalize)
    out = sc.mutation_map(Q, u if weighted else None)
    sc.close()
    beta = coef.astype(LD)
    if normalize:
        dt = np.sqrt(np.array([_K(t, w, t, w, l, c, both) for t, w in zip(T, wt)]))
        beta = np.where(coef != 0, beta / np.where(coef != 0, dt, 1), 0)
    worst = 0.0
    for q, s in enumerate(Q):
        P = len(s) - l + 1
        for i in range(len(s)):
            cover = (np.arange(P) >= i - l + 1) & (np.arange(P) <= i)
            uc = np.where(cover, 1 if u[q] is None else u[q], 0)
            row = lambda x, cc: np.array([_K(x, uc, t, w, l, cc, both) for t, w in zip(T, wt)])  # noqa: E731
            base, abase = row(s, c), row(s, np.abs(c))
            for b in range(4):
                mut = _put(s, i, "ACGT"[b])
                amut = row(mut, np.abs(c)) + abase
                tol = ((4 * l + 2 * (d + 1) + l + 16) * LD(2.0) ** -52 * (amut @ np.abs(beta))
                       + LD(2.0) ** -79 * np.abs(beta).max() * amut.sum())
                err = abs(LD(out[q, i, b]) - (row(mut, c) - base) @ beta)
                worst = max(worst, float(err / max(tol, np.finfo(LD).tiny)))
                assert err <= tol, (q, i, b)
    print("max err / tol", worst)
    assert out.any() and not out[2, l:].any()


def test_alone_batched_slabbed(engine, monkeypatch):
    rng = np.random.default_rng(79)
    Q = [_put(_seq(rng, n), n // 2) for n in (19, 101, 7, 64, 130, 33, 9, 70)]
    sc, _, _, _ = _scorer(engine, 9, True, False)
    together = sc.mutation_map(Q)
    monkeypatch.setenv("KMG_MUTATE_SLAB", "3")
    engine.ctx.reload_tuning()
    try:
        slabbed = sc.mutation_map(Q)
    finally:
        monkeypatch.delenv("KMG_MUTATE_SLAB")
        engine.ctx.reload_tuning()
    assert together.any() and together.tobytes() == slabbed.tobytes()
    for q, s in enumerate(Q):
        assert sc.mutation_map([s])[0].tobytes() == together[q, :len(s)].tobytes()
    sc.close()


@pytest.mark.parametrize("case", ["spectrum", "ld_out", "weights", "empty"])
def test_refusals(engine, case):
    codes, lens = E.encode(["ACGTTGCAAGCTTAGGCATC", "ACGTTGCAAGCT"])
    out = np.empty((2, 20, 4))
    sc, _, _, _ = _scorer(engine, 5, False, False)
    if case == "empty":
        assert sc.mutation_map([]).shape == (0, 0, 4)
    else:
        with pytest.raises(L.KmgError) as e:
            if case == "weights":  # 16 words in the longest row
                sc._s.mutate(codes, lens, np.ones((2, 15), dtype=np.uint8))
            else:
                sp = engine.scorer("SP_k5", ["ACGTTGCAAGCT"] * 2, np.ones(2)) if case == "spectrum" else sc
                L.check(engine.ctx.lib.kmg_gkm_scorer_mutate(
                    engine.ctx.handle, sp._s._h, L.ptr(codes), L.ptr(lens), 2, 20, None, 0, L.ptr(out),
                    20 if sp is not sc else 19))
        assert e.value.status == L.KMG_EINVAL
    sc.close()
