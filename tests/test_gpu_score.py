"""Scoring new sequences against a fitted model from one k-mer table (kmg_scorer_*,
kmg_score.hip) against K[Q, T] . beta of the CPU oracle's exact integer Gram over [T; Q].

Tolerance (derived, not measured): tol_q = (N P + 4 k + P + 16) 2^-52 sum_t |beta_t| K^(q, t),
the (chain depth) u bound, doubled, of a sum whose elementary terms all enter with positive
integer multiplicities: N P list entries a table entry, 4 k butterfly additions, P windows a
query, 16 for the weights, the wave tree and the normalisation.  The butterfly takes t = 4
digits a launch, so k = 1 is less than a tile, k = 4, 12 whole tiles, k = 5, 9 leave a
one-digit last tile and k = 7 a three-digit one.
"""
import numpy as np
import pandas as pd
import pytest

import cpu_ref
import golden_io

pytestmark = pytest.mark.gpu

N, Q, LEN = 96, 17, 101
LD = np.longdouble


@pytest.fixture(scope="module")
def rows():
    """[T; Q]: mutated copies of four parents, so rows share windows."""
    rng = np.random.default_rng(20240)
    parents = rng.integers(0, 4, size=(4, LEN), dtype=np.uint8)
    codes = parents[rng.integers(0, 4, size=N + Q)]
    hit = rng.random(codes.shape) < 0.08
    codes = np.where(hit, rng.integers(0, 4, size=codes.shape, dtype=np.uint8), codes)
    beta = rng.standard_normal(N)
    return codes.astype(np.uint8), np.full(N + Q, LEN, dtype=np.int32), beta


def reference(codes, lens, beta, kind, k, m, normalize, nt):
    """f_ref (longdouble) and tol_q for the queries codes[nt:] against the rows codes[:nt]."""
    if kind == "SP":
        K = cpu_ref.spectrum_windows(codes, lens, k)
        P = int(lens.max()) - k + 1
    else:
        K = cpu_ref.mismatch_raw_windows(codes, lens, k, m)
        P = 101 - k + 1
    Kh = K.astype(LD)
    if normalize and K[0, 0] != 1:
        d = np.sqrt(np.diag(Kh))
        with np.errstate(invalid="ignore", divide="ignore"):
            Kh = Kh / np.outer(d, d)
    block = Kh[nt:, :nt]
    assert K[nt:, :nt].any()
    tol = (nt * P + 4 * k + P + 16) * 2.0 ** -52 * (block * np.abs(beta).astype(LD)).sum(axis=1)
    return block @ beta.astype(LD), tol


def params(kind, k, m=0, normalize=0):
    from kmgram import _lib as L, params as P
    if kind == "SP":
        return P.make(L.KMG_SPECTRUM, k=k, normalize=normalize)
    return P.make(L.KMG_MISMATCH, k=k, m=m, window=101, normalize=normalize)


def check_values(ctx, codes, lens, beta, kind, k, m, normalize, nt):
    sc = ctx.scorer(params(kind, k, m, normalize), codes[:nt], lens[:nt], beta)
    f = sc.score(codes[nt:], lens[nt:])
    sc.close()
    ref, tol = reference(codes, lens, beta, kind, k, m, normalize, nt)
    err = np.abs(f.astype(LD) - ref)
    print(kind, k, m, normalize, "max err / tol", float(np.nanmax(err / np.maximum(tol, 1e-300))))
    ok = np.isfinite(ref)
    assert np.array_equal(np.isnan(f), ~ok)  # 0 / 0 only where the reference has it
    assert (err[ok] <= tol[ok]).all()
    return f


@pytest.mark.parametrize("kind,k,m,normalize", [
    ("SP", 3, 0, 0), ("SP", 8, 0, 0), ("SP", 12, 0, 0), ("SP", 5, 0, 1), ("MM", 1, 1, 1), ("MM", 4, 1, 1),
    ("MM", 5, 2, 1), ("MM", 7, 1, 0), ("MM", 9, 1, 1), ("MM", 12, 1, 1)])
def test_values(ctx, rows, kind, k, m, normalize):
    codes, lens, beta = rows
    if kind == "SP":  # a non-ACGT symbol on either side, a row of 60 symbols, a query shorter than k
        codes, lens = codes.copy(), lens.copy()
        codes[3, 40] = codes[N + 2, 10] = 4
        lens[5] = 60
        lens[N + 4] = 2
        codes[5, 60:] = codes[N + 4, 2:] = 255
    f = check_values(ctx, codes, lens, beta, kind, k, m, normalize, N)
    if kind == "SP":  # no valid window: the bias alone, or the Gram epilogue's 0 / 0
        assert np.isnan(f[4]) if normalize else f[4] == 0.0


@pytest.mark.parametrize("tiny", [-1e-30, 1e-30, -1e-300])
def test_tiny_coefficient_beside_large_ones(ctx, rows, tiny):
    """A coefficient far below 2^-90 max|beta| contributes (nearly) nothing, whatever its sign."""
    codes, lens, beta = rows
    beta = beta.copy()
    beta[:8] = tiny
    check_values(ctx, codes, lens, beta, "SP", 8, 0, 0, N)


@pytest.mark.parametrize("kind,k,m,normalize", [("SP", 8, 0, 0), ("MM", 9, 1, 1)])
def test_reproducible_and_bias_once(ctx, rows, kind, k, m, normalize):
    codes, lens, beta = rows
    out = []
    for _ in range(2):
        sc = ctx.scorer(params(kind, k, m, normalize), codes[:N], lens[:N], beta)
        out.append((sc.score(codes[N:], lens[N:]), sc.score(codes[N:], lens[N:], bias=0.75)))
        sc.close()
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1].tobytes() == out[1][1].tobytes()
    assert np.array_equal(out[0][1], out[0][0] + 0.75) and out[0][0].any()


def test_through_a_learner(engine):
    from kmgram import encode as E
    from kmgram.learners import KRR
    codes, lens = golden_io.load_xtr0()
    seqs = E.decode(codes[:150], lens[:150])
    K = engine.mismatch(seqs, 5, 1)
    ID = np.arange(150)
    y = 2.0 * np.random.default_rng(5).integers(0, 2, size=150) - 1.0
    model = KRR(K, ID, lbda=0.1)
    model.fit(pd.DataFrame({"Id": ID[:120]}), pd.DataFrame({"Id": ID[:120], "Bound": y[:120]}))
    new = pd.DataFrame({"Id": ID[120:]})
    f_K = model.decision_function(new)
    sc = model.scorer(seqs, "MM_k5_m1")
    f = sc.decision_function(seqs[120:])
    P = 101 - 5 + 1
    tol = (len(model.a) * P + 4 * 5 + P + 16) * 2.0 ** -52 * (
        np.abs(model.a) @ K[np.ix_(model.idx_sv, ID[120:])])
    print("max err / tol", float(np.max(np.abs(f - f_K) / tol)))
    assert (np.abs(f - f_K) <= tol).all()
    sure = np.abs(f_K) > tol
    assert sure.any() and np.array_equal(sc.predict(seqs[120:])[sure], model.predict(new)[sure])


@pytest.mark.parametrize("case", ["sp_k13", "mm_m3", "wd", "method", "coef"])
def test_refusals(ctx, engine, rows, case):
    from kmgram import _lib as L, params as P
    codes, lens, beta = rows
    seqs = ["ACGT" * 26] * 3
    if case in ("method", "coef"):
        with pytest.raises(ValueError):
            if case == "method":
                engine.scorer("SS_l0.5_k3", seqs, np.ones(3))
            else:
                engine.scorer("SP_k4", seqs, np.ones(4))
    else:
        p = {"sp_k13": params("SP", 13), "mm_m3": params("MM", 5, 3, 1),
             "wd": P.make(L.KMG_WD, d=3)}[case]
        with pytest.raises(L.KmgUnsupported):
            ctx.scorer(p, codes[:N], lens[:N], beta)
    check_values(ctx, codes[N - 8:N + 4], lens[N - 8:N + 4], beta[:8], "SP", 3, 0, 0, 8)
