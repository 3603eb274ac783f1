"""The gapped k-mer (gkm) kernel, K = sum_{a,b} h[ham(x_a, y_b)], h[m] = C(l - m, k) for
m <= d, against a brute-force numpy restatement of that formula.  Every comparison is exact:
the raw values are integers below 2^31, and the normalised form is K / outer(s, s) with
s = sqrt(diag K) and a unit diagonal, which is normalize_K bit for bit."""
import ctypes
import functools
import math

import numpy as np
import pytest

from kmgram import GramEngine
from kmgram import _lib as L
from kmgram import encode as E
from kmgram import params as P

gpu = pytest.mark.gpu
RNG_SEED = 20141
MIXES = ("short30", "ragged101", "ragged150")


@functools.lru_cache(maxsize=None)
def _seqs(mix, n=37, length=40):
    """n seeded rows.  Row 0 has the mix's greatest length, row 1 (30 letters or more) an N in
    its middle, row 2 exactly 10 letters (one word at l = 10)."""
    rng = np.random.default_rng([RNG_SEED, MIXES.index(mix) if mix in MIXES else length])
    top = {"short30": 30, "ragged101": 101, "ragged150": 150}.get(mix, length)
    lens = [top] * n if mix in ("short30", "fixed") else [top, top // 2] + list(rng.integers(12, top + 1, n - 2))
    rows = ["".join("ACGT"[c] for c in rng.integers(0, 4, ln)) for ln in lens]
    if mix != "fixed":
        rows[1] = rows[1][:len(rows[1]) // 2] + "N" + rows[1][len(rows[1]) // 2 + 1:]
        rows[2] = rows[2][:10]
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def _ref(seqs, l, k, d):
    """Raw int64 K of the formula: per pair of rows, the Hamming distances of all word pairs."""
    h = np.array([math.comb(l - m, k) if m <= d else 0 for m in range(l + 1)], dtype=np.int64)
    words = []
    for s in seqs:
        w = [s[a:a + l] for a in range(len(s) - l + 1) if set(s[a:a + l]) <= set("ACGT")]
        words.append(np.frombuffer("".join(w).encode(), dtype=np.uint8).reshape(len(w), l))
    K = np.zeros((len(seqs), len(seqs)), dtype=np.int64)
    for i, u in enumerate(words):
        for j in range(i, len(words)):
            K[i, j] = K[j, i] = h[(u[:, None, :] != words[j][None, :, :]).sum(-1)].sum()
    return K


def _normalised(K):
    s = np.sqrt(np.diag(K).astype(np.float64))
    Kn = K.astype(np.float64) / np.outer(s, s)
    np.fill_diagonal(Kn, 1.0)
    return Kn


@gpu
@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("n", [1, 16, 17, 37])
def test_tile_and_lane_edges(engine, n, mix):
    """pmax 21, 92 and 141 (1, 3 and 5 row words a lane; a column half that ends early), tiles
    of 1, 16, 16 + 1 and 2 * 16 + 5 rows; rows with an N and with a single word."""
    seqs = _seqs(mix)[:n]
    ref = _ref(_seqs(mix), 10, 6, 3)[:n, :n]
    raw = engine.gkm(seqs, 10, 6, 3, normalize=False, out_dtype=L.KMG_I32)
    assert raw.dtype == np.int32 and np.array_equal(raw, ref)
    assert np.array_equal(engine.gkm(seqs, 10, 6, 3), _normalised(ref))


@gpu
@pytest.mark.parametrize("l,k,d", [(4, 2, 2), (10, 6, 3), (10, 6, 4), (11, 7, 0), (16, 8, 3),
                                   (16, 16, 0), (1, 1, 0)])
def test_parameters(engine, l, k, d):
    """l = 16 is the unmasked 32-bit word; d < l - k truncates; float32 is the float64 result
    rounded once."""
    seqs = _seqs("fixed", 17, 40)
    ref = _ref(seqs, l, k, d)
    assert np.array_equal(engine.gkm(seqs, l, k, d, normalize=False, out_dtype=L.KMG_I32), ref)
    Kn = engine.gkm(seqs, l, k, d)
    assert np.array_equal(Kn, _normalised(ref))
    assert np.array_equal(engine.gkm(seqs, l, k, d, out_dtype=L.KMG_F32), Kn.astype(np.float32))
    if (l, k) == (10, 6) and d == 3:
        assert np.array_equal(engine.gkm(seqs, l, k), Kn)  # d=None is min(3, l - k)


@gpu
@pytest.mark.parametrize("l", [5, 8])
def test_spectrum_identity(engine, l):
    """g = 0, h = (1, 0, ...): the spectrum kernel of the same word length."""
    seqs = _seqs("ragged101")
    assert np.array_equal(engine.gkm(seqs, l, l, d=0, normalize=False, out_dtype=L.KMG_I32),
                          engine.spectrum(seqs, l, out_dtype=L.KMG_I32))


@gpu
@pytest.mark.parametrize("dt,norm", [(L.KMG_I32, False), (L.KMG_F64, True)])
def test_row_ranges_equal_symmetric_build(ctx, dt, norm):
    """kmg_gram_device: rows [0,5), [5,21), [21,37) (every tile computed, unaligned row0)
    against all 37 rows at once (upper block triangle, transposed stores)."""
    seqs = _seqs("ragged101")
    codes, lens = E.encode(seqs)
    n, ldc = codes.shape
    p = P.gkm(10, 6, 3, normalize=norm)
    d_codes, d_lens = ctx.dmalloc(codes.nbytes), ctx.dmalloc(lens.nbytes)
    d_K = ctx.dmalloc(n * n * 8)
    try:
        ctx.h2d(d_codes, codes)
        ctx.h2d(d_lens, lens)

        def rows(r0, r1):
            ctx.gram_device(p, d_codes, d_lens, n, ldc, r0, r1, dt, d_K, n)
            ctx.synchronize()
            return ctx.d2h(np.empty((r1 - r0, n), dtype=L.DTYPES[dt]), d_K)
        full = rows(0, n)
        parts = np.concatenate([rows(0, 5), rows(5, 21), rows(21, n)])
    finally:
        for q in (d_K, d_codes, d_lens):
            ctx.dfree(q)
    ref = _ref(seqs, 10, 6, 3)
    assert np.array_equal(full, _normalised(ref) if norm else ref)
    assert np.array_equal(parts, full)


@pytest.mark.parametrize("l,k,d", [(17, 6, 0), (10, 0, 0), (10, 11, 0), (10, 6, 5)])
def test_bad_parameters_raise_before_any_device_work(l, k, d):
    with pytest.raises(ValueError, match="gkm"):
        GramEngine(0).gkm(["ACGT" * 10], l, k, d)


def test_row_without_a_word_raises_under_normalisation():
    with pytest.raises(ValueError, match="sequence 1 "):
        GramEngine(0).gkm(["ACGT" * 10, "ACGTNACGT"], 5, 3)


@gpu
@pytest.mark.parametrize("fields,dt,status", [
    (dict(k=17, g=4, m=0), L.KMG_F64, L.KMG_EINVAL), (dict(k=10, g=10, m=0), L.KMG_F64, L.KMG_EINVAL),
    (dict(k=10, g=4, m=5), L.KMG_F64, L.KMG_EINVAL), (dict(k=10, g=4, m=-1), L.KMG_F64, L.KMG_EINVAL),
    (dict(k=10, g=4, m=3, normalize=1), L.KMG_I32, L.KMG_EINVAL),
    (dict(k=4, g=2, m=2), L.KMG_F64, L.KMG_EUNSUPPORTED)])  # 260 - 4 + 1 = 257 words a row
def test_abi_refusals(ctx, fields, dt, status):
    codes, lens = E.synthetic(3, 260, seed=1)
    out = np.zeros((3, 3), dtype=L.DTYPES[dt])
    p = P.make(L.KMG_GKM, **fields)
    assert ctx.lib.kmg_gram(ctx.handle, ctypes.byref(p), L.ptr(codes), L.ptr(lens), 3, 260, dt,
                            L.ptr(out), 3) == status
    assert b"gkm" in ctx.lib.kmg_last_error() or dt == L.KMG_I32


@gpu
def test_scorer_refuses_gkm(ctx):
    codes, lens = E.synthetic(3, 101, seed=1)
    with pytest.raises(L.KmgUnsupported, match="gkm"):
        ctx.scorer(P.gkm(10, 6, 3), codes, lens, np.ones(3))
