"""The position-weighted gkm kernel (kmg_gkm_cross_w, gram_gkmx_kernel<.., WT>):
Kw(x, y) = sum_{a,b} u_x[a] v_y[b] (h[ham(x_a, y_b)] [+ h[ham(x_a, rc(y_b))]]) against a brute-force
numpy restatement on strings in int64.  Every comparison is exact: the raw values are integers,
the normalised form one division by the weighted diagonals, float32 the float64 rounded once."""
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


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


@functools.lru_cache(maxsize=None)
def _rows(seed, lens):
    rng = np.random.default_rng([20147, seed])
    return tuple("".join("ACGT"[c] for c in rng.integers(0, 4, ln)) for ln in lens)


def _weights(seed, seqs, l):
    """Seeded uniform 0..255 a word, distinct a position; a few forced to 0 and to 255."""
    rng = np.random.default_rng([20148, seed])
    ws = [rng.integers(0, 256, max(0, len(s) - l + 1)).astype(np.uint8) for s in seqs]
    for w in ws:
        w[5::7] = 0
        w[3::11] = 255
        w[:1] |= 1  # (a row of one word keeps a non-zero diagonal)
    return ws


@functools.lru_cache(maxsize=None)
def _H(x, y, l, k, d, both):
    """int64 [windows of x, windows of y]: h[ham] (+ the reverse-complement term), 0 where either
    window holds a non-ACGT letter."""
    h = np.array([math.comb(l - m, k) if m <= d else 0 for m in range(l + 1)], dtype=np.int64)

    def words(s, f=lambda w: w):
        ok = np.array([set(s[a:a + l]) <= set("ACGT") for a in range(len(s) - l + 1)], dtype=bool)
        w = [f(s[a:a + l]) if o else "A" * l for a, o in enumerate(ok)]
        return np.frombuffer("".join(w).encode(), dtype=np.uint8).reshape(len(w), l), ok
    (u, uo), (v, vo) = words(x), words(y)
    H = h[(u[:, None, :] != v[None, :, :]).sum(-1)]
    if both:
        H = H + h[(u[:, None, :] != words(y, rc)[0][None, :, :]).sum(-1)]
    return H * np.outer(uo, vo)


def _ref(sa, wa, sb, wb, l, k, d, both):
    """(raw int64 Kw [na, nb], sqrt Kw(A_i, A_i), sqrt Kw(B_j, B_j)); w None is all ones."""
    def kw(x, u, y, v):
        H = _H(x, y, l, k, d, both)
        u = np.ones(H.shape[0], np.int64) if u is None else u[:H.shape[0]].astype(np.int64)
        v = np.ones(H.shape[1], np.int64) if v is None else v[:H.shape[1]].astype(np.int64)
        return int(u @ H @ v)
    wa, wb = wa or [None] * len(sa), wb or [None] * len(sb)
    K = np.array([[kw(x, u, y, v) for y, v in zip(sb, wb)] for x, u in zip(sa, wa)], dtype=np.int64)
    return (K, np.sqrt(np.array([kw(x, u, x, u) for x, u in zip(sa, wa)], dtype=np.float64)),
            np.sqrt(np.array([kw(y, v, y, v) for y, v in zip(sb, wb)], dtype=np.float64)))


def _check(engine, sa, wa, sb, wb, l, k, d, both):
    K, da, db = _ref(sa, wa, sb, wb, l, k, d, both)
    kw = dict(both_strands=both, weights_a=wa, weights_b=wb)
    raw = engine.gkm_cross(sa, sb, l, k, d, normalize=False, **kw)
    assert raw.dtype == np.float64 and np.array_equal(raw, K)
    # int32 where the documented bound strands W_a W_b P_a P_b h[0] allows it, refused elsewhere
    top = ((2 if both else 1) * (255 if wa else 1) * (255 if wb else 1) * math.comb(l, k)
           * max(len(s) - l + 1 for s in sa) * max(len(s) - l + 1 for s in sb))
    if top < 2 ** 31:
        raw = engine.gkm_cross(sa, sb, l, k, d, normalize=False, out_dtype=L.KMG_I32, **kw)
        assert raw.dtype == np.int32 and np.array_equal(raw, K)
    else:
        with pytest.raises(L.KmgError) as e:
            engine.gkm_cross(sa, sb, l, k, d, normalize=False, out_dtype=L.KMG_I32, **kw)
        assert e.value.status == L.KMG_EINVAL
    Kn = engine.gkm_cross(sa, sb, l, k, d, **kw)
    assert np.array_equal(Kn, K.astype(np.float64) / np.outer(da, db))
    assert np.array_equal(engine.gkm_cross(sa, sb, l, k, d, out_dtype=L.KMG_F32, **kw),
                          Kn.astype(np.float32))


def _edge_sets():
    sa = list(_rows(1, tuple([1, 31, 32, 33, 64, 65][i % 6] + 9 for i in range(17))))
    sb = list(_rows(2, tuple([33, 291][j % 2] + 9 for j in range(9))))
    sa[4] = sa[4][:36] + "N" + sa[4][37:]
    sb[1] = sb[1][:150] + "N" + sb[1][151:]
    return sa, sb


@gpu
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("na,nb", [(17, 9), (1, 9), (17, 1), (1, 1)])
def test_block_edges(engine, na, nb, both):
    """17 rows of 1, 31, 32, 33, 64, 65 words (row 4 with an N mid-row) against 9 rows of 33 and
    291 words (row 1 with an N; 291 is one block past the 256-word chunk, so the partials are
    flushed and started again across B chunks) at l = 10; 17 rows are three 8-row tiles."""
    sa, sb = _edge_sets()
    wa, wb = _weights(1, sa, 10), _weights(2, sb, 10)
    _check(engine, sa[:na], wa[:na], sb[:nb], wb[:nb], 10, 6, 3, both)


@gpu
@pytest.mark.parametrize("l,k,d", [(4, 2, 2), (8, 4, 3), (9, 5, 3), (16, 8, 3), (1, 1, 0)])
def test_word_lengths(engine, l, k, d):
    sa, sb = _rows(3, (40, 47, 70, 53, 66)), _rows(4, (70, 41, 58, 64, 45, 69, 50))
    _check(engine, sa, _weights(3, sa, l), sb, _weights(4, sb, l), l, k, d, True)


@gpu
def test_one_sided_and_trivial_weights(engine):
    sa, sb = _edge_sets()
    sa, sb = sa[:9], sb[:3]
    wa, wb = _weights(5, sa, 10), _weights(6, sb, 10)
    _check(engine, sa, wa, sb, None, 10, 6, 3, True)
    _check(engine, sa, None, sb, wb, 10, 6, 3, False)
    ones = lambda seqs: [np.ones(len(s), dtype=np.uint8) for s in seqs]  # noqa: E731
    for normalize in (False, True):
        assert np.array_equal(
            engine.gkm_cross(sa, sb, 10, 6, 3, normalize, both_strands=True,
                             weights_a=ones(sa), weights_b=ones(sb)),
            engine.gkm_cross(sa, sb, 10, 6, 3, normalize, both_strands=True))
    # 0/1 weights on B: the unweighted block of B with those words cut out of the sum
    keep = [(w & 1).astype(np.uint8) for w in wb]
    cut = np.array([[int(_H(x, y, 10, 6, 3, False)[:, m[:len(y) - 9] == 1].sum())
                     for y, m in zip(sb, keep)] for x in sa], dtype=np.int64)
    assert np.array_equal(engine.gkm_cross(sa, sb, 10, 6, 3, normalize=False, weights_b=keep), cut)


@gpu
def test_largest_partials(engine):
    """(AT)^n alternates two words of 16 letters, so with d = 0 a lane's B word matches 8 of its
    16 A words in all 8 blocks of a chunk: T = 8 * 255 * 12870 and uA * T > 2^32, the 64-bit
    flush.  The bound W_a W_b P_a P_b h[0] must stay below 2^53: 3265 words a row, (AT)^1640,
    are the most that 255 * 255 * C(16, 8) lets through ((AT)^2008 with its 4001 words has a bound of
    1.34e16 >= 2^53 although its value 6.70e15 is below, so it is refused like any row of its
    length); with both strands the bound doubles and the same call is refused."""
    s, l = ["AT" * 1640], 16
    w = [np.full(3265, 255, dtype=np.uint8)]
    K = engine.gkm_cross(s, s, l, 8, 0, normalize=False, weights_a=w, weights_b=w)
    assert K.dtype == np.float64 and K[0, 0] == float(65025 * (1633 ** 2 + 1632 ** 2) * 12870)
    assert 65025 * 3265 ** 2 * 12870 < 2 ** 53 <= 2 * 65025 * 3265 ** 2 * 12870
    big = ["AT" * 2008]
    for seqs, ww, kw, status in [
            (s, w, dict(both_strands=True), L.KMG_EUNSUPPORTED),
            (big, [np.full(4001, 255, dtype=np.uint8)], {}, L.KMG_EUNSUPPORTED),
            (s, w, dict(out_dtype=L.KMG_I32), L.KMG_EINVAL)]:
        with pytest.raises(L.KmgError) as e:
            engine.gkm_cross(seqs, seqs, l, 8, 0, normalize=False, weights_a=ww, weights_b=ww, **kw)
        assert e.value.status == status


@gpu
@pytest.mark.parametrize("kind,fields,dt,ldw,status", [
    (L.KMG_GKM, dict(k=10, g=4, m=3), L.KMG_F64, 91, L.KMG_EINVAL),  # 92 words a row
    (L.KMG_MISMATCH, dict(k=10, m=1), L.KMG_F64, 92, L.KMG_EUNSUPPORTED),
    (L.KMG_GKM, dict(k=10, g=4, m=3, normalize=1), L.KMG_I32, 92, L.KMG_EINVAL)])
def test_abi_refusals(ctx, kind, fields, dt, ldw, status):
    codes, lens = E.synthetic(3, 101, seed=1)
    out, w = np.zeros((3, 3), dtype=L.DTYPES[dt]), np.ones((3, 92), dtype=np.uint8)
    p = P.make(kind, **fields)
    assert ctx.lib.kmg_gkm_cross_w(ctx.handle, ctypes.byref(p), L.ptr(codes), L.ptr(lens), 3, 101,
                                   L.ptr(w), ldw, L.ptr(codes), L.ptr(lens), 3, 101, L.ptr(w), ldw,
                                   dt, L.ptr(out), 3) == status


@pytest.mark.parametrize("M,H", [(50, 50), (254, 5)])
@pytest.mark.parametrize("length,l", [(101, 10), (100, 11), (12, 12)])
def test_center_weights(length, l, M, H):
    w = P.gkm_center_weights(length, l, M, H)
    ref = [min(255, math.floor(M * math.pow(2.0, -abs(2 * a + l - length) / (2 * H))) + 1)
           for a in range(length - l + 1)]
    assert w.dtype == np.uint8 and w.tolist() == ref and w.tolist() == ref[::-1]
    centre = [a for a in range(length - l + 1) if 2 * a + l == length]
    assert all(w[a] == M + 1 == w.max() for a in centre) and w.max() <= M + 1


@pytest.mark.parametrize("wa,normalize", [
    ([np.ones(30, np.uint8)], False),            # 31 words need 31 entries
    ([np.full(31, 256)], False),                 # outside 0..255
    ([np.full(31, -1)], False),
    ([np.ones(31)], False),                      # not integers
    ([np.ones(31, np.uint8)] * 2, False),        # two rows for one sequence
    ([np.zeros(31, np.uint8)], True)])           # a zero diagonal under normalisation
def test_bad_weights_raise_before_any_device_work(wa, normalize):
    with pytest.raises(ValueError, match="gkm"):
        GramEngine(0).gkm_cross(["ACGT" * 10], ["ACGT" * 10], 10, 6, 3, normalize, weights_a=wa)
