"""The rectangular gkm kernel (kmg_gkm_cross, kmg_gkmx.hip): Kx[i][j] = sum_{a,b} h[ham(A_i word
a, B_j word b)], h[m] = C(l - m, k) for m <= d, against a brute-force numpy restatement of that
formula which counts T^16.  Every comparison is exact: the raw values are integers, and the
normalised form is raw / outer(sqrt K(A_i, A_i), sqrt K(B_j, B_j)), one division, with float32
the float64 result rounded once."""
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


@functools.lru_cache(maxsize=None)
def _rows(seed, lens):
    rng = np.random.default_rng([20142, seed])
    return tuple("".join("ACGT"[c] for c in rng.integers(0, 4, ln)) for ln in lens)


@functools.lru_cache(maxsize=None)
def _ref(sa, sb, l, k, d):
    """(raw int64 [na, nb], sqrt K(A_i, A_i), sqrt K(B_j, B_j)) of the formula."""
    h = np.array([math.comb(l - m, k) if m <= d else 0 for m in range(l + 1)], dtype=np.int64)

    def words(s):
        w = [s[a:a + l] for a in range(len(s) - l + 1) if set(s[a:a + l]) <= set("ACGT")]
        return np.frombuffer("".join(w).encode(), dtype=np.uint8).reshape(len(w), l)

    def pair(u, v):
        return h[(u[:, None, :] != v[None, :, :]).sum(-1)].sum()
    wa, wb = [words(s) for s in sa], [words(s) for s in sb]
    K = np.array([[pair(u, v) for v in wb] for u in wa], dtype=np.int64)
    return (K, np.sqrt(np.array([pair(u, u) for u in wa], dtype=np.float64)),
            np.sqrt(np.array([pair(v, v) for v in wb], dtype=np.float64)))


def _check_all(engine, sa, sb, l, k, d, ref):
    K, da, db = ref
    raw = engine.gkm_cross(sa, sb, l, k, d, normalize=False, out_dtype=L.KMG_I32)
    assert raw.dtype == np.int32 and np.array_equal(raw, K)
    Kn = engine.gkm_cross(sa, sb, l, k, d)
    assert np.array_equal(Kn, K.astype(np.float64) / np.outer(da, db))
    assert np.array_equal(engine.gkm_cross(sa, sb, l, k, d, out_dtype=L.KMG_F32),
                          Kn.astype(np.float32))


def _edge_sets():
    """17 rows of 1, 31, 32, 33, 64, 65 words (row 4 with an N in its middle) against 9 rows of
    33 and 291 words (row 1 with an N) at l = 10: one more than the 16 x 8 tile each way."""
    sa = list(_rows(1, tuple([1, 31, 32, 33, 64, 65][i % 6] + 9 for i in range(17))))
    sb = list(_rows(2, tuple([33, 291][j % 2] + 9 for j in range(9))))
    sa[4] = sa[4][:36] + "N" + sa[4][37:]
    sb[1] = sb[1][:150] + "N" + sb[1][151:]
    return tuple(sa), tuple(sb)


@gpu
@pytest.mark.parametrize("na,nb", [(17, 9), (1, 9), (17, 1), (1, 1)])
def test_block_edges(engine, na, nb):
    sa, sb = _edge_sets()
    K, da, db = _ref(sa, sb, 10, 6, 3)
    _check_all(engine, sa[:na], sb[:nb], 10, 6, 3, (K[:na, :nb], da[:na], db[:nb]))


@gpu
@pytest.mark.parametrize("l,k,d", [(4, 2, 2), (8, 4, 3), (9, 5, 3), (16, 8, 3), (16, 16, 0),
                                   (1, 1, 0)])
def test_word_lengths(engine, l, k, d):
    """One MFMA step, exactly one, two, and full width, where T^16 (rows A[2] and B[3] hold
    T * 20) is a word like any other."""
    sa, sb = list(_rows(3, (40, 47, 70, 53, 66))), list(_rows(4, (70, 41, 58, 64, 45, 69, 50)))
    sa[2] = sa[2][:25] + "T" * 20 + sa[2][45:]
    sb[3] = sb[3][:7] + "T" * 20 + sb[3][27:]
    sa, sb = tuple(sa), tuple(sb)
    ref = _ref(sa, sb, l, k, d)
    assert l < 16 or ref[0][2, 3] >= 25 * math.comb(16, k)
    _check_all(engine, sa, sb, l, k, d, ref)


@gpu
def test_equals_the_square_path(engine):
    rng = np.random.default_rng(20143)
    s = list(_rows(5, tuple([101, 50] + list(rng.integers(12, 102, 19)))))
    s[1] = s[1][:25] + "N" + s[1][26:]
    assert np.array_equal(engine.gkm_cross(s, s, 10, 6, 3, normalize=False),
                          engine.gkm(s, 10, 6, 3, normalize=False))


@gpu
def test_lane_sums_flush_into_int64(engine):
    """4000 x 4000 poly-A words of 16 letters: 125 x 125 blocks x 16 adds of C(16, 8) a lane."""
    s = ["A" * 4015]
    K = engine.gkm_cross(s, s, 16, 8, 0, normalize=False)
    assert K.dtype == np.float64 and K[0, 0] == float(4000 ** 2 * 12870)
    with pytest.raises(L.KmgError) as e:
        engine.gkm_cross(s, s, 16, 8, 0, normalize=False, out_dtype=L.KMG_I32)
    assert e.value.status == L.KMG_EINVAL


@gpu
def test_device_form_equals_host_form(ctx):
    sa, sb = _edge_sets()
    (ca, la), (cb, lb) = E.encode(sa), E.encode(sb)
    p = P.gkm(10, 6, 3, normalize=True)
    host = ctx.gkm_cross(p, ca, la, cb, lb)
    bufs = [ctx.dmalloc(a.nbytes) for a in (ca, la, cb, lb, host)]
    try:
        for q, a in zip(bufs, (ca, la, cb, lb)):
            ctx.h2d(q, a)
        ctx.gkm_cross_device(p, bufs[0], bufs[1], len(la), ca.shape[1], bufs[2], bufs[3], len(lb),
                             cb.shape[1], L.KMG_F64, bufs[4], len(lb))
        ctx.synchronize()
        dev = ctx.d2h(np.empty_like(host), bufs[4])
    finally:
        for q in bufs:
            ctx.dfree(q)
    assert np.array_equal(dev, host)


@gpu
@pytest.mark.parametrize("kind,fields,dt,status", [
    (L.KMG_MISMATCH, dict(k=10, m=1), L.KMG_F64, L.KMG_EUNSUPPORTED),
    (L.KMG_GKM, dict(k=17, g=4, m=0), L.KMG_F64, L.KMG_EINVAL),
    (L.KMG_GKM, dict(k=10, g=4, m=3, normalize=1), L.KMG_I32, L.KMG_EINVAL)])
def test_abi_refusals(ctx, kind, fields, dt, status):
    codes, lens = E.synthetic(3, 101, seed=1)
    out = np.zeros((3, 3), dtype=L.DTYPES[dt])
    p = P.make(kind, **fields)
    assert ctx.lib.kmg_gkm_cross(ctx.handle, ctypes.byref(p), L.ptr(codes), L.ptr(lens), 3, 101,
                                 L.ptr(codes), L.ptr(lens), 3, 101, dt, L.ptr(out), 3) == status
    assert kind == L.KMG_GKM or b"gkm cross" in ctx.lib.kmg_last_error()


@pytest.mark.parametrize("l,k,d", [(17, 6, 0), (10, 0, 0), (10, 11, 0), (10, 6, 5)])
def test_bad_parameters_raise_before_any_device_work(l, k, d):
    with pytest.raises(ValueError, match="gkm"):
        GramEngine(0).gkm_cross(["ACGT" * 10], ["ACGT" * 10], l, k, d)


@pytest.mark.parametrize("sa,sb,where", [(["ACGT" * 10, "ACGTNACGT"], ["ACGT" * 10], "1 of side a"),
                                         (["ACGT" * 10], ["ACGTNACGT"], "0 of side b")])
def test_row_without_a_word_raises_under_normalisation(sa, sb, where):
    with pytest.raises(ValueError, match="sequence " + where):
        GramEngine(0).gkm_cross(sa, sb, 5, 3)
