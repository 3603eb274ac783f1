"""The gkm mismatch profile and real-valued filters (kmg_gkm_profile, kmg_gkm_cross_f,
gram_gkmx_kernel<.., PF>): N_m(x, y) = #{(a, b) : ham(x_a, y_b) = m} (+ the same against
rc(y_b)) against a brute-force numpy Hamming histogram on strings in int64, and sum_m c[m] N_m
against the ascending-m float64 expression on that histogram.  Every comparison is exact."""
import ctypes
import functools

import numpy as np
import pytest

from kmgram import GramEngine
from kmgram import _lib as L
from kmgram import encode as E
from kmgram import params as P

gpu = pytest.mark.gpu


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _hist(x, y, l, both):
    """int64 [l + 1]: the pairs of all-ACGT windows of x and y by Hamming distance (both: and by
    the distance to the reverse complement of y's window)."""
    def words(s, f=lambda w: w):
        ok = np.array([set(s[a:a + l]) <= set("ACGT") for a in range(len(s) - l + 1)], dtype=bool)
        w = [f(s[a:a + l]) if o else "A" * l for a, o in enumerate(ok)]
        return np.frombuffer("".join(w).encode(), dtype=np.uint8).reshape(len(w), l), ok
    (u, uo), (v, vo) = words(x), words(y)
    ok = np.outer(uo, vo)
    n = np.bincount((u[:, None, :] != v[None, :, :]).sum(-1)[ok], minlength=l + 1)
    if both:
        n = n + np.bincount((u[:, None, :] != words(y, rc)[0][None, :, :]).sum(-1)[ok], minlength=l + 1)
    return n.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _sides(l):
    """17 and 9 seeded ragged rows (tile edges): shorter than l, exactly l, l + 32 letters (33
    words, a block edge), 300 letters (past the 256-word chunk), N in two of them, and the
    homopolymer words T^l and A^l."""
    rng = np.random.default_rng([20149, l])
    la = [l - 1, l, l + 32, 300] + [l + 3 + 7 * i for i in range(13)]
    lb = [300, l + 32, l, l - 1] + [l + 40 + 11 * j for j in range(5)]
    sa, sb = ([("".join("ACGT"[c] for c in rng.integers(0, 4, n))) for n in ln] for ln in (la, lb))
    sa[3] = sa[3][:140] + "N" + sa[3][141:]
    sb[5] = sb[5][:l + 2] + "N" + sb[5][l + 3:]
    sa[6], sb[6] = "T" * l + sa[6], sb[6] + "A" * (l + 1)
    return tuple(sa), tuple(sb)


@functools.lru_cache(maxsize=None)
def _ref(l, both):
    """(N [17, 9, l], N(A_i, A_i) [17, l], N(B_j, B_j) [9, l]) of _sides(l), bins 0 .. l - 1."""
    sa, sb = _sides(l)
    return (np.array([[_hist(x, y, l, both) for y in sb] for x in sa])[..., :l],
            np.array([_hist(x, x, l, both) for x in sa])[:, :l],
            np.array([_hist(y, y, l, both) for y in sb])[:, :l])


def _apply(c, N):
    """((c[0] N_0 + c[1] N_1) + c[2] N_2) + ...: separate float64 products and sums."""
    x = c[0] * N[..., 0].astype(np.float64)
    for m in range(1, len(c)):
        x = x + c[m] * N[..., m].astype(np.float64)
    return x


@gpu
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("l,d", [(4, 3), (10, 3), (16, 5), (9, 8)])
def test_profile(engine, l, d, both):
    """One and two MFMA steps; one, two and three passes of four bins; d = l - 1."""
    sa, sb = _sides(l)
    N = engine.gkm_profile(sa, sb, l, d, both_strands=both)
    assert N.dtype == np.int64 and N.shape == (17, 9, d + 1)
    assert np.array_equal(N, _ref(l, both)[0][..., :d + 1])


@gpu
@pytest.mark.parametrize("both", [False, True])
def test_field_overflow(engine, both):
    """66 blocks a row give 66^2 * 16 = 69 696 hits to one lane's bin-0 field: past 16 bits
    where a flush is missing or late."""
    sa, sb = ["A" * 2100], ["A" * 2100, "T" * 2100]
    ref = np.array([[_hist(sa[0], y, 4, both)[:4] for y in sb]])
    assert ref[0, 0, 0] == 2097 ** 2 and ref[0, 1, 0] == (2097 ** 2 if both else 0)
    assert np.array_equal(engine.gkm_profile(sa, sb, 4, 3, both_strands=both), ref)


@gpu
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("l,k,d", [(10, 6, 3), (16, 11, 5)])
def test_binomial_filter_equals_integer_kernel(engine, l, k, d, both):
    sa, sb = (tuple(s for s in side if len(s) >= l) for side in _sides(l))
    f = P.gkm_binomial_filter(l, k, d)
    for normalize in (False, True):
        K = engine.gkm_cross(sa, sb, l, None, normalize=normalize, both_strands=both, filter=f)
        assert K.dtype == np.float64 and np.array_equal(
            K, engine.gkm_cross(sa, sb, l, k, d, normalize=normalize, both_strands=both))


@gpu
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("l,d", [(10, 3), (16, 5), (9, 8)])  # fused; two and three passes + filter kernel
def test_real_filter(engine, l, d, both):
    rng = np.random.default_rng([20150, l])
    c = np.abs(rng.normal(size=d + 1))
    c[0], c[1], c[2] = 3.0 + c[0], 0.0, -c[2] / 64
    N, Na, Nb = (r[..., :d + 1] for r in _ref(l, both))
    keep_a, keep_b = (np.array([len(s) >= l for s in side]) for side in _sides(l))
    xa, xb = _apply(c, Na)[keep_a], _apply(c, Nb)[keep_b]
    assert (xa > 0).all() and (xb > 0).all()  # the reference's own diagonals: the filter's choice
    sa, sb = _sides(l)
    kw = dict(normalize=False, both_strands=both, filter=c)
    raw = engine.gkm_cross(sa, sb, l, **kw)
    assert raw.dtype == np.float64 and np.array_equal(raw, _apply(c, N))
    assert np.array_equal(engine.gkm_cross(sa, sb, l, out_dtype=L.KMG_F32, **kw), raw.astype(np.float32))
    sa, sb = (tuple(s for s in side if len(s) >= l) for side in (sa, sb))
    Kn = engine.gkm_cross(sa, sb, l, both_strands=both, filter=c)
    assert np.array_equal(Kn, _apply(c, N)[keep_a][:, keep_b] / np.outer(np.sqrt(xa), np.sqrt(xb)))
    assert np.array_equal(engine.gkm_cross(sa, sb, l, both_strands=both, filter=c, out_dtype=L.KMG_F32),
                          Kn.astype(np.float32))


@gpu
def test_row_slabs_of_the_workspace(ctx, tune):
    """A workspace of one 16-row tile: the 17 rows go through two slabs, normalised."""
    l, d = 16, 5
    sb, sa = (tuple(s for s in side if len(s) >= l) for side in _sides(l))
    sa = (sa * 3)[:17]
    c = np.array([3.5, 0.0, -0.015625, 0.75, 1.25, 0.3])
    (ca, la), (cb, lb) = E.encode(sa), E.encode(sb)
    p = P.gkm_profile(l, d, normalize=True)
    whole = ctx.gkm_cross(p, ca, la, cb, lb, filter=c)
    tune(KMG_GKM_PROF_WS=0)
    assert not np.isnan(whole).any() and np.array_equal(ctx.gkm_cross(p, ca, la, cb, lb, filter=c), whole)
    N = ctx.gkm_profile(p, ca, la, cb, lb)
    Na, Nb = (np.array([_hist(x, x, l, False)[:d + 1] for x in s]) for s in (sa, sb))
    assert np.array_equal(whole, _apply(c, N) / np.outer(np.sqrt(_apply(c, Na)), np.sqrt(_apply(c, Nb))))


def _cross_f(ctx, p, n, ldc, bufs, nfilter, dt):
    f = np.ones(16)
    return ctx.lib.kmg_gkm_cross_f_device(ctx.handle, ctypes.byref(p), bufs, bufs, n, ldc, bufs, bufs,
                                          n, ldc, L.ptr(f), nfilter, dt, bufs, n)


@gpu
@pytest.mark.parametrize("fields,nfilter,dt,ldc,status", [
    (dict(k=10, g=4, m=3), 3, L.KMG_F64, 101, L.KMG_EINVAL),           # nfilter != d + 1
    (dict(k=10, g=4, m=3), 5, L.KMG_F64, 101, L.KMG_EINVAL),
    (dict(k=10, g=10, m=10), 11, L.KMG_F64, 101, L.KMG_EINVAL),        # d > l - 1
    (dict(k=10, g=4, m=3), 4, L.KMG_I32, 101, L.KMG_EINVAL),
    # strands P_a P_b >= 2^53 is refused before anything is read: no buffer stands behind these
    (dict(k=10, g=4, m=3), 4, L.KMG_F64, 1 << 27, L.KMG_EUNSUPPORTED),
    (dict(k=10, g=4, m=3, strands=2), 4, L.KMG_F64, 70_000_000, L.KMG_EUNSUPPORTED),
    (dict(k=10, g=4, m=3), 4, L.KMG_F64, 70_000_000, L.KMG_EINVAL)])   # in bounds: "NULL buffer"
def test_abi_refusals(ctx, fields, nfilter, dt, ldc, status):
    assert _cross_f(ctx, P.make(L.KMG_GKM, **fields), 1, ldc, None, nfilter, dt) == status


@gpu
def test_other_kinds_weights_and_empty_sides(ctx, engine):
    p = P.make(L.KMG_MISMATCH, k=10, m=1)
    assert _cross_f(ctx, p, 1, 101, None, 2, L.KMG_F64) == L.KMG_EUNSUPPORTED
    assert ctx.lib.kmg_gkm_profile_device(ctx.handle, ctypes.byref(p), None, None, 1, 101, None, None,
                                          1, 101, None, 1) == L.KMG_EUNSUPPORTED
    codes, lens = np.zeros((1, 12), np.uint8), np.full(1, 12, np.int32)
    with pytest.raises(L.KmgUnsupported):
        ctx.gkm_cross(P.gkm_profile(10, 1), codes, lens, codes, lens, filter=np.ones(2),
                      weights_a=np.ones((1, 3), np.uint8))
    # an empty side: KMG_OK, nothing written, no buffer read
    p = P.gkm_profile(10, 3)
    assert _cross_f(ctx, p, 0, 101, None, 4, L.KMG_F64) == L.KMG_OK
    assert ctx.lib.kmg_gkm_profile_device(ctx.handle, ctypes.byref(p), None, None, 0, 101, None, None,
                                          3, 101, None, 3) == L.KMG_OK
    assert engine.gkm_profile([], ["ACGT" * 5], 10, 3).shape == (0, 1, 4)
    assert engine.gkm_cross(["ACGT" * 5], [], 10, filter=np.ones(4)).shape == (1, 0)


def test_binomial_filter():
    f = P.gkm_binomial_filter(10, 6, 3)
    assert f.dtype == np.float64 and f.tolist() == [210.0, 84.0, 28.0, 7.0]
    assert P.gkm_binomial_filter(16, 8, 0).tolist() == [12870.0]
    assert f.tolist() == [float(h) for h in P.gkm_weights(10, 6, 3)[:4]]
    with pytest.raises(ValueError, match="gkm"):
        P.gkm_binomial_filter(10, 6, 5)


@pytest.mark.parametrize("call", [
    lambda e, s: e.gkm_cross(s, s, 10, filter=np.ones(4), weights_a=[np.ones(31, np.uint8)]),
    lambda e, s: e.gkm_cross(s, s, 10, filter=np.ones(11)),             # d = 10 > l - 1
    lambda e, s: e.gkm_cross(s, s, 10, filter=np.ones((2, 2))),
    lambda e, s: e.gkm_cross(s, s, 10, d=2, filter=np.ones(4)),         # d disagrees with the filter
    lambda e, s: e.gkm_cross(s, s, 10, 6, filter=np.ones(6)),           # d = 5 > l - k
    lambda e, s: e.gkm_cross(s, s, 10, filter=np.ones(4), out_dtype=L.KMG_I32),
    lambda e, s: e.gkm_cross(s, s, 10),                                 # neither k nor a filter
    lambda e, s: e.gkm_profile(s, s, 10, 10),
    lambda e, s: e.gkm_profile(s, s, 17, 3)])
def test_bad_arguments_raise_before_any_device_work(call):
    with pytest.raises(ValueError, match="gkm"):
        call(GramEngine(0), ["ACGT" * 10])
