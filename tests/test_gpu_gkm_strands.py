"""Both strands in the gkm kernels (strands = 2): K2(x, y) = K(x, y) + K(x, rc(y)) against a
brute-force numpy restatement on strings, the gkm formula applied to y and to the reversed and
complemented y, added in int64.  Every comparison is exact: the raw values are integers, the
normalised form one division by the both-strands diagonals, float32 the float64 rounded once."""
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
    rng = np.random.default_rng([20144, seed])
    return tuple("".join("ACGT"[c] for c in rng.integers(0, 4, ln)) for ln in lens)


@functools.lru_cache(maxsize=None)
def _ref(sa, sb, l, k, d):
    """(raw int64 K2 [na, nb], sqrt K2(A_i, A_i), sqrt K2(B_j, B_j)) of the formula."""
    h = np.array([math.comb(l - m, k) if m <= d else 0 for m in range(l + 1)], dtype=np.int64)

    def words(s):
        w = [s[a:a + l] for a in range(len(s) - l + 1) if set(s[a:a + l]) <= set("ACGT")]
        return np.frombuffer("".join(w).encode(), dtype=np.uint8).reshape(len(w), l)

    def pair(x, y):
        u = words(x)
        return sum(int(h[(u[:, None, :] != v[None, :, :]).sum(-1)].sum())
                   for v in (words(y), words(rc(y))))
    K = np.array([[pair(x, y) for y in sb] for x in sa], dtype=np.int64)
    return (K, np.sqrt(np.array([pair(x, x) for x in sa], dtype=np.float64)),
            np.sqrt(np.array([pair(y, y) for y in sb], dtype=np.float64)))


def _check_cross(engine, sa, sb, l, k, d, ref):
    K, da, db = ref
    raw = engine.gkm_cross(sa, sb, l, k, d, normalize=False, out_dtype=L.KMG_I32, both_strands=True)
    assert raw.dtype == np.int32 and np.array_equal(raw, K)
    Kn = engine.gkm_cross(sa, sb, l, k, d, both_strands=True)
    assert np.array_equal(Kn, K.astype(np.float64) / np.outer(da, db))
    assert np.array_equal(engine.gkm_cross(sa, sb, l, k, d, out_dtype=L.KMG_F32, both_strands=True),
                          Kn.astype(np.float32))


@gpu
@pytest.mark.parametrize("na,nb", [(17, 9), (1, 9), (17, 1), (1, 1)])
def test_block_edges(engine, na, nb):
    """17 rows of 1, 31, 32, 33, 64, 65 words (row 4 with an N mid-row) against 9 rows of 33 and
    291 words (row 1 with an N; 291 is one block past the 256-word chunk) at l = 10."""
    sa = list(_rows(1, tuple([1, 31, 32, 33, 64, 65][i % 6] + 9 for i in range(17))))
    sb = list(_rows(2, tuple([33, 291][j % 2] + 9 for j in range(9))))
    sa[4] = sa[4][:36] + "N" + sa[4][37:]
    sb[1] = sb[1][:150] + "N" + sb[1][151:]
    K, da, db = _ref(tuple(sa), tuple(sb), 10, 6, 3)
    _check_cross(engine, sa[:na], sb[:nb], 10, 6, 3, (K[:na, :nb], da[:na], db[:nb]))


@gpu
@pytest.mark.parametrize("l,k,d", [(4, 2, 2), (8, 4, 3), (9, 5, 3), (16, 8, 3), (16, 16, 0),
                                   (1, 1, 0)])
def test_word_lengths(engine, l, k, d):
    """A[2] holds T * 20 and B[3] holds A * 20: at l = 16 the reverse complement of A^16 is T^16,
    a word like any other here."""
    sa, sb = list(_rows(3, (40, 47, 70, 53, 66))), list(_rows(4, (70, 41, 58, 64, 45, 69, 50)))
    sa[2] = sa[2][:25] + "T" * 20 + sa[2][45:]
    sb[3] = sb[3][:7] + "A" * 20 + sb[3][27:]
    ref = _ref(tuple(sa), tuple(sb), l, k, d)
    assert l < 16 or ref[0][2, 3] >= 25 * math.comb(16, k)
    _check_cross(engine, sa, sb, l, k, d, ref)


@gpu
def test_sum_of_the_single_strand_blocks(engine):
    """K2(A, B) = K(A, B) + K(A, rc(B)); B[2] = s + rc(s) is its own reverse complement, so its
    column is twice the single-strand one."""
    sa, sb = _rows(5, (101, 64, 30, 77, 45)), list(_rows(6, (90, 33, 40, 101)))
    sb[2] = sb[2] + rc(sb[2])
    one = engine.gkm_cross(sa, sb, 10, 6, 3, normalize=False)
    both = engine.gkm_cross(sa, sb, 10, 6, 3, normalize=False, both_strands=True)
    other = engine.gkm_cross(sa, [rc(b) for b in sb], 10, 6, 3, normalize=False)
    assert np.array_equal(both, one + other)
    assert np.array_equal(both[:, 2], 2 * one[:, 2]) and one[:, 2].min() > 0


@gpu
def test_lane_sums_flush_into_int64_with_both_sets(engine):
    """The 4001 words of (AT)^2008 alternate two reverse-palindromic words of 16 letters."""
    s = ["AT" * 2008]
    K = engine.gkm_cross(s, s, 16, 8, 0, normalize=False, both_strands=True)
    assert K.dtype == np.float64 and K[0, 0] == float(2 * (2001 ** 2 + 2000 ** 2) * 12870)
    with pytest.raises(L.KmgError) as e:
        engine.gkm_cross(s, s, 16, 8, 0, normalize=False, out_dtype=L.KMG_I32, both_strands=True)
    assert e.value.status == L.KMG_EINVAL


@gpu
def test_bounds_count_both_strands(engine):
    """300 words a row: 300^2 C(16, 8) < 2^31 <= 2 * 300^2 C(16, 8)."""
    s = _rows(7, (315,))
    assert engine.gkm_cross(s, s, 16, 8, 0, normalize=False, out_dtype=L.KMG_I32).dtype == np.int32
    with pytest.raises(L.KmgError) as e:
        engine.gkm_cross(s, s, 16, 8, 0, normalize=False, out_dtype=L.KMG_I32, both_strands=True)
    assert e.value.status == L.KMG_EINVAL


@gpu
@pytest.mark.parametrize("l,k,d,n", [(10, 6, 3, 33), (15, 8, 3, 9)])
def test_square_path(engine, l, k, d, n):
    """Ragged rows of l + 2 .. 101 letters, row 1 with an N: SYM, then rows [5, min(21, n))."""
    lens = np.random.default_rng(l).integers(l + 2, 102, n - 2)
    s = list(_rows(8, tuple([101, 50] + list(lens))))
    s[1] = s[1][:25] + "N" + s[1][26:]
    K = _ref(tuple(s), tuple(s), l, k, d)[0]
    raw = engine.gkm(s, l, k, d, normalize=False, out_dtype=L.KMG_I32, both_strands=True)
    assert np.array_equal(raw, K)
    assert np.array_equal(raw, engine.gkm_cross(s, s, l, k, d, normalize=False, both_strands=True))
    sq = np.sqrt(np.diag(K).astype(np.float64))
    Kn = K.astype(np.float64) / np.outer(sq, sq)
    np.fill_diagonal(Kn, 1.0)
    assert np.array_equal(engine.gkm(s, l, k, d, both_strands=True), Kn)

    ctx, (codes, lens), r0, r1 = engine.ctx, E.encode(s), 5, min(21, n)
    part = np.empty((r1 - r0, n), dtype=np.int32)
    bufs = [ctx.dmalloc(a.nbytes) for a in (codes, lens, part)]
    try:
        ctx.h2d(bufs[0], codes)
        ctx.h2d(bufs[1], lens)
        ctx.gram_device(P.gkm(l, k, d, False, True), bufs[0], bufs[1], n, codes.shape[1], r0, r1,
                        L.KMG_I32, bufs[2], n)
        ctx.synchronize()
        ctx.d2h(part, bufs[2])
    finally:
        for q in bufs:
            ctx.dfree(q)
    assert np.array_equal(part, K[r0:r1])


@gpu
@pytest.mark.parametrize("kind,fields,status", [
    (L.KMG_GKM, dict(k=10, g=4, m=3, strands=3), L.KMG_EINVAL),
    (L.KMG_MISMATCH, dict(k=10, m=1, window=101, strands=2), L.KMG_EUNSUPPORTED),
    (L.KMG_GKM, dict(k=16, g=8, m=3, strands=2), L.KMG_EUNSUPPORTED)])  # the square path at l = 16
def test_abi_refusals(ctx, kind, fields, status):
    codes, lens = E.synthetic(3, 101, seed=1)
    out = np.zeros((3, 3), dtype=np.float64)
    p = P.make(kind, **fields)
    assert ctx.lib.kmg_gram(ctx.handle, ctypes.byref(p), L.ptr(codes), L.ptr(lens), 3, 101,
                            L.KMG_F64, L.ptr(out), 3) == status
    assert fields["k"] != 16 or b"kmg_gkm_cross" in ctx.lib.kmg_last_error()


def test_square_path_refuses_both_strands_at_l16_before_any_device_work():
    with pytest.raises(ValueError, match="gkm"):
        GramEngine(0).gkm(["ACGT" * 10], 16, 8, both_strands=True)
