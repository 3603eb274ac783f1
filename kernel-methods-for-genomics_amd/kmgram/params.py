"""Kernel parameters: the reference's coefficient formulas and the mismatch weights.

Everything here is scalar host arithmetic evaluated exactly as the reference's Python
does it, so that the float64 coefficients handed to the device are the same bits.
"""
from math import comb

from . import _lib as L


def beta(d, k):
    """WD degree weight, kernels.py:53-61: 2 * (d - k + 1) / d / (d + 1)."""
    return 2 * (d - k + 1) / d / (d + 1)


def delta(s):
    """WDS shift weight, kernels.py:106-112: 1/2/(s+1)."""
    return 1 / 2 / (s + 1)


def mismatch_weights(k, m):
    """w_m(h) = #{b : ham(u,b) <= m and ham(v,b) <= m} for two k-mers u, v at Hamming
    distance h.  Then <Phi_x, Phi_y> = sum_{a,b} w_m(ham(x_a, y_b)) where Phi is the
    mismatch feature map of get_phi_km (kernels.py:161-175).  For m=1: (1+3k, 4, 2, 0...).
    """
    w = []
    for h in range(k + 1):
        tot = 0
        for i in range(k - h + 1):  # letters changed where u and v agree
            for a in range(h + 1):  # differing positions where b takes u's letter
                for b in range(h - a + 1):  # ... where b takes v's letter
                    c = h - a - b  # ... where b takes a third letter (2 choices)
                    if i + b + c <= m and i + a + c <= m:
                        tot += comb(k - h, i) * 3 ** i * comb(h, a) * comb(h - a, b) * 2 ** c
        w.append(tot)
    return w


def gkm_weights(l, k, d):
    """h[m] = C(l - m, k) for m <= d, else 0 (m = 0..l): the gapped k-mers -- l-mers with k
    informative positions -- two words at Hamming distance m share (gkm-SVM, Ghandi et al.
    2014), truncated at d mismatches.  The device table is built from the same integers."""
    return [comb(l - m, k) if m <= d else 0 for m in range(l + 1)]


def gkm(l, k, d=None, normalize=True, both_strands=False):
    """KmgParams of the gapped k-mer kernel: word length l (1..16), k informative positions
    (1..l), truncation d (0..l - k; None = min(3, l - k), gkm-SVM's default).  The struct
    carries them as k = l, g = l - k, m = d.  both_strands=True (strands = 2) counts every word
    together with its reverse complement: K(x, y) + K(x, rc(y)), gkm-SVM's default."""
    l, k = int(l), int(k)
    if not 1 <= l <= 16:
        raise ValueError(f"gkm: word length l={l} outside 1..16")
    if not 1 <= k <= l:
        raise ValueError(f"gkm: k={k} informative positions outside 1..l (l={l})")
    d = min(3, l - k) if d is None else int(d)
    if not 0 <= d <= l - k:
        raise ValueError(f"gkm: truncation d={d} outside 0..l-k (l-k={l - k})")
    return make(L.KMG_GKM, k=l, g=l - k, m=d, normalize=1 if normalize else 0,
                strands=2 if both_strands else 0)


def gkm_profile(l, d, both_strands=False, normalize=False):
    """KmgParams of a mismatch-profile or filtered gkm call: word length l (1..16), bins
    m = 0..d (0 <= d <= l - 1).  No k enters: the struct carries k = l, m = d and g = d, the
    least the gkm parameter rule (g >= m) lets through."""
    l, d = int(l), int(d)
    if not 1 <= l <= 16:
        raise ValueError(f"gkm: word length l={l} outside 1..16")
    if not 0 <= d <= l - 1:
        raise ValueError(f"gkm: profile truncation d={d} outside 0..l-1 (l={l})")
    return make(L.KMG_GKM, k=l, g=d, m=d, normalize=1 if normalize else 0,
                strands=2 if both_strands else 0)


def gkm_binomial_filter(l, k, d):
    """float64 [d + 1]: C(l - m, k) for m = 0..d, the filter under which
    ``GramEngine.gkm_cross(filter=)`` equals the integer gkm kernel of (l, k, d) bit for bit.
    The estimated l-mer filters of gkm-SVM 2.0 / LS-GKM (truncated, full) have no closed form
    shipped here -- they could not be pinned against those programs -- so the caller supplies
    such coefficients."""
    import numpy as np
    gkm(l, k, d)  # the parameter rules
    return np.array(gkm_weights(int(l), int(k), int(d))[:int(d) + 1], dtype=np.float64)


def gkm_center_weights(length, l, M=50, H=50):
    """uint8 position weights of the words a = 0 .. length - l of a row of ``length`` letters,
    for the weighted gkm kernel (``GramEngine.gkm_cross(weights_a=, weights_b=)``):
    min(255, floor(M * 2 ** (-D_a / H)) + 1), D_a = |2a + l - length| / 2 the distance from the
    word's centre to the row's centre, so the weight is M + 1 at the centre and halves every H
    letters.  Modelled on the -M / -H options of LS-GKM's centre-weighted kernel (wgkm); LS-GKM
    was not at hand when this was written, so parity with its weights is unpinned."""
    import numpy as np
    length, l, M, H = int(length), int(l), int(M), int(H)
    if M < 0 or H < 1:
        raise ValueError(f"gkm_center_weights: M={M} must be >= 0 and H={H} >= 1")
    return np.array([min(255, int(M * 2.0 ** (-abs(2 * a + l - length) / 2 / H)) + 1)
                     for a in range(max(0, length - l + 1))], dtype=np.uint8)


def make(kind, **kw):
    """Fill a KmgParams struct."""
    p = L.KmgParams()
    p.kind = kind
    for name in ("k", "m", "d", "S", "g", "window", "normalize", "smith", "la_mode", "span",
                 "strands"):
        if name in kw:
            setattr(p, name, int(kw[name]))
    if "lbda" in kw:
        lbda = kw["lbda"]
        p.lambda_ = float(lbda)
        p.lambda2 = float(lbda ** 2)  # lbda**2 exactly as the reference evaluates it (kernels.py:340)
    for name in ("la_e", "la_d", "la_beta"):
        if name in kw:
            setattr(p, name, float(kw[name]))
    if kind in (L.KMG_WD, L.KMG_WDS):
        d = int(kw["d"])
        if d > L.KMG_MAX_COEF:
            raise L.KmgUnsupported(L.KMG_EUNSUPPORTED, f"d={d} > {L.KMG_MAX_COEF}")
        for k in range(1, d + 1):
            p.coef_a[k - 1] = beta(d, k)
    if kind == L.KMG_WDS:
        S = int(kw["S"])
        if S + 1 > L.KMG_MAX_COEF:
            raise L.KmgUnsupported(L.KMG_EUNSUPPORTED, f"S={S} too large")
        for s in range(S + 1):
            p.coef_b[s] = delta(s)
    p.diag_value = float("nan")
    return p
