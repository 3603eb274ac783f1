"""GramEngine: host orchestration of the device Gram kernels (one HIP device).

Each method takes a list of sequences (str) and returns the full symmetric
``np.ndarray (n, n) float64`` the matching reference function returns
(kernels.py:28-455).  All arithmetic runs in libkmgram.so on the GPU; the host only
encodes sequences, validates reference-visible error cases and copies results back.
"""
import os
import re
import threading

import numpy as np

from . import _lib as L
from . import encode as E
from . import params as P


class GramEngine:
    def __init__(self, device=None):
        if device is None:
            device = int(os.environ.get("KMG_DEVICE", "0"))
        self.device = device
        self._ctx = None
        self._lock = threading.Lock()

    @property
    def ctx(self):
        with self._lock:
            if self._ctx is None:
                self._ctx = L.Context(self.device)
            return self._ctx

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    # ------------------------------------------------------------------ helpers
    def _run(self, params, seqs, out_dtype=L.KMG_F64):
        codes, lens = E.encode(seqs)
        n = len(lens)
        if n == 0:
            return np.zeros((0, 0), dtype=L.DTYPES[out_dtype])
        return self.ctx.gram(params, codes, lens, out_dtype)

    @staticmethod
    def _require_acgt(seqs):
        """format() maps A,C,G,T -> 1..4 and int()s every character (kernels.py:184,193):
        any other character raises ValueError there; so do we."""
        for s in seqs:
            bad = set(s) - set(E.ACGT)
            if bad:
                ch = sorted(bad)[0]
                raise ValueError(f"invalid literal for int() with base 10: '{ch}'")

    # ------------------------------------------------------------------ kernels
    def spectrum(self, seqs, k, out_dtype=L.KMG_F64):
        """get_spectrum_K (kernels.py:28-47): K_ij = <phi_i, phi_j>, integer counts."""
        k = int(k)
        if k < 1:
            raise ValueError("k must be >= 1")
        return self._run(P.make(L.KMG_SPECTRUM, k=k), seqs, out_dtype)

    def mismatch(self, seqs, k, m, normalize=True, window=101, out_dtype=L.KMG_F64):
        """get_mismatch_K (kernels.py:196-217): <Phi_i, Phi_j> then normalize_K."""
        seqs = list(seqs)
        self._require_acgt(seqs)
        short = [len(s) for s in seqs if len(s) < window]
        if short:
            # get_phi_km slices windows up to 101 (kernels.py:171): a shorter sequence
            # yields k-mers of the wrong shape and numpy raises while comparing them.
            raise ValueError(f"operands could not be broadcast together (sequence of length "
                             f"{short[0]} < {window})")
        p = P.make(L.KMG_MISMATCH, k=int(k), m=int(m), window=window,
                   normalize=1 if normalize else 0)
        return self._run(p, seqs, out_dtype)

    def wd(self, seqs, d):
        """get_WD_K (kernels.py:84-101)."""
        return self._run(P.make(L.KMG_WD, d=int(d)), seqs)

    def wds(self, seqs, d, S):
        """get_WDShifts_K (kernels.py:138-155); rows of any lengths (the clipped-slice
        suffix matches of kernels.py:133 are counted on the device)."""
        return self._run(P.make(L.KMG_WDS, d=int(d), S=int(S)), seqs)

    @staticmethod
    def _pair_codes(x, y, length):
        """x and y cut or padded to ``length`` symbols with a code neither uses.  Slices of
        the padded strings that end inside them compare exactly like the reference's
        clipped slices: two clipped slices are equal iff they have the same length and
        symbols, and the padded ones iff they hold the same symbols and pad positions."""
        codes, lens = E.encode([x, y])
        used = set(np.unique(codes[0, :lens[0]]).tolist()) | set(np.unique(codes[1, :lens[1]]).tolist())
        pad = next((c for c in range(4, 255) if c not in used), None)
        if pad is None:
            raise ValueError("no free symbol code to pad the pair with")
        ldc = max(4, -(-length // 4) * 4)
        out = np.full((2, ldc), 255, dtype=np.uint8)
        for r in range(2):
            m = min(int(lens[r]), length)
            out[r, :m] = codes[r, :m]
            out[r, m:length] = pad
        return out, np.full(2, length, dtype=np.int32)

    def _pair_value(self, params, codes, lens):
        return float(self.ctx.gram(params, codes, lens, L.KMG_F64)[0, 1])

    def wd_pair(self, x, y, d, span):
        """get_WD_d(x, y, d, L=span) (kernels.py:64-81) for any L: windows end at or before
        L, so x and y padded to L symbols give every clipped comparison."""
        span = int(span)
        if span <= 1:
            return 0.0  # range(1, L - k + 1) is empty for every k
        codes, lens = self._pair_codes(x, y, span)
        return self._pair_value(P.make(L.KMG_WD, d=int(d), span=span), codes, lens)

    def wds_pair(self, x, y, d, S, span):
        """get_WDShifts_d(x, y, d, S, L=span) (kernels.py:115-135) for any L: windows end
        at or before L + S, so the pair is padded to L + S symbols and the sums run to L."""
        span, S = int(span), int(S)
        if span <= 1:
            return 0.0
        codes, lens = self._pair_codes(x, y, span + S)
        return self._pair_value(P.make(L.KMG_WDS, d=int(d), S=S, span=span), codes, lens)

    def substring(self, seqs, lbda, k):
        """get_string_K (kernels.py:367-382)."""
        return self._run(P.make(L.KMG_SUBSTRING, k=int(k), lbda=lbda), seqs)

    def local_alignment(self, seqs, e=11, d=1, beta=0.5, smith=0, eig=1, intended=False):
        """get_LA_K (kernels.py:273-302), reference semantics (the reference
        always returns an all-zero K, and raises ArpackError for eig=1, n >= 8).

        intended=True: the local-alignment kernel the reference means — five DP arrays
        instead of one aliased array, every cell up to [n_x, n_y], gap opening / extension
        factors exp(-beta e) / exp(-beta d) (g(n) = e + d(n-1), the docstring's affine
        gap) — computed on the device (gram_la_kernel; parity unpinned: the reference
        never produces it).  Like the reference, K itself is returned (its eig step only
        builds K1, kernels.py:288-302)."""
        seqs = list(seqs)
        self._require_acgt(seqs)
        n = len(seqs)
        if intended:
            if not beta > 0:
                raise ValueError("LA kernel needs beta > 0")
            p = P.make(L.KMG_LOCALALIGN, smith=int(smith), la_mode=L.KMG_LA_INTENDED,
                       la_e=e, la_d=d, la_beta=beta)
            return self._run(p, seqs)
        if eig == 1 and n >= 8:
            # eigs(K1) on the all-zero K: ARPACK info=-9 (kernels.py:294)
            from scipy.sparse.linalg import ArpackError
            raise ArpackError(-9)
        p = P.make(L.KMG_LOCALALIGN, smith=int(smith), la_mode=L.KMG_LA_REFERENCE,
                   la_e=e, la_d=d, la_beta=beta)
        return self._run(p, seqs)

    def gappy(self, seqs, k, g, intended=False):
        """get_gappy_K (kernels.py:436-455).

        intended=True: the kernel the reference means to compute (report §3.7) instead of
        its numpy-2 failure: phi_b(x) = [the (k-g)-mer b is an order-preserving
        subsequence of some window x[a:a+k], a in range(101 - k + 1)], K = normalize_K of
        the feature inner products (parity unpinned: the reference never produces it)."""
        seqs = list(seqs)
        self._require_acgt(seqs)
        k, g = int(k), int(g)
        if intended:
            if not (0 <= g < k):
                raise ValueError("intended gappy kernel needs 0 <= g < k")
            short = [len(s) for s in seqs if len(s) < 101]
            if short:
                raise ValueError(f"sequence of length {short[0]} shorter than the 101 window")
            p = P.make(L.KMG_GAPPY, k=k, g=g, window=101, normalize=1,
                       la_mode=L.KMG_MODE_INTENDED)
            return self._run(p, seqs)
        for s in seqs:
            gappy_reference_errors(len(s), k, g)
        return self._run(P.make(L.KMG_GAPPY, k=k, g=g, window=101), seqs)

    def gkm(self, seqs, l, k, d=None, normalize=True, out_dtype=L.KMG_F64, *, both_strands=False):
        """Gapped k-mer kernel of gkm-SVM / LS-GKM (Ghandi et al. 2014; no reference
        counterpart): K_ij = sum_{a,b} h[ham(x_i[a:a+l], x_j[b:b+l])], h[m] = C(l - m, k) for
        m <= d, over the all-ACGT words of the whole rows (a word holding any other character
        is not counted); d=None is min(3, l - k).  normalize=True applies normalize_K, and a
        sequence without a valid word (its K_ii would be 0) raises ValueError.
        both_strands=True counts a word together with its reverse complement, as gkm-SVM does
        by default: K(x, y) + K(x, rc(y)), symmetric, the diagonals of normalize_K included.
        It needs l <= 15 here (ValueError otherwise); ``gkm_cross`` serves l = 16.  The square
        path takes no position weights: ``gkm_cross(s, s, weights_a=w, weights_b=w)`` is the
        weighted square Gram."""
        p = P.gkm(l, k, d, normalize, both_strands)
        if both_strands and int(l) == 16:
            raise ValueError("gkm: both_strands=True at l=16 is served by gkm_cross only (the "
                             "reverse complement of A*16 is the square path's invalid-word marker)")
        seqs = list(seqs)
        if normalize:
            if out_dtype == L.KMG_I32:
                raise ValueError("gkm: normalised output needs a floating dtype")
            word = re.compile("[ACGT]{%d}" % int(l))
            for i, s in enumerate(seqs):
                if not word.search(s):
                    raise ValueError(f"gkm: sequence {i} has no all-ACGT word of length {int(l)}; "
                                     "its diagonal would be 0 under normalize=True")
        return self._run(p, seqs, out_dtype)

    @staticmethod
    def _gkm_weights(side, weights, seqs, l, normalize):
        """uint8 [n, ldw] of one side's position weights (None stays None); ValueError for a
        row with too few entries, a value outside 0..255 and, under normalize, a row whose valid
        words all have weight 0."""
        if weights is None:
            return None
        rows = list(weights)
        if len(rows) != len(seqs):
            raise ValueError(f"gkm: weights_{side} has {len(rows)} rows for {len(seqs)} sequences")
        words = [max(0, len(s) - l + 1) for s in seqs]
        out = np.zeros((len(seqs), max(words + [1])), dtype=np.uint8)
        for i, (w, nw, s) in enumerate(zip(rows, words, seqs)):
            w = np.asarray(w)
            if w.ndim != 1 or w.shape[0] < nw:
                raise ValueError(f"gkm: weights_{side}[{i}] needs {nw} entries (one a word)")
            w = w[:nw]
            if w.dtype.kind not in "iu" or (nw and (w.min() < 0 or w.max() > 255)):
                raise ValueError(f"gkm: weights_{side}[{i}] must be integers in 0..255")
            out[i, :nw] = w
            if normalize and not any(out[i, a] and set(s[a:a + l]) <= set("ACGT")
                                     for a in range(nw)):
                raise ValueError(f"gkm: every valid word of sequence {i} of side {side} has "
                                 "weight 0; its diagonal would be 0 under normalize=True")
        return out

    def gkm_profile(self, seqs_a, seqs_b, l, d, both_strands=False):
        """int64 [len(seqs_a), len(seqs_b), d + 1] mismatch profile, the quantity under every
        gkm kernel variant: N_m = #{(a, b) : ham(A_i[a:a+l], B_j[b:b+l]) = m} for m = 0..d,
        0 <= d <= l - 1, with ``gkm_cross``'s word rules (kmg_gkm_profile: int8 MFMA, exact).
        both_strands=True adds the counts against the reverse complement of B's words into the
        same bins.  Any gkm kernel value at this l is a dot product with it: one profile serves
        a model selection over (k, d) or a filter of the caller's."""
        p = P.gkm_profile(l, d, both_strands)
        seqs_a, seqs_b = list(seqs_a), list(seqs_b)
        if not seqs_a or not seqs_b:
            return np.zeros((len(seqs_a), len(seqs_b), int(d) + 1), dtype=np.int64)
        codes_a, lens_a = E.encode(seqs_a)
        codes_b, lens_b = E.encode(seqs_b)
        return self.ctx.gkm_profile(p, codes_a, lens_a, codes_b, lens_b)

    def gkm_cross(self, seqs_a, seqs_b, l, k=None, d=None, normalize=True, out_dtype=L.KMG_F64, *,
                  both_strands=False, weights_a=None, weights_b=None, filter=None):
        """Rectangular gapped k-mer block [len(seqs_a), len(seqs_b)]:
        K_ij = sum_{a,b} h[ham(A_i[a:a+l], B_j[b:b+l])] with ``gkm``'s h and word rules, rows
        of any length, T^16 counted (kmg_gkm_cross: int8 MFMA).  This is K(queries, support
        vectors) for prediction; ``gkm_cross(s, s)`` is the way to a square gkm Gram of rows
        longer than ``gkm`` takes.  normalize=True divides by sqrt(K(A_i, A_i) K(B_j, B_j)),
        and a row without a valid word on either side raises ValueError.  both_strands=True:
        K(A_i, B_j) + K(A_i, rc(B_j)) in one pass over the same staged words (l = 16 included),
        normalised by the both-strands diagonals.
        weights_a / weights_b (the position-weighted kernel, LS-GKM's wgkm; kmg_gkm_cross_w): a
        sequence of per-row integer arrays, or one 2-D array, row i with at least
        len(seq_i) - l + 1 entries in 0..255 (``params.gkm_center_weights``); the word starting at
        letter a of row i counts with weight [i][a], a pair with the product of its two
        weights, a reverse-complement word with the weight of the window it was made from, and
        the normalising diagonals with their own side's weights.  None is all ones.  Bad shapes
        or values and, under normalize=True, a row whose valid words all weigh 0 raise
        ValueError before any device work.
        filter (kmg_gkm_cross_f): real coefficients c[0..d] in place of h, K_ij = sum_m c[m]
        N_m(A_i, B_j) over the mismatch profile of ``gkm_profile``, summed in float64 in
        ascending m, each product and sum rounded on its own; d = len(filter) - 1 <= l - 1 and k
        may be None.  ``params.gkm_binomial_filter(l, k, d)`` gives the integer kernel back bit
        for bit; the estimated l-mer filters of gkm-SVM 2.0 / LS-GKM are the caller's to supply.
        Under normalize=True a filter with a non-positive diagonal gives inf / NaN there.  A
        filter together with weights, an integer out_dtype or a d that disagrees with its length
        raises ValueError."""
        if filter is not None:
            filter = np.asarray(filter, dtype=np.float64)
            if weights_a is not None or weights_b is not None:
                raise ValueError("gkm: filter= is not served together with position weights")
            if filter.ndim != 1 or not 1 <= filter.shape[0] <= int(l):
                raise ValueError(f"gkm: filter needs 1..l coefficients c[0..d], d <= l-1 (l={int(l)})")
            if d is not None and int(d) != filter.shape[0] - 1:
                raise ValueError(f"gkm: d={d} but the filter has {filter.shape[0]} coefficients")
            if out_dtype == L.KMG_I32:
                raise ValueError("gkm: a filtered block needs a floating dtype")
            d = filter.shape[0] - 1
            p = (P.gkm_profile(l, d, both_strands, normalize) if k is None
                 else P.gkm(l, k, d, normalize, both_strands))
        elif k is None:
            raise ValueError("gkm: k is needed where no filter= is given")
        else:
            p = P.gkm(l, k, d, normalize, both_strands)
        seqs_a, seqs_b = list(seqs_a), list(seqs_b)
        wa = self._gkm_weights("a", weights_a, seqs_a, int(l), normalize)
        wb = self._gkm_weights("b", weights_b, seqs_b, int(l), normalize)
        if normalize:
            if out_dtype == L.KMG_I32:
                raise ValueError("gkm: normalised output needs a floating dtype")
            word = re.compile("[ACGT]{%d}" % int(l))
            for side, seqs in (("a", seqs_a), ("b", seqs_b)):
                for i, s in enumerate(seqs):
                    if not word.search(s):
                        raise ValueError(f"gkm: sequence {i} of side {side} has no all-ACGT word "
                                         f"of length {int(l)}; its diagonal would be 0 under "
                                         "normalize=True")
        if not seqs_a or not seqs_b:
            return np.zeros((len(seqs_a), len(seqs_b)), dtype=L.DTYPES[out_dtype])
        codes_a, lens_a = E.encode(seqs_a)
        codes_b, lens_b = E.encode(seqs_b)
        return self.ctx.gkm_cross(p, codes_a, lens_a, codes_b, lens_b, out_dtype, wa, wb, filter)

    # ------------------------------------------------------------------ scoring
    def scorer(self, method, seqs, coef):
        """Scorer of f(q) = sum_t coef[t] K(q, seqs[t]) + bias for K = select_method(., method),
        without building any K (kmg_scorer_create).  ``method`` follows select_method's grammar
        (kernels.py:461-505), restricted to ``SP_k{k}`` (raw counts) and ``MM_k{k}_m{m}``
        (normalised, as get_mismatch_K returns it); anything else raises ValueError."""
        tok = str(method).split('_')
        try:
            if tok[0] == 'SP' and len(tok) == 2 and tok[1][:1] == 'k':
                p = P.make(L.KMG_SPECTRUM, k=int(tok[1][1:]))
            elif tok[0] == 'MM' and len(tok) == 3 and tok[1][:1] == 'k' and tok[2][:1] == 'm':
                p = P.make(L.KMG_MISMATCH, k=int(tok[1][1:]), m=int(tok[2][1:]), window=101,
                           normalize=1)
            else:
                raise ValueError
        except ValueError:
            raise ValueError(f"scorer: method {method!r} is not SP_k{{k}} or MM_k{{k}}_m{{m}}") from None
        seqs = list(seqs)
        mm = p.kind == L.KMG_MISMATCH
        self._check_scored(seqs, mm)
        codes, lens = E.encode(seqs)
        return EngineScorer(self, self.ctx.scorer(p, codes, lens, coef), mm)

    def gkm_scorer(self, seqs, coef, l, k=None, d=None, *, both_strands=False, weights=None,
                   filter=None, normalize=True, center_weights=None):
        """Scorer of f(q) = sum_t coef[t] K(q, seqs[t]) + bias for the gapped k-mer kernel K of
        ``gkm_cross`` with the same (l, k, d, both_strands, filter, normalize), from one table
        of 4^l l-mer weights and without any Gram block (kmg_gkm_scorer_create: gkm-SVM's
        gkmpredict and l-mer weight export).  l <= 12 and d <= 4 (a filter of at most five
        coefficients), else KmgUnsupported.  weights: the training rows' position weights as in
        ``gkm_cross(weights_b=)``; unlike the block, a filter and weights are served together
        when normalize=False.  center_weights=(M, H): ``params.gkm_center_weights`` of every
        training row, and of every scored row that brings no weights of its own.  Under
        normalize=True a training row without a valid word whose coef is not 0 raises
        ValueError; a scored row without one gives NaN.  Returns an ``EngineGkmScorer``."""
        seqs, l = list(seqs), int(l)
        if filter is not None:
            filter = np.asarray(filter, dtype=np.float64)
            if filter.ndim != 1 or not 1 <= filter.shape[0] <= l:
                raise ValueError(f"gkm: filter needs 1..l coefficients c[0..d], d <= l-1 (l={l})")
            if d is not None and int(d) != filter.shape[0] - 1:
                raise ValueError(f"gkm: d={d} but the filter has {filter.shape[0]} coefficients")
            d = filter.shape[0] - 1
            p = (P.gkm_profile(l, d, both_strands, normalize) if k is None
                 else P.gkm(l, k, d, normalize, both_strands))
        elif k is None:
            raise ValueError("gkm: k is needed where no filter= is given")
        else:
            p = P.gkm(l, k, d, normalize, both_strands)
        coef = np.asarray(coef, dtype=np.float64).reshape(-1)
        if coef.shape[0] != len(seqs):
            raise ValueError(f"gkm: coef has {coef.shape[0]} entries for {len(seqs)} sequences")
        if center_weights is not None and weights is None:
            weights = [P.gkm_center_weights(len(s), l, *center_weights) for s in seqs]
        w = self._gkm_weights("t", weights, seqs, l, False)
        if normalize:
            word = re.compile("[ACGT]{%d}" % l)
            for i, s in enumerate(seqs):
                if coef[i] != 0 and not word.search(s):
                    raise ValueError(f"gkm: training sequence {i} has no all-ACGT word of length "
                                     f"{l}; its diagonal would be 0 under normalize=True")
        codes, lens = E.encode(seqs)
        return EngineGkmScorer(self, self.ctx.gkm_scorer(p, codes, lens, coef, w, filter), l,
                               center_weights)

    def _check_scored(self, seqs, mm):
        """Mismatch rows: get_mismatch_K's own refusals (see ``mismatch``)."""
        if not mm:
            return
        self._require_acgt(seqs)
        short = [len(s) for s in seqs if len(s) < 101]
        if short:
            raise ValueError(f"operands could not be broadcast together (sequence of length "
                             f"{short[0]} < 101)")

    # ------------------------------------------------------------------ feature maps
    def features(self, kind, seqs, k, cols, m=0, g=0):
        """float64 [len(seqs), len(cols)]: the reference's per-sequence feature map of each
        sequence at the k-mer codes cols (uint32, base 4, first letter most significant;
        0xFFFFFFFF = a beta no window can equal), on the device (kmg_features):
        KMG_SPECTRUM get_phi_u (kernels.py:12-25), KMG_MISMATCH get_phi_km (161-175),
        KMG_GAPPY gappy_k at k=1, g=0 (420-433)."""
        codes, lens = E.encode(seqs)
        p = P.make(kind, k=int(k), m=int(m), g=int(g), window=101)
        return self.ctx.features(p, codes, lens, cols)

    def features_sym(self, kind, codes, lens, k, col_syms, m=0, bcast=False):
        """float64 [n, len(col_syms)] over symbol columns (kmg_features_sym): codes / lens are
        the rows in the caller's symbol code space, col_syms uint8 [ncols, 16] the betas' codes
        in the same space; bcast: get_phi_km's numpy broadcast of short k-mers (rows shorter
        than the 101 window)."""
        p = P.make(kind, k=int(k), m=int(m), window=101)
        return self.ctx.features_sym(p, codes, lens, col_syms,
                                     L.KMG_FEATURES_BCAST if bcast else 0)

    def substring_b_pair(self, x, y, lbda, k):
        """B_k(lbda, k, x, y) of the substring kernel's recursion (kernels.py:322-342) at the
        full strings, from the device sweep (la_mode KMG_MODE_SS_B)."""
        p = P.make(L.KMG_SUBSTRING, k=int(k), lbda=lbda, la_mode=L.KMG_MODE_SS_B)
        return float(self._run(p, [x, y])[0, 1])

    def normalize(self, K):
        """normalize_K (kernels.py:398-415) in place on a float64 C-contiguous matrix."""
        return self.ctx.normalize(K)

    def center(self, K):
        """center_K (kernels.py:387-395)."""
        return self.ctx.center(np.ascontiguousarray(K, dtype=np.float64))


class EngineScorer:
    """What ``GramEngine.scorer`` returns: ``score(seqs, bias)`` on strings."""

    def __init__(self, engine, scorer, mm):
        self.engine, self._s, self._mm = engine, scorer, mm

    def score(self, seqs, bias=0.0):
        seqs = list(seqs)
        if not seqs:
            return np.zeros(0, dtype=np.float64)
        self.engine._check_scored(seqs, self._mm)
        codes, lens = E.encode(seqs)
        return self._s.score(codes, lens, bias)

    def close(self):
        self._s.close()


class EngineGkmScorer:
    """What ``GramEngine.gkm_scorer`` returns: ``score(seqs, bias, weights)`` on strings,
    ``mutation_map(seqs, weights)``, the score difference of every single-letter substitution,
    and ``lmer_weights()``, the 4^l l-mer weights of the model."""

    def __init__(self, engine, scorer, l, center_weights=None):
        self.engine, self._s, self.l, self._center = engine, scorer, l, center_weights

    def score(self, seqs, bias=0.0, weights=None):
        """float64 [len(seqs)]: f(q) + bias for strings (or a DataFrame's ``seq`` column);
        weights as in ``gkm_cross(weights_a=)``."""
        seqs = E.as_sequence_list(seqs)
        if not seqs:
            return np.zeros(0, dtype=np.float64)
        if weights is None and self._center is not None:
            weights = [P.gkm_center_weights(len(s), self.l, *self._center) for s in seqs]
        w = GramEngine._gkm_weights("q", weights, seqs, self.l, False)
        codes, lens = E.encode(seqs)
        return self._s.score(codes, lens, bias, w)

    def mutation_map(self, seqs, weights=None):
        """float64 [len(seqs), longest row, 4]: the effect of every single-letter substitution
        on the raw score (saturation mutagenesis; deltaSVM for every variant of a query):
        out[q, i, b] = f_raw(seqs[q] with letter "ACGT"[b] at position i) - f_raw(seqs[q]), a sum
        of l-mer weight differences over the at most l words that cover i, in one kernel on the
        device (kmg_gkm_scorer_mutate).  The bias cancels; a normalised model's coef_t / sqrt(K_tt)
        is in the table, the query's own 1 / sqrt(K_qq) is not applied (a mutant has its own
        diagonal).  Zero at the query's own letter, past a row's end and in a row shorter than
        l; at an N all four entries are the full sums; a word with a second non-ACGT letter
        adds nothing.  weights and the stored center_weights as in ``score``."""
        seqs = E.as_sequence_list(seqs)
        if not seqs:
            return np.zeros((0, 0, 4), dtype=np.float64)
        if weights is None and self._center is not None:
            weights = [P.gkm_center_weights(len(s), self.l, *self._center) for s in seqs]
        w = GramEngine._gkm_weights("q", weights, seqs, self.l, False)
        codes, lens = E.encode(seqs)
        return self._s.mutate(codes, lens, w)

    def lmer_weights(self):
        """float64 [4^l]: the score of every l-mer under the model (deltaSVM's input), word z
        at its base-4 code, A C G T = 0 1 2 3, first letter most significant; with
        both_strands the entries of a word and of its reverse complement hold the same bits."""
        return self._s.table()

    def close(self):
        self._s.close()


def gappy_reference_errors(n_x, k, g, window=101):
    """Raise what gappy_k (kernels.py:420-433) raises under numpy 2 for a sequence of
    length n_x, before any work: combinations(x[i:i+k], k-g) refuses r = k-g < 0 once a
    window exists, and `b in gap_set` compares a length-k beta array with each (k-g)-tuple:
    the shapes (k,) and (r,) broadcast only when r == k, r == 1 or k == 1, and the result's
    truth value is defined only for one element.  Returns quietly when gap_set is empty
    (nothing is compared) or k=1, g=0."""
    r = k - g
    if window - k + 1 <= 0:
        return  # no window: gap_set = []
    if r < 0:
        raise ValueError("r must be non-negative")
    # the longest slice x[0:k] holds min(n_x, k) symbols: gap_set is non-empty iff r fits
    if min(n_x, k) < r:
        return
    if r in (k, 1) or k == 1:
        size = 0 if r == 0 else max(r, k)
        if size == 1:
            return
        if size == 0 or r == 0:
            raise ValueError("The truth value of an empty array is ambiguous. Use "
                             "`array.size > 0` to check that an array is not empty.")
        raise ValueError("The truth value of an array with more than one element is "
                         "ambiguous. Use a.any() or a.all()")
    raise ValueError(f"operands could not be broadcast together with shapes ({k},) ({r},) ")


_default = None
_default_lock = threading.Lock()


def default_engine():
    global _default
    with _default_lock:
        if _default is None:
            _default = GramEngine()
        return _default
