#!/usr/bin/env python3
"""Times the gkm table scorer against the Gram route on §6e's seeded rows
(L = 101, l = 10, k = 6, d = 3, raw), one strand and both:

  scorer  kmg_gkm_scorer_create over N support vectors ("vtab", "butterfly" stages) and
          kmg_gkm_scorer_score_device over N queries ("score" stage)
  block   kmg_gkm_cross_device, N queries x N support vectors, float64 ("gkmx" stage); its
          product with beta is taken on the host for the comparison and is not timed (one read
          of the 8 N^2 bytes of the block: at least 0.08 ms at N = 9000 and 8 TB/s)

and a deltaSVM-shaped case: 10^5 queries of 2 l - 1 letters scored with the lanes a query the
library picks (8) and with a wave a query (KMG_GKM_SCORE_G=64), the same table, "score" stage.
All routes alternate in one process after a warm-up of each; stages are the library's device
events, medians over the repetitions.  The scores are compared with block . beta at the timed
size.  One JSON file.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kernel-methods-for-genomics_amd"))

from kmgram import _lib as L  # noqa: E402
from kmgram import encode as E  # noqa: E402
from kmgram import params as P  # noqa: E402

LW, KI, D = 10, 6, 3


def at(d, off):
    return ctypes.c_void_p(d.value + int(off))


def run(ctx, n, reps, both, rng):
    codes, lens = E.synthetic(2 * n, 101, seed=5)  # rows [0, n): support vectors, [n, 2n): queries
    ldc = codes.shape[1]
    beta = rng.standard_normal(n)
    p = P.gkm(LW, KI, D, normalize=False, both_strands=both)
    d_codes, d_lens, d_f = ctx.dmalloc(codes.nbytes), ctx.dmalloc(lens.nbytes), ctx.dmalloc(8 * n)
    ctx.h2d(d_codes, codes)
    ctx.h2d(d_lens, lens)
    d_K = ctx.dmalloc(8 * n * n)
    dq_codes, dq_lens = at(d_codes, n * ldc), at(d_lens, 4 * n)
    ctx.set_timing(True)
    ms = {s: [] for s in ("vtab", "butterfly", "score", "gkmx")}
    sc = None
    for rep in range(reps + 1):  # one warm-up round of every route
        if sc is not None:
            sc.close()
        sc = ctx.gkm_scorer(p, codes[:n], lens[:n], beta)
        create = {s: ctx.stage_ms(s) for s in ("vtab", "butterfly")}
        sc.score_device(dq_codes, dq_lens, n, ldc, 0.0, d_f)
        ctx.synchronize()
        score = ctx.stage_ms("score")
        ctx.gkm_cross_device(p, dq_codes, dq_lens, n, ldc, d_codes, d_lens, n, ldc, L.KMG_F64, d_K, n)
        ctx.synchronize()
        gkmx = ctx.stage_ms("gkmx")
        if rep >= 1:
            ms["score"].append(score)
            ms["gkmx"].append(gkmx)
            for s, v in create.items():
                ms[s].append(v)
    f = ctx.d2h(np.empty(n, dtype=np.float64), d_f)
    g, mag = np.empty(n), np.empty(n)
    for r0 in range(0, n, 1000):  # block . beta in row slabs on the host
        rows = ctx.d2h(np.empty((min(1000, n - r0), n)), at(d_K, 8 * r0 * n))
        g[r0:r0 + 1000], mag[r0:r0 + 1000] = rows @ beta, np.abs(rows) @ np.abs(beta)
    pw = 101 - LW + 1
    tol = (4 * LW + 2 * (D + 1) + pw + 16 + (n + 4) / 2) * 2.0 ** -52 * mag
    sc.close()
    for d in (d_codes, d_lens, d_f, d_K):
        ctx.dfree(d)
    med = {s: float(np.median(v)) for s, v in ms.items()}
    t4 = 4 ** LW
    return {"n": n, "queries": n, "strands": 2 if both else 1, "reps": reps, "stage_ms_median": med,
            "stage_ms_all": ms, "scorer_ms": med["vtab"] + med["butterfly"] + med["score"],
            "block_ms": med["gkmx"],
            "ratio_block_over_scorer": med["gkmx"] / (med["vtab"] + med["butterfly"] + med["score"]),
            "bytes": {"vtab": n * 4 * (ldc // 16 + 2 + ldc // 32 + 2) + 16 * n + 3 * 16 * t4 + 8 * t4,
                      "score": n * 4 * (ldc // 16 + 2 + ldc // 32 + 2) + 8 * n * pw + 8 * n},
            "atomics": {"vtab": 2 * n * pw},
            "max_err_over_tol": float(np.max(np.abs(f - g) / np.maximum(tol, 1e-300))),
            "nonzero_scores": int(np.count_nonzero(f))}


def run_delta(ctx, nq, reps, rng):
    """deltaSVM's shape: nq rows of 2 l - 1 letters (l words) against one table."""
    codes, lens = E.synthetic(9000, 101, seed=5)
    sc = ctx.gkm_scorer(P.gkm(LW, KI, D, normalize=False, both_strands=True), codes, lens,
                        rng.standard_normal(9000))
    q, ql = E.synthetic(nq, 2 * LW - 1, seed=8)
    ldc = q.shape[1]
    d_q, d_l, d_f = ctx.dmalloc(q.nbytes), ctx.dmalloc(ql.nbytes), ctx.dmalloc(8 * nq)
    ctx.h2d(d_q, q)
    ctx.h2d(d_l, ql)
    ctx.set_timing(True)
    lanes = {"auto": None, "wave": "64"}
    ms, out = {r: [] for r in lanes}, {}
    for rep in range(reps + 1):
        for r, g in lanes.items():
            os.environ.pop("KMG_GKM_SCORE_G", None)
            if g:
                os.environ["KMG_GKM_SCORE_G"] = g
            ctx.reload_tuning()
            sc.score_device(d_q, d_l, nq, ldc, 0.0, d_f)
            ctx.synchronize()
            if rep >= 1:
                ms[r].append(ctx.stage_ms("score"))
            out[r] = ctx.d2h(np.empty(nq, dtype=np.float64), d_f)
    os.environ.pop("KMG_GKM_SCORE_G", None)
    ctx.reload_tuning()
    sc.close()
    for d in (d_q, d_l, d_f):
        ctx.dfree(d)
    med = {r: float(np.median(v)) for r, v in ms.items()}
    return {"queries": nq, "letters": 2 * LW - 1, "words_a_query": LW, "reps": reps,
            "lanes_a_query": {"auto": 8, "wave": 64}, "stage_ms_median": med, "stage_ms_all": ms,
            "ratio_wave_over_auto": med["wave"] / med["auto"],
            "max_abs_difference": float(np.max(np.abs(out["auto"] - out["wave"]))),
            "nonzero_scores": int(np.count_nonzero(out["auto"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gkm_scorer_timing.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=9000)
    ap.add_argument("--delta", type=int, default=100000)
    a = ap.parse_args()
    ctx = L.Context(0)
    rng = np.random.default_rng(14)
    res = {"l": LW, "k": KI, "d": D, "predict": [run(ctx, a.n, a.reps, both, rng) for both in (False, True)],
           "delta": run_delta(ctx, a.delta, a.reps, rng)}
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps([{k: v for k, v in r.items() if k != "stage_ms_all"}
                      for r in res["predict"] + [res["delta"]]]))


if __name__ == "__main__":
    main()
