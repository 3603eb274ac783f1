#!/usr/bin/env python3
"""Times the gkm substitution map against the explicit-mutant route, the only
one there was before it, on one both-strands (10, 6, 3) raw model of §6e's 9000 seeded rows:

  map       kmg_gkm_scorer_mutate_device over the queries ("mutate" stage)
  explicit  the 3 L single-letter mutants of every query written out on the host, uploaded, and
            scored with the queries themselves by kmg_gkm_scorer_score_device ("score" stage);
            the host wall time of writing and uploading the mutants is reported beside the
            device time, not inside it (they are uploaded once, before the repetitions)

Shapes: 9000 rows of 101 letters (§6e's seeded queries), 10^5 rows of 19 letters (deltaSVM's
2 l - 1), 256 rows of 1000 letters.  The two routes alternate in one process after a warm-up
of each; stages are the library's device events, medians over the repetitions.  The map is
compared with the differences of the explicit scores.  One JSON file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kernel-methods-for-genomics_amd"))

from kmgram import _lib as L  # noqa: E402
from kmgram import encode as E  # noqa: E402
from kmgram import params as P  # noqa: E402

LW, KI, D = 10, 6, 3


def mutants(q):
    """uint8 [nq * 3 L + nq, L]: row (qi * L + i) * 3 + t is query qi with the t-th other letter
    at position i; the queries themselves follow.  Also the letters written."""
    nq, n = q.shape
    m = np.repeat(q, 3 * n, axis=0)
    r = np.arange(nq * 3 * n)
    col = (r // 3) % n
    letter = ((q.reshape(-1)[r // 3] + 1 + r % 3) & 3).astype(np.uint8)
    m[r, col] = letter
    return np.concatenate([m, q]), letter


def run(ctx, sc, q, ql, reps):
    nq, n = q.shape
    d_q, d_l, d_map = ctx.dmalloc(q.nbytes), ctx.dmalloc(ql.nbytes), ctx.dmalloc(32 * nq * n)
    ctx.h2d(d_q, q)
    ctx.h2d(d_l, ql)
    t0 = time.perf_counter()
    m, letter = mutants(q)
    ml = np.full(m.shape[0], n, dtype=np.int32)
    t1 = time.perf_counter()
    d_m, d_ml, d_f = ctx.dmalloc(m.nbytes), ctx.dmalloc(ml.nbytes), ctx.dmalloc(8 * m.shape[0])
    ctx.h2d(d_m, m)
    ctx.h2d(d_ml, ml)
    ctx.synchronize()
    t2 = time.perf_counter()
    ms = {"mutate": [], "score": []}
    for rep in range(reps + 1):  # one warm-up round of both routes
        sc.mutate_device(d_q, d_l, nq, n, d_map, n)
        ctx.synchronize()
        a = ctx.stage_ms("mutate")
        sc.score_device(d_m, d_ml, m.shape[0], n, 0.0, d_f)
        ctx.synchronize()
        b = ctx.stage_ms("score")
        if rep >= 1:
            ms["mutate"].append(a)
            ms["score"].append(b)
    out = ctx.d2h(np.empty((nq, n, 4), dtype=np.float64), d_map)
    f = ctx.d2h(np.empty(m.shape[0], dtype=np.float64), d_f)
    for d in (d_q, d_l, d_map, d_m, d_ml, d_f):
        ctx.dfree(d)
    delta = f[:-nq] - np.repeat(f[-nq:], 3 * n)
    got = out.reshape(nq * n, 4)[np.arange(nq * 3 * n) // 3, letter]
    med = {s: float(np.median(v)) for s, v in ms.items()}
    words = n - LW + 1
    cover = sum(min(i, words - 1) - max(0, i - LW + 1) + 1 for i in range(n))
    return {"queries": nq, "letters": n, "mutants": int(m.shape[0] - nq), "reps": reps,
            "stage_ms_median": {"map_mutate": med["mutate"], "explicit_score": med["score"]},
            "stage_ms_all": {"map_mutate": ms["mutate"], "explicit_score": ms["score"]},
            "ratio_explicit_over_map": med["score"] / med["mutate"],
            "explicit_host_s": {"write_mutants": t1 - t0, "upload_mutants": t2 - t1},
            "h2d_bytes": {"map": int(q.nbytes + ql.nbytes), "explicit": int(m.nbytes + ml.nbytes)},
            "table_reads": {"map": 4 * cover * nq, "explicit": int(m.shape[0]) * words},
            "output_bytes": {"map": 32 * nq * n, "explicit": 8 * int(m.shape[0])},
            "max_abs_difference": float(np.max(np.abs(got - delta))),
            "max_abs_delta": float(np.max(np.abs(delta))),
            "own_letter_all_zero": bool(not out.reshape(nq * n, 4)[np.arange(nq * n), q.reshape(-1)].any())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gkm_mutate_timing.json"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    ctx = L.Context(0)
    rng = np.random.default_rng(14)
    codes, lens = E.synthetic(18000, 101, seed=5)  # rows [0, 9000): support vectors, then queries
    sc = ctx.gkm_scorer(P.gkm(LW, KI, D, normalize=False, both_strands=True), codes[:9000], lens[:9000],
                        rng.standard_normal(9000))
    ctx.set_timing(True)
    shapes = [(np.ascontiguousarray(codes[9000:]), lens[9000:]), E.synthetic(100000, 2 * LW - 1, seed=8),
              E.synthetic(256, 1000, seed=9)]
    res = {"l": LW, "k": KI, "d": D, "strands": 2, "shapes": [run(ctx, sc, q, ql, a.reps) for q, ql in shapes]}
    sc.close()
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps([{k: v for k, v in r.items() if k != "stage_ms_all"} for r in res["shapes"]]))


if __name__ == "__main__":
    main()
