#!/usr/bin/env python3
"""Times the two routes to f(q) = sum_t beta_t K(q, x_t) for a batch of new sequences
("Scoring without K"):

  (a) the square Gram of the N + Q rows on the device (the only route before the scorer),
      K[Q, T] . beta then taken on the host from the last Q rows (not timed);
  (b) kmg_scorer_create + kmg_scorer_score_device.

Both routes alternate in one process, after a warm-up of each; every call is timed by the
host clock around a call that ends in a synchronise, and its stages by the library's device
events (kmg_stage_stats).  The outputs are compared at the timed sizes against
tol_q = (N P + 4 k + P + 16) 2^-52 sum_t |beta_t| K^(q, t).  One JSON file is written.
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

HBM_PEAK = 8.0e12
STAGES = ("place", "fine", "pack", "diag", "vtab", "butterfly", "score", "gram", "mirror", "lists",
          "nbfill")


def stage_bytes(n, q, k, m, mm, ldc):
    """Bytes every scorer stage must move (DESIGN.md formulas)."""
    p = 101 - k + 1
    t4 = 4 ** k
    nt = min(2 * m, k) + 1 if mm else 1
    launches = -(-k // 4)
    ldp = (ldc // 16 + 2) + (ldc // 32 + 2)
    return {
        "vtab": 4 * (t4 + 1) + 2 * n * p + 16 * n + 8 * t4,
        "butterfly": (8 * t4 * (1 + nt) + 2 * 8 * t4 * nt * (launches - 2) + 8 * t4 * (nt + 1)
                      if mm and launches > 1 else (8 * t4 * 2 if mm else 0)),
        "score": 4 * q * ldp + 8 * q * p + 8 * q,
    }


def run(ctx, name, params, out_dtype, n, q, seed, reps, rng):
    codes, lens = E.synthetic(n + q, 101, seed=seed)
    ldc = codes.shape[1]
    beta = rng.standard_normal(n)
    mm = params.kind == L.KMG_MISMATCH
    tot = n + q
    esz = np.dtype(L.DTYPES[out_dtype]).itemsize
    d_codes, d_lens = ctx.dmalloc(codes.nbytes), ctx.dmalloc(lens.nbytes)
    d_K, d_f = ctx.dmalloc(tot * tot * esz), ctx.dmalloc(8 * q)
    ctx.h2d(d_codes, codes)
    ctx.h2d(d_lens, lens)
    dq_codes = L.ctypes.c_void_p(d_codes.value + n * ldc)
    dq_lens = L.ctypes.c_void_p(d_lens.value + 4 * n)
    ctx.set_timing(True)
    wall = {"gram": [], "create": [], "score": []}
    sc = None
    for rep in range(reps + 2):  # two warm-up rounds of every route
        if rep == 2:
            ctx.timing_reset()
            stats = {r: {s: [0.0, 0] for s in STAGES} for r in wall}
        for route in ("gram", "create", "score"):
            t0 = time.perf_counter()
            if route == "gram":
                ctx.gram_device(params, d_codes, d_lens, tot, ldc, 0, tot, out_dtype, d_K, tot)
            elif route == "create":
                if sc is not None:
                    sc.close()
                sc = ctx.scorer(params, codes[:n], lens[:n], beta)
            else:
                sc.score_device(dq_codes, dq_lens, q, ldc, 0.0, d_f)
            ctx.synchronize()
            if rep >= 2:
                wall[route].append((time.perf_counter() - t0) * 1e3)
                for s in STAGES:
                    ms = ctx.stage_ms(s)
                    if ms >= 0:
                        stats[route][s][0] += ms
                        stats[route][s][1] += 1
    f_b = ctx.d2h(np.empty(q, dtype=np.float64), d_f)
    # route (a)'s answer: the last q rows of K against beta, in row slabs on the host
    f_a, mag = np.empty(q), np.empty(q)
    slab = max(1, (1 << 28) // (tot * esz))
    for r0 in range(0, q, slab):
        r1 = min(q, r0 + slab)
        rows = np.empty((r1 - r0, tot), dtype=L.DTYPES[out_dtype])
        ctx.d2h(rows, L.ctypes.c_void_p(d_K.value + (n + r0) * tot * esz))
        blk = rows[:, :n].astype(np.float64)
        f_a[r0:r1] = blk @ beta
        mag[r0:r1] = blk @ np.abs(beta)
    pw = 101 - params.k + 1
    tol = (n * pw + 4 * params.k + pw + 16) * 2.0 ** -52 * mag
    ratio = float(np.max(np.abs(f_a - f_b) / np.maximum(tol, 1e-300)))
    sc.close()
    for d in (d_codes, d_lens, d_K, d_f):
        ctx.dfree(d)
    nbytes = stage_bytes(n, q, params.k, params.m, mm, ldc)
    med = {r: float(np.median(v)) for r, v in wall.items()}
    stage_ms = {r: {s: t / c for s, (t, c) in st.items() if c} for r, st in stats.items()}
    frac = {s: nbytes[s] / (stage_ms[r][s] * 1e-3) / HBM_PEAK
            for r, s in (("create", "vtab"), ("create", "butterfly"), ("score", "score"))
            if s in stage_ms[r] and nbytes[s]}
    return {"name": name, "n": n, "q": q, "reps": reps, "wall_ms_median": med,
            "wall_ms_min": {r: float(np.min(v)) for r, v in wall.items()},
            "stage_ms_mean": stage_ms, "stage_bytes": nbytes, "fraction_of_8TBs": frac,
            "max_err_over_tol": ratio, "nonzero_scores": int(np.count_nonzero(f_b))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink both workloads (rehearsal)")
    a = ap.parse_args()
    ctx = L.Context(0)
    rng = np.random.default_rng(11)
    sz = lambda v: max(64, int(v * a.scale))  # noqa: E731
    res = [run(ctx, "spectrum_k8", P.make(L.KMG_SPECTRUM, k=8), L.KMG_I32, sz(100000), sz(10000),
               4, a.reps, rng),
           run(ctx, "mismatch_k9_m1", P.make(L.KMG_MISMATCH, k=9, m=1, window=101, normalize=1),
               L.KMG_F64, sz(20000), sz(2000), 3, a.reps, rng)]
    ctx.close()
    with open(a.out, "w") as f:
        json.dump({"workloads": res}, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
