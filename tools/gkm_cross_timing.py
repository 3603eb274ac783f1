#!/usr/bin/env python3
"""Times the rectangular gkm kernel against the square path's row-range form on
the same seeded sequences (L = 101, l = 10, k = 6, d = 3, raw int32):

  cross  kmg_gkm_cross_device, rows [0, N/2) x rows [N/2, N)       (gram_gkmx_kernel, int8 MFMA)
  rows   kmg_gram_device, KMG_GKM, rows [0, N/2) x all N columns   (gram_gkm_kernel, not SYM);
         twice the pairs, so its time is halved for the comparison

Both alternate in one process after a warm-up of each; the kernel stage of every call is timed
by the library's device events.  A sample of the cross result is checked against the formula at
the timed sizes.  One point has no yardstick: 256 rows of 1000 letters against themselves,
reported as word pairs a second.  One JSON file.

--strands runs the both-strands comparison of DESIGN.md §6f instead and writes
profiles/gkm_strands_timing.json: at the same sizes, one both-strands call (strands = 2) of rows
[0, N/2) x [N/2, N) against the two single-strand calls that compute the same thing (B, and B
reverse-complemented on the host), "gkmx" stages, alternated in one process; and at the first
size one both-strands square call (kmg_gram_device, all rows, SYM) against twice the
single-strand "gkm" stage.  A both-strands call counts two evaluations a word pair.

--weighted times the position-weighted kernel of DESIGN.md §6g instead and writes
profiles/gkm_weighted_timing.json: at the same sizes and at the long-row point, the weighted
call (kmg_gkm_cross_w_device, seeded uniform 0..255 weights on both sides) against the
unweighted one (kmg_gkm_cross_device) on the same rows, raw float64 (int32 is refused at these
weights), "gkmx" stages, alternated in one process; once with one strand, once with both.
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


def formula(ca, cb):
    h = np.array(P.gkm_weights(LW, KI, D), dtype=np.int64)
    w = np.lib.stride_tricks.sliding_window_view
    return int(h[(w(ca, LW)[:, None, :] != w(cb, LW)[None, :, :]).sum(-1)].sum())


def at(d, off):
    return ctypes.c_void_p(d.value + int(off))


def sampled_wrong(ctx, d_K, codes_a, codes_b, rng, count=32):
    na, nb = len(codes_a), len(codes_b)
    pairs = [(0, 0), (na - 1, nb - 1), (0, nb - 1), (na - 1, 0)] + \
            [(int(rng.integers(0, na)), int(rng.integers(0, nb))) for _ in range(count - 4)]
    row = np.empty(nb, dtype=np.int32)
    bad = 0
    for i, j in pairs:
        ctx.d2h(row, at(d_K, 4 * i * nb))
        bad += int(row[j]) != formula(codes_a[i], codes_b[j])
    return bad, len(pairs)


def run(ctx, n, reps, rng):
    codes, lens = E.synthetic(n, 101, seed=5)
    ldc, h = codes.shape[1], n // 2
    d_codes, d_lens, d_K = ctx.dmalloc(codes.nbytes), ctx.dmalloc(lens.nbytes), ctx.dmalloc(4 * h * n)
    ctx.h2d(d_codes, codes)
    ctx.h2d(d_lens, lens)
    p = P.gkm(LW, KI, D, normalize=False)
    ctx.set_timing(True)
    dev = {"cross": [], "rows": []}
    for rep in range(reps + 1):  # one warm-up round of both routes
        ctx.gram_device(p, d_codes, d_lens, n, ldc, 0, h, L.KMG_I32, d_K, n)
        ctx.synchronize()
        if rep >= 1:
            dev["rows"].append(ctx.stage_ms("gkm"))
        ctx.gkm_cross_device(p, d_codes, d_lens, h, ldc, at(d_codes, h * ldc), at(d_lens, 4 * h),
                             n - h, ldc, L.KMG_I32, d_K, n - h)
        ctx.synchronize()
        if rep >= 1:
            dev["cross"].append(ctx.stage_ms("gkmx"))
    bad, cnt = sampled_wrong(ctx, d_K, codes[:h], codes[h:], rng)
    for d in (d_codes, d_lens, d_K):
        ctx.dfree(d)
    pw = 101 - LW + 1
    pairs = h * (n - h) * pw * pw  # word pairs of the cross block
    med = {r: float(np.median(v)) for r, v in dev.items()}
    same = {"cross": med["cross"], "rows": med["rows"] * (n - h) / n}  # ms at the cross block's pairs
    return {"n": n, "reps": reps, "words_a_row": pw, "stage_ms_median": med, "stage_ms_all": dev,
            "ms_at_equal_pairs": same, "ratio_rows_over_cross": same["rows"] / same["cross"],
            "word_pairs": pairs, "word_pairs_per_s": {r: pairs / (same[r] * 1e-3) for r in same},
            "sampled_entries_wrong": bad, "sampled_entries": cnt}


def run_long(ctx, n, length, reps, rng):
    codes, lens = E.synthetic(n, length, seed=6)
    ldc = codes.shape[1]
    d_codes, d_lens, d_K = ctx.dmalloc(codes.nbytes), ctx.dmalloc(lens.nbytes), ctx.dmalloc(4 * n * n)
    ctx.h2d(d_codes, codes)
    ctx.h2d(d_lens, lens)
    p = P.gkm(LW, KI, D, normalize=False)
    ctx.set_timing(True)
    ms = []
    for rep in range(reps + 1):
        ctx.gkm_cross_device(p, d_codes, d_lens, n, ldc, d_codes, d_lens, n, ldc, L.KMG_I32, d_K, n)
        ctx.synchronize()
        if rep >= 1:
            ms.append(ctx.stage_ms("gkmx"))
    bad, cnt = sampled_wrong(ctx, d_K, codes[:, :length], codes[:, :length], rng, 8)
    for d in (d_codes, d_lens, d_K):
        ctx.dfree(d)
    pw = length - LW + 1
    med = float(np.median(ms))
    return {"n": n, "length": length, "reps": reps, "words_a_row": pw, "stage_ms_median": med,
            "stage_ms_all": ms, "word_pairs": n * n * pw * pw,
            "word_pairs_per_s": n * n * pw * pw / (med * 1e-3),
            "sampled_entries_wrong": bad, "sampled_entries": cnt}


def run_strands(ctx, n, reps, rng):
    """cross: both-strands gkmx stage vs the sum of the two single-strand ones (B and rc(B))."""
    codes, lens = E.synthetic(n, 101, seed=5)
    ldc, h = codes.shape[1], n // 2
    rcb = np.ascontiguousarray(codes[h:, ::-1] ^ 3)  # every row is ldc = 101 letters long
    d_codes, d_lens, d_rcb = ctx.dmalloc(codes.nbytes), ctx.dmalloc(lens.nbytes), ctx.dmalloc(rcb.nbytes)
    d_K = ctx.dmalloc(4 * h * (n - h))
    ctx.h2d(d_codes, codes)
    ctx.h2d(d_lens, lens)
    ctx.h2d(d_rcb, rcb)
    p1, p2 = P.gkm(LW, KI, D, normalize=False), P.gkm(LW, KI, D, normalize=False, both_strands=True)
    ctx.set_timing(True)
    routes = {"fwd": (p1, at(d_codes, h * ldc)), "rc": (p1, d_rcb), "both": (p2, at(d_codes, h * ldc))}
    dev = {r: [] for r in routes}
    for rep in range(reps + 1):  # one warm-up round of every route; "both" last: it is checked
        for r, (p, d_b) in routes.items():
            ctx.gkm_cross_device(p, d_codes, d_lens, h, ldc, d_b, at(d_lens, 4 * h), n - h, ldc,
                                 L.KMG_I32, d_K, n - h)
            ctx.synchronize()
            if rep >= 1:
                dev[r].append(ctx.stage_ms("gkmx"))
    K = ctx.d2h(np.empty((h, n - h), dtype=np.int32), d_K)
    pairs = [(0, 0), (h - 1, n - h - 1)] + [(int(rng.integers(0, h)), int(rng.integers(0, n - h)))
                                            for _ in range(30)]
    bad = sum(int(K[i, j]) != formula(codes[i], codes[h + j]) + formula(codes[i], rcb[j])
              for i, j in pairs)
    for d in (d_codes, d_lens, d_rcb, d_K):
        ctx.dfree(d)
    pw = 101 - LW + 1
    evals = 2 * h * (n - h) * pw * pw  # two evaluations a word pair
    med = {r: float(np.median(v)) for r, v in dev.items()}
    two = med["fwd"] + med["rc"]
    return {"n": n, "reps": reps, "stage_ms_median": med, "stage_ms_all": dev,
            "two_single_strand_calls_ms": two, "ratio_both_over_two_calls": med["both"] / two,
            "evaluations": evals, "evaluations_per_s": {"both": evals / (med["both"] * 1e-3),
                                                        "two_calls": evals / (two * 1e-3)},
            "sampled_entries_wrong": bad, "sampled_entries": len(pairs)}


def run_weighted(ctx, codes, lens, h, reps, rng, both):
    """rows [0, h) x rows [h, n): the weighted gkmx stage against the unweighted one."""
    n, ldc = codes.shape[0], codes.shape[1]
    length = int(lens.max())
    pw = length - LW + 1
    wts = np.random.default_rng(13).integers(0, 256, (n, pw)).astype(np.uint8)
    bufs = [ctx.dmalloc(a.nbytes) for a in (codes, lens, wts)] + [ctx.dmalloc(8 * h * (n - h))]
    d_codes, d_lens, d_wts, d_K = bufs
    for d, a in zip(bufs, (codes, lens, wts)):
        ctx.h2d(d, a)
    p = P.gkm(LW, KI, D, normalize=False, both_strands=both)
    ctx.set_timing(True)
    d_b, d_lb = at(d_codes, h * ldc), at(d_lens, 4 * h)
    dev = {"plain": [], "weighted": []}
    for rep in range(reps + 1):  # one warm-up round of both routes; "weighted" last: it is checked
        ctx.gkm_cross_device(p, d_codes, d_lens, h, ldc, d_b, d_lb, n - h, ldc, L.KMG_F64, d_K, n - h)
        ctx.synchronize()
        if rep >= 1:
            dev["plain"].append(ctx.stage_ms("gkmx"))
        ctx.gkm_cross_w_device(p, d_codes, d_lens, h, ldc, d_wts, pw, d_b, d_lb, n - h, ldc,
                               at(d_wts, h * pw), pw, L.KMG_F64, d_K, n - h)
        ctx.synchronize()
        if rep >= 1:
            dev["weighted"].append(ctx.stage_ms("gkmx"))
    K = ctx.d2h(np.empty((h, n - h), dtype=np.float64), d_K)
    hh = np.array(P.gkm_weights(LW, KI, D), dtype=np.int64)
    win = np.lib.stride_tricks.sliding_window_view

    def formula_w(i, j):
        x, y = win(codes[i, :length], LW), win(codes[h + j, :length], LW)
        H = hh[(x[:, None, :] != y[None, :, :]).sum(-1)]
        if both:
            H = H + hh[(x[:, None, :] != (y[:, ::-1] ^ 3)[None, :, :]).sum(-1)]
        return int(wts[i].astype(np.int64) @ H @ wts[h + j].astype(np.int64))
    pairs = [(0, 0), (h - 1, n - h - 1)] + [(int(rng.integers(0, h)), int(rng.integers(0, n - h)))
                                            for _ in range(14)]
    bad = sum(int(K[i, j]) != formula_w(i, j) for i, j in pairs)
    for d in bufs:
        ctx.dfree(d)
    med = {r: float(np.median(v)) for r, v in dev.items()}
    evals = (2 if both else 1) * h * (n - h) * pw * pw
    return {"n": n, "rows_a": h, "rows_b": n - h, "length": length, "words_a_row": pw, "reps": reps,
            "strands": 2 if both else 1, "stage_ms_median": med, "stage_ms_all": dev,
            "plain_spread": (max(dev["plain"]) - min(dev["plain"])) / med["plain"],
            "ratio_weighted_over_plain": med["weighted"] / med["plain"], "evaluations": evals,
            "evaluations_per_s": {r: evals / (med[r] * 1e-3) for r in med},
            "sampled_entries_wrong": bad, "sampled_entries": len(pairs)}


def run_strands_square(ctx, n, reps, rng):
    """square: one both-strands kmg_gram_device call (SYM) vs twice the single-strand stage."""
    codes, lens = E.synthetic(n, 101, seed=5)
    ldc = codes.shape[1]
    d_codes, d_lens, d_K = ctx.dmalloc(codes.nbytes), ctx.dmalloc(lens.nbytes), ctx.dmalloc(4 * n * n)
    ctx.h2d(d_codes, codes)
    ctx.h2d(d_lens, lens)
    routes = {"one": P.gkm(LW, KI, D, normalize=False),
              "both": P.gkm(LW, KI, D, normalize=False, both_strands=True)}
    ctx.set_timing(True)
    dev = {r: [] for r in routes}
    for rep in range(reps + 1):
        for r, p in routes.items():
            ctx.gram_device(p, d_codes, d_lens, n, ldc, 0, n, L.KMG_I32, d_K, n)
            ctx.synchronize()
            if rep >= 1:
                dev[r].append(ctx.stage_ms("gkm"))
    K = ctx.d2h(np.empty((n, n), dtype=np.int32), d_K)
    pairs = [(0, 0), (n - 1, 0)] + [(int(rng.integers(0, n)), int(rng.integers(0, n))) for _ in range(30)]
    bad = sum(int(K[i, j]) != formula(codes[i], codes[j]) + formula(codes[i], codes[j, ::-1] ^ 3)
              for i, j in pairs)
    for d in (d_codes, d_lens, d_K):
        ctx.dfree(d)
    med = {r: float(np.median(v)) for r, v in dev.items()}
    return {"n": n, "reps": reps, "stage_ms_median": med, "stage_ms_all": dev,
            "twice_single_strand_ms": 2 * med["one"],
            "ratio_both_over_twice_single": med["both"] / (2 * med["one"]),
            "sampled_entries_wrong": bad, "sampled_entries": len(pairs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gkm_cross_timing.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="2000,9000")
    ap.add_argument("--long", default="256x1000")
    ap.add_argument("--strands", action="store_true",
                    help="the both-strands comparison (DESIGN.md §6f) instead of the routes above")
    ap.add_argument("--weighted", action="store_true",
                    help="the position-weighted kernel against the unweighted one (DESIGN.md §6g)")
    a = ap.parse_args()
    ctx = L.Context(0)
    rng = np.random.default_rng(12)
    if a.weighted:
        ln, ll = (int(v) for v in a.long.split("x"))
        sets = [E.synthetic(int(n), 101, seed=5) + (int(n) // 2,) for n in a.sizes.split(",")]
        cl, ll_ = E.synthetic(ln, ll, seed=6)
        sets.append((np.concatenate([cl, cl]), np.concatenate([ll_, ll_]), ln))  # the rows x themselves
        res = {"l": LW, "k": KI, "d": D}
        for name, both in (("one_strand", False), ("both_strands", True)):
            res[name] = [run_weighted(ctx, c, n_, h, a.reps, rng, both) for c, n_, h in sets]
        ctx.close()
        with open(a.out.replace("gkm_cross_timing.json", "gkm_weighted_timing.json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps([{k: v for k, v in r.items() if k != "stage_ms_all"}
                          for r in res["one_strand"] + res["both_strands"]]))
        return
    if a.strands:
        sizes = [int(n) for n in a.sizes.split(",")]
        res = {"l": LW, "k": KI, "d": D, "cross": [run_strands(ctx, n, a.reps, rng) for n in sizes],
               "square": run_strands_square(ctx, sizes[0], a.reps, rng)}
        ctx.close()
        out = a.out.replace("gkm_cross_timing.json", "gkm_strands_timing.json")
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps([{k: v for k, v in r.items() if k != "stage_ms_all"}
                          for r in res["cross"] + [res["square"]]]))
        return
    res = [run(ctx, int(n), a.reps, rng) for n in a.sizes.split(",")]
    ln, ll = (int(v) for v in a.long.split("x"))
    long_res = run_long(ctx, ln, ll, a.reps, rng)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump({"l": LW, "k": KI, "d": D, "sizes": res, "long_rows": long_res}, f, indent=1)
    print(json.dumps([{k: v for k, v in r.items() if k != "stage_ms_all"} for r in res + [long_res]]))


if __name__ == "__main__":
    main()
