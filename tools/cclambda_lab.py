#!/usr/bin/env python
"""
One Lambda iteration against one T iteration of the SAME dmk_rccsd handle ("Lambda"): dmk_rccsd_lambda_update (the
reverse sweep of the amplitude equations) and dmk_rccsd_update (the amplitude equations, unchanged by the Lambda work).

Default shape o = 32, v = 128 (--nocc 64 --nvir 192 where memory allows).  The Fock matrix is diagonal with a gap, the six unpacked
blocks are random of scale 0.01 / v, the packed (vv|vv) block is lam X^T Y from 12 packed factor rows as in tools/ccsd_lab.py; the
amplitudes are random of scale 0.05 and are set again before every timed call, so both iterations always see the same operands
(the time of a contraction does not depend on the values).  dmk_rccsd_lambda_update keeps its T-only intermediates between calls as
long as t is not set again; they are therefore made once, in the warm-up, by a first update that is not timed: the timed Lambda
call is the sweep alone, as every iteration of dmk_rccsd_lambda_run after the first.

Warm-up rounds, then the median of --reps repetitions of each, interleaved (T, Lambda, T, ...), HIP events around each call; spread
= (max - min) / median.  With --breakdown the per-family times of the context's profile are added for one call of each.  By
contraction count the sweep issues one ladder and at most two products per forward product: <= 2 x the T iteration is expected.
Prints one JSON line; --out writes it to a file as well.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nocc", type=int, default=32)
    ap.add_argument("--nvir", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--breakdown", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from libdmet_preview_amd._lib import lib, get_ctx, c_vp
    ctx = get_ctx()
    o, v = a.nocc, a.nvir
    n, npair = o + v, v * (v + 1) // 2
    rng = np.random.default_rng(128)
    fock = np.diag(np.concatenate([np.linspace(-2.0, -1.0, o), np.linspace(1.0, 2.0, v)]))
    sizes = [o ** 4, o ** 3 * v, o * o * v * v, o * o * v * v, o * o * v * v, o * v ** 3]
    dev = [ctx.to_device(fock)] + [ctx.to_device((0.01 / v) * rng.standard_normal(k)) for k in sizes]
    naux, lam = 12, 0.05 / v
    d_X, d_Y = ctx.to_device(rng.standard_normal((naux, npair))), ctx.to_device(rng.standard_normal((naux, npair)))
    d_W = ctx.zeros((npair, npair), np.float64)
    ctx.check(lib.dmk_dgemm_tn_acc_rect(ctx.h, npair, npair, naux, lam, d_X.ptr, npair, d_Y.ptr, npair, d_W.ptr, npair))
    t2 = 0.05 * rng.standard_normal((o, o, v, v))
    d_t1, d_t2 = ctx.to_device(0.05 * rng.standard_normal((o, v))), ctx.to_device(0.5 * (t2 + t2.transpose(1, 0, 3, 2)))
    h = c_vp()
    ctx.check(lib.dmk_rccsd_create(ctx.h, o, v, *([d.ptr for d in dev] + [d_W.ptr, npair, 0, C.byref(h)])))

    def t_iter():
        ctx.check(lib.dmk_rccsd_update(h))

    def l_iter():
        ctx.check(lib.dmk_rccsd_lambda_update(h))

    def timed(f, prepare):
        prepare()
        ctx.timer_start()
        f()
        return ctx.timer_stop()

    def set_t():
        ctx.check(lib.dmk_rccsd_set(h, d_t1.ptr, d_t2.ptr))

    def set_l():          # t again, the kept intermediates made (untimed), l = the same numbers
        set_t()
        ctx.check(lib.dmk_rccsd_lambda_set(h, d_t1.ptr, d_t2.ptr))
        ctx.check(lib.dmk_rccsd_lambda_update(h))
        ctx.check(lib.dmk_rccsd_lambda_set(h, d_t1.ptr, d_t2.ptr))

    def stats(x):
        x = np.asarray(x)
        med = float(np.median(x))
        return {"median_ms": med, "min_ms": float(x.min()), "max_ms": float(x.max()), "spread": float((x.max() - x.min()) / med)}

    try:
        for _ in range(a.warmup):
            timed(t_iter, set_t)
            timed(l_iter, set_l)
        ctx.sync()
        t = {"T": [], "Lambda": []}
        for _ in range(a.reps):
            t["T"].append(timed(t_iter, set_t))
            t["Lambda"].append(timed(l_iter, set_l))
        res = {"nocc": o, "nvir": v, "reps": a.reps, "warmup": a.warmup, "T": stats(t["T"]), "Lambda": stats(t["Lambda"]),
               "T_ms_all": [round(x, 3) for x in t["T"]], "Lambda_ms_all": [round(x, 3) for x in t["Lambda"]]}
        res["ratio_Lambda_over_T"] = res["Lambda"]["median_ms"] / res["T"]["median_ms"]
        if a.breakdown:
            ctx.profile(True)
            for name, f, prep in (("T", t_iter, set_t), ("Lambda", l_iter, set_l)):
                prep()
                ctx.sync()
                ctx.profile_read(reset=True)
                f()
                ctx.sync()
                res[name]["families_ms"] = {k: round(float(x[0]), 3) for k, x in ctx.profile_read(reset=True).items() if x[1]}
            ctx.profile(False)
    finally:
        ctx.check(lib.dmk_rccsd_free(h))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
