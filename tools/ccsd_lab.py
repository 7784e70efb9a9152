#!/usr/bin/env python
"""
The particle-particle ladder kernel of CCSD (dmk_cc_ladder_s4) against the same contraction composed from calls the
library had before it:   out[r][a][b] = sum_cd tau[r][c][d] (ac|bd),   r over the o^2 occupied pairs.

Default shape o = 64, v = 192: m = 4096 rows, the 4-fold packed (vv|vv) block 18528 x 18528 (2.7 GB), filled on the device as
lam X^T Y from two sets of 12 packed factor rows (no bra <-> ket symmetry), tau random.

    new        dmk_cc_ladder_s4 on the packed block (it is never unpacked)
    composed   ONCE, outside the timed region: the block unpacked to v^4 (dmk_dmet_h2_scaled 4-fold -> 1-fold with every index an
               "impurity" index: weight 1, a plain copy; 10.9 GB).  Timed: v launches of dmk_dgemm_batched, launch c adding
               tau[:, c, :] . (ac|. .)^T for every a (the batch) into out[:, a, :]  (M = m, N = K = v, batch = v).

Warm-up rounds, then the median of --reps repetitions of each, interleaved (new, composed, new, ...); spread = (max - min) / median.
The 2-norm of the difference of the two results is a device-side cross-check.  TFLOP/s: the algorithmic 2 m v^4 flop, and for the new
kernel also the flop its launch issues to the matrix pipe (padded tiles and K chunks included), over the median time; the roof is
the 78.6 TFLOP/s of tools/coissue_probe.hip.  Prints one JSON line; --out writes it to a file as well.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOF_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nocc", type=int, default=64)
    ap.add_argument("--nvir", type=int, default=192)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from libdmet_preview_amd._lib import lib, get_ctx, c_vp
    ctx = get_ctx()
    o, v = a.nocc, a.nvir
    m, npair, vv = o * o, v * (v + 1) // 2, v * v
    rng = np.random.default_rng(192)
    naux, lam = 12, 0.05 / v
    d_X, d_Y = ctx.to_device(rng.standard_normal((naux, npair))), ctx.to_device(rng.standard_normal((naux, npair)))
    d_W = ctx.zeros((npair, npair), np.float64)
    ctx.check(lib.dmk_dgemm_tn_acc_rect(ctx.h, npair, npair, naux, lam, d_X.ptr, npair, d_Y.ptr, npair, d_W.ptr, npair))
    d_tau = ctx.to_device(rng.standard_normal((m, v, v)))
    d_new, d_base = ctx.empty((m, v, v), np.float64), ctx.empty((m, v, v), np.float64)
    # the composed path's operand: g[a][c][b][d] = (ac|bd), unpacked once
    d_g = ctx.empty((vv, vv), np.float64)
    every = np.arange(v, dtype=np.int32)
    ctx.check(lib.dmk_dmet_h2_scaled(ctx.h, v, every.ctypes.data, v, 4, d_W.ptr, npair, 1, d_g.ptr, vv))

    def new():
        ctx.check(lib.dmk_cc_ladder_s4(ctx.h, m, v, d_W.ptr, npair, d_tau.ptr, 1.0, 0.0, d_new.ptr))

    def composed():
        for c in range(v):
            ctx.check(lib.dmk_dgemm_batched(ctx.h, 0, 1, m, v, v, v, 1.0, c_vp(d_tau.address + 8 * c * v), vv, 0,
                                            c_vp(d_g.address + 8 * c * vv), v, v * vv, 1.0 if c else 0.0, d_base.ptr, vv, v))

    def timed(f):
        ctx.timer_start()
        f()
        return ctx.timer_stop()

    def stats(x):
        x = np.asarray(x)
        med = float(np.median(x))
        return {"median_ms": med, "min_ms": float(x.min()), "max_ms": float(x.max()), "spread": float((x.max() - x.min()) / med)}

    ctx.profile_read_flops(reset=True)
    new()
    executed = ctx.profile_read_flops(reset=True)["dgemm"]
    composed()
    d_ss = ctx.empty((1,), np.float64)
    ctx.check(lib.dmk_sub_sumsq(ctx.h, d_new.size, d_new.ptr, d_base.ptr, None, d_ss.ptr))
    diff2 = float(np.sqrt(d_ss.get()[0]))
    for _ in range(a.warmup):
        new()
        composed()
    ctx.sync()
    t = {"new": [], "composed": []}
    for _ in range(a.reps):
        t["new"].append(timed(new))
        t["composed"].append(timed(composed))
    algorithmic = 2.0 * m * float(v) ** 4
    res = {"nocc": o, "nvir": v, "m": m, "packed_block_GB": 8.0 * npair * npair / 1e9, "unpacked_GB": 8.0 * vv * vv / 1e9, "reps": a.reps,
           "warmup": a.warmup, "roof_TFLOPs": ROOF_TFLOPS, "new": stats(t["new"]), "composed": stats(t["composed"]),
           "new_ms_all": [round(x, 3) for x in t["new"]], "composed_ms_all": [round(x, 3) for x in t["composed"]],
           "norm2_difference": diff2, "algorithmic_TFLOP": algorithmic / 1e12, "executed_TFLOP_new": executed / 1e12}
    for k in ("new", "composed"):
        res[k]["algorithmic_TFLOPs"] = algorithmic / 1e12 / (res[k]["median_ms"] * 1e-3)
        res[k]["fraction_of_roof"] = res[k]["algorithmic_TFLOPs"] / ROOF_TFLOPS
    res["new"]["executed_TFLOPs"] = executed / 1e12 / (res["new"]["median_ms"] * 1e-3)
    res["ratio_new_over_composed"] = res["new"]["median_ms"] / res["composed"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
