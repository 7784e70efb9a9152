#!/usr/bin/env python
"""
The mixed-spin particle-particle ladder of UCCSD (dmk_cc_ladder_s4_ab)
    out[r][a][B] = sum_{c,D} tau[r][c][D] (ac|BD),   r over the oa ob occupied pairs,
against (a) the same-spin kernel dmk_cc_ladder_s4 in the same interleaved run and (b) the contraction composed from calls the library
had before it.  Modelled on tools/ccsd_lab.py.

Default shape m = 4096, va = vb = 192: the packed (vv|VV) block 18528 x 18528 (2.7 GB), filled on the device as lam X^T Y from two
sets of 12 packed factor rows (no bra <-> ket symmetry), tau random.  --nvir-a 160 --nvir-b 224 is the rectangular case.

    mixed      dmk_cc_ladder_s4_ab on the packed block (it is never unpacked)
    same       dmk_cc_ladder_s4 with nvir = --nvir-same (default: va when va = vb, else 192) on a square packed block of its own and a tau
               of its own: at va = vb the same block, the same tau and the same result, bit for bit (checked)
    composed   ONCE, outside the timed region: the block in full, g[a][c][B][D] = lam X1^T Y1 from the factor rows expanded to (a, c)
               and (B, D) on the host.  Timed: va launches of dmk_dgemm_batched, launch c adding tau[:, c, :] . (ac|. .)^T for every a
               (the batch) into out[:, a, :]  (M = m, N = K = vb, batch = va).

Warm-up rounds, then the median of --reps repetitions of each, interleaved (mixed, same, composed, mixed, ...); spread = (max - min) /
median.  TFLOP/s: the algorithmic 2 m va^2 vb^2 flop over the median time.  Prints one JSON line; --out writes it to a file as well.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _pair_index(v):
    idx = np.zeros((v, v), dtype=np.int64)
    i, j = np.tril_indices(v)
    idx[i, j] = idx[j, i] = np.arange(len(i))
    return idx.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--nvir-a", type=int, default=192)
    ap.add_argument("--nvir-b", type=int, default=192)
    ap.add_argument("--nvir-same", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from libdmet_preview_amd._lib import lib, get_ctx, c_vp
    ctx = get_ctx()
    m, va, vb = a.m, a.nvir_a, a.nvir_b
    vs = a.nvir_same or (va if va == vb else 192)
    npa, npb, nps = va * (va + 1) // 2, vb * (vb + 1) // 2, vs * (vs + 1) // 2
    rng = np.random.default_rng(192)
    naux, lam = 12, 0.05 / max(va, vb)
    X, Y = rng.standard_normal((naux, npa)), rng.standard_normal((naux, npb))
    d_X, d_Y = ctx.to_device(X), ctx.to_device(Y)
    d_W = ctx.zeros((npa, npb), np.float64)
    ctx.check(lib.dmk_dgemm_tn_acc_rect(ctx.h, npa, npb, naux, lam, d_X.ptr, npa, d_Y.ptr, npb, d_W.ptr, npb))
    d_tau = ctx.to_device(rng.standard_normal((m, va, vb)))
    d_mixed, d_base = ctx.empty((m, va, vb), np.float64), ctx.empty((m, va, vb), np.float64)
    shared = va == vb == vs                                   # the same-spin kernel can read the very same block and tau
    if shared:
        d_Ws, d_taus = d_W, d_tau
    else:
        d_Xs, d_Ys = ctx.to_device(rng.standard_normal((naux, nps))), ctx.to_device(rng.standard_normal((naux, nps)))
        d_Ws = ctx.zeros((nps, nps), np.float64)
        ctx.check(lib.dmk_dgemm_tn_acc_rect(ctx.h, nps, nps, naux, lam, d_Xs.ptr, nps, d_Ys.ptr, nps, d_Ws.ptr, nps))
        d_taus = ctx.to_device(rng.standard_normal((m, vs, vs)))
    d_same = ctx.empty((m, vs, vs), np.float64)
    # the composed path's operand: g[a][c][B][D] = (ac|BD) in full, made once
    d_X1, d_Y1 = ctx.to_device(np.ascontiguousarray(X[:, _pair_index(va)])), ctx.to_device(np.ascontiguousarray(Y[:, _pair_index(vb)]))
    d_g = ctx.zeros((va * va, vb * vb), np.float64)
    ctx.check(lib.dmk_dgemm_tn_acc_rect(ctx.h, va * va, vb * vb, naux, lam, d_X1.ptr, va * va, d_Y1.ptr, vb * vb, d_g.ptr, vb * vb))

    def mixed():
        ctx.check(lib.dmk_cc_ladder_s4_ab(ctx.h, m, va, vb, d_W.ptr, npb, d_tau.ptr, 1.0, 0.0, d_mixed.ptr))

    def same():
        ctx.check(lib.dmk_cc_ladder_s4(ctx.h, m, vs, d_Ws.ptr, nps, d_taus.ptr, 1.0, 0.0, d_same.ptr))

    def composed():
        for c in range(va):
            ctx.check(lib.dmk_dgemm_batched(ctx.h, 0, 1, m, vb, vb, va, 1.0, c_vp(d_tau.address + 8 * c * vb), va * vb, 0,
                                            c_vp(d_g.address + 8 * c * vb * vb), vb, va * vb * vb, 1.0 if c else 0.0, d_base.ptr,
                                            va * vb, vb))

    def timed(f):
        ctx.timer_start()
        f()
        return ctx.timer_stop()

    def stats(x):
        x = np.asarray(x)
        med = float(np.median(x))
        return {"median_ms": med, "min_ms": float(x.min()), "max_ms": float(x.max()), "spread": float((x.max() - x.min()) / med)}

    mixed()
    same()
    composed()
    d_ss = ctx.empty((1,), np.float64)
    ctx.check(lib.dmk_sub_sumsq(ctx.h, d_mixed.size, d_mixed.ptr, d_base.ptr, None, d_ss.ptr))
    diff2 = float(np.sqrt(d_ss.get()[0]))
    same_bits = None
    if shared:
        ctx.check(lib.dmk_sub_sumsq(ctx.h, d_mixed.size, d_mixed.ptr, d_same.ptr, None, d_ss.ptr))
        same_bits = float(d_ss.get()[0]) == 0.0
    for _ in range(a.warmup):
        mixed()
        same()
        composed()
    ctx.sync()
    t = {"mixed": [], "same": [], "composed": []}
    for _ in range(a.reps):
        t["mixed"].append(timed(mixed))
        t["same"].append(timed(same))
        t["composed"].append(timed(composed))
    flop = {"mixed": 2.0 * m * float(va) ** 2 * float(vb) ** 2, "same": 2.0 * m * float(vs) ** 4}
    flop["composed"] = flop["mixed"]
    res = {"m": m, "nvir_a": va, "nvir_b": vb, "nvir_same": vs, "packed_block_GB": 8.0 * npa * npb / 1e9, "full_block_GB": 8.0 * (va * vb) ** 2 / 1e9,
           "reps": a.reps, "warmup": a.warmup, "norm2_difference_mixed_composed": diff2, "mixed_equals_same_bitwise": same_bits}
    for k in t:
        res[k] = stats(t[k])
        res[k]["ms_all"] = [round(x, 3) for x in t[k]]
        res[k]["algorithmic_TFLOPs"] = flop[k] / 1e12 / (res[k]["median_ms"] * 1e-3)
    res["ratio_mixed_over_same_time"] = res["mixed"]["median_ms"] / res["same"]["median_ms"]
    res["ratio_mixed_over_same_rate"] = res["mixed"]["algorithmic_TFLOPs"] / res["same"]["algorithmic_TFLOPs"]
    res["ratio_mixed_over_composed_time"] = res["mixed"]["median_ms"] / res["composed"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
