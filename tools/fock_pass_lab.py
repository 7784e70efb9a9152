#!/usr/bin/env python
"""
One-pass Fock build against the two passes it replaces.

One resident 4-fold block at n = 256 (8.66 GB), filled on the device as lam L^T L from 12 packed factor rows.  Timed with HIP events,
in one process on the same buffers:

    fused   dmk_fock_s4            J and K from one pass over the block
    pair    dmk_jk_s4 J-only, then dmk_jk_s4 K-only   (jk_j_kernel, then the K-only family of the same row kernel in csrc/jk.hip)

Warm-up calls, then the median of --reps repetitions of each, interleaved (fused, pair, fused, ...) so that clock drift hits both
alike; the spread reported is (max - min) / median.  Also the wall time of one converged RHF at the same n, with its iteration
count, through both Fock builds.  Prints one JSON line; --out writes it to a file as well.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from libdmet_preview_amd._lib import lib, get_ctx
    from libdmet_preview_amd.solver import scf
    ctx = get_ctx()
    n = a.n
    npair = n * (n + 1) // 2
    rng = np.random.default_rng(256)
    naux, lam = 12, 0.05 / n
    sym = lambda x: 0.5 * (x + np.swapaxes(x, -1, -2))
    A = sym(rng.standard_normal((naux, n, n)))
    ti, tj = np.tril_indices(n)
    d_L = ctx.to_device(A[:, ti, tj])
    d_E = ctx.zeros((npair, npair), np.float64)
    ctx.check(lib.dmk_dgemm_tn_acc_rect(ctx.h, npair, npair, naux, lam, d_L.ptr, npair, d_L.ptr, npair, d_E.ptr, npair))
    d_dm = ctx.to_device(sym(rng.standard_normal((n, n))))
    d_vj, d_vk = ctx.empty((n, n), np.float64), ctx.empty((n, n), np.float64)

    def fused():
        ctx.check(lib.dmk_fock_s4(ctx.h, n, d_E.ptr, npair, d_dm.ptr, d_dm.ptr, d_vj.ptr, d_vk.ptr))

    def j_only():
        ctx.check(lib.dmk_jk_s4(ctx.h, n, d_E.ptr, npair, d_dm.ptr, None, None, d_vj.ptr, None, None))

    def k_only():
        ctx.check(lib.dmk_jk_s4(ctx.h, n, d_E.ptr, npair, None, None, d_dm.ptr, None, None, d_vk.ptr))

    def pair():
        j_only()
        k_only()

    def timed(f):
        ctx.timer_start()
        f()
        return ctx.timer_stop()

    fused()
    ref_j, ref_k = d_vj.get(), d_vk.get()
    pair()
    agree = max(float(np.abs(ref_j - d_vj.get()).max()), float(np.abs(ref_k - d_vk.get()).max()))
    for _ in range(a.warmup):
        fused()
        pair()
    ctx.sync()
    t = {"fused": [], "pair": [], "j_only": [], "k_only": []}
    for _ in range(a.reps):
        t["fused"].append(timed(fused))
        t["pair"].append(timed(pair))
        t["j_only"].append(timed(j_only))
        t["k_only"].append(timed(k_only))
    block_bytes = 8.0 * npair * npair
    passes = {"fused": 1, "pair": 2, "j_only": 1, "k_only": 1}
    res = {"n": n, "block_GB": block_bytes / 1e9, "reps": a.reps, "warmup": a.warmup, "max_abs_difference_fused_vs_pair": agree}
    for k, v in t.items():
        v = np.asarray(v)
        med = float(np.median(v))
        res[k] = {"median_ms": med, "min_ms": float(v.min()), "max_ms": float(v.max()), "spread": float((v.max() - v.min()) / med),
                  "TB_per_s": passes[k] * block_bytes / (med * 1e-3) / 1e12}
    res["ratio_fused_over_pair"] = res["fused"]["median_ms"] / res["pair"]["median_ms"]

    # one converged RHF at the same n, through both Fock builds
    levels = np.linspace(0.0, 1.0, n)
    levels[n // 2:] += 1.5
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    h1 = sym((q * (levels - levels.mean())) @ q.T)
    for name, two_pass in (("rhf_fused", False), ("rhf_two_pass", True)):
        scf.TWO_PASS_FOCK = two_pass
        s = scf.SCF(newton_ah=False)
        s.set_system(n, 0, False, True)
        s.set_integral_dev(n, 0.0, ctx.to_device(h1[None]), None, [d_E])
        s.HF(tol=1e-10)              # warm-up: scratch growth, first launches
        ctx.sync()
        t0 = time.perf_counter()
        E, _ = s.HF(tol=1e-10)
        ctx.sync()
        res[name] = {"wall_s": time.perf_counter() - t0, "diagonalisations": s.mf.cycles, "converged": bool(s.mf.converged), "E": E}
    scf.TWO_PASS_FOCK = False
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
