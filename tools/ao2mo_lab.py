#!/usr/bin/env python
"""
The four-index MO transform against a transform composed from calls the library had before it.

One resident 4-fold block at n = 256 (8.66 GB), filled on the device as lam L^T L from 12 packed factor rows, and one random
orthogonal coefficient matrix.  Two workloads, timed with HIP events in one process on the same buffers:

    full    all four indices over the n orbitals       new: both PACK flags (a 4-fold block again)   baseline: unpacked
    ovov    (ov|ov) with nocc = n / 2                  new and baseline unpacked

    new        dmk_ao2mo_s4
    baseline   per slab of k: dmk_sym_unpack over a batch of packed rows, two dmk_dgemm_batched (M C4, then C3^T .) -- the ket half;
               dmk_copy_rows_f64 (rows pair(p, q) -> (p, q)), two dmk_dgemm_batched (C2^T . per p, then C1^T . over p) -- the bra half.
               It has no way to keep a pair index packed in the bra half, so it executes more flop than the new call.

Warm-up rounds, then the median of --reps repetitions of each, interleaved (new, baseline, new, ...); spread = (max - min) / median.
The first k slab of the baseline doubles as a device-side cross-check of the new kernel (the 2-norm of the difference bounds its
largest entry).  Executed TFLOP/s of the new call are the flop its launches issue to the matrix pipe (padded tiles included) over the
median time; the roof is the 78.6 TFLOP/s of tools/coissue_probe.hip.  Also the wall time of one converged RHF + MP2 at the same n.
Prints one JSON line; --out writes it to a file as well.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOF_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--base-kw", type=int, default=32, help="k slab of the composed baseline for the full transform")
    ap.add_argument("--skip-mp2", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from libdmet_preview_amd._lib import lib, get_ctx, c_vp
    from libdmet_preview_amd.solver import scf, mp
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
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d_C = ctx.to_device(q)
    col = lambda c0: c_vp(d_C.address + 8 * c0)
    idx = np.zeros((n, n), dtype=np.int32)
    idx[ti, tj] = idx[tj, ti] = np.arange(npair, dtype=np.int32)
    d_idx = ctx.to_device(idx.reshape(-1))
    o = n // 2
    RB = 1024

    def new_call(rngs, flags, out):
        args = []
        for c0, w in rngs:
            args += [col(c0), n, w]
        ctx.check(lib.dmk_ao2mo_s4(ctx.h, n, d_E.ptr, npair, *(args + [flags, 0, out.ptr])))

    def gemm(opA, opB, M, N, K, batch, A_, lda, sA, B_, ldb, sB, C_, ldc, sC):
        ctx.check(lib.dmk_dgemm_batched(ctx.h, opA, opB, M, N, K, batch, 1.0, A_, lda, sA, B_, ldb, sB, 0.0, C_, ldc, sC))

    def baseline_slab(rngs, k0, kw, buf):
        (c1, n1), (c2, n2), (c3, n3), (c4, n4) = rngs
        ncol = kw * n4
        for r0 in range(0, npair, RB):
            nr = min(RB, npair - r0)
            ctx.check(lib.dmk_sym_unpack(ctx.h, n, nr, c_vp(d_E.address + 8 * r0 * npair), None, buf["full"].ptr))
            gemm(0, 0, n, n4, n, nr, buf["full"].ptr, n, n * n, col(c4), n, 0, buf["T"].ptr, n4, n * n4)
            gemm(1, 0, kw, n4, n, nr, col(c3 + k0), n, 0, buf["T"].ptr, n4, n * n4, c_vp(buf["H"].address + 8 * r0 * ncol), n4, ncol)
        ctx.check(lib.dmk_copy_rows_f64(ctx.h, n * n, ncol, d_idx.ptr, buf["H"].ptr, buf["U"].ptr, 0))
        gemm(1, 0, n2, ncol, n, n, col(c2), n, 0, buf["U"].ptr, ncol, n * ncol, buf["W"].ptr, ncol, n2 * ncol)
        gemm(1, 0, n1, n2 * ncol, n, 1, col(c1), n, 0, buf["W"].ptr, n2 * ncol, 0, buf["out"].ptr, n2 * ncol, 0)

    def baseline_buffers(rngs, kw):
        (_, n1), (_, n2), (_, n3), (_, n4) = rngs
        ncol = kw * n4
        return {"full": ctx.empty((RB, n, n), np.float64), "T": ctx.empty((RB, n, n4), np.float64),
                "H": ctx.empty((npair, ncol), np.float64), "U": ctx.empty((n * n, ncol), np.float64),
                "W": ctx.empty((n, n2, ncol), np.float64), "out": ctx.empty((n1 * n2, ncol), np.float64)}

    def timed(f):
        ctx.timer_start()
        f()
        return ctx.timer_stop()

    def stats(v):
        v = np.asarray(v)
        med = float(np.median(v))
        return {"median_ms": med, "min_ms": float(v.min()), "max_ms": float(v.max()), "spread": float((v.max() - v.min()) / med)}

    res = {"n": n, "block_GB": 8.0 * npair * npair / 1e9, "reps": a.reps, "warmup": a.warmup, "roof_TFLOPs": ROOF_TFLOPS}
    workloads = {"full": ([(0, n)] * 4, 3, a.base_kw), "ovov": ([(0, o), (o, n - o), (0, o), (o, n - o)], 0, o)}
    for name, (rngs, flags, kw) in workloads.items():
        (_, n1), (_, n2), (_, n3), (_, n4) = rngs
        rows = n1 * (n1 + 1) // 2 if flags & 1 else n1 * n2
        cols = n3 * (n3 + 1) // 2 if flags & 2 else n3 * n4
        plan = (C.c_int64 * 3)()
        assert lib.dmk_ao2mo_plan(n, n1, n2, n3, n4, flags, 0, plan) == 0
        out_new = ctx.empty((rows, cols), np.float64)
        buf = baseline_buffers(rngs, kw)
        new = lambda: new_call(rngs, flags, out_new)

        def base():
            for k0 in range(0, n3, kw):
                baseline_slab(rngs, k0, min(kw, n3 - k0), buf)

        # cross-check on the first k slab: the new kernel, unpacked, restricted to the slab's columns of c3
        chk = ctx.empty((n1 * n2, kw * n4), np.float64)
        new_call([rngs[0], rngs[1], (rngs[2][0], kw), rngs[3]], 0, chk)
        baseline_slab(rngs, 0, kw, buf)
        d_ss = ctx.empty((1,), np.float64)
        ctx.check(lib.dmk_sub_sumsq(ctx.h, chk.size, chk.ptr, buf["out"].ptr, None, d_ss.ptr))
        diff2 = float(np.sqrt(d_ss.get()[0]))
        chk.free()
        ctx.profile_read_flops(reset=True)
        new()
        flops = ctx.profile_read_flops(reset=True)["dgemm"]
        algorithmic = npair * (2.0 * n * n * min(n3, n4) + 2.0 * n * n3 * n4) + cols * (2.0 * n * n * min(n1, n2) + 2.0 * n * n1 * n2)
        for _ in range(a.warmup):
            new()
            base()
        ctx.sync()
        t = {"new": [], "baseline": []}
        for _ in range(a.reps):
            t["new"].append(timed(new))
            t["baseline"].append(timed(base))
        # what allocating and releasing the workspace costs by itself (the call owns it for its own duration only): the same bytes
        # through dmk_malloc / dmk_free, host clock
        alloc_ms = []
        for _ in range(a.reps):
            ctx.sync()
            t0 = time.perf_counter()
            p_ws = c_vp()
            ctx.check(lib.dmk_malloc(ctx.h, int(plan[1]), C.byref(p_ws)))
            ctx.check(lib.dmk_free(ctx.h, p_ws))
            alloc_ms.append((time.perf_counter() - t0) * 1e3)
        r = {"new": stats(t["new"]), "baseline": stats(t["baseline"]), "slabs_new": int(plan[0]), "workspace_GB_new": plan[1] / 1e9,
             "new_ms_all": [round(x, 3) for x in t["new"]], "workspace_alloc_free": stats(alloc_ms),
             "workspace_alloc_free_ms_all": [round(x, 3) for x in alloc_ms],
             "norm2_difference_first_slab": diff2, "executed_TFLOP_new": flops / 1e12, "algorithmic_TFLOP_new": algorithmic / 1e12}
        r["executed_TFLOPs_new"] = flops / 1e12 / (r["new"]["median_ms"] * 1e-3)
        r["fraction_of_roof"] = r["executed_TFLOPs_new"] / ROOF_TFLOPS
        r["ratio_new_over_baseline"] = r["new"]["median_ms"] / r["baseline"]["median_ms"]
        gain = r["baseline"]["median_ms"] - r["new"]["median_ms"]
        spreads = (r["new"]["max_ms"] - r["new"]["min_ms"]) + (r["baseline"]["max_ms"] - r["baseline"]["min_ms"])
        r["faster_by_more_than_the_two_spreads"] = bool(gain > spreads)
        res[name] = r
        sys.stderr.write("%s: %s\n" % (name, json.dumps(r)))
        for b in buf.values():
            b.free()
        out_new.free()
        ctx.trim()

    if not a.skip_mp2:          # one converged RHF + MP2 at the same n
        levels = np.linspace(0.0, 1.0, n)
        levels[n // 2:] += 1.5
        q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
        h1 = sym((q2 * (levels - levels.mean())) @ q2.T)
        s = scf.SCF(newton_ah=False)
        s.set_system(n, 0, False, True)
        s.set_integral_dev(n, 0.0, ctx.to_device(h1[None]), None, [d_E])
        s.HF(tol=1e-10)
        mp.run_mp2(s)                # warm-up
        ctx.sync()
        t0 = time.perf_counter()
        E, _ = s.HF(tol=1e-10)
        ctx.sync()
        t1 = time.perf_counter()
        e_corr, rdm1 = mp.run_mp2(s)
        ctx.sync()
        t2 = time.perf_counter()
        res["rhf_mp2"] = {"hf_wall_s": t1 - t0, "mp2_wall_s": t2 - t1, "E_hf": E, "e_corr": e_corr, "trace_rdm1": float(2.0 * np.trace(rdm1[0])),
                          "converged": bool(s.mf.converged)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
