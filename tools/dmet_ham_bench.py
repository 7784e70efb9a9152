#!/usr/bin/env python
"""
tools/dmet_ham_bench.py -- timings of the code behind the solver at production size (profiles/dmet_ham_notes.txt).
Run it in a fresh process on the GPU:

    python tools/dmet_ham_bench.py [--n 256] [--reps 12] [--skip-rho]

1. dmk_dmet_h2_scaled at n = 256 (one spin block, 8.66 GB in 4-fold storage): 4 -> 4 out of place, 4 -> 4 in place, 4 -> 1,
   each against a device-to-device copy that moves the same number of bytes (read + written), taken in the same run with the
   variants alternating.  HIP events around each call; 3 warm-up rounds.  The kernel passes if its median stays within the
   copy's own spread ((max - min) / median over the repetitions) plus 10 %.
2. The democratic global density at C5 size (mesh 6 x 6 x 6, nlo 200, neo 256, two spins): dmk_rho_glob (HIP events), the whole
   get_rho_glob_R call from host arrays (wall clock), and the reference's loop over cells restated in numpy
   (tests/dmet_ham_ref.rho_glob_R) timed on 4 of the 216 cells and EXTRAPOLATED by the cell count.
One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    ms = sorted(ms)
    med = ms[len(ms) // 2]
    return {"median_ms": med, "min_ms": ms[0], "max_ms": ms[-1], "spread": (ms[-1] - ms[0]) / med}


def bench_scaling(ctx, lib, n, reps):
    npair, nn = n * (n + 1) // 2, n * n
    b4, b1 = npair * npair * 8, nn * nn * 8
    imp = np.arange(n // 2, dtype=np.int32)
    d_in, d_out4 = ctx.empty((npair * npair,), np.float64), ctx.empty((npair * npair,), np.float64)
    d_out1 = ctx.empty((nn * nn,), np.float64)
    half = (b4 + b1) // 2 // 8                       # a copy of this many doubles moves what the 4 -> 1 form moves
    d_scr = ctx.empty((half,), np.float64)
    # finite, bounded content: one period uploaded, doubled by device copies
    period = 1 << 20
    d_in.offset(0, (period,)).set(np.random.default_rng(0).standard_normal(period))
    have = period
    while have < npair * npair:
        m = min(have, npair * npair - have)
        ctx.check(lib.dmk_memcpy_d2d(ctx.h, d_in.offset(have, (m,)).ptr, d_in.ptr, m * 8))
        have += m
    d_out1.zero_()

    def scaled(d_i, d_o, out_sym):
        return lambda: ctx.check(lib.dmk_dmet_h2_scaled(ctx.h, n, imp.ctypes.data, imp.size, 4, d_i.ptr, npair, out_sym, d_o.ptr,
                                                        npair if out_sym == 4 else nn))
    variants = [
        ("copy_4fold_bytes", lambda: ctx.check(lib.dmk_memcpy_d2d(ctx.h, d_out4.ptr, d_in.ptr, b4)), 2 * b4),
        ("scaled_4to4", scaled(d_in, d_out4, 4), 2 * b4),
        ("scaled_4to4_inplace", scaled(d_in, d_in, 4), 2 * b4),
        ("copy_4to1_bytes", lambda: ctx.check(lib.dmk_memcpy_d2d(ctx.h, d_scr.ptr, d_out1.ptr, half * 8)), 2 * half * 8),
        ("scaled_4to1", scaled(d_in, d_out1, 1), b4 + b1),
    ]
    times = {name: [] for name, _, _ in variants}
    for it in range(3 + reps):
        for name, fn, _ in variants:
            ctx.sync()
            ctx.timer_start()
            fn()
            ms = ctx.timer_stop()
            if it >= 3:
                times[name].append(ms)
    res = {}
    for name, _, nbytes in variants:
        res[name] = dict(stats(times[name]), bytes_moved=nbytes)
        res[name]["TB_per_s"] = nbytes / res[name]["median_ms"] / 1e9
    for kern, base in (("scaled_4to4", "copy_4fold_bytes"), ("scaled_4to4_inplace", "copy_4fold_bytes"), ("scaled_4to1", "copy_4to1_bytes")):
        bound = res[base]["median_ms"] * (1.0 + res[base]["spread"] + 0.10)
        res[kern]["vs_copy"] = res[kern]["median_ms"] / res[base]["median_ms"]
        res[kern]["bound_ms"] = bound
        res[kern]["within_bound"] = bool(res[kern]["median_ms"] <= bound)
    for name, _, _ in variants:
        print(json.dumps(dict(res[name], what=name, n=n, reps=reps)), flush=True)
    for d in (d_in, d_out4, d_out1, d_scr):
        d.free()
    ctx.trim()


def bench_rho(ctx, lib, reps):
    from libdmet_preview_amd._lib import mesh3
    from libdmet_preview_amd.system.lattice import Lattice
    from libdmet_preview_amd.routine import slater_helper as sh
    from tests import dmet_ham_ref as ref
    mesh, nlo, neo, spin = (6, 6, 6), 200, 256, 2
    nc = 216
    rng = np.random.default_rng(17)
    basis = rng.standard_normal((spin, nc, nlo, neo)) / np.sqrt(nc * nlo)
    rho = rng.standard_normal((spin, neo, neo))
    rho = 0.5 * (rho + rho.transpose(0, 2, 1))
    imp = np.arange(nlo, dtype=np.int32)
    L = Lattice(nlo, mesh)
    L.set_val_virt_core(list(range(nlo)), [], [])
    d_b, d_r, d_o = ctx.to_device(basis), ctx.to_device(rho), ctx.empty((spin, nc, nlo, nlo), np.float64)
    ms = []
    for it in range(2 + reps):
        ctx.sync()
        ctx.timer_start()
        ctx.check(lib.dmk_rho_glob(ctx.h, mesh3(mesh), nlo, neo, spin, d_b.ptr, d_r.ptr, imp.ctypes.data, nlo, d_o.ptr))
        t = ctx.timer_stop()
        if it >= 2:
            ms.append(t)
    print(json.dumps(dict(stats(ms), what="dmk_rho_glob_C5", mesh=mesh, nlo=nlo, neo=neo, spin=spin)), flush=True)
    wall = []
    for it in range(3):
        t0 = time.perf_counter()
        got = sh.get_rho_glob_R(basis, L, rho)
        wall.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"what": "get_rho_glob_R_C5_host_to_host", "wall_ms": wall}), flush=True)
    sub = ref.mesh_subtract(mesh)
    cells = [0, 1, 7, 215]
    ref.rho_glob_R(basis, sub, imp, rho, cells=[0])          # warm the BLAS threads
    t0 = time.perf_counter()
    part = ref.rho_glob_R(basis, sub, imp, rho, cells=cells)
    t_np = time.perf_counter() - t0
    print(json.dumps({"what": "numpy_cell_loop_C5", "cells_timed": len(cells), "seconds_timed": t_np,
                      "seconds_extrapolated_216_cells": t_np / len(cells) * nc, "extrapolated": True,
                      "threads": os.environ.get("OMP_NUM_THREADS")}), flush=True)
    # the partial loop against the device result restricted to what those cells contribute would need the full loop; the full
    # comparison is the GPU test's job (tests/test_gpu_dmet_ham.py) -- here only a sanity figure on cell 0's block
    print(json.dumps({"what": "sanity", "device_max_abs": float(np.abs(got).max()), "partial_loop_max_abs": float(np.abs(part).max())}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--skip-rho", action="store_true")
    ap.add_argument("--skip-scaling", action="store_true")
    args = ap.parse_args()
    from libdmet_preview_amd import _lib
    ctx = _lib.get_ctx()
    if not args.skip_scaling:
        bench_scaling(ctx, _lib.lib, args.n, args.reps)
    if not args.skip_rho:
        bench_rho(ctx, _lib.lib, args.reps)


if __name__ == "__main__":
    main()
