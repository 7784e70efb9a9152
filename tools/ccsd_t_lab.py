#!/usr/bin/env python
"""
The perturbative triples of restricted CCSD (dmk_rccsd_t) against the same energy composed from what the library had
before it: strided copies, dmk_dgemm_batched and a plain elementwise combine.

Operands: random blocks (ia|bc), (ia|jk), (ia|jb) = (jb|ia), a Fock matrix with a gap of 2 and random f_ov, random symmetric
amplitudes of scale 0.1 / sqrt(o v); the handle's other blocks are zero and never read.

    new        dmk_rccsd_t with a workspace budget of --budget-gb
    composed   ONCE, outside the timed region: (ia|jm) copied to [a][i][j][m] and t2 to [b][c][m][k].  Timed, in a host loop over the
               pairs a >= b with every c <= b as the batch: per permutation of (a, b, c) one dmk_dgemm_batched for the particle term
               (M = o, N = o^2, K = v) and one for the hole term (M = o^2, N = o, K = o), each added into W[c][i][j][k] through a
               permuted view (a strided device add, torch), then V, r3, the division, the multiplicity and the sum as elementwise
               device operations (torch), accumulated into one device scalar.  No host read-back inside the loop.

Warm-up rounds, then --reps repetitions of each, interleaved (new, composed, new, ...), timed with HIP events on the context's stream
(the legacy default stream, which orders torch's work too); medians, spread = (max - min) / median.  TFLOP/s: the algorithmic
2 o^3 v^3 (o + v) flop over the median time, against the 78.6 TFLOP/s roof of tools/coissue_probe.hip; for the new path also the flop
its launches issue to the matrix pipe (unique triples only, padded tiles and K chunks included).  Prints one JSON line per shape;
--out appends them to a file.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOF_TFLOPS = 78.6
PERMS = list(itertools.permutations(range(3)))


def run_shape(o, v, reps, warmup, budget_gb, with_composed):
    import torch
    from libdmet_preview_amd._lib import lib, get_ctx, c_vp, c_dbl
    ctx = get_ctx()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 * o + v)
    f64 = torch.float64
    rnd = lambda *s: torch.randn(*s, dtype=f64, device=dev, generator=gen)
    n = o + v
    ovvv, ovoo = rnd(o, v, v, v) / v, rnd(o, v, o, o) / v
    ovov = rnd(o * v, o * v) / v
    ovov = (0.5 * (ovov + ovov.T)).reshape(o, v, o, v).contiguous()
    scale = 0.1 / np.sqrt(o * v)
    t1 = scale * rnd(o, v)
    t2 = scale * rnd(o, o, v, v)
    t2 = (0.5 * (t2 + t2.permute(1, 0, 3, 2))).contiguous()
    fock = 0.01 * rnd(n, n)
    fock = 0.5 * (fock + fock.T)
    lev = torch.cat([-1.0 - torch.rand(o, dtype=f64, device=dev, generator=gen), 1.0 + torch.rand(v, dtype=f64, device=dev, generator=gen)])
    fock = (fock - torch.diag(torch.diag(fock)) + torch.diag(lev)).contiguous()
    npair = v * (v + 1) // 2
    zero = {"oooo": torch.zeros(o ** 4, dtype=f64, device=dev), "oovv": torch.zeros(o * o * v * v, dtype=f64, device=dev),
            "ovvo": torch.zeros(o * o * v * v, dtype=f64, device=dev), "vvvv": torch.zeros(npair * npair, dtype=f64, device=dev)}
    ptr = lambda x, off=0: c_vp(x.data_ptr() + 8 * off)
    torch.cuda.synchronize()
    h = c_vp()
    ctx.check(lib.dmk_rccsd_create(ctx.h, o, v, ptr(fock), ptr(zero["oooo"]), ptr(ovoo), ptr(ovov), ptr(zero["oovv"]), ptr(zero["ovvo"]),
                                   ptr(ovvv), ptr(zero["vvvv"]), npair, 0, C.byref(h)))
    ctx.check(lib.dmk_rccsd_set(h, ptr(t1), ptr(t2)))
    budget = int(budget_gb * (1 << 30))
    res = (c_dbl * 2)()

    def new():
        ctx.check(lib.dmk_rccsd_t(h, budget, res))
        return float(res[0])

    # ---- the composed path ----------------------------------------------------------------------------------------------------------
    o2, o3, v2, v3 = o * o, o ** 3, v * v, v ** 3
    fov, eo, ev = fock[:o, o:].contiguous(), lev[:o], lev[o:]
    eijk = eo[:, None, None] + eo[None, :, None] + eo[None, None, :]
    if with_composed:
        ovoo_a = ovoo.permute(1, 0, 2, 3).contiguous()          # [a][i][j][m]
        t2T = t2.permute(2, 3, 0, 1).contiguous()               # [b][c][m][k]
        Wb = torch.empty(v, o, o, o, dtype=f64, device=dev)
        Cp, Ch = torch.empty(v, o, o2, dtype=f64, device=dev), torch.empty(v, o2, o, dtype=f64, device=dev)

    def gemm(M, N, K, batch, alpha, A, lda, sa, opB, B, ldb, sb, Cm, ldc):
        ctx.check(lib.dmk_dgemm_batched(ctx.h, 0, opB, M, N, K, batch, alpha, A, lda, sa, B, ldb, sb, 0.0, ptr(Cm), ldc, o3))

    def composed():
        e = torch.zeros((), dtype=f64, device=dev)
        for a in range(v):
            for b in range(a + 1):
                nb = b + 1
                x = (a, b, None)
                W = Wb[:nb]
                for q, p in enumerate(PERMS):
                    X, Y, Z = x[p[0]], x[p[1]], x[p[2]]                    # None: the batch index c
                    z = lambda t: 0 if t is None else t
                    # particle: Cp[c][p][(r, q)] = sum_f (pX|Yf) t_rq^Zf
                    gemm(o, o2, v, nb, 1.0, ptr(ovvv, z(X) * v2 + z(Y) * v), v3, v2 if X is None else (v if Y is None else 0),
                         1, ptr(t2, z(Z) * v), v2, v if Z is None else 0, Cp, o2)
                    # hole: Ch[c][(p, q)][r] = - sum_m (pX|qm) t_mr^YZ
                    gemm(o2, o, o, nb, -1.0, ptr(ovoo_a, z(X) * o3), o, o3 if X is None else 0,
                         0, ptr(t2T, (z(Y) * v + z(Z)) * o2), o, v * o2 if Y is None else (o2 if Z is None else 0), Ch, o)
                    Wv = W.permute(0, 1 + p[0], 1 + p[1], 1 + p[2])      # dims (c, p, q, r)
                    if q == 0:
                        Wv.copy_(Ch[:nb].view(nb, o, o, o))
                    else:
                        Wv.add_(Ch[:nb].view(nb, o, o, o))
                    Wv.add_(Cp[:nb].view(nb, o, o, o).permute(0, 1, 3, 2))
                # V = W + 1/2 P6[(ia|jb) t_kc + t_ij^ab f_kc], c the batch
                Xs = torch.zeros_like(W)
                g_ab, t_ab = ovov[:, a, :, b], t2[:, :, a, b]                                      # (i, j)
                g_ac, t_ac = ovov[:, a, :, :nb].permute(2, 0, 1), t2[:, :, a, :nb].permute(2, 0, 1)  # (c, i, k)
                g_bc, t_bc = ovov[:, b, :, :nb].permute(2, 0, 1), t2[:, :, b, :nb].permute(2, 0, 1)  # (c, j, k)
                t1c, fc = t1[:, :nb].T, fov[:, :nb].T                                              # (c, k)
                gs, ts = g_ab + ovov[:, b, :, a].T, t_ab + t2[:, :, b, a].T
                Xs += gs[None, :, :, None] * t1c[:, None, None, :] + ts[None, :, :, None] * fc[:, None, None, :]
                # pairs (i, a), (k, c) in both orders, the third pair (j, b)
                gs, ts = g_ac + ovov[:, :nb, :, a].permute(1, 2, 0), t_ac + t2[:, :, :nb, a].permute(2, 1, 0)
                Xs += gs[:, :, None, :] * t1[None, None, :, b, None] + ts[:, :, None, :] * fov[None, None, :, b, None]
                # pairs (j, b), (k, c) in both orders, the third pair (i, a)
                gs, ts = g_bc + ovov[:, :nb, :, b].permute(1, 2, 0), t_bc + t2[:, :, :nb, b].permute(2, 1, 0)
                Xs += gs[:, None, :, :] * t1[None, :, a, None, None] + ts[:, None, :, :] * fov[None, :, a, None, None]
                r3 = (4.0 * W + W.permute(0, 2, 3, 1) + W.permute(0, 3, 1, 2)
                      - 2.0 * (W.permute(0, 3, 2, 1) + W.permute(0, 1, 3, 2) + W.permute(0, 2, 1, 3)))
                D = eijk[None] - (ev[a] + ev[b] + ev[:nb])[:, None, None, None]
                y = (r3 * (W + 0.5 * Xs) / D).sum(dim=(1, 2, 3))
                mult = torch.full((nb,), 1.0 if a == b else 2.0, dtype=f64, device=dev)
                mult[b] = 1.0 / 3.0 if a == b else 1.0
                e += (mult * y).sum()
        return float(e)

    def timed(f):
        ctx.timer_start()
        val = f()
        return ctx.timer_stop(), val

    def stats(xs):
        xs = np.asarray(xs)
        med = float(np.median(xs))
        return {"median_ms": med, "min_ms": float(xs.min()), "max_ms": float(xs.max()), "spread": float((xs.max() - xs.min()) / med)}

    ctx.profile_read_flops(reset=True)
    e_new = new()
    executed = ctx.profile_read_flops(reset=True)["dgemm"]
    batches = int(res[1])
    paths = [("new", new)] + ([("composed", composed)] if with_composed else [])
    e_comp = composed() if with_composed else None
    for _ in range(max(warmup - 1, 0)):
        for _, f in paths:
            f()
    ctx.sync()
    t = {k: [] for k, _ in paths}
    for _ in range(reps):
        for k, f in paths:
            t[k].append(timed(f)[0])
    algorithmic = 2.0 * float(o) ** 3 * float(v) ** 3 * (o + v)
    out = {"nocc": o, "nvir": v, "unique_triples": v * (v + 1) * (v + 2) // 6, "batches": batches, "budget_GB": budget_gb, "reps": reps,
           "warmup": warmup, "roof_TFLOPs": ROOF_TFLOPS, "algorithmic_TFLOP": algorithmic / 1e12, "executed_TFLOP_new": executed / 1e12,
           "e_t_new": e_new, "e_t_composed": e_comp}
    for k, _ in paths:
        out[k] = stats(t[k])
        out[k]["ms_all"] = [round(x, 3) for x in t[k]]
        out[k]["algorithmic_TFLOPs"] = algorithmic / 1e12 / (out[k]["median_ms"] * 1e-3)
        out[k]["fraction_of_roof"] = out[k]["algorithmic_TFLOPs"] / ROOF_TFLOPS
    out["new"]["executed_TFLOPs"] = executed / 1e12 / (out["new"]["median_ms"] * 1e-3)
    if with_composed:
        out["ratio_new_over_composed"] = out["new"]["median_ms"] / out["composed"]["median_ms"]
        out["energy_difference"] = e_new - e_comp
        out["energy_relative_difference"] = abs(e_new - e_comp) / abs(e_comp)
    lib.dmk_rccsd_free(h)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x96,64x192", help="comma-separated nocc x nvir")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--budget-gb", type=float, default=8.0)
    ap.add_argument("--no-composed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for s in a.shapes.split(","):
        o, v = (int(x) for x in s.split("x"))
        line = json.dumps(run_shape(o, v, a.reps, a.warmup, a.budget_gb, not a.no_composed))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
