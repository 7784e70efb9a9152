"""A/B timing of the invariant step-2 planes on the table-driven kernel: pipeline.iteration on the C4 synthetic system (mesh 4x4x4,
nao 104, naux 416, nemb 136, RHF, DF blocks resident in HBM) in three modes, each in a fresh process:

    dense   DMK_ERI_INV=0: step 2 of every kL over the whole block triangle
    cold    with the cache, emptied before every timed step: every kL misses and stores its region (the price of filling)
    warm    with the cache filled by the warm-up step: every kL hits and step 2 leaves out the block rows of the region

Per mode: one warm-up step, then the best and the spread of --reps timed steps (host clock around a step that ends in a device
synchronise, profiling off), then ONE more step with the library's per-family event timers on for the zgemm_half2 kernel time
and its executed flop.  A digest of sampled ERI rows tells whether the modes computed the same numbers.

    python tools/inv_tab_ab.py [--reps 5] [--rounds 2] [--base DIR] [--out notes.txt]

--base DIR: another checkout of this repository (built), whose dense mode is timed in the same session, alternating with this
one's: the comparison base for "faster" (the child only uses pipeline.iteration and DMK_ERI_INV there).
--mode M runs one mode in this process and prints one JSON line (what the driver starts)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(mode, reps, root, workload):
    sys.path.insert(0, root)
    if mode == "dense":
        os.environ["DMK_ERI_INV"] = "0"
    else:
        os.environ.pop("DMK_ERI_INV", None)
    import numpy as np
    from libdmet_preview_amd import _lib, pipeline
    ctx = _lib.get_ctx()
    sysm = pipeline.SyntheticSystem.from_workload(ctx, workload)
    held = sysm.make_df_resident(None, 0.8)
    if held == 0:
        raise SystemExit("the DF blocks do not fit in device memory")
    nemb = sysm.nlo + sysm.nval
    npair = nemb * (nemb + 1) // 2
    eri = ctx.zeros((sysm.spin * (sysm.spin + 1) // 2, npair, npair), np.float64)

    def step():
        if mode == "cold" and sysm.eri_inv_cache is not None:
            sysm.eri_inv_cache.drop()
        eri.zero_()
        ctx.sync()
        timers = {}
        t0 = time.perf_counter()
        pipeline.iteration(ctx, sysm, eri_dev=eri, timers=timers, eri_exchange="none")
        ctx.sync()
        return time.perf_counter() - t0, timers.get("eri", 0.0)

    step()                                                   # warm-up (fills the cache in the warm mode)
    times, eri_times = zip(*[step() for _ in range(reps)])
    stats = sysm.eri_inv_cache.stats() if sysm.eri_inv_cache is not None else None
    ctx.profile(True)
    ctx.profile_read(reset=True)
    ctx.profile_read_flops(reset=True)
    step()
    prof, flops = ctx.profile_read(reset=True), ctx.profile_read_flops(reset=True)
    ctx.profile(False)
    h2_ms, h2_n = prof["zgemm_half2"]
    rows = [0, npair // 3, npair - 1]
    digest = hashlib.sha1(b"".join(eri.offset(r * npair, (npair,)).get().tobytes() for r in rows)).hexdigest()
    print(json.dumps({"mode": mode, "root": root, "step_ms": [1e3 * t for t in times], "eri_stage_ms": [1e3 * t for t in eri_times],
                      "half2_ms": h2_ms, "half2_launches": h2_n, "half2_flop": flops["zgemm_half2"],
                      "half2_tflops": flops["zgemm_half2"] / (h2_ms * 1e9) if h2_ms > 0 else None,
                      "misc_ms": prof.get("misc", (None, 0))[0], "cache": stats, "df_resident_GB": held / 1e9, "digest": digest}))


def run_child(mode, reps, root, workload, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--reps", str(reps), "--root", root,
                        "--workload", workload], capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("mode %s (%s) failed with status %d" % (mode, root, r.returncode))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("dense", "cold", "warm"))
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--rounds", type=int, default=2, help="how often the whole set of modes is repeated (fresh processes)")
    p.add_argument("--root", default=HERE)
    p.add_argument("--base", default=None)
    p.add_argument("--workload", default="C4")
    p.add_argument("--timeout", type=float, default=240.0, help="seconds per child process")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.reps < 3:
        raise SystemExit("--reps: at least 3")
    if a.mode:
        return child(a.mode, a.reps, a.root, a.workload)
    plan = ([("base dense", "dense", a.base)] if a.base else []) + [("dense", "dense", a.root), ("cold", "cold", a.root),
                                                                  ("warm", "warm", a.root)]
    runs = {}
    for _ in range(a.rounds):                                  # the modes alternate; a failing child ends the job
        for label, mode, root in plan:
            runs.setdefault(label, []).append(run_child(mode, a.reps, os.path.abspath(root), a.workload, a.timeout))
    lines = ["%s, %d round(s) of fresh processes x %d timed steps after one warm-up; ms" % (a.workload, a.rounds, a.reps),
             "%-11s %9s %9s %9s | %9s | %9s %7s %9s | %s" % ("mode", "best", "median", "worst", "eri best", "half2 ms", "TF/s", "misc ms", "cache")]
    best = {}
    for label, _, _ in plan:
        rs = runs[label]
        t = sorted(x for r in rs for x in r["step_ms"])
        e = min(x for r in rs for x in r["eri_stage_ms"])
        best[label] = t[0]
        r = min(rs, key=lambda q: q["half2_ms"])
        lines.append("%-11s %9.2f %9.2f %9.2f | %9.2f | %9.3f %7.2f %9.3f | %s"
                     % (label, t[0], t[len(t) // 2], t[-1], e, r["half2_ms"], r["half2_tflops"] or 0.0, r["misc_ms"] or 0.0,
                        json.dumps(r["cache"])))
        lines.append("%-11s per process best: %s" % ("", ", ".join("%.2f" % min(q["step_ms"]) for q in rs)))
    digests = {label: sorted(set(r["digest"] for r in runs[label])) for label in runs}
    lines.append("ERI digests: %s" % json.dumps(digests))
    lines.append("all modes bit-identical: %s" % (len(set(d for v in digests.values() for d in v)) == 1))
    ref = best.get("base dense", best["dense"])
    lines.append("against %s (%.2f ms): dense %+.2f %%, cold %+.2f %%, warm %+.2f %%"
                 % ("base dense" if a.base else "dense", ref, 100 * (best["dense"] / ref - 1), 100 * (best["cold"] / ref - 1),
                    100 * (best["warm"] / ref - 1)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n" + "\n".join(json.dumps(r) for v in runs.values() for r in v) + "\n")


if __name__ == "__main__":
    main()
