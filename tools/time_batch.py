"""Measurement aid: milliseconds per sweep of a replica batch against R single engines swept one after another, on planted
partitions at Q = 4, c = 5 (DESIGN.md "Replica batches").

    python3 tools/time_batch.py [--sizes 10000 100000 1000000] [--replicas 1 4 16] [--out profiles/batch_sweeps.json]
                                [--parent-lib PATH]

Per (N, R) it times
  (a) the batch: ReplicaBatch.sweep
  (b) R single engines with gather mode 1 (the same kernel form), swept one after another
  (c) the same with gather mode 0 (the engine's default form)
and reports (b)/(a) and (c)/(a). Every sweep call ends in a device synchronise, so the host clock around it is the time of
the work; a call also uploads parameters and initialises the field, so each figure is the SLOPE between a short and a long
call, (t(n2) - t(n1)) / (n2 - n1), taken after a warm-up call of every shape; the three variants alternate inside each
repetition and the median over the repetitions is kept, with the spread (max - min) / median beside it.
--parent-lib: a build of the parent commit's library; `python3 bench.py --gpus 1` then runs on both libraries in turn
(SBMBP_LIB), three times each, and both ms_per_step series go into the output."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sbm_bp_amd as S  # noqa: E402
from sbm_bp_amd import synth  # noqa: E402

Q, C_DEG, EPS = 4, 5.0, 0.2
N1, N2 = 20, 120


def slope(call):
    t0 = time.perf_counter()
    call(N1)
    t1 = time.perf_counter()
    call(N2)
    t2 = time.perf_counter()
    return ((t2 - t1) - (t1 - t0)) * 1e3 / (N2 - N1)


def measure(N, R, reps):
    pairs, cin, cout = synth.planted_partition(N, Q, C_DEG, EPS, 12345)
    g = S.Graph.from_edges(pairs, N)
    tc = synth.true_conf(N, Q)
    st = S.bp_blockmodel_state(synth.cab_matrix(Q, cin, cout), np.bincount(tc, minlength=Q))
    bm = S.blockmodel_t(g, Q, 0)
    b = S.ReplicaBatch(g, Q, 0, R)
    b.init_messages_device(tc, list(range(R)))
    b.set_params(st)
    singles = []
    for r in range(R):
        bp = S.bp_conditional()
        bp.init_messages_device(bm, tc, r)
        bp.expand_bp_params(st)
        singles.append(bp)

    def run_batch(n):
        b.sweep(n, 1.0)

    def run_singles(mode):
        def f(n):
            for bp in singles:
                bp.sweep(n, 1.0, want_diff=False)
        for bp in singles:
            bp.set_gather_mode(mode)
        return f

    variants = [("batch", lambda: run_batch), ("singles_gather1", lambda: run_singles(1)), ("singles_gather0", lambda: run_singles(0))]
    for _, make in variants:  # warm-up of every shape
        make()(N1)
    t = {k: [] for k, _ in variants}
    for _ in range(reps):
        for k, make in variants:
            t[k].append(slope(make()))
    out = {"N": N, "R": R, "E2": int(g.E2), "segments": int(b.stats().n_blocks)}
    for k in t:
        med = float(np.median(t[k]))
        out[k + "_ms_per_sweep"] = med
        out[k + "_spread"] = float((max(t[k]) - min(t[k])) / med) if med > 0 else None
    out["ratio_gather1_over_batch"] = out["singles_gather1_ms_per_sweep"] / out["batch_ms_per_sweep"]
    out["ratio_gather0_over_batch"] = out["singles_gather0_ms_per_sweep"] / out["batch_ms_per_sweep"]
    out["batch_ns_per_edge_msg"] = out["batch_ms_per_sweep"] * 1e6 / (R * g.E2)
    b.close()
    return out


def bench_pair(parent_lib, runs=3):
    res = {"parent": [], "this": []}
    for _ in range(runs):  # alternating
        for who, lib in (("parent", parent_lib), ("this", None)):
            env = dict(os.environ)
            if lib:
                env["SBMBP_LIB"] = lib
            else:
                env.pop("SBMBP_LIB", None)
            p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "5", "--no-cpu-baseline"],
                               capture_output=True, text=True, env=env, timeout=900)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not line:
                raise RuntimeError("bench.py failed: " + p.stderr[-2000:])
            res[who].append(json.loads(line[-1])["ms_per_step"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--replicas", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_sweeps.json"))
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    S.load_library()
    rows = []
    for N in args.sizes:
        for R in args.replicas:
            try:
                rows.append(measure(N, R, args.reps))
            except S.SbmbpError as e:
                if e.code != -7:  # only "does not fit" is a result; anything else is a failure
                    raise
                rows.append({"N": N, "R": R, "skipped": "out of memory"})
            print(json.dumps(rows[-1]), flush=True)
    out = {"workload": {"Q": Q, "c": C_DEG, "eps": EPS, "graph_seed": 12345, "kernel_form": "blockIdx.y = replica"},
           "method": "slope between sweep calls of %d and %d sweeps, host clock around calls that end in a device synchronise; median of %d alternating repetitions"
                     % (N1, N2, args.reps), "rows": rows}
    if args.parent_lib:
        out["bench_ms_per_step"] = bench_pair(args.parent_lib)
        print(json.dumps(out["bench_ms_per_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
