"""Measurement aid: milliseconds per COLOURED sweep of a replica batch against R single engines in the coloured order swept
one after another, with the synchronous batch for scale (DESIGN.md section 4 "Coloured order in a batch").

    python3 tools/time_batch_coloured.py [--workloads q4_1e4 q4_1e5 q4_1e6 c2] [--replicas 1 4 16] [--reps 5]
                                         [--no-converge] [--out profiles/batch_coloured.json]

Workloads: planted partitions at Q = 4, c = 5, eps = 0.2, N = 1e4 / 1e5 / 1e6 (tools/time_batch.py's graphs and generator) and
Q = 2, c = 3, eps = 0.1, N = 1e6 (C2 of bench.py). Per (workload, R) it times
  (a) a batch in the coloured order: ReplicaBatch.sweep after set_sweep_order("coloured")
  (b) R single engines in the coloured order, swept one after another in this process
  (c) a second batch, same graph and seeds, in the synchronous order
(two batches, so that no order is switched and no table rebuilt between timed calls: the first launches behind fresh
allocations are slower, and with one batch switched back and forth the slope at N = 1e6, R = 1 came out negative)
and reports (b)/(a) per repetition (median, minimum, maximum: the spread), (a)/(c), and the launches per sweep of (a) and (b)
as the step tables give them. Method as tools/time_batch.py: every sweep call ends in a device synchronise, and a call also
uploads parameters and recomputes the field, so each figure is the SLOPE between a short and a long call, taken after a
warm-up call of every shape; the variants alternate inside each repetition and the median over the repetitions is kept.
Unless --no-converge is given it then converges every replica in both orders (criterion 1e-6, at most 1000 sweeps, fresh
states from the same seeds) and records the stopping sweep of each."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sbm_bp_amd as S  # noqa: E402
from sbm_bp_amd import synth  # noqa: E402

WORKLOADS = {"q4_1e4": (10_000, 4, 5.0, 0.2), "q4_1e5": (100_000, 4, 5.0, 0.2), "q4_1e6": (1_000_000, 4, 5.0, 0.2), "c2": (1_000_000, 2, 3.0, 0.1)}
N1, N2 = 10, 60
CRIT, LIMIT = 1e-6, 1000


def slope(call):
    t0 = time.perf_counter()
    call(N1)
    t1 = time.perf_counter()
    call(N2)
    t2 = time.perf_counter()
    return ((t2 - t1) - (t1 - t0)) * 1e3 / (N2 - N1)


def measure(name, R, reps, converge):
    N, Q, c, eps = WORKLOADS[name]
    pairs, cin, cout = synth.planted_partition(N, Q, c, eps, 12345)
    g = S.Graph.from_edges(pairs, N)
    tc = synth.true_conf(N, Q)
    st = S.bp_blockmodel_state(synth.cab_matrix(Q, cin, cout), np.bincount(tc, minlength=Q))
    bm = S.blockmodel_t(g, Q, 0)
    batches = {}
    for order in ("coloured", "jacobi"):
        b = S.ReplicaBatch(g, Q, 0, R)
        b.init_messages_device(tc, list(range(R)))
        b.set_params(st)
        b.set_sweep_order(order)
        batches[order] = b
    singles = []
    for r in range(R):
        bp = S.bp_conditional()
        bp.init_messages_device(bm, tc, r)
        bp.expand_bp_params(st)
        bp.set_sweep_order("coloured")
        singles.append(bp)

    def run_batch(order):
        return lambda n: batches[order].sweep(n, 1.0)

    def run_singles(n):
        for bp in singles:
            bp.sweep(n, 1.0)

    variants = [("batch_coloured", lambda: run_batch("coloured")), ("singles_coloured", lambda: run_singles), ("batch_jacobi", lambda: run_batch("jacobi"))]
    for _, make in variants:  # warm-up of every shape
        make()(N1)
        make()(N2)
    t = {k: [] for k, _ in variants}
    for _ in range(reps):
        for k, make in variants:
            t[k].append(slope(make()))
    b = batches["coloured"]
    order, n_colours, n_steps = b.sweep_order
    hubs = int(b.stats().n_hub_rows)
    out = {"workload": name, "N": N, "Q": Q, "c": c, "R": R, "E2": int(g.E2), "colours": n_colours, "steps": n_steps, "hub_rows": hubs}
    for k in t:
        med = float(np.median(t[k]))
        out[k + "_ms_per_sweep"] = med
        out[k + "_spread"] = float((max(t[k]) - min(t[k])) / med) if med > 0 else None
    ratios = [s / a for s, a in zip(t["singles_coloured"], t["batch_coloured"])]
    out["ratio_singles_over_batch"] = {"median": float(np.median(ratios)), "min": float(min(ratios)), "max": float(max(ratios))}
    out["ratio_coloured_over_jacobi_batch"] = out["batch_coloured_ms_per_sweep"] / out["batch_jacobi_ms_per_sweep"]
    # (graphs without hub rows; with them, 2 R more per step that holds one)
    out["launches_per_sweep"] = {"batch": 2 * n_steps, "singles": 2 * n_steps * R}
    if converge:
        sweeps = {}
        for order in ("coloured", "jacobi"):
            batches[order].init_messages_device(tc, list(range(R)))
            niter, _ = batches[order].converge(CRIT, LIMIT, 1.0)
            sweeps[order] = [int(x) for x in niter]
        out["niter_per_replica"] = sweeps
    for x in batches.values():
        x.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", nargs="+", default=list(WORKLOADS), choices=list(WORKLOADS))
    ap.add_argument("--replicas", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-converge", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_coloured.json"))
    args = ap.parse_args()
    S.load_library()
    rows = []
    for name in args.workloads:
        for R in args.replicas:
            try:
                rows.append(measure(name, R, args.reps, not args.no_converge))
            except S.SbmbpError as e:
                if e.code != -7:  # only "does not fit" is a result; anything else is a failure
                    raise
                rows.append({"workload": name, "R": R, "skipped": "out of memory"})
            print(json.dumps(rows[-1]), flush=True)
    out = {"graph_seed": 12345,
           "method": "slope between sweep calls of %d and %d sweeps, host clock around calls that end in a device synchronise; median of %d "
                     "alternating repetitions; niter: criterion %g, at most %d sweeps, -1 = not converged" % (N1, N2, args.reps, CRIT, LIMIT),
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
