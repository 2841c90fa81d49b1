"""Measurement aid: wall time of multi-start EM as one replica batch against R single engines learning one after another, on
planted partitions at Q = 4, c = 5 with the initial cab off the planted values (DESIGN.md "Replica batches").

    python3 tools/time_batch_learn.py [--sizes 10000 100000 1000000] [--replicas 1 4 16] [--reps 3]
                                      [--out profiles/batch_learn.json] [--parent-tree DIR]

Per (N, R) it times, from the same R initial states and parameters,
  (a) ReplicaBatch.learning                                   (sbmbp_batch_learning)
  (b) R single engines with gather mode 1, one after another  (the same kernel form: isolates the batching)
  (c) the same with gather mode 0                             (the engine's default form)
and reports (b)/(a) and (c)/(a) with the EM steps and sweeps each variant took. A learning call ends in a device
synchronise, so the host clock around it is the time of the work; the states are put back before every call, outside the
clock; the three variants alternate inside each repetition after one warm-up call of each, and the median over the
repetitions is kept with the spread (max - min) / median beside it.
Every (N, R) point runs in a process of its own under a time limit, and so does every bench.py run of --parent-tree (a built
checkout of the parent commit, whose library does not have this commit's entry points: `python3 bench.py --gpus 1` then runs
in that checkout and in this one in turn, three times each). The points are chained: after a point that fails or runs out
of time nothing more is started."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q, C_DEG, EPS = 4, 5.0, 0.2
LCRIT, TMAX, LR, DAMP = 1e-6, 100, 0.2, 1.0
POINT_LIMIT_S, BENCH_LIMIT_S = 420, 300


def measure(N, R, reps):
    import sbm_bp_amd as S
    from sbm_bp_amd import synth
    S.load_library()
    pairs, cin, cout = synth.planted_partition(N, Q, C_DEG, EPS, 12345)
    g = S.Graph.from_edges(pairs, N)
    tc = synth.true_conf(N, Q)
    start = S.bp_blockmodel_state(synth.cab_matrix(Q, 0.9 * cin, 1.8 * cout), np.bincount(tc, minlength=Q))
    bm = S.blockmodel_t(g, Q, 0)
    seeds = list(range(R))
    b = S.ReplicaBatch(g, Q, 0, R)
    singles = []
    for r in range(R):
        bp = S.bp_basic()
        bp.init_messages_device(bm, tc, seeds[r])
        singles.append(bp)

    def run_batch():
        b.init_messages_device(tc, seeds)
        b.set_params(start)
        t0 = time.perf_counter()
        res, _, _, _ = b.learning(LCRIT, TMAX, LR, DAMP)
        dt = time.perf_counter() - t0
        return dt, [x.em_steps for x in res], [int(x.total_sweeps) for x in res], [x.free_energy for x in res]

    def run_singles(mode):
        dt, steps, sweeps, fs = 0.0, [], [], []
        for r, bp in enumerate(singles):
            bp.reinit_messages_device(tc, seeds[r])
            bp.set_gather_mode(mode)
            t0 = time.perf_counter()
            res = bp.learning(bm, start, LCRIT, TMAX, LR, DAMP)
            dt += time.perf_counter() - t0
            steps.append(res.em_steps)
            sweeps.append(int(res.total_sweeps))
            fs.append(res.free_energy)
        return dt, steps, sweeps, fs

    variants = [("batch", run_batch), ("singles_gather1", lambda: run_singles(1)), ("singles_gather0", lambda: run_singles(0))]
    for _, f in variants:  # warm-up of every shape
        f()
    t = {k: [] for k, _ in variants}
    info = {}
    for _ in range(reps):
        for k, f in variants:
            dt, steps, sweeps, fs = f()
            t[k].append(dt * 1e3)
            info[k] = (steps, sweeps, fs)
    out = {"N": N, "R": R, "E2": int(g.E2), "segments": int(b.stats().n_blocks)}
    for k in t:
        med = float(np.median(t[k]))
        out[k + "_ms"] = med
        out[k + "_spread"] = float((max(t[k]) - min(t[k])) / med) if med > 0 else None
        out[k + "_em_steps"] = info[k][0]
        out[k + "_sweeps"] = int(sum(info[k][1]))
    out["ratio_gather1_over_batch"] = out["singles_gather1_ms"] / out["batch_ms"]
    out["ratio_gather0_over_batch"] = out["singles_gather0_ms"] / out["batch_ms"]
    out["max_free_energy_difference_batch_vs_gather1"] = float(np.abs(np.array(info["batch"][2]) - np.array(info["singles_gather1"][2])).max())
    b.close()
    return out


def bench_once(tree):
    env = dict(os.environ)
    env.pop("SBMBP_LIB", None)
    p = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "50", "--warmup", "5", "--no-cpu-baseline"],
                       capture_output=True, text=True, env=env, cwd=tree, timeout=BENCH_LIMIT_S)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not line:
        raise RuntimeError("bench.py failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    return json.loads(line[-1])["ms_per_step"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--replicas", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_learn.json"))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--point", type=int, nargs=2, default=None, help="(internal) measure one (N, R) point in this process")
    args = ap.parse_args()
    if args.point:
        print(json.dumps(measure(args.point[0], args.point[1], args.reps)), flush=True)
        return 0
    out = {"workload": {"Q": Q, "c": C_DEG, "eps": EPS, "graph_seed": 12345, "start": "cab = (0.9 cin, 1.8 cout)", "learning_conv_crit": LCRIT,
                        "learning_max_time": TMAX, "learning_rate": LR},
           "method": "host clock around learning calls that end in a device synchronise; states put back outside the clock; median of %d alternating "
                     "repetitions after one warm-up of each variant; every point in its own process" % args.reps,
           "rows": []}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    for N in args.sizes:
        for R in args.replicas:
            cmd = [sys.executable, os.path.abspath(__file__), "--point", str(N), str(R), "--reps", str(args.reps)]
            try:
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=POINT_LIMIT_S)
            except subprocess.TimeoutExpired:
                print("point N=%d R=%d ran out of time: nothing more is started" % (N, R), flush=True)
                save()
                return 1
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not line:
                print("point N=%d R=%d failed (%d): nothing more is started\n%s" % (N, R, p.returncode, p.stderr[-2000:]), flush=True)
                save()
                return 1
            out["rows"].append(json.loads(line[-1]))
            print(line[-1], flush=True)
            save()
    if args.parent_tree:
        res = {"parent": [], "this": []}
        for _ in range(3):  # alternating
            for who, tree in (("parent", os.path.abspath(args.parent_tree)), ("this", ROOT)):
                res[who].append(bench_once(tree))
        out["bench_ms_per_step"] = res
        print(json.dumps(res), flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
