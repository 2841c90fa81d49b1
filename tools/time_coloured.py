"""Measurement aid: the coloured sweep order (sbmbp_set_sweep_order) beside the synchronous default on the bench workloads,
from the device initial state at crit 5e-6: colours, steps, host time of the plan, ms per sweep, sweeps and wall time of
converge, and the free energy both runs end on. One JSON line per workload on stdout (and appended to --out).
  python3 tools/time_coloured.py C2 C5 C4 C3 [--step_fraction 0.125] [--max_sweeps 1000] [--out profiles/coloured.json]
SBMBP_LIB selects another build of the library for the whole run (e.g. the parent commit's, for its synchronous numbers)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import sbm_bp_amd as S
from sbm_bp_amd import synth
from bench import WORKLOADS

CRIT = 5e-6


def engine(g, Q, dc, cab, N):
    bp = S.bp_conditional()
    bp.init_messages_device(S.blockmodel_t(g, Q, dc), synth.true_conf(N, Q), 1234)
    bp.expand_bp_params(S.bp_blockmodel_state(cab, np.array(synth.group_sizes(N, Q), dtype=np.uint32)))
    bp.set_schedule(1.0, 8)  # the host reads the convergence state every 8 sweeps, as bin/bp does
    return bp


def run(bp, sweeps_timed=20):
    bp.sweep(2, 1.0, want_diff=False)  # warm-up (and the first, message-gather, sweep of the synchronous order)
    torch.cuda.synchronize()
    t = time.perf_counter()
    bp.sweep(sweeps_timed, 1.0, want_diff=False)
    torch.cuda.synchronize()
    ms_sweep = (time.perf_counter() - t) * 1e3 / sweeps_timed
    return ms_sweep


def measure(wl, step_fraction, max_sweeps, jacobi_only):
    N, Q, c, eps, dc, gseed = WORKLOADS[wl]
    if wl == "C4":
        pairs, cab, _ = synth.dc_sbm_powerlaw(N, Q, c, eps, gseed)
    else:
        pairs, cin, cout = synth.planted_partition(N, Q, c, eps, gseed)
        cab = synth.cab_matrix(Q, cin, cout)
    g = S.Graph.from_edges(pairs, N)
    del pairs
    out = {"workload": wl, "N": N, "Q": Q, "dc": dc, "E2": int(g.E2), "crit": CRIT, "lib": os.path.basename(os.path.dirname(S.lib_path())) + "/" + os.path.basename(S.lib_path())}
    for order in (["jacobi"] if jacobi_only else ["jacobi", "coloured"]):
        bp = engine(g, Q, dc, cab, N)
        r = {}
        if order == "coloured":
            t = time.perf_counter()
            nc, ns, _, _ = S.coloured_plan(g, None, step_fraction)
            r["plan_host_ms"] = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            bp.set_sweep_order("coloured", None, step_fraction)
            r["set_order_ms"] = (time.perf_counter() - t) * 1e3  # plan again + segment tables + upload
            r["colours"], r["steps"], r["step_fraction"] = nc, ns, step_fraction or 0.125
        r["ms_per_sweep"] = run(bp)
        bp = engine(g, Q, dc, cab, N)  # converge from the device initial state itself
        if order == "coloured":
            bp.set_sweep_order("coloured", None, step_fraction)
        torch.cuda.synchronize()
        t = time.perf_counter()
        niter, last = bp.converge(CRIT, max_sweeps, 1.0)
        torch.cuda.synchronize()
        r["converge_wall_ms"] = (time.perf_counter() - t) * 1e3
        r["niter"], r["sweeps"], r["last_maxdiff"] = niter, int(bp.stats().sweeps), last
        r["relaxation"] = list(bp.relaxation())
        r["free_energy"] = bp.compute_free_energy()
        r["overlap"] = bp.compute_overlap()
        out[order] = r
        del bp
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="+", choices=sorted(WORKLOADS))
    ap.add_argument("--step_fraction", type=float, default=0.0)
    ap.add_argument("--max_sweeps", type=int, default=1000)
    ap.add_argument("--jacobi_only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S.load_library()
    for wl in a.workloads:
        line = json.dumps(measure(wl, a.step_fraction, a.max_sweeps, a.jacobi_only))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
