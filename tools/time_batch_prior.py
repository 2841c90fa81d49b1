"""Measurement aid: what per-vertex priors (sbmbp_batch_set_vertex_prior) cost a replica batch per sweep. N = 1e6, c = 10
planted partition from synth.py, R = 4 replicas, device initial state, 10 warm-up sweeps, then 50 timed sweeps: a batch has
no device timers, so the figure is the host clock's slope between a call of 10 and a call of 60 sweeps (every call ends in a
device synchronise and pays the same parameter upload). One fresh process per window, --repeats windows per configuration,
the configurations alternating inside every repeat:
  a  the library named by --parent (a build of the parent commit)
  b  this tree's library, no table
  c  this tree's library, ONE shared random positive table
  d  this tree's library, R own random positive tables
One JSON line per Q on stdout (and appended to --out): ms per sweep (all R replicas) of every window, median and spread
(max - min), bytes_per_sweep, and the three expectations of DESIGN.md section 4:
  b within a's spread of a;   d <= a * (1 + 8 Q N / bytes_per_sweep) + spread of a;   c <= d
  python3 tools/time_batch_prior.py --parent parent/libsbmbp_hip.so [--Q 4 8] [--N 1000000] [--R 4] [--repeats 5] [--out FILE]
Without --parent only b, c and d are measured. A run without a GPU fails: nothing here is an estimate."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, SHORT, TIMED, C_MEAN, EPS, GSEED = 10, 10, 50, 10.0, 0.1, 7


def window(N, Q, R, tables, pairs_file):
    """ms per sweep of one timed window on the library this process loaded; tables: "none", "shared" or "own" """
    import numpy as np
    import torch
    import sbm_bp_amd as S
    from sbm_bp_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("time_batch_prior: no GPU")
    if os.environ.get("SBMBP_LIB"):  # a build of the parent commit has no batch prior entry points: bind what it exports
        import ctypes
        from sbm_bp_amd import capi
        raw = ctypes.CDLL(S.lib_path())
        for name in [n for n in capi.SYMBOLS if not hasattr(raw, n)]:
            assert "prior" in name, name
            del capi.SYMBOLS[name]
    pairs = np.load(pairs_file)
    cin = C_MEAN * Q / ((Q - 1) * EPS + 1)  # synth.planted_partition's affinities
    cout = EPS * cin
    g = S.Graph.from_edges(pairs, N)
    del pairs
    b = S.ReplicaBatch(g, Q, 0, R)
    b.init_messages_device(synth.true_conf(N, Q), [1234 + r for r in range(R)])
    b.set_params(S.bp_blockmodel_state(synth.cab_matrix(Q, cin, cout), np.array(synth.group_sizes(N, Q), dtype=np.uint32)))
    rng = np.random.default_rng(1)
    if tables == "shared":
        b.set_vertex_prior(rng.uniform(0.25, 4.0, size=(N, Q)))
    elif tables == "own":
        for r in range(R):
            b.set_vertex_prior(rng.uniform(0.25, 4.0, size=(N, Q)), r)
    b.sweep(WARMUP, 1.0)
    t0 = time.perf_counter()
    b.sweep(SHORT, 1.0)
    t1 = time.perf_counter()
    b.sweep(SHORT + TIMED, 1.0)
    t2 = time.perf_counter()
    st = b.stats()
    assert st.sweeps == R * (WARMUP + 2 * SHORT + TIMED) and st.psi_form_sweeps == 0
    return {"ms": [((t2 - t1) - (t1 - t0)) * 1e3 / TIMED], "bytes_per_sweep": st.bytes_per_sweep, "E2": int(g.E2)}


def child(lib, N, Q, R, tables, pairs_file):
    env = dict(os.environ)
    if lib:
        env["SBMBP_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pairs_file, "--N", str(N), "--Q", str(Q), "--R", str(R), "--tables", tables],
                       env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("time_batch_prior: child failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def stat(ms):
    s = sorted(ms)
    return {"median": s[len(s) // 2], "spread": s[-1] - s[0]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--Q", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--R", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(internal) one window on the pairs in this .npy file")
    ap.add_argument("--tables", default="none", choices=["none", "shared", "own"])
    a = ap.parse_args()
    if a.child:
        print(json.dumps(window(a.N, a.Q[0], a.R, a.tables, a.child)), flush=True)
        sys.exit(0)
    import tempfile
    import numpy as np
    from sbm_bp_amd import synth
    for Q in a.Q:
        pairs, cin, cout = synth.planted_partition(a.N, Q, C_MEAN, EPS, GSEED)
        assert abs(cin - C_MEAN * Q / ((Q - 1) * EPS + 1)) < 1e-12 and abs(cout - EPS * cin) < 1e-12
        tmp = tempfile.NamedTemporaryFile(suffix=".npy", delete=False)
        tmp.close()
        np.save(tmp.name, pairs)
        del pairs
        runs = {"a": [], "b": [], "c": [], "d": []}
        info = {}
        for _ in range(a.repeats):
            for key, lib, tables in (("a", a.parent, "none"), ("b", None, "none"), ("c", None, "shared"), ("d", None, "own")):
                if key == "a" and not a.parent:
                    continue
                r = child(lib, a.N, Q, a.R, tables, tmp.name)
                runs[key] += r["ms"]
                info[key] = r
                print("# Q %d %s %.4f ms" % (Q, key, r["ms"][0]), file=sys.stderr, flush=True)
        os.unlink(tmp.name)
        out = {"N": a.N, "Q": Q, "R": a.R, "c": C_MEAN, "E2": info["b"]["E2"], "warmup": WARMUP, "timed": TIMED, "repeats": a.repeats}
        for key in runs:
            if runs[key]:
                out[key] = dict(stat(runs[key]), ms=runs[key], bytes_per_sweep=info[key]["bytes_per_sweep"])
        share = out["d"]["bytes_per_sweep"] / out["b"]["bytes_per_sweep"] - 1.0
        out["added_byte_share"] = share
        out["c_at_most_d"] = out["c"]["median"] <= out["d"]["median"]
        if runs["a"]:
            bound = out["a"]["median"] * (1.0 + share) + out["a"]["spread"]
            out["bound_ms"], out["d_within_bound"] = bound, out["d"]["median"] <= bound
            out["b_equals_a"] = abs(out["b"]["median"] - out["a"]["median"]) <= out["a"]["spread"]
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
