"""Measurement aid: what a per-vertex prior (sbmbp_set_vertex_prior) costs per sweep. N = 1e6, c = 10 planted partition from
synth.py, device initial state, message-gather sweeps timed with device events (set_timing): 10 warm-up sweeps, then
--repeats windows of 50 sweeps per configuration, the configurations alternating inside every repeat:
  a  the library named by --parent (a build of the parent commit), set_gather_mode(1)   [own process: one library each]
  b  this tree's library, no prior, set_gather_mode(1)
  c  this tree's library, a random positive prior on every row
One JSON line per Q on stdout (and appended to --out): ms per sweep of every window, median and spread (max - min over the
repeats), bytes_per_sweep, and the acceptance bound  c <= a * (1 + added-byte share) + spread of a.
  python3 tools/time_prior.py --parent parent/libsbmbp_hip.so [--Q 4 8] [--N 1000000] [--repeats 5] [--out profiles/prior.json]
Without --parent only b and c are measured. A run without a GPU fails: nothing here is an estimate."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, TIMED, C_MEAN, EPS, GSEED = 10, 50, 10.0, 0.1, 7


def windows(N, Q, prior, repeats, pairs_file):
    """ms per sweep of `repeats` timed windows on the library this process loaded"""
    import numpy as np
    import torch
    import sbm_bp_amd as S
    from sbm_bp_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("time_prior: no GPU")
    if os.environ.get("SBMBP_LIB"):  # a build of the parent commit has no prior entry points: bind what it exports
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
    bp = S.bp_conditional()
    bp.init_messages_device(S.blockmodel_t(g, Q, 0), synth.true_conf(N, Q), 1234)
    bp.expand_bp_params(S.bp_blockmodel_state(synth.cab_matrix(Q, cin, cout), np.array(synth.group_sizes(N, Q), dtype=np.uint32)))
    bp.set_gather_mode(1)
    if prior:
        bp.set_vertex_prior(np.random.default_rng(1).uniform(0.25, 4.0, size=(N, Q)))
    bp.sweep(WARMUP, 1.0, want_diff=False)
    bp.set_timing(True)
    out = []
    for _ in range(repeats):
        bp.reset_stats()
        bp.sweep(TIMED, 1.0, want_diff=False)
        st = bp.stats()
        assert st.sweeps == TIMED and st.psi_form_sweeps == 0
        out.append(st.sweep_kernel_ms / TIMED)
    return {"ms": out, "bytes_per_sweep": bp.stats().bytes_per_sweep, "E2": int(g.E2)}


def child(lib, N, Q, prior, repeats, pairs_file):
    env = dict(os.environ)
    if lib:
        env["SBMBP_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", pairs_file, "--N", str(N), "--Q", str(Q), "--repeats", str(repeats)]
                       + (["--prior"] if prior else []), env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("time_prior: child failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def stat(ms):
    s = sorted(ms)
    return {"median": s[len(s) // 2], "spread": s[-1] - s[0]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--Q", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(internal) one configuration on the pairs in this .npy file")
    ap.add_argument("--prior", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(windows(a.N, a.Q[0], a.prior, a.repeats, a.child)), flush=True)
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
        # one window per configuration and repeat, the configurations alternating (other work shares the machine)
        runs = {"a": [], "b": [], "c": []}
        info = {}
        for _ in range(a.repeats):
            for key, lib, prior in (("a", a.parent, False), ("b", None, False), ("c", None, True)):
                if key == "a" and not a.parent:
                    continue
                r = child(lib, a.N, Q, prior, 1, tmp.name)
                runs[key] += r["ms"]
                info[key] = r
        os.unlink(tmp.name)
        out = {"N": a.N, "Q": Q, "c": C_MEAN, "E2": info["b"]["E2"], "warmup": WARMUP, "timed": TIMED, "repeats": a.repeats}
        for key in runs:
            if runs[key]:
                out[key] = dict(stat(runs[key]), ms=runs[key], bytes_per_sweep=info[key]["bytes_per_sweep"])
        share = out["c"]["bytes_per_sweep"] / out["b"]["bytes_per_sweep"] - 1.0
        out["added_byte_share"] = share
        if runs["a"]:
            bound = out["a"]["median"] * (1.0 + share) + out["a"]["spread"]
            out["bound_ms"], out["within_bound"] = bound, out["c"]["median"] <= bound
        line = json.dumps(out)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
