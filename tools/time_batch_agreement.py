"""Measurement aid: what one sbmbp_batch_agreement costs, against the byte floor and against the only route there was before it.
Sizes: N = 1e6 and 1e7 with (Q, R) = (4, 8) and (16, 16), all R replicas in the call. The call reads marginals only, so the graph
is a ring on the first 1024 vertices with the rest isolated (the message buffers stay small) and the states are the device
initialisation's random marginals.
Per size, one JSON line on stdout (and appended to --out, default profiles/batch_agreement.json):
  agreement_ms[kind]  median / min / max of --repeats calls after --warmup calls. A batch keeps its stream to itself, so no
                      event of the caller's can bracket its launches: the figure is the host clock around the call, which ends in
                      a device synchronise. It therefore contains the launches, the n n Q Q copy and the O(n^2 Q^3) assignment on
                      the host as well: an upper bound of the kernel time, and what a caller waits for.
  floor_ms            N n Q 8 bytes at 8 TB/s;  floor_fraction[kind] = floor_ms / median. Recorded, not judged: at CP = 256 the
                      matrix cores bound the call, not HBM ("Agreement of replicas").
  download_ms         the parent commit's route, first part: R calls of sbmbp_batch_get_state (marginals only), host clock, summed
  numpy_ms            its second part: the Gram matrix of the R tables in numpy (float64 matmul), where the tables fit --host_gb;
                      null above
  faster_than_download[kind]  the one condition: the call takes less time than the download alone
  python3 tools/time_batch_agreement.py [--sizes 1000000 10000000] [--repeats 7] [--warmup 3] [--host_gb 8] [--out FILE]
A run without a GPU fails: nothing here is an estimate."""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("soft", "hard_soft", "hard")
HBM_BYTES_PER_S = 8.0e12
RING = 1024


def median(xs):
    s = sorted(xs)
    return s[len(s) // 2]


def measure(N, Q, R, repeats, warmup, host_gb):
    import numpy as np
    import sbm_bp_amd as S
    ring = np.stack([np.arange(RING), (np.arange(RING) + 1) % RING], 1).astype(np.uint32)
    g = S.Graph.from_edges(ring, N)
    b = S.ReplicaBatch(g, Q, 0, R)
    b.init_messages_device((np.arange(N) % Q).astype(np.uint32), [1234 + r for r in range(R)])
    out = {"N": N, "Q": Q, "R": R, "columns": R * Q, "repeats": repeats, "warmup": warmup, "agreement_ms": {}, "floor_fraction": {},
           "faster_than_download": {}}
    floor_ms = N * R * Q * 8 / HBM_BYTES_PER_S * 1e3
    out["floor_ms"] = floor_ms
    results = {}
    for kind in KINDS:
        for _ in range(warmup):
            b.agreement(kind)
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            results[kind] = b.agreement(kind)
            ms.append((time.perf_counter() - t0) * 1e3)
        out["agreement_ms"][kind] = {"median": median(ms), "min": min(ms), "max": max(ms)}
        out["floor_fraction"][kind] = floor_ms / median(ms)
    # the route of the parent commit: R downloads, then a product on the host
    keep = N * R * Q * 8 <= host_gb * 2 ** 30
    psi = np.zeros((N, Q))
    table = np.zeros((N, R * Q)) if keep else None
    lib = S.load_library()
    down = []
    for rep in range(2):  # the first pass faults the pages of the destination in; the second is the figure
        total = 0.0
        for r in range(R):
            t0 = time.perf_counter()
            S.capi.check(lib.sbmbp_batch_get_state(b._h, r, psi.ctypes.data_as(S.capi.c_dp), None))
            total += time.perf_counter() - t0
            if keep and rep == 1:
                table[:, r * Q:(r + 1) * Q] = psi
        down.append(total * 1e3)
    out["download_ms"] = down[1]
    out["download_first_pass_ms"] = down[0]
    out["numpy_ms"] = None
    if keep:
        t0 = time.perf_counter()
        G = table.T @ table
        out["numpy_ms"] = (time.perf_counter() - t0) * 1e3
        C = results["soft"][1]  # and the call agrees with that route
        Gc = C.transpose(0, 2, 1, 3).reshape(R * Q, R * Q)
        out["soft_max_rel_diff_to_numpy"] = float(np.max(np.abs(Gc - G) / np.abs(G)))
    for kind in KINDS:
        out["faster_than_download"][kind] = out["agreement_ms"][kind]["median"] < out["download_ms"]
    b.close()
    del b, g, psi, table
    gc.collect()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--shapes", type=int, nargs="+", default=[4, 8, 16, 16], help="Q R pairs")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host_gb", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_agreement.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_batch_agreement: no GPU")
    for N in a.sizes:
        for Q, R in zip(a.shapes[0::2], a.shapes[1::2]):
            line = json.dumps(measure(N, Q, R, a.repeats, a.warmup, a.host_gb))
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")
