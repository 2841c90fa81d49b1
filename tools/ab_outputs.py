"""Measurement aid for changes that must leave every output as it is: walks the launch paths of the engine on small graphs and
prints one SHA-256 line per output, so that two builds of the library can be compared line by line.
    SBMBP_LIB=<parent build>/libsbmbp_hip.so python3 tools/ab_outputs.py > parent.txt
    python3 tools/ab_outputs.py > new.txt && diff parent.txt new.txt
Run each build in a fresh process. A line counts only if a build reproduces it in a second run of its own.
Under `rocprofv3 --kernel-trace --stats -- python3 tools/ab_outputs.py` the same walk gives the launch census of a build
(kernel name -> calls), which must be the same table for both.

Graphs: the committed fixtures q4_n400, c1, hub_n600 and q10_n1000 with the parameters of their golden runs, the boundary
graph of tests/boundary_graph.py for Q = 5, 9 and 14, and the smallest Q = 17 case of tests/wide_cases.py; every
deg_corr_flag the engine takes at that label count (the fixtures' cab divided by the squared mean degree under degree
correction, as tests/boundary_graph.py does). Outputs per graph: the state after three sweeps from the device state, a host
state, a host state with clamped rows, in the message-gather form (damped) and with a vertex prior; free energy and entropy
with their parts under the exact non-edge term, the series orders 1 .. 4 and the automatic choice, on the fused and on the
separate reduction kernels; EM expectations; two coloured sweeps; a batch of three replicas (state, em_step); two shards of
two chunks (state and reductions, from the device and from a host state)."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import sbm_bp_amd as S
from sbm_bp_amd.distributed import LocalShards
import boundary_graph as bg
import wide_cases as wc

GOLD = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("q4_tight_seed0", "c1_matched_tight_seed0", "hub_dc0_tight_seed0", "q10_tight_seed1")
NONEDGE = [(1, 0)] + [(2, k) for k in (1, 2, 3, 4)] + [(0, 0)]  # (mode, series order)


def emit(label, *values):
    h = hashlib.sha256()

    def feed(v):
        if isinstance(v, (tuple, list)):
            for x in v:
                feed(x)
        else:
            h.update(np.ascontiguousarray(v, dtype=np.float64).tobytes())

    feed(values)
    print("%s  %s" % (h.hexdigest(), label), flush=True)


def graphs():
    """(name, graph, Q, N, cab for dc 0, na, true_conf, seed)"""
    for name in FIXTURES:
        a = json.load(open(os.path.join(GOLD, name + ".json")))["args"]
        n = [int(x) for x in str(a["n"]).split(",")]
        N, Q = sum(n), len(n)
        g = S.load_edge_list(os.path.join(GOLD, a["l"]), N)
        st = S.bp_param_from_direct(S.blockmodel_t(g, Q, 0), [float(x) for x in str(a["pa"]).split(",")], [float(x) for x in str(a["cab"]).split(",")])
        yield a["l"].split(".")[0], g, Q, N, np.array(st.cab, dtype=np.float64).reshape(Q, Q), np.array(st.na, dtype=np.uint32), np.repeat(np.arange(Q), n).astype(np.uint32), int(a["d"])
    for Q in (5, 9, 14):
        t = bg.instance(Q, 0)
        yield "boundary_q%d" % Q, S.Graph.from_edges(t["pairs"], t["N"]), Q, t["N"], t["cab"], t["na"], t["tc"], t["seed"]
    case = wc.FIELD[0]
    cab, na, tc = case.arrays()
    yield "wide_q%d" % case.Q, S.load_edge_list(wc.HUB_PATH, wc.HUB_N), case.Q, wc.HUB_N, cab, na, tc, case.seed


def walk(name, g, Q, N, cab0, na, tc, seed, dc):
    tag = "%s dc%d" % (name, dc)
    cab = cab0 / (g.E2 / N) ** 2 if dc else cab0
    state = S.bp_blockmodel_state(cab, na)
    conf = np.where(np.arange(N) % 7 == 0, tc.astype(np.int32), -1).astype(np.int32)
    wide = Q > 16

    def engine(init):
        bp = S.bp_conditional()
        bm = S.blockmodel_t(g, Q, dc)
        if init == "device":
            bp.init_messages_device(bm, tc, seed)
        else:
            bp.init_messages(bm, 1 if init == "clamped" else 0, conf if init == "clamped" else None, tc, seed)
        bp.expand_bp_params(state)
        return bp

    def reductions(bp, what):
        for mode, order in NONEDGE:
            bp.set_nonedge_mode(mode, order)
            emit("%s %s free energy, nonedge mode %d order %d" % (tag, what, mode, order), bp.compute_free_energy(parts=True))
            emit("%s %s entropy, nonedge mode %d order %d" % (tag, what, mode, order), bp.compute_entropy(parts=True))
        bp.set_nonedge_mode(0, 0)
        emit("%s %s EM expectations" % (tag, what), bp.em_expectations())
        emit("%s %s overlap, confusion" % (tag, what), bp.compute_overlap(), bp.confusion())

    for variant in ("device", "host", "clamped", "gather", "prior"):
        if variant == "prior" and wide:
            continue
        bp = engine(variant if variant in ("device", "host", "clamped") else "host")
        damp = 1.0
        if variant == "gather":
            bp.set_gather_mode(1)
            damp = 0.7
        if variant == "prior":
            bp.set_vertex_prior(np.random.default_rng(11).uniform(0.5, 1.5, size=(N, Q)))
        d = [bp.sweep(1, damp) for _ in range(3)]
        emit("%s %s three sweeps" % (tag, variant), d, bp.get_state())
        if variant != "clamped":
            reductions(bp, variant)
    if wide:
        return
    bp = engine("host")
    bp.set_sweep_order("coloured")
    emit("%s two coloured sweeps" % tag, [bp.sweep(1, 0.8) for _ in range(2)], bp.get_state(), bp.h())
    with S.ReplicaBatch(g, Q, dc, 3) as rb:
        rb.init_messages(0, None, tc, (3, 4, 5))
        for r, s in enumerate(bg.BATCH_SCALES):
            rb.set_params(S.bp_blockmodel_state(cab * s, na), 1.0, r)
        emit("%s batch three sweeps" % tag, rb.sweep(3, 0.9), [rb.get_state(r) for r in range(3)])
        emit("%s batch em_step" % tag, rb.em_step())
        emit("%s batch free energy, entropy of every replica" % tag, rb.compute_free_energy(parts=True), rb.compute_entropy(parts=True))
    for init in ("device", "host"):
        sb = LocalShards(g, Q, dc, 2, n_chunks=2)
        try:
            if init == "device":
                sb.init_messages_device(seed, tc)
            else:
                sb.init_messages(0, None, tc, seed, True)
            sb.expand_bp_params(cab, na, 1.0)
            emit("%s shards %s three sweeps" % (tag, init), sb.sweep(3, 1.0), sb.global_state())
            emit("%s shards %s reductions" % (tag, init), sb.compute_free_energy(parts=True), sb.compute_entropy(parts=True), sb.em_expectations(), sb.compute_overlap())
        finally:
            sb.close()


if __name__ == "__main__":
    S.load_library()
    print("# library: %s" % os.path.abspath(S.lib_path()), file=sys.stderr)
    for name, g, Q, N, cab0, na, tc, seed in graphs():
        for dc in ((0, 1) if Q > 16 else (0, 1, 2)):
            walk(name, g, Q, N, cab0, na, tc, seed, dc)
