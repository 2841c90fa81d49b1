"""The shard kernels ON their edges: the recipes of tests/shard_boundary_graph.py (a segment whose send-slot list is full, one
slot short and empty; hub rows first and last in a rank and a chunk, read by every peer, with halo neighbours only, with a
fragment boundary between own and halo neighbours, alone in a rank; empty chunks; a rank without an edge; 64, 65 and 129
segments in the per-rank fold) at every compiled label count below 17, the ranks as threads on one GPU (LocalShards), against
the oracle. Every case first checks that every rank segments its rows as the chunked model does, so a moved cut fails here
instead of quietly moving the rows off the edges. tests/test_shard_boundary_cpu.py holds the CPU side: where every condition
shows, and that the oracle is finite and converges on every case run here.
Tolerances are the project's (tests/test_gpu_fuzz.py, tests/test_gpu_sharded.py): 1e-11 per sweep on marginals, messages and
the reported maximum; 1e-9 relative on free-energy parts and EM expectations, 1e-8 on the entropy, 1e-11 on the overlap; 1e-7
on converged marginals. Each case prints the largest differences it saw."""
import os
import subprocess
import sys

import numpy as np
import pytest

import shard_boundary_graph as sg
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


def _rel(a, b):
    """max |a - b| / max(1, max |b|) over the entries where b is finite; a must be finite there"""
    a, b = np.atleast_1d(np.asarray(a, dtype=float)), np.atleast_1d(np.asarray(b, dtype=float))
    fin = np.isfinite(b)
    assert np.isfinite(a[fin]).all(), (a, b)
    return float(np.abs(a[fin] - b[fin]).max() / max(1.0, np.abs(b[fin]).max())) if fin.any() else 0.0


class _Seen:
    """the largest differences of one case, printed at its end"""

    def __init__(self, label):
        self.label, self.sweep, self.parts, self.entropy, self.overlap, self.fixed = label, 0.0, 0.0, 0.0, 0.0, 0.0

    def per_sweep(self, x, what):
        self.sweep = max(self.sweep, float(x))
        assert x < 1e-11, (self.label, what, x)

    def reduction(self, a, b, what):
        d = _rel(a, b)
        self.parts = max(self.parts, d)
        assert d <= 1e-9, (self.label, what, d, a, b)

    def entropy_parts(self, a, b):
        d = _rel(a, b)
        self.entropy = max(self.entropy, d)
        assert d <= 1e-8, (self.label, "entropy parts", d, a, b)

    def report(self, extra=""):
        print("shard boundary %s: per sweep %.3g, free energy parts / EM expectations %.3g, entropy %.3g, overlap %.3g, converged marginals %.3g%s"
              % (self.label, self.sweep, self.parts, self.entropy, self.overlap, self.fixed, extra))


_engine_graphs = {}


def _graph(S, t):
    key = id(t["pairs"])  # (the recipes build every graph once per process)
    if key not in _engine_graphs:
        _engine_graphs[key] = (S.Graph.from_edges(t["pairs"], t["N"]), t["pairs"])
    return _engine_graphs[key][0]


def _shards(S, t, n_chunks):
    from sbm_bp_amd.distributed import LocalShards
    sb = LocalShards(_graph(S, t), t["Q"], t["dc"], t["world"], n_chunks=n_chunks)
    sb.init_messages(t["flag"], t["conf"], t["tc"], t["seed"], True)
    sb.expand_bp_params(t["cab"], t["na"], 1.0)
    return sb


def _assert_plan(sb, t, n_chunks):
    """every rank's rows, halo, chunks, segments and hub rows are the models'"""
    _, ranks = sg.rank_models(t["row_ptr"], t["nbr"], t["world"], n_chunks, t["cap"], t["rcap"])
    for r, (m, st, sh) in enumerate(zip(ranks, sb.stats(), sb.ranks)):
        sp = m["plan"]
        assert (sh.row0, sh.n_own, sh.n_halo, sh.n_edges, sh.info.n_chunks) == (sp.row0, sp.n_own, sp.n_halo, sp.n_edges, n_chunks), r
        assert (st.n_blocks, st.n_hub_rows, st.hub_edges) == (m["n_blocks"], m["n_hub_rows"], m["hub_edges"]), \
            (r, st.n_blocks, st.n_hub_rows, st.hub_edges, m["n_blocks"], m["n_hub_rows"], m["hub_edges"])
    return ranks


# the oracle's run of a case: computed once, shared by the chunk counts and knobs that run the same case, never changed
_reference = {}


def _exact_nonedge(t):
    """the oracle's exact non-edge terms are O(N^2 Q^2) without degree correction (3.5 s at N = 1000, Q = 64): where that is
    above a second the site and edge parts are compared"""
    return t["dc"] != 0 or float(t["N"]) ** 2 * t["Q"] ** 2 <= 7e8


def _oracle_run(orc, t, key, msg_form=False, damps=sg.DAMPS, converge=True):
    if key in _reference:
        return _reference[key]
    if len(_reference) >= 4:
        _reference.pop(next(iter(_reference)))
    og = orc.Graph.from_edges(t["pairs"], t["N"])
    ob = orc.OracleBP(og, t["Q"], t["dc"])
    ob.init_messages(t["flag"], t["conf"], t["tc"], orc.Rng(t["seed"]))
    ob.set_params(t["cab"], t["na"], 1.0)
    if msg_form:
        ob.set_msg_form(True)
    ref = dict(d=[], psi=[], msg=[], E2=og.E2)
    for damp in damps:
        ref["d"].append(ob.sweep_sync(damp))
        psi, msg = ob.get_state()
        ref["psi"].append(psi.copy())
        ref["msg"].append(msg.copy())
    ob.compute_h()
    exact = _exact_nonedge(t)
    ref["f_parts"] = np.array(ob.free_energy(0 if exact else 2)[1])
    ref["e_parts"] = None if t["dc"] else np.array(ob.entropy(0 if exact else 2)[1])
    ref["em"] = [np.array(x) for x in ob.em_expect()]
    ref["overlap"] = ob.overlap()
    if converge:
        ref["niter"], ref["last"] = ob.converge_sync(1e-10, 600, 1.0)
        ref["fixed"] = ob.get_state()[0].copy()
    _reference[key] = ref
    return ref


def _sweeps_against(seen, sb, ref, damps):
    for k, damp in enumerate(damps):
        d = sb.sweep(1, damp)
        psi, msg = sb.global_state()
        seen.per_sweep(np.abs(psi - ref["psi"][k]).max(), "marginals after sweep %d" % k)
        seen.per_sweep(np.abs(msg - ref["msg"][k]).max(initial=0.0), "messages after sweep %d" % k)
        seen.per_sweep(abs(d - ref["d"][k]), "difference of sweep %d" % k)
    return psi, msg


def _grouped_sweeps_against(seen, sb, ref, damps):
    """the same sweeps with equal dampings queued in ONE call each. A call of one sweep starts from a freshly packed halo and a
    freshly summed field; only inside a longer call does sweep j + 1 read what the send pass of sweep j left in the receive
    buffer, and take its field from the rows that k_fold_records and the gathered k_finalize folded after sweep j."""
    k = 0
    while k < len(damps):
        n = 1
        while k + n < len(damps) and damps[k + n] == damps[k]:
            n += 1
        d = sb.sweep(n, damps[k])
        k += n
        psi, msg = sb.global_state()
        seen.per_sweep(np.abs(psi - ref["psi"][k - 1]).max(), "marginals after sweep %d (queued together)" % (k - 1))
        seen.per_sweep(np.abs(msg - ref["msg"][k - 1]).max(initial=0.0), "messages after sweep %d (queued together)" % (k - 1))
        seen.per_sweep(abs(d - ref["d"][k - 1]), "difference of sweep %d (queued together)" % (k - 1))


def _reductions_against(seen, sb, t, ref):
    exact = _exact_nonedge(t)
    fp = sb.compute_free_energy(parts=True)[1]
    seen.reduction(fp if exact else fp[:2], ref["f_parts"] if exact else ref["f_parts"][:2], "free energy parts")
    e, ep = sb.compute_entropy(parts=True)
    if t["dc"]:
        assert np.isnan(e)
    else:
        # the reference's site entropy multiplies a row's factors directly and is NaN once a hub row underflows: the finite
        # parts are compared (tests/test_gpu_boundary.py)
        assert np.isfinite(ep).all()
        seen.entropy_parts(ep if exact else ep[:2], ref["e_parts"] if exact else ref["e_parts"][:2])
    for a, b in zip(sb.em_expectations(), ref["em"]):
        seen.reduction(a, b, "EM expectations")
    seen.overlap = max(seen.overlap, abs(sb.compute_overlap() - ref["overlap"]))
    assert seen.overlap < 1e-11, (seen.label, "overlap", seen.overlap)


def _converge_against(seen, sb, ref, key):
    n1, l1 = sb.converge(1e-10, 600, 1.0)
    n2, l2 = ref["niter"], ref["last"]
    if key in sg.NOT_CONVERGING:  # both at the limit: nothing more to compare
        assert n1 < 0 and n2 < 0, (seen.label, n1, n2, l1, l2)
        return n1, n2
    # the same sweep; where a decision of the convergence machine was a tie between sums folded in different orders, within
    # the two sweeps tests/test_gpu_wide_relax.py allows (stricter than the sharded fuzz's "either within 4e-9": with the
    # criterion at 1e-10 that holds for any two converged runs)
    assert n2 >= 0 and n1 >= 0 and abs(n1 - n2) <= 2, (seen.label, n1, n2, l1, l2)
    assert l1 < 1e-10
    seen.fixed = float(np.abs(sb.global_state()[0] - ref["fixed"]).max())
    assert seen.fixed < 1e-7, (seen.label, "converged marginals", seen.fixed)
    return n1, n2


# ---------------------------------------------------------------------------------------------------------------------
# a. the threshold cases against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _threshold_case(S, orc, Q, dc, world, n_chunks, variant="default"):
    t = sg.instance(Q, dc, world, clamp=variant == "clamped")
    seen = _Seen("cap %d Q %d dc %d world %d chunks %d %s" % (t["cap"], Q, dc, world, n_chunks, variant))
    msg_form = variant != "default"  # on shards a clamped run takes the message-gather form throughout
    key = ("threshold", Q, dc, world) + (() if variant == "default" else (variant,))
    ref = _oracle_run(orc, t, key, msg_form)
    sb = _shards(S, t, n_chunks)
    try:
        assert sb.E2_global == ref["E2"] == 2 * len(t["pairs"])
        _assert_plan(sb, t, n_chunks)
        if variant == "gather":
            sb.set_gather_mode(1)
        psi0 = sb.global_state()[0]
        sb.reset_stats()
        _sweeps_against(seen, sb, ref, sg.DAMPS)
        # two damped sweeps and the first undamped one in the message-gather form (a damped message pair is not the one the
        # marginals were formed from: dist.hip run() leaves `consistent` false, as the single engine does), then two in the
        # marginal-gather form (sweep_psi on every chunk); never with deg_corr_flag 2, clamped rows or when the messages
        # are asked for
        want = 0 if variant != "default" or dc == 2 else 2
        assert [st.psi_form_sweeps for st in sb.stats()] == [want] * world
        if variant == "clamped":
            rows = sg.clamp_rows(t)
            assert np.array_equal(sb.global_state()[0][rows], psi0[rows]) and (psi0[rows, t["tc"][rows]] == 1.0).all()
        _reductions_against(seen, sb, t, ref)
    finally:
        sb.close()
    sb = _shards(S, t, n_chunks)  # a second run: two damped sweeps in one call, three undamped in the next
    try:
        if variant == "gather":
            sb.set_gather_mode(1)
        _grouped_sweeps_against(seen, sb, ref, sg.DAMPS)
        assert [st.psi_form_sweeps for st in sb.stats()] == [want] * world
        _reductions_against(seen, sb, t, ref)
        n1, n2 = _converge_against(seen, sb, ref, key)
        if variant == "clamped":
            assert np.array_equal(sb.global_state()[0][rows], psi0[rows])
    finally:
        sb.close()
    seen.report(", sweeps to converge: engine %d, oracle %d" % (n1, n2))
    return seen


@pytest.mark.parametrize("Q,dc,world,n_chunks", [(Q, dc, w, c) for Q, dc in sg.THRESHOLD for w, c in sg.LAYOUTS])
def test_threshold_cases_against_the_oracle(S, orc, Q, dc, world, n_chunks):
    _threshold_case(S, orc, Q, dc, world, n_chunks)


@pytest.mark.parametrize("Q", sg.CLAMPED_Q)
def test_clamped_threshold_rows(S, orc, Q):
    _threshold_case(S, orc, Q, 0, 3, 4, "clamped")


def test_message_gather_mode_on_a_threshold_case(S, orc):
    _threshold_case(S, orc, 8, 1, 3, 4, "gather")


# ---------------------------------------------------------------------------------------------------------------------
# b. every compiled label count on shards: the (128, 64) recipe, three ranks, two chunks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,dc", sg.LABELS)
def test_every_label_count_on_shards(S, orc, Q, dc):
    t = sg.instance(Q, dc, 3, cls=(128, 64))
    seen = _Seen("labels Q %d dc %d (caps %d, %d)" % (Q, dc, t["cap"], t["rcap"]))
    damps = sg.DAMPS[1:]  # a damped and an undamped sweep in the message-gather form, two in the marginal-gather form unless dc 2
    ref = _oracle_run(orc, t, ("labels", Q, dc), damps=damps, converge=False)
    sb = _shards(S, t, 2)
    try:
        ranks = _assert_plan(sb, t, 2)
        assert ranks[1]["n_hub_rows"] > 0 and sb.stats()[1].n_hub_rows > 0  # the hub kernels with io, on a rank other than 0
        sb.reset_stats()
        _sweeps_against(seen, sb, ref, damps)
        assert [st.psi_form_sweeps for st in sb.stats()] == [0 if dc == 2 else 2] * 3
    finally:
        sb.close()
    sb = _shards(S, t, 2)
    try:
        _grouped_sweeps_against(seen, sb, ref, damps)
        assert [st.psi_form_sweeps for st in sb.stats()] == [0 if dc == 2 else 2] * 3
        _reductions_against(seen, sb, t, ref)
    finally:
        sb.close()
    seen.report()


# ---------------------------------------------------------------------------------------------------------------------
# c. the per-rank fold: 64, 65 and 129 segments on rank 0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,segments,clamp", sg.FOLD)
def test_per_rank_fold_at_64_65_and_129_segments(S, orc, Q, segments, clamp):
    t = sg.instance(Q, 0, 2, clamp=clamp, ring=segments)
    seen = _Seen("fold Q %d, %d segments%s" % (Q, segments, ", clamped" if clamp else ""))
    damps = (1.0, 1.0, 1.0, 1.0)
    ref = _oracle_run(orc, t, ("fold", Q, segments, clamp), msg_form=clamp, damps=damps, converge=False)
    sb = _shards(S, t, 1)
    try:
        _assert_plan(sb, t, 1)
        assert sb.stats()[0].n_blocks == segments
        sb.reset_stats()
        _sweeps_against(seen, sb, ref, damps)  # the reported maximum goes through k_fold_records and the gathered k_finalize
        assert [st.psi_form_sweeps for st in sb.stats()] == [0 if clamp else 3] * 2  # (the first sweep gathers the messages)
    finally:
        sb.close()
    sb = _shards(S, t, 1)  # the four sweeps in one call: every sweep's field comes from the folded rows of the sweep before
    try:
        _grouped_sweeps_against(seen, sb, ref, damps)
        assert [st.psi_form_sweeps for st in sb.stats()] == [0 if clamp else 3] * 2
        _reductions_against(seen, sb, t, ref)
    finally:
        sb.close()
    seen.report()


# ---------------------------------------------------------------------------------------------------------------------
# d. the knobs that change which device code runs
# ---------------------------------------------------------------------------------------------------------------------
_default_runs = {}


def _default_run(S, Q, world, n_chunks):
    key = (Q, world, n_chunks)
    if key not in _default_runs:
        _default_runs[key] = sg.run_case(S, sg.instance(Q, 1, world), n_chunks)
    return _default_runs[key]


def _against_reference(seen, run, ref):
    """run_case queues the two damped sweeps in one call and the three undamped ones in the next: states after sweeps 1 and 4"""
    d, psi, msg, _ = run
    assert len(d) == 2
    for j, k in enumerate((1, 4)):
        seen.per_sweep(np.abs(psi[j] - ref["psi"][k]).max(), "marginals after sweep %d" % k)
        seen.per_sweep(abs(d[j] - ref["d"][k]), "difference of sweep %d" % k)
    seen.per_sweep(np.abs(msg - ref["msg"][-1]).max(), "messages after the last sweep")


@pytest.mark.parametrize("Q", sg.KNOB_Q)
def test_full_width_halo(S, orc, monkeypatch, Q):
    """SBMBP_HALO_COMPRESS=0: all Q components of a marginal on the wire - the ncomp == Q branch of the halo gather, the
    full-width pack, unpack and send pass"""
    t = sg.instance(Q, 1, 3)
    seen = _Seen("full-width halo Q %d" % Q)
    ref = _oracle_run(orc, t, ("threshold", Q, 1, 3))
    assert _default_run(S, Q, 3, 4)[3] == Q - 1
    monkeypatch.setenv("SBMBP_HALO_COMPRESS", "0")
    sb = _shards(S, t, 4)
    monkeypatch.delenv("SBMBP_HALO_COMPRESS")
    try:
        assert [sh.info.halo_components for sh in sb.ranks] == [Q] * 3
        _assert_plan(sb, t, 4)
        sb.reset_stats()
        _sweeps_against(seen, sb, ref, sg.DAMPS)
        assert [st.psi_form_sweeps for st in sb.stats()] == [2] * 3
    finally:
        sb.close()
    monkeypatch.setenv("SBMBP_HALO_COMPRESS", "0")
    sb = _shards(S, t, 4)
    monkeypatch.delenv("SBMBP_HALO_COMPRESS")
    try:
        assert [sh.info.halo_components for sh in sb.ranks] == [Q] * 3
        _grouped_sweeps_against(seen, sb, ref, sg.DAMPS)  # the full-width send pass feeds the next sweep
        _reductions_against(seen, sb, t, ref)
        n1, n2 = _converge_against(seen, sb, ref, ("threshold", Q, 1, 3))
    finally:
        sb.close()
    seen.report(", sweeps to converge: engine %d, oracle %d" % (n1, n2))


@pytest.mark.parametrize("Q", sg.KNOB_Q)
def test_all_chunks_on_one_stream(S, orc, monkeypatch, Q):
    """SBMBP_SHARD_STREAMS=1: the same kernels in the same order on the compute stream - bit for bit the default run"""
    t = sg.instance(Q, 1, 3)
    seen = _Seen("one stream Q %d" % Q)
    ref = _oracle_run(orc, t, ("threshold", Q, 1, 3))
    default = _default_run(S, Q, 3, 4)
    monkeypatch.setenv("SBMBP_SHARD_STREAMS", "1")
    one = sg.run_case(S, t, 4)
    monkeypatch.delenv("SBMBP_SHARD_STREAMS")
    _against_reference(seen, one, ref)
    assert all(np.array_equal(a, b) for a, b in zip(one[:3], default[:3]))
    seen.report()


def test_natural_workgroup_numbering_in_a_fresh_process(S, orc, tmp_path):
    """SBMBP_SHARD_XCD=0 (read once per process): the chunk launches number their workgroups naturally. The partials are
    indexed by segment, not by workgroup, so the run is bit for bit the default one"""
    Q, world, n_chunks = 9, 3, 4
    t = sg.instance(Q, 1, world)
    seen = _Seen("natural numbering Q %d" % Q)
    ref = _oracle_run(orc, t, ("threshold", Q, 1, world))
    out = tmp_path / "state.npz"
    env = dict(os.environ, SBMBP_SHARD_XCD="0")
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "shard_knob_worker.py"), str(out), str(Q), "1", str(world), str(n_chunks)],
                        env=env, timeout=300, capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr[-3000:]
    res = np.load(out)
    assert str(res["xcd"]) == "0"
    child = (res["d"], res["psi"], res["msg"], None)
    _against_reference(seen, child, ref)
    default = _default_run(S, Q, world, n_chunks)
    assert all(np.array_equal(a, b) for a, b in zip(child[:3], default[:3]))
    seen.report()
