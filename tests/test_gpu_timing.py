"""The counters behind the benchmark's headline kernel time: bench.py reports sweep_kernel_ms / sweep_launches, and both are fed
by the event pairs the engine puts around what a sweep times (engine.hip timing_begin / timing_end, added up by collect_timing).
Every sweep path takes its pair from the same pool, so each path is pinned here: with timing on, n sweeps give n pairs and a
positive time; with timing off, the sweeps go on counting and the two timing counters stand still.

Single engine: one pair per sweep on every path (around the frame kernel; around k_wsweep above Q = 16; around the whole step
sequence in the coloured order, although such a sweep is 2 x steps launches or more). Shards: one pair per chunk that has
segments in the marginal-gather form, one pair per sweep in the message-gather form, and collect_timing divides the pairs of a
call by the number of chunks (rounding down) - the model of tests/shard_boundary_graph.py says which chunks have segments."""
import math

import numpy as np
import pytest

import boundary_graph as bg
import shard_boundary_graph as sg
import wide_cases as wc

pytestmark = pytest.mark.gpu

CALLS = (2, 1)  # n = 3 sweeps as two calls: the pairs of every call are collected at its end
N_SWEEPS = sum(CALLS)


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


def _engine(S, t, device_init=False):
    g = S.Graph.from_edges(t["pairs"], t["N"])
    bp = S.bp_conditional()
    bm = S.blockmodel_t(g, t["Q"], t["dc"])
    if device_init:
        bp.init_messages_device(bm, t["tc"], t["seed"])
    else:
        bp.init_messages(bm, t["flag"], t["conf"], t["tc"], t["seed"])
    bp.expand_bp_params(S.bp_blockmodel_state(t["cab"], t["na"]))
    return bp


def _timed(st):
    return st.sweeps, st.sweep_launches, st.sweep_kernel_ms


def _pin(label, eng, stats, calls, launches):
    """calls: sweeps per sweep() call; launches(n): the sweep_launches expected of every engine behind stats() after n sweeps.
    Returns the stats after the timed sweeps (one entry per engine)."""
    n = sum(calls)
    eng.reset_stats()
    eng.set_timing(True)
    for k in calls:
        eng.sweep(k, 1.0)
    on = stats()
    want = launches(n)
    print("timing %s: %s, expected launches %s" % (label, [_timed(st) for st in on], want))
    for st, w in zip(on, want):
        assert st.sweeps == n and st.sweep_launches == w, (label, _timed(st), n, w)
        assert math.isfinite(st.sweep_kernel_ms) and st.sweep_kernel_ms > 0.0, (label, st.sweep_kernel_ms)
    eng.set_timing(False)
    for k in calls:
        eng.sweep(k, 1.0)
    for st, before in zip(stats(), on):
        assert st.sweeps == 2 * n, (label, st.sweeps)
        assert st.sweep_launches == before.sweep_launches and st.sweep_kernel_ms == before.sweep_kernel_ms, (label, _timed(st), _timed(before))
    return on


def _pin_single(label, bp, calls=CALLS):
    return _pin(label, bp, lambda: [bp.stats()], calls, lambda n: [n])[0]


def test_marginal_gather_form(S):
    bp = _engine(S, bg.instance(4, 0), device_init=True)  # device initial state, undamped: every sweep is a k_sweep_psi
    assert bp.stats().n_hub_rows > 0
    assert _pin_single("marginal-gather Q 4 dc 0", bp).psi_form_sweeps == N_SWEEPS


def test_message_gather_form(S):
    bp = _engine(S, bg.instance(4, 2))
    bp.set_gather_mode(1)
    assert _pin_single("message-gather Q 4 dc 2", bp).psi_form_sweeps == 0


def test_with_a_vertex_prior(S):
    t = bg.instance(5, 1)
    bp = _engine(S, t)
    bp.set_vertex_prior(np.random.default_rng(5).uniform(0.5, 1.5, size=(t["N"], t["Q"])))
    assert _pin_single("prior Q 5 dc 1", bp).psi_form_sweeps == 0


def test_coloured_order(S):
    bp = _engine(S, bg.instance(3, 0))
    bp.set_sweep_order("coloured")
    assert bp.sweep_order()[2] > 1  # several steps, so several launches, and still one pair per sweep
    _pin_single("coloured Q 3", bp)


def test_wide_path(S):
    case = wc.FIELD[0]
    assert case.Q == 17
    cab, na, tc = case.arrays()
    bp = S.bp_conditional()
    bp.init_messages(S.blockmodel_t(S.load_edge_list(wc.HUB_PATH, wc.HUB_N), case.Q, 0), 0, None, tc, case.seed)
    bp.expand_bp_params(S.bp_blockmodel_state(cab, na))
    _pin_single("wide Q 17", bp)


def test_event_pool_grows_inside_a_call(S):
    # the pool grows by 256 events = 128 pairs, and the pairs of a call are handed back at its end: the 129th sweep of ONE call
    # is the first to grow it a second time
    _pin_single("pool growth Q 2", _engine(S, bg.instance(2, 0)), calls=(129,))


@pytest.mark.parametrize("init", ["device", "host"])
@pytest.mark.parametrize("n_chunks", [1, 4])
def test_shards(S, n_chunks, init):
    """World 2 (a layout with an empty chunk between two others at four chunks), Q = 4, ONE call of n sweeps, so that the
    division by the number of chunks rounds once. From the device initial state every sweep takes the marginal-gather form:
    pairs = n x chunks with segments. From a host state the first sweep gathers the messages themselves
    (sbmbp_shard_sweep_explicit: one pair for the whole shard) and the others follow in the marginal-gather form:
    pairs = 1 + (n - 1) x chunks with segments."""
    from sbm_bp_amd.distributed import LocalShards
    n, world = N_SWEEPS, 2
    t = sg.instance(4, 0, world)
    _, ranks = sg.rank_models(t["row_ptr"], t["nbr"], world, n_chunks, t["cap"], t["rcap"])
    filled = [int((np.diff(m["chunk_blk"]) > 0).sum()) for m in ranks]
    assert all(filled) and (n_chunks == 1 or min(filled) < n_chunks), filled  # (the empty chunk is there)

    def launches(n):
        if init == "device":
            return [n * f // n_chunks for f in filled]
        return [(1 + (n - 1) * f) // n_chunks for f in filled]

    sb = LocalShards(S.Graph.from_edges(t["pairs"], t["N"]), t["Q"], t["dc"], world, n_chunks=n_chunks)
    try:
        if init == "device":
            sb.init_messages_device(t["seed"], t["tc"])
        else:
            sb.init_messages(t["flag"], t["conf"], t["tc"], t["seed"], True)
        sb.expand_bp_params(t["cab"], t["na"], 1.0)
        on = _pin("shards %s state, %d chunk(s), chunks with segments %s" % (init, n_chunks, filled), sb, sb.stats, (n,), launches)
        assert [st.n_blocks for st in on] == [m["n_blocks"] for m in ranks]
        assert [st.psi_form_sweeps for st in on] == [n if init == "device" else n - 1] * world
    finally:
        sb.close()
