"""Replica batches of the HIP engine (include/sbmbp.h sbmbp_batch_*; csrc/kernels_batch.h k_sweep_batch / k_finalize_batch):
R independent BP runs over one graph, against the oracle's synchronous sweeps in the message form, against R single engines
with set_gather_mode(1), and the reference's goldens. Every instance has N <= 1000."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, args_of, golden, gpath
from test_gpu_coloured import _hub_instance
from test_gpu_parity import engine_from, oracle_from

pytestmark = pytest.mark.gpu

F_Q10_MERGED = -20.181041243116  # q10_tight_seed1's graph and parameters from seed 7: the merged-groups fixed point


@pytest.fixture(scope="module")
def S():
    import sbm_bp_amd as S
    S.load_library()
    return S


def batch_from(S, a, seeds, scale=None):
    """a batch on fixture a with one replica per seed; scale = {replica: factor on cab}"""
    g = S.load_edge_list(a["path"], a["N"])
    bm = S.blockmodel_t(g, a["Q"], a["dc"])
    st = S.bp_param_from_epsilon_c(bm, a["eps"], a["c"]) if "eps" in a else S.bp_param_from_direct(bm, a["pa"], a["cab_upper"])
    b = S.ReplicaBatch(g, a["Q"], a["dc"], len(seeds))
    b.init_messages(a["init_flag"], a.get("beliefs"), a["true_conf"], seeds)
    b.set_params(st, a["beta"])
    for r, s in (scale or {}).items():
        b.set_params(S.bp_blockmodel_state(st.cab * s, st.na), a["beta"], r)
    return g, b, st


def oracle_for(orc, a, seed, scale=1.0):
    og, ob, _ = oracle_from(orc, dict(a, seed=seed))
    if scale != 1.0:
        cab, na = ob.get_params()
        ob.set_params(cab * scale, na, a["beta"])
    ob.set_msg_form(True)
    return og, ob


@functools.lru_cache(maxsize=None)
def _oracle_converged(name, seed, crit, tmax):
    """the oracle's synchronous run (message form) of fixture `name` from `seed`: computed once, shared, never modified"""
    import oracle as orc
    a = args_of(golden(name))
    _, ob = oracle_for(orc, a, seed)
    niter, last = ob.converge_sync(crit, tmax, 1.0)
    psi, msg = ob.get_state()
    levels = ob.ar_levels()
    ob.compute_h()
    f, _ = ob.free_energy(0)
    e, _ = ob.entropy(0)
    for x in (psi, msg):
        x.setflags(write=False)
    return dict(niter=niter, last=last, psi=psi, msg=msg, levels=levels, f=f, e=e, overlap=ob.overlap())


def _check_initial(S, b, r, ob, single=None):
    psi, msg = b.get_state(r)
    opsi, omsg = ob.get_state()
    # bit-exact: the same mt19937 draws in the same fill order. The device keeps Q-1 components of a message and restores the
    # largest as max(0, 1 - sum of the others), so at this boundary ONE entry per message, the largest, comes back rounded.
    # How far: the oracle's message was normalised by Q divisions, so its components sum to 1 + d with |d| <= (Q + 1) 2^-53
    # (Q quotients of relative error 2^-53 whose values sum to 1, and the sum itself); the restored entry is 1 - s with s the
    # floating-point sum of the Q - 1 others (Q - 2 additions of partial sums below 1: <= (Q - 2) 2^-54) and one subtraction
    # (<= 2^-54). Together below 2 Q 2^-53: 4.4e-16 at Q = 2, 2.2e-15 at Q = 10.
    Q = psi.shape[1]
    assert (psi == opsi).all()
    assert ((msg != omsg).sum(1) <= 1).all() and (msg.size == 0 or np.abs(msg - omsg).max() <= 2 * Q * 2.0 ** -53)
    rows = np.flatnonzero((msg != omsg).any(1))
    assert (np.argmax(omsg[rows], 1) == np.argmax(msg[rows] != omsg[rows], 1)).all()  # only the largest component moves
    if single is not None:  # and bit for bit what sbmbp_init_messages leaves on a single engine
        spsi, smsg = single.get_state()
        assert np.array_equal(psi, spsi) and np.array_equal(msg, smsg)


DAMPS = (0.7, 0.7, 1.0, 1.0)


def _sweep_parity(S, orc, g, b, oracles, tol=1e-11):
    for r, ob in enumerate(oracles):
        _check_initial(S, b, r, ob)
    for k, damp in enumerate(DAMPS):
        d = b.sweep(1, damp)
        for r, ob in enumerate(oracles):
            do = ob.sweep_sync(damp)
            psi, msg = b.get_state(r)
            opsi, omsg = ob.get_state()
            assert np.abs(psi - opsi).max() < tol, ("marginals", k, r)
            assert msg.size == 0 or np.abs(msg - omsg).max() < tol, ("messages", k, r)
            assert abs(d[r] - do) < tol, ("difference", k, r, d[r], do)
    f, parts = b.compute_free_energy(parts=True)
    ov = b.compute_overlap()
    for r, ob in enumerate(oracles):
        ob.compute_h()
        fo, oparts = ob.free_energy(0)
        assert np.abs(parts[r] - oparts).max() <= 1e-9 * max(1.0, np.abs(oparts).max()), (r, parts[r], oparts)
        assert abs(f[r] - fo) <= 1e-9 * max(1.0, abs(fo))
        assert abs(ov[r] - ob.overlap()) < 1e-11
    st = b.stats()
    assert st.sweeps == len(DAMPS) * len(oracles) and st.edge_msg_updates == st.sweeps * g.E2 and st.psi_form_sweeps == 0


PARITY = ["q4_tight_seed0", "c1_dc1_tight_seed0", "c1_dc2_tight_seed0", "c1_matched_beta08_seed0", "q10_tight_seed1"]


@pytest.mark.parametrize("name", PARITY)
def test_every_sweep_of_every_replica_equals_the_oracle(S, orc, name):
    a = args_of(golden(name))
    seeds = [a["seed"], a["seed"] + 1, a["seed"] + 2]
    g, b, _ = batch_from(S, a, seeds, {2: 1.1})
    oracles = [oracle_for(orc, a, s, 1.1 if r == 2 else 1.0)[1] for r, s in enumerate(seeds)]
    _sweep_parity(S, orc, g, b, oracles)
    b.close()


def _hub_batch(S, orc, dc=0, seeds=(3, 4, 5)):
    Q, N = 9, 300
    pairs, cab, na, tc = _hub_instance(Q, N)
    if dc:
        cab = cab / 36.0
    g = S.Graph.from_edges(pairs, N)
    og = orc.Graph.from_edges(pairs, N)
    b = S.ReplicaBatch(g, Q, dc, len(seeds))
    b.init_messages(0, None, tc, list(seeds))
    b.set_params(S.bp_blockmodel_state(cab, na))
    b.set_params(S.bp_blockmodel_state(cab * 1.1, na), 1.0, 2)
    oracles = []
    for r, s in enumerate(seeds):
        ob = orc.OracleBP(og, Q, dc)
        ob.init_messages(0, None, tc, orc.Rng(s))
        ob.set_params(cab * (1.1 if r == 2 else 1.0), na, 1.0)
        ob.set_msg_form(True)
        oracles.append(ob)
    return g, b, oracles


@pytest.mark.parametrize("dc", [0, 1])
def test_a_row_above_the_segment_capacity_in_a_batch(S, orc, dc):
    """Q = 9: a segment holds 128 edges, so the row of 140 edges is updated by the fragment launches of every replica"""
    g, b, oracles = _hub_batch(S, orc, dc)
    assert b.stats().n_hub_rows == 1 and g.max_degree >= 140
    _sweep_parity(S, orc, g, b, oracles)
    b.close()


def _singles(S, a, seeds, scale=None):
    out = []
    for r, s in enumerate(seeds):
        _, _, bp, st = engine_from(S, a, seed=s)
        if scale and r in scale:
            bp.expand_bp_params(S.bp_blockmodel_state(st.cab * scale[r], st.na))
        bp.set_gather_mode(1)
        out.append(bp)
    return out


@pytest.mark.parametrize("name", ["q4_tight_seed0", "c1_dc2_tight_seed0", "c1_planted_i1_seed0"])
def test_batch_equals_three_single_engines(S, name):
    a = args_of(golden(name))
    seeds = [a["seed"], a["seed"] + 1, a["seed"] + 2]
    g, b, _ = batch_from(S, a, seeds, {2: 1.1})
    singles = _singles(S, a, seeds, {2: 1.1})
    for r, bp in enumerate(singles):
        assert all(np.array_equal(x, y) for x, y in zip(b.get_state(r), bp.get_state()))
    for k, damp in enumerate(DAMPS):
        d = b.sweep(1, damp)
        for r, bp in enumerate(singles):
            ds = bp.sweep(1, damp)
            (p1, m1), (p2, m2) = b.get_state(r), bp.get_state()
            assert np.abs(p1 - p2).max() < 1e-12 and np.abs(m1 - m2).max() < 1e-12 and abs(d[r] - ds) < 1e-12, (k, r)
            assert np.abs(b.h(r) - bp.h()).max() <= 1e-12 * max(1.0, np.abs(bp.h()).max())
    b.close()


def test_zeros_in_cab_and_clamped_rows_against_the_single_engine(S):
    """a forbidden group pair and clamped one-hot rows (-i 1 with a conf): b == 0 occurs, so the exact cavity runs. Compared
    with the single engine only: the oracle keeps the reference's `b == 0` quirk there"""
    rng = np.random.default_rng(21)
    Q, N = 3, 240
    pairs = rng.integers(0, N, size=(700, 2)).astype(np.uint32)
    cab = np.array([[8.0, 0.0, 1.0], [0.0, 7.0, 1.5], [1.0, 1.5, 6.0]])
    tc = rng.integers(0, Q, size=N).astype(np.uint32)
    na = np.bincount(tc, minlength=Q).astype(np.uint32)
    conf = np.full(N, -1, dtype=np.int32)
    fixed = rng.choice(N, 40, replace=False)
    conf[fixed] = tc[fixed]
    g = S.Graph.from_edges(pairs, N)
    seeds = [0, 1, 2]
    b = S.ReplicaBatch(g, Q, 0, 3)
    b.init_messages(1, conf, tc, seeds)
    b.set_params(S.bp_blockmodel_state(cab, na))
    singles = []
    for s in seeds:
        bp = S.bp_conditional()
        bp.init_messages(S.blockmodel_t(g, Q, 0), 1, conf, tc, s)
        bp.expand_bp_params(S.bp_blockmodel_state(cab, na))
        bp.set_gather_mode(1)
        singles.append(bp)
    rp = g.csr()[0].astype(np.int64)
    edge_row = np.repeat(np.arange(N), np.diff(rp))
    held = np.isin(edge_row, fixed)
    init = [b.get_state(r) for r in range(3)]
    zero_seen = False
    for k, damp in enumerate(DAMPS):
        d = b.sweep(1, damp)
        for r, bp in enumerate(singles):
            ds = bp.sweep(1, damp)
            (p1, m1), (p2, m2) = b.get_state(r), bp.get_state()
            assert np.isfinite(p1).all() and np.isfinite(m1).all()
            assert np.abs(p1 - p2).max() < 1e-12 and np.abs(m1 - m2).max() < 1e-12 and abs(d[r] - ds) < 1e-12, (k, r)
            assert np.array_equal(p1[fixed], init[r][0][fixed]) and np.array_equal(m1[held], init[r][1][held]), (k, r)
            zero_seen = zero_seen or bool((m1 == 0.0).any())
    assert zero_seen  # the instance does reach exact zeros in its messages
    b.close()


def test_replicas_stop_on_their_own(S, orc):
    name, seeds, crit, limit = "q10_tight_seed1", [7, 1, 0], 1e-13, 2000
    gd = golden(name)
    a = args_of(gd)
    ref = [_oracle_converged(name, s, crit, limit) for s in seeds]
    print("oracle niter for seeds %s: %s" % (seeds, [x["niter"] for x in ref]))
    assert all(x["niter"] >= 0 for x in ref) and len({x["niter"] for x in ref}) == 3
    g, b, _ = batch_from(S, a, seeds)
    niter, last = b.converge(crit, limit, 1.0)
    assert list(niter) == [x["niter"] for x in ref], (niter, last)
    assert (last < crit).all()
    for r, x in enumerate(ref):  # the state of ITS sweep: a replica that stopped early stayed frozen while the others went on
        psi, msg = b.get_state(r)
        assert np.abs(psi - x["psi"]).max() < 1e-9 and np.abs(msg - x["msg"]).max() < 1e-9, r
    f = b.compute_free_energy()
    assert abs(f[0] - F_Q10_MERGED) < 1e-9, f
    assert abs(f[1] - gd["result"]["f"]) < 1e-9 and abs(f[2] - gd["result"]["f"]) < 1e-9, f
    assert b.stats().sweeps == sum(x["niter"] + 1 for x in ref)
    for r in range(3):
        assert b.relaxation(r)[:2] == ref[r]["levels"]
    b.close()
    # inference: the fixed point of lowest free energy is the one kept
    g, b, _ = batch_from(S, a, seeds)
    res, best = b.inference(crit, limit, 1.0)
    fs = [x.free_energy for x in res]
    assert [x.niter for x in res] == [x["niter"] for x in ref]
    assert fs[best] == min(fs) and best in (1, 2)
    for r, x in enumerate(ref):
        assert abs(res[r].free_energy - x["f"]) < 1e-9 and abs(res[r].entropy - x["e"]) < 1e-8 and abs(res[r].overlap - x["overlap"]) < 1e-9
    b.close()
    g, b, _ = batch_from(S, a, [7, 1])
    res, best = b.inference(crit, limit, 1.0)
    assert best == 1 and res[1].free_energy < res[0].free_energy
    b.close()


def test_relaxation_is_per_replica_q4(S, orc):
    name, seeds = "q4_tight_seed0", [0, 3]
    gd = golden(name)
    a = args_of(gd)
    ref = [_oracle_converged(name, s, a["crit"], a["tmax"]) for s in seeds]
    print("oracle niter / levels for seeds %s: %s" % (seeds, [(x["niter"], x["levels"]) for x in ref]))
    assert [x["levels"] for x in ref] == [(0, -1), (1, -1)]
    g, b, _ = batch_from(S, a, seeds)
    niter, last = b.converge(a["crit"], a["tmax"], 1.0)
    assert [b.relaxation(r)[:2] for r in range(2)] == [(0, -1), (1, -1)]
    assert list(niter) == [x["niter"] for x in ref], (niter, last)
    f = b.compute_free_energy()
    assert np.abs(f - gd["result"]["f"]).max() < 1e-9, f
    b.close()


def test_relaxation_is_per_replica_hub(S, orc):
    name, seeds, crit = "hub_dc0_tight_seed0", [0, 1, 2], 1e-12
    gs = [golden("hub_dc0_tight_seed%d" % d) for d in (0, 1)]
    a = args_of(gs[0])
    ref = [_oracle_converged(name, s, crit, a["tmax"]) for s in seeds]
    print("oracle niter / f for seeds %s: %s" % (seeds, [(x["niter"], x["f"]) for x in ref]))
    g, b, _ = batch_from(S, a, seeds)
    res, best = b.inference(crit, a["tmax"], 1.0)
    fs = np.array([x.free_energy for x in res])
    assert [x.niter for x in res] == [x["niter"] for x in ref]
    assert np.abs(fs - np.array([x["f"] for x in ref])).max() < 1e-9, fs
    assert abs(fs[0] - gs[0]["result"]["f"]) < 1e-9 and abs(fs[1] - gs[1]["result"]["f"]) < 1e-9
    assert min(abs(fs[0] - fs[1]), abs(fs[0] - fs[2]), abs(fs[1] - fs[2])) > 1e-4  # three distinct fixed points
    assert best == 1
    assert [b.relaxation(r)[:2] for r in range(3)] == [x["levels"] for x in ref]
    b.close()


def test_reproducible_and_isolated(S):
    a = args_of(golden("q4_tight_seed0"))
    seeds = [0, 1, 2]
    out = []
    for _ in range(2):
        g, b, st = batch_from(S, a, seeds)
        b.sweep(7, 0.9)
        out.append([b.get_state(r) + (b.h(r),) for r in range(3)])
        b.close()
    for x, y in zip(out[0], out[1]):
        assert all(np.array_equal(u, v) for u, v in zip(x, y))
    # replica 1 with other parameters, then with another state: replicas 0 and 2 do not notice
    g, b, st = batch_from(S, a, seeds)
    b.set_params(S.bp_blockmodel_state(st.cab * 1.3, st.na), 0.9, 1)
    b.sweep(3, 1.0)
    g2, b2, _ = batch_from(S, a, seeds)
    p, m = b2.get_state(2)
    b2.set_state(1, p, m)
    b2.sweep(3, 1.0)
    g3, b3, _ = batch_from(S, a, seeds)
    b3.sweep(3, 1.0)
    for r in (0, 2):
        for other in (b, b2):
            assert all(np.array_equal(u, v) for u, v in zip(other.get_state(r), b3.get_state(r))), r
    assert not np.array_equal(b.get_state(1)[0], b3.get_state(1)[0])
    assert np.abs(b2.get_state(1)[0] - b3.get_state(2)[0]).max() < 1e-12  # (a state set from outside is re-encoded: not bitwise)
    cab1, na1, beta1 = b.get_params(1)
    assert np.array_equal(cab1, st.cab * 1.3) and beta1 == 0.9 and np.array_equal(b.get_params(0)[0], st.cab)
    for x in (b, b2, b3):
        x.close()


def test_one_replica_equals_the_single_engine(S):
    a = args_of(golden("c1_dc1_tight_seed0"))
    g, b, _ = batch_from(S, a, [a["seed"]])
    bp = _singles(S, a, [a["seed"]])[0]
    for damp in DAMPS:
        d, ds = b.sweep(1, damp), bp.sweep(1, damp)
        (p1, m1), (p2, m2) = b.get_state(0), bp.get_state()
        assert np.abs(p1 - p2).max() < 1e-12 and np.abs(m1 - m2).max() < 1e-12 and abs(d[0] - ds) < 1e-12
    n1, l1 = b.converge(a["crit"], a["tmax"], 1.0)
    n2, l2 = bp.converge(a["crit"], a["tmax"], 1.0)
    assert n1[0] == n2 and abs(l1[0] - l2) < 1e-12
    assert abs(b.compute_free_energy()[0] - bp.compute_free_energy()) < 1e-12
    for x, y in zip(b.em_expectations(0), bp.em_expectations()):
        assert np.abs(x - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
    b.close()


def test_refusals(S):
    rng = np.random.default_rng(0)
    N = 200
    g = S.Graph.from_edges(rng.integers(0, N, size=(600, 2)).astype(np.uint32), N)
    with pytest.raises(S.SbmbpError) as ei:
        S.ReplicaBatch(g, 20, 0, 2)
    assert ei.value.code == -6 and "Q = 16" in str(ei.value)
    b = S.ReplicaBatch(g, 3, 0, 2)
    for call in (lambda: b.get_state(2), lambda: b.h(5), lambda: b.relaxation(2), lambda: b.get_params(2),
                 lambda: b.set_params(S.bp_blockmodel_state(np.ones((3, 3)), [60, 70, 70]), 1.0, 2)):
        with pytest.raises(S.SbmbpError) as ei:
            call()
        assert ei.value.code == -1 and "replica" in str(ei.value)
    with pytest.raises(S.SbmbpError) as ei:  # call order, as on the single engine
        b.converge(1e-6, 10, 1.0)
    assert ei.value.code == -4
    b.close()
    b.close()  # idempotent
    b = S.ReplicaBatch(g, 3, 0, 2)
    del g  # a batch outlives the graph it was made from
    b.init_messages(0, None, rng.integers(0, 3, size=N), [0, 1])
    b.set_params(S.bp_blockmodel_state(np.array([[5.0, 1, 1], [1, 5, 1], [1, 1, 5]]), [60, 70, 70]))
    assert np.isfinite(b.sweep(2, 1.0)).all()
    del b


BP = os.path.join(ROOT, "bin", "bp")


def _run(*args):
    p = subprocess.run([BP] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def test_cli_restarts(S, tmp_path):
    name, crit, limit = "q10_tight_seed1", 1e-13, 2000
    a = args_of(golden(name))
    common = ["-l", gpath("q10_n1000.edgelist"), "-n"] + a["n"] + ["--pa"] + a["pa"] + ["--cab"] + a["cab_upper"] + ["-t", limit, "-e", crit]
    base = common + ["-m", "infer"]
    ref = [_oracle_converged(name, s, crit, limit) for s in (7, 8)]
    cand = [k for k, x in enumerate(ref) if x["niter"] >= 0] or [0, 1]
    want = min(cand, key=lambda k: ref[k]["f"])
    mj = tmp_path / "m.json"
    rc, out, err = _run(*base, "--seed", 7, "--restarts", 2, "--precision", 15, "--metrics_json", mj)
    assert rc == 0, err
    e, f, ov, niter = out.split("\n")[0].split()
    x = ref[want]
    assert abs(float(f) - x["f"]) < 1e-9 and abs(float(e) - x["e"]) < 1e-8 and abs(float(ov) - x["overlap"]) < 1e-9 and int(niter) == x["niter"]
    m = json.load(open(mj))
    assert m["restarts"] == 2 and m["best"] == want and m["seed"] == [7, 8] and m["niter"] == [y["niter"] for y in ref]
    assert np.abs(np.array(m["free_energy"]) - [y["f"] for y in ref]).max() < 1e-9
    assert np.abs(np.array(m["overlap"]) - [y["overlap"] for y in ref]).max() < 1e-9
    assert m["field_level"] == [y["levels"][0] for y in ref] and m["generic_level"] == [y["levels"][1] for y in ref]
    assert m["sweeps"] == sum(y["niter"] + 1 for y in ref)
    # the best replica's marginals
    rc, out2, err = _run(*base, "--seed", 7, "--restarts", 2, "--if_output_marginals")
    lines = out2.split("\n")
    psi = np.array([[float(v) for v in ln.split()] for ln in lines[1:1 + a["N"]]])
    assert rc == 0 and psi.shape == (a["N"], a["Q"]) and np.abs(psi - x["psi"]).max() < 1e-5  # printed with 6 digits
    # without --restarts, and with --restarts 1, the single-engine path prints what it prints
    rc, plain, _ = _run(*base, "--seed", 7)
    rc1, one, _ = _run(*base, "--seed", 7, "--restarts", 1)
    assert rc == 0 and rc1 == 0 and plain == one and len(plain.split()) == 4
    ref_line = "%g %g %g %d \n" % (ref[0]["e"], ref[0]["f"], ref[0]["overlap"], ref[0]["niter"])
    assert plain.split()[:3] == ref_line.split()[:3]
    # what it cannot be combined with
    for extra, word in ((["-m", "learn", "--restarts", 2], "learn"), (["-m", "infer", "--restarts", 2, "--gpus", 2], "--gpus"),
                        (["-m", "infer", "--restarts", 2, "--schedule", "coloured"], "coloured"), (["-m", "infer", "--restarts", 0], "at least 1")):
        rc, o, err = _run(*common, *extra)
        assert rc == 1 and o == "" and "--restarts" in err and word in err, (extra, err)
    sizes = [50] * 20
    rc, o, err = _run("-l", gpath("q10_n1000.edgelist"), "-n", *sizes, "--epsilon_c", 0.1, 5.0, "-m", "infer", "--restarts", 2)
    assert rc == 1 and o == "" and "--restarts" in err and "16" in err
