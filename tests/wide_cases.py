"""Instances for the label counts above 16 that the random and boundary graphs do not reach (no test in this file):

A. runs on the committed hub graph (tests/golden/hub_n600.edgelist, N = 600) on which the adaptive relaxation acts (plain
   Jacobi sweeps do not converge on any of them but the one named in JACOBI_CONVERGES), so that converge() above Q = 16
   leaves the line `conv = md < crit && field_ok` of k_wfinalize and walks its restated
   convergence machine: the field ladder (F), the probe and the generic (damped) ladder, the exhausted ladder, the machine
   switched off, and a fixed field mix with the field gate rf.
B. a ring with chords of more than 16 * 1024 vertices: every segment of the wide plan closes at its row limit, so the graph has
   ceil(N / 16) segments and the [n_blk][stride] records take the two-stage fold (engine.hip fold_stage: rows > 4 FOLD_BLOCKS)
   on every sweep and every reduction.

tests/test_wide_cpu.py proves on the oracle alone that every instance does what this file says (levels, stability under a
perturbation of the initial state, segment counts); tests/test_gpu_wide_relax.py then compares the engine with the oracle."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HUB_PATH, HUB_N = os.path.join(GOLD, "hub_n600.edgelist"), 600
CRIT = 1e-10

# the ladders of the adaptive relaxation, restated (kernels.h ar_field_cap / ar_gen_mix / ar_gen_damp, bp_oracle.cpp ar_t)
FIELD_CAP = (1.0, 0.25, 0.1, 0.05)
GEN_MIX = {-1: 1.0, 0: 0.5, 1: 0.25, 2: 0.5, 3: 0.25, 4: 0.1, 5: 0.25, 6: 0.1}
GEN_DAMP = {-1: 1.0, 0: 1.0, 1: 1.0, 2: 0.5, 3: 0.5, 4: 0.5, 5: 0.25, 6: 0.25}


def mix_damp(fl, gl, base_mix=1.0):
    """(field mix, damping factor) of levels (fl, gl)"""
    return min(base_mix, FIELD_CAP[fl], GEN_MIX[gl]), GEN_DAMP[gl]


def super3(Q, cin, cout):
    """three super-groups of labels: cin inside one, cout between two"""
    s = np.arange(Q) * 3 // Q
    return np.where(s[:, None] == s[None, :], float(cin), float(cout))


def diag(Q, cin, cout):
    return np.where(np.eye(Q, dtype=bool), float(cin), float(cout))


FAMILIES = {"super3": super3, "diag": diag}


class Relax:
    """one run on the hub graph: dc 0, true_conf i Q // N, init flag 0 with Rng(seed), message form, crit 1e-10, damping 1.
    niter / levels: what the oracle's converge_sync does (measured on the CPU; test_wide_cpu.py asserts it)"""

    def __init__(self, family, cin, cout, Q, seed, niter, levels, tmax=700, auto=True, fixed_mix=None):
        self.family, self.cin, self.cout, self.Q, self.seed = family, cin, cout, Q, seed
        self.niter, self.levels, self.tmax, self.auto, self.fixed_mix = niter, levels, tmax, auto, fixed_mix

    @property
    def id(self):
        tag = "" if self.auto else ("-mix%g" % self.fixed_mix if self.fixed_mix is not None else "-noauto")
        return "%s(%g,%g)-Q%d-s%d%s" % (self.family, self.cin, self.cout, self.Q, self.seed, tag)

    @property
    def converges(self):
        return self.niter >= 0

    def arrays(self):
        Q = self.Q
        tc = (np.arange(HUB_N) * Q // HUB_N).astype(np.uint32)
        return FAMILIES[self.family](Q, self.cin, self.cout), np.bincount(tc, minlength=Q).astype(np.uint32), tc

    def oracle(self, orc, perturb=None):
        """the oracle in the initial state; perturb = seed of a relative 1e-13 perturbation of marginals and messages"""
        cab, na, tc = self.arrays()
        og = orc.Graph.from_edgelist(HUB_PATH, HUB_N)
        ob = orc.OracleBP(og, self.Q, 0)
        ob.init_messages(0, None, tc, orc.Rng(self.seed))
        ob.set_params(cab, na, 1.0)
        ob.set_msg_form(True)  # the wide path reports 1-step differences on every sweep
        if perturb is not None:
            rng = np.random.default_rng(perturb)
            psi, msg = ob.get_state()
            ob.set_state(psi * (1.0 + 1e-13 * rng.uniform(-1.0, 1.0, psi.shape)), msg * (1.0 + 1e-13 * rng.uniform(-1.0, 1.0, msg.shape)))
        ob.set_auto_relax(self.auto)
        if self.fixed_mix is not None:
            ob.set_field_mix(self.fixed_mix)
        return og, ob

    def run_oracle(self, orc, perturb=None):
        og, ob = self.oracle(orc, perturb)
        n, last = ob.converge_sync(CRIT, self.tmax, 1.0)
        return ob, n, last


# the field ladder (1, -1) at every tile count QT = ceil(Q / 16) and at the odd / even store paths of k_wsweep
FIELD = [Relax("super3", 9, 1.5, Q, 0, n, (1, -1)) for Q, n in ((17, 102), (33, 121), (40, 114), (49, 113), (64, 114))]
# the window rule (W) and the generic ladder: damped levels, the field level forgotten at the first damped one (the probe
# runs in all of them, damped sweeps included, and finds no period 2)
DAMPED = [
    Relax("super3", 15, 0.75, 17, 0, 357, (0, 2)),
    Relax("diag", 30, 1, 17, 0, 526, (0, 2)),
    Relax("diag", 30, 0.5, 20, 0, 658, (0, 2)),
    Relax("diag", 30, 0.5, 33, 1, 453, (0, 2)),
    Relax("diag", 25, 0.5, 24, 0, 474, (0, 2)),
    Relax("diag", 25, 0.5, 17, 0, 1143, (0, 4), tmax=1500),
    # four tiles of labels. (Here plain Jacobi converges by itself, in 84 sweeps: the swing of the first sweeps fires (F) at
    # sweep 5, the run then crawls at mix 0.25 until (W) at sweep 131 forgets the field level for the first damped one.)
    Relax("diag", 45, 1, 49, 1, 278, (0, 2)),
]
JACOBI_CONVERGES = {DAMPED[-1].id}
# the probe's own escalation (P): three super-groups that repel each other make the messages swing with period 2 while the
# field sums stand still; the 2-step difference k_wsweep reads at sweep 6 sends the run straight to the first damped level
PROBE = [Relax("super3", 1, 3, Q, 0, n, (0, 2)) for Q, n in ((17, 133), (20, 132))]
EXHAUSTED = [Relax("super3", 15, 0.75, 24, 0, -1, (0, 6), tmax=1500)]
NO_AUTO = [Relax("super3", 9, 1.5, 17, 0, -1, (0, -1), tmax=300, auto=False)]
FIXED_MIX = [Relax("super3", 9, 1.5, Q, 0, n, (0, -1), tmax=300, auto=False, fixed_mix=0.25) for Q, n in ((17, 85), (40, 89))]
PERTURB_SEEDS = (1, 2, 3)


# ---------------------------------------------------------------------------------------------------------------------
# B. more than 1024 wide segments
# ---------------------------------------------------------------------------------------------------------------------
WCAP, WRCAP, FOLD_BLOCKS = 64, 16, 256  # kernels_wide.h, engine.hip
# N: (segments, rows per first-stage workgroup, first-stage workgroups, rows of the last one); chunk 0 = single stage
RING_SIZES = {16384: (1024, 0, 0, 0), 16400: (1025, 5, 205, 5), 16432: (1027, 5, 206, 2)}
RING = [(17, 0, 16432), (17, 1, 16432), (33, 0, 16432), (64, 0, 16432), (17, 0, 16384), (17, 0, 16400)]  # (Q, dc, N)
RING_DAMPS = (0.7, 0.7, 1.0, 1.0)  # as tests/test_gpu_wide.py


def ring_pairs(N):
    """ring i - (i + 1) % N plus the chords i - i + N / 2 for i < N / 2, i % 3 != 0: degrees 2 and 3, nothing random"""
    i = np.arange(N)
    c = np.arange(N // 2)
    c = c[c % 3 != 0]
    return np.concatenate([np.stack([i, (i + 1) % N], 1), np.stack([c, c + N // 2], 1)]).astype(np.uint32)


def fold_model(rows):
    """engine.hip fold_stage on `rows` records: (chunk, workgroups, rows of the last workgroup), zeros for a single stage"""
    if rows <= 4 * FOLD_BLOCKS:
        return 0, 0, 0
    chunk = (rows + FOLD_BLOCKS - 1) // FOLD_BLOCKS
    nb = (rows + chunk - 1) // chunk
    return chunk, nb, rows - (nb - 1) * chunk


_RING = {}


def ring_instance(Q, dc, N):
    """cab = (U + U^T) / 2 + 0.35 Q I with U uniform(0.8, 1.2), divided by 9 under degree correction; init flag 1 with every
    ninth vertex clamped to true_conf = i Q // N. (The arrays are shared between the cases: read-only.)"""
    key = (Q, dc, N)
    if key not in _RING:
        rng = np.random.default_rng(9000 + Q)
        U = rng.uniform(0.8, 1.2, size=(Q, Q))
        cab = (U + U.T) / 2 + 0.35 * Q * np.eye(Q)
        if dc:
            cab = cab / 9.0
        tc = (np.arange(N, dtype=np.int64) * Q // N).astype(np.uint32)
        conf = np.where(np.arange(N) % 9 == 0, tc.astype(np.int32), -1).astype(np.int32)
        pairs = ring_pairs(N)
        _RING[key] = dict(N=N, Q=Q, dc=dc, pairs=pairs, tc=tc, cab=cab, na=np.bincount(tc, minlength=Q).astype(np.uint32), conf=conf,
                          flag=1, seed=Q + dc, deg=np.bincount(pairs.astype(np.int64).ravel(), minlength=N))
    return _RING[key]


def ring_oracle(orc, t):
    og = orc.Graph.from_edges(t["pairs"], t["N"])
    ob = orc.OracleBP(og, t["Q"], t["dc"])
    ob.init_messages(t["flag"], t["conf"], t["tc"], orc.Rng(t["seed"]))
    ob.set_params(t["cab"], t["na"], 1.0)
    ob.set_msg_form(True)
    return og, ob
