"""Host-side mirror of the reference's BP interface over the C ABI (include/sbmbp.h).

Names follow the reference (belief_propagation.h:96-142, blockmodel.h:18-107,
graph_utilities.h:14-22). The std::mt19937 engine object of the reference cannot cross the ABI;
`seed` takes its place (the engine draws the same stream from it).
"""
import ctypes as C
import os

import numpy as np

from sbm_bp_amd.capi import (InferResult, LearnResult, Stats, c_dp, c_i32p, c_u32p, c_u64p, check, load_library)


def _dp(a):
    return None if a is None else a.ctypes.data_as(c_dp)


class Graph:
    """Flat CSR adjacency in the engine's layout (replaces adj_list_t, types.h:14-15)."""

    def __init__(self, handle):
        self._lib = load_library()
        self._h = C.c_void_p(handle)
        self.N = self._lib.sbmbp_graph_num_vertices(self._h)
        self.E2 = self._lib.sbmbp_graph_num_directed_edges(self._h)
        self.max_degree = self._lib.sbmbp_graph_max_degree(self._h)

    @classmethod
    def from_edges(cls, pairs, num_vertices=0):
        """edge_to_adj (graph_utilities.cpp:60-77)"""
        lib = load_library()
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        h = C.c_void_p()
        check(lib.sbmbp_graph_from_edges(C.byref(h), pairs.ctypes.data_as(c_u32p), pairs.shape[0], num_vertices))
        return cls(h.value)

    @classmethod
    def from_csr(cls, row_ptr, nbr, rev=None):
        lib = load_library()
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
        nbr = np.ascontiguousarray(nbr, dtype=np.uint32)
        rv = None if rev is None else np.ascontiguousarray(rev, dtype=np.uint32)
        h = C.c_void_p()
        check(lib.sbmbp_graph_from_csr(C.byref(h), len(row_ptr) - 1, len(nbr), row_ptr.ctypes.data_as(c_u64p),
                                       nbr.ctypes.data_as(c_u32p), None if rv is None else rv.ctypes.data_as(c_u32p)))
        return cls(h.value)

    def csr(self):
        row_ptr = np.zeros(self.N + 1, dtype=np.uint64)
        nbr = np.zeros(self.E2, dtype=np.uint32)
        rev = np.zeros(self.E2, dtype=np.uint32)
        check(self._lib.sbmbp_graph_copy_csr(self._h, row_ptr.ctypes.data_as(c_u64p), nbr.ctypes.data_as(c_u32p),
                                             rev.ctypes.data_as(c_u32p)))
        return row_ptr, nbr, rev

    def initial_state(self, Q, flag=0, conf=None, seed=0):
        """the state init_messages (belief_propagation.cpp:101-217) produces from std::mt19937(seed), computed on the
        host without an engine: (psi N x Q, msg_out E2 x Q)"""
        psi = np.empty((self.N, Q), dtype=np.float64)
        msg = np.empty((self.E2, Q), dtype=np.float64)
        cf = None if conf is None else np.ascontiguousarray(conf, dtype=np.int32)
        check(self._lib.sbmbp_host_init_state(self._h, Q, flag, None if cf is None else cf.ctypes.data_as(c_i32p), seed,
                                              psi.ctypes.data_as(c_dp), msg.ctypes.data_as(c_dp)))
        return psi, msg

    def __del__(self):
        try:
            self._lib.sbmbp_graph_destroy(self._h)
        except Exception:
            pass


def load_edge_list(edge_list_path, num_vertices=0):
    """load_edge_list + edge_to_adj (graph_utilities.cpp:42-77). A missing file raises."""
    lib = load_library()
    h = C.c_void_p()
    check(lib.sbmbp_graph_load_edgelist(C.byref(h), os.fsencode(edge_list_path), num_vertices))
    return Graph(h.value)


def coloured_plan(graph, colour=None, step_fraction=0):
    """the plan of the coloured sweep order (sbmbp.h sbmbp_coloured_plan), host only: (n_colours, n_steps, colour[N], step[N]).
    colour=None: the built-in greedy colouring; a caller's colouring is validated (improper: SbmbpError, code -1)"""
    lib = load_library()
    nc, ns = C.c_uint32(0), C.c_uint32(0)
    col = np.zeros(graph.N, dtype=np.uint32)
    st = np.zeros(graph.N, dtype=np.uint32)
    cin = None
    if colour is not None:
        cin = np.ascontiguousarray(colour, dtype=np.uint32)
        if len(cin) != graph.N:
            raise ValueError("colour needs N entries")
    check(lib.sbmbp_coloured_plan(graph._h, None if cin is None else cin.ctypes.data_as(c_u32p), float(step_fraction),
                                  C.byref(nc), C.byref(ns), col.ctypes.data_as(c_u32p), st.ctypes.data_as(c_u32p)))
    return nc.value, ns.value, col, st


def load_beliefs(path):
    """load_beliefs (graph_utilities.cpp:8-23): one int per line, -1 = unknown"""
    return np.loadtxt(path, dtype=np.int32, ndmin=1)


def load_priors(path, N, Q):
    """per-vertex prior file (sbmbp.h sbmbp_prior_load): lines "vertex w_0 ... w_{Q-1}" in any order -> dense (N, Q) table,
    ones where no line names the vertex. A bad file raises SbmbpError (code -5 unreadable, -1 otherwise)"""
    lib = load_library()
    pr = np.empty((int(N), int(Q)), dtype=np.float64)
    given = C.c_uint64(0)
    check(lib.sbmbp_prior_load(os.fsencode(path), int(N), int(Q), pr.ctypes.data_as(c_dp), C.byref(given)))
    return pr


def load_confs(path):
    """load_confs (graph_utilities.cpp:25-40)"""
    return np.loadtxt(path, dtype=np.uint32, ndmin=1)


class blockmodel_t:
    """What BP consumes of blockmodel_t (blockmodel.cpp:7-49, getters :51,:89-101)."""

    def __init__(self, graph, Q, deg_corr_flag=0):
        self.graph, self._Q, self._dc = graph, int(Q), int(deg_corr_flag)

    def get_N(self):
        return self.graph.N

    def get_Q(self):
        return self._Q

    def get_E(self):
        return self.graph.E2 // 2

    def get_deg_corr_flag(self):
        return self._dc

    def get_graph_max_degree(self):
        return self.graph.max_degree


class bp_blockmodel_state:
    """types.h:23-26"""

    def __init__(self, cab, na):
        self.cab = np.ascontiguousarray(cab, dtype=np.float64)
        self.na = np.ascontiguousarray(na, dtype=np.uint32)


def bp_param_from_epsilon_c(blockmodel, epsilon, c):
    """blockmodel.cpp:229-272"""
    lib = load_library()
    Q = blockmodel.get_Q()
    cab = np.zeros((Q, Q))
    na = np.zeros(Q, dtype=np.uint32)
    check(lib.sbmbp_param_from_epsilon_c(blockmodel.get_N(), Q, epsilon, c, _dp(cab), na.ctypes.data_as(c_u32p)))
    return bp_blockmodel_state(cab, na)


def bp_param_from_direct(blockmodel, pa, cab):
    """blockmodel.cpp:274-302 (cab = upper triangle, row-major)"""
    lib = load_library()
    Q = blockmodel.get_Q()
    pa = np.ascontiguousarray(pa, dtype=np.float64)
    cu = np.ascontiguousarray(cab, dtype=np.float64)
    if len(pa) != Q or len(cu) != Q * (Q + 1) // 2:
        raise ValueError("pa needs Q entries and cab Q(Q+1)/2 entries")
    full = np.zeros((Q, Q))
    na = np.zeros(Q, dtype=np.uint32)
    check(lib.sbmbp_param_from_direct(blockmodel.get_N(), Q, _dp(pa), _dp(cu), _dp(full), na.ctypes.data_as(c_u32p)))
    return bp_blockmodel_state(full, na)


class BeliefPropagation:
    """class belief_propagation (belief_propagation.h:18-142) on the GPU engine."""

    conditional = True

    def __init__(self, device=-1):
        self._lib = load_library()
        self._h = None
        self._device = device
        self._beta = 1.0
        self.if_output_marginals_ = False
        self.Q = self.N = self.E2 = 0
        self._prior = None

    def __del__(self):
        try:
            if self._h:
                self._lib.sbmbp_destroy(self._h)
        except Exception:
            pass

    # -- life cycle -------------------------------------------------------------------------
    def bp_allocate(self, blockmodel):
        """belief_propagation.cpp:223-288"""
        if self._h:
            self._lib.sbmbp_destroy(self._h)
            self._h = None
        h = C.c_void_p()
        check(self._lib.sbmbp_create(C.byref(h), blockmodel.graph._h, blockmodel.get_Q(), blockmodel.get_deg_corr_flag(),
                                     self._device))
        self._h = h
        self._graph = blockmodel.graph  # the reference keeps a raw pointer (belief_propagation.h:27)
        self.Q, self.N, self.E2 = blockmodel.get_Q(), blockmodel.get_N(), blockmodel.graph.E2
        # the prior belongs to the engine like the graph: a new engine over a model of the same shape takes it over
        if self._prior is not None and self._prior.shape == (self.N, self.Q):
            check(self._lib.sbmbp_set_vertex_prior(self._h, _dp(self._prior)))
        else:
            self._prior = None

    def init_messages(self, blockmodel, bp_messages_init_flag, conf, true_conf, seed):
        """belief_propagation.cpp:101-217"""
        self.bp_allocate(blockmodel)
        tc = np.ascontiguousarray(true_conf, dtype=np.uint32)
        if len(tc) != self.N:
            raise ValueError("true_conf needs N entries")
        cf = None
        if conf is not None and len(conf):
            cf = np.ascontiguousarray(conf, dtype=np.int32)
            if len(cf) != self.N:
                raise ValueError("conf needs N entries (-1 = unknown)")
        check(self._lib.sbmbp_init_messages(self._h, bp_messages_init_flag, None if cf is None else cf.ctypes.data_as(c_i32p),
                                            tc.ctypes.data_as(c_u32p), seed, int(self.conditional)))

    def init_messages_device(self, blockmodel, true_conf, seed):
        self.bp_allocate(blockmodel)
        tc = np.ascontiguousarray(true_conf, dtype=np.uint32)
        check(self._lib.sbmbp_init_messages_device(self._h, seed, tc.ctypes.data_as(c_u32p)))

    def reinit_messages_device(self, true_conf, seed):
        """the same device-side initial state again on the existing engine (no reallocation)"""
        tc = np.ascontiguousarray(true_conf, dtype=np.uint32)
        check(self._lib.sbmbp_init_messages_device(self._h, seed, tc.ctypes.data_as(c_u32p)))

    def init_special_needs(self, if_output_marginals):
        self.if_output_marginals_ = bool(if_output_marginals)

    def set_beta(self, beta):
        self._beta = float(beta)

    def expand_bp_params(self, state):
        """belief_propagation.cpp:290-317"""
        cab = np.ascontiguousarray(state.cab, dtype=np.float64)
        na = np.ascontiguousarray(state.na, dtype=np.uint32)
        check(self._lib.sbmbp_set_params(self._h, _dp(cab), na.ctypes.data_as(c_u32p), self._beta))

    def set_schedule(self, field_mix=1.0, check_every=1):
        check(self._lib.sbmbp_set_schedule(self._h, field_mix, check_every))

    def set_gather_mode(self, mode=0):
        """0 = automatic (marginal-gather sweep when exact), 1 = always gather messages"""
        check(self._lib.sbmbp_set_gather_mode(self._h, mode))

    def set_auto_relax(self, on=True):
        """adaptive relaxation of converge / inference / learning (sbmbp.h); off = plain synchronous sweeps"""
        check(self._lib.sbmbp_set_auto_relax(self._h, int(on)))

    def relaxation(self):
        """(field level, generic level, field_mix, damping factor) the last converge call ended on; (0, -1, ., 1.0): never relaxed"""
        fl, gl, mix, dmp = C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        check(self._lib.sbmbp_get_relaxation(self._h, C.byref(fl), C.byref(gl), C.byref(mix), C.byref(dmp)))
        return fl.value, gl.value, mix.value, dmp.value

    def set_learning_schedule(self, field_mix=0.3, snap=1.0):
        """field relaxation inside the EM loop's BP runs and the snap tolerance of the group-size truncation (sbmbp.h)"""
        check(self._lib.sbmbp_set_learning_schedule(self._h, field_mix, snap))

    def set_sweep_order(self, order="coloured", colour=None, step_fraction=0):
        """"jacobi" / 0: synchronous sweeps (default); "coloured" / 1: coloured Gauss-Seidel sweeps with the field refreshed
        inside a sweep (sbmbp.h sbmbp_set_sweep_order). colour=None: built-in greedy colouring; step_fraction 0 = 1/8"""
        code = {"jacobi": 0, "coloured": 1}.get(order, order)
        cin = None
        if colour is not None:
            cin = np.ascontiguousarray(colour, dtype=np.uint32)
            if len(cin) != self.N:
                raise ValueError("colour needs N entries")
        check(self._lib.sbmbp_set_sweep_order(self._h, int(code), None if cin is None else cin.ctypes.data_as(c_u32p),
                                              float(step_fraction)))

    def sweep_order(self):
        """(order, n_colours, n_steps); order 0 = synchronous (the counts are 0), 1 = coloured"""
        o, nc, ns = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
        check(self._lib.sbmbp_get_sweep_order(self._h, C.byref(o), C.byref(nc), C.byref(ns)))
        return o.value, nc.value, ns.value

    def set_nonedge_mode(self, mode=0, series_order=0):
        check(self._lib.sbmbp_set_nonedge_mode(self._h, mode, series_order))

    def set_vertex_prior(self, prior):
        """per-vertex label prior (sbmbp.h sbmbp_set_vertex_prior): an (N, Q) array of weights >= 0 with a positive one in
        every row, stored as given; row i is updated with eta_q * prior[i, q] in place of eta_q. None removes the prior.
        Single engine, Q <= 16, synchronous sweep order; while set, the engine runs the message-gather form only"""
        if prior is None:
            check(self._lib.sbmbp_set_vertex_prior(self._h, None))
            self._prior = None
            return
        pr = np.array(prior, dtype=np.float64, order="C")
        if not self._h:  # no engine yet (init_messages allocates it): the library says so
            check(self._lib.sbmbp_set_vertex_prior(None, _dp(pr)))
        if pr.shape != (self.N, self.Q):
            raise ValueError("prior needs shape (N, Q)")
        check(self._lib.sbmbp_set_vertex_prior(self._h, _dp(pr)))
        self._prior = pr

    def vertex_prior(self):
        """the (N, Q) prior table the engine holds, or None"""
        present = C.c_int(0)
        check(self._lib.sbmbp_get_vertex_prior(self._h, None, C.byref(present)))
        if not present.value:
            return None
        pr = np.zeros((self.N, self.Q))
        check(self._lib.sbmbp_get_vertex_prior(self._h, _dp(pr), C.byref(present)))
        return pr

    # -- hot path ---------------------------------------------------------------------------
    def converge(self, conv_crit, time_conv, dumping_rate):
        """belief_propagation.cpp:386-415; returns (niter, last max|delta|)"""
        niter, last = C.c_int(0), C.c_double(0.0)
        check(self._lib.sbmbp_converge(self._h, conv_crit, time_conv, dumping_rate, C.byref(niter), C.byref(last)))
        return niter.value, last.value

    def sweep(self, n_sweeps=1, dumping_rate=1.0, want_diff=True):
        """exactly n_sweeps synchronous sweeps; returns the last max|delta message| (an extra streaming
        pass over both message buffers in the marginal-gather form) unless want_diff is False"""
        if not want_diff:
            check(self._lib.sbmbp_sweep(self._h, dumping_rate, n_sweeps, None))
            return None
        last = C.c_double(0.0)
        check(self._lib.sbmbp_sweep(self._h, dumping_rate, n_sweeps, C.byref(last)))
        return last.value

    def compute_free_energy(self, parts=False):
        f = C.c_double(0.0)
        p = np.zeros(3)
        check(self._lib.sbmbp_free_energy(self._h, C.byref(f), _dp(p)))
        return (f.value, p) if parts else f.value

    def compute_entropy(self, parts=False):
        e = C.c_double(0.0)
        p = np.zeros(3)
        check(self._lib.sbmbp_entropy(self._h, C.byref(e), _dp(p)))
        return (e.value, p) if parts else e.value

    def compute_overlap(self):
        ov = C.c_double(0.0)
        check(self._lib.sbmbp_overlap(self._h, C.byref(ov)))
        return ov.value

    def confusion(self):
        Cm = np.zeros((self.Q, self.Q))
        check(self._lib.sbmbp_confusion(self._h, _dp(Cm)))
        return Cm

    def em_expectations(self, cab=True):
        """compute_na_expect + compute_cab_expect (belief_propagation.cpp:428-440, 892-989), for every Q the engine takes;
        cab=False: the group sizes only (cab_expect comes back as zeros)"""
        na, nna, cabe = np.zeros(self.Q), np.zeros(self.Q), np.zeros((self.Q, self.Q))
        check(self._lib.sbmbp_em_expectations(self._h, _dp(na), _dp(nna), _dp(cabe) if cab else None))
        return na, nna, cabe

    def inference(self, blockmodel, state, conv_crit, time_conv, dumping_rate):
        """belief_propagation.cpp:77-99; returns the result struct (format_infer_line prints it)"""
        self.expand_bp_params(state)
        res = InferResult()
        check(self._lib.sbmbp_inference(self._h, conv_crit, time_conv, dumping_rate, C.byref(res)))
        return res

    def learning(self, blockmodel, state, learning_conv_crit, learning_max_time, learning_rate, dumping_rate):
        """belief_propagation.cpp:14-51"""
        self.expand_bp_params(state)
        res = LearnResult()
        check(self._lib.sbmbp_learning(self._h, learning_conv_crit, learning_max_time, learning_rate, dumping_rate,
                                       C.byref(res)))
        return res

    # -- state access -----------------------------------------------------------------------
    def get_params(self):
        cab = np.zeros((self.Q, self.Q))
        na = np.zeros(self.Q, dtype=np.uint32)
        check(self._lib.sbmbp_get_params(self._h, _dp(cab), na.ctypes.data_as(c_u32p)))
        return cab, na

    def get_state(self, psi=True, msg=True):
        p = np.zeros((self.N, self.Q)) if psi else None
        m = np.zeros((self.E2, self.Q)) if msg else None
        check(self._lib.sbmbp_get_state(self._h, _dp(p), _dp(m)))
        return p, m

    def set_state(self, psi, msg_out):
        p = None if psi is None else np.ascontiguousarray(psi, dtype=np.float64)
        m = None if msg_out is None else np.ascontiguousarray(msg_out, dtype=np.float64)
        check(self._lib.sbmbp_set_state(self._h, _dp(p), _dp(m)))

    def real_psi(self):
        return self.get_state(True, False)[0]

    def h(self):
        h = np.zeros(self.Q)
        check(self._lib.sbmbp_get_field(self._h, _dp(h)))
        return h

    def stats(self):
        s = Stats()
        check(self._lib.sbmbp_get_stats(self._h, C.byref(s)))
        return s

    def reset_stats(self):
        check(self._lib.sbmbp_reset_stats(self._h))

    def set_timing(self, on):
        check(self._lib.sbmbp_set_timing(self._h, int(on)))

    def set_stream(self, hip_stream):
        check(self._lib.sbmbp_set_stream(self._h, C.c_void_p(hip_stream)))


class bp_basic(BeliefPropagation):
    """belief_propagation.cpp:1079-1098 — every row is updated (learn mode, main.cpp:319-320)"""
    conditional = False


class bp_conditional(BeliefPropagation):
    """belief_propagation.cpp:1100-1126 — rows with a planted label are clamped (infer mode)"""
    conditional = True


class ReplicaBatch:
    """R independent BP runs over one graph in one launch sequence per sweep (sbmbp.h: sbmbp_batch_*). Every replica has its
    own initial state, its own (cab, na, beta) and its own convergence and relaxation state; arrays over replicas have
    shape [R, ...]. Q = 2 .. 16, synchronous sweeps in the message-gather form, or coloured sweeps (set_sweep_order)."""

    def __init__(self, graph, Q, deg_corr_flag=0, n_replicas=1, device=-1):
        self._lib = load_library()
        self._h = None
        h = C.c_void_p()
        check(self._lib.sbmbp_batch_create(C.byref(h), graph._h, int(Q), int(deg_corr_flag), int(n_replicas), int(device)))
        self._h = h
        self._graph = graph  # (the batch copies what it needs; kept so that the caller's graph outlives the views it handed out)
        self.R, self.Q, self.N, self.E2 = int(n_replicas), int(Q), graph.N, graph.E2

    def close(self):
        if self._h:
            self._lib.sbmbp_batch_destroy(self._h)
            self._h = None

    def __del__(self):  # the batch holds no pointer into the graph: the order in which the two are collected does not matter
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _replica(self, r):
        r = int(r)
        if r < 0:
            raise ValueError("replica index must be >= 0")
        return r

    # -- state and parameters ---------------------------------------------------------------
    def init_messages(self, bp_messages_init_flag, conf, true_conf, seeds, conditional=True):
        """replica r starts bit for bit as BeliefPropagation.init_messages(..., seeds[r]) does"""
        tc = np.ascontiguousarray(true_conf, dtype=np.uint32)
        if len(tc) != self.N:
            raise ValueError("true_conf needs N entries")
        cf = None
        if conf is not None and len(conf):
            cf = np.ascontiguousarray(conf, dtype=np.int32)
            if len(cf) != self.N:
                raise ValueError("conf needs N entries (-1 = unknown)")
        sd = np.ascontiguousarray(seeds, dtype=np.uint32)
        if len(sd) != self.R:
            raise ValueError("seeds needs one entry per replica")
        check(self._lib.sbmbp_batch_init_messages(self._h, bp_messages_init_flag, None if cf is None else cf.ctypes.data_as(c_i32p),
                                                  tc.ctypes.data_as(c_u32p), sd.ctypes.data_as(c_u32p), int(conditional)))

    def init_messages_device(self, true_conf, seeds):
        tc = np.ascontiguousarray(true_conf, dtype=np.uint32)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        if len(sd) != self.R:
            raise ValueError("seeds needs one entry per replica")
        check(self._lib.sbmbp_batch_init_messages_device(self._h, sd.ctypes.data_as(c_u64p), tc.ctypes.data_as(c_u32p)))

    def set_params(self, state, beta=1.0, replica=-1):
        """replica = -1: all replicas"""
        cab = np.ascontiguousarray(state.cab, dtype=np.float64)
        na = np.ascontiguousarray(state.na, dtype=np.uint32)
        check(self._lib.sbmbp_batch_set_params(self._h, int(replica), _dp(cab), na.ctypes.data_as(c_u32p), float(beta)))

    def get_params(self, replica):
        cab = np.zeros((self.Q, self.Q))
        na = np.zeros(self.Q, dtype=np.uint32)
        beta = C.c_double(0.0)
        check(self._lib.sbmbp_batch_get_params(self._h, self._replica(replica), _dp(cab), na.ctypes.data_as(c_u32p), C.byref(beta)))
        return cab, na, beta.value

    def get_state(self, replica, psi=True, msg=True):
        p = np.zeros((self.N, self.Q)) if psi else None
        m = np.zeros((self.E2, self.Q)) if msg else None
        check(self._lib.sbmbp_batch_get_state(self._h, self._replica(replica), _dp(p), _dp(m)))
        return p, m

    def set_state(self, replica, psi, msg_out):
        p = None if psi is None else np.ascontiguousarray(psi, dtype=np.float64)
        m = None if msg_out is None else np.ascontiguousarray(msg_out, dtype=np.float64)
        check(self._lib.sbmbp_batch_set_state(self._h, self._replica(replica), _dp(p), _dp(m)))

    def h(self, replica):
        h = np.zeros(self.Q)
        check(self._lib.sbmbp_batch_get_field(self._h, self._replica(replica), _dp(h)))
        return h

    def set_vertex_prior(self, prior, replica=-1):
        """per-vertex label priors (sbmbp.h sbmbp_batch_set_vertex_prior): an (N, Q) array as BeliefPropagation.set_vertex_prior
        takes it, or None. replica = -1: every replica reads this ONE table (stored once), or with None all tables are removed;
        replica = r: replica r gets a table of its own (overriding the shared one), or with None reads none"""
        replica = int(replica)
        if prior is None:
            check(self._lib.sbmbp_batch_set_vertex_prior(self._h, replica, None))
            return
        pr = np.array(prior, dtype=np.float64, order="C")
        if pr.shape != (self.N, self.Q):
            raise ValueError("prior needs shape (N, Q)")
        check(self._lib.sbmbp_batch_set_vertex_prior(self._h, replica, _dp(pr)))

    def vertex_prior(self, replica):
        """(state, table) of replica: state 0 = none (table None), 1 = the batch's shared table, 2 = its own; table (N, Q)"""
        present = C.c_int(0)
        check(self._lib.sbmbp_batch_get_vertex_prior(self._h, self._replica(replica), None, C.byref(present)))
        if not present.value:
            return 0, None
        pr = np.zeros((self.N, self.Q))
        check(self._lib.sbmbp_batch_get_vertex_prior(self._h, self._replica(replica), _dp(pr), C.byref(present)))
        return present.value, pr

    def relaxation(self, replica):
        """(field level, generic level, field_mix, damping factor) replica's last converge call ended on"""
        fl, gl, mix, dmp = C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        check(self._lib.sbmbp_batch_get_relaxation(self._h, self._replica(replica), C.byref(fl), C.byref(gl), C.byref(mix), C.byref(dmp)))
        return fl.value, gl.value, mix.value, dmp.value

    def set_schedule(self, field_mix=1.0, check_every=1):
        check(self._lib.sbmbp_batch_set_schedule(self._h, field_mix, check_every))

    def set_auto_relax(self, on=True):
        check(self._lib.sbmbp_batch_set_auto_relax(self._h, int(on)))

    def set_nonedge_mode(self, mode=0, series_order=0):
        check(self._lib.sbmbp_batch_set_nonedge_mode(self._h, mode, series_order))

    def set_sweep_order(self, order="coloured", colour=None, step_fraction=0):
        """the sweep order of all replicas, as BeliefPropagation.set_sweep_order takes it: "jacobi" / 0 = synchronous (default),
        "coloured" / 1 = coloured Gauss-Seidel sweeps with the field refreshed inside a sweep (sbmbp.h
        sbmbp_batch_set_sweep_order). colour=None: built-in greedy colouring; step_fraction 0 = 1/8. Every replica keeps its state"""
        code = {"jacobi": 0, "coloured": 1}.get(order, order)
        cin = None
        if colour is not None:
            cin = np.ascontiguousarray(colour, dtype=np.uint32)
            if len(cin) != self.N:
                raise ValueError("colour needs N entries")
        check(self._lib.sbmbp_batch_set_sweep_order(self._h, int(code), None if cin is None else cin.ctypes.data_as(c_u32p),
                                                    float(step_fraction)))

    @property
    def sweep_order(self):
        """(order, n_colours, n_steps), the tuple BeliefPropagation.sweep_order() returns: order 0 = synchronous (the counts
        are 0), 1 = coloured"""
        o, nc, ns = C.c_int(0), C.c_uint32(0), C.c_uint32(0)
        check(self._lib.sbmbp_batch_get_sweep_order(self._h, C.byref(o), C.byref(nc), C.byref(ns)))
        return o.value, nc.value, ns.value

    # -- hot path ---------------------------------------------------------------------------
    def sweep(self, n_sweeps=1, dumping_rate=1.0):
        """exactly n_sweeps sweeps of every replica; returns the last max|delta message| of each, shape [R]"""
        last = np.zeros(self.R)
        check(self._lib.sbmbp_batch_sweep(self._h, dumping_rate, n_sweeps, _dp(last)))
        return last

    def converge(self, conv_crit, time_conv, dumping_rate):
        """(niter [R], last max|delta| [R]): each replica stops at its own sweep and keeps the state of that sweep"""
        niter = np.zeros(self.R, dtype=np.int32)
        last = np.zeros(self.R)
        check(self._lib.sbmbp_batch_converge(self._h, conv_crit, time_conv, dumping_rate, niter.ctypes.data_as(C.POINTER(C.c_int)), _dp(last)))
        return niter, last

    def compute_free_energy(self, parts=False):
        f = np.zeros(self.R)
        p = np.zeros((self.R, 3))
        check(self._lib.sbmbp_batch_free_energy(self._h, _dp(f), _dp(p)))
        return (f, p) if parts else f

    def compute_entropy(self, parts=False):
        e = np.zeros(self.R)
        p = np.zeros((self.R, 3))
        check(self._lib.sbmbp_batch_entropy(self._h, _dp(e), _dp(p)))
        return (e, p) if parts else e

    def compute_overlap(self):
        ov = np.zeros(self.R)
        check(self._lib.sbmbp_batch_overlap(self._h, _dp(ov)))
        return ov

    def em_expectations(self, replica, cab=True):
        na, nna, cabe = np.zeros(self.Q), np.zeros(self.Q), np.zeros((self.Q, self.Q))
        check(self._lib.sbmbp_batch_em_expectations(self._h, self._replica(replica), _dp(na), _dp(nna), _dp(cabe) if cab else None))
        return na, nna, cabe

    def set_learning_schedule(self, field_mix=0.3, snap=1.0):
        """the two schedule rules of the EM loop (BeliefPropagation.set_learning_schedule), common to all replicas"""
        check(self._lib.sbmbp_batch_set_learning_schedule(self._h, field_mix, snap))

    def em_step(self):
        """the reductions of one EM step for every replica from one launch sequence:
        (na_expect [R, Q], nna_expect [R, Q], cab_expect [R, Q, Q], free energy [R], its parts [R, 3])"""
        na, nna = np.zeros((self.R, self.Q)), np.zeros((self.R, self.Q))
        cabe, f, parts = np.zeros((self.R, self.Q, self.Q)), np.zeros(self.R), np.zeros((self.R, 3))
        check(self._lib.sbmbp_batch_em_step(self._h, _dp(na), _dp(nna), _dp(cabe), _dp(f), _dp(parts)))
        return na, nna, cabe, f, parts

    def learning(self, learning_conv_crit, learning_max_time, learning_rate, dumping_rate):
        """multi-start EM: every replica learns from its own state and parameters, in lock-step rounds.
        Returns (list of R LearnResult, eta [R, Q], cab [R, Q, Q], index of the best replica)."""
        res = (LearnResult * self.R)()
        eta, cab = np.zeros((self.R, self.Q)), np.zeros((self.R, self.Q, self.Q))
        best = C.c_uint32(0)
        check(self._lib.sbmbp_batch_learning(self._h, learning_conv_crit, learning_max_time, learning_rate, dumping_rate, res, _dp(eta), _dp(cab),
                                             C.byref(best)))
        return list(res), eta, cab, best.value

    def inference(self, conv_crit, time_conv, dumping_rate):
        """inference of every replica: (list of R result structs, index of the replica of lowest free energy)"""
        res = (InferResult * self.R)()
        best = C.c_uint32(0)
        check(self._lib.sbmbp_batch_inference(self._h, conv_crit, time_conv, dumping_rate, res, C.byref(best)))
        return list(res), best.value

    def stats(self):
        s = Stats()
        check(self._lib.sbmbp_batch_get_stats(self._h, C.byref(s)))
        return s

    # -- agreement of the replicas (sbmbp.h sbmbp_batch_agreement) --------------------------------
    def agreement(self, kind="hard", replicas=None):
        """pairwise agreement of the listed replicas (None = all R, in index order): (overlap[n, n], confusion[n, n, Q, Q],
        perm[n, n, Q]). kind "soft" / "hard_soft" / "hard" (or 0 / 1 / 2) selects the confusion matrix; overlap[x, y] is its
        best trace / N over ALL relabellings and perm[x, y, a] the label of y that label a of x corresponds to. Reads the
        marginals where they lie on the device and changes nothing."""
        k = AGREEMENT_KINDS[kind] if isinstance(kind, str) else int(kind)
        lst = None
        n = self.R
        if replicas is not None:
            lst = np.ascontiguousarray(replicas, dtype=np.uint32).ravel()
            n = len(lst)
            if n == 0:  # an empty list is refused by the library, which needs a pointer that is not NULL to tell it from "all"
                lst = np.zeros(1, dtype=np.uint32)
        Q = self.Q
        conf = np.zeros((n, n, Q, Q))
        ov = np.zeros((n, n))
        perm = np.zeros((n, n, Q), dtype=np.uint32)
        check(self._lib.sbmbp_batch_agreement(self._h, k, None if lst is None else lst.ctypes.data_as(c_u32p), n, _dp(conf), _dp(ov),
                                              perm.ctypes.data_as(c_u32p)))
        return ov, conf, perm

    def agreement_groups(self, threshold, kind="hard", replicas=None):
        """(group[n], n_groups, overlap): the groups of agreement_groups() on the overlap matrix of agreement(kind, replicas)"""
        ov = self.agreement(kind, replicas)[0]
        group, n_groups = agreement_groups(ov, threshold)
        return group, n_groups, ov


AGREEMENT_KINDS = {"soft": 0, "hard_soft": 1, "hard": 2}


def agreement_groups(overlap, threshold):
    """groups of runs from an n x n overlap matrix (sbmbp.h sbmbp_agreement_groups; host only, no GPU): run x joins the group of
    the first earlier group leader g with overlap[g, x] >= threshold, else it leads a new group. Returns (group[n], n_groups)."""
    ov = np.ascontiguousarray(overlap, dtype=np.float64)
    if ov.ndim != 2 or ov.shape[0] != ov.shape[1]:
        raise ValueError("overlap must be a square matrix")
    n = ov.shape[0]
    group = np.zeros(n, dtype=np.uint32)
    ng = C.c_uint32(0)
    check(load_library().sbmbp_agreement_groups(n, _dp(ov), float(threshold), group.ctypes.data_as(c_u32p), C.byref(ng)))
    return group, ng.value


def format_infer_line(res):
    """the stdout line of belief_propagation.cpp:88 at the default 6 significant digits"""
    def g(x):
        return "-nan" if x != x else "%g" % x
    return "%s %s %s %d \n" % (g(res.entropy), g(res.free_energy), g(res.overlap), res.niter)
