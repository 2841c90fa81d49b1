// Device engine + C ABI (include/sbmbp.h). Host logic is C++14; kernels are in kernels.h.
// There is no CPU fallback anywhere in this file: without a GPU sbmbp_create fails with
// SBMBP_ERR_NODEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <string>
#include <memory>
#include <vector>

#include "../../include/sbmbp.h"
#include "device_buffer.h"
#include "host_graph.h"
#include "host_loops.h"
#include "host_reduce.h"
#include "kernels.h"
#include "kernels_wide.h"
#include "kernels_batch.h"

using namespace sbmbp;

#define HIPCHK(call)                                                                          \
    do {                                                                                      \
        hipError_t _e = (call);                                                               \
        if (_e != hipSuccess) {                                                               \
            set_error(std::string(#call) + ": " + hipGetErrorString(_e));                     \
            return SBMBP_ERR_HIP;                                                             \
        }                                                                                     \
    } while (0)

#define CHK(call)                  \
    do {                           \
        int _r = (call);           \
        if (_r != SBMBP_OK) return _r; \
    } while (0)

struct conv_state { double maxdiff; int conv_iter, sweep_idx, stop, have_prev, hinted, exact, last_exact, pause, ar_fl, ar_gl; };
static_assert(offsetof(dev_params, ar_gl) - offsetof(dev_params, maxdiff) == offsetof(conv_state, ar_gl), "conv_state mirrors dev_params from maxdiff on");

// The engine's stream and events, as a base of the engine: the buffers are members of sbmbp_engine, so they are released after
// ~sbmbp_engine has drained the stream and before this destructor destroys it.
struct engine_stream {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t ev_cs[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> ev;  // the pool of the sweep timing
    ~engine_stream() {
        for (auto x : ev) (void)hipEventDestroy(x);
        for (auto x : ev_cs) if (x) (void)hipEventDestroy(x);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

struct sbmbp_engine : engine_stream {
    uint32_t N = 0, Q = 0, dc = 0;  // N = rows this engine updates (all vertices, or the owned range of a shard)
    bool wide = false;              // Q > 16: the matrix-core kernels of kernels_wide.h (full Q-component message records)
    device_buffer<dev_wide> d_Pw;
    uint64_t E2 = 0;
    // sharding (sbmbp_shard_create): marginal table = owned rows followed by halo vertices
    bool sharded = false;
    uint32_t Nglob = 0, n_halo = 0, row0 = 0;
    uint64_t edge0 = 0;
    device_buffer<double> d_red;  // shards: the reduction hand-off buffer, borrowed from the caller (sbmbp_shard_desc::red_buf)
    device_buffer<double> d_Min;  // shards: materialised incoming messages for the reductions (allocated on first use)
    device_buffer<uint32_t> d_snd_ptr, d_snd_slot;  // shards: fused exchange buffers (sbmbp_shard_set_io)
    double *io_sendbuf = nullptr;
    const double *io_stage[2] = {nullptr, nullptr};
    uint32_t io_ncomp = 0;
    std::vector<uint32_t> chunk_blk, chunk_hub;  // per row chunk: first segment / first hub row (n_chunks+1 entries)
    // graph + work decomposition in HBM
    device_buffer<uint32_t> d_row_ptr, d_rev, d_nbr, d_src;
    device_buffer<uint32_t> d_deg;     // dc 2: degree of every row of the marginal table (own rows, then halo vertices on a shard)
    uint64_t n_halo_msgs = 0;      // shards: message records received from peers, kept behind the own records (rev points there)
    int incoming_src = 0;          // shards, reductions: 0 = incoming messages materialised from the marginals, 1 = gathered through rev
    device_buffer<uint32_t> d_blk_row, d_blk_e0, d_hub_row, d_hub_blk, d_true;
    // hub rows cut into fragments of BLOCK edges (marginal-gather sweep: k_hub_frag_product / k_hub_frag_cavity)
    device_buffer<uint32_t> d_frag_hub, d_hub_frag0;
    device_buffer<double> d_hub_b, d_hub_pA;
    device_buffer<int> d_hub_pE;
    uint32_t n_frag = 0;
    uint64_t hub_edges = 0;
    std::vector<uint32_t> h_hub_frag0;  // [n_hub + 1]
    device_buffer<uint32_t> d_fold_counters;  // arrival counter of k_fold_finalize (zero between launches)
    device_buffer<int32_t> d_clamp;
    device_buffer<double> d_prior;  // per-vertex prior [N*Q] (sbmbp_set_vertex_prior), or null: none. Belongs to the engine like the graph
    uint32_t n_blk = 0, n_hub = 0;
    // state in HBM
    // (borrowed: d_psi of a shard is the caller's, sbmbp_shard_desc::psi_buf0/1; d_M, d_psi, d_P and d_prior of a batch's engine
    // point into the batch's buffers while a replica is bound)
    device_buffer<double> d_M[2];
    int cur = 0;
    device_buffer<double> d_psi[2];  // marginals, double buffered (the marginal-gather sweep reads one, writes the other)
    int pcur = 0;
    device_buffer<dev_params> d_P;
    device_buffer<double> d_partials;  // grown on demand (ensure_partials)
    device_buffer<double> d_stage;  // first-stage fold output: FOLD_BLOCKS rows
    device_buffer<double> d_small;  // folded results, grown on demand
    device_buffer<double> d_hist;
    uint32_t hist_cap = 0;
    device_buffer<double> d_mats;  // 3 * Q*Q small matrices for the non-edge kernels
    uint64_t device_bytes = 0;
    // host mirrors
    std::vector<double> cab, W;
    std::vector<uint32_t> na;
    std::vector<double> eta;
    std::vector<uint32_t> true_conf;
    std::vector<uint32_t> h_row_ptr;  // host copy of the row offsets (fill order of init_messages)
    double beta = 1.0;
    double sum_log_didl = 0.0;  // sum over directed edges of log(d_i d_l) (dc 1 constant of f_site/f_edge)
    bool have_params = false, have_state = false, has_clamp = false, field_fresh = false;
    pinned_buffer<conv_state> h_cs;  // two convergence-state slots for the pipelined batch loop (with ev_cs)
    bool init_from_psi = false;  // device initialisation: every message equals its sender's marginal, so the first
                                 // marginal-gather sweep takes the neighbours' marginals as the incoming messages
    bool clamp_onehot = false;  // the clamped rows hold the one-hot state of init flag 1/3: the marginal-gather sweep stays exact
    bool w_positive = false;     // every cab entry > 0: the marginal-gather sweep is well defined
    bool psi_consistent = false; // psi == marginals of the message pair held in d_M (set by an undamped sweep)
    int gather_mode = 0;         // 0 = automatic, 1 = always gather messages (explicit form)
    uint64_t psi_sweeps = 0;     // sweeps executed by k_sweep_psi
    double field_mix = 1.0;
    // results of the fused reduction pass (k_fe_psi) for the current state: inference and every EM step ask for the site /
    // edge terms, the adjacent pairs of the non-edge term and the EM numerators one after the other; one pass serves them all
    struct { bool valid = false, entropy = false, em = false; double se[4] = {0, 0, 0, 0}, adj[2] = {0, 0}; std::vector<double> tri; } fz;
    int fused_reductions = 1;    // 0: always the separate kernels (SBMBP_FUSED_REDUCTIONS=0)
    bool auto_relax = true;      // adaptive relaxation of converge (sbmbp_set_auto_relax; kernels.h dev_params::ar_*)
    int ar_fl = 0, ar_gl = -1;   // levels the last converge call ended on
    double learn_field_mix = 0.3, learn_snap = 1.0;  // sbmbp_set_learning_schedule
    uint32_t check_every = 1;
    int nonedge_mode = 0, series_order = 0;
    // coloured sweep order (sbmbp_set_sweep_order; kernels.h k_sweep_step): per step a row list cut into segments, and the
    // step's hub rows in a fragment table of their own (the scratch of the fragments, d_hub_b / pA / pE, is shared)
    int sweep_order = 0;
    bool cs_last = false;  // the last sweeps ran in the coloured order: the field on the device followed them step by step
    uint32_t cs_colours = 0, cs_steps = 0, cs_max_rec = 0;
    std::vector<uint32_t> cs_seg0, cs_hub0, cs_frag0;  // [cs_steps + 1]: first segment / hub / fragment of every step
    struct coloured_tables {
        device_buffer<uint32_t> rows, loff, seg_row0, hub_row, hub_rec, frag_hub, hub_frag0;
    } cs;
    // stats
    uint64_t sweeps = 0, sweep_launches = 0;
    double sweep_ms = 0.0;
    bool timing = false;
    size_t ev_used = 0;
    ~sbmbp_engine() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

// The current device is a per-thread setting of the HIP runtime: every entry point that takes an engine selects the
// engine's GPU for the duration of the call and puts the caller's choice back (a process may hold engines on several GPUs).
struct device_scope {
    int prev = -1;
    explicit device_scope(const sbmbp_engine *e) {
        if (e && hipGetDevice(&prev) == hipSuccess && prev != e->device) (void)hipSetDevice(e->device);
        else prev = -1;
    }
    ~device_scope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

namespace {

// memory of the engine (and of its batch): counted in device_bytes
template <typename T> int dev_alloc(sbmbp_engine *e, device_buffer<T> &b, size_t count) { return b.alloc(count, &e->device_bytes); }
int ensure_partials(sbmbp_engine *e, size_t doubles) { return e->d_partials.ensure(doubles, &e->device_bytes); }
int ensure_small(sbmbp_engine *e, size_t doubles) { return e->d_small.ensure(doubles, &e->device_bytes); }

// dev_alloc and the copy of n host values behind it on the engine's stream (none when n is 0): complete at the caller's
// next synchronisation, until which the host array must live
template <typename T> int dev_upload(sbmbp_engine *e, device_buffer<T> &b, const T *h, size_t n) {
    CHK(dev_alloc(e, b, n));
    if (n) HIPCHK(hipMemcpyAsync(b, h, n * sizeof(T), hipMemcpyHostToDevice, e->stream));
    return SBMBP_OK;
}
template <typename T> int dev_upload(sbmbp_engine *e, device_buffer<T> &b, const std::vector<T> &h) { return dev_upload(e, b, h.data(), h.size()); }

constexpr uint32_t FOLD_BLOCKS = 256, FOLD_STRIDE_MAX = 128;

// two-stage fold: when there are many partial rows, reduce them to FOLD_BLOCKS rows first.
// Returns the pointer/row count the final single-workgroup stage should read.
const double *fold_stage(sbmbp_engine *e, uint32_t *rows, int ncols_sum, int has_max, uint32_t stride) {
    if (*rows <= 4 * FOLD_BLOCKS || stride > FOLD_STRIDE_MAX) return e->d_partials;
    const uint32_t chunk = (*rows + FOLD_BLOCKS - 1) / FOLD_BLOCKS;
    const uint32_t nb = (*rows + chunk - 1) / chunk;
    hipLaunchKernelGGL(k_fold_stage, dim3(nb), dim3(BLOCK), 0, e->stream, e->d_partials, *rows, chunk, ncols_sum, has_max,
                       stride, e->d_stage);
    *rows = nb;
    return e->d_stage;
}

inline int frame_cap(uint32_t Q) {
    if (Q > 16) return WCAP;
    return (Q <= 4 ? FTPB : SBMBP_FRAME_TPB_HI) * (Q <= 2 ? SBMBP_EPT_LO : (Q <= 4 ? SBMBP_EPT_MID : (Q <= 8 ? SBMBP_EPT_HI : 1)));
}
inline int frame_rcap(uint32_t Q) { if (Q > 16) return WRCAP; const int cap = frame_cap(Q); return cap / 2 > 64 ? cap / 2 : 64; }
inline size_t rec_len(const sbmbp_engine *e) { return e->wide ? e->Q : e->Q - 1; }  // doubles per message record in HBM

// label counts above 16: QT = tiles of 16 labels (kernels_wide.h)
#define DISPATCH_QT(Qv, ...)                                            \
    switch (((Qv) + 15) / 16) {                                         \
        case 2: { constexpr int QT = 2; __VA_ARGS__; } break;           \
        case 3: { constexpr int QT = 3; __VA_ARGS__; } break;           \
        case 4: { constexpr int QT = 4; __VA_ARGS__; } break;           \
        default: set_error("unsupported Q"); return SBMBP_ERR_UNSUPPORTED; \
    }

// Q/dc dispatch over the templated kernels. -DSBMBP_ONLY_Q=<q> instantiates ONE label count: tuning builds that compile in a
// fraction of the time (sbm_bp_amd.build.build_variant; never the shipped library).
#ifdef SBMBP_ONLY_Q
#define DISPATCH_Q(Qv, ...)                                             \
    switch (Qv) {                                                       \
        case SBMBP_ONLY_Q: { constexpr int QQ = SBMBP_ONLY_Q; __VA_ARGS__; } break; \
        default: set_error("this tuning build holds one label count only"); return SBMBP_ERR_UNSUPPORTED; \
    }
#else
#define DISPATCH_Q(Qv, ...)                                             \
    switch (Qv) {                                                       \
        case 2: { constexpr int QQ = 2; __VA_ARGS__; } break;           \
        case 3: { constexpr int QQ = 3; __VA_ARGS__; } break;           \
        case 4: { constexpr int QQ = 4; __VA_ARGS__; } break;           \
        case 5: { constexpr int QQ = 5; __VA_ARGS__; } break;           \
        case 6: { constexpr int QQ = 6; __VA_ARGS__; } break;           \
        case 7: { constexpr int QQ = 7; __VA_ARGS__; } break;           \
        case 8: { constexpr int QQ = 8; __VA_ARGS__; } break;           \
        case 9: { constexpr int QQ = 9; __VA_ARGS__; } break;           \
        case 10: { constexpr int QQ = 10; __VA_ARGS__; } break;         \
        case 11: { constexpr int QQ = 11; __VA_ARGS__; } break;         \
        case 12: { constexpr int QQ = 12; __VA_ARGS__; } break;         \
        case 13: { constexpr int QQ = 13; __VA_ARGS__; } break;         \
        case 14: { constexpr int QQ = 14; __VA_ARGS__; } break;         \
        case 15: { constexpr int QQ = 15; __VA_ARGS__; } break;         \
        case 16: { constexpr int QQ = 16; __VA_ARGS__; } break;         \
        default: set_error("unsupported Q"); return SBMBP_ERR_UNSUPPORTED; \
    }
#endif

// The label count and ONE run-time bool bound together: the statement sees QQ (QT) and `constexpr bool BB`, so a kernel with
// a bool template parameter is launched by one statement with one argument list.
#define DISPATCH_QB(Qv, flag, ...)                                                      \
    do {                                                                                \
        if (flag) { DISPATCH_Q(Qv, { constexpr bool BB = true; __VA_ARGS__; }) }        \
        else { DISPATCH_Q(Qv, { constexpr bool BB = false; __VA_ARGS__; }) }            \
    } while (0)
#define DISPATCH_QTB(Qv, flag, ...)                                                     \
    do {                                                                                \
        if (flag) { DISPATCH_QT(Qv, { constexpr bool BB = true; __VA_ARGS__; }) }       \
        else { DISPATCH_QT(Qv, { constexpr bool BB = false; __VA_ARGS__; }) }           \
    } while (0)

// Kernels that exist for a range of label counts only (k_fe_psi<Q, true> up to 8, k_em_edges_batch above EM_FRAME_QMAX) are
// named with q_clamp(QQ, lo, hi) in a dispatch: outside the range, where a run-time test keeps the launch from happening,
// the statement names an instantiation that exists anyway and adds none.
constexpr int q_clamp(int q, int lo, int hi) { return q < lo ? lo : (q > hi ? hi : q); }

// Event pair around what a sweep times (collect_timing adds the pairs up). timing_begin grows the pool, records the first
// event on st and leaves the second in *stop for timing_end; *stop is null when timing is off or there is nothing to time.
int timing_begin(sbmbp_engine *e, hipStream_t st, bool anything, hipEvent_t *stop) {
    *stop = nullptr;
    if (!e->timing || !anything) return SBMBP_OK;
    if (e->ev_used + 2 > e->ev.size()) {
        size_t old = e->ev.size();
        e->ev.resize(old + 256);
        for (size_t i = old; i < e->ev.size(); ++i) HIPCHK(hipEventCreate(&e->ev[i]));
    }
    const hipEvent_t start = e->ev[e->ev_used++];
    *stop = e->ev[e->ev_used++];
    HIPCHK(hipEventRecord(start, st));
    return SBMBP_OK;
}
int timing_end(hipEvent_t stop, hipStream_t st) {
    if (stop) HIPCHK(hipEventRecord(stop, st));
    return SBMBP_OK;
}

// The buffers of sweep j of the running call: message and marginal buffers alternate per sweep, from the engine's current pair.
struct sweep_bufs {
    int pc;  // index of the marginal table the sweep reads
    const double *Mold;
    double *Mnew;
    const double *psi_old;
    double *psi_new;
    const int32_t *clamp;
};
sweep_bufs bufs_of_sweep(const sbmbp_engine *e, uint32_t j) {
    const int mc = (e->cur + int(j)) & 1, pc = (e->pcur + int(j)) & 1;
    return sweep_bufs{pc, e->d_M[mc], e->d_M[mc ^ 1], e->d_psi[pc], e->d_psi[pc ^ 1], e->has_clamp ? e->d_clamp.get() : nullptr};
}

int upload_params(sbmbp_engine *e, double crit, bool hinted = false) {
    dev_params P;
    std::memset(&P, 0, sizeof P);
    const uint32_t Q = e->Q;
    if (e->wide) {  // the Q x Q matrices and Q-vectors live in dev_wide; dev_params keeps the scalars and the convergence state
        std::unique_ptr<dev_wide> Wd(new dev_wide());
        std::memset(Wd.get(), 0, sizeof(dev_wide));
        std::vector<double> cl(Q * Q);
        for (uint32_t a = 0; a < Q * Q; ++a) {
            Wd->cab[a] = e->cab[a];
            Wd->W[a] = (e->dc == 0) ? std::pow(e->cab[a], e->beta) : e->cab[a];
            Wd->logcab[a] = std::log(e->cab[a]);
            cl[a] = e->cab[a] * Wd->logcab[a];
        }
        for (uint32_t q = 0; q < Q; ++q) { Wd->eta[q] = e->eta[q]; Wd->logeta[q] = std::log(e->eta[q]); }
        wide_tiles(Wd->W, int(Q), Wd->tW);
        wide_tiles_v(Wd->W, int(Q), Wd->tWv);
        wide_tiles(Wd->cab, int(Q), Wd->tC);
        wide_tiles(cl.data(), int(Q), Wd->tCL);
        HIPCHK(hipMemcpyAsync(e->d_Pw, Wd.get(), sizeof(dev_wide), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    } else
    for (uint32_t a = 0; a < Q * Q; ++a) {
        P.cab[a] = e->cab[a];
        P.W[a] = (e->dc == 0) ? std::pow(e->cab[a], e->beta) : (e->dc == 1 ? e->cab[a] : e->cab[a] / double(e->Nglob));
    }
    for (uint32_t q = 0; q < Q && !e->wide; ++q) {
        P.eta[q] = e->eta[q];
        P.logeta[q] = std::log(e->eta[q]);
    }
    for (uint32_t a = 0; a < Q * Q && !e->wide; ++a) P.logcab[a] = std::log(e->cab[a]);
    P.beta = e->beta;
    P.invN = 1.0 / double(e->Nglob);
    P.field_mix = e->field_mix;
    P.crit = crit;
    P.maxdiff = 0.0;
    P.conv_iter = -1;
    P.sweep_idx = 0;
    P.stop = 0;
    P.have_prev = 0;
    P.hinted = hinted ? 1 : 0;  // the sweeps of this run report 2-step hints until k_finalize arms the exact criterion
    P.exact = 0;
    P.last_exact = 1;
    P.pause = 0;
    P.ar_on = (e->auto_relax && crit >= 0) ? 1 : 0;  // fixed sweep counts (crit < 0) are plain Jacobi sweeps
    P.ar_psi_ok = hinted ? 1 : 0;
    P.ar_gl = -1;
    P.ar_base_mix = e->field_mix;
    P.damp_auto = 1.0;
    P.ar_v1 = P.ar_v2 = P.ar_pmin = P.ar_d1p = -1.0;
    P.ar_wmin = 1e300;
    HIPCHK(hipMemcpyAsync(e->d_P, &P, sizeof P, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));  // P is a stack object
    return SBMBP_OK;
}

// Fragment tables of the hub rows (kernels.h: hub_frags): hub h owns fragments hub_frag0[h] .. hub_frag0[h+1], of BLOCK
// edges each (the last one shorter). The edge-field scratch costs 8 Q bytes per hub edge, rounded up to whole fragments.
int setup_hub_frags(sbmbp_engine *e, const std::vector<uint32_t> &hub_row, const std::vector<uint32_t> &rp32) {
    std::vector<uint32_t> frag_hub;
    e->h_hub_frag0.assign(1, 0u);
    for (size_t h = 0; h < hub_row.size(); ++h) {
        const uint32_t d = rp32[hub_row[h] + 1] - rp32[hub_row[h]];
        e->hub_edges += d;
        for (uint32_t k = 0; k < (d + BLOCK - 1) / BLOCK; ++k) frag_hub.push_back(uint32_t(h));
        e->h_hub_frag0.push_back(uint32_t(frag_hub.size()));
    }
    e->n_frag = uint32_t(frag_hub.size());
    if (!e->n_frag) return SBMBP_OK;
    CHK(dev_upload(e, e->d_frag_hub, frag_hub));
    CHK(dev_upload(e, e->d_hub_frag0, e->h_hub_frag0));
    CHK(dev_alloc(e, e->d_hub_b, size_t(e->n_frag) * BLOCK * e->Q));
    CHK(dev_alloc(e, e->d_hub_pA, size_t(e->n_frag) * e->Q));
    CHK(dev_alloc(e, e->d_hub_pE, size_t(e->n_frag) * e->Q));
    HIPCHK(hipStreamSynchronize(e->stream));  // frag_hub is a local
    return SBMBP_OK;
}

// What every engine holds of its graph, however it was created: row offsets, neighbour table (and the reverse index when
// with_rev), the segment and hub tables of `plan` (with the fragment tables of the hub rows when hub_frags), the label and
// clamp vectors, zeroed partials (allocated by the caller), the dc 1 constant and the dc 2 source rows. e->N / E2 / Q / dc /
// stream are set. The uploads are complete on return.
int setup_graph_tables(sbmbp_engine *e, const segment_plan_t &plan, const uint64_t *row_ptr, const uint32_t *nbr, const uint32_t *rev,
                       bool with_rev, bool hub_frags) {
    std::vector<uint32_t> rp32(size_t(e->N) + 1);
    for (size_t i = 0; i <= e->N; ++i) rp32[i] = uint32_t(row_ptr[i]);
    e->h_row_ptr = rp32;
    e->n_blk = uint32_t(plan.blk_row.size() - 1);
    e->n_hub = uint32_t(plan.hub_row.size());
    CHK(dev_upload(e, e->d_row_ptr, rp32));
    CHK(dev_upload(e, e->d_nbr, nbr, e->E2));
    if (with_rev) CHK(dev_upload(e, e->d_rev, rev, e->E2));
    if (!e->E2) {  // the sweeps' branch-free loads read nbr[0] / rev[0] even when there are no edges
        HIPCHK(hipMemsetAsync(e->d_nbr, 0, 4, e->stream));
        if (with_rev) HIPCHK(hipMemsetAsync(e->d_rev, 0, 4, e->stream));
    }
    CHK(dev_upload(e, e->d_blk_row, plan.blk_row));
    CHK(dev_upload(e, e->d_blk_e0, plan.blk_e0));
    CHK(dev_upload(e, e->d_hub_row, plan.hub_row));
    CHK(dev_upload(e, e->d_hub_blk, plan.hub_blk));
    if (e->n_hub && hub_frags) CHK(setup_hub_frags(e, plan.hub_row, rp32));
    CHK(dev_alloc(e, e->d_true, e->N));
    CHK(dev_alloc(e, e->d_clamp, e->N));
    HIPCHK(hipMemsetAsync(e->d_true, 0, size_t(e->N) * 4, e->stream));
    HIPCHK(hipMemsetAsync(e->d_clamp, 0xff, size_t(e->N) * 4, e->stream));
    HIPCHK(hipMemsetAsync(e->d_partials, 0, e->d_partials.capacity() * 8, e->stream));
    if (e->dc == 1) {  // sum over the directed edges of these rows of log(d_i d_l) = 2 sum_i d_i log d_i (constant of f_site / f_edge)
        double s = 0.0;
        for (uint32_t i = 0; i < e->N; ++i) { const double d = double(rp32[i + 1] - rp32[i]); if (d > 0) s += 2.0 * d * std::log(d); }
        e->sum_log_didl = s;
    }
    if (e->dc == 2) {
        CHK(dev_alloc(e, e->d_src, e->E2));
        hipLaunchKernelGGL(k_fill_src, dim3((e->N + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->N, e->d_src);
    }
    HIPCHK(hipStreamSynchronize(e->stream));  // rp32 is a local
    return SBMBP_OK;
}

// marginal-gather update of hub rows [h0, h0 + nh): two launches over their fragments
int launch_hub_psi(sbmbp_engine *e, hipStream_t st, uint32_t h0, uint32_t nh, double *Mio, const double *psi_old, double *psi_new,
                   const int32_t *clamp, const shard_io &io, const double *Mcmp, int first) {
    if (!nh) return SBMBP_OK;
    const uint32_t f0 = e->h_hub_frag0[h0], nf = e->h_hub_frag0[h0 + nh] - f0;
    const hub_frags hf{e->d_frag_hub, e->d_hub_frag0, e->d_hub_b, e->d_hub_pA, e->d_hub_pE};
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_hub_frag_product<QQ>), dim3(nf), dim3(BLOCK), 0, st, e->d_row_ptr, e->d_nbr, Mio, psi_old,
                                        e->d_hub_row, e->d_hub_blk, hf, f0, e->d_P, e->d_partials, clamp, io, first));
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_hub_frag_cavity<QQ>), dim3(nf), dim3(BLOCK), 0, st, e->d_row_ptr, Mio, psi_old, psi_new,
                                        e->d_hub_row, e->d_hub_blk, hf, f0, e->d_P, int(e->dc), e->d_partials, clamp, io, Mcmp));
    return SBMBP_OK;
}

// message-gather update of all hub rows: the same two launches over their fragments, incoming messages gathered through rev.
// P, partials and prior are the engine's own, or those of one replica of a batch (batch_launch_sweep)
int launch_hub_msg(sbmbp_engine *e, hipStream_t st, const double *Mold, double *Mnew, const double *psi_old, double *psi_new,
                   const int32_t *clamp, double damp, dev_params *P, double *partials, const double *prior) {
    if (!e->n_hub) return SBMBP_OK;
    const uint32_t nf = e->n_frag;
    const hub_frags hf{e->d_frag_hub, e->d_hub_frag0, e->d_hub_b, e->d_hub_pA, e->d_hub_pE};
    DISPATCH_QB(e->Q, e->dc == 2, hipLaunchKernelGGL((k_hub_frag_product_msg<QQ, BB>), dim3(nf), dim3(BLOCK), 0, st, e->d_row_ptr, e->d_rev, e->d_nbr,
                                                     e->d_deg, Mold, e->d_hub_row, e->d_hub_blk, hf, 0u, P, partials, clamp));
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_hub_frag_cavity_msg<QQ>), dim3(nf), dim3(BLOCK), 0, st, e->d_row_ptr, Mold, Mnew, psi_old, psi_new,
                                        e->d_hub_row, e->d_hub_blk, hf, 0u, P, int(e->dc != 0), damp,
                                        partials, clamp, prior));
    return SBMBP_OK;
}

// h from the current psi (init_h, bp.cpp:320-332); mode 1 = converge start, 2 = exact refresh
// wide path: fold of [rows][Q + 1] records (long tables to <= FOLD_BLOCKS rows first) + k_wfinalize
int launch_wfinalize(sbmbp_engine *e, uint32_t rows, int mode) {
    const double *part = fold_stage(e, &rows, int(e->Q), 1, e->Q + 1);
    hipLaunchKernelGGL(k_wfinalize, dim3(1), dim3(BLOCK), 0, e->stream, part, rows, mode, e->d_P, e->d_Pw, int(e->Q), e->d_hist, e->hist_cap);
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

int launch_field(sbmbp_engine *e, int mode) {
    const uint32_t rows_per_blk = 4096;
    const uint32_t nb = std::max<uint32_t>(1, (e->N + rows_per_blk - 1) / rows_per_blk);
    CHK(ensure_partials(e, size_t(nb) * (e->Q + 1)));
    if (e->wide) {
        hipLaunchKernelGGL(k_wpsi_sum, dim3(nb), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->d_psi[e->pcur], e->N, rows_per_blk, int(e->Q),
                           int(e->dc != 0), e->d_partials);
        return launch_wfinalize(e, nb, mode);
    }
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_psi_sum<QQ>), dim3(nb), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->d_psi[e->pcur],
                                        e->N, rows_per_blk, int(e->dc != 0), e->d_partials));
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_finalize<QQ>), dim3(1), dim3(BLOCK), 0, e->stream, e->d_partials, nb, mode, e->d_P,
                                        (double *)nullptr, 0u, 0));
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

// One synchronous sweep, sweep number `j` of the current run_sweeps call (buffers alternate per
// sweep). psi_form: reconstruct incoming messages from the neighbours' marginals (k_sweep_psi)
// instead of gathering them from the message array (k_sweep).
int launch_sweep(sbmbp_engine *e, uint32_t j, double damp, bool psi_form, bool first_from_psi = false) {
    const sweep_bufs s = bufs_of_sweep(e, j);
    hipEvent_t stop;
    if (e->wide) {  // Q > 16: one kernel for rows of any degree, then the fold and K2 for a run-time Q
        CHK(timing_begin(e, e->stream, true, &stop));
        DISPATCH_QT(e->Q, hipLaunchKernelGGL((k_wsweep<QT>), dim3(e->n_blk), dim3(WTPB), 0, e->stream, e->d_row_ptr, e->d_rev, s.Mold, s.Mnew, s.psi_old,
                                             s.psi_new, s.clamp, e->d_blk_row, e->d_blk_e0, e->d_P, e->d_Pw, int(e->Q), int(e->dc), damp, e->d_partials));
        CHK(timing_end(stop, e->stream));
        return launch_wfinalize(e, e->n_blk, 0);
    }
    // Hub rows first, in fragments, on the sweep's own stream (disjoint rows and edges from the frame kernel's; they are
    // throughput-bound like it: beside it on a second stream they gained nothing, C4 0.545 vs 0.533 ms per sweep; round 3
    // let the fragment PRODUCTS ride at the head of the frame launch instead of a launch of their own, and the frame kernel
    // grew by exactly the product kernel's 0.037 ms: the fragments cost what their edges cost wherever they run).
    if (e->n_hub) {
        if (psi_form) CHK(launch_hub_psi(e, e->stream, 0, e->n_hub, s.Mnew, s.psi_old, s.psi_new, s.clamp, shard_io{}, s.Mold, int(first_from_psi)));
        else CHK(launch_hub_msg(e, e->stream, s.Mold, s.Mnew, s.psi_old, s.psi_new, s.clamp, damp, e->d_P, e->d_partials, e->d_prior));
    }
    CHK(timing_begin(e, e->stream, true, &stop));  // around the frame kernel only
    if (psi_form) {
        DISPATCH_QB(e->Q, s.clamp != nullptr,
                    hipLaunchKernelGGL((k_sweep_psi<QQ, BB, false>), dim3(xcd_grid(e->n_blk)), dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr, e->d_nbr,
                                       s.Mnew, s.psi_old, s.psi_new, e->d_blk_row, e->d_blk_e0, e->d_P, int(e->dc), e->d_partials, s.clamp, shard_io{}, e->n_blk,
                                       SBMBP_XCD_REMAP, s.Mold, int(first_from_psi)));
    } else if (e->d_prior != nullptr) {  // a per-vertex prior is set: the prior twin of k_sweep
        DISPATCH_QB(e->Q, e->dc == 2,
                    hipLaunchKernelGGL((k_sweep_prior<QQ, BB>), dim3(e->n_blk), dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr, e->d_rev, e->d_nbr,
                                       e->d_deg, s.Mold, s.Mnew, s.psi_old, s.psi_new, s.clamp, e->d_blk_row, e->d_blk_e0, e->d_P, int(e->dc != 0), damp,
                                       e->d_partials, e->d_prior));
    } else {
        DISPATCH_QB(e->Q, e->dc == 2,
                    hipLaunchKernelGGL((k_sweep<QQ, BB>), dim3(e->n_blk), dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr, e->d_rev, e->d_nbr, e->d_deg,
                                       s.Mold, s.Mnew, s.psi_old, s.psi_new, s.clamp, e->d_blk_row, e->d_blk_e0, e->d_P, int(e->dc != 0), damp, e->d_partials));
    }
    CHK(timing_end(stop, e->stream));
    // fold of the segment records + K2 in one launch (k_fold_finalize): <= FOLD_BLOCKS workgroups of >= 2048 records each
    if (!e->d_fold_counters) {
        CHK(dev_alloc(e, e->d_fold_counters, 1));
        HIPCHK(hipMemsetAsync(e->d_fold_counters, 0, 4, e->stream));
    }
    const uint32_t rows = e->n_blk;
    // (one workgroup for C2's 5860 records instead of three and their ticket: 0.070 -> 0.071 ms per step, not better)
    const uint32_t nb = std::min<uint32_t>(FOLD_BLOCKS, std::max<uint32_t>(1, (rows + 2047) / 2048));
    const uint32_t chunk = (rows + nb - 1) / nb;
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_fold_finalize<QQ>), dim3(nb), dim3(BLOCK), 0, e->stream, e->d_partials, rows, chunk, e->d_P, e->d_hist,
                                        e->hist_cap, int(!psi_form), e->d_stage, e->d_fold_counters));
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

int collect_timing(sbmbp_engine *e) {
    size_t pieces = 0;
    for (size_t i = 0; i + 1 < e->ev_used; i += 2) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e->ev[i], e->ev[i + 1]));
        e->sweep_ms += double(ms);
        ++pieces;
    }
    // a chunked shard sweep is timed per chunk; the chunks of one sweep together process the shard's edges once
    const size_t per_sweep = e->sharded ? std::max<size_t>(1, e->chunk_blk.size() - 1) : 1;
    e->sweep_launches += pieces / per_sweep;
    e->ev_used = 0;
    return SBMBP_OK;
}

int read_conv_state(sbmbp_engine *e, conv_state *cs) {
    HIPCHK(hipMemcpyAsync(cs, reinterpret_cast<const char *>(e->d_P.get()) + offsetof(dev_params, maxdiff), sizeof(conv_state),
                          hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SBMBP_OK;
}

// the convergence state without blocking the host: record copies it into page-locked slot 0/1 behind the work queued so
// far, wait blocks until that point of the stream and returns it
int record_conv_state(sbmbp_engine *e, int slot) {
    if (!e->h_cs) {
        CHK(e->h_cs.alloc(2));
        for (auto &ev : e->ev_cs) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    HIPCHK(hipMemcpyAsync(e->h_cs + slot, reinterpret_cast<const char *>(e->d_P.get()) + offsetof(dev_params, maxdiff),
                          sizeof(conv_state), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipEventRecord(e->ev_cs[slot], e->stream));
    return SBMBP_OK;
}
// the host's answer to a pause (adaptive relaxation asked for damping in the middle of a marginal-gather run): the queued
// sweeps behind it were skipped; the run goes on in the message-gather form
int resume_run(sbmbp_engine *e) {
    hipLaunchKernelGGL(k_resume, dim3(1), dim3(64), 0, e->stream, e->d_P);
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}
int wait_conv_state(sbmbp_engine *e, int slot, conv_state *cs) {
    HIPCHK(hipEventSynchronize(e->ev_cs[slot]));
    *cs = e->h_cs[slot];
    return SBMBP_OK;
}

// exact criterion of the reference's converge(): max |m^{t+1} - m^t| over the two message buffers
int message_diff(sbmbp_engine *e, double *out) {
    const uint64_t n = e->E2;  // message records
    if (n == 0) { *out = 0.0; return SBMBP_OK; }
    const uint32_t nb = uint32_t(std::min<uint64_t>(2048, (n + BLOCK - 1) / BLOCK));
    CHK(ensure_partials(e, size_t(nb) * 2));
    if (e->wide) hipLaunchKernelGGL(k_wmsg_diff, dim3(nb), dim3(BLOCK), 0, e->stream, e->d_M[0], e->d_M[1], n * e->Q, e->d_partials);
    else
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_msg_diff<QQ>), dim3(nb), dim3(BLOCK), 0, e->stream, e->d_M[0], e->d_M[1], n, e->d_partials));
    hipLaunchKernelGGL(k_fold_stage, dim3(1), dim3(BLOCK), 0, e->stream, e->d_partials, nb, nb, 1, 1, 2u, e->d_stage);
    HIPCHK(hipGetLastError());
    double r[2];
    HIPCHK(hipMemcpyAsync(r, e->d_stage, 16, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    *out = r[1];
    return SBMBP_OK;
}

bool psi_form_allowed(const sbmbp_engine *e, double damping) {
    // (under a per-vertex prior the marginal-gather form would still be exact - psi_l carries the prior - but its kernels do not
    // take one: DESIGN.md section 9)
    return !e->wide && e->gather_mode == 0 && damping == 1.0 && (!e->has_clamp || e->clamp_onehot) && e->dc != 2 && e->w_positive && e->E2 > 0 &&
           e->d_prior == nullptr;
}

void free_coloured(sbmbp_engine *e) {
    e->cs = sbmbp_engine::coloured_tables();
    e->cs_seg0.clear(); e->cs_hub0.clear(); e->cs_frag0.clear();
    e->cs_colours = e->cs_steps = e->cs_max_rec = 0;
}

// Device tables of the coloured order from the step of every vertex (host_graph.cpp coloured_plan): the tables are
// coloured_step_tables' (host_graph.cpp), with fragments of BLOCK edges as setup_hub_frags cuts them.
int build_coloured(sbmbp_engine *e, const std::vector<uint32_t> &step, uint32_t n_colours, uint32_t n_steps) {
    free_coloured(e);
    coloured_tables_t t;
    coloured_step_tables(e->h_row_ptr.data(), e->N, step.data(), n_steps, uint32_t(frame_cap(e->Q)), uint32_t(frame_rcap(e->Q)), uint32_t(BLOCK), t);
    if (t.frag_hub.size() != e->n_frag) { set_error("coloured order: fragment tables disagree"); return SBMBP_ERR_STATE; }
    CHK(dev_upload(e, e->cs.rows, t.rows));
    CHK(dev_upload(e, e->cs.loff, t.loff));
    CHK(dev_upload(e, e->cs.seg_row0, t.seg_row0));
    CHK(dev_upload(e, e->cs.hub_row, t.hub_row));
    CHK(dev_upload(e, e->cs.hub_rec, t.hub_rec));
    CHK(dev_upload(e, e->cs.frag_hub, t.frag_hub));
    CHK(dev_upload(e, e->cs.hub_frag0, t.hub_frag0));
    HIPCHK(hipStreamSynchronize(e->stream));  // the tables are locals
    e->cs_colours = n_colours;
    e->cs_steps = n_steps;
    e->cs_seg0.swap(t.seg0); e->cs_hub0.swap(t.hub0); e->cs_frag0.swap(t.frag0);
    e->cs_max_rec = t.max_rec;
    return SBMBP_OK;
}

// One sweep of the coloured order: per step the hub launches (if the step has hubs), k_sweep_step over the step's segments
// and k_step_finalize, all in place on the current message buffer and marginal table.
int launch_coloured_sweep(sbmbp_engine *e, double damp) {
    double *M = e->d_M[e->cur], *psi = e->d_psi[e->pcur];
    const int32_t *clamp = e->has_clamp ? e->d_clamp.get() : nullptr;
    hipEvent_t stop;  // one pair per sweep: the step kernels AND their finalize launches (a sweep is nothing but their sequence)
    CHK(timing_begin(e, e->stream, true, &stop));
    const hub_frags hf{e->cs.frag_hub, e->cs.hub_frag0, e->d_hub_b, e->d_hub_pA, e->d_hub_pE};
    for (uint32_t s = 0; s < e->cs_steps; ++s) {
        const uint32_t seg0 = e->cs_seg0[s], nseg = e->cs_seg0[s + 1] - seg0, nh = e->cs_hub0[s + 1] - e->cs_hub0[s];
        if (nh) {
            const uint32_t f0 = e->cs_frag0[s], nf = e->cs_frag0[s + 1] - f0;
            DISPATCH_QB(e->Q, e->dc == 2, hipLaunchKernelGGL((k_hub_frag_product_msg<QQ, BB>), dim3(nf), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->d_rev,
                                                             e->d_nbr, e->d_deg, M, e->cs.hub_row, e->cs.hub_rec, hf, f0, e->d_P, e->d_partials, clamp));
            DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_hub_step_cavity<QQ>), dim3(nf), dim3(BLOCK), 0, e->stream, e->d_row_ptr, M, psi, e->cs.hub_row,
                                                e->cs.hub_rec, hf, f0, e->d_P, int(e->dc != 0), damp, e->d_partials, clamp));
        }
        if (nseg)
            DISPATCH_QB(e->Q, e->dc == 2, hipLaunchKernelGGL((k_sweep_step<QQ, BB>), dim3(nseg), dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr, e->d_rev,
                                                             e->d_nbr, e->d_deg, M, psi, clamp, e->cs.rows, e->cs.loff, e->cs.seg_row0, seg0, e->d_P,
                                                             int(e->dc != 0), damp, e->d_partials));
        DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_step_finalize<QQ>), dim3(1), dim3(BLOCK), 0, e->stream, e->d_partials, nseg + nh, int(s + 1 == e->cs_steps),
                                            e->d_P, e->d_hist, e->hist_cap));
    }
    CHK(timing_end(stop, e->stream));
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

// run_sweeps in the coloured order: the field sums are recomputed from the marginals at the start of every call (inside a
// call they move by differences, step by step), the decision stays on the device (stop flag, queued no-op launches) and the
// host reads the convergence state once per batch of check_every sweeps, one batch queued ahead.
int run_sweeps_coloured(sbmbp_engine *e, double crit, uint32_t max_sweeps, double damping, int *niter, double *last) {
    if (!e->have_params || !e->have_state) { set_error("set_params and init_messages/set_state must precede converge"); return SBMBP_ERR_STATE; }
    CHK(upload_params(e, crit, false));
    CHK(launch_field(e, 1));
    CHK(ensure_partials(e, size_t(std::max<uint32_t>(std::max(e->n_blk, e->cs_max_rec), 1)) * (e->Q + 1)));
    conv_state cs{0.0, -1, 0, 0, 0, 0, 0, 1, 0, 0, -1};
    const uint32_t batch_max = std::max<uint32_t>(1, e->check_every);
    uint32_t done = 0;
    auto queue_batch = [&](int slot) -> int {
        const uint32_t batch = std::min(batch_max, max_sweeps - done);
        for (uint32_t b = 0; b < batch; ++b) CHK(launch_coloured_sweep(e, damping));
        done += batch;
        return record_conv_state(e, slot);
    };
    auto wait_batch = [&](int slot, bool *stopped) -> int {
        CHK(wait_conv_state(e, slot, &cs));
        *stopped = cs.stop != 0;
        return SBMBP_OK;
    };
    if (max_sweeps > 0) CHK(queue_ahead(max_sweeps, done, queue_batch, wait_batch));
    else HIPCHK(hipStreamSynchronize(e->stream));
    if (e->timing) CHK(collect_timing(e));
    const uint32_t executed = uint32_t(cs.sweep_idx);
    e->sweeps += executed;
    if (executed > 0) {
        e->fz.valid = false;
        // the marginal table is no longer the product the marginal-gather form assumes: the next synchronous sweep or
        // reduction takes the message-gather kernels, as after sbmbp_set_state
        e->psi_consistent = false;
        e->init_from_psi = false;
    }
    e->field_fresh = true;  // (of the current marginals: recomputed at the start, moved with every step since)
    e->cs_last = true;
    e->ar_fl = 0;
    e->ar_gl = -1;
    if (niter) *niter = cs.conv_iter;
    if (last) *last = cs.maxdiff;
    return SBMBP_OK;
}

// run sweeps until convergence (crit >= 0) or exactly max_sweeps (crit < 0: never converges). The whole decision runs on
// the device (k_finalize: 2-step hints arm the exact criterion, the exact criterion sets the stop flag; kernels.h
// dev_params), so the host only reads the convergence state once per batch.
int run_sweeps(sbmbp_engine *e, double crit, uint32_t max_sweeps, double damping, int *niter, double *last) {
    if (e->sweep_order == 1) return run_sweeps_coloured(e, crit, max_sweeps, damping, niter, last);
    if (!e->have_params || !e->have_state) { set_error("set_params and init_messages/set_state must precede converge"); return SBMBP_ERR_STATE; }
    e->cs_last = false;
    const bool psi_ok = psi_form_allowed(e, damping);
    CHK(ensure_partials(e, size_t(std::max<uint32_t>(e->n_blk, 1)) * (e->Q + 1)));
    CHK(upload_params(e, crit, psi_ok));
    CHK(launch_field(e, 1));
    conv_state cs{0.0, -1, 0, 0, 0, 0, 0, 1, 0, 0, -1};
    // the first sweep after a state or parameter change gathers the messages themselves (explicit form), unless the
    // state is the device initialisation "message = sender's marginal", which the marginal-gather form starts from
    const bool first_from_psi = psi_ok && e->init_from_psi;
    const bool first_explicit = !e->psi_consistent && !first_from_psi;
    batch_planner plan(std::max<uint32_t>(1, e->check_every), crit);
    uint32_t psi_count = 0;
    // (adaptive relaxation can ask for damping in the middle of a run: converge_run queues the rest in the message-gather form)
    auto queue_batch = [&](int slot, uint32_t first, uint32_t n, bool form_psi) -> int {
        for (uint32_t j = first; j < first + n; ++j) {
            const bool pf = form_psi && !(j == 0 && first_explicit);
            CHK(launch_sweep(e, j, damping, pf, pf && j == 0 && first_from_psi));
        }
        return record_conv_state(e, slot);
    };
    auto wait_batch = [&](int slot, conv_state *st) { return wait_conv_state(e, slot, st); };
    CHK(converge_run(max_sweeps, plan, psi_ok, first_explicit, queue_batch, wait_batch, [&]() { return resume_run(e); }, &cs, &psi_count));
    if (e->timing) CHK(collect_timing(e));
    const uint32_t executed = uint32_t(cs.sweep_idx);
    e->cur = (e->cur + int(executed)) & 1;
    e->pcur = (e->pcur + int(executed)) & 1;
    double exact = cs.maxdiff;
    // the last executed sweep reported a 2-step hint: measure the reference's 1-step difference when the caller wants it
    if (executed > 0 && last != nullptr && !cs.last_exact) CHK(message_diff(e, &exact));
    e->sweeps += executed;
    e->psi_sweeps += psi_count;
    if (executed > 0) e->fz.valid = false;
    const bool relaxed = cs.ar_fl > 0 || cs.ar_gl >= 0;
    const double damp_eff = damping * ar_gen_damp(cs.ar_gl);
    if (executed > 0) {
        e->psi_consistent = (damp_eff == 1.0 && (!e->has_clamp || e->clamp_onehot) && e->w_positive);
        e->init_from_psi = false;
    }
    e->field_fresh = (e->field_mix >= 1.0) && !relaxed && executed > 0;
    e->ar_fl = cs.ar_fl;
    e->ar_gl = cs.ar_gl;
    if (niter) *niter = cs.conv_iter;
    if (last) *last = exact;
    return SBMBP_OK;
}

// fold [rows][stride] partials into d_small[0..cols) and copy to host
int fold_to_host(sbmbp_engine *e, uint32_t rows, uint32_t cols, uint32_t stride, double *out) {
    CHK(ensure_small(e, cols));
    const double *part = fold_stage(e, &rows, int(cols), 0, stride);
    hipLaunchKernelGGL(k_fold_rows_sum, dim3(1), dim3(BLOCK), 0, e->stream, part, rows, cols, stride, e->d_small);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, e->d_small, size_t(cols) * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SBMBP_OK;
}

// same fold, result left in device memory (no host sync): shard steps hand it to a collective
int fold_to_device(sbmbp_engine *e, uint32_t rows, uint32_t cols, uint32_t stride, double *d_out) {
    const double *part = fold_stage(e, &rows, int(cols), 0, stride);
    hipLaunchKernelGGL(k_fold_rows_sum, dim3(1), dim3(BLOCK), 0, e->stream, part, rows, cols, stride, d_out);
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

// [rows][cols] partials (stride = cols) -> d_out[cols]: row-parallel two-stage fold for narrow matrices,
// column-parallel serial fold for wide ones (moment tensors)
int fold_matrix_to_device(sbmbp_engine *e, uint32_t rows, uint32_t cols, double *d_out) {
    if (cols <= FOLD_STRIDE_MAX) return fold_to_device(e, rows, cols, cols, d_out);
    hipLaunchKernelGGL(k_fold_columns, dim3((cols + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, e->stream, e->d_partials, rows, cols, d_out);
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

int refresh_field(sbmbp_engine *e) {
    if (!e->have_params || !e->have_state) { set_error("engine has no parameters or no state"); return SBMBP_ERR_STATE; }
    CHK(launch_field(e, 2));
    e->field_fresh = true;
    return SBMBP_OK;
}

// the three Q x Q matrices of the non-edge term (host_reduce.h nonedge_mats, over the vertices of the whole graph) in d_mats
// (a shard allocates it on first use)
int upload_nonedge_mats(sbmbp_engine *e, std::vector<double> &mats, double *wmax_out) {
    mats.assign(3 * e->Q * e->Q, 0.0);
    nonedge_mats(e->Q, e->Nglob, e->cab.data(), e->beta, mats.data(), wmax_out);
    if (!e->d_mats) CHK(dev_alloc(e, e->d_mats, mats.size()));
    HIPCHK(hipMemcpyAsync(e->d_mats, mats.data(), mats.size() * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SBMBP_OK;
}
inline bool nonedge_exact(const sbmbp_engine *e) { return nonedge_is_exact(e->nonedge_mode, e->N); }

// copy of n folded doubles to the host; returns when they have arrived
int read_doubles(sbmbp_engine *e, const double *d_src, size_t n, double *out) {
    HIPCHK(hipMemcpyAsync(out, d_src, n * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SBMBP_OK;
}

// moment tensors of orders 1 .. K of this engine's rows (T = series_len(Q, K) doubles), folded into d_out
int moments_to_device(sbmbp_engine *e, int K, uint32_t T, double *d_out) {
    const uint32_t rows_per_blk = 512;  // one thread per output entry loops over staged rows: keep chunks small, workgroups many
    const uint32_t nb = std::max<uint32_t>(1, (e->N + rows_per_blk - 1) / rows_per_blk);
    CHK(ensure_partials(e, size_t(nb) * T));
    hipLaunchKernelGGL(k_moments, dim3(nb), dim3(BLOCK), 0, e->stream, e->d_psi[e->pcur], e->N, int(e->Q), K, rows_per_blk, int(T), e->d_partials);
    HIPCHK(hipGetLastError());
    return fold_matrix_to_device(e, nb, T, d_out);
}

// adjacent pairs of the non-edge term over this engine's rows, folded into d_out[0 .. NE_NP): in the form of the exact loop
// (P = d_mats + Q Q) or of the series (w = d_mats)
int adjacent_pairs_to_device(sbmbp_engine *e, bool exact, bool want_entropy, double *d_out) {
    const uint32_t Q = e->Q;
    const double invN = 1.0 / double(e->Nglob);
    const double *d_cab = e->d_mats + 2 * Q * Q;
    CHK(ensure_partials(e, size_t(std::max<uint32_t>(e->n_blk, 1)) * (NE_NP + 1)));
    if (exact) {
        DISPATCH_Q(Q, hipLaunchKernelGGL((k_nonedge_exact_adj<QQ>), dim3(e->n_blk), dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr,
                                         e->d_nbr, e->d_psi[e->pcur], e->d_mats + Q * Q, d_cab, e->d_blk_row, invN, int(want_entropy),
                                         e->d_partials));
    } else {
        DISPATCH_Q(Q, hipLaunchKernelGGL((k_nonedge_adj<QQ>), dim3(e->n_blk), dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr,
                                         e->d_nbr, e->d_psi[e->pcur], e->d_mats, d_cab, e->d_blk_row, invN, int(want_entropy), e->d_partials));
    }
    HIPCHK(hipGetLastError());
    return fold_to_device(e, e->n_blk, NE_NP, NE_NP + 1, d_out);
}

// May the reductions take the fused pass on the marginal-gather reconstruction (k_fe_psi)? It needs exactly what the
// marginal-gather SWEEP needs, and psi must be the marginals of the message pair in d_M: the state a converge call leaves.
bool fused_ok(const sbmbp_engine *e) {
    return e->fused_reductions && !e->sharded && e->psi_consistent && psi_form_allowed(e, 1.0);
}

inline bool use_fz(const sbmbp_engine *e) { return e->wide || fused_ok(e); }  // (the wide path has no other reduction kernels)

// ONE pass: site / edge terms of free energy (and entropy), adjacent pairs of the non-edge term (dc 0), EM numerators.
// Results stay in e->fz until the state changes.
int fused_pass(sbmbp_engine *e, bool want_entropy, bool want_em) {
    const uint32_t Q = e->Q;
    want_em = want_em && Q <= 8;  // Q (Q+1) / 2 accumulators per lane: above Q = 8 the EM numerators keep their own kernel
    if (e->fz.valid && (e->fz.entropy || !want_entropy) && (e->fz.em || !want_em)) return SBMBP_OK;
    if (!e->field_fresh) { CHK(launch_field(e, 2)); e->field_fresh = true; }  // the site terms read h of the current marginals
    int adj_mode = 0;
    const double *d_w = nullptr;
    if (e->dc == 0) {
        std::vector<double> mats;
        CHK(upload_nonedge_mats(e, mats, nullptr));
        adj_mode = nonedge_exact(e) ? 2 : 1;
        d_w = adj_mode == 2 ? e->d_mats + Q * Q : e->d_mats;
    }
    if (e->wide) {  // Q > 16: k_wreduce (message-gather, matrix cores), hub rows included
        CHK(ensure_partials(e, size_t(std::max<uint32_t>(e->n_blk, 1)) * (WR_NP + 1)));
        CHK(ensure_small(e, WR_NP));
        DISPATCH_QTB(Q, want_entropy, hipLaunchKernelGGL((k_wreduce<QT, BB>), dim3(e->n_blk), dim3(WTPB), 0, e->stream, e->d_row_ptr, e->d_rev, e->d_nbr,
                                                         e->d_M[e->cur], e->d_psi[e->pcur], e->d_blk_row, e->d_blk_e0, e->d_P, e->d_Pw, int(Q), int(e->dc),
                                                         adj_mode, d_w, e->d_partials));
        HIPCHK(hipGetLastError());
        double o6[WR_NP];
        CHK(fold_to_host(e, e->n_blk, WR_NP, WR_NP + 1, o6));
        for (int x = 0; x < 4; ++x) e->fz.se[x] = o6[x];
        e->fz.adj[0] = o6[FE_NP];
        e->fz.adj[1] = o6[FE_NP + 1];
        e->fz.tri.clear();
        e->fz.valid = true;
        e->fz.entropy = want_entropy;
        e->fz.em = false;
        return SBMBP_OK;
    }
    const uint32_t T = want_em ? Q * (Q + 1) / 2 : 0, NP = FE_NP + NE_NP + T, rows = e->n_blk + e->n_hub;
    CHK(ensure_partials(e, size_t(std::max<uint32_t>(rows, 1)) * (NP + 1)));
    CHK(ensure_small(e, NP));
    const double *Mcur = e->d_M[e->cur], *Mprev = e->d_M[e->cur ^ 1], *psi = e->d_psi[e->pcur];
    // (want_em holds up to Q = 8 only, see above)
    DISPATCH_QB(Q, want_em, constexpr int QF = BB ? q_clamp(QQ, 2, 8) : QQ;
                hipLaunchKernelGGL((k_fe_psi<QF, BB>), dim3(xcd_grid(e->n_blk)), dim3(frame_cfg<QF>::TPB), 0, e->stream, e->d_row_ptr, e->d_nbr, Mcur, Mprev,
                                   psi, e->d_blk_row, e->d_blk_e0, e->d_P, int(e->dc), int(want_entropy), adj_mode, d_w, e->n_blk, e->d_partials));
    if (e->n_hub)  // site and edge terms of the hub rows, in records of their own behind the segments'
        DISPATCH_Q(Q, hipLaunchKernelGGL((k_fe_hub<QQ, false>), dim3(e->n_hub), dim3(BLOCK), 0, e->stream, e->d_row_ptr,
                                         e->d_rev, e->d_nbr, e->d_deg, Mcur, (const double *)nullptr, e->d_hub_row, e->d_hub_blk, e->d_P,
                                         int(e->dc), int(want_entropy), e->d_partials, NP + 1, e->n_blk));
    HIPCHK(hipGetLastError());
    std::vector<double> out(NP);
    CHK(fold_to_host(e, rows, NP, NP + 1, out.data()));
    for (int x = 0; x < 4; ++x) e->fz.se[x] = out[x];
    e->fz.adj[0] = out[FE_NP];
    e->fz.adj[1] = out[FE_NP + 1];
    e->fz.tri.assign(out.begin() + FE_NP + NE_NP, out.end());
    e->fz.valid = true;
    e->fz.entropy = want_entropy;
    e->fz.em = want_em;
    return SBMBP_OK;
}

int site_edge_terms(sbmbp_engine *e, bool want_entropy, double out[4], double *d_out = nullptr) {
    if (d_out == nullptr && use_fz(e)) {
        CHK(fused_pass(e, want_entropy, false));
        for (int x = 0; x < 4; ++x) out[x] = e->fz.se[x];
        return SBMBP_OK;
    }
    CHK(ensure_partials(e, size_t(std::max<uint32_t>(e->n_blk, 1)) * (FE_NP + 1)));
    const double *M = e->d_M[e->cur];
    const double *Min = (e->sharded && e->incoming_src == 0) ? e->d_Min.get() : nullptr;
    const bool dc2 = e->dc == 2;
    const int dcf = int(e->dc != 0);  // (the DC2 variants take 1, the others dc, which is 0 or 1 there)
    if (e->d_prior != nullptr) {  // a per-vertex prior is set: the prior twins, whose site products take the row's prior line
        DISPATCH_QB(e->Q, dc2, hipLaunchKernelGGL((k_fe_frame_prior<QQ, BB>), dim3(e->n_blk), dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr, e->d_rev,
                                                  e->d_nbr, e->d_deg, M, Min, e->d_blk_row, e->d_blk_e0, e->d_P, dcf, int(want_entropy), e->d_partials, e->d_prior));
        if (e->n_hub)
            DISPATCH_QB(e->Q, dc2, hipLaunchKernelGGL((k_fe_hub_prior<QQ, BB>), dim3(e->n_hub), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->d_rev, e->d_nbr,
                                                      e->d_deg, M, Min, e->d_hub_row, e->d_hub_blk, e->d_P, dcf, int(want_entropy), e->d_partials,
                                                      uint32_t(FE_NP + 1), 0xffffffffu, e->d_prior));
    } else {
        DISPATCH_QB(e->Q, dc2, hipLaunchKernelGGL((k_fe_frame<QQ, BB>), dim3(e->n_blk), dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr, e->d_rev, e->d_nbr,
                                                  e->d_deg, M, Min, e->d_blk_row, e->d_blk_e0, e->d_P, dcf, int(want_entropy), e->d_partials));
        if (e->n_hub)
            DISPATCH_QB(e->Q, dc2, hipLaunchKernelGGL((k_fe_hub<QQ, BB>), dim3(e->n_hub), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->d_rev, e->d_nbr,
                                                      e->d_deg, M, Min, e->d_hub_row, e->d_hub_blk, e->d_P, dcf, int(want_entropy), e->d_partials,
                                                      uint32_t(FE_NP + 1), 0xffffffffu));
    }
    HIPCHK(hipGetLastError());
    if (d_out) return fold_to_device(e, e->n_blk, FE_NP, FE_NP + 1, d_out);
    return fold_to_host(e, e->n_blk, FE_NP, FE_NP + 1, out);
}

// non-edge terms: out[0] = f_nonedge, out[1] = e_nonedge (if want_entropy)   (bp.cpp:675-741)
int nonedge_terms(sbmbp_engine *e, bool want_entropy, double out[2]) {
    out[0] = out[1] = 0.0;
    if (e->dc != 0) return SBMBP_OK;  // exactly 0 in the reference (:687-700, :721-727)
    const uint32_t Q = e->Q, N = e->N;
    const double invN = 1.0 / double(N);
    std::vector<double> mats;
    double wmax = 0.0;
    CHK(upload_nonedge_mats(e, mats, &wmax));
    const double *d_Pm = e->d_mats + Q * Q, *d_cab = e->d_mats + 2 * Q * Q;
    const bool exact = nonedge_exact(e);
    double adj[2] = {0.0, 0.0}, all[2] = {0.0, 0.0};
    const bool adj_known = use_fz(e) && e->fz.valid && (e->fz.entropy || !want_entropy);  // the fused pass has the adjacent pairs already
    if (e->wide && !adj_known) { set_error("internal: the wide reductions run site_edge_terms first"); return SBMBP_ERR_STATE; }
    if (adj_known) { adj[0] = e->fz.adj[0]; adj[1] = e->fz.adj[1]; }
    if (exact) {
        const uint32_t g = (N + BLOCK - 1) / BLOCK;
        CHK(ensure_partials(e, size_t(g) * g * (NE_NP + 1)));
        if (e->wide) {
            const uint32_t gw = (N + 63) / 64;
            CHK(ensure_partials(e, size_t(gw) * gw * (NE_NP + 1)));
            hipLaunchKernelGGL(k_wnonedge_exact, dim3(gw, gw), dim3(BLOCK), 0, e->stream, e->d_psi[e->pcur], N, int(Q), d_Pm, d_cab, invN,
                               int(want_entropy), e->d_partials);
            HIPCHK(hipGetLastError());
            CHK(fold_to_host(e, gw * gw, NE_NP, NE_NP + 1, all));
        } else {
        DISPATCH_Q(Q, hipLaunchKernelGGL((k_nonedge_exact<QQ>), dim3(g, g), dim3(BLOCK), 0, e->stream, e->d_psi[e->pcur], N,
                                         e->d_psi[e->pcur], N, d_Pm, d_cab, invN, int(want_entropy), e->d_partials));
        HIPCHK(hipGetLastError());
        CHK(fold_to_host(e, g * g, NE_NP, NE_NP + 1, all));
        }
    } else {
        const int K = series_order(Q, N, e->series_order, wmax);
        const uint32_t T = series_len(Q, K);
        CHK(ensure_small(e, T));
        CHK(moments_to_device(e, K, T, e->d_small));
        std::vector<double> Mk(T);
        CHK(read_doubles(e, e->d_small, T, Mk.data()));
        nonedge_series(Q, N, K, want_entropy, Mk.data(), mats.data(), all);
    }
    if (!adj_known) {
        CHK(ensure_small(e, NE_NP));
        CHK(adjacent_pairs_to_device(e, exact, want_entropy, e->d_small));
        CHK(read_doubles(e, e->d_small, NE_NP, adj));
    }
    nonedge_finish(all, adj, N, out);
    return SBMBP_OK;
}

int row_sums(sbmbp_engine *e, std::vector<double> &out /* 2Q + Q*Q */) {
    const uint32_t Q = e->Q;
    const uint32_t T = 2 * Q + Q * Q;
    const uint32_t rows_per_blk = 512;  // one thread per output entry loops over staged rows: keep chunks small, workgroups many
    const uint32_t nb = std::max<uint32_t>(1, (e->N + rows_per_blk - 1) / rows_per_blk);
    CHK(ensure_partials(e, size_t(nb) * T));
    CHK(ensure_small(e, T));
    if (e->wide)
        hipLaunchKernelGGL(k_wrow_sums, dim3(nb), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->d_psi[e->pcur], e->d_true, e->N, rows_per_blk,
                           int(Q), e->d_partials);
    else
    DISPATCH_Q(Q, hipLaunchKernelGGL((k_row_sums<QQ>), dim3(nb), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->d_psi[e->pcur],
                                     e->d_true, e->N, rows_per_blk, e->d_partials));
    HIPCHK(hipGetLastError());
    CHK(fold_matrix_to_device(e, nb, T, e->d_small));
    out.resize(T);
    HIPCHK(hipMemcpyAsync(out.data(), e->d_small, size_t(T) * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return SBMBP_OK;
}

int em_expect(sbmbp_engine *e, double *na_e, double *nna_e, double *cab_e) {
    if (!e->have_params || !e->have_state) { set_error("engine has no parameters or no state"); return SBMBP_ERR_STATE; }
    const uint32_t Q = e->Q;
    std::vector<double> rs;
    CHK(row_sums(e, rs));
    const double *na = rs.data(), *nna = rs.data() + Q;
    const uint32_t T = Q * (Q + 1) / 2;
    std::vector<double> tri(T);
    if (e->wide) {  // Q > 16: the numerators as a labels x labels product over the edges on the matrix cores (k_wem)
        if (cab_e) {
            const uint32_t nbw = uint32_t(std::min<uint64_t>(1024, std::max<uint64_t>(1, (e->E2 + WCAP - 1) / WCAP)));
            CHK(ensure_partials(e, size_t(nbw) * Q * Q));
            CHK(ensure_small(e, size_t(Q) * Q));
            DISPATCH_QT(Q, hipLaunchKernelGGL((k_wem<QT>), dim3(nbw), dim3(WTPB), 0, e->stream, e->d_rev, e->d_M[e->cur], uint64_t(e->E2),
                                              e->d_Pw, int(Q), e->d_partials));
            HIPCHK(hipGetLastError());
            CHK(fold_matrix_to_device(e, nbw, Q * Q, e->d_small));
            std::vector<double> G(size_t(Q) * Q);
            HIPCHK(hipMemcpyAsync(G.data(), e->d_small, G.size() * 8, hipMemcpyDeviceToHost, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
            uint32_t t = 0;
            for (uint32_t q1 = 0; q1 < Q; ++q1)
                for (uint32_t q2 = q1; q2 < Q; ++q2, ++t)
                    tri[t] = e->cab[q1 * Q + q2] * (q1 == q2 ? G[q1 * Q + q1] : G[q1 * Q + q2] + G[q2 * Q + q1]);
        }
    } else
    if (fused_ok(e) && Q <= 8) {
        // the numerators come out of the fused pass, which also leaves the free-energy terms the EM loop asks for next
        CHK(fused_pass(e, false, true));
        tri = e->fz.tri;
    } else {
    const uint32_t nb = uint32_t(std::min<uint64_t>(2048, std::max<uint64_t>(1, (e->E2 + BLOCK - 1) / BLOCK)));
    CHK(ensure_partials(e, size_t(nb) * (T + 1)));
    // k_em_edges reads cab/invN from the parameter block, which is in sync with the host mirror here:
    // sbmbp_set_params uploads, and inside learning the preceding converge uploaded.
    const double *M = e->d_M[e->cur];
    const double *Min = (e->sharded && e->incoming_src == 0) ? e->d_Min.get() : nullptr;
    DISPATCH_QB(Q, e->dc == 2, hipLaunchKernelGGL((k_em_edges<QQ, BB>), dim3(nb), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->d_rev,
                                                  e->d_nbr, e->d_deg, e->d_src, M, Min, uint32_t(e->E2), e->d_P, e->d_partials));
    HIPCHK(hipGetLastError());
    CHK(fold_to_host(e, nb, T, T + 1, tri.data()));
    }
    std::vector<double> ce(Q * Q, 0.0);
    em_rescale(Q, e->N, e->dc, na, nna, tri.data(), ce.data());
    if (na_e) std::copy(na, na + Q, na_e);
    if (nna_e) std::copy(nna, nna + Q, nna_e);
    if (cab_e) std::copy(ce.begin(), ce.end(), cab_e);
    return SBMBP_OK;
}

int free_energy_impl(sbmbp_engine *e, double *f, double *parts) {
    if (!e->field_fresh) CHK(refresh_field(e));
    double se[4], ne[2];
    CHK(site_edge_terms(e, false, se));
    CHK(nonedge_terms(e, false, ne));
    double p[4];
    site_edge_parts(e->N, e->dc == 1 ? &e->sum_log_didl : nullptr, se, p);
    const double fp[3] = {p[0], p[1], ne[0]};
    if (parts) std::copy(fp, fp + 3, parts);
    if (f) *f = free_energy_of(fp);
    return SBMBP_OK;
}

int entropy_impl(sbmbp_engine *e, double *ent, double *parts) {
    if (e->dc != 0) {  // the reference evaluates 0/0 in e_site for deg_corr_flag != 0 (bp.cpp:550-556)
        const double nan = std::numeric_limits<double>::quiet_NaN();
        if (parts) { parts[0] = nan; parts[1] = nan; parts[2] = 0.0; }
        if (ent) *ent = nan;
        return SBMBP_OK;
    }
    if (!e->field_fresh) CHK(refresh_field(e));
    double se[4], ne[2];
    CHK(site_edge_terms(e, true, se));
    CHK(nonedge_terms(e, true, ne));
    double p[4];
    site_edge_parts(e->N, nullptr, se, p);
    const double ep[3] = {p[2], p[3], ne[1]};
    if (parts) std::copy(ep, ep + 3, parts);
    if (ent) *ent = entropy_of(ep);
    return SBMBP_OK;
}

int overlap_impl(sbmbp_engine *e, double *ov, double *Cout) {
    if (!e->have_state) { set_error("engine has no state"); return SBMBP_ERR_STATE; }
    const uint32_t Q = e->Q;
    std::vector<double> rs;
    CHK(row_sums(e, rs));
    const double *C = rs.data() + 2 * Q;
    if (Cout) std::copy(C, C + Q * Q, Cout);
    if (ov) *ov = best_overlap(Q, e->N, C);
    return SBMBP_OK;
}

void apply_params_host(sbmbp_engine *e, const double *cab, const uint32_t *na, double beta) {
    const uint32_t Q = e->Q;
    e->cab.assign(cab, cab + Q * Q);
    e->na.assign(na, na + Q);
    e->eta.resize(Q);
    for (uint32_t q = 0; q < Q; ++q) e->eta[q] = 1.0 * e->na[q] / e->Nglob;  // bp.cpp:307
    e->beta = beta;
    e->have_params = true;
    e->field_fresh = false;
    e->psi_consistent = false; e->fz.valid = false;  // the reconstruction psi / (W^T m) needs the W the marginals were formed with
    e->w_positive = true;
    for (uint32_t a = 0; a < Q * Q; ++a)
        if (!(cab[a] > 0.0) || !(cab[a] < 1e300)) e->w_positive = false;
}

}  // namespace

// =============================================== C ABI ==========================================
#define NOT_SHARD(e) do { if ((e)->sharded) { set_error("not available on a sharded engine: use the shard steps (sbm-bp_amd/distributed.py)"); return SBMBP_ERR_UNSUPPORTED; } } while (0)
#define IS_SHARD(e) do { if (!(e) || !(e)->sharded) { set_error("engine was not created with sbmbp_shard_create"); return SBMBP_ERR_ARG; } } while (0)

extern "C" {

const char *sbmbp_strerror(int code) {
    switch (code) {
        case SBMBP_OK: return "ok";
        case SBMBP_ERR_ARG: return "invalid argument";
        case SBMBP_ERR_HIP: return "HIP runtime error";
        case SBMBP_ERR_NODEVICE: return "no usable GPU (this engine has no CPU fallback)";
        case SBMBP_ERR_STATE: return "call order violated";
        case SBMBP_ERR_IO: return "I/O error";
        case SBMBP_ERR_UNSUPPORTED: return "unsupported configuration";
        case SBMBP_ERR_NOMEM: return "out of device memory";
        case SBMBP_ERR_COMM: return "collective communication failed";
        default: return "unknown error";
    }
}
const char *sbmbp_last_error(void) { return get_error().c_str(); }
const char *sbmbp_version(void) { return "sbmbp-hip 0.2 (gfx950)"; }
int sbmbp_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int sbmbp_graph_load_edgelist(sbmbp_graph_t **out, const char *path, uint32_t n_vertices) {
    if (!out || !path) return arg_error(__func__, __LINE__);
    std::vector<uint32_t> pairs;
    CHK(read_edgelist(path, pairs));
    auto *g = new sbmbp_graph();
    int r = graph_from_pairs(*g, pairs.data(), pairs.size() / 2, n_vertices);
    if (r != SBMBP_OK) { delete g; return r; }
    *out = g;
    return SBMBP_OK;
}
int sbmbp_graph_from_edges(sbmbp_graph_t **out, const uint32_t *pairs, uint64_t n_pairs, uint32_t n_vertices) {
    if (!out || (!pairs && n_pairs)) return arg_error(__func__, __LINE__);
    auto *g = new sbmbp_graph();
    int r = graph_from_pairs(*g, pairs, n_pairs, n_vertices);
    if (r != SBMBP_OK) { delete g; return r; }
    *out = g;
    return SBMBP_OK;
}
int sbmbp_graph_from_csr(sbmbp_graph_t **out, uint32_t n, uint64_t e2, const uint64_t *row_ptr, const uint32_t *nbr,
                         const uint32_t *rev) {
    if (!out) return arg_error(__func__, __LINE__);
    auto *g = new sbmbp_graph();
    int r = graph_from_csr(*g, n, e2, row_ptr, nbr, rev);
    if (r != SBMBP_OK) { delete g; return r; }
    *out = g;
    return SBMBP_OK;
}
uint32_t sbmbp_graph_num_vertices(const sbmbp_graph_t *g) { return g ? g->n : 0; }
uint64_t sbmbp_graph_num_directed_edges(const sbmbp_graph_t *g) { return g ? g->e2() : 0; }
uint32_t sbmbp_graph_max_degree(const sbmbp_graph_t *g) { return g ? g->max_degree : 0; }
int sbmbp_graph_copy_csr(const sbmbp_graph_t *g, uint64_t *row_ptr, uint32_t *nbr, uint32_t *rev) {
    if (!g) return arg_error(__func__, __LINE__);
    if (row_ptr) std::copy(g->row_ptr.begin(), g->row_ptr.end(), row_ptr);
    if (nbr) std::copy(g->nbr.begin(), g->nbr.end(), nbr);
    if (rev) std::copy(g->rev.begin(), g->rev.end(), rev);
    return SBMBP_OK;
}
void sbmbp_graph_destroy(sbmbp_graph_t *g) { delete g; }

int sbmbp_param_from_epsilon_c(uint32_t N, uint32_t Q, double epsilon, double c, double *cab, uint32_t *na) {
    if (!cab || !na || Q < 1) return arg_error(__func__, __LINE__);
    param_from_epsilon_c(N, Q, epsilon, c, cab, na);
    return SBMBP_OK;
}
int sbmbp_param_from_direct(uint32_t N, uint32_t Q, const double *pa, const double *cab_upper, double *cab, uint32_t *na) {
    if (!cab || !na || !pa || !cab_upper || Q < 1) return arg_error(__func__, __LINE__);
    param_from_direct(N, Q, pa, cab_upper, cab, na);
    return SBMBP_OK;
}

// sbmbp_create; own_state = false leaves the message, marginal and parameter buffers to the caller (the replica batch)
static int create_engine(sbmbp_engine_t **out, const sbmbp_graph_t *g, uint32_t Q, uint32_t dc, int device, bool own_state) {
    if (Q < 2 || Q > SBMBP_MAX_Q) { set_error("Q must be in [2, 64]"); return SBMBP_ERR_UNSUPPORTED; }
    if (dc > 2) { set_error("deg_corr_flag must be 0, 1 or 2"); return SBMBP_ERR_ARG; }
    if (Q > 16 && dc == 2) { set_error("deg_corr_flag 2 is implemented up to Q = 16"); return SBMBP_ERR_UNSUPPORTED; }
    if (g->n == 0) { set_error("empty graph"); return SBMBP_ERR_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        set_error("no HIP device visible; the engine has no CPU fallback");
        return SBMBP_ERR_NODEVICE;
    }
    if (device >= 0) HIPCHK(hipSetDevice(device));
    std::unique_ptr<sbmbp_engine> owner(new sbmbp_engine());
    sbmbp_engine *e = owner.get();
    HIPCHK(hipGetDevice(&e->device));
    e->N = g->n;
    e->Nglob = g->n;
    e->Q = Q;
    e->dc = dc;
    e->wide = Q > 16;
    e->E2 = g->e2();
    HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    e->own_stream = true;
    segment_plan_t plan;  // one chunk: the shard's decomposition (sbmbp_shard_create) without boundaries inside
    segment_plan(g->row_ptr.data(), g->n, uint32_t(frame_cap(Q)), uint32_t(frame_rcap(Q)), {}, plan);
    CHK(ensure_partials(e, (plan.blk_row.size() - 1) * (QMAX + 1)));
    CHK(setup_graph_tables(e, plan, g->row_ptr.data(), g->nbr.data(), g->rev.data(), true, !e->wide));  // (the wide sweep walks a long row itself)
    if (own_state) {
        CHK(dev_alloc(e, e->d_M[0], std::max<uint64_t>(e->E2, 1) * rec_len(e)));  // records of Q-1 components (Q above 16 labels); >= one record: the sweep's loads are branch-free
        CHK(dev_alloc(e, e->d_M[1], std::max<uint64_t>(e->E2, 1) * rec_len(e)));
        CHK(dev_alloc(e, e->d_psi[0], size_t(e->N) * Q));
        CHK(dev_alloc(e, e->d_psi[1], size_t(e->N) * Q));
        CHK(dev_alloc(e, e->d_P, 1));
    }
    if (e->wide) CHK(dev_alloc(e, e->d_Pw, 1));
    CHK(dev_alloc(e, e->d_mats, 3 * Q * Q));
    if (const char *fr = std::getenv("SBMBP_FUSED_REDUCTIONS")) e->fused_reductions = std::atoi(fr);
    e->hist_cap = 4096;
    CHK(dev_alloc(e, e->d_hist, e->hist_cap));
    CHK(dev_alloc(e, e->d_fold_counters, 1));
    HIPCHK(hipMemsetAsync(e->d_fold_counters, 0, 4, e->stream));
    CHK(ensure_small(e, 8192));
    CHK(dev_alloc(e, e->d_stage, size_t(FOLD_BLOCKS) * FOLD_STRIDE_MAX));
    std::vector<uint32_t> deg(dc == 2 ? e->N : 0);
    if (dc == 2) {
        for (uint32_t i = 0; i < g->n; ++i) deg[i] = g->deg(i);
        CHK(dev_upload(e, e->d_deg, deg));
    }
    HIPCHK(hipStreamSynchronize(e->stream));  // (deg is a local)
    *out = owner.release();
    return SBMBP_OK;
}

int sbmbp_create(sbmbp_engine_t **out, const sbmbp_graph_t *g, uint32_t Q, uint32_t dc, int device) {
    if (!out || !g) return arg_error(__func__, __LINE__);
    return create_engine(out, g, Q, dc, device, true);
}

// ~sbmbp_engine drains the stream, the buffers go with the members, ~engine_stream destroys the events and the stream
void sbmbp_destroy(sbmbp_engine_t *e) { delete e; }

int sbmbp_set_stream(sbmbp_engine_t *e, void *hip_stream) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->own_stream && e->stream) HIPCHK(hipStreamDestroy(e->stream));
    e->stream = static_cast<hipStream_t>(hip_stream);  // 0 is the (legacy) default stream, e.g. torch's current stream
    e->own_stream = false;
    return SBMBP_OK;
}

static int upload_labels(sbmbp_engine_t *e, const int32_t *conf, const uint32_t *true_conf, uint32_t flag, int conditional) {
    if (true_conf) {
        for (uint32_t i = 0; i < e->N; ++i)
            if (true_conf[i] >= e->Q) { set_error("true_conf entry out of range"); return SBMBP_ERR_ARG; }
        e->true_conf.assign(true_conf, true_conf + e->N);
        HIPCHK(hipMemcpyAsync(e->d_true, true_conf, size_t(e->N) * 4, hipMemcpyHostToDevice, e->stream));
    }
    // bp_conditional skips rows with conf_planted_ != -1 (bp.cpp:1104); with -i 0 the planted vector
    // is never stored, so nothing is clamped.
    e->has_clamp = false;
    if (conditional && flag != 0 && conf) {
        for (uint32_t i = 0; i < e->N; ++i) {
            if (conf[i] < -1 || conf[i] >= int32_t(e->Q)) { set_error("conf entry out of range"); return SBMBP_ERR_ARG; }
            if (conf[i] != -1) e->has_clamp = true;
        }
        HIPCHK(hipMemcpyAsync(e->d_clamp, conf, size_t(e->N) * 4, hipMemcpyHostToDevice, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return SBMBP_OK;
}

int sbmbp_init_messages(sbmbp_engine_t *e, uint32_t flag, const int32_t *conf, const uint32_t *true_conf, uint32_t seed,
                        int conditional) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    if (flag >= 4) { set_error("bp_messages_init_flag must be < 4"); return SBMBP_ERR_ARG; }  // assert at bp.cpp:106
    if (flag != 0 && !conf) { set_error("init flag != 0 needs a conf vector"); return SBMBP_ERR_ARG; }
    CHK(upload_labels(e, conf, true_conf, flag, conditional));
    // the state is generated in slabs of consecutive vertices and each slab is uploaded (marginal rows as they are,
    // messages through the Q -> Q-1 record conversion) while the host already generates the next one
    const uint32_t Q = e->Q;
    device_buffer<double> tmp;                // the Q-component messages of a slab, grown to the largest slab
    pinned_buffer<double> pin_psi, pin_msg;  // page-locked slab buffers: the uploads run at link speed
    state_sink sink;
    sink.alloc = [&](uint64_t np, uint64_t nm, double **pb, double **mb) {  // (false: the generator takes pageable buffers)
        if (pin_psi.alloc(np) != SBMBP_OK || pin_msg.alloc(nm) != SBMBP_OK) return false;
        *pb = pin_psi;
        *mb = pin_msg;
        return true;
    };
    auto put = [&](uint32_t lo, uint32_t hi, const double *prow, const double *mrow) -> int {
        HIPCHK(hipMemcpyAsync(e->d_psi[e->pcur] + size_t(lo) * Q, prow, size_t(hi - lo) * Q * 8, hipMemcpyHostToDevice, e->stream));
        const uint64_t k0 = e->h_row_ptr[lo], nm = uint64_t(e->h_row_ptr[hi]) - k0;
        if (nm && e->wide) {  // full records: straight into the message buffer
            HIPCHK(hipMemcpyAsync(e->d_M[e->cur] + k0 * Q, mrow, nm * Q * 8, hipMemcpyHostToDevice, e->stream));
        } else if (nm) {
            CHK(tmp.ensure(nm * Q));  // (nothing in flight reads it: every slab ends with a synchronisation)
            HIPCHK(hipMemcpyAsync(tmp, mrow, nm * Q * 8, hipMemcpyHostToDevice, e->stream));
            hipLaunchKernelGGL(k_msgs_to_records, dim3(uint32_t((nm + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, e->stream, tmp.get(), nm,
                               int(Q), e->d_M[e->cur] + k0 * (Q - 1));
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(e->stream));  // the slab buffers are reused by the next slab
        return SBMBP_OK;
    };
    int put_rc = SBMBP_OK;  // the first failure: the slabs behind it are dropped
    sink.put = [&](uint32_t lo, uint32_t hi, const double *prow, const double *mrow) {
        if (put_rc == SBMBP_OK && hi > lo) put_rc = put(lo, hi, prow, mrow);
    };
    init_state_host(e->N, e->h_row_ptr.data(), e->E2, Q, flag, conf, seed, nullptr, nullptr, &sink);
    CHK(put_rc);
    // a sharded engine takes the declared state as (psi^0, m^-1): sweep 0 reads the buffer it then overwrites
    if (e->E2 && e->sharded)
        HIPCHK(hipMemcpyAsync(e->d_M[e->cur ^ 1], e->d_M[e->cur], e->E2 * (Q - 1) * 8, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->have_state = true;
    e->field_fresh = false;
    e->psi_consistent = false; e->fz.valid = false;
    e->init_from_psi = false;
    e->clamp_onehot = (flag == 1 || flag == 3);  // clamped rows now hold one-hot marginals and messages
    return SBMBP_OK;
}

int sbmbp_host_init_state(const sbmbp_graph_t *g, uint32_t Q, uint32_t flag, const int32_t *conf, uint32_t seed, double *psi,
                          double *msg_out) {
    if (!g || !psi || (!msg_out && !g->nbr.empty()) || Q < 1 || Q > SBMBP_MAX_Q) return arg_error(__func__, __LINE__);
    if (flag >= 4) { set_error("bp_messages_init_flag must be < 4"); return SBMBP_ERR_ARG; }
    if (flag != 0 && !conf) { set_error("init flag != 0 needs a conf vector"); return SBMBP_ERR_ARG; }
    std::vector<uint32_t> rp32(g->row_ptr.begin(), g->row_ptr.end());
    init_state_host(g->n, rp32.data(), g->nbr.size(), Q, flag, conf, seed, psi, msg_out);
    return SBMBP_OK;
}

int sbmbp_init_messages_device(sbmbp_engine_t *e, uint64_t seed, const uint32_t *true_conf) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    CHK(upload_labels(e, nullptr, true_conf, 0, 0));
    // random marginals (counter-based generator keyed by the GLOBAL row id, so shards draw what the single engine draws);
    // every out-message of a row starts as the row's marginal
    hipLaunchKernelGGL(k_init_random, dim3((e->N + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, e->stream, e->d_psi[e->pcur], uint64_t(e->N),
                       int(e->Q), int(e->Q), seed, 0x1234567ull, uint64_t(e->row0));
    if (e->E2 && e->wide)
        hipLaunchKernelGGL(k_winit_msgs_from_psi, dim3(e->N), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->d_psi[e->pcur], e->N, int(e->Q),
                           e->d_M[0], e->d_M[1]);
    else if (e->E2) {
        DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_init_msgs_from_psi_seg<QQ>), dim3(e->n_blk), dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr,
                                            e->d_psi[e->pcur], e->d_blk_row, e->d_blk_e0, e->d_M[0], e->d_M[1]));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    e->have_state = true;
    e->field_fresh = false;
    e->psi_consistent = false; e->fz.valid = false;
    e->init_from_psi = true;
    e->clamp_onehot = false;
    return SBMBP_OK;
}

int sbmbp_set_params(sbmbp_engine_t *e, const double *cab, const uint32_t *na, double beta) {
    device_scope dev_(e);
    if (!e || !cab || !na) return arg_error(__func__, __LINE__);
    apply_params_host(e, cab, na, beta);
    if (e->wide && !e->w_positive) { set_error("above Q = 16 every cab entry must be > 0"); e->have_params = false; return SBMBP_ERR_UNSUPPORTED; }
    return upload_params(e, 0.0);
}
int sbmbp_get_params(sbmbp_engine_t *e, double *cab, uint32_t *na) {
    device_scope dev_(e);
    if (!e || !e->have_params) return SBMBP_ERR_STATE;
    if (cab) std::copy(e->cab.begin(), e->cab.end(), cab);
    if (na) std::copy(e->na.begin(), e->na.end(), na);
    return SBMBP_OK;
}

// The boundary speaks Q components per message; the device keeps records of Q-1 (kernels.h: msg_rec). The
// conversion runs on the device, through a bounded staging buffer.
static constexpr uint64_t STATE_SLAB = uint64_t(16) << 20;  // messages per staging pass

static int upload_messages(sbmbp_engine *e, const double *msg_out, double *dst) {
    if (e->wide) {  // full records on the device too
        HIPCHK(hipMemcpyAsync(dst, msg_out, e->E2 * e->Q * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return SBMBP_OK;
    }
    const uint64_t slab = std::min<uint64_t>(e->E2, STATE_SLAB);
    device_buffer<double> tmp;
    CHK(tmp.alloc(slab * e->Q));
    for (uint64_t k0 = 0; k0 < e->E2; k0 += slab) {
        const uint64_t n = std::min(slab, e->E2 - k0);
        HIPCHK(hipMemcpyAsync(tmp, msg_out + k0 * e->Q, n * e->Q * 8, hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(k_msgs_to_records, dim3(uint32_t((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, e->stream, tmp.get(), n,
                           int(e->Q), dst + k0 * (e->Q - 1));
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return SBMBP_OK;
}

static int download_messages(sbmbp_engine *e, const double *src, double *msg_out) {
    if (e->wide) {
        HIPCHK(hipMemcpyAsync(msg_out, src, e->E2 * e->Q * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return SBMBP_OK;
    }
    const uint64_t slab = std::min<uint64_t>(e->E2, STATE_SLAB);
    device_buffer<double> tmp;
    CHK(tmp.alloc(slab * e->Q));
    for (uint64_t k0 = 0; k0 < e->E2; k0 += slab) {
        const uint64_t n = std::min(slab, e->E2 - k0);
        hipLaunchKernelGGL(k_records_to_msgs, dim3(uint32_t((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, e->stream, src + k0 * (e->Q - 1), n,
                           int(e->Q), tmp.get());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(msg_out + k0 * e->Q, tmp, n * e->Q * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return SBMBP_OK;
}

int sbmbp_set_state(sbmbp_engine_t *e, const double *psi, const double *msg_out) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    if (psi) HIPCHK(hipMemcpyAsync(e->d_psi[e->pcur], psi, size_t(e->N) * e->Q * 8, hipMemcpyHostToDevice, e->stream));
    if (msg_out && e->E2) CHK(upload_messages(e, msg_out, e->d_M[e->cur]));
    // a sharded engine takes the declared state as (psi^0, m^-1): sweep 0 reads the buffer it then overwrites
    if (msg_out && e->E2 && e->sharded)
        HIPCHK(hipMemcpyAsync(e->d_M[e->cur ^ 1], e->d_M[e->cur], e->E2 * (e->Q - 1) * 8, hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (psi && (msg_out || e->E2 == 0)) e->have_state = true;  // a graph without edges has no messages
    e->field_fresh = false;
    e->psi_consistent = false; e->fz.valid = false;
    e->init_from_psi = false;
    e->clamp_onehot = false;  // an arbitrary state: clamped rows need the general (message-gather) sweep
    return SBMBP_OK;
}

// ---- per-vertex prior ------------------------------------------------------------------------------
// first row of an N x Q table that is no prior line (a negative, NaN or Inf entry, or no positive one), or N
static uint32_t first_bad_prior_row(const double *prior, uint32_t N, uint32_t Q, std::string *why) {
    for (uint32_t i = 0; i < N; ++i) {
        bool pos = false;
        for (uint32_t q = 0; q < Q; ++q) {
            const double w = prior[size_t(i) * Q + q];
            if (!(w >= 0.0) || std::isinf(w)) { *why = "entry " + std::to_string(q) + " is negative, NaN or Inf"; return i; }
            pos = pos || w > 0.0;
        }
        if (!pos) { *why = "no entry is positive"; return i; }
    }
    return N;
}

int sbmbp_set_vertex_prior(sbmbp_engine_t *e, const double *prior) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    if (prior == nullptr) {  // remove
        if (e->d_prior) {
            HIPCHK(hipStreamSynchronize(e->stream));
            e->d_prior.reset();
            e->psi_consistent = false; e->fz.valid = false;
        }
        return SBMBP_OK;
    }
    if (e->wide) { set_error("a per-vertex prior is implemented up to Q = 16 (the lane-per-edge kernels); Q = " + std::to_string(e->Q)); return SBMBP_ERR_UNSUPPORTED; }
    if (e->sharded) { set_error("a per-vertex prior runs on the single engine only: a shard engine takes none"); return SBMBP_ERR_UNSUPPORTED; }
    if (e->sweep_order == 1) { set_error("a per-vertex prior cannot be combined with the coloured sweep order: sbmbp_set_sweep_order(e, 0, ...) first"); return SBMBP_ERR_UNSUPPORTED; }
    std::string why;
    const uint32_t bad = first_bad_prior_row(prior, e->N, e->Q, &why);
    if (bad < e->N) { set_error("sbmbp_set_vertex_prior: prior row of vertex " + std::to_string(bad) + ": " + why); return SBMBP_ERR_ARG; }
    if (!e->d_prior) CHK(dev_alloc(e, e->d_prior, size_t(e->N) * e->Q));
    HIPCHK(hipMemcpyAsync(e->d_prior, prior, size_t(e->N) * e->Q * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->psi_consistent = false; e->fz.valid = false;
    return SBMBP_OK;
}
int sbmbp_get_vertex_prior(sbmbp_engine_t *e, double *prior, int *present) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    if (present) *present = e->d_prior ? 1 : 0;
    if (prior && e->d_prior) {
        HIPCHK(hipMemcpyAsync(prior, e->d_prior, size_t(e->N) * e->Q * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return SBMBP_OK;
}
int sbmbp_prior_load(const char *path, uint32_t n_vertices, uint32_t Q, double *prior, uint64_t *n_rows_given) {
    if (!path || !prior || Q < 1) return arg_error(__func__, __LINE__);
    return read_prior_table(path, n_vertices, Q, prior, n_rows_given);
}

int sbmbp_get_state(sbmbp_engine_t *e, double *psi, double *msg_out) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    if (psi) HIPCHK(hipMemcpyAsync(psi, e->d_psi[e->pcur], size_t(e->N) * e->Q * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (msg_out && e->E2) CHK(download_messages(e, e->d_M[e->cur], msg_out));
    return SBMBP_OK;
}
int sbmbp_get_field(sbmbp_engine_t *e, double *h) {
    device_scope dev_(e);
    if (!e || !h) return arg_error(__func__, __LINE__);
    NOT_SHARD(e);
    // behind coloured sweeps the field on the device is the one the sweeps maintained step by step: report THAT one
    if (!(e->cs_last && e->field_fresh)) CHK(refresh_field(e));
    if (e->wide) {
        std::vector<double> hn(e->Q);
        HIPCHK(hipMemcpyAsync(hn.data(), reinterpret_cast<const char *>(e->d_Pw.get()) + offsetof(dev_wide, hN), size_t(e->Q) * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (uint32_t q = 0; q < e->Q; ++q) h[q] = hn[q] * double(e->N);
        return SBMBP_OK;
    }
    dev_params P;
    HIPCHK(hipMemcpyAsync(&P, e->d_P, sizeof P, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (uint32_t q = 0; q < e->Q; ++q) h[q] = P.hN[q] * double(e->N);
    return SBMBP_OK;
}

int sbmbp_set_schedule(sbmbp_engine_t *e, double field_mix, uint32_t check_every) {
    device_scope dev_(e);
    if (!e || !(field_mix > 0.0) || field_mix > 1.0 || check_every < 1) return arg_error(__func__, __LINE__);
    e->field_mix = field_mix;
    e->check_every = check_every;
    return SBMBP_OK;
}

int sbmbp_set_learning_schedule(sbmbp_engine_t *e, double field_mix, double snap) {
    device_scope dev_(e);
    if (!e || !(field_mix > 0.0) || field_mix > 1.0 || !(snap >= 0.0)) return arg_error(__func__, __LINE__);
    e->learn_field_mix = field_mix;
    e->learn_snap = snap;
    return SBMBP_OK;
}

int sbmbp_set_auto_relax(sbmbp_engine_t *e, int on) {
    if (!e) return arg_error(__func__, __LINE__);
    e->auto_relax = on != 0;
    return SBMBP_OK;
}
int sbmbp_get_relaxation(const sbmbp_engine_t *e, int *field_level, int *generic_level, double *field_mix, double *damping_factor) {
    if (!e) return arg_error(__func__, __LINE__);
    if (field_level) *field_level = e->ar_fl;
    if (generic_level) *generic_level = e->ar_gl;
    if (field_mix) *field_mix = e->sweep_order == 1 ? 1.0 : std::min(std::min(e->field_mix, ar_field_cap(e->ar_fl)), ar_gen_mix(e->ar_gl));
    if (damping_factor) *damping_factor = ar_gen_damp(e->ar_gl);
    return SBMBP_OK;
}

int sbmbp_set_gather_mode(sbmbp_engine_t *e, int mode) {
    device_scope dev_(e);
    if (!e || mode < 0 || mode > 1) return arg_error(__func__, __LINE__);
    e->gather_mode = mode;
    return SBMBP_OK;
}

int sbmbp_coloured_plan(const sbmbp_graph_t *g, const uint32_t *colour_in, double step_fraction, uint32_t *n_colours, uint32_t *n_steps,
                        uint32_t *colour, uint32_t *step) {
    if (!g) return arg_error(__func__, __LINE__);
    std::vector<uint32_t> col, st;
    CHK(coloured_plan(g->n, g->row_ptr.data(), g->nbr.data(), colour_in, step_fraction, col, st, n_colours, n_steps));
    if (colour) std::copy(col.begin(), col.end(), colour);
    if (step) std::copy(st.begin(), st.end(), step);
    return SBMBP_OK;
}

int sbmbp_set_sweep_order(sbmbp_engine_t *e, int order, const uint32_t *colour, double step_fraction) {
    device_scope dev_(e);
    if (!e || order < 0 || order > 1) return arg_error(__func__, __LINE__);
    if (order == 0) { e->sweep_order = 0; return SBMBP_OK; }
    if (e->sharded) { set_error("the coloured sweep order runs on the single engine only: a shard engine sweeps synchronously"); return SBMBP_ERR_UNSUPPORTED; }
    if (e->wide) { set_error("the coloured sweep order is implemented up to Q = 16"); return SBMBP_ERR_UNSUPPORTED; }
    if (e->d_prior) { set_error("the coloured sweep order takes no per-vertex prior: remove it first (sbmbp_set_vertex_prior(e, NULL))"); return SBMBP_ERR_UNSUPPORTED; }
    // the engine keeps the row offsets on the host; the neighbour lists come back from the device (first use only)
    std::vector<uint64_t> rp(e->h_row_ptr.begin(), e->h_row_ptr.end());
    std::vector<uint32_t> nbr(e->E2);
    if (e->E2) HIPCHK(hipMemcpyAsync(nbr.data(), e->d_nbr, e->E2 * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<uint32_t> col, st;
    uint32_t nc = 0, ns = 0;
    CHK(coloured_plan(e->N, rp.data(), nbr.data(), colour, step_fraction, col, st, &nc, &ns));
    int r = build_coloured(e, st, nc, ns);
    if (r != SBMBP_OK) { free_coloured(e); e->sweep_order = 0; return r; }
    e->sweep_order = 1;
    return SBMBP_OK;
}
int sbmbp_get_sweep_order(const sbmbp_engine_t *e, int *order, uint32_t *n_colours, uint32_t *n_steps) {
    if (!e) return arg_error(__func__, __LINE__);
    if (order) *order = e->sweep_order;
    if (n_colours) *n_colours = e->sweep_order == 1 ? e->cs_colours : 0;
    if (n_steps) *n_steps = e->sweep_order == 1 ? e->cs_steps : 0;
    return SBMBP_OK;
}

int sbmbp_converge(sbmbp_engine_t *e, double crit, uint32_t max_sweeps, double damping, int *niter, double *last) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    NOT_SHARD(e);
    return run_sweeps(e, crit, max_sweeps, damping, niter, last);
}
int sbmbp_sweep(sbmbp_engine_t *e, double damping, uint32_t n_sweeps, double *last) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    NOT_SHARD(e);
    const uint32_t keep = e->check_every;
    e->check_every = std::max<uint32_t>(keep, 64);  // no convergence test: sync rarely
    int r = run_sweeps(e, -1.0, n_sweeps, damping, nullptr, last);
    e->check_every = keep;
    return r;
}

int sbmbp_free_energy(sbmbp_engine_t *e, double *f, double *parts) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    NOT_SHARD(e);
    return free_energy_impl(e, f, parts);
}
int sbmbp_entropy(sbmbp_engine_t *e, double *ent, double *parts) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    NOT_SHARD(e);
    return entropy_impl(e, ent, parts);
}
int sbmbp_set_nonedge_mode(sbmbp_engine_t *e, int mode, int order) {
    device_scope dev_(e);
    if (!e || mode < 0 || mode > 2 || order < 0 || order > 4) return arg_error(__func__, __LINE__);
    if (mode != e->nonedge_mode || order != e->series_order) e->fz.valid = false;  // the fused pass's adjacent pairs are of one form
    e->nonedge_mode = mode;
    e->series_order = order;
    return SBMBP_OK;
}
int sbmbp_em_expectations(sbmbp_engine_t *e, double *na_e, double *nna_e, double *cab_e) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    NOT_SHARD(e);
    return em_expect(e, na_e, nna_e, cab_e);
}
int sbmbp_confusion(sbmbp_engine_t *e, double *C) {
    device_scope dev_(e);
    if (!e || !C) return arg_error(__func__, __LINE__);
    NOT_SHARD(e);
    return overlap_impl(e, nullptr, C);
}
int sbmbp_overlap(sbmbp_engine_t *e, double *ov) {
    device_scope dev_(e);
    if (!e || !ov) return arg_error(__func__, __LINE__);
    NOT_SHARD(e);
    return overlap_impl(e, ov, nullptr);
}

static int inference_reductions(sbmbp_engine *e, sbmbp_infer_result *out);
int sbmbp_inference(sbmbp_engine_t *e, float conv_crit, uint32_t time_conv, float dumping_rate, sbmbp_infer_result *out) {
    device_scope dev_(e);
    if (!e || !out) return arg_error(__func__, __LINE__);
    NOT_SHARD(e);
    // belief_propagation::inference (bp.cpp:77-99); crit and damping arrive as float, compared as double (:406)
    CHK(run_sweeps(e, double(conv_crit), time_conv, double(dumping_rate), &out->niter, &out->last_maxdiff));
    return inference_reductions(e, out);
}

// free energy, entropy and overlap of the state a converge call left (the second half of inference, bp.cpp:77-99)
static int inference_reductions(sbmbp_engine *e, sbmbp_infer_result *out) {
    if (e->dc != 0) {  // entropy is NaN in the reference for deg_corr_flag != 0: only the free-energy pass runs
        CHK(free_energy_impl(e, &out->free_energy, nullptr));
        CHK(entropy_impl(e, &out->entropy, nullptr));
    } else {  // one pass over the messages yields the site/edge/non-edge terms of both quantities
        if (!e->field_fresh) CHK(refresh_field(e));
        double se[4], ne[2];
        CHK(site_edge_terms(e, true, se));
        CHK(nonedge_terms(e, true, ne));
        double p[4];
        site_edge_parts(e->N, nullptr, se, p);
        const double fp[3] = {p[0], p[1], ne[0]}, ep[3] = {p[2], p[3], ne[1]};
        out->free_energy = free_energy_of(fp);
        out->entropy = entropy_of(ep);
    }
    CHK(overlap_impl(e, &out->overlap, nullptr));
    return SBMBP_OK;
}

int sbmbp_learning(sbmbp_engine_t *e, float learning_conv_crit, uint32_t learning_max_time, float learning_rate,
                   float dumping_rate, sbmbp_learn_result *out) {
    device_scope dev_(e);
    if (!e || !out) return arg_error(__func__, __LINE__);
    NOT_SHARD(e);
    if (!e->have_params || !e->have_state) { set_error("set_params and init_messages must precede learning"); return SBMBP_ERR_STATE; }
    // The reference maintains the global field h incrementally inside its random-sequential sweeps; in the synchronous
    // schedule h lags one sweep, and with poorly matched parameters (the early EM steps) that lag keeps BP near a
    // symmetric saddle the reference leaves (fixture q4_learn_seed2). Relaxing the field, S <- (1-a) S + a sum psi, has
    // the same fixed points and follows the reference there; a = 1 restores plain Jacobi. em_loop
    // lowers field_mix to learn_field_mix for its duration.
    struct front_end {
        sbmbp_engine *e;
        uint32_t max_sweeps;  // of a BP run
        double damping;
        sbmbp_learn_result *out;
        int converge(const double *crit, const uint8_t *, uint32_t *executed) {
            const uint64_t sweeps0 = e->sweeps;
            int niter;
            double last;
            CHK(run_sweeps(e, crit[0], max_sweeps, damping, &niter, &last));
            executed[0] = uint32_t(e->sweeps - sweeps0);
            return SBMBP_OK;
        }
        int expect(const uint8_t *, double *na_e, double *nna_e, double *cab_e, double *f) {
            CHK(em_expect(e, na_e, nna_e, cab_e));
            return free_energy_impl(e, f, nullptr);
        }
        void params(uint32_t, std::vector<uint32_t> &na, std::vector<double> &cab) { na = e->na; cab = e->cab; }
        int apply(uint32_t, const uint32_t *na, const double *cab) { apply_params_host(e, cab, na, e->beta); return SBMBP_OK; }
        int finish(uint32_t) {
            CHK(upload_params(e, 0.0));
            e->field_fresh = false;  // (the parameter block starts from a zero field again)
            return overlap_impl(e, &out->overlap, nullptr);
        }
    } fe{e, learning_max_time, double(dumping_rate), out};
    return em_loop(fe, 1, e->Q, e->N, learning_conv_crit, learning_max_time, double(learning_rate), e->learn_snap, e->field_mix,
                   e->learn_field_mix, out);
}

int sbmbp_get_stats(sbmbp_engine_t *e, sbmbp_stats *out) {
    device_scope dev_(e);
    if (!e || !out) return arg_error(__func__, __LINE__);
    out->sweeps = e->sweeps;
    out->edge_msg_updates = e->sweeps * e->E2;
    out->sweep_kernel_ms = e->sweep_ms;
    out->sweep_launches = e->sweep_launches;
    // B_sweep = E2 (3*8Q + 4) + N (8Q + 8): SURVEY 8(d); dc 2 adds the neighbour index (4 B/edge)
    out->bytes_per_sweep = double(e->E2) * (24.0 * e->Q + 4.0 + (e->dc == 2 ? 4.0 : 0.0)) + double(e->N) * (8.0 * e->Q + 8.0);
    if (e->d_prior) out->bytes_per_sweep += 8.0 * e->Q * double(e->N);  // every row reads its prior line once
    out->device_bytes = e->device_bytes;
    out->n_blocks = e->n_blk;
    out->n_hub_rows = e->n_hub;
    out->hub_edges = e->hub_edges;
    out->psi_form_sweeps = e->psi_sweeps;
    return SBMBP_OK;
}
int sbmbp_reset_stats(sbmbp_engine_t *e) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    e->sweeps = 0;
    e->psi_sweeps = 0;
    e->sweep_ms = 0.0;
    e->sweep_launches = 0;
    return SBMBP_OK;
}
int sbmbp_set_timing(sbmbp_engine_t *e, int on) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    e->timing = on != 0;
    return SBMBP_OK;
}

// ------------------------------------------ shard steps ------------------------------------------

int sbmbp_shard_create(sbmbp_engine_t **out, const sbmbp_shard_desc *d, uint32_t Q, uint32_t dc, int device) {
    if (!out || !d || !d->row_ptr || (!d->nbr_local && d->n_edges) || !d->psi_buf0 || !d->psi_buf1 || !d->red_buf) { set_error("sbmbp_shard_create: null argument"); return SBMBP_ERR_ARG; }
    if (Q < 2 || Q > 16) { set_error("sharded engines: Q must be in [2, 16]"); return SBMBP_ERR_UNSUPPORTED; }
    if (dc > 2) { set_error("deg_corr_flag must be 0, 1 or 2"); return SBMBP_ERR_ARG; }
    if (dc == 2 && (!d->rev_local || !d->table_deg)) { set_error("a dc 2 shard needs rev_local and table_deg (it runs the message-gather sweep)"); return SBMBP_ERR_ARG; }
    if (d->n_halo_msgs && !d->rev_local) { set_error("n_halo_msgs without rev_local"); return SBMBP_ERR_ARG; }
    if (d->rev_local)
        for (uint64_t k = 0; k < d->n_edges; ++k)
            if (d->rev_local[k] >= d->n_edges + d->n_halo_msgs) { set_error("rev_local entry outside the message buffer"); return SBMBP_ERR_ARG; }
    if (d->n_own == 0 || d->n_global == 0) { set_error("empty shard"); return SBMBP_ERR_ARG; }
    if (d->row_ptr[0] != 0 || d->row_ptr[d->n_own] != d->n_edges || d->n_edges >= (uint64_t(1) << 32)) { set_error("shard row_ptr does not span [0, n_edges]"); return SBMBP_ERR_ARG; }
    const uint64_t table_rows = uint64_t(d->n_own) + d->n_halo;
    for (uint64_t k = 0; k < d->n_edges; ++k)
        if (d->nbr_local[k] >= table_rows) { set_error("nbr_local entry outside the marginal table"); return SBMBP_ERR_ARG; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("no HIP device visible; the engine has no CPU fallback"); return SBMBP_ERR_NODEVICE; }
    if (device >= 0) HIPCHK(hipSetDevice(device));
    std::unique_ptr<sbmbp_engine> owner(new sbmbp_engine());
    sbmbp_engine *e = owner.get();
    HIPCHK(hipGetDevice(&e->device));
    e->sharded = true;
    e->N = d->n_own;
    e->Nglob = d->n_global;
    e->n_halo = d->n_halo;
    e->row0 = d->row0;
    e->edge0 = d->edge0;
    e->Q = Q;
    e->dc = dc;
    e->E2 = d->n_edges;
    e->d_psi[0].borrow(static_cast<double *>(d->psi_buf0));  // the three are the caller's, and stay the caller's
    e->d_psi[1].borrow(static_cast<double *>(d->psi_buf1));
    e->d_red.borrow(static_cast<double *>(d->red_buf));
    e->n_halo_msgs = d->n_halo_msgs;
    HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    e->own_stream = true;
    std::vector<uint32_t> chunk_row;  // segments never straddle a chunk boundary
    if (d->n_chunks > 1 && d->chunk_row) chunk_row.assign(d->chunk_row, d->chunk_row + d->n_chunks + 1);
    else chunk_row = {0u, d->n_own};
    if (chunk_row.front() != 0 || chunk_row.back() != d->n_own) { set_error("chunk_row must span [0, n_own]"); return SBMBP_ERR_ARG; }
    for (size_t c = 1; c < chunk_row.size(); ++c)
        if (chunk_row[c] < chunk_row[c - 1]) { set_error("chunk_row not monotone"); return SBMBP_ERR_ARG; }
    for (uint32_t i = 0; i < d->n_own; ++i)
        if (d->row_ptr[i + 1] < d->row_ptr[i]) {
            set_error("shard row_ptr not monotone at local row " + std::to_string(i) + " of " + std::to_string(d->n_own) + ": " +
                      std::to_string(d->row_ptr[i]) + " then " + std::to_string(d->row_ptr[i + 1]) + " (n_edges " + std::to_string(d->n_edges) + ")");
            return SBMBP_ERR_ARG;
        }
    segment_plan_t plan;
    segment_plan(d->row_ptr, d->n_own, uint32_t(frame_cap(Q)), uint32_t(frame_rcap(Q)), chunk_row, plan);
    e->chunk_blk = plan.chunk_blk;
    e->chunk_hub = plan.chunk_hub;
    CHK(ensure_partials(e, std::max<size_t>(plan.blk_row.size() - 1, 64) * (QMAX + 1)));
    CHK(setup_graph_tables(e, plan, d->row_ptr, d->nbr_local, d->rev_local, d->rev_local != nullptr, true));
    // records of Q-1 components; >= one record: the sweep's loads are branch-free. With a reverse index the records received
    // from the peers (the incoming messages of the cut edges) live behind the own ones, so rev addresses one array.
    CHK(dev_alloc(e, e->d_M[0], std::max<uint64_t>(e->E2 + e->n_halo_msgs, 1) * (Q - 1)));
    CHK(dev_alloc(e, e->d_M[1], std::max<uint64_t>(e->E2 + e->n_halo_msgs, 1) * (Q - 1)));
    CHK(dev_alloc(e, e->d_P, 1));
    e->hist_cap = 4096;
    CHK(dev_alloc(e, e->d_hist, e->hist_cap));
    if (dc == 2) CHK(dev_upload(e, e->d_deg, d->table_deg, size_t(d->n_own) + d->n_halo));
    if (e->n_halo_msgs) {  // defined content before the first exchange
        HIPCHK(hipMemsetAsync(e->d_M[0] + e->E2 * (Q - 1), 0, e->n_halo_msgs * (Q - 1) * 8, e->stream));
        HIPCHK(hipMemsetAsync(e->d_M[1] + e->E2 * (Q - 1), 0, e->n_halo_msgs * (Q - 1) * 8, e->stream));
    }
    CHK(ensure_small(e, 8192));
    CHK(dev_alloc(e, e->d_stage, size_t(FOLD_BLOCKS) * FOLD_STRIDE_MAX));
    HIPCHK(hipStreamSynchronize(e->stream));
    *out = owner.release();
    return SBMBP_OK;
}

int sbmbp_shard_set_labels(sbmbp_engine_t *e, const int32_t *conf, const uint32_t *true_conf, uint32_t flag, int conditional,
                           int any_clamp_global) {
    device_scope dev_(e);
    IS_SHARD(e);
    CHK(upload_labels(e, conf, true_conf, flag, conditional));
    // whether clamped rows exist is a property of the whole graph: every shard takes the same kernel variants
    e->has_clamp = any_clamp_global != 0;
    e->clamp_onehot = e->has_clamp && (flag == 1 || flag == 3);
    return SBMBP_OK;
}

int sbmbp_shard_query(sbmbp_engine_t *e, int what) {
    device_scope dev_(e);
    if (!e) return arg_error(__func__, __LINE__);
    switch (what) {
        case 0: return e->w_positive ? 1 : 0;
        case 1: return e->has_clamp ? 1 : 0;
        case 2: return e->clamp_onehot ? 1 : 0;
        case 3: return e->init_from_psi ? 1 : 0;
        case 4: return e->d_rev ? 1 : 0;
        default: return SBMBP_ERR_ARG;
    }
}

int sbmbp_shard_set_incoming(sbmbp_engine_t *e, int source) {
    device_scope dev_(e);
    IS_SHARD(e);
    if (source != 0 && !(source == 1 && e->d_rev)) return arg_error(__func__, __LINE__);
    e->incoming_src = source;
    return SBMBP_OK;
}

void *sbmbp_shard_msg_halo(sbmbp_engine_t *e, uint32_t j) {
    if (!e || !e->sharded) return nullptr;
    return e->d_M[(e->cur + int(j)) & 1] + e->E2 * (e->Q - 1);
}

int sbmbp_shard_pack_msgs(sbmbp_engine_t *e, uint32_t j, const uint32_t *d_edge_idx, uint32_t n, double *d_out) {
    device_scope dev_(e);
    IS_SHARD(e);
    if (n == 0) return SBMBP_OK;
    const int mc = int(e->Q) - 1;  // records are rows of Q-1 words: the generic row gather copies them verbatim
    const uint64_t tot = uint64_t(n) * mc;
    hipLaunchKernelGGL(k_pack_rows, dim3(uint32_t((tot + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, e->stream, e->d_M[(e->cur + int(j)) & 1],
                       d_edge_idx, n, mc, mc, d_out);
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

// message-gather form of sweep j on a shard (any damping, clamped rows, dc 2, zeros in cab): incoming messages of the cut
// edges are read from the records the caller received behind the own ones (sbmbp_shard_msg_halo of the same j)
int sbmbp_shard_sweep_explicit(sbmbp_engine_t *e, uint32_t j, double damping) {
    device_scope dev_(e);
    IS_SHARD(e);
    if (!e->d_rev) { set_error("shard was created without a reverse index"); return SBMBP_ERR_STATE; }
    const sweep_bufs s = bufs_of_sweep(e, j);
    CHK(ensure_partials(e, size_t(std::max<uint32_t>(e->n_blk, 1)) * (e->Q + 1)));
    hipEvent_t stop;
    CHK(timing_begin(e, e->stream, e->n_blk != 0, &stop));
    if (e->n_blk)
        DISPATCH_QB(e->Q, e->dc == 2,
                    hipLaunchKernelGGL((k_sweep<QQ, BB>), dim3(e->n_blk), dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr, e->d_rev, e->d_nbr, e->d_deg,
                                       s.Mold, s.Mnew, s.psi_old, s.psi_new, s.clamp, e->d_blk_row, e->d_blk_e0, e->d_P, int(e->dc != 0), damping, e->d_partials));
    CHK(timing_end(stop, e->stream));
    CHK(launch_hub_msg(e, e->stream, s.Mold, s.Mnew, s.psi_old, s.psi_new, s.clamp, damping, e->d_P, e->d_partials, e->d_prior));
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

int sbmbp_shard_state_record(sbmbp_engine_t *e, int slot) {
    device_scope dev_(e);
    IS_SHARD(e);
    if (slot < 0 || slot > 1) return arg_error(__func__, __LINE__);
    return record_conv_state(e, slot);
}
int sbmbp_shard_state_wait(sbmbp_engine_t *e, int slot, sbmbp_conv_state *out) {
    device_scope dev_(e);
    IS_SHARD(e);
    if (slot < 0 || slot > 1 || !out || !e->h_cs) return arg_error(__func__, __LINE__);
    conv_state cs;
    CHK(wait_conv_state(e, slot, &cs));
    out->maxdiff = cs.maxdiff;
    out->conv_iter = cs.conv_iter;
    out->sweep_idx = cs.sweep_idx;
    out->stop = cs.stop;
    out->last_exact = cs.last_exact;
    out->pause = cs.pause;
    out->ar_field_level = cs.ar_fl;
    out->ar_generic_level = cs.ar_gl;
    return SBMBP_OK;
}

int sbmbp_shard_resume(sbmbp_engine_t *e) {
    device_scope dev_(e);
    IS_SHARD(e);
    return resume_run(e);
}

int sbmbp_shard_begin(sbmbp_engine_t *e, double crit, int hinted) {
    device_scope dev_(e);
    IS_SHARD(e);
    if (!e->have_params || !e->have_state) { set_error("set_params and an initial state must precede shard sweeps"); return SBMBP_ERR_STATE; }
    if (hinted && !e->w_positive) { set_error("the marginal-gather sweep needs every cab entry > 0"); return SBMBP_ERR_UNSUPPORTED; }
    return upload_params(e, crit, hinted != 0);
}

int sbmbp_shard_read_buffer(sbmbp_engine_t *e, uint32_t j) { return (e && e->sharded) ? ((e->pcur + int(j)) & 1) : SBMBP_ERR_ARG; }

int sbmbp_shard_set_io(sbmbp_engine_t *e, const uint32_t *snd_ptr, const uint32_t *snd_slot, double *d_sendbuf,
                       const double *d_stage0, const double *d_stage1, uint32_t ncomp) {
    device_scope dev_(e);
    IS_SHARD(e);
    if (!snd_ptr || (ncomp != e->Q && ncomp + 1 != e->Q)) return arg_error(__func__, __LINE__);
    const uint32_t n_slots = snd_ptr[e->N];
    if ((n_slots && (!snd_slot || !d_sendbuf)) || (e->n_halo && (!d_stage0 || !d_stage1))) return arg_error(__func__, __LINE__);
    CHK(dev_upload(e, e->d_snd_ptr, snd_ptr, size_t(e->N) + 1));  // (tables of an earlier call are released, and leave device_bytes, here)
    CHK(dev_upload(e, e->d_snd_slot, snd_slot, size_t(n_slots)));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->io_sendbuf = d_sendbuf;
    e->io_stage[0] = d_stage0;
    e->io_stage[1] = d_stage1;
    e->io_ncomp = ncomp;
    return SBMBP_OK;
}

int sbmbp_shard_pack(sbmbp_engine_t *e, uint32_t j, const uint32_t *d_idx, uint32_t n, double *d_out, uint32_t ncomp) {
    device_scope dev_(e);
    IS_SHARD(e);
    if (ncomp != e->Q && ncomp + 1 != e->Q) return arg_error(__func__, __LINE__);
    if (n == 0) return SBMBP_OK;
    const double *table = e->d_psi[(e->pcur + int(j)) & 1];
    const uint64_t tot = uint64_t(n) * ncomp;
    hipLaunchKernelGGL(k_pack_rows, dim3(uint32_t((tot + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, e->stream, table, d_idx, n, int(e->Q),
                       int(ncomp), d_out);
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

int sbmbp_shard_unpack(sbmbp_engine_t *e, uint32_t j, const double *d_in, const uint32_t *d_halo_row, uint32_t n, uint32_t ncomp) {
    device_scope dev_(e);
    IS_SHARD(e);
    if ((ncomp != e->Q && ncomp + 1 != e->Q) || n > e->n_halo || (n && !d_halo_row)) return arg_error(__func__, __LINE__);
    if (n == 0) return SBMBP_OK;
    double *table = e->d_psi[(e->pcur + int(j)) & 1];
    hipLaunchKernelGGL(k_unpack_rows, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, e->stream, d_in, n, int(e->Q), int(ncomp), table,
                       e->N, d_halo_row);
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

int sbmbp_shard_field_partial(sbmbp_engine_t *e, uint32_t j) {
    device_scope dev_(e);
    IS_SHARD(e);
    const uint32_t rows_per_blk = 4096;
    const uint32_t nb = std::max<uint32_t>(1, (e->N + rows_per_blk - 1) / rows_per_blk);
    CHK(ensure_partials(e, size_t(nb) * (e->Q + 1)));
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_psi_sum<QQ>), dim3(nb), dim3(BLOCK), 0, e->stream, e->d_row_ptr,
                                        e->d_psi[(e->pcur + int(j)) & 1], e->N, rows_per_blk, int(e->dc != 0), e->d_partials));
    hipLaunchKernelGGL(k_fold_stage, dim3(1), dim3(BLOCK), 0, e->stream, e->d_partials, nb, nb, int(e->Q), 1, e->Q + 1, e->d_red);
    HIPCHK(hipGetLastError());  // k_psi_sum writes 0 into the max column, so red[Q] = 0
    return SBMBP_OK;
}

int sbmbp_shard_sweep_chunk(sbmbp_engine_t *e, uint32_t j, uint32_t c) { return sbmbp_shard_sweep_chunk_on(e, j, c, e ? e->stream : nullptr); }

int sbmbp_shard_sweep_chunk_on(sbmbp_engine_t *e, uint32_t j, uint32_t c, void *hip_stream) {
    device_scope dev_(e);
    IS_SHARD(e);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (c + 1 >= e->chunk_blk.size()) { set_error("chunk index out of range"); return SBMBP_ERR_ARG; }
    // s.Mnew is read and written in place; s.Mold is read only once the exact criterion is armed (dev_params::exact); the
    // chunk kernels take no clamp vector
    const sweep_bufs s = bufs_of_sweep(e, j);
    const int first = (j == 0 && e->init_from_psi) ? 1 : 0;
    shard_io io;
    std::memset(&io, 0, sizeof io);
    if (e->d_snd_ptr) {  // fused exchange buffers: gather the halo of table pc from its receive buffer, drop new marginals into the send slots
        io.snd_ptr = e->d_snd_ptr;
        io.snd_slot = e->d_snd_slot;
        io.sendbuf = e->io_sendbuf;
        io.halo_stage = e->io_stage[s.pc];
        io.n_own = e->N;
        io.ncomp = int(e->io_ncomp);
    }
    CHK(ensure_partials(e, size_t(std::max<uint32_t>(e->n_blk, 1)) * (e->Q + 1)));
    const uint32_t b0 = e->chunk_blk[c], nb = e->chunk_blk[c + 1] - b0;
    const uint32_t h0 = e->chunk_hub[c], nh = e->chunk_hub[c + 1] - h0;
    hipEvent_t stop;
    CHK(timing_begin(e, stream, nb != 0, &stop));  // per chunk, and only a chunk that has segments
    // XCD-aware numbering of the chunk launches too (1 chunk 0.371 -> 0.363 ms, 4 chunks 0.419 -> 0.412 ms per rank of the 8-rank C3 plan):
    // with the fused exchange buffers only
    static const int shard_xcd = std::getenv("SBMBP_SHARD_XCD") ? std::atoi(std::getenv("SBMBP_SHARD_XCD")) : SBMBP_XCD_REMAP;
    const int xcd = io.snd_ptr ? shard_xcd : 0;
    if (nb)
        DISPATCH_QB(e->Q, io.snd_ptr != nullptr,
                    hipLaunchKernelGGL((k_sweep_psi<QQ, false, BB>), dim3(xcd ? xcd_grid(nb) : nb), dim3(frame_cfg<QQ>::TPB), 0, stream, e->d_row_ptr, e->d_nbr,
                                       s.Mnew, s.psi_old, s.psi_new, e->d_blk_row + b0, e->d_blk_e0 + b0, e->d_P, int(e->dc),
                                       e->d_partials + size_t(b0) * (e->Q + 1), (const int32_t *)nullptr, io, nb, xcd, s.Mold, first));
    CHK(timing_end(stop, stream));
    CHK(launch_hub_psi(e, stream, h0, nh, s.Mnew, s.psi_old, s.psi_new, (const int32_t *)nullptr, io, s.Mold, first));
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

// ONE launch: the block partials of all chunks -> SBMBP_FOLD_ROWS rows in red (workgroups without rows write zeros, neutral
// for the sums and for the maximum of non-negative differences). The caller all-gathers these rows of every rank and
// k_finalize folds the lot: no second fold stage per rank.
int sbmbp_shard_sweep_fold(sbmbp_engine_t *e) {
    device_scope dev_(e);
    IS_SHARD(e);
    const uint32_t rows = e->n_blk;
    const uint32_t chunk = std::max<uint32_t>(1, (rows + SBMBP_FOLD_ROWS - 1) / SBMBP_FOLD_ROWS);
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_fold_records<QQ>), dim3(SBMBP_FOLD_ROWS), dim3(BLOCK), 0, e->stream, e->d_partials, rows, chunk, e->d_red));
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

int sbmbp_shard_sweep_partial(sbmbp_engine_t *e, uint32_t j) {
    device_scope dev_(e);
    IS_SHARD(e);
    for (uint32_t c = 0; c + 1 < e->chunk_blk.size(); ++c) CHK(sbmbp_shard_sweep_chunk(e, j, c));
    return sbmbp_shard_sweep_fold(e);
}

int sbmbp_shard_finalize(sbmbp_engine_t *e, int mode, uint32_t n_rows, int md_exact) {
    device_scope dev_(e);
    IS_SHARD(e);
    if ((mode != 0 && mode != 1) || n_rows == 0 || n_rows > 64u * SBMBP_FOLD_ROWS) return arg_error(__func__, __LINE__);
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_finalize<QQ>), dim3(1), dim3(BLOCK), 0, e->stream, e->d_red + SBMBP_RED_GATHER_OFFSET, n_rows, mode, e->d_P, e->d_hist, e->hist_cap, md_exact));
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

int sbmbp_shard_msgdiff_partial(sbmbp_engine_t *e) {
    device_scope dev_(e);
    IS_SHARD(e);
    const uint64_t n = e->E2;  // message records
    if (n == 0) { HIPCHK(hipMemsetAsync(e->d_red, 0, 8, e->stream)); return SBMBP_OK; }
    const uint32_t nb = uint32_t(std::min<uint64_t>(2048, (n + BLOCK - 1) / BLOCK));
    CHK(ensure_partials(e, size_t(nb) * 2));
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_msg_diff<QQ>), dim3(nb), dim3(BLOCK), 0, e->stream, e->d_M[0], e->d_M[1], n, e->d_partials));
    hipLaunchKernelGGL(k_fold_stage, dim3(1), dim3(BLOCK), 0, e->stream, e->d_partials, nb, nb, 1, 1, 2u, e->d_stage);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(e->d_red, e->d_stage + 1, 8, hipMemcpyDeviceToDevice, e->stream));
    return SBMBP_OK;
}

int sbmbp_shard_rowsums_partial(sbmbp_engine_t *e) {
    device_scope dev_(e);
    IS_SHARD(e);
    const uint32_t Q = e->Q, T = 2 * Q + Q * Q;
    const uint32_t rows_per_blk = 512;  // one thread per output entry loops over staged rows: keep chunks small, workgroups many
    const uint32_t nb = std::max<uint32_t>(1, (e->N + rows_per_blk - 1) / rows_per_blk);
    CHK(ensure_partials(e, size_t(nb) * T));
    DISPATCH_Q(Q, hipLaunchKernelGGL((k_row_sums<QQ>), dim3(nb), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->d_psi[e->pcur],
                                     e->d_true, e->N, rows_per_blk, e->d_partials));
    HIPCHK(hipGetLastError());
    return fold_matrix_to_device(e, nb, T, e->d_red);
}

int sbmbp_shard_poll(sbmbp_engine_t *e, sbmbp_conv_state *out) {
    device_scope dev_(e);
    IS_SHARD(e);
    if (!out) return arg_error(__func__, __LINE__);
    conv_state cs;
    CHK(read_conv_state(e, &cs));
    if (e->timing) CHK(collect_timing(e));
    out->maxdiff = cs.maxdiff;
    out->conv_iter = cs.conv_iter;
    out->sweep_idx = cs.sweep_idx;
    out->stop = cs.stop;
    out->last_exact = cs.last_exact;
    out->pause = cs.pause;
    out->ar_field_level = cs.ar_fl;
    out->ar_generic_level = cs.ar_gl;
    e->ar_fl = cs.ar_fl;
    e->ar_gl = cs.ar_gl;
    return SBMBP_OK;
}

int sbmbp_shard_commit(sbmbp_engine_t *e, uint32_t executed) {
    device_scope dev_(e);
    IS_SHARD(e);
    e->cur = (e->cur + int(executed)) & 1;
    e->pcur = (e->pcur + int(executed)) & 1;
    e->sweeps += executed;
    e->psi_sweeps += executed;
    if (executed) e->init_from_psi = false;
    return SBMBP_OK;
}

}  // extern "C"

// ---- reductions on shards: partial -> (caller all-reduces red) -> finish ----------------------------
static int shard_materialize(sbmbp_engine_t *e) {
    if (e->incoming_src == 1) return SBMBP_OK;  // the reductions gather the incoming messages through rev (halo records in place)
    if (!e->d_Min) CHK(dev_alloc(e, e->d_Min, e->E2 * (e->Q - 1)));
    if (e->E2 == 0) return SBMBP_OK;
    const uint32_t nb = uint32_t(std::min<uint64_t>(4096, (e->E2 + BLOCK - 1) / BLOCK));
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_materialize_in<QQ>), dim3(nb), dim3(BLOCK), 0, e->stream, e->d_nbr, e->d_M[e->cur ^ 1],
                                        e->d_psi[e->pcur], uint32_t(e->E2), e->d_P, e->d_Min));
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

extern "C" {

// red[0..4) = {sum log Z_i, sum log norm_L, e_site sum, e_edge sum} over owned rows/edges; red[4] = sum 2 d log d
int sbmbp_shard_fe_partial(sbmbp_engine_t *e, int want_entropy) {
    device_scope dev_(e);
    IS_SHARD(e);
    CHK(shard_materialize(e));
    double dummy[4];
    CHK(site_edge_terms(e, want_entropy != 0, dummy, e->d_red));
    const double c = e->dc == 1 ? e->sum_log_didl : 0.0;
    HIPCHK(hipMemcpyAsync(e->d_red + 4, &c, 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));  // c is a stack object
    return SBMBP_OK;
}

// out = {f_site, f_edge, e_site, e_edge} from the all-reduced red[0..5)
int sbmbp_shard_fe_finish(sbmbp_engine_t *e, double *out) {
    device_scope dev_(e);
    IS_SHARD(e);
    double r[5];
    CHK(read_doubles(e, e->d_red, 5, r));
    site_edge_parts(e->Nglob, e->dc == 1 ? r + 4 : nullptr, r, out);
    return SBMBP_OK;
}

// moment tensors of the owned rows (orders 1..K packed) at red[0..T), adjacent-pair sums at red[T], red[T+1];
// returns the number of doubles to all-reduce (T + 2) in *n_values and the order used in *order
int sbmbp_shard_nonedge_partial(sbmbp_engine_t *e, int want_entropy, uint32_t *n_values, int *order) {
    device_scope dev_(e);
    IS_SHARD(e);
    if (!n_values || !order) return arg_error(__func__, __LINE__);
    const uint32_t Q = e->Q;
    if (e->dc != 0) { *n_values = 0; *order = 0; return SBMBP_OK; }
    std::vector<double> mats;
    double wmax;
    CHK(upload_nonedge_mats(e, mats, &wmax));
    const int K = series_order(Q, e->Nglob, e->series_order, wmax);
    const uint32_t T = series_len(Q, K);
    if (T + 2 > 8192) { set_error("moment tensors do not fit the reduction buffer"); return SBMBP_ERR_UNSUPPORTED; }
    CHK(moments_to_device(e, K, T, e->d_red));
    CHK(adjacent_pairs_to_device(e, false, want_entropy != 0, e->d_red + T));
    *n_values = T + 2;
    *order = K;
    return SBMBP_OK;
}

// Exact non-edge term on shards (small graphs, where the moment series is not accurate enough): d_psi_all = the marginals
// of ALL vertices in global row order (the caller all-reduces the shards' own rows into it). Leaves in red[0..4)
// {all-pairs f, all-pairs e, adjacent f, adjacent e} over (own i, every l); after a SUM all-reduce of the 4 values
// f_nonedge = (red[0] - red[2]) / 2N, e_nonedge = (red[1] - red[3]) / 2N   (bp.cpp:675-741).
int sbmbp_shard_nonedge_exact_partial(sbmbp_engine_t *e, const double *d_psi_all, int want_entropy) {
    device_scope dev_(e);
    IS_SHARD(e);
    if (!d_psi_all) return arg_error(__func__, __LINE__);
    const uint32_t Q = e->Q;
    if (e->dc != 0) { HIPCHK(hipMemsetAsync(e->d_red, 0, 4 * 8, e->stream)); return SBMBP_OK; }
    std::vector<double> mats;
    CHK(upload_nonedge_mats(e, mats, nullptr));
    const double *d_Pm = e->d_mats + Q * Q, *d_cab = e->d_mats + 2 * Q * Q;
    const double invN = 1.0 / double(e->Nglob);
    const uint32_t gi = (e->N + BLOCK - 1) / BLOCK, gl = (e->Nglob + BLOCK - 1) / BLOCK;
    CHK(ensure_partials(e, size_t(gi) * gl * (NE_NP + 1)));
    DISPATCH_Q(Q, hipLaunchKernelGGL((k_nonedge_exact<QQ>), dim3(gi, gl), dim3(BLOCK), 0, e->stream, e->d_psi[e->pcur], e->N, d_psi_all,
                                     e->Nglob, d_Pm, d_cab, invN, want_entropy, e->d_partials));
    HIPCHK(hipGetLastError());
    CHK(fold_to_device(e, gi * gl, NE_NP, NE_NP + 1, e->d_red));
    return adjacent_pairs_to_device(e, true, want_entropy != 0, e->d_red + 2);
}

// out = {f_nonedge, e_nonedge} from the all-reduced moments and adjacent sums
int sbmbp_shard_nonedge_finish(sbmbp_engine_t *e, int want_entropy, int order, double *out) {
    device_scope dev_(e);
    IS_SHARD(e);
    out[0] = out[1] = 0.0;
    if (e->dc != 0 || order <= 0) return SBMBP_OK;
    const uint32_t Q = e->Q, T = series_len(Q, order);
    std::vector<double> r(T + 2), mats(3 * Q * Q);
    CHK(read_doubles(e, e->d_red, r.size(), r.data()));
    nonedge_mats(Q, e->Nglob, e->cab.data(), e->beta, mats.data(), nullptr);
    double all[2];
    nonedge_series(Q, e->Nglob, order, want_entropy != 0, r.data(), mats.data(), all);
    nonedge_finish(all, r.data() + T, e->Nglob, out);
    return SBMBP_OK;
}

// red[0..2Q+Q*Q) row sums (na, nna, confusion), then the Q(Q+1)/2 EM numerators; *n_values doubles to all-reduce
int sbmbp_shard_em_partial(sbmbp_engine_t *e, uint32_t *n_values) {
    device_scope dev_(e);
    IS_SHARD(e);
    if (!n_values) return arg_error(__func__, __LINE__);
    const uint32_t Q = e->Q, R = 2 * Q + Q * Q, T = Q * (Q + 1) / 2;
    CHK(shard_materialize(e));
    CHK(sbmbp_shard_rowsums_partial(e));
    const uint32_t nb = uint32_t(std::min<uint64_t>(2048, std::max<uint64_t>(1, (e->E2 + BLOCK - 1) / BLOCK)));
    CHK(ensure_partials(e, size_t(nb) * (T + 1)));
    const double *Min = e->incoming_src == 0 ? e->d_Min.get() : nullptr;
    DISPATCH_QB(Q, e->dc == 2, hipLaunchKernelGGL((k_em_edges<QQ, BB>), dim3(nb), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->d_rev, e->d_nbr, e->d_deg,
                                                  e->d_src, e->d_M[e->cur], Min, uint32_t(e->E2), e->d_P, e->d_partials));
    HIPCHK(hipGetLastError());
    CHK(fold_to_device(e, nb, T, T + 1, e->d_red + R));
    *n_values = R + T;
    return SBMBP_OK;
}

int sbmbp_shard_em_finish(sbmbp_engine_t *e, double *na_e, double *nna_e, double *cab_e) {
    device_scope dev_(e);
    IS_SHARD(e);
    const uint32_t Q = e->Q, R = 2 * Q + Q * Q, T = Q * (Q + 1) / 2;
    std::vector<double> r(R + T);
    CHK(read_doubles(e, e->d_red, r.size(), r.data()));
    const double *na = r.data(), *nna = r.data() + Q, *tri = r.data() + R;
    std::vector<double> ce(Q * Q, 0.0);
    em_rescale(Q, e->Nglob, e->dc, na, nna, tri, ce.data());
    if (na_e) std::copy(na, na + Q, na_e);
    if (nna_e) std::copy(nna, nna + Q, nna_e);
    if (cab_e) std::copy(ce.begin(), ce.end(), cab_e);
    return SBMBP_OK;
}

}  // extern "C"

// =========================================== replica batches ===========================================
// R independent BP states over one graph (sbmbp.h: sbmbp_batch_*; kernels_batch.h). The batch owns ONE engine: the graph
// tables, the label vectors, the scratch of the reductions and the stream are that engine's. The engine's own message /
// marginal / parameter buffers are replaced by the replica-major batch buffers, and for everything that is not the sweep
// (initial state, state access, field, free energy, entropy, overlap, EM expectations) the engine is bound to replica r:
// its state pointers then point into the batch buffers and its host mirrors hold replica r's parameters, so the existing
// host code and reduction kernels run on replica r as they are.
struct batch_replica {
    std::vector<double> cab, eta;
    std::vector<uint32_t> na;
    double beta = 1.0;
    bool have_params = false, have_state = false, field_fresh = false, w_positive = false;
    int par = 0;                // which of the two buffers holds the current state
    int ar_fl = 0, ar_gl = -1;  // levels the last converge call ended on
    int prior_state = 0;        // per-vertex prior (sbmbp_batch_set_vertex_prior): 0 = none, 1 = the batch's shared table, 2 = own
    device_buffer<double> d_prior;  // the own table [N*Q] (state 2)
    bool cs_last = false;       // the replica's last sweeps ran in the coloured order (sbmbp_engine::cs_last, per replica)
};
// The batch's engine and events, as a base of the batch: the buffers are members of sbmbp_batch and are counted in the engine's
// device_bytes, so they are released after ~sbmbp_batch has drained the stream and before the engine goes here.
struct batch_engine {
    sbmbp_engine *e = nullptr;
    hipEvent_t ev_cs[2] = {nullptr, nullptr};
    ~batch_engine() {
        for (auto ev : ev_cs) if (ev) (void)hipEventDestroy(ev);
        sbmbp_destroy(e);
    }
};
struct sbmbp_batch : batch_engine {
    uint32_t R = 0;
    device_buffer<double> d_M, d_psi, d_rec;
    device_buffer<dev_params> d_P;
    device_buffer<int> d_par;
    device_buffer<uint32_t> d_cs;  // [R] convergence states, gathered (k_batch_conv_states)
    size_t msg_stride = 0, psi_stride = 0, rec_stride = 0;  // doubles per replica
    std::vector<batch_replica> rep;
    std::vector<int> call_par;  // parities at the start of the running call
    pinned_buffer<conv_state> h_cs;  // two slots of R convergence states (with ev_cs)
    uint64_t sweeps = 0;
    // batched reductions of an EM step (batch_reductions): inputs [R][3 Q Q] matrices, then parities / mask / refresh mask
    // as ints; partial tables; one result row per replica. The partial and result tables grow on demand.
    device_buffer<double> d_em_in, d_em_part[3], d_em_res;
    pinned_buffer<char> h_em_in;
    pinned_buffer<double> h_em_res;
    // per-vertex priors: the ONE table of the shared replicas, the table of ones that replicas without a table read while
    // another replica holds one (allocated on first need), and per replica the table it reads (device, [R]; what
    // k_sweep_batch_prior and k_em_frame_batch_prior index with blockIdx.y). n_prior = replicas that hold a table: while it is
    // 0 the batch launches what it launches without this feature.
    device_buffer<double> d_prior_shared, d_prior_ones;
    device_buffer<const double *> d_prior_tab;
    uint32_t n_prior = 0;
    // agreement of replicas (sbmbp_batch_agreement), all allocated on first need: the slots of the listed replicas, the
    // partial tables of k_agree (grown like the EM partials), the folded n n Q Q results, and the page-locked host side
    // (AG_MAXN slots, then the results). Not counted in device_bytes: the call leaves every statistic alone
    device_buffer<uint32_t> d_ag_slot;
    device_buffer<double> d_ag_part, d_ag_res;
    pinned_buffer<char> h_ag;
    ~sbmbp_batch() {
        if (!e) return;
        (void)hipSetDevice(e->device);
        if (e->stream) (void)hipStreamSynchronize(e->stream);
    }
};

namespace {

// the prior table replica r reads: null while no replica of the batch holds one; else the shared table, its own, or the ones
const double *batch_prior_of(const sbmbp_batch *b, uint32_t r) {
    if (!b->n_prior) return nullptr;
    const batch_replica &p = b->rep[r];
    return p.prior_state == 2 ? p.d_prior.get() : (p.prior_state == 1 ? b->d_prior_shared.get() : b->d_prior_ones.get());
}

// binds the batch's engine to replica r for the lifetime of the object
struct bound_replica {
    sbmbp_batch *b;
    uint32_t r;
    bound_replica(sbmbp_batch *b_, uint32_t r_) : b(b_), r(r_) {
        sbmbp_engine *e = b->e;
        batch_replica &p = b->rep[r];
        for (int k = 0; k < 2; ++k) {
            e->d_M[k].borrow(b->d_M + (size_t(k) * b->R + r) * b->msg_stride);
            e->d_psi[k].borrow(b->d_psi + (size_t(k) * b->R + r) * b->psi_stride);
        }
        e->d_P.borrow(b->d_P + r);
        e->d_prior.borrow(const_cast<double *>(batch_prior_of(b, r)));  // the reductions and hub launches of the bound engine take the prior kernels
        e->cur = e->pcur = p.par;
        e->cab = p.cab; e->eta = p.eta; e->na = p.na; e->beta = p.beta;
        e->have_params = p.have_params; e->have_state = p.have_state; e->field_fresh = p.field_fresh; e->w_positive = p.w_positive;
        e->ar_fl = p.ar_fl; e->ar_gl = p.ar_gl;
        e->cs_last = p.cs_last;
        e->psi_consistent = false; e->init_from_psi = false; e->fz.valid = false;  // message-gather form only
    }
    ~bound_replica() {
        sbmbp_engine *e = b->e;
        batch_replica &p = b->rep[r];
        p.cab = e->cab; p.eta = e->eta; p.na = e->na; p.beta = e->beta;
        p.have_params = e->have_params; p.have_state = e->have_state; p.field_fresh = e->field_fresh; p.w_positive = e->w_positive;
        p.par = e->cur;
        for (int k = 0; k < 2; ++k) { e->d_M[k].reset(); e->d_psi[k].reset(); }  // unbound: the engine holds no state, and no prior
        e->d_P.reset();
        e->d_prior.reset();
        e->cs_last = false;
        e->have_state = e->have_params = false;
    }
};

batch_view view_of(const sbmbp_batch *b) {
    return batch_view{b->d_M, b->d_psi, b->d_P, b->d_rec, b->d_par, b->msg_stride, b->psi_stride, b->rec_stride, b->R};
}

int batch_replica_arg(const sbmbp_batch *b, int64_t replica) {
    if (replica < 0 || replica >= int64_t(b->R)) {
        set_error("replica index " + std::to_string(replica) + " outside the batch of " + std::to_string(b->R));
        return SBMBP_ERR_ARG;
    }
    return SBMBP_OK;
}

// sweep j of the running call for all replicas: hub rows per replica (the single engine's fragment pair on offset
// pointers), ONE frame launch, ONE fold + update launch
int batch_launch_sweep(sbmbp_batch *b, const batch_view &bv, uint32_t j, double damp) {
    sbmbp_engine *e = b->e;
    const int32_t *clamp = e->has_clamp ? e->d_clamp.get() : nullptr;
    if (e->n_hub) {
        for (uint32_t r = 0; r < b->R; ++r) {
            const int mc = (b->call_par[r] + int(j)) & 1;
            CHK(launch_hub_msg(e, e->stream, b->d_M + (size_t(mc) * b->R + r) * b->msg_stride, b->d_M + (size_t(mc ^ 1) * b->R + r) * b->msg_stride,
                               b->d_psi + (size_t(mc) * b->R + r) * b->psi_stride, b->d_psi + (size_t(mc ^ 1) * b->R + r) * b->psi_stride, clamp, damp,
                               b->d_P + r, b->d_rec + size_t(r) * b->rec_stride, batch_prior_of(b, r)));
        }
    }
    const dim3 grid(e->n_blk, b->R);
    if (b->n_prior) {  // a replica holds a per-vertex prior: the prior twin, every replica over the table d_prior_tab names for it
        DISPATCH_QB(e->Q, e->dc == 2, hipLaunchKernelGGL((k_sweep_batch_prior<QQ, BB>), grid, dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr, e->d_rev,
                                                         e->d_nbr, e->d_deg, clamp, e->d_blk_row, e->d_blk_e0, bv.M, bv.psi, bv.P, bv.rec, bv.par, bv.msg_stride,
                                                         bv.psi_stride, bv.rec_stride, j, int(e->dc != 0), damp, b->d_prior_tab));
    } else {
        DISPATCH_QB(e->Q, e->dc == 2, hipLaunchKernelGGL((k_sweep_batch<QQ, BB>), grid, dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr, e->d_rev, e->d_nbr,
                                                         e->d_deg, clamp, e->d_blk_row, e->d_blk_e0, bv.M, bv.psi, bv.P, bv.rec, bv.par, bv.msg_stride, bv.psi_stride,
                                                         bv.rec_stride, bv.R, j, int(e->dc != 0), damp));
    }
    DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_finalize_batch<QQ>), dim3(b->R), dim3(BLOCK), 0, e->stream, bv.P, bv.rec, bv.rec_stride, e->n_blk));
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

// One sweep of the coloured order for all replicas (launch_coloured_sweep with the replica as the grid's second dimension):
// per step the hub pair of every replica (the single engine's kernels on offset pointers, over the step-ordered fragment
// tables; the fragment scratch is shared, and the launches of one replica follow each other in the one stream), ONE
// k_sweep_step_batch and ONE k_step_finalize_batch, all in place on the buffer call_par[r] of every replica.
int batch_launch_coloured_sweep(sbmbp_batch *b, const batch_view &bv, double damp) {
    sbmbp_engine *e = b->e;
    const int32_t *clamp = e->has_clamp ? e->d_clamp.get() : nullptr;
    const hub_frags hf{e->cs.frag_hub, e->cs.hub_frag0, e->d_hub_b, e->d_hub_pA, e->d_hub_pE};
    for (uint32_t s = 0; s < e->cs_steps; ++s) {
        const uint32_t seg0 = e->cs_seg0[s], nseg = e->cs_seg0[s + 1] - seg0, nh = e->cs_hub0[s + 1] - e->cs_hub0[s];
        if (nh) {
            const uint32_t f0 = e->cs_frag0[s], nf = e->cs_frag0[s + 1] - f0;
            for (uint32_t r = 0; r < b->R; ++r) {
                double *M = bv.M + (size_t(b->call_par[r]) * b->R + r) * bv.msg_stride, *psi = bv.psi + (size_t(b->call_par[r]) * b->R + r) * bv.psi_stride;
                double *rec = bv.rec + size_t(r) * bv.rec_stride;
                DISPATCH_QB(e->Q, e->dc == 2, hipLaunchKernelGGL((k_hub_frag_product_msg<QQ, BB>), dim3(nf), dim3(BLOCK), 0, e->stream, e->d_row_ptr, e->d_rev,
                                                                 e->d_nbr, e->d_deg, M, e->cs.hub_row, e->cs.hub_rec, hf, f0, bv.P + r, rec, clamp));
                DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_hub_step_cavity<QQ>), dim3(nf), dim3(BLOCK), 0, e->stream, e->d_row_ptr, M, psi, e->cs.hub_row,
                                                    e->cs.hub_rec, hf, f0, bv.P + r, int(e->dc != 0), damp, rec, clamp));
            }
        }
        if (nseg)
            DISPATCH_QB(e->Q, e->dc == 2, hipLaunchKernelGGL((k_sweep_step_batch<QQ, BB>), dim3(nseg, b->R), dim3(frame_cfg<QQ>::TPB), 0, e->stream, e->d_row_ptr,
                                                             e->d_rev, e->d_nbr, e->d_deg, bv.M, bv.psi, clamp, e->cs.rows, e->cs.loff, e->cs.seg_row0, seg0,
                                                             bv.P, bv.par, bv.msg_stride, bv.psi_stride, bv.rec_stride, int(e->dc != 0), damp, bv.rec));
        DISPATCH_Q(e->Q, hipLaunchKernelGGL((k_step_finalize_batch<QQ>), dim3(b->R), dim3(BLOCK), 0, e->stream, bv.P, bv.rec, bv.rec_stride, nseg + nh,
                                            int(s + 1 == e->cs_steps)));
    }
    HIPCHK(hipGetLastError());
    return SBMBP_OK;
}

int batch_check_ready(const sbmbp_batch *b, const char *what) {
    for (uint32_t r = 0; r < b->R; ++r)
        if (!b->rep[r].have_params || !b->rep[r].have_state) {
            set_error(std::string("set_params and init_messages/set_state must precede ") + what + " (replica " + std::to_string(r) + ")");
            return SBMBP_ERR_STATE;
        }
    return SBMBP_OK;
}
// run_sweeps for the batch: every replica starts from its current state, stops at its own sweep (device side, P[r].stop)
// and keeps the state of that sweep; the call ends when all have stopped or after max_sweeps
// crit[r] is replica r's criterion. active (null = all): a replica that is not active is frozen: its parameter block is not
// uploaded again, its stop flag is set, and its state and parity stay untouched; executed[r] (may be null) = sweeps replica
// r executed in this call.
// In the coloured order (sbmbp_batch_set_sweep_order) the sweeps of the call are batch_launch_coloured_sweep's: in place, so
// no replica's parity moves, and without relaxation of any kind (step_update), as run_sweeps_coloured on the single engine.
int batch_run(sbmbp_batch *b, const double *crit, const uint8_t *active, uint32_t max_sweeps, double damping, int *niter, double *last,
              uint32_t *executed_out = nullptr) {
    sbmbp_engine *e = b->e;
    const uint32_t R = b->R;
    CHK(batch_check_ready(b, "converge"));
    CHK(ensure_partials(e, size_t(std::max<uint32_t>(e->n_blk, 1)) * (e->Q + 1)));
    const bool coloured = e->sweep_order == 1;
    b->call_par.resize(R);
    for (uint32_t r = 0; r < R; ++r) {  // parameter block and initial field of every replica (once per call: a loop)
        b->call_par[r] = b->rep[r].par;
        if (active && !active[r]) {
            static const int one = 1;
            HIPCHK(hipMemcpyAsync(reinterpret_cast<char *>(b->d_P + r) + offsetof(dev_params, stop), &one, sizeof(int), hipMemcpyHostToDevice, e->stream));
            continue;
        }
        bound_replica v(b, r);
        CHK(upload_params(e, crit[r], false));
        CHK(launch_field(e, 1));
    }
    HIPCHK(hipMemcpyAsync(b->d_par, b->call_par.data(), size_t(R) * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const batch_view bv = view_of(b);
    conv_state *slots = b->h_cs;
    std::vector<conv_state> cs(R, conv_state{0.0, -1, 0, 0, 0, 0, 0, 1, 0, 0, -1});
    uint32_t done = 0;
    const uint32_t batch_max = std::max<uint32_t>(1, e->check_every);
    // batches are queued one ahead, as in run_sweeps: the GPU never idles while the host reads the states
    auto queue_batch = [&](int slot) -> int {
        const uint32_t n = std::min(batch_max, max_sweeps - done);
        for (uint32_t k = 0; k < n; ++k) CHK(coloured ? batch_launch_coloured_sweep(b, bv, damping) : batch_launch_sweep(b, bv, done + k, damping));
        done += n;
        constexpr uint32_t words = sizeof(conv_state) / 4;
        hipLaunchKernelGGL(k_batch_conv_states, dim3(std::min<uint32_t>(64, (R * words + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, e->stream, b->d_P, R,
                           uint32_t(offsetof(dev_params, maxdiff)), words, b->d_cs);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(slots + size_t(slot) * R, b->d_cs, size_t(R) * sizeof(conv_state), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipEventRecord(b->ev_cs[slot], e->stream));
        return SBMBP_OK;
    };
    auto wait_batch = [&](int slot, bool *stopped) -> int {  // stopped = every replica has
        HIPCHK(hipEventSynchronize(b->ev_cs[slot]));
        std::copy(slots + size_t(slot) * R, slots + size_t(slot + 1) * R, cs.begin());
        *stopped = std::all_of(cs.begin(), cs.end(), [](const conv_state &s) { return s.stop != 0; });
        return SBMBP_OK;
    };
    CHK(queue_ahead(max_sweeps, done, queue_batch, wait_batch));
    for (uint32_t r = 0; r < R; ++r) {
        if (executed_out) executed_out[r] = 0;
        if (active && !active[r]) continue;  // frozen: P[r] still holds the records of its last run
        batch_replica &p = b->rep[r];
        const uint32_t executed = uint32_t(cs[r].sweep_idx);
        if (executed_out) executed_out[r] = executed;
        b->sweeps += executed;
        p.cs_last = coloured;
        if (coloured) {  // in place: the parity stays; the field followed the marginals step by step (run_sweeps_coloured)
            p.field_fresh = true;
            p.ar_fl = 0;
            p.ar_gl = -1;
        } else {
            p.par = (p.par + int(executed)) & 1;
            const bool relaxed = cs[r].ar_fl > 0 || cs[r].ar_gl >= 0;
            p.field_fresh = (e->field_mix >= 1.0) && !relaxed && executed > 0;
            p.ar_fl = cs[r].ar_fl;
            p.ar_gl = cs[r].ar_gl;
        }
        if (niter) niter[r] = cs[r].conv_iter;
        if (last) last[r] = cs[r].maxdiff;  // message-gather sweeps report the 1-step difference
    }
    return SBMBP_OK;
}

// The reductions of ONE EM step for every replica of the mask (null = all), from one launch sequence and one copy to the
// host (kernels_batch.h): field refresh where the field is stale, frame pass (+ k_fe_hub per replica where the graph has
// hub rows), the numerators' own kernel above EM_FRAME_QMAX labels, all-pairs non-edge term under dc 0 (exact or moment
// series, as sbmbp_batch_set_nonedge_mode says), folds, ONE device-to-host copy, ONE synchronisation. The O(Q^2) host work
// per replica (matrices of the non-edge term, contraction of the series, rescaling) stays a host loop.
// Outputs (any may be null): na_e / nna_e [R][Q], cab_e [R][Q*Q], f [R], parts [R][3]. Rows of replicas outside the mask are
// left untouched.
int batch_reductions(sbmbp_batch *b, const uint8_t *mask, double *na_e, double *nna_e, double *cab_e, double *f, double *parts) {
    sbmbp_engine *e = b->e;
    const uint32_t R = b->R, Q = e->Q, N = e->N, QQ2 = Q * Q, T = Q * (Q + 1) / 2;
    const uint32_t NP = uint32_t(em_np(int(Q)));
    const bool em_in_frame = Q <= uint32_t(EM_FRAME_QMAX);
    const bool nonedge = e->dc == 0, exact = nonedge && nonedge_exact(e);
    const int adj_mode = nonedge ? (exact ? 2 : 1) : 0;

    // ---- host: per-replica matrices, series order, masks -> one upload
    const size_t in_doubles = size_t(R) * 3 * QQ2, in_bytes = in_doubles * 8 + size_t(3) * R * sizeof(int);
    if (!b->h_em_in) {
        CHK(b->h_em_in.alloc(in_bytes));
        CHK(dev_alloc(e, b->d_em_in, in_bytes / 8 + 1));
    }
    double *h_mats = reinterpret_cast<double *>(b->h_em_in.get());
    int *h_par = reinterpret_cast<int *>(h_mats + in_doubles), *h_act = h_par + R, *h_ref = h_act + R;
    const double *d_mats = b->d_em_in;
    const int *d_par = reinterpret_cast<const int *>(b->d_em_in + in_doubles), *d_act = d_par + R, *d_ref = d_act + R;
    std::vector<int> Kr(R, 0);
    int K = 0;
    bool any_refresh = false, any = false;
    for (uint32_t r = 0; r < R; ++r) {
        const batch_replica &p = b->rep[r];
        const bool on = !mask || mask[r];
        h_par[r] = p.par;
        h_act[r] = on ? 1 : 0;
        h_ref[r] = (on && !p.field_fresh) ? 1 : 0;
        any = any || on;
        any_refresh = any_refresh || h_ref[r];
        double *wmat = h_mats + size_t(r) * 3 * QQ2, wmax = 0.0;
        if (on) nonedge_mats(Q, N, p.cab.data(), p.beta, wmat, &wmax);
        else for (uint32_t a = 0; a < 3 * QQ2; ++a) wmat[a] = a < QQ2 ? double(N) : 0.0;  // the matrices of P = cab = 0: never read, but uploaded
        if (on && nonedge && !exact) { Kr[r] = series_order(Q, N, e->series_order, wmax); K = std::max(K, Kr[r]); }
    }
    if (!any) return SBMBP_OK;
    const uint32_t Tm = series_len(Q, K);
    const uint32_t n_all = nonedge ? (exact ? 1u : Tm) : 0u, RES = NP + n_all;

    // ---- buffers
    const uint32_t nbf = std::max<uint32_t>(1, (N + 4095) / 4096), rows = e->n_blk + e->n_hub;
    const uint32_t nbe = uint32_t(std::min<uint64_t>(1024, std::max<uint64_t>(1, (e->E2 + BLOCK - 1) / BLOCK)));
    const uint32_t g = (N + BLOCK - 1) / BLOCK, nbm = std::max<uint32_t>(1, (N + 511) / 512);
    const size_t part0 = size_t(R) * std::max<size_t>(size_t(rows) * NP, size_t(nbf) * (Q + 1));  // field partials are folded before the frame pass writes
    const size_t part1 = em_in_frame ? 0 : size_t(R) * nbe * T;
    const size_t part2 = !nonedge ? 0 : (exact ? size_t(R) * g * g : size_t(R) * nbm * Tm);
    const size_t part[3] = {part0, part1, part2};
    for (int k = 0; k < 3; ++k) CHK(b->d_em_part[k].ensure(part[k], &e->device_bytes));
    CHK(b->d_em_res.ensure(size_t(R) * RES, &e->device_bytes));
    CHK(b->h_em_res.ensure(size_t(R) * RES));

    // ---- device: one launch sequence for all replicas
    hipStream_t st = e->stream;
    HIPCHK(hipMemcpyAsync(b->d_em_in, b->h_em_in.get(), in_bytes, hipMemcpyHostToDevice, st));
    if (any_refresh) {  // the site terms read h of the current marginals (k_psi_sum + k_finalize mode 2)
        DISPATCH_Q(Q, hipLaunchKernelGGL((k_psi_sum_batch<QQ>), dim3(nbf, R), dim3(BLOCK), 0, st, e->d_row_ptr, b->d_psi, d_par, d_ref, b->psi_stride,
                                         R, N, 4096u, int(e->dc != 0), b->d_em_part[0]));
        DISPATCH_Q(Q, hipLaunchKernelGGL((k_field_refresh_batch<QQ>), dim3(R), dim3(BLOCK), 0, st, b->d_P, d_ref, b->d_em_part[0], nbf));
    }
    const dim3 fgrid(e->n_blk, R);
    const bool dc2 = e->dc == 2;
    const int dcf = int(e->dc != 0);  // (the DC2 variants take 1, the others dc, which is 0 or 1 there)
    // (the frame pass carries the numerators exactly for the label counts up to EM_FRAME_QMAX: EM is a function of QQ)
    if (b->n_prior) {  // a replica holds a per-vertex prior: the prior twin, log Z_i of every row with the line of its replica's table
        DISPATCH_QB(Q, dc2, hipLaunchKernelGGL((k_em_frame_batch_prior<QQ, BB, (QQ <= EM_FRAME_QMAX)>), fgrid, dim3(frame_cfg<QQ>::TPB), 0, st, e->d_row_ptr,
                                               e->d_rev, e->d_nbr, e->d_deg, e->d_blk_row, e->d_blk_e0, b->d_M, b->d_psi, b->d_P, d_par, d_act, d_mats,
                                               b->msg_stride, b->psi_stride, R, dcf, adj_mode, rows, b->d_em_part[0], b->d_prior_tab));
    } else {
        DISPATCH_QB(Q, dc2, hipLaunchKernelGGL((k_em_frame_batch<QQ, BB, (QQ <= EM_FRAME_QMAX)>), fgrid, dim3(frame_cfg<QQ>::TPB), 0, st, e->d_row_ptr, e->d_rev,
                                               e->d_nbr, e->d_deg, e->d_blk_row, e->d_blk_e0, b->d_M, b->d_psi, b->d_P, d_par, d_act, d_mats, b->msg_stride,
                                               b->psi_stride, R, dcf, adj_mode, rows, b->d_em_part[0]));
    }
    if (e->n_hub)  // site and edge terms of the rows above a segment's capacity: k_fe_hub per replica on offset pointers
        for (uint32_t r = 0; r < R; ++r) {
            if (!h_act[r]) continue;
            const double *M = b->d_M + (size_t(h_par[r]) * R + r) * b->msg_stride;
            double *part = b->d_em_part[0] + size_t(r) * rows * NP;
            if (b->n_prior) {
                DISPATCH_QB(Q, dc2, hipLaunchKernelGGL((k_fe_hub_prior<QQ, BB>), dim3(e->n_hub), dim3(BLOCK), 0, st, e->d_row_ptr, e->d_rev, e->d_nbr, e->d_deg,
                                                       M, (const double *)nullptr, e->d_hub_row, e->d_hub_blk, b->d_P + r, dcf, 0, part, NP, e->n_blk,
                                                       batch_prior_of(b, r)));
            } else {
                DISPATCH_QB(Q, dc2, hipLaunchKernelGGL((k_fe_hub<QQ, BB>), dim3(e->n_hub), dim3(BLOCK), 0, st, e->d_row_ptr, e->d_rev, e->d_nbr, e->d_deg, M,
                                                       (const double *)nullptr, e->d_hub_row, e->d_hub_blk, b->d_P + r, dcf, 0, part, NP, e->n_blk));
            }
        }
    auto fold = [&](const double *in, uint32_t n_rows, uint32_t cols, uint32_t off) {
        hipLaunchKernelGGL(k_fold_batch, dim3((cols + BLOCK / 64 - 1) / (BLOCK / 64), R), dim3(BLOCK), 0, st, in, d_act, n_rows, cols, b->d_em_res, RES, off);
    };
    fold(b->d_em_part[0], rows, NP, 0);
    if (!em_in_frame) {
        DISPATCH_QB(Q, dc2, hipLaunchKernelGGL((k_em_edges_batch<q_clamp(QQ, EM_FRAME_QMAX + 1, 16), BB>), dim3(nbe, R), dim3(BLOCK), 0, st, e->d_row_ptr,
                                               e->d_rev, e->d_nbr, e->d_deg, e->d_src, b->d_M, b->d_P, d_par, d_act, b->msg_stride, R, uint32_t(e->E2),
                                               b->d_em_part[1]));
        fold(b->d_em_part[1], nbe, T, uint32_t(EM_NA) + 2 * Q);
    }
    if (nonedge && exact) {
        DISPATCH_Q(Q, hipLaunchKernelGGL((k_nonedge_exact_batch<QQ>), dim3(g, g, R), dim3(BLOCK), 0, st, b->d_psi, d_par, d_act, d_mats, b->psi_stride, R, N,
                                         b->d_em_part[2]));
        fold(b->d_em_part[2], g * g, 1, NP);
    } else if (nonedge && Tm) {
        hipLaunchKernelGGL(k_moments_batch, dim3(nbm, R), dim3(BLOCK), 0, st, b->d_psi, d_par, d_act, b->psi_stride, R, N, int(Q), K, 512u, int(Tm),
                           b->d_em_part[2]);
        fold(b->d_em_part[2], nbm, Tm, NP);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(b->h_em_res, b->d_em_res, size_t(R) * RES * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // the round's one synchronisation

    // ---- host: per replica
    const double *res = b->h_em_res;
    std::vector<double> ce(QQ2);
    for (uint32_t r = 0; r < R; ++r) {
        if (!h_act[r]) continue;
        batch_replica &p = b->rep[r];
        if (h_ref[r]) p.field_fresh = true;
        const double *row = res + size_t(r) * RES, *na = row + EM_NA, *nna = na + Q, *tri = nna + Q;
        if (na_e) std::copy(na, na + Q, na_e + size_t(r) * Q);
        if (nna_e) std::copy(nna, nna + Q, nna_e + size_t(r) * Q);
        if (cab_e) {
            em_rescale(Q, N, e->dc, na, nna, tri, ce.data());
            std::copy(ce.begin(), ce.end(), cab_e + size_t(r) * QQ2);
        }
        if (f || parts) {
            const double sums[4] = {row[0], row[1], 0.0, 0.0}, adj[2] = {row[EM_ADJ], 0.0};
            double p4[4], all[2] = {0.0, 0.0}, ne[2] = {0.0, 0.0};
            site_edge_parts(N, e->dc == 1 ? &e->sum_log_didl : nullptr, sums, p4);
            if (nonedge) {
                if (exact) all[0] = row[NP];
                else nonedge_series(Q, N, Kr[r], false, row + NP, h_mats + size_t(r) * 3 * QQ2, all);
                nonedge_finish(all, adj, N, ne);
            }
            const double fp[3] = {p4[0], p4[1], ne[0]};
            if (parts) std::copy(fp, fp + 3, parts + 3 * size_t(r));
            if (f) f[r] = free_energy_of(fp);
        }
    }
    return SBMBP_OK;
}

// ---- agreement of replicas (sbmbp.h: sbmbp_batch_agreement; kernels_batch.h: k_agree, k_agree_fold) ---------------------
// kind and tiles per wave bound together, in the manner of DISPATCH_QB: the statement sees `constexpr int KK, TT`
#define DISPATCH_AGREE_T(tpw, ...)                                       \
    switch (tpw) {                                                       \
        case 1: { constexpr int TT = 1; __VA_ARGS__; } break;            \
        case 4: { constexpr int TT = 4; __VA_ARGS__; } break;            \
        default: { constexpr int TT = 16; __VA_ARGS__; } break;          \
    }
#define DISPATCH_AGREE(kind, tpw, ...)                                               \
    switch (kind) {                                                                  \
        case 0: { constexpr int KK = 0; DISPATCH_AGREE_T(tpw, __VA_ARGS__) } break;  \
        case 1: { constexpr int KK = 1; DISPATCH_AGREE_T(tpw, __VA_ARGS__) } break;  \
        default: { constexpr int KK = 2; DISPATCH_AGREE_T(tpw, __VA_ARGS__) } break; \
    }

constexpr size_t AG_PART_BUDGET = size_t(8) << 20;  // doubles (64 MiB): the most the partial tables of k_agree may take
constexpr uint32_t AG_GRID = 1024;                  // workgroups of one k_agree launch, about four per CU

template <int KIND, int TPW>
int launch_agree(hipStream_t st, dim3 grid, size_t lds, const double *psi, const uint32_t *slot, size_t psi_stride, uint32_t N, uint32_t Q, uint32_t n,
                 uint32_t tile_rows, double *partials) {
    // (above 64 KB of dynamic LDS the runtime wants to be told; CP = 256 takes 68.5 KB)
    if (lds > 65536) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_agree<KIND, TPW>), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    hipLaunchKernelGGL((k_agree<KIND, TPW>), grid, dim3(AG_TPB), lds, st, psi, slot, psi_stride, N, Q, n, tile_rows, partials);
    return SBMBP_OK;
}

// The arguments have been checked. Reads the marginal tables of the listed replicas and nothing else; writes only the
// agreement buffers of the batch. The parities are the host's: every call that moves a replica's parity (batch_run, the
// state setters) returns after the stream has drained, so rep[r].par is current, while d_par holds the parities at the START
// of the last run and stays untouched here. The launches go behind whatever the stream holds.
int batch_agreement(sbmbp_batch *b, int kind, const uint32_t *list, uint32_t n, double *confusion, double *overlap, uint32_t *perm) {
    sbmbp_engine *e = b->e;
    const uint32_t R = b->R, Q = e->Q, N = e->N, nQ = n * Q, CT = (nQ + 15) / 16, CP = 16 * CT;
    // tiles per wave and tile rows per workgroup: 4 TPW accumulator tiles hold tile_rows rows of CT tiles
    const int tpw = CT * CT <= 4 ? 1 : (CT * CT <= 16 ? 4 : 16);
    const uint32_t tile_rows = std::min<uint32_t>(CT, uint32_t(4 * tpw) / CT), gy = (CT + tile_rows - 1) / tile_rows;
    const uint32_t n_trips = std::max<uint32_t>(1, (N + AG_V - 1) / AG_V);
    // workgroups along the vertices: at least four trips each (the set-up of the tile keys and the final store are paid once),
    // at most AG_GRID in the launch, and partial tables within the budget (at CP = 256 a table is 512 KB: 128 of them)
    const uint32_t gx = uint32_t(std::max<size_t>(1, std::min<size_t>({size_t((n_trips + 3) / 4), size_t(AG_GRID / gy), AG_PART_BUDGET / (size_t(CP) * CP)})));
    const size_t n_res = size_t(nQ) * nQ, h_bytes = size_t(AG_MAXN) * sizeof(uint32_t) + n_res * 8;
    // grown, never shrunk, like the EM partials - but outside device_bytes: the call changes no statistic of the batch
    CHK(b->d_ag_slot.ensure(AG_MAXN));
    CHK(b->d_ag_part.ensure(size_t(gx) * CP * CP));
    CHK(b->d_ag_res.ensure(n_res));
    CHK(b->h_ag.ensure(h_bytes));
    uint32_t *h_slot = reinterpret_cast<uint32_t *>(b->h_ag.get());
    const double *res = reinterpret_cast<const double *>(h_slot + AG_MAXN);
    for (uint32_t x = 0; x < n; ++x) {
        const uint32_t r = list ? list[x] : x;
        h_slot[x] = uint32_t(b->rep[r].par) * R + r;
    }
    hipStream_t st = e->stream;
    HIPCHK(hipMemcpyAsync(b->d_ag_slot, h_slot, size_t(n) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    DISPATCH_AGREE(kind, tpw, CHK((launch_agree<KK, TT>(st, dim3(gx, gy), agree_lds_bytes(CP, n), b->d_psi, b->d_ag_slot, b->psi_stride, N, Q, n, tile_rows,
                                                        b->d_ag_part))));
    hipLaunchKernelGGL(k_agree_fold, dim3(uint32_t((n_res + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, b->d_ag_part, gx, CP, Q, n, b->d_ag_res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(const_cast<double *>(res), b->d_ag_res, n_res * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (confusion) std::copy(res, res + n_res, confusion);
    if (overlap || perm) {
        std::vector<uint32_t> pi(Q);
        for (size_t xy = 0; xy < size_t(n) * n; ++xy) {
            const double s = best_assignment(Q, res + xy * Q * Q, pi.data());
            if (overlap) overlap[xy] = s / double(N);
            if (perm) std::copy(pi.begin(), pi.end(), perm + xy * Q);
        }
    }
    return SBMBP_OK;
}

}  // namespace

#define BATCH_ARGS(b) do { if (!(b)) return arg_error(__func__, __LINE__); } while (0)

extern "C" {

int sbmbp_batch_create(sbmbp_batch_t **out, const sbmbp_graph_t *g, uint32_t Q, uint32_t dc, uint32_t n_replicas, int device) {
    if (!out || !g) return arg_error(__func__, __LINE__);
    *out = nullptr;
    if (n_replicas == 0) { set_error("a replica batch needs n_replicas >= 1"); return SBMBP_ERR_ARG; }
    if (n_replicas > 65535) { set_error("n_replicas above 65535: the replica index is the second grid dimension of the sweep launch"); return SBMBP_ERR_ARG; }
    if (Q < 2) { set_error("Q must be at least 2"); return SBMBP_ERR_ARG; }
    if (dc > 2) { set_error("deg_corr_flag must be 0, 1 or 2"); return SBMBP_ERR_ARG; }
    if (Q > 16) { set_error("replica batches are implemented up to Q = 16 (the lane-per-edge kernels); Q = " + std::to_string(Q)); return SBMBP_ERR_UNSUPPORTED; }
    std::unique_ptr<sbmbp_batch> b(new sbmbp_batch());
    CHK(create_engine(&b->e, g, Q, dc, device, false));  // the message, marginal and parameter buffers are the batch's
    sbmbp_engine *e = b->e;
    device_scope dev_(e);
    b->R = n_replicas;
    e->gather_mode = 1;  // message-gather form only: the reductions of a bound replica take the message-gather kernels too
    b->msg_stride = size_t(std::max<uint64_t>(e->E2, 1)) * (Q - 1);  // >= one record: the sweep's loads are branch-free
    b->psi_stride = size_t(e->N) * Q;
    b->rec_stride = size_t(std::max<uint32_t>(e->n_blk, 1)) * (Q + 1);
    const uint64_t R = n_replicas;
    const uint64_t need = R * (2 * uint64_t(b->msg_stride) + 2 * uint64_t(b->psi_stride)) * 8;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b) {
        set_error("a batch of " + std::to_string(R) + " replicas needs " + std::to_string(need) + " B of HBM for its states, " + std::to_string(free_b) + " B are free");
        return SBMBP_ERR_NOMEM;
    }
    CHK(dev_alloc(e, b->d_M, 2 * R * b->msg_stride));
    CHK(dev_alloc(e, b->d_psi, 2 * R * b->psi_stride));
    CHK(dev_alloc(e, b->d_rec, R * b->rec_stride));
    CHK(dev_alloc(e, b->d_P, R));
    CHK(dev_alloc(e, b->d_par, R));
    CHK(dev_alloc(e, b->d_cs, R * (sizeof(conv_state) / 4)));
    CHK(dev_alloc(e, b->d_prior_tab, R));  // filled when a table is set; never read before
    HIPCHK(hipMemsetAsync(b->d_rec, 0, R * b->rec_stride * 8, e->stream));
    HIPCHK(hipMemsetAsync(b->d_P, 0, R * sizeof(dev_params), e->stream));
    HIPCHK(hipMemsetAsync(b->d_par, 0, R * sizeof(int), e->stream));
    CHK(b->h_cs.alloc(2 * R));
    for (auto &ev : b->ev_cs) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHK(hipStreamSynchronize(e->stream));
    b->rep.resize(n_replicas);
    *out = b.release();
    return SBMBP_OK;
}

// ~sbmbp_batch drains the stream, the buffers go with the members, ~batch_engine destroys the events and the engine
void sbmbp_batch_destroy(sbmbp_batch_t *b) { delete b; }

uint32_t sbmbp_batch_num_replicas(const sbmbp_batch_t *b) { return b ? b->R : 0; }

int sbmbp_batch_init_messages(sbmbp_batch_t *b, uint32_t flag, const int32_t *conf, const uint32_t *true_conf, const uint32_t *seeds,
                              int conditional) {
    if (!b || !seeds) return arg_error(__func__, __LINE__);
    device_scope dev_(b->e);
    for (uint32_t r = 0; r < b->R; ++r) {
        bound_replica v(b, r);
        CHK(sbmbp_init_messages(b->e, flag, conf, true_conf, seeds[r], conditional));
    }
    return SBMBP_OK;
}
int sbmbp_batch_init_messages_device(sbmbp_batch_t *b, const uint64_t *seeds, const uint32_t *true_conf) {
    if (!b || !seeds) return arg_error(__func__, __LINE__);
    device_scope dev_(b->e);
    for (uint32_t r = 0; r < b->R; ++r) {
        bound_replica v(b, r);
        CHK(sbmbp_init_messages_device(b->e, seeds[r], true_conf));
    }
    return SBMBP_OK;
}

int sbmbp_batch_set_params(sbmbp_batch_t *b, int replica, const double *cab, const uint32_t *na, double beta) {
    if (!b || !cab || !na) return arg_error(__func__, __LINE__);
    if (replica != -1) CHK(batch_replica_arg(b, replica));
    device_scope dev_(b->e);
    for (uint32_t r = 0; r < b->R; ++r) {
        if (replica != -1 && uint32_t(replica) != r) continue;
        bound_replica v(b, r);
        CHK(sbmbp_set_params(b->e, cab, na, beta));
    }
    return SBMBP_OK;
}
int sbmbp_batch_get_params(sbmbp_batch_t *b, uint32_t replica, double *cab, uint32_t *na, double *beta) {
    BATCH_ARGS(b);
    CHK(batch_replica_arg(b, replica));
    const batch_replica &p = b->rep[replica];
    if (!p.have_params) return SBMBP_ERR_STATE;
    if (cab) std::copy(p.cab.begin(), p.cab.end(), cab);
    if (na) std::copy(p.na.begin(), p.na.end(), na);
    if (beta) *beta = p.beta;
    return SBMBP_OK;
}

int sbmbp_batch_set_state(sbmbp_batch_t *b, uint32_t replica, const double *psi, const double *msg_out) {
    BATCH_ARGS(b);
    CHK(batch_replica_arg(b, replica));
    device_scope dev_(b->e);
    bound_replica v(b, replica);
    return sbmbp_set_state(b->e, psi, msg_out);
}
int sbmbp_batch_get_state(sbmbp_batch_t *b, uint32_t replica, double *psi, double *msg_out) {
    BATCH_ARGS(b);
    CHK(batch_replica_arg(b, replica));
    device_scope dev_(b->e);
    bound_replica v(b, replica);
    return sbmbp_get_state(b->e, psi, msg_out);
}
// ---- per-vertex priors of a batch: every replica reads no table, the batch's one shared table, or its own -------------
int sbmbp_batch_set_vertex_prior(sbmbp_batch_t *b, int replica, const double *prior) {
    BATCH_ARGS(b);
    if (replica != -1) CHK(batch_replica_arg(b, replica));
    sbmbp_engine *e = b->e;
    const uint32_t R = b->R;
    const size_t n = size_t(e->N) * e->Q;
    if (prior && e->sweep_order == 1) {
        set_error("a per-vertex prior cannot be combined with the coloured sweep order: sbmbp_batch_set_sweep_order(b, 0, ...) first");
        return SBMBP_ERR_UNSUPPORTED;
    }
    if (prior) {
        std::string why;
        const uint32_t bad = first_bad_prior_row(prior, e->N, e->Q, &why);
        if (bad < e->N) {
            set_error("sbmbp_batch_set_vertex_prior: prior row of vertex " + std::to_string(bad) +
                      (replica >= 0 ? " (replica " + std::to_string(replica) + ")" : std::string()) + ": " + why);
            return SBMBP_ERR_ARG;
        }
    }
    device_scope dev_(e);
    // the states this call leaves: which tables are still read, and whether some replica needs the table of ones
    std::vector<int> next(R);
    uint32_t held = 0, shared = 0;
    for (uint32_t r = 0; r < R; ++r) {
        next[r] = (replica == -1 || uint32_t(replica) == r) ? (prior ? (replica == -1 ? 1 : 2) : 0) : b->rep[r].prior_state;
        held += next[r] != 0;
        shared += next[r] == 1;
    }
    const bool need_ones = held && held < R;
    // allocations first, into locals: a table that does not fit leaves the batch as it was
    device_buffer<double> &slot = replica == -1 ? b->d_prior_shared : b->rep[replica].d_prior;
    device_buffer<double> new_ones, new_slot;
    const bool fresh_ones = need_ones && !b->d_prior_ones;
    if (fresh_ones) CHK(dev_alloc(e, new_ones, n));
    if (prior && !slot) CHK(dev_alloc(e, new_slot, n));
    HIPCHK(hipStreamSynchronize(e->stream));  // nothing in flight reads a table that is overwritten or freed below
    if (new_ones) b->d_prior_ones = std::move(new_ones);
    if (new_slot) slot = std::move(new_slot);
    std::vector<double> ones;
    if (fresh_ones) {
        ones.assign(n, 1.0);
        HIPCHK(hipMemcpyAsync(b->d_prior_ones, ones.data(), n * 8, hipMemcpyHostToDevice, e->stream));
    }
    if (prior) HIPCHK(hipMemcpyAsync(slot, prior, n * 8, hipMemcpyHostToDevice, e->stream));
    for (uint32_t r = 0; r < R; ++r) {
        batch_replica &p = b->rep[r];
        p.prior_state = next[r];
        if (next[r] != 2) p.d_prior.reset();
    }
    if (!shared) b->d_prior_shared.reset();
    if (!need_ones) b->d_prior_ones.reset();
    b->n_prior = held;
    // (what the batch caches about a replica's state is its field, which no prior enters; the engine's caches, psi_consistent
    // and the fused pass, are dropped whenever a replica is bound)
    std::vector<const double *> tab(R, nullptr);
    if (held) {
        for (uint32_t r = 0; r < R; ++r) tab[r] = batch_prior_of(b, r);
        HIPCHK(hipMemcpyAsync(b->d_prior_tab, tab.data(), size_t(R) * sizeof(const double *), hipMemcpyHostToDevice, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return SBMBP_OK;
}
int sbmbp_batch_get_vertex_prior(sbmbp_batch_t *b, uint32_t replica, double *prior, int *present) {
    BATCH_ARGS(b);
    CHK(batch_replica_arg(b, replica));
    const batch_replica &p = b->rep[replica];
    if (present) *present = p.prior_state;
    if (prior && p.prior_state) {
        sbmbp_engine *e = b->e;
        device_scope dev_(e);
        HIPCHK(hipMemcpyAsync(prior, p.prior_state == 2 ? p.d_prior.get() : b->d_prior_shared.get(), size_t(e->N) * e->Q * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return SBMBP_OK;
}

int sbmbp_batch_get_field(sbmbp_batch_t *b, uint32_t replica, double *h) {
    if (!b || !h) return arg_error(__func__, __LINE__);
    CHK(batch_replica_arg(b, replica));
    device_scope dev_(b->e);
    bound_replica v(b, replica);
    return sbmbp_get_field(b->e, h);
}
int sbmbp_batch_get_relaxation(const sbmbp_batch_t *b, uint32_t replica, int *field_level, int *generic_level, double *field_mix,
                               double *damping_factor) {
    BATCH_ARGS(b);
    CHK(batch_replica_arg(b, replica));
    const batch_replica &p = b->rep[replica];
    if (b->e->sweep_order == 1) {  // no relaxation of any kind in the coloured order
        if (field_level) *field_level = 0;
        if (generic_level) *generic_level = -1;
        if (field_mix) *field_mix = 1.0;
        if (damping_factor) *damping_factor = 1.0;
        return SBMBP_OK;
    }
    if (field_level) *field_level = p.ar_fl;
    if (generic_level) *generic_level = p.ar_gl;
    if (field_mix) *field_mix = std::min(std::min(b->e->field_mix, ar_field_cap(p.ar_fl)), ar_gen_mix(p.ar_gl));
    if (damping_factor) *damping_factor = ar_gen_damp(p.ar_gl);
    return SBMBP_OK;
}

int sbmbp_batch_set_schedule(sbmbp_batch_t *b, double field_mix, uint32_t check_every) {
    BATCH_ARGS(b);
    return sbmbp_set_schedule(b->e, field_mix, check_every);
}
int sbmbp_batch_set_auto_relax(sbmbp_batch_t *b, int on) {
    BATCH_ARGS(b);
    return sbmbp_set_auto_relax(b->e, on);
}
int sbmbp_batch_set_nonedge_mode(sbmbp_batch_t *b, int nonedge_mode, int series_order) {
    BATCH_ARGS(b);
    return sbmbp_set_nonedge_mode(b->e, nonedge_mode, series_order);
}

// The order is common to all replicas: the colouring and the step tables belong to the graph, and they are the single
// engine's (sbmbp_set_sweep_order on the batch's engine: coloured_plan, coloured_step_tables, build_coloured). A step's
// records are (Q + 1) doubles per segment and hub row of the step, so the record table of every replica grows to
// max(n_blk, cs_max_rec) records here; going back to order 0 keeps tables and records (a later switch is cheap, and the
// synchronous sweep reads the stride it is given).
int sbmbp_batch_set_sweep_order(sbmbp_batch_t *b, int order, const uint32_t *colour, double step_fraction) {
    if (!b || order < 0 || order > 1) return arg_error(__func__, __LINE__);
    sbmbp_engine *e = b->e;
    device_scope dev_(e);
    if (order == 1 && b->n_prior) {
        set_error("the coloured sweep order takes no per-vertex prior: remove it first (sbmbp_batch_set_vertex_prior(b, -1, NULL))");
        return SBMBP_ERR_UNSUPPORTED;
    }
    CHK(sbmbp_set_sweep_order(e, order, colour, step_fraction));
    if (order == 0) return SBMBP_OK;
    const size_t need = size_t(std::max<uint32_t>(std::max(e->n_blk, e->cs_max_rec), 1)) * (e->Q + 1);
    if (need > b->rec_stride) {
        HIPCHK(hipStreamSynchronize(e->stream));  // nothing in flight writes the records that are freed
        const int r = b->d_rec.replace(size_t(b->R) * need, &e->device_bytes);  // (a failure leaves the records as they were)
        if (r != SBMBP_OK) { e->sweep_order = 0; return r; }
        b->rec_stride = need;
        HIPCHK(hipMemsetAsync(b->d_rec, 0, size_t(b->R) * need * 8, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return SBMBP_OK;
}
int sbmbp_batch_get_sweep_order(const sbmbp_batch_t *b, int *order, uint32_t *n_colours, uint32_t *n_steps) {
    BATCH_ARGS(b);
    return sbmbp_get_sweep_order(b->e, order, n_colours, n_steps);
}

int sbmbp_batch_sweep(sbmbp_batch_t *b, double damping, uint32_t n_sweeps, double *last) {
    BATCH_ARGS(b);
    device_scope dev_(b->e);
    const uint32_t keep = b->e->check_every;
    b->e->check_every = std::max<uint32_t>(keep, 64);  // no convergence test: sync rarely
    const std::vector<double> crit(b->R, -1.0);
    const int r = batch_run(b, crit.data(), nullptr, n_sweeps, damping, nullptr, last);
    b->e->check_every = keep;
    return r;
}
int sbmbp_batch_converge(sbmbp_batch_t *b, double crit, uint32_t max_sweeps, double damping, int *niter, double *last) {
    BATCH_ARGS(b);
    device_scope dev_(b->e);
    const std::vector<double> crits(b->R, crit);
    return batch_run(b, crits.data(), nullptr, max_sweeps, damping, niter, last);
}

int sbmbp_batch_free_energy(sbmbp_batch_t *b, double *f, double *parts) {
    BATCH_ARGS(b);
    device_scope dev_(b->e);
    for (uint32_t r = 0; r < b->R; ++r) {
        bound_replica v(b, r);
        CHK(free_energy_impl(b->e, f ? f + r : nullptr, parts ? parts + 3 * size_t(r) : nullptr));
    }
    return SBMBP_OK;
}
int sbmbp_batch_entropy(sbmbp_batch_t *b, double *ent, double *parts) {
    BATCH_ARGS(b);
    device_scope dev_(b->e);
    for (uint32_t r = 0; r < b->R; ++r) {
        bound_replica v(b, r);
        CHK(entropy_impl(b->e, ent ? ent + r : nullptr, parts ? parts + 3 * size_t(r) : nullptr));
    }
    return SBMBP_OK;
}
int sbmbp_batch_overlap(sbmbp_batch_t *b, double *ov) {
    if (!b || !ov) return arg_error(__func__, __LINE__);
    device_scope dev_(b->e);
    for (uint32_t r = 0; r < b->R; ++r) {
        bound_replica v(b, r);
        CHK(overlap_impl(b->e, ov + r, nullptr));
    }
    return SBMBP_OK;
}
int sbmbp_batch_em_expectations(sbmbp_batch_t *b, uint32_t replica, double *na_e, double *nna_e, double *cab_e) {
    BATCH_ARGS(b);
    CHK(batch_replica_arg(b, replica));
    device_scope dev_(b->e);
    bound_replica v(b, replica);
    return em_expect(b->e, na_e, nna_e, cab_e);
}

int sbmbp_batch_inference(sbmbp_batch_t *b, float conv_crit, uint32_t time_conv, float dumping_rate, sbmbp_infer_result *out, uint32_t *best) {
    if (!b || !out) return arg_error(__func__, __LINE__);
    device_scope dev_(b->e);
    std::vector<int> niter(b->R);
    std::vector<double> last(b->R);
    const std::vector<double> crits(b->R, double(conv_crit));
    CHK(batch_run(b, crits.data(), nullptr, time_conv, double(dumping_rate), niter.data(), last.data()));
    for (uint32_t r = 0; r < b->R; ++r) {
        bound_replica v(b, r);
        out[r].niter = niter[r];
        out[r].last_maxdiff = last[r];
        CHK(inference_reductions(b->e, &out[r]));
    }
    if (best) {  // lowest free energy among the converged replicas (among all when none converged); NaN never; ties: lowest index
        std::vector<double> f(b->R);
        std::vector<int> rank(b->R);
        for (uint32_t r = 0; r < b->R; ++r) { f[r] = out[r].free_energy; rank[r] = out[r].niter >= 0 ? 0 : 1; }
        *best = best_replica(b->R, f.data(), rank.data(), 2);
    }
    return SBMBP_OK;
}

int sbmbp_batch_set_learning_schedule(sbmbp_batch_t *b, double field_mix, double snap) {
    BATCH_ARGS(b);
    return sbmbp_set_learning_schedule(b->e, field_mix, snap);
}

int sbmbp_batch_em_step(sbmbp_batch_t *b, double *na_expect, double *nna_expect, double *cab_expect, double *f, double *parts) {
    BATCH_ARGS(b);
    for (uint32_t r = 0; r < b->R; ++r)
        if (!b->rep[r].have_params || !b->rep[r].have_state) {
            set_error("replica " + std::to_string(r) + " has no parameters or no state");
            return SBMBP_ERR_STATE;
        }
    device_scope dev_(b->e);
    return batch_reductions(b, nullptr, na_expect, nna_expect, cab_expect, f, parts);
}

int sbmbp_batch_learning(sbmbp_batch_t *b, float learning_conv_crit, uint32_t learning_max_time, float learning_rate, float dumping_rate,
                         sbmbp_learn_result *out, double *eta, double *cab, uint32_t *best) {
    if (!b || !out) return arg_error(__func__, __LINE__);
    CHK(batch_check_ready(b, "learning"));
    sbmbp_engine *e = b->e;
    device_scope dev_(e);
    const uint32_t R = b->R, Q = e->Q;
    struct front_end {
        sbmbp_batch *b;
        uint32_t max_sweeps;
        double damping;
        sbmbp_learn_result *out;
        int converge(const double *crit, const uint8_t *active, uint32_t *executed) {
            return batch_run(b, crit, active, max_sweeps, damping, nullptr, nullptr, executed);
        }
        int expect(const uint8_t *active, double *na_e, double *nna_e, double *cab_e, double *f) {
            return batch_reductions(b, active, na_e, nna_e, cab_e, f, nullptr);
        }
        void params(uint32_t r, std::vector<uint32_t> &na, std::vector<double> &cab) { na = b->rep[r].na; cab = b->rep[r].cab; }
        int apply(uint32_t r, const uint32_t *na, const double *cab) {
            bound_replica v(b, r);
            apply_params_host(b->e, cab, na, b->e->beta);
            return SBMBP_OK;
        }
        int finish(uint32_t r) {
            bound_replica v(b, r);
            CHK(upload_params(b->e, 0.0));
            b->e->field_fresh = false;  // (the parameter block starts from a zero field again)
            return overlap_impl(b->e, &out[r].overlap, nullptr);
        }
    } fe{b, learning_max_time, double(dumping_rate), out};
    CHK(em_loop(fe, R, Q, e->N, learning_conv_crit, learning_max_time, double(learning_rate), e->learn_snap, e->field_mix, e->learn_field_mix, out));
    std::vector<int> rank(R);
    std::vector<double> fold(R);
    for (uint32_t r = 0; r < R; ++r) {
        fold[r] = out[r].free_energy;
        rank[r] = out[r].status == 1 ? 0 : (out[r].status == 0 ? 1 : -1);
        const batch_replica &p = b->rep[r];
        if (eta) std::copy(p.eta.begin(), p.eta.end(), eta + size_t(r) * Q);
        if (cab) std::copy(p.cab.begin(), p.cab.end(), cab + size_t(r) * Q * Q);
    }
    if (best) *best = best_replica(R, fold.data(), rank.data(), 2);
    return SBMBP_OK;
}

int sbmbp_learning_step_host(uint32_t Q, uint32_t n_vertices, double learning_rate, double snap, double crit, const double *na_expect,
                             const double *cab_expect, uint32_t *na, double *cab) {
    if (Q < 1 || !na_expect || !cab_expect || !na || !cab) return arg_error(__func__, __LINE__);
    learning_step_host(Q, n_vertices, learning_rate, snap, crit, na_expect, cab_expect, na, cab);
    return SBMBP_OK;
}

int sbmbp_best_replica(uint32_t n, const double *free_energy, const int *rank, int n_ranks, uint32_t *best) {
    if (!n || !free_energy || !rank || !best) return arg_error(__func__, __LINE__);
    *best = best_replica(n, free_energy, rank, n_ranks);
    return SBMBP_OK;
}

int sbmbp_batch_get_stats(sbmbp_batch_t *b, sbmbp_stats *out) {
    if (!b || !out) return arg_error(__func__, __LINE__);
    const sbmbp_engine *e = b->e;
    std::memset(out, 0, sizeof *out);
    out->sweeps = b->sweeps;  // replica-sweeps actually executed
    out->edge_msg_updates = b->sweeps * e->E2;
    out->bytes_per_sweep = double(e->E2) * (24.0 * e->Q + 4.0 + (e->dc == 2 ? 4.0 : 0.0)) + double(e->N) * (8.0 * e->Q + 8.0);  // of ONE replica
    if (b->n_prior) out->bytes_per_sweep += 8.0 * e->Q * double(e->N);  // every row reads the line of its replica's table once
    out->device_bytes = e->device_bytes;
    out->n_blocks = e->n_blk;
    out->n_hub_rows = e->n_hub;
    out->hub_edges = e->hub_edges;
    out->psi_form_sweeps = 0;
    return SBMBP_OK;
}

int sbmbp_batch_agreement(sbmbp_batch_t *b, int kind, const uint32_t *replicas, uint32_t n, double *confusion, double *overlap, uint32_t *perm) {
    if (!b) { set_error("sbmbp_batch_agreement: null batch"); return SBMBP_ERR_ARG; }
    if (kind < 0 || kind > 2) { set_error("sbmbp_batch_agreement: kind " + std::to_string(kind) + " (0 soft, 1 hard-soft, 2 hard)"); return SBMBP_ERR_ARG; }
    const uint32_t R = b->R, Q = b->e->Q;
    if (replicas && n == 0) { set_error("sbmbp_batch_agreement: a replica list needs n >= 1"); return SBMBP_ERR_ARG; }
    if (!replicas) n = R;
    std::vector<char> seen(R, 0);
    for (uint32_t x = 0; x < n; ++x) {
        const uint32_t r = replicas ? replicas[x] : x;
        if (r >= R) { set_error("sbmbp_batch_agreement: replica index " + std::to_string(r) + " outside the batch of " + std::to_string(R)); return SBMBP_ERR_ARG; }
        if (seen[r]) { set_error("sbmbp_batch_agreement: replica " + std::to_string(r) + " is listed twice"); return SBMBP_ERR_ARG; }
        seen[r] = 1;
    }
    if (uint64_t(n) * Q > uint64_t(AG_CPMAX)) {
        set_error("sbmbp_batch_agreement: " + std::to_string(n) + " replicas of " + std::to_string(Q) + " labels are " + std::to_string(uint64_t(n) * Q) +
                  " columns, above " + std::to_string(AG_CPMAX) + ": pass a subset list of replicas");
        return SBMBP_ERR_UNSUPPORTED;
    }
    for (uint32_t x = 0; x < n; ++x) {
        const uint32_t r = replicas ? replicas[x] : x;
        if (!b->rep[r].have_state) {
            set_error("sbmbp_batch_agreement: replica " + std::to_string(r) + " has no state (init_messages / set_state first)");
            return SBMBP_ERR_STATE;
        }
    }
    device_scope dev_(b->e);
    return batch_agreement(b, kind, replicas, n, confusion, overlap, perm);
}

int sbmbp_agreement_groups(uint32_t n, const double *overlap, double threshold, uint32_t *group, uint32_t *n_groups) {
    if ((n && (!overlap || !group)) || !n_groups) return arg_error(__func__, __LINE__);
    *n_groups = agreement_groups(n, overlap, threshold, group);
    return SBMBP_OK;
}

}  // extern "C"
