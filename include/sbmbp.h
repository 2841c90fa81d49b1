/*
 * sbmbp.h — C ABI of the MI355X-native belief-propagation engine for the (degree-corrected)
 * stochastic block model. This is the drop-in boundary for the reference's BP path: every entry
 * point names the reference interface (file:line under junipertcy/sbm-bp `src/`) it replaces.
 *
 * The reference has no FFI layer; its de-facto source-level boundary is the public interface of
 * `class belief_propagation` as `main.cpp:318-365` drives it (belief_propagation.h:96-142), plus
 * `blockmodel.h:105-107` (parameter constructors) and `graph_utilities.h:14-22` (graph input).
 * A maintainer binds these functions from `main.cpp` as shown in INTEGRATION.md.
 *
 * Conventions: plain C types only; 0 = SBMBP_OK, negative = error (sbmbp_strerror);
 * the caller owns every host array it passes (the library copies); the library owns all device
 * memory; one engine handle = one GPU = one host thread; no exceptions cross the boundary.
 * All floating-point state is IEEE double, as in the reference (types.h:38-41).
 *
 * Data layout (HBM): CSR rows = vertices, neighbours ascending (== std::set order of
 * types.h:14-15); rev[k] = index of the reverse directed edge; messages are OUT-ordered AoS:
 * msg[k*Q+q] = message from row(k) to nbr[k]. The reference's in-ordered mmap_[i][l][q]
 * (belief_propagation.h:65-66) is msg[rev[row_ptr[i]+l]*Q+q]. That is the layout AT THIS BOUNDARY
 * (sbmbp_set_state / sbmbp_get_state / sbmbp_host_init_state). On the device a message is kept as Q-1 of
 * its components (messages are distributions: every row of msg must sum to 1, as every message the
 * reference produces does): all but the largest, which is restored as max(0, 1 - sum of the others);
 * sbmbp_get_state therefore returns that ONE component per message within a few ulp of what
 * sbmbp_set_state was given, the others bit for bit.
 */
#ifndef SBMBP_H
#define SBMBP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBMBP_OK 0
#define SBMBP_ERR_ARG (-1)         /* invalid argument / shape mismatch */
#define SBMBP_ERR_HIP (-2)         /* a HIP runtime call failed (detail in sbmbp_last_error) */
#define SBMBP_ERR_NODEVICE (-3)    /* no usable GPU: the engine never falls back to the CPU */
#define SBMBP_ERR_STATE (-4)       /* call order violated (e.g. converge before set_params) */
#define SBMBP_ERR_IO (-5)          /* file could not be read */
#define SBMBP_ERR_UNSUPPORTED (-6) /* e.g. Q above SBMBP_MAX_Q */
#define SBMBP_ERR_NOMEM (-7)
#define SBMBP_ERR_COMM (-8)        /* a collective (RCCL or the caller's transport) failed */

#define SBMBP_MAX_Q 64 /* label counts 2 .. 16: lane-per-edge kernels (every mode, sharded too); 17 .. 64: matrix-core kernels
                          (single engine, deg_corr_flag 0 / 1, cab > 0; kernels_wide.h) */

typedef struct sbmbp_graph sbmbp_graph_t;   /* host-side CSR graph */
typedef struct sbmbp_engine sbmbp_engine_t; /* device engine (one GPU) */

const char *sbmbp_strerror(int code);
const char *sbmbp_last_error(void); /* thread-local detail string of the last failure */
const char *sbmbp_version(void);
int sbmbp_device_count(void); /* GPUs visible to this process (0 if none) */

/* ---------------------------------------------------------------------------------------------
 * Graph input. Replaces load_edge_list + edge_to_adj (graph_utilities.cpp:42-77: text "a b" per
 * line, symmetrised, de-duplicated, neighbours sorted, vertex count grown to the largest id) and
 * the graph_neis_/graph_neis_inv_ build of bp_allocate (belief_propagation.cpp:246-266).
 * Deviation (documented): a missing file is an error here, not an empty graph.
 * ------------------------------------------------------------------------------------------- */
int sbmbp_graph_load_edgelist(sbmbp_graph_t **out, const char *path, uint32_t n_vertices);
int sbmbp_graph_from_edges(sbmbp_graph_t **out, const uint32_t *pairs /* [2*n_pairs] */, uint64_t n_pairs,
                           uint32_t n_vertices);
/* adopt an existing CSR (rev may be NULL: it is then computed). Arrays are copied and validated. */
int sbmbp_graph_from_csr(sbmbp_graph_t **out, uint32_t n_vertices, uint64_t n_directed,
                         const uint64_t *row_ptr, const uint32_t *nbr, const uint32_t *rev);
uint32_t sbmbp_graph_num_vertices(const sbmbp_graph_t *g);
uint64_t sbmbp_graph_num_directed_edges(const sbmbp_graph_t *g); /* E2 = 2|E| */
uint32_t sbmbp_graph_max_degree(const sbmbp_graph_t *g);         /* blockmodel_t::get_graph_max_degree, blockmodel.cpp:51 */
int sbmbp_graph_copy_csr(const sbmbp_graph_t *g, uint64_t *row_ptr, uint32_t *nbr, uint32_t *rev);
void sbmbp_graph_destroy(sbmbp_graph_t *g);

/* ---------------------------------------------------------------------------------------------
 * Model parameters. Replace bp_param_from_epsilon_c (blockmodel.cpp:229-272) and
 * bp_param_from_direct (blockmodel.cpp:274-302) incl. the na[q]=unsigned(int(pa[q]*N)) truncation.
 * cab is Q*Q row-major; cab_upper is the upper triangle, row-major, as `--cab` passes it.
 * ------------------------------------------------------------------------------------------- */
int sbmbp_param_from_epsilon_c(uint32_t n_vertices, uint32_t Q, double epsilon, double c, double *cab, uint32_t *na);
int sbmbp_param_from_direct(uint32_t n_vertices, uint32_t Q, const double *pa, const double *cab_upper,
                            double *cab, uint32_t *na);

/* ---------------------------------------------------------------------------------------------
 * Engine life cycle. sbmbp_create replaces bp_allocate (belief_propagation.cpp:223-288): it
 * uploads the CSR and allocates messages/marginals in HBM. device < 0 selects the current device.
 * Q = 2 .. SBMBP_MAX_Q (the reference has no cap, main.cpp:271). Up to 16 labels a lane owns a directed edge; above, an
 * edge is spread over four lanes and W^T m runs on the matrix cores (csrc/kernels_wide.h): every entry point below works
 * there too (converge / sweep / free energy / entropy / EM expectations / overlap / inference / learning, damping, beta,
 * clamped rows, deg_corr_flag 0 and 1, the adaptive relaxation), except deg_corr_flag 2 and cab entries <= 0, which
 * return SBMBP_ERR_UNSUPPORTED; the shard entry points and the multi-GPU driver take Q <= 16.
 * ------------------------------------------------------------------------------------------- */
int sbmbp_create(sbmbp_engine_t **out, const sbmbp_graph_t *g, uint32_t Q, uint32_t deg_corr_flag, int device);
void sbmbp_destroy(sbmbp_engine_t *e);
/* run all work of this engine on an existing HIP stream (hipStream_t passed as void*; 0 = the default
 * stream). Engines start on a private non-blocking stream. */
int sbmbp_set_stream(sbmbp_engine_t *e, void *hip_stream);

/* init_messages (belief_propagation.cpp:101-217): same std::mt19937(seed) stream and fill order as
 * the reference for flag 0/1 (per vertex: psi, then its out-messages in ascending neighbour
 * order). conf: N entries, -1 = unknown, may be NULL for flag 0. true_conf: N entries.
 * conditional != 0 selects bp_conditional semantics (rows with conf != -1 are clamped,
 * belief_propagation.cpp:1100-1126); 0 selects bp_basic. Flags 2/3: see DESIGN.md (reference
 * asserts). */
int sbmbp_init_messages(sbmbp_engine_t *e, uint32_t flag, const int32_t *conf, const uint32_t *true_conf,
                        uint32_t seed, int conditional);
/* the same initial state on the host only (no device, no engine): psi N*Q and msg_out E2*Q doubles in the
 * layout of sbmbp_set_state; what sbmbp_init_messages uploads. */
int sbmbp_host_init_state(const sbmbp_graph_t *g, uint32_t Q, uint32_t flag, const int32_t *conf, uint32_t seed,
                          double *psi, double *msg_out);
/* device-side random initialisation (counter-based generator) for large synthetic runs where the
 * sequential mt19937 fill would dominate; not stream-compatible with the reference. */
int sbmbp_init_messages_device(sbmbp_engine_t *e, uint64_t seed, const uint32_t *true_conf);

/* expand_bp_params + set_beta (belief_propagation.cpp:290-317, 417-419) */
int sbmbp_set_params(sbmbp_engine_t *e, const double *cab, const uint32_t *na, double beta);
int sbmbp_get_params(sbmbp_engine_t *e, double *cab, uint32_t *na);

/* direct state access (the reference keeps real_psi_/mmap_ protected, belief_propagation.h:45,66) */
int sbmbp_set_state(sbmbp_engine_t *e, const double *psi /* N*Q or NULL */, const double *msg_out /* E2*Q or NULL */);
int sbmbp_get_state(sbmbp_engine_t *e, double *psi /* or NULL */, double *msg_out /* or NULL */);
int sbmbp_get_field(sbmbp_engine_t *e, double *h /* Q */); /* h_ of belief_propagation.cpp:320-360 */

/* Per-vertex label prior (no reference counterpart: the reference knows free vertices and vertices clamped to one label only;
 * DESIGN.md section 2). prior[N*Q]: doubles >= 0, finite, at least one entry > 0 in every row; stored as given, never
 * normalised. Row i is updated as without a prior, with eta_q replaced by eta_q * prior[i*Q+q]: in its marginal, in every
 * message it sends (the cavity) and in the exact cavity product the sweep falls back to when a division is unusable - the
 * prior acts like the field of one more incoming edge. It also enters the site terms of the free energy and of the entropy;
 * the field h, the edge and non-edge terms and the EM numerators are formed as before. Scaling row i by a constant c > 0
 * changes no marginal and no message; it adds log(c)/N to parts[0] (f_site) of sbmbp_free_energy, so the free energy, which
 * takes f_site with a minus sign, moves by -log(c)/N. A row of ones is "no prior" for that vertex; a zero entry forbids the
 * label (marginal and out-message entries exactly 0). Clamped rows are not updated, so their prior row is ignored by the sweeps.
 * The prior belongs to the engine like the graph: it survives sbmbp_init_messages*, sbmbp_set_params and sbmbp_set_state, is
 * replaced by the next sbmbp_set_vertex_prior and removed by prior == NULL; setting or removing it drops what the engine
 * caches about the state. sbmbp_learning applies the reference's update rules unchanged with the prior held fixed.
 * While a prior is set the engine runs the message-gather form only, as for general clamped rows: psi_form_sweeps of
 * sbmbp_stats does not grow, the reductions take the message-form kernels, and bytes_per_sweep grows by 8 Q N.
 * SBMBP_ERR_ARG (before any device work; the message names the first offending vertex): a negative, NaN or Inf entry, a row
 * without a positive entry. SBMBP_ERR_UNSUPPORTED: Q > 16; a shard engine; an engine in the coloured sweep order - and
 * sbmbp_set_sweep_order(e, 1, ...) on an engine that holds a prior. Replica batches take theirs through
 * sbmbp_batch_set_vertex_prior (one shared table or one per replica); sbmbp_dist_* take no prior.
 * sbmbp_get_vertex_prior: *present = 1 and the table copied into prior (N*Q, or NULL) when one is set, else *present = 0.
 * sbmbp_prior_load: host only, no device. Reads the text format "vertex w_0 ... w_{Q-1}", one line per annotated vertex in any
 * order, into a dense table (ones where no line names the vertex); *n_rows_given = lines read. SBMBP_ERR_IO: unreadable;
 * SBMBP_ERR_ARG with the line number: vertex id >= n_vertices, a vertex named twice, a wrong column count, a bad value. */
int sbmbp_set_vertex_prior(sbmbp_engine_t *e, const double *prior /* N*Q, or NULL: remove */);
int sbmbp_get_vertex_prior(sbmbp_engine_t *e, double *prior /* N*Q or NULL */, int *present);
int sbmbp_prior_load(const char *path, uint32_t n_vertices, uint32_t Q, double *prior /* N*Q */, uint64_t *n_rows_given);

/* Schedule of the synchronous sweep (no reference counterpart: the reference is random-sequential,
 * belief_propagation.cpp:394-401). field_mix in (0,1]: relaxation of the global field between
 * sweeps (1 = plain Jacobi). check_every >= 1: sweeps enqueued between two host reads of the
 * convergence flag (the returned niter is exact regardless). */
int sbmbp_set_schedule(sbmbp_engine_t *e, double field_mix, uint32_t check_every);

/* Adaptive relaxation of converge / inference / learning (on by default; no reference counterpart). The reference sweeps
 * random-sequentially and keeps h_ current inside a sweep (belief_propagation.cpp:394-401, 1088-1095); synchronous sweeps can
 * oscillate where it converges. With this on, the device-side convergence logic watches for (F) a period-2 swing of the
 * field sums, (P) a period-2 swing of the messages, (W) a window of sweeps without progress, and lowers field_mix
 * (1 -> 0.25 -> 0.1 -> 0.05) or moves down a (field_mix cap, damping factor) ladder ((0.5,1), (0.25,1), (0.5,0.5),
 * (0.25,0.5), (0.1,0.5), (0.25,0.25), (0.1,0.25)); the fixed points do not move, and runs that never oscillate are untouched. Fixed sweep
 * counts (sbmbp_sweep) are never relaxed. sbmbp_get_relaxation reports where the last converge call ended
 * (field level 0 and generic level -1: it never relaxed). */
int sbmbp_set_auto_relax(sbmbp_engine_t *e, int on);
int sbmbp_get_relaxation(const sbmbp_engine_t *e, int *field_level, int *generic_level, double *field_mix, double *damping_factor);

/* Which form of the sweep kernel runs. 0 = automatic: incoming messages are reconstructed from the
 * neighbours' marginals (same iterates, cache-friendly gather) whenever that is exact — damping 1,
 * every cab entry > 0, no clamped rows, deg_corr_flag != 2 — with the reference's 1-step message
 * criterion verified on the message buffers before convergence is declared; otherwise, and always
 * with mode 1, incoming messages are gathered from the message array. */
int sbmbp_set_gather_mode(sbmbp_engine_t *e, int mode);

/* Sweep order (no reference counterpart in this form). order 0 = synchronous (default), 1 = coloured
 * Gauss-Seidel: like the reference's converge (belief_propagation.cpp:394-401, 1088-1095) it never updates two neighbours
 * at once and keeps the global field h_ current inside a sweep. Colouring: vertices in order (degree descending, index
 * ascending) take the smallest colour no neighbour holds (self-loops ignored). Steps: classes in colour order, rows ascending
 * inside a class, consecutive chunks of at most max(1, ceil(step_fraction * N)) rows; a step updates its rows at once, in
 * place, from the current state and the current field, then the field is moved by the step's change of the marginals.
 * The sweep's reported difference is the maximum over its steps of the undamped 1-step message difference.
 * sbmbp_coloured_plan: host only, no device: the plan the engine would use. colour_in NULL = built-in greedy colouring.
 * colour / step: N entries or NULL; step = index of the field-refresh step that updates the vertex.
 * sbmbp_set_sweep_order: colour NULL = built-in, else N entries, validated (colour[i] != colour[j] for every edge i != j and
 * every value < N, else SBMBP_ERR_ARG); step_fraction 0 = default 1/8, 1 = one step per class, <= 1/N = one vertex per step.
 * sbmbp_sweep / sbmbp_converge / sbmbp_inference / sbmbp_learning follow the order set; damping is honoured. Under order 1
 * the adaptive relaxation never engages (sbmbp_get_relaxation reports (0, -1, 1, 1)) and field_mix of sbmbp_set_schedule /
 * sbmbp_set_learning_schedule and sbmbp_set_gather_mode are ignored; sbmbp_stats counts coloured sweeps in sweeps and
 * edge_msg_updates, never in psi_form_sweeps, and sweep_kernel_ms covers a coloured sweep's whole launch sequence.
 * SBMBP_ERR_UNSUPPORTED: Q > 16, shard engines (so the multi-GPU driver sbmbp_dist_* always sweeps synchronously). */
int sbmbp_coloured_plan(const sbmbp_graph_t *g, const uint32_t *colour_in, double step_fraction, uint32_t *n_colours,
                        uint32_t *n_steps, uint32_t *colour, uint32_t *step);
int sbmbp_set_sweep_order(sbmbp_engine_t *e, int order, const uint32_t *colour, double step_fraction);
int sbmbp_get_sweep_order(const sbmbp_engine_t *e, int *order, uint32_t *n_colours, uint32_t *n_steps);

/* converge (belief_propagation.cpp:386-415): returns in *niter the 0-based index of the first sweep
 * whose max |delta message| < crit, or -1 after max_sweeps. damping == dumping_rate. */
int sbmbp_converge(sbmbp_engine_t *e, double crit, uint32_t max_sweeps, double damping, int *niter,
                   double *last_maxdiff);
/* exactly n_sweeps synchronous sweeps, no convergence test (benchmarking / stepping) */
int sbmbp_sweep(sbmbp_engine_t *e, double damping, uint32_t n_sweeps, double *last_maxdiff);

/* compute_free_energy (belief_propagation.cpp:744-750) = -f_site + f_edge + f_nonedge;
 * parts = {f_site, f_edge, f_nonedge} (:442-504, :562-612, :675-709). The non-edge term is exact
 * (tiled N^2 kernel) for N <= the exact limit, else the moment series of DESIGN.md section 4, whose order is
 * capped at 4 (Q <= 8), 3 (Q = 9..16) and 2 (Q = 17..64): where the cap is reached (silently) the error is
 * N (w/N)^(K+1) / (2(K+1)) at the cap, not 1e-12 (measured at N = 4e4, c = 10: 3e-11 at Q = 12, 1e-7 at Q = 32). */
int sbmbp_free_energy(sbmbp_engine_t *e, double *f, double *parts /* 3 or NULL */);
/* compute_entropy (belief_propagation.cpp:752-758); NaN for deg_corr_flag != 0 as the reference */
int sbmbp_entropy(sbmbp_engine_t *e, double *entropy, double *parts /* 3 or NULL */);
/* nonedge_mode: 0 = automatic, 1 = force exact N^2, 2 = force series; series_order 0 = automatic */
int sbmbp_set_nonedge_mode(sbmbp_engine_t *e, int nonedge_mode, int series_order);

/* compute_na_expect + compute_cab_expect (belief_propagation.cpp:428-440, 892-989) */
int sbmbp_em_expectations(sbmbp_engine_t *e, double *na_expect, double *nna_expect, double *cab_expect);
/* confusion matrix C[a*Q+b] = sum_{i: true_i = a} psi_i[b] and compute_overlap (:775-811) */
int sbmbp_confusion(sbmbp_engine_t *e, double *C);
int sbmbp_overlap(sbmbp_engine_t *e, double *overlap);

/* inference (belief_propagation.cpp:77-99): converge, free energy, entropy, overlap */
typedef struct sbmbp_infer_result {
    double entropy, free_energy, overlap;
    int niter;
    double last_maxdiff;
} sbmbp_infer_result;
int sbmbp_inference(sbmbp_engine_t *e, float conv_crit, uint32_t time_conv, float dumping_rate,
                    sbmbp_infer_result *out);

/* learning + learning_step (belief_propagation.cpp:14-75): EM loop with the reference's stopping
 * rule (criterion shrinks by 0.1 whenever fdiff falls below it; -e is not used).
 * On return eta/cab hold what the reference prints (:48-49). status: 0 = ran out of steps,
 * 1 = "fdiff < learning_conv_crit", 2 = free energy became NaN/Inf. */
typedef struct sbmbp_learn_result {
    int em_steps;
    int status;
    double free_energy;
    double overlap;
    uint64_t total_sweeps;
} sbmbp_learn_result;
int sbmbp_learning(sbmbp_engine_t *e, float learning_conv_crit, uint32_t learning_max_time, float learning_rate,
                   float dumping_rate, sbmbp_learn_result *out);
/* Two schedule rules of the EM loop (no reference counterpart). field_mix: relaxation of the global
 * field inside the BP runs of the EM loop (default 0.3; the smaller of this and sbmbp_set_schedule's value is used; 1 =
 * plain Jacobi). snap: the integer truncation of the group sizes (belief_propagation.cpp:58-63) treats a value within
 * min(snap * N * learning_conv_crit, 0.01) BELOW an integer as that integer (default snap = 1; 0 = truncate exactly). */
int sbmbp_set_learning_schedule(sbmbp_engine_t *e, double field_mix, double snap);
/* host only, no device: one learning_step (belief_propagation.cpp:53-75 with the snap rule above); na / cab in and out.
 * Group i < Q - 1 becomes unsigned(int(learning_rate * na_expect[i] + (1 - learning_rate) * na[i] + s)) with
 * s = min(snap * n_vertices * crit, 0.01) (:58-63), the last group takes the rest (:64), and cab is mixed entry by entry
 * (:66-72). sbmbp_learning and sbmbp_batch_learning run exactly this function. */
int sbmbp_learning_step_host(uint32_t Q, uint32_t n_vertices, double learning_rate, double snap, double crit,
                             const double *na_expect, const double *cab_expect, uint32_t *na, double *cab);
/* host only, no device: which of n runs over one graph is best. Passes k = 0 .. n_ranks - 1 look at the runs with
 * rank[r] == k (a negative rank is never looked at) and the first pass with a candidate ends the search: its lowest free
 * energy wins, a NaN free energy is never best, ties go to the lowest index. No candidate at all: *best = 0.
 * sbmbp_batch_inference ranks converged runs 0 and the others 1; sbmbp_batch_learning ranks status 1 as 0, status 0 as 1. */
int sbmbp_best_replica(uint32_t n, const double *free_energy, const int *rank, int n_ranks, uint32_t *best);

/* counters for the metric "BP edge-message updates per second" */
typedef struct sbmbp_stats {
    uint64_t sweeps;             /* synchronous sweeps executed so far */
    uint64_t edge_msg_updates;   /* sweeps * E2 */
    double sweep_kernel_ms;      /* HIP-event time of the sweep kernels (sum) on the engine's stream */
    uint64_t sweep_launches;     /* sweeps timed: one event pair per sweep (under sweep order 1 around its whole launch sequence).
                                  * A shard times every chunk that has segments: the pairs of a call / n_chunks, rounded down */
    double bytes_per_sweep;      /* algorithmic bytes of one sweep */
    uint64_t device_bytes;       /* HBM held by this engine */
    uint32_t n_blocks;           /* workgroups of one sweep launch */
    uint32_t n_hub_rows;         /* rows above one segment's edge capacity: updated in fragments of 256 edges by launches of their own, not by the frame kernel */
    uint64_t psi_form_sweeps;    /* of `sweeps`, how many ran the marginal-gather form */
    uint64_t hub_edges;          /* directed edges of those rows (sweep_kernel_ms times the frame kernel: it moves the other edges) */
} sbmbp_stats;
int sbmbp_get_stats(sbmbp_engine_t *e, sbmbp_stats *out);
int sbmbp_reset_stats(sbmbp_engine_t *e);
/* when on, every sweep launch is bracketed by HIP events on the engine's stream (bench.py) */
int sbmbp_set_timing(sbmbp_engine_t *e, int on);

/* ---------------------------------------------------------------------------------------------
 * Replica batches: R independent BP runs over ONE graph on one GPU (csrc/kernels_batch.h). No reference counterpart: the
 * reference runs one state per process. BP on a block model is multistable, so it is run from several starts and the fixed
 * point of lowest free energy is kept; a batch uploads the CSR once and advances all replicas with one launch sequence per
 * sweep. Every replica has its own initial state, its own (cab, na, beta) and its own convergence and adaptive-relaxation
 * state: replica r stops at its own sweep and keeps the state of that sweep, exactly as a single engine with
 * sbmbp_set_gather_mode(e, 1) started from the same state would.
 * Layout in HBM (replica-major): messages [2][R][E2][Q-1], marginals [2][R][N][Q], parameter blocks [R], sweep records
 * [R][n_segments][Q+1].
 * Supported: Q = 2 .. 16, deg_corr_flag 0 / 1 / 2, zeros in cab, clamped rows, rows of any degree, damping, beta; the
 * synchronous sweep order in the message-gather form and, through sbmbp_batch_set_sweep_order, the coloured order. Refused
 * with SBMBP_ERR_UNSUPPORTED: Q > 16. A batch has no shard form and no marginal-gather form (there are no entry points
 * that would select them).
 * SBMBP_ERR_ARG: n_replicas = 0 or above 65535 (the replica is the second grid dimension), Q < 2, a replica index >= R.
 * SBMBP_ERR_NOMEM: R (2 E2 (Q-1) + 2 N Q) 8 bytes of state do not fit the free HBM. Argument errors are reported before
 * any device work; without a GPU the call returns SBMBP_ERR_NODEVICE as sbmbp_create does.
 * The calls mirror the single-engine ones (same reference citations); arrays over replicas have R leading entries.
 * ------------------------------------------------------------------------------------------- */
typedef struct sbmbp_batch sbmbp_batch_t;
int sbmbp_batch_create(sbmbp_batch_t **out, const sbmbp_graph_t *g, uint32_t Q, uint32_t deg_corr_flag, uint32_t n_replicas, int device);
void sbmbp_batch_destroy(sbmbp_batch_t *b);
uint32_t sbmbp_batch_num_replicas(const sbmbp_batch_t *b);
/* replica r is bit for bit what sbmbp_init_messages produces with seeds[r]; conf / true_conf / conditional are common */
int sbmbp_batch_init_messages(sbmbp_batch_t *b, uint32_t flag, const int32_t *conf, const uint32_t *true_conf,
                              const uint32_t *seeds /* R */, int conditional);
int sbmbp_batch_init_messages_device(sbmbp_batch_t *b, const uint64_t *seeds /* R */, const uint32_t *true_conf);
/* replica = -1: all replicas */
int sbmbp_batch_set_params(sbmbp_batch_t *b, int replica, const double *cab, const uint32_t *na, double beta);
int sbmbp_batch_get_params(sbmbp_batch_t *b, uint32_t replica, double *cab, uint32_t *na, double *beta /* each may be NULL */);
int sbmbp_batch_set_state(sbmbp_batch_t *b, uint32_t replica, const double *psi, const double *msg_out);
int sbmbp_batch_get_state(sbmbp_batch_t *b, uint32_t replica, double *psi, double *msg_out);
int sbmbp_batch_get_field(sbmbp_batch_t *b, uint32_t replica, double *h /* Q */);
/* Per-vertex label priors of a batch. Every replica is in one of three states: NONE, SHARED (it reads the batch's one shared
 * table) or OWN (a table of its own). prior: N*Q doubles as sbmbp_set_vertex_prior takes them, or NULL.
 *   replica = -1, table: every replica becomes SHARED with this table, which is stored ONCE in HBM whatever R is; every own
 *                        table is freed (mirrors sbmbp_batch_set_params(b, -1, ...))
 *   replica = -1, NULL:  every replica becomes NONE and all tables are freed
 *   replica = r, table:  replica r becomes OWN (this overrides the shared table for r)
 *   replica = r, NULL:   replica r becomes NONE
 * A table means for its replica exactly what sbmbp_set_vertex_prior documents for the single engine: it multiplies eta_q in
 * the marginal, in every message sent and in the exact cavity fallback, and in the site terms of the free energy and of the
 * entropy; it is not in h, the edge terms, the non-edge terms or the EM numerators; a zero forbids a label exactly; clamped
 * rows ignore it; it is stored as given. The tables belong to the batch like the graph: they survive
 * sbmbp_batch_init_messages*, sbmbp_batch_set_params and sbmbp_batch_set_state; setting or removing one drops what the batch
 * caches about the replica's state. sbmbp_batch_learning and sbmbp_batch_em_step hold the priors fixed and apply the
 * reference's rules unchanged. One use is a semi-supervised run from R starts (one shared table); another is R folds of a
 * label hold-out, or one graph under R annotation sets, from one launch sequence (own tables).
 * Two consequences:
 * - While some replicas hold a table and others do not, those without one are advanced by the prior kernels over ONE table of
 *   ones that the batch keeps (allocated on first need, N Q 8 bytes, freed when no replica or every replica holds a table).
 *   Such a replica goes through the states of a single engine with an all-ones prior, bit for bit; that is the no-prior run
 *   up to rounding (1e-13), not to the bit. A batch in which no replica holds a table launches exactly what it launches
 *   without this call.
 * - Scaling a row by c moves the free energy by -log(c)/N. *best of sbmbp_batch_inference / sbmbp_batch_learning compares
 *   free energies as they are, so it compares like with like only among replicas that read the same table.
 * bytes_per_sweep of sbmbp_batch_get_stats (one replica's) grows by 8 Q N while any replica holds a table; device_bytes
 * counts every table.
 * Errors, before any device work: SBMBP_ERR_ARG for a replica index outside -1 .. R-1 and for a bad row (a negative, NaN or
 * Inf entry, no positive entry; the message names the vertex, and the replica when one was given); SBMBP_ERR_NOMEM for a
 * table that does not fit, which leaves the batch as it was.
 * sbmbp_batch_get_vertex_prior: *present = 0 NONE, 1 SHARED, 2 OWN; when it is not 0 the table is copied into prior (N*Q, or
 * NULL). */
int sbmbp_batch_set_vertex_prior(sbmbp_batch_t *b, int replica, const double *prior /* N*Q, or NULL */);
int sbmbp_batch_get_vertex_prior(sbmbp_batch_t *b, uint32_t replica, double *prior /* N*Q or NULL */, int *present);
int sbmbp_batch_get_relaxation(const sbmbp_batch_t *b, uint32_t replica, int *field_level, int *generic_level, double *field_mix,
                               double *damping_factor);
/* common to all replicas */
int sbmbp_batch_set_schedule(sbmbp_batch_t *b, double field_mix, uint32_t check_every);
int sbmbp_batch_set_auto_relax(sbmbp_batch_t *b, int on);
int sbmbp_batch_set_nonedge_mode(sbmbp_batch_t *b, int nonedge_mode, int series_order);
/* Sweep order of the batch, common to all replicas (the colouring and the step tables belong to the graph). The arguments
 * mean what sbmbp_set_sweep_order's mean: order 0 = synchronous (default), 1 = coloured Gauss-Seidel; colour NULL = the
 * built-in greedy colouring, else N entries, validated; step_fraction 0 = default 1/8. The plan and the device tables are the
 * single engine's. Under order 1 sbmbp_batch_sweep / _converge / _inference / _em_step / _learning advance every replica by
 * the coloured launch sequence: per step one launch over (segments of the step, R) and one fold-and-update launch with a
 * workgroup per replica, plus the hub pair of every replica in steps that hold rows above a segment's capacity. Replica r
 * goes through the states of a single engine in the same order with the same step_fraction: in place on the buffer that
 * holds its state, so its stopping sweep, niter[r], last_maxdiff[r] (the maximum over the steps of the undamped 1-step
 * difference) and state are its own. No relaxation of any kind: sbmbp_batch_get_relaxation reports (0, -1, 1, 1) for every
 * replica while the order is 1; field_mix of sbmbp_batch_set_schedule / sbmbp_batch_set_learning_schedule and
 * sbmbp_batch_set_auto_relax are ignored; damping is honoured. Switching the order keeps every replica's state; going back to
 * order 0 keeps the tables. The sweep records of a replica grow to max(n_segments, records of the largest step) (Q + 1)
 * doubles when order 1 is set.
 * SBMBP_ERR_UNSUPPORTED: order 1 while a replica holds a per-vertex prior, and sbmbp_batch_set_vertex_prior with a table
 * while the order is 1 (the step kernels take no prior). SBMBP_ERR_ARG: b NULL, an order other than 0 / 1, an invalid
 * colouring. sbmbp_batch_get_sweep_order: as sbmbp_get_sweep_order (n_colours = n_steps = 0 under order 0). */
int sbmbp_batch_set_sweep_order(sbmbp_batch_t *b, int order, const uint32_t *colour, double step_fraction);
int sbmbp_batch_get_sweep_order(const sbmbp_batch_t *b, int *order, uint32_t *n_colours, uint32_t *n_steps);
/* exactly n_sweeps sweeps of every replica (never relaxed); last_maxdiff: R entries or NULL */
int sbmbp_batch_sweep(sbmbp_batch_t *b, double damping, uint32_t n_sweeps, double *last_maxdiff);
/* niter[r] / last_maxdiff[r]: sbmbp_converge's meaning for replica r alone. The call ends when every replica has stopped
 * or after max_sweeps; the host reads the R convergence states every check_every sweeps (one copy). */
int sbmbp_batch_converge(sbmbp_batch_t *b, double crit, uint32_t max_sweeps, double damping, int *niter /* R */,
                         double *last_maxdiff /* R */);
/* per replica, through the single engine's reduction kernels and host code on replica r's buffers */
int sbmbp_batch_free_energy(sbmbp_batch_t *b, double *f /* R */, double *parts /* 3 R or NULL */);
int sbmbp_batch_entropy(sbmbp_batch_t *b, double *entropy /* R */, double *parts /* 3 R or NULL */);
int sbmbp_batch_overlap(sbmbp_batch_t *b, double *overlap /* R */);
int sbmbp_batch_em_expectations(sbmbp_batch_t *b, uint32_t replica, double *na_expect, double *nna_expect, double *cab_expect);
/* inference of every replica; *best (may be NULL) = the replica of lowest free energy among those with niter >= 0, among
 * all when none converged; a NaN free energy is never best; ties go to the lowest index */
int sbmbp_batch_inference(sbmbp_batch_t *b, float conv_crit, uint32_t time_conv, float dumping_rate, sbmbp_infer_result *out /* R */,
                          uint32_t *best);
/* sweeps = sum over replicas of the sweeps actually executed, edge_msg_updates = sweeps * E2, psi_form_sweeps = 0;
 * bytes_per_sweep is one replica's (8 Q N more while any replica holds a prior table); the kernel-time fields are 0 */
int sbmbp_batch_get_stats(sbmbp_batch_t *b, sbmbp_stats *out);

/* Multi-start EM: belief_propagation::learning (belief_propagation.cpp:14-75) for every replica in lock-step rounds.
 * Round t: every replica still learning applies `if (fdiff < crit) crit *= 0.1` (:29-31) to its OWN criterion; ONE batched
 * BP run advances them all (per-replica criterion; replicas that have stopped learning are frozen: state, parity and
 * parameter block untouched); ONE launch sequence yields the reductions of all of them (kernels_batch.h) and one copy
 * brings them to the host, where each replica runs the stop tests (:38-45) or sbmbp_learning_step_host (:53-75).
 * Replica r goes through the states, parameters, em_steps, status and total_sweeps of a single engine in message-gather
 * form (sbmbp_set_gather_mode(e, 1)) with the same schedule started from its state and parameters, up to the summation
 * order of the reductions. SBMBP_ERR_STATE: a replica has no parameters or no state. */
int sbmbp_batch_set_learning_schedule(sbmbp_batch_t *b, double field_mix, double snap);   /* common to all replicas */
/* the reductions of one EM step for every replica from one launch sequence: na_expect / nna_expect R*Q, cab_expect R*Q*Q,
 * f R, parts 3R; any pointer may be NULL */
int sbmbp_batch_em_step(sbmbp_batch_t *b, double *na_expect, double *nna_expect, double *cab_expect, double *f, double *parts);
/* out[R]; eta R*Q and cab R*Q*Q as the reference prints them (:48-49); *best: lowest free energy among status 1, else
 * among status 0, a NaN free energy never, ties to the lowest index */
int sbmbp_batch_learning(sbmbp_batch_t *b, float learning_conv_crit, uint32_t learning_max_time, float learning_rate,
                         float dumping_rate, sbmbp_learn_result *out, double *eta, double *cab, uint32_t *best);

/* Agreement of replicas: how many different fixed points the starts of a batch found, which replicas are the same state up
 * to a relabelling of the groups, and whether the best run is an outlier. No reference counterpart.
 * A call takes a list of n replicas x = 0 .. n-1 of the batch; replicas == NULL means all R in index order.
 *   psi^x_i  = the marginal row of vertex i that sbmbp_batch_get_state(b, replicas[x], psi, NULL) would return at the time of the
 *              call: the table of the replica's current parity, in whichever sweep order it last ran, with or without priors
 *   l^x_i    = the label of the largest entry of that row; ties go to the lowest index, a NaN never wins, a row of NaNs gives 0
 * For every ordered pair (x, y) the Q x Q confusion matrix, by kind:
 *   SBMBP_AGREE_SOFT       C_xy[a][b] = sum_i psi^x_i[a] psi^y_i[b]
 *   SBMBP_AGREE_HARD_SOFT  C_xy[a][b] = sum_{i : l^x_i = a} psi^y_i[b]: compute_overlap's confusion (sbmbp_confusion) with the
 *                          labels of replica x as the true configuration
 *   SBMBP_AGREE_HARD       C_xy[a][b] = #{ i : l^x_i = a and l^y_i = b }: symmetric, exact (integer sums), overlap_xx = 1
 *   overlap_xy = max over ALL permutations pi of sum_a C_xy[a][pi(a)] / N, and perm_xy a maximising pi: label a of x
 *                corresponds to label pi(a) of y. Exact for every Q (maximum-weight assignment on the host, O(Q^3)); the
 *                identity rule above Q = 8 belongs to sbmbp_overlap, the overlap with the true configuration, which is unchanged.
 * The confusion matrices are ONE Gram matrix over the marginal tables where they lie in HBM (csrc/kernels_batch.h: k_agree, on
 * the matrix cores), folded without atomics: two calls return the same bits. The call reads the marginals and changes nothing:
 * not a replica's state, parity, stop flag or cached flags, no statistic (the buffers it allocates on first need are not in
 * device_bytes), not the engine's binding. It runs on the batch's stream behind whatever is queued.
 * Refused before any device work: SBMBP_ERR_ARG for a null batch, a kind outside 0 .. 2, n = 0 with a list, a listed replica
 * >= R or listed twice; SBMBP_ERR_UNSUPPORTED for n Q > 256 (pass a subset list); SBMBP_ERR_STATE for a listed replica
 * without a state.
 * sbmbp_agreement_groups: host only, no device. Replicas in ascending order: x joins the group of the FIRST earlier group leader
 * g with overlap[g n + x] >= threshold, else x becomes the leader of a new group; group[x] = the group's number in order of
 * creation. Deterministic, no linkage beyond the leaders (0-1 and 1-2 above the threshold and 0-2 below it: 2 leads a group).
 * Meant for kind HARD, where the overlap of a replica with itself is 1; any matrix is accepted. */
#define SBMBP_AGREE_SOFT 0
#define SBMBP_AGREE_HARD_SOFT 1
#define SBMBP_AGREE_HARD 2
int sbmbp_batch_agreement(sbmbp_batch_t *b, int kind, const uint32_t *replicas /* n, or NULL = all R */, uint32_t n,
                          double *confusion /* n*n*Q*Q: [((x*n + y)*Q + a)*Q + b], or NULL */,
                          double *overlap   /* n*n, or NULL */,
                          uint32_t *perm    /* n*n*Q: [(x*n + y)*Q + a] = pi(a), or NULL */);
int sbmbp_agreement_groups(uint32_t n, const double *overlap /* n*n */, double threshold,
                           uint32_t *group /* n */, uint32_t *n_groups);

/* ---------------------------------------------------------------------------------------------
 * Vertex-range sharding: the per-shard STEPS (one engine per GPU). No reference counterpart: the
 * reference is single-process. A shard owns a contiguous range of rows, their out-messages and
 * marginals; the marginals of remote neighbours ("halo") live behind the owned rows in the same
 * table, so nbr_local indexes one array, and the message records received for the cut edges sit
 * behind the own records of each message buffer, so rev_local does too. The caller of these steps is
 * the C++ multi-GPU driver further down (sbmbp_dist_*, csrc/dist.hip), which moves the data between
 * the shards itself over its RCCL communicators (sbmbp_comm_*): boundary marginals (marginal-gather
 * sweep) or cut-edge messages (message-gather sweep) once per sweep, the Q+1 reduction values by one
 * all-gather. Every sweep form of the single engine runs sharded: damping, clamped rows,
 * deg_corr_flag 2, zeros in cab take the message-gather sweep. The device buffers named in the
 * descriptor are owned by the caller (the driver) so that its collectives can address them.
 * ------------------------------------------------------------------------------------------- */
typedef struct sbmbp_shard_desc {
    uint32_t n_global;          /* vertices of the whole graph (field scaling, eta) */
    uint32_t n_own;             /* rows owned by this shard */
    uint32_t n_halo;            /* remote vertices whose marginals this shard reads */
    uint32_t row0;              /* global id of the first owned row */
    uint64_t n_edges;           /* directed edges leaving the owned rows */
    uint64_t edge0;             /* global index of the first owned directed edge (device RNG stream) */
    const uint64_t *row_ptr;    /* host [n_own+1], local offsets */
    const uint32_t *nbr_local;  /* host [n_edges]: index into the marginal table: own < n_own <= halo */
    void *psi_buf0, *psi_buf1;  /* device, (n_own+n_halo)*Q doubles each */
    void *red_buf;              /* device, >= SBMBP_RED_GATHER_OFFSET + n_ranks * SBMBP_FOLD_ROWS * 17 doubles (and >= 8192):
                                   reduction hand-off buffer */
    uint32_t n_chunks;          /* row chunks for overlapping the halo exchange with the sweep (0 or 1 = none) */
    const uint32_t *chunk_row;  /* host [n_chunks+1] local row boundaries, chunk_row[0] = 0, last = n_own */
    /* optional: what the message-gather sweep needs on a shard (any damping, clamped rows, deg_corr_flag 2, zeros in cab) */
    const uint32_t *rev_local;  /* host [n_edges] or NULL: record holding the reverse message of every edge: < n_edges for an own
                                   neighbour, n_edges + r for the r-th record received from the peers */
    uint64_t n_halo_msgs;       /* records received from the peers, kept behind the own records of each message buffer */
    const uint32_t *table_deg;  /* host [n_own + n_halo] or NULL: degree of every vertex of the marginal table (deg_corr_flag 2) */
} sbmbp_shard_desc;

typedef struct sbmbp_conv_state {
    double maxdiff; /* of the last executed sweep: the 1-step message difference if last_exact, else the 2-step hint */
    int conv_iter;  /* first sweep whose 1-step difference fell below the criterion, or -1 */
    int sweep_idx;  /* sweeps executed since sbmbp_shard_begin */
    int stop;       /* queued sweeps after the trigger were skipped */
    int last_exact;
    int pause;      /* with stop: adaptive relaxation asked for damping; answer with sbmbp_shard_resume and go on in the
                       message-gather form from sweep_idx */
    int ar_field_level, ar_generic_level; /* levels of the adaptive relaxation (sbmbp_get_relaxation) */
} sbmbp_conv_state;

int sbmbp_shard_create(sbmbp_engine_t **out, const sbmbp_shard_desc *desc, uint32_t Q, uint32_t deg_corr_flag, int device);
/* start a run of sweeps: uploads parameters and the convergence criterion (< 0: never converges). The sweeps report
 * 2-step hints until one falls below 8 * crit; from then on they report the reference's 1-step difference and the
 * device-side stop flag works on it (all on the device: no host round trip) */
int sbmbp_shard_begin(sbmbp_engine_t *e, double crit, int hinted /* 1: the run uses the marginal-gather sweep */);
/* planted configuration and true labels of the owned rows (init_messages, belief_propagation.cpp:106-108, 132-216);
 * any_clamp_global: some vertex of the WHOLE graph is clamped (every shard must take the same kernel variants) */
int sbmbp_shard_set_labels(sbmbp_engine_t *e, const int32_t *conf_local, const uint32_t *true_conf_local, uint32_t flag,
                           int conditional, int any_clamp_global);
/* 0: every cab entry > 0; 1: clamped rows exist; 2: they hold the one-hot state of init flag 1/3; 3: the state is the device
 * initialisation (message = sender's marginal); 4: the shard has a reverse index */
int sbmbp_shard_query(sbmbp_engine_t *e, int what);
/* message-gather form of sweep j over all owned rows (k_sweep: belief_propagation.cpp:991-1071 as the single engine runs
 * it). The incoming messages of the cut edges are the records behind the own ones of the buffer sweep j reads:
 * sbmbp_shard_msg_halo(e, j) is where the caller receives them (n_halo_msgs records of Q-1 doubles, in rev_local's
 * numbering) and sbmbp_shard_pack_msgs gathers the records it has to send from the same buffer. */
int sbmbp_shard_sweep_explicit(sbmbp_engine_t *e, uint32_t j, double damping);
void *sbmbp_shard_msg_halo(sbmbp_engine_t *e, uint32_t j);
int sbmbp_shard_pack_msgs(sbmbp_engine_t *e, uint32_t j, const uint32_t *d_edge_idx, uint32_t n, double *d_out);
/* where the reductions below take the incoming messages from: 0 = materialised from the marginal table (needs marginals
 * consistent with the messages and cab > 0), 1 = gathered through rev_local (the caller received the halo records of the
 * current buffer, sbmbp_shard_msg_halo(e, 0)) */
int sbmbp_shard_set_incoming(sbmbp_engine_t *e, int source);
/* gather rows idx[0..n) of the marginal table that sweep j READS into out (device pointers), ncomp
 * components per row: Q, or Q-1 to ship the marginals without their last component (they sum to 1) */
int sbmbp_shard_pack(sbmbp_engine_t *e, uint32_t j, const uint32_t *d_idx, uint32_t n, double *d_out, uint32_t ncomp);
/* expand n received (staged) rows of ncomp components into the halo rows d_halo_row[0..n) (each < n_halo) of the
 * table sweep j reads */
int sbmbp_shard_unpack(sbmbp_engine_t *e, uint32_t j, const double *d_in, const uint32_t *d_halo_row, uint32_t n, uint32_t ncomp);
/* Fused exchange buffers (optional; without this call every sweep needs sbmbp_shard_pack before and sbmbp_shard_unpack
 * after the exchange). snd_ptr[n_own+1] / snd_slot[snd_ptr[n_own]] (host, copied): the rows of d_sendbuf (ncomp
 * components each) that ship the marginal of every own row. d_stage0/1: receive buffers of halo table 0/1, n_halo rows of
 * ncomp components in halo order. With them sbmbp_shard_sweep_chunk writes each new marginal of the chunk into its send
 * slots and gathers halo marginals of the table it reads from the matching receive buffer; the halo ROWS of the marginal
 * tables are then only refreshed by sbmbp_shard_unpack (needed before the reductions, not between sweeps). */
int sbmbp_shard_set_io(sbmbp_engine_t *e, const uint32_t *snd_ptr, const uint32_t *snd_slot, double *d_sendbuf,
                       const double *d_stage0, const double *d_stage1, uint32_t ncomp);
/* which of the two marginal buffers sweep j reads (0/1); the other one is written */
int sbmbp_shard_read_buffer(sbmbp_engine_t *e, uint32_t j);
/* red[0..Q) = sum over owned rows of g_i psi_i of the buffer sweep j reads (field initialisation) */
int sbmbp_shard_field_partial(sbmbp_engine_t *e, uint32_t j);
/* sweep j over the owned rows; red[0..Q) = partial sums of the new marginals, red[Q] = hint */
int sbmbp_shard_sweep_partial(sbmbp_engine_t *e, uint32_t j);
/* the same in pieces: sweep j over row chunk c only (the caller ships chunk c's new marginals while chunk c+1 runs), then
 * ONE fold launch of all chunks' partials into SBMBP_FOLD_ROWS rows at red[0..): the caller all-gathers those rows of every
 * rank behind red + SBMBP_RED_GATHER_OFFSET and sbmbp_shard_finalize folds them (n_rows = n_ranks * SBMBP_FOLD_ROWS) */
int sbmbp_shard_sweep_chunk(sbmbp_engine_t *e, uint32_t j, uint32_t c);
/* the same on another HIP stream of the engine's device (the caller orders it against the engine's stream with events):
 * consecutive chunks on alternating streams overlap each other's tail */
int sbmbp_shard_sweep_chunk_on(sbmbp_engine_t *e, uint32_t j, uint32_t c, void *hip_stream);
int sbmbp_shard_sweep_fold(sbmbp_engine_t *e);
#define SBMBP_FOLD_ROWS 64          /* rows of (Q+1) doubles sbmbp_shard_sweep_fold leaves at red[0..) */
#define SBMBP_RED_GATHER_OFFSET 2048 /* > SBMBP_FOLD_ROWS * 17 (sharded engines: Q <= 16): gathered rows never overlap a shard's own rows */
/* consume the reduction values: n_rows rows of (Q+1) doubles starting at red + SBMBP_RED_GATHER_OFFSET (the caller
 * all-gathers every shard's red[0..Q] there; n_rows = number of shards). Rows are folded in order —
 * sums for the Q field entries, max for the hint. mode 0 after a sweep, 1 field initialisation */
int sbmbp_shard_finalize(sbmbp_engine_t *e, int mode, uint32_t n_rows, int md_exact /* the sweep was a message-gather sweep */);
/* red[0] = max |m_a - m_b| over the two message buffers of this shard (exact 1-step criterion) */
int sbmbp_shard_msgdiff_partial(sbmbp_engine_t *e);
/* red[0..2Q+Q*Q) = na_expect, nna_expect, confusion sums over the owned rows (current marginals) */
int sbmbp_shard_rowsums_partial(sbmbp_engine_t *e);
/* Reductions at compute_* time (belief_propagation.cpp:744-758, 428-440, 892-989) on shards: each
 * *_partial leaves this shard's sums in red, the caller all-reduces (SUM) the stated number of doubles,
 * *_finish turns them into the reference's quantities on the host. Incoming messages are first
 * materialised from the marginal table (whose halo must be current) and the previous own messages.
 * The non-edge term uses the moment series (the exact all-pairs kernel would need every marginal). */
int sbmbp_shard_fe_partial(sbmbp_engine_t *e, int want_entropy);                 /* all-reduce red[0..5) */
int sbmbp_shard_fe_finish(sbmbp_engine_t *e, double *out /* f_site, f_edge, e_site, e_edge */);
int sbmbp_shard_nonedge_partial(sbmbp_engine_t *e, int want_entropy, uint32_t *n_values, int *order);
int sbmbp_shard_nonedge_finish(sbmbp_engine_t *e, int want_entropy, int order, double *out /* f_nonedge, e_nonedge */);
/* exact non-edge term for small graphs: d_psi_all = marginals of ALL vertices, global row order (device); leaves 4 doubles
 * in red (all-pairs f/e over (own i, every l), adjacent f/e): all-reduce, then f = (red[0]-red[2])/2N, e = (red[1]-red[3])/2N */
int sbmbp_shard_nonedge_exact_partial(sbmbp_engine_t *e, const double *d_psi_all, int want_entropy);
int sbmbp_shard_em_partial(sbmbp_engine_t *e, uint32_t *n_values);
int sbmbp_shard_em_finish(sbmbp_engine_t *e, double *na_expect, double *nna_expect, double *cab_expect);

/* wait for the stream and read the convergence state */
int sbmbp_shard_poll(sbmbp_engine_t *e, sbmbp_conv_state *out);
/* the same without idling the GPU: record queues a copy of the state into page-locked slot 0/1 behind the work queued so far,
 * wait blocks until that copy has landed (the caller may queue the next batch in between) */
int sbmbp_shard_state_record(sbmbp_engine_t *e, int slot);
int sbmbp_shard_state_wait(sbmbp_engine_t *e, int slot, sbmbp_conv_state *out);
int sbmbp_shard_resume(sbmbp_engine_t *e);
/* after a poll: `executed` sweeps of the queued batch really ran; flips the buffer parities */
int sbmbp_shard_commit(sbmbp_engine_t *e, uint32_t executed);
/* ---------------------------------------------------------------------------------------------
 * Multi-GPU: communicators and the per-rank driver (csrc/dist.hip). No reference counterpart; this is what replaces the
 * call sequence of main.cpp:318-365 when the graph is sharded over the GPUs of one node. One sbmbp_dist_t = one rank = one
 * GPU = one host thread. The ranks of a run are processes (one per GPU; they share a communicator id) or threads of one
 * process (bin/bp --gpus N). All ranks hold the whole host graph and make the same calls in the same order; every
 * convergence decision is taken on the device from identical all-gathered values, so no rank ever needs to be told.
 * Per sweep: the boundary marginals travel by grouped ncclSend/ncclRecv over xGMI while the next row chunk is swept, then
 * ONE all-gather of Q+1 doubles per rank (field sums + message difference). The message-gather sweep (damping, clamped
 * rows, deg_corr_flag 2, zeros in cab, first sweep after a state or parameter change) ships the messages of the cut edges
 * instead. Results are partition invariant up to the summation order of the Q field sums.
 * ------------------------------------------------------------------------------------------- */
typedef struct sbmbp_comm sbmbp_comm_t;
typedef struct sbmbp_dist sbmbp_dist_t;
#define SBMBP_COMM_ID_BYTES 256
/* RCCL: rank 0 draws an id (two ncclUniqueId: one communicator for the halo exchange, one for the reductions) and hands it
 * to the other ranks by whatever means the launcher has (torch.distributed in bench.py, shared memory between threads) */
int sbmbp_comm_unique_id(void *id_out /* SBMBP_COMM_ID_BYTES */);
int sbmbp_comm_init_rank(sbmbp_comm_t **out, const void *id, int n_ranks, int rank, int device);
/* the ranks are n threads of this process (possibly sharing one GPU, where RCCL refuses duplicate devices): fills out[0..n),
 * one handle per rank thread. Tests and rehearsals. */
int sbmbp_comm_init_local(sbmbp_comm_t **out, int n_ranks);
/* the ranks are processes with the caller's own transport between them (e.g. gloo): buffers are staged through host memory.
 * Rows for / from peer p are contiguous, in rank order; every function returns 0 on success. Rehearsals on a 1-GPU box. */
typedef struct sbmbp_comm_callbacks {
    void *user;
    int (*exchange)(void *user, const double *send, const uint64_t *send_rows, double *recv, const uint64_t *recv_rows, int row_doubles);
    int (*allgather)(void *user, const double *in, uint64_t n, double *out /* n_ranks * n */);
    int (*allreduce)(void *user, double *buf, uint64_t n, int op /* 0 sum, 1 max */);
} sbmbp_comm_callbacks;
int sbmbp_comm_init_callbacks(sbmbp_comm_t **out, int n_ranks, int rank, const sbmbp_comm_callbacks *cb);
/* measurement only: rank `rank` of an n-rank plan alone on the GPU; exchanges deliver nothing, every peer "reports" this
 * rank's reduction values (tools/shard_budget.py: what one rank of the 8-GPU run executes per sweep) */
int sbmbp_comm_init_null(sbmbp_comm_t **out, int n_ranks, int rank);
void sbmbp_comm_destroy(sbmbp_comm_t *c);
/* a rank that gives up (an error outside a collective) tells its peers, so that none of them blocks waiting for it: the
 * in-process transport fails every later collective of the group (it also times out after SBMBP_LOCAL_TIMEOUT_S, default
 * 600 s), RCCL communicators are aborted (ncclCommAbort) */
void sbmbp_comm_abort(sbmbp_comm_t *c);
int sbmbp_comm_rank(const sbmbp_comm_t *c);
int sbmbp_comm_size(const sbmbp_comm_t *c);
const char *sbmbp_comm_transport(const sbmbp_comm_t *c); /* "rccl" | "local" | "callbacks" */

typedef struct sbmbp_dist_info_t {
    int rank, world;
    uint32_t n_global, row0, n_own, n_halo, n_chunks, halo_components;
    uint64_t n_edges, e2_global, n_halo_msgs;
    uint64_t sent_rows_per_sweep, busiest_peer_rows; /* marginal rows shipped per marginal-gather sweep */
} sbmbp_dist_info_t;

/* the shard of rank sbmbp_comm_rank(comm): plan (row range balanced on sum(deg+2), halo, send lists, cut edges), device
 * buffers, shard engine. g is borrowed and must outlive the engine (as the adjacency must in the reference,
 * belief_propagation.h:27). n_chunks = 0: default (4, or SBMBP_SHARD_CHUNKS; 1 for a single rank). */
int sbmbp_dist_create(sbmbp_dist_t **out, sbmbp_comm_t *comm, const sbmbp_graph_t *g, uint32_t Q, uint32_t deg_corr_flag, int device,
                      uint32_t n_chunks);
void sbmbp_dist_destroy(sbmbp_dist_t *d);
int sbmbp_dist_info(const sbmbp_dist_t *d, sbmbp_dist_info_t *out);
int sbmbp_dist_peer_rows(const sbmbp_dist_t *d, uint64_t *send_rows /* [world] or NULL */, uint64_t *recv_rows);
/* the calls below mirror the single-engine ones above (same reference citations); conf / true_conf are the GLOBAL vectors */
int sbmbp_dist_init_messages(sbmbp_dist_t *d, uint32_t flag, const int32_t *conf, const uint32_t *true_conf, uint32_t seed,
                             int conditional);
int sbmbp_dist_init_messages_device(sbmbp_dist_t *d, uint64_t seed, const uint32_t *true_conf);
int sbmbp_dist_set_state(sbmbp_dist_t *d, const double *psi_own /* n_own*Q */, const double *msg_own /* n_edges*Q */);
int sbmbp_dist_get_state(sbmbp_dist_t *d, double *psi_own, double *msg_own);
int sbmbp_dist_gather_marginals(sbmbp_dist_t *d, double *psi_all /* n_global*Q, filled on every rank */);
int sbmbp_dist_set_params(sbmbp_dist_t *d, const double *cab, const uint32_t *na, double beta);
int sbmbp_dist_get_params(sbmbp_dist_t *d, double *cab, uint32_t *na);
int sbmbp_dist_set_schedule(sbmbp_dist_t *d, double field_mix, uint32_t check_every);
int sbmbp_dist_set_learning_schedule(sbmbp_dist_t *d, double field_mix, double snap);
int sbmbp_dist_set_gather_mode(sbmbp_dist_t *d, int mode);
int sbmbp_dist_set_auto_relax(sbmbp_dist_t *d, int on);
int sbmbp_dist_get_relaxation(const sbmbp_dist_t *d, int *field_level, int *generic_level);
int sbmbp_dist_converge(sbmbp_dist_t *d, double crit, uint32_t max_sweeps, double damping, int *niter, double *last_maxdiff);
int sbmbp_dist_sweep(sbmbp_dist_t *d, double damping, uint32_t n_sweeps, double *last_maxdiff);
int sbmbp_dist_free_energy(sbmbp_dist_t *d, double *f, double *parts);
int sbmbp_dist_entropy(sbmbp_dist_t *d, double *entropy, double *parts);
int sbmbp_dist_em_expectations(sbmbp_dist_t *d, double *na_expect, double *nna_expect, double *cab_expect);
int sbmbp_dist_confusion(sbmbp_dist_t *d, double *C);
int sbmbp_dist_overlap(sbmbp_dist_t *d, double *overlap);
int sbmbp_dist_inference(sbmbp_dist_t *d, float conv_crit, uint32_t time_conv, float dumping_rate, sbmbp_infer_result *out);
int sbmbp_dist_learning(sbmbp_dist_t *d, float learning_conv_crit, uint32_t learning_max_time, float learning_rate, float dumping_rate,
                        sbmbp_learn_result *out);
int sbmbp_dist_get_stats(sbmbp_dist_t *d, sbmbp_stats *out); /* kernel times and bytes are this rank's; sweeps are the run's */
int sbmbp_dist_reset_stats(sbmbp_dist_t *d);
int sbmbp_dist_set_timing(sbmbp_dist_t *d, int on);
/* while timing is on: mean ms per marginal-gather sweep on this rank's compute stream spent in {chunk kernels (with whatever
 * exchange time they could not hide), fold + all-gather + finalize, waiting for exchanges still in flight} */
int sbmbp_dist_phase_times(sbmbp_dist_t *d, double ms_per_sweep[3], uint64_t *n_sweeps);
/* the plan without a device (tests, dry runs) */
int sbmbp_plan_summary(const sbmbp_graph_t *g, int world, int rank, uint32_t n_chunks, sbmbp_dist_info_t *info, uint64_t *send_rows,
                       uint64_t *recv_rows, uint64_t *msg_rows);
int sbmbp_plan_arrays(const sbmbp_graph_t *g, int world, int rank, uint32_t n_chunks, uint32_t *nbr_local, uint32_t *halo_global,
                      uint32_t *chunk_row, uint64_t *send_counts_cp, uint64_t *recv_counts_cp, uint32_t *send_idx_chunked,
                      uint32_t *snd_ptr, uint32_t *snd_slot, uint32_t *rev_local, uint32_t *msg_send_edge);

#ifdef __cplusplus
}
#endif
#endif /* SBMBP_H */
