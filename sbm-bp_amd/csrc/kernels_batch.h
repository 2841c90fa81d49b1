// Replica batches: R independent BP states over ONE graph, advanced by one launch sequence per sweep (gfx950).
//
// BP on a block model is multistable, so it is run from several starts (or at several parameter points) over the same
// graph. The batch keeps the graph tables once and the states replica-major in HBM:
//     messages  [2][R][E2][Q-1]      marginals [2][R][N][Q]      dev_params P[R]      sweep records [R][n_segments][Q+1]
// Replica r reads P[r]: its own cab / eta / beta, field, convergence state and adaptive-relaxation ladder. The sweep is the
// synchronous sweep in the message-gather form, and it IS k_sweep's: both kernels include the one body in
// sweep_msg_body.inc, and k_sweep_batch adds only where replica r's buffers start;
// blockIdx.y is the replica, so the segment tables (row offsets, rev, under dc 2 nbr / ndeg) are read by R workgroups
// that run side by side and share them in L2. A replica whose stop flag is set returns before any barrier: it costs an
// empty workgroup and its state stays where its last sweep left it.
// The same holds below the sweep: every batch kernel here is the replica's addressing, a call of the single engine's
// __device__ rule in kernels.h (finalize_update, psi_row_add, em_edge_terms, moments_chunk, nonedge_pair_sums) and its
// own final store. The stores stay apart because block_sum_store and block_reduce_store fold in different orders.
// The coloured sweep order (sbmbp_batch_set_sweep_order) has the same shape: k_sweep_step_batch includes sweep_step_body.inc,
// the body of k_sweep_step, and k_step_finalize_batch calls step_update; the records are then [R][max(n_segments, records of
// the largest step)][Q+1].
// Per-vertex priors (sbmbp_batch_set_vertex_prior): k_sweep_batch_prior and k_em_frame_batch_prior are the twins of the two
// kernels whose row products a prior line enters, over the same bodies; they find the table of replica r in prior_tab[r].
#ifndef SBMBP_KERNELS_BATCH_H
#define SBMBP_KERNELS_BATCH_H

#include "kernels.h"
#include "kernels_wide.h"  // d4: the accumulator of v_mfma_f64_16x16x4_f64 (k_agree)

namespace sbmbp {

// where the replica states live (host side). The kernels take the fields as separate arguments: with the struct passed by
// value the sweep took up to 20 more vector registers than k_sweep (Q = 8, dc 0: 141 against 121); with separate
// arguments it takes k_sweep's.
struct batch_view {
    double *M;          // [2][R][msg_stride]
    double *psi;        // [2][R][psi_stride]
    dev_params *P;      // [R]
    double *rec;        // [R][rec_stride]: one (Q + 1)-record per segment and sweep
    const int *par;     // [R]: which of the two buffers held replica r's state when the current call started
    size_t msg_stride, psi_stride, rec_stride;  // doubles
    uint32_t R;
};

// ------------------------------------------------------------------------------------------------
// K1b: sweep j of the current call over segment blockIdx.x of replica blockIdx.y. Replicas stop at different sweeps, so
// the buffer a replica reads is its OWN parity par[r] moved on by j (a stopped replica executes nothing more in this call,
// so the sweeps it did execute were sweeps 0 .. sweep_idx - 1 of the call).
// The body is sweep_msg_body.inc, shared with k_sweep; the hooks below are all that is the batch's own. Included as text
// and not called as a function: see the head of that file.
// ------------------------------------------------------------------------------------------------
template <int Q, bool DC2>
__global__ void __launch_bounds__(frame_cfg<Q>::TPB) __attribute__((amdgpu_waves_per_eu(sweep_waves<Q>::N)))
k_sweep_batch(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ rev, const uint32_t *__restrict__ nbr,
              const uint32_t *__restrict__ ndeg /* degree of every row (DC2 only) */, const int32_t *__restrict__ clamp,
              const uint32_t *__restrict__ blk_row, const uint32_t *__restrict__ blk_e0, double *__restrict__ Mall, double *__restrict__ psi_all,
              const dev_params *__restrict__ Pall, double *__restrict__ rec_all, const int *__restrict__ par_all, size_t msg_stride,
              size_t psi_stride, size_t rec_stride, uint32_t R, uint32_t j, int dc, double damp) {
    // (the replica's base pointers are formed where they are first needed, not held in scalar registers next to P's
    // matrices through the whole kernel)
#define SWEEP_REPLICA                                    \
    const uint32_t rep = blockIdx.y;                     \
    const dev_params *__restrict__ P = Pall + rep;       \
    const int par = par_all[rep];
#define SWEEP_MOLD                                       \
    const int mc = (par + int(j)) & 1;                   \
    const double *__restrict__ Mold = Mall + (size_t(mc) * R + rep) * msg_stride;
#define SWEEP_PSI                                                                         \
    const double *__restrict__ psi_old = psi_all + (size_t(mc) * R + rep) * psi_stride;  \
    double *__restrict__ psi = psi_all + (size_t(mc ^ 1) * R + rep) * psi_stride;
#define SWEEP_MNEW double *__restrict__ Mnew = Mall + (size_t(mc ^ 1) * R + rep) * msg_stride;
#define SWEEP_RECORD rec_all + size_t(rep) * rec_stride + size_t(blockIdx.x) * (Q + 1)
#define SWEEP_ROW_START(r, v) _Pragma("unroll") for (int q = 0; q < Q; ++q) v[q] = 1.0;
#define SWEEP_ROW_FACTOR(r, v, x)
#include "sweep_msg_body.inc"
#undef SWEEP_REPLICA
#undef SWEEP_MOLD
#undef SWEEP_PSI
#undef SWEEP_MNEW
#undef SWEEP_RECORD
#undef SWEEP_ROW_START
#undef SWEEP_ROW_FACTOR
}

// K1bv: k_sweep_batch under per-vertex priors (sbmbp_batch_set_vertex_prior): the fourth includer of the body, with
// k_sweep_batch's replica hooks and k_sweep_prior's row hooks over the table of replica blockIdx.y. prior_tab[r] points to the
// table replica r reads: the batch's one shared table, the replica's own, or the batch's table of ones for a replica that holds
// none. Shared replicas read the same lines, so the R workgroups of a segment share them in L2 as they share the segment
// tables. The pointer is loaded where a row's line is first needed, not held in scalar registers through the kernel.
template <int Q, bool DC2>
__global__ void __launch_bounds__(frame_cfg<Q>::TPB) __attribute__((amdgpu_waves_per_eu(sweep_waves<Q>::N)))
k_sweep_batch_prior(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ rev, const uint32_t *__restrict__ nbr,
                    const uint32_t *__restrict__ ndeg /* degree of every row (DC2 only) */, const int32_t *__restrict__ clamp,
                    const uint32_t *__restrict__ blk_row, const uint32_t *__restrict__ blk_e0, double *__restrict__ Mall, double *__restrict__ psi_all,
                    const dev_params *__restrict__ Pall, double *__restrict__ rec_all, const int *__restrict__ par_all, size_t msg_stride,
                    size_t psi_stride, size_t rec_stride, uint32_t j, int dc, double damp,
                    const double *const *__restrict__ prior_tab /* [R]: tables of N*Q entries >= 0, a positive one in every row */) {
    // (R is the grid's second dimension and is read from there: with R as one more argument beside the table, four of the
    // thirty instantiations reserve 20 bytes of scratch, as three of k_sweep_batch's do; this way none has any)
#define SWEEP_REPLICA                                    \
    const uint32_t rep = blockIdx.y;                     \
    const uint32_t R = gridDim.y;                        \
    const dev_params *__restrict__ P = Pall + rep;       \
    const int par = par_all[rep];
#define SWEEP_MOLD                                       \
    const int mc = (par + int(j)) & 1;                   \
    const double *__restrict__ Mold = Mall + (size_t(mc) * R + rep) * msg_stride;
#define SWEEP_PSI                                                                         \
    const double *__restrict__ psi_old = psi_all + (size_t(mc) * R + rep) * psi_stride;  \
    double *__restrict__ psi = psi_all + (size_t(mc ^ 1) * R + rep) * psi_stride;
#define SWEEP_MNEW double *__restrict__ Mnew = Mall + (size_t(mc ^ 1) * R + rep) * msg_stride;
#define SWEEP_RECORD rec_all + size_t(rep) * rec_stride + size_t(blockIdx.x) * (Q + 1)
#define SWEEP_ROW_START(r, v) load_vec<Q>(prior_tab[rep] + size_t(r0 + uint32_t(r)) * Q, v);
#define SWEEP_ROW_FACTOR(r, v, x) { prior_factor<Q>(prior_tab[rep] + size_t(r0 + uint32_t(r)) * Q, v, x); }
#include "sweep_msg_body.inc"
#undef SWEEP_REPLICA
#undef SWEEP_MOLD
#undef SWEEP_PSI
#undef SWEEP_MNEW
#undef SWEEP_RECORD
#undef SWEEP_ROW_START
#undef SWEEP_ROW_FACTOR
}

// ------------------------------------------------------------------------------------------------
// K2b: workgroup r folds replica r's records in a fixed order and runs the update of k_finalize on P[r]: every replica
// carries its own stop flag, conv_iter, maxdiff, relaxation ladder, damp_auto and field mix (finalize_update, field_table).
// ------------------------------------------------------------------------------------------------
template <int Q>
__global__ void __launch_bounds__(BLOCK)
k_finalize_batch(dev_params *__restrict__ Pall, const double *__restrict__ rec_all, size_t rec_stride, uint32_t n_rec) {
    dev_params *__restrict__ P = Pall + blockIdx.x;
    if (P->stop) return;
    __shared__ double sacc[(BLOCK / 64) * (Q + 1)];
    __shared__ double sout[Q + 1];
    __shared__ double s_hN[Q];
    fold_rows<Q, false>(rec_all + size_t(blockIdx.x) * rec_stride, 0, n_rec, sacc, sout);
    if (threadIdx.x == 0) finalize_update<Q>(P, sout, 0, nullptr, 0u, 1, s_hN);
    __syncthreads();
    field_table<Q>(P, s_hN);
}

// ------------------------------------------------------------------------------------------------
// Coloured sweep order in a batch (sbmbp_batch_set_sweep_order). The colouring and the step tables belong to the graph, so
// all replicas walk the same steps; a step is ONE launch over (segments of the step, R).
// K1sb: k_sweep_step over segment seg_base + blockIdx.x of replica blockIdx.y, in place on the buffer that holds the
// replica's current state, par[r]: the coloured order never alternates buffers, so no sweep number enters the address and
// the host leaves the parity where it was. The body is sweep_step_body.inc, shared with k_sweep_step; M and psi are formed
// per replica where they are first needed, unqualified as there (read and written). R is the grid's second dimension and is
// read from there (see k_sweep_batch_prior). A stopped replica returns before any barrier and nothing of its state is touched.
// The replica's slot par[r] R + r is formed ONCE, at the top: with the parity loaded again at each of the two places that
// need it the kernel took 2 - 3 more vector registers than k_sweep_step from Q = 9 on (scalar registers spilled into them)
// and Q = 16 reserved 12 / 32 bytes of scratch where k_sweep_step has none (tools/kernel_resources.py).
// ------------------------------------------------------------------------------------------------
template <int Q, bool DC2>
__global__ void __launch_bounds__(frame_cfg<Q>::TPB) __attribute__((amdgpu_waves_per_eu(sweep_waves<Q>::N)))
k_sweep_step_batch(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ rev, const uint32_t *__restrict__ nbr,
                   const uint32_t *__restrict__ ndeg /* degree of every row (DC2 only) */, double *Mall, double *psi_all,
                   const int32_t *__restrict__ clamp, const uint32_t *__restrict__ rows, const uint32_t *__restrict__ loff,
                   const uint32_t *__restrict__ seg_row0, uint32_t seg_base, const dev_params *__restrict__ Pall,
                   const int *__restrict__ par_all, size_t msg_stride, size_t psi_stride, size_t rec_stride, int dc, double damp,
                   double *__restrict__ rec_all) {
#define STEP_REPLICA                                     \
    const uint32_t rep = blockIdx.y;                     \
    const dev_params *__restrict__ P = Pall + rep;       \
    const size_t slot = size_t(par_all[rep]) * gridDim.y + rep;
#define STEP_M double *M = Mall + slot * msg_stride;
#define STEP_PSI double *psi = psi_all + slot * psi_stride;
#define STEP_RECORD rec_all + size_t(rep) * rec_stride + size_t(blockIdx.x) * (Q + 1)
#include "sweep_step_body.inc"
#undef STEP_REPLICA
#undef STEP_M
#undef STEP_PSI
#undef STEP_RECORD
}

// K2sb: workgroup r folds replica r's n_rec records of the step in k_step_finalize's order and runs step_update on P[r]:
// every replica carries its own cs_md, maxdiff, conv_iter, sweep_idx and stop flag (no difference history in a batch)
template <int Q>
__global__ void __launch_bounds__(BLOCK)
k_step_finalize_batch(dev_params *__restrict__ Pall, const double *__restrict__ rec_all, size_t rec_stride, uint32_t n_rec, int last_step) {
    dev_params *__restrict__ P = Pall + blockIdx.x;
    if (P->stop) return;
    __shared__ double sacc[(BLOCK / 64) * (Q + 1)];
    __shared__ double sout[Q + 1];
    __shared__ double s_hN[Q];
    fold_rows<Q, false>(rec_all + size_t(blockIdx.x) * rec_stride, 0, n_rec, sacc, sout);
    if (threadIdx.x == 0) step_update<Q>(P, sout, last_step, nullptr, 0u, s_hN);
    __syncthreads();
    field_table<Q>(P, s_hN);
}

// n_words 32-bit words from byte offset `off` of every P[r] -> out[r][n_words]: the convergence states of all replicas in
// one contiguous block, so that the host polls them with one copy
__global__ void __launch_bounds__(BLOCK)
k_batch_conv_states(const dev_params *__restrict__ P, uint32_t R, uint32_t off, uint32_t n_words, uint32_t *__restrict__ out) {
    for (uint32_t x = blockIdx.x * BLOCK + threadIdx.x; x < R * n_words; x += gridDim.x * BLOCK) {
        const uint32_t r = x / n_words, w = x - r * n_words;
        out[x] = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(P + r) + off)[w];
    }
}

// ================================================================================================
// The reductions of one EM step for all replicas (sbmbp_batch_em_step, sbmbp_batch_learning): the replica is a grid
// dimension of every kernel, `active` [R] says which replicas take part (a mask argument, not the stop flag: a replica that
// has stopped SWEEPING is exactly the one whose reductions are wanted). A replica that is not active returns before any
// barrier. The state of replica r is the buffer par[r] (the host's parity, uploaded with the mask).
// ================================================================================================

// field refresh (k_psi_sum + k_finalize mode 2): chunk blockIdx.x of replica blockIdx.y -> partials[r][chunk][Q + 1]
template <int Q>
__global__ void __launch_bounds__(BLOCK)
k_psi_sum_batch(const uint32_t *__restrict__ row_ptr, const double *__restrict__ psi_all, const int *__restrict__ par_all,
                const int *__restrict__ active, size_t psi_stride, uint32_t R, uint32_t n_rows, uint32_t rows_per_blk, int dc,
                double *__restrict__ partials) {
    const uint32_t rep = blockIdx.y;
    if (!active[rep]) return;
    __shared__ double sred[4 * (Q + 1)];
    const double *__restrict__ psi = psi_all + (size_t(par_all[rep]) * R + rep) * psi_stride;
    double S[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) S[q] = 0.0;
    const uint32_t lo = blockIdx.x * rows_per_blk;
    const uint32_t hi = min(n_rows, lo + rows_per_blk);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += BLOCK) psi_row_add<Q>(row_ptr, psi, i, dc, S);
    block_reduce_store<Q>(S, 0.0, sred, partials + (size_t(rep) * gridDim.x + blockIdx.x) * (Q + 1));
}
// workgroup r: fold of replica r's chunks in a fixed order, then the exact field of P[r] (finalize_update mode 2)
template <int Q>
__global__ void __launch_bounds__(BLOCK)
k_field_refresh_batch(dev_params *__restrict__ Pall, const int *__restrict__ active, const double *__restrict__ partials, uint32_t n_part) {
    if (!active[blockIdx.x]) return;
    dev_params *__restrict__ P = Pall + blockIdx.x;
    __shared__ double sacc[(BLOCK / 64) * (Q + 1)];
    __shared__ double sout[Q + 1];
    __shared__ double s_hN[Q];
    fold_rows<Q, false>(partials + size_t(blockIdx.x) * n_part * (Q + 1), 0, n_part, sacc, sout);
    if (threadIdx.x == 0) finalize_update<Q>(P, sout, 2, nullptr, 0u, 0, s_hN);
    __syncthreads();
    field_table<Q>(P, s_hN);
}

// block sums of NS lane values -> out[0 .. NS) (no max slot), fixed order; sred holds NW * NS doubles and is free again
// after the closing barrier
template <int NS, int NW> __device__ __forceinline__ void block_sum_store(double (&s)[NS], double *sred, double *out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NS; ++q) s[q] = wave_sum(s[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NS; ++q) sred[wave * NS + q] = s[q];
    }
    __syncthreads();
    for (int q = threadIdx.x; q < NS; q += NW * 64) {
        double a = sred[q];
#pragma unroll
        for (int w = 1; w < NW; ++w) a += sred[w * NS + q];
        out[q] = a;
    }
    __syncthreads();
}

// Record of the batched frame pass, EM_NP(Q) doubles per segment (and per hub row behind the segments: k_fe_hub fills the
// FE_NP + 1 leading slots of those and zeroes the rest):
//   [0] sum log Z_i   [1] sum log(m_in^T W m_out)   [2..4] unused (entropy terms and max slot of k_fe_hub's record)
//   [5] adjacent pairs of the non-edge term (dc 0)   [6 .. 6+Q) na_expect   [6+Q .. 6+2Q) nna_expect   then Q(Q+1)/2 EM numerators
constexpr int EM_ADJ = FE_NP + 1, EM_NA = FE_NP + 2;
__host__ __device__ constexpr int em_np(int Q) { return EM_NA + 2 * Q + Q * (Q + 1) / 2; }
// the EM numerators stay in the frame pass up to this label count (Q (Q + 1) / 2 accumulators and as many terms per lane:
// tools/kernel_resources.py); above it k_em_edges_batch computes them
constexpr int EM_FRAME_QMAX = 8;

// per directed edge (i, l): adjacent-pair term of the non-edge sum. adj_mode 1: series form (k_nonedge_adj, mat = N (1 -
// (1 - cab/N)^beta)); 2: exact form (k_nonedge_exact_adj, mat = (1 - cab/N)^beta)
template <int Q>
__device__ __forceinline__ double adj_pair_term(const double *__restrict__ psi, uint32_t i, uint32_t l, const double *__restrict__ mat,
                                                double invN, int adj_mode) {
    double pi[Q], pl[Q];
    load_vec<Q>(psi + size_t(i) * Q, pi);
    load_vec<Q>(psi + size_t(l) * Q, pl);
    double y = 0.0;
#pragma unroll
    for (int q1 = 0; q1 < Q; ++q1) {
#pragma unroll
        for (int q2 = 0; q2 < Q; ++q2) y += mat[q1 * Q + q2] * (pi[q1] * pl[q2]);
    }
    if (adj_mode == 1) return log1p(-y * invN);
    return y != 0.0 ? log(y) : 0.0;
}

// ------------------------------------------------------------------------------------------------
// K3b: frame pass of the EM step over segment blockIdx.x of replica blockIdx.y: k_fe_frame's site and edge terms of the
// free energy, the adjacent pairs of the non-edge term (dc 0), the row sums na_expect / nna_expect and, with EM, the
// numerators of cab_expect. The numerators leave the registers (block_sum_store) before the lane-per-row phase starts, so
// they are never live together with the row sums.
// A hub row (a segment above CAP edges) has its site and edge terms from k_fe_hub; here its edges are walked by the whole
// workgroup for the adjacent pairs and the numerators, and lane 0 adds its row sums.
// The body is em_frame_body.inc, shared with the twin below; included as text, like the sweep's.
// ------------------------------------------------------------------------------------------------
template <int Q, bool DC2, bool EM>
__global__ void __launch_bounds__(frame_cfg<Q>::TPB)
k_em_frame_batch(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ rev, const uint32_t *__restrict__ nbr,
                 const uint32_t *__restrict__ ndeg, const uint32_t *__restrict__ blk_row, const uint32_t *__restrict__ blk_e0,
                 const double *__restrict__ Mall, const double *__restrict__ psi_all, const dev_params *__restrict__ Pall,
                 const int *__restrict__ par_all, const int *__restrict__ active, const double *__restrict__ mats_all /* [R][3 Q Q] */,
                 size_t msg_stride, size_t psi_stride, uint32_t R, int dc, int adj_mode, uint32_t rec_rows /* records per replica */,
                 double *__restrict__ partials) {
#define EM_SITE_FACTOR(i, v, x)
#include "em_frame_body.inc"
#undef EM_SITE_FACTOR
}

// K3v: k_em_frame_batch under per-vertex priors (sbmbp_batch_set_vertex_prior): the line of row i in the table of replica
// blockIdx.y is one more factor of the product log Z_i is formed from, as in k_fe_frame_prior. A nullable table argument in
// k_em_frame_batch itself was tried first and made it other code, so the twin: same body, other hook,
// and k_em_frame_batch is the code it was (tools/kernel_isa_diff.py). Hub rows take k_fe_hub_prior on the replica's table.
template <int Q, bool DC2, bool EM>
__global__ void __launch_bounds__(frame_cfg<Q>::TPB)
k_em_frame_batch_prior(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ rev, const uint32_t *__restrict__ nbr,
                       const uint32_t *__restrict__ ndeg, const uint32_t *__restrict__ blk_row, const uint32_t *__restrict__ blk_e0,
                       const double *__restrict__ Mall, const double *__restrict__ psi_all, const dev_params *__restrict__ Pall,
                       const int *__restrict__ par_all, const int *__restrict__ active, const double *__restrict__ mats_all /* [R][3 Q Q] */,
                       size_t msg_stride, size_t psi_stride, uint32_t R, int dc, int adj_mode, uint32_t rec_rows /* records per replica */,
                       double *__restrict__ partials, const double *const *__restrict__ prior_tab /* [R]: the table replica r reads */) {
#define EM_SITE_FACTOR(i, v, x) prior_factor<Q>(prior_tab[rep] + size_t(i) * Q, v, x);
#include "em_frame_body.inc"
#undef EM_SITE_FACTOR
}

// K5b: the EM numerators of k_em_edges for replica blockIdx.y (label counts above EM_FRAME_QMAX): grid-stride over the
// directed edges, partials[r][blockIdx.x][T]
template <int Q, bool DC2>
__global__ void __launch_bounds__(BLOCK)
k_em_edges_batch(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ rev, const uint32_t *__restrict__ nbr,
                 const uint32_t *__restrict__ ndeg, const uint32_t *__restrict__ src, const double *__restrict__ Mall,
                 const dev_params *__restrict__ Pall, const int *__restrict__ par_all, const int *__restrict__ active, size_t msg_stride,
                 uint32_t R, uint32_t n_edges, double *__restrict__ partials) {
    constexpr int T = Q * (Q + 1) / 2;
    const uint32_t rep = blockIdx.y;
    if (!active[rep]) return;
    __shared__ double sred[4 * T];
    const dev_params *__restrict__ P = Pall + rep;
    const double *__restrict__ M = Mall + (size_t(par_all[rep]) * R + rep) * msg_stride;
    double acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.0;
    for (uint32_t k = blockIdx.x * BLOCK + threadIdx.x; k < n_edges; k += gridDim.x * BLOCK) {
        double mi[Q], mo[Q];
        load_msg<Q>(M, size_t(rev[k]), mi);
        load_msg<Q>(M, size_t(k), mo);
        double didl = 0.0;
        if (DC2) {
            const uint32_t i = src[k], l = nbr[k];
            didl = double(row_ptr[i + 1] - row_ptr[i]) * double(ndeg[l]);
        }
        em_edge_terms<Q, DC2>(P, mi, mo, didl, acc);
    }
    block_sum_store<T, 4>(acc, sred, partials + (size_t(rep) * gridDim.x + blockIdx.x) * T);
}

// K4b with the replica as blockIdx.y: moment tensors of replica r's marginals, partials[r][blockIdx.x][T] (k_moments)
__global__ void __launch_bounds__(BLOCK)
k_moments_batch(const double *__restrict__ psi_all, const int *__restrict__ par_all, const int *__restrict__ active, size_t psi_stride,
                uint32_t R, uint32_t n_rows, int Q, int K, uint32_t rows_per_blk, int T, double *__restrict__ partials) {
    const uint32_t rep = blockIdx.y;
    if (!active[rep]) return;
    moments_chunk(psi_all + (size_t(par_all[rep]) * R + rep) * psi_stride, n_rows, Q, rows_per_blk, T,
                  partials + (size_t(rep) * gridDim.x + blockIdx.x) * T);
}

// K4x with the replica as blockIdx.z: log(psi_i^T P_r psi_l) over all ordered pairs of replica r (k_nonedge_exact without
// the entropy term), partials[r][blockIdx.y * gridDim.x + blockIdx.x]
template <int Q>
__global__ void __launch_bounds__(BLOCK)
k_nonedge_exact_batch(const double *__restrict__ psi_all, const int *__restrict__ par_all, const int *__restrict__ active,
                      const double *__restrict__ mats_all /* [R][3 Q Q]; P_r is the second matrix */, size_t psi_stride, uint32_t R,
                      uint32_t n, double *__restrict__ partials) {
    const uint32_t rep = blockIdx.z;
    if (!active[rep]) return;
    __shared__ double sl[BLOCK * Q];
    __shared__ double sred[4];
    const double *__restrict__ psi = psi_all + (size_t(par_all[rep]) * R + rep) * psi_stride;
    const double *__restrict__ Pmat = mats_all + size_t(rep) * 3 * Q * Q + Q * Q;
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t l0 = blockIdx.y * BLOCK;
    const uint32_t cnt = min(uint32_t(BLOCK), n - l0);
    for (uint32_t x = threadIdx.x; x < cnt * Q; x += BLOCK) sl[x] = psi[size_t(l0) * Q + x];
    __syncthreads();
    double acc[1] = {0.0}, no_entropy = 0.0;
    if (i < n) nonedge_pair_sums<Q>(psi, i, sl, cnt, Pmat, nullptr, 0.0, 0, acc[0], no_entropy);
    block_sum_store<1, 4>(acc, sred, partials + size_t(rep) * gridDim.x * gridDim.y + size_t(blockIdx.y) * gridDim.x + blockIdx.x);
}

// fold of [R][rows][cols] partials to out[r * out_stride + out_off + c], c < cols: replica blockIdx.y, one wave per column
// (lanes stride the rows, then the fixed shuffle tree of wave_sum): the order depends on nothing but the shape
__global__ void __launch_bounds__(BLOCK)
k_fold_batch(const double *__restrict__ in, const int *__restrict__ active, uint32_t rows, uint32_t cols, double *__restrict__ out,
             uint32_t out_stride, uint32_t out_off) {
    const uint32_t rep = blockIdx.y;
    if (!active[rep]) return;
    const uint32_t c = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (c >= cols) return;  // wave-uniform; no barrier below
    const double *__restrict__ p = in + size_t(rep) * rows * cols + c;
    double a = 0.0;
    for (uint32_t r = threadIdx.x & 63; r < rows; r += 64) a += p[size_t(r) * cols];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) out[size_t(rep) * out_stride + out_off + c] = a;
}

// ================================================================================================
// Agreement of replicas (sbmbp_batch_agreement): the Gram matrix G = X^T Y over the marginal tables of the n listed
// replicas. Rows = vertices, column c = x Q + q (listed replica x, label q), padded with zeros to CP = 16 ceil(n Q / 16) <= 256.
//   kind 0 (soft)       X = Y = Psi          kind 2 (hard)   X = Y = H, the one-hot image of l_i = argmax_q psi_i[q]
//   kind 1 (hard-soft)  X = H, Y = Psi       C_xy = the Q x Q block of G at (x Q, y Q)
// It is k_wem's shape of work (kernels_wide.h) with the vertices as the long axis, and k_wem's operand mapping of
// v_mfma_f64_16x16x4_f64: A: lane l holds X[vertex 4 step + (l >> 4)][16 at + (l & 15)], B: Y likewise with bt, C/D: lane l,
// register r = row (l >> 4) + 4 r, column l & 15.
// A workgroup walks trips of AG_V vertices (trip blockIdx.x, + gridDim.x, ...). Staging: the AG_V rows of listed replica x
// are AG_V Q consecutive doubles at (slot[x] psi_stride + v0 Q), slot[x] = parity R + replica; the flat index over (x, row,
// label) goes over the threads, so a wave reads consecutive addresses, with the streaming loads of the reductions, eight in
// flight per thread before the first is stored. The image is [vertex][column] with a row stride of S = CP or CP + 16 doubles,
// whichever is 16 mod 32: lanes l and l + 16 of an operand read (ds_read_b64: 64 banks of 4 bytes, conflicts inside a
// 32-lane half) then sit on opposite halves of the bank row. Columns >= n Q and vertices >= N are written as zeros on EVERY
// trip. The hard kinds keep no one-hot image: a byte per (vertex, replica) holds l_i (254 for a vertex >= N), and an operand
// is (label == the lane's q) ? 1 : 0 with the lane's (x, q) of every tile packed in a register before the first trip (a
// column >= n Q asks for label 255, which no row has). Ties go to the lowest label, a NaN never wins, a row of NaNs gives 0.
// Every wave owns the tiles wave + 4 u, u < TPW, of its workgroup's tile rows [blockIdx.y tile_rows, + tile_rows) in
// accumulators; the host picks TPW in {1, 4, 16} and tile_rows so that 4 TPW >= tile_rows CP / 16: one pass up to CP = 128,
// 2 .. 4 workgroup rows above, each of which stages the whole table again (from L2 / Infinity Cache).
// A workgroup writes its sums once: partials[blockIdx.x][CP][CP]; k_agree_fold adds them in index order. No atomics: two
// calls give the same bits. In kind 2 every term is 0 or 1, so the sums are exact whatever the order.
// ================================================================================================
constexpr int AG_V = 32, AG_TPB = 256, AG_MAXN = 128, AG_CPMAX = 256;
static_assert(AG_V % 4 == 0 && (AG_V & (AG_V - 1)) == 0, "a trip is whole MFMA steps; the staging shifts by log2(AG_V)");
__host__ __device__ constexpr uint32_t agree_row_stride(uint32_t CP) { return (CP & 16u) ? CP : CP + 16u; }
// dynamic LDS of k_agree: the image and the label bytes
__host__ __device__ constexpr size_t agree_lds_bytes(uint32_t CP, uint32_t n) { return size_t(AG_V) * agree_row_stride(CP) * 8 + size_t(AG_V) * ((n + 7u) & ~7u); }

template <int KIND, int TPW>
__global__ void __launch_bounds__(AG_TPB)
k_agree(const double *__restrict__ psi_all, const uint32_t *__restrict__ slot /* [n] */, size_t psi_stride, uint32_t N, uint32_t Q, uint32_t n,
        uint32_t tile_rows, double *__restrict__ partials) {
    extern __shared__ double ag_img[];  // [AG_V][S], then the labels [AG_V][LN]
    __shared__ uint32_t s_slot[AG_MAXN];
    constexpr bool HARD_A = KIND != 0, HARD_B = KIND == 2;
    const uint32_t nQ = n * Q, CT = (nQ + 15u) / 16u, CP = 16u * CT, S = agree_row_stride(CP), LN = (n + 7u) & ~7u;
    uint8_t *s_lab = reinterpret_cast<uint8_t *>(ag_img + size_t(AG_V) * S);
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, le = lane & 15u, g = lane >> 4;
    const uint32_t magic = ((1u << 20) + Q - 1u) / Q;  // m / Q == (m * magic) >> 20 for m < 65536, Q <= 16
    const uint32_t tr0 = blockIdx.y * tile_rows;
    const uint32_t n_tiles = min(tile_rows, CT - tr0) * CT;  // of this workgroup; the host keeps tr0 < CT

    // what the lane fetches for tile u: the image column, or (x << 8 | q) of its column for a hard operand
    auto key_of = [&](uint32_t col, bool hard) -> uint32_t {
        if (!hard) return col;
        if (col >= nQ) return 255u;
        const uint32_t x = (col * magic) >> 20;
        return (x << 8) | (col - x * Q);
    };
    uint32_t ka[TPW], kb[TPW];
    d4 acc[TPW];
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        const uint32_t t = min(wave + 4u * uint32_t(u), n_tiles - 1u), tr = t / CT;
        ka[u] = key_of(16u * (tr0 + tr) + le, HARD_A);
        kb[u] = key_of(16u * (t - tr * CT) + le, HARD_B);
        acc[u] = d4{0.0, 0.0, 0.0, 0.0};
    }
    for (uint32_t x = tid; x < n; x += AG_TPB) s_slot[x] = slot[x];

    const uint32_t total = uint32_t(AG_V) * nQ;  // doubles of a trip, flat over (x, row, label)
    const uint32_t n_trips = (N + AG_V - 1u) / AG_V;
    for (uint32_t trip = blockIdx.x; trip < n_trips; trip += gridDim.x) {
        const uint32_t v0 = trip * AG_V;
        __syncthreads();  // the trip before has been consumed (and s_slot is there)
        for (uint32_t f0 = tid; f0 < total; f0 += 8u * AG_TPB) {
            double val[8];
            uint32_t dst[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t f = f0 + uint32_t(k) * AG_TPB;
                val[k] = 0.0;
                dst[k] = ~0u;
                if (f < total) {
                    const uint32_t row = (f * magic) >> 20, x = row / AG_V, v = row % AG_V, q = f - row * Q;  // row = x AG_V + v
                    dst[k] = v * S + x * Q + q;
                    if (v0 + v < N) val[k] = __builtin_nontemporal_load(psi_all + size_t(s_slot[x]) * psi_stride + size_t(v0) * Q + (f - x * AG_V * Q));
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (dst[k] != ~0u) ag_img[dst[k]] = val[k];
        }
        if (!HARD_B)  // the image is an operand: its padding columns are zeros on every trip
            for (uint32_t z = tid; z < uint32_t(AG_V) * 16u; z += AG_TPB) {
                const uint32_t c = nQ + (z & 15u);
                if (c < CP) ag_img[(z >> 4) * S + c] = 0.0;
            }
        if (HARD_A) {
            __syncthreads();
            for (uint32_t p = tid; p < uint32_t(AG_V) * n; p += AG_TPB) {
                const uint32_t x = p / AG_V, v = p % AG_V;
                const double *row = ag_img + v * S + x * Q;
                uint32_t idx = 0;
                double best = row[0];
                if (best != best) best = -INFINITY;
                for (uint32_t q = 1; q < Q; ++q) {
                    const double w = row[q];
                    if (w > best) { best = w; idx = q; }
                }
                s_lab[v * LN + x] = uint8_t(v0 + v < N ? idx : 254u);
            }
        }
        __syncthreads();
#pragma unroll 2
        for (uint32_t step = 0; step < uint32_t(AG_V) / 4u; ++step) {
            const double *irow = ag_img + (4u * step + g) * S;
            const uint8_t *lrow = s_lab + (4u * step + g) * LN;
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                if (wave + 4u * uint32_t(u) < n_tiles) {  // wave-uniform
                    const double a = HARD_A ? (uint32_t(lrow[ka[u] >> 8]) == (ka[u] & 255u) ? 1.0 : 0.0) : irow[ka[u]];
                    const double b = HARD_B ? (uint32_t(lrow[kb[u] >> 8]) == (kb[u] & 255u) ? 1.0 : 0.0) : irow[kb[u]];
                    acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[u], 0, 0, 0);
                }
            }
        }
    }
    // C/D layout: lane l, register r: row (l >> 4) + 4 r of the tile, column l & 15
    double *__restrict__ out = partials + size_t(blockIdx.x) * CP * CP;
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        const uint32_t t = wave + 4u * uint32_t(u);
        if (t < n_tiles) {
            const uint32_t tr = t / CT, at = tr0 + tr, bt = t - tr * CT;
            const double v[4] = {acc[u].x, acc[u].y, acc[u].z, acc[u].w};
#pragma unroll
            for (int r = 0; r < 4; ++r) out[size_t(16u * at + g + 4u * uint32_t(r)) * CP + 16u * bt + le] = v[r];
        }
    }
}

// fold of the n_part partial tables in index order, one thread per entry of the n Q x n Q result, written in the layout
// of the interface: out[((x n + y) Q + a) Q + b]
__global__ void __launch_bounds__(BLOCK)
k_agree_fold(const double *__restrict__ partials, uint32_t n_part, uint32_t CP, uint32_t Q, uint32_t n, double *__restrict__ out) {
    const uint32_t nQ = n * Q, idx = blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= nQ * nQ) return;
    const uint32_t i = idx / nQ, j = idx - i * nQ;
    const double *__restrict__ p = partials + size_t(i) * CP + j;
    double s = 0.0;
    for (uint32_t k = 0; k < n_part; ++k) s += p[size_t(k) * CP * CP];
    const uint32_t x = i / Q, a = i - x * Q, y = j / Q, b = j - y * Q;
    out[((size_t(x) * n + y) * Q + a) * Q + b] = s;
}

}  // namespace sbmbp
#endif
