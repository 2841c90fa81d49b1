// Replica batches: R independent BP states over ONE graph, advanced by one launch sequence per sweep (gfx950).
//
// BP on a block model is multistable, so it is run from several starts (or at several parameter points) over the same
// graph. The batch keeps the graph tables once and the states replica-major in HBM:
//     messages  [2][R][E2][Q-1]      marginals [2][R][N][Q]      dev_params P[R]      sweep records [R][n_segments][Q+1]
// Replica r reads P[r]: its own cab / eta / beta, field, convergence state and adaptive-relaxation ladder. The sweep is the
// synchronous sweep in the message-gather form with k_sweep's equations (kernels.h), built from the same device helpers;
// blockIdx.y is the replica, so the segment tables (row offsets, rev, under dc 2 nbr / ndeg) are read by R workgroups
// that run side by side and share them in L2. A replica whose stop flag is set returns before any barrier: it costs an
// empty workgroup and its state stays where its last sweep left it.
#ifndef SBMBP_KERNELS_BATCH_H
#define SBMBP_KERNELS_BATCH_H

#include "kernels.h"

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
// ------------------------------------------------------------------------------------------------
template <int Q, bool DC2>
__global__ void __launch_bounds__(frame_cfg<Q>::TPB) __attribute__((amdgpu_waves_per_eu(sweep_waves<Q>::N)))
k_sweep_batch(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ rev, const uint32_t *__restrict__ nbr,
              const uint32_t *__restrict__ ndeg /* degree of every row (DC2 only) */, const int32_t *__restrict__ clamp,
              const uint32_t *__restrict__ blk_row, const uint32_t *__restrict__ blk_e0, double *__restrict__ Mall, double *__restrict__ psi_all,
              const dev_params *__restrict__ Pall, double *__restrict__ rec_all, const int *__restrict__ par_all, size_t msg_stride,
              size_t psi_stride, size_t rec_stride, uint32_t R, uint32_t j, int dc, double damp) {
    constexpr int EPT = frame_cfg<Q>::EPT, CAP = frame_cfg<Q>::CAP, RCAP = frame_cfg<Q>::RCAP;
    __shared__ double sb[CAP * Q];     // b_e[q] of every edge of the segment
    __shared__ double sA[RCAP * Q];    // unnormalised marginal of every row
    __shared__ uint32_t srp[RCAP + 1]; // row offsets relative to the segment
    __shared__ uint16_t srow[CAP];     // row (within segment) of every edge
    __shared__ uint8_t sfl[RCAP];      // 1 = clamped row
    __shared__ double sred[frame_cfg<Q>::WAVES * (Q + 1)];
    __shared__ int sbig;               // the segment holds a row above BIG_ROW edges

    const int tid = threadIdx.x;
    const uint32_t rep = blockIdx.y;
    const dev_params *__restrict__ P = Pall + rep;
    const int stop = P->stop;
    const int par = par_all[rep];
    const uint32_t r0 = blk_row[blockIdx.x], r1 = blk_row[blockIdx.x + 1];
    const uint32_t e0 = blk_e0[blockIdx.x];
    const int nrows = int(r1 - r0), ne = int(blk_e0[blockIdx.x + 1] - e0);
    if (stop || ne > CAP) return;  // converged replica, or hub row (the fragment kernels own it): uniform exit before any barrier
    const int mc = (par + int(j)) & 1;
    // (the replica's other base pointers are formed where they are first needed, not held in scalar registers next to P's
    // matrices through the whole kernel)
    const double *__restrict__ Mold = Mall + (size_t(mc) * R + rep) * msg_stride;

    // ---- phase 1: lane per directed edge: gather incoming message, b = W^T m -> LDS
    constexpr int RPT = RCAP / frame_cfg<Q>::TPB + 1;
    double mo[EPT][Q];
    uint32_t rk[EPT], kk[EPT];
#pragma unroll
    for (int x = 0; x < EPT; ++x) {
        const int le = x * frame_cfg<Q>::TPB + tid;
        kk[x] = (ne > 0) ? e0 + uint32_t(le < ne ? le : 0) : 0u;
    }
#pragma unroll
    for (int x = 0; x < EPT; ++x) rk[x] = load_idx_stream(rev + kk[x]);
#pragma unroll
    for (int x = 0; x < EPT; ++x) load_msg_stream<Q>(Mold, kk[x], mo[x]);
    uint32_t rpv[RPT];
#pragma unroll
    for (int t = 0; t < RPT; ++t) { const int r = tid + t * frame_cfg<Q>::TPB; rpv[t] = row_ptr[r0 + uint32_t(r < nrows ? r : nrows)]; }
    double mi[EPT][Q];
#pragma unroll
    for (int x = 0; x < EPT; ++x) load_msg<Q>(Mold, rk[x], mi[x]);
    if (tid == 0) sbig = 0;
#pragma unroll
    for (int t = 0; t < RPT; ++t) { const int r = tid + t * frame_cfg<Q>::TPB; if (r <= nrows) srp[r] = rpv[t] - e0; }
    __syncthreads();  // srp visible
    for (int r = tid; r < nrows; r += frame_cfg<Q>::TPB) {
        const int es = int(srp[r]), ee = int(srp[r + 1]);
        if (ee - es > BIG_ROW) sbig = 1;
        for (int e = es; e < ee; ++e) srow[e] = uint16_t(r);
        sfl[r] = (clamp != nullptr && clamp[r0 + r] != -1) ? 1 : 0;
    }
    if (DC2) __syncthreads();  // per-edge weights need the edge -> row map
#pragma unroll
    for (int x = 0; x < EPT; ++x) {
        const int le = x * frame_cfg<Q>::TPB + tid;
        if (le < ne) {
            double didl = 0.0;
            if (DC2) {
                const int r = srow[le];
                const uint32_t l = nbr[e0 + le];
                didl = double(srp[r + 1] - srp[r]) * double(ndeg[l]);
            }
            double b[Q];
            edge_field<Q, DC2>(P, mi[x], didl, b);
            store_vec<Q>(&sb[le * Q], b);
        }
    }
    __syncthreads();

    // ---- phase 2: lane per row (a wave per row above BIG_ROW edges): psi_i = normalise(prod_e b_e * eta * F_i)
    const double *__restrict__ psi_old = psi_all + (size_t(mc) * R + rep) * psi_stride;
    double *__restrict__ psi = psi_all + (size_t(mc ^ 1) * R + rep) * psi_stride;
    double Sacc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) Sacc[q] = 0.0;
    auto finish_row = [&](int r, double di, double (&A)[Q], const int *ae /* per-component exponents of a long row, or null */,
                          const double *ft = nullptr /* the row's line of P->ftab, or null */) {
        double pv[Q];
        double tot;
        if (ae) {
            int x[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) x[q] = ae[q];
            tot = apply_field_x<Q>(P, dc, di, A, x);
        } else {
            tot = apply_field<Q>(P, dc, di, A, ft);
        }
        store_vec<Q>(&sA[r * Q], A);
        const double inv = 1.0 / tot;
        const double gi = dc ? di : 1.0;
#pragma unroll
        for (int q = 0; q < Q; ++q) { pv[q] = A[q] * inv; Sacc[q] += gi * pv[q]; }
        store_vec<Q>(psi + size_t(r0 + r) * Q, pv);
    };
    for (int r = tid; r < nrows; r += frame_cfg<Q>::TPB) {
        const int es = int(srp[r]), ee = int(srp[r + 1]);
        const double di = double(ee - es);
        if (sfl[r]) {  // clamped: marginal and out-messages stay as initialised
            double pv[Q];
            load_vec<Q>(psi_old + size_t(r0 + r) * Q, pv);
            store_vec<Q>(psi + size_t(r0 + r) * Q, pv);
            const double gi = dc ? di : 1.0;
#pragma unroll
            for (int q = 0; q < Q; ++q) Sacc[q] += gi * pv[q];
        } else if (ee - es <= BIG_ROW) {
            double A[Q], ft[Q];
            const bool tab = dc != 0 && ee - es <= FT_D;
            if (tab) load_vec<Q>(P->ftab + size_t(ee - es) * QMAX, ft);
#pragma unroll
            for (int q = 0; q < Q; ++q) A[q] = 1.0;
            for (int e = es; e < ee; ++e) {
                double b[Q];
                load_vec<Q>(&sb[e * Q], b);
#pragma unroll
                for (int q = 0; q < Q; ++q) A[q] *= b[q];
                rescale_pow2<Q>(A);
            }
            finish_row(r, di, A, nullptr, tab ? ft : nullptr);
        }
    }
    if (sbig)  // uniform: written before the barrier that ends phase 1
    for (int r = tid >> 6; r < nrows; r += frame_cfg<Q>::WAVES) {  // wave-uniform row index
        const int es = int(srp[r]), ee = int(srp[r + 1]);
        if (ee - es > BIG_ROW && !sfl[r]) {
            double A[Q];
            int ae[Q];
            row_product_wave<Q>(sb, es, ee, A, ae);
            if ((tid & 63) == 0) finish_row(r, double(ee - es), A, ae);
        }
    }
    __syncthreads();

    // ---- phase 3: lane per directed edge: cavity, normalise, damp, store
    double *__restrict__ Mnew = Mall + (size_t(mc ^ 1) * R + rep) * msg_stride;
    double md = 0.0;
    const int probe2 = P->ar_probe2;  // the probe sweep of the adaptive relaxation: |m^{t+1} - m^{t-1}| (m^{t-1} sits in the slot written below)
    damp *= P->damp_auto;
#pragma unroll
    for (int x = 0; x < EPT; ++x) {
        const int le = x * frame_cfg<Q>::TPB + tid;
        if (le < ne) {
            const int r = srow[le];
            double out[Q];
            if (sfl[r]) {
#pragma unroll
                for (int q = 0; q < Q; ++q) out[q] = mo[x][q];
            } else {
                double A[Q], b[Q], cav[Q];
                load_vec<Q>(&sA[r * Q], A);
                load_vec<Q>(&sb[le * Q], b);
                bool ok = true;
                double tot = 0.0;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    cav[q] = A[q] / b[q];
                    ok = ok && (b[q] > 0.0) && (cav[q] <= 1.7e308);
                    tot += cav[q];
                }
                if (!ok) {  // exact cavity product when a division is unusable (b == 0 or overflow)
                    const int es = int(srp[r]), ee = int(srp[r + 1]);
                    const double di = double(ee - es);
                    int ce[Q];
#pragma unroll
                    for (int q = 0; q < Q; ++q) { cav[q] = 1.0; ce[q] = 0; }
                    for (int e = es; e < ee; ++e) {
                        if (e == le) continue;
#pragma unroll
                        for (int q = 0; q < Q; ++q) cav[q] *= sb[e * Q + q];
                        x_norm<Q>(cav, ce);
                    }
                    tot = apply_field_x<Q>(P, dc, di, cav, ce);
                }
                const double inv = 1.0 / tot;
                double ref[Q];
                if (probe2) {  // uniform
                    load_msg<Q>(Mnew, size_t(e0 + le), ref);
                } else {
#pragma unroll
                    for (int q = 0; q < Q; ++q) ref[q] = mo[x][q];
                }
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const double nv = cav[q] * inv;
                    out[q] = damp * nv + (1.0 - damp) * mo[x][q];
                    md = nanmax(md, probe2 ? fabs(ref[q] - out[q]) / damp : fabs(ref[q] - nv));
                }
            }
            store_msg_stream<Q>(Mnew, size_t(e0 + le), out);
        }
    }
    block_reduce_store<Q, frame_cfg<Q>::WAVES>(Sacc, md, sred, rec_all + size_t(rep) * rec_stride + size_t(blockIdx.x) * (Q + 1));
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

// n_words 32-bit words from byte offset `off` of every P[r] -> out[r][n_words]: the convergence states of all replicas in
// one contiguous block, so that the host polls them with one copy
__global__ void __launch_bounds__(BLOCK)
k_batch_conv_states(const dev_params *__restrict__ P, uint32_t R, uint32_t off, uint32_t n_words, uint32_t *__restrict__ out) {
    for (uint32_t x = blockIdx.x * BLOCK + threadIdx.x; x < R * n_words; x += gridDim.x * BLOCK) {
        const uint32_t r = x / n_words, w = x - r * n_words;
        out[x] = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(P + r) + off)[w];
    }
}

}  // namespace sbmbp
#endif
