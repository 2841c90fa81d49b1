// The body of the batched frame pass of an EM step: THE definition of k_em_frame_batch and of its twin under per-vertex
// priors, k_em_frame_batch_prior (kernels_batch.h), which include this file between their braces, as k_fe_frame and
// k_fe_frame_prior include fe_frame_body.inc. Not a header: no guard, no namespace; it reads the kernel's parameters by name:
//     row_ptr rev nbr ndeg blk_row blk_e0 Mall psi_all Pall par_all active mats_all msg_stride psi_stride R dc adj_mode
//     rec_rows partials
// Hook, defined by the including kernel before the include and undefined after it:
//     EM_SITE_FACTOR(i, v, x)   one more factor of row i's site product (log Z_i) into (v, x) before log_partition_x
//                               normalises the exponents: nothing in k_em_frame_batch, the line of row i in the table of
//                               replica `rep` in the twin (where FE_SITE_FACTOR sits in fe_frame_body.inc)
    constexpr int EPT = frame_cfg<Q>::EPT, CAP = frame_cfg<Q>::CAP, RCAP = frame_cfg<Q>::RCAP, TPB = frame_cfg<Q>::TPB, NW = frame_cfg<Q>::WAVES;
    constexpr int T = Q * (Q + 1) / 2, NP = em_np(Q), NRED = (EM && T > 2 * Q) ? T : 2 * Q;
    const uint32_t rep = blockIdx.y;
    if (!active[rep]) return;  // uniform, before any barrier
    __shared__ double sb[CAP * Q];
    __shared__ uint32_t srp[RCAP + 1];
    __shared__ uint16_t srow[CAP];
    __shared__ double sred[NW * NRED];
    __shared__ double ssc[3];
    const int tid = threadIdx.x;
    const dev_params *__restrict__ P = Pall + rep;
    const int par = par_all[rep];
    const double *__restrict__ M = Mall + (size_t(par) * R + rep) * msg_stride;
    const double *__restrict__ psi = psi_all + (size_t(par) * R + rep) * psi_stride;
    const double *__restrict__ mat = mats_all + size_t(rep) * 3 * Q * Q + (adj_mode == 2 ? Q * Q : 0);
    const double invN = P->invN;
    const uint32_t r0 = blk_row[blockIdx.x], r1 = blk_row[blockIdx.x + 1];
    const int nrows = int(r1 - r0);
    const uint32_t e0 = blk_e0[blockIdx.x];
    const int ne = int(blk_e0[blockIdx.x + 1] - e0);
    double *__restrict__ rec = partials + (size_t(rep) * rec_rows + blockIdx.x) * NP;
    double f_site = 0.0, f_edge = 0.0, f_adj = 0.0;
    double tri[T];  // the numerators (lane-per-edge phase; dead without EM)
#pragma unroll
    for (int u = 0; u < T; ++u) tri[u] = 0.0;
    double rs[2 * Q];  // na_expect, nna_expect (lane-per-row phase)
#pragma unroll
    for (int x = 0; x < 2 * Q; ++x) rs[x] = 0.0;
    if (ne > CAP) {  // hub row (uniform)
        const double di = double(ne);
        for (int le = tid; le < ne; le += TPB) {
            const uint32_t k = e0 + uint32_t(le);
            if (EM) {
                double mi[Q], mo[Q];
                load_msg<Q>(M, size_t(rev[k]), mi);
                load_msg<Q>(M, size_t(k), mo);
                em_edge_terms<Q, DC2>(P, mi, mo, DC2 ? di * double(ndeg[nbr[k]]) : 0.0, tri);
            }
            if (adj_mode) f_adj += adj_pair_term<Q>(psi, r0, nbr[k], mat, invN, adj_mode);
        }
        if (tid == 0) {
            double pv[Q];
            load_vec<Q>(psi + size_t(r0) * Q, pv);
#pragma unroll
            for (int q = 0; q < Q; ++q) { rs[q] = pv[q]; rs[Q + q] = di * pv[q]; }
        }
    } else {
        constexpr int RPT = RCAP / TPB + 1;
        uint32_t kk[EPT], rk[EPT], rpv[RPT];
        double mo_[EPT][Q], mi_[EPT][Q];
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int le = j * TPB + tid;
            kk[j] = (ne > 0) ? e0 + uint32_t(le < ne ? le : 0) : 0u;
        }
#pragma unroll
        for (int j = 0; j < EPT; ++j) rk[j] = rev[kk[j]];
#pragma unroll
        for (int j = 0; j < EPT; ++j) load_msg<Q>(M, size_t(kk[j]), mo_[j]);
#pragma unroll
        for (int t = 0; t < RPT; ++t) { const int r = tid + t * TPB; rpv[t] = row_ptr[r0 + uint32_t(r < nrows ? r : nrows)]; }
#pragma unroll
        for (int j = 0; j < EPT; ++j) load_msg<Q>(M, size_t(rk[j]), mi_[j]);
#pragma unroll
        for (int t = 0; t < RPT; ++t) { const int r = tid + t * TPB; if (r <= nrows) srp[r] = rpv[t] - e0; }
        __syncthreads();
        if (DC2 || adj_mode) {  // uniform: per-edge weights and the adjacent pairs need the edge -> row map
            for (int r = tid; r < nrows; r += TPB)
                for (int e = int(srp[r]); e < int(srp[r + 1]); ++e) srow[e] = uint16_t(r);
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int le = j * TPB + tid;
            if (le < ne) {
                double (&mi)[Q] = mi_[j];
                double (&mo)[Q] = mo_[j];
                double b[Q];
                double didl = 0.0;
                if (DC2) {
                    const int r = srow[le];
                    didl = double(srp[r + 1] - srp[r]) * double(ndeg[nbr[e0 + le]]);
                }
                edge_field<Q, DC2>(P, mi, didl, b);
                store_vec<Q>(&sb[le * Q], b);
                double ln, en;
                edge_terms<Q, DC2>(P, mi, mo, didl, 0, ln, en);
                f_edge += ln;
                if (EM) em_edge_terms<Q, DC2>(P, mi, mo, didl, tri);
                if (adj_mode) f_adj += adj_pair_term<Q>(psi, r0 + uint32_t(srow[le]), nbr[e0 + le], mat, invN, adj_mode);
            }
        }
    }
    // the lane-per-edge sums leave the registers here (the barriers inside also complete sb)
    if (EM) {
        block_sum_store<T, NW>(tri, sred, rec + EM_NA + 2 * Q);
    } else {
        for (int u = tid; u < T; u += TPB) rec[EM_NA + 2 * Q + u] = 0.0;  // k_em_edges_batch has them
        __syncthreads();
    }
    if (ne <= CAP) {  // uniform
        for (int r = tid; r < nrows; r += TPB) {
            const int es = int(srp[r]), ee = int(srp[r + 1]);
            const double di = double(ee - es);
            double A[Q];
            int ae[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) { A[q] = 1.0; ae[q] = 0; }
            for (int e = es; e < ee; ++e) {
#pragma unroll
                for (int q = 0; q < Q; ++q) A[q] *= sb[e * Q + q];
                if (((e - es) & 7) == 7) x_norm<Q>(A, ae);
            }
            x_norm<Q>(A, ae);
            EM_SITE_FACTOR(r0 + uint32_t(r), A, ae)
            f_site += log_partition_x<Q>(P, dc, di, A, ae);
            double pv[Q];
            load_vec<Q>(psi + size_t(r0 + r) * Q, pv);
#pragma unroll
            for (int q = 0; q < Q; ++q) { rs[q] += pv[q]; rs[Q + q] += di * pv[q]; }
        }
    }
    block_sum_store<2 * Q, NW>(rs, sred, rec + EM_NA);
    double sc[3] = {f_site, f_edge, f_adj};
    block_sum_store<3, NW>(sc, sred, ssc);
    if (tid == 0) {
        rec[0] = ssc[0]; rec[1] = ssc[1]; rec[2] = 0.0; rec[3] = 0.0; rec[4] = 0.0;
        rec[EM_ADJ] = ssc[2];
    }
