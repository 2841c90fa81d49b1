// The body of the frame pass of the free energy and the entropy: THE definition of k_fe_frame and of its twin under a
// per-vertex prior, k_fe_frame_prior (kernels.h), which include this file between their braces, as k_sweep and k_sweep_batch
// include sweep_msg_body.inc. Not a header: no guard, no namespace; it reads the kernel's parameters by name:
//     row_ptr rev nbr ndeg M Min blk_row blk_e0 P dc want_entropy partials
// Hook, defined by the including kernel before the include and undefined after it:
//     FE_SITE_FACTOR(i, v, x)   one more factor of row i's site products (log Z_i, and the entropy's C product) into (v, x)
//                               before the exponents are normalised: nothing in k_fe_frame, the row's prior line in the twin
    constexpr int EPT = frame_cfg<Q>::EPT, CAP = frame_cfg<Q>::CAP, RCAP = frame_cfg<Q>::RCAP;
    __shared__ double sb[CAP * Q];
    __shared__ double sc[CAP * Q];  // entropy: b with plain cab weights (no beta)
    __shared__ uint32_t srp[RCAP + 1];
    __shared__ uint16_t srow[CAP];
    __shared__ double sred[frame_cfg<Q>::WAVES * (FE_NP + 1)];
    const int tid = threadIdx.x;
    // as in the sweep kernels: segment bounds from one level of scalar loads, then every load of the lane-per-edge phase is
    // issued branch-free and back to back (reverse index, own record, row offsets, then the gathers) before anything waits
    const uint32_t r0 = blk_row[blockIdx.x], r1 = blk_row[blockIdx.x + 1];
    const int nrows = int(r1 - r0);
    const uint32_t e0 = blk_e0[blockIdx.x];
    const int ne = int(blk_e0[blockIdx.x + 1] - e0);
    double acc[FE_NP] = {0.0, 0.0, 0.0, 0.0};
    if (ne <= CAP) {
        constexpr int RPT = RCAP / frame_cfg<Q>::TPB + 1;
        uint32_t kk[EPT], rk[EPT], rpv[RPT];
        double mo_[EPT][Q], mi_[EPT][Q];
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int le = j * frame_cfg<Q>::TPB + tid;
            kk[j] = (ne > 0) ? e0 + uint32_t(le < ne ? le : 0) : 0u;
        }
        if (Min == nullptr) {  // uniform
#pragma unroll
            for (int j = 0; j < EPT; ++j) rk[j] = rev[kk[j]];
        }
#pragma unroll
        for (int j = 0; j < EPT; ++j) load_msg<Q>(M, size_t(kk[j]), mo_[j]);
#pragma unroll
        for (int t = 0; t < RPT; ++t) { const int r = tid + t * frame_cfg<Q>::TPB; rpv[t] = row_ptr[r0 + uint32_t(r < nrows ? r : nrows)]; }
#pragma unroll
        for (int j = 0; j < EPT; ++j) load_msg<Q>(Min ? Min : M, Min ? size_t(kk[j]) : size_t(rk[j]), mi_[j]);
#pragma unroll
        for (int t = 0; t < RPT; ++t) { const int r = tid + t * frame_cfg<Q>::TPB; if (r <= nrows) srp[r] = rpv[t] - e0; }
        __syncthreads();
        if (DC2) {  // per-edge weights need the edge -> row map
            for (int r = tid; r < nrows; r += frame_cfg<Q>::TPB)
                for (int e = int(srp[r]); e < int(srp[r + 1]); ++e) srow[e] = uint16_t(r);
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int le = j * frame_cfg<Q>::TPB + tid;
            if (le < ne) {
                double (&mi)[Q] = mi_[j];
                double (&mo)[Q] = mo_[j];
                double b[Q];
                double didl = 0.0;
                if (DC2) {
                    const int r = srow[le];
                    const uint32_t l = nbr[e0 + le];
                    didl = double(srp[r + 1] - srp[r]) * double(ndeg[l]);
                }
                edge_field<Q, DC2>(P, mi, didl, b);
                store_vec<Q>(&sb[le * Q], b);
                if (want_entropy) {
                    double c[Q];
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        double a = 0.0;
#pragma unroll
                        for (int t = 0; t < Q; ++t) a += P->cab[t * Q + q] * mi[t];
                        c[q] = a;
                    }
                    store_vec<Q>(&sc[le * Q], c);
                }
                double ln, en;
                edge_terms<Q, DC2>(P, mi, mo, didl, want_entropy, ln, en);
                acc[1] += ln;
                if (want_entropy) acc[3] += en;
            }
        }
        __syncthreads();
        for (int r = tid; r < nrows; r += frame_cfg<Q>::TPB) {
            const int es = int(srp[r]), ee = int(srp[r + 1]);
            const double di = double(ee - es);
            double A[Q];
            int ae[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) { A[q] = 1.0; ae[q] = 0; }
            for (int e = es; e < ee; ++e) {
#pragma unroll
                for (int q = 0; q < Q; ++q) A[q] *= sb[e * Q + q];
                if (((e - es) & 7) == 7) x_norm<Q>(A, ae);  // eight factors of O(W) stay far inside the double range
            }
            x_norm<Q>(A, ae);
            FE_SITE_FACTOR(r0 + uint32_t(r), A, ae)
            acc[0] += log_partition_x<Q>(P, dc, di, A, ae);  // log Z_i  (bp.cpp:446-502)
            if (want_entropy) {  // e_site (bp.cpp:506-560): no beta, weights exp(a + log eta - h/N)
                double C[Q];
                int ce[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) { C[q] = 1.0; ce[q] = 0; }
                for (int e = es; e < ee; ++e) {
#pragma unroll
                    for (int q = 0; q < Q; ++q) C[q] *= sc[e * Q + q];
                    if (((e - es) & 7) == 7) x_norm<Q>(C, ce);
                }
                x_norm<Q>(C, ce);
                FE_SITE_FACTOR(r0 + uint32_t(r), C, ce)
                acc[2] += entropy_site_x<Q>(P, C, ce);
            }
        }
    }
    block_reduce_store<FE_NP, frame_cfg<Q>::WAVES>(acc, 0.0, sred, partials + size_t(blockIdx.x) * (FE_NP + 1));
