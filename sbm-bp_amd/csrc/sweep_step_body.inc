// The body of one step of the coloured sweep order: THE definition of k_sweep_step (kernels.h) and k_sweep_step_batch
// (kernels_batch.h), which include this file between their braces. Not a header: no guard, no namespace, and it reads the
// kernel's parameters by name:
//     row_ptr rev nbr ndeg clamp rows loff seg_row0 seg_base dc damp     both kernels
//     P M psi                                                            parameters of k_sweep_step; the batch kernel forms
//                                                                        them per replica in the hooks below
// M and psi are read AND written through unqualified pointers (no __restrict__) in both: see the head of k_sweep_step.
// The including kernel defines the hooks before the include and undefines them after it (k_sweep_step: all empty but the last):
//     STEP_REPLICA   after tid: the replica and its P
//     STEP_M         behind the uniform exits and the row tables, before phase 1: M, the replica's current message buffer
//     STEP_PSI       before phase 2: psi, the replica's current marginal table
//     STEP_RECORD    an expression: where the segment's (Q + 1)-record goes
// A textual include and not a __device__ function, for the reason given at the head of sweep_msg_body.inc.
    constexpr int EPT = frame_cfg<Q>::EPT, CAP = frame_cfg<Q>::CAP, RCAP = frame_cfg<Q>::RCAP, TPB = frame_cfg<Q>::TPB;
    __shared__ double sb[CAP * Q];      // b_e[q] of every edge of the segment
    __shared__ double sA[RCAP * Q];     // unnormalised marginal of every row
    __shared__ uint32_t srp[RCAP + 1];  // edge offsets of the rows relative to the segment
    __shared__ uint32_t sbase[RCAP];    // row_ptr of every row
    __shared__ uint32_t sid[RCAP];      // vertex of every row
    __shared__ uint16_t srow[CAP];      // row (within segment) of every edge
    __shared__ uint8_t sfl[RCAP];       // 1 = clamped row
    __shared__ double sred[frame_cfg<Q>::WAVES * (Q + 1)];
    __shared__ int sbig;                // the segment holds a row above BIG_ROW edges

    const int tid = threadIdx.x;
    STEP_REPLICA
    if (P->stop) return;  // stopped run or replica: uniform exit before any barrier
    const uint32_t b = seg_base + blockIdx.x;
    const uint32_t l0 = seg_row0[b];
    const int nrows = int(seg_row0[b + 1] - l0);
    const uint32_t *lo = loff + size_t(l0) + b;
    const int ne = (nrows >= 0 && nrows <= RCAP) ? int(lo[nrows]) : CAP + 1;
    if (nrows > RCAP || ne > CAP) return;  // never with the host's tables (uniform): nothing is indexed beyond the LDS arrays
    if (tid == 0) sbig = 0;
    for (int r = tid; r <= nrows; r += TPB) srp[r] = lo[r];
    for (int r = tid; r < nrows; r += TPB) {
        const uint32_t i = rows[l0 + r];
        sid[r] = i;
        sbase[r] = row_ptr[i];
        sfl[r] = (clamp != nullptr && clamp[i] != -1) ? 1 : 0;
    }
    __syncthreads();
    for (int r = tid; r < nrows; r += TPB) {
        const int es = int(srp[r]), ee = int(srp[r + 1]);
        if (ee - es > BIG_ROW) sbig = 1;
        for (int e = es; e < ee; ++e) srow[e] = uint16_t(r);
    }
    __syncthreads();
    STEP_M

    // ---- phase 1: lane per directed edge: own old message kept, incoming message gathered, b = W^T m -> LDS
    double mo[EPT][Q];
    uint32_t kk[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int le = j * TPB + tid;
        kk[j] = 0u;
#pragma unroll
        for (int q = 0; q < Q; ++q) mo[j][q] = 0.0;
        if (le < ne) {
            const int r = srow[le];
            kk[j] = sbase[r] + (uint32_t(le) - srp[r]);
            const uint32_t rk = rev[kk[j]];
            double mi[Q];
            load_msg<Q>(M, size_t(kk[j]), mo[j]);
            load_msg<Q>(M, size_t(rk), mi);
            double didl = 0.0;
            if (DC2) didl = double(srp[r + 1] - srp[r]) * double(ndeg[nbr[kk[j]]]);
            double bv[Q];
            edge_field<Q, DC2>(P, mi, didl, bv);
            store_vec<Q>(&sb[le * Q], bv);
        }
    }
    __syncthreads();
    STEP_PSI

    // ---- phase 2: lane per row (a wave per row above BIG_ROW edges), as k_sweep; the marginal is replaced in place and
    //      its change enters the field sums
    double Sacc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) Sacc[q] = 0.0;
    auto finish_row = [&](int r, double di, double (&A)[Q], const int *ae, const double *ft = nullptr) {
        double pv[Q], pold[Q];
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
        double *prow = psi + size_t(sid[r]) * Q;
#pragma unroll
        for (int q = 0; q < Q; ++q) pold[q] = prow[q];
#pragma unroll
        for (int q = 0; q < Q; ++q) { pv[q] = A[q] * inv; Sacc[q] += gi * (pv[q] - pold[q]); }
#pragma unroll
        for (int q = 0; q < Q; ++q) prow[q] = pv[q];
    };
    for (int r = tid; r < nrows; r += TPB) {
        const int es = int(srp[r]), ee = int(srp[r + 1]);
        if (!sfl[r] && ee - es <= BIG_ROW) {  // (clamped rows keep marginal and out-messages, bp.cpp:1115-1124)
            double A[Q], ft[Q];
            const bool tab = dc != 0 && ee - es <= FT_D;
            if (tab) load_vec<Q>(P->ftab + size_t(ee - es) * QMAX, ft);
#pragma unroll
            for (int q = 0; q < Q; ++q) A[q] = 1.0;
            for (int e = es; e < ee; ++e) {
                double bv[Q];
                load_vec<Q>(&sb[e * Q], bv);
#pragma unroll
                for (int q = 0; q < Q; ++q) A[q] *= bv[q];
                rescale_pow2<Q>(A);
            }
            finish_row(r, double(ee - es), A, nullptr, tab ? ft : nullptr);
        }
    }
    if (sbig)  // uniform: written before the barrier that precedes phase 1
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

    // ---- phase 3: lane per directed edge: cavity, normalise, damp, store over the own old message
    double md = 0.0;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int le = j * TPB + tid;
        if (le < ne) {
            const int r = srow[le];
            if (sfl[r]) continue;
            double A[Q], bv[Q], cav[Q], out[Q];
            load_vec<Q>(&sA[r * Q], A);
            load_vec<Q>(&sb[le * Q], bv);
            bool ok = true;
            double tot = 0.0;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                cav[q] = A[q] / bv[q];
                ok = ok && (bv[q] > 0.0) && (cav[q] <= 1.7e308);
                tot += cav[q];
            }
            if (!ok) {  // exact cavity product when a division is unusable (b == 0 or overflow)
                const int es = int(srp[r]), ee = int(srp[r + 1]);
                int ce[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) { cav[q] = 1.0; ce[q] = 0; }
                for (int e = es; e < ee; ++e) {
                    if (e == le) continue;
#pragma unroll
                    for (int q = 0; q < Q; ++q) cav[q] *= sb[e * Q + q];
                    x_norm<Q>(cav, ce);
                }
                tot = apply_field_x<Q>(P, dc, double(ee - es), cav, ce);
            }
            const double inv = 1.0 / tot;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const double nv = cav[q] * inv;
                out[q] = damp * nv + (1.0 - damp) * mo[j][q];
                md = nanmax(md, fabs(mo[j][q] - nv));  // against the undamped value (bp.cpp:1059-1063)
            }
            store_msg<Q>(M, size_t(kk[j]), out);
        }
    }
    block_reduce_store<Q, frame_cfg<Q>::WAVES>(Sacc, md, sred, STEP_RECORD);
