// The body of the synchronous message-gather sweep: THE definition of k_sweep, k_sweep_prior (kernels.h), k_sweep_batch and
// k_sweep_batch_prior (kernels_batch.h), which include this file between their braces. Not a header: no guard, no namespace, and it reads the
// kernel's parameters by name:
//     row_ptr rev nbr ndeg clamp blk_row blk_e0 dc damp          both kernels
//     P Mold Mnew psi_old psi                                    parameters of k_sweep; the batch kernel forms them per
//                                                                replica in the hooks below, where each is first needed
// The including kernel defines the hooks before the include and undefines them after it (k_sweep: all empty but the last):
//     SWEEP_REPLICA   after tid: the replica, its P and its parity
//     SWEEP_MOLD      behind the uniform exit: the buffer of this sweep and Mold in it
//     SWEEP_PSI       before phase 2: psi_old, psi
//     SWEEP_MNEW      before phase 3: Mnew
//     SWEEP_RECORD    an expression: where the segment's (Q + 1)-record goes
//     SWEEP_ROW_START(r, v)       phase 2, lane per row: v[Q] = the factor the product of row r starts from (all ones; the
//                                 row's prior line in k_sweep_prior, the line of the replica's table in
//                                 k_sweep_batch_prior), issued with the ftab line before the product loop
//     SWEEP_ROW_FACTOR(r, v, x)   behind a product with per-component exponents (the wave product of a row above BIG_ROW,
//                                 the exact cavity of phase 3): one more factor into (v, x) before apply_field_x normalises
//                                 the exponents (nothing; the row's prior line in k_sweep_prior)
// It is a textual include and not a __device__ function because the function form, inlined, is other code for this
// compiler in every instantiation (DESIGN.md section 8 has the register counts; tools/kernel_isa_diff.py compares builds).
    constexpr int EPT = frame_cfg<Q>::EPT, CAP = frame_cfg<Q>::CAP, RCAP = frame_cfg<Q>::RCAP;
    __shared__ double sb[CAP * Q];     // b_e[q] of every edge of the segment
    __shared__ double sA[RCAP * Q];    // unnormalised marginal of every row
    __shared__ uint32_t srp[RCAP + 1]; // row offsets relative to the segment
    __shared__ uint16_t srow[CAP];     // row (within segment) of every edge
    __shared__ uint8_t sfl[RCAP];      // 1 = clamped row
    __shared__ double sred[frame_cfg<Q>::WAVES * (Q + 1)];
    __shared__ int sbig;               // the segment holds a row above BIG_ROW edges

    // bounds and stop flag from one level of scalar loads; streams issued before the row offsets -> LDS fill
    const int tid = threadIdx.x;
    SWEEP_REPLICA
    const int stop = P->stop;
    const uint32_t r0 = blk_row[blockIdx.x], r1 = blk_row[blockIdx.x + 1];
    const uint32_t e0 = blk_e0[blockIdx.x];
    const int nrows = int(r1 - r0), ne = int(blk_e0[blockIdx.x + 1] - e0);
    if (stop || ne > CAP) return;  // stopped run or replica, or hub row (the fragment kernels own it): uniform exit before any barrier
    SWEEP_MOLD

    // ---- phase 1: lane per directed edge: gather incoming message, b = W^T m -> LDS (branch-free loads,
    // see k_sweep_psi)
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

    // ---- phase 2: lane per row (a wave per row above BIG_ROW edges): A[q] = prod_e b_e[q];
    //      psi_i = normalise(A * eta * F_i)
    SWEEP_PSI
    double Sacc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) Sacc[q] = 0.0;
    auto finish_row = [&](int r, double di, double (&A)[Q], const int *ae /* per-component exponents of a long row, or null */,
                          const double *ft = nullptr /* the row's line of P->ftab (rows of <= FT_D edges under dc), or null */) {
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
        if (sfl[r]) {  // clamped: marginal and out-messages stay as initialised (bp.cpp:1115-1124)
            double pv[Q];
            load_vec<Q>(psi_old + size_t(r0 + r) * Q, pv);
            store_vec<Q>(psi + size_t(r0 + r) * Q, pv);
            const double gi = dc ? di : 1.0;
#pragma unroll
            for (int q = 0; q < Q; ++q) Sacc[q] += gi * pv[q];
        } else if (ee - es <= BIG_ROW) {
            double A[Q], ft[Q];
            const bool tab = dc != 0 && ee - es <= FT_D;  // the field factors of this degree: loaded while the product runs
            if (tab) load_vec<Q>(P->ftab + size_t(ee - es) * QMAX, ft);
            SWEEP_ROW_START(r, A)
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
            if ((tid & 63) == 0) {
                SWEEP_ROW_FACTOR(r, A, ae)
                finish_row(r, double(ee - es), A, ae);
            }
        }
    }
    __syncthreads();

    // ---- phase 3: lane per directed edge: cavity, normalise, damp, store
    SWEEP_MNEW
    double md = 0.0;
    const int probe2 = P->ar_probe2;  // adaptive relaxation's probe sweep: report |m^{t+1} - m^{t-1}| (m^{t-1} sits in the slot written below)
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
                    SWEEP_ROW_FACTOR(r, cav, ce)
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
                    // 1-step: against the undamped value (bp.cpp:1059-1063); the probe compares what is stored, and a damped
                    // message moves by damp * (new - old) per sweep, so it is scaled back to compare like with like
                    md = nanmax(md, probe2 ? fabs(ref[q] - out[q]) / damp : fabs(ref[q] - nv));
                }
            }
            store_msg_stream<Q>(Mnew, size_t(e0 + le), out);
        }
    }
    block_reduce_store<Q, frame_cfg<Q>::WAVES>(Sacc, md, sred, SWEEP_RECORD);
