// The body of the hub pass of the free energy and the entropy: THE definition of k_fe_hub and of its twin under a per-vertex
// prior, k_fe_hub_prior (kernels.h), which include this file between their braces (see fe_frame_body.inc). It reads the
// kernel's parameters by name:
//     row_ptr rev nbr ndeg M Min hub_row hub_blk P dc want_entropy partials rec_stride rec_first
// Hook: FE_SITE_FACTOR(i, v, x), as in fe_frame_body.inc.
    __shared__ double sAq[BLOCK * Q];
    __shared__ double sCq[BLOCK * Q];
    __shared__ int sEq[BLOCK * Q];
    __shared__ double sred[4 * (FE_NP + 1)];
    const int tid = threadIdx.x;
    const uint32_t i = hub_row[blockIdx.x];
    const uint32_t e0 = row_ptr[i], d = row_ptr[i + 1] - e0;
    const double di = double(d);
    double acc[FE_NP] = {0.0, 0.0, 0.0, 0.0};
    double A[Q], C[Q];
    int ae[Q], ce[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) { A[q] = 1.0; C[q] = 1.0; ae[q] = 0; ce[q] = 0; }
    for (uint32_t le = tid; le < d; le += BLOCK) {
        double mi[Q], mo[Q], b[Q];
        load_msg<Q>(Min ? Min : M, Min ? size_t(e0 + le) : size_t(rev[e0 + le]), mi);
        load_msg<Q>(M, size_t(e0 + le), mo);
        double didl = 0.0;
        if (DC2) { const uint32_t l = nbr[e0 + le]; didl = di * double(ndeg[l]); }
        edge_field<Q, DC2>(P, mi, didl, b);
#pragma unroll
        for (int q = 0; q < Q; ++q) A[q] *= b[q];
        x_norm<Q>(A, ae);
        if (want_entropy) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                double a = 0.0;
#pragma unroll
                for (int t = 0; t < Q; ++t) a += P->cab[t * Q + q] * mi[t];
                C[q] *= a;
            }
            x_norm<Q>(C, ce);
        }
        double ln, en;
        edge_terms<Q, DC2>(P, mi, mo, didl, want_entropy, ln, en);
        acc[1] += ln;
        if (want_entropy) acc[3] += en;
    }
    block_product_x<Q>(A, ae, sAq, sEq);
    if (want_entropy) {  // uniform
        __syncthreads();
        block_product_x<Q>(C, ce, sCq, sEq);
    }
    if (tid == 0) {
        FE_SITE_FACTOR(i, A, ae)
        if (want_entropy) { FE_SITE_FACTOR(i, C, ce) }
        acc[0] += log_partition_x<Q>(P, dc, di, A, ae);
        if (want_entropy) acc[2] += entropy_site_x<Q>(P, C, ce);
    }
    double *rec = partials + size_t(rec_first == 0xffffffffu ? hub_blk[blockIdx.x] : rec_first + blockIdx.x) * rec_stride;
    block_reduce_store<FE_NP>(acc, 0.0, sred, rec);
    for (uint32_t x = FE_NP + 1 + tid; x < rec_stride; x += BLOCK) rec[x] = 0.0;  // the other columns of a wider record (k_fe_psi)
