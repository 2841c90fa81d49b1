// Host arithmetic shared by the single engine, the shard ranks and the replica batch (C++14, standard headers only: no
// device code, usable from a plain host program): what turns the folded sums of the reduction kernels into the numbers the
// product prints - free energy and entropy parts, the moment series of the non-edge term, the EM expectations, the overlap.
// Every function takes plain numbers and pointers; N is the number of vertices of the whole graph (a shard rank passes the
// global count). The formulas are the reference's (bp.cpp:675-758, belief_propagation.cpp:967-988); the order of the
// operations inside each expression is part of the contract: the engines agree bit for bit because they all come here.
#ifndef SBMBP_HOST_REDUCE_H
#define SBMBP_HOST_REDUCE_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <numeric>
#include <vector>

namespace sbmbp {

// length of the packed moment tensors of orders 1 .. K: Q + Q^2 + ... + Q^K
inline uint32_t series_len(uint32_t Q, int K) {
    uint64_t T = 0, sz = 1;
    for (int k = 1; k <= K; ++k) { sz *= Q; T += sz; }
    return uint32_t(T);
}

// highest series order whose moment tensors fit k_moments (20 entries per thread of a 256-thread workgroup = 5120) and the
// reduction buffers: 4 up to Q = 8, 3 up to Q = 16, 2 above
inline int max_series_order(uint32_t Q) {
    int K = 0;
    uint64_t T = 0, sz = 1;
    while (K < 4) {
        sz *= Q;
        if (T + sz > 5120) break;
        T += sz;
        ++K;
    }
    return K;
}

// order of the series: the requested one (> 0) clamped to the cap, else the smallest K with
// N (wmax/N)^(K+1) / (2(K+1)) < 1e-12  (SURVEY A.4 truncation bound); where no K up to the cap meets it, the cap - silently,
// and then the bound of the cap is what holds (1e-7 at Q = 32, N = 4e4, c = 10)
inline int series_order(uint32_t Q, uint32_t N, int requested, double wmax) {
    const int Kmax = max_series_order(Q);
    if (requested > 0) return std::min(requested, Kmax);
    for (int K = 1; K <= Kmax; ++K) {
        double err = double(N) * std::pow(wmax / double(N), K + 1) / (2.0 * (K + 1));
        if (err < 1e-12) return K;
    }
    return Kmax;
}

// non-edge mode 1 = always the exact O(N^2) loop, 2 = always the series, 0 = automatic: exact up to N = 32768
inline bool nonedge_is_exact(int mode, uint32_t N) { return (mode == 1) || (mode == 0 && N <= 32768); }

// the three Q x Q matrices of the non-edge term, out[0 .. 3 Q Q): w = N(1 - (1-cab/N)^beta), P = (1-cab/N)^beta, cab
// (bp.cpp:675-741); *wmax = the largest entry of w and cab
inline void nonedge_mats(uint32_t Q, uint32_t N, const double *cab, double beta, double *out, double *wmax_out) {
    double *wmat = out, *Pmat = out + Q * Q, *cabm = out + 2 * Q * Q;
    double wmax = 0.0;
    for (uint32_t a = 0; a < Q * Q; ++a) {
        Pmat[a] = std::pow(1.0 - cab[a] / double(N), beta);
        wmat[a] = double(N) * (1.0 - Pmat[a]);
        cabm[a] = cab[a];
        wmax = std::max(wmax, std::max(wmat[a], cabm[a]));
    }
    if (wmax_out) *wmax_out = wmax;
}

// contraction <M_k, (m_0 x ... x m_{k-1}) M_k> of SURVEY A.4: the matrices are applied one tensor mode after the other
// (k Q^(k+1) multiplications; summing all Q^2k terms directly took 0.1 s per call at Q = 64, k = 2 or Q = 16, k = 3 - ten
// times the device side of the whole reduction pass). Mode j is digit j of the index, the least significant first.
inline double contract(const double *Mk, uint32_t Q, unsigned k, const std::vector<const double *> &mats) {
    size_t T = 1;
    for (unsigned j = 0; j < k; ++j) T *= Q;
    std::vector<double> cur(Mk, Mk + T), nxt(T);
    size_t stride = 1;
    for (unsigned j = 0; j < k; ++j) {
        const double *m = mats[j];
        const size_t outer = T / (stride * Q);
        for (size_t hi = 0; hi < outer; ++hi)
            for (uint32_t a = 0; a < Q; ++a) {
                double *dst = nxt.data() + (hi * Q + a) * stride;
                for (size_t lo = 0; lo < stride; ++lo) dst[lo] = 0.0;
                for (uint32_t b = 0; b < Q; ++b) {
                    const double w = m[a * Q + b];
                    const double *src = cur.data() + (hi * Q + b) * stride;
                    for (size_t lo = 0; lo < stride; ++lo) dst[lo] += w * src[lo];
                }
            }
        cur.swap(nxt);
        stride *= Q;
    }
    double acc = 0.0;
    for (size_t a = 0; a < T; ++a) acc += Mk[a] * cur[a];
    return acc;
}

// the all-pairs sums of the series from the packed moment tensors Mk of orders 1 .. K (mats as nonedge_mats fills them):
// all[0] = -sum_k <M_k, (w x ... x w) M_k> / (k N^k); with want_entropy all[1] = sum_k <M_k, (v x cab^(k-1)) M_k> / N^k,
// v = cab log cab (term k-1 of the entropy is (u/N)(y/N)^(k-1))
inline void nonedge_series(uint32_t Q, uint32_t N, int K, bool want_entropy, const double *Mk, const double *mats, double all[2]) {
    const double *wmat = mats, *cabm = mats + 2 * Q * Q;
    std::vector<double> vmat(want_entropy ? Q * Q : 0);
    for (size_t a = 0; a < vmat.size(); ++a) vmat[a] = cabm[a] * std::log(cabm[a]);
    all[0] = all[1] = 0.0;
    double Nk = 1.0;
    size_t off = 0, tsz = 1;
    for (int k = 1; k <= K; ++k) {
        tsz *= Q;
        Nk *= double(N);
        std::vector<const double *> ms(k, wmat);
        all[0] -= contract(Mk + off, Q, unsigned(k), ms) / (double(k) * Nk);
        if (want_entropy) {
            std::vector<const double *> me(k, cabm);
            me[0] = vmat.data();
            all[1] += contract(Mk + off, Q, unsigned(k), me) / Nk;
        }
        off += tsz;
    }
}

// {f_nonedge, e_nonedge} from the sums over all pairs and over the adjacent pairs
inline void nonedge_finish(const double all[2], const double adj[2], uint32_t N, double out[2]) {
    out[0] = (all[0] - adj[0]) / (2.0 * N);
    out[1] = (all[1] - adj[1]) / (2.0 * N);
}

// {f_site, f_edge, e_site, e_edge} from sums = {sum log Z_i, sum log norm_L, e_site sum, e_edge sum}; dc1_const = the sum
// over the directed edges of log(d_i d_l) under dc 1 (SURVEY A.3 dc-1 note), null otherwise
inline void site_edge_parts(uint32_t N, const double *dc1_const, const double sums[4], double out[4]) {
    const double Nd = double(N);
    out[0] = sums[0] / Nd;
    out[1] = sums[1] / (2.0 * Nd);
    if (dc1_const) { out[0] += *dc1_const / Nd; out[1] += *dc1_const / (2.0 * Nd); }
    out[2] = sums[2] / Nd;
    out[3] = sums[3] / (2.0 * Nd);
}
// parts = {site, edge, non-edge}   (bp.cpp:744-758)
inline double free_energy_of(const double parts[3]) { return -parts[0] + parts[1] + parts[2]; }
inline double entropy_of(const double parts[3]) { return -parts[0] + parts[1] - parts[2]; }

// cab_expect from the Q (Q + 1) / 2 numerators: symmetric fill and the rescaling of belief_propagation.cpp:967-988
inline void em_rescale(uint32_t Q, uint32_t N, uint32_t dc, const double *na, const double *nna, const double *tri, double *ce) {
    uint32_t t = 0;
    for (uint32_t q1 = 0; q1 < Q; ++q1)
        for (uint32_t q2 = q1; q2 < Q; ++q2, ++t) { ce[q1 * Q + q2] = tri[t]; ce[q2 * Q + q1] = tri[t]; }
    const double EPS = 1.0e-50;
    const double *nn = (dc == 0) ? na : nna;
    for (uint32_t q1 = 0; q1 < Q; ++q1)
        for (uint32_t q2 = q1; q2 < Q; ++q2)
            if (na[q1] > EPS && na[q2] > EPS) {
                if (q1 != q2) {
                    ce[q1 * Q + q2] *= double(N) / (nn[q1] * nn[q2]);
                    ce[q2 * Q + q1] = ce[q1 * Q + q2];
                } else {
                    ce[q1 * Q + q2] *= 2. * double(N) / (nn[q1] * nn[q2]);
                }
            }
}

// compute_overlap (bp.cpp:775-811) from the Q x Q confusion matrix C: the best trace / N over all Q! permutations of the
// labels for Q <= 8, the identity alone above (:784-790)
inline double best_overlap(uint32_t Q, uint32_t N, const double *C) {
    std::vector<uint32_t> perm(Q);
    std::iota(perm.begin(), perm.end(), 0u);
    double best = -1.0;
    do {
        double s = 0.0;
        for (uint32_t a = 0; a < Q; ++a) s += C[a * Q + perm[a]];
        s /= double(N);
        if (s > best) best = s;
        if (Q > 8) break;
    } while (std::next_permutation(perm.begin(), perm.end()));
    return best;
}

// Agreement of two runs (sbmbp.h: sbmbp_batch_agreement): the permutation perm of the labels that maximises
// sum_a C[a * Q + perm[a]] over all Q! of them, exactly, for any Q: the maximum-weight assignment by the Hungarian method
// with potentials (O(Q^3); rows are inserted one after the other along shortest augmenting paths of the costs -C). A NaN
// entry counts as 0. Returns the sum of the C entries the assignment picks, added in the order a = 0 .. Q-1. best_overlap
// above is the reference's rule for the overlap with the TRUE configuration and stays what it is.
inline double best_assignment(uint32_t Q, const double *C, uint32_t *perm) {
    const double INF = std::numeric_limits<double>::infinity();
    auto cost = [&](uint32_t a, uint32_t b) { const double c = C[size_t(a) * Q + b]; return std::isnan(c) ? 0.0 : -c; };
    // 1-based rows / columns; column 0 is the virtual start. row_of[b] = row matched to column b (0 = none)
    std::vector<double> u(Q + 1, 0.0), v(Q + 1, 0.0), minv(Q + 1);
    std::vector<uint32_t> row_of(Q + 1, 0u), way(Q + 1, 0u);
    std::vector<char> used(Q + 1);
    for (uint32_t a = 1; a <= Q; ++a) {
        row_of[0] = a;
        uint32_t b0 = 0;
        std::fill(minv.begin(), minv.end(), INF);
        std::fill(used.begin(), used.end(), char(0));
        do {
            used[b0] = 1;
            const uint32_t a0 = row_of[b0];
            double delta = INF;
            uint32_t b1 = 0;
            for (uint32_t b = 1; b <= Q; ++b) {
                if (used[b]) continue;
                const double cur = cost(a0 - 1, b - 1) - u[a0] - v[b];
                if (cur < minv[b]) { minv[b] = cur; way[b] = b0; }
                if (b1 == 0 || minv[b] < delta) { delta = minv[b]; b1 = b; }  // b1 != 0 after the first free column: an Inf entry cannot strand the search
            }
            for (uint32_t b = 0; b <= Q; ++b) {
                if (used[b]) { u[row_of[b]] += delta; v[b] -= delta; }
                else minv[b] -= delta;
            }
            b0 = b1;
        } while (row_of[b0] != 0);
        do {  // augment along the path found
            const uint32_t b1 = way[b0];
            row_of[b0] = row_of[b1];
            b0 = b1;
        } while (b0 != 0);
    }
    for (uint32_t b = 1; b <= Q; ++b) perm[row_of[b] - 1] = b - 1;
    double s = 0.0;
    for (uint32_t a = 0; a < Q; ++a) s += C[size_t(a) * Q + perm[a]];
    return s;
}

// Groups of runs from their n x n overlap matrix (sbmbp.h: sbmbp_agreement_groups): runs in ascending order; x joins the
// group of the FIRST earlier leader g with overlap[g * n + x] >= threshold, else it leads a new group. Returns the number
// of groups; group[x] = the group's number in order of creation. A NaN overlap never passes.
inline uint32_t agreement_groups(uint32_t n, const double *overlap, double threshold, uint32_t *group) {
    std::vector<uint32_t> leader;
    for (uint32_t x = 0; x < n; ++x) {
        uint32_t k = 0;
        while (k < leader.size() && !(overlap[size_t(leader[k]) * n + x] >= threshold)) ++k;
        if (k == leader.size()) leader.push_back(x);
        group[x] = k;
    }
    return uint32_t(leader.size());
}

// which of n runs is best (sbmbp.h: sbmbp_best_replica): the lowest free energy that is not NaN among the runs of the
// first rank that has one; 0 when there is none
inline uint32_t best_replica(uint32_t n, const double *f, const int *rank, int n_ranks) {
    int pick = -1;
    for (int pass = 0; pass < n_ranks && pick < 0; ++pass)
        for (uint32_t r = 0; r < n; ++r) {
            if (rank[r] != pass || std::isnan(f[r])) continue;
            if (pick < 0 || f[r] < f[pick]) pick = int(r);
        }
    return pick < 0 ? 0u : uint32_t(pick);
}

}  // namespace sbmbp
#endif
