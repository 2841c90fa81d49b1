// best_assignment and agreement_groups of csrc/host_reduce.h under -fsanitize=address,undefined (tests/test_agreement_cpu.py
// builds and runs this program): the maximum-weight assignment against the brute-force maximum for Q = 2 .. 9, against a planted
// permutation for Q = 10 .. 16, on matrices where every assignment ties, and the leader rule of the groups.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../../sbm-bp_amd/csrc/host_reduce.h"

using namespace sbmbp;

static int failures = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static bool is_permutation_of_labels(const std::vector<uint32_t> &p) {
    std::vector<char> seen(p.size(), 0);
    for (uint32_t v : p) {
        if (v >= p.size() || seen[v]) return false;
        seen[v] = 1;
    }
    return true;
}

static double value_of(uint32_t Q, const std::vector<double> &C, const std::vector<uint32_t> &p) {
    double s = 0.0;
    for (uint32_t a = 0; a < Q; ++a) s += C[size_t(a) * Q + p[a]];
    return s;
}

int main() {
    std::mt19937 rng(12345);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    int n_brute = 0, n_planted = 0;
    // Q = 2 .. 9: the brute-force maximum over all Q! permutations. The sums differ by the order of the additions at most:
    // Q terms below N = 1000, so 1e-9 is far above the rounding and far below any real gap.
    for (uint32_t Q = 2; Q <= 9; ++Q) {
        const int reps = Q <= 7 ? 40 : (Q == 8 ? 6 : 2);
        for (int rep = 0; rep < reps; ++rep) {
            std::vector<double> C(size_t(Q) * Q);
            for (double &c : C) c = (rep & 1) ? std::floor(1000.0 * U(rng)) : 1000.0 * U(rng);  // integers tie often
            std::vector<uint32_t> p(Q, 99u), q(Q);
            const double got = best_assignment(Q, C.data(), p.data());
            EXPECT(is_permutation_of_labels(p));
            EXPECT(got == value_of(Q, C, p));
            std::iota(q.begin(), q.end(), 0u);
            double best = -1.0;
            do best = std::max(best, value_of(Q, C, q)); while (std::next_permutation(q.begin(), q.end()));
            EXPECT(std::fabs(got - best) <= 1e-9);
            ++n_brute;
        }
    }
    // Q = 10 .. 16: a planted permutation of weight 100 plus noise below 1 (half the planted margin is 50): the planted
    // permutation is the unique maximum, since moving k >= 2 rows off it loses at least 100 k - k and gains less than k
    for (uint32_t Q = 10; Q <= 16; ++Q)
        for (int rep = 0; rep < 5; ++rep) {
            std::vector<uint32_t> planted(Q), p(Q, 99u), q(Q);
            std::iota(planted.begin(), planted.end(), 0u);
            std::shuffle(planted.begin(), planted.end(), rng);
            std::vector<double> C(size_t(Q) * Q);
            for (double &c : C) c = U(rng);
            for (uint32_t a = 0; a < Q; ++a) C[size_t(a) * Q + planted[a]] += 100.0;
            const double got = best_assignment(Q, C.data(), p.data());
            EXPECT(is_permutation_of_labels(p));
            EXPECT(p == planted);
            EXPECT(got == value_of(Q, C, planted));
            std::iota(q.begin(), q.end(), 0u);
            for (int k = 0; k < 1000; ++k) {
                std::shuffle(q.begin(), q.end(), rng);
                EXPECT(value_of(Q, C, q) <= got);
            }
            ++n_planted;
        }
    // every assignment ties; zeros; a NaN entry counts as 0 and must not derail the search
    for (uint32_t Q = 1; Q <= 16; ++Q) {
        for (double fill : {0.0, 1.0, 7.5}) {
            std::vector<double> C(size_t(Q) * Q, fill);
            std::vector<uint32_t> p(Q, 99u);
            const double got = best_assignment(Q, C.data(), p.data());
            EXPECT(is_permutation_of_labels(p));
            EXPECT(got == fill * Q);
        }
        std::vector<double> C(size_t(Q) * Q, 1.0);
        C[0] = std::nan("");
        std::vector<uint32_t> p(Q, 99u);
        (void)best_assignment(Q, C.data(), p.data());
        EXPECT(is_permutation_of_labels(p));
    }
    // groups: identity, all ones, the chain 0-1, 1-2 without 0-2 (2 leads: no linkage beyond the leaders), a NaN never passes
    {
        uint32_t g[4];
        const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        EXPECT(agreement_groups(3, I3, 0.5, g) == 3 && g[0] == 0 && g[1] == 1 && g[2] == 2);
        const double J3[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
        EXPECT(agreement_groups(3, J3, 1.0, g) == 1 && g[0] == 0 && g[1] == 0 && g[2] == 0);
        const double chain[9] = {1, 0.95, 0.2, 0.95, 1, 0.95, 0.2, 0.95, 1};
        EXPECT(agreement_groups(3, chain, 0.9, g) == 2 && g[0] == 0 && g[1] == 0 && g[2] == 1);
        const double nan2[4] = {1, std::nan(""), std::nan(""), 1};
        EXPECT(agreement_groups(2, nan2, 0.0, g) == 2 && g[1] == 1);
        EXPECT(agreement_groups(0, nullptr, 0.5, g) == 0);
    }
    if (failures) { std::printf("agreement_sanitize: %d failures\n", failures); return 1; }
    std::printf("agreement_sanitize ok: %d brute-force cases, %d planted cases\n", n_brute, n_planted);
    return 0;
}
