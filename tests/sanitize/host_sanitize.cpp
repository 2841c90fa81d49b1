// Host-side sanitizer job: the engine's host code (csrc/host_graph.cpp: edge-list parser, CSR
// builder, the std::mt19937-compatible initial state, parameter constructors) and the CPU restatement (oracle/bp_oracle.cpp)
// built with -fsanitize=address,undefined and driven through their edge cases. CPU build only; no GPU code is involved.
// Exit code 0 and no sanitizer report = pass (tests/test_capi_cpu.py::test_host_code_under_asan_ubsan).
// Also the host drivers every front end shares: the segment plan (host_graph.h) against hand-worked tables and its
// invariants, the batch planner against hand-worked values, and the queue-ahead loop, the convergence run and the EM loop
// (host_loops.h) over scripted fakes, call for call against traces recorded from the loops they replaced (loop_fakes.h).
// And the reduction arithmetic they share (host_reduce.h): hand-derivable tables, the moment series against the oracle's at
// every order, and every function bit for bit against what the copies it replaced gave on fixed inputs (parent_reduce.inc).
// And the step tables of the coloured order (host_graph.h coloured_step_tables): a hand-worked case, their invariants, and
// entry for entry what the engine built before the construction became host code (parent_step_tables.inc).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "../../sbm-bp_amd/csrc/host_graph.h"
#include "../../sbm-bp_amd/csrc/host_loops.h"
#include "../../sbm-bp_amd/csrc/host_reduce.h"
#include "loop_fakes.h"

extern "C" {
void *orc_graph_from_edges(const uint32_t *pairs, uint64_t n_pairs, uint32_t N);
void *orc_graph_load_edgelist(const char *path, uint32_t N);
void orc_graph_free(void *g);
uint32_t orc_graph_n(void *g);
uint64_t orc_graph_e2(void *g);
void orc_graph_copy(void *g, uint64_t *row_ptr, uint32_t *nbr, uint32_t *rev);
void *orc_rng_create(unsigned seed);
void orc_rng_free(void *r);
void orc_param_from_epsilon_c(uint32_t N, uint32_t Q, double eps, double c, double *cab, uint32_t *na);
void *orc_bp_create(void *g, uint32_t Q, uint32_t dc);
void orc_bp_free(void *s);
void orc_bp_init_messages(void *s, unsigned flag, const int32_t *conf, const uint32_t *true_conf, void *rng);
void orc_bp_set_params(void *s, const double *cab, const uint32_t *na, double beta);
void orc_bp_get_state(void *s, double *psi, double *msg);
int orc_bp_converge_async(void *s, float crit, unsigned tmax, float damp, void *rng, int conditional);
int orc_bp_converge_sync(void *s, double crit, unsigned tmax, double damp, double *last);
double orc_bp_free_energy(void *s, int series_K, double *parts);
double orc_bp_entropy(void *s, int series_K, double *parts);
void orc_bp_nonedge(void *s, int series_K, double *out);
void orc_bp_em_expect(void *s, double *na_e, double *nna_e, double *cab_e);
double orc_bp_overlap(void *s);
int orc_bp_learning(void *s, float lcrit, unsigned tmax, float lr, float damp, void *rng, int sync, int series_K, double *f);
}

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "host_sanitize: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

static int run(const char *dataset) {
    using namespace sbmbp;
    // ---- parser: the shipped data set, a ragged file (blank lines, trailing spaces, no final newline), a missing file
    std::vector<uint32_t> pairs;
    REQUIRE(read_edgelist(dataset, pairs) == 0 && pairs.size() == 2 * 1498);
    const std::string tmp = std::string(std::getenv("TMPDIR") ? std::getenv("TMPDIR") : "/tmp") + "/host_sanitize_ragged.txt";
    { std::ofstream f(tmp); f << "0 1\n\n  2   3  \n3 4\r\n7 7\n5 6"; }
    std::vector<uint32_t> ragged;
    REQUIRE(read_edgelist(tmp.c_str(), ragged) == 0 && ragged.size() >= 10);
    std::vector<uint32_t> none;
    REQUIRE(read_edgelist("/nonexistent/edge/list", none) != 0);
    { std::ofstream f(tmp); }  // an empty file
    std::vector<uint32_t> empty;
    (void)read_edgelist(tmp.c_str(), empty);
    std::remove(tmp.c_str());
    // ---- CSR builder: duplicates, self-loops, isolated vertices, ids at the upper bound, an empty graph, one hub row
    sbmbp_graph g;
    REQUIRE(graph_from_pairs(g, pairs.data(), pairs.size() / 2, 1000) == 0 && g.n == 1000 && g.e2() == 2996);
    for (uint64_t k = 0; k < g.e2(); ++k) REQUIRE(g.rev[g.rev[k]] == k);
    sbmbp_graph g0;
    REQUIRE(graph_from_pairs(g0, nullptr, 0, 5) == 0 && g0.e2() == 0 && g0.n == 5);
    const uint32_t odd[] = {0, 0, 1, 2, 2, 1, 1, 2, 4, 4, 3, 0};
    sbmbp_graph g1;
    REQUIRE(graph_from_pairs(g1, odd, 6, 5) == 0 && g1.n == 5);
    std::vector<uint32_t> star;
    for (uint32_t v = 1; v < 700; ++v) { star.push_back(0); star.push_back(v); }
    sbmbp_graph gs;
    REQUIRE(graph_from_pairs(gs, star.data(), star.size() / 2, 700) == 0 && gs.max_degree == 699);
    sbmbp_graph gc;
    REQUIRE(graph_from_csr(gc, g.n, g.e2(), g.row_ptr.data(), g.nbr.data(), g.rev.data()) == 0 && gc.e2() == g.e2());
    const uint32_t beyond[] = {0, 9};
    sbmbp_graph gb;
    (void)graph_from_pairs(gb, beyond, 1, 5);  // an id >= n: grows or is rejected, must not write out of bounds
    // ---- parameters, incl. the truncation quirks and epsilon < 0
    double cab[9];
    uint32_t na[3];
    param_from_epsilon_c(1001, 3, 0.1, 3.0, cab, na);
    REQUIRE(na[0] == 333 && na[1] == 333 && na[2] == 333);
    param_from_epsilon_c(1000, 2, -1.0, 3.0, cab, na);
    const double pa[2] = {0.5, 0.5}, cu[3] = {3.63, 2.36, 3.63};
    param_from_direct(1000, 2, pa, cu, cab, na);
    REQUIRE(cab[1] == 2.36 && cab[2] == 2.36);
    // ---- the reference-compatible initial state: every init flag, with and without a sink, equal to the oracle's bit for bit
    std::vector<uint32_t> rp32(g.row_ptr.begin(), g.row_ptr.end());
    std::vector<uint32_t> tc(1000);
    for (uint32_t i = 0; i < 1000; ++i) tc[i] = i / 500;
    std::vector<int32_t> conf(1000, -1);
    for (uint32_t i = 0; i < 1000; i += 7) conf[i] = int32_t(tc[i]);
    void *og = orc_graph_from_edges(pairs.data(), pairs.size() / 2, 1000);
    REQUIRE(orc_graph_n(og) == 1000 && orc_graph_e2(og) == g.e2());
    for (unsigned flag = 0; flag < 4; ++flag) {
        std::vector<double> psi(size_t(1000) * 2), msg(g.e2() * 2), opsi(psi.size()), omsg(msg.size());
        init_state_host(1000, rp32.data(), g.e2(), 2, flag, flag ? conf.data() : nullptr, 11 + flag, psi.data(), msg.data());
        void *bp = orc_bp_create(og, 2, 0);
        void *rng = orc_rng_create(11 + flag);
        orc_bp_init_messages(bp, flag, flag ? conf.data() : nullptr, tc.data(), rng);
        orc_bp_get_state(bp, opsi.data(), omsg.data());
        REQUIRE(std::memcmp(psi.data(), opsi.data(), psi.size() * 8) == 0 && std::memcmp(msg.data(), omsg.data(), msg.size() * 8) == 0);
        orc_rng_free(rng);
        orc_bp_free(bp);
        // the streamed form: slabs handed to a sink
        std::vector<double> spsi(psi.size()), smsg(msg.size());
        state_sink sink;
        sink.put = [&](uint32_t lo, uint32_t hi, const double *pr, const double *mr) {
            std::memcpy(spsi.data() + size_t(lo) * 2, pr, size_t(hi - lo) * 2 * 8);
            std::memcpy(smsg.data() + size_t(rp32[lo]) * 2, mr, size_t(rp32[hi] - rp32[lo]) * 2 * 8);
        };
        init_state_host(1000, rp32.data(), g.e2(), 2, flag, flag ? conf.data() : nullptr, 11 + flag, nullptr, nullptr, &sink);
        REQUIRE(std::memcmp(psi.data(), spsi.data(), psi.size() * 8) == 0 && std::memcmp(msg.data(), smsg.data(), msg.size() * 8) == 0);
    }
    // ---- the oracle: both schedules (the synchronous one with its adaptive relaxation), reductions, learning, a hub graph
    double pcab[4];
    uint32_t pna[2];
    orc_param_from_epsilon_c(1000, 2, 0.1, 3.0, pcab, pna);
    for (uint32_t dc = 0; dc < 3; ++dc) {
        double c2[4] = {pcab[0], pcab[1], pcab[2], pcab[3]};
        if (dc) for (double &x : c2) x /= 9.0;
        void *bp = orc_bp_create(og, 2, dc);
        void *rng = orc_rng_create(0);
        orc_bp_init_messages(bp, 0, nullptr, tc.data(), rng);
        orc_bp_set_params(bp, c2, pna, 1.0);
        REQUIRE(orc_bp_converge_async(bp, 5e-6f, 200, 1.0f, rng, 1) >= 0);
        double last = 0, parts[3];
        REQUIRE(orc_bp_converge_sync(bp, 1e-9, 500, 1.0, &last) >= 0 && last < 1e-9);
        REQUIRE(std::isfinite(orc_bp_free_energy(bp, dc ? 2 : 0, parts)));
        (void)orc_bp_entropy(bp, 2, parts);
        double nae[2], nnae[2], cabe[4];
        orc_bp_em_expect(bp, nae, nnae, cabe);
        REQUIRE(orc_bp_overlap(bp) > 0.5);
        orc_rng_free(rng);
        orc_bp_free(bp);
    }
    {
        void *bp = orc_bp_create(og, 2, 0);
        void *rng = orc_rng_create(0);
        orc_bp_init_messages(bp, 0, nullptr, tc.data(), rng);
        const double c5[4] = {5, 1, 1, 5};
        orc_bp_set_params(bp, c5, pna, 1.0);
        double f = 0;
        REQUIRE(orc_bp_learning(bp, 1e-4f, 40, 0.2f, 1.0f, nullptr, 1, 2, &f) > 0 && std::isfinite(f));
        orc_rng_free(rng);
        orc_bp_free(bp);
    }
    {
        void *sg = orc_graph_from_edges(star.data(), star.size() / 2, 700);  // one row of 699 edges: the long-row products
        std::vector<uint32_t> t3(700);
        for (uint32_t i = 0; i < 700; ++i) t3[i] = i % 3;
        const double c3[9] = {9, 1.5, 1.5, 1.5, 9, 1.5, 1.5, 1.5, 9};
        const uint32_t n3[3] = {234, 233, 233};
        void *bp = orc_bp_create(sg, 3, 0);
        void *rng = orc_rng_create(3);
        orc_bp_init_messages(bp, 0, nullptr, t3.data(), rng);
        orc_bp_set_params(bp, c3, n3, 1.0);
        double last = 0;
        (void)orc_bp_converge_sync(bp, 1e-9, 300, 1.0, &last);
        REQUIRE(last == last);
        orc_rng_free(rng);
        orc_bp_free(bp);
        orc_graph_free(sg);
    }
    orc_graph_free(og);
    return 0;
}

// ------------------------------------------------------------------------------------------ segment plan
typedef std::vector<uint32_t> u32s;

static int check_plan(const std::vector<uint64_t> &rp, uint32_t n, uint32_t cap, uint32_t rcap, const u32s &chunks, sbmbp::segment_plan_t &p) {
    sbmbp::segment_plan(rp.data(), n, cap, rcap, chunks, p);
    const u32s ch = chunks.empty() ? u32s{0u, n} : chunks;
    const size_t nb = p.blk_row.size() - 1;
    REQUIRE(p.blk_row.size() >= 1 && p.blk_row.front() == 0 && p.blk_row.back() == n && p.blk_e0.size() == p.blk_row.size());
    REQUIRE(p.hub_row.size() == p.hub_blk.size());
    REQUIRE(p.chunk_blk.size() == ch.size() && p.chunk_hub.size() == ch.size());
    REQUIRE(p.chunk_blk.front() == 0 && p.chunk_blk.back() == nb && p.chunk_hub.front() == 0 && p.chunk_hub.back() == p.hub_row.size());
    std::vector<char> is_hub(nb + 1, 0);
    for (size_t h = 0; h < p.hub_row.size(); ++h) {
        REQUIRE(p.hub_blk[h] < nb && p.blk_row[p.hub_blk[h]] == p.hub_row[h] && p.blk_row[p.hub_blk[h] + 1] == p.hub_row[h] + 1);
        REQUIRE(rp[p.hub_row[h] + 1] - rp[p.hub_row[h]] > cap);
        REQUIRE(h == 0 || p.hub_row[h] > p.hub_row[h - 1]);
        is_hub[p.hub_blk[h]] = 1;
    }
    auto starts_chunk = [&](uint32_t row) { return std::find(ch.begin() + 1, ch.end() - 1, row) != ch.end() - 1; };
    for (size_t b = 0; b < nb; ++b) {
        const uint32_t r0 = p.blk_row[b], r1 = p.blk_row[b + 1];
        REQUIRE(r0 < r1);  // strictly rising
        REQUIRE(p.blk_e0[b] == rp[r0]);
        for (size_t c = 1; c + 1 < ch.size(); ++c) REQUIRE(!(r0 < ch[c] && ch[c] < r1));  // no segment straddles a chunk boundary
        if (is_hub[b]) continue;
        const uint64_t edges = rp[r1] - rp[r0];
        REQUIRE(edges <= cap && r1 - r0 <= rcap);
        for (uint32_t i = r0; i < r1; ++i) REQUIRE(rp[i + 1] - rp[i] <= cap);
        if (r1 < n) {  // closed for a reason: the next row would not fit, is a hub, or starts a chunk
            const uint64_t d = rp[r1 + 1] - rp[r1];
            REQUIRE(d > cap || edges + d > cap || r1 - r0 + 1 > rcap || starts_chunk(r1));
        }
    }
    REQUIRE(p.blk_e0[nb] == rp[n]);
    for (size_t c = 0; c + 1 < ch.size(); ++c) {
        REQUIRE(p.chunk_blk[c] <= p.chunk_blk[c + 1] && p.chunk_hub[c] <= p.chunk_hub[c + 1]);
        for (uint32_t b = p.chunk_blk[c]; b < p.chunk_blk[c + 1]; ++b) REQUIRE(p.blk_row[b] >= ch[c] && p.blk_row[b + 1] <= ch[c + 1]);
        for (uint32_t h = p.chunk_hub[c]; h < p.chunk_hub[c + 1]; ++h) REQUIRE(p.hub_row[h] >= ch[c] && p.hub_row[h] < ch[c + 1]);
    }
    return 0;
}

struct plan_case { u32s deg, chunks, blk_row, blk_e0, hub_row, hub_blk, chunk_blk, chunk_hub; };

static int test_segment_plan(const char *dataset) {
    // cap 4, rcap 3; the tables are worked out by hand
    const plan_case cases[] = {
        {{0}, {}, {0, 1}, {0, 0}, {}, {}, {0, 1}, {0, 0}},
        {{0, 0, 0, 0}, {}, {0, 3, 4}, {0, 0, 0}, {}, {}, {0, 2}, {0, 0}},                        // the row limit splits at 3
        {{4}, {}, {0, 1}, {0, 4}, {}, {}, {0, 1}, {0, 0}},                                       // exactly cap: no hub
        {{5}, {}, {0, 1}, {0, 5}, {0}, {0}, {0, 1}, {0, 1}},
        {{5, 1, 1}, {}, {0, 1, 3}, {0, 5, 7}, {0}, {0}, {0, 2}, {0, 1}},                         // a hub first
        {{1, 1, 5}, {}, {0, 2, 3}, {0, 2, 7}, {2}, {1}, {0, 2}, {0, 1}},                         // a hub last
        {{5, 6}, {}, {0, 1, 2}, {0, 5, 11}, {0, 1}, {0, 1}, {0, 2}, {0, 2}},                     // adjacent hubs
        {{2, 2, 1}, {}, {0, 2, 3}, {0, 4, 5}, {}, {}, {0, 2}, {0, 0}},                           // the edge limit splits after two rows
        {{1, 1, 1, 1, 5, 1}, {}, {0, 3, 4, 5, 6}, {0, 3, 4, 9, 10}, {4}, {2}, {0, 4}, {0, 1}},
        {{1, 1, 1, 1, 5, 1}, {0, 2, 6}, {0, 2, 4, 5, 6}, {0, 2, 4, 9, 10}, {4}, {2}, {0, 1, 4}, {0, 0, 1}},        // a boundary inside a would-be segment
        {{1, 1, 1, 1, 5, 1}, {0, 0, 6}, {0, 3, 4, 5, 6}, {0, 3, 4, 9, 10}, {4}, {2}, {0, 0, 4}, {0, 0, 1}},        // an empty leading chunk
        {{1, 1, 1, 1, 5, 1}, {0, 6, 6}, {0, 3, 4, 5, 6}, {0, 3, 4, 9, 10}, {4}, {2}, {0, 4, 4}, {0, 1, 1}},        // an empty trailing chunk
        {{1, 1, 1, 1, 5, 1}, {0, 4, 5, 6}, {0, 3, 4, 5, 6}, {0, 3, 4, 9, 10}, {4}, {2}, {0, 2, 3, 4}, {0, 0, 1, 1}},  // boundaries around the hub
    };
    for (const plan_case &c : cases) {
        std::vector<uint64_t> rp(c.deg.size() + 1, 0);
        for (size_t i = 0; i < c.deg.size(); ++i) rp[i + 1] = rp[i] + c.deg[i];
        sbmbp::segment_plan_t p;
        REQUIRE(check_plan(rp, uint32_t(c.deg.size()), 4, 3, c.chunks, p) == 0);
        REQUIRE(p.blk_row == c.blk_row && p.blk_e0 == c.blk_e0 && p.hub_row == c.hub_row && p.hub_blk == c.hub_blk);
        REQUIRE(p.chunk_blk == c.chunk_blk && p.chunk_hub == c.chunk_hub);
    }
    {   // no rows at all: one empty chunk, no segment
        const std::vector<uint64_t> rp{0};
        sbmbp::segment_plan_t p;
        REQUIRE(check_plan(rp, 0, 4, 3, {}, p) == 0);
        REQUIRE(p.blk_row == u32s{0} && p.hub_row.empty() && p.chunk_blk == (u32s{0, 0}));
    }
    // the shipped graphs at the caps of the Q <= 2 frame, whole and in chunks
    const std::string dir = std::string(dataset).substr(0, std::string(dataset).find_last_of('/') + 1);
    for (const char *name : {"c1_dataset.edgelist", "hub_n600.edgelist"}) {
        std::vector<uint32_t> pairs;
        REQUIRE(sbmbp::read_edgelist((dir + name).c_str(), pairs) == 0);
        uint32_t n = 0;
        for (uint32_t v : pairs) n = std::max(n, v + 1);
        sbmbp_graph g;
        REQUIRE(sbmbp::graph_from_pairs(g, pairs.data(), pairs.size() / 2, n) == 0);
        sbmbp::segment_plan_t p;
        REQUIRE(check_plan(g.row_ptr, g.n, 256, 128, {}, p) == 0);
        REQUIRE(check_plan(g.row_ptr, g.n, 256, 128, {0, g.n / 3, g.n / 3, g.n - 1, g.n}, p) == 0);
        REQUIRE(check_plan(g.row_ptr, g.n, 64, 64, {0, g.n / 2, g.n}, p) == 0);  // (the Q 9..16 frame: hub_n600's rows of 102, 80, 71 edges are hubs)
        REQUIRE(p.hub_row.empty() == (g.max_degree <= 64));
    }
    return 0;
}

// Plans worked out elsewhere (tests/boundary_graph.py segment_model on the boundary graphs): per plan one line
// `cap rcap n n_bounds n_hubs`, then the n degrees, the segment boundaries and the hub rows. segment_plan must give exactly
// these, and pass its invariants.
static int test_plans_from_file(const char *path, size_t *count) {
    std::ifstream f(path);
    REQUIRE(f.good());
    uint32_t cap, rcap, n, nb, nh;
    for (*count = 0; f >> cap >> rcap >> n >> nb >> nh; ++*count) {
        u32s deg(n), bounds(nb), hubs(nh);
        for (u32s *v : {&deg, &bounds, &hubs}) for (uint32_t &x : *v) REQUIRE(bool(f >> x));
        std::vector<uint64_t> rp(size_t(n) + 1, 0);
        for (uint32_t i = 0; i < n; ++i) rp[i + 1] = rp[i] + deg[i];
        sbmbp::segment_plan_t p;
        REQUIRE(check_plan(rp, n, cap, rcap, {}, p) == 0);
        if (p.blk_row != bounds || p.hub_row != hubs) {
            std::fprintf(stderr, "host_sanitize: plan %zu (cap %u, rcap %u, %u rows): segment_plan gives %zu segments and %zu hub rows, the file %zu and %zu\n",
                         *count, cap, rcap, n, p.blk_row.size() - 1, p.hub_row.size(), bounds.size() - 1, hubs.size());
            for (size_t b = 0; b < std::min(p.blk_row.size(), bounds.size()); ++b)
                if (p.blk_row[b] != bounds[b]) { std::fprintf(stderr, "  first difference: boundary %zu is row %u, the file says %u\n", b, p.blk_row[b], bounds[b]); break; }
            return 1;
        }
    }
    REQUIRE(f.eof() && *count > 0);
    return 0;
}

// Chunked plans worked out elsewhere (tests/shard_boundary_graph.py chunked_segment_model on the rows of every rank of the
// shard recipes, cut as tests/plan_model.py cuts them): per plan one line `cap rcap n n_chunks n_bounds n_hubs`, then the n
// degrees, the n_chunks + 1 chunk boundaries, the segment boundaries, the hub rows, and chunk_blk and chunk_hub (n_chunks + 1
// each). segment_plan with these chunk boundaries must give exactly these tables, and pass its invariants.
static int test_chunk_plans_from_file(const char *path, size_t *count) {
    std::ifstream f(path);
    REQUIRE(f.good());
    uint32_t cap, rcap, n, nc, nb, nh;
    for (*count = 0; f >> cap >> rcap >> n >> nc >> nb >> nh; ++*count) {
        u32s deg(n), chunks(nc + 1), bounds(nb), hubs(nh), cblk(nc + 1), chub(nc + 1);
        for (u32s *v : {&deg, &chunks, &bounds, &hubs, &cblk, &chub}) for (uint32_t &x : *v) REQUIRE(bool(f >> x));
        std::vector<uint64_t> rp(size_t(n) + 1, 0);
        for (uint32_t i = 0; i < n; ++i) rp[i + 1] = rp[i] + deg[i];
        sbmbp::segment_plan_t p;
        REQUIRE(check_plan(rp, n, cap, rcap, chunks, p) == 0);
        const char *what = p.blk_row != bounds ? "blk_row" : p.hub_row != hubs ? "hub_row" : p.chunk_blk != cblk ? "chunk_blk" : p.chunk_hub != chub ? "chunk_hub" : nullptr;
        if (what) {
            std::fprintf(stderr, "host_sanitize: chunked plan %zu (cap %u, rcap %u, %u rows, %u chunks): %s differs; segment_plan gives %zu segments and %zu hub rows, the file %zu and %zu\n",
                         *count, cap, rcap, n, nc, what, p.blk_row.size() - 1, p.hub_row.size(), bounds.size() - 1, hubs.size());
            return 1;
        }
        for (size_t h = 0; h < hubs.size(); ++h) REQUIRE(p.blk_row[p.hub_blk[h]] == hubs[h]);
    }
    REQUIRE(f.eof() && *count > 0);
    return 0;
}

// ------------------------------------------------------------------------------------------ the coloured order's tables
// Step plans as a stream of numbers (tests/boundary_graph.py step_plan_model on the layouts of tests/coloured_step_graph.py):
// per plan `cap rcap n n_steps max_rec` and the lengths of rows, loff, seg_row0, hub_row, hub_rec, frag_hub, hub_frag0, seg0,
// hub0, frag0; then the n degrees, the step of every row, and the ten tables. coloured_step_tables (fragments of 256 edges)
// must give exactly these, and pass its invariants.
static int check_step_plans(const u32s &tok, size_t *count, const char *what) {
    size_t at = 0;
    for (*count = 0; at < tok.size(); ++*count) {
        REQUIRE(at + 15 <= tok.size());
        const uint32_t cap = tok[at], rcap = tok[at + 1], n = tok[at + 2], n_steps = tok[at + 3], max_rec = tok[at + 4];
        const uint32_t *len = &tok[at + 5];
        size_t total = 2 * size_t(n);
        for (int k = 0; k < 10; ++k) total += len[k];
        at += 15;
        REQUIRE(at + total <= tok.size());
        std::vector<uint32_t> rp(size_t(n) + 1, 0);
        for (uint32_t i = 0; i < n; ++i) rp[i + 1] = rp[i] + tok[at + i];
        const u32s step(tok.begin() + at + n, tok.begin() + at + 2 * size_t(n));
        for (uint32_t s : step) REQUIRE(s < n_steps);
        at += 2 * size_t(n);
        sbmbp::coloured_tables_t t;
        sbmbp::coloured_step_tables(rp.data(), n, step.data(), n_steps, cap, rcap, 256, t);
        const u32s *got[10] = {&t.rows, &t.loff, &t.seg_row0, &t.hub_row, &t.hub_rec, &t.frag_hub, &t.hub_frag0, &t.seg0, &t.hub0, &t.frag0};
        static const char *const names[10] = {"rows", "loff", "seg_row0", "hub_row", "hub_rec", "frag_hub", "hub_frag0", "seg0", "hub0", "frag0"};
        for (int k = 0; k < 10; ++k) {
            const u32s want(tok.begin() + at, tok.begin() + at + len[k]);
            at += len[k];
            if (*got[k] != want) {
                std::fprintf(stderr, "host_sanitize: %s plan %zu (cap %u, rcap %u, %u rows, %u steps): %s differs (%zu entries, expected %zu)\n", what, *count, cap,
                             rcap, n, n_steps, names[k], got[k]->size(), want.size());
                for (size_t i = 0; i < std::min(want.size(), got[k]->size()); ++i)
                    if ((*got[k])[i] != want[i]) { std::fprintf(stderr, "  first difference: entry %zu is %u, expected %u\n", i, (*got[k])[i], want[i]); break; }
                return 1;
            }
        }
        if (t.max_rec != max_rec) { std::fprintf(stderr, "host_sanitize: %s plan %zu: max_rec %u, expected %u\n", what, *count, t.max_rec, max_rec); return 1; }
        // the invariants the kernels rely on
        const size_t nseg = t.seg_row0.size() - 1, nhub = t.hub_row.size();
        REQUIRE(t.seg0.size() == size_t(n_steps) + 1 && t.hub0.size() == t.seg0.size() && t.frag0.size() == t.seg0.size());
        REQUIRE(t.seg0.back() == nseg && t.hub0.back() == nhub && t.frag0.back() == t.frag_hub.size() && t.hub_frag0.size() == nhub + 1);
        REQUIRE(t.rows.size() + nhub == n && t.loff.size() == t.rows.size() + nseg && t.hub_rec.size() == nhub);
        for (size_t b = 0; b < nseg; ++b) {  // a segment's block of loff: its rows' offsets, then its edge total
            const uint32_t r0 = t.seg_row0[b], r1 = t.seg_row0[b + 1];
            const uint32_t *lo = &t.loff[r0 + b];
            REQUIRE(r1 > r0 && r1 - r0 <= rcap && lo[0] == 0 && lo[r1 - r0] <= cap);
            for (uint32_t x = r0; x < r1; ++x) {
                REQUIRE(lo[x - r0 + 1] - lo[x - r0] == rp[t.rows[x] + 1] - rp[t.rows[x]] && step[t.rows[x]] == step[t.rows[r0]]);
                REQUIRE(x == r0 || t.rows[x] > t.rows[x - 1]);
            }
        }
        for (uint32_t s = 0; s < n_steps; ++s) {
            REQUIRE(t.seg0[s] <= t.seg0[s + 1] && t.hub0[s] <= t.hub0[s + 1] && t.frag0[s] == t.hub_frag0[t.hub0[s]]);
            REQUIRE(t.seg0[s + 1] - t.seg0[s] + t.hub0[s + 1] - t.hub0[s] <= t.max_rec);
            for (uint32_t b = t.seg0[s]; b < t.seg0[s + 1]; ++b) REQUIRE(step[t.rows[t.seg_row0[b]]] == s);
            for (uint32_t h = t.hub0[s]; h < t.hub0[s + 1]; ++h) {
                const uint32_t d = rp[t.hub_row[h] + 1] - rp[t.hub_row[h]];
                REQUIRE(step[t.hub_row[h]] == s && d > cap && t.hub_rec[h] == t.seg0[s + 1] - t.seg0[s] + h - t.hub0[s]);
                REQUIRE(t.hub_frag0[h + 1] - t.hub_frag0[h] == (d + 255) / 256);
                for (uint32_t f = t.hub_frag0[h]; f < t.hub_frag0[h + 1]; ++f) REQUIRE(t.frag_hub[f] == h);
            }
        }
    }
    REQUIRE(*count > 0);
    return 0;
}

static int test_step_plans_from_file(const char *path, size_t *count) {
    std::ifstream f(path);
    REQUIRE(f.good());
    u32s tok;
    for (uint32_t x; f >> x;) tok.push_back(x);
    REQUIRE(f.eof());
    return check_step_plans(tok, count, "step");
}

static int test_step_tables() {
    {   // cap 4, rcap 3, fragments of 256 edges, worked out by hand. Rows 0 .. 8 of 1 5 2 2 1 0 6 1 1 edges in steps
        // 1 0 1 1 1 2 0 1 1: step 0 is the two hubs alone; step 1 packs rows 0 2 | 3 4 7 | 8 (the edge limit, then the row
        // limit); step 2 is one row without an edge
        const u32s tok = {4, 3, 9, 3, 3, 7, 11, 5, 2, 2, 2, 3, 4, 4, 4,
                          1, 5, 2, 2, 1, 0, 6, 1, 1,  1, 0, 1, 1, 1, 2, 0, 1, 1,
                          0, 2, 3, 4, 7, 8, 5,  0, 1, 3, 0, 2, 3, 4, 0, 1, 0, 0,  0, 2, 5, 6, 7,  1, 6,  0, 1,  0, 1,  0, 1, 2,
                          0, 0, 3, 4,  0, 2, 2, 2,  0, 2, 2, 2};
        size_t count = 0;
        REQUIRE(check_step_plans(tok, &count, "hand-worked") == 0 && count == 1);
    }
    {   // no rows, no steps: the sentinels alone
        sbmbp::coloured_tables_t t;
        const uint32_t rp0 = 0;
        sbmbp::coloured_step_tables(&rp0, 0, nullptr, 0, 4, 3, 256, t);
        REQUIRE(t.rows.empty() && t.loff.empty() && t.seg_row0 == u32s{0} && t.hub_frag0 == u32s{0} && t.seg0 == u32s{0} && t.max_rec == 1);
    }
    // what build_coloured (engine.hip) built before the construction moved to host_graph.cpp, on two layouts
    static const uint32_t parent[] = {
#include "parent_step_tables.inc"
    };
    size_t count = 0;
    REQUIRE(check_step_plans(u32s(parent, parent + sizeof parent / sizeof parent[0]), &count, "recorded") == 0 && count == 2);
    return 0;
}

// ------------------------------------------------------------------------------------------ batch planner
static int test_planner() {
    using sbmbp::batch_planner;
    {
        batch_planner p(4, 1e-3);
        REQUIRE(p.next == 4);
        p.step(0.1, 2, 2);
        REQUIRE(p.next == 4);  // the first reading: nothing to compare with
        p.step(0.025, 4, 4);   // rate 0.5 per sweep, 0.025 -> 1e-3 needs ceil(4.64) = 5 more, none queued ahead
        REQUIRE(p.next == 4 && p.prev_md == 0.025 && p.prev_idx == 4);
    }
    {
        batch_planner p(8, 1e-3);
        p.step(0.1, 2, 2);
        p.step(0.025, 4, 8);  // 4 queued ahead of the reading: 5 - 4
        REQUIRE(p.next == 1);
        p.step(0.025, 5, 9);  // a reading that did not fall
        REQUIRE(p.next == 8 && p.prev_idx == 5);
        p.step(0.0, 6, 10);   // no difference reported: the previous reading stays
        REQUIRE(p.next == 8 && p.prev_md == 0.025 && p.prev_idx == 5);
        p.step(0.0005, 7, 10);  // already below the criterion
        REQUIRE(p.next == 1);
        p.reset();
        REQUIRE(p.next == 8 && p.prev_md == -1.0);
    }
    for (double crit : {0.0, -1.0}) {  // a criterion that is not positive
        batch_planner p(8, crit);
        p.step(0.1, 2, 2);
        p.step(0.025, 4, 8);
        REQUIRE(p.next == 8);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ the loops over fakes
struct shared_driver {
    static std::string planned(fakes::device &dev, double crit, uint32_t max_sweeps, uint32_t batch_max, bool psi_ok, bool first_explicit) {
        fakes::state cs{0.0, -1, 0, 0, 0};
        uint32_t psi = 0;
        sbmbp::batch_planner plan(std::max<uint32_t>(1, batch_max), crit);
        const int rc = sbmbp::converge_run(
            max_sweeps, plan, psi_ok, first_explicit,
            [&](int slot, uint32_t first, uint32_t n, bool form_psi) {
                for (uint32_t j = first; j < first + n; ++j) dev.sweep(j, form_psi && !(j == 0 && first_explicit));
                return dev.record(slot);
            },
            [&](int slot, fakes::state *st) {
                const int w = dev.wait(slot);
                if (w == 0) *st = dev.slots[slot][0];
                return w;
            },
            [&]() { return dev.resume(); }, &cs, &psi);
        return dev.end(rc, psi, plan.next, {cs});
    }
    static std::string fixed(fakes::device &dev, uint32_t max_sweeps, uint32_t batch_max) {
        std::vector<fakes::state> cs(dev.cur.size(), fakes::state{0.0, -1, 0, 0, 0});
        uint32_t done = 0;
        const int rc = sbmbp::queue_ahead(
            max_sweeps, done,
            [&](int slot) {
                const uint32_t n = std::min(batch_max, max_sweeps - done);
                for (uint32_t k = 0; k < n; ++k) dev.sweep(done + k, false);
                done += n;
                return dev.record(slot);
            },
            [&](int slot, bool *stopped) {
                const int w = dev.wait(slot);
                if (w != 0) return w;
                cs = dev.slots[slot];
                *stopped = std::all_of(cs.begin(), cs.end(), [](const fakes::state &s) { return s.stop != 0; });
                return 0;
            });
        return dev.end(rc, 0, batch_max, cs);
    }
    struct front {
        fakes::em_front &fe;
        uint32_t R;
        int converge(const double *crit, const uint8_t *active, uint32_t *executed) {
            for (uint32_t r = 0; r < R; ++r) executed[r] = active[r] ? fe.converge(r, crit[r]) : 0;
            return 0;
        }
        int expect(const uint8_t *active, double *na_e, double *, double *cab_e, double *f) {
            for (uint32_t r = 0; r < R; ++r) if (active[r]) f[r] = fe.expect(r, na_e + size_t(r) * fe.Q, cab_e + size_t(r) * fe.Q * fe.Q);
            return 0;
        }
        void params(uint32_t r, std::vector<uint32_t> &na, std::vector<double> &cab) { na = fe.na[r]; cab = fe.cab[r]; }
        int apply(uint32_t r, const uint32_t *na, const double *cab) { fe.apply(r, na, cab); return 0; }
        int finish(uint32_t r) { mix_at_finish = *mix; fe.finish(r); return 0; }
        const double *mix;
        double mix_at_finish;
    };
    static std::string em(fakes::em_front &fe, float crit, uint32_t max_time, double lr) {
        double field_mix = 1.0;
        const uint32_t R = uint32_t(fe.f.size());
        std::vector<fakes::em_result> out(R);
        front f{fe, R, &field_mix, -1.0};
        const int rc = sbmbp::em_loop(f, R, fe.Q, fe.N, crit, max_time, double(float(lr)), 1.0, field_mix, 0.3, out.data());
        return fakes::em_end(fe, rc, out, f.mix_at_finish, field_mix);
    }
};

static int test_loops() {
    static const char *const expected[] = {
#include "parent_traces.inc"
    };
    const std::vector<std::string> got = fakes::run_cases<shared_driver>();
    REQUIRE(got.size() == sizeof expected / sizeof expected[0]);
    for (size_t i = 0; i < got.size(); ++i)
        if (got[i] != expected[i]) {
            std::fprintf(stderr, "host_sanitize: loop case %zu\n  got      %s\n  expected %s\n", i, got[i].c_str(), expected[i]);
            return 1;
        }
    // what the recorded traces say, spelled out for the cases that matter most (so that a wrong recording cannot pass either)
    const auto head = [&](size_t i) { return got[i].substr(0, got[i].find(" |")); };
    REQUIRE(head(0).empty() && head(10).empty());                                     // max_sweeps = 0 queues nothing
    REQUIRE(head(1) == " s0m r0 w0");                                                 // one queue, one wait, no drain
    REQUIRE(head(2) == " s0m s1m r0 s2m s3m r1 w0 s4m r0 w1 w0");                     // 2, 2, 1 on slots 0, 1, 0
    REQUIRE(got[2].find("inflight=2") != std::string::npos);
    REQUIRE(head(3) == " s0m s1m r0 s2m s3m r1 w0 s4m s5m r0 w1 w0");                 // the stop shows in slot 1: one more wait, on slot 0
    REQUIRE(got[3].find("[3,1,0,3,") != std::string::npos);
    REQUIRE(head(4) == head(2));                                                      // a stop in the final batch: no further wait
    REQUIRE(head(15) == " s0p s1p s2p r0 s3p s4p s5p r1 w0 w1 R s3m s4m s5m r0 s6m s7m s8m r1 w0 s9m r0 w1 w0");
    REQUIRE(got[15].find("psi=3 next=3") != std::string::npos && got[15].find("[10,0,0,") != std::string::npos);
    REQUIRE(head(7) == " s0m s1m r0 s2m s3m r1" && head(8) == " s0m s1m r0 s2m s3m r1 w0" && head(9) == " s0m s1m r0");  // errors end it at once
    for (size_t i : {7, 8, 9, 19, 20}) REQUIRE(got[i].find("rc=7") != std::string::npos);
    REQUIRE(got[22].find("[1,1,-1.5,7]") != std::string::npos);                       // constant: status 1 after one step; 3 + 4 sweeps
    REQUIRE(got[23].find(" A") == std::string::npos && got[23].find("[0,2,nan,3]") != std::string::npos);
    REQUIRE(got[24].find(" A") == std::string::npos && got[24].find("[0,2,inf,3]") != std::string::npos);
    REQUIRE(got[25].find("[6,0,6,33]") != std::string::npos);                         // out of steps: status 0, em_steps = max_time
    REQUIRE(got[26].find(" C0:" + fakes::num(double(float(2.0 * 0.1)))) == 0);        // tightened before the first run
    REQUIRE(head(27) == " F0" && got[27].find("[0,0,0,0]") != std::string::npos);     // no round, one finish
    const auto result = [&](size_t i, size_t k) {  // the k-th [..] group of case i
        size_t at = got[i].find(" |");
        for (size_t x = 0; x <= k; ++x) at = got[i].find('[', at + 1);
        return got[i].substr(at, got[i].find(']', at) - at + 1);
    };
    for (size_t r = 0; r < 3; ++r) REQUIRE(result(28, r) == result(29 + r, 0));        // in a batch as alone
    REQUIRE(head(28).rfind(" C0:") == head(28).find(" C0:", 10) && head(28).find(" E0", head(28).find(" A1:53")) == std::string::npos);  // an ended run is left alone
    for (size_t i = 22; i < got.size(); ++i) REQUIRE(got[i].find("mix=" + fakes::num(0.3) + "/1 ") != std::string::npos);  // lowered until the last finish, then restored
    return 0;
}

// ------------------------------------------------------------------------------------------ reduction arithmetic
static int test_reduce_tables() {
    using namespace sbmbp;
    // the 5120-entry budget: 8 + 64 + 512 + 4096 = 4680, 16 + 256 + 4096 = 4368, 17 + 289 + 4913 = 5219 > 5120
    const uint32_t qs[] = {2, 8, 9, 16, 17, 64};
    const int caps[] = {4, 4, 3, 3, 2, 2};
    for (int i = 0; i < 6; ++i) REQUIRE(max_series_order(qs[i]) == caps[i]);
    REQUIRE(series_len(8, 4) == 4680 && series_len(16, 3) == 4368 && series_len(17, 3) == 5219 && series_len(64, 2) == 4160);
    REQUIRE(series_len(5, 0) == 0 && series_len(5, 1) == 5);
    // a requested order is honoured and clamped to the cap
    REQUIRE(series_order(2, 1000000, 3, 100.0) == 3 && series_order(2, 1000000, 7, 0.1) == 4 && series_order(9, 1000000, 4, 0.1) == 3);
    // N = 1e6: order 1 leaves wmax^2 / 4N, order 2 wmax^3 / 6N^2 (< 1e-12 below wmax = 6^(1/3) = 1.817), order 3 wmax^4 / 8N^3
    REQUIRE(series_order(2, 1000000, 0, 1.8) == 2 && series_order(2, 1000000, 0, 1.85) == 3);
    REQUIRE(series_order(2, 1000000, 0, 1e-4) == 1);
    // Q = 17, N = 4e4, wmax = 10: the cap's order 2 leaves 1e3 / (6 * 1.6e9) = 1e-7, no order meets the bound
    REQUIRE(series_order(17, 40000, 0, 10.0) == 2);
    for (uint32_t N : {32768u, 32769u}) {
        REQUIRE(nonedge_is_exact(0, N) == (N == 32768));
        REQUIRE(nonedge_is_exact(1, N) && !nonedge_is_exact(2, N));
    }
    {
        const double sums[4] = {8, 16, 2, 4}, c = 4;
        double p[4];
        site_edge_parts(4, nullptr, sums, p);
        REQUIRE(p[0] == 2 && p[1] == 2 && p[2] == 0.5 && p[3] == 0.5);
        site_edge_parts(4, &c, sums, p);  // the dc 1 constant: + c / N and + c / 2N, the entropy twin untouched
        REQUIRE(p[0] == 3 && p[1] == 2.5 && p[2] == 0.5 && p[3] == 0.5);
        const double fp[3] = {3, 2.5, 0.25}, ep[3] = {0.5, 0.75, 0.5};
        REQUIRE(free_energy_of(fp) == -0.25 && entropy_of(ep) == -0.25);
        const double all[2] = {10, 7}, adj[2] = {2, 3};
        double ne[2];
        nonedge_finish(all, adj, 4, ne);
        REQUIRE(ne[0] == 1 && ne[1] == 0.5);
    }
    {   // numerators (0,0), (0,1), (1,1) = 3, 5, 7 at N = 10
        const double tri[3] = {3, 5, 7}, na0[2] = {4, 0}, na[2] = {4, 8}, nna[2] = {8, 16};
        double ce[4];
        em_rescale(2, 10, 0, na0, nna, tri, ce);  // label 1 has no mass: only (0,0) is scaled, by 2 N / (4 * 4)
        REQUIRE(ce[0] == 3.75 && ce[1] == 5 && ce[2] == 5 && ce[3] == 7);
        em_rescale(2, 10, 0, na, nna, tri, ce);   // dc 0 divides by na: 3 * 20 / 16, 5 * 10 / 32, 7 * 20 / 64
        REQUIRE(ce[0] == 3.75 && ce[1] == 1.5625 && ce[2] == 1.5625 && ce[3] == 2.1875);
        em_rescale(2, 10, 1, na, nna, tri, ce);   // dc 1 by nna: 3 * 20 / 64, 5 * 10 / 128, 7 * 20 / 256
        REQUIRE(ce[0] == 0.9375 && ce[1] == 0.390625 && ce[2] == 0.390625 && ce[3] == 0.546875);
    }
    for (uint32_t Q : {3u, 9u}) {  // 1 on the diagonal, 5 one step to the right of it: the cyclic shift collects 5 Q, the identity Q
        std::vector<double> C(Q * Q, 0.0);
        for (uint32_t a = 0; a < Q; ++a) { C[a * Q + a] = 1; C[a * Q + (a + 1) % Q] = 5; }
        REQUIRE(best_overlap(Q, 20, C.data()) == (Q == 3 ? 15.0 / 20.0 : 9.0 / 20.0));
    }
    {
        const double nanv = std::nan(""), f[4] = {-1.0, nanv, -3.0, -2.0};
        const int r0[4] = {1, 0, 1, 0}, r1[4] = {1, 0, 1, 1};
        REQUIRE(best_replica(4, f, r0, 2) == 3 && best_replica(4, f, r1, 2) == 2 && best_replica(1, f + 1, r0 + 1, 2) == 0);
    }
    return 0;
}

// the oracle's converged marginals on a shipped graph; moment tensors and adjacent-pair sums formed here with plain loops in
// row order; {f_nonedge, e_nonedge} through host_reduce.h against the oracle's series at every order the engine can take
static int test_reduce_against_oracle(const std::string &path, uint32_t N, uint32_t Q, double eps, double c) {
    using namespace sbmbp;
    void *og = orc_graph_load_edgelist(path.c_str(), N);
    REQUIRE(orc_graph_n(og) == N && orc_graph_e2(og) > 0);
    const uint64_t E2 = orc_graph_e2(og);
    std::vector<uint64_t> rp(size_t(N) + 1);
    std::vector<uint32_t> nbr(E2), rev(E2), tc(N), na(Q);
    orc_graph_copy(og, rp.data(), nbr.data(), rev.data());
    for (uint32_t i = 0; i < N; ++i) tc[i] = uint32_t(uint64_t(i) * Q / N);
    std::vector<double> cab(Q * Q), psi(size_t(N) * Q), msg(E2 * Q);
    orc_param_from_epsilon_c(N, Q, eps, c, cab.data(), na.data());
    void *bp = orc_bp_create(og, Q, 0);
    void *rng = orc_rng_create(1);
    orc_bp_init_messages(bp, 0, nullptr, tc.data(), rng);
    orc_bp_set_params(bp, cab.data(), na.data(), 1.0);
    double last = 1.0;
    REQUIRE(orc_bp_converge_sync(bp, 1e-9, 2000, 1.0, &last) >= 0 && last < 1e-9);
    orc_bp_get_state(bp, psi.data(), msg.data());
    std::vector<double> mats(3 * Q * Q), v(Q * Q);
    double wmax = 0.0;
    nonedge_mats(Q, N, cab.data(), 1.0, mats.data(), &wmax);
    REQUIRE(wmax >= *std::max_element(cab.begin(), cab.end()));
    const double *wmat = mats.data(), *cabm = mats.data() + 2 * Q * Q;
    for (uint32_t a = 0; a < Q * Q; ++a) v[a] = cabm[a] * std::log(cabm[a]);
    const int Kmax = max_series_order(Q);
    std::vector<double> Mk(series_len(Q, Kmax), 0.0), t, tn;
    for (uint32_t i = 0; i < N; ++i) {  // M_k[a_0 + Q a_1 + ...] = sum_i psi_i[a_0] psi_i[a_1] ...
        const double *p = psi.data() + size_t(i) * Q;
        t.assign(1, 1.0);
        size_t off = 0;
        for (int k = 1; k <= Kmax; ++k) {
            tn.resize(t.size() * Q);
            for (size_t rest = 0; rest < t.size(); ++rest)
                for (uint32_t a = 0; a < Q; ++a) tn[a + Q * rest] = p[a] * t[rest];
            t.swap(tn);
            for (size_t x = 0; x < t.size(); ++x) Mk[off + x] += t[x];
            off += t.size();
        }
    }
    double adj[2] = {0.0, 0.0};
    for (uint32_t i = 0; i < N; ++i)
        for (uint64_t k = rp[i]; k < rp[i + 1]; ++k) {
            const double *pi = psi.data() + size_t(i) * Q, *pl = psi.data() + size_t(nbr[k]) * Q;
            double y = 0.0, u = 0.0, yc = 0.0;
            for (uint32_t a = 0; a < Q; ++a)
                for (uint32_t b = 0; b < Q; ++b) {
                    const double pp = pi[a] * pl[b];
                    y += wmat[a * Q + b] * pp;
                    u += v[a * Q + b] * pp;
                    yc += cabm[a * Q + b] * pp;
                }
            adj[0] += std::log1p(-y / N);
            adj[1] += (u / N) / (1.0 - yc / N);
        }
    double worst = 0.0;
    for (int K = 1; K <= Kmax; ++K) {
        double all[2], got[2], want[2];
        nonedge_series(Q, N, K, true, Mk.data(), mats.data(), all);
        nonedge_finish(all, adj, N, got);
        orc_bp_nonedge(bp, K, want);
        for (int x = 0; x < 2; ++x) {
            const double rel = std::fabs(got[x] - want[x]) / std::max(1.0, std::fabs(want[x]));
            worst = std::max(worst, rel);
            if (!(rel <= 1e-11)) {
                std::fprintf(stderr, "host_sanitize: non-edge series Q=%u K=%d part %d: %.17g, the oracle %.17g (relative %.3g)\n", Q, K, x, got[x], want[x], rel);
                return 1;
            }
        }
        double f_only[2];  // without the entropy the free-energy half is the same number
        nonedge_series(Q, N, K, false, Mk.data(), mats.data(), f_only);
        REQUIRE(f_only[0] == all[0] && f_only[1] == 0.0);
    }
    std::printf("host_sanitize: non-edge series Q=%u, orders 1..%d against the oracle: largest relative difference %.3g\n", Q, Kmax, worst);
    orc_rng_free(rng);
    orc_bp_free(bp);
    orc_graph_free(og);
    return 0;
}

// Fixed inputs of the bit-for-bit comparison: N of the whole graph is not the rows of a shard, beta is not 1.
struct reduce_case {
    uint32_t Q, N;
    double beta, dc1, sums[4], adj[2];
    std::vector<double> cab, Mk, na, nna, tri, C;
};
static reduce_case make_reduce_case(uint32_t Q) {
    reduce_case c;
    c.Q = Q;
    c.N = 50021;  // (three shards of 16674, 16674 and 16673 rows)
    c.beta = 0.8;
    uint64_t s = 0x9e3779b97f4a7c15ull * Q;
    auto u = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return double(s >> 11) * (1.0 / 9007199254740992.0); };
    c.cab.resize(Q * Q);
    for (uint32_t a = 0; a < Q; ++a)
        for (uint32_t b = a; b < Q; ++b) c.cab[a * Q + b] = c.cab[b * Q + a] = (a == b ? 9.25 : 1.75) + 0.5 * u();
    const int Kmax = sbmbp::max_series_order(Q);
    c.Mk.resize(sbmbp::series_len(Q, Kmax));
    size_t off = 0, tsz = 1;
    for (int k = 1; k <= Kmax; ++k) {
        tsz *= Q;
        for (size_t x = 0; x < tsz; ++x) c.Mk[off + x] = double(c.N) * (0.5 + u()) / double(tsz);
        off += tsz;
    }
    c.na.resize(Q); c.nna.resize(Q);
    for (uint32_t q = 0; q < Q; ++q) { c.na[q] = double(c.N) * (0.5 + u()) / Q; c.nna[q] = 6.5 * c.na[q] * (0.9 + 0.2 * u()); }
    c.tri.resize(Q * (Q + 1) / 2);
    for (double &x : c.tri) x = 40.0 * u();
    c.C.resize(Q * Q);
    for (double &x : c.C) x = double(c.N) * u() / Q;
    for (double &x : c.sums) x = -3.0 * double(c.N) * (0.5 + u());
    for (double &x : c.adj) x = -7.0 * (0.5 + u());
    c.dc1 = 2.0 * double(c.N) * (1.0 + u());
    return c;
}

// every value host_reduce.h computes from a case, in the order parent_reduce.inc holds them
static std::vector<double> reduce_values(const reduce_case &c) {
    using namespace sbmbp;
    const uint32_t Q = c.Q, N = c.N;
    std::vector<double> out, mats(3 * Q * Q);
    double wmax = 0.0;
    nonedge_mats(Q, N, c.cab.data(), c.beta, mats.data(), &wmax);
    out = mats;
    out.push_back(wmax);
    const int Kmax = max_series_order(Q);
    for (double wm : {wmax, 0.5, 40.0, 3000.0})
        for (int req = 0; req <= 5; ++req) out.push_back(double(series_order(Q, N, req, wm)));
    for (int K = 0; K <= Kmax; ++K) out.push_back(double(series_len(Q, K)));
    double ne[2] = {0.0, 0.0};
    for (int K = 1; K <= Kmax; ++K)
        for (int ent = 0; ent < 2; ++ent) {
            double all[2];
            nonedge_series(Q, N, K, ent != 0, c.Mk.data(), mats.data(), all);
            nonedge_finish(all, c.adj, N, ne);
            out.insert(out.end(), {all[0], all[1], ne[0], ne[1]});
        }
    for (int dc1 = 0; dc1 < 2; ++dc1) {  // (ne: the last series above, highest order with the entropy)
        double p[4];
        site_edge_parts(N, dc1 ? &c.dc1 : nullptr, c.sums, p);
        const double fp[3] = {p[0], p[1], ne[0]}, ep[3] = {p[2], p[3], ne[1]};
        out.insert(out.end(), {p[0], p[1], p[2], p[3], free_energy_of(fp), entropy_of(ep)});
    }
    for (uint32_t dc = 0; dc < 2; ++dc) {
        std::vector<double> ce(Q * Q, 0.0);
        em_rescale(Q, N, dc, c.na.data(), c.nna.data(), c.tri.data(), ce.data());
        out.insert(out.end(), ce.begin(), ce.end());
    }
    out.push_back(best_overlap(Q, N, c.C.data()));
    return out;
}

static int test_reduce_against_parent() {
    static const char *const expected[] = {  // hex floats as text: C++14 has no hexadecimal floating literal
#include "parent_reduce.inc"
    };
    const size_t n_expected = sizeof expected / sizeof expected[0];
    size_t at = 0;
    for (uint32_t Q : {2u, 5u, 16u}) {
        const std::vector<double> got = reduce_values(make_reduce_case(Q));
        REQUIRE(at + got.size() <= n_expected);
        for (size_t i = 0; i < got.size(); ++i, ++at) {
            const double want = std::strtod(expected[at], nullptr);
            if (std::memcmp(&got[i], &want, 8) != 0) {
                std::fprintf(stderr, "host_sanitize: reduce case Q=%u value %zu: %a, the replaced code gave %s\n", Q, i, got[i], expected[at]);
                return 1;
            }
        }
    }
    REQUIRE(at == n_expected);
    return 0;
}

static int test_reduce(const char *dataset) {
    const std::string dir = std::string(dataset).substr(0, std::string(dataset).find_last_of('/') + 1);
    if (test_reduce_tables() != 0) return 1;
    if (test_reduce_against_oracle(dir + "q4_n400.edgelist", 400, 4, 0.05, 6.0) != 0) return 1;
    if (test_reduce_against_oracle(dir + "q10_n1000.edgelist", 1000, 10, 0.05, 15.0) != 0) return 1;
    return test_reduce_against_parent();
}

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: host_sanitize <edge list of the shipped data set> [--plans <file> | --chunk-plans <file> | --step-plans <file>]\n"); return 2; }
    if (argc == 4 && std::strcmp(argv[2], "--plans") == 0) {  // the plan comparison alone
        size_t count = 0;
        const int prc = test_plans_from_file(argv[3], &count);
        if (prc == 0) std::printf("host_sanitize ok: %zu plans\n", count);
        return prc;
    }
    if (argc == 4 && std::strcmp(argv[2], "--chunk-plans") == 0) {  // the chunked plan comparison alone
        size_t count = 0;
        const int prc = test_chunk_plans_from_file(argv[3], &count);
        if (prc == 0) std::printf("host_sanitize ok: %zu chunked plans\n", count);
        return prc;
    }
    if (argc == 4 && std::strcmp(argv[2], "--step-plans") == 0) {  // the step tables of the coloured order alone
        size_t count = 0;
        const int prc = test_step_plans_from_file(argv[3], &count);
        if (prc == 0) std::printf("host_sanitize ok: %zu step plans\n", count);
        return prc;
    }
    int rc = run(argv[1]);
    if (rc == 0) rc = test_segment_plan(argv[1]);
    if (rc == 0) rc = test_step_tables();
    if (rc == 0) rc = test_planner();
    if (rc == 0) rc = test_loops();
    if (rc == 0) rc = test_reduce(argv[1]);
    if (rc == 0) std::printf("host_sanitize ok\n");
    return rc;
}
