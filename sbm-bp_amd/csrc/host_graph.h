// Host-side graph + parameter utilities of the engine (C++14, no device code).
#ifndef SBMBP_HOST_GRAPH_H
#define SBMBP_HOST_GRAPH_H

#include <cstdint>
#include <string>
#include <functional>
#include <vector>

struct sbmbp_graph {
    uint32_t n = 0;                 // vertices
    std::vector<uint64_t> row_ptr;  // n+1
    std::vector<uint32_t> nbr;      // E2, ascending per row
    std::vector<uint32_t> rev;      // E2, index of the reverse directed edge
    uint32_t max_degree = 0;
    uint64_t e2() const { return nbr.size(); }
    uint32_t deg(uint32_t i) const { return uint32_t(row_ptr[i + 1] - row_ptr[i]); }
};

namespace sbmbp {

void set_error(const std::string &msg);
const std::string &get_error();
int arg_error(const char *func, int line);  // SBMBP_ERR_ARG with a message that names the check (never a stale one)

// returns 0 or an SBMBP_ERR_* code
int graph_from_pairs(sbmbp_graph &g, const uint32_t *pairs, uint64_t n_pairs, uint32_t n_vertices);
int graph_from_csr(sbmbp_graph &g, uint32_t n, uint64_t e2, const uint64_t *row_ptr, const uint32_t *nbr,
                   const uint32_t *rev);
int read_edgelist(const char *path, std::vector<uint32_t> &pairs);
int read_int_column(const char *path, std::vector<int64_t> &values);  // load_beliefs/load_confs format
// per-vertex prior file (sbmbp_prior_load): one line "vertex w_0 .. w_{Q-1}" per annotated vertex, any order; prior[n*Q] is
// filled with ones where no line names the vertex. SBMBP_ERR_IO: unreadable; SBMBP_ERR_ARG with the line number: id >= n, a
// vertex named twice, a wrong column count, a value that is no finite number >= 0, a line without a positive weight
int read_prior_table(const char *path, uint32_t n, uint32_t Q, double *prior, uint64_t *n_rows_given);

void param_from_epsilon_c(uint32_t N, uint32_t Q, double epsilon, double c, double *cab, uint32_t *na);
void param_from_direct(uint32_t N, uint32_t Q, const double *pa, const double *cab_upper, double *cab, uint32_t *na);

// init_messages (belief_propagation.cpp:101-217) on the out-ordered layout; fills psi (N*Q) and
// msg (E2*Q), both caller-allocated (need not be initialised), from std::mt19937(seed) in the reference's
// draw order.
// With a sink, psi/msg may be null: the rows are produced in slabs of consecutive vertices [lo, hi) and each slab is
// handed over when complete (psi_rows: (hi-lo)*Q doubles, msg_rows: (row_ptr[hi]-row_ptr[lo])*Q doubles, valid during the
// call) while the generator already works on the next one.
struct state_sink {
    // optional: provide the two slab buffers (e.g. page-locked memory); default new[]
    std::function<bool(uint64_t psi_doubles, uint64_t msg_doubles, double **psi_buf, double **msg_buf)> alloc;
    std::function<void(uint32_t lo, uint32_t hi, const double *psi_rows, const double *msg_rows)> put;
};
void init_state_host(uint32_t n, const uint32_t *row_ptr, uint64_t e2, uint32_t Q, uint32_t flag, const int32_t *conf,
                     uint32_t seed, double *psi, double *msg, const state_sink *sink = nullptr);

// the coloured sweep order (sbmbp_coloured_plan): colour and step of every vertex; colour_in null = greedy colouring
int coloured_plan(uint32_t n, const uint64_t *row_ptr, const uint32_t *nbr, const uint32_t *colour_in, double step_fraction,
                  std::vector<uint32_t> &colour, std::vector<uint32_t> &step, uint32_t *n_colours, uint32_t *n_steps);

// The work decomposition of a row range: greedy segments of at most cap edges and rcap rows; a row above cap is a hub
// segment of its own. chunk_row = the row chunks' boundaries (first 0, last n, monotone; empty = one chunk [0, n]): no
// segment straddles one. Segment b covers rows blk_row[b] .. blk_row[b + 1] and starts at edge blk_e0[b]; hub h is row
// hub_row[h] = segment hub_blk[h]; chunk c owns segments chunk_blk[c] .. chunk_blk[c + 1] and hubs chunk_hub[c] .. [c + 1].
struct segment_plan_t {
    std::vector<uint32_t> blk_row, blk_e0, hub_row, hub_blk, chunk_blk, chunk_hub;
};
void segment_plan(const uint64_t *row_ptr, uint32_t n, uint32_t cap, uint32_t rcap, const std::vector<uint32_t> &chunk_row,
                  segment_plan_t &out);

// The tables of the coloured order from the step of every vertex (coloured_plan): rows ascending inside a step, greedy
// segments of at most cap edges and rcap rows; a row above cap is a hub of its step, set aside WITHOUT closing the open
// segment. Segment b (numbered over all steps) holds rows[seg_row0[b] .. seg_row0[b + 1]]; loff holds, per segment, the
// edge offset of each of its rows relative to the segment and then the segment's edge total, so the block of segment b
// starts at loff[seg_row0[b] + b]. Hubs are numbered in step order: hub h is row hub_row[h], writes record hub_rec[h] =
// (segments of its step) + (its index among the step's hubs) and owns fragments hub_frag0[h] .. hub_frag0[h + 1] of `frag`
// edges, frag_hub[f] = hub of fragment f. Step s owns segments seg0[s] .. seg0[s + 1], hubs hub0[s] .. hub0[s + 1] and
// fragments frag0[s] .. frag0[s + 1]; max_rec = the most records (segments + hubs) of any step, at least 1.
struct coloured_tables_t {
    std::vector<uint32_t> rows, loff, seg_row0, hub_row, hub_rec, frag_hub, hub_frag0, seg0, hub0, frag0;
    uint32_t max_rec = 1;
};
void coloured_step_tables(const uint32_t *row_ptr, uint32_t n, const uint32_t *step, uint32_t n_steps, uint32_t cap, uint32_t rcap,
                          uint32_t frag, coloured_tables_t &out);

// learning_step (bp.cpp:53-75): the new group sizes and affinities of one EM step, in place in na / cab
void learning_step_host(uint32_t Q, uint32_t N, double learning_rate, double learn_snap, double crit, const double *na_e,
                        const double *cab_e, uint32_t *na, double *cab);

}  // namespace sbmbp
#endif
