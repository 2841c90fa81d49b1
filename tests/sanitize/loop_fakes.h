// Scripted stand-ins for the device side of the host drivers (csrc/host_loops.h), and the cases they are driven through.
// A driver is the host loop under test with its device calls replaced by these fakes; every fake call is appended to a
// trace. The expected traces (parent_traces.inc) were recorded by giving run_cases() drivers made of the loops as they stood
// BEFORE they were shared (run_sweeps, run_sweeps_coloured / batch_run, sbmbp_learning, sbmbp_batch_learning, copied out with
// the same substitutions), so the shared loops are held to what the separate ones did, call for call.
#ifndef SBMBP_TEST_LOOP_FAKES_H
#define SBMBP_TEST_LOOP_FAKES_H

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

namespace fakes {

struct state { double maxdiff; int conv_iter, sweep_idx, stop, pause; };

inline std::string num(double v) { char b[40]; std::snprintf(b, sizeof b, "%.17g", v); return b; }

// R replicas behind one in-order stream. Replica r stops after its stop_at[r]-th executed sweep (never if < 0); a stop of a
// marginal-gather sweep with pause_at_stop is a pause. A stopped replica skips the sweeps queued behind the stop. The
// difference halves with every executed sweep. fail_queue / fail_wait: the n-th record / wait call (from 0) returns 7.
struct device {
    std::vector<int> stop_at;
    bool pause_at_stop = false;
    int fail_queue = -1, fail_wait = -1;
    std::vector<state> cur, slots[2];
    std::string trace;
    int n_record = 0, n_wait = 0, in_flight = 0, max_in_flight = 0;
    explicit device(std::vector<int> stop_at_) : stop_at(std::move(stop_at_)), cur(stop_at.size(), state{0.0, -1, 0, 0, 0}) {
        slots[0] = slots[1] = cur;
    }
    void sweep(uint32_t j, bool form_psi) {
        trace += " s" + std::to_string(j) + (form_psi ? "p" : "m");
        for (size_t r = 0; r < cur.size(); ++r) {
            state &c = cur[r];
            if (c.stop) continue;
            c.sweep_idx++;
            c.maxdiff = std::ldexp(1.0, -c.sweep_idx);
            if (c.sweep_idx == stop_at[r]) {
                c.stop = 1;
                c.conv_iter = c.sweep_idx;
                if (pause_at_stop && form_psi) { c.pause = 1; c.conv_iter = -1; pause_at_stop = false; stop_at[r] = -1; }
            }
        }
    }
    int record(int slot) {
        trace += " r" + std::to_string(slot);
        if (n_record++ == fail_queue) return 7;
        slots[slot] = cur;
        max_in_flight = std::max(max_in_flight, ++in_flight);
        return 0;
    }
    int wait(int slot) {
        trace += " w" + std::to_string(slot);
        if (n_wait++ == fail_wait) return 7;
        --in_flight;
        return 0;
    }
    int resume() {
        trace += " R";
        for (state &c : cur) c.stop = c.pause = 0;
        return 0;
    }
    std::string end(int rc, uint32_t psi_count, uint32_t next_batch, const std::vector<state> &fin) {
        std::string s = trace + " | rc=" + std::to_string(rc) + " psi=" + std::to_string(psi_count) + " next=" + std::to_string(next_batch) +
                        " inflight=" + std::to_string(max_in_flight);
        for (const state &c : fin)
            s += " [" + std::to_string(c.sweep_idx) + "," + std::to_string(c.stop) + "," + std::to_string(c.pause) + "," + std::to_string(c.conv_iter) + "," + num(c.maxdiff) + "]";
        return s;
    }
};

// an EM front end: run r's free energy in round t is f[r][t] (the last value repeats), its converge call executes
// 3 + t sweeps, the expectations are fixed (nothing depends on r: a run in a batch must fare as it does alone)
struct em_front {
    std::vector<std::vector<double>> f;
    std::vector<int> round;
    std::vector<std::vector<uint32_t>> na;
    std::vector<std::vector<double>> cab;
    std::string trace;
    uint32_t Q = 2, N = 100;
    explicit em_front(std::vector<std::vector<double>> f_) : f(std::move(f_)), round(f.size(), 0) {
        for (size_t r = 0; r < f.size(); ++r) { na.push_back({50u, 50u}); cab.push_back({4.0, 1.0, 1.0, 4.0}); }
    }
    uint32_t converge(uint32_t r, double crit) {
        trace += " C" + std::to_string(r) + ":" + num(crit);
        return 3u + uint32_t(round[r]);
    }
    double expect(uint32_t r, double *na_e, double *cab_e) {
        trace += " E" + std::to_string(r);
        na_e[0] = 60.25; na_e[1] = 39.75;
        cab_e[0] = 5.0; cab_e[1] = cab_e[2] = 0.5; cab_e[3] = 3.0;
        const std::vector<double> &s = f[r];
        const double v = s[std::min<size_t>(size_t(round[r]), s.size() - 1)];
        round[r]++;
        return v;
    }
    void apply(uint32_t r, const uint32_t *na_, const double *cab_) {
        na[r].assign(na_, na_ + Q);
        cab[r].assign(cab_, cab_ + Q * Q);
        trace += " A" + std::to_string(r) + ":" + std::to_string(na_[0]) + "," + std::to_string(na_[1]) + ":" + num(cab_[0]) + "," + num(cab_[1]);
    }
    void finish(uint32_t r) { trace += " F" + std::to_string(r); }
};

struct em_result { int em_steps, status; double free_energy; uint64_t total_sweeps; };

inline std::string em_end(const em_front &fe, int rc, const std::vector<em_result> &out, double field_mix_inside, double field_mix_after) {
    std::string s = fe.trace + " | rc=" + std::to_string(rc) + " mix=" + num(field_mix_inside) + "/" + num(field_mix_after);
    for (const em_result &o : out)
        s += " [" + std::to_string(o.em_steps) + "," + std::to_string(o.status) + "," + num(o.free_energy) + "," + std::to_string(o.total_sweeps) + "]";
    return s;
}

// Drivers:
//   std::string D::planned(device &, double crit, uint32_t max_sweeps, uint32_t batch_max, bool psi_ok, bool first_explicit)
//       the convergence run of the single engine / a shard rank (planned batches, pause handling); one replica
//   std::string D::fixed(device &, uint32_t max_sweeps, uint32_t batch_max)
//       fixed batches, stopped = every replica has (the replica batch; the coloured order with one replica)
//   std::string D::em(em_front &, float crit, uint32_t max_time, double lr)      R = fe.f.size() runs in step
template <class D> std::vector<std::string> run_cases() {
    std::vector<std::string> out;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto planned = [&](std::vector<int> stop_at, bool pause, int fq, int fw, double crit, uint32_t max_sweeps, uint32_t batch_max, bool psi_ok,
                       bool first_explicit) {
        device dev(stop_at);
        dev.pause_at_stop = pause; dev.fail_queue = fq; dev.fail_wait = fw;
        out.push_back(D::planned(dev, crit, max_sweeps, batch_max, psi_ok, first_explicit));
    };
    auto fixed = [&](std::vector<int> stop_at, int fq, int fw, uint32_t max_sweeps, uint32_t batch_max) {
        device dev(stop_at);
        dev.fail_queue = fq; dev.fail_wait = fw;
        out.push_back(D::fixed(dev, max_sweeps, batch_max));
    };
    // ---- queue-ahead, fixed batches
    fixed({-1}, -1, -1, 0, 4);              // 0: nothing to do
    fixed({-1}, -1, -1, 1, 1);              // 1: one sweep
    fixed({-1}, -1, -1, 5, 2);              // 2: 2, 2, 1 on slots 0, 1, 0
    fixed({3}, -1, -1, 10, 2);              // 3: stop seen with a batch queued ahead
    fixed({5}, -1, -1, 5, 2);               // 4: stop in the final batch
    fixed({2, 5, 3}, -1, -1, 12, 2);        // 5: three replicas: ends when the last has stopped
    fixed({2, -1, 3}, -1, -1, 7, 3);        // 6: one replica never stops
    fixed({-1}, 1, -1, 9, 2);               // 7: the second queue fails
    fixed({-1}, -1, 0, 9, 2);               // 8: the first wait fails
    fixed({-1}, 0, -1, 9, 2);               // 9: the first queue fails
    // ---- planned batches and the pause
    planned({-1}, false, -1, -1, -1.0, 0, 4, true, false);     // 10
    planned({-1}, false, -1, -1, -1.0, 1, 1, true, true);      // 11
    planned({-1}, false, -1, -1, -1.0, 5, 2, false, false);    // 12
    planned({3}, false, -1, -1, -1.0, 10, 2, true, false);     // 13
    planned({5}, false, -1, -1, -1.0, 5, 2, true, true);       // 14
    planned({3}, true, -1, -1, -1.0, 10, 3, true, false);      // 15: pause at sweep 3 of 10 with 6 queued
    planned({3}, true, -1, -1, -1.0, 10, 3, true, true);       // 16: the same, sweep 0 in the explicit form
    planned({12}, false, -1, -1, 1e-3, 40, 4, true, false);    // 17: the planner shortens the batches near 2^-10 < 1e-3
    planned({9}, true, -1, -1, 1e-3, 40, 4, true, false);      // 18: a pause while the planner is at work
    planned({-1}, false, 2, -1, -1.0, 9, 2, true, false);      // 19: the third queue fails
    planned({-1}, false, -1, 1, -1.0, 9, 2, true, false);      // 20: the second wait fails
    planned({2}, true, -1, -1, -1.0, 2, 2, true, false);       // 21: pause at the very last sweep
    // ---- EM loop
    auto em = [&](std::vector<std::vector<double>> f, float crit, uint32_t max_time, double lr) {
        em_front fe(f);
        out.push_back(D::em(fe, crit, max_time, lr));
    };
    em({{-1.5}}, 1e-4f, 10, 0.2);                                  // 22: constant: status 1 after one step
    em({{nan}}, 1e-4f, 10, 0.2);                                   // 23
    em({{inf}}, 1e-4f, 10, 0.2);                                   // 24
    em({{1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12}}, 1e-4f, 6, 0.2);  // 25: keeps changing: status 0
    em({{-1.5, -1.25, -1.25}}, 2.0f, 10, 0.2);                     // 26: the criterion is tightened before the first run
    em({{-1.5}}, 1e-4f, 0, 0.2);                                   // 27: no round, one finish
    em({{-1.5}, {1, 2, 3, 4, 5, 6, 7, 8}, {0.5, 0.25, nan}}, 1e-4f, 5, 0.2);  // 28: three runs in step
    em({{-1.5}}, 1e-4f, 5, 0.2);                                   // 29..31: each of them alone
    em({{1, 2, 3, 4, 5, 6, 7, 8}}, 1e-4f, 5, 0.2);
    em({{0.5, 0.25, nan}}, 1e-4f, 5, 0.2);
    em({{-2, -1.9, -1.89, -1.889, -1.8889, -1.8889}}, 0.05f, 10, 1.0);  // 32: tightening in later rounds
    return out;
}

}  // namespace fakes
#endif
