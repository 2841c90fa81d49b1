// Host drivers shared by the single engine, the shard ranks and the replica batch (C++14, standard headers only: no device
// code, usable from a plain host program): the queue-ahead batch loop, the batch-size planner, the convergence run with
// its pause handling, and the EM loop. Hooks return 0 or an SBMBP_ERR_* code; the first code that is not 0 ends the loop
// and is returned as it is.
#ifndef SBMBP_HOST_LOOPS_H
#define SBMBP_HOST_LOOPS_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "host_graph.h"

namespace sbmbp {

// Batches of sweeps are queued one ahead: while the host waits for the convergence state of one batch, the next is already
// in the stream, so the GPU never idles at a batch boundary. The state of a batch lives in slot 0 or 1, alternating.
//   queue(slot)          queues the next batch (at least one sweep) and the read-back of the state into `slot`, and
//                        advances `done` by the sweeps it queued
//   wait(slot, &stopped) blocks until the state of `slot` has arrived; stopped = the device skips whatever follows
//                        (on entry: false, or true when the call drains the batch queued ahead of a stop)
// Ends when the run has stopped or max_sweeps are queued; a batch queued ahead of a stop is drained (its sweeps were no-ops),
// so the last wait() call is the one whose state describes the end of the run. Nothing is queued when done >= max_sweeps.
template <class Queue, class Wait> int queue_ahead(uint32_t max_sweeps, const uint32_t &done, Queue &&queue, Wait &&wait) {
    if (done >= max_sweeps) return 0;
    int r = queue(0);
    for (int k = 0; r == 0; ++k) {
        const bool more = done < max_sweeps;
        if (more && (r = queue((k + 1) & 1)) != 0) break;
        bool stopped = false;
        if ((r = wait(k & 1, &stopped)) != 0) break;
        if (stopped || !more) return more ? wait((k + 1) & 1, &stopped) : 0;
    }
    return r;
}

// Batch sizes follow the decay of the reported difference: from two readings the host estimates the rate per sweep and how
// many sweeps are still needed, and queues no more than that (minus what is already in the stream), so that only a sweep or
// two are left as no-ops behind the stop. The ranks of a sharded run plan from the same states, hence identically.
struct batch_planner {
    uint32_t batch_max;
    double crit;
    uint32_t next;
    double prev_md;
    int prev_idx;
    batch_planner(uint32_t batch_max_, double crit_) : batch_max(batch_max_), crit(crit_) { reset(); }
    void reset() { next = batch_max; prev_md = -1.0; prev_idx = 0; }
    // a reading: the difference after sweep_idx executed sweeps, with `done` sweeps queued so far
    void step(double maxdiff, int sweep_idx, uint32_t done) {
        if (crit > 0 && prev_md > 0 && maxdiff > 0 && maxdiff < prev_md && sweep_idx > prev_idx) {
            const double rate = std::pow(maxdiff / prev_md, 1.0 / double(sweep_idx - prev_idx));
            const double need = maxdiff > crit ? std::ceil(std::log(crit / maxdiff) / std::log(rate)) : 1.0;
            const double ahead = double(done) - double(sweep_idx);  // queued, not yet seen
            next = uint32_t(std::min<double>(batch_max, std::max(1.0, need - ahead)));
        } else {
            next = batch_max;
        }
        if (maxdiff > 0) { prev_md = maxdiff; prev_idx = sweep_idx; }
    }
};

// A convergence run of up to max_sweeps sweeps in planned batches (single engine and shard rank). State carries maxdiff,
// sweep_idx, stop and pause.
//   queue(slot, first, n, form_psi)  queues sweeps first .. first + n of the run and the read-back of the state into `slot`;
//                                    form_psi = the marginal-gather form is still allowed
//   wait(slot, &state)               blocks until the state of `slot` has arrived and copies it out
//   resume()                         clears the device's stop and pause flags
// A state with stop and pause set means the device asked for damped sweeps in the middle of a marginal-gather run: what was
// queued behind that sweep did not run, so the run goes back to sweep_idx, resumes, plans afresh and queues the rest in the
// message-gather form. *cs = the state at the end of the run (untouched when max_sweeps is 0), *psi_count = the sweeps that
// ran in the marginal-gather form (first_explicit: sweep 0 of the run does not, whatever form_psi says).
template <class State, class Queue, class Wait, class Resume>
int converge_run(uint32_t max_sweeps, batch_planner &plan, bool psi_ok, bool first_explicit, Queue &&queue, Wait &&wait, Resume &&resume,
                 State *cs, uint32_t *psi_count) {
    uint32_t done = 0;
    bool form_psi = psi_ok;
    *psi_count = 0;
    while (done < max_sweeps) {
        const uint32_t start = done;
        int r = queue_ahead(
            max_sweeps, done,
            [&](int slot) {
                const uint32_t n = std::min(plan.next, max_sweeps - done);
                const int q = queue(slot, done, n, form_psi);
                done += n;
                return q;
            },
            [&](int slot, bool *stopped) {
                const int w = wait(slot, cs);
                if (w != 0) return w;
                if (!*stopped) plan.step(cs->maxdiff, cs->sweep_idx, done);  // (a drained batch is no reading: its sweeps did not run)
                *stopped = cs->stop != 0;
                return 0;
            });
        if (r != 0) return r;
        if (form_psi) *psi_count += uint32_t(cs->sweep_idx) - start - ((first_explicit && start == 0 && cs->sweep_idx > 0) ? 1 : 0);
        if (!(cs->stop && cs->pause)) break;
        done = uint32_t(cs->sweep_idx);
        form_psi = false;
        if ((r = resume()) != 0) return r;
        plan.reset();
    }
    return 0;
}

// a value lowered to at most `cap` for the lifetime of the object (the relaxed field of the EM loop's BP runs)
struct lowered {
    double &ref;
    const double keep;
    lowered(double &ref_, double cap) : ref(ref_), keep(ref_) { ref = std::min(ref, cap); }
    ~lowered() { ref = keep; }
};

// belief_propagation::learning (bp.cpp:27-47) for R runs in step (R = 1: the single engine, a shard rank). Per round and run:
// tighten the criterion, converge, take the expectations and the free energy, compare, set the status (1 = "fdiff <
// learning_conv_crit", 2 = free energy NaN / Inf), else learning_step and apply. A run that ends keeps the state and the
// parameters of its last round and is left out of every later hook call. The criterion is a float as in the reference and
// is compared and handed on as a double. field_mix is lowered to learn_field_mix until every run is finished.
// Front end F:
//   int converge(const double *crit, const uint8_t *active, uint32_t *executed)   active runs to their criteria
//   int expect(const uint8_t *active, double *na_e, double *nna_e, double *cab_e, double *f)   [R][Q] twice, [R][Q Q], [R]: active rows
//   void params(uint32_t r, std::vector<uint32_t> &na, std::vector<double> &cab)  run r's current parameters
//   int apply(uint32_t r, const uint32_t *na, const double *cab)
//   int finish(uint32_t r)                                                        once per run, after the last round
// Result carries em_steps, status, free_energy and total_sweeps (the sum of the executed sweeps).
template <class F, class Result>
int em_loop(F &fe, uint32_t R, uint32_t Q, uint32_t N, float learning_conv_crit, uint32_t learning_max_time, double learning_rate,
            double learn_snap, double &field_mix, double learn_field_mix, Result *out) {
    const lowered relaxed(field_mix, learn_field_mix);
    std::vector<float> crit(R, learning_conv_crit);
    std::vector<double> critd(R), fold(R, 0.0), fdiff(R, 1.0), fnew(R), na_e(size_t(R) * Q), nna_e(size_t(R) * Q), cab_e(size_t(R) * Q * Q), cab;
    std::vector<uint8_t> active(R, 1);
    std::vector<uint32_t> executed(R), na;
    for (uint32_t r = 0; r < R; ++r) { out[r].em_steps = 0; out[r].status = 0; out[r].total_sweeps = 0; }
    uint32_t n_active = R;
    int rc;
    for (uint32_t t = 0; t < learning_max_time && n_active; ++t) {
        for (uint32_t r = 0; r < R; ++r) {
            if (active[r] && fdiff[r] < crit[r]) crit[r] = float(double(crit[r]) * 0.1);
            critd[r] = double(crit[r]);
        }
        if ((rc = fe.converge(critd.data(), active.data(), executed.data())) != 0) return rc;
        if ((rc = fe.expect(active.data(), na_e.data(), nna_e.data(), cab_e.data(), fnew.data())) != 0) return rc;
        for (uint32_t r = 0; r < R; ++r) {
            if (!active[r]) continue;
            out[r].total_sweeps += executed[r];
            fdiff[r] = std::fabs(fnew[r] - fold[r]);
            fold[r] = fnew[r];
            if (std::isnan(fold[r]) || std::isinf(fold[r])) out[r].status = 2;
            else if (fdiff[r] < crit[r]) out[r].status = 1;
            if (out[r].status) { active[r] = 0; --n_active; continue; }
            fe.params(r, na, cab);
            learning_step_host(Q, N, learning_rate, learn_snap, double(crit[r]), na_e.data() + size_t(r) * Q, cab_e.data() + size_t(r) * Q * Q,
                               na.data(), cab.data());
            if ((rc = fe.apply(r, na.data(), cab.data())) != 0) return rc;
            out[r].em_steps++;
        }
    }
    for (uint32_t r = 0; r < R; ++r) {
        out[r].free_energy = fold[r];
        if ((rc = fe.finish(r)) != 0) return rc;
    }
    return 0;
}

}  // namespace sbmbp
#endif
