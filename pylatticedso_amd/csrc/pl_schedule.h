// The host's look schedule of the PCG loops: how many iterations are queued before the next download of the residual
// history.  Plain C++ (no HIP, nothing of the project), so that a host program can drive it: tests/test_look_schedule.py.
//
// With the default (check_every <= 0) the chunk adapts: 32 while far from the target, then what the observed decay rate
// predicts is still needed - a fixed chunk overshoots by 16 iterations on average, 8 % of a 200-iteration solve.  The device
// runs every chunk to its end, so in the ordinary form the schedule decides which iterate a solve returns.  (Every rank of a
// multi-GPU run sees the same all-reduced history, hence takes the same decisions.)
#pragma once
#include <algorithm>
#include <cmath>

namespace pl {

struct LookParams {
  int check_every = 0;        // <= 0: adaptive, chunks of at most 32; > 0: fixed chunks of that many iterations
  int max_iter = 0;
  double target = 0.0;        // ||r||^2 at which the loop ends
  double rr0 = 0.0;           // ||r||^2 before iteration k0
  int k0 = 0;                 // iterations done before this schedule begins (restarts of the fp32 modes)
  int extra = 0;              // added to the predicted chunk (single-reduction form: its history lags one update behind)
  // A handle preconditioned by a dense FACTOR of its own matrix (precond = 5; the assembled Schur matrix of a DDM handle,
  // precond = 2) converges in one or two steps: look after two (32 queued iterations of a 9-node cell were 0.5 ms of the
  // 0.57 ms a column of pl_schur took)
  bool dd_ready = false;
  bool ref_cg = false;        // reference-CG mode: no first chunk from the previous solve
  // A design loop solves a slowly changing system over and over: the iteration count of the previous converged solve on
  // this handle (identical on every rank) is where the first look at the history is worth taking - three iterations before
  // it - instead of every 32 iterations on the way there (each look drains the stream: 30-50 us).
  int last_iterations = 0;
};

class LookSchedule {
 public:
  explicit LookSchedule(const LookParams &q)
      : adaptive_(q.check_every <= 0), direct_(adaptive_ && q.dd_ready), chunk_(adaptive_ ? 32 : q.check_every),
        extra_(q.extra), max_iter_(q.max_iter), target_(q.target), rr_prev_(q.rr0), k_prev_(q.k0) {
    first_ = direct_ ? std::min(2, q.max_iter)
                     : ((adaptive_ && !q.ref_cg && q.last_iterations > 40) ? std::min(q.last_iterations - 3, q.max_iter) : chunk_);
    next_ = first_;
  }
  // the largest chunk todo() can return: the size of the host's history buffer
  int max_chunk() const { return std::max(chunk_, first_); }
  // iterations to queue when k are done
  int todo(int k) const { return std::min(next_, max_iter_ - k); }
  // a chunk has ended at k iterations with ||r||^2 = rr_end, above the target
  void missed(int k, double rr_end) {
    if (!adaptive_) return;
    next_ = direct_ && k < 16 ? 2 : chunk_;
    if (rr_end < rr_prev_ && rr_end > target_) {
      const double per_it = std::log(rr_end / rr_prev_) / (double)(k - k_prev_);      // < 0
      const double need = std::log(target_ / rr_end) / per_it;
      if (need < 2.0 * chunk_) next_ = std::max(2, std::min(chunk_, (int)std::ceil(0.75 * need) + extra_));
    }
    rr_prev_ = rr_end;
    k_prev_ = k;
  }

 private:
  bool adaptive_, direct_;
  int chunk_, extra_, max_iter_, first_ = 0, next_ = 0;
  double target_, rr_prev_;
  int k_prev_;
};

}  // namespace pl
