// The re-ranks of one rank change of a session (SessionCore::lift, the collective lift's LiftTrial,
// SessionCore::project): every problem re-ranked so far goes back to r_old unless the change is committed.  Host only
// (no HIP) and templated on the problem type -- anything with `int rerank(int)` -- so that a CPU program can drive it.
#pragma once
#include <string>
#include <vector>

#include "../../include/dcora_hip.h"

namespace dcora {

void set_last_error(const std::string &s);

template <class Problem>
class RankChange {
 public:
  explicit RankChange(int r_old) : r_old_(r_old) {}
  RankChange(const RankChange &) = delete;
  RankChange &operator=(const RankChange &) = delete;
  ~RankChange() { rollback(); }
  // p at r_new, remembered when that succeeded (a re-rank that fails leaves its problem at r_old)
  int add(Problem *p, int r_new) {
    const int rc = p->rerank(r_new);
    if (!rc) done_.push_back(p);
    return rc;
  }
  // every remembered problem back at r_old, the last added first; the error that led here stays the one reported, and a
  // re-rank that fails on the way back does not keep the rest from theirs
  void rollback() {
    if (done_.empty()) return;
    const std::string keep = dcora_last_error();
    for (size_t i = done_.size(); i-- > 0;) (void)done_[i]->rerank(r_old_);
    done_.clear();
    set_last_error(keep);
  }
  void commit() { done_.clear(); }  // the point of no return: the problems stay where they are
  int r_old() const { return r_old_; }

 private:
  int r_old_;
  std::vector<Problem *> done_;
};

}  // namespace dcora
