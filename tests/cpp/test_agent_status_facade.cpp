// DCORA::Agent's status and team rules through the facade (ref include/DCORA/Agent.h:427-458, src/Agent.cpp:558-586,
// 1123-1156, 1280-1330): after iterate(true) getStatus() carries what the session stored -- the relative change of the
// update, the local termination flag, the iteration number --, shouldTerminate() is false while a teammate's status
// has not been handed over and true once every robot's has and all are ready.
// usage: test_agent_status_facade <file.g2o>.  Exit code 0 = pass, 2 = no GPU (the library has no CPU fallback), 1 = failure.
#include <cmath>
#include <cstdio>
#include <vector>

#include "DCORA/Agent.h"
#include "DCORA/DCORA_utils.h"

namespace {
int failures = 0;
#define EXPECT(cond)                                          \
  do {                                                        \
    if (!(cond)) {                                            \
      std::printf("line %d: %s is false\n", __LINE__, #cond); \
      ++failures;                                             \
    }                                                         \
  } while (0)

// LiftedArray::maxTranslationDistance (ref src/manifold/Elements.cpp:59-69) on the host
double max_translation_distance(const DCORA::Matrix &A, const DCORA::Matrix &B, unsigned r, unsigned d) {
  double m = 0;
  for (size_t i = 0; i < A.cols() / (d + 1); ++i) {
    double s = 0;
    for (unsigned k = 0; k < r; ++k) {
      const double e = A(k, i * (d + 1) + d) - B(k, i * (d + 1) + d);
      s += e * e;
    }
    m = std::fmax(m, std::sqrt(s));
  }
  return m;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: %s file.g2o\n", argv[0]);
    return 1;
  }
  if (dcora_device_count() < 1) {
    std::printf("no GPU: facade compiled and linked, compute skipped\n");
    return 2;
  }
  dcora_dataset_t ds;
  DCORA::check_status(dcora_dataset_load_g2o(argv[1], &ds), "load");
  int di = 0, ni = 0, mi = 0;
  DCORA::check_status(dcora_dataset_info(ds, &di, &ni, &mi), "info");
  const unsigned d = (unsigned)di, n = (unsigned)ni, num_robots = 5, r = 5, dh = d + 1, k = dh * n, per = n / num_robots;
  std::vector<double> T((size_t)d * k);
  DCORA::check_status(dcora_dataset_chordal_init(ds, T.data()), "chordal");
  DCORA::Matrix X0(r, k);
  for (unsigned c = 0; c < k; ++c)
    for (unsigned i = 0; i < d; ++i) X0(i, c) = T[(size_t)c * d + i];

  DCORA::AgentParameters options(d, r, num_robots);
  options.acceleration = true;
  options.relChangeTol = 1e9;  // every optimised agent is ready: the team rule alone decides
  auto team = DCORA::AgentTeam::create(ds, options);
  auto &agents = team->agents;
  for (unsigned robot = 0; robot < num_robots; ++robot) {
    const unsigned lo = robot * per, hi = (robot == num_robots - 1) ? n : (robot + 1) * per;
    DCORA::Matrix Xb(r, (hi - lo) * dh);
    for (unsigned c = 0; c < (hi - lo) * dh; ++c)
      for (unsigned i = 0; i < r; ++i) Xb(i, c) = X0(i, lo * dh + c);
    agents[robot]->setX(Xb);
  }
  {  // nobody has optimised yet
    const DCORA::AgentStatus st = agents[0]->getStatus();
    EXPECT(st.agentID == 0 && st.state == DCORA::AgentState::INITIALIZED && st.iterationNumber == 0);
    EXPECT(!st.readyToTerminate && st.relativeChange == 0);
    EXPECT(!agents[0]->shouldTerminate());
    EXPECT(!agents[0]->shouldUpdateMeasurementWeights());
  }
  // one round per robot, round-robin; the agents read the session's mirror (nothing is handed over)
  for (unsigned round = 0; round < num_robots; ++round) {
    const unsigned selected = round;
    DCORA::Matrix before, after;
    agents[selected]->getX(&before);
    for (auto &a : agents)
      if (a->getID() != selected) a->iterate(false);
    EXPECT(agents[selected]->iterate(true));
    agents[selected]->getX(&after);
    const DCORA::AgentStatus st = agents[selected]->getStatus();
    dcora_agent_status cs;
    int known = 0;
    DCORA::check_status(dcora_rbcd_agent_status(team->session(), (int)selected, &cs, &known), "status");
    const double want = max_translation_distance(after, before, r, d);
    EXPECT(known == 1);
    EXPECT(st.agentID == selected && st.iterationNumber == round + 1 && st.instanceNumber == 0);
    EXPECT((int)st.iterationNumber == cs.iteration_number);
    EXPECT(st.relativeChange == cs.relative_change);
    EXPECT(st.readyToTerminate == (cs.ready_to_terminate != 0) && st.readyToTerminate);
    EXPECT(want > 0 && std::fabs(st.relativeChange - want) <= 1e-14 * want);
    // a robot that has not optimised yet: the fields the rule reads stay at their defaults
    if (round + 1 < num_robots) {
      const DCORA::AgentStatus idle = agents[round + 1]->getStatus();
      EXPECT(!idle.readyToTerminate && idle.relativeChange == 0 && idle.iterationNumber == round + 1);
    }
    std::printf("round %u: agent %u relative change %.6e (host %.6e)\n", round + 1, selected, st.relativeChange, want);
  }
  // the team rule at agent 0: its teammates' statuses arrive one by one
  DCORA::Agent &a0 = *agents[0];
  EXPECT(!a0.shouldTerminate());
  for (unsigned q = 1; q < num_robots; ++q) {
    EXPECT(!a0.hasNeighborStatus(q));
    a0.setNeighborStatus(agents[q]->getStatus());
    EXPECT(a0.hasNeighborStatus(q) && a0.getNeighborStatus(q).agentID == q);
    EXPECT(a0.shouldTerminate() == (q == num_robots - 1));
  }
  EXPECT(!a0.shouldUpdateMeasurementWeights());  // L2: never (ref src/Agent.cpp:1282-1283)
  // one teammate that is not ready keeps the team going
  DCORA::AgentStatus busy = agents[2]->getStatus();
  busy.readyToTerminate = false;
  a0.setNeighborStatus(busy);
  EXPECT(!a0.shouldTerminate());
  a0.setNeighborStatus(agents[2]->getStatus());
  EXPECT(a0.shouldTerminate());
  // an agent that was handed nothing decides on its own status alone: not enough
  EXPECT(!agents[1]->shouldTerminate());
  dcora_dataset_destroy(ds);
  std::printf("agent status facade: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
