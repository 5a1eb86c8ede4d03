// Unit test of dcora_amd/csrc/rank_change.h -- the re-ranks of one rank change of a session and their roll-back -- with
// stand-in problems that count their rerank calls and fail at a chosen call; built with g++ under ASan + UBSan by
// tests/test_session_blocks_cpu.py.  Prints "ok <n>" per passed group and nothing that says FAILED.
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "rank_change.h"

namespace dcora {
static std::string g_err;
void set_last_error(const std::string &s) { g_err = s; }
}  // namespace dcora
extern "C" const char *dcora_last_error(void) { return dcora::g_err.c_str(); }

namespace {

int g_call = 0, g_fail_at = -1;

// every call overwrites the last error, as a real failure on the way back would: the roll-back has to restore it
struct Fake {
  int id = 0, r = 0, calls = 0;
  int rerank(int r_new) {
    ++calls;
    if (++g_call == g_fail_at) {
      dcora::set_last_error("rerank of problem " + std::to_string(id) + " failed");
      return 7;
    }
    dcora::set_last_error("noise of problem " + std::to_string(id));
    r = r_new;
    return 0;
  }
};

std::vector<Fake> fresh(int r) {  // the central problem and three agents
  std::vector<Fake> p(4);
  for (int i = 0; i < 4; ++i) p[(size_t)i].id = i, p[(size_t)i].r = r;
  g_call = 0;
  g_fail_at = -1;
  dcora::g_err.clear();
  return p;
}

#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);          \
      return 1;                                                           \
    }                                                                     \
  } while (0)

}  // namespace

int main() {
  using dcora::RankChange;
  const int r_old = 3, r_new = 4;
  // 1. the failure at every position: what was re-ranked is back, the rest untouched, the failing call's text survives
  for (int pos = 0; pos < 4; ++pos) {
    std::vector<Fake> p = fresh(r_old);
    g_fail_at = pos + 1;
    int rc = 0;
    {
      RankChange<Fake> change(r_old);
      for (int i = 0; i < 4 && !rc; ++i) rc = change.add(&p[(size_t)i], r_new);
      CHECK(rc == 7);
    }  // (leaving the scope uncommitted)
    for (int i = 0; i < 4; ++i) {
      CHECK(p[(size_t)i].r == r_old);
      CHECK(p[(size_t)i].calls == (i < pos ? 2 : (i == pos ? 1 : 0)));
    }
    CHECK(dcora::g_err == "rerank of problem " + std::to_string(pos) + " failed");
    std::printf("ok 1.%d\n", pos);
  }
  // 2. commit, then destruction: nothing is re-ranked again
  {
    std::vector<Fake> p = fresh(r_old);
    {
      RankChange<Fake> change(r_old);
      for (Fake &q : p) CHECK(change.add(&q, r_new) == 0);
      change.commit();
      change.rollback();  // (nothing to take back either)
    }
    for (const Fake &q : p) CHECK(q.r == r_new && q.calls == 1);
    std::printf("ok 2\n");
  }
  // 3. destruction without commit rolls back and keeps the error that stood when it began
  {
    std::vector<Fake> p = fresh(r_old);
    {
      RankChange<Fake> change(r_old);
      for (Fake &q : p) CHECK(change.add(&q, r_new) == 0);
      dcora::set_last_error("what led here");
    }
    for (const Fake &q : p) CHECK(q.r == r_old && q.calls == 2);
    CHECK(dcora::g_err == "what led here");
    std::printf("ok 3\n");
  }
  // 4. an explicit roll-back is not repeated by the destructor; an owner that goes away rolls back (the lift's trial)
  {
    std::vector<Fake> p = fresh(r_old);
    {
      RankChange<Fake> change(r_old);
      for (Fake &q : p) CHECK(change.add(&q, r_new) == 0);
      change.rollback();
      for (const Fake &q : p) CHECK(q.r == r_old && q.calls == 2);
    }
    for (const Fake &q : p) CHECK(q.calls == 2);
    struct Owner {
      explicit Owner(int r) : change(r) {}
      std::vector<double> buffers{1.0, 2.0};
      RankChange<Fake> change;
    };
    p = fresh(r_old);
    std::unique_ptr<Owner> t(new Owner(r_old));
    for (Fake &q : p) CHECK(t->change.add(&q, r_new) == 0);
    t.reset();
    for (const Fake &q : p) CHECK(q.r == r_old && q.calls == 2);
    std::printf("ok 4\n");
  }
  // 5. a roll-back whose own rerank fails still visits the rest
  for (int bad = 5; bad <= 8; ++bad) {  // (calls 5 .. 8 are the four of the roll-back)
    std::vector<Fake> p = fresh(r_old);
    {
      RankChange<Fake> change(r_old);
      for (Fake &q : p) CHECK(change.add(&q, r_new) == 0);
      dcora::set_last_error("what led here");
      g_fail_at = bad;
    }
    int back = 0;
    for (const Fake &q : p) {
      CHECK(q.calls == 2);
      back += q.r == r_old;
    }
    CHECK(back == 3);
    CHECK(dcora::g_err == "what led here");
    std::printf("ok 5.%d\n", bad);
  }
  return 0;
}
