// Unit test of dcora_amd/csrc/host_threads.h -- run_threads, parallel_for and the C ABI's guard abi_call -- built with
// g++ under ASan + UBSan by tests/test_abi_guard_cpu.py.  Prints "ok" when every check passes.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "host_threads.h"

namespace dcora {
static std::string g_err;
void set_last_error(const std::string &s) { g_err = s; }
}  // namespace dcora

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

int main() {
  using namespace dcora;
  // one body runs on the calling thread
  {
    std::thread::id id;
    run_threads(1, [&](int) { id = std::this_thread::get_id(); });
    CHECK(id == std::this_thread::get_id());
  }
  // body(0) on the caller, the others on threads of their own
  {
    std::vector<std::thread::id> ids(4);
    run_threads(4, [&](int t) { ids[(size_t)t] = std::this_thread::get_id(); });
    CHECK(ids[0] == std::this_thread::get_id());
    for (int t = 1; t < 4; ++t) CHECK(ids[(size_t)t] != ids[0]);
  }
  // a throwing body reaches the caller only after every other body has finished; the lowest t that threw wins
  {
    const int n = 6;
    std::atomic<int> finished(0);
    std::string what;
    try {
      run_threads(n, [&](int t) {
        if (t == 0 || t == 4) throw std::runtime_error("body " + std::to_string(t));
        std::this_thread::sleep_for(std::chrono::milliseconds(40 * t));
        ++finished;
      });
    } catch (const std::runtime_error &e) {
      what = e.what();
    }
    CHECK(what == "body 0");
    CHECK(finished.load() == n - 2);
  }
  // parallel_for visits each index exactly once
  {
    const int n = 10007;
    std::vector<std::atomic<int>> seen(n);
    for (auto &s : seen) s.store(0);
    parallel_for(n, 8, 7, [&](int i) { seen[(size_t)i].fetch_add(1); });
    for (int i = 0; i < n; ++i) CHECK(seen[(size_t)i].load() == 1);
    int calls = 0;
    parallel_for(0, 8, 4, [&](int) { ++calls; });
    CHECK(calls == 0);
  }
  // the guard: exceptions become DCORA_ERR_HIP with the last error set
  {
    g_err.clear();
    CHECK(abi_call({}, []() -> int { throw std::bad_alloc(); }) == DCORA_ERR_HIP);
    CHECK(g_err == "host allocation failed");
    CHECK(abi_call({}, []() -> int { throw std::runtime_error("boom"); }) == DCORA_ERR_HIP);
    CHECK(g_err == "exception: boom");
    CHECK(abi_call({}, []() -> int { throw 42; }) == DCORA_ERR_HIP);
    CHECK(g_err == "exception of unknown type");
  }
  // a NULL required pointer is refused without running the body; the body's status passes through
  {
    int x = 0;
    bool ran = false;
    g_err.clear();
    CHECK(abi_call({&x, nullptr}, [&] {
            ran = true;
            return 0;
          }) == DCORA_ERR_BAD_ARG);
    CHECK(!ran && g_err == "null argument");
    CHECK(abi_call({&x}, [] { return DCORA_ERR_NOT_PD; }) == DCORA_ERR_NOT_PD);
    CHECK(abi_call({&x}, [] { return 0; }) == 0);
  }
  std::printf("ok\n");
  return 0;
}
