// The library's host threads and the guard of its C ABI: the only places that start a std::thread or catch at the
// boundary.  Host only (no HIP), so that the sanitizer tests compile it with g++.
#pragma once
#include <algorithm>
#include <atomic>
#include <exception>
#include <initializer_list>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dcora_hip.h"

namespace dcora {

void set_last_error(const std::string &s);

// body(0) on the calling thread and body(1 .. n - 1) on threads of their own.  Returns once every body has finished,
// then rethrows the exception of the lowest t that threw.  A thread that cannot be started runs its body on the calling
// thread after body(0), so what is computed never depends on it.
template <class F>
void run_threads(int n, F &&body) {
  std::vector<std::exception_ptr> err((size_t)std::max(n, 1));
  auto run = [&](int t) {
    try {
      body(t);
    } catch (...) {
      err[(size_t)t] = std::current_exception();
    }
  };
  std::vector<std::thread> th;
  std::vector<int> refused;
  th.reserve((size_t)std::max(n - 1, 0));
  refused.reserve(th.capacity());
  for (int t = 1; t < n; ++t) {
    try {
      th.emplace_back(run, t);
    } catch (...) {  // std::system_error, or no memory for the thread's state
      refused.push_back(t);
    }
  }
  if (n >= 1) run(0);
  for (int t : refused) run(t);
  for (std::thread &x : th) x.join();
  for (std::exception_ptr &e : err)
    if (e) std::rethrow_exception(e);
}

// body(i) for i in [0, n) on up to nthreads threads, dynamic chunks
template <class F>
void parallel_for(int n, int nthreads, int chunk, F body) {
  std::atomic<int> next(0);
  run_threads(std::max(1, std::min(nthreads, (n + chunk - 1) / chunk)), [&](int) {
    for (;;) {
      const int i0 = next.fetch_add(chunk);
      if (i0 >= n) break;
      const int i1 = std::min(n, i0 + chunk);
      for (int i = i0; i < i1; ++i) body(i);
    }
  });
}

namespace abi_detail {
inline int fail(int status, const char *msg) noexcept {
  try {
    set_last_error(msg);
  } catch (...) {
  }
  return status;
}
}  // namespace abi_detail

// Every exported entry point with a failure path runs through this: DCORA_ERR_BAD_ARG ("null argument") when one of
// `required` is NULL, the body not run; otherwise the body's status, an exception turned into DCORA_ERR_HIP with the
// last error set.
template <class F>
int abi_call(std::initializer_list<const void *> required, F &&body) noexcept {
  for (const void *p : required)
    if (!p) return abi_detail::fail(DCORA_ERR_BAD_ARG, "null argument");
  try {
    return body();
  } catch (const std::bad_alloc &) {
    return abi_detail::fail(DCORA_ERR_HIP, "host allocation failed");
  } catch (const std::exception &e) {
    try {
      set_last_error(std::string("exception: ") + e.what());
    } catch (...) {
    }
    return DCORA_ERR_HIP;
  } catch (...) {
    return abi_detail::fail(DCORA_ERR_HIP, "exception of unknown type");
  }
}

}  // namespace dcora
