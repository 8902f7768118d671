// common.h — shared host-side helpers for libparaformer_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <mutex>
#include <stdexcept>
#include <string>

#include "../../include/paraformer_hip.h"

namespace pf {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

void set_last_error(const std::string& msg);

#define PF_HIP(expr)                                                                      \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess)                                                                 \
      throw ::pf::Error(PF_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

#define PF_CHECK(cond, code, msg)                     \
  do {                                                \
    if (!(cond)) throw ::pf::Error((code), (msg));    \
  } while (0)

using half_t = _Float16;

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// PF_CU_CAP=n: limits PERSISTENT grid sizes (and their tile-shape rules) to n compute units.  It does not partition the
// device: the hardware still places those workgroups where it likes, and the non-persistent kernels (attention, the
// row-complete and short-input GEMMs) ignore it (tools/: the two-engine overlap experiment of round 4)
// An integer knob read from the environment.  Call sites keep the result in a function-local `static const`, whose
// initialisation C++11 makes thread-safe: launchers run concurrently from the recognizer pool's caller threads.
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return (e && e[0]) ? atoi(e) : dflt; }
inline int cu_limit(int cus) {
  static const int cap = [] { const char* e = getenv("PF_CU_CAP"); return e ? atoi(e) : 0; }();   // thread-safe initialiser
  return cap > 0 && cap < cus ? cap : cus;
}

// ---- per-device start-up of a launcher.  Engines on different devices launch from different host threads (one engine
// per GPU, include/paraformer_hip.h pf_group_*), so what a launcher does once per device is done under a lock.
// compute units of the current device, looked up once per device (k_gemm.hip): all of them, and as PF_CU_CAP limits them
int device_cu_count();
int device_cus();
// `static DeviceOnce once; once.run([] { set_max_lds(kernel, bytes); ... });` runs the callable on the first launch
// from that launcher on the current device (kernel attributes are per device, and are set lazily, not at library load)
struct DeviceOnce {
  template <class F>
  void run(F&& f) {
    int dev = 0;
    PF_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (!done[dev & 63]) { f(); done[dev & 63] = true; }
  }
 private:
  std::mutex mu;
  bool done[64] = {false};
};
// a kernel that asks for more than 64 KiB of dynamic LDS must be allowed to
inline void set_max_lds(const void* kernel, int bytes) {
  PF_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
}

// ---- the state block of the streaming endpoint detector (paraformer_hip.h "Voice-activity endpointing, streaming"): the word
// indices both forms use (hostutil.cpp host_endpoint_update, k_endpoint.hip)
enum EndpointWord { kEpHist = 0, kEpState = 8, kEpLastOne = 9, kEpRunFirst = 10, kEpPrevEnd = 11, kEpCount = 12, kEpFloorLo = 13,
                    kEpFloorHi = 14, kEpFlushed = 15 };
static_assert(kEpFlushed + 1 == PF_ENDPOINT_STATE_INTS, "the endpoint state block");

}  // namespace pf
