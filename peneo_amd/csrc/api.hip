// Error plumbing + version of libpeneo_hip.so.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>

#include "common.h"

namespace peneo {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return PENEO_ERR_LAUNCH;
  }
  return PENEO_OK;
}

static int g_det_mode = -1;   // -1: not read yet (PENEO_DETERMINISTIC)
static std::atomic<uint64_t> g_order_dependent{0};

int det_mode() {
  if (g_det_mode < 0) {
    const char* e = getenv("PENEO_DETERMINISTIC");
    const int m = e ? atoi(e) : 0;
    g_det_mode = m < 0 ? 0 : (m > 2 ? 2 : m);
  }
  return g_det_mode;
}

int order_dependent(const char* entry_point) {
  g_order_dependent.fetch_add(1, std::memory_order_relaxed);
  if (det_mode() == 2) {
    set_error("%s: this call takes an order-dependent accumulation path (float atomics), refused under deterministic mode 2", entry_point);
    return PENEO_ERR_INVALID;
  }
  return PENEO_OK;
}

}  // namespace peneo

extern "C" void peneo_set_deterministic(int mode) { peneo::g_det_mode = mode < 0 ? 0 : (mode > 2 ? 2 : mode); }
extern "C" int peneo_deterministic(void) { return peneo::det_mode(); }
extern "C" uint64_t peneo_order_dependent_launches(void) { return peneo::g_order_dependent.load(std::memory_order_relaxed); }

extern "C" int peneo_version(void) { return 113; }
extern "C" const char* peneo_last_error(void) { return peneo::g_err; }
