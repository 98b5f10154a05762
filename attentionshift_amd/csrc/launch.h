// Host-side launch helpers: the per-device state a launcher needs exists once, here.  A launcher keeps no
// per-process device state of its own -- no `static` flag, CU count or stream that the first device to come by would fill.
#pragma once
#include <atomic>
#include "common.h"

constexpr int kAsMaxDev = 16;

// the current device's index into the tables below; -1 when there is none or it lies outside them
inline int as_device_slot() {
  int d = -1;
  return hipGetDevice(&d) == hipSuccess && d >= 0 && d < kAsMaxDev ? d : -1;
}

// ---------------------------------------------------------------------------------------------
// Dynamic-LDS opt-in of kernel `Kern` on the current device: the driver call is made when `bytes` exceeds what this device
// has granted this kernel so far (every time for a device outside the table).  The kernel is a template argument, so each
// kernel owns its table and two kernels cannot share a flag.  The call's result is ignored: the launch reports the error.
// No lock: a race between two host threads only repeats an idempotent call.
// ---------------------------------------------------------------------------------------------
template <auto Kern> void as_lds_optin(size_t bytes) {
  static std::atomic<unsigned> granted[kAsMaxDev];
  const int d = as_device_slot();
  if (d >= 0 && bytes <= granted[d].load(std::memory_order_relaxed)) return;
  (void)hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (d < 0) return;
  unsigned seen = granted[d].load(std::memory_order_relaxed);
  while (seen < bytes && !granted[d].compare_exchange_weak(seen, (unsigned)bytes, std::memory_order_relaxed)) {}
}

// multiprocessor count of the current device (256 when it cannot be read); the callers round it their own way
inline int as_cu_count() {
  static std::atomic<int> cus[kAsMaxDev];
  const int d = as_device_slot();
  int n = d >= 0 ? cus[d].load(std::memory_order_relaxed) : 256;
  if (n > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n <= 0) n = 256;
  cus[d].store(n, std::memory_order_relaxed);
  return n;
}

// ---------------------------------------------------------------------------------------------
// Fork / join onto helper streams inside one C call: independent launch chains run side by side (a chain of
// one-workgroup-per-CU launches leaves most of every CU free; two half-empty last rounds fill each other's slots).  The
// caller's stream forks with an event, the helper chains run on the side streams, and the caller's stream waits for each
// chain's last launch before the call returns -- so the caller sees ordinary stream order.
// One set of NS streams + events PER DEVICE (a thread alternating between devices reuses each device's set instead of
// re-creating -- and leaking -- one on every switch); a set whose creation fails half-way is destroyed and stays off.
// Instances are `static thread_local` in the launcher that uses them.
// ---------------------------------------------------------------------------------------------
template <int NS> struct AsSide {
  struct Set {
    hipStream_t st[NS] = {};
    hipEvent_t join[NS] = {};
    hipEvent_t fork = nullptr;
    int state = 0;                                      // 0 = not tried, 1 = ready, -1 = failed (do not retry)
  };
  Set sets[kAsMaxDev];
  Set* cur = nullptr;                                   // the CURRENT device's set (null: none)
  static void drop(Set& se) {
    if (se.fork) (void)hipEventDestroy(se.fork);
    for (int i = NS - 1; i >= 0; --i) {
      if (se.join[i]) (void)hipEventDestroy(se.join[i]);
      if (se.st[i]) (void)hipStreamDestroy(se.st[i]);
    }
    se = Set();
  }
  bool init() {
    cur = nullptr;
    const int d = as_device_slot();
    if (d < 0) return false;
    Set& se = sets[d];
    if (se.state == 0) {
      bool made = hipEventCreateWithFlags(&se.fork, hipEventDisableTiming) == hipSuccess;
      for (int i = 0; i < NS && made; ++i)
        made = hipStreamCreateWithFlags(&se.st[i], hipStreamNonBlocking) == hipSuccess &&
               hipEventCreateWithFlags(&se.join[i], hipEventDisableTiming) == hipSuccess;
      if (!made) {
        drop(se);
        (void)hipGetLastError();                        // the caller falls back to its own stream: not its error
      }
      se.state = made ? 1 : -1;
    }
    if (se.state == 1) cur = &se;
    return cur != nullptr;
  }
  // thread exit: give the streams and events back.  Errors are ignored -- at process exit the HIP runtime may already be gone.
  ~AsSide() {
    for (Set& se : sets)
      if (se.state == 1) drop(se);
    (void)hipGetLastError();
  }
};
// the first n side streams wait behind an event of `s`; false (no set, a lost device): the caller keeps everything on `s`
template <int NS> bool as_side_fork(AsSide<NS>& sd, hipStream_t s, int n = NS) {
  if (!sd.init() || hipEventRecord(sd.cur->fork, s) != hipSuccess) return false;
  for (int i = 0; i < n; ++i)
    if (hipStreamWaitEvent(sd.cur->st[i], sd.cur->fork, 0) != hipSuccess) return false;
  return true;
}
// `s` waits for everything queued on side stream i so far
template <int NS> void as_side_join(AsSide<NS>& sd, int i, hipStream_t s) {
  if (hipEventRecord(sd.cur->join[i], sd.cur->st[i]) != hipSuccess || hipStreamWaitEvent(s, sd.cur->join[i], 0) != hipSuccess)
    (void)hipStreamSynchronize(sd.cur->st[i]);          // (a lost device; keeps the order safe)
}
