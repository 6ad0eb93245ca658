// glrm_devmem.hpp -- who owns device memory and which device is current (included by glrm_engine.hpp, after fail()).
//   DeviceScope  every extern "C" entry point that touches the device opens one: the handle's device inside, the caller's again on return
//   DevArena     owner of device allocations: glrm_handle::mem for everything the handle keeps, Shard::mem (glrm_multigpu.hip) for a
//                shard's replica of a sharded fit, a local one for a function's scratch.
//                A pointer belongs to exactly one arena from alloc to free; the T* a kernel argument struct is filled from stays raw.
#pragma once

#include <algorithm>
#include <vector>

// the only hipMalloc / hipFree of the engine (glrm_testhooks.hip: the test build also counts the live allocations)
hipError_t glrm_device_alloc(void** p, size_t bytes);
void glrm_device_free(void* p);

struct DeviceScope {
  int prev = -1;
  bool ok = true;
  explicit DeviceScope(int dev = -1) { // -1: only remember (the multi-device entry points select their shards' devices themselves)
    if (hipGetDevice(&prev) != hipSuccess) ok = false;
    if (ok && dev >= 0 && prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
  }
  ~DeviceScope() {
    int cur;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

class DevArena {
  std::vector<void*> owned;

 public:
  DevArena() = default;
  DevArena(DevArena&& o) noexcept : owned(std::move(o.owned)) { o.owned.clear(); }
  DevArena& operator=(DevArena&&) = delete;
  ~DevArena() { free_all(); }

  // count elements (at least one); what: the out-of-memory message of a site that has one of its own
  template <class T>
  int alloc(T** p, size_t count, const char* what = nullptr) {
    *p = nullptr;
    const hipError_t e = glrm_device_alloc((void**)p, std::max<size_t>(1, count) * sizeof(T));
    if (e == hipErrorOutOfMemory && what) return fail(GLRM_ERR_OOM, "%s", what);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? GLRM_ERR_OOM : GLRM_ERR_HIP, "device allocation of %zu x %zu bytes failed: %s", count, sizeof(T), hipGetErrorString(e));
    owned.push_back(*p);
    return GLRM_OK;
  }
  // frees one allocation now (nullptr, or a pointer of somebody else's such as a borrowed array: only nulled)
  template <class T>
  void release(T** p) {
    if (detach(*p)) glrm_device_free(*p);
    *p = nullptr;
  }
  // ownership of one pointer moves from arena to arena: detach + adopt = move_to
  bool detach(const void* p) {
    const auto it = std::find(owned.begin(), owned.end(), p);
    if (p == nullptr || it == owned.end()) return false;
    owned.erase(it);
    return true;
  }
  void adopt(void* p) { if (p) owned.push_back(p); }
  void move_to(DevArena& to, void* p) { if (detach(p)) to.adopt(p); }
  void free_all() {
    for (void* p : owned) glrm_device_free(p);
    owned.clear();
  }
};
