// scratch.cc -- the stream-ordered scratch blocks of the batch calls.
//
// Every batch call takes a small scratch block (unit counters, a processing
// order, nonces and ADs of a record layer's batch) that lives from the call's
// first kernel to its last, in stream order.  Rounds 1-6 took them from HIP's
// stream-ordered pool (hipMallocAsync / hipFreeAsync).  On ROCm 7 a
// hipFreeAsync of a block that the pool had recycled on the same stream while
// its earlier free was still pending WAITS ON THE HOST for that earlier free:
// the second of two batches enqueued back to back on a busy stream blocked
// until the stream had drained (tests/test_stream_order_gpu.py, DESIGN.md §2:
// 156-162 ms behind a 160 ms gate, in the free alone), which breaks the
// headers' "only enqueues work on hip_stream and never synchronises it".
//
// So the blocks come from a small cache of our own with the same ordering
// rule and no host wait: a freed block carries the stream it was freed on and
// an event recorded there; it is handed out again at once to a call on that
// same stream (stream order keeps the earlier use ahead of the new one), to
// any other stream once the event has completed (hipEventQuery, never a wait),
// and otherwise a new block is allocated.  Blocks come in power-of-two sizes,
// so a server's steady state allocates nothing.
#include <hip/hip_runtime.h>

#include <mutex>
#include <unordered_map>
#include <vector>

#include "internal.h"

namespace bssl_amd {
namespace {

struct Block {
  void *ptr;
  size_t cap;
  int device;
  hipStream_t stream;  // the stream of the last free
  hipEvent_t freed;    // recorded there
};

std::mutex g_mu;
std::vector<Block> g_free;
std::unordered_map<void *, Block> g_busy;
size_t g_cached_bytes = 0;
// Above this many cached bytes a free releases the idle blocks whose event
// has completed (hipFree may wait for the device: rare, and never on a block
// that is still in use).
constexpr size_t kCacheLimit = size_t(1) << 30;

size_t size_class(size_t n) {
  size_t cap = 256;
  while (cap < n) cap <<= 1;
  return cap;
}

}  // namespace

hipError_t scratch_alloc(void **out, size_t bytes, hipStream_t stream) {
  *out = nullptr;
  int device = -1;
  hipError_t e = hipGetDevice(&device);
  if (e != hipSuccess) return e;
  const size_t cap = size_class(bytes);
  {
    std::lock_guard<std::mutex> lock(g_mu);
    bool pending = false;
    for (size_t i = 0; i < g_free.size(); i++) {
      Block &b = g_free[i];
      if (b.cap != cap || b.device != device) continue;
      if (b.stream != stream && hipEventQuery(b.freed) != hipSuccess) {
        pending = true;
        continue;
      }
      Block taken = b;
      g_free[i] = g_free.back();
      g_free.pop_back();
      g_cached_bytes -= taken.cap;
      g_busy.emplace(taken.ptr, taken);
      *out = taken.ptr;
      break;
    }
    // (a pending event's hipErrorNotReady is no error of the caller's)
    if (pending) (void)hipGetLastError();
    if (*out) return hipSuccess;
  }
  Block fresh = {nullptr, cap, device, stream, nullptr};
  e = hipMalloc(&fresh.ptr, cap);
  if (e != hipSuccess) return e;
  e = hipEventCreateWithFlags(&fresh.freed, hipEventDisableTiming);
  if (e != hipSuccess) {
    hipFree(fresh.ptr);
    return e;
  }
  std::lock_guard<std::mutex> lock(g_mu);
  g_busy.emplace(fresh.ptr, fresh);
  *out = fresh.ptr;
  return hipSuccess;
}

hipError_t scratch_free(void *ptr, hipStream_t stream) {
  if (!ptr) return hipSuccess;
  std::vector<Block> release;
  hipError_t e;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    auto it = g_busy.find(ptr);
    if (it == g_busy.end()) return hipErrorInvalidValue;
    Block b = it->second;
    g_busy.erase(it);
    b.stream = stream;
    e = hipEventRecord(b.freed, stream);
    g_free.push_back(b);
    g_cached_bytes += b.cap;
    if (g_cached_bytes > kCacheLimit) {
      bool pending = false;
      for (size_t i = 0; i < g_free.size();) {
        if (g_free[i].device != b.device) {
          i++;
        } else if (hipEventQuery(g_free[i].freed) == hipSuccess) {
          release.push_back(g_free[i]);
          g_cached_bytes -= g_free[i].cap;
          g_free[i] = g_free.back();
          g_free.pop_back();
        } else {
          pending = true;
          i++;
        }
      }
      if (pending) (void)hipGetLastError();
    }
  }
  for (const Block &r : release) {
    hipEventDestroy(r.freed);
    hipFree(r.ptr);
  }
  return e;
}

}  // namespace bssl_amd
