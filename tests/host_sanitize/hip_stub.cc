// A stand-in for the HIP runtime, for the HOST-SIDE sanitizer builds of the library (tests/test_host_sanitizers.py): every source under
// torch-assimilate_amd/csrc is compiled host-only (`hipcc --cuda-host-only`: kernels become launch stubs) with -fsanitize=address,undefined
// or -fsanitize=thread and linked against this file instead of libamdhip64.  "Device" memory is host memory, kernels do nothing (their
// launches are counted), events complete at once.  What runs for real is what the sanitizers are here for: the step driver's two launch
// threads, job queues, slot rotation, per-workspace tables, option snapshots, the custom-communicator callbacks.
// An opt-in call trace (mia_stub_trace_enable; off for the sanitizer driver) keeps one line per launch, event operation, asynchronous
// fill / copy and note of the driver in memory, for tests/test_step_call_trace.py: kernels by the name their registration gave
// (template arguments included), streams as the small integers the driver passes, events numbered by first appearance.
// Test infrastructure only: nothing in the product links it.
#include <hip/hip_runtime_api.h>
#include <cxxabi.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

namespace {
std::atomic<long long> g_launches{0}, g_events{0};
std::mutex g_mu;
std::set<void*> g_allocs;
thread_local struct { dim3 g, b; size_t shm; hipStream_t s; } t_cfg;
struct StubEvent { std::atomic<long long> recorded{0}; };
// ---- call trace
std::atomic<bool> g_trace{false}, g_trace_attr{false};
std::map<const void*, std::string>& kernel_names() { static auto* m = new std::map<const void*, std::string>(); return *m; }      // (filled by static initialisers)
std::map<const void*, int> g_event_ids;
int g_event_next = 0;
std::vector<std::string> g_lines;
// "void mia::kernel<2, 3, false>(args...)" -> "mia::kernel<2,3,false>"
std::string short_name(const char* mangled) {
  int status = 0;
  char* d = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
  std::string full = (status == 0 && d) ? d : mangled, out;
  free(d);
  if (full.compare(0, 5, "void ") == 0) full.erase(0, 5);
  for (size_t at; (at = full.find("(anonymous namespace)::")) != std::string::npos;) full.erase(at, 23);
  int depth = 0;
  for (char c : full) {
    if (c == '<') ++depth;
    if (c == '>') --depth;
    if (c == '(' && depth == 0) break;
    if (c != ' ') out += c;
  }
  return out;
}
int event_id(const void* e) {      // (g_mu held)
  if (!e) return -1;
  auto it = g_event_ids.find(e);
  if (it == g_event_ids.end()) it = g_event_ids.emplace(e, g_event_next++).first;
  return it->second;
}
unsigned long sid(hipStream_t s) { return (unsigned long)reinterpret_cast<uintptr_t>(s); }
void trace(const char* fmt, ...) {      // (g_mu held)
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_lines.emplace_back(buf);
}
void trace_launch(const char* how, const void* f, dim3 g, dim3 b, size_t shm, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  if (!g_trace.load(std::memory_order_relaxed)) return;
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = kernel_names().find(f);
  const std::string n = it == kernel_names().end() ? "?" : short_name(it->second.c_str());
  if (e0 || e1 || how[0] == 'e')
    trace("%s %s grid %u %u %u block %u %u %u lds %zu stream %#lx start ev %d stop ev %d", how, n.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, shm, sid(s),
          event_id(e0), event_id(e1));
  else
    trace("%s %s grid %u %u %u block %u %u %u lds %zu stream %#lx", how, n.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, shm, sid(s));
}
#define TRACE_EVENT(what, e, s) do { if (g_trace.load(std::memory_order_relaxed)) { std::lock_guard<std::mutex> lk_(g_mu); trace(what " ev %d stream %#lx", event_id(e), sid(s)); } } while (0)
#define TRACE_BYTES(what, n, s) do { if (g_trace.load(std::memory_order_relaxed)) { std::lock_guard<std::mutex> lk_(g_mu); trace(what " %zu stream %#lx", (size_t)(n), sid(s)); } } while (0)

void* dev_alloc(size_t n) {
  void* p = nullptr;
  if (posix_memalign(&p, 256, n ? n : 1) != 0) return nullptr;
  memset(p, 0, n);
  std::lock_guard<std::mutex> lk(g_mu);
  g_allocs.insert(p);
  return p;
}
}  // namespace

extern "C" long long mia_stub_launch_count() { return g_launches.load(); }
extern "C" long long mia_stub_live_allocations() { std::lock_guard<std::mutex> lk(g_mu); return (long long)g_allocs.size(); }
// the call trace: switch it on or off; add a line of the driver's own (a communicator callback); print what was collected and forget it
// (bit 2 adds an "attr <kernel> <bytes>" line per hipFuncSetAttribute, for tests/test_tile_launch_trace.py; 1 alone traces as ever)
extern "C" void mia_stub_trace_enable(int on) { g_trace.store(on != 0); g_trace_attr.store((on & 2) != 0); }
extern "C" void mia_stub_trace_note(const char* text) {
  if (!g_trace.load()) return;
  std::lock_guard<std::mutex> lk(g_mu);
  g_lines.emplace_back(text);
}
extern "C" void mia_stub_trace_flush(FILE* to) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (const auto& l : g_lines) fprintf(to, "%s\n", l.c_str());
  g_lines.clear();
}

extern "C" {
hipError_t hipMalloc(void** p, size_t n) { *p = dev_alloc(n); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipExtMallocWithFlags(void** p, size_t n, unsigned) { *p = dev_alloc(n); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) {
  if (!p) return hipSuccess;
  { std::lock_guard<std::mutex> lk(g_mu); if (!g_allocs.erase(p)) return hipErrorInvalidValue; }
  free(p);
  return hipSuccess;
}
hipError_t hipMemset(void* p, int v, size_t n) { memset(p, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t s) { memset(p, v, n); TRACE_BYTES("memset", n, s); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t st) { memcpy(d, s, n); TRACE_BYTES("memcpy", n, st); return hipSuccess; }
hipError_t hipMemcpy2DAsync(void* d, size_t dp, const void* s, size_t sp, size_t w, size_t h, hipMemcpyKind, hipStream_t) {
  for (size_t r = 0; r < h; ++r) memcpy((char*)d + r * dp, (const char*)s + r * sp, w);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = reinterpret_cast<hipEvent_t>(new StubEvent()); ++g_events; return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) { if (!a || !b || !ms) return hipErrorInvalidHandle; *ms = 0.01f; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) {
  if (g_trace.load(std::memory_order_relaxed)) { std::lock_guard<std::mutex> lk(g_mu); g_event_ids.erase(e); }      // (ids exist only while tracing; the address may come back as another event)
  delete reinterpret_cast<StubEvent*>(e); --g_events; return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { if (!e) return hipErrorInvalidHandle; ++reinterpret_cast<StubEvent*>(e)->recorded; TRACE_EVENT("record", e, s); return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t e) { if (!e) return hipErrorInvalidHandle; (void)reinterpret_cast<StubEvent*>(e)->recorded.load(); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { if (!e) return hipErrorInvalidHandle; (void)reinterpret_cast<StubEvent*>(e)->recorded.load(); if (g_trace.load(std::memory_order_relaxed)) { std::lock_guard<std::mutex> lk(g_mu); trace("sync ev %d", event_id(e)); } return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t s) { return (reinterpret_cast<uintptr_t>(s) & 4) ? hipErrorNotReady : hipSuccess; }      // (some streams busy, some idle)
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { if (!e) return hipErrorInvalidHandle; (void)reinterpret_cast<StubEvent*>(e)->recorded.load(); TRACE_EVENT("wait", e, s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* st) { *st = hipStreamCaptureStatusNone; return hipSuccess; }
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute, int bytes) {
  if (g_trace_attr.load(std::memory_order_relaxed)) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = kernel_names().find(f);
    trace("attr %s %d", it == kernel_names().end() ? "?" : short_name(it->second.c_str()).c_str(), bytes);
  }
  return hipSuccess;
}
hipError_t hipIpcGetMemHandle(hipIpcMemHandle_t*, void*) { return hipErrorNotSupported; }
hipError_t hipIpcOpenMemHandle(void**, hipIpcMemHandle_t, unsigned) { return hipErrorNotSupported; }
hipError_t hipIpcCloseMemHandle(void*) { return hipErrorNotSupported; }
hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t shm, hipStream_t s) { ++g_launches; trace_launch("launch", f, g, b, shm, s, nullptr, nullptr); return hipSuccess; }
hipError_t hipExtLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t shm, hipStream_t s, hipEvent_t start, hipEvent_t stop, int) {
  ++g_launches;
  trace_launch("extlaunch", f, g, b, shm, s, start, stop);
  if (start) ++reinterpret_cast<StubEvent*>(start)->recorded;
  if (stop) ++reinterpret_cast<StubEvent*>(stop)->recorded;
  return hipSuccess;
}
// what clang's kernel-launch stubs and fat-binary registration call
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t shm, hipStream_t s) { t_cfg.g = g; t_cfg.b = b; t_cfg.shm = shm; t_cfg.s = s; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* shm, hipStream_t* s) { *g = t_cfg.g; *b = t_cfg.b; *shm = t_cfg.shm; *s = t_cfg.s; return hipSuccess; }
void** __hipRegisterFatBinary(const void*) { static void* handle = nullptr; return &handle; }
void __hipRegisterFunction(void**, const void* host, char* name, const char*, unsigned, void*, void*, void*, void*, int*) {
  kernel_names()[host] = name ? name : "?";      // host stub pointer -> device name (static initialisers: one thread)
}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipRegisterManagedVar(void**, void**, void*, const char*, size_t, unsigned) {}
void __hipUnregisterFatBinary(void**) {}
}
