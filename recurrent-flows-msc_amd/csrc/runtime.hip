// What every translation unit of librfn_hip.so relies on: the per-thread error text behind rfn_last_error(), the ABI
// version that rfn_hip.lib checks on load, and the per-device split-K workspace of the convolutions.
#include "common.h"
#include "../../include/rfn_hip.h"
#include <stdarg.h>
#include <map>
#include <mutex>
#include <vector>

static thread_local char g_err[512] = "";
void rfn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* rfn_last_error(void) { return g_err; }
extern "C" int rfn_abi_version(void) { return 2; }

float* rfn_workspace(hipStream_t s, size_t floats) {
    // ONE buffer per device, whatever the stream: a hipGraph is captured on a fresh stream of its own, which must find
    // the buffer its eager warm-up runs (on other streams) have grown.  Consequence, stated in include/rfn_hip.h: split-K
    // convolutions issued on DIFFERENT streams of one device must not overlap in time.
    static std::mutex mu;
    static std::map<int, std::pair<float*, size_t>> tab;
    std::lock_guard<std::mutex> lock(mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    auto& e = tab[dev];
    if (e.second >= floats) return e.first;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone) {
        rfn_set_error("split-K workspace must grow to %zu floats during a hipGraph capture: run this shape eagerly first", floats);
        return nullptr;
    }
    // An outgrown buffer is NOT freed: a captured hipGraph has its address baked into kernel arguments and may be replayed
    // after an eager call of a larger shape made the buffer grow (generation between training steps).  Growth is geometric,
    // so the retired buffers add up to less than the live one; all of them go with the process.
    static std::vector<float*> retired;
    if (e.first) retired.push_back(e.first);
    e.first = nullptr;
    e.second = 0;
    const size_t want = 2 * floats + 1024;
    float* ptr = nullptr;
    if (hipMalloc(&ptr, want * sizeof(float)) != hipSuccess) {
        rfn_set_error("split-K workspace: hipMalloc of %zu bytes failed", want * sizeof(float));
        return nullptr;
    }
    e.first = ptr;
    e.second = want;
    return ptr;
}
