// hip_host.hpp — the host plumbing every *_api.hip shares: the last-error path, owning device buffers, streams and events
// that are destroyed on every way out of a C-ABI entry point (the error macro returns early), hipcub's two-call protocol,
// and the small helpers around a launch.  Host code only: nothing here reaches a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/defuse_dsa.h"

// (hidden: the library exports its C ABI, not the inline functions of this header)
namespace __attribute__((visibility("hidden"))) hiphost {

// printf into a module's last-error string; returns `code`, so that an entry point can `return fail(...)`.  The sinks stay
// with the modules (the C ABI has one *_last_error() each) and are thread_local there: tools call from helper threads.
inline int fail(std::string& sink, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    sink = buf;
    return code;
}

inline int hip_failed(std::string& sink, const char* call, hipError_t e, const char* file, int line)
{
    return fail(sink, DSA_E_DEVICE, "%s failed: %s (%s:%d)", call, hipGetErrorString(e), file, line);
}

// Run a HIP call; on failure leave "<call> failed: <text> (<file>:<line>)" in `sink` and return DSA_E_DEVICE from the
// calling function.  A module aliases it once with its own sink (#define EST_HIP(call) HIPHOST_TRY(g_est_err, call)).
#define HIPHOST_TRY(sink, call)                                                                          \
    do {                                                                                                 \
        const hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) return hiphost::hip_failed(sink, #call, e_, __FILE__, __LINE__);            \
    } while (0)

// DSA_OK if `device` is an ordinal this process can use, else DSA_E_DEVICE (and the reason in *sink, if given).
inline int check_device(int device, std::string* sink = nullptr)
{
    int n = 0;
    if (hipGetDeviceCount(&n) == hipSuccess && device >= 0 && device < n) return DSA_OK;
    if (sink) fail(*sink, DSA_E_DEVICE, "no usable HIP device %d", device);
    return DSA_E_DEVICE;
}

// How many elements a buffer allocates for a request of n.
struct ExactSize {
    static size_t of(size_t n) { return std::max<size_t>(n, 1); }
};
// dsa_api.hip's per-context buffers: a batch slightly larger than the last one does not re-allocate.
struct GrowSize {
    static size_t of(size_t n) { return n + n / 8 + 64; }
};

// Owning device memory, freed on every way out.  reserve(n) keeps what is there if it holds n elements, else frees it and
// allocates Size::of(n); after a successful reserve p is never null, whatever n.  The contents do not survive a growth.
template <typename T, class Size = ExactSize>
struct DeviceBuffer {
    T* p = nullptr;
    size_t cap = 0;   // elements
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { release(); }
    hipError_t reserve(size_t n)
    {
        if (p && n <= cap) return hipSuccess;
        release();
        const size_t want = Size::of(n);
        const hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    void swap(DeviceBuffer& o)
    {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
};

// The leading elements grow_keep carries over: a type of its own, so that a call cannot swap it with the size it asks for.
struct Keep {
    size_t n;
};

// Room for `need` elements without losing the first keep.n, whatever the buffer's Size policy.  Growth is geometric, so the
// bytes copied over a stream of pieces stay linear in its size.  The stream is synchronised before the old memory is freed.
template <typename T, class Size>
hipError_t grow_keep(DeviceBuffer<T, Size>& b, Keep keep, size_t need, hipStream_t st)
{
    if (b.p && need <= b.cap) return hipSuccess;
    const size_t want = std::max(Size::of(need), 2 * b.cap);
    DeviceBuffer<T, Size> next;
    hipError_t e = hipMalloc((void**)&next.p, want * sizeof(T));
    if (e != hipSuccess) return e;
    next.cap = want;
    if (keep.n && b.p) e = hipMemcpyAsync(next.p, b.p, keep.n * sizeof(T), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) b.swap(next);
    return e;
}

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create(unsigned flags = hipStreamDefault) { return hipStreamCreateWithFlags(&s, flags); }
    operator hipStream_t() const { return s; }
};

// One T in pinned host memory, which kernels store results into and the host reads after a synchronise.
template <typename T>
struct PinnedHost {
    T* p = nullptr;
    PinnedHost() = default;
    PinnedHost(const PinnedHost&) = delete;
    PinnedHost& operator=(const PinnedHost&) = delete;
    ~PinnedHost() { if (p) (void)hipHostFree(p); }
    hipError_t alloc() { return hipHostMalloc((void**)&p, sizeof(T)); }
    T* operator->() const { return p; }
};

// hipcub's two-call protocol: run(nullptr, bytes) asks for the temp size, tmp grows to it if it has to, run(tmp.p, bytes)
// does the work.  `run` is a callable (void* tmp, size_t& bytes) -> hipError_t around ONE hipcub call.  Call sites that size
// one temp buffer for several primitives up front, or query outside a loop and run inside, keep the two calls written out.
template <class Size, class Run>
hipError_t cub_run(DeviceBuffer<uint8_t, Size>& tmp, Run run)
{
    size_t bytes = 0;
    hipError_t e = run(nullptr, bytes);
    if (e == hipSuccess) e = tmp.reserve(bytes);
    if (e == hipSuccess) e = run(tmp.p, bytes);
    return e;
}

// workgroups of `block` threads that cover n items
inline unsigned grid_of(int64_t n, int block = 256) { return (unsigned)((n + block - 1) / block); }

// milliseconds between two recorded events; 0 if either has not completed
inline float elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}

}  // namespace hiphost
