// host_launch.h — what every entry point's host side does before and at a
// launch: argument alignment, the devices of the calling thread and of the
// stream, the launch itself and a chain of launches (Chain), a layer's
// workspace (Carver, Workspace), and the device copies of a host table
// (device_ok, upload, free_all).  Host only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <tuple>
#include <type_traits>
#include <utility>

#include "sccsum.h"
#include "wire.h"

namespace host_launch {

// p is not a multiple of a (a power of two); a null pointer is aligned.
inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// The calling thread's current device (*cur) and the device a launch on `s`
// runs on (*sdev): hipStreamGetDevice for a real stream, the current device
// for the null stream.  Returns the HIP error that stopped it; *cur is written
// once hipGetDevice has succeeded, *sdev only on success.  What the error, or a
// stream of another device, means is each caller's own rule.
inline hipError_t stream_devices(hipStream_t s, int* cur, int* sdev) {
    int c = 0;
    hipError_t e = hipGetDevice(&c);
    if (e != hipSuccess) return e;
    *cur = c;
    hipDevice_t sd = c;
    if (s != nullptr && (e = hipStreamGetDevice(s, &sd)) != hipSuccess) return e;
    *sdev = sd;
    return hipSuccess;
}

// The rx / tx layers' rule: the launches run on the stream's device, which must
// be `want` (a table's device), or with want < 0 the calling thread's current
// one, where the data is.
inline int stream_ok(hipStream_t s, int want) {
    int dev = -1, sd = -1;  // dev stays -1 when there is no current device to ask for
    const hipError_t e = stream_devices(s, &dev, &sd);
    if (e != hipSuccess) return e == hipErrorNoDevice && dev < 0 ? SCCSUM_ENODEV : static_cast<int>(e);
    return sd != (want < 0 ? dev : want) ? SCCSUM_EINVAL : SCCSUM_OK;
}

// Every launch goes through hipLaunchKernel, which returns THIS launch's
// error: the caller's pending HIP error from an earlier, unrelated call is
// neither dropped nor read as this launch failing.  The
// arguments are converted to the kernel's own parameter types first.
template <typename... P, typename... A>
hipError_t launch_kernel(void (*k)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, A&&... a) {
    static_assert(sizeof...(P) == sizeof...(A), "argument count");
    std::tuple<std::decay_t<P>...> t(static_cast<std::decay_t<P>>(std::forward<A>(a))...);
    void* args[sizeof...(P)];
    std::apply([&](auto&... x) {
        size_t i = 0;
        ((args[i++] = static_cast<void*>(&x)), ...);
    }, t);
    return hipLaunchKernel(reinterpret_cast<const void*>(k), grid, block, args, lds_bytes, s);
}

// An entry point's launches, in order, on one stream: each runs only while none
// has failed, and rc() is the first failure's own error.  A helper that returns
// a hipError_t joins in as `if (c.ok()) c.e = helper(stream, ...);`.
struct Chain {
    hipStream_t s;
    hipError_t e = hipSuccess;

    bool ok() const { return e == hipSuccess; }
    int rc() const { return static_cast<int>(e); }
    template <typename... P, typename... A>
    void launch(void (*k)(P...), dim3 grid, dim3 block, size_t lds_bytes, A&&... a) {
        if (e == hipSuccess) e = launch_kernel(k, grid, block, lds_bytes, s, std::forward<A>(a)...);
    }
};

// Lays a workspace out: take() gives the next array's offset, its start rounded
// up to `align` (a power of two), and end() the size, rounded up likewise, that
// a layer's *_workspace function returns.
struct Carver {
    uint64_t at = 0;

    uint64_t take(uint64_t bytes, uint64_t align = 1) {
        const uint64_t here = end(align);
        at = here + bytes;
        return here;
    }
    uint64_t end(uint64_t align = 16) const { return (at + align - 1) & ~(align - 1); }
};

// The caller's workspace: the array a Carver put at `offset`, with its element
// type named at the call site (u32 and u64 are the two most arrays have).
struct Workspace {
    uint8_t* base;

    explicit Workspace(void* d_workspace) : base(static_cast<uint8_t*>(d_workspace)) {}
    template <typename T>
    T* at(uint64_t offset) const { return reinterpret_cast<T*>(base + offset); }
    uint32_t* u32(uint64_t offset) const { return at<uint32_t>(offset); }
    uint64_t* u64(uint64_t offset) const { return at<uint64_t>(offset); }
};

// `device` can hold a table's device copy: SCCSUM_OK, SCCSUM_ENODEV for a
// device that is not there (or no device at all), or the HIP error.
inline int device_ok(int device) {
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess) return e == hipErrorNoDevice ? SCCSUM_ENODEV : static_cast<int>(e);
    return device < 0 || device >= ndev || device >= wire::kMaxDevices ? SCCSUM_ENODEV : SCCSUM_OK;
}

// One array of a host table.
struct HostArray {
    const void* data;
    size_t bytes;
};

// What the *_destroy of a table does with its device copies (null ones are
// skipped): every one is freed, the first error is returned.
inline hipError_t free_all(std::initializer_list<void*> copies) {
    hipError_t first = hipSuccess;
    for (void* d : copies) {
        const hipError_t e = d ? hipFree(d) : hipSuccess;
        if (first == hipSuccess) first = e;
    }
    return first;
}

// A copy of every array on `device`, dev[i] for arrays.begin()[i]; the caller's
// device is put back.  On a failure nothing stays allocated and every dev[i]
// is null.  Returns SCCSUM_OK or the HIP error, as device_ok does.
inline int upload(int device, std::initializer_list<HostArray> arrays, void** dev) {
    for (size_t i = 0; i < arrays.size(); ++i) dev[i] = nullptr;
    int cur = 0;
    hipError_t e = hipGetDevice(&cur);
    if (e == hipSuccess) e = hipSetDevice(device);
    if (e != hipSuccess) return static_cast<int>(e);
    for (size_t i = 0; i < arrays.size(); ++i) {
        const HostArray& a = arrays.begin()[i];
        if (e == hipSuccess) e = hipMalloc(&dev[i], a.bytes);
        if (e == hipSuccess) e = hipMemcpy(dev[i], a.data, a.bytes, hipMemcpyHostToDevice);
    }
    (void)hipSetDevice(cur);  // the caller's binding is put back
    if (e != hipSuccess) {
        for (size_t i = 0; i < arrays.size(); ++i) {
            if (dev[i]) (void)hipFree(dev[i]);
            dev[i] = nullptr;
        }
    }
    return static_cast<int>(e);
}

}  // namespace host_launch
