// host_launch.h — what every entry point's host side does before and at a
// launch (sccsum.hip, steer.hip, send.hip): argument alignment, the devices of
// the calling thread and of the stream, and the launch itself.  Host only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <tuple>
#include <type_traits>
#include <utility>

#include "sccsum.h"

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

}  // namespace host_launch
