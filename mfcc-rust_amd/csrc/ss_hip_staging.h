// What the host-pointer wrappers share on the HIP side: a HIP error as a status, the device probe and an owned device buffer.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "ss_internal.h"

namespace ss {

inline int hip_fail(hipError_t e, const char *what) { return fail(SS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

inline bool have_device()
{
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
}

// `path`: how the call site names itself ("hot path" in ss_api.hip)
inline int no_device(const char *path = "path")
{
    return fail(SS_ERR_HIP, std::string("no usable HIP device: the speechsauce_amd ") + path + " has no CPU fallback");
}

// A device allocation freed with its scope.  A request of 0 bytes still allocates (16 bytes): p is never null after alloc().
struct DeviceBuf {
    void *p = nullptr;
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf &) = delete;
    DeviceBuf &operator=(const DeviceBuf &) = delete;
    ~DeviceBuf()
    {
        if (p) (void)hipFree(p);
    }
    hipError_t hip_alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }  // for a chain of HIP calls with one message
    int alloc(size_t bytes)
    {
        const hipError_t e = hip_alloc(bytes);
        return e == hipSuccess ? SS_OK : hip_fail(e, "hipMalloc(&p, bytes ? bytes : 16)");
    }
    template <typename T>
    T *as() { return static_cast<T *>(p); }
};

}  // namespace ss
