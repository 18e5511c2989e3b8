// What the host-pointer wrappers share on the HIP side: a HIP error as a status, the device probe, an owned device buffer and
// HostStage, the staging of one host-pointer call (ss_host_stage.h) over the HIP runtime.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "ss_host_stage.h"
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
    int alloc(size_t bytes)
    {
        const hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        return e == hipSuccess ? SS_OK : hip_fail(e, "hipMalloc(&p, bytes ? bytes : 16)");
    }
    template <typename T>
    T *as() { return static_cast<T *>(p); }
};

// HostStageT's steps as blocking HIP calls
struct HipStageBackend {
    static const char *text(hipError_t e) { return e == hipSuccess ? nullptr : hipGetErrorString(e); }
    const char *alloc(void **p, size_t bytes) { return text(hipMalloc(p, bytes)); }
    void free(void *p) { (void)hipFree(p); }
    const char *up(void *dev, const void *host, size_t bytes) { return text(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice)); }
    const char *down(void *host, const void *dev, size_t bytes) { return text(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost)); }
    const char *sync() { return text(hipDeviceSynchronize()); }
};

// The stager of the library's host-pointer calls.  The two strided copies of the dense forms: `rows` rows of `width` bytes between
// the caller's block (pitch bytes from row to row) and a compact device block.
struct HostStage : HostStageT<HipStageBackend> {
    using HostStageT::HostStageT;
    void up_rows(void *dev, const void *host, size_t pitch, size_t width, size_t rows)
    {
        if (ok()) staged(HipStageBackend::text(hipMemcpy2D(dev, width, host, pitch, width, rows, hipMemcpyHostToDevice)));
    }
    void down_rows(void *host, size_t pitch, const void *dev, size_t width, size_t rows)
    {
        if (ok()) downed(HipStageBackend::text(hipMemcpy2D(host, pitch, dev, width, width, rows, hipMemcpyDeviceToHost)));
    }
};

}  // namespace ss
