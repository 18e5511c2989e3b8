// The staging of one synchronous host-pointer call: upload, run the device form, synchronise, download.  A HostStageT owns the
// call's device blocks and one sticky status -- the first failure stays and every later step is a no-op -- and it is the one place
// of the three fixed messages (a failed allocation or upload, "<name>: device error", a failed download).  What it keeps: nothing
// is written to the caller's buffers after a failure, and a pool is scattered only once everything before succeeded.  Nothing is
// pooled, cached or asynchronous: one allocation per block, one copy per transfer.
// Pure host C++17 over a backend B -- no HIP include -- so tools/hosttest/test_host_stage.cpp runs the sequencing against a logging
// fake under the sanitizers; ss_hip_staging.h supplies the HIP backend and the HostStage the library uses.  B's steps return null,
// or the error's text:
//   const char *alloc(void **p, size_t bytes);   void free(void *p);   const char *sync();
//   const char *up(void *dev, const void *host, size_t bytes);   const char *down(void *host, const void *dev, size_t bytes);
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "ss_host_checks.h"

namespace ss {

template <class B>
class HostStageT {
public:
    // the staged form of a pool's named rows (PoolRows): the slot table 0 .. n_active - 1 and the compact block of rows
    struct Pool {
        const int32_t *slots;
        float *rows;  // null where the pool has no state (len == 0): nothing is allocated for it
    };

    // `name`: how the call names itself in "<name>: device error"
    explicit HostStageT(const char *name, B backend = B()) : name_(name), b_(backend) {}
    HostStageT(const HostStageT &) = delete;
    HostStageT &operator=(const HostStageT &) = delete;
    ~HostStageT()
    {
        for (void *p : blocks_)
            if (p) b_.free(p);
    }

    bool ok() const { return rc_ == SS_OK; }
    int status() const { return rc_; }

    // a device block of `bytes`; 0 bytes still allocates (16): the pointer is null only after a failure
    template <typename T>
    T *room(size_t bytes)
    {
        if (!ok()) return nullptr;
        blocks_.push_back(nullptr);
        staged(b_.alloc(&blocks_.back(), bytes ? bytes : 16));
        return static_cast<T *>(blocks_.back());
    }
    // the caller's `bytes` at host into (the start of) a block; 0 bytes: nothing is copied
    void fill(void *dev, const void *host, size_t bytes)
    {
        if (ok() && bytes) staged(b_.up(dev, host, bytes));
    }
    // a device block holding the caller's `bytes` at host
    template <typename T>
    T *up(const T *host, size_t bytes)
    {
        T *p = room<T>(bytes);
        fill(p, host, bytes);
        return p;
    }
    Pool up_pool(const PoolRows &named)
    {
        Pool d{up(named.iota.data(), named.iota.size() * sizeof(int32_t)), nullptr};
        if (named.len > 0) d.rows = up(named.rows_host.data(), named.bytes());
        return d;
    }

    // the status of the device form, or of any other step of the call: `if (st.ok()) st.ran(ss_xxx_device(..))`
    void ran(int rc) { rc_ = rc; }
    void sync()
    {
        if (ok() && b_.sync()) rc_ = fail(SS_ERR_HIP, std::string(name_) + ": device error");
    }
    // `bytes` of a device block to the caller; `what` goes between the download message's fixed head and the error's text
    void down(void *host, const void *dev, size_t bytes, const char *what = "")
    {
        if (ok() && bytes) downed(b_.down(host, dev, bytes), what);
    }
    // the named rows come down into their staging block; the caller's pool is written by scatter(), the call's last step
    void down_pool(PoolRows &named, const Pool &d, const char *what = "")
    {
        if (named.len > 0) down(named.rows_host.data(), d.rows, named.bytes(), what);
    }
    void scatter(const PoolRows &named, float *pool, const int32_t *slots) const
    {
        if (ok()) named.scatter(pool, slots);
    }

protected:
    void staged(const char *err)
    {
        if (err) rc_ = fail(SS_ERR_HIP, std::string("host staging: ") + err);
    }
    void downed(const char *err, const char *what = "")
    {
        if (err) rc_ = fail(SS_ERR_HIP, std::string("hipMemcpy D2H") + what + ": " + err);
    }

private:
    const char *name_;
    B b_;
    int rc_ = SS_OK;
    std::vector<void *> blocks_;
};

}  // namespace ss
