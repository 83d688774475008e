// host_scratch.hpp -- what the host forms of the C boundary share: finding the device, and device buffers that live for
// one call.  A host form checks its arguments, calls open_device, holds a DevScratch on the stream the call works on, runs
// the device form and downloads the result; every way out, the early returns of MI_HIP included, waits for that stream
// and frees what the call allocated.
#pragma once
#include <vector>

#include "common.hpp"

namespace mi {

// the number of visible devices; none at all is MI_ERR_NO_DEVICE
inline int visible_devices(int* ndev) {
    int rc = mi_device_count(ndev);
    if (rc) return rc;
    if (*ndev == 0) return fail(MI_ERR_NO_DEVICE, "no HIP device visible");
    return MI_OK;
}

// a host form's first device call, after every argument check
inline int open_device(int device) {
    int ndev = 0;
    int rc = visible_devices(&ndev);
    if (rc) return rc;
    MI_HIP(hipSetDevice(device));
    return MI_OK;
}

// Device buffers of one call, bound to the stream `st` the call works on.  The destructor waits for `st` alone -- never for
// the device, `st` may be a handle's stream -- and frees every buffer handed out, so nothing is freed under work that reads it.
// Every member returns a status: a failed allocation is MI_ERR_NOMEM "out of device memory" with HIP's sticky error
// cleared, a failed copy or wait is MI_HIP's mapping (hipErrorOutOfMemory -> MI_ERR_NOMEM, anything else -> MI_ERR_HIP).
class DevScratch {
  public:
    explicit DevScratch(hipStream_t st) : st_(st) {}
    DevScratch(const DevScratch&) = delete;
    DevScratch& operator=(const DevScratch&) = delete;
    ~DevScratch() {
        (void)hipStreamSynchronize(st_);
        for (void* q : bufs_) (void)hipFree(q);
    }
    // *p = a buffer of `bytes` (0: one byte, so that the pointer is never null)
    template <typename T>
    int alloc(T** p, size_t bytes) {
        void* q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 1) != hipSuccess) {
            (void)hipGetLastError();
            return fail(MI_ERR_NOMEM, "out of device memory");
        }
        bufs_.push_back(q);
        *p = (T*)q;
        return MI_OK;
    }
    // *p = a buffer holding the `bytes` at `host`, copied on the stream (the host array outlives the call's last wait)
    template <typename T>
    int upload(T** p, const void* host, size_t bytes) {
        int rc = alloc(p, bytes);
        if (rc) return rc;
        MI_HIP(hipMemcpyAsync(*p, host, bytes, hipMemcpyHostToDevice, st_));
        return MI_OK;
    }
    // wait for what was enqueued, report a launch that failed, then copy `bytes` at `dev` out and wait for the copy
    int download(void* host, const void* dev, size_t bytes) {
        MI_HIP(hipStreamSynchronize(st_));
        MI_HIP(hipGetLastError());
        MI_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st_));
        MI_HIP(hipStreamSynchronize(st_));
        return MI_OK;
    }

  private:
    hipStream_t st_;
    std::vector<void*> bufs_;
};

}  // namespace mi
