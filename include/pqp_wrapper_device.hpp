// pqp_wrapper_device.hpp — PathOptimizationNS::detail::DeviceArray: the device memory of the wrappers that keep distance layers on the
// GPU (FootprintChecker, AgentOverlay).  Apart from pqp_wrapper_detail.hpp because only those two include the HIP runtime API.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "pqp_wrapper_detail.hpp"

namespace PathOptimizationNS {
namespace detail {

inline hipStream_t stream_of(const OwnedHandle& h) { return (hipStream_t)h.stream(); }

// grow-only, freed with its owner; what it held is not kept when it grows
class DeviceArray {
 public:
    DeviceArray() = default;
    DeviceArray(const DeviceArray&) = delete;
    DeviceArray& operator=(const DeviceArray&) = delete;
    ~DeviceArray() { if (p_) (void)hipFree(p_); }

    bool grow(size_t bytes) {
        if (bytes <= cap_) return true;
        if (p_) (void)hipFree(p_);
        p_ = nullptr; cap_ = 0;
        if (hipMalloc(&p_, bytes) != hipSuccess) { p_ = nullptr; return false; }
        cap_ = bytes;
        return true;
    }
    // the layers a wrapper is built on: a blocking copy, on `device`
    bool upload(int device, const void* host, size_t bytes) {
        return hipSetDevice(device) == hipSuccess && grow(bytes) && hipMemcpy(p_, host, bytes, hipMemcpyHostToDevice) == hipSuccess;
    }
    template <class T> T* as() const { return static_cast<T*>(p_); }

 private:
    void* p_ = nullptr;
    size_t cap_ = 0;
};

}  // namespace detail
}  // namespace PathOptimizationNS
