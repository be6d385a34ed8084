// Host-side launch helpers shared by the .hip files: the dynamic-LDS opt-in and the CU count, both per DEVICE.
// (A process may use several devices: hipFuncSetAttribute acts on the function object of the current device only.)
#pragma once
#include <atomic>
#include "common.h"

constexpr int LAUNCH_MAX_DEVICES = 64;   // device indices with a cache slot

// Index of the current device in the per-device caches below, or < 0 where there is none (the runtime cannot say, or the index has
// no slot).  A launcher that needs the CU count for its grid asks once and hands the index to device_cus8() and launch_dyn_on().
inline int current_device() {
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < LAUNCH_MAX_DEVICES ? dev : -1;
}

// Launch KERNEL on the current device (dev = current_device()) with lds_bytes of dynamic LDS (above the 64 KiB a kernel gets
// without asking): the opt-in is made once per (instantiation, device).  Returns 0, the HIP error of the opt-in or of the launch,
// or M3AE_ERR_UNSUPPORTED for a device without a slot.
template <auto KERNEL, class... A>
int launch_dyn_on(int dev, dim3 grid, dim3 block, int lds_bytes, hipStream_t s, const A&... args) {
    static std::atomic<bool> opted_in[LAUNCH_MAX_DEVICES];
    if (dev < 0) return M3AE_ERR_UNSUPPORTED;
    if (!opted_in[dev].load(std::memory_order_relaxed)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();   // reported here, not by the next call's hip_launch_status()
            return (int)e;
        }
        opted_in[dev].store(true, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(KERNEL, grid, block, lds_bytes, s, args...);
    return hip_launch_status();
}
template <auto KERNEL, class... A>
int launch_dyn(dim3 grid, dim3 block, int lds_bytes, hipStream_t s, const A&... args) {
    return launch_dyn_on<KERNEL>(current_device(), grid, block, lds_bytes, s, args...);
}

// compute units of device dev (256 if the runtime cannot say)
inline int device_cus(int dev = current_device()) {
    static std::atomic<int> cus[LAUNCH_MAX_DEVICES];   // 0: not asked yet
    if (dev < 0) return 256;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        hipDeviceProp_t prop;
        n = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}
// ... rounded down to a multiple of 8: a persistent grid of that size keeps every tile on the XCD of its one-tile-per-workgroup launch
inline int device_cus8(int dev = current_device()) { return device_cus(dev) / 8 * 8; }
