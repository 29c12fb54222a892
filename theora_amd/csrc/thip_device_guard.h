// thip_device_guard.h -- for the host side of thip_decode.hip and thip_encode.hip.
#pragma once
#include <hip/hip_runtime.h>

// Makes `device` current for the calling host thread for the lifetime of the object (HIP's current
// device is per thread) and puts the previous one back: a state may live on any GPU of the node
// whatever the caller's current device is.
struct DeviceGuard {
  int prev = -1, want;
  explicit DeviceGuard(int device) : want(device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != want) (void)hipSetDevice(want);
  }
  ~DeviceGuard() {
    if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
  }
};
