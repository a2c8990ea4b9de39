// mse_host.h -- host-side pieces the library's translation units share.
#pragma once

#include <hip/hip_runtime.h>

// sets mse_last_error() and returns `status` (defined in mse_lib.hip, beside the thread's last-error string)
int mse_internal_fail(int status, const char *msg);

// compute units of the current device; 0 without one
static inline int cu_count()
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return cus;
}
