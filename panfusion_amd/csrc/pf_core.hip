// Status / error plumbing of the C ABI (include/panfusion_hip.h), and the dynamic-LDS helper every launcher with large tiles shares.
#include "pf_common.h"

namespace pf {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// hipFuncAttributeMaxDynamicSharedMemorySize of one kernel instantiation, set once per device: `done` is that instantiation's
// bitmask of the devices it is set on.  The steady-state launch pays a device-id lookup only.
pf_status allow_dynamic_lds(const void* kernel, size_t bytes, std::atomic<unsigned long long>& done, const char* what) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    const unsigned long long bit = dev >= 0 && dev < 64 ? 1ULL << dev : 0;      // (a device past 63 sets it on every launch)
    if (e == hipSuccess && (done.load(std::memory_order_relaxed) & bit)) return PF_OK;
    if (e == hipSuccess) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
    if (e != hipSuccess) { set_error("%s: hipFuncSetAttribute failed: %s", what, hipGetErrorString(e)); return PF_ERR_LAUNCH; }
    done.fetch_or(bit, std::memory_order_relaxed);
    return PF_OK;
}
}  // namespace pf

extern "C" int pf_version(void) { return 101; }
extern "C" const char* pf_last_error_string(void) { return pf::g_err; }
