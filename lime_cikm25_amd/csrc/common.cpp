// Error reporting, the cached CU count and the ABI version of liblime_hip.so.
#include "common.h"

static thread_local char g_err[512] = "";

void lime_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static thread_local char g_kernel[160] = "";

void lime_set_last_linear_kernel(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kernel, sizeof(g_kernel), fmt, ap);
    va_end(ap);
}

int lime_num_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, cus = 0;
        const bool ok = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess;
        n = (ok && cus > 0) ? cus : 256;
    }
    return n;
}

extern "C" int64_t lime_device_cus(void) { return lime_num_cus(); }
extern "C" const char* lime_last_linear_kernel(void) { return g_kernel; }
extern "C" int lime_abi_version(void) { return LIME_ABI_VERSION; }
extern "C" const char* lime_last_error_string(void) { return g_err; }
