// rm_numerics_probe.hip -- the checked numerics of the strict plain-walk kernels (rm_trace.inc RM_CHECKED) beside the
// compiler's own square root and division, argument by argument, on the device.  A test hook, not part of the ABI
// (tests/test_gpu_checked_numerics.py): v_rsq_f64 cannot be emulated on a CPU, so the bit-equality the kernels rest on is
// checked where they run.
#define RM_KERNEL_GROUP 0
#define RM_KERNEL_FAST 0
#include "rm_render_kernel.hpp"

#pragma clang fp contract(off)

namespace {

// out[i]: bit 0 -- the checked norm differs from __builtin_sqrt(x) | 1 -- its reciprocal from 1. / that | 2 -- the
// discriminant's root from __builtin_sqrt(x) | 3 -- the guard says "outside" | 4 -- the norm's significand is all ones
__global__ __launch_bounds__(256) void rm_numerics_probe_kernel(const double *__restrict__ x, uint8_t *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    const rmdev_strict_checked::CheckedNorm c = rmdev_strict_checked::checked_norm(v);
    const double thc = rmdev_strict_checked::sqrt_discriminant(v);
    const double norm = __builtin_sqrt(v);
    const double inv = 1. / norm;
    auto bits = [](double d) { return __builtin_bit_cast(unsigned long long, d); };
    const unsigned long long nb = bits(c.norm);
    const bool ones = (nb & 0x000FFFFFFFFFFFFFull) == 0x000FFFFFFFFFFFFFull;
    out[i] = (uint8_t)((bits(c.norm) != bits(norm) ? 1u : 0u) | (bits(c.inv) != bits(inv) ? 2u : 0u) | (bits(thc) != bits(norm) ? 4u : 0u) |
                       (c.outside ? 8u : 0u) | (ones ? 16u : 0u));
}

}  // namespace

extern "C" rm_status rmi_numerics_probe(int device, const double *x, uint8_t *out, uint64_t n) {
    if (!x || !out || n == 0 || n > (1ull << 31)) { rm_set_host_error("rmi_numerics_probe: bad argument"); return RM_ERR_INVALID_ARG; }
    double *d_x = nullptr;
    uint8_t *d_out = nullptr;
    auto fail = [&](const char *what, hipError_t e) {
        rm_set_host_error(std::string("rmi_numerics_probe: ") + what + ": " + hipGetErrorString(e));
        if (d_x) (void)hipFree(d_x);
        if (d_out) (void)hipFree(d_out);
        return RM_ERR_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail("hipSetDevice", e);
    if ((e = hipMalloc(&d_x, n * sizeof(double))) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMalloc(&d_out, n)) != hipSuccess) return fail("hipMalloc", e);
    if ((e = hipMemcpy(d_x, x, n * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return fail("hipMemcpy", e);
    hipLaunchKernelGGL(rm_numerics_probe_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, 0, d_x, d_out, (size_t)n);
    if ((e = hipGetLastError()) != hipSuccess) return fail("launch", e);
    if ((e = hipMemcpy(out, d_out, n, hipMemcpyDeviceToHost)) != hipSuccess) return fail("hipMemcpy", e);
    (void)hipFree(d_x);
    (void)hipFree(d_out);
    return RM_OK;
}
