// ubench_rsqrt.hip -- the relative error of v_rsq_f64 alone and after ONE Newton step (vfclik_amd/csrc/vfik_device.h's own rsqrt_1nr_pos,
// through the include vfik_aux.hip uses: nothing is restated here; rsqrt_1nr is the same sequence behind a clamp at 1e-300, and
// tests/test_gpu_blocks.py holds the two to the same bits), in units of u = 2^-53, against 1 / sqrtl(x) in the host's long double
// (64-bit mantissa): 2^20 arguments, mantissas from a fixed linear congruential sequence, exponents cycling over 1e-20 ... 1e4 --
// the squared distances |o - p|^2 a decay repeller can see between the 1e-10 floor tests and a workspace of 100 m.
// Prints the largest and the root-mean-square error of both; the figures quoted in DESIGN 6.2 come from this program on an MI355X.
#include "../vfclik_amd/csrc/vfik_kernel.h"

#include <cmath>
#include <cstdio>
#include <vector>

namespace vfik {
namespace {
#include "../vfclik_amd/csrc/vfik_device.h"
}  // namespace
}  // namespace vfik

__global__ void __launch_bounds__(256) k(const double* x, double* raw, double* one, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    raw[i] = __builtin_amdgcn_rsq(x[i]);
    one[i] = vfik::rsqrt_1nr_pos(x[i]);
}

int main() {
    const int n = 1 << 20;
    std::vector<double> x(n), raw(n), one(n);
    unsigned long long s = 88172645463325252ull;
    for (int i = 0; i < n; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const double m = 1.0 + (double)(s >> 11) * 0x1.0p-53;           // [1, 2)
        x[i] = std::ldexp(m, -67 + (i % 81));                           // 2^-67 = 6.8e-21 ... 2^13 = 8192
    }
    double *dx, *dr, *d1;
    if (hipMalloc(&dx, n * sizeof(double)) != hipSuccess || hipMalloc(&dr, n * sizeof(double)) != hipSuccess ||
        hipMalloc(&d1, n * sizeof(double)) != hipSuccess) { std::printf("hipMalloc failed\n"); return 1; }
    hipMemcpy(dx, x.data(), n * sizeof(double), hipMemcpyHostToDevice);
    k<<<n / 256, 256>>>(dx, dr, d1, n);
    if (hipDeviceSynchronize() != hipSuccess) { std::printf("kernel failed\n"); return 1; }
    hipMemcpy(raw.data(), dr, n * sizeof(double), hipMemcpyDeviceToHost);
    hipMemcpy(one.data(), d1, n * sizeof(double), hipMemcpyDeviceToHost);
    const long double u = 0x1.0p-53L;
    long double mr = 0, m1 = 0, sr = 0, s1 = 0;
    for (int i = 0; i < n; ++i) {
        const long double ref = 1.0L / sqrtl((long double)x[i]);
        const long double er = fabsl(((long double)raw[i] - ref) / ref) / u, e1 = fabsl(((long double)one[i] - ref) / ref) / u;
        mr = er > mr ? er : mr; m1 = e1 > m1 ? e1 : m1; sr += er * er; s1 += e1 * e1;
    }
    std::printf("v_rsq_f64 alone:     max %.4Lg u (%.3Lg relative), rms %.4Lg u\n", mr, mr * u, sqrtl(sr / n));
    std::printf("one Newton step:     max %.4Lg u (%.3Lg relative), rms %.4Lg u\n", m1, m1 * u, sqrtl(s1 / n));
    hipFree(dx); hipFree(dr); hipFree(d1);
    return 0;
}
