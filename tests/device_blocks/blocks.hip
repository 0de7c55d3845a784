// blocks.hip -- a TEST-ONLY harness around the float64 building blocks of vfclik_amd/csrc/vfik_device.h: one trivial kernel per block,
// out[i] = f(in[i]), so that tests/test_gpu_blocks.py can hold each block to the 50-digit reference of tests/hp_blocks.py at arguments of
// its own choosing.  The header is included as vfik_aux.hip includes it (after vfik_kernel.h, inside `namespace vfik { namespace {`) and its
// own functions are called: nothing is restated here.  Never linked into the product (libvfik_blocks.so, tests/device_blocks/Makefile).
//
// Blocks are 64 threads = one wave: element i is lane i mod 64 of wave i div 64, so the order of the test's input decides the composition
// of every wave (pow_order dispatches on it).  Rows are row-major: `cols` doubles in, OUT_COLS[block] doubles out per element.
#include "../../vfclik_amd/csrc/vfik_kernel.h"

namespace vfik {
namespace {
#include "../../vfclik_amd/csrc/vfik_device.h"

#define BLOCK_KERNEL(name, IC, OC, ...)                                                                       \
    __global__ void __launch_bounds__(64) name(const double* in, double* out, long count, const double* table) { \
        const long i = (long)blockIdx.x * 64 + threadIdx.x;                                                   \
        if (i >= count) return;                                                                               \
        const double* x = in + i * IC;                                                                        \
        double* y = out + i * OC;                                                                             \
        (void)table;                                                                                          \
        __VA_ARGS__                                                                                           \
    }

BLOCK_KERNEL(k_rcp_raw, 1, 1, y[0] = __builtin_amdgcn_rcp(x[0]);)
BLOCK_KERNEL(k_rsq_raw, 1, 1, y[0] = __builtin_amdgcn_rsq(x[0]);)
BLOCK_KERNEL(k_rcp_nr, 1, 1, y[0] = rcp_nr(x[0]);)
BLOCK_KERNEL(k_rcp_1nr, 1, 1, y[0] = rcp_1nr(x[0]);)
BLOCK_KERNEL(k_rsqrt_1nr, 1, 1, y[0] = rsqrt_1nr(x[0]);)
BLOCK_KERNEL(k_rsqrt_1nr_pos, 1, 1, y[0] = rsqrt_1nr_pos(x[0]);)
BLOCK_KERNEL(k_sqrt_rsqrt, 1, 2, double r, v; sqrt_rsqrt(x[0], r, v); y[0] = r; y[1] = v;)
BLOCK_KERNEL(k_rsqrt_n4, 4, 4, double a[4], v[4]; for (int j = 0; j < 4; ++j) a[j] = x[j]; rsqrt_n<4>(a, v);
             for (int j = 0; j < 4; ++j) y[j] = v[j];)
BLOCK_KERNEL(k_sincos_fast, 1, 2, double s, c; sincos_fast(x[0], s, c); y[0] = s; y[1] = c;)
BLOCK_KERNEL(k_sincos_fast_n4, 4, 8, double a[4], s[4], c[4]; for (int j = 0; j < 4; ++j) a[j] = x[j]; sincos_fast_n<4>(a, s, c);
             for (int j = 0; j < 4; ++j) { y[j] = s[j]; y[4 + j] = c[j]; })
BLOCK_KERNEL(k_powi_uniform, 2, 1, y[0] = powi_uniform(x[0], (int)x[1]);)
BLOCK_KERNEL(k_pow_order, 2, 1, y[0] = pow_order(x[0], x[1]);)
BLOCK_KERNEL(k_atan_kernel, 1, 1, y[0] = atan_kernel(x[0]);)
BLOCK_KERNEL(k_atan2_pos, 2, 1, y[0] = atan2_pos(x[0], x[1]);)
BLOCK_KERNEL(k_mac_unfused, 3, 1, y[0] = mac_unfused(x[0], x[1], x[2]);)
BLOCK_KERNEL(k_mul_unfused, 2, 1, y[0] = mul_unfused(x[0], x[1]);)

// sincos_tab_n reads (sin, cos)(k pi/32) from the wave's LDS copy of the table: the 64 x 2 doubles the test passes, as the cycle kernels stage
// the last KiB of the constants' image
__global__ void __launch_bounds__(64) k_sincos_tab_n4(const double* in, double* out, long count, const double* table) {
    __shared__ __attribute__((aligned(16))) double tab[128];
    tab[2 * threadIdx.x] = table[2 * threadIdx.x];
    tab[2 * threadIdx.x + 1] = table[2 * threadIdx.x + 1];
    __syncthreads();
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    double a[4], s[4], c[4];
    for (int j = 0; j < 4; ++j) a[j] = in[i * 4 + j];
    sincos_tab_n<4>(a, reinterpret_cast<const char*>(tab), s, c);
    for (int j = 0; j < 4; ++j) { out[i * 8 + j] = s[j]; out[i * 8 + 4 + j] = c[j]; }
}

typedef void (*BlockKernel)(const double*, double*, long, const double*);
struct BlockDesc { BlockKernel k; int in_cols, out_cols; };
const BlockDesc BLOCKS[] = {
    {k_rcp_raw, 1, 1}, {k_rsq_raw, 1, 1}, {k_rcp_nr, 1, 1}, {k_rcp_1nr, 1, 1}, {k_rsqrt_1nr, 1, 1}, {k_rsqrt_1nr_pos, 1, 1},
    {k_sqrt_rsqrt, 1, 2}, {k_rsqrt_n4, 4, 4}, {k_sincos_fast, 1, 2}, {k_sincos_fast_n4, 4, 8}, {k_sincos_tab_n4, 4, 8},
    {k_powi_uniform, 2, 1}, {k_pow_order, 2, 1}, {k_atan_kernel, 1, 1}, {k_atan2_pos, 2, 1}, {k_mac_unfused, 3, 1}, {k_mul_unfused, 2, 1}};
constexpr int N_BLOCKS = (int)(sizeof(BLOCKS) / sizeof(BLOCKS[0]));
constexpr int BLOCK_TAB = 10;
}  // namespace
}  // namespace vfik

// The one entry: block id (index into BLOCKS; tests/hp_blocks.py names them), `count` rows of `cols` doubles at `in` (host), the result rows
// at `out` (host, count x the block's output columns), `table` = 128 doubles (host) for sincos_tab_n, else ignored.  The batch is padded
// to whole waves with copies of its last row, so that every lane of every wave is active and a padding lane never changes a wave's
// composition.  Allocates, copies, launches, synchronises, copies back, frees; returns the HIP error (hipErrorInvalidValue for a bad request).
extern "C" int vfik_blocks_run(int block, const double* in, int cols, double* out, long count, const double* table) {
    using namespace vfik;
    if (block < 0 || block >= N_BLOCKS || !in || !out || count <= 0 || count > (1L << 24)) return (int)hipErrorInvalidValue;
    const BlockDesc& d = BLOCKS[block];
    if (cols != d.in_cols || (block == BLOCK_TAB && !table)) return (int)hipErrorInvalidValue;
    const long npad = (count + 63) / 64 * 64;
    std::string host((size_t)npad * cols * sizeof(double), '\0');
    double* hp = reinterpret_cast<double*>(&host[0]);
    std::copy(in, in + count * cols, hp);
    for (long i = count; i < npad; ++i) std::copy(in + (count - 1) * cols, in + count * cols, hp + i * cols);
    double *din = nullptr, *dout = nullptr, *dtab = nullptr;
    hipError_t e = hipMalloc(&din, (size_t)npad * cols * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&dout, (size_t)npad * d.out_cols * sizeof(double));
    if (e == hipSuccess && block == BLOCK_TAB) e = hipMalloc(&dtab, 128 * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(din, hp, (size_t)npad * cols * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && dtab) e = hipMemcpy(dtab, table, 128 * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        d.k<<<dim3((unsigned)(npad / 64)), dim3(64)>>>(din, dout, npad, dtab);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)count * d.out_cols * sizeof(double), hipMemcpyDeviceToHost);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    if (dtab) (void)hipFree(dtab);
    return (int)e;
}
