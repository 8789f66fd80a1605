// fbx_wave_reduce_test.hip -- the wave reductions of fbx_common.hpp by themselves (tests/test_wave_reduce_gpu.py).  Not part of
// libfbx.so (build.py compiles csrc/*.hip only): build.py build_wave_reduce_test() makes libfbx_wavered.so from this file alone.
// One launch of ONE wavefront walks `nsets` input sets of [16][64] doubles (row = value, column = lane) and writes per set
//   [ 0, 16)  wave_sum(row k)                      k = 0 .. 15
//   [16, 32)  wave_sum_lean(row k)
//   [32, 34)  wave_sum_n<2>  over rows 0 .. 1
//   [34, 40)  wave_sum_n<6>  over rows 0 .. 5
//   [40, 56)  wave_sum_n<16> over rows 0 .. 15
//   [56, 72)  wave_max(row k)
//   [72, 88)  wave_max_lean(row k)
// as raw doubles (the test compares bits).
#include "../fbx_common.hpp"
#include <hip/hip_runtime.h>

namespace {

constexpr int ROWS = 16, OUT = 88;

__global__ void __launch_bounds__(64) wave_reduce_kernel(const double* __restrict__ in, int nsets, double* __restrict__ out) {
    const int lane = threadIdx.x;
    for (int s = 0; s < nsets; ++s) {
        const double* x = in + (size_t)s * ROWS * 64;
        double* o = out + (size_t)s * OUT;
        double v[ROWS];
#pragma unroll
        for (int k = 0; k < ROWS; ++k) v[k] = x[k * 64 + lane];
        double r[OUT];
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            r[k] = fbx::wave_sum(v[k]); r[16 + k] = fbx::wave_sum_lean(v[k]);
            r[56 + k] = fbx::wave_max(v[k]); r[72 + k] = fbx::wave_max_lean(v[k]);
        }
        { double a[2]; for (int k = 0; k < 2; ++k) a[k] = v[k]; fbx::wave_sum_n(a); for (int k = 0; k < 2; ++k) r[32 + k] = a[k]; }
        { double a[6]; for (int k = 0; k < 6; ++k) a[k] = v[k]; fbx::wave_sum_n(a); for (int k = 0; k < 6; ++k) r[34 + k] = a[k]; }
        { double a[16]; for (int k = 0; k < 16; ++k) a[k] = v[k]; fbx::wave_sum_n(a); for (int k = 0; k < 16; ++k) r[40 + k] = a[k]; }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < OUT; ++k) o[k] = r[k];
        }
    }
}

}  // namespace

// host pointers in and out; returns the HIP error code (0 = success)
extern "C" __attribute__((visibility("default"))) int fbx_test_wave_reduce(const double* in, int nsets, double* out) {
    if (nsets <= 0) return -1;
    const size_t nin = sizeof(double) * (size_t)nsets * ROWS * 64, nout = sizeof(double) * (size_t)nsets * OUT;
    double *d_in = nullptr, *d_out = nullptr;
    hipError_t e = hipMalloc(&d_in, nin);
    if (e == hipSuccess) e = hipMalloc(&d_out, nout);
    if (e == hipSuccess) e = hipMemcpy(d_in, in, nin, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(wave_reduce_kernel, dim3(1), dim3(64), 0, 0, d_in, nsets, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, nout, hipMemcpyDeviceToHost);
    if (d_in) (void)hipFree(d_in);
    if (d_out) (void)hipFree(d_out);
    return (int)e;
}
