// math_device.hip -- the operations of calibr8_amd/csrc/c8_math.hpp on the device, one lane per case (TEST
// INFRASTRUCTURE, no part of libc8.so).  The kernel calls the table of tests/math_ops.hpp, the same one the CPU hook
// c8emu_math_op compiles, so tests/test_gpu_dual_math.py sees the device build of the header (c8_rcp's v_rcp_f64 path,
// the device libm, the compiler's contraction) on its own.
#include <hip/hip_runtime.h>

#include "../math_ops.hpp"

// case c: operation op[c] on in[18 c ..], din[18 c ..] -> out[21 c ..], dout[21 c ..]
__global__ void math_kernel(int const* __restrict__ op, double const* __restrict__ in, double const* __restrict__ din,
                            int n_cases, double* __restrict__ out, double* __restrict__ dout, int* __restrict__ rc) {
  int const c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cases) return;
  double x[c8_math_ops::MO_NIN], dx[c8_math_ops::MO_NIN], y[c8_math_ops::MO_NOUT], dy[c8_math_ops::MO_NOUT];
  for (int k = 0; k < c8_math_ops::MO_NIN; ++k) {
    x[k] = in[(size_t)c * c8_math_ops::MO_NIN + k];
    dx[k] = din[(size_t)c * c8_math_ops::MO_NIN + k];
  }
  rc[c] = c8_math_ops::math_op(op[c], x, dx, y, dy);
  for (int k = 0; k < c8_math_ops::MO_NOUT; ++k) {
    out[(size_t)c * c8_math_ops::MO_NOUT + k] = y[k];
    dout[(size_t)c * c8_math_ops::MO_NOUT + k] = dy[k];
  }
}

// Host arrays in, host arrays out: copies, one launch, copies back.  op, rc: [n_cases]; in, din: [n_cases][18]; out, dout:
// [n_cases][21]; rc[c] is the number of result slots of case c (-1: unknown operation).  Returns 0 or the HIP error.
extern "C" int c8mathdev_run(int const* op, double const* in, double const* din, int n_cases, double* out, double* dout,
                             int* rc) {
  if (n_cases <= 0) return 0;
  size_t const n = (size_t)n_cases;
  size_t const b_in = n * c8_math_ops::MO_NIN * sizeof(double), b_out = n * c8_math_ops::MO_NOUT * sizeof(double);
  int *d_op = nullptr, *d_rc = nullptr;
  double *d_in = nullptr, *d_din = nullptr, *d_out = nullptr, *d_dout = nullptr;
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
  if (ok(hipMalloc(&d_op, n * sizeof(int))) && ok(hipMalloc(&d_rc, n * sizeof(int))) && ok(hipMalloc(&d_in, b_in)) &&
      ok(hipMalloc(&d_din, b_in)) && ok(hipMalloc(&d_out, b_out)) && ok(hipMalloc(&d_dout, b_out)) &&
      ok(hipMemcpy(d_op, op, n * sizeof(int), hipMemcpyHostToDevice)) && ok(hipMemcpy(d_in, in, b_in, hipMemcpyHostToDevice)) &&
      ok(hipMemcpy(d_din, din, b_in, hipMemcpyHostToDevice))) {
    int const block = 64;
    math_kernel<<<dim3((unsigned)((n + block - 1) / block)), dim3(block)>>>(d_op, d_in, d_din, n_cases, d_out, d_dout, d_rc);
    ok(hipGetLastError());
    ok(hipDeviceSynchronize());
    ok(hipMemcpy(out, d_out, b_out, hipMemcpyDeviceToHost));
    ok(hipMemcpy(dout, d_dout, b_out, hipMemcpyDeviceToHost));
    ok(hipMemcpy(rc, d_rc, n * sizeof(int), hipMemcpyDeviceToHost));
  }
  void* const bufs[6] = {d_op, d_rc, d_in, d_din, d_out, d_dout};
  for (void* p : bufs) (void)hipFree(p);
  return (int)e;
}
