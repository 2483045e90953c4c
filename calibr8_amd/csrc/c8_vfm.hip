// c8_vfm.hip -- the virtual fields method through the C ABI (c8_vfm_* in include/c8.h): the launches of the V, FS and A
// kernels (c8_assemble_vfm.hpp, c8_kernels.hip: k_vfm) and the single-block pass that sums their per-block partials.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/c8.h"
#include "c8_api_internal.hpp"

using namespace c8;

static int fail(int code, std::string const& msg) { return c8_fail(code, msg); }
#define C8_HIP(call)                                                                               \
  do {                                                                                             \
    hipError_t err__ = (call);                                                                     \
    if (err__ != hipSuccess) return fail(C8_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(err__)); \
  } while (0)

// out_v (if not null) += sum_b part[0][b]; out_g[i] += sum_b part[nv + i][b].  Thread t sums the blocks t, t + 256, ...
// in order, then a fixed tree over the threads: the same bits on every run.
constexpr int REDUCE_THREADS = 256;
__global__ void __launch_bounds__(REDUCE_THREADS) k_vfm_reduce(double const* part, int nblocks, int nout, double* out_v, double* out_g) {
  __shared__ double s[REDUCE_THREADS];
  int const t = threadIdx.x;
  int const nv = out_v ? 1 : 0;
  for (int o = 0; o < nout; ++o) {
    double a = 0.;
    for (int b = t; b < nblocks; b += REDUCE_THREADS) a += part[(size_t)o * nblocks + b];
    s[t] = a;
    __syncthreads();
    for (int w = REDUCE_THREADS / 2; w > 0; w >>= 1) {
      if (t < w) s[t] += s[t + w];
      __syncthreads();
    }
    if (t == 0) {
      double* dst = (o < nv) ? out_v : out_g + (o - nv);
      *dst += s[0];
    }
    __syncthreads();
  }
}

static int vfm_check(c8_ctx* c, char const* what) {
  if (!c) return fail(C8_ERR_ARG, std::string(what) + ": null ctx");
  if (c->nres != 1 || !c->ks.vfm_power)
    return fail(C8_ERR_UNSUPPORTED, std::string(what) + ": the virtual fields method applies to one-residual systems "
                                    "('mechanics_plane_stress' on tri3); under 'mechanics' the pressure is not measured");
  return C8_OK;
}

static bool vfm_state(const c8_state* st) { return st && st->x[0] && st->x_prev[0] && st->xi_prev && st->xi; }

// one kernel launch over the whole mesh, then the fixed-order sum of its partials into out_v / out_g
static int vfm_run(c8_ctx* c, VfmFn fn, const c8_state* st, VfmArgs const& va, double* b, double* out_v, double* out_g, char const* what) {
  if (!fn) return fail(C8_ERR_UNSUPPORTED, std::string(what) + ": not available for this element/model");
  int const nelems = c->mesh.nelems;
  int const gpb = c->ks.vfm_groups_per_block;
  int const nblocks = (nelems + gpb - 1) / gpb;
  int const nout = (out_v ? 1 : 0) + (out_g ? va.nact : 0);
  size_t const need = (size_t)(nout > 0 ? nout : 1) * (size_t)(nblocks > 0 ? nblocks : 1);
  if (need > c->vfm_part_n) {
    if (c->d_vfm_part) C8_HIP(hipFree(c->d_vfm_part));
    c->d_vfm_part = nullptr;
    c->vfm_part_n = 0;
    C8_HIP(hipMalloc((void**)&c->d_vfm_part, need * sizeof(double)));
    c->vfm_part_n = need;
  }
  SystemArgs sa{{{nullptr, nullptr}, {nullptr, nullptr}}, {b, nullptr}, c->d_status, 1};
  MeshTables const mt{c->d_conn, c->d_coords, c->d_nodeptr, c->d_pos, c->d_elem_set, nullptr, c->d_params, nullptr};
  FieldArgs const fa{st->x[0], st->x[1], st->x_prev[0], st->x_prev[1], st->xi_prev, st->xi};
  LaunchArgs a{mt, c->ms, fa, AdjointArgs{}, sa, 0, nelems, c->stream};
  C8_HIP(fn(a, va, c->d_vfm_part));
  if (nout > 0 && nelems > 0) {
    hipLaunchKernelGGL(k_vfm_reduce, dim3(1), dim3(REDUCE_THREADS), 0, c->stream, c->d_vfm_part, nblocks, nout, out_v, out_g);
    C8_HIP(hipGetLastError());
  }
  if (c->async) return C8_OK;
  return c8_status(c);
}

static VfmArgs vfm_args(c8_ctx const* c) { return VfmArgs{c->d_vfm_w, nullptr, nullptr, nullptr, 0., c->d_active, 0}; }

extern "C" {

int c8_vfm_set_virtual_field(c8_ctx* c, const double* w) {
  int const rc = vfm_check(c, "c8_vfm_set_virtual_field");
  if (rc) return rc;
  if (!w) return fail(C8_ERR_ARG, "c8_vfm_set_virtual_field: null w");
  c->d_vfm_w = w;
  return C8_OK;
}

int c8_vfm_internal_power(c8_ctx* c, const c8_state* st, double* b, double* ivw) {
  int const rc = vfm_check(c, "c8_vfm_internal_power");
  if (rc) return rc;
  if (!vfm_state(st) || !ivw) return fail(C8_ERR_ARG, "c8_vfm_internal_power: null argument");
  if (!c->d_vfm_w) return fail(C8_ERR_ARG, "c8_vfm_internal_power: no virtual field (c8_vfm_set_virtual_field)");
  return vfm_run(c, c->ks.vfm_power, st, vfm_args(c), b, ivw, nullptr, "c8_vfm_internal_power");
}

int c8_vfm_forward_sens(c8_ctx* c, const c8_state* st, const double* S_prev, double* S, double* ivw, double* divw) {
  int const rc = vfm_check(c, "c8_vfm_forward_sens");
  if (rc) return rc;
  VfmArgs va = vfm_args(c);
  va.nact = c8_num_active_params(c);
  va.S_prev = S_prev;
  va.S = S;
  if (!vfm_state(st) || !ivw || !divw || (va.nact > 0 && !S)) return fail(C8_ERR_ARG, "c8_vfm_forward_sens: null argument");
  if (S_prev && S_prev == S) return fail(C8_ERR_ARG, "c8_vfm_forward_sens: S_prev and S must be distinct arrays");
  if (!c->d_vfm_w) return fail(C8_ERR_ARG, "c8_vfm_forward_sens: no virtual field (c8_vfm_set_virtual_field)");
  return vfm_run(c, c->ks.vfm_forward_sens, st, va, nullptr, ivw, divw, "c8_vfm_forward_sens");
}

int c8_vfm_adjoint_step(c8_ctx* c, const c8_state* st, double cm, double* h, double* grad) {
  int const rc = vfm_check(c, "c8_vfm_adjoint_step");
  if (rc) return rc;
  if (!vfm_state(st) || !h || !grad) return fail(C8_ERR_ARG, "c8_vfm_adjoint_step: null argument");
  if (!c->d_vfm_w) return fail(C8_ERR_ARG, "c8_vfm_adjoint_step: no virtual field (c8_vfm_set_virtual_field)");
  VfmArgs va = vfm_args(c);
  va.nact = c8_num_active_params(c);
  va.h = h;
  va.c = cm;
  return vfm_run(c, c->ks.vfm_adjoint, st, va, nullptr, nullptr, grad, "c8_vfm_adjoint_step");
}

}  // extern "C"
