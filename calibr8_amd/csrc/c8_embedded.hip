// c8_embedded.hip -- the embedded network of hybrid_hyper_J2_plane_stress through the C ABI (c8_*_embedded_* in
// include/c8.h): its description and weights in a device buffer the kernels read (c8_models.hpp: nn_value_slope), and
// the launch of the weight-gradient kernel (c8_assemble_nn.hpp) after the conventional K5.
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

static bool is_hybrid(c8_ctx const* c) { return c && c->model == MODEL_HYBRID_HYPER_J2_PLANE_STRESS; }

// NN(0) into the buffer's header, evaluated on the device by the code the kernels evaluate NN(s_in alpha) with: at
// alpha = 0 the hardening is then exactly 0
__global__ void k_nn_at_zero(double* nn) {
  C8_NN_WORK(w);
  double y, dy;
  nn_value_slope(nn, 0., w, y, dy);
  nn[NN_HEADER - 4] = y;
}

extern "C" {

int c8_set_embedded_model(c8_ctx* c, const c8_embedded_model_desc* d) {
  if (!c || !d) return fail(C8_ERR_ARG, "c8_set_embedded_model: null argument");
  if (!is_hybrid(c)) return fail(C8_ERR_UNSUPPORTED, "c8_set_embedded_model: the model has no embedded network");
  if (c->gather_pending) return fail(C8_ERR_ARG, "c8_set_embedded_model: a staged assembly is waiting for c8_gather_finish");
  if (d->activation < C8_ACT_RELU || d->activation > C8_ACT_TANH) return fail(C8_ERR_ARG, "c8_set_embedded_model: unknown activation");
  int const n = d->num_layers;
  if (n < 3 || n > NN_MAX_HIDDEN + 2 || !d->topology)
    return fail(C8_ERR_ARG, "c8_set_embedded_model: the topology needs 3 to 6 entries (at most 4 hidden layers)");
  if (d->topology[0] != 1 || d->topology[n - 1] != 1) return fail(C8_ERR_ARG, "c8_set_embedded_model: input and output widths must be 1");
  int ntheta = 0;
  for (int l = 0; l < n; ++l) {
    if (l > 0 && l < n - 1 && (d->topology[l] < 1 || d->topology[l] > NN_MAX_WIDTH))
      return fail(C8_ERR_ARG, "c8_set_embedded_model: hidden widths must be 1 .. 64");
    if (l + 1 < n) ntheta += d->topology[l + 1] * (d->topology[l] + 1);
  }
  std::vector<double> nn((size_t)NN_HEADER + ntheta, 0.);
  nn[0] = d->activation;
  nn[1] = n;
  for (int l = 0; l < n; ++l) nn[2 + l] = d->topology[l];
  nn[NN_HEADER - 6] = d->input_scale;
  nn[NN_HEADER - 5] = d->output_scale;
  if (c->d_nn) C8_HIP(hipFree(c->d_nn));
  c->d_nn = nullptr;
  c->nn_ready = false;
  c->nn_ntheta = 0;
  C8_HIP(hipMalloc((void**)&c->d_nn, nn.size() * sizeof(double)));
  c->nn_host = nn;
  c->nn_ntheta = ntheta;
  return C8_OK;
}

int c8_num_embedded_params(const c8_ctx* c) {
  if (!c) return C8_ERR_ARG;
  return is_hybrid(c) ? c->nn_ntheta : 0;
}

int c8_set_embedded_params(c8_ctx* c, const double* theta) {
  if (!c || !theta) return fail(C8_ERR_ARG, "c8_set_embedded_params: null argument");
  if (!is_hybrid(c)) return fail(C8_ERR_UNSUPPORTED, "c8_set_embedded_params: the model has no embedded network");
  if (c->gather_pending) return fail(C8_ERR_ARG, "c8_set_embedded_params: a staged assembly is waiting for c8_gather_finish");
  if (c->nn_ntheta <= 0) return fail(C8_ERR_ARG, "c8_set_embedded_params: no network (c8_set_embedded_model)");
  std::copy(theta, theta + c->nn_ntheta, c->nn_host.begin() + NN_HEADER);
  C8_HIP(hipMemcpyAsync(c->d_nn, c->nn_host.data(), c->nn_host.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_nn_at_zero, dim3(1), dim3(1), 0, c->stream, c->d_nn);
  C8_HIP(hipGetLastError());
  C8_HIP(hipMemcpyAsync(&c->nn_host[NN_HEADER - 4], c->d_nn + NN_HEADER - 4, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  C8_HIP(hipStreamSynchronize(c->stream));
  c->nn_ready = true;
  return C8_OK;
}

int c8_get_embedded_params(const c8_ctx* c, double* theta) {
  if (!c || !theta) return fail(C8_ERR_ARG, "c8_get_embedded_params: null argument");
  if (!is_hybrid(c)) return fail(C8_ERR_UNSUPPORTED, "c8_get_embedded_params: the model has no embedded network");
  if (c->nn_ntheta <= 0) return fail(C8_ERR_ARG, "c8_get_embedded_params: no network (c8_set_embedded_model)");
  std::copy(c->nn_host.begin() + NN_HEADER, c->nn_host.end(), theta);
  return C8_OK;
}

int c8_num_grad_params(const c8_ctx* c) {
  if (!c) return C8_ERR_ARG;
  return c8_num_active_params(c) + c8_num_embedded_params(c);
}

}  // extern "C"

int c8_embedded_param_gradient(c8_ctx* c, const c8_state* st, const double* phi, double* grad) {
  if (!is_hybrid(c)) return C8_OK;
  if (!c->nn_ready) return fail(C8_ERR_ARG, "c8_param_gradient: the embedded network is not set");
  int const npts = c->mesh.nelems * c->npts0;
  int const nblocks = nn_grad_blocks(npts);
  size_t const need = (size_t)nblocks * c->nn_ntheta;
  if (need > c->nn_part_n) {
    if (c->d_nn_part) C8_HIP(hipFree(c->d_nn_part));
    c->d_nn_part = nullptr;
    c->nn_part_n = 0;
    C8_HIP(hipMalloc((void**)&c->d_nn_part, need * sizeof(double)));
    c->nn_part_n = need;
  }
  NnGradArgs const ga{c->d_nn, st->xi, phi, c->d_elem_set, c->d_params, npts, c->npts0, c->nloc, c->nparams,
                      c->ms.abs_tol, c->nn_ntheta, c->d_nn_part};
  C8_HIP(launch_nn_param_gradient(ga, grad + c8_num_active_params(c), c->stream));
  return C8_OK;
}
