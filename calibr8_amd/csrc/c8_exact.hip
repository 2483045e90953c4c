// c8_exact.hip -- c8_eval_exact_errors and c8_eval_linearization_errors: the directional derivative of the adjoint-weighted
// element residuals along (fine state - stored state), and the residuals linearised there (c8_exact.hpp), one lane per
// (element, point).  A translation unit of its own: the instantiations of the other units keep their code generation.
#include <hip/hip_runtime.h>

#include <string>

// the embedded network's work buffer is the lane's, as in c8_error.hip (every lane has a point of its own)
#define C8_NN_WORK(name)              \
  double name##_buf[4 * NN_MAX_WIDTH]; \
  double* const name = name##_buf

#include "../../include/c8.h"
#include "c8_api_internal.hpp"
#include "c8_exact.hpp"
#include "c8_registry.hpp"

namespace c8 {

constexpr int EXACT_BLOCK = 256;
// whole elements only, as k_error: hex8 32, tet4 51, tri3 64, tri3 plane stress 256
template <class E> constexpr int exact_elems_per_block() { return EXACT_BLOCK / error_lanes<E>(); }

// Block layout, LDS slots and the order of the sums are those of k_error (c8_error.hip): EPB = 256 / L consecutive elements
// a block, the lanes of ip set 0 element-major, then those of ip set 1; every value to the slot [element of the block]
// [point of set 0, then point of set 1]; after the barrier lane t < EPB sums the slots of element t in that order and
// SUBTRACTS the sums from the two outputs (E += -sum): no atomics, the same inputs give the same bytes.  LIN: the
// linearization errors (value + tangent), else the exact errors (tangent).  One wavefront per SIMD: 512 registers a lane.
template <class E, template <class> class ModelT, bool LIN>
__global__ void __launch_bounds__(EXACT_BLOCK, 1)
k_exact(MeshTables mt, ModelSettings ms, FieldArgs fa, FieldArgs ff, ErrorArgs ea, double* E_R, double* E_C, int nelems) {
  constexpr int S = error_slots<E>(), L = error_lanes<E>(), EPB = exact_elems_per_block<E>();
  constexpr int N0 = EPB * E::NP0, L1 = L - E::NP0, N1 = EPB * L1;
  __shared__ double part_R[EPB * S], part_C[EPB * E::NP0];
  int const t = threadIdx.x;
  long long const e0 = (long long)blockIdx.x * EPB;
  if (t < N0 + N1) {
    int const el = t < N0 ? t / E::NP0 : (t - N0) / (L1 > 0 ? L1 : 1);
    int const slot = t < N0 ? t % E::NP0 : E::NP0 + (t - N0) % (L1 > 0 ? L1 : 1);
    double er = 0., ec = 0., er_same = 0.;
    if (e0 + el < nelems) exact_terms<E, ModelT, LIN>(mt, ms, fa, ff, ea, (int)(e0 + el), slot, er, ec, er_same);
    part_R[el * S + slot] = er;
    if (slot < E::NP0) {
      part_C[el * E::NP0 + slot] = ec;
      if constexpr (error_shares_points<E>()) part_R[el * S + E::NP0 + slot] = er_same;
    }
  }
  __syncthreads();
  if (t < EPB && e0 + t < nelems) {
    double sr = 0., sc = 0.;
    C8_UNROLL
    for (int s = 0; s < S; ++s) sr += part_R[t * S + s];
    C8_UNROLL
    for (int s = 0; s < E::NP0; ++s) sc += part_C[t * E::NP0 + s];
    E_R[e0 + t] += -sr;
    E_C[e0 + t] += -sc;
  }
}

typedef hipError_t (*ExactFn)(MeshTables const&, ModelSettings const&, FieldArgs const&, FieldArgs const&, ErrorArgs const&,
                              double* E_R, double* E_C, int nelems, hipStream_t);

template <class E, template <class> class ModelT, bool LIN>
static hipError_t launch_exact(MeshTables const& mt, ModelSettings const& ms, FieldArgs const& fa, FieldArgs const& ff,
                               ErrorArgs const& ea, double* E_R, double* E_C, int nelems, hipStream_t stream) {
  if (nelems <= 0) return hipSuccess;
  constexpr int EPB = exact_elems_per_block<E>();
  unsigned const grid = (unsigned)(((long long)nelems + EPB - 1) / EPB);
  hipLaunchKernelGGL((k_exact<E, ModelT, LIN>), dim3(grid), dim3(EXACT_BLOCK), 0, stream, mt, ms, fa, ff, ea, E_R, E_C, nelems);
  return hipGetLastError();
}
template <class E, template <class> class ModelT> static ExactFn exact_fn(ModelTag<ModelT>, bool lin) {
  return lin ? &launch_exact<E, ModelT, true> : &launch_exact<E, ModelT, false>;
}

// the row of the model table on the element class it runs on, as error_kernel (c8_error.hip)
static ExactFn exact_kernel(int elem_type, int model, bool lin) {
  ExactFn fn = nullptr;
  visit_models([&](auto row) {
    using R = decltype(row);
    if (row.id != model) return;
    if constexpr (R::dim == 3) {
      if (elem_type == C8_HEX8) fn = exact_fn<Elem<C8_HEX8>>(row, lin);
      if (elem_type == C8_TET4) fn = exact_fn<Elem<C8_TET4>>(row, lin);
    } else {
      if (elem_type == C8_TRI3) fn = exact_fn<typename R::Elem2D>(row, lin);
    }
  });
  return fn;
}

static int eval_exact(char const* who, bool lin, c8_ctx* c, const c8_state* st, const c8_state* sf, const double* const z[2],
                      const double* phi, double* E_R, double* E_C) {
  std::string const name(who);
  if (!c || !st || !sf || !z || !phi || !E_R || !E_C) return c8_fail(C8_ERR_ARG, name + ": null argument");
  if (!st->xi || !st->xi_prev || !sf->xi || !sf->xi_prev) return c8_fail(C8_ERR_ARG, name + ": null local state");
  for (int i = 0; i < c->nres; ++i) {  // under mechanics_plane_stress (one residual) the entries [1] are ignored
    if (!st->x[i] || !st->x_prev[i] || !sf->x[i] || !sf->x_prev[i]) return c8_fail(C8_ERR_ARG, name + ": null global state");
    if (!z[i]) return c8_fail(C8_ERR_ARG, name + ": null adjoint solution");
  }
  if (c->model == MODEL_HYBRID_HYPER_J2_PLANE_STRESS && !c->nn_ready)
    return c8_fail(C8_ERR_ARG, name + ": the embedded network is not set (c8_set_embedded_model, c8_set_embedded_params)");
  ExactFn const fn = exact_kernel(c->mesh.elem_type, c->model, lin);
  if (!fn) return c8_fail(C8_ERR_UNSUPPORTED, name + ": not available for this element/model");
  MeshTables const mt{c->d_conn, c->d_coords, c->d_nodeptr, c->d_pos, c->d_elem_set, nullptr, c->d_params, nullptr, c->d_nn};
  FieldArgs const fa{st->x[0], st->x[1], st->x_prev[0], st->x_prev[1], st->xi_prev, st->xi};
  FieldArgs const ff{sf->x[0], sf->x[1], sf->x_prev[0], sf->x_prev[1], sf->xi_prev, sf->xi};  // read only
  ErrorArgs const ea{z[0], c->nres == 2 ? z[1] : nullptr, phi};
  hipError_t const err = fn(mt, c->ms, fa, ff, ea, E_R, E_C, c->mesh.nelems, c->stream);
  if (err != hipSuccess) return c8_fail(C8_ERR_DEVICE, name + ": " + hipGetErrorString(err));
  return c->async ? C8_OK : c8_status(c);
}

}  // namespace c8

using namespace c8;

extern "C" int c8_eval_exact_errors(c8_ctx* c, const c8_state* st, const c8_state* st_fine, const double* const z[2],
                                    const double* phi, double* E_R, double* E_C) {
  return eval_exact("c8_eval_exact_errors", false, c, st, st_fine, z, phi, E_R, E_C);
}

extern "C" int c8_eval_linearization_errors(c8_ctx* c, const c8_state* st, const c8_state* st_fine, const double* const z[2],
                                            const double* phi, double* E_lin_R, double* E_lin_C) {
  return eval_exact("c8_eval_linearization_errors", true, c, st, st_fine, z, phi, E_lin_R, E_lin_C);
}
