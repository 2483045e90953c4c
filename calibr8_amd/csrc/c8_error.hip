// c8_error.hip -- c8_eval_error_contributions: the adjoint-weighted element residuals E_R and E_C (c8_error.hpp), one lane
// per (element, point).  A translation unit of its own: the instantiations of c8_kernels.hip keep their
// code generation.
#include <hip/hip_runtime.h>

#include <string>

// The embedded network of hybrid_hyper_J2_plane_stress: c8_models.hpp keeps its work buffer in LDS, one per group of six
// lanes that evaluate the same point.  Here every lane has a point of its own, so the buffer is the lane's (4 x 64 doubles,
// indexed by the layer loops: private memory, 2 KiB of scratch per lane of that one instance).
#define C8_NN_WORK(name)              \
  double name##_buf[4 * NN_MAX_WIDTH]; \
  double* const name = name##_buf

#include "../../include/c8.h"
#include "c8_api_internal.hpp"
#include "c8_error.hpp"
#include "c8_registry.hpp"

namespace c8 {

constexpr int ERROR_BLOCK = 256;
// wavefronts per SIMD the register budget is set for.  1: 512 registers a lane, which the hex8 instances need to stay out of
// scratch (264 to 470 of them).  -DC8_TUNE_ERROR_WAVES=2 (tuning build, same results) halves the budget:
// those instances then keep 28 to 880 bytes of a lane in scratch and the small_J2 one is slower by a third (measured).
#ifndef C8_TUNE_ERROR_WAVES
#define C8_TUNE_ERROR_WAVES 1
#endif
// whole elements only: an element's points never straddle a workgroup (hex8 32, tet4 51, tri3 64, tri3 plane stress 256)
template <class E> constexpr int error_elems_per_block() { return ERROR_BLOCK / error_lanes<E>(); }

// A block takes EPB = 256 / L consecutive elements, L = error_lanes<E>() the evaluations of an element: NP0 + NP1, or NP0
// where the two ip sets share their points (hex8: the lane of point pt of set 0 also returns the pressure term of point pt
// of set 1, for which it has everything in hand -- half the lanes and half the gathers of a lane per point of either set).
// Its first EPB * NP0 lanes evaluate the points of ip set 0 (element-major, so the NP0 lanes of an element share its
// connectivity row and nodal lines), the next EPB * (L - NP0) lanes the points of ip set 1, the rest (fewer than L) idle: the
// two kinds of point differ by the whole constitutive evaluation, and kept apart they share a wavefront only at the seam.
// Every value goes to the LDS slot [element of the block][point of set 0, then point of set 1]; after the barrier lane
// t < EPB sums the slots of element t in that order and adds the sums to E_R and E_C: one read-modify-write of 8 bytes per
// lane at consecutive addresses, no atomics, the order of every sum fixed by the element class alone.
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(ERROR_BLOCK, C8_TUNE_ERROR_WAVES)
k_error(MeshTables mt, ModelSettings ms, FieldArgs fa, ErrorArgs ea, double* E_R, double* E_C, int nelems) {
  constexpr int S = error_slots<E>(), L = error_lanes<E>(), EPB = error_elems_per_block<E>();
  constexpr int N0 = EPB * E::NP0, L1 = L - E::NP0, N1 = EPB * L1;
  __shared__ double part_R[EPB * S], part_C[EPB * E::NP0];
  int const t = threadIdx.x;
  long long const e0 = (long long)blockIdx.x * EPB;
  if (t < N0 + N1) {
    int const el = t < N0 ? t / E::NP0 : (t - N0) / (L1 > 0 ? L1 : 1);
    int const slot = t < N0 ? t % E::NP0 : E::NP0 + (t - N0) % (L1 > 0 ? L1 : 1);
    double er = 0., ec = 0., er_same = 0.;
    if (e0 + el < nelems) error_point<E, ModelT>(mt, ms, fa, ea, (int)(e0 + el), slot, er, ec, er_same);
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
    E_R[e0 + t] += sr;
    E_C[e0 + t] += sc;
  }
}

typedef hipError_t (*ErrorFn)(MeshTables const&, ModelSettings const&, FieldArgs const&, ErrorArgs const&, double* E_R, double* E_C,
                              int nelems, hipStream_t);

template <class E, template <class> class ModelT>
static hipError_t launch_error(MeshTables const& mt, ModelSettings const& ms, FieldArgs const& fa, ErrorArgs const& ea, double* E_R,
                               double* E_C, int nelems, hipStream_t stream) {
  if (nelems <= 0) return hipSuccess;
  constexpr int EPB = error_elems_per_block<E>();
  unsigned const grid = (unsigned)(((long long)nelems + EPB - 1) / EPB);
  hipLaunchKernelGGL((k_error<E, ModelT>), dim3(grid), dim3(ERROR_BLOCK), 0, stream, mt, ms, fa, ea, E_R, E_C, nelems);
  return hipGetLastError();
}
template <class E, template <class> class ModelT> static ErrorFn error_fn(ModelTag<ModelT>) { return &launch_error<E, ModelT>; }

// the row of the model table on the element class it runs on: 3-D rows on hex8 and tet4, 2-D rows on the row's tri3 class
static ErrorFn error_kernel(int elem_type, int model) {
  ErrorFn fn = nullptr;
  visit_models([&](auto row) {
    using R = decltype(row);
    if (row.id != model) return;
    if constexpr (R::dim == 3) {
      if (elem_type == C8_HEX8) fn = error_fn<Elem<C8_HEX8>>(row);
      if (elem_type == C8_TET4) fn = error_fn<Elem<C8_TET4>>(row);
    } else {
      if (elem_type == C8_TRI3) fn = error_fn<typename R::Elem2D>(row);
    }
  });
  return fn;
}

}  // namespace c8

using namespace c8;

extern "C" int c8_eval_error_contributions(c8_ctx* c, const c8_state* st, const double* const z[2], const double* phi, double* E_R,
                                           double* E_C) {
  if (!c || !st || !z || !phi || !E_R || !E_C) return c8_fail(C8_ERR_ARG, "c8_eval_error_contributions: null argument");
  if (!st->xi || !st->xi_prev) return c8_fail(C8_ERR_ARG, "c8_eval_error_contributions: null local state");
  for (int i = 0; i < c->nres; ++i) {  // under mechanics_plane_stress (one residual) the entries [1] are ignored
    if (!st->x[i] || !st->x_prev[i]) return c8_fail(C8_ERR_ARG, "c8_eval_error_contributions: null global state");
    if (!z[i]) return c8_fail(C8_ERR_ARG, "c8_eval_error_contributions: null adjoint solution");
  }
  if (c->model == MODEL_HYBRID_HYPER_J2_PLANE_STRESS && !c->nn_ready)
    return c8_fail(C8_ERR_ARG,
                   "c8_eval_error_contributions: the embedded network is not set (c8_set_embedded_model, c8_set_embedded_params)");
  ErrorFn const fn = error_kernel(c->mesh.elem_type, c->model);
  if (!fn) return c8_fail(C8_ERR_UNSUPPORTED, "c8_eval_error_contributions: not available for this element/model");
  MeshTables const mt{c->d_conn, c->d_coords, c->d_nodeptr, c->d_pos, c->d_elem_set, nullptr, c->d_params, nullptr, c->d_nn};
  FieldArgs const fa{st->x[0], st->x[1], st->x_prev[0], st->x_prev[1], st->xi_prev, st->xi};
  ErrorArgs const ea{z[0], c->nres == 2 ? z[1] : nullptr, phi};
  hipError_t const err = fn(mt, c->ms, fa, ea, E_R, E_C, c->mesh.nelems, c->stream);
  if (err != hipSuccess) return c8_fail(C8_ERR_DEVICE, std::string("c8_eval_error_contributions: ") + hipGetErrorString(err));
  return c->async ? C8_OK : c8_status(c);
}
