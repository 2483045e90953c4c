// c8_cauchy.hip -- c8_eval_cauchy: the Cauchy stress field at the local-state points (c8_cauchy.hpp), one lane per
// (element, point) pair.  A translation unit of its own: the instantiations of c8_kernels.hip keep their code generation.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/c8.h"
#include "c8_api_internal.hpp"
#include "c8_cauchy.hpp"
#include "c8_registry.hpp"

namespace c8 {

constexpr int CAUCHY_BLOCK = 256;

// Lane q of the launch evaluates point q % NP0 of element q / NP0: consecutive lanes take the points of one element, so the
// NP0 lanes of an element read the same connectivity row and the same nodal lines (L1), and a block's 256 results are one
// contiguous piece of sigma (256 x 72 bytes).  A lane's nine values lie 72 bytes from its neighbour's, so stored as they
// stand each of the nine store instructions of a wavefront touches 36 lines of 128 bytes with 8 bytes per lane.  Instead
// the block passes its piece through LDS and writes it out in order: 16 bytes per lane, 1 KiB contiguous per wavefront
// instruction (8 bytes per lane where the caller's sigma is not 16-byte aligned).  -DC8_TUNE_CAUCHY_DIRECT (tuning build,
// same results) stores the nine values directly; DESIGN.md has both times.
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(CAUCHY_BLOCK) k_cauchy(MeshTables mt, ModelSettings ms, FieldArgs fa, double* sigma,
                                                        long long npoints, int wide) {
  long long const q = (long long)blockIdx.x * CAUCHY_BLOCK + threadIdx.x;
  double s[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
  if (q < npoints) cauchy_point<E, ModelT>(mt, ms, fa, (int)(q / E::NP0), (int)(q % E::NP0), s);
#ifdef C8_TUNE_CAUCHY_DIRECT
  if (q < npoints) {
    C8_UNROLL
    for (int j = 0; j < 9; ++j) sigma[(size_t)q * 9 + j] = s[j];
  }
#else
  __shared__ double tile[CAUCHY_BLOCK * 9];
  int const t = threadIdx.x;
  C8_UNROLL
  for (int j = 0; j < 9; ++j) tile[t * 9 + j] = s[j];
  __syncthreads();
  size_t const base = (size_t)blockIdx.x * (CAUCHY_BLOCK * 9);  // even: as aligned as sigma itself
  size_t const total = (size_t)npoints * 9;
  if (wide) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    C8_UNROLL
    for (int k = 0; k < (CAUCHY_BLOCK * 9 / 2 + CAUCHY_BLOCK - 1) / CAUCHY_BLOCK; ++k) {
      int const i = 2 * (k * CAUCHY_BLOCK + t);
      if (i < CAUCHY_BLOCK * 9) {
        if (base + i + 1 < total) {
          d2 w;
          w.x = tile[i];
          w.y = tile[i + 1];
          *reinterpret_cast<d2*>(sigma + base + i) = w;
        } else if (base + i < total) {  // the last value of an odd number of points
          sigma[base + i] = tile[i];
        }
      }
    }
  } else {
    C8_UNROLL
    for (int k = 0; k < 9; ++k) {
      int const i = k * CAUCHY_BLOCK + t;
      if (base + i < total) sigma[base + i] = tile[i];
    }
  }
#endif
}

typedef hipError_t (*CauchyFn)(MeshTables const&, ModelSettings const&, FieldArgs const&, double* sigma, int nelems, hipStream_t);

// the grid follows from the mesh alone: one lane per point, 256 per block
template <class E, template <class> class ModelT>
static hipError_t launch_cauchy(MeshTables const& mt, ModelSettings const& ms, FieldArgs const& fa, double* sigma, int nelems,
                                hipStream_t stream) {
  long long const npoints = (long long)nelems * E::NP0;
  if (npoints <= 0) return hipSuccess;
  unsigned const grid = (unsigned)((npoints + CAUCHY_BLOCK - 1) / CAUCHY_BLOCK);
  int const wide = (reinterpret_cast<uintptr_t>(sigma) & 15) == 0;
  hipLaunchKernelGGL((k_cauchy<E, ModelT>), dim3(grid), dim3(CAUCHY_BLOCK), 0, stream, mt, ms, fa, sigma, npoints, wide);
  return hipGetLastError();
}
template <class E, template <class> class ModelT> static CauchyFn cauchy_fn(ModelTag<ModelT>) { return &launch_cauchy<E, ModelT>; }

// the row of the model table on the element class it runs on: 3-D rows on hex8 and tet4, 2-D rows on the row's tri3 class
static CauchyFn cauchy_kernel(int elem_type, int model) {
  CauchyFn fn = nullptr;
  visit_models([&](auto row) {
    using R = decltype(row);
    if (row.id != model) return;
    if constexpr (R::dim == 3) {
      if (elem_type == C8_HEX8) fn = cauchy_fn<Elem<C8_HEX8>>(row);
      if (elem_type == C8_TET4) fn = cauchy_fn<Elem<C8_TET4>>(row);
    } else {
      if (elem_type == C8_TRI3) fn = cauchy_fn<typename R::Elem2D>(row);
    }
  });
  return fn;
}

}  // namespace c8

using namespace c8;

extern "C" int c8_eval_cauchy(c8_ctx* c, const c8_state* st, double* sigma) {
  if (!c || !st || !sigma) return c8_fail(C8_ERR_ARG, "c8_eval_cauchy: null argument");
  if (!st->xi || !st->xi_prev) return c8_fail(C8_ERR_ARG, "c8_eval_cauchy: null local state");
  for (int i = 0; i < c->nres; ++i)  // under mechanics_plane_stress (one residual) the entries [1] are ignored
    if (!st->x[i] || !st->x_prev[i]) return c8_fail(C8_ERR_ARG, "c8_eval_cauchy: null global state");
  if (c->model == MODEL_HYBRID_HYPER_J2_PLANE_STRESS && !c->nn_ready)
    return c8_fail(C8_ERR_ARG, "c8_eval_cauchy: the embedded network is not set (c8_set_embedded_model, c8_set_embedded_params)");
  CauchyFn const fn = cauchy_kernel(c->mesh.elem_type, c->model);
  if (!fn) return c8_fail(C8_ERR_UNSUPPORTED, "c8_eval_cauchy: not available for this element/model");
  MeshTables const mt{c->d_conn, c->d_coords, c->d_nodeptr, c->d_pos, c->d_elem_set, nullptr, c->d_params, nullptr, c->d_nn};
  FieldArgs const fa{st->x[0], st->x[1], st->x_prev[0], st->x_prev[1], st->xi_prev, st->xi};
  hipError_t const err = fn(mt, c->ms, fa, sigma, c->mesh.nelems, c->stream);
  if (err != hipSuccess) return c8_fail(C8_ERR_DEVICE, std::string("c8_eval_cauchy: ") + hipGetErrorString(err));
  return c->async ? C8_OK : c8_status(c);
}
