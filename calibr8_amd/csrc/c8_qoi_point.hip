// c8_qoi_point.hip -- the subdomain objectives (c8_set_qoi_subdomain; c8_qoi_point.hpp) beside the adjoint kernels, which
// run with a zero objective under them: the value (what K6 would add), g -= dJ/dxi before K3, b -= dJ/dx after K3 and
// grad += dJ/dp with K5.  A translation unit of its own: the instantiations of c8_kernels.hip keep their code generation.
//
// Lanes.  The value, the pre-pass and the gradient kernel: lane q of the launch is point q % NP0 of element q / NP0, as in
// c8_cauchy.hip.  The post-pass: one lane per node.
// Summation orders (every output is bitwise repeatable):
//   J, grad   the 256 values of a block by a fixed tree in LDS -> part[block]; then one block sums the partials, thread t
//             the blocks t, t + 256, ... ascending, then the same tree (the scheme of c8_vfm.hip)
//   g         one lane per entry: no sum
//   b         per node over the node's elements ascending (the node -> element lists of the staged assembly), the points of
//             an element ascending; one subtraction from b per entry.  No atomics.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/c8.h"
#include "c8_api_internal.hpp"
#include "c8_qoi_point.hpp"
#include "c8_registry.hpp"

namespace c8 {

constexpr int QP_BLOCK = 256;
constexpr int QP_MAX_ACTIVE = 8;  // c8_set_active_params

struct ActiveSet {
  int n;                   // active parameters of the chosen element set
  int idx[QP_MAX_ACTIVE];  // their indices
};

// the block's sum of v in a fixed order; valid in thread 0
__device__ double block_sum(double v, double* s) {
  int const t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int w = QP_BLOCK / 2; w > 0; w >>= 1) {
    if (t < w) s[t] += s[t + w];
    __syncthreads();
  }
  double const r = s[0];
  __syncthreads();
  return r;
}

// out[o] += sum_b part[o][b], o < nout
__global__ void __launch_bounds__(QP_BLOCK) k_qoi_reduce(double const* part, int nblocks, int nout, double* out) {
  __shared__ double s[QP_BLOCK];
  for (int o = 0; o < nout; ++o) {
    double a = 0.;
    for (int b = threadIdx.x; b < nblocks; b += QP_BLOCK) a += part[(size_t)o * nblocks + b];
    double const r = block_sum(a, s);
    if (threadIdx.x == 0) out[o] += r;
  }
}

template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(QP_BLOCK) k_qoi_value(MeshTables mt, FieldArgs fa, SubdomainQoi sq, long long npoints, double* part) {
  __shared__ double s[QP_BLOCK];
  long long const q = (long long)blockIdx.x * QP_BLOCK + threadIdx.x;
  double v = 0.;
  if (q < npoints && qoi_in_set(mt, sq, (int)(q / E::NP0))) {
    QoiPoint<ModelT> d;
    qoi_point_load<E, ModelT>(mt, fa, (int)(q / E::NP0), (int)(q % E::NP0), d);
    v = qoi_point_value<E, ModelT>(mt, sq, d);
  }
  double const r = block_sum(v, s);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// the pre-pass: rec[q][QOI_REC] = the x-record of point q, g[q][j] -= dJ/dxi_j.  Points of other element sets: untouched.
// The tangents are taken one after the other in loops that stay loops: one copy of the model's dev_cauchy per kernel.
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(QP_BLOCK) k_qoi_pre(MeshTables mt, FieldArgs fa, SubdomainQoi sq, long long npoints, double* rec, double* g) {
  constexpr int NL = ModelT<double>::NLOC;
  long long const q = (long long)blockIdx.x * QP_BLOCK + threadIdx.x;
  if (q >= npoints || !qoi_in_set(mt, sq, (int)(q / E::NP0))) return;
  QoiPoint<ModelT> d;
  qoi_point_load<E, ModelT>(mt, fa, (int)(q / E::NP0), (int)(q % E::NP0), d);
  if (sq.kind != C8_QOI_AVG_LOCAL_VAR) {
#pragma clang loop unroll(disable)
    for (int t = 0; t < QOI_REC; ++t) rec[(size_t)q * QOI_REC + t] = qoi_point_dx<E, ModelT>(mt, sq, d, t);
  }
  if (sq.kind != C8_QOI_DISP_COMP) {
#pragma clang loop unroll(disable)
    for (int j = 0; j < NL; ++j) g[(size_t)q * NL + j] -= qoi_point_dxi<E, ModelT>(mt, sq, d, j);
  }
}

// part[k][block] = the block's sum of dq/d(param act.idx[k])
template <class E, template <class> class ModelT>
__global__ void __launch_bounds__(QP_BLOCK) k_qoi_grad(MeshTables mt, FieldArgs fa, SubdomainQoi sq, ActiveSet act, long long npoints, double* part) {
  __shared__ double s[QP_BLOCK];
  long long const q = (long long)blockIdx.x * QP_BLOCK + threadIdx.x;
  bool const mine = q < npoints && qoi_in_set(mt, sq, (int)(q / E::NP0));
  QoiPoint<ModelT> d;
  if (mine) qoi_point_load<E, ModelT>(mt, fa, (int)(q / E::NP0), (int)(q % E::NP0), d);
#pragma clang loop unroll(disable)
  for (int k = 0; k < act.n; ++k) {
    double const r = block_sum(mine ? qoi_point_dparam<E, ModelT>(mt, sq, d, act.idx[k]) : 0., s);
    if (threadIdx.x == 0) part[(size_t)k * gridDim.x + blockIdx.x] = r;
  }
}

// the post-pass: b0[n][i] -= sum over the elements of node n in the set, and their points, of the record contracted with
// N_n and grad N_n; b1[n] the same with the pressure entry (two residuals).  A node with no element in the set: untouched.
template <class E>
__global__ void __launch_bounds__(QP_BLOCK) k_qoi_post(MeshTables mt, int32_t const* nodeelem_ptr, int32_t const* nodeelem, SubdomainQoi sq,
                                                      double const* rec, int nnodes, double* b0, double* b1) {
  int const n = blockIdx.x * QP_BLOCK + threadIdx.x;
  if (n >= nnodes) return;
  double su[3] = {0., 0., 0.}, sp = 0.;
  bool any = false;
  for (int k = nodeelem_ptr[n]; k < nodeelem_ptr[n + 1]; ++k) {
    int const e = nodeelem[k] >> 3, a = nodeelem[k] & 7;
    if (!qoi_in_set(mt, sq, e)) continue;
    any = true;
    NodeAtPoint<E> sh;
    C8_UNROLL
    for (int m = 0; m < E::NN; ++m) {
      size_t const node = (size_t)mt.conn[(size_t)e * E::NN + m];
      C8_UNROLL
      for (int i = 0; i < 3; ++i) sh.X[m][i] = (i < E::DIM) ? mt.coords[node * 3 + i] : 0.;
    }
    for (int pt = 0; pt < E::NP0; ++pt) {
      double r[QOI_REC], du[3], dp;
      C8_UNROLL
      for (int t = 0; t < QOI_REC; ++t) r[t] = rec[((size_t)e * E::NP0 + pt) * QOI_REC + t];
      qoi_node_contract<E>(sh, pt, a, r, du, dp);
      su[0] += du[0]; su[1] += du[1]; su[2] += du[2];
      sp += dp;
    }
  }
  if (!any) return;
  C8_UNROLL
  for (int i = 0; i < E::DIM; ++i) b0[(size_t)n * E::DIM + i] -= su[i];
  if (E::NRES == 2) b1[n] -= sp;
}

struct SubQoiFns {
  hipError_t (*value)(MeshTables const&, FieldArgs const&, SubdomainQoi const&, int nelems, double* part, hipStream_t);
  hipError_t (*pre)(MeshTables const&, FieldArgs const&, SubdomainQoi const&, int nelems, double* rec, double* g, hipStream_t);
  hipError_t (*grad)(MeshTables const&, FieldArgs const&, SubdomainQoi const&, ActiveSet const&, int nelems, double* part, hipStream_t);
  hipError_t (*post)(MeshTables const&, int32_t const*, int32_t const*, SubdomainQoi const&, double const* rec, int nnodes, double* b0,
                     double* b1, hipStream_t);
  int np0;
};

// the grids follow from the mesh alone: one lane per point (per node), 256 per block
static unsigned blocks_of(long long n) { return (unsigned)((n + QP_BLOCK - 1) / QP_BLOCK); }

template <class E, template <class> class ModelT>
static hipError_t launch_value(MeshTables const& mt, FieldArgs const& fa, SubdomainQoi const& sq, int nelems, double* part, hipStream_t s) {
  long long const np = (long long)nelems * E::NP0;
  hipLaunchKernelGGL((k_qoi_value<E, ModelT>), dim3(blocks_of(np)), dim3(QP_BLOCK), 0, s, mt, fa, sq, np, part);
  return hipGetLastError();
}
template <class E, template <class> class ModelT>
static hipError_t launch_pre(MeshTables const& mt, FieldArgs const& fa, SubdomainQoi const& sq, int nelems, double* rec, double* g, hipStream_t s) {
  long long const np = (long long)nelems * E::NP0;
  hipLaunchKernelGGL((k_qoi_pre<E, ModelT>), dim3(blocks_of(np)), dim3(QP_BLOCK), 0, s, mt, fa, sq, np, rec, g);
  return hipGetLastError();
}
template <class E, template <class> class ModelT>
static hipError_t launch_grad(MeshTables const& mt, FieldArgs const& fa, SubdomainQoi const& sq, ActiveSet const& act, int nelems, double* part,
                              hipStream_t s) {
  long long const np = (long long)nelems * E::NP0;
  hipLaunchKernelGGL((k_qoi_grad<E, ModelT>), dim3(blocks_of(np)), dim3(QP_BLOCK), 0, s, mt, fa, sq, act, np, part);
  return hipGetLastError();
}
template <class E>
static hipError_t launch_post(MeshTables const& mt, int32_t const* nodeelem_ptr, int32_t const* nodeelem, SubdomainQoi const& sq, double const* rec,
                              int nnodes, double* b0, double* b1, hipStream_t s) {
  hipLaunchKernelGGL((k_qoi_post<E>), dim3(blocks_of(nnodes)), dim3(QP_BLOCK), 0, s, mt, nodeelem_ptr, nodeelem, sq, rec, nnodes, b0, b1);
  return hipGetLastError();
}
template <class E, template <class> class ModelT> static SubQoiFns fns_of(ModelTag<ModelT>) {
  return SubQoiFns{&launch_value<E, ModelT>, &launch_pre<E, ModelT>, &launch_grad<E, ModelT>, &launch_post<E>, E::NP0};
}

// the row of the model table on the element class it runs on: 3-D rows on hex8 and tet4, 2-D rows on the row's tri3 class
static SubQoiFns subqoi_kernels(int elem_type, int model) {
  SubQoiFns fn{};
  visit_models([&](auto row) {
    using R = decltype(row);
    if (row.id != model) return;
    if constexpr (R::dim == 3) {
      if (elem_type == C8_HEX8) fn = fns_of<Elem<C8_HEX8>>(row);
      if (elem_type == C8_TET4) fn = fns_of<Elem<C8_TET4>>(row);
    } else {
      if (elem_type == C8_TRI3) fn = fns_of<typename R::Elem2D>(row);
    }
  });
  return fn;
}

}  // namespace c8

using namespace c8;

#define QP(call)                                                                                   \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) return c8_fail(C8_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

static MeshTables sub_tables(c8_ctx const* c) {
  return MeshTables{c->d_conn, c->d_coords, c->d_nodeptr, c->d_pos, c->d_elem_set, nullptr, c->d_params, nullptr, c->d_nn};
}
static SubdomainQoi sub_desc(c8_ctx const* c) { return SubdomainQoi{c->sub_kind, c->sub_set, c->sub_index}; }

static int sub_ready(c8_ctx* c, SubQoiFns& fn, char const* what) {
  fn = subqoi_kernels(c->mesh.elem_type, c->model);
  if (!fn.value) return c8_fail(C8_ERR_UNSUPPORTED, std::string(what) + ": subdomain objective: not available for this element/model");
  if (c->model == MODEL_HYBRID_HYPER_J2_PLANE_STRESS && !c->nn_ready)
    return c8_fail(C8_ERR_ARG, std::string(what) + ": the embedded network is not set (c8_set_embedded_model, c8_set_embedded_params)");
  return C8_OK;
}

// out[0 .. nout) += the sums of part[nout][nblocks]
static int sub_reduce(c8_ctx* c, int nblocks, int nout, double* out) {
  hipLaunchKernelGGL(k_qoi_reduce, dim3(1), dim3(QP_BLOCK), 0, c->stream, c->d_qoi_part, nblocks, nout, out);
  QP(hipGetLastError());
  return C8_OK;
}

// ---- used by c8_api.hip ----------------------------------------------------------------------------------------------
// *J += the value of the step
int c8_subqoi_value(c8_ctx* c, FieldArgs const& fa, double* J) {
  SubQoiFns fn;
  int const rc = sub_ready(c, fn, "c8_eval_qoi");
  if (rc) return rc;
  QP(fn.value(sub_tables(c), fa, sub_desc(c), c->mesh.nelems, c->d_qoi_part, c->stream));
  return sub_reduce(c, (int)blocks_of((long long)c->mesh.nelems * fn.np0), 1, J);
}

// before K3: g -= dJ/dxi, and the x-records of the points for c8_subqoi_post
int c8_subqoi_pre(c8_ctx* c, FieldArgs const& fa, double* g) {
  SubQoiFns fn;
  int const rc = sub_ready(c, fn, "c8_assemble_adjoint_jacobian");
  if (rc) return rc;
  QP(fn.pre(sub_tables(c), fa, sub_desc(c), c->mesh.nelems, c->d_qoi_rec, g, c->stream));
  return C8_OK;
}

// after K3: b -= dJ/dx (b1 is not read under one residual).  The local-variable objective does not depend on x.
int c8_subqoi_post(c8_ctx* c, double* b0, double* b1) {
  if (c->sub_kind == C8_QOI_AVG_LOCAL_VAR) return C8_OK;
  SubQoiFns fn;
  int const rc = sub_ready(c, fn, "c8_assemble_adjoint_jacobian");
  if (rc) return rc;
  QP(fn.post(sub_tables(c), c->d_nodeelem_ptr, c->d_nodeelem, sub_desc(c), c->d_qoi_rec, c->mesh.nnodes, b0, b1, c->stream));
  return C8_OK;
}

// with K5: grad[slot] += dJ/dp for the active parameters of the chosen element set, in K5's slot layout (the sets'
// active parameters one after the other).  Only the stress objective depends on the parameters.
int c8_subqoi_grad(c8_ctx* c, FieldArgs const& fa, double* grad) {
  if (c->sub_kind != C8_QOI_AVG_STRESS) return C8_OK;
  ActiveSet act{};
  int ofs = 0;
  for (int es = 0; es < c->sub_set; ++es) ofs += (int)c->active[es].size();
  act.n = (int)c->active[c->sub_set].size();  // <= 8 (c8_set_active_params)
  if (act.n == 0) return C8_OK;
  for (int k = 0; k < act.n; ++k) act.idx[k] = c->active[c->sub_set][k];
  SubQoiFns fn;
  int const rc = sub_ready(c, fn, "c8_param_gradient");
  if (rc) return rc;
  QP(fn.grad(sub_tables(c), fa, sub_desc(c), act, c->mesh.nelems, c->d_qoi_part, c->stream));
  return sub_reduce(c, (int)blocks_of((long long)c->mesh.nelems * fn.np0), act.n, grad + ofs);
}

extern "C" int c8_set_qoi_subdomain(c8_ctx* c, const c8_subdomain_qoi_desc* d) {
  if (!c || !d) return c8_fail(C8_ERR_ARG, "c8_set_qoi_subdomain: null argument");
  if (d->kind != C8_QOI_AVG_STRESS && d->kind != C8_QOI_AVG_LOCAL_VAR && d->kind != C8_QOI_DISP_COMP)
    return c8_fail(C8_ERR_ARG, "c8_set_qoi_subdomain: unknown kind");
  if (d->elem_set < 0 || d->elem_set >= c->mesh.nsets) return c8_fail(C8_ERR_ARG, "c8_set_qoi_subdomain: element set out of range");
  bool has_local = true;
  visit_models([&](auto row) { if (row.id == c->model && row.dim == c->ndims) has_local = decltype(row)::Real::HAS_LOCAL; });
  if (d->kind == C8_QOI_AVG_LOCAL_VAR) {
    if (!has_local) return c8_fail(C8_ERR_UNSUPPORTED, "c8_set_qoi_subdomain: C8_QOI_AVG_LOCAL_VAR needs a model with local state");
    if (d->index < 0 || d->index >= c->nloc) return c8_fail(C8_ERR_ARG, "c8_set_qoi_subdomain: local dof out of range");
  }
  if (d->kind == C8_QOI_DISP_COMP && (d->index < 0 || d->index >= c->ndims))
    return c8_fail(C8_ERR_ARG, "c8_set_qoi_subdomain: displacement component out of range");
  SubQoiFns const fn = subqoi_kernels(c->mesh.elem_type, c->model);
  if (!fn.value) return c8_fail(C8_ERR_UNSUPPORTED, "c8_set_qoi_subdomain: not available for this element/model");
  // the x-records of the points and the per-block partial sums (one row per active parameter of a set)
  size_t const npoints = (size_t)c->mesh.nelems * fn.np0;
  size_t const npart = (size_t)QP_MAX_ACTIVE * blocks_of((long long)npoints);
  if (!c->d_qoi_rec) QP(hipMalloc((void**)&c->d_qoi_rec, npoints * QOI_REC * sizeof(double)));
  if (!c->d_qoi_part) QP(hipMalloc((void**)&c->d_qoi_part, npart * sizeof(double)));
  c->sub_kind = d->kind;
  c->sub_set = d->elem_set;
  c->sub_index = d->kind == C8_QOI_AVG_STRESS ? 0 : d->index;
  c->qoi_kind = 2;
  return C8_OK;
}
