// c8_spr.hip -- c8_spr_recover, c8_interpolate_to_points, c8_spr_table: superconvergent patch recovery of a point field to
// the nodes (c8_spr.hpp) and the interpolation that feeds it in the reference's perform_SPR.  A translation unit of its own.
//
// Set-up, once per context (spr_setup): k_spr_points caches the sample positions, k_spr_fit fits every node over its own
// elements (one lane per node) and flags the nodes whose patch has too few points or is rank-deficient; the host expands the
// flagged patches (spr_build_patch), refits them, and builds the patch table of all nodes.  Per call: k_spr_apply, one
// weighted sum per node and component.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/c8.h"
#include "c8_api_internal.hpp"
#include "c8_spr.hpp"

namespace c8 {

constexpr int SPR_BLOCK = 256;

template <class E>
__global__ void __launch_bounds__(SPR_BLOCK) k_spr_points(int32_t const* __restrict__ conn, double const* __restrict__ coords,
                                                          double* __restrict__ pts, long long npoints) {
  long long const q = (long long)blockIdx.x * SPR_BLOCK + threadIdx.x;
  if (q >= npoints) return;
  double x[E::DIM];
  spr_point<E>(conn, coords, (int)(q / E::NP0), (int)(q % E::NP0), x);
  C8_UNROLL
  for (int d = 0; d < E::DIM; ++d) pts[q * E::DIM + d] = x[d];
}

// one lane per node: the fit over the node's own elements (the packed lists of the staged assembly, element << 3 | slot)
template <class E>
__global__ void __launch_bounds__(SPR_BLOCK) k_spr_fit(int32_t const* __restrict__ ne_ptr, int32_t const* __restrict__ ne,
                                                       double const* __restrict__ pts, double const* __restrict__ coords,
                                                       double* __restrict__ g, double* __restrict__ h, int32_t* __restrict__ flag,
                                                       int nnodes) {
  int const n = blockIdx.x * SPR_BLOCK + threadIdx.x;
  if (n >= nnodes) return;
  constexpr int T = E::DIM + 1;
  int const b = ne_ptr[n], nel = ne_ptr[n + 1] - b;
  double gn[T], hn;
  double const ratio = spr_fit<E::DIM>(ne + b, nel, 3, E::NP0, pts, coords + (size_t)n * 3, gn, &hn);
  C8_UNROLL
  for (int i = 0; i < T; ++i) g[(size_t)n * T + i] = gn[i];
  h[n] = hn;
  flag[n] = (!spr_enough_points(E::NP0, nel, T) || !(ratio > SPR_RANK_TOL)) ? 1 : 0;
}

// The hot path.  A group of G lanes per node (G a power of two <= 64, SPR_BLOCK / G nodes per block).  Lane l of the group
// takes samples l, l + G, ... of the node's patch: sample s is point s % NP0 of element patch_elems[ptr + s / NP0], its
// weight w_s = g . terms((x_s - x_n) / h) comes from the cached positions, and the lane adds w_s v_s[c] to NC partial sums
// in registers (c < ncomp <= NC).  The group then adds its partial sums by xor shuffles, halving the distance from G / 2
// to 1: a fixed order, so two calls give the same bytes, and no atomics.  Lanes c < ncomp of the group store the node's
// values, one contiguous piece of `nodal`.  Patches with more samples than G are looped over.
template <class E, int G, int NC>
__global__ void __launch_bounds__(SPR_BLOCK) k_spr_apply(int64_t const* __restrict__ patch_ptr, int32_t const* __restrict__ patch_elems,
                                                         double const* __restrict__ g, double const* __restrict__ h,
                                                         double const* __restrict__ pts, double const* __restrict__ coords,
                                                         double const* __restrict__ field, double* __restrict__ nodal, int nnodes,
                                                         int ncomp) {
  constexpr int T = E::DIM + 1;
  int const lane = threadIdx.x % G;
  int const n = blockIdx.x * (SPR_BLOCK / G) + threadIdx.x / G;
  bool const live = n < nnodes;
  double acc[NC];
  C8_UNROLL
  for (int c = 0; c < NC; ++c) acc[c] = 0.;
  if (live) {
    int64_t const b = patch_ptr[n];
    int const ns = (int)(patch_ptr[n + 1] - b) * E::NP0;
    double gn[T], xn[E::DIM];
    C8_UNROLL
    for (int i = 0; i < T; ++i) gn[i] = g[(size_t)n * T + i];
    C8_UNROLL
    for (int d = 0; d < E::DIM; ++d) xn[d] = coords[(size_t)n * 3 + d];
    double const inv_h = 1. / h[n];
    for (int s = lane; s < ns; s += G) {
      size_t const q = (size_t)patch_elems[b + s / E::NP0] * E::NP0 + s % E::NP0;
      double t[T];
      spr_terms<E::DIM>(pts + q * E::DIM, xn, inv_h, t);
      double w = 0.;
      C8_UNROLL
      for (int i = 0; i < T; ++i) w += gn[i] * t[i];
      double const* v = field + q * ncomp;
      C8_UNROLL
      for (int c = 0; c < NC; ++c)
        if (c < ncomp) acc[c] += w * v[c];
    }
  }
  // every lane of the wavefront takes part in the shuffles (groups past the last node carry zeros)
  C8_UNROLL
  for (int off = G / 2; off >= 1; off >>= 1) {
    C8_UNROLL
    for (int c = 0; c < NC; ++c) acc[c] += __shfl_xor(acc[c], off, G);
  }
  if (live) {
    for (int c0 = lane; c0 < ncomp; c0 += G) {
      double out = 0.;
      C8_UNROLL
      for (int c = 0; c < NC; ++c) out = (c == c0) ? acc[c] : out;
      nodal[(size_t)n * ncomp + c0] = out;
    }
  }
}

// interpolate_to_cell_center of the reference, at the coupled points: one lane per (element, point)
template <class E>
__global__ void __launch_bounds__(SPR_BLOCK) k_interp_points(int32_t const* __restrict__ conn, double const* __restrict__ nodal,
                                                             double* __restrict__ ip_field, long long npoints, int ncomp) {
  long long const q = (long long)blockIdx.x * SPR_BLOCK + threadIdx.x;
  if (q >= npoints) return;
  int const e = (int)(q / E::NP0);
  double xi[3], w;
  E::point(0, (int)(q % E::NP0), xi, w);
  double N[E::NN];
  int32_t na[E::NN];
  C8_UNROLL
  for (int a = 0; a < E::NN; ++a) {
    N[a] = E::N(a, xi);
    na[a] = conn[(size_t)e * E::NN + a];
  }
  for (int c = 0; c < ncomp; ++c) {
    double s = 0.;
    C8_UNROLL
    for (int a = 0; a < E::NN; ++a) s += N[a] * nodal[(size_t)na[a] * ncomp + c];
    ip_field[(size_t)q * ncomp + c] = s;
  }
}

// group widths of k_spr_apply: 16 lanes on hex8 (64 samples round an interior node: four trips per lane), 8 lanes on tet4
// and tri3 (24 and 6 centroids round an interior node of the structured splits); measured against 4 .. 64 lanes, DESIGN.md
// section 17 has the times
// (-DC8_TUNE_SPR_GROUP_HEX=n / -DC8_TUNE_SPR_GROUP_SIMPLEX=n, powers of two up to 64: tuning builds, same sums per lane
// count, different order between counts)
#ifndef C8_TUNE_SPR_GROUP_HEX
#define C8_TUNE_SPR_GROUP_HEX 16
#endif
#ifndef C8_TUNE_SPR_GROUP_SIMPLEX
#define C8_TUNE_SPR_GROUP_SIMPLEX 8
#endif
template <class E> struct SprGroup { static constexpr int G = C8_TUNE_SPR_GROUP_SIMPLEX; };
template <> struct SprGroup<Elem<C8_HEX8>> { static constexpr int G = C8_TUNE_SPR_GROUP_HEX; };

template <class E, int NC>
static void launch_apply_nc(c8_ctx* c, int ncomp, double const* field, double* nodal) {
  constexpr int G = SprGroup<E>::G;
  int const per_block = SPR_BLOCK / G;
  unsigned const grid = (unsigned)((c->mesh.nnodes + per_block - 1) / per_block);
  hipLaunchKernelGGL((k_spr_apply<E, G, NC>), dim3(grid), dim3(SPR_BLOCK), 0, c->stream, c->spr.d_patch_ptr, c->spr.d_patch_elems,
                     c->spr.d_g, c->spr.d_h, c->spr.d_pts, c->d_coords, field, nodal, c->mesh.nnodes, ncomp);
}

// the accumulators are registers, so their number is a template argument: the smallest of 1, 4, 9, 16 that holds ncomp
template <class E> static hipError_t launch_apply(c8_ctx* c, int ncomp, double const* field, double* nodal) {
  if (ncomp <= 1) launch_apply_nc<E, 1>(c, ncomp, field, nodal);
  else if (ncomp <= 4) launch_apply_nc<E, 4>(c, ncomp, field, nodal);
  else if (ncomp <= 9) launch_apply_nc<E, 9>(c, ncomp, field, nodal);
  else launch_apply_nc<E, 16>(c, ncomp, field, nodal);
  return hipGetLastError();
}

template <class E> static hipError_t launch_interp(c8_ctx* c, int ncomp, double const* nodal, double* ip_field) {
  long long const npoints = (long long)c->mesh.nelems * E::NP0;
  unsigned const grid = (unsigned)((npoints + SPR_BLOCK - 1) / SPR_BLOCK);
  hipLaunchKernelGGL((k_interp_points<E>), dim3(grid), dim3(SPR_BLOCK), 0, c->stream, c->d_conn, nodal, ip_field, npoints, ncomp);
  return hipGetLastError();
}

template <class E> static hipError_t launch_setup(c8_ctx* c, int32_t* d_flag) {
  long long const npoints = (long long)c->mesh.nelems * E::NP0;
  unsigned const grid = (unsigned)((npoints + SPR_BLOCK - 1) / SPR_BLOCK);
  hipLaunchKernelGGL((k_spr_points<E>), dim3(grid), dim3(SPR_BLOCK), 0, c->stream, c->d_conn, c->d_coords, c->spr.d_pts, npoints);
  unsigned const ngrid = (unsigned)((c->mesh.nnodes + SPR_BLOCK - 1) / SPR_BLOCK);
  hipLaunchKernelGGL((k_spr_fit<E>), dim3(ngrid), dim3(SPR_BLOCK), 0, c->stream, c->d_nodeelem_ptr, c->d_nodeelem, c->spr.d_pts,
                     c->d_coords, c->spr.d_g, c->spr.d_h, d_flag, c->mesh.nnodes);
  return hipGetLastError();
}

}  // namespace c8

using namespace c8;

#define SPR_HIP(call)                                                                                                 \
  do {                                                                                                                \
    hipError_t err__ = (call);                                                                                        \
    if (err__ != hipSuccess) return c8_fail(C8_ERR_DEVICE, std::string("c8_spr: " #call ": ") + hipGetErrorString(err__)); \
  } while (0)

void c8_spr_release(c8_ctx* c) {
  void* bufs[] = {c->spr.d_pts, c->spr.d_g, c->spr.d_h, c->spr.d_patch_ptr, c->spr.d_patch_elems};
  for (void* b : bufs) (void)hipFree(b);
  c->spr = c8_spr_tables();
}

// the tables of the context, built at the first use and kept
static int spr_setup(c8_ctx* c) {
  c8_spr_tables& t = c->spr;
  if (t.built) return C8_OK;
  int const et = c->mesh.elem_type, nnodes = c->mesh.nnodes, nelems = c->mesh.nelems;
  int const dim = spr_dim(et), np0 = spr_np0(et), T = dim + 1;
  size_t const npts = (size_t)nelems * np0 * dim;
  int32_t* d_flag = nullptr;
  auto fail_with = [&](int rc) {
    (void)hipFree(d_flag);
    c8_spr_release(c);
    return rc;
  };
  auto const t0 = std::chrono::steady_clock::now();
  if (hipMalloc((void**)&t.d_pts, npts * sizeof(double)) != hipSuccess || hipMalloc((void**)&t.d_g, (size_t)nnodes * T * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&t.d_h, (size_t)nnodes * sizeof(double)) != hipSuccess || hipMalloc((void**)&d_flag, (size_t)nnodes * sizeof(int32_t)) != hipSuccess)
    return fail_with(c8_fail(C8_ERR_DEVICE, "c8_spr: cannot allocate the recovery tables"));
  hipError_t err = et == C8_HEX8 ? launch_setup<Elem<C8_HEX8>>(c, d_flag) : (et == C8_TET4 ? launch_setup<Elem<C8_TET4>>(c, d_flag) : launch_setup<Elem<C8_TRI3>>(c, d_flag));
  std::vector<int32_t> flag((size_t)nnodes);
  t.g.resize((size_t)nnodes * T);
  t.h.resize((size_t)nnodes);
  if (err == hipSuccess) err = hipMemcpyAsync(flag.data(), d_flag, flag.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
  if (err == hipSuccess) err = hipMemcpyAsync(t.g.data(), t.d_g, t.g.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (err == hipSuccess) err = hipMemcpyAsync(t.h.data(), t.d_h, t.h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
  if (err != hipSuccess) return fail_with(c8_fail(C8_ERR_DEVICE, std::string("c8_spr: set-up kernels: ") + hipGetErrorString(err)));
  auto const t1 = std::chrono::steady_clock::now();
  // host step: the flagged nodes only
  size_t nflag = 0;
  for (int32_t f : flag) nflag += f != 0;
  t.stages.assign((size_t)nnodes, 0);
  std::vector<std::vector<int32_t>> grown;  // patches of the flagged nodes, in node order
  if (nflag) {
    std::vector<double> pts(npts);
    if (hipMemcpyAsync(pts.data(), t.d_pts, npts * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      return fail_with(c8_fail(C8_ERR_DEVICE, "c8_spr: cannot read the sample positions back"));
    SprMesh const m{et, nnodes, nelems, c->mesh.coords.data(), c->mesh.conn.data(), c->graph.nodeelem_ptr.data(), c->graph.nodeelem.data(), 3, pts.data()};
    grown.reserve(nflag);
    for (int n = 0; n < nnodes; ++n) {
      if (!flag[n]) continue;
      grown.emplace_back();
      double gn[4] = {0., 0., 0., 0.}, hn = 1.;
      int st = 0;
      if (!spr_build_patch(m, n, grown.back(), gn, &hn, &st))
        return fail_with(c8_fail(C8_ERR_ARG, "c8_spr: the patch of node " + std::to_string(n) +
                                                 " cannot be completed: it stopped growing without enough points of full rank (all hope is lost)"));
      for (int i = 0; i < T; ++i) t.g[(size_t)n * T + i] = gn[i];
      t.h[n] = hn;
      t.stages[n] = st;
    }
  }
  // the table of all nodes: an unflagged node's list is its node -> element list
  t.patch_ptr.assign((size_t)nnodes + 1, 0);
  {
    size_t k = 0;
    for (int n = 0; n < nnodes; ++n)
      t.patch_ptr[n + 1] = t.patch_ptr[n] + (flag[n] ? (int64_t)grown[k++].size() : (int64_t)(c->graph.nodeelem_ptr[n + 1] - c->graph.nodeelem_ptr[n]));
    t.patch_elems.resize((size_t)t.patch_ptr[nnodes]);
    k = 0;
    for (int n = 0; n < nnodes; ++n) {
      int32_t* out = t.patch_elems.data() + t.patch_ptr[n];
      if (flag[n]) {
        std::vector<int32_t> const& p = grown[k++];
        std::copy(p.begin(), p.end(), out);
      } else {
        for (int32_t q = c->graph.nodeelem_ptr[n]; q < c->graph.nodeelem_ptr[n + 1]; ++q) *out++ = c->graph.nodeelem[q] >> 3;
      }
    }
  }
  auto const t2 = std::chrono::steady_clock::now();
  (void)hipFree(d_flag);
  d_flag = nullptr;
  if (hipMalloc((void**)&t.d_patch_ptr, t.patch_ptr.size() * sizeof(int64_t)) != hipSuccess ||
      hipMalloc((void**)&t.d_patch_elems, std::max<size_t>(t.patch_elems.size(), 1) * sizeof(int32_t)) != hipSuccess)
    return fail_with(c8_fail(C8_ERR_DEVICE, "c8_spr: cannot allocate the patch table"));
  err = hipMemcpyAsync(t.d_patch_ptr, t.patch_ptr.data(), t.patch_ptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream);
  if (err == hipSuccess) err = hipMemcpyAsync(t.d_patch_elems, t.patch_elems.data(), t.patch_elems.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
  if (err == hipSuccess && nflag) err = hipMemcpyAsync(t.d_g, t.g.data(), t.g.size() * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (err == hipSuccess && nflag) err = hipMemcpyAsync(t.d_h, t.h.data(), t.h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
  if (err != hipSuccess) return fail_with(c8_fail(C8_ERR_DEVICE, std::string("c8_spr: table upload: ") + hipGetErrorString(err)));
  auto const t3 = std::chrono::steady_clock::now();
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  t.info[0] = ms(t0, t1);        // device: positions, fit, read-back
  t.info[1] = ms(t1, t2);        // host: expansion of the flagged nodes and the table
  t.info[2] = ms(t2, t3);        // upload
  t.info[3] = (double)nflag;     // flagged nodes
  t.built = true;
  return C8_OK;
}

static int spr_refuse_halo(c8_ctx* c, char const* who) {
  if (c->halo) return c8_fail(C8_ERR_UNSUPPORTED, std::string(who) + ": not available with a halo attached (patches cross part boundaries)");
  return C8_OK;
}

extern "C" int c8_spr_recover(c8_ctx* c, int ncomp, const double* ip_field, double* nodal) {
  if (!c || !ip_field || !nodal) return c8_fail(C8_ERR_ARG, "c8_spr_recover: null argument");
  if (ncomp < 1 || ncomp > SPR_MAX_COMP) return c8_fail(C8_ERR_ARG, "c8_spr_recover: ncomp must be between 1 and 16");
  int rc = spr_refuse_halo(c, "c8_spr_recover");
  if (rc != C8_OK || (rc = spr_setup(c)) != C8_OK) return rc;
  int const et = c->mesh.elem_type;
  hipError_t const err = et == C8_HEX8 ? launch_apply<Elem<C8_HEX8>>(c, ncomp, ip_field, nodal)
                                       : (et == C8_TET4 ? launch_apply<Elem<C8_TET4>>(c, ncomp, ip_field, nodal) : launch_apply<Elem<C8_TRI3>>(c, ncomp, ip_field, nodal));
  if (err != hipSuccess) return c8_fail(C8_ERR_DEVICE, std::string("c8_spr_recover: ") + hipGetErrorString(err));
  return c->async ? C8_OK : c8_status(c);
}

extern "C" int c8_interpolate_to_points(c8_ctx* c, int ncomp, const double* nodal, double* ip_field) {
  if (!c || !ip_field || !nodal) return c8_fail(C8_ERR_ARG, "c8_interpolate_to_points: null argument");
  if (ncomp < 1 || ncomp > SPR_MAX_COMP) return c8_fail(C8_ERR_ARG, "c8_interpolate_to_points: ncomp must be between 1 and 16");
  int const et = c->mesh.elem_type;
  hipError_t const err = et == C8_HEX8 ? launch_interp<Elem<C8_HEX8>>(c, ncomp, nodal, ip_field)
                                       : (et == C8_TET4 ? launch_interp<Elem<C8_TET4>>(c, ncomp, nodal, ip_field) : launch_interp<Elem<C8_TRI3>>(c, ncomp, nodal, ip_field));
  if (err != hipSuccess) return c8_fail(C8_ERR_DEVICE, std::string("c8_interpolate_to_points: ") + hipGetErrorString(err));
  return c->async ? C8_OK : c8_status(c);
}

extern "C" int c8_spr_table(c8_ctx* c, int which, int64_t* n, const void** data) {
  if (!c || !n || !data) return c8_fail(C8_ERR_ARG, "c8_spr_table: null argument");
  if (which < 0 || which > 5) return c8_fail(C8_ERR_ARG, "c8_spr_table: which must be 0..5");
  int rc = spr_refuse_halo(c, "c8_spr_table");
  if (rc != C8_OK || (rc = spr_setup(c)) != C8_OK) return rc;
  c8_spr_tables const& t = c->spr;
  switch (which) {
    case 0: *n = (int64_t)t.patch_ptr.size(); *data = t.patch_ptr.data(); break;
    case 1: *n = (int64_t)t.patch_elems.size(); *data = t.patch_elems.data(); break;
    case 2: *n = (int64_t)t.g.size(); *data = t.g.data(); break;
    case 3: *n = (int64_t)t.h.size(); *data = t.h.data(); break;
    case 4: *n = (int64_t)t.stages.size(); *data = t.stages.data(); break;
    default: *n = 4; *data = t.info; break;
  }
  return C8_OK;
}
