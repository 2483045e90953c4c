// c8_krylov.hip -- the device-resident linear solve of the step drivers (c8_krylov_solve in include/c8.h):
// right-preconditioned BiCGStab on the four-block system as the drivers hold it, preconditioned with the inverse of
// every node's own diagonal block (node-block Jacobi).  DESIGN.md section 13.
//
//   vectors   one flat array per vector: the u segment [nnodes * ND], then the p segment [nnodes] (two residuals); the
//             matrix stays in its four CSR value arrays (layout of DESIGN.md section 3.2), nothing is re-interleaved
//   residual  r = b - A x at the start, at every restart and on exit comes from k_true_residual (plain CSR order, see there)
//   kernels   per iteration: k_prec (p update + M^-1 p) -> k_spmv (v = A phat, partials of rhat.v) -> k_reduce (alpha)
//             -> k_prec (s = r - alpha v, M^-1 s) -> k_spmv (t = A shat, partials of t.s, t.t) -> k_reduce (omega)
//             -> k_update (x, r, partials of rhat.r, r.r) -> k_reduce (rho, beta, |r|^2, stop flag, iteration count)
//   scalars   alpha, omega, beta, rho live in device memory (KryScalars) and are read from there by the next kernel; the
//             host copies the struct back every `check_every` iterations only
//   sums      per-block partials in a fixed order, then one block adds the partials in a fixed order (the pattern of
//             k_vfm_reduce): no floating-point atomics, a solve is a pure function of its inputs
//   stop      once the recursive residual meets the tolerance (stop = 1) or a breakdown is seen (stop = 2) every later
//             kernel of the batch returns at once: x and the iteration count stay those of that iteration
//
// With c8_krylov_set_preconditioner(C8_PRECOND_BLOCK_SGS) the two k_prec launches become k_vec (the vector update alone,
// out = 0) followed by the multicolour Gauss-Seidel sweeps of k_sgs_color, one launch per colour;
// every other launch of the iteration is the same.  With the four aggregation kinds the sweeps start from a coarse
// correction x = P_0 M_1^-1 P_0^T rhs instead of 0, over a list of aggregated levels of which the last is solved densely
// (DESIGN.md sections 13d to 13h); the set-up of a solve forms every level's matrix and the dense inverse.  One code path
// per error discipline serves them:
//   c8_krylov_coarse.hpp        aggregation, P, the kernels between level 0 and level 1, the dense last level
//   c8_krylov_multilevel.hpp    the block levels and the cycle; levels_setup / levels_apply of one part.
//                               C8_PRECOND_TWO_LEVEL is a list of one level (k_restrict, k_coarse_apply, k_prolong),
//                               C8_PRECOND_MULTILEVEL a list built by further aggregation
//   c8_krylov_parts_levels.hpp  parts_levels_setup / parts_levels_apply over parts: part-local aggregates, level 1 and below
//                               replicated on every rank, two more all-reduces per apply.  C8_PRECOND_TWO_LEVEL_PARTS and
//                               C8_PRECOND_MULTILEVEL_PARTS; without a halo they are the kinds of one part
//
// Over the parts of a multi-part mesh (c8_krylov_solve_parts, second half of this file) the iteration is the same up to
// the order of the sums.  Vectors keep the layout above with nnodes = the part's LOCAL count, so that ghost and phantom
// entries are addressable and the halo's import tables apply to {v, v + nnodes * ND}; every kernel runs over the OWNED
// nodes only.  A x: start the import of phat (shat), multiply the owned rows that have only owned columns (the interior
// list), finish the import, multiply the other owned rows (the boundary list).  An inner product: per-block partials in
// fixed slots (interior blocks, then boundary blocks) -> k_sums (one block, the local sums) -> one all-reduce of the 1-2
// doubles over the communicator -> k_scalars (alpha / omega / rho, beta, |r|^2, stop flag from the GLOBAL sums, in device
// memory).  THREE ALL-REDUCES AND TWO IMPORTS PER ITERATION.  Every scalar and the stop flag derive from all-reduced
// values only; at every host read the ranks all-reduce (iterations, stop flag, failure marker) and leave together.
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/c8.h"
#include "c8_api_internal.hpp"

static int fail(int code, std::string const& msg) { return c8_fail(code, msg); }
#define C8_HIP(call)                                                                               \
  do {                                                                                             \
    hipError_t err__ = (call);                                                                     \
    if (err__ != hipSuccess) return fail(C8_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(err__)); \
  } while (0)

namespace {

constexpr int TPB = 256;
constexpr int UPDATE_MAX_BLOCKS = 2048;  // grid of the elementwise kernel (grid-stride beyond)
constexpr double BREAKDOWN = 1e-300;

struct KryScalars {
  double rho, alpha, omega, beta, rr;
  int32_t stop;      // 0 running, 1 recursive residual within tolerance, 2 breakdown
  int32_t iters;     // completed iterations
  int32_t bad_node;  // set-up kernel: smallest node whose diagonal block cannot be inverted (INT_MAX: none)
  int32_t pad;
};

struct Blocks {
  double const *A00, *A01, *A10, *A11;
};

// the dispatcher deals workgroups round-robin over the 8 XCDs: XCD x takes the x-th contiguous eighth of the node order
// in every kernel that walks the nodes, so that a node's rows, its inverse block and its neighbours' vector entries meet
// in one L2 from kernel to kernel
__device__ __forceinline__ int xcd_block(int b, int nblocks) {
  int const chunk = (nblocks + 7) >> 3;
  return (b & 7) * chunk + (b >> 3);
}
inline int xcd_grid(int nblocks) { return ((nblocks + 7) / 8) * 8; }

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.79769313486231570e308; }  // false for NaN

// sum of a over the block in a fixed order (shuffle tree per wavefront, then the wavefronts in order); valid in thread 0
__device__ __forceinline__ double block_sum(double a, double* sm) {
  for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
  __syncthreads();  // sm may still be read from a previous call
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
  __syncthreads();
  double tot = 0.;
  if (threadIdx.x == 0)
    for (int w = 0; w < TPB / 64; ++w) tot += sm[w];
  return tot;
}

// ---- node-block Jacobi set-up: one work item per node gathers the node's own NB x NB block out of the four value
// arrays (node's own position ks in its graph row) and inverts it by Gauss-Jordan with partial pivoting.  Every index
// below is a compile-time constant after unrolling (row swaps are selects): the block stays in registers.
template <int ND, int NRES>
__global__ void __launch_bounds__(TPB) k_setup(int nn, int nblocks, int32_t const* __restrict__ nodeptr, int32_t const* __restrict__ nodeadj,
                                               Blocks A, double* __restrict__ minv, KryScalars* S) {
  constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const node = lb * TPB + threadIdx.x;
  if (node >= nn) return;
  int64_t const np = nodeptr[node];
  int const deg = (int)(nodeptr[node + 1] - np);
  int ks = -1;
  for (int k = 0; k < deg; ++k)
    if (nodeadj[np + k] == node) ks = k;
  double a[NB][NB], inv[NB][NB];
  bool ok = ks >= 0;
  if (ks < 0) ks = 0;
#pragma unroll
  for (int ri = 0; ri < NB; ++ri)
#pragma unroll
    for (int cj = 0; cj < NB; ++cj) {
      int const i = ri < ND ? 0 : 1, eq = ri < ND ? ri : 0, j = cj < ND ? 0 : 1, e = cj < ND ? cj : 0;
      int const ni = i ? 1 : ND, nj = j ? 1 : ND;
      double const* vals = i ? (j ? A.A11 : A.A10) : (j ? A.A01 : A.A00);
      a[ri][cj] = deg > 0 ? vals[np * ni * nj + (int64_t)eq * deg * nj + (int64_t)ks * nj + e] : 0.;
      inv[ri][cj] = ri == cj ? 1. : 0.;
    }
#pragma unroll
  for (int c = 0; c < NB; ++c) {
#pragma unroll
    for (int r = c + 1; r < NB; ++r) {  // after these selects row c holds the largest |entry| of column c
      bool const sw = fabs(a[r][c]) > fabs(a[c][c]);
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        double const a0 = a[c][k], a1 = a[r][k], i0 = inv[c][k], i1 = inv[r][k];
        a[c][k] = sw ? a1 : a0;
        a[r][k] = sw ? a0 : a1;
        inv[c][k] = sw ? i1 : i0;
        inv[r][k] = sw ? i0 : i1;
      }
    }
    double const piv = a[c][c];
    if (piv == 0. || !finite_d(piv)) ok = false;
    double const ip = 1. / piv;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      a[c][k] *= ip;
      inv[c][k] *= ip;
    }
#pragma unroll
    for (int r = 0; r < NB; ++r) {
      if (r == c) continue;
      double const f = a[r][c];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        a[r][k] -= f * a[c][k];
        inv[r][k] -= f * inv[c][k];
      }
    }
  }
#pragma unroll
  for (int ri = 0; ri < NB; ++ri)
#pragma unroll
    for (int cj = 0; cj < NB; ++cj) {
      if (!finite_d(inv[ri][cj])) ok = false;
      minv[(size_t)node * NB * NB + ri * NB + cj] = inv[ri][cj];
    }
  if (!ok) atomicMin(&S->bad_node, node);  // (integer) the smallest such node, whatever the order of the blocks
}

// ---- vector update fused with the preconditioner apply, one work item per node
//   SECOND = 0:  p = r + beta (p - omega v),  out = M^-1 p      (p updated in place)
//   SECOND = 1:  s = r - alpha v,             out = M^-1 s
template <int ND, int NRES, int SECOND>
__global__ void __launch_bounds__(TPB) k_prec(int nn, int nblocks, double const* __restrict__ minv, double const* __restrict__ r,
                                              double const* __restrict__ v, double* __restrict__ w, double* __restrict__ out,
                                              KryScalars const* S) {
  constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  if (S->stop) return;
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const node = lb * TPB + threadIdx.x;
  if (node >= nn) return;
  size_t const n0 = (size_t)nn * ND;
  double const alpha = S->alpha, omega = S->omega, beta = S->beta;
  double y[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    size_t const idx = k < ND ? (size_t)node * ND + k : n0 + node;
    y[k] = SECOND ? r[idx] - alpha * v[idx] : r[idx] + beta * (w[idx] - omega * v[idx]);
    w[idx] = y[k];
  }
  double const* m = minv + (size_t)node * NB * NB;
#pragma unroll
  for (int ri = 0; ri < NB; ++ri) {
    double acc = 0.;
#pragma unroll
    for (int cj = 0; cj < NB; ++cj) acc += m[ri * NB + cj] * y[cj];
    out[ri < ND ? (size_t)node * ND + ri : n0 + node] = acc;
  }
}

// ---- y = A x over the four blocks, G lanes per node: lane l takes the neighbours l, l + G, ... of the node's graph row
// and all NB rows of the node at once (consecutive lanes read consecutive ND-vectors of a CSR row), then a butterfly over
// the G lanes.  The inner products the method needs of y leave as one partial per block.
//   MODE 0:  v = A phat;      part[lb] = rhat . v                                   (y = v, a0 = rhat)
//   MODE 1:  t = A shat;      part[lb] = t . s,  part[nblocks + lb] = t . t         (y = t, a0 = s)
template <int ND, int NRES, int G, int MODE>
__global__ void __launch_bounds__(TPB) k_spmv(int nn, int nblocks, int32_t const* __restrict__ nodeptr, int32_t const* __restrict__ nodeadj,
                                              Blocks A, double const* __restrict__ x, double* __restrict__ y, double const* __restrict__ a0,
                                              double* __restrict__ part, KryScalars const* S) {
  constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  constexpr int NPB = TPB / G;
  __shared__ double sm[TPB / 64];
  if (S->stop) return;
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const node = lb * NPB + threadIdx.x / G, lane = threadIdx.x % G;
  size_t const n0 = (size_t)nn * ND;
  double acc[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) acc[k] = 0.;
  if (node < nn) {
    int64_t const np = nodeptr[node];
    int const deg = (int)(nodeptr[node + 1] - np);
    for (int k = lane; k < deg; k += G) {
      int const cn = nodeadj[np + k];
      double xv[NB];
#pragma unroll
      for (int e = 0; e < NB; ++e) xv[e] = x[e < ND ? (size_t)cn * ND + e : n0 + cn];
#pragma unroll
      for (int ri = 0; ri < ND; ++ri) {
        double const* row = A.A00 + np * ND * ND + (int64_t)ri * deg * ND + (int64_t)k * ND;
#pragma unroll
        for (int e = 0; e < ND; ++e) acc[ri] += row[e] * xv[e];
        if (NRES == 2) acc[ri] += A.A01[np * ND + (int64_t)ri * deg + k] * xv[NB - 1];
      }
      if (NRES == 2) {
        double const* row = A.A10 + np * ND + (int64_t)k * ND;
#pragma unroll
        for (int e = 0; e < ND; ++e) acc[NB - 1] += row[e] * xv[e];
        acc[NB - 1] += A.A11[np + k] * xv[NB - 1];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NB; ++k)
    for (int o = G / 2; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, G);
  double d0 = 0., d1 = 0.;
  if (node < nn && lane == 0) {
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      size_t const idx = k < ND ? (size_t)node * ND + k : n0 + node;
      y[idx] = acc[k];
      d0 += a0[idx] * acc[k];
      if (MODE == 1) d1 += acc[k] * acc[k];
    }
  }
  double const s0 = block_sum(d0, sm);
  if (threadIdx.x == 0) part[lb] = s0;
  if (MODE == 1) {
    double const s1 = block_sum(d1, sm);
    if (threadIdx.x == 0) part[nblocks + lb] = s1;
  }
}

// ---- the TRUE residual: r = b - A x, rhat = r, p = v = 0, part[lb] = r . r -- the start, every restart, and the number a
// solve reports and is judged by.  At the tolerance the residual is a difference of numbers 1 / rel_tol times larger, so
// two summation orders of A x differ in |b - A x| by eps |A| |x| / |r|: 1e-6 to 3e-4 relative between the lane-parallel
// sums of k_spmv and a host's row-by-row product on the test systems.  The reported value is therefore DEFINED by the
// plain CSR order -- each row summed from zero over the columns of the u block, then of the p block, in the order of the
// graphs, every product and sum rounded separately (no fused multiply-add) -- which is the order of a host recomputation
// from the downloaded blocks (SciPy's csr_matvec), so that a caller can check the number and not only its magnitude.  One
// work item per node; runs a few times per solve, not per iteration.
template <int ND, int NRES>
__global__ void __launch_bounds__(TPB) k_true_residual(int nn, int nblocks, int32_t const* __restrict__ nodeptr, int32_t const* __restrict__ nodeadj,
                                                       Blocks A, double const* __restrict__ x, double const* __restrict__ b0,
                                                       double const* __restrict__ b1, double* __restrict__ r, double* __restrict__ rhat,
                                                       double* __restrict__ p, double* __restrict__ v, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double sm[TPB / 64];
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const node = lb * TPB + threadIdx.x;
  size_t const n0 = (size_t)nn * ND;
  double d0 = 0.;
  if (node < nn) {
    int64_t const np = nodeptr[node];
    int const deg = (int)(nodeptr[node + 1] - np);
    for (int ri = 0; ri < ND + (NRES == 2 ? 1 : 0); ++ri) {
      bool const prow = ri == ND;
      double const* a0 = prow ? A.A10 + np * ND : A.A00 + np * ND * ND + (int64_t)ri * deg * ND;   // the row in the u-column block
      double sum = 0.;
      for (int k = 0; k < deg; ++k) {
        int const cn = nodeadj[np + k];
        for (int e = 0; e < ND; ++e) sum = sum + a0[(int64_t)k * ND + e] * x[(size_t)cn * ND + e];
      }
      if (NRES == 2) {
        double const* a1 = prow ? A.A11 + np : A.A01 + np * ND + (int64_t)ri * deg;                // ... in the p-column block
        for (int k = 0; k < deg; ++k) sum = sum + a1[k] * x[n0 + nodeadj[np + k]];
      }
      size_t const idx = prow ? n0 + node : (size_t)node * ND + ri;
      double const rn = (prow ? b1[node] : b0[(size_t)node * ND + ri]) - sum;
      r[idx] = rn;
      rhat[idx] = rn;
      p[idx] = 0.;
      v[idx] = 0.;
      d0 = d0 + rn * rn;
    }
  }
  double const s0 = block_sum(d0, sm);
  if (threadIdx.x == 0) part[lb] = s0;
}

// ---- x += alpha phat + omega shat,  r = s - omega t;  part[b] = rhat . r,  part[gridDim + b] = r . r
__global__ void __launch_bounds__(TPB) k_update(size_t n, double* __restrict__ x, double* __restrict__ r, double const* __restrict__ s,
                                                double const* __restrict__ t, double const* __restrict__ phat, double const* __restrict__ shat,
                                                double const* __restrict__ rhat, double* __restrict__ part, KryScalars const* S) {
  __shared__ double sm[TPB / 64];
  if (S->stop) return;
  double const alpha = S->alpha, omega = S->omega;
  double d0 = 0., d1 = 0.;
  for (size_t i = blockIdx.x * (size_t)TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) {
    x[i] += alpha * phat[i] + omega * shat[i];
    double const rn = s[i] - omega * t[i];
    r[i] = rn;
    d0 += rhat[i] * rn;
    d1 += rn * rn;
  }
  double const s0 = block_sum(d0, sm);
  double const s1 = block_sum(d1, sm);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s0;
    part[gridDim.x + blockIdx.x] = s1;
  }
}

// ---- one block adds the partials (thread t the blocks t, t + TPB, ... in order, then the fixed tree of block_sum) and
// forms the scalars of the recurrence in device memory
//   KIND 0: alpha = rho / (rhat . v)           KIND 1: omega = (t . s) / (t . t)
//   KIND 2: |r|^2, iteration count, stop flag, beta = (rho' / rho) (alpha / omega), rho = rho'
//   KIND 3: start / restart: rho = |r|^2 (rhat = r), beta = 0, alpha = omega = 1, stop = 0
template <int KIND>
__global__ void __launch_bounds__(TPB) k_reduce(double const* __restrict__ part, int nb, double tol2, KryScalars* S) {
  __shared__ double sm[TPB / 64];
  if (KIND != 3 && S->stop) return;
  double a0 = 0., a1 = 0.;
  for (int b = threadIdx.x; b < nb; b += TPB) a0 += part[b];
  if (KIND == 1 || KIND == 2)
    for (int b = threadIdx.x; b < nb; b += TPB) a1 += part[nb + b];
  double const s0 = block_sum(a0, sm);
  double const s1 = (KIND == 1 || KIND == 2) ? block_sum(a1, sm) : 0.;
  if (threadIdx.x != 0) return;
  if (KIND == 0) {
    double const alpha = S->rho / s0;
    if (!finite_d(alpha) || fabs(s0) < BREAKDOWN) S->stop = 2;
    else S->alpha = alpha;
  } else if (KIND == 1) {
    double const omega = s0 / s1;
    if (!finite_d(omega) || fabs(omega) < BREAKDOWN) S->stop = 2;
    else S->omega = omega;
  } else if (KIND == 2) {
    S->rr = s1;
    S->iters += 1;
    if (s1 <= tol2) S->stop = 1;
    else if (!finite_d(s1) || !finite_d(s0) || fabs(s0) < BREAKDOWN) S->stop = 2;
    else {
      S->beta = (s0 / S->rho) * (S->alpha / S->omega);
      S->rho = s0;
    }
  } else {
    S->rr = s0;
    S->rho = s0;
    S->beta = 0.;
    S->alpha = 1.;
    S->omega = 1.;
    S->stop = 0;
  }
}

// ---- multicolour node-block Gauss-Seidel (c8_krylov_set_preconditioner).  One launch per colour:
//   x_i <- x_i + D_i^-1 (rhs_i - sum_j A_ij x_j)   for the nodes i of list[0 .. nlist), j over the columns < colbound
// of the node's graph row.  Lane mapping of k_spmv_list (G lanes per node over the neighbours, all NB rows at once, a
// butterfly over the G lanes); lane ri < NB of the node then forms row ri of D_i^-1 (rhs_i - sum) and adds it to x in place.
// No two nodes of a list are neighbours, so every x entry a launch reads from another node is one it does not write: x is
// read and written through the same plain pointer (no __restrict__, no read-only path).  A node's own entry is read by its
// own lanes only, before the butterfly that its store depends on.  colbound = the number of local nodes, or num_owned
// for the part-local operator (ghost and phantom columns dropped).
template <int ND, int NRES, int G>
__global__ void __launch_bounds__(TPB) k_sgs_color(int32_t const* __restrict__ list, int nlist, int nn, int nblocks, int colbound,
                                                   int32_t const* __restrict__ nodeptr, int32_t const* __restrict__ nodeadj, Blocks A,
                                                   double const* __restrict__ minv, double const* __restrict__ rhs, double* x,
                                                   KryScalars const* S) {
  constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  constexpr int NPB = TPB / G;
  if (S->stop) return;
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const li = lb * NPB + threadIdx.x / G, lane = threadIdx.x % G;
  bool const live = li < nlist;
  int const node = live ? list[li] : 0;
  size_t const n0 = (size_t)nn * ND;
  double acc[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) acc[k] = 0.;
  if (live) {
    int64_t const np = nodeptr[node];
    int const deg = (int)(nodeptr[node + 1] - np);
    for (int k = lane; k < deg; k += G) {
      int const cn = nodeadj[np + k];
      if (cn >= colbound) continue;
      double xv[NB];
#pragma unroll
      for (int e = 0; e < NB; ++e) xv[e] = x[e < ND ? (size_t)cn * ND + e : n0 + cn];
#pragma unroll
      for (int ri = 0; ri < ND; ++ri) {
        double const* row = A.A00 + np * ND * ND + (int64_t)ri * deg * ND + (int64_t)k * ND;
#pragma unroll
        for (int e = 0; e < ND; ++e) acc[ri] += row[e] * xv[e];
        if (NRES == 2) acc[ri] += A.A01[np * ND + (int64_t)ri * deg + k] * xv[NB - 1];
      }
      if (NRES == 2) {
        double const* row = A.A10 + np * ND + (int64_t)k * ND;
#pragma unroll
        for (int e = 0; e < ND; ++e) acc[NB - 1] += row[e] * xv[e];
        acc[NB - 1] += A.A11[np + k] * xv[NB - 1];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NB; ++k)
    for (int o = G / 2; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, G);
  if (live && lane < NB) {
    double const* m = minv + (size_t)node * NB * NB + lane * NB;
    double d = 0.;
#pragma unroll
    for (int cj = 0; cj < NB; ++cj) d += m[cj] * (rhs[cj < ND ? (size_t)node * ND + cj : n0 + node] - acc[cj]);
    size_t const idx = lane < ND ? (size_t)node * ND + lane : n0 + node;
    x[idx] += d;
  }
}

// ---- the vector update of k_prec without its preconditioner apply, over the two owned ranges of k_update_own; out = 0
// is the start of the Gauss-Seidel sweeps that follow
//   SECOND = 0:  p = r + beta (p - omega v)  (in place, w = p)        SECOND = 1:  s = r - alpha v  (w = s)
template <int SECOND>
__global__ void __launch_bounds__(TPB) k_vec(size_t nu, size_t np_, size_t n0, double const* __restrict__ r, double const* __restrict__ v,
                                             double* __restrict__ w, double* __restrict__ out, KryScalars const* S) {
  if (S->stop) return;
  double const alpha = S->alpha, omega = S->omega, beta = S->beta;
  for (size_t j = blockIdx.x * (size_t)TPB + threadIdx.x; j < nu + np_; j += (size_t)gridDim.x * TPB) {
    size_t const i = j < nu ? j : n0 + (j - nu);
    w[i] = SECOND ? r[i] - alpha * v[i] : r[i] + beta * (w[i] - omega * v[i]);
    out[i] = 0.;
  }
}

template <class T>
int grow(T** buf, size_t* have, size_t need) {
  if (need <= *have) return C8_OK;
  if (*buf) C8_HIP(hipFree(*buf));
  *buf = nullptr;
  *have = 0;
  C8_HIP(hipMalloc((void**)buf, need * sizeof(T)));
  *have = need;
  return C8_OK;
}

#include "c8_krylov_coarse.hpp"

struct Solve {
  c8_ctx* c;
  int nn, nb_node, nb_spmv, nb_upd;
  size_t n;  // length of a vector
  Blocks A;
  double const *b0, *b1;
  double *x, *r, *rhat, *p, *v, *s, *t, *phat, *shat, *part, *minv;
  KryScalars* S;
  double tol2 = 0.;
  // the aggregation kinds: the levels below level 0 ([k] is level k + 1), the wording of the kind, level 0
  std::vector<c8_kry_level> const* lv = nullptr;
  bool multi = false;
  Level0 l0{};
};

template <int ND, int NRES>
int launch_setup(Solve const& q) {
  hipLaunchKernelGGL((k_setup<ND, NRES>), dim3(xcd_grid(q.nb_node)), dim3(TPB), 0, q.c->stream, q.nn, q.nb_node, q.c->d_nodeptr,
                     q.c->d_nodeadj, q.A, q.minv, q.S);
  C8_HIP(hipGetLastError());
  return C8_OK;
}

// r = b - A x, rhat = r, p = v = 0 and the scalars of a fresh recurrence; S->rr = |b - A x|^2
template <int ND, int NRES>
int launch_residual(Solve const& q) {
  hipLaunchKernelGGL((k_true_residual<ND, NRES>), dim3(xcd_grid(q.nb_node)), dim3(TPB), 0, q.c->stream, q.nn, q.nb_node, q.c->d_nodeptr,
                     q.c->d_nodeadj, q.A, q.x, q.b0, q.b1, q.r, q.rhat, q.p, q.v, q.part);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_reduce<3>), dim3(1), dim3(TPB), 0, q.c->stream, q.part, q.nb_node, 0., q.S);
  C8_HIP(hipGetLastError());
  return C8_OK;
}

template <int ND, int NRES, int G>
int launch_iteration(Solve const& q) {
  hipStream_t const st = q.c->stream;
  int32_t const *np = q.c->d_nodeptr, *na = q.c->d_nodeadj;
  hipLaunchKernelGGL((k_prec<ND, NRES, 0>), dim3(xcd_grid(q.nb_node)), dim3(TPB), 0, st, q.nn, q.nb_node, q.minv, q.r, q.v, q.p, q.phat, q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_spmv<ND, NRES, G, 0>), dim3(xcd_grid(q.nb_spmv)), dim3(TPB), 0, st, q.nn, q.nb_spmv, np, na, q.A, q.phat, q.v, q.rhat,
                     q.part, q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_reduce<0>), dim3(1), dim3(TPB), 0, st, q.part, q.nb_spmv, 0., q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_prec<ND, NRES, 1>), dim3(xcd_grid(q.nb_node)), dim3(TPB), 0, st, q.nn, q.nb_node, q.minv, q.r, q.v, q.s, q.shat, q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_spmv<ND, NRES, G, 1>), dim3(xcd_grid(q.nb_spmv)), dim3(TPB), 0, st, q.nn, q.nb_spmv, np, na, q.A, q.shat, q.t, q.s,
                     q.part, q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_reduce<1>), dim3(1), dim3(TPB), 0, st, q.part, q.nb_spmv, 0., q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_update, dim3(q.nb_upd), dim3(TPB), 0, st, q.n, q.x, q.r, q.s, q.t, q.phat, q.shat, q.rhat, q.part, q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_reduce<2>), dim3(1), dim3(TPB), 0, st, q.part, q.nb_upd, q.tol2, q.S);
  C8_HIP(hipGetLastError());
  return C8_OK;
}

// x = M^-1 rhs by the context's number of symmetric sweeps, x = 0 on entry (k_vec): colours 0 .. nc - 1, then nc - 2 .. 0,
// one launch each.  Every launch is the general form -- the first forward sweep reads the zeros of the colours it has not
// reached yet -- except colour 0 of the first sweep, which reads no column at all (colbound 0: x_i = D_i^-1 rhs_i).
// from_zero = false (the aggregation kinds: x holds the coarse correction on entry) gives that launch the full bound too.
template <int ND, int NRES, int G>
hipError_t launch_sgs(Solve const& q, int colbound, double const* rhs, double* x, bool from_zero = true) {
  c8_ctx const* c = q.c;
  int const nc = (int)c->kry_color_ptr.size() - 1;
  auto color = [&](int k, int bound) {
    int const lo = c->kry_color_ptr[k], n = c->kry_color_ptr[k + 1] - lo, nblocks = (n + TPB / G - 1) / (TPB / G);
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL((k_sgs_color<ND, NRES, G>), dim3(xcd_grid(nblocks)), dim3(TPB), 0, c->stream, c->d_kry_colors + lo, n, q.nn, nblocks, bound,
                       c->d_nodeptr, c->d_nodeadj, q.A, q.minv, rhs, x, q.S);
    return hipGetLastError();
  };
  hipError_t e;
  for (int s = 0; s < c->kry_sweeps; ++s) {
    for (int k = 0; k < nc; ++k)
      if ((e = color(k, from_zero && s == 0 && k == 0 ? 0 : colbound)) != hipSuccess) return e;
    for (int k = nc - 2; k >= 0; --k)
      if ((e = color(k, colbound)) != hipSuccess) return e;
  }
  return hipSuccess;
}

void color_graph(int n, std::vector<int32_t> const& gp, std::vector<int32_t> const& ga, std::vector<int32_t>* color_ptr,
                 std::vector<int32_t>* color_nodes);
#include "c8_krylov_multilevel.hpp"

// The levels of q and its level 0 for a kind of one part, after the kind's refusals (coarse_refusals, multilevel_refusals)
void use_levels(Solve& q, bool multi) {
  q.lv = multi ? &q.c->kry_levels : &q.c->kry_agg_levels;
  q.multi = multi;
  q.l0 = level0(q.c);
}

// launch_iteration with the Gauss-Seidel sweeps in the place of the D^-1 multiplication; COARSE (the aggregation kinds):
// the sweeps start from the coarse correction of their right-hand side
template <int ND, int NRES, int G, bool COARSE>
int launch_iteration_sgs(Solve const& q) {
  hipStream_t const st = q.c->stream;
  int32_t const *np = q.c->d_nodeptr, *na = q.c->d_nodeadj;
  size_t const n0 = (size_t)q.nn * ND;
  hipLaunchKernelGGL((k_vec<0>), dim3(q.nb_upd), dim3(TPB), 0, st, q.n, (size_t)0, n0, q.r, q.v, q.p, q.phat, q.S);
  C8_HIP(hipGetLastError());
  if (COARSE) C8_HIP((levels_apply<ND, NRES>(q, q.p, q.phat)));
  C8_HIP((launch_sgs<ND, NRES, G>(q, q.nn, q.p, q.phat, !COARSE)));
  hipLaunchKernelGGL((k_spmv<ND, NRES, G, 0>), dim3(xcd_grid(q.nb_spmv)), dim3(TPB), 0, st, q.nn, q.nb_spmv, np, na, q.A, q.phat, q.v, q.rhat,
                     q.part, q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_reduce<0>), dim3(1), dim3(TPB), 0, st, q.part, q.nb_spmv, 0., q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_vec<1>), dim3(q.nb_upd), dim3(TPB), 0, st, q.n, (size_t)0, n0, q.r, q.v, q.s, q.shat, q.S);
  C8_HIP(hipGetLastError());
  if (COARSE) C8_HIP((levels_apply<ND, NRES>(q, q.s, q.shat)));
  C8_HIP((launch_sgs<ND, NRES, G>(q, q.nn, q.s, q.shat, !COARSE)));
  hipLaunchKernelGGL((k_spmv<ND, NRES, G, 1>), dim3(xcd_grid(q.nb_spmv)), dim3(TPB), 0, st, q.nn, q.nb_spmv, np, na, q.A, q.shat, q.t, q.s,
                     q.part, q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_reduce<1>), dim3(1), dim3(TPB), 0, st, q.part, q.nb_spmv, 0., q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_update, dim3(q.nb_upd), dim3(TPB), 0, st, q.n, q.x, q.r, q.s, q.t, q.phat, q.shat, q.rhat, q.part, q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_reduce<2>), dim3(1), dim3(TPB), 0, st, q.part, q.nb_upd, q.tol2, q.S);
  C8_HIP(hipGetLastError());
  return C8_OK;
}

inline bool aggregation_kind(int kind) {
  return kind == C8_PRECOND_TWO_LEVEL || kind == C8_PRECOND_MULTILEVEL || kind == C8_PRECOND_TWO_LEVEL_PARTS || kind == C8_PRECOND_MULTILEVEL_PARTS;
}
inline bool multilevel_kind(int kind) { return kind == C8_PRECOND_MULTILEVEL || kind == C8_PRECOND_MULTILEVEL_PARTS; }

struct Launchers {
  int (*setup)(Solve const&);
  int (*residual)(Solve const&);
  int (*iteration)(Solve const&);
  int (*levels)(Solve const&, int);  // the levels of an aggregation kind for the matrix (levels_setup)
  int group;
};
template <int ND, int NRES, int G>
Launchers launchers(int kind) {
  return Launchers{launch_setup<ND, NRES>, launch_residual<ND, NRES>,
                   aggregation_kind(kind) ? launch_iteration_sgs<ND, NRES, G, true>
                   : kind == C8_PRECOND_BLOCK_SGS ? launch_iteration_sgs<ND, NRES, G, false> : launch_iteration<ND, NRES, G>,
                   levels_setup<ND, NRES, G>, G};
}
// the one dispatch over (ndims, nres) of the solve of one part (false: no kernels)
bool launchers_of(c8_ctx const* c, Launchers* L) {
  bool const two = c->nres == 2;
  if (c->ndims == 3 && two) *L = launchers<3, 2, 16>(c->kry_precond);
  else if (c->ndims == 2 && two) *L = launchers<2, 2, 8>(c->kry_precond);
  else if (c->ndims == 2 && !two) *L = launchers<2, 1, 8>(c->kry_precond);
  else return false;
  return true;
}

int read_scalars(Solve const& q, KryScalars* h) {
  C8_HIP(hipMemcpyAsync(h, q.S, sizeof(KryScalars), hipMemcpyDeviceToHost, q.c->stream));
  C8_HIP(hipStreamSynchronize(q.c->stream));
  return C8_OK;
}

// ======================================================================================================================
// The kernels of the multi-part solve.  nown = owned nodes (the rows this part iterates on), nn = local nodes (owned,
// ghost, phantom: the p segment of a vector starts at nn * ND).  Nothing in a ghost or phantom entry enters a sum.
// ======================================================================================================================

// k_prec over the owned nodes
template <int ND, int NRES, int SECOND>
__global__ void __launch_bounds__(TPB) k_prec_own(int nown, int nn, int nblocks, double const* __restrict__ minv, double const* __restrict__ r,
                                                  double const* __restrict__ v, double* __restrict__ w, double* __restrict__ out,
                                                  KryScalars const* S) {
  constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  if (S->stop) return;
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const node = lb * TPB + threadIdx.x;
  if (node >= nown) return;
  size_t const n0 = (size_t)nn * ND;
  double const alpha = S->alpha, omega = S->omega, beta = S->beta;
  double y[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    size_t const idx = k < ND ? (size_t)node * ND + k : n0 + node;
    y[k] = SECOND ? r[idx] - alpha * v[idx] : r[idx] + beta * (w[idx] - omega * v[idx]);
    w[idx] = y[k];
  }
  double const* m = minv + (size_t)node * NB * NB;
#pragma unroll
  for (int ri = 0; ri < NB; ++ri) {
    double acc = 0.;
#pragma unroll
    for (int cj = 0; cj < NB; ++cj) acc += m[ri * NB + cj] * y[cj];
    out[ri < ND ? (size_t)node * ND + ri : n0 + node] = acc;
  }
}

// k_spmv with the row taken from a node list (same lane mapping: G lanes per node): block lb of this launch multiplies
// the nodes list[lb * NPB ...] and leaves its partials in slot slot0 + lb (and nslots + slot0 + lb) of `part`
template <int ND, int NRES, int G, int MODE>
__global__ void __launch_bounds__(TPB) k_spmv_list(int32_t const* __restrict__ list, int nlist, int nn, int nblocks, int slot0, int nslots,
                                                   int32_t const* __restrict__ nodeptr, int32_t const* __restrict__ nodeadj, Blocks A,
                                                   double const* __restrict__ x, double* __restrict__ y, double const* __restrict__ a0,
                                                   double* __restrict__ part, KryScalars const* S) {
  constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  constexpr int NPB = TPB / G;
  __shared__ double sm[TPB / 64];
  if (S->stop) return;
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const li = lb * NPB + threadIdx.x / G, lane = threadIdx.x % G;
  bool const live = li < nlist;
  int const node = live ? list[li] : 0;
  size_t const n0 = (size_t)nn * ND;
  double acc[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) acc[k] = 0.;
  if (live) {
    int64_t const np = nodeptr[node];
    int const deg = (int)(nodeptr[node + 1] - np);
    for (int k = lane; k < deg; k += G) {
      int const cn = nodeadj[np + k];
      double xv[NB];
#pragma unroll
      for (int e = 0; e < NB; ++e) xv[e] = x[e < ND ? (size_t)cn * ND + e : n0 + cn];
#pragma unroll
      for (int ri = 0; ri < ND; ++ri) {
        double const* row = A.A00 + np * ND * ND + (int64_t)ri * deg * ND + (int64_t)k * ND;
#pragma unroll
        for (int e = 0; e < ND; ++e) acc[ri] += row[e] * xv[e];
        if (NRES == 2) acc[ri] += A.A01[np * ND + (int64_t)ri * deg + k] * xv[NB - 1];
      }
      if (NRES == 2) {
        double const* row = A.A10 + np * ND + (int64_t)k * ND;
#pragma unroll
        for (int e = 0; e < ND; ++e) acc[NB - 1] += row[e] * xv[e];
        acc[NB - 1] += A.A11[np + k] * xv[NB - 1];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NB; ++k)
    for (int o = G / 2; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, G);
  double d0 = 0., d1 = 0.;
  if (live && lane == 0) {
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      size_t const idx = k < ND ? (size_t)node * ND + k : n0 + node;
      y[idx] = acc[k];
      d0 += a0[idx] * acc[k];
      if (MODE == 1) d1 += acc[k] * acc[k];
    }
  }
  double const s0 = block_sum(d0, sm);
  if (threadIdx.x == 0) part[slot0 + lb] = s0;
  if (MODE == 1) {
    double const s1 = block_sum(d1, sm);
    if (threadIdx.x == 0) part[nslots + slot0 + lb] = s1;
  }
}

// k_true_residual over the owned rows, in the same plain CSR order: a row's value equals a host recomputation from the
// gathered global matrix (x holds the owners' values in its ghost and phantom entries: imported before the launch)
template <int ND, int NRES>
__global__ void __launch_bounds__(TPB) k_true_residual_own(int nown, int nn, int nblocks, int32_t const* __restrict__ nodeptr,
                                                           int32_t const* __restrict__ nodeadj, Blocks A, double const* __restrict__ x,
                                                           double const* __restrict__ b0, double const* __restrict__ b1, double* __restrict__ r,
                                                           double* __restrict__ rhat, double* __restrict__ p, double* __restrict__ v,
                                                           double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double sm[TPB / 64];
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const node = lb * TPB + threadIdx.x;
  size_t const n0 = (size_t)nn * ND;
  double d0 = 0.;
  if (node < nown) {
    int64_t const np = nodeptr[node];
    int const deg = (int)(nodeptr[node + 1] - np);
    for (int ri = 0; ri < ND + (NRES == 2 ? 1 : 0); ++ri) {
      bool const prow = ri == ND;
      double const* a0 = prow ? A.A10 + np * ND : A.A00 + np * ND * ND + (int64_t)ri * deg * ND;
      double sum = 0.;
      for (int k = 0; k < deg; ++k) {
        int const cn = nodeadj[np + k];
        for (int e = 0; e < ND; ++e) sum = sum + a0[(int64_t)k * ND + e] * x[(size_t)cn * ND + e];
      }
      if (NRES == 2) {
        double const* a1 = prow ? A.A11 + np : A.A01 + np * ND + (int64_t)ri * deg;
        for (int k = 0; k < deg; ++k) sum = sum + a1[k] * x[n0 + nodeadj[np + k]];
      }
      size_t const idx = prow ? n0 + node : (size_t)node * ND + ri;
      double const rn = (prow ? b1[node] : b0[(size_t)node * ND + ri]) - sum;
      r[idx] = rn;
      rhat[idx] = rn;
      p[idx] = 0.;
      v[idx] = 0.;
      d0 = d0 + rn * rn;
    }
  }
  double const s0 = block_sum(d0, sm);
  if (threadIdx.x == 0) part[lb] = s0;
}

// k_update over the two owned ranges: [0, nu) of the u segment and [0, np_) of the p segment (which starts at n0)
__global__ void __launch_bounds__(TPB) k_update_own(size_t nu, size_t np_, size_t n0, double* __restrict__ x, double* __restrict__ r,
                                                    double const* __restrict__ s, double const* __restrict__ t, double const* __restrict__ phat,
                                                    double const* __restrict__ shat, double const* __restrict__ rhat, double* __restrict__ part,
                                                    KryScalars const* S) {
  __shared__ double sm[TPB / 64];
  if (S->stop) return;
  double const alpha = S->alpha, omega = S->omega;
  double d0 = 0., d1 = 0.;
  for (size_t j = blockIdx.x * (size_t)TPB + threadIdx.x; j < nu + np_; j += (size_t)gridDim.x * TPB) {
    size_t const i = j < nu ? j : n0 + (j - nu);
    x[i] += alpha * phat[i] + omega * shat[i];
    double const rn = s[i] - omega * t[i];
    r[i] = rn;
    d0 += rhat[i] * rn;
    d1 += rn * rn;
  }
  double const s0 = block_sum(d0, sm);
  double const s1 = block_sum(d1, sm);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = s0;
    part[gridDim.x + blockIdx.x] = s1;
  }
}

// one block adds this part's partials in the fixed order of k_reduce: sums[0] (and sums[1] for KIND 1, 2), to be
// all-reduced over the parts.  KIND as in k_reduce.
template <int KIND>
__global__ void __launch_bounds__(TPB) k_sums(double const* __restrict__ part, int nb, double* __restrict__ sums, KryScalars const* S) {
  __shared__ double sm[TPB / 64];
  if (KIND != 3 && S->stop) return;
  double a0 = 0., a1 = 0.;
  for (int b = threadIdx.x; b < nb; b += TPB) a0 += part[b];
  if (KIND == 1 || KIND == 2)
    for (int b = threadIdx.x; b < nb; b += TPB) a1 += part[nb + b];
  double const s0 = block_sum(a0, sm);
  double const s1 = (KIND == 1 || KIND == 2) ? block_sum(a1, sm) : 0.;
  if (threadIdx.x != 0) return;
  sums[0] = s0;
  if (KIND == 1 || KIND == 2) sums[1] = s1;
}

// the scalars of the recurrence from the GLOBAL sums (the formulas of k_reduce): the same on every rank
template <int KIND>
__global__ void __launch_bounds__(64) k_scalars(double const* __restrict__ sums, double tol2, KryScalars* S) {
  if (threadIdx.x != 0 || (KIND != 3 && S->stop)) return;
  double const s0 = sums[0], s1 = (KIND == 1 || KIND == 2) ? sums[1] : 0.;
  if (KIND == 0) {
    double const alpha = S->rho / s0;
    if (!finite_d(alpha) || !(fabs(s0) >= BREAKDOWN)) S->stop = 2;
    else S->alpha = alpha;
  } else if (KIND == 1) {
    double const omega = s0 / s1;
    if (!finite_d(omega) || !(fabs(omega) >= BREAKDOWN)) S->stop = 2;
    else S->omega = omega;
  } else if (KIND == 2) {
    S->rr = s1;
    S->iters += 1;
    if (s1 <= tol2) S->stop = 1;
    else if (!finite_d(s1) || !finite_d(s0) || !(fabs(s0) >= BREAKDOWN)) S->stop = 2;
    else {
      S->beta = (s0 / S->rho) * (S->alpha / S->omega);
      S->rho = s0;
    }
  } else {
    S->rr = s0;
    S->rho = s0;
    S->beta = 0.;
    S->alpha = 1.;
    S->omega = 1.;
    S->stop = 0;
  }
}

// ---- host side of the multi-part solve.  A rank that meets a device error goes on through the collective sequence of the
// batch as a bystander (`failed`: no device work, the transport's degraded entries) and reports at the next host read, where
// all ranks leave together: a rank that stopped exchanging on its own would hang the others.
struct Parts {
  Solve q;
  c8_halo* h = nullptr;
  c8_comm* cm = nullptr;
  int rank = 0, nranks = 1;
  int nown = 0, n_int = 0, n_bnd = 0, nb_own = 0, nb_int = 0, nb_bnd = 0, nb_upd = 0;
  int32_t const* list = nullptr;
  double* sums = nullptr;
  double *x1 = nullptr, *phat1 = nullptr, *shat1 = nullptr;  // the p segments (null with one residual)
  bool failed = false;
  std::string err;
  void note(int rc) {
    if (rc != C8_OK && !failed) { failed = true; err = c8_last_error(); }
  }
  void hip(hipError_t e, char const* what) {
    if (e != hipSuccess && !failed) { failed = true; err = std::string(what) + ": " + hipGetErrorString(e); }
  }
};
#define C8_PARTS_LAUNCH(P, kernel, grid, block, ...)                        \
  do {                                                                      \
    if (!(P).failed && (grid) > 0) {                                        \
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, (P).q.c->stream, __VA_ARGS__); \
      (P).hip(hipGetLastError(), #kernel);                                  \
    }                                                                       \
  } while (0)

// all-reduce of the n local sums and the scalars of KIND from the global ones
template <int KIND>
void parts_scalars(Parts& P, int nb) {
  C8_PARTS_LAUNCH(P, (k_sums<KIND>), 1, TPB, P.q.part, nb, P.sums, P.q.S);
  P.note(c8_comm_allreduce_device(P.cm, P.q.c->stream, P.sums, (KIND == 1 || KIND == 2) ? 2 : 1, P.failed));
  C8_PARTS_LAUNCH(P, (k_scalars<KIND>), 1, 64, P.sums, P.q.tol2, P.q.S);
}

// y = A x over the owned rows, the import of x's copies overlapped with the interior rows
template <int ND, int NRES, int G, int MODE>
void parts_spmv(Parts& P, double* x, double* x1, double* y, double const* a0) {
  Solve const& q = P.q;
  int32_t const *np = q.c->d_nodeptr, *na = q.c->d_nodeadj;
  int const nslots = P.nb_int + P.nb_bnd;
  P.note(c8_halo_import_start(P.h, x, x1, P.failed));
  C8_PARTS_LAUNCH(P, (k_spmv_list<ND, NRES, G, MODE>), xcd_grid(P.nb_int), TPB, P.list, P.n_int, q.nn, P.nb_int, 0, nslots, np, na, q.A, x, y, a0,
                  q.part, q.S);
  P.note(c8_halo_import_finish(P.h, x, x1, P.failed));
  C8_PARTS_LAUNCH(P, (k_spmv_list<ND, NRES, G, MODE>), xcd_grid(P.nb_bnd), TPB, P.list + P.n_int, P.n_bnd, q.nn, P.nb_bnd, P.nb_int, nslots, np, na,
                  q.A, x, y, a0, q.part, q.S);
}

template <int ND, int NRES>
void parts_setup(Parts& P) {
  Solve const& q = P.q;
  C8_PARTS_LAUNCH(P, (k_setup<ND, NRES>), xcd_grid(P.nb_own), TPB, P.nown, P.nb_own, q.c->d_nodeptr, q.c->d_nodeadj, q.A, q.minv, q.S);
}

// r = b - A x on the owned rows (x imported first), the scalars of a fresh recurrence; S->rr = |b - A x|^2 over all parts
template <int ND, int NRES>
void parts_residual(Parts& P) {
  Solve const& q = P.q;
  P.note(c8_halo_import_start(P.h, q.x, P.x1, P.failed));
  P.note(c8_halo_import_finish(P.h, q.x, P.x1, P.failed));
  C8_PARTS_LAUNCH(P, (k_true_residual_own<ND, NRES>), xcd_grid(P.nb_own), TPB, P.nown, q.nn, P.nb_own, q.c->d_nodeptr, q.c->d_nodeadj, q.A, q.x,
                  q.b0, q.b1, q.r, q.rhat, q.p, q.v, q.part);
  parts_scalars<3>(P, P.nb_own);
}

template <int ND, int NRES, int G>
void parts_iteration(Parts& P) {
  Solve const& q = P.q;
  size_t const n0 = (size_t)q.nn * ND;
  C8_PARTS_LAUNCH(P, (k_prec_own<ND, NRES, 0>), xcd_grid(P.nb_own), TPB, P.nown, q.nn, P.nb_own, q.minv, q.r, q.v, q.p, q.phat, q.S);
  parts_spmv<ND, NRES, G, 0>(P, q.phat, P.phat1, q.v, q.rhat);
  parts_scalars<0>(P, P.nb_int + P.nb_bnd);
  C8_PARTS_LAUNCH(P, (k_prec_own<ND, NRES, 1>), xcd_grid(P.nb_own), TPB, P.nown, q.nn, P.nb_own, q.minv, q.r, q.v, q.s, q.shat, q.S);
  parts_spmv<ND, NRES, G, 1>(P, q.shat, P.shat1, q.t, q.s);
  parts_scalars<1>(P, P.nb_int + P.nb_bnd);
  C8_PARTS_LAUNCH(P, k_update_own, P.nb_upd, TPB, (size_t)P.nown * ND, NRES == 2 ? (size_t)P.nown : (size_t)0, n0, q.x, q.r, q.s, q.t, q.phat,
                  q.shat, q.rhat, q.part, q.S);
  parts_scalars<2>(P, P.nb_upd);
}

#include "c8_krylov_parts_levels.hpp"

// parts_iteration with the part-local Gauss-Seidel sweeps (columns < num_owned) in the place of the D^-1 multiplication;
// COARSE (the aggregation kinds over parts): the sweeps start from the coarse correction of their right-hand side, which
// makes two imports and five all-reduces per iteration
template <int ND, int NRES, int G, bool COARSE>
void parts_iteration_sgs(Parts& P) {
  Solve const& q = P.q;
  size_t const n0 = (size_t)q.nn * ND, nu = (size_t)P.nown * ND, np_ = NRES == 2 ? (size_t)P.nown : (size_t)0;
  C8_PARTS_LAUNCH(P, (k_vec<0>), P.nb_upd, TPB, nu, np_, n0, q.r, q.v, q.p, q.phat, q.S);
  if (COARSE) parts_levels_apply<ND, NRES>(P, q.p, q.phat);
  if (!P.failed) P.hip(launch_sgs<ND, NRES, G>(q, P.nown, q.p, q.phat, !COARSE), "k_sgs_color");
  parts_spmv<ND, NRES, G, 0>(P, q.phat, P.phat1, q.v, q.rhat);
  parts_scalars<0>(P, P.nb_int + P.nb_bnd);
  C8_PARTS_LAUNCH(P, (k_vec<1>), P.nb_upd, TPB, nu, np_, n0, q.r, q.v, q.s, q.shat, q.S);
  if (COARSE) parts_levels_apply<ND, NRES>(P, q.s, q.shat);
  if (!P.failed) P.hip(launch_sgs<ND, NRES, G>(q, P.nown, q.s, q.shat, !COARSE), "k_sgs_color");
  parts_spmv<ND, NRES, G, 1>(P, q.shat, P.shat1, q.t, q.s);
  parts_scalars<1>(P, P.nb_int + P.nb_bnd);
  C8_PARTS_LAUNCH(P, k_update_own, P.nb_upd, TPB, nu, np_, n0, q.x, q.r, q.s, q.t, q.phat, q.shat, q.rhat, q.part, q.S);
  parts_scalars<2>(P, P.nb_upd);
}

struct PartsLaunchers {
  void (*setup)(Parts&);
  void (*residual)(Parts&);
  void (*iteration)(Parts&);
  void (*levels)(Parts&, int);  // the levels of an aggregation kind over parts for the matrix (parts_levels_setup)
  int group;
};
template <int ND, int NRES, int G>
PartsLaunchers parts_launchers(int kind) {
  return PartsLaunchers{parts_setup<ND, NRES>, parts_residual<ND, NRES>,
                        (kind == C8_PRECOND_MULTILEVEL_PARTS || kind == C8_PRECOND_TWO_LEVEL_PARTS) ? parts_iteration_sgs<ND, NRES, G, true>
                        : kind == C8_PRECOND_BLOCK_SGS ? parts_iteration_sgs<ND, NRES, G, false> : parts_iteration<ND, NRES, G>,
                        parts_levels_setup<ND, NRES, G>, G};
}
// the one dispatch over (ndims, nres) of the solve over parts (false: no kernels)
bool parts_launchers_of(c8_ctx const* c, PartsLaunchers* L) {
  bool const two = c->nres == 2;
  if (c->ndims == 3 && two) *L = parts_launchers<3, 2, 16>(c->kry_precond);
  else if (c->ndims == 2 && two) *L = parts_launchers<2, 2, 8>(c->kry_precond);
  else if (c->ndims == 2 && !two) *L = parts_launchers<2, 1, 8>(c->kry_precond);
  else return false;
  return true;
}

// The dense copy of A_level of a list over parts on every rank: the code behind c8_krylov_level_matrix (multi: the levels
// of C8_PRECOND_MULTILEVEL_PARTS) and c8_krylov_coarse_matrix (the two-level list, level 1) with a halo attached.
// COLLECTIVE; without out_host the two-level list asks for its size alone and builds no tables.
int parts_level_matrix(c8_ctx* c, const c8_system* sys, bool multi, int32_t level, int32_t* n_level, double* out_host, char const* who) {
  Parts P = parts_of(c);
  int rc = (multi || out_host) ? parts_levels_prepare(c, P, who, multi) : parts_coarse_refusals(c, P, who);
  if (rc != C8_OK) return rc;
  std::vector<c8_kry_level> const& lv = multi ? c->kry_pl_levels : c->kry_pc_levels;
  int const nc = coarse_columns(c);
  if (multi && (rc = level_matrix_refusals(lv, level, nc)) != C8_OK) return rc;
  *n_level = lv[level - 1].n * nc;
  if (!out_host) return C8_OK;
  PartsLaunchers L;
  if (!parts_launchers_of(c, &L)) return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": no kernels for this number of dimensions and residuals");
  P.q.A = Blocks{sys->A[0][0], sys->A[0][1], sys->A[1][0], sys->A[1][1]};
  L.levels(P, level);
  std::vector<double> blocks;
  if (!P.failed) P.hip(level_copy_start(c, lv, level, nc, out_host, &blocks), "hipMemcpyAsync");
  if (!P.failed) P.hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  if (!P.failed) level_copy_finish(lv, level, nc, out_host, blocks);
  return parts_agree(P, who, -1., [&](int, long long) { return C8_OK; });
}

// The host read of the scalars, COLLECTIVE: the ranks all-reduce (iterations, stop flag, their squares, failure marker).
// Every rank sees the same five sums, so all of them return the same code: C8_ERR_DEVICE when a rank failed, or when the
// iteration counts or stop flags are not the same everywhere (n * sum of squares = square of the sum only for equal values).
int parts_read(Parts& P, KryScalars* h) {
  if (!P.failed) {
    P.hip(hipMemcpyAsync(h, P.q.S, sizeof(KryScalars), hipMemcpyDeviceToHost, P.q.c->stream), "hipMemcpyAsync");
    if (!P.failed) P.hip(hipStreamSynchronize(P.q.c->stream), "hipStreamSynchronize");
  }
  double const it = P.failed ? 0. : (double)h->iters, st = P.failed ? 0. : (double)h->stop;
  double v[5] = {it, st, it * it, st * st, P.failed ? 1. : 0.};
  if (c8_comm_allreduce_sum(P.cm, v, 5) != C8_OK) return C8_ERR_DEVICE;  // (the message is the transport's)
  if (v[4] > 0.)
    return fail(C8_ERR_DEVICE, P.failed ? "c8_krylov_solve_parts: rank " + std::to_string(P.rank) + ": " + P.err
                                        : std::string("c8_krylov_solve_parts: another rank met a device error; all ranks leave the solve"));
  if (!(P.nranks * v[2] == v[0] * v[0]) || !(P.nranks * v[3] == v[1] * v[1]))
    return fail(C8_ERR_DEVICE, "c8_krylov_solve_parts: the ranks disagree on the iteration count or the stop flag (this rank: " +
                               std::to_string(h->iters) + ", " + std::to_string(h->stop) + "); all ranks leave the solve");
  return C8_OK;
}

// the two node lists of A x, from the host graph: owned nodes with owned columns only, then the others
int build_part_lists(c8_ctx* c) {
  int const nown = c8_halo_num_owned(c->halo);
  if (c->kry_list_owned == nown && (nown == 0 || c->d_kry_list)) return C8_OK;
  std::vector<int32_t> interior, boundary;
  for (int n = 0; n < nown; ++n) {
    bool inner = true;
    for (int32_t k = c->graph.nodeptr[n]; k < c->graph.nodeptr[n + 1]; ++k) inner = inner && c->graph.nodeadj[k] < nown;
    (inner ? interior : boundary).push_back(n);
  }
  c->kry_n_interior = (int)interior.size();
  c->kry_list = interior;
  c->kry_list.insert(c->kry_list.end(), boundary.begin(), boundary.end());
  if (c->d_kry_list) C8_HIP(hipFree(c->d_kry_list));
  c->d_kry_list = nullptr;
  c->kry_list_owned = -1;
  if (nown > 0) {
    C8_HIP(hipMalloc((void**)&c->d_kry_list, (size_t)nown * sizeof(int32_t)));
    C8_HIP(hipMemcpy(c->d_kry_list, c->kry_list.data(), (size_t)nown * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  c->kry_list_owned = nown;
  return C8_OK;
}

// greedy colouring of the first n nodes of a graph over their sub-graph: nodes in ascending id, each takes the smallest
// colour no already-coloured neighbour has; nodes color_nodes[color_ptr[k] .. color_ptr[k + 1]) have colour k, ascending
void color_graph(int n, std::vector<int32_t> const& gp, std::vector<int32_t> const& ga, std::vector<int32_t>* color_ptr,
                 std::vector<int32_t>* color_nodes) {
  std::vector<int32_t> color(std::max(n, 0), -1), used;
  int nc = 0;
  for (int i = 0; i < n; ++i) {
    used.assign(nc + 1, 0);
    for (int32_t k = gp[i]; k < gp[i + 1]; ++k) {
      int32_t const j = ga[k];
      if (j < i && color[j] >= 0) used[color[j]] = 1;  // (j < i < n: already coloured, and owned)
    }
    int col = 0;
    while (used[col]) ++col;
    color[i] = col;
    nc = std::max(nc, col + 1);
  }
  color_ptr->assign(nc + 1, 0);
  for (int i = 0; i < n; ++i) (*color_ptr)[color[i] + 1]++;
  for (int k = 0; k < nc; ++k) (*color_ptr)[k + 1] += (*color_ptr)[k];
  color_nodes->assign(std::max(n, 0), 0);
  std::vector<int32_t> at(color_ptr->begin(), color_ptr->end() - 1);
  for (int i = 0; i < n; ++i) (*color_nodes)[at[color[i]]++] = i;
}

// the colour lists of the Gauss-Seidel sweeps from the host graph (greedy, ascending node id, smallest free colour) and
// their device mirror: all nodes, or the owned nodes over the owned sub-graph when a halo is attached
int build_colors(c8_ctx* c) {
  int const want = c->halo ? c8_halo_num_owned(c->halo) : -1;
  if (c->kry_colors_for == want) return C8_OK;
  int const n = c->halo ? want : c->mesh.nnodes;
  c->kry_colors_for = -2;
  color_graph(n, c->graph.nodeptr, c->graph.nodeadj, &c->kry_color_ptr, &c->kry_color_nodes);
  if (c->d_kry_colors) C8_HIP(hipFree(c->d_kry_colors));
  c->d_kry_colors = nullptr;
  if (n > 0) {
    C8_HIP(hipMalloc((void**)&c->d_kry_colors, (size_t)n * sizeof(int32_t)));
    C8_HIP(hipMemcpy(c->d_kry_colors, c->kry_color_nodes.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  c->kry_colors_for = want;
  return C8_OK;
}

// c8_krylov_precondition: the set-up and the true-residual kernel at x = 0 give the block inverses, r = v, its norm (the
// refusal of non-finite input) and the scalars of a fresh recurrence (alpha = 1, the work vector v = 0), with which the
// second preconditioner step of an iteration, s = r - alpha v = v, shat = M^-1 s, is the apply asked for.  Nothing is
// exchanged: with a halo the owned rows, and x = 0 in place of an import.
template <int ND, int NRES, int G>
int precondition(c8_ctx* c, const c8_system* sys, const double* const v[2], double* const y[2]) {
  constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  if ((c->kry_precond == C8_PRECOND_TWO_LEVEL_PARTS || c->kry_precond == C8_PRECOND_MULTILEVEL_PARTS) && c->halo)
    return precondition_parts<ND, NRES, G>(c, sys, v, y);  // (collective)
  bool const coarse = aggregation_kind(c->kry_precond), multilevel = multilevel_kind(c->kry_precond);
  bool const sgs = c->kry_precond == C8_PRECOND_BLOCK_SGS || coarse;
  Solve q{};
  q.c = c;
  q.nn = c->mesh.nnodes;
  int const nown = c->halo ? c8_halo_num_owned(c->halo) : q.nn;
  if (q.nn <= 0) return fail(C8_ERR_ARG, "c8_krylov_precondition: empty mesh");
  if (coarse) {
    int const rcc = multilevel ? multilevel_refusals(c, "c8_krylov_precondition") : coarse_refusals(c, "c8_krylov_precondition");
    if (rcc != C8_OK) return rcc;
    use_levels(q, multilevel);
  }
  if (nown <= 0) return C8_OK;
  size_t const n0 = (size_t)q.nn * ND, nu = (size_t)nown * ND, np_ = NRES == 2 ? (size_t)nown : (size_t)0;
  q.n = n0 + (NRES == 2 ? (size_t)q.nn : 0);
  q.nb_node = (nown + TPB - 1) / TPB;
  q.nb_upd = (int)std::min<size_t>((nu + np_ + TPB - 1) / TPB, (size_t)UPDATE_MAX_BLOCKS);
  int rc;
  if (sgs && (rc = build_colors(c)) != C8_OK) return rc;
  if ((rc = grow(&c->d_kry_minv, &c->kry_minv_n, (size_t)q.nn * NB * NB)) != C8_OK) return rc;
  if ((rc = grow(&c->d_kry_vec, &c->kry_vec_n, 9 * q.n)) != C8_OK) return rc;
  if ((rc = grow(&c->d_kry_part, &c->kry_part_n, 2 * (size_t)std::max(q.nb_node, q.nb_upd))) != C8_OK) return rc;
  if (!c->d_kry_scalars) C8_HIP(hipMalloc(&c->d_kry_scalars, sizeof(KryScalars)));
  q.A = Blocks{sys->A[0][0], sys->A[0][1], sys->A[1][0], sys->A[1][1]};
  double* vec = c->d_kry_vec;
  q.x = vec, q.r = vec + q.n, q.rhat = vec + 2 * q.n, q.p = vec + 3 * q.n, q.v = vec + 4 * q.n, q.s = vec + 5 * q.n;
  q.t = vec + 6 * q.n, q.phat = vec + 7 * q.n, q.shat = vec + 8 * q.n;
  q.part = c->d_kry_part;
  q.minv = c->d_kry_minv;
  q.S = (KryScalars*)c->d_kry_scalars;
  hipStream_t const st = c->stream;
  KryScalars h{};
  h.bad_node = INT_MAX;
  C8_HIP(hipMemcpyAsync(q.S, &h, sizeof(h), hipMemcpyHostToDevice, st));
  C8_HIP(hipMemsetAsync(vec, 0, 9 * q.n * sizeof(double), st));
  hipLaunchKernelGGL((k_setup<ND, NRES>), dim3(xcd_grid(q.nb_node)), dim3(TPB), 0, st, nown, q.nb_node, c->d_nodeptr, c->d_nodeadj, q.A, q.minv, q.S);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_true_residual_own<ND, NRES>), dim3(xcd_grid(q.nb_node)), dim3(TPB), 0, st, nown, q.nn, q.nb_node, c->d_nodeptr, c->d_nodeadj,
                     q.A, q.x, v[0], v[1], q.r, q.rhat, q.p, q.v, q.part);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_reduce<3>), dim3(1), dim3(TPB), 0, st, q.part, q.nb_node, 0., q.S);
  C8_HIP(hipGetLastError());
  if ((rc = read_scalars(q, &h)) != C8_OK) return rc;
  if (h.bad_node != INT_MAX)
    return fail(C8_ERR_ARG, "c8_krylov_precondition: the diagonal block of node " + std::to_string(h.bad_node) +
                            " is singular or not finite (node-block Jacobi preconditioner)");
  if (!std::isfinite(h.rr)) return fail(C8_ERR_ARG, "c8_krylov_precondition: the vector or the matrix is not finite");
  if (coarse && (rc = levels_setup<ND, NRES, G>(q, -1)) != C8_OK) return rc;
  if (sgs) {
    hipLaunchKernelGGL((k_vec<1>), dim3(q.nb_upd), dim3(TPB), 0, st, nu, np_, n0, q.r, q.v, q.s, q.shat, q.S);
    C8_HIP(hipGetLastError());
    if (coarse) C8_HIP((levels_apply<ND, NRES>(q, q.s, q.shat)));
    C8_HIP((launch_sgs<ND, NRES, G>(q, nown, q.s, q.shat, !coarse)));
  } else {
    hipLaunchKernelGGL((k_prec_own<ND, NRES, 1>), dim3(xcd_grid(q.nb_node)), dim3(TPB), 0, st, nown, q.nn, q.nb_node, q.minv, q.r, q.v, q.s, q.shat, q.S);
    C8_HIP(hipGetLastError());
  }
  C8_HIP(hipMemcpyAsync(y[0], q.shat, nu * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (NRES == 2) C8_HIP(hipMemcpyAsync(y[1], q.shat + n0, np_ * sizeof(double), hipMemcpyDeviceToDevice, st));
  return C8_OK;
}

}  // namespace

extern "C" {

static int solve(c8_ctx* c, const c8_system* sys, double* const dx[2], const c8_krylov_opts* opts, c8_krylov_info* info);
int c8_krylov_solve(c8_ctx* c, const c8_system* sys, double* const dx[2], const c8_krylov_opts* opts, c8_krylov_info* info) {
  int const rc = solve(c, sys, dx, opts, info);
  if (info) info->status = rc;  // whatever path returned: argument, device and unsupported errors included
  return rc;
}
static int solve(c8_ctx* c, const c8_system* sys, double* const dx[2], const c8_krylov_opts* opts, c8_krylov_info* info) {
  if (info) *info = c8_krylov_info{0, 0, C8_ERR_ARG, 0., 0.};
  if (!c || !sys || !dx) return fail(C8_ERR_ARG, "c8_krylov_solve: null argument");
  bool const two = c->nres == 2;
  if (!sys->A[0][0] || !sys->b[0] || !dx[0] || (two && (!sys->A[0][1] || !sys->A[1][0] || !sys->A[1][1] || !sys->b[1] || !dx[1])))
    return fail(C8_ERR_ARG, "c8_krylov_solve: null array in the system or in dx");
  if (c->halo) {
    if (info) info->status = C8_ERR_UNSUPPORTED;
    return fail(C8_ERR_UNSUPPORTED, "c8_krylov_solve: a halo is attached to the context; the multi-part solve (halo exchange inside A x, "
                                    "inner products summed over the parts) is c8_krylov_solve_parts, a collective call");
  }
  int const max_iters = (opts && opts->max_iters > 0) ? opts->max_iters : 20000;
  int const check_every = (opts && opts->check_every > 0) ? opts->check_every : 10;
  int const max_restarts = (opts && opts->max_restarts > 0) ? opts->max_restarts : 5;
  double const rel_tol = (opts && opts->rel_tol > 0.) ? opts->rel_tol : 1e-10;
  double const abs_tol = (opts && opts->abs_tol > 0.) ? opts->abs_tol : 0.;

  // (no halo here: a kind over parts is the kind of one part)
  bool const coarse = aggregation_kind(c->kry_precond), multilevel = multilevel_kind(c->kry_precond);
  bool const sgs = c->kry_precond == C8_PRECOND_BLOCK_SGS || coarse;
  Launchers L;
  if (!launchers_of(c, &L)) {
    if (info) info->status = C8_ERR_UNSUPPORTED;
    return fail(C8_ERR_UNSUPPORTED, "c8_krylov_solve: no kernels for this number of dimensions and residuals");
  }
  int const nb = c->ndims + (two ? 1 : 0);

  Solve q{};
  q.c = c;
  q.nn = c->mesh.nnodes;
  size_t const n0 = (size_t)q.nn * c->ndims;
  q.n = n0 + (two ? (size_t)q.nn : 0);
  q.nb_node = (q.nn + TPB - 1) / TPB;
  q.nb_spmv = (q.nn + TPB / L.group - 1) / (TPB / L.group);
  q.nb_upd = (int)std::min<size_t>((q.n + TPB - 1) / TPB, (size_t)UPDATE_MAX_BLOCKS);
  if (q.nn <= 0) return fail(C8_ERR_ARG, "c8_krylov_solve: empty mesh");
  int rc;
  if (coarse && (rc = multilevel ? multilevel_refusals(c, "c8_krylov_solve") : coarse_refusals(c, "c8_krylov_solve")) != C8_OK) {
    if (info) info->status = rc;
    return rc;
  }
  if (coarse) use_levels(q, multilevel);
  if (sgs && (rc = build_colors(c)) != C8_OK) return rc;
  if ((rc = grow(&c->d_kry_minv, &c->kry_minv_n, (size_t)q.nn * nb * nb)) != C8_OK) return rc;
  if ((rc = grow(&c->d_kry_vec, &c->kry_vec_n, 9 * q.n)) != C8_OK) return rc;
  if ((rc = grow(&c->d_kry_part, &c->kry_part_n, 2 * (size_t)std::max(q.nb_spmv, q.nb_upd))) != C8_OK) return rc;
  if (!c->d_kry_scalars) C8_HIP(hipMalloc(&c->d_kry_scalars, sizeof(KryScalars)));
  q.A = Blocks{sys->A[0][0], sys->A[0][1], sys->A[1][0], sys->A[1][1]};
  q.b0 = sys->b[0];
  q.b1 = sys->b[1];
  double* vec = c->d_kry_vec;
  q.x = vec, q.r = vec + q.n, q.rhat = vec + 2 * q.n, q.p = vec + 3 * q.n, q.v = vec + 4 * q.n, q.s = vec + 5 * q.n;
  q.t = vec + 6 * q.n, q.phat = vec + 7 * q.n, q.shat = vec + 8 * q.n;
  q.part = c->d_kry_part;
  q.minv = c->d_kry_minv;
  q.S = (KryScalars*)c->d_kry_scalars;

  // set-up: the inverses of the diagonal blocks, x = 0, r = rhat = b
  KryScalars h{};
  h.bad_node = INT_MAX;
  C8_HIP(hipMemcpyAsync(q.S, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
  C8_HIP(hipMemsetAsync(q.x, 0, q.n * sizeof(double), c->stream));
  if ((rc = L.setup(q)) != C8_OK) return rc;
  if ((rc = L.residual(q)) != C8_OK) return rc;
  if ((rc = read_scalars(q, &h)) != C8_OK) return rc;
  if (h.bad_node != INT_MAX)
    return fail(C8_ERR_ARG, "c8_krylov_solve: the diagonal block of node " + std::to_string(h.bad_node) +
                            " is singular or not finite (node-block Jacobi preconditioner)");
  double const b_norm = std::sqrt(h.rr);
  if (!std::isfinite(b_norm)) return fail(C8_ERR_ARG, "c8_krylov_solve: the right-hand side or the matrix is not finite");
  auto store = [&]() -> int {  // the iterate to the caller's arrays
    C8_HIP(hipMemcpyAsync(dx[0], q.x, n0 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (two) C8_HIP(hipMemcpyAsync(dx[1], q.x + n0, (size_t)q.nn * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return C8_OK;
  };
  if (b_norm == 0.) {
    if (info) *info = c8_krylov_info{0, 0, C8_OK, 0., 0.};
    return store();
  }
  double const tol = std::max(rel_tol * b_norm, abs_tol);
  q.tol2 = tol * tol;
  if (coarse && (rc = L.levels(q, -1)) != C8_OK) return rc;  // every A_l = P^T A P and the inverse of the last one for this matrix

  int restarts = 0, status = C8_NOT_CONVERGED;
  double true_norm = b_norm;
  while (true) {
    int const batch = std::min(check_every, max_iters - h.iters);
    for (int k = 0; k < batch; ++k)
      if ((rc = L.iteration(q)) != C8_OK) return rc;
    if ((rc = read_scalars(q, &h)) != C8_OK) return rc;
    if (h.stop == 0 && h.iters < max_iters) continue;
    // the recursive residual met the tolerance, the recurrence broke down, or the budget is spent: the TRUE residual
    // decides (this also resets the recurrence at the current iterate: r = b - A x, rhat = r)
    int const iters = h.iters;
    if ((rc = L.residual(q)) != C8_OK) return rc;
    if ((rc = read_scalars(q, &h)) != C8_OK) return rc;
    true_norm = std::sqrt(h.rr);
    if (true_norm <= tol) { status = C8_OK; break; }
    if (iters >= max_iters || restarts >= max_restarts || !std::isfinite(true_norm)) break;
    restarts++;
  }
  if (info) *info = c8_krylov_info{h.iters, restarts, status, b_norm, true_norm};
  if ((rc = store()) != C8_OK) return rc;
  if (status != C8_OK)
    return fail(C8_NOT_CONVERGED, "c8_krylov_solve: |b - A x| / |b| = " + std::to_string(true_norm / b_norm) + " after " +
                                  std::to_string(h.iters) + " iterations and " + std::to_string(restarts) + " restarts");
  return C8_OK;
}

int c8_krylov_linear_solve(void* user, const c8_system* sys, double* const dx[2]) {
  c8_krylov_user* u = (c8_krylov_user*)user;
  if (!u || !u->ctx) return fail(C8_ERR_ARG, "c8_krylov_linear_solve: user must point to a c8_krylov_user with its ctx set");
  int const rc = c8_krylov_solve(u->ctx, sys, dx, &u->opts, &u->info);
  u->total_iters += u->info.iters;
  u->solves += 1;
  return rc;
}

// ---- the solve over the parts of a multi-part mesh ---------------------------------------------------------------------
static int solve_parts(c8_ctx* c, const c8_system* sys, double* const dx[2], const c8_krylov_opts* opts, c8_krylov_info* info);
int c8_krylov_solve_parts(c8_ctx* c, const c8_system* sys, double* const dx[2], const c8_krylov_opts* opts, c8_krylov_info* info) {
  if (c && !c->halo) return c8_krylov_solve(c, sys, dx, opts, info);
  int const rc = solve_parts(c, sys, dx, opts, info);
  if (info) info->status = rc;
  return rc;
}
static int solve_parts(c8_ctx* c, const c8_system* sys, double* const dx[2], const c8_krylov_opts* opts, c8_krylov_info* info) {
  if (info) *info = c8_krylov_info{0, 0, C8_ERR_ARG, 0., 0.};
  // (argument errors are the caller's on every rank alike: they return before anything is exchanged)
  if (!c || !sys || !dx) return fail(C8_ERR_ARG, "c8_krylov_solve_parts: null argument");
  bool const two = c->nres == 2;
  if (!sys->A[0][0] || !sys->b[0] || !dx[0] || (two && (!sys->A[0][1] || !sys->A[1][0] || !sys->A[1][1] || !sys->b[1] || !dx[1])))
    return fail(C8_ERR_ARG, "c8_krylov_solve_parts: null array in the system or in dx");
  int const max_iters = (opts && opts->max_iters > 0) ? opts->max_iters : 20000;
  int const check_every = (opts && opts->check_every > 0) ? opts->check_every : 10;
  int const max_restarts = (opts && opts->max_restarts > 0) ? opts->max_restarts : 5;
  double const rel_tol = (opts && opts->rel_tol > 0.) ? opts->rel_tol : 1e-10;
  double const abs_tol = (opts && opts->abs_tol > 0.) ? opts->abs_tol : 0.;

  if (c->kry_precond == C8_PRECOND_TWO_LEVEL) return coarse_refusals(c, "c8_krylov_solve_parts");  // (a halo is attached: refused)
  if (c->kry_precond == C8_PRECOND_MULTILEVEL) return multilevel_refusals(c, "c8_krylov_solve_parts");
  bool const multi = c->kry_precond == C8_PRECOND_MULTILEVEL_PARTS, coarse = multi || c->kry_precond == C8_PRECOND_TWO_LEVEL_PARTS;
  bool const sgs = c->kry_precond == C8_PRECOND_BLOCK_SGS || coarse;
  PartsLaunchers L;
  if (!parts_launchers_of(c, &L)) return fail(C8_ERR_UNSUPPORTED, "c8_krylov_solve_parts: no kernels for this number of dimensions and residuals");
  int const nb = c->ndims + (two ? 1 : 0);

  Parts P;
  Solve& q = P.q;
  q = Solve{};
  q.c = c;
  q.nn = c->mesh.nnodes;
  if (q.nn <= 0) return fail(C8_ERR_ARG, "c8_krylov_solve_parts: empty mesh");
  P.h = c->halo;
  P.cm = c8_halo_comm(c->halo);
  P.rank = c8_halo_rank(c->halo);
  P.nranks = c8_halo_num_ranks(c->halo);
  P.nown = c8_halo_num_owned(c->halo);
  size_t const n0 = (size_t)q.nn * c->ndims;
  q.n = n0 + (two ? (size_t)q.nn : 0);
  int rc;
  // the aggregation kinds over parts: the tables of level 0, the replicated levels and the cap on the dense last level,
  // before anything is assembled or iterated (collective at the first use; every rank returns the same code)
  if (coarse && (rc = parts_levels_prepare(c, P, "c8_krylov_solve_parts", multi)) != C8_OK) return rc;
  // from here on every rank goes through the same sequence of collectives, whatever happens to it
  P.note(build_part_lists(c));
  if (sgs) P.note(build_colors(c));
  P.n_int = c->kry_n_interior;
  P.n_bnd = P.nown - P.n_int;
  int const npb = TPB / L.group;
  P.nb_own = (P.nown + TPB - 1) / TPB;
  P.nb_int = (P.n_int + npb - 1) / npb;
  P.nb_bnd = (P.n_bnd + npb - 1) / npb;
  P.nb_upd = (int)std::min<size_t>(std::max<size_t>(((size_t)P.nown * nb + TPB - 1) / TPB, 1), (size_t)UPDATE_MAX_BLOCKS);
  P.note(grow(&c->d_kry_minv, &c->kry_minv_n, (size_t)q.nn * nb * nb));
  P.note(grow(&c->d_kry_vec, &c->kry_vec_n, 9 * q.n));
  P.note(grow(&c->d_kry_part, &c->kry_part_n, 2 * (size_t)std::max(std::max(P.nb_int + P.nb_bnd, P.nb_upd), std::max(P.nb_own, 1))));
  if (!c->d_kry_scalars) P.hip(hipMalloc(&c->d_kry_scalars, sizeof(KryScalars)), "hipMalloc");
  if (!c->d_kry_sums) P.hip(hipMalloc((void**)&c->d_kry_sums, 64 * sizeof(double)), "hipMalloc");
  q.A = Blocks{sys->A[0][0], sys->A[0][1], sys->A[1][0], sys->A[1][1]};
  q.b0 = sys->b[0];
  q.b1 = sys->b[1];
  double* vec = c->d_kry_vec;
  q.x = vec, q.r = vec + q.n, q.rhat = vec + 2 * q.n, q.p = vec + 3 * q.n, q.v = vec + 4 * q.n, q.s = vec + 5 * q.n;
  q.t = vec + 6 * q.n, q.phat = vec + 7 * q.n, q.shat = vec + 8 * q.n;
  q.part = c->d_kry_part;
  q.minv = c->d_kry_minv;
  q.S = (KryScalars*)c->d_kry_scalars;
  P.list = c->d_kry_list;
  P.sums = c->d_kry_sums;
  P.x1 = two ? q.x + n0 : nullptr;
  P.phat1 = two ? q.phat + n0 : nullptr;
  P.shat1 = two ? q.shat + n0 : nullptr;

  // set-up: the inverses of the owned diagonal blocks (complete after the gather), x = 0, r = rhat = b
  KryScalars h{};
  h.bad_node = INT_MAX;
  if (!P.failed) P.hip(hipMemcpyAsync(q.S, &h, sizeof(h), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
  if (!P.failed) P.hip(hipMemsetAsync(vec, 0, 9 * q.n * sizeof(double), c->stream), "hipMemsetAsync");  // the copies' entries too
  L.setup(P);
  L.residual(P);
  if ((rc = parts_read(P, &h)) != C8_OK) return rc;
  {  // the bad-node decision over the ranks: slot r holds rank r's smallest bad node + 1
    std::vector<double> bad(P.nranks, 0.);
    if (h.bad_node != INT_MAX) bad[P.rank] = (double)h.bad_node + 1.;
    if ((rc = c8_comm_allreduce_sum(P.cm, bad.data(), P.nranks)) != C8_OK) return rc;
    for (int r = 0; r < P.nranks; ++r)
      if (bad[r] > 0.)
        return fail(C8_ERR_ARG, "c8_krylov_solve_parts: the diagonal block of node " + std::to_string((long long)bad[r] - 1) + " (local id) of rank " +
                                std::to_string(r) + " is singular or not finite (node-block Jacobi preconditioner)");
  }
  double const b_norm = std::sqrt(h.rr);  // of the global owned system: the same on every rank
  if (!std::isfinite(b_norm)) return fail(C8_ERR_ARG, "c8_krylov_solve_parts: the right-hand side or the matrix is not finite");
  auto store = [&]() -> int {
    C8_HIP(hipMemcpyAsync(dx[0], q.x, n0 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (two) C8_HIP(hipMemcpyAsync(dx[1], q.x + n0, (size_t)q.nn * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return C8_OK;
  };
  if (b_norm == 0.) {
    if (info) *info = c8_krylov_info{0, 0, C8_OK, 0., 0.};
    return store();
  }
  double const tol = std::max(rel_tol * b_norm, abs_tol);
  q.tol2 = tol * tol;
  if (coarse) {  // A_1 over all parts, every A_l below it and the inverse of the last one, the outcome agreed over the ranks
    L.levels(P, -1);
    if ((rc = parts_levels_agree(P, "c8_krylov_solve_parts")) != C8_OK) return rc;
  }

  int restarts = 0, status = C8_NOT_CONVERGED;
  double true_norm = b_norm;
  while (true) {
    int const batch = std::min(check_every, max_iters - h.iters);
    for (int k = 0; k < batch; ++k) L.iteration(P);
    if ((rc = parts_read(P, &h)) != C8_OK) return rc;
    if (h.stop == 0 && h.iters < max_iters) continue;
    int const iters = h.iters;
    L.residual(P);
    if ((rc = parts_read(P, &h)) != C8_OK) return rc;
    true_norm = std::sqrt(h.rr);
    if (true_norm <= tol) { status = C8_OK; break; }
    if (iters >= max_iters || restarts >= max_restarts || !std::isfinite(true_norm)) break;
    restarts++;
  }
  if (info) *info = c8_krylov_info{h.iters, restarts, status, b_norm, true_norm};
  if ((rc = store()) != C8_OK) return rc;
  if (status != C8_OK)
    return fail(C8_NOT_CONVERGED, "c8_krylov_solve_parts: |b - A x| / |b| = " + std::to_string(true_norm / b_norm) + " after " +
                                  std::to_string(h.iters) + " iterations and " + std::to_string(restarts) + " restarts");
  return C8_OK;
}

int c8_krylov_linear_solve_parts(void* user, const c8_system* sys, double* const dx[2]) {
  c8_krylov_user* u = (c8_krylov_user*)user;
  if (!u || !u->ctx) return fail(C8_ERR_ARG, "c8_krylov_linear_solve_parts: user must point to a c8_krylov_user with its ctx set");
  int const rc = c8_krylov_solve_parts(u->ctx, sys, dx, &u->opts, &u->info);
  u->total_iters += u->info.iters;
  u->solves += 1;
  return rc;
}

int c8_krylov_part_lists(c8_ctx* c, int32_t* num_interior, int32_t* num_boundary, const int32_t** nodes) {
  if (!c || !num_interior || !num_boundary || !nodes) return fail(C8_ERR_ARG, "c8_krylov_part_lists: null argument");
  if (!c->halo) return fail(C8_ERR_ARG, "c8_krylov_part_lists: no halo is attached to the context");
  int const rc = build_part_lists(c);
  if (rc != C8_OK) return rc;
  *num_interior = c->kry_n_interior;
  *num_boundary = (int32_t)c->kry_list.size() - c->kry_n_interior;
  *nodes = c->kry_list.data();
  return C8_OK;
}

int c8_krylov_set_preconditioner(c8_ctx* c, int kind, int sweeps) {
  if (!c) return fail(C8_ERR_ARG, "c8_krylov_set_preconditioner: null context");
  if (c->gather_pending) return fail(C8_ERR_ARG, "c8_krylov_set_preconditioner: a staged assembly is waiting for c8_gather_finish");
  if (kind != C8_PRECOND_BLOCK_JACOBI && kind != C8_PRECOND_BLOCK_SGS && kind != C8_PRECOND_TWO_LEVEL && kind != C8_PRECOND_MULTILEVEL &&
      kind != C8_PRECOND_TWO_LEVEL_PARTS && kind != C8_PRECOND_MULTILEVEL_PARTS)
    return fail(C8_ERR_ARG, "c8_krylov_set_preconditioner: unknown preconditioner " + std::to_string(kind));
  c->kry_precond = kind;
  c->kry_sweeps = sweeps > 0 ? sweeps : 1;
  return C8_OK;
}

int c8_krylov_get_preconditioner(const c8_ctx* c) {
  if (!c) return fail(C8_ERR_ARG, "c8_krylov_get_preconditioner: null context");
  return c->kry_precond;
}

int c8_krylov_colors(c8_ctx* c, int32_t* num_colors, const int32_t** color_ptr, const int32_t** nodes) {
  if (!c || !num_colors || !color_ptr || !nodes) return fail(C8_ERR_ARG, "c8_krylov_colors: null argument");
  int const rc = build_colors(c);
  if (rc != C8_OK) return rc;
  *num_colors = (int32_t)c->kry_color_ptr.size() - 1;
  *color_ptr = c->kry_color_ptr.data();
  *nodes = c->kry_color_nodes.data();
  return C8_OK;
}

int c8_krylov_aggregates(c8_ctx* c, int32_t* num_aggregates, const int32_t** aggregate_of_node) {
  if (!c || !num_aggregates || !aggregate_of_node) return fail(C8_ERR_ARG, "c8_krylov_aggregates: null argument");
  if (c->halo && (c->kry_precond == C8_PRECOND_TWO_LEVEL_PARTS || c->kry_precond == C8_PRECOND_MULTILEVEL_PARTS)) {  // this rank's, by local id (collective at the first use)
    Parts P = parts_of(c);
    int const rcp = parts_aggregates(c, P);  // (reported above the cap of the coarse solve too)
    if (rcp != C8_OK) return rcp;
    *num_aggregates = c->kry_pc_nagg;
    *aggregate_of_node = c->kry_pc_agg_of.data();
    return C8_OK;
  }
  if (c->halo) return coarse_refusals(c, "c8_krylov_aggregates");
  if (c->mesh.nnodes <= 0) return fail(C8_ERR_ARG, "c8_krylov_aggregates: empty mesh");
  int const rc = build_aggregates(c);  // (reported above the cap of the coarse solve too)
  if (rc != C8_OK) return rc;
  *num_aggregates = c->kry_nagg;
  *aggregate_of_node = c->kry_agg_of.data();
  return C8_OK;
}

int c8_krylov_aggregate_base(c8_ctx* c, int32_t* base, int32_t* total_aggregates) {
  if (!c || !base || !total_aggregates) return fail(C8_ERR_ARG, "c8_krylov_aggregate_base: null argument");
  if (!c->halo) {  // one part: its aggregates are all there are
    if (c->mesh.nnodes <= 0) return fail(C8_ERR_ARG, "c8_krylov_aggregate_base: empty mesh");
    int const rc = build_aggregates(c);
    if (rc != C8_OK) return rc;
    *base = 0;
    *total_aggregates = c->kry_nagg;
    return C8_OK;
  }
  if (c->kry_precond != C8_PRECOND_TWO_LEVEL_PARTS && c->kry_precond != C8_PRECOND_MULTILEVEL_PARTS)
    return fail(C8_ERR_UNSUPPORTED, "c8_krylov_aggregate_base: with a halo attached to the context only C8_PRECOND_TWO_LEVEL_PARTS and "
                                    "C8_PRECOND_MULTILEVEL_PARTS have aggregates");
  Parts P = parts_of(c);
  int const rc = parts_aggregates(c, P);
  if (rc != C8_OK) return rc;
  if (c->kry_pc_total > INT_MAX) return fail(C8_ERR_UNSUPPORTED, "c8_krylov_aggregate_base: more than 2^31 aggregates");
  *base = (int32_t)c->kry_pc_base;
  *total_aggregates = (int32_t)c->kry_pc_total;
  return C8_OK;
}

// The dense copy of A_level of a list of one part: the code behind c8_krylov_level_matrix (multi: the levels of
// C8_PRECOND_MULTILEVEL) and c8_krylov_coarse_matrix (the two-level list, level 1)
static int level_matrix(c8_ctx* c, const c8_system* sys, bool multi, int32_t level, int32_t* n_level, double* out_host, char const* who) {
  int rc = multi ? multilevel_refusals(c, who) : coarse_refusals(c, who);
  if (rc != C8_OK) return rc;
  std::vector<c8_kry_level> const& lv = multi ? c->kry_levels : c->kry_agg_levels;
  int const nc = coarse_columns(c);
  if (multi && (rc = level_matrix_refusals(lv, level, nc)) != C8_OK) return rc;
  *n_level = lv[level - 1].n * nc;
  if (!out_host) return C8_OK;
  Launchers L;
  if (!launchers_of(c, &L)) return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": no kernels for this number of dimensions and residuals");
  Solve q{};
  q.c = c;
  q.nn = c->mesh.nnodes;
  q.A = Blocks{sys->A[0][0], sys->A[0][1], sys->A[1][0], sys->A[1][1]};
  use_levels(q, multi);
  if ((rc = L.levels(q, level)) != C8_OK) return rc;
  std::vector<double> blocks;
  C8_HIP(level_copy_start(c, lv, level, nc, out_host, &blocks));
  C8_HIP(hipStreamSynchronize(c->stream));
  level_copy_finish(lv, level, nc, out_host, blocks);
  return C8_OK;
}

int c8_krylov_coarse_matrix(c8_ctx* c, const c8_system* sys, int32_t* n_coarse, double* out_host) {
  if (!c || !sys || !n_coarse) return fail(C8_ERR_ARG, "c8_krylov_coarse_matrix: null argument");
  bool const two = c->nres == 2;
  if (!sys->A[0][0] || (two && (!sys->A[0][1] || !sys->A[1][0] || !sys->A[1][1])))
    return fail(C8_ERR_ARG, "c8_krylov_coarse_matrix: null array in the system");
  // level 1 of the two-level list, whichever kind is selected; over parts collective: the global A_c, the same on every rank
  if (c->halo && (c->kry_precond == C8_PRECOND_TWO_LEVEL_PARTS || c->kry_precond == C8_PRECOND_MULTILEVEL_PARTS))
    return parts_level_matrix(c, sys, false, 1, n_coarse, out_host, "c8_krylov_coarse_matrix");
  return level_matrix(c, sys, false, 1, n_coarse, out_host, "c8_krylov_coarse_matrix");
}

int c8_krylov_set_multilevel(c8_ctx* c, int32_t coarse_max, int32_t max_levels) {
  if (!c) return fail(C8_ERR_ARG, "c8_krylov_set_multilevel: null context");
  if (c->gather_pending) return fail(C8_ERR_ARG, "c8_krylov_set_multilevel: a staged assembly is waiting for c8_gather_finish");
  if (max_levels == 1) return fail(C8_ERR_ARG, "c8_krylov_set_multilevel: max_levels counts level 0 and must be at least 2");
  c->kry_ml_coarse_max = coarse_max > 0 ? coarse_max : 0;
  c->kry_ml_max_levels = max_levels > 0 ? max_levels : 0;
  c->kry_ml_built = false;  // the levels are rebuilt at the next use, of one part ...
  c->kry_pl_for = -1;       // ... and over parts
  return C8_OK;
}

int c8_krylov_levels(c8_ctx* c, int32_t* num_levels) {
  if (!c || !num_levels) return fail(C8_ERR_ARG, "c8_krylov_levels: null argument");
  if (c->halo && c->kry_precond == C8_PRECOND_MULTILEVEL_PARTS) {  // collective at the first use (reported above the cap too)
    Parts P = parts_of(c);
    int const rcp = parts_levels_build(c, P, "c8_krylov_levels", true);
    if (rcp != C8_OK) return rcp;
    *num_levels = (int32_t)c->kry_pl_levels.size() + 1;
    return C8_OK;
  }
  if (c->halo) return multilevel_refusals(c, "c8_krylov_levels");
  if (c->mesh.nnodes <= 0) return fail(C8_ERR_ARG, "c8_krylov_levels: empty mesh");
  int const rc = build_levels(c);  // (reported with a last level above the cap too)
  if (rc != C8_OK) return rc;
  *num_levels = (int32_t)c->kry_levels.size() + 1;
  return C8_OK;
}

int c8_krylov_level(c8_ctx* c, int32_t level, int32_t* num_nodes, const int32_t** aggregate_of_node, int32_t* num_colors,
                    const int32_t** color_ptr, const int32_t** nodes) {
  if (!c || !num_nodes || !aggregate_of_node || !num_colors || !color_ptr || !nodes) return fail(C8_ERR_ARG, "c8_krylov_level: null argument");
  bool const parts = c->halo && c->kry_precond == C8_PRECOND_MULTILEVEL_PARTS;  // the rank's own level 0, the replicated levels below
  if (c->halo && !parts) return multilevel_refusals(c, "c8_krylov_level");
  if (c->mesh.nnodes <= 0) return fail(C8_ERR_ARG, "c8_krylov_level: empty mesh");
  int rc;
  if (parts) {  // (collective at the first use)
    Parts P = parts_of(c);
    rc = parts_levels_build(c, P, "c8_krylov_level", true);
  } else rc = build_levels(c);
  if (rc != C8_OK) return rc;
  std::vector<c8_kry_level> const& lv = parts ? c->kry_pl_levels : c->kry_levels;
  int const nl = (int)lv.size();
  if (level < 0 || level > nl) return fail(C8_ERR_ARG, "c8_krylov_level: level " + std::to_string(level) + " of " + std::to_string(nl + 1));
  if (level == 0) {
    if ((rc = build_colors(c)) != C8_OK) return rc;
    *num_nodes = parts ? c8_halo_num_owned(c->halo) : c->mesh.nnodes;
    *aggregate_of_node = parts ? c->kry_pc_agg_of.data() : c->kry_agg_of.data();
    *num_colors = (int32_t)c->kry_color_ptr.size() - 1;
    *color_ptr = c->kry_color_ptr.data();
    *nodes = c->kry_color_nodes.data();
    return C8_OK;
  }
  c8_kry_level const& L = lv[level - 1];
  bool const last = level == nl;  // dense: no aggregates and no sweeps
  *num_nodes = L.n;
  *aggregate_of_node = last ? nullptr : L.agg_of.data();
  *num_colors = last ? 0 : (int32_t)L.color_ptr.size() - 1;
  *color_ptr = last ? nullptr : L.color_ptr.data();
  *nodes = last ? nullptr : L.color_nodes.data();
  return C8_OK;
}

int c8_krylov_level_matrix(c8_ctx* c, const c8_system* sys, int32_t level, int32_t* n_level, double* out_host) {
  if (!c || !sys || !n_level) return fail(C8_ERR_ARG, "c8_krylov_level_matrix: null argument");
  bool const two = c->nres == 2;
  if (!sys->A[0][0] || (two && (!sys->A[0][1] || !sys->A[1][0] || !sys->A[1][1])))
    return fail(C8_ERR_ARG, "c8_krylov_level_matrix: null array in the system");
  if (c->halo && c->kry_precond == C8_PRECOND_MULTILEVEL_PARTS)
    return parts_level_matrix(c, sys, true, level, n_level, out_host, "c8_krylov_level_matrix");  // (collective)
  return level_matrix(c, sys, true, level, n_level, out_host, "c8_krylov_level_matrix");
}

int c8_krylov_precondition(c8_ctx* c, const c8_system* sys, const double* const v[2], double* const y[2]) {
  if (!c || !sys || !v || !y) return fail(C8_ERR_ARG, "c8_krylov_precondition: null argument");
  bool const two = c->nres == 2;
  if (!sys->A[0][0] || !v[0] || !y[0] || (two && (!sys->A[0][1] || !sys->A[1][0] || !sys->A[1][1] || !v[1] || !y[1])))
    return fail(C8_ERR_ARG, "c8_krylov_precondition: null array in the system, in v or in y");
  if (c->ndims == 3 && two) return precondition<3, 2, 16>(c, sys, v, y);
  if (c->ndims == 2 && two) return precondition<2, 2, 8>(c, sys, v, y);
  if (c->ndims == 2 && !two) return precondition<2, 1, 8>(c, sys, v, y);
  return fail(C8_ERR_UNSUPPORTED, "c8_krylov_precondition: no kernels for this number of dimensions and residuals");
}

}  // extern "C"

void c8_krylov_release(c8_ctx* c) {
  free_levels(c);
  free_level_list(c->kry_pl_levels);  // (kry_agg_levels and kry_pc_levels hold no device buffers)
  if (c->kry_rocblas) (void)rocblas_destroy_handle((rocblas_handle)c->kry_rocblas);
  c->kry_rocblas = nullptr;
}
