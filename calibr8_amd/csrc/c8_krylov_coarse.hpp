// c8_krylov_coarse.hpp -- the coarse level of the two-level preconditioner of the device solve (C8_PRECOND_TWO_LEVEL in
// include/c8.h).  Included by c8_krylov.hip inside its unnamed namespace, after the kernels of the
// one-level solve (TPB, Blocks, KryScalars, xcd_block, grow, Solve; rocSOLVER's header is included there).
//
//   aggregates   three passes over the host node graph, once per context (build_aggregates); the device mirror holds the
//                aggregate of every node, the node list and the neighbour list of every aggregate, and for every entry of
//                the node graph the position of the column's aggregate in the neighbour list of the row's aggregate
//   P            never stored: aggregate id, the node's offset from the aggregate's centroid, the constrained-row flags
//   set-up       k_constrained (flags) -> k_galerkin (A_c = P^T A P, dense, row-major, leading dimension lda) ->
//                coarse_invert (in place) -> k_coarse_check; every solve, because the matrix changes every Newton iteration
//   apply        k_restrict (r_c = P^T v) -> k_coarse_apply (e = A_c^-1 r_c) -> k_prolong (x = P e), then the sweeps of
//                k_sgs_color started from this x
// Every sum has a fixed order and no kernel uses a floating-point atomic.  The multilevel kind (c8_krylov_multilevel.hpp) uses
// the same aggregation (aggregate_graph) on every level, these kernels between levels 0 and 1, and the dense solve on its last level.
constexpr int COARSE_CAP = 8192;          // n_coarse of the dense coarse solve: a 512 MB inverse
constexpr size_t GALERKIN_LDS = 64 * 1024;  // largest tile of k_galerkin

template <int ND, int NRES>
struct CoarseDims {
  static constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  static constexpr int NROT = ND == 3 ? 3 : 1;
  static constexpr int NC = ND + NROT + (NRES == 2 ? 1 : 0);  // translations, rotations, constant p
};

// entry (equation r of the node, column c of its aggregate) of P before the constrained-row flags; d = x_i - centroid.
// Columns: ND translations, the rotations e_m x d (3-D) or (-d_y, d_x) (2-D), constant p.  Called with r a compile-time
// constant (unrolled loops), so that d is indexed by constants.
template <int ND, int NRES>
__device__ __forceinline__ double p_entry(int r, int c, double const* d) {
  constexpr int NROT = ND == 3 ? 3 : 1;
  if (c < ND) return r == c ? 1. : 0.;
  if (c < ND + NROT) {
    if (r >= ND) return 0.;
    if (ND == 2) return r == 0 ? -d[1] : d[0];
    int const m = c - ND;  // (e_m x d)_r = eps(r, m, k) d_k
    if (m == r) return 0.;
    return m == (r + 1) % 3 ? d[(r + 2) % 3] : -d[(r + 1) % 3];
  }
  return r == ND ? 1. : 0.;
}

// ---- constrained rows: bit r of flags[node] is set when every off-diagonal entry of the node's equation r is exactly 0
// in all blocks (the rows c8_apply_dirichlet leaves).  Lane mapping of k_spmv, an OR over the node's G lanes.
template <int ND, int NRES, int G>
__global__ void __launch_bounds__(TPB) k_constrained(int nn, int nblocks, int32_t const* __restrict__ nodeptr, int32_t const* __restrict__ nodeadj,
                                                     Blocks A, int32_t* __restrict__ flags) {
  constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  constexpr int NPB = TPB / G;
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const node = lb * NPB + threadIdx.x / G, lane = threadIdx.x % G;
  int nz = 0;  // bit r: equation r has a non-zero off-diagonal entry
  if (node < nn) {
    int64_t const np = nodeptr[node];
    int const deg = (int)(nodeptr[node + 1] - np);
    for (int k = lane; k < deg; k += G) {
      bool const self = nodeadj[np + k] == node;
#pragma unroll
      for (int ri = 0; ri < ND; ++ri) {
        double const* row = A.A00 + np * ND * ND + (int64_t)ri * deg * ND + (int64_t)k * ND;
#pragma unroll
        for (int e = 0; e < ND; ++e)
          if (!(self && e == ri) && row[e] != 0.) nz |= 1 << ri;
        if (NRES == 2 && A.A01[np * ND + (int64_t)ri * deg + k] != 0.) nz |= 1 << ri;
      }
      if (NRES == 2) {
        double const* row = A.A10 + np * ND + (int64_t)k * ND;
#pragma unroll
        for (int e = 0; e < ND; ++e)
          if (row[e] != 0.) nz |= 1 << ND;
        if (!self && A.A11[np + k] != 0.) nz |= 1 << ND;
      }
    }
  }
  for (int o = G / 2; o > 0; o >>= 1) nz |= __shfl_xor(nz, o, G);
  if (node < nn && lane == 0) flags[node] = ~nz & ((1 << NB) - 1);
}

struct AggTables {  // device mirror of the aggregates (c8_ctx::d_kry_agg and its offsets)
  int32_t const *agg_of, *ptr, *nodes, *nbr_ptr, *nbr, *slot;
  double const* off;  // [nnodes][ND]: x_i - centroid of the node's aggregate
  int32_t const* flags;
};

// ---- A_c = P^T A P.  One workgroup owns the block row of aggregate I: NC rows of A_c, its tile in LDS has one NC x NC
// block per neighbouring aggregate (tile[r][slot * NC + c], neighbours in ascending id).  A work item owns the tile columns
// q = slot * NC + c, q = thread, thread + TPB, ...: it walks the aggregate's nodes in ascending id and each node's graph
// row in column order, and for the entries whose column node lies in the aggregate of `slot` adds P_i^T (A_ij P_j[:, c])
// to its NC tile entries -- one owner per entry, the sum of an entry in one fixed order.  A column of P that is zero (every
// row of the mode constrained, or a one-node aggregate's rotation) gets a unit diagonal.  The tile is then written to
// A_c, every entry once; the other entries of A_c are the zeros of the memset before the launch.  SPARSE (the multilevel
// kind, c8_krylov_multilevel.hpp): the tile goes to the block-sparse A_1 instead, the NC x NC block of neighbour `slot` to
// graph entry nbr_ptr[I] + slot of level 1; the sums are the same.
template <int ND, int NRES, bool SPARSE = false>
__global__ void __launch_bounds__(TPB) k_galerkin(AggTables T, int32_t const* __restrict__ nodeptr, int32_t const* __restrict__ nodeadj, Blocks A,
                                                  double* __restrict__ Ac, int lda) {
  constexpr int NB = CoarseDims<ND, NRES>::NB, NC = CoarseDims<ND, NRES>::NC;
  extern __shared__ double tile[];
  int const I = blockIdx.x;
  int const a0 = T.ptr[I], a1 = T.ptr[I + 1], b0 = T.nbr_ptr[I];
  int const W = (T.nbr_ptr[I + 1] - b0) * NC;
  for (int q = threadIdx.x; q < W; q += TPB) {
    int const sl = q / NC, c = q % NC;
    bool const own = T.nbr[b0 + sl] == I;
    bool colnz = false;
    double acc[NC];
#pragma unroll
    for (int r = 0; r < NC; ++r) acc[r] = 0.;
    for (int a = a0; a < a1; ++a) {
      int const node = T.nodes[a];
      int const fi = T.flags[node];
      double di[ND];
#pragma unroll
      for (int e = 0; e < ND; ++e) di[e] = T.off[(size_t)node * ND + e];
      if (own) {
#pragma unroll
        for (int e = 0; e < NB; ++e)
          if (!((fi >> e) & 1) && p_entry<ND, NRES>(e, c, di) != 0.) colnz = true;
      }
      int64_t const np = nodeptr[node];
      int const deg = (int)(nodeptr[node + 1] - np);
      for (int k = 0; k < deg; ++k) {
        if (T.slot[np + k] != sl) continue;
        int const cn = nodeadj[np + k];
        int const fj = T.flags[cn];
        double dj[ND], pj[NB], w[NB];
#pragma unroll
        for (int e = 0; e < ND; ++e) dj[e] = T.off[(size_t)cn * ND + e];
#pragma unroll
        for (int e = 0; e < NB; ++e) pj[e] = ((fj >> e) & 1) ? 0. : p_entry<ND, NRES>(e, c, dj);
#pragma unroll
        for (int ri = 0; ri < ND; ++ri) {
          double const* row = A.A00 + np * ND * ND + (int64_t)ri * deg * ND + (int64_t)k * ND;
          double s = 0.;
#pragma unroll
          for (int e = 0; e < ND; ++e) s += row[e] * pj[e];
          if (NRES == 2) s += A.A01[np * ND + (int64_t)ri * deg + k] * pj[NB - 1];
          w[ri] = s;
        }
        if (NRES == 2) {
          double const* row = A.A10 + np * ND + (int64_t)k * ND;
          double s = 0.;
#pragma unroll
          for (int e = 0; e < ND; ++e) s += row[e] * pj[e];
          w[NB - 1] = s + A.A11[np + k] * pj[NB - 1];
        }
#pragma unroll
        for (int r = 0; r < NC; ++r) {
          double s = 0.;
#pragma unroll
          for (int ri = 0; ri < NB; ++ri) s += (((fi >> ri) & 1) ? 0. : p_entry<ND, NRES>(ri, r, di)) * w[ri];
          acc[r] += s;
        }
      }
    }
    bool const unit = own && !colnz;
#pragma unroll
    for (int r = 0; r < NC; ++r) tile[r * W + q] = (unit && r == c) ? 1. : acc[r];
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < NC * W; idx += TPB) {
    int const r = idx / W, q = idx % W;
    if (SPARSE) Ac[((size_t)(b0 + q / NC) * NC + r) * NC + q % NC] = tile[idx];
    else Ac[(size_t)(I * NC + r) * lda + (size_t)T.nbr[b0 + q / NC] * NC + q % NC] = tile[idx];
  }
}

// ---- r_c = P^T v: one wavefront per aggregate, lane l takes the nodes l, l + 64, ... of the aggregate's list, then a
// fixed butterfly over the lanes
template <int ND, int NRES>
__global__ void __launch_bounds__(TPB) k_restrict(int nagg, AggTables T, int nn, double const* __restrict__ v, double* __restrict__ rc,
                                                  KryScalars const* S) {
  constexpr int NB = CoarseDims<ND, NRES>::NB, NC = CoarseDims<ND, NRES>::NC;
  if (S->stop) return;
  int const I = blockIdx.x * (TPB / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
  size_t const n0 = (size_t)nn * ND;
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.;
  if (I < nagg) {
    for (int a = T.ptr[I] + lane; a < T.ptr[I + 1]; a += 64) {
      int const node = T.nodes[a];
      int const f = T.flags[node];
      double d[ND], vv[NB];
#pragma unroll
      for (int e = 0; e < ND; ++e) d[e] = T.off[(size_t)node * ND + e];
#pragma unroll
      for (int e = 0; e < NB; ++e) vv[e] = ((f >> e) & 1) ? 0. : v[e < ND ? (size_t)node * ND + e : n0 + node];
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < NB; ++e) acc[c] += p_entry<ND, NRES>(e, c, d) * vv[e];
    }
  }
#pragma unroll
  for (int c = 0; c < NC; ++c)
    for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o);
  if (I < nagg && lane == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) rc[(size_t)I * NC + c] = acc[c];
  }
}

// ---- e = A_c^-1 r_c, the dense row-major inverse: one wavefront per row, 16-byte loads (lda is even, the padding entries
// of a row and of r_c are zero), a fixed butterfly over the lanes
__global__ void __launch_bounds__(TPB) k_coarse_apply(int n, int lda, double const* __restrict__ Ainv, double const* __restrict__ rc,
                                                      double* __restrict__ e, KryScalars const* S) {
  if (S->stop) return;
  int const row = blockIdx.x * (TPB / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
  double s = 0.;
  if (row < n) {
    double2 const* a = (double2 const*)(Ainv + (size_t)row * lda);
    double2 const* x = (double2 const*)rc;
    for (int j = lane; j < lda / 2; j += 64) {
      double2 const av = a[j], xv = x[j];
      s += av.x * xv.x;
      s += av.y * xv.y;
    }
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (row < n && lane == 0) e[row] = s;
}

// ---- x = P e, one work item per node: the start of the Gauss-Seidel sweeps in the place of x = 0
template <int ND, int NRES>
__global__ void __launch_bounds__(TPB) k_prolong(int nn, int nblocks, AggTables T, double const* __restrict__ e, double* __restrict__ x,
                                                 KryScalars const* S) {
  constexpr int NB = CoarseDims<ND, NRES>::NB, NC = CoarseDims<ND, NRES>::NC;
  if (S->stop) return;
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const node = lb * TPB + threadIdx.x;
  if (node >= nn) return;
  int const f = T.flags[node];
  double const* ea = e + (size_t)T.agg_of[node] * NC;
  double d[ND], ev[NC];
#pragma unroll
  for (int k = 0; k < ND; ++k) d[k] = T.off[(size_t)node * ND + k];
#pragma unroll
  for (int c = 0; c < NC; ++c) ev[c] = ea[c];
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    double s = 0.;
#pragma unroll
    for (int c = 0; c < NC; ++c) s += p_entry<ND, NRES>(r, c, d) * ev[c];
    x[r < ND ? (size_t)node * ND + r : (size_t)nn * ND + node] = ((f >> r) & 1) ? 0. : s;
  }
}

// ---- the smallest row of the inverse with an entry that is not finite (INT_MAX: none); an integer atomic
__global__ void __launch_bounds__(TPB) k_coarse_check(int n, int lda, double const* __restrict__ Ainv, int32_t* bad) {
  size_t const total = (size_t)n * lda;
  int worst = INT_MAX;
  for (size_t i = blockIdx.x * (size_t)TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB)
    if (!finite_d(Ainv[i])) worst = min(worst, (int)(i / lda));
  if (worst != INT_MAX) atomicMin(bad, worst);
}

// ---- host side ----------------------------------------------------------------------------------------------------------

inline int coarse_columns(c8_ctx const* c) { return c->ndims + (c->ndims == 3 ? 3 : 1) + (c->nres == 2 ? 1 : 0); }

// The aggregates of a graph of n nodes (rows sorted, a node among its own neighbours) with positions x[n][3]:
//   pass 1  nodes in ascending id: a node whose whole graph row (itself included) is free opens an aggregate of that row
//   pass 2  nodes in ascending id: a free node joins the pass-1 aggregate of its lowest-id neighbour that pass 1 aggregated
//   pass 3  nodes in ascending id: a node still free becomes an aggregate of its own
struct Aggregates {
  int nagg = 0, max_nbr = 0;                          // max_nbr: most neighbouring aggregates of one aggregate (itself included)
  std::vector<int32_t> agg, ptr, nodes, nbr_ptr, nbr, slot;
  std::vector<double> off;                            // [n][nd] node - centroid of its aggregate
  std::vector<double> centroid;                       // [nagg][3]
};
Aggregates aggregate_graph(int nn, int nd, std::vector<int32_t> const& gp, std::vector<int32_t> const& ga, double const* x) {
  Aggregates H;
  std::vector<int32_t>& agg = H.agg;
  agg.assign(nn, -1);
  int nagg = 0;
  for (int i = 0; i < nn; ++i) {
    bool free_row = true;
    for (int32_t k = gp[i]; k < gp[i + 1]; ++k) free_row = free_row && agg[ga[k]] < 0;
    if (!free_row) continue;
    for (int32_t k = gp[i]; k < gp[i + 1]; ++k) agg[ga[k]] = nagg;
    agg[i] = nagg++;
  }
  std::vector<int32_t> const first = agg;
  for (int i = 0; i < nn; ++i) {
    if (agg[i] >= 0) continue;
    for (int32_t k = gp[i]; k < gp[i + 1]; ++k)  // (rows are sorted: the first hit is the lowest id)
      if (first[ga[k]] >= 0) { agg[i] = first[ga[k]]; break; }
  }
  for (int i = 0; i < nn; ++i)
    if (agg[i] < 0) agg[i] = nagg++;
  // node lists (ascending id), centroids, offsets
  std::vector<int32_t>&ptr = H.ptr, &nodes = H.nodes;
  ptr.assign(nagg + 1, 0), nodes.assign(nn, 0);
  for (int i = 0; i < nn; ++i) ptr[agg[i] + 1]++;
  for (int a = 0; a < nagg; ++a) ptr[a + 1] += ptr[a];
  {
    std::vector<int32_t> at(ptr.begin(), ptr.end() - 1);
    for (int i = 0; i < nn; ++i) nodes[at[agg[i]]++] = i;
  }
  H.off.assign((size_t)nn * nd, 0.);
  H.centroid.assign((size_t)nagg * 3, 0.);
  for (int a = 0; a < nagg; ++a)
    for (int d = 0; d < nd; ++d) {
      double sum = 0.;
      for (int k = ptr[a]; k < ptr[a + 1]; ++k) sum += x[(size_t)nodes[k] * 3 + d];
      double const mean = sum / (double)(ptr[a + 1] - ptr[a]);
      H.centroid[(size_t)a * 3 + d] = mean;
      for (int k = ptr[a]; k < ptr[a + 1]; ++k) H.off[(size_t)nodes[k] * nd + d] = x[(size_t)nodes[k] * 3 + d] - mean;
    }
  // neighbouring aggregates of every aggregate (ascending id, itself included) and the slot of every graph entry
  std::vector<int32_t>&nbr_ptr = H.nbr_ptr, &nbr = H.nbr, &slot = H.slot;
  std::vector<int32_t> where(nagg, -1);
  nbr_ptr.assign(nagg + 1, 0), slot.assign(ga.size(), 0);
  for (int a = 0; a < nagg; ++a) {
    size_t const lo = nbr.size();
    for (int k = ptr[a]; k < ptr[a + 1]; ++k)
      for (int32_t e = gp[nodes[k]]; e < gp[nodes[k] + 1]; ++e)
        if (where[agg[ga[e]]] != a) { where[agg[ga[e]]] = a; nbr.push_back(agg[ga[e]]); }
    std::sort(nbr.begin() + lo, nbr.end());
    nbr_ptr[a + 1] = (int32_t)nbr.size();
    H.max_nbr = std::max(H.max_nbr, (int)(nbr.size() - lo));
    for (int k = ptr[a]; k < ptr[a + 1]; ++k)
      for (int32_t e = gp[nodes[k]]; e < gp[nodes[k] + 1]; ++e)
        slot[e] = (int32_t)(std::lower_bound(nbr.begin() + lo, nbr.end(), agg[ga[e]]) - (nbr.begin() + lo));
  }
  H.nagg = nagg;
  return H;
}

// the device mirror of the aggregates: one buffer of int32 (agg_of, ptr, nodes, nbr_ptr, nbr, slot; at[k] = where each
// starts) and the offsets
int upload_aggregates(Aggregates const& H, int32_t** d_agg, size_t at[6], double** d_off) {
  std::vector<int32_t> pack;
  std::vector<int32_t> const* parts[6] = {&H.agg, &H.ptr, &H.nodes, &H.nbr_ptr, &H.nbr, &H.slot};
  for (int k = 0; k < 6; ++k) {
    at[k] = pack.size();
    pack.insert(pack.end(), parts[k]->begin(), parts[k]->end());
  }
  *d_agg = nullptr, *d_off = nullptr;
  C8_HIP(hipMalloc((void**)d_agg, pack.size() * sizeof(int32_t)));
  C8_HIP(hipMemcpy(*d_agg, pack.data(), pack.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  C8_HIP(hipMalloc((void**)d_off, H.off.size() * sizeof(double)));
  C8_HIP(hipMemcpy(*d_off, H.off.data(), H.off.size() * sizeof(double), hipMemcpyHostToDevice));
  return C8_OK;
}

// The aggregates of the context's node graph, once per context, and their device mirror; the graph and the positions of
// level 1 (the neighbour lists and the centroids) stay on the host for the multilevel kind.
int build_aggregates(c8_ctx* c) {
  if (c->kry_nagg >= 0) return C8_OK;
  int const nn = c->mesh.nnodes;
  Aggregates H = aggregate_graph(nn, c->ndims, c->graph.nodeptr, c->graph.nodeadj, c->mesh.coords.data());
  if (c->d_kry_agg) C8_HIP(hipFree(c->d_kry_agg));
  if (c->d_kry_agg_off) C8_HIP(hipFree(c->d_kry_agg_off));
  if (c->d_kry_cflags) C8_HIP(hipFree(c->d_kry_cflags));
  c->d_kry_agg = nullptr, c->d_kry_agg_off = nullptr, c->d_kry_cflags = nullptr;
  int const rc = upload_aggregates(H, &c->d_kry_agg, c->kry_agg_at, &c->d_kry_agg_off);
  if (rc != C8_OK) return rc;
  C8_HIP(hipMalloc((void**)&c->d_kry_cflags, (size_t)nn * sizeof(int32_t)));
  c->kry_agg_of = std::move(H.agg);
  c->kry_agg_nbr_ptr = std::move(H.nbr_ptr), c->kry_agg_nbr = std::move(H.nbr), c->kry_agg_x = std::move(H.centroid);
  c->kry_agg_max_nbr = H.max_nbr;
  c->kry_nagg = H.nagg;
  return C8_OK;
}

inline AggTables agg_tables(c8_ctx const* c) {
  int32_t const* b = c->d_kry_agg;
  size_t const* o = c->kry_agg_at;
  return AggTables{b + o[0], b + o[1], b + o[2], b + o[3], b + o[4], b + o[5], c->d_kry_agg_off, c->d_kry_cflags};
}

// what a call must refuse before any device work of the two-level kind: a halo, the cap of the dense coarse solve
int coarse_refusals(c8_ctx* c, char const* who) {
  if (c->halo)
    return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": the two-level preconditioner (C8_PRECOND_TWO_LEVEL) is not supported with a halo "
                                    "attached to the context: its coarse space covers one part only");
  if (c->mesh.nnodes <= 0) return fail(C8_ERR_ARG, std::string(who) + ": empty mesh");
  int const rc = build_aggregates(c);
  if (rc != C8_OK) return rc;
  long long const n = (long long)c->kry_nagg * coarse_columns(c);
  if (n > COARSE_CAP)
    return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": the two-level preconditioner solves its coarse problem densely: n_coarse = " +
                                    std::to_string(n) + " (" + std::to_string(c->kry_nagg) + " aggregates) exceeds the cap of " +
                                    std::to_string(COARSE_CAP));
  return C8_OK;
}

// The dense inverse of the n x n row-major matrix A (leading dimension lda), in place, on the context's stream: LU with
// partial pivoting and the inverse from it (rocSOLVER: dgetrf + dgetri; row-major A is the column-major A^T, whose inverse
// is the row-major A^-1).  info[0], info[1] (device) receive the two routines' codes: i > 0 = pivot i is zero.  The one
// place that knows the library: a later change may replace it.
int coarse_invert(c8_ctx* c, int n, int lda, double* A, int32_t* ipiv, int32_t* info) {
  if (!c->kry_rocblas) {
    rocblas_handle h = nullptr;
    if (rocblas_create_handle(&h) != rocblas_status_success) return fail(C8_ERR_DEVICE, "c8_krylov: rocblas_create_handle failed");
    c->kry_rocblas = h;
  }
  rocblas_handle const h = (rocblas_handle)c->kry_rocblas;
  rocblas_status st = rocblas_set_stream(h, c->stream);
  if (st == rocblas_status_success) st = rocsolver_dgetrf(h, n, n, A, lda, ipiv, info);
  if (st == rocblas_status_success) st = rocsolver_dgetri(h, n, A, lda, ipiv, info + 1);
  if (st != rocblas_status_success)
    return fail(C8_ERR_DEVICE, "c8_krylov: the dense inverse of the coarse matrix failed (rocSOLVER status " + std::to_string((int)st) + ")");
  return C8_OK;
}

// The coarse level for the matrix of q, up to A_c (invert = false: c8_krylov_coarse_matrix) or to its checked inverse.
// Needs coarse_refusals() passed.
template <int ND, int NRES, int G>
int coarse_setup(Solve const& q, bool invert) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  c8_ctx* c = q.c;
  int const nagg = c->kry_nagg, n = nagg * NC, lda = (n + 1) & ~1;
  size_t const lds = (size_t)c->kry_agg_max_nbr * NC * NC * sizeof(double);
  if (lds > GALERKIN_LDS)
    return fail(C8_ERR_UNSUPPORTED, "c8_krylov: an aggregate has " + std::to_string(c->kry_agg_max_nbr) +
                                    " neighbouring aggregates: the block row of the coarse matrix does not fit the tile of k_galerkin");
  int rc;
  if ((rc = grow(&c->d_kry_Ac, &c->kry_Ac_n, (size_t)n * lda)) != C8_OK) return rc;
  if ((rc = grow(&c->d_kry_cvec, &c->kry_cvec_n, 2 * (size_t)lda)) != C8_OK) return rc;
  if ((rc = grow(&c->d_kry_ipiv, &c->kry_ipiv_n, (size_t)n + 4)) != C8_OK) return rc;
  hipStream_t const st = c->stream;
  int32_t* info = c->d_kry_ipiv + n;  // getrf, getri, first row of the inverse that is not finite
  int32_t h_info[3] = {0, 0, INT_MAX};
  C8_HIP(hipMemcpyAsync(info, h_info, sizeof(h_info), hipMemcpyHostToDevice, st));
  C8_HIP(hipMemsetAsync(c->d_kry_Ac, 0, (size_t)n * lda * sizeof(double), st));
  C8_HIP(hipMemsetAsync(c->d_kry_cvec, 0, 2 * (size_t)lda * sizeof(double), st));
  int const nb_g = (q.nn + TPB / G - 1) / (TPB / G);
  hipLaunchKernelGGL((k_constrained<ND, NRES, G>), dim3(xcd_grid(nb_g)), dim3(TPB), 0, st, q.nn, nb_g, c->d_nodeptr, c->d_nodeadj, q.A, c->d_kry_cflags);
  C8_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_galerkin<ND, NRES>), dim3(nagg), dim3(TPB), lds, st, agg_tables(c), c->d_nodeptr, c->d_nodeadj, q.A, c->d_kry_Ac, lda);
  C8_HIP(hipGetLastError());
  if (!invert) return C8_OK;
  if ((rc = coarse_invert(c, n, lda, c->d_kry_Ac, c->d_kry_ipiv, info)) != C8_OK) return rc;
  int const nb_c = (int)std::min<size_t>(((size_t)n * lda + TPB - 1) / TPB, (size_t)UPDATE_MAX_BLOCKS);
  hipLaunchKernelGGL(k_coarse_check, dim3(nb_c), dim3(TPB), 0, st, n, lda, c->d_kry_Ac, info + 2);
  C8_HIP(hipGetLastError());
  C8_HIP(hipMemcpyAsync(h_info, info, sizeof(h_info), hipMemcpyDeviceToHost, st));
  C8_HIP(hipStreamSynchronize(st));
  int const bad = h_info[0] > 0 ? h_info[0] - 1 : h_info[1] > 0 ? h_info[1] - 1 : h_info[2] != INT_MAX ? h_info[2] : -1;
  if (bad >= 0)
    return fail(C8_ERR_ARG, "c8_krylov: the coarse matrix of the two-level preconditioner is singular or not finite at aggregate " +
                            std::to_string(bad / NC) + " (coarse row " + std::to_string(bad) + " of " + std::to_string(n) + ")");
  return C8_OK;
}

// x = P A_c^-1 P^T rhs
template <int ND, int NRES>
hipError_t launch_coarse(Solve const& q, double const* rhs, double* x) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  c8_ctx const* c = q.c;
  int const nagg = c->kry_nagg, n = nagg * NC, lda = (n + 1) & ~1, wpb = TPB / 64;
  AggTables const T = agg_tables(c);
  double *rc = c->d_kry_cvec, *e = c->d_kry_cvec + lda;
  hipLaunchKernelGGL((k_restrict<ND, NRES>), dim3((nagg + wpb - 1) / wpb), dim3(TPB), 0, c->stream, nagg, T, q.nn, rhs, rc, q.S);
  hipLaunchKernelGGL(k_coarse_apply, dim3((n + wpb - 1) / wpb), dim3(TPB), 0, c->stream, n, lda, c->d_kry_Ac, rc, e, q.S);
  hipLaunchKernelGGL((k_prolong<ND, NRES>), dim3(xcd_grid(q.nb_node)), dim3(TPB), 0, c->stream, q.nn, q.nb_node, T, e, x, q.S);
  return hipGetLastError();
}
