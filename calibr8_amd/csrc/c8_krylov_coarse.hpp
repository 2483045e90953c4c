// c8_krylov_coarse.hpp -- what the four aggregation preconditioners of the device solve share between level 0 and level 1
// (C8_PRECOND_TWO_LEVEL, C8_PRECOND_MULTILEVEL and their forms over parts in include/c8.h; DESIGN.md sections 13d to 13h).
// Included by c8_krylov.hip inside its unnamed namespace, after the kernels of the one-level solve (TPB, Blocks, KryScalars,
// xcd_block, grow, Solve; rocSOLVER's header is included there).
//
//   aggregates   three passes over a host node graph (aggregate_graph); the device mirror holds the aggregate of every node,
//                the node list and the neighbour list of every aggregate, and for every entry of the node graph the position
//                of the column's aggregate in the neighbour list of the row's aggregate
//   P            never stored: aggregate id, the node's offset from the aggregate's centroid, the constrained-row flags
//   level 0      one descriptor (Level0) for one part and for a part among several: the tables, the first global id of the
//                part's aggregates (base), their count, the count over all parts, the owned nodes.  One part: base 0,
//                total = nagg, nown = nnodes.  The kernels take these and are the same for both.
//   set-up       k_constrained (flags) -> k_galerkin (A_1 = P^T A P: dense, row-major, leading dimension lda, or block-sparse)
//   apply        k_restrict (r_1 = P^T v) ... k_prolong (x = P e_1); the sweeps of k_sgs_color start from this x
//   last level   dense: coarse_invert (in place) -> k_coarse_check at set-up, k_coarse_apply (e = A^-1 r) in the apply
// Over parts every entry of A_1 and of r_1 is written by one rank and zero on the others, so that the all-reduce between
// the ranks is exact.  Every sum has a fixed order and no kernel uses a floating-point atomic.  The block levels below
// level 1 and the single-part host path are in c8_krylov_multilevel.hpp, the host path over parts in c8_krylov_parts_levels.hpp.
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
// in all blocks (the rows c8_apply_dirichlet leaves).  Lane mapping of k_spmv, an OR over the node's G lanes.  Rows
// 0 .. n_rows - 1: all nodes of one part, or the owned nodes of a part among several (over the whole row: off-part columns
// included).
template <int ND, int NRES, int G>
__global__ void __launch_bounds__(TPB) k_constrained(int n_rows, int nblocks, int32_t const* __restrict__ nodeptr, int32_t const* __restrict__ nodeadj,
                                                     Blocks A, int32_t* __restrict__ flags) {
  constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  constexpr int NPB = TPB / G;
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const node = lb * NPB + threadIdx.x / G, lane = threadIdx.x % G;
  int nz = 0;  // bit r: equation r has a non-zero off-diagonal entry
  if (node < n_rows) {
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
  if (node < n_rows && lane == 0) flags[node] = ~nz & ((1 << NB) - 1);
}

struct AggTables {  // device mirror of the aggregates (c8_ctx::d_kry_agg and its offsets)
  int32_t const *agg_of, *ptr, *nodes, *nbr_ptr, *nbr, *slot;
  double const* off;  // [nnodes][ND]: x_i - centroid of the node's aggregate
  int32_t const* flags;
};
// Level 0 as the launches between level 0 and level 1 see it.  Over parts the tables are local-sized (owned nodes, then the
// copies with the owners' P imported), T.agg_of and T.nbr hold GLOBAL aggregate ids, T.ptr / T.nodes / T.nbr_ptr the part's
// own aggregates counted from 0.
struct Level0 {
  AggTables T;
  int base, nagg, total;  // first global id of the part's aggregates, their number, the number over all parts
  int nown;               // nodes whose rows the part owns: the first nown of its nodes
  int max_nbr;            // most neighbouring aggregates of one aggregate (itself included): the tile of k_galerkin
};

// ---- the part's block rows of A_1 = P^T A P.  One workgroup owns the block row of the part's aggregate I (global id
// base + I): NC rows of A_1, its tile in LDS has one NC x NC block per neighbouring aggregate on any part
// (tile[r][slot * NC + c], T.nbr in ascending global id).  A work item owns the tile columns q = slot * NC + c,
// q = thread, thread + TPB, ...: it walks the aggregate's nodes in ascending id and each node's graph row in column order,
// and for the entries whose column node lies in the aggregate of `slot` adds P_i^T (A_ij P_j[:, c]) to its NC tile entries
// -- one owner per entry, the sum of an entry in one fixed order.  P_j of a ghost or phantom column comes from the imported
// entries of T.agg_of / T.off / T.flags.  A column of P that is zero (every row of the mode constrained, or a one-node
// aggregate's rotation) gets a unit diagonal, the owner's.  Output, every entry once:
//   dense    rows (base + I) * NC ... of the row-major matrix; the other entries are the zeros of the memset before the launch
//   SPARSE   the NC x NC block of neighbour `slot` to graph entry nbr_ptr_global[base + I] + slot of the block-sparse A_1.
//            The part's aggregates are consecutive rows of that graph and T.nbr_ptr counts the same lists from the part's
//            first row, so the entry is nbr_ptr_global[base] + T.nbr_ptr[I] + slot and Ac points at entry nbr_ptr_global[base].
template <int ND, int NRES, bool SPARSE = false>
__global__ void __launch_bounds__(TPB) k_galerkin(AggTables T, int base, int32_t const* __restrict__ nodeptr, int32_t const* __restrict__ nodeadj, Blocks A,
                                                  double* __restrict__ Ac, int lda) {
  constexpr int NB = CoarseDims<ND, NRES>::NB, NC = CoarseDims<ND, NRES>::NC;
  extern __shared__ double tile[];
  int const I = blockIdx.x;
  int const a0 = T.ptr[I], a1 = T.ptr[I + 1], b0 = T.nbr_ptr[I];
  int const W = (T.nbr_ptr[I + 1] - b0) * NC;
  for (int q = threadIdx.x; q < W; q += TPB) {
    int const sl = q / NC, c = q % NC;
    bool const own = T.nbr[b0 + sl] == base + I;
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
        int const cn = nodeadj[np + k];  // owned, ghost or phantom: the tables are local-sized
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
    else Ac[(size_t)((base + I) * NC + r) * lda + (size_t)T.nbr[b0 + q / NC] * NC + q % NC] = tile[idx];
  }
}

// ---- r_1 = P^T v over all aggregates of all parts: one wavefront per GLOBAL aggregate.  Those of this part
// (base <= id < base + nagg): lane l takes the nodes l, l + 64, ... of the aggregate's list, then a fixed butterfly over
// the lanes.  The others get the zeros the all-reduce needs.  v is local-sized (p at nn * ND).
template <int ND, int NRES>
__global__ void __launch_bounds__(TPB) k_restrict(int ntotal, int base, int nagg, AggTables T, int nn, double const* __restrict__ v,
                                                  double* __restrict__ rc, KryScalars const* S) {
  constexpr int NB = CoarseDims<ND, NRES>::NB, NC = CoarseDims<ND, NRES>::NC;
  if (S->stop) return;
  int const gI = blockIdx.x * (TPB / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
  int const I = gI - base;
  bool const mine = gI < ntotal && I >= 0 && I < nagg;
  size_t const n0 = (size_t)nn * ND;
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.;
  if (mine) {
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
  if (gI < ntotal && lane == 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c) rc[(size_t)gI * NC + c] = acc[c];
  }
}

// ---- rows [row0, row0 + nrows) of e = A^-1 r, the dense row-major inverse of the last level: one wavefront per row,
// 16-byte loads (lda is even, the padding entries of a row and of r are zero), a fixed butterfly over the lanes.  Over
// parts with level 1 the last level a rank forms the rows of its own aggregates only: the others are not its to prolong.
__global__ void __launch_bounds__(TPB) k_coarse_apply(int row0, int nrows, int lda, double const* __restrict__ Ainv,
                                                      double const* __restrict__ rc, double* __restrict__ e, KryScalars const* S) {
  if (S->stop) return;
  int const k = blockIdx.x * (TPB / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
  int const row = row0 + k;
  double s = 0.;
  if (k < nrows) {
    double2 const* a = (double2 const*)(Ainv + (size_t)row * lda);
    double2 const* x = (double2 const*)rc;
    for (int j = lane; j < lda / 2; j += 64) {
      double2 const av = a[j], xv = x[j];
      s += av.x * xv.x;
      s += av.y * xv.y;
    }
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (k < nrows && lane == 0) e[row] = s;
}

// ---- x = P e on the owned nodes of a local-sized vector (the p segment starts at nn * ND), one work item per node: the
// start of the Gauss-Seidel sweeps in the place of x = 0.  T.agg_of indexes e: global ids over parts.
template <int ND, int NRES>
__global__ void __launch_bounds__(TPB) k_prolong(int nown, int nn, int nblocks, AggTables T, double const* __restrict__ e, double* __restrict__ x,
                                                 KryScalars const* S) {
  constexpr int NB = CoarseDims<ND, NRES>::NB, NC = CoarseDims<ND, NRES>::NC;
  if (S->stop) return;
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const node = lb * TPB + threadIdx.x;
  if (node >= nown) return;
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
// The neighbouring aggregates of every aggregate of H (ascending id, itself included) and the slot of every entry of the
// graph (gp, ga) in the list of its row's aggregate, from H.agg (the aggregate of every node of the graph, ids below
// `nids`) and the node lists H.ptr, H.nodes of the H.nagg aggregates whose rows are walked.  aggregate_graph: local ids,
// all of them.  Over parts: global ids at all local nodes, the whole owned rows of the rank's own aggregates.
void neighbour_lists(Aggregates& H, int nids, std::vector<int32_t> const& gp, std::vector<int32_t> const& ga) {
  std::vector<int32_t> const &agg = H.agg, &ptr = H.ptr, &nodes = H.nodes;
  std::vector<int32_t>&nbr_ptr = H.nbr_ptr, &nbr = H.nbr, &slot = H.slot;
  std::vector<int32_t> where(nids, -1);
  nbr.clear(), H.max_nbr = 0;
  nbr_ptr.assign(H.nagg + 1, 0), slot.assign(ga.size(), 0);
  for (int a = 0; a < H.nagg; ++a) {
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
}

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
  H.nagg = nagg;
  neighbour_lists(H, nagg, gp, ga);
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

// The aggregates of the context's node graph, once per context, and their device mirror.  Level 1 (its graph is the
// neighbour lists, its positions the centroids) is the one entry of the two-level kind's list of levels, kry_agg_levels;
// the multilevel kind copies it and builds on the copy (build_levels).
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
  c->kry_agg_levels.assign(1, c8_kry_level{});
  c8_kry_level& L1 = c->kry_agg_levels[0];
  L1.n = H.nagg;
  L1.gp = std::move(H.nbr_ptr), L1.ga = std::move(H.nbr), L1.x = std::move(H.centroid);
  c->kry_agg_max_nbr = H.max_nbr;
  c->kry_nagg = H.nagg;
  return C8_OK;
}

// level 0 of one part (no halo): the tables of build_aggregates
inline Level0 level0(c8_ctx const* c) {
  int32_t const* b = c->d_kry_agg;
  size_t const* o = c->kry_agg_at;
  return Level0{AggTables{b + o[0], b + o[1], b + o[2], b + o[3], b + o[4], b + o[5], c->d_kry_agg_off, c->d_kry_cflags},
                0, c->kry_nagg, c->kry_nagg, c->mesh.nnodes, c->kry_agg_max_nbr};
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
