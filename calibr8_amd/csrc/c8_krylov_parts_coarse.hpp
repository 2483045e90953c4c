// c8_krylov_parts_coarse.hpp -- the coarse level of the two-level preconditioner over the parts of a multi-part mesh
// (C8_PRECOND_TWO_LEVEL_PARTS in include/c8.h).  Included by c8_krylov.hip inside its unnamed
// namespace, after the host side of the multi-part solve (Parts, C8_PARTS_LAUNCH, launch_sgs) and after
// c8_krylov_coarse.hpp, whose host rules (aggregate_graph, coarse_invert), P (p_entry, CoarseDims) and tables (AggTables)
// it shares; its kernels are its own.
//
//   aggregates   aggregate_graph over the OWNED sub-graph of every rank (columns >= num_owned dropped); global id = base of
//                the rank + local id, the counts of the ranks travel in one all-reduce of one slot per rank
//   imported     the owner's P_j at the ghost and phantom copies of node j: global aggregate id and offset from the
//                centroid once per attached halo, constrained flags at every set-up, all through the import (C3) tables
//   set-up       k_constrained_own (flags of the owned rows) -> import of the flags -> k_galerkin_parts (this rank's block
//                rows of the dense global A_c, the other rows zero) -> one all-reduce of A_c -> coarse_invert on every rank
//                -> k_coarse_check; the ranks then agree on the outcome (parts_coarse_agree)
//   apply        k_restrict_parts (own slots of r_c, zeros elsewhere) -> one all-reduce of r_c -> k_coarse_apply_rows (e on
//                the rows of the rank's own aggregates) -> k_prolong_own (x = P e on the owned nodes), then the part-local
//                sweeps of k_sgs_color started from this x
// Every entry of an all-reduced buffer is written by one rank and zero on the others: the sums are exact, for any number of
// parts and any order of summation.  Every other sum has a fixed order; no kernel uses a floating-point atomic.

// ---- constrained rows of the owned nodes (the rule of k_constrained, over the whole row: off-part columns included)
template <int ND, int NRES, int G>
__global__ void __launch_bounds__(TPB) k_constrained_own(int nown, int nblocks, int32_t const* __restrict__ nodeptr,
                                                         int32_t const* __restrict__ nodeadj, Blocks A, int32_t* __restrict__ flags) {
  constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  constexpr int NPB = TPB / G;
  int const lb = xcd_block(blockIdx.x, nblocks);
  if (lb >= nblocks) return;
  int const node = lb * NPB + threadIdx.x / G, lane = threadIdx.x % G;
  int nz = 0;  // bit r: equation r has a non-zero off-diagonal entry
  if (node < nown) {
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
  if (node < nown && lane == 0) flags[node] = ~nz & ((1 << NB) - 1);
}

// ---- the flags on their way through the import tables, which move doubles: component 0 of the node's u entries
__global__ void __launch_bounds__(TPB) k_flags_pack(int nown, int nd, int32_t const* __restrict__ flags, double* __restrict__ buf) {
  int const node = blockIdx.x * TPB + threadIdx.x;
  if (node < nown) buf[(size_t)node * nd] = (double)flags[node];
}
__global__ void __launch_bounds__(TPB) k_flags_unpack(int nown, int nn, int nd, double const* __restrict__ buf, int32_t* __restrict__ flags) {
  int const node = nown + blockIdx.x * TPB + threadIdx.x;
  if (node < nn) flags[node] = (int32_t)buf[(size_t)node * nd];
}

// ---- this rank's block rows of A_c = P^T A P.  k_galerkin with the tables of a part: one workgroup per OWNED aggregate
// I (global id base + I), the tile has one NC x NC block per neighbouring aggregate on any rank (T.nbr holds global ids,
// ascending), P_j of a ghost or phantom column comes from the imported entries of T.agg_of / T.off / T.flags (local-sized
// arrays).  Ownership and order of the sums are those of k_galerkin: a work item owns its tile columns and walks the
// aggregate's nodes in ascending id and each node's graph row in column order.  The unit diagonal of a zero column of P is
// the owner's.  Output: rows (base + I) * NC ... of the dense global matrix; every other row of this rank's copy stays zero.
// SPARSE (the multilevel kind over parts, c8_krylov_parts_multilevel.hpp): the tile goes to the block-sparse replicated A_1
// instead, the NC x NC block of neighbour `slot` to graph entry nbr_ptr_global[base + I] + slot of level 1.  The rank's
// aggregates are consecutive rows of that graph and T.nbr_ptr counts the same lists from the rank's first row, so the entry
// is nbr_ptr_global[base] + T.nbr_ptr[I] + slot and Ac points at entry nbr_ptr_global[base]; the sums are the same.
template <int ND, int NRES, bool SPARSE = false>
__global__ void __launch_bounds__(TPB) k_galerkin_parts(AggTables T, int base, int32_t const* __restrict__ nodeptr,
                                                        int32_t const* __restrict__ nodeadj, Blocks A, double* __restrict__ Ac, int lda) {
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

// ---- r_c = P^T v over all aggregates of all ranks: one wavefront per GLOBAL aggregate; those of this rank (base <= id <
// base + nagg) are summed as in k_restrict, the others get the zeros the all-reduce needs.  v is local-sized (p at nn * ND).
template <int ND, int NRES>
__global__ void __launch_bounds__(TPB) k_restrict_parts(int ntotal, int base, int nagg, AggTables T, int nn, double const* __restrict__ v,
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

// ---- rows [row0, row0 + nrows) of e = A_c^-1 r_c: k_coarse_apply over a row range (one wavefront per row, 16-byte loads,
// a fixed butterfly); the other rows of e are not this rank's to prolong
__global__ void __launch_bounds__(TPB) k_coarse_apply_rows(int row0, int nrows, int lda, double const* __restrict__ Ainv,
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

// ---- x = P e on the owned nodes of a local-sized vector (the p segment starts at nn * ND); T.agg_of holds global ids
template <int ND, int NRES>
__global__ void __launch_bounds__(TPB) k_prolong_own(int nown, int nn, int nblocks, AggTables T, double const* __restrict__ e,
                                                     double* __restrict__ x, KryScalars const* S) {
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

// ---- host side ----------------------------------------------------------------------------------------------------------

// the part of a Parts that the coarse level needs, for the calls outside the solve
inline Parts parts_of(c8_ctx* c) {
  Parts P;
  P.q = Solve{};
  P.q.c = c;
  P.q.nn = c->mesh.nnodes;
  P.h = c->halo;
  P.cm = c8_halo_comm(c->halo);
  P.rank = c8_halo_rank(c->halo);
  P.nranks = c8_halo_num_ranks(c->halo);
  P.nown = c8_halo_num_owned(c->halo);
  P.nb_own = (P.nown + TPB - 1) / TPB;
  return P;
}

inline AggTables parts_agg_tables(c8_ctx const* c) {
  int32_t const* b = c->d_kry_pc_agg;
  size_t const* o = c->kry_pc_at;
  return AggTables{b + o[0], b + o[1], b + o[2], b + o[3], b + o[4], b + o[5], c->d_kry_pc_off, c->d_kry_pc_flags};
}

// The ranks agree on a failure of the collective calls of this file, by the rule of the bad-node decision of the solve: slot r
// of an all-reduced vector holds rank r's finding + 1 (0: none), one more slot counts the ranks with a device error.  Every
// rank sees the same vector and returns the same code; `what(r, finding)` words the message.
template <class F>
int parts_agree(Parts& P, char const* who, double finding, F what) {
  std::vector<double> v(P.nranks + 1, 0.);
  if (!P.failed && finding >= 0.) v[P.rank] = finding + 1.;
  v[P.nranks] = P.failed ? 1. : 0.;
  if (c8_comm_allreduce_sum(P.cm, v.data(), P.nranks + 1) != C8_OK) return C8_ERR_DEVICE;  // (the message is the transport's)
  if (!(v[P.nranks] == 0.))
    return fail(C8_ERR_DEVICE, P.failed ? std::string(who) + ": rank " + std::to_string(P.rank) + ": " + P.err
                                        : std::string(who) + ": another rank met a device error; all ranks leave the call");
  for (int r = 0; r < P.nranks; ++r)
    if (v[r] > 0.) return what(r, (long long)v[r] - 1);
  return C8_OK;
}

// The aggregates of this rank's owned sub-graph and the counts of all ranks (host only; COLLECTIVE at the first use and after
// num_owned changed: one all-reduce of one slot per rank, every slot written by one rank).
int parts_aggregates(c8_ctx* c, Parts& P) {
  if (c->kry_pc_host_for == P.nown) return C8_OK;
  c->kry_pc_host_for = -1, c->kry_pc_for = -1, c->kry_pl_for = -1;
  int const nown = P.nown;
  std::vector<int32_t> gp(nown + 1, 0), ga;
  for (int i = 0; i < nown; ++i) {
    for (int32_t k = c->graph.nodeptr[i]; k < c->graph.nodeptr[i + 1]; ++k)
      if (c->graph.nodeadj[k] < nown) ga.push_back(c->graph.nodeadj[k]);
    gp[i + 1] = (int32_t)ga.size();
  }
  Aggregates H = aggregate_graph(nown, c->ndims, gp, ga, c->mesh.coords.data());
  std::vector<double> counts(P.nranks, 0.);
  counts[P.rank] = (double)H.nagg;
  int const rc = c8_comm_allreduce_sum(P.cm, counts.data(), P.nranks);
  if (rc != C8_OK) return rc;
  long long total = 0, base = 0;
  for (int r = 0; r < P.nranks; ++r) {
    if (r < P.rank) base += (long long)counts[r];
    total += (long long)counts[r];
  }
  c->kry_pc_agg_of = std::move(H.agg);
  c->kry_pc_ptr = std::move(H.ptr), c->kry_pc_nodes = std::move(H.nodes), c->kry_pc_off = std::move(H.off);
  c->kry_pc_x = std::move(H.centroid);
  c->kry_pc_nagg = H.nagg;
  c->kry_pc_base = base, c->kry_pc_total = total;
  c->kry_pc_host_for = nown;
  return C8_OK;
}

// What a call of the kind over parts refuses before any device work, the same on every rank: the cap of the dense coarse
// solve on the GLOBAL count.  COLLECTIVE (parts_aggregates).
int parts_coarse_refusals(c8_ctx* c, Parts& P, char const* who) {
  if (c->mesh.nnodes <= 0) return fail(C8_ERR_ARG, std::string(who) + ": empty mesh");
  int const rc = parts_aggregates(c, P);
  if (rc != C8_OK) return rc;
  long long const n = c->kry_pc_total * coarse_columns(c);
  if (n > COARSE_CAP)
    return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": the two-level preconditioner over parts solves its coarse problem densely on every rank: n_c = " +
                                    std::to_string(n) + " (" + std::to_string(c->kry_pc_total) + " aggregates over " + std::to_string(P.nranks) +
                                    " parts) exceeds the cap of " + std::to_string(COARSE_CAP));
  return C8_OK;
}

// The device tables of the coarse level: the owners' global aggregate ids and offsets imported at the copies, the node lists
// of the rank's aggregates, their neighbour lists over all ranks and the slot of every entry of the owned graph rows.  Once
// per attached halo (c8_halo_attach resets kry_pc_for) and when num_owned changes.  COLLECTIVE: two imports, and the
// agreement on device errors and on the tile of k_galerkin_parts.  Needs parts_coarse_refusals() passed.
int parts_coarse_build(c8_ctx* c, Parts& P, char const* who) {
  if (c->kry_pc_for == P.nown) return C8_OK;
  int const nn = c->mesh.nnodes, nown = P.nown, nd = c->ndims, nc = coarse_columns(c);
  int const base = (int)c->kry_pc_base, total = (int)c->kry_pc_total;
  c->kry_pc_for = -1, c->kry_pl_for = -1;
  for (void* b : {(void*)c->d_kry_pc_agg, (void*)c->d_kry_pc_off, (void*)c->d_kry_pc_flags, (void*)c->d_kry_pc_imp}) P.hip(hipFree(b), "hipFree");
  c->d_kry_pc_agg = nullptr, c->d_kry_pc_off = nullptr, c->d_kry_pc_flags = nullptr, c->d_kry_pc_imp = nullptr;
  size_t const nu = (size_t)nn * nd;
  std::vector<double> hoff(nu, 0.), hgid(nu + nn, 0.);
  std::copy(c->kry_pc_off.begin(), c->kry_pc_off.end(), hoff.begin());  // [num_owned][nd] first
  for (int i = 0; i < nn; ++i) hgid[(size_t)i * nd] = i < nown ? (double)(base + c->kry_pc_agg_of[i]) : -1.;
  if (!P.failed) P.hip(hipMalloc((void**)&c->d_kry_pc_off, std::max<size_t>(nu, 1) * sizeof(double)), "hipMalloc");
  if (!P.failed) P.hip(hipMalloc((void**)&c->d_kry_pc_imp, (nu + nn) * sizeof(double)), "hipMalloc");
  if (!P.failed) P.hip(hipMalloc((void**)&c->d_kry_pc_flags, (size_t)nn * sizeof(int32_t)), "hipMalloc");
  if (!P.failed) P.hip(hipMemcpyAsync(c->d_kry_pc_off, hoff.data(), nu * sizeof(double), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
  if (!P.failed) P.hip(hipMemcpyAsync(c->d_kry_pc_imp, hgid.data(), (nu + nn) * sizeof(double), hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync");
  if (!P.failed) P.hip(hipMemsetAsync(c->d_kry_pc_flags, 0, (size_t)nn * sizeof(int32_t), c->stream), "hipMemsetAsync");
  double* const seg1 = c->nres == 2 && c->d_kry_pc_imp ? c->d_kry_pc_imp + nu : nullptr;  // (the p segment moves with every import: scratch)
  P.note(c8_halo_import_start(P.h, c->d_kry_pc_imp, seg1, P.failed));
  P.note(c8_halo_import_finish(P.h, c->d_kry_pc_imp, seg1, P.failed));
  P.note(c8_halo_import_start(P.h, c->d_kry_pc_off, seg1, P.failed));
  P.note(c8_halo_import_finish(P.h, c->d_kry_pc_off, seg1, P.failed));
  if (!P.failed) P.hip(hipMemcpyAsync(hgid.data(), c->d_kry_pc_imp, nu * sizeof(double), hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
  if (!P.failed) P.hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  Aggregates H;
  if (!P.failed) {
    H.agg.assign(nn, 0);
    for (int i = 0; i < nn && !P.failed; ++i) {
      double const g = hgid[(size_t)i * nd];
      if (!(g >= 0. && g < (double)total)) {
        P.failed = true;
        P.err = "local node " + std::to_string(i) + " received no aggregate from its owner (is it in the halo's import tables?)";
      } else H.agg[i] = (int32_t)g;
    }
  }
  if (!P.failed) {
    std::vector<int32_t> const &gp = c->graph.nodeptr, &ga = c->graph.nodeadj;
    int const nagg = c->kry_pc_nagg;
    H.nagg = nagg;
    H.ptr = c->kry_pc_ptr, H.nodes = c->kry_pc_nodes;
    H.nbr_ptr.assign(nagg + 1, 0), H.slot.assign(ga.size(), 0);
    std::vector<int32_t> where(total, -1);
    for (int a = 0; a < nagg; ++a) {  // the neighbour rule of aggregate_graph over the whole owned rows, by global id
      size_t const lo = H.nbr.size();
      for (int k = H.ptr[a]; k < H.ptr[a + 1]; ++k)
        for (int32_t e = gp[H.nodes[k]]; e < gp[H.nodes[k] + 1]; ++e)
          if (where[H.agg[ga[e]]] != a) { where[H.agg[ga[e]]] = a; H.nbr.push_back(H.agg[ga[e]]); }
      std::sort(H.nbr.begin() + lo, H.nbr.end());
      H.nbr_ptr[a + 1] = (int32_t)H.nbr.size();
      H.max_nbr = std::max(H.max_nbr, (int)(H.nbr.size() - lo));
      for (int k = H.ptr[a]; k < H.ptr[a + 1]; ++k)
        for (int32_t e = gp[H.nodes[k]]; e < gp[H.nodes[k] + 1]; ++e)
          H.slot[e] = (int32_t)(std::lower_bound(H.nbr.begin() + lo, H.nbr.end(), H.agg[ga[e]]) - (H.nbr.begin() + lo));
    }
    c->kry_pc_nbr_ptr = H.nbr_ptr, c->kry_pc_nbr = H.nbr;  // (rows of the level-1 graph of the multilevel kind over parts)
    double* none = nullptr;  // (the offsets are on the device already, imported: upload_aggregates gets one placeholder entry)
    H.off.assign(1, 0.);
    P.note(upload_aggregates(H, &c->d_kry_pc_agg, c->kry_pc_at, &none));
    (void)hipFree(none);
  }
  c->kry_pc_max_nbr = H.max_nbr;
  size_t const cap_nbr = GALERKIN_LDS / ((size_t)nc * nc * sizeof(double));
  int const rc = parts_agree(P, who, (size_t)H.max_nbr > cap_nbr ? (double)H.max_nbr : -1., [&](int r, long long nbr) {
    return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": an aggregate of rank " + std::to_string(r) + " has " + std::to_string(nbr) +
                                    " neighbouring aggregates: the block row of the coarse matrix does not fit the tile of k_galerkin_parts");
  });
  if (rc != C8_OK) return rc;
  c->kry_pc_for = nown;
  return C8_OK;
}

// Refusals and tables in one: what every entry of the kind over parts calls first.  COLLECTIVE.
int parts_coarse_prepare(c8_ctx* c, Parts& P, char const* who) {
  int rc = parts_coarse_refusals(c, P, who);
  if (rc != C8_OK) return rc;
  return parts_coarse_build(c, P, who);
}

// The constrained flags of the gathered matrix of P.q at every local node: the owned rows' by k_constrained_own, the copies'
// imported from their owners.  One import.
template <int ND, int NRES, int G>
void parts_flags(Parts& P) {
  Solve const& q = P.q;
  c8_ctx* c = q.c;
  int const nb_g = (P.nown + TPB / G - 1) / (TPB / G), nb_copy = (q.nn - P.nown + TPB - 1) / TPB;
  double* const imp = c->d_kry_pc_imp;
  double* const seg1 = NRES == 2 ? imp + (size_t)q.nn * ND : nullptr;
  C8_PARTS_LAUNCH(P, (k_constrained_own<ND, NRES, G>), xcd_grid(nb_g), TPB, P.nown, nb_g, c->d_nodeptr, c->d_nodeadj, q.A, c->d_kry_pc_flags);
  C8_PARTS_LAUNCH(P, k_flags_pack, P.nb_own, TPB, P.nown, ND, c->d_kry_pc_flags, imp);
  P.note(c8_halo_import_start(P.h, imp, seg1, P.failed));
  P.note(c8_halo_import_finish(P.h, imp, seg1, P.failed));
  C8_PARTS_LAUNCH(P, k_flags_unpack, nb_copy, TPB, P.nown, q.nn, ND, imp, c->d_kry_pc_flags);
}

// The coarse level for the gathered matrix of P.q, up to the all-reduced A_c (invert = false) or to its checked inverse.
// Errors go to P; parts_coarse_agree() after it gives every rank the same code.
template <int ND, int NRES, int G>
void parts_coarse_setup(Parts& P, bool invert) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  Solve const& q = P.q;
  c8_ctx* c = q.c;
  int const nagg = c->kry_pc_nagg, base = (int)c->kry_pc_base, n = (int)c->kry_pc_total * NC, lda = (n + 1) & ~1;
  size_t const lds = (size_t)c->kry_pc_max_nbr * NC * NC * sizeof(double);
  P.note(grow(&c->d_kry_Ac, &c->kry_Ac_n, (size_t)n * lda));
  P.note(grow(&c->d_kry_cvec, &c->kry_cvec_n, 2 * (size_t)lda));
  P.note(grow(&c->d_kry_ipiv, &c->kry_ipiv_n, (size_t)n + 4));
  hipStream_t const st = c->stream;
  int32_t* info = c->d_kry_ipiv ? c->d_kry_ipiv + n : nullptr;  // getrf, getri, first row of the inverse that is not finite
  int32_t h_info[3] = {0, 0, INT_MAX};
  if (!P.failed) P.hip(hipMemcpyAsync(info, h_info, sizeof(h_info), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (!P.failed) P.hip(hipMemsetAsync(c->d_kry_Ac, 0, (size_t)n * lda * sizeof(double), st), "hipMemsetAsync");
  if (!P.failed) P.hip(hipMemsetAsync(c->d_kry_cvec, 0, 2 * (size_t)lda * sizeof(double), st), "hipMemsetAsync");
  parts_flags<ND, NRES, G>(P);
  if (!P.failed && nagg > 0) {
    hipLaunchKernelGGL((k_galerkin_parts<ND, NRES>), dim3(nagg), dim3(TPB), lds, st, parts_agg_tables(c), base, c->d_nodeptr, c->d_nodeadj, q.A,
                       c->d_kry_Ac, lda);
    P.hip(hipGetLastError(), "k_galerkin_parts");
  }
  P.note(c8_comm_allreduce_device_long(P.cm, st, c->d_kry_Ac, (size_t)n * lda, P.failed));
  c->kry_pc_bad = -1;
  if (!invert || P.failed) return;
  P.note(coarse_invert(c, n, lda, c->d_kry_Ac, c->d_kry_ipiv, info));
  int const nb_c = (int)std::min<size_t>(((size_t)n * lda + TPB - 1) / TPB, (size_t)UPDATE_MAX_BLOCKS);
  C8_PARTS_LAUNCH(P, k_coarse_check, nb_c, TPB, n, lda, c->d_kry_Ac, info + 2);
  if (!P.failed) P.hip(hipMemcpyAsync(h_info, info, sizeof(h_info), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  if (!P.failed) P.hip(hipStreamSynchronize(st), "hipStreamSynchronize");
  if (!P.failed) c->kry_pc_bad = h_info[0] > 0 ? h_info[0] - 1 : h_info[1] > 0 ? h_info[1] - 1 : h_info[2] != INT_MAX ? h_info[2] : -1;
}

// the outcome of parts_coarse_setup, agreed over the ranks.  COLLECTIVE.
int parts_coarse_agree(Parts& P, char const* who) {
  c8_ctx* c = P.q.c;
  int const nc = coarse_columns(c);
  long long const n = c->kry_pc_total * nc;
  return parts_agree(P, who, (double)c->kry_pc_bad, [&](int r, long long bad) {
    return fail(C8_ERR_ARG, std::string(who) + ": the coarse matrix of the two-level preconditioner over parts is singular or not finite at aggregate " +
                            std::to_string(bad / nc) + " (global id; coarse row " + std::to_string(bad) + " of " + std::to_string(n) +
                            "), as found by rank " + std::to_string(r));
  });
}

// x = P A_c^-1 P^T rhs on the owned nodes: one all-reduce of the n_c doubles of r_c between restrict and apply
template <int ND, int NRES>
void parts_coarse(Parts& P, double const* rhs, double* x) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  Solve const& q = P.q;
  c8_ctx const* c = q.c;
  int const nagg = c->kry_pc_nagg, base = (int)c->kry_pc_base, total = (int)c->kry_pc_total, n = total * NC, lda = (n + 1) & ~1, wpb = TPB / 64;
  AggTables const T = parts_agg_tables(c);
  double *rc = c->d_kry_cvec, *e = c->d_kry_cvec + lda;
  C8_PARTS_LAUNCH(P, (k_restrict_parts<ND, NRES>), (total + wpb - 1) / wpb, TPB, total, base, nagg, T, q.nn, rhs, rc, q.S);
  P.note(c8_comm_allreduce_device_long(P.cm, c->stream, rc, (size_t)n, P.failed));
  C8_PARTS_LAUNCH(P, k_coarse_apply_rows, (nagg * NC + wpb - 1) / wpb, TPB, base * NC, nagg * NC, lda, c->d_kry_Ac, rc, e, q.S);
  C8_PARTS_LAUNCH(P, (k_prolong_own<ND, NRES>), xcd_grid(P.nb_own), TPB, P.nown, q.nn, P.nb_own, T, e, x, q.S);
}

// parts_iteration_sgs with the part-local sweeps started from the coarse correction of their right-hand side: two imports
// and five all-reduces per iteration
template <int ND, int NRES, int G>
void parts_iteration_two_level(Parts& P) {
  Solve const& q = P.q;
  size_t const n0 = (size_t)q.nn * ND, nu = (size_t)P.nown * ND, np_ = NRES == 2 ? (size_t)P.nown : (size_t)0;
  C8_PARTS_LAUNCH(P, (k_vec<0>), P.nb_upd, TPB, nu, np_, n0, q.r, q.v, q.p, q.phat, q.S);
  parts_coarse<ND, NRES>(P, q.p, q.phat);
  if (!P.failed) P.hip(launch_sgs<ND, NRES, G>(q, P.nown, q.p, q.phat, false), "k_sgs_color");
  parts_spmv<ND, NRES, G, 0>(P, q.phat, P.phat1, q.v, q.rhat);
  parts_scalars<0>(P, P.nb_int + P.nb_bnd);
  C8_PARTS_LAUNCH(P, (k_vec<1>), P.nb_upd, TPB, nu, np_, n0, q.r, q.v, q.s, q.shat, q.S);
  parts_coarse<ND, NRES>(P, q.s, q.shat);
  if (!P.failed) P.hip(launch_sgs<ND, NRES, G>(q, P.nown, q.s, q.shat, false), "k_sgs_color");
  parts_spmv<ND, NRES, G, 1>(P, q.shat, P.shat1, q.t, q.s);
  parts_scalars<1>(P, P.nb_int + P.nb_bnd);
  C8_PARTS_LAUNCH(P, k_update_own, P.nb_upd, TPB, nu, np_, n0, q.x, q.r, q.s, q.t, q.phat, q.shat, q.rhat, q.part, q.S);
  parts_scalars<2>(P, P.nb_upd);
}

int build_colors(c8_ctx* c);
// (c8_krylov_parts_multilevel.hpp, included after this file: the same four steps for C8_PRECOND_MULTILEVEL_PARTS)
int parts_levels_prepare(c8_ctx* c, Parts& P, char const* who);
template <int ND, int NRES, int G>
void parts_levels_setup(Parts& P, int upto);
int parts_levels_agree(Parts& P, char const* who);
template <int ND, int NRES>
void parts_levels_apply(Parts& P, double const* rhs, double* x);

// c8_krylov_precondition with a kind over parts selected (two levels, or the multilevel one) and a halo attached: y = M^-1 v on the owned entries.  COLLECTIVE:
// the set-up of the coarse level and the all-reduce of the apply; the refusals (a bad diagonal block, a vector or matrix that
// is not finite, a singular A_c) are agreed over the ranks.
template <int ND, int NRES, int G>
int precondition_parts(c8_ctx* c, const c8_system* sys, const double* const v[2], double* const y[2]) {
  constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  char const* who = "c8_krylov_precondition";
  Parts P = parts_of(c);
  Solve& q = P.q;
  if (q.nn <= 0) return fail(C8_ERR_ARG, "c8_krylov_precondition: empty mesh");
  bool const multi = c->kry_precond == C8_PRECOND_MULTILEVEL_PARTS;
  int rc = multi ? parts_levels_prepare(c, P, who) : parts_coarse_prepare(c, P, who);
  if (rc != C8_OK) return rc;
  int const nown = P.nown;
  size_t const n0 = (size_t)q.nn * ND, nu = (size_t)nown * ND, np_ = NRES == 2 ? (size_t)nown : (size_t)0;
  q.n = n0 + (NRES == 2 ? (size_t)q.nn : 0);
  q.nb_node = std::max(P.nb_own, 1);
  P.nb_upd = q.nb_upd = (int)std::min<size_t>(std::max<size_t>((nu + np_ + TPB - 1) / TPB, 1), (size_t)UPDATE_MAX_BLOCKS);
  P.note(build_colors(c));
  P.note(grow(&c->d_kry_minv, &c->kry_minv_n, (size_t)q.nn * NB * NB));
  P.note(grow(&c->d_kry_vec, &c->kry_vec_n, 9 * q.n));
  P.note(grow(&c->d_kry_part, &c->kry_part_n, 2 * (size_t)std::max(q.nb_node, q.nb_upd)));
  if (!c->d_kry_scalars) P.hip(hipMalloc(&c->d_kry_scalars, sizeof(KryScalars)), "hipMalloc");
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
  if (!P.failed) P.hip(hipMemcpyAsync(q.S, &h, sizeof(h), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
  if (!P.failed) P.hip(hipMemsetAsync(vec, 0, 9 * q.n * sizeof(double), st), "hipMemsetAsync");
  C8_PARTS_LAUNCH(P, (k_setup<ND, NRES>), xcd_grid(P.nb_own), TPB, nown, P.nb_own, c->d_nodeptr, c->d_nodeadj, q.A, q.minv, q.S);
  C8_PARTS_LAUNCH(P, (k_true_residual_own<ND, NRES>), xcd_grid(P.nb_own), TPB, nown, q.nn, P.nb_own, c->d_nodeptr, c->d_nodeadj, q.A, q.x, v[0], v[1],
                  q.r, q.rhat, q.p, q.v, q.part);
  C8_PARTS_LAUNCH(P, (k_reduce<3>), 1, TPB, q.part, P.nb_own, 0., q.S);
  if (!P.failed) P.hip(hipMemcpyAsync(&h, q.S, sizeof(KryScalars), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
  if (!P.failed) P.hip(hipStreamSynchronize(st), "hipStreamSynchronize");
  rc = parts_agree(P, who, h.bad_node != INT_MAX ? (double)h.bad_node : -1., [&](int r, long long node) {
    return fail(C8_ERR_ARG, "c8_krylov_precondition: the diagonal block of node " + std::to_string(node) + " (local id) of rank " + std::to_string(r) +
                            " is singular or not finite (node-block Jacobi preconditioner)");
  });
  if (rc != C8_OK) return rc;
  rc = parts_agree(P, who, (nown > 0 && !std::isfinite(h.rr)) ? 0. : -1., [&](int r, long long) {
    return fail(C8_ERR_ARG, "c8_krylov_precondition: the vector or the matrix is not finite on rank " + std::to_string(r));
  });
  if (rc != C8_OK) return rc;
  if (multi) parts_levels_setup<ND, NRES, G>(P, -1);
  else parts_coarse_setup<ND, NRES, G>(P, true);
  if ((rc = multi ? parts_levels_agree(P, who) : parts_coarse_agree(P, who)) != C8_OK) return rc;
  C8_PARTS_LAUNCH(P, (k_vec<1>), P.nb_upd, TPB, nu, np_, n0, q.r, q.v, q.s, q.shat, q.S);
  if (multi) parts_levels_apply<ND, NRES>(P, q.s, q.shat);
  else parts_coarse<ND, NRES>(P, q.s, q.shat);
  if (!P.failed) P.hip(launch_sgs<ND, NRES, G>(q, nown, q.s, q.shat, false), "k_sgs_color");
  if (!P.failed && nu > 0) P.hip(hipMemcpyAsync(y[0], q.shat, nu * sizeof(double), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
  if (!P.failed && NRES == 2 && np_ > 0) P.hip(hipMemcpyAsync(y[1], q.shat + n0, np_ * sizeof(double), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
  return parts_agree(P, who, -1., [&](int, long long) { return C8_OK; });
}
