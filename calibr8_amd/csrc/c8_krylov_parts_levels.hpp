// c8_krylov_parts_levels.hpp -- the aggregation preconditioners over the parts of a multi-part mesh: C8_PRECOND_TWO_LEVEL_PARTS
// (a list of one level) and C8_PRECOND_MULTILEVEL_PARTS (include/c8.h, DESIGN.md sections 13f, 13g, 13h).  Included by
// c8_krylov.hip inside its unnamed namespace, after the host side of the multi-part solve (Parts, C8_PARTS_LAUNCH,
// launch_sgs), c8_krylov_coarse.hpp (the aggregation rules, P, the kernels between level 0 and level 1, the dense last
// level) and c8_krylov_multilevel.hpp (the block levels, levels_begin / levels_form / levels_invert, the cycle).  The
// kernels are those files'; this one has the host path with the error discipline of Parts: a rank that fails goes on
// through every collective and the ranks agree on the outcome before every return.
//
//   aggregates   aggregate_graph over the OWNED sub-graph of every rank (columns >= num_owned dropped); global id = base of
//                the rank + local id, the counts of the ranks travel in one all-reduce of one slot per rank
//   imported     the owner's P_j at the ghost and phantom copies of node j: global aggregate id and offset from the
//                centroid once per attached halo, constrained flags at every set-up, all through the import (C3) tables
//   level 1      one node per aggregate of any rank.  Two-level kind: dense, only its size is known to the list.  Multilevel
//                kind: its graph (the neighbour lists of the ranks' own aggregates) and its positions (the centroids) are
//                REPLICATED on every rank by three host all-reduces in which every entry is written by one rank and is zero
//                elsewhere: exact, and bitwise equal everywhere
//   levels >= 2  extend_levels on that level 1: the same host code on the same bits gives every rank the same hierarchy
//                without a message
//   set-up       k_constrained (flags of the owned rows) -> import of the flags -> k_galerkin (this rank's block rows of A_1,
//                the other entries zero) -> one all-reduce of A_1 (dense: n * lda doubles; block-sparse: nnz_1 * NC^2) ->
//                levels_form, levels_invert on every rank; the ranks then agree on the outcome (parts_levels_agree)
//   apply        k_restrict (own slots of r_1, zeros elsewhere) -> one all-reduce of r_1 -> launch_level_cycle on every rank
//                (with one level: k_coarse_apply on the rows of the rank's own aggregates) -> k_prolong (x = P_0 e_1 on the
//                owned nodes), then the part-local sweeps of k_sgs_color started from this x: two imports and five
//                all-reduces per iteration
// Every entry of an all-reduced buffer is written by one rank and zero on the others: the sums are exact, for any number of
// parts and any order of summation.  Every other sum has a fixed order; no kernel uses a floating-point atomic.

// ---- the flags on their way through the import tables, which move doubles: component 0 of the node's u entries
__global__ void __launch_bounds__(TPB) k_flags_pack(int nown, int nd, int32_t const* __restrict__ flags, double* __restrict__ buf) {
  int const node = blockIdx.x * TPB + threadIdx.x;
  if (node < nown) buf[(size_t)node * nd] = (double)flags[node];
}
__global__ void __launch_bounds__(TPB) k_flags_unpack(int nown, int nn, int nd, double const* __restrict__ buf, int32_t* __restrict__ flags) {
  int const node = nown + blockIdx.x * TPB + threadIdx.x;
  if (node < nn) flags[node] = (int32_t)buf[(size_t)node * nd];
}

// ---- host side ----------------------------------------------------------------------------------------------------------

// the part of a Parts that the levels need, for the calls outside the solve
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

// level 0 of this rank: the tables of parts_level0_build, the counts of parts_aggregates
inline Level0 parts_level0(c8_ctx const* c, Parts const& P) {
  int32_t const* b = c->d_kry_pc_agg;
  size_t const* o = c->kry_pc_at;
  return Level0{AggTables{b + o[0], b + o[1], b + o[2], b + o[3], b + o[4], b + o[5], c->d_kry_pc_off, c->d_kry_pc_flags},
                (int)c->kry_pc_base, c->kry_pc_nagg, (int)c->kry_pc_total, P.nown, c->kry_pc_max_nbr};
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
  c->kry_pc_levels.assign(1, c8_kry_level{});  // the two-level kind's list: level 1, dense (used below the cap only)
  c->kry_pc_levels[0].n = (int)std::min<long long>(total, INT_MAX);
  c->kry_pc_host_for = nown;
  return C8_OK;
}

// What a call of the two-level kind over parts refuses before any device work, the same on every rank: the cap of the dense
// coarse solve on the GLOBAL count.  COLLECTIVE (parts_aggregates).
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

// The device tables of level 0: the owners' global aggregate ids and offsets imported at the copies, the node lists
// of the rank's aggregates, their neighbour lists over all ranks and the slot of every entry of the owned graph rows.  Once
// per attached halo (c8_halo_attach resets kry_pc_for) and when num_owned changes.  COLLECTIVE: two imports, and the
// agreement on device errors and on the tile of k_galerkin.  (The message keeps the name that kernel had while the kinds
// over parts had a copy of their own: the text is kept for the callers that match on it.)  Needs parts_aggregates().
int parts_level0_build(c8_ctx* c, Parts& P, char const* who) {
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
    H.nagg = c->kry_pc_nagg;
    H.ptr = c->kry_pc_ptr, H.nodes = c->kry_pc_nodes;
    neighbour_lists(H, total, c->graph.nodeptr, c->graph.nodeadj);  // over the whole owned rows, by global id
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

// Level 0 and the list of levels below it.  The two-level kind: its cap, the tables of level 0; the list is the one entry
// of parts_aggregates.  The multilevel kind (multi): the tables, then the replicated levels, once per attached halo, per
// num_owned and per setting of c8_krylov_set_multilevel; no cap on the last level here (c8_krylov_levels reports above it
// too).  COLLECTIVE: parts_aggregates, parts_level0_build, the three all-reduces of the replication and the agreement on a
// device error of the uploads.
int parts_levels_build(c8_ctx* c, Parts& P, char const* who, bool multi) {
  int rc;
  if (!multi) {
    if ((rc = parts_coarse_refusals(c, P, who)) != C8_OK) return rc;
    return parts_level0_build(c, P, who);
  }
  if (c->mesh.nnodes <= 0) return fail(C8_ERR_ARG, std::string(who) + ": empty mesh");
  if ((rc = parts_aggregates(c, P)) != C8_OK) return rc;
  int const nc = coarse_columns(c), nd = c->ndims;
  if (c->kry_pc_total * nc > (long long)INT_MAX)
    return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": level 1 of the multilevel preconditioner over parts has more than 2^31 unknowns");
  if ((rc = parts_level0_build(c, P, who)) != C8_OK) return rc;
  if (c->kry_pl_for == P.nown) return C8_OK;
  c->kry_pl_for = -1;
  free_level_list(c->kry_pl_levels);
  int const total = (int)c->kry_pc_total, base = (int)c->kry_pc_base, nagg = c->kry_pc_nagg;
  // every buffer below: this rank's entries in its own slots, zeros elsewhere; ids travel as doubles (exact below 2^53)
  std::vector<double> len(total, 0.);
  for (int a = 0; a < nagg; ++a) len[base + a] = (double)(c->kry_pc_nbr_ptr[a + 1] - c->kry_pc_nbr_ptr[a]);
  if ((rc = c8_comm_allreduce_sum(P.cm, len.data(), total)) != C8_OK) return rc;
  c8_kry_level L1;
  L1.n = total;
  L1.gp.assign(total + 1, 0);
  long long nnz = 0;
  for (int i = 0; i < total; ++i) {
    nnz += (long long)len[i];
    L1.gp[i + 1] = (int32_t)std::min<long long>(nnz, INT_MAX);
  }
  if (nnz * nc * nc > (long long)INT_MAX)  // (the same sum on every rank)
    return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": the matrix of level 1 of the multilevel preconditioner over parts has " + std::to_string(nnz) +
                                    " blocks: more than one all-reduce moves");
  std::vector<double> cols((size_t)nnz, 0.);
  if (L1.gp[base + nagg] - L1.gp[base] == (int32_t)c->kry_pc_nbr.size())
    for (size_t k = 0; k < c->kry_pc_nbr.size(); ++k) cols[(size_t)L1.gp[base] + k] = (double)c->kry_pc_nbr[k];
  if ((rc = c8_comm_allreduce_sum(P.cm, cols.data(), (int)nnz)) != C8_OK) return rc;
  L1.ga.resize((size_t)nnz);
  for (size_t k = 0; k < (size_t)nnz; ++k) L1.ga[k] = (int32_t)cols[k];
  std::vector<double> cen((size_t)total * nd, 0.);
  for (int a = 0; a < nagg; ++a)
    for (int d = 0; d < nd; ++d) cen[(size_t)(base + a) * nd + d] = c->kry_pc_x[(size_t)a * 3 + d];
  if ((rc = c8_comm_allreduce_sum(P.cm, cen.data(), total * nd)) != C8_OK) return rc;
  L1.x.assign((size_t)total * 3, 0.);
  for (int i = 0; i < total; ++i)
    for (int d = 0; d < nd; ++d) L1.x[(size_t)i * 3 + d] = cen[(size_t)i * nd + d];
  std::vector<c8_kry_level>& lv = c->kry_pl_levels;
  lv.push_back(std::move(L1));
  P.note(extend_levels(c, lv));
  if ((rc = parts_agree(P, who, -1., [&](int, long long) { return C8_OK; })) != C8_OK) return rc;
  c->kry_pl_for = P.nown;
  return C8_OK;
}

// What every entry of a kind over parts calls first: parts_levels_build, then what the kind refuses before anything is
// assembled or iterated, the same on every rank without a message -- a block row of a replicated level that does not fit
// the tile of k_level_galerkin, a last level of the multilevel kind above the cap of the dense solve (the two-level kind's
// cap comes before its tables, in parts_levels_build).  Leaves the list and level 0 in P.q.  COLLECTIVE.
int parts_levels_prepare(c8_ctx* c, Parts& P, char const* who, bool multi) {
  int const rc = parts_levels_build(c, P, who, multi);
  if (rc != C8_OK) return rc;
  std::vector<c8_kry_level> const& lv = multi ? c->kry_pl_levels : c->kry_pc_levels;
  int const nl = (int)lv.size(), nc = coarse_columns(c);
  for (int k = 0; k + 1 < nl; ++k)
    if ((size_t)lv[k].max_nbr * nc * nc * sizeof(double) > GALERKIN_LDS)
      return fail(C8_ERR_UNSUPPORTED, std::string(who) + ": an aggregate of level " + std::to_string(k + 1) + " has " + std::to_string(lv[k].max_nbr) +
                                      " neighbouring aggregates: the block row of a coarse matrix does not fit the tile of k_level_galerkin");
  long long const n = (long long)lv.back().n * nc;
  if (multi && n > COARSE_CAP)
    return fail(C8_ERR_UNSUPPORTED,
                std::string(who) + ": the multilevel preconditioner over parts solves its last level densely on every rank: level " + std::to_string(nl) +
                    " has n = " + std::to_string(n) + " unknowns (" + std::to_string(lv.back().n) + " aggregates over " + std::to_string(P.nranks) +
                    " parts), which exceeds the cap of " + std::to_string(COARSE_CAP) + "; " +
                    (nl + 1 >= ml_max_levels(c) ? "max_levels = " + std::to_string(ml_max_levels(c)) + " (c8_krylov_set_multilevel) ends the recursion there"
                                                    : std::string("aggregation no longer reduces the node count")));
  P.q.lv = &lv, P.q.multi = multi, P.q.l0 = parts_level0(c, P);
  return C8_OK;
}

// The constrained flags of the gathered matrix of P.q at every local node: the owned rows' by k_constrained, the copies'
// imported from their owners.  One import.
template <int ND, int NRES, int G>
void parts_flags(Parts& P) {
  Solve const& q = P.q;
  c8_ctx* c = q.c;
  int const nb_g = (P.nown + TPB / G - 1) / (TPB / G), nb_copy = (q.nn - P.nown + TPB - 1) / TPB;
  double* const imp = c->d_kry_pc_imp;
  double* const seg1 = NRES == 2 ? imp + (size_t)q.nn * ND : nullptr;
  C8_PARTS_LAUNCH(P, (k_constrained<ND, NRES, G>), xcd_grid(nb_g), TPB, P.nown, nb_g, c->d_nodeptr, c->d_nodeadj, q.A, c->d_kry_pc_flags);
  C8_PARTS_LAUNCH(P, k_flags_pack, P.nb_own, TPB, P.nown, ND, c->d_kry_pc_flags, imp);
  P.note(c8_halo_import_start(P.h, imp, seg1, P.failed));
  P.note(c8_halo_import_finish(P.h, imp, seg1, P.failed));
  C8_PARTS_LAUNCH(P, k_flags_unpack, nb_copy, TPB, P.nown, q.nn, ND, imp, c->d_kry_pc_flags);
}

// The levels of P.q (parts_levels_prepare) for the gathered matrix of P.q: A_1 .. A_upto (upto < 0: all levels, then the
// checked inverse of the last one).  A_1 is completed by one all-reduce: of the dense n * lda doubles when level 1 is the last
// level, else of the nnz_1 * NC^2 doubles of its blocks.  Errors go to P, the finding to kry_pc_bad; parts_levels_agree()
// after it gives every rank the same code.
template <int ND, int NRES, int G>
void parts_levels_setup(Parts& P, int upto) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  Solve const& q = P.q;
  c8_ctx* c = q.c;
  std::vector<c8_kry_level> const& lv = *q.lv;
  int const nl = (int)lv.size(), n = lv.back().n * NC, lda = (n + 1) & ~1;
  bool const invert = upto < 0;
  if (invert) upto = nl;
  c->kry_pc_bad = -1.;
  hipStream_t const st = c->stream;
  int32_t* info = nullptr;
  std::vector<int32_t> h_info;
  if (!P.failed) P.note(levels_begin<NC>(c, lv, &h_info, &info));
  parts_flags<ND, NRES, G>(P);
  double* const A1 = nl == 1 ? c->d_kry_Ac : lv[0].d_A;
  size_t const n1 = nl == 1 ? (size_t)n * lda : lv[0].ga.size() * NC * NC;
  if (!P.failed) P.hip(hipMemsetAsync(A1, 0, n1 * sizeof(double), st), "hipMemsetAsync");
  if (!P.failed) P.hip(launch_level0_galerkin<ND, NRES>(q), "k_galerkin");
  P.note(c8_comm_allreduce_device_long(P.cm, st, A1, n1, P.failed));
  if (!P.failed && nl > 1 && upto >= nl) P.hip(hipMemsetAsync(c->d_kry_Ac, 0, (size_t)n * lda * sizeof(double), st), "hipMemsetAsync");
  if (!P.failed) P.note(levels_form<ND, NRES>(c, lv, upto, info));
  if (!invert || P.failed) return;
  P.note(levels_invert<NC>(c, lv, info, &h_info));
  if (P.failed) return;
  double const two32 = 4294967296.;
  for (int k = nl - 2; k >= 0; --k)  // (the finding of the finest such level wins, as in levels_setup)
    if (h_info[3 + k] != INT_MAX) c->kry_pc_bad = (k + 1) * two32 + h_info[3 + k];
  if (c->kry_pc_bad < 0. && levels_bad_row(h_info) >= 0) c->kry_pc_bad = nl * two32 + levels_bad_row(h_info);
}

// the outcome of parts_levels_setup, agreed over the ranks, in the words of the kind.  (A singular level 1 that is the last
// level has the two-level kind's sentence with either kind: the text is kept.)  COLLECTIVE.
int parts_levels_agree(Parts& P, char const* who) {
  c8_ctx* c = P.q.c;
  int const nl = (int)P.q.lv->size(), nc = coarse_columns(c);
  long long const n = (long long)P.q.lv->back().n * nc;
  bool const multi = P.q.multi && nl > 1;
  return parts_agree(P, who, c->kry_pc_bad, [&](int r, long long f) {
    int const level = (int)(f >> 32);
    long long const at = f & 0xffffffffLL;
    if (level < nl)
      return fail(C8_ERR_ARG, std::string(who) + ": the diagonal block of aggregate " + std::to_string(at) + " (global id) on level " + std::to_string(level) +
                              " of the multilevel preconditioner over parts is singular or not finite, as found by rank " + std::to_string(r));
    if (!multi)
      return fail(C8_ERR_ARG, std::string(who) + ": the coarse matrix of the two-level preconditioner over parts is singular or not finite at aggregate " +
                              std::to_string(at / nc) + " (global id; coarse row " + std::to_string(at) + " of " + std::to_string(n) +
                              "), as found by rank " + std::to_string(r));
    return fail(C8_ERR_ARG, std::string(who) + ": the matrix of level " + std::to_string(nl) +
                            " (the last) of the multilevel preconditioner over parts is singular or not finite at aggregate " + std::to_string(at / nc) +
                            " (row " + std::to_string(at) + " of " + std::to_string(n) + "), as found by rank " + std::to_string(r));
  });
}

// x = P_0 M_1^-1 P_0^T rhs on the owned nodes: one all-reduce of the n_1 doubles of r_1 between the restriction and the
// cycle over the levels.  Every rank runs the cycle on the whole of the replicated levels; when level 1 is the last level
// the dense solve is all there is, and a rank forms only the rows of e_1 that it prolongs: those of its own aggregates.
template <int ND, int NRES>
void parts_levels_apply(Parts& P, double const* rhs, double* x) {
  constexpr int NC = CoarseDims<ND, NRES>::NC;
  Solve const& q = P.q;
  c8_ctx const* c = q.c;
  std::vector<c8_kry_level> const& lv = *q.lv;
  Level0 const& l0 = q.l0;
  int const wpb = TPB / 64;
  bool const one = lv.size() == 1;
  double *r1 = level_rhs<NC>(c, lv, 0), *e1 = level_x<NC>(c, lv, 0);
  C8_PARTS_LAUNCH(P, (k_restrict<ND, NRES>), (l0.total + wpb - 1) / wpb, TPB, l0.total, l0.base, l0.nagg, l0.T, q.nn, rhs, r1, q.S);
  P.note(c8_comm_allreduce_device_long(P.cm, c->stream, r1, (size_t)l0.total * NC, P.failed));
  if (!P.failed)
    P.hip(launch_level_cycle<ND, NRES>(c, lv, one ? l0.base * NC : 0, one ? l0.nagg * NC : lv.back().n * NC, q.S), "launch_level_cycle");
  C8_PARTS_LAUNCH(P, (k_prolong<ND, NRES>), xcd_grid(P.nb_own), TPB, P.nown, q.nn, P.nb_own, l0.T, e1, x, q.S);
}

int build_colors(c8_ctx* c);

// c8_krylov_precondition with a kind over parts selected and a halo attached: y = M^-1 v on the owned entries.  COLLECTIVE:
// the set-up of the levels and the all-reduce of the apply; the refusals (a bad diagonal block, a vector or matrix that is
// not finite, a singular level) are agreed over the ranks.
template <int ND, int NRES, int G>
int precondition_parts(c8_ctx* c, const c8_system* sys, const double* const v[2], double* const y[2]) {
  constexpr int NB = ND + (NRES == 2 ? 1 : 0);
  char const* who = "c8_krylov_precondition";
  Parts P = parts_of(c);
  Solve& q = P.q;
  if (q.nn <= 0) return fail(C8_ERR_ARG, "c8_krylov_precondition: empty mesh");
  int rc = parts_levels_prepare(c, P, who, c->kry_precond == C8_PRECOND_MULTILEVEL_PARTS);
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
  parts_levels_setup<ND, NRES, G>(P, -1);
  if ((rc = parts_levels_agree(P, who)) != C8_OK) return rc;
  C8_PARTS_LAUNCH(P, (k_vec<1>), P.nb_upd, TPB, nu, np_, n0, q.r, q.v, q.s, q.shat, q.S);
  parts_levels_apply<ND, NRES>(P, q.s, q.shat);
  if (!P.failed) P.hip(launch_sgs<ND, NRES, G>(q, nown, q.s, q.shat, false), "k_sgs_color");
  if (!P.failed && nu > 0) P.hip(hipMemcpyAsync(y[0], q.shat, nu * sizeof(double), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
  if (!P.failed && NRES == 2 && np_ > 0) P.hip(hipMemcpyAsync(y[1], q.shat + n0, np_ * sizeof(double), hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
  return parts_agree(P, who, -1., [&](int, long long) { return C8_OK; });
}
