// c8_api_internal.hpp -- the context behind the opaque c8_ctx of include/c8.h, shared by the
// translation units that implement the C ABI.
#pragma once

#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "../../include/c8.h"
#include "c8_host.hpp"
#include "c8_kernels.hpp"

int c8_fail(int code, std::string const& msg);  // records c8_last_error() and returns code

// a level l >= 1 of an aggregation preconditioner (c8_krylov_multilevel.hpp): one node per aggregate of the level above.
// Over parts only n is set in the one-level list of the two-level kind (the dense last level needs no more).
struct c8_kry_level {
  int n = 0;                          // nodes
  std::vector<int32_t> gp, ga;        // graph: the neighbour lists of the aggregates it came from (sorted, self included)
  std::vector<double> x;              // [n][3] positions: the centroids of those aggregates
  // ... what follows only where a level below exists (not on the last level, which is dense)
  int nagg = 0, max_nbr = 0;          // aggregates of this level's nodes; most neighbouring aggregates of one of them
  std::vector<int32_t> agg_of;        // [n]
  std::vector<int32_t> color_ptr, color_nodes;  // colour lists of the level's sweeps (layout of kry_color_*)
  int32_t* d_graph = nullptr;         // gp, then ga
  int32_t* d_agg = nullptr;           // layout of c8_ctx::d_kry_agg
  size_t agg_at[6] = {0, 0, 0, 0, 0, 0};
  double* d_off = nullptr;            // [n][ndims] node - centroid of its aggregate
  int32_t* d_flags = nullptr;         // [n] constrained-row flags of the current matrix
  int32_t* d_colors = nullptr;        // device mirror of color_nodes
  double* d_A = nullptr;              // [graph entries][NC * NC] block-sparse matrix of the level
  double* d_minv = nullptr;           // [n][NC * NC] inverses of the diagonal blocks
  double* d_vec = nullptr;            // right-hand side and iterate of the level, [n][NC] each
};

// superconvergent patch recovery (c8_spr.hip): the tables of c8_spr_recover, built at its first call
struct c8_spr_tables {
  bool built = false;
  double* d_pts = nullptr;            // [nelems][coupled points][ndims] sample positions
  double* d_g = nullptr;              // [nnodes][ndims + 1]
  double* d_h = nullptr;              // [nnodes]
  int64_t* d_patch_ptr = nullptr;     // [nnodes + 1]
  int32_t* d_patch_elems = nullptr;
  std::vector<int64_t> patch_ptr;     // host copies (c8_spr_table)
  std::vector<int32_t> patch_elems, stages;
  std::vector<double> g, h;
  double info[4] = {0., 0., 0., 0.};  // set-up: ms on the device, ms on the host, ms of upload, flagged nodes
};

struct c8_ctx {
  // (namespace c8 types)
  c8::HostMesh mesh;
  c8::HostGraph graph;
  std::vector<int32_t> order, color_off;
  int model = c8::MODEL_NONE;
  int nloc = 0, nparams = 0, npts0 = 0;
  int ndims = 3;                      // 3, or 2 on tri3 meshes: u has ndims equations per node
  int nres = 2;                       // global residuals: 2 (`mechanics`: u, p), 1 (`mechanics_plane_stress`: u)
  c8::ModelSettings ms{};
  std::vector<double> params;
  std::vector<std::vector<int32_t>> active;
  c8::KernelSet ks{};
  // device mirrors
  int32_t* d_conn = nullptr;
  double* d_coords = nullptr;
  int32_t* d_nodeptr = nullptr;
  int32_t* d_nodeadj = nullptr;   // node-graph columns (boundary conditions, A x)
  double* d_scalar = nullptr;     // reduction result
  double* d_work[4] = {nullptr, nullptr, nullptr, nullptr};  // Newton driver: dx[2], A dx[2]
  double* d_xi_saved = nullptr;   // Newton driver: local state at the base point of a line search
  uint8_t* d_pos = nullptr;
  int32_t* d_elem_set = nullptr;
  int32_t* d_order = nullptr;
  int32_t* d_nodeelem_ptr = nullptr;  // node -> elements (staged assembly)
  int32_t* d_nodeelem = nullptr;
  double* d_stage = nullptr;          // [ring][stage_stride], allocated at the first staged assembly
  int32_t* d_node_order = nullptr;
  c8::StagePlan plan;                 // staged assembly: chunks, ring, node order
  int stage_min_chunk = 0;            // 0: automatic (c8_api.hip: stage_setup)
  // staged assembly with the row sums of chunk k beside the assembly of chunk k + 1 (c8_set_stage_overlap): the row-sum
  // launches go to sum_stream, events order the two streams both ways
  int stage_overlap = 0;
  hipStream_t sum_stream = nullptr;
  std::vector<hipEvent_t> ev_asm, ev_sum;
  // staged assembly in two parts (c8_set_gather_early_nodes): the rows of nodes [early_begin, early_end) are summed by
  // the assembly call, the other rows by c8_gather_finish
  int early_begin = 0, early_end = 0, early_count = 0;
  bool gather_pending = false;
  c8::GatherArgs pending_ga{};
  // row-per-node forward assembly (C8_KERNEL_NODE) in two parts: the fields the second part reads
  bool pending_node_rows = false, pending_adjoint = false;
  c8::FieldArgs pending_fa{};
  c8::AdjointArgs pending_aa{};
  double* d_shape = nullptr;          // cached shape tables of the wave kernels, [nelems][ks.shape_stride] (hex8; null: computed per call)
  double* d_params = nullptr;
  double* d_cf_const = nullptr;  // [nsets][ks.num_constants]: MeshTables::cf_const, refilled whenever d_params is written (fill_constants)
  int32_t* d_active = nullptr;  // [nsets][10]: {grad offset, n_active, indices...}
  int* d_status = nullptr;
  unsigned long long* d_stamps = nullptr;  // -DC8_STAMPS diagnostic build only
  // objective: 0 = average displacement, 1 = calibration, 3 = reaction (c8_qoi.hip), 2 = subdomain (c8_qoi_point.hip)
  int qoi_kind = 0;
  int sub_kind = 0, sub_set = 0, sub_index = 0;  // c8_subdomain_qoi_desc
  double* d_qoi_rec = nullptr;      // [nelems][points][QOI_REC] x-records of the points, from the pre-pass to the post-pass
  double* d_qoi_part = nullptr;     // [8][blocks] per-block partial sums of the value and the gradient kernel
  int32_t* d_cal_faces = nullptr;   // [cal_nfaces][4] node ids of the element faces on the displacement side set
  double* d_cal_S = nullptr;        // [nelems][coupled points][3] load-plane sums of grad N
  double const* d_u_meas = nullptr; // caller's measured displacement of the current step (device)
  int cal_nfaces = 0, cal_nf = 0, cal_comp = 0;
  double cal_area = 0., cal_w[3] = {1., 1., 1.}, cal_balance = 0., cal_dt_over_T = 1.;
  double cal_load_meas = 0., cal_total_load = 0., cal_load_mismatch = 0.;
  double cal_area_local = 0.;       // this part's share of the side-set area
  c8_allreduce_fn allreduce = nullptr;  // SUM over the parts (null: one part)
  void* allreduce_user = nullptr;
  int num_parts = 1;
  c8_halo* halo = nullptr;              // multi-part mesh: exchanges and reductions (c8_halo_attach), not owned
  hipStream_t stream = nullptr;
  int scatter_mode = C8_SCATTER_COLORED;
  bool scatter_auto = false;         // the mode was chosen by c8_create, not by the caller (see run() in c8_api.hip)
  int kernel_variant = C8_KERNEL_AUTO;
  int assign_mode = 0;               // staged Jacobian assemblies assign their outputs instead of adding to them
  int async = 0;
  int32_t const* subset = nullptr;   // set for the duration of a *_subset call
  int subset_count = 0;
  // virtual fields method (c8_vfm.hip)
  double const* d_vfm_w = nullptr;   // caller's virtual field (device, kept by pointer)
  double* d_vfm_part = nullptr;      // per-block partial sums of the VFM kernels
  size_t vfm_part_n = 0;
  // embedded network of hybrid_hyper_J2_plane_stress (c8_embedded.hip)
  std::vector<double> nn_host;       // the device buffer's contents (c8_models.hpp: nn_value_slope)
  int nn_ntheta = 0;                 // 0: no network described yet
  bool nn_ready = false;             // the network and its weights are set
  double* d_nn = nullptr;
  double* d_nn_part = nullptr;       // per-block partial rows of the weight-gradient kernel
  size_t nn_part_n = 0;
  // device-resident Krylov solve (c8_krylov.hip): node-block Jacobi inverses, work vectors, dot partials and scalars
  double* d_kry_minv = nullptr;      // [nnodes][NB * NB]
  double* d_kry_vec = nullptr;       // nine vectors of the system's length (x, r, rhat, p, v, s, t, phat, shat)
  double* d_kry_part = nullptr;      // per-block partial sums of the inner products
  void* d_kry_scalars = nullptr;     // rho, alpha, omega, beta, |r|^2, stop flag, iteration count (+ the set-up kernel's flag)
  size_t kry_minv_n = 0, kry_vec_n = 0, kry_part_n = 0;
  // ... over parts (c8_krylov_solve_parts): the owned nodes without / with a ghost or phantom column, interior first
  std::vector<int32_t> kry_list;
  int kry_list_owned = -1;           // num_owned the lists were built for (-1: not built)
  int kry_n_interior = 0;
  int32_t* d_kry_list = nullptr;
  double* d_kry_sums = nullptr;      // the local sums of an inner product, all-reduced in place
  // ... preconditioner of both solves (c8_krylov_set_preconditioner) and the colour lists of the Gauss-Seidel sweeps:
  // nodes kry_color_nodes[kry_color_ptr[c] .. kry_color_ptr[c + 1]) have colour c (ascending); all nodes, or the owned
  // nodes coloured over the owned sub-graph when a halo is attached
  int kry_precond = C8_PRECOND_BLOCK_JACOBI, kry_sweeps = 1;
  std::vector<int32_t> kry_color_ptr, kry_color_nodes;
  int kry_colors_for = -2;           // what the colour lists were built for: -1 no halo, else num_owned (-2: not built)
  int32_t* d_kry_colors = nullptr;   // device mirror of kry_color_nodes
  // ... level 0 of C8_PRECOND_TWO_LEVEL and C8_PRECOND_MULTILEVEL (c8_krylov_coarse.hpp): aggregates of the node graph, built
  // at first use, and the dense last level of every aggregation kind
  int kry_nagg = -1;                 // number of aggregates (-1: not built)
  int kry_agg_max_nbr = 0;           // most neighbouring aggregates of one aggregate (itself included)
  std::vector<int32_t> kry_agg_of;   // [nnodes] aggregate of a node (c8_krylov_aggregates)
  int32_t* d_kry_agg = nullptr;      // one buffer: aggregate of a node, node lists, neighbour lists, slot of every graph entry
  size_t kry_agg_at[6] = {0, 0, 0, 0, 0, 0};  // ... where each of them starts
  double* d_kry_agg_off = nullptr;   // [nnodes][ndims] node - centroid of its aggregate
  int32_t* d_kry_cflags = nullptr;   // [nnodes] constrained-row flags of the current matrix
  double* d_kry_Ac = nullptr;        // A_c, then its inverse: dense, row-major, even leading dimension
  double* d_kry_cvec = nullptr;      // r_c and e
  int32_t* d_kry_ipiv = nullptr;     // pivots of the LU factorisation, then the status words of the set-up (3 + one per level)
  size_t kry_Ac_n = 0, kry_cvec_n = 0, kry_ipiv_n = 0;
  void* kry_rocblas = nullptr;       // rocblas_handle of the dense inverse (workspace inside), made at first use
  std::vector<c8_kry_level> kry_agg_levels;           // the list of C8_PRECOND_TWO_LEVEL: level 1 alone (n, graph = the neighbour
                                                      // lists of the aggregates, positions = their centroids); no device buffers
  // ... the levels of C8_PRECOND_MULTILEVEL below level 0 (c8_krylov_multilevel.hpp), built at first use and again after
  // c8_krylov_set_multilevel: a copy of kry_agg_levels extended downwards, a list of its own so that switching between
  // the kinds rebuilds neither
  int kry_ml_coarse_max = 0, kry_ml_max_levels = 0;   // (set by c8_krylov.hip: <= 0 until the first use = the defaults)
  bool kry_ml_built = false;
  std::vector<c8_kry_level> kry_levels;               // [k] is level k + 1; freed by c8_krylov_release
  // ... level 0 of C8_PRECOND_TWO_LEVEL_PARTS and C8_PRECOND_MULTILEVEL_PARTS (c8_krylov_parts_levels.hpp): aggregates of
  // the owned sub-graph
  int kry_pc_host_for = -1;          // num_owned the host lists and the counts were built for (-1: not built)
  int kry_pc_for = -1;               // num_owned the device tables were built for (-1: not built; reset by c8_halo_attach)
  int kry_pc_nagg = 0, kry_pc_max_nbr = 0;                   // this rank's aggregates; widest block row
  double kry_pc_bad = -1.;           // finding of the last set-up of either kind: level * 2^32 + block or row (-1: none)
  long long kry_pc_base = 0, kry_pc_total = 0;               // aggregates of the ranks below this one, of all ranks
  std::vector<int32_t> kry_pc_agg_of, kry_pc_ptr, kry_pc_nodes;  // [num_owned] LOCAL aggregate ids; node lists of the aggregates
  std::vector<double> kry_pc_off;    // [num_owned][ndims] node - centroid
  int32_t* d_kry_pc_agg = nullptr;   // layout of d_kry_agg: GLOBAL aggregate of every local node, node lists, neighbour lists, slots
  size_t kry_pc_at[6] = {0, 0, 0, 0, 0, 0};
  double* d_kry_pc_off = nullptr;    // [nnodes][ndims], the copies' entries imported from their owners
  int32_t* d_kry_pc_flags = nullptr; // [nnodes] constrained-row flags of the current matrix, the copies' imported
  double* d_kry_pc_imp = nullptr;    // a vector's worth of doubles: what the import tables move the ids and the flags in
  std::vector<c8_kry_level> kry_pc_levels;            // the list of C8_PRECOND_TWO_LEVEL_PARTS: level 1 alone, n = kry_pc_total
  // ... the levels of C8_PRECOND_MULTILEVEL_PARTS below level 0: level 1 is the graph of
  // the aggregates of all ranks, replicated on every rank from the lists below; a list of its own, so that switching
  // between the kinds rebuilds neither
  std::vector<int32_t> kry_pc_nbr_ptr, kry_pc_nbr;  // neighbouring aggregates (GLOBAL ids, ascending) of this rank's aggregates
  std::vector<double> kry_pc_x;      // [kry_pc_nagg][3] centroids of this rank's aggregates
  int kry_pl_for = -1;               // num_owned the levels were built for (-1: not built; reset by c8_halo_attach and c8_krylov_set_multilevel)
  std::vector<c8_kry_level> kry_pl_levels;            // [k] is level k + 1; freed by c8_krylov_release
  c8_spr_tables spr;
};
void c8_spr_release(c8_ctx* c);      // c8_spr.hip: frees the recovery tables
void c8_krylov_release(c8_ctx* c);   // c8_krylov.hip: what c8_destroy cannot free with hipFree
// c8_embedded.hip: grad[c8_num_active_params ..] += the weight gradient (hybrid model; no-op for the others)
int c8_embedded_param_gradient(c8_ctx* c, const c8_state* st, const double* phi, double* grad);


// c8_qoi.hip
c8::QoiArgs c8_qoi_args(c8_ctx const* c);
int c8_qoi_prepare(c8_ctx* c, c8::FieldArgs const& fa);
int c8_qoi_surface(c8_ctx* c, double const* u, double* J, double* b0);
int c8_qoi_postprocess(c8_ctx* c, double* J);
int c8_qoi_reaction_value(c8_ctx* c, c8::FieldArgs const& fa, double* J);  // *J += the total load / num_parts
// c8_qoi_point.hip: the subdomain objectives beside the adjoint kernels (qoi_kind == 2)
int c8_subqoi_value(c8_ctx* c, c8::FieldArgs const& fa, double* J);  // *J += the value of the step
int c8_subqoi_pre(c8_ctx* c, c8::FieldArgs const& fa, double* g);    // before K3: g -= dJ/dxi
int c8_subqoi_post(c8_ctx* c, double* b0, double* b1);               // after K3: b -= dJ/dx
int c8_subqoi_grad(c8_ctx* c, c8::FieldArgs const& fa, double* grad);  // with K5: grad += dJ/dp
// c8_halo.hip: multi-part helpers for the other translation units
int c8_parts_allreduce(c8_ctx* c, double* values, int n);  // SUM over the parts: caller's callback, else the halo's communicator; no-op on one part
int c8_halo_num_owned(c8_halo const* h);
void c8_halo_detach_ctx(c8_ctx* c);  // c8_destroy: the halo attached to c (if any) forgets the context and its communicator
// ... for the multi-part Krylov solve (c8_krylov.hip).  `degraded`: this rank has met a device error and only keeps the
// collective sequence of the other ranks going (host transport: the callbacks are entered with the host buffers, NaN in an
// all-reduce; no device work); its return values are then meaningless.
int c8_halo_rank(c8_halo const* h);
int c8_halo_num_ranks(c8_halo const* h);
c8_comm* c8_halo_comm(c8_halo const* h);
int c8_halo_import_start(c8_halo* h, double* v0, double* v1, bool degraded);   // C3 of the vector {v0, v1}: pack and send
int c8_halo_import_finish(c8_halo* h, double* v0, double* v1, bool degraded);  // ... store what arrived in the copies
// in-place SUM over the ranks of n <= 64 doubles in DEVICE memory, ordered after and before the work on `stream`
int c8_comm_allreduce_device(c8_comm* cm, hipStream_t stream, double* d_values, int n, bool degraded);
// ... of a device buffer of any length (the coarse matrix and the coarse residual of C8_PRECOND_TWO_LEVEL_PARTS)
int c8_comm_allreduce_device_long(c8_comm* cm, hipStream_t stream, double* d_values, size_t n, bool degraded);
