/* c8.h -- C ABI of the MI355X assembly / adjoint-sensitivity path of CALIBR8.
 *
 * This is the drop-in boundary.  Each entry point replaces one
 * of the reference's `eval_*` free functions (source/calibr8/src/evaluations.hpp:23-84);
 * the arrays it reads and writes are the raw arrays those functions reach through
 * Tpetra / apf today:
 *   nodal fields x[i]     disc->primal(step).global[i]          (evaluations.cpp:24-27)
 *   point fields xi       disc->primal(step).local[model_form]  (apf IP fields)
 *   A[i][j]               la->A[GHOST][i][j] local CSR `values` (global_residual.cpp:529-537)
 *   b[i]                  la->b[GHOST][i]  get1dViewNonConst()  (global_residual.cpp:469)
 * Residual index 0 = u (3 equations per node), 1 = p (1 equation per node):
 * `mechanics` with the mixed formulation (mechanics.cpp:16-55).  Local row id of
 * (node, eq) in block i is node*neq_i + eq (disc.cpp:263-265 get_dof).
 *
 * Conventions
 *   - No exceptions, no C++ types.  Every function returns an int status:
 *       C8_OK (0); C8_LOCAL_SOLVE_FAILED (-1) = some local Newton solve did not converge,
 *       outputs undefined -- the reference's convention (evaluations.hpp:19,
 *       evaluations.cpp:95-97); < -1 = API misuse or device error, see c8_last_error().
 *   - c8_mesh_desc / c8_model_desc hold HOST pointers, copied at c8_create().
 *   - c8_state / c8_system and all other array arguments of the assembly calls are
 *     DEVICE pointers (HBM).  The caller owns them.
 *   - Outputs A, b, grad are ACCUMULATED INTO (+=), like scatter_lhs/scatter_rhs
 *     (global_residual.cpp:463-479,556-586); the caller zeroes first (primal.cpp:98).
 *   - One in-flight call per ctx; different ctxs (different GPUs/streams) are independent.
 */
#ifndef C8_H
#define C8_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct c8_ctx c8_ctx;

enum { C8_ELEM_TRI3 = 3, C8_ELEM_TET4 = 4, C8_ELEM_HEX8 = 8 };
enum { C8_OK = 0, C8_LOCAL_SOLVE_FAILED = -1, C8_ERR_ARG = -2, C8_ERR_DEVICE = -3, C8_ERR_UNSUPPORTED = -4 };
/* ATOMIC: one launch, f64 atomic adds.  COLORED: one launch per element colour, plain adds, reproducible.
 * GATHER: element matrices are staged element-major in a context-owned buffer (8.4 KB per hex8, 2.2 KB per
 * tet4 element) and a second kernel sums each node's rows in ascending element order: no atomics, bitwise
 * reproducible; the fastest mode on both element types and the DEFAULT of c8_create wherever no node has more than
 * 64 neighbours.  If the stage cannot be allocated at the first Jacobian assembly, a context still in its default
 * mode switches to COLORED and says so in c8_last_error(). */
enum { C8_SCATTER_ATOMIC = 0, C8_SCATTER_COLORED = 1, C8_SCATTER_GATHER = 2 };
enum { C8_KERNEL_AUTO = 0, C8_KERNEL_SLOT = 1, C8_KERNEL_WAVE = 2, C8_KERNEL_WAVE_AD = 3, C8_KERNEL_NODE = 4 };

/* One mesh part (what Disc holds after loadMdsMesh, disc.cpp:31-39): all nodes that touch a
 * local element, local (GHOST) numbering. */
typedef struct {
  int32_t elem_type;       /* C8_ELEM_TET4 / C8_ELEM_TRI3 (what the reference runs in 3-D / 2-D, disc.cpp:165) or
                              C8_ELEM_HEX8.  On a tri3 mesh `mechanics` has 2 + 1 equations per node (mechanics.cpp:34):
                              every u array is [num_nodes*2]; coords stay [num_nodes][3] with z = 0. */
  int32_t num_nodes;
  int32_t num_elems;
  int32_t num_elem_sets;   /* material blocks, disc->num_elem_sets() */
  const double* coords;    /* [num_nodes][3] */
  const int32_t* conn;     /* [num_elems][nodes per element], local node ids */
  const int32_t* elem_set; /* [num_elems] element-set id, or NULL when num_elem_sets == 1 */
  /* Extra (row node, col node) couplings to reserve in the graphs besides those of the local
   * elements: on a multi-part mesh, the off-part columns of owned interface rows, so that the owned
   * rows already have the union pattern of compute_owned_graph (disc.cpp:389-398) and the halo
   * ADD of linear_alg.cpp:53-63 can land in place.  NULL / 0 on a single part. */
  int32_t num_extra_pairs;
  const int32_t* extra_pairs; /* [num_extra_pairs][2] */
} c8_mesh_desc;

/* The `residuals:` block of a deck (global_residual.cpp:620-630, local_residual.cpp:893-933). */
typedef struct {
  const char* global_type;          /* "mechanics" (mixed u-p formulation, two residuals), or on tri3 meshes
                                       "mechanics_plane_stress" (mechanics_plane_stress.cpp: ONE residual, u; it pairs
                                       with the *_plane_stress local residuals and only with them) */
  const char* local_type;           /* "elastic" | "small_J2" | "hyper_J2" | "small_hill" | "isotropic_elastic" |
                                       "hypo_hill" | "small_hosford" | "hypo_hosford" | "hypo_barlat"; on tri3 meshes "small_J2" | "small_hill_plane_strain" |
                                       "hyper_J2_plane_strain" | "hypo_hill_plane_strain", and under
                                       mechanics_plane_stress "small_hill_plane_stress" | "hyper_J2_plane_stress" |
                                       "hypo_hill_plane_stress" | "hybrid_hyper_J2_plane_stress" (the names of
                                       local_residual.cpp:893-933; the hybrid model needs c8_set_embedded_model) */
  double stabilization_multiplier;  /* mechanics.cpp:47 */
  int32_t local_max_iters;          /* "nonlinear max iters" of the local residual */
  double local_abs_tol;             /* "nonlinear absolute tol" */
  double local_rel_tol;             /* "nonlinear relative tol" */
  int32_t num_params;               /* elastic 4 (E nu cte delta_T), small_J2 6 (E nu K Y cte delta_T),
                                       hyper_J2 8 (E nu Y S D A n K), small_hill / hypo_hill 11 (E nu Y R00 R11 R22
                                       R01 R02 R12 S D), isotropic_elastic 2 (E nu), small_hosford / hypo_hosford 7 (E nu Y a K S D),
                                       hypo_barlat 25 (those seven + sp_01 sp_02 sp_10 sp_12 sp_20 sp_21 sp_33 sp_44 sp_55
                                       and dp_01 .. dp_55), small_hill_plane_strain /
                                       hypo_hill_plane_strain 9 (E nu Y S D R00 R11 R22 R01), hyper_J2_plane_strain 6 (E nu K Y Y_inf delta),
                                       small_hill_plane_stress 9 (as plane strain), hyper_J2_plane_stress 8 (as hyper_J2),
                                       hypo_hill_plane_stress 13 (the nine + Q00 Q01 Q10 Q11),
                                       hybrid_hyper_J2_plane_stress 3 (E nu Y) */
  const double* params;             /* [num_elem_sets][num_params] */
  double thickness;                 /* mechanics_plane_stress.cpp:22 "thickness"; 0 = the reference's default 1 */
  /* `line search:` sublist of the local residual (line_search.hpp:40-49), used by the local Newton iteration of
   * small_hosford / hypo_hosford / hypo_barlat; 0 in a field = the reference's default (1e-4, 0.5, 0.9, 4 evaluations) */
  double ls_sufficient_decrease;
  double ls_min_backtrack;
  double ls_max_backtrack;
  int32_t ls_max_evals;
} c8_model_desc;

/* Primal state at one load step (DEVICE pointers).  Under mechanics_plane_stress (c8_num_residuals() == 1) the entries
 * [1] of a state, of a system (A[i][j] with i or j = 1, b[1]) and of an adjoint vector z are not read and may be NULL. */
typedef struct {
  const double* x[2];      /* x[0] = u [num_nodes*3], x[1] = p [num_nodes]  at step n   */
  const double* x_prev[2]; /* same at step n-1                                           */
  const double* xi_prev;   /* [num_elems][c8_num_local_points][c8_num_local_dofs], step n-1 */
  double* xi;              /* same at step n: written by the forward assembly, read by the others */
} c8_state;

/* Linear system in GHOST distribution (DEVICE pointers). */
typedef struct {
  double* A[2][2]; /* CSR values over the graphs reported by c8_graph() */
  double* b[2];    /* b[0] [num_nodes*3], b[1] [num_nodes] */
} c8_system;

/* ---- lifetime ------------------------------------------------------------------------- */
/* Builds host tables (node graph, element colouring) and their device mirrors on the current
 * HIP device.  Replaces State::State + Disc::build_data for this path (state.cpp:33-46,
 * disc.cpp:563-583). */
int c8_create(const c8_mesh_desc* mesh, const c8_model_desc* model, c8_ctx** out);
void c8_destroy(c8_ctx* ctx);
const char* c8_last_error(void);
/* "id=<sha of sources and flags> flags=<compiler flags>" of this library build (calibr8_amd/build.py): profiles carry
 * the id of the build they were measured on. */
const char* c8_build_info(void);

/* ---- discretisation queries (host arrays) ------------------------------------------------ */
int c8_num_local_dofs(const c8_ctx* ctx);    /* LocalResidual::num_dofs: 1 / 7 / 8 (3-D), 4 (2-D) */
int c8_num_dims(const c8_ctx* ctx);          /* 3, or 2 on a tri3 mesh: equations per node of residual 0 */
int c8_num_residuals(const c8_ctx* ctx);     /* GlobalResidual::num_residuals: 2 (mechanics: u, p) or 1 (mechanics_plane_stress: u) */
int c8_num_local_points(const c8_ctx* ctx);  /* points of the local-state field per element */
int c8_num_colors(const c8_ctx* ctx);
/* Block (i,j) CSR graph = m_graphs[GHOST][i][j] (disc.cpp:356-387): sorted columns. */
int64_t c8_graph_nnz(const c8_ctx* ctx, int i, int j);
int c8_graph(const c8_ctx* ctx, int i, int j, int64_t* rowptr, int32_t* colidx);
/* LocalResidual::init_variables (local_residual.cpp:35-74): initial local state, HOST array
 * [num_elems][points][dofs]. */
int c8_init_variables(const c8_ctx* ctx, double* xi_host);

/* ---- run-time settings ------------------------------------------------------------------- */
int c8_set_params(c8_ctx* ctx, const double* params_host); /* LocalResidual::set_params; [sets][num_params] */
/* Active (differentiated) parameters of one element set, LocalResidual::m_active_indices
 * (small_J2.cpp:96-98 default = {0}; objective.cpp:110-115 overrides from the inverse block). */
int c8_set_active_params(c8_ctx* ctx, int elem_set, int n, const int32_t* param_idx);
int c8_num_active_params(const c8_ctx* ctx); /* total over element sets = length of grad */

/* ---- embedded network of "hybrid_hyper_J2_plane_stress" (hybrid_hyper_J2_plane_stress.cpp, NN.cpp) ----------------
 * The hardening is sigma_y = Y + output_scale (NN(input_scale alpha) - NN(0)) with a feed-forward network NN: hidden
 * layers x_{i+1} = act(W_i x_i + b_i), a linear last layer.  The entries map to the deck's `embedded model` sublist:
 *   activation    "activation function": "relu" -> C8_ACT_RELU, "sigmoid" -> C8_ACT_SIGMOID, "tanh" -> C8_ACT_TANH
 *   topology      "topology" (num_layers entries, at least 3; input and output width 1, at most 4 hidden layers of at
 *                 most 64 units; HOST array, copied)
 *   input_scale   "input scale";  output_scale  "output scale"
 *   theta         "read parameters": the file nn_params.in, one value per line, in the order of c8_set_embedded_params
 * NN(0) is evaluated on the device by the code that evaluates NN(input_scale alpha), so the hardening is exactly Y at
 * alpha = 0.  The weights theta are the reference's DFAD parameters: layer by layer W_i row-major (topology[i+1] rows,
 * topology[i] columns), then b_i.  c8_param_gradient and c8_adjoint_solve_step append their gradient to grad:
 * grad[c8_num_active_params .. + c8_num_embedded_params) (evaluations.cpp:873-879); that needs a mesh with one element
 * set (main_objective.cpp:259-261, else C8_ERR_UNSUPPORTED).  Assemblies of a hybrid context return C8_ERR_ARG until
 * the network and theta are set.  The c8_vfm_* entry points do not support the hybrid model. */
enum { C8_ACT_RELU = 0, C8_ACT_SIGMOID = 1, C8_ACT_TANH = 2 };
typedef struct {
  int32_t activation, num_layers;
  const int32_t* topology;  /* HOST, copied */
  double input_scale, output_scale;
} c8_embedded_model_desc;
int c8_set_embedded_model(c8_ctx* ctx, const c8_embedded_model_desc* desc); /* C8_ERR_UNSUPPORTED for other models */
int c8_num_embedded_params(const c8_ctx* ctx);                               /* 0 for other models */
int c8_set_embedded_params(c8_ctx* ctx, const double* theta_host);
int c8_get_embedded_params(const c8_ctx* ctx, double* theta_host);
int c8_num_grad_params(const c8_ctx* ctx); /* c8_num_active_params + c8_num_embedded_params = length of grad */
int c8_set_stream(c8_ctx* ctx, void* hip_stream);
int c8_set_scatter_mode(c8_ctx* ctx, int mode); /* C8_SCATTER_GATHER (default, see above), C8_SCATTER_ATOMIC or C8_SCATTER_COLORED */
int c8_get_scatter_mode(const c8_ctx* ctx);
/* C8_SCATTER_GATHER tuning: elements are staged in chunks of at least `min_chunk` elements (the chunk is never
 * smaller than the element bandwidth of the mesh) through a ring of three chunks.  Default: the whole mesh in one
 * chunk while its stage stays under 12 GB (8.4 KB per hex8, 2.2 KB per tet4 element), else chunks of 262144. */
int c8_set_stage_chunk(c8_ctx* ctx, int min_chunk);
/* C8_SCATTER_GATHER in several chunks: on = 1 issues the row sums of chunk k on a stream of the context's own, beside
 * the assembly of chunk k + 1 on the caller's stream (events order the two both ways; the caller's stream continues
 * only after the last row sums, so the call keeps its stream semantics).  Same values bit for bit. */
int c8_set_stage_overlap(c8_ctx* ctx, int on);
/* C8_SCATTER_GATHER in two parts, for a caller that exchanges ghost rows (LinearAlg::gather_A / gather_b,
 * linear_alg.cpp:53-86): with an early node range set, a Jacobian assembly stages every element and sums the rows of
 * the nodes [node_begin, node_end) only -- the ghost rows, which the caller can then pack and send -- and
 * c8_gather_finish sums the rows of all other nodes while the exchange is in flight.  Every assembly must then be
 * followed by c8_gather_finish before the system is used.  Needs the whole mesh in one staged chunk; an empty range
 * (the default) turns the split off. */
int c8_set_gather_early_nodes(c8_ctx* ctx, int node_begin, int node_end);
int c8_gather_finish(c8_ctx* ctx);
/* C8_SCATTER_GATHER, assign mode (default off = the reference's accumulate-into semantics): the two Jacobian assemblies
 * ASSIGN the rows of A (all four blocks) and b of every node that has elements instead of adding to them, i.e.
 * la->zero_all() followed by eval_forward_jacobian / eval_adjoint_jacobian (primal.cpp:98-99, adjoint.cpp:123-125) in one
 * call: the caller's zeroing pass and the row sums' read of the old values (3.5 of 15.9 GB on a million hex8 elements)
 * both go away.  Rows of nodes without elements are not touched.  The other entry points (residual-only assembly,
 * boundary conditions, ...) keep adding; a Jacobian assembly in another scatter mode is refused while the mode is on. */
int c8_set_assign_mode(c8_ctx* ctx, int on);
/* Shape-table cache (default on; hex8 wave kernels): the geometry of a context is static, so dN/dx, w dv and the element
 * size are computed once at c8_create (1.7 KB per element) instead of by every call (weight.cpp:5-25 recomputes them for
 * every AD pass).  on = 0 frees the tables; results are the same either way. */
int c8_set_shape_cache(c8_ctx* ctx, int on);
/* Forward-assembly kernel: C8_KERNEL_SLOT = one lane group per element (any element type);
 * C8_KERNEL_WAVE = one wavefront per element (hex8); C8_KERNEL_AUTO picks WAVE where available.  Where a model has a
 * closed form of its local equations (small_J2 on 3-D meshes: radial return and consistent tangent), the forward WAVE
 * kernel -- and, under C8_KERNEL_AUTO, the lane-group kernel of an element type without a wave kernel (tet4) -- uses it
 * in place of the local Newton iteration and the automatic-differentiation passes: the same converged state and
 * Jacobian as the iterated form to within the local Newton tolerance (2e-13 measured).  C8_KERNEL_WAVE_AD (hex8) and an
 * explicit C8_KERNEL_SLOT keep the iterated, automatically differentiated form; it also runs whenever
 * local_max_iters < 8, so that a local solve that cannot converge within the caller's budget still reports
 * C8_LOCAL_SOLVE_FAILED as the reference does.
 * C8_KERNEL_NODE (hex8, models with a closed form, C8_SCATTER_GATHER): eval_forward_jacobian with one wavefront per NODE --
 * the wavefront forms the node's four CSR rows from the node's elements (closed form recomputed per node, every 4 x 4
 * block of an element matrix formed once, by its row node) and writes them once: no element stage, no atomics, bitwise
 * reproducible, a third of the staged form's memory traffic.  C8_KERNEL_AUTO takes it where it applies (cached shape
 * tables present, st->xi and st->xi_prev distinct arrays); C8_KERNEL_WAVE keeps the staged one-wavefront-per-element form.
 * It honours c8_set_assign_mode and c8_set_gather_early_nodes / c8_gather_finish like the staged form; between the
 * assembly call and c8_gather_finish the arrays of `st` must stay as they were (the second part reads them).
 * Under C8_KERNEL_AUTO / C8_KERNEL_NODE c8_assemble_adjoint_jacobian takes the same form and c8_solve_adjoint_local the
 * model's closed form of the local adjoint solve (no dual numbers, no elimination of dC/dxi; same results to rounding);
 * c8_param_gradient likewise takes the closed form of the point's share of the gradient. */
int c8_set_kernel_variant(c8_ctx* ctx, int variant);
/* async = 1: assembly calls only enqueue and return C8_OK; c8_status() then synchronises the
 * stream and reports C8_OK / C8_LOCAL_SOLVE_FAILED for everything enqueued since the last call. */
int c8_set_async(c8_ctx* ctx, int async);
int c8_status(c8_ctx* ctx);

/* ---- the objective (QoI) of the adjoint path ---------------------------------------------------------
 * Default: "average displacement" (avg_disp.cpp).  "calibration" (calibration.cpp, 3-D form):
 *   J_step = dt/T [ 1/(2 area) int_side sum_d w_d (u_d - u_meas_d)^2 dS * (coupled points per element)
 *                   + 1/2 balance (load - load_meas)^2 ],
 * load = internal force component `reaction_comp` summed over the nodes with |x[coord_idx] - coord_value| <
 * coord_tol.  The factor "coupled points per element" is the reference's: it adds the face integral at every
 * coupled integration point of the element (1 for tet4, 8 for this library's hex8 extension).  On a tri3 mesh the
 * displacement term is the reference's 2-D branch (calibration.cpp:76-104, :163-222): the integral runs over the
 * ELEMENTS -- all of them (num_faces = 0), or the listed ones (a distance field with a threshold in the reference) --
 * and `area` is the sum of their areas. */
typedef struct {
  int32_t num_faces, nodes_per_face;  /* displacement side set: faces as node ids, 3 per face (tet4) or 4 (hex8); on a
                                         tri3 mesh a list of ELEMENT ids (nodes_per_face = 1), or 0 for every element */
  const int32_t* faces;               /* HOST array [num_faces][nodes_per_face] */
  double weights[3];                  /* "displacement weights" */
  double balance_factor;
  int32_t coord_idx;                  /* "coordinate index" / "coordinate value" / "coordinate tolerance" */
  double coord_value, coord_tol;
  int32_t reaction_comp;              /* "reaction force component" */
  double dt_over_total_time;          /* m_dt / m_total_time */
} c8_calibration_desc;
/* Multi-part meshes: the calibration objective sums the side-set area and the reaction load over all parts
 * (PCU_Add_Double, calibration.cpp:138, :351) and shares the load term of J between the parts (:375-378).  The
 * caller supplies the SUM all-reduce over its communicator (HOST doubles, in place) and the number of parts; the
 * library calls it from c8_qoi_preprocess and from the entry points that run preprocess_qoi. */
typedef void (*c8_allreduce_fn)(void* user, double* values, int n);
int c8_set_allreduce(c8_ctx* ctx, c8_allreduce_fn fn, void* user, int num_parts);
int c8_set_qoi_avg_disp(c8_ctx* ctx);
int c8_set_qoi_calibration(c8_ctx* ctx, const c8_calibration_desc* desc);
/* measured data of the current step: nodal displacements (DEVICE array [nodes][3], kept by reference) and load */
int c8_set_measured(c8_ctx* ctx, const double* u_meas, double load_meas);
/* preprocess_qoi (evaluations.cpp:262-347); the adjoint entry points below run it themselves, this call only
 * reports: out (HOST, 3 doubles, may be NULL) = {side-set area, total load, load mismatch}. */
int c8_qoi_preprocess(c8_ctx* ctx, const c8_state* st, double* out);
/* Subdomain objectives (avg_stress.cpp, avg_local_var.cpp, disp_comp.cpp): the value of a load step is the sum over the
 * elements of ONE element set and their local-state points of w dv q,
 *   C8_QOI_AVG_STRESS      q = |dev_cauchy|, the Frobenius norm of the model's deviatoric Cauchy stress over its
 *                              ndims x ndims block
 *   C8_QOI_AVG_LOCAL_VAR   q = xi[index], `index` the flat position in the point's local state
 *   C8_QOI_DISP_COMP       q = u[index] interpolated at the point
 * Plain integrals: not divided by the volume, as in the reference.  The caller sums the steps; on a part of a multi-part
 * mesh the sum covers the part's own elements and the caller sums the parts, as for "average displacement".
 * Deliberate difference: |D| is not differentiable at D = 0, where the reference's derivative is NaN; here a point with
 * |dev_cauchy| == 0 contributes value 0 and derivative 0.
 * The adjoint kernels run with a zero objective; kernels of their own (c8_qoi_point.hip) add the value, subtract dJ/dxi
 * from g before the adjoint Jacobian is assembled, subtract dJ/dx from b after it and add dJ/dp to the gradient, all in a
 * fixed summation order (bitwise repeatable), on the context's stream.
 * Returns C8_ERR_ARG for an element set, local dof or component out of range (C8_QOI_DISP_COMP: index >= c8_num_dims),
 * C8_ERR_UNSUPPORTED for C8_QOI_AVG_LOCAL_VAR on a model without local state. */
enum { C8_QOI_AVG_STRESS = 0, C8_QOI_AVG_LOCAL_VAR = 1, C8_QOI_DISP_COMP = 2 };
typedef struct { int32_t kind, elem_set, index; } c8_subdomain_qoi_desc;   /* index: local dof k / component c / 0 */
int c8_set_qoi_subdomain(c8_ctx* ctx, const c8_subdomain_qoi_desc* desc);
/* Reaction (reaction.cpp without "compute torque"): the internal force component `reaction_comp` summed over the nodes
 * with |x[coord_idx] - coord_value| < coord_tol -- out[1] of c8_qoi_preprocess.  The load term of "calibration" with no
 * measured data and no face term: the adjoint kernels carry it themselves.  Multi-part meshes: the load is summed over
 * the parts (c8_set_allreduce) and every part reports 1 / num_parts of it, so that the caller's sum counts it once. */
typedef struct { int32_t coord_idx; double coord_value, coord_tol; int32_t reaction_comp; } c8_reaction_desc;
int c8_set_qoi_reaction(c8_ctx* ctx, const c8_reaction_desc* desc);

/* ---- the hot path (all array arguments are DEVICE pointers) --------------------------------- */
/* eval_forward_jacobian (evaluations.cpp:12-154): R and dR/dx with the local state condensed;
 * writes the converged local state to st->xi. */
int c8_assemble_forward_jacobian(c8_ctx* ctx, const c8_state* st, const c8_system* sys);
/* The same over a subset of the elements (`elems`: DEVICE array of `count` distinct element ids), with atomic
 * adds.  For overlapping the halo exchange with the assembly: assemble the elements that touch
 * ghost nodes, start the exchange, assemble the rest.  The context must be in C8_SCATTER_ATOMIC mode. */
int c8_assemble_forward_jacobian_subset(c8_ctx* ctx, const c8_state* st, const c8_system* sys, const int32_t* elems, int count);
/* eval_global_residual (evaluations.cpp:156-259): R only, from the stored local state. */
int c8_assemble_residual(c8_ctx* ctx, const c8_state* st, const c8_system* sys);
/* eval_adjoint_jacobian (evaluations.cpp:349-526) for the context's objective:
 * A += (dR/dx total)^T, b += -dJ/dx + f + (dxi/dx)^T g, and g -= dJ/dxi in place.
 * g [elems][points][local dofs], f [elems][points][element dofs]. */
int c8_assemble_adjoint_jacobian(c8_ctx* ctx, const c8_state* st, double* g, const double* f, const c8_system* sys);
/* solve_adjoint_local (evaluations.cpp:528-659): phi from the global adjoint z, then the
 * history vectors f, g for the previous step (overwritten). */
int c8_solve_adjoint_local(c8_ctx* ctx, const c8_state* st, const double* const z[2], double* phi, double* g, double* f);
/* eval_qoi_gradient (evaluations.cpp:758-925): grad[c8_num_active_params] +=
 * sum_e sum_pt (dC/dp)^T phi + dJ/dp + (dR/dp)^T z. */
int c8_param_gradient(c8_ctx* ctx, const c8_state* st, const double* const z[2], const double* phi, double* grad);
/* eval_qoi (evaluations.cpp:662-756), "average displacement" (avg_disp.cpp:16-33): *J += value. */
int c8_eval_qoi(c8_ctx* ctx, const c8_state* st, double* J);
/* eval_cauchy (evaluations.cpp:1659-1748): sigma [num_elems][c8_num_local_points][3][3], DEVICE, OVERWRITTEN.
 * Row-major; entries with a row or column index >= c8_num_dims() are 0, as in the reference's apf::Matrix3x3.
 * The local model's cauchy() at every local-state point (ip set 0), from the stored state st->xi of that point and
 * st->x interpolated there: no local solve, nothing is written but sigma.  Parameters are those of the element's
 * element set.  The finite-deformation models also gather st->x_prev[0]; under mechanics_plane_stress x[1] and
 * x_prev[1] are not read.  The reference returns a zero field for step 0; this call always evaluates (the caller
 * knows its step: calibr8_amd.PrimalDriver.cauchy).  Stream, async mode and return value as c8_assemble_residual
 * (nothing here can fail a local solve).  Not collective: on a part of a multi-part mesh the ghost and phantom
 * entries of x must have been imported (c8_halo_scatter_x), as for every other entry point; sigma covers the part's
 * own elements.  hybrid_hyper_J2_plane_stress needs its embedded network set, as the assembly entry points do. */
int c8_eval_cauchy(c8_ctx* ctx, const c8_state* st, double* sigma);
/* eval_error_contributions (evaluations.cpp:930-1073): the adjoint-weighted residuals that localise the error estimate
 * of the objective, two numbers per element, both ACCUMULATED INTO (the caller sums its steps into one pair of fields):
 *   E_R[e] += z_e . R_e(x)          R the context's global residual, the integrand c8_assemble_residual scatters: per
 *                                   point of ip set 0  w dv (Gu : grad z_u + Vp z_p + Gp . grad z_p)  with z interpolated by
 *                                   the element's shape functions, plus  w dv flux_pressure z_p  on ip set 1 (`mechanics`);
 *   E_C[e] += sum_pt phi_pt . C     C the local model's residual at (st->x interpolated, st->xi, st->xi_prev), on the
 *                                   branch the model itself chooses (the reference's force_path is not supported);
 *                                   `elastic` contributes nothing.
 * Evaluated at the STORED state: no local solve, no AD, nothing is written but E_R and E_C [num_elems].  z as in
 * c8_solve_adjoint_local (z[1] is not read when c8_num_residuals() == 1), phi [elems][c8_num_local_points]
 * [c8_num_local_dofs]; DEVICE pointers.  The reference also scatters R into b (:1030); callers get that from
 * c8_assemble_residual.  No floating-point atomics: every element's two sums are formed in a fixed order (ip set 0
 * ascending, then ip set 1), the same inputs give the same bytes.  Stream, async mode and return value as
 * c8_assemble_residual (nothing here can fail a local solve).  Not collective: on a part of a multi-part mesh the ghost
 * and phantom entries of x and z must have been imported; the outputs cover the part's own elements, each of which
 * belongs to exactly one part.  hybrid_hyper_J2_plane_stress needs its embedded network set.
 * Model-form error (calibr8_amd.model_form_error): z and phi come from c8_adjoint_solve_step on a context of the richer
 * model, linearised about the state of the cheaper one.  Under C8_KERNEL_AUTO the row-per-node adjoint kernels (small_J2 on
 * hex8) recompute the local state from xi_prev and never read st->xi -- for such a prolonged state the wrong linearisation
 * point -- so a context used that way must be put on C8_KERNEL_WAVE_AD (c8_set_kernel_variant) first. */
int c8_eval_error_contributions(c8_ctx* ctx, const c8_state* st, const double* const z[2], const double* phi, double* E_R,
                                double* E_C);
/* eval_exact_errors (evaluations.cpp:1462-1654): the derivative of the same two sums along the direction from the stored
 * state st to a second state st_fine (same mesh, same local layout), both outputs [num_elems], ACCUMULATED INTO:
 *   E_R[e] += -z_e . (dR/dx dx + dR/dxi dxi)                                      dx = st_fine->x - st->x, ...
 *   E_C[e] += -sum_pt phi_pt . (dC/dx dx + dC/dxi dxi + dC/dx_prev dx_prev + dC/dxi_prev dxi_prev)
 * The six Jacobians the reference builds by AD are never formed: the differences are taken in the kernel (fine minus
 * stored) and seeded as the one tangent of a single evaluation of the model at st -- nodal u and p carry dx, u_prev of the
 * finite-deformation models dx_prev, xi and xi_prev their differences.  R is differentiated along x and xi only, as in the
 * reference (:1608): no model's global flux reads x_prev or xi_prev, so the one pass gives exactly that, and a direction
 * that moves only x_prev and xi_prev leaves E_R unchanged.  The branch is the one the model chooses from the values at st
 * (the reference's force_path is not supported).  On ip set 1 the pressure flux enters with its tangent along dx.
 * Nothing of st_fine is written; its xi is only read.  With st_fine == st both outputs are unchanged.
 * Null rules (st_fine's entries as st's), one-residual rules (entries [1] of x, x_prev and z ignored), the embedded
 * network of hybrid_hyper_J2_plane_stress, the fixed order of the sums (no atomics, the same inputs give the same bytes),
 * stream, async mode, return value and "not collective" are those of c8_eval_error_contributions. */
int c8_eval_exact_errors(c8_ctx* ctx, const c8_state* st, const c8_state* st_fine, const double* const z[2], const double* phi,
                         double* E_R, double* E_C);
/* eval_linearization_errors (evaluations.cpp:1075-1266), per element (the reference returns two scalars; the caller adds
 * the fields up, in an order of its choice): the residuals linearised about st, evaluated at st_fine,
 *   E_lin_R[e] += -z_e . (R + dR/dx dx + dR/dxi dxi)
 *   E_lin_C[e] += -sum_pt phi_pt . (C + dC/dx dx + dC/dxi dxi + dC/dx_prev dx_prev + dC/dxi_prev dxi_prev)
 * i.e. what c8_eval_exact_errors adds minus what c8_eval_error_contributions adds, term by term; the values R and C are
 * those of c8_eval_error_contributions, so with st_fine == st the fields are its negated outputs.  Where R and C are
 * linear in the state (`elastic`, `isotropic_elastic`) these are the negated error contributions AT st_fine.  For a
 * linear objective and z, phi from the adjoint march about the history of st, the sum over steps and elements of
 * E_R + E_C of c8_eval_exact_errors is J(fine) - J(stored) (calibr8_amd.model_form_error_verify).
 * Everything else as c8_eval_exact_errors. */
int c8_eval_linearization_errors(c8_ctx* ctx, const c8_state* st, const c8_state* st_fine, const double* const z[2],
                                 const double* phi, double* E_lin_R, double* E_lin_C);

/* ---- virtual fields method (VFM): the local constitutive update driven by MEASURED displacements, the internal-force
 * residual contracted with a fixed nodal virtual field w; no global linear solve (virtual_power.cpp).  One-residual
 * systems only ('mechanics_plane_stress' on tri3, virtual_power.cpp:110,148); under 'mechanics' every entry returns
 * C8_ERR_UNSUPPORTED.  st holds the measured x (step n) and x_prev (step n-1) and the local states xi_prev, xi.
 * Values are per part: the caller sums them over the parts, as with c8_eval_qoi and c8_param_gradient.  The sums are
 * formed in a fixed order (no floating-point atomics): the same inputs give the same bits.  DEVICE pointers. */
/* w [num_nodes][2], kept by pointer until the next call. */
int c8_vfm_set_virtual_field(c8_ctx* ctx, const double* w);
/* eval_measured_residual (evaluations.cpp:1750-1845) + VirtualPower::compute_at_step (virtual_power.cpp:135-139):
 * the local solve from xi_prev, the converged state written to st->xi, *ivw += w^T R.  b (may be NULL) += R. */
int c8_vfm_internal_power(c8_ctx* ctx, const c8_state* st, double* b, double* ivw);
/* eval_measured_residual_and_grad (evaluations.cpp:1847-1973) + VirtualPower::compute_at_step_forward_sens
 * (virtual_power.cpp:141-186): as c8_vfm_internal_power, and the local sensitivities
 * S = -(dC/dxi)^-1 (dC/dp + dC/dxi_prev S_prev), divw[c8_num_active_params] += [(dR/dxi)^T w]^T S + (dR/dp)^T w.
 * S, S_prev: [elems][points][local dofs][c8_num_active_params] (column = position of the parameter in grad);
 * S_prev NULL = 0 (first step).  An element writes, and reads of S_prev, only the columns of its own element set's
 * parameters: the other columns of its rows keep what S held before the call.  Without active parameters S may be NULL. */
int c8_vfm_forward_sens(c8_ctx* ctx, const c8_state* st, const double* S_prev, double* S, double* ivw, double* divw);
/* eval_vfm_adjoint_gradient (evaluations.cpp:1975-2143) at the stored state of step n, c = the step's scaled mismatch:
 * phi = (dC/dxi)^-T (-c (dR/dxi)^T w - h), h <- (dC/dxi_prev)^T phi (in place, [elems][points][local dofs], zero
 * before the last step), grad[c8_num_active_params] += c (dR/dp)^T w + (dC/dp)^T phi. */
int c8_vfm_adjoint_step(c8_ctx* ctx, const c8_state* st, double c, double* h, double* grad);

/* ---- next to the hot path: boundary conditions and the Newton step driver ----- */
/* One Dirichlet condition = one entry of the deck's `dirichlet bcs` block (dbcs.cpp:59-66): residual
 * index, equation, node set, and the prescribed value at every node of the set (the caller evaluates
 * the expression or reads the measured field, dbcs.cpp:76 / :183-185).  DEVICE pointers. */
typedef struct {
  int32_t resid, eq, n;
  const int32_t* nodes;   /* [n] local node ids */
  const double* values;   /* [n] */
} c8_dbc;
/* One traction condition (tbcs.cpp:17-86) on the sides of the mesh: tri3 faces of tet4 meshes and the edges of tri3
 * meshes with the reference's 1-point rule, quad4 faces of hex8 meshes with the 2x2 rule.  DEVICE pointers. */
typedef struct {
  int32_t resid, n, nodes_per_face;  /* 2 (edges of a 2-D mesh), 3 or 4 */
  const int32_t* faces;    /* [n][nodes_per_face] local node ids */
  const double* traction;  /* [n][points][3], points = 1 (edge, tri3) or 4 (quad4); on a 2-D mesh the third entry is ignored */
} c8_tbc;
/* apply_primal_dbcs (dbcs.cpp:28-121): for every constrained row keep the diagonal entry, zero the rest
 * of the row in every block, b[row] = diag * (x[row] - value), or 0 when is_adjoint.  Conditions apply in list order
 * (the later one wins on a shared row).  Both calls check every condition before they apply the first: after
 * C8_ERR_ARG the system is as it was. */
int c8_apply_dirichlet(c8_ctx* ctx, int n, const c8_dbc* dbcs, const double* const x[2], const c8_system* sys, int is_adjoint);
/* apply_primal_tbcs (tbcs.cpp:88-98): b[row(node, d)] -= T_d N_node w dv over the faces. */
int c8_apply_traction(c8_ctx* ctx, int n, const c8_tbc* tbcs, const c8_system* sys);
/* Integration points of boundary sides (HOST arrays; coords [.][3]): xyz [n][points][3], for evaluating traction expressions. */
int c8_face_points(int nodes_per_face, int n, const double* coords, const int32_t* faces, double* xyz);
/* LinearAlg::apply_A (linear_alg.cpp:158-175): y = A x over the four blocks (DEVICE pointers). */
int c8_apply_A(c8_ctx* ctx, const c8_system* sys, const double* const x[2], double* const y[2]);

/* The linear solve is out of scope (Belos/Teko/MueLu in the reference, linear_solve.cpp): the driver
 * calls back with the assembled system (b already scaled to -R, primal.cpp:131) and device arrays to
 * receive dx.  Return 0 on success. */
typedef int (*c8_linear_solve_fn)(void* user, const c8_system* sys, double* const dx[2]);
typedef struct {
  int32_t max_iters;            /* "nonlinear max iters" of the global residual */
  double abs_tol, rel_tol;      /* "nonlinear absolute/relative tol" */
  int32_t line_search;          /* 1 = Armijo/cubic backtracking (line_search.hpp), 0 = full steps */
  double sufficient_decrease;   /* 1e-4 */
  double min_backtrack, max_backtrack; /* 0.5, 0.9 */
  int32_t max_evals;            /* 4 */
} c8_newton_opts;
/* Primal::solve_at_step (primal.cpp:31-209): Newton iterations on st->x (updated in place, st->xi receives the
 * converged local state) with the reference's convergence tests and line search.  With a halo attached to the context
 * (c8_halo_attach) the step runs over all parts: every rank calls it collectively, the assembly is followed by the
 * status all-reduce (primal.cpp:100,164), gather_A / gather_b (:110-111), boundary conditions and norms on the OWNED
 * rows, and the solution increment is imported to the ghost copies (disc.cpp:944-947); the callback then solves the
 * distributed owned system and must fill dx on the owned nodes.  Returns C8_OK, C8_LOCAL_SOLVE_FAILED (base point
 * or every line-search trial failed, on any part), or C8_NOT_CONVERGED; *iters = Newton iterations taken. */
enum { C8_NOT_CONVERGED = -5 };
int c8_primal_solve_step(c8_ctx* ctx, const c8_state* st, const c8_system* sys, int ndbc, const c8_dbc* dbcs, int ntbc,
                         const c8_tbc* tbcs, const c8_newton_opts* opts, c8_linear_solve_fn solve, void* user,
                         int32_t* iters);

/* Adjoint::solve_at_step (adjoint.cpp:76-189) followed by eval_qoi_gradient (adjoint_objective.cpp:86-94)
 * for one load step of one part: zero + c8_assemble_adjoint_jacobian, adjoint Dirichlet rows, the
 * caller's linear solve (system passed as assembled: A = (dR/dx)^T, b = right-hand side, NOT negated;
 * the solution is written to z), c8_solve_adjoint_local, and grad += this step's contribution.
 * March the steps from the last to the first with the same g, f arrays (zero before the last step). */
int c8_adjoint_solve_step(c8_ctx* ctx, const c8_state* st, const c8_system* sys, int ndbc, const c8_dbc* dbcs,
                          c8_linear_solve_fn solve, void* user, double* const z[2], double* phi, double* g, double* f,
                          double* grad);

/* ---- device-resident linear solve for the step drivers -----------------------------------------------------
 * Right-preconditioned BiCGStab on the system as the drivers hold it (the four CSR value arrays over the context's
 * graphs, or A[0][0] / b[0] alone when c8_num_residuals() == 1), preconditioned with the inverse of every node's own
 * diagonal block over its equations (u and p of the node: 4 x 4, 3 x 3 on tri3 meshes, 2 x 2 under
 * mechanics_plane_stress).  Everything stays in HBM on the context's stream; the host reads the residual norm every
 * `check_every` iterations.  No floating-point atomics: the same inputs give the same bits.  This stands in for the
 * reference's Belos / Teko / MueLu stack on one part.  With block Jacobi the iteration counts grow like 1 / h.
 * c8_krylov_set_preconditioner below selects multicolour node-block symmetric Gauss-Seidel instead: several times fewer
 * iterations at about three times the matrix traffic per iteration, the same growth with 1 / h, the same
 * reproducibility; or C8_PRECOND_TWO_LEVEL, which adds a coarse space of rigid-body modes per aggregate of nodes:
 * two levels, dense coarse solve, capped at 8192 coarse unknowns (meshes up to roughly 10^5 nodes).  It is no
 * multilevel method; C8_PRECOND_MULTILEVEL is: it repeats the aggregation on the coarse matrix until that is small and
 * inverts only the last level densely, which lifts the cap. */
typedef struct {
  int32_t max_iters;      /* iterations (two A x each); default 20000 when <= 0 */
  int32_t check_every;    /* host reads the residual norm every this many iterations; default 10 */
  int32_t max_restarts;   /* restarts of the recurrence from the current iterate, after a breakdown or after a recursive
                             residual that met the tolerance while the true residual did not (one budget); default 5 */
  double rel_tol;         /* ||b - A x|| <= rel_tol ||b||; default 1e-10 */
  double abs_tol;         /* or <= abs_tol; default 0 */
} c8_krylov_opts;
typedef struct {
  int32_t iters, restarts, status;  /* status = the return value of the solve */
  double b_norm, residual_norm;     /* residual_norm = ||b - A x||, recomputed from x on exit */
} c8_krylov_info;
/* dx (DEVICE pointers, as b) is overwritten; the start vector is 0.  opts NULL (or a field <= 0) = the defaults; info
 * may be NULL.  Returns C8_OK; C8_NOT_CONVERGED with dx holding the last iterate and info filled; C8_ERR_ARG for null
 * pointers, a right-hand side that is not finite, or a node whose diagonal block is singular or not finite (the
 * message of c8_last_error names the node; nothing is iterated); C8_ERR_UNSUPPORTED when a halo is attached to the
 * context: a multi-part solve needs the halo exchange inside A x and inner products summed over the parts, which is
 * c8_krylov_solve_parts below.  b = 0 returns dx = 0 after 0 iterations. */
int c8_krylov_solve(c8_ctx* ctx, const c8_system* sys, double* const dx[2], const c8_krylov_opts* opts,
                    c8_krylov_info* info);
/* The same as a c8_linear_solve_fn for c8_primal_solve_step / c8_adjoint_solve_step: `user` points to a
 * c8_krylov_user; `info` receives the last solve, `total_iters` and `solves` add up over the calls. */
typedef struct {
  c8_ctx* ctx;
  c8_krylov_opts opts;
  c8_krylov_info info;
  int64_t total_iters, solves;
} c8_krylov_user;
int c8_krylov_linear_solve(void* user, const c8_system* sys, double* const dx[2]);
/* The same solve over the parts of a multi-part mesh (a halo attached to the context, c8_halo_attach).  COLLECTIVE: every
 * rank of the halo's communicator calls it with its local system as the step drivers hold it after c8_halo_gather: the
 * first num_owned node rows are the owned system, columns address owned, ghost and phantom local ids, ghost rows are
 * scratch.  A x runs over the owned rows with the import (C3) of the multiplied vector inside it: the rows without a ghost
 * or phantom column are multiplied while the messages travel, the others afterwards.  Inner products are local partials in
 * a fixed order, then one all-reduce of the 1-2 sums through the communicator (device buffers under RCCL: ncclAllReduce on
 * the communicator's stream, ordered by events, no host wait; copy down / callback / copy up under the host transport): three
 * all-reduces and two imports per iteration.  Every scalar and the stop flag derive from all-reduced values only, and at
 * every host read the ranks all-reduce (iterations, stop flag, failure marker): ranks that disagree, or a rank with a
 * device error, make EVERY rank return C8_ERR_DEVICE instead of entering another batch.  dx is written on the owned nodes
 * (ghost and phantom entries unspecified: the drivers import them afterwards); info->b_norm and info->residual_norm are
 * norms of the global owned system; iters, restarts and status are the same on all ranks, and so is the return value of
 * the refusals of a non-finite right-hand side and of a singular diagonal block (the message names the node by local id
 * and rank).  For one partition the result is a pure function of the inputs and of the transport's all-reduce (no
 * floating-point atomics).  Without a halo the call is c8_krylov_solve. */
int c8_krylov_solve_parts(c8_ctx* ctx, const c8_system* sys, double* const dx[2], const c8_krylov_opts* opts,
                          c8_krylov_info* info);
/* ... as a c8_linear_solve_fn (`user` points to a c8_krylov_user), for the step drivers over parts. */
int c8_krylov_linear_solve_parts(void* user, const c8_system* sys, double* const dx[2]);
/* Diagnostic / test access: the two node lists of the multi-part A x (HOST array owned by the context, built from the
 * graph at the first use; needs a halo): nodes[0 .. num_interior) are the owned nodes whose graph row has only owned
 * columns, nodes[num_interior .. num_interior + num_boundary) the other owned nodes. */
int c8_krylov_part_lists(c8_ctx* ctx, int32_t* num_interior, int32_t* num_boundary, const int32_t** nodes);
/* The preconditioner M^-1 of c8_krylov_solve and c8_krylov_solve_parts: context state, block Jacobi after c8_create.
 * C8_PRECOND_BLOCK_SGS is `sweeps` symmetric multicolour Gauss-Seidel sweeps over the node blocks (sweeps <= 0: one).
 *   colours   greedy over the node graph (block (1,1) of c8_graph), on the host: nodes in ascending id, each takes the
 *             smallest colour no already-coloured neighbour has
 *   y = M^-1 v   x = 0; one symmetric sweep visits the colours 0, 1, ..., nc - 1, then nc - 2, ..., 0; for every node i of
 *             the current colour  x_i <- x_i + D_i^-1 (v_i - sum_j A_ij x_j),  j over the node's whole graph row, A_ij the
 *             block of the node pair over all equations of a node, D_i^-1 the inverse the Jacobi preconditioner uses; y = x
 *   parts     with a halo attached only the owned nodes are coloured (over the owned sub-graph) and columns with local id
 *             >= num_owned are skipped: a part-local (hybrid) Gauss-Seidel, no message inside the preconditioner
 * Nodes of one colour do not couple: the apply has no floating-point atomics and is a pure function of its inputs.
 * An unknown kind, or a call while a staged assembly waits for c8_gather_finish, returns C8_ERR_ARG.
 *
 * C8_PRECOND_TWO_LEVEL is a coarse correction followed by `sweeps` of those symmetric sweeps (sweeps <= 0: one).  One part
 * only: with a halo attached c8_krylov_solve_parts, c8_krylov_precondition, c8_krylov_aggregates and
 * c8_krylov_coarse_matrix return C8_ERR_UNSUPPORTED while this kind is selected (one rank included).
 *   aggregates   on the host, over the node graph.  Pass 1, nodes in ascending id: a node whose whole graph row (itself
 *             included) is still unaggregated opens a new aggregate holding that row.  Pass 2, ascending id: a node still
 *             free joins the pass-1 aggregate of its lowest-id neighbour that pass 1 aggregated.  Pass 3, ascending id: a
 *             node still free becomes an aggregate of its own.  Aggregate ids are in order of creation.
 *   P         every aggregate carries the rigid-body modes about its centroid (the mean of its nodes' coordinates, summed in
 *             ascending id) and a constant pressure where there is a p equation.  3-D mechanics, 7 columns: 3 translations,
 *             3 rotations e_m x (x_i - centroid), constant p; tri3 mechanics, 4 columns: 2 translations, the rotation
 *             (-(y - ybar), x - xbar), constant p; mechanics_plane_stress, 3 columns.  Columns in this order,
 *             aggregate-major.  An equation row of A is CONSTRAINED when every off-diagonal entry of the row is exactly 0
 *             in all blocks (the rows c8_apply_dirichlet leaves; found on the device at every set-up): its row of P is zero.
 *   A_c       = P^T A P, formed on the device at every solve, dense, then inverted (LU with partial pivoting, rocSOLVER).  A
 *             column of P that is zero (every row of a mode constrained; the rotations of a one-node aggregate) gets a
 *             unit diagonal.  n_coarse = aggregates x columns must not exceed 8192 (a 512 MB inverse): above it the solve
 *             and the apply return C8_ERR_UNSUPPORTED, the message names n_coarse and the cap, nothing is iterated.  That
 *             makes this kind a method for meshes up to roughly 10^5 nodes; the recursive coarse solve of
 *             C8_PRECOND_MULTILEVEL below lifts the cap.  A_c singular or not finite: C8_ERR_ARG, the message names the
 *             aggregate.
 *   y = M^-1 v   x = P A_c^-1 P^T v, then the symmetric sweeps above started from this x instead of 0 (every colour launch
 *             reads the whole graph row); y = x.  A fixed linear operator: BiCGStab stays valid.
 * Reproducibility: every kernel of this library in the set-up and in the apply sums in a fixed order without
 * floating-point atomics, so A_c, and everything downstream of a given inverse, are pure functions of their inputs.  The
 * inverse itself comes from rocSOLVER (dgetrf, dgetri), which this library does not control; on the library versions it was
 * tested with, repeated solves in one process and in a fresh process gave the same bits (tests/test_gpu_krylov_two_level.py
 * asserts it). */
enum { C8_PRECOND_BLOCK_JACOBI = 0, C8_PRECOND_BLOCK_SGS = 1 };
enum { C8_PRECOND_TWO_LEVEL = 3 };  /* 2 stays unassigned: callers have been told since the Gauss-Seidel kind that
                                       2 is refused as an unknown kind, and it still is */
/* C8_PRECOND_MULTILEVEL repeats the two-level construction on the coarse matrix: a V-cycle of `sweeps` symmetric sweeps per
 * level (sweeps <= 0: one) over a dense solve on the last level.  One part only: with a halo attached every call that would
 * use it (c8_krylov_solve_parts, c8_krylov_precondition, c8_krylov_levels, c8_krylov_level, c8_krylov_level_matrix) returns
 * C8_ERR_UNSUPPORTED, one rank included; the message says "multilevel" and "halo".  NC = the columns per aggregate of the
 * two-level kind (7, 4 or 3).
 *   levels    Level 0 is the system: node blocks over the node graph.  Level l >= 1 has one node per aggregate of level
 *             l - 1, with NC unknowns (the rigid-body modes, then p) and a position: the aggregate's centroid (the unweighted
 *             mean of its members' positions, summed in ascending id).  Graph of level l + 1: I and J are neighbours when a
 *             node of I is a neighbour of a node of J in the graph of level l, self included.  Aggregates and colours of
 *             every level come from that level's graph by the two host rules above, unchanged.  Level 1 always exists;
 *             another level is built while n_l x NC > coarse_max, fewer than max_levels levels exist (level 0 counts) and
 *             aggregation still reduces the node count.
 *   P_l       P_0 is the P of the two-level kind.  l >= 1, node a of level l in aggregate I: d = x_a - centroid(I); the
 *             NC x NC block is the identity (translations, rotations, p pass to themselves) plus rotation m -> translation
 *             e_m x d (2-D: (-d_y, d_x)).  At every level a row of P_l is zero when its equation in A_l is constrained by
 *             the rule above (every off-diagonal entry of the row exactly 0): the Dirichlet rows on level 0, the
 *             unit-diagonal unknowns of zero columns on the coarser levels.
 *   A_l+1     = P_l^T A_l P_l, a zero column of P_l gets a unit diagonal; block-sparse over the level's graph except the
 *             last level, which is dense and inverted as A_c above.  The last level must not exceed the 8192 of the
 *             two-level kind: otherwise C8_ERR_UNSUPPORTED, the message names its size, the cap and what ended the recursion
 *             (max_levels, or aggregation that no longer reduces), nothing is iterated.
 *   M_l^-1 v  on the last level the dense inverse times v; otherwise x = P_l M_l+1^-1 P_l^T v, then `sweeps` symmetric
 *             multicolour block Gauss-Seidel sweeps on A_l started from x, with that level's colours and the inverses of its
 *             NC x NC (level 0: node) diagonal blocks, every colour launch over the whole row.  M^-1 = M_0^-1: a fixed
 *             linear operator.  With max_levels = 2, or when level 1 fits coarse_max, it is the two-level operator.
 * A singular or non-finite diagonal block: C8_ERR_ARG; on level 0 the message names the node, on a coarser level the level
 * and the aggregate.  Every sum of the set-up and of the apply has a fixed order (no floating-point atomics); the inverse of
 * the last level comes from rocSOLVER as above. */
enum { C8_PRECOND_MULTILEVEL = 5 };
/* C8_PRECOND_TWO_LEVEL_PARTS is the two-level kind with a coarse space over the parts of a multi-part mesh: two levels, a
 * dense coarse problem over ALL parts, replicated on every rank.  Without a halo it IS C8_PRECOND_TWO_LEVEL (the same
 * launches); c8_krylov_solve keeps refusing a halo.  With a halo attached (c8_krylov_solve_parts; NC = 7, 4 or 3 as above):
 *   aggregates   every rank runs the three passes above over its OWNED sub-graph: the first num_owned nodes, columns with
 *             local id >= num_owned skipped (as the part-local colouring does).  No aggregate crosses a part boundary.
 *             Global id = base_r + local id, base_r = the number of aggregates of the ranks below r; the counts travel in one
 *             all-reduce of a vector with one slot per rank (each slot written by one rank: the sum is exact).  Centroid: the
 *             unweighted mean of the member positions, summed in ascending local id.
 *   P         the P above (rigid-body modes about the centroid, constant p), with rows for OWNED nodes only.  A row is zero
 *             where its equation is constrained by the rule above, applied to the whole owned row after c8_halo_gather,
 *             off-part columns included.  Never stored.
 *   imported  the owner's P_j is needed at the ghost and phantom copies of node j: global aggregate id, offset from the
 *             centroid, constrained flags.  They travel through the halo's owner -> copy (import) tables, the ones A x uses:
 *             ids and offsets once per attached halo, flags at every set-up.  Copies are exact.
 *   A_c       = P^T A P over all parts, dense, n_c = NC x (sum of the ranks' aggregates).  Rank r forms the block rows of its
 *             own aggregates: every column j of an owned row contributes, ghost and phantom columns with the imported P_j;
 *             the rows of other ranks are zero.  One all-reduce of the n_c^2 doubles gives every rank the same matrix: every
 *             entry is one value plus zeros, so the result does not depend on the transport's order of summation, for any
 *             number of parts.  A zero column of P gets a unit diagonal.  Every rank inverts its copy as above.  n_c must not
 *             exceed 8192: above it every rank returns C8_ERR_UNSUPPORTED, the message names n_c and the cap, before anything
 *             is assembled or iterated.
 *   y = M^-1 v   r_c = P^T v: rank r fills the slots of its own aggregates, zeros elsewhere; one all-reduce of the n_c
 *             doubles (exact for the same reason); e = A_c^-1 r_c for the rows of the rank's own aggregates; x = P e on the
 *             owned nodes; then `sweeps` part-local symmetric sweeps (C8_PRECOND_BLOCK_SGS over parts) started from this x,
 *             every colour launch over the owned columns.  A fixed linear operator.  An iteration of the solve makes two
 *             imports and five all-reduces.
 * A singular or non-finite A_c, a bad diagonal block, a device error on one rank and an aggregate with too many neighbouring
 * aggregates for the kernel's tile are agreed over the ranks (one slot per rank in an all-reduced vector): every rank returns
 * the same code.  With this kind selected and a halo attached, c8_krylov_aggregates returns the rank's LOCAL ids
 * (aggregate_of_node[i], i < num_owned) and c8_krylov_aggregate_base the base; c8_krylov_coarse_matrix is COLLECTIVE and
 * downloads the global A_c on every rank; c8_krylov_precondition is COLLECTIVE and applies the operator to the owned
 * entries.  The first of these calls (or the first solve) after a halo is attached is collective too: it counts the
 * aggregates over the ranks.  With the other coarse kinds selected all of them keep refusing a halo. */
enum { C8_PRECOND_TWO_LEVEL_PARTS = 7 };  /* 6 stays unassigned, as 2 and 4 */
/* C8_PRECOND_MULTILEVEL_PARTS is the multilevel kind over the parts of a multi-part mesh: the distributed level 0 of
 * C8_PRECOND_TWO_LEVEL_PARTS over the block-sparse levels of C8_PRECOND_MULTILEVEL, which are replicated on every rank from
 * level 1 down.  It lifts the cap of 8192 coarse unknowns of the two-level kind over parts.  Without a halo it IS
 * C8_PRECOND_MULTILEVEL (the same launches); c8_krylov_solve keeps refusing a halo.  With a halo attached
 * (c8_krylov_solve_parts, c8_krylov_linear_solve_parts, c8_krylov_precondition; NC = 7, 4 or 3 as above):
 *   level 0   that of C8_PRECOND_TWO_LEVEL_PARTS, unchanged: aggregates of the rank's owned sub-graph, global id = base_r +
 *             local id, centroids summed in ascending local id, P_0 zero on constrained equations by the rule over the whole
 *             owned row, ids, offsets and flags imported at the ghost and phantom copies.
 *   level 1 graph   global, replicated on every rank.  Aggregates I and J of any ranks are neighbours when an owned node of I
 *             has a graph column (owned, ghost or phantom) whose owner put it into J, self included; rows in ascending global
 *             id.  Every rank knows the rows of its own aggregates; host all-reduces over the halo's communicator, in which
 *             every entry is written by one rank and is zero elsewhere, carry the row lengths (one slot per global
 *             aggregate), then the column ids, then the centroids (total x ND); ids travel as doubles.  The result is exact
 *             and bitwise equal on every rank, for any number of parts.  Done once per attached halo, again when num_owned
 *             changes and when c8_krylov_set_multilevel changes a setting (that call serves both multilevel kinds).
 *   levels >= 2   from the replicated level 1 by the host rules of C8_PRECOND_MULTILEVEL (aggregates, colours, the
 *             continuation rule: level 1 always exists; another level is built while n_l x NC > coarse_max, fewer than
 *             max_levels levels exist, level 0 counting, and aggregation still reduces the node count).  The same host code on
 *             the same bits gives every rank the same hierarchy without a message.  P_l for l >= 1, the constrained rule on
 *             A_l, the unit diagonal of a zero column and the dense last level are those of C8_PRECOND_MULTILEVEL.  A last
 *             level above 8192 unknowns: C8_ERR_UNSUPPORTED on every rank before anything is assembled or iterated, the
 *             message names its size and what ended the recursion.
 *   A_1       = P_0^T A P_0 over all parts, block-sparse over the level-1 graph, one row-major NC x NC block per graph entry,
 *             replicated.  Rank r forms the block rows of its own aggregates, ghost and phantom columns with the imported
 *             P_j; one all-reduce of the nnz_1 x NC^2 doubles follows (every entry is one value plus zeros: exact in any
 *             order).  A_l, l >= 2, is then formed and set up on every rank.
 *   y = M^-1 v   r_1 = P_0^T v in the rank's own slots and zeros elsewhere, one all-reduce of the n_1 doubles; every rank
 *             runs the cycle of C8_PRECOND_MULTILEVEL on the whole level-1 vector (down the replicated levels, the dense
 *             solve, up with `sweeps` coloured sweeps per block level, level 1 included); x = P_0 e on the owned nodes; then
 *             `sweeps` part-local sweeps on level 0 started from this x.  A fixed linear operator; an iteration of the solve
 *             makes two imports and five all-reduces, as with C8_PRECOND_TWO_LEVEL_PARTS.  When level 1 is the last level
 *             (n_1 x NC <= coarse_max, or max_levels = 2) the launches are those of C8_PRECOND_TWO_LEVEL_PARTS and the results
 *             have its bytes.
 * A singular or non-finite diagonal block on any level, a singular last level, a device error on a rank and an aggregate with
 * too many neighbours for a kernel's tile are agreed over the ranks: every rank returns the same code; a bad node block of
 * level 0 names node and rank.  With this kind selected and a halo attached: c8_krylov_aggregates, c8_krylov_aggregate_base
 * and c8_krylov_coarse_matrix (cap included) behave as with C8_PRECOND_TWO_LEVEL_PARTS; c8_krylov_levels gives the level
 * count, level 0 included; c8_krylov_level(0) the rank's own view (num_owned nodes, local aggregate ids, the part-local
 * colour lists), c8_krylov_level(l >= 1) the replicated level; c8_krylov_level_matrix(l >= 1) is COLLECTIVE and downloads the
 * dense global A_l on every rank; c8_krylov_precondition is COLLECTIVE and applies the operator to the owned entries.  The
 * first of these calls after a halo is attached or a setting changed is collective too.  C8_PRECOND_TWO_LEVEL and
 * C8_PRECOND_MULTILEVEL keep refusing a halo. */
enum { C8_PRECOND_MULTILEVEL_PARTS = 9 };  /* 8 stays unassigned, as 2, 4 and 6 */
int c8_krylov_set_preconditioner(c8_ctx* ctx, int kind, int sweeps);
/* The two settings of C8_PRECOND_MULTILEVEL and C8_PRECOND_MULTILEVEL_PARTS (<= 0: the default): coarse_max, default 1024 unknowns, and max_levels, default
 * 8, at least 2.  The levels are rebuilt at the next use.  C8_ERR_ARG for a null context, for max_levels = 1, and while a
 * staged assembly waits for c8_gather_finish. */
int c8_krylov_set_multilevel(c8_ctx* ctx, int32_t coarse_max, int32_t max_levels);
int c8_krylov_get_preconditioner(const c8_ctx* ctx);  /* C8_PRECOND_* (C8_ERR_ARG for a null context) */
/* Diagnostic / test access: the colour lists of the Gauss-Seidel sweeps (HOST arrays owned by the context, built at the
 * first use, rebuilt when a halo has been attached since): nodes[color_ptr[c] .. color_ptr[c + 1]) are the nodes of
 * colour c, ascending.  With a halo attached only the owned nodes are listed. */
int c8_krylov_colors(c8_ctx* ctx, int32_t* num_colors, const int32_t** color_ptr, const int32_t** nodes);
/* Diagnostic / test access: the aggregates of C8_PRECOND_TWO_LEVEL (HOST array owned by the context, built at the first
 * use, freed by c8_destroy): aggregate_of_node[i] in [0, num_aggregates) for every node i.  Reported above the cap of the
 * coarse solve too.  C8_ERR_UNSUPPORTED with a halo attached. */
int c8_krylov_aggregates(c8_ctx* ctx, int32_t* num_aggregates, const int32_t** aggregate_of_node);
/* Diagnostic / test access: where this rank's aggregates start in the global numbering of C8_PRECOND_TWO_LEVEL_PARTS, and how
 * many there are over all ranks (n_c = NC x total_aggregates).  Without a halo: 0 and the count of c8_krylov_aggregates.
 * With a halo attached and another kind selected: C8_ERR_UNSUPPORTED. */
int c8_krylov_aggregate_base(c8_ctx* ctx, int32_t* base, int32_t* total_aggregates);
/* Diagnostic / test access: runs the set-up of C8_PRECOND_TWO_LEVEL on `sys` up to A_c = P^T A P (whatever kind is
 * selected) and copies the dense row-major n_coarse x n_coarse matrix to out_host (HOST memory); out_host NULL returns
 * n_coarse only.  C8_ERR_UNSUPPORTED with a halo attached or above the cap. */
int c8_krylov_coarse_matrix(c8_ctx* ctx, const c8_system* sys, int32_t* n_coarse, double* out_host);
/* Diagnostic / test access: the levels of C8_PRECOND_MULTILEVEL under the current settings (HOST arrays owned by the
 * context, built at the first use, valid until c8_krylov_set_multilevel or c8_destroy).  c8_krylov_levels: their number,
 * level 0 included; reported with a last level above the cap too.  c8_krylov_level, level in [0, num_levels): the node
 * count, the aggregate of every node and the colour lists in the layout of c8_krylov_colors; the last level has neither
 * (aggregate_of_node, color_ptr, nodes = NULL, num_colors = 0).  C8_ERR_UNSUPPORTED with a halo attached. */
int c8_krylov_levels(c8_ctx* ctx, int32_t* num_levels);
int c8_krylov_level(c8_ctx* ctx, int32_t level, int32_t* num_nodes, const int32_t** aggregate_of_node, int32_t* num_colors,
                    const int32_t** color_ptr, const int32_t** nodes);
/* Diagnostic / test access: runs the set-up of C8_PRECOND_MULTILEVEL on `sys` up to A_level, level in [1, num_levels)
 * (whatever kind is selected), and copies it as a dense row-major n_level x n_level matrix to out_host (HOST memory);
 * out_host NULL returns n_level only.  C8_ERR_UNSUPPORTED with a halo attached, and when this level or the last one is
 * above the cap. */
int c8_krylov_level_matrix(c8_ctx* ctx, const c8_system* sys, int32_t level, int32_t* n_level, double* out_host);
/* y = M^-1 v, once, with the context's current preconditioner: the block inverses and the kernels of the solve, and its
 * refusals (C8_ERR_ARG for a singular diagonal block, the node named, and for a vector or matrix that is not finite).
 * v and y are DEVICE pointers laid out as b and dx (v[1], y[1] unused when c8_num_residuals() == 1).  Not collective: with
 * a halo attached the part-local operator is applied and y is written on the owned nodes.  The last copy into y is
 * enqueued on the context's stream (c8_set_stream) and the call returns without waiting for it: y is valid for later work
 * on that stream, and for the host after the stream has been synchronised. */
int c8_krylov_precondition(c8_ctx* ctx, const c8_system* sys, const double* const v[2], double* const y[2]);

/* ---- multi-part meshes: owned/ghost halo and reductions ---------------------------------
 * One process per GPU, one mesh part per process, elements not ghosted, nodes on part boundaries shared -- the
 * reference's MPI scheme (disc.cpp:237,297).  Local node numbering of a part: OWNED nodes, then GHOST nodes (touched
 * by a local element, owned elsewhere), then PHANTOM nodes (not touched locally: columns of owned interface rows,
 * reserved in the graphs through c8_mesh_desc.extra_pairs), so that the OWNED matrix and vectors are prefix views of
 * the local arrays and every exchange lands in place.  What replaces what:
 *   C1  c8_halo_gather (C8_HALO_B)      LinearAlg::gather_b, Tpetra Export ADD          linear_alg.cpp:78-86
 *   C2  c8_halo_gather (C8_HALO_A)      LinearAlg::gather_A                             linear_alg.cpp:53-63
 *   C3  c8_halo_scatter_x               apf::synchronize in Disc::add_to_soln / Import  disc.cpp:944-947, :1001
 *   C4  c8_comm_allreduce_sum           PCU_Add_Doubles(grad)                           adjoint_objective.cpp:109
 *   C5  c8_comm_allreduce_sum           PCU_Add_Double(J), PCU_Add_Int(status)          adjoint_objective.cpp:39,99; primal.cpp:100,164
 * Transport: RCCL point-to-point over xGMI (grouped ncclSend/ncclRecv, one message per neighbour and exchange, on a
 * stream of its own; pack and unpack-add are HIP kernels on the context's stream), or a caller-supplied host exchange
 * (an MPI host without device-aware transport; several ranks sharing one card, which RCCL refuses).  The received
 * contributions of a value are added in ascending source-rank order: the gathered system is bitwise reproducible. */
typedef struct c8_comm c8_comm;
typedef struct c8_halo c8_halo;
enum { C8_COMM_ID_BYTES = 128 };
/* RCCL: rank 0 calls c8_comm_rccl_id, the caller broadcasts the 128 bytes by whatever it has (MPI_Bcast in the
 * reference's host code, torch.distributed in this repo's bench), every rank calls c8_comm_create_rccl with its HIP
 * device current.  librccl is loaded at the first of these calls (C8_RCCL_LIB overrides the search). */
int c8_comm_rccl_id(void* id_out);
int c8_comm_create_rccl(const void* id, int rank, int nranks, c8_comm** out);
/* Host transport.  exchange: chunk r of `send` (send_counts[r] doubles, chunks back to back in rank order) goes to
 * rank r, chunk r of `recv` (recv_counts[r] doubles) comes from rank r; HOST buffers; blocking.  allreduce: in-place
 * SUM of n HOST doubles.  Both return 0 on success. */
typedef int (*c8_host_exchange_fn)(void* user, const double* send, const int64_t* send_counts, double* recv,
                                   const int64_t* recv_counts);
typedef int (*c8_host_allreduce_fn)(void* user, double* values, int n);
int c8_comm_create_host(int rank, int nranks, c8_host_exchange_fn exchange, c8_host_allreduce_fn allreduce, void* user,
                        c8_comm** out);
void c8_comm_destroy(c8_comm* comm);
int c8_comm_rank(const c8_comm* comm);
int c8_comm_size(const c8_comm* comm);
/* C4 / C5: in-place SUM over the ranks of n HOST doubles (gradient, objective, failure flag packed by the caller). */
int c8_comm_allreduce_sum(c8_comm* comm, double* values, int n);

/* The exchange lists of one part (HOST arrays, copied).  What Tpetra derives from the OWNED and GHOST maps
 * (disc.cpp:316-332); the caller gets them from its mesh database (PUMI's remote copies in the reference).
 * Rows travel whole, in the SENDER's graph order; the receiver needs the sender's column lists once. */
typedef struct {
  int32_t num_owned, num_touched;   /* local nodes [0, num_owned) owned, [num_owned, num_touched) ghost, rest phantom */
  /* export, C1/C2: my ghost rows, grouped by owner rank; send_ptr [nranks+1] */
  const int64_t* send_ptr;
  const int32_t* send_nodes;        /* local (ghost) node ids */
  /* rows I own that rank r sends me, in r's order, with r's column list of each row in MY local ids */
  const int64_t* recv_ptr;          /* [nranks+1] */
  const int32_t* recv_nodes;        /* local (owned) node ids */
  const int64_t* recv_col_ptr;      /* [recv_ptr[nranks] + 1] */
  const int32_t* recv_cols;         /* local node ids (owned, ghost or phantom) */
  /* import, C3: nodes whose values I receive (every ghost and phantom node), grouped by owner rank; and the owned
   * nodes I send to each importing rank, in the importer's order */
  const int64_t* import_ptr;        /* [nranks+1] */
  const int32_t* import_nodes;
  const int64_t* export_ptr;        /* [nranks+1] */
  const int32_t* export_nodes;
  /* shape of the systems the tables are for: equations per node of residual 0 (c8_num_dims: 3, or 2 on tri3 meshes) and
   * the number of residuals (c8_num_residuals: 2, or 1 under mechanics_plane_stress); 0 = 3 and 2 */
  int32_t num_dims, num_residuals;
} c8_halo_desc;
/* Index tables of the exchanges, built on the host from the part's node graph (= block (1,1) of c8_graph(): one row
 * per node, sorted neighbour ids) -- needs no device. */
int c8_halo_build(int32_t num_nodes, const int64_t* node_rowptr, const int32_t* node_colidx, const c8_halo_desc* desc,
                  int rank, int nranks, c8_halo** out);
/* Device mirrors of the tables, message buffers, events, on the context's device; the context's graph must be the one
 * the tables were built from.  Also registers the halo with the context: the step drivers (c8_primal_solve_step,
 * c8_adjoint_solve_step) and the calibration objective then work over all parts. */
int c8_halo_attach(c8_halo* halo, c8_ctx* ctx, c8_comm* comm);
void c8_halo_destroy(c8_halo* halo);
enum { C8_HALO_B = 1, C8_HALO_A = 2 };
/* C1 and/or C2 in ONE message per neighbour: ghost rows of b (C8_HALO_B), of the four blocks of A (C8_HALO_A) or both
 * are packed on the context's stream and sent; c8_halo_gather_finish adds what arrived into the owned rows, on the
 * context's stream.  Work enqueued on the context's stream between the two calls (interior elements, the owned rows'
 * sums: c8_gather_finish) overlaps the exchange.  Afterwards the first num_owned node rows hold the OWNED system;
 * ghost rows are scratch.  c8_halo_gather = start + finish. */
int c8_halo_gather_start(c8_halo* halo, const c8_system* sys, int what);
int c8_halo_gather_finish(c8_halo* halo, const c8_system* sys);
int c8_halo_gather(c8_halo* halo, const c8_system* sys, int what);
/* C3: owner values of a nodal field pair x = {u [nodes*num_dims], p [nodes]} (x[1] unused with one residual) copied to
 * every ghost and phantom copy. */
int c8_halo_scatter_x(c8_halo* halo, double* const x[2]);
/* bytes this rank sends per exchange (what = C8_HALO_A | C8_HALO_B, or 0 for the C3 import) */
int64_t c8_halo_send_bytes(const c8_halo* halo, int what);
/* Diagnostic / test access to the host tables (tests/ replay the exchanges in numpy without a device):
 * which = 0 gather send codes, 1 gather send counts per rank, 2 gather recv counts, 3 unpack destinations (codes),
 * 4 unpack source offsets, 5 unpack source list; 10..15 the same for C8_HALO_B alone; 20 import send codes (C3),
 * 21 its send counts, 22 its recv counts, 23 its destination codes.  A code is (segment << 56) | offset with segment
 * 0..3 = A00 A01 A10 A11, 4 = b[0] / x[0], 5 = b[1] / x[1]. */
int c8_halo_table(const c8_halo* halo, int which, int64_t* n, const int64_t** data);

/* ---- canonical optimisation variables (HOST arrays) -------------------------------
 * Objective::transform_params / transform_gradient (objective.cpp:41-61,125-137) and their Python twins
 * (python/calibr8/util/parameter_transforms.py:31-59).  kind[i]: C8_SCALE_NONE (identity),
 * C8_SCALE_LOG (a = reference value: canonical = log(value / a)), C8_SCALE_BOUNDS (a = lower, b = upper:
 * canonical = (clip(value) - mean) / span in [-1, 1]). */
enum { C8_SCALE_NONE = 0, C8_SCALE_LOG = 1, C8_SCALE_BOUNDS = 2 };
int c8_transform_params(int n, const double* values, const int32_t* kind, const double* a, const double* b,
                        int from_canonical, double* out);
/* d(objective)/d(canonical) from d(objective)/d(physical); `values` are the CANONICAL values for log
 * scales, as in grad_transform (parameter_transforms.py:53-59). */
int c8_transform_gradient(int n, const double* grad, const double* values, const int32_t* kind, const double* a,
                          const double* b, double* out);

/* ---- superconvergent patch recovery (cspr.cpp: spr_recovery) ------------------------------
 * A point field [num_elems][c8_num_local_points][ncomp] brought to the nodes [num_nodes][ncomp]: per node and component
 * the least-squares polynomial 1, x, y(, z) through the samples of the node's patch, evaluated at the node.  Samples are
 * the local-state points (ip set 0) at their isoparametric positions.  The patch of a node starts as its elements
 * (getInitialPatch) and is accepted when points_per_element * |patch| >= 1.1 * terms and the fit matrix, in coordinates
 * centred at the node and scaled by h = max_s |x_s - x_n|_inf, has no |R_kk| <= 1e-8 sqrt(samples) in its QR
 * factorisation; otherwise it grows as expandAsNecessary does, with "shares an entity of dimension d-1, ..., 0 with an
 * element of the frozen patch" read as "has at least m nodes in common": m = 3, 2, 1 (tet4), 4, 2, 1 (hex8), 2, 1 (tri3),
 * tested after every stage, repeated from the grown patch while it grows.  A patch that stops growing unaccepted fails
 * the call: C8_ERR_ARG, the message names the node ("all hope is lost").  The linear fit only (the mesh is linear).
 *
 * c8_spr_recover: ip_field and nodal are DEVICE pointers, the layouts of sigma (ncomp 9) and xi (ncomp =
 * c8_num_local_dofs); nodal is OVERWRITTEN, ip_field is not written.  1 <= ncomp <= 16 and non-null pointers, else
 * C8_ERR_ARG.  The tables (patches, one coefficient vector g [num_dims + 1] and one h per node) depend on the mesh alone:
 * they are built at the first call (device fit of every node, host expansion of the few nodes it flags) and kept.  A
 * call is one kernel without atomics: two calls give the same bytes.  Stream, async mode and return value as
 * c8_eval_cauchy (the first call also waits for its set-up).  With a halo attached (c8_halo_attach): C8_ERR_UNSUPPORTED,
 * patches cross part boundaries. */
int c8_spr_recover(c8_ctx* ctx, int ncomp, const double* ip_field, double* nodal);
/* interpolate_to_cell_center (main_spr_error.cpp), at the local-state points: ip_field [num_elems][c8_num_local_points]
 * [ncomp] = sum_a N_a(point) nodal[node a][ncomp] (tet4, tri3: the centroid, as there).  DEVICE pointers, ip_field
 * OVERWRITTEN; arguments, stream, async mode and return value as c8_spr_recover.  Not collective: needs the ghost entries
 * of nodal imported, like every other entry point. */
int c8_interpolate_to_points(c8_ctx* ctx, int ncomp, const double* nodal, double* ip_field);
/* Diagnostic / test access to the HOST copies of the tables, in the manner of c8_halo_table (built if needed; valid
 * until c8_destroy): which = 0 patch_ptr (int64 [num_nodes + 1]), 1 patch_elems (int32, ascending per node), 2 g (double
 * [num_nodes][num_dims + 1]), 3 h (double [num_nodes]), 4 expansion stages run per node (int32 [num_nodes]; 0: the
 * node's own elements were enough), 5 set-up record (double [4]: ms device fit and read-back, ms host expansion and table,
 * ms upload, nodes the device fit flagged).  C8_ERR_UNSUPPORTED with a halo attached. */
int c8_spr_table(c8_ctx* ctx, int which, int64_t* n, const void** data);
/* The same set-up on the host with the same functions (c8_spr.hpp): no context, no device, HOST arrays.  patch_ptr
 * [num_nodes + 1] is always filled; with patch_elems == NULL nothing else is needed (the caller sizes patch_elems from
 * patch_ptr[num_nodes]); otherwise patch_elems has `capacity` entries (too few: C8_ERR_ARG) and g [num_nodes][dims + 1],
 * h [num_nodes], stages [num_nodes] are filled where not NULL.  A patch that cannot be completed: C8_ERR_ARG,
 * *failed_node (may be NULL; else -1) is the node, the message names it. */
int c8_spr_build_host(int elem_type, int32_t num_nodes, int32_t num_elems, const double* coords, const int32_t* conn,
                      int64_t* patch_ptr, int32_t* patch_elems, int64_t capacity, double* g, double* h, int32_t* stages,
                      int32_t* failed_node);

/* ---- host helpers for synthetic problems -------------------------------- */
/* Structured hex8 brick; coords [(nx+1)(ny+1)(nz+1)][3], conn [nx*ny*nz][8] (host arrays). */
int c8_brick_mesh(int nx, int ny, int nz, double lx, double ly, double lz, double* coords, int32_t* conn);
/* Block partition px*py*pz of that brick: part id per element (host array). */
int c8_brick_partition(int nx, int ny, int nz, int px, int py, int pz, int32_t* elem_part);

/* ---- outer optimiser: bound-constrained L-BFGS on the canonical variables, with the controls of
 * the reference's ROL set-up (main_inverse.cpp:21-28, :83-120: secant storage, iteration limit, gradient and step
 * tolerances, function evaluations per line search).  HOST arrays; `fn` returns 0, or non-zero when the objective
 * cannot be evaluated at x (the line search then shortens the step). */
typedef int (*c8_objective_fn)(void* user, int n, const double* x, double* f, double* grad);
typedef struct {
  int32_t max_iters;      /* "iteration limit" (20) */
  double grad_tol;        /* "gradient tolerance" (1e-12), on the projected gradient */
  double step_tol;        /* "step tolerance" (1e-12) */
  int32_t max_ls_evals;   /* "max line search evals" (5) */
  int32_t memory;         /* secant storage (20) */
} c8_lbfgs_opts;
enum { C8_LBFGS_ITERATION_LIMIT = 0, C8_LBFGS_GRADIENT_TOL = 1, C8_LBFGS_STEP_TOL = 2, C8_LBFGS_LINE_SEARCH_FAILED = 3 };
typedef struct {
  int32_t iters, evals, status;
  double f, projected_gradient_norm;
} c8_lbfgs_result;
int c8_lbfgs_minimize(int n, double* x, const double* lo, const double* hi, c8_objective_fn fn, void* user,
                      const c8_lbfgs_opts* opts, c8_lbfgs_result* res);

#ifdef __cplusplus
}
#endif
#endif /* C8_H */
