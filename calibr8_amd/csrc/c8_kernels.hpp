// c8_kernels.hpp -- launcher table between the C ABI (c8_api.hip) and the kernels.
#pragma once

#include <hip/hip_runtime_api.h>

#include "c8_assemble_adjoint.hpp"
#include "c8_assemble_vfm.hpp"
#include "c8_assemble_nn.hpp"
#include "c8_registry.hpp"

namespace c8 {

struct LaunchArgs {
  MeshTables mt;
  ModelSettings ms;
  FieldArgs fa;
  AdjointArgs aa;
  SystemArgs sa;
  int first, count;  // range of the element order to process
  hipStream_t stream;
};

typedef hipError_t (*LaunchFn)(LaunchArgs const&);
typedef hipError_t (*GatherFn)(GatherArgs const&, int first, int count, int max_degree, hipStream_t);
// aa = null: forward assembly; aa != null: adjoint assembly (objective "average displacement")
typedef hipError_t (*NodeRowsFn)(MeshTables const&, ModelSettings const&, FieldArgs const&, AdjointArgs const* aa, GatherArgs const&, int first,
                                 int count, int max_degree, int max_node_elems, hipStream_t);
// the VFM kernels (c8_assemble_vfm.hpp): the whole mesh in one launch, one partial sum per output and block into part
typedef hipError_t (*VfmFn)(LaunchArgs const&, VfmArgs const&, double* part);

// the closed form's per-set constants from the device parameters (Model::closed_form_constants): table[nsets][num_constants]
typedef hipError_t (*ConstantsFn)(double const* params, double* table, int nsets, hipStream_t);

struct KernelSet {
  LaunchFn forward_jacobian;   // K1, one lane group (NDOF lanes) per element
  LaunchFn forward_jacobian_wave;  // K1, one wavefront per element (hex8 only, else null)
  LaunchFn residual;           // K2
  LaunchFn residual_wave;      // K2, eight hex8 elements per wavefront, atomic adds (hex8 only, else null)
  LaunchFn adjoint_jacobian;   // K3
  LaunchFn adjoint_jacobian_wave;  // K3, one wavefront per element (hex8 only, else null)
  LaunchFn adjoint_local;      // K4 (per-point outputs only: one launch, no colouring)
  LaunchFn param_gradient;     // K5 (grid-stride, one atomic per lane at the end)
  LaunchFn adjoint_local_wave;     // K4, one wavefront per element (hex8 only, else null)
  LaunchFn adjoint_local_closed;   // K4 in the model's closed form, eight elements per wavefront (hex8 models with one, else null)
  LaunchFn param_gradient_closed;  // K5 likewise
  LaunchFn param_gradient_wave;    // K5, one wavefront per element (hex8 only, else null)
  LaunchFn qoi;                // K6 (hex8: eight elements per wavefront)
  LaunchFn qoi_slot;           // K6, one lane per point of a lane group (any element type)
  hipError_t (*shape_tables)(MeshTables const&, double* tab, int nelems, hipStream_t);  // cached shape tables of the wave kernels (hex8, else null)
  int shape_stride;            // doubles per element in that table
  GatherFn gather_rows;        // staged assembly: node rows summed from the element-major stage
  NodeRowsFn node_rows;        // K1 and K3, one wavefront per node, no stage (hex8 models with a closed form, else null)
  int stage_stride;            // doubles per element in the stage
  bool adjoint_slot_stages;    // the slot-per-lane K3 can store into the stage (it transposes through LDS first)
  bool can_stage;              // staged (gather) assembly available for this element type
  // virtual fields method: Tri3PlaneStress (one residual) only, else null
  VfmFn vfm_power = nullptr;         // V
  VfmFn vfm_forward_sens = nullptr;  // FS
  VfmFn vfm_adjoint = nullptr;       // A
  int vfm_groups_per_block = 0;      // element groups per block of those kernels (blocks = partial sums per output)
  // the row-per-node kernels read the closed form's parameter-only values from a table (MeshTables::cf_const): its filling
  // kernel and the doubles per element set; null / 0 where node_rows is null
  ConstantsFn closed_form_constants = nullptr;
  int num_constants = 0;
};

// the weight gradient of the embedded network (c8_assemble_nn.hpp): the partial rows of nn_grad_blocks(npts) blocks,
// then out[0 .. ntheta) += their sum in block order
hipError_t launch_nn_param_gradient(NnGradArgs const& ga, double* out, hipStream_t stream);

// the kernels of a row of the model table (c8_registry.hpp) on an element type; empty if there is none
KernelSet get_kernels(int elem_type, int model);

}  // namespace c8
