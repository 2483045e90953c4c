// c8_registry.hpp -- the constitutive models: one row per (reference name, mesh dimension), read by the C ABI
// (c8_api.hip), the kernel registry (c8_kernels.hip) and the CPU lane emulator (tests/emul).  HIP-free.
#pragma once

#include <type_traits>

#include "c8_element.hpp"
#include "c8_models.hpp"

namespace c8 {

enum { MODEL_NONE = -1, MODEL_ELASTIC = 0, MODEL_SMALL_J2 = 1, MODEL_HYPER_J2 = 2, MODEL_SMALL_HILL = 3, MODEL_ISOTROPIC_ELASTIC = 4, MODEL_HYPO_HILL = 5,
       MODEL_SMALL_HILL_PLANE_STRAIN = 6, MODEL_HYPER_J2_PLANE_STRAIN = 7, MODEL_HYPO_HILL_PLANE_STRAIN = 8,
       MODEL_SMALL_HILL_PLANE_STRESS = 9, MODEL_HYPER_J2_PLANE_STRESS = 10, MODEL_HYPO_HILL_PLANE_STRESS = 11,
       MODEL_SMALL_HOSFORD = 12, MODEL_HYPO_HOSFORD = 13, MODEL_HYPO_BARLAT = 14, MODEL_HYBRID_HYPER_J2_PLANE_STRESS = 15 };

// X(id, name, mesh dimension, model class template, compile part on hex8, compile part on tet4), the names those of the
// reference's factory (local_residual.cpp:893-933).  The compile parts of c8_kernels.hip (-DC8_KERNEL_PART): 0 hex8
// elastic / small_J2 / isotropic_elastic, 1 hyper_J2 / small_hill, 2 hypo_hill, 3 tet4, 4 tri3 (every 2-D row),
// 5 Hosford / Barlat; -1: not on that element.
#define C8_MODEL_TABLE(X)                                                                            \
  X(MODEL_ELASTIC, "elastic", 3, Elastic, 0, 3)                                                      \
  X(MODEL_SMALL_J2, "small_J2", 3, SmallJ2, 0, 3)                                                    \
  X(MODEL_HYPER_J2, "hyper_J2", 3, HyperJ2, 1, 3)                                                    \
  X(MODEL_SMALL_HILL, "small_hill", 3, SmallHill, 1, 3)                                              \
  X(MODEL_ISOTROPIC_ELASTIC, "isotropic_elastic", 3, IsotropicElastic, 0, 3)                         \
  X(MODEL_HYPO_HILL, "hypo_hill", 3, HypoHill, 2, 3)                                                 \
  X(MODEL_SMALL_HOSFORD, "small_hosford", 3, SmallHosford, 5, 5)                                     \
  X(MODEL_HYPO_HOSFORD, "hypo_hosford", 3, HypoHosford, 5, 5)                                        \
  X(MODEL_HYPO_BARLAT, "hypo_barlat", 3, HypoBarlat, 5, 5)                                           \
  /* 2-D: the models of the reference's 2-D decks on `mechanics` (2 + 1 equations per node) ... */   \
  X(MODEL_SMALL_J2, "small_J2", 2, SmallJ2Plane, -1, -1)                                             \
  X(MODEL_SMALL_HILL_PLANE_STRAIN, "small_hill_plane_strain", 2, SmallHillPlaneStrain, -1, -1)       \
  X(MODEL_HYPER_J2_PLANE_STRAIN, "hyper_J2_plane_strain", 2, HyperJ2PlaneStrain, -1, -1)             \
  X(MODEL_HYPO_HILL_PLANE_STRAIN, "hypo_hill_plane_strain", 2, HypoHillPlaneStrain, -1, -1)          \
  /* ... and on `mechanics_plane_stress` (2 equations per node, no pressure) */                      \
  X(MODEL_SMALL_HILL_PLANE_STRESS, "small_hill_plane_stress", 2, SmallHillPlaneStress, -1, -1)       \
  X(MODEL_HYPER_J2_PLANE_STRESS, "hyper_J2_plane_stress", 2, HyperJ2PlaneStress, -1, -1)             \
  X(MODEL_HYPO_HILL_PLANE_STRESS, "hypo_hill_plane_stress", 2, HypoHillPlaneStress, -1, -1)          \
  X(MODEL_HYBRID_HYPER_J2_PLANE_STRESS, "hybrid_hyper_J2_plane_stress", 2, HybridHyperJ2PlaneStress, -1, -1)

// One row.  Its type carries the model's class template M and everything but the name as constants.  A kernel template
// takes M by deduction from the row's ModelTag<M> base: that gives the template itself, so the kernel symbols name the model.
template <template <class> class M> struct ModelTag {};
template <template <class> class M, int ID, int DIM, int HEX8_PART, int TET4_PART> struct ModelRow : ModelTag<M> {
  static constexpr int id = ID, dim = DIM, hex8_part = HEX8_PART, tet4_part = TET4_PART, tri3_part = DIM == 2 ? 4 : -1;
  using Real = M<double>;  // NLOC, NPARAMS, init_variables
  // the plane-stress models carry sigma_zz = 0 and no pressure: they run on `mechanics_plane_stress` and only there
  static constexpr bool plane_stress = is_plane_stress<Real>::value;
  using Elem2D = std::conditional_t<plane_stress, Tri3PlaneStress, Elem<C8_TRI3>>;  // the element class of a 2-D row
  char const* name;
};

// f(row) for every row of the table, in its order
template <class F> void visit_models(F&& f) {
#define C8_VISIT_ROW(ID, NAME, DIM, M, HEX8_PART, TET4_PART) f(ModelRow<M, ID, DIM, HEX8_PART, TET4_PART>{{}, NAME});
  C8_MODEL_TABLE(C8_VISIT_ROW)
#undef C8_VISIT_ROW
}

inline bool model_is_plane_stress(int m) {
  bool ps = false;
  visit_models([&](auto row) { if (row.id == m) ps = row.plane_stress; });
  return ps;
}

}  // namespace c8
