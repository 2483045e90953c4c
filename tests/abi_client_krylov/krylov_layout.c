/* tests/abi_client_krylov/krylov_layout.c -- TEST INFRASTRUCTURE.  Compiled as C11 (gcc) and as C++17 (g++) against
 * include/c8.h, no device needed.  Prints sizeof / offsetof of the structs of the device-resident linear solve as JSON;
 * tests/test_abi_krylov.py compares both outputs with the ctypes mirror in calibr8_amd/lib.py. */
#include <stddef.h>
#include <stdio.h>

#include "c8.h"

#define S(type) printf("%s \"%s\": {\"sizeof\": %zu", first++ ? ",\n" : "", #type, sizeof(type))
#define F(type, field) printf(", \"%s\": %zu", #field, offsetof(type, field))
#define E() printf("}")

int main(void) {
  int first = 0;
  /* the entry points have the types the ctypes table gives them (checked by the compiler, not evaluated: nothing to link) */
  int (*solve)(c8_ctx*, const c8_system*, double* const[2], const c8_krylov_opts*, c8_krylov_info*) = 0;
  c8_linear_solve_fn callback = 0;
  (void)sizeof(solve = c8_krylov_solve);
  (void)sizeof(callback = c8_krylov_linear_solve);
  printf("{\n");
  S(c8_krylov_opts); F(c8_krylov_opts, max_iters); F(c8_krylov_opts, check_every); F(c8_krylov_opts, max_restarts);
  F(c8_krylov_opts, rel_tol); F(c8_krylov_opts, abs_tol); E();
  S(c8_krylov_info); F(c8_krylov_info, iters); F(c8_krylov_info, restarts); F(c8_krylov_info, status); F(c8_krylov_info, b_norm);
  F(c8_krylov_info, residual_norm); E();
  S(c8_krylov_user); F(c8_krylov_user, ctx); F(c8_krylov_user, opts); F(c8_krylov_user, info); F(c8_krylov_user, total_iters);
  F(c8_krylov_user, solves); E();
  printf("\n}\n");
  return 0;
}
