"""The oracle's total adjoint gradient dJ/dp, parameter by parameter, against Richardson-extrapolated central differences
of the converged objective (gradient_cases.fd_gradient): the one reference that shares no algorithm with the adjoint.  The
differences use the forward path only, which the deck pins fix to the reference, and Newton converges to the residual's root
whatever the Jacobian does.  Every row of C8_MODEL_TABLE, every parameter of the row, on hex8 and tet4 (3-D rows) or tri3.

Asserted per parameter k, with span_k = |p_k| (1 where p_k = 0) and scale = max_j |g_j span_j|:

    |g_k - R_k| span_k <= BAR scale

and, on the reference alone, so that a bad reference can neither hide a failure nor invent one: every one of the six
perturbed solves has the base solve's per-step mask of yielding points, and the two extrapolants agree within BAR / 10.

BAR is ten times the worst ratio |g_k - R_k| span_k / scale measured over all cases (the factor allows for the noise of J,
about 1e-15 from a Newton tolerance of 1e-12, divided by the step) and may never exceed 1e-7, the bar of the directional
check in test_oracle_checks.py.  Measured worst ratio per row (s = 1e-3 unless noted), over the row's cases:

    row                              worst ratio    where
    elastic                          2.0e-11        hex8
    small_J2 (3-D)                   2.3e-11        hex8
    hyper_J2                         3.9e-10        hex8
    small_hill                       4.3e-09        hex8, two element sets (one set: 1.9e-09; calibration: 9.8e-10)
    isotropic_elastic                4.5e-11        hex8
    hypo_hill                        1.7e-09        tet4
    small_hosford                    1.2e-09        hex8
    hypo_hosford                     5.1e-10        hex8
    hypo_barlat                      6.6e-10        hex8
    small_J2 (2-D)                   1.1e-12        tri3
    small_hill_plane_strain          5.0e-11        tri3 (s = 5e-4)
    hyper_J2_plane_strain            3.1e-10        tri3
    hypo_hill_plane_strain           1.4e-10        tri3
    small_hill_plane_stress          6.9e-09        tri3 (calibration: 2.3e-09)
    hyper_J2_plane_stress            1.4e-09        tri3
    hypo_hill_plane_stress           1.3e-09        tri3
    hybrid_hyper_J2_plane_stress     7.5e-10        tri3, E nu Y and the four weights

The worst is 6.9e-09, so BAR = 7e-8.  Where the ratio is ~1e-9 the two extrapolants agree to ~1e-12: the difference is the
adjoint's, which linearises about states converged to the Newton tolerances, not the reference's.
"""
import numpy as np
import pytest

import gradient_cases as gc

BAR = 7e-8
assert BAR <= 1e-7


def test_every_parameter_of_every_row_has_a_case():
    # every row of C8_MODEL_TABLE on every mesh it runs on; the oracle refuses a parameter vector whose length is not the
    # row's NPARAMS (c8o_create), and the gradient tests loop over every entry of that vector
    have = {(c.model, c.kind) for c in gc.CASES if c.objective == "avg_disp" and c.elem_set is None}
    rows = gc.model_table()
    assert len(rows) >= 17
    for model, dim in rows:
        for kind in (("hex8", "tet4") if dim == 3 else ("tri3",)):
            assert (model, kind) in have, "no gradient case for %s on %s" % (model, kind)
            case = gc.BY_NAME["%s-%s" % (model, kind)]
            orc = case.oracle(case.params)  # raises unless len(params) == NPARAMS of the row
            nparams = orc.params.shape[1]
            assert [k for _, k in case.slots] == list(range(nparams)), (case.name, case.slots, nparams)
            assert set(case.zero) <= set(range(nparams))
    # the exact-zero parameters are the named ones only: parameters the model carries and never reads
    named = {c.model: c.zero for c in gc.CASES if c.zero}
    assert named == {"small_J2": (4, 5), "hypo_hosford": (4,)}, named


def test_meshes_and_objectives_of_the_case_table():
    for kind, want in (("hex8", {1, 2, 4}), ("tet4", {1, 2, 4}), ("tri3", {2, 8})):
        et, c, conn, sets = gc.mesh(kind)
        assert want <= set(gc.elems_per_node(kind).tolist()), kind
        assert len(conn) <= 10
        for name, nodes in sets.items():  # the node sets stayed planar
            d = "xyz".index(name[0])
            assert np.ptp(c[nodes, d]) == 0.0 and len(nodes) >= 2
    et, c, conn, _ = gc.mesh("hex8")
    for e in conn:  # no hex8 element is a parallelepiped: opposite edges differ
        X = c[e]
        assert np.abs((X[1] - X[0]) - (X[2] - X[3])).max() > 1e-2 or np.abs((X[4] - X[0]) - (X[5] - X[1])).max() > 1e-2
    cal = sorted((c.model, c.kind) for c in gc.CASES if c.objective == "calibration")
    assert cal == [("hyper_J2", "tet4"), ("small_hill", "hex8"), ("small_hill_plane_stress", "tri3")]
    two = [c for c in gc.CASES if c.elem_set is not None]
    assert len(two) == 1 and two[0].kind == "hex8" and len(two[0].slots) == 9
    assert [len(v) for _, v in sorted(two[0].groups_all().items())] == [8, 1]
    assert not np.array_equal(two[0].params[0], two[0].params[1])


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_oracle_adjoint_gradient_matches_differences_per_parameter(case):
    J, g, pr = gc.oracle_reference(case)
    gc.check_history(case, pr)
    p = case.p0()
    sp = gc.spans(p)
    assert len(g) == len(p) == len(case.slots)
    scale = np.abs(g * sp).max()
    assert scale > 0.0 and J != 0.0
    if case.objective == "calibration":  # the explicit dJ/dp term of K5 is there: the load mismatch is not zero
        pr.begin_qoi_step(gc.NSTEPS)
        assert abs(pr.be.qoi_preprocess(pr.u[-1], pr.p[-1], pr.u[-2], pr.p[-2], pr.xi[-2], pr.xi[-1])[2]) > 1e-3
    base = gc.yielded_masks(pr, case.hardening)
    worst, bad_reference, bad = 0.0, [], []  # every parameter is judged before the test fails: the report names all that miss
    for k in range(len(p)):
        R, R2, masks = gc.fd_gradient(case.solve, p, k, sp[k], case.s, case.hardening)
        ratio, gap = abs(g[k] - R) * sp[k] / scale, abs(R - R2) * sp[k] / scale
        print("%s slot %d %r: g %.9e R %.9e ratio %.2e extrapolants %.2e" % (case.name, k, case.slots[k], g[k], R, ratio, gap))
        # the reference alone
        assert len(masks) == 6
        if not all(len(m) == len(base) and all(np.array_equal(a, b) for a, b in zip(m, base)) for m in masks):
            bad_reference.append((k, "yielded masks differ"))
        if not gap <= 0.1 * BAR:
            bad_reference.append((k, "extrapolants", gap))
        # the adjoint against it
        if k in case.zero:
            if not (g[k] == 0.0 and R == 0.0 and R2 == 0.0):
                bad.append((k, case.slots[k], g[k], R, R2))
            continue
        if not ratio <= BAR:
            bad.append((k, case.slots[k], g[k], R, ratio))
        worst = max(worst, ratio)
    print("%s worst ratio %.2e" % (case.name, worst))
    assert not bad_reference, (case.name, "the difference reference fails its own conditions", bad_reference)
    assert not bad, (case.name, "adjoint components off the difference reference (slot, (set, parameter), g, R, ratio)", bad)
