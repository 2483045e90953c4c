"""Host-side mirror of the reference's evaluation interface for the hot path.

`Assembler` plays the role of the (State, Disc) pair the reference's `eval_*` functions
take (evaluations.hpp:23-84): it owns the discretisation tables through a c8_ctx and
exposes one method per entry point with the same meaning and error behaviour
(0 / -1 for a failed local solve; everything else raises).  All field arrays are torch
float64 tensors resident in HBM; nothing here computes.
"""
import ctypes as C

import numpy as np

from . import lib as _l

NUM_PARAMS = {"elastic": 4, "small_J2": 6, "hyper_J2": 8, "small_hill": 11, "hypo_hill": 11, "isotropic_elastic": 2}
NEQ = (3, 1)


def brick_mesh(nx, ny, nz, lx=1.0, ly=1.0, lz=1.0):
    """Structured hex8 brick (SURVEY.md section 8d synthetic meshes): coords [N,3], conn [E,8]."""
    L = _l.load_library()
    coords = np.zeros(((nx + 1) * (ny + 1) * (nz + 1), 3))
    conn = np.zeros((nx * ny * nz, 8), dtype=np.int32)
    _l.check(L.c8_brick_mesh(nx, ny, nz, lx, ly, lz, coords.ctypes.data_as(_l.dp), conn.ctypes.data_as(_l.i32p)))
    return coords, conn


def brick_partition(nx, ny, nz, px, py, pz):
    L = _l.load_library()
    part = np.zeros(nx * ny * nz, dtype=np.int32)
    _l.check(L.c8_brick_partition(nx, ny, nz, px, py, pz, part.ctypes.data_as(_l.i32p)))
    return part


def spr_build_host(elem_type, coords, conn):
    """The set-up of Assembler.spr_recover on the host (c8_spr_build_host; needs no GPU): dict of patch_ptr, patch_elems, g,
    h, stages as in Assembler.spr_patches.  A patch that cannot be completed raises C8Error; its `node` is the node."""
    L = _l.load_library()
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    conn = np.ascontiguousarray(conn, dtype=np.int32)
    nnodes, nelems, T = len(coords), len(conn), (3 if int(elem_type) == _l.C8_ELEM_TRI3 else 4)
    assert coords.shape == (nnodes, 3) and conn.shape == (nelems, int(elem_type))
    ptr = np.zeros(nnodes + 1, dtype=np.int64)
    bad = C.c_int32(-1)

    def call(elems, cap, g, h, st):
        p = lambda a, t: None if a is None else a.ctypes.data_as(t)
        rc = L.c8_spr_build_host(int(elem_type), nnodes, nelems, coords.ctypes.data_as(_l.dp), conn.ctypes.data_as(_l.i32p),
                                 ptr.ctypes.data_as(_l.i64p), p(elems, _l.i32p), cap, p(g, _l.dp), p(h, _l.dp), p(st, _l.i32p),
                                 C.byref(bad))
        if rc < 0:
            err = _l.C8Error(rc, L.c8_last_error().decode())
            err.node = bad.value
            raise err

    call(None, 0, None, None, None)
    elems = np.zeros(int(ptr[-1]), dtype=np.int32)
    g, h, st = np.zeros((nnodes, T)), np.zeros(nnodes), np.zeros(nnodes, dtype=np.int32)
    call(elems, len(elems), g, h, st)
    return {"patch_ptr": ptr, "patch_elems": elems, "g": g, "h": h, "stages": st}


# the flat position of the hardening variable alpha in a point's local state where it is not the last unknown
_ALPHA_DOF = {"hypo_hill_plane_strain": 3, "hypo_hill_plane_stress": 3}
_NO_ALPHA = ("elastic", "isotropic_elastic")


def local_dof(local_type, nloc, name):
    """The flat index into a point's local state xi of the scalar local unknown `name` of the model `local_type` with
    `nloc` local unknowns (the reference names a scalar local residual; the library indexes xi): "alpha", the hardening
    variable, of the plasticity models."""
    if name != "alpha" or local_type in _NO_ALPHA:
        raise ValueError("local_dof: %s has no scalar local unknown %r" % (local_type, name))
    return _ALPHA_DOF.get(local_type, nloc - 1)


class LinearSystem:
    """A[i][j] CSR values and b[i] in GHOST distribution, as device tensors (la->A, la->b)."""

    def __init__(self, asm):
        import torch
        # one allocation, the six arrays are views of it: zero_all is one fill and the halo exchange packs and
        # unpacks all of them with one gather / one index_add (distributed.Halo.start_gather)
        sizes = [asm.nnz[i][j] for i in range(2) for j in range(2)] + [asm.nnodes * asm.neq[i] for i in range(2)]
        self.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)  # A00 A01 A10 A11 b0 b1
        self.flat = torch.zeros(int(self.offsets[-1]), dtype=torch.float64, device=asm.device)
        v = [self.flat[int(self.offsets[k]):int(self.offsets[k + 1])] for k in range(6)]
        self.A = [[v[0], v[1]], [v[2], v[3]]]
        self.b = [v[4], v[5]]

    def zero(self):  # la->zero_all(), primal.cpp:98
        self.flat.zero_()

    def c_struct(self):
        s = _l.System()
        for i in range(2):
            s.b[i] = self.b[i].data_ptr()
            for j in range(2):
                s.A[i][j] = self.A[i][j].data_ptr()
        return s


class Assembler:
    def __init__(self, elem_type, coords, conn, local_type, params, elem_set=None, stab_mult=1.0, max_iters=500,
                 abs_tol=1e-12, rel_tol=1e-12, device="cuda:0", scatter=None, extra_pairs=None, global_type=None,
                 thickness=0.0, line_search=None, embedded=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("calibr8_amd needs a HIP device: there is no CPU execution path")
        self.L = _l.load_library()
        self.torch = torch
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.coords = np.ascontiguousarray(coords, dtype=np.float64)
        self.conn = np.ascontiguousarray(conn, dtype=np.int32)
        self.elem_type = int(elem_type)
        self.nnodes, self.nelems, self.nn = self.coords.shape[0], self.conn.shape[0], self.conn.shape[1]
        self.local_type = local_type
        self.local_abs_tol = float(abs_tol)  # of the local Newton iteration: |C|_2 of a converged point is below it
        self.params = np.ascontiguousarray(np.atleast_2d(np.asarray(params, dtype=np.float64)))
        self.nsets = self.params.shape[0]
        self._es = None if elem_set is None else np.ascontiguousarray(elem_set, dtype=np.int32)
        self._xp = None if extra_pairs is None or len(extra_pairs) == 0 else \
            np.ascontiguousarray(extra_pairs, dtype=np.int32).reshape(-1, 2)
        md = _l.MeshDesc(self.elem_type, self.nnodes, self.nelems, self.nsets, self.coords.ctypes.data_as(_l.dp),
                         self.conn.ctypes.data_as(_l.i32p),
                         self._es.ctypes.data_as(_l.i32p) if self._es is not None else None,
                         0 if self._xp is None else len(self._xp),
                         None if self._xp is None else self._xp.ctypes.data_as(_l.i32p))
        if global_type is None:  # the pairing of the reference's decks
            global_type = "mechanics_plane_stress" if local_type.endswith("_plane_stress") else "mechanics"
        mo = _l.ModelDesc(global_type.encode(), local_type.encode(), stab_mult, max_iters, abs_tol, rel_tol,
                          self.params.shape[1], self.params.ctypes.data_as(_l.dp), float(thickness),
                          *((0.0, 0.0, 0.0, 0) if line_search is None else  # (c1, min factor, max factor, max evals)
                            (float(line_search[0]), float(line_search[1]), float(line_search[2]), int(line_search[3]))))
        h = C.c_void_p()
        _l.check(self.L.c8_create(C.byref(md), C.byref(mo), C.byref(h)))
        self.h = h
        self.nloc = self.L.c8_num_local_dofs(h)
        self.npts = self.L.c8_num_local_points(h)
        self.ncolors = self.L.c8_num_colors(h)
        self.ndims = self.L.c8_num_dims(h)  # 3, or 2 on tri3 meshes (u arrays are [nnodes * ndims])
        self.nres = self.L.c8_num_residuals(h)  # 2, or 1 under mechanics_plane_stress: the p arrays / blocks are not used
        self.neq = (self.ndims, 1)
        self.ndofs = (self.ndims + (1 if self.nres == 2 else 0)) * self.nn
        self.nnz = [[int(self.L.c8_graph_nnz(h, i, j)) for j in range(2)] for i in range(2)]
        self._graph = None
        self.kernel = "auto"            # what set_kernel asked for last
        self.objective = ("avg_disp",)  # ... and set_qoi_avg_disp / set_qoi_calibration: what two contexts must share
        if scatter is not None:  # None: the library's default (staged assembly, see c8_set_scatter_mode)
            self.set_scatter(scatter)
        self.use_current_stream()
        if embedded is not None:  # the `embedded model` sublist of hybrid_hyper_J2_plane_stress
            self.set_embedded_model(embedded["activation"], embedded["topology"], embedded["input_scale"],
                                    embedded["output_scale"])
            if embedded.get("params") is not None:
                self.set_embedded_params(embedded["params"])

    def __del__(self):
        if getattr(self, "h", None):
            self.L.c8_destroy(self.h)
            self.h = None

    # ---- discretisation ------------------------------------------------------------------
    @property
    def graph(self):
        """(rowptr[i][j], colidx[i][j]) host arrays of the four CSR blocks."""
        if self._graph is None:
            rp = [[None, None], [None, None]]
            ci = [[None, None], [None, None]]
            for i in range(2):
                for j in range(2):
                    r = np.zeros(self.nnodes * self.neq[i] + 1, dtype=np.int64)
                    c = np.zeros(self.nnz[i][j], dtype=np.int32)
                    _l.check(self.L.c8_graph(self.h, i, j, r.ctypes.data_as(_l.i64p), c.ctypes.data_as(_l.i32p)))
                    rp[i][j], ci[i][j] = r, c
            self._graph = (rp, ci)
        return self._graph

    @property
    def rowptr(self):
        return self.graph[0]

    @property
    def colidx(self):
        return self.graph[1]

    def new_state(self):
        xi = np.zeros((self.nelems, self.npts, self.nloc))
        _l.check(self.L.c8_init_variables(self.h, xi.ctypes.data_as(_l.dp)))
        return self.torch.from_numpy(xi).to(self.device)

    def new_linsys(self):
        return LinearSystem(self)

    def dev(self, a):
        return self.torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)

    # ---- settings ----------------------------------------------------------------------------
    def set_params(self, params):
        self.params = np.ascontiguousarray(np.atleast_2d(np.asarray(params, dtype=np.float64)))
        _l.check(self.L.c8_set_params(self.h, self.params.ctypes.data_as(_l.dp)))

    def set_active(self, es, idx):
        a = np.ascontiguousarray(idx, dtype=np.int32)
        _l.check(self.L.c8_set_active_params(self.h, es, len(a), a.ctypes.data_as(_l.i32p)))

    def set_embedded_model(self, activation, topology, input_scale, output_scale):
        """Network of hybrid_hyper_J2_plane_stress: activation "relu" | "sigmoid" | "tanh" (or a C8_ACT_* value)."""
        act = _l.C8_ACT[activation] if isinstance(activation, str) else int(activation)
        self._topology = np.ascontiguousarray(topology, dtype=np.int32)
        d = _l.EmbeddedModelDesc(act, len(self._topology), self._topology.ctypes.data_as(_l.i32p), float(input_scale),
                                 float(output_scale))
        _l.check(self.L.c8_set_embedded_model(self.h, C.byref(d)))

    @property
    def num_embedded_params(self):
        return self.L.c8_num_embedded_params(self.h)

    @property
    def num_grad_params(self):
        """Length of the gradient: the active parameters, then the network weights."""
        return self.L.c8_num_grad_params(self.h)

    def set_embedded_params(self, theta):
        """Network weights in the reference's order (a `nn_params.in` file read with np.loadtxt)."""
        t = np.ascontiguousarray(theta, dtype=np.float64).ravel()
        if t.size != self.num_embedded_params:
            raise ValueError("expected %d network weights, got %d" % (self.num_embedded_params, t.size))
        _l.check(self.L.c8_set_embedded_params(self.h, t.ctypes.data_as(_l.dp)))

    def get_embedded_params(self):
        t = np.zeros(self.num_embedded_params)
        _l.check(self.L.c8_get_embedded_params(self.h, t.ctypes.data_as(_l.dp)))
        return t

    def set_scatter(self, mode):
        m = {"colored": _l.C8_SCATTER_COLORED, "atomic": _l.C8_SCATTER_ATOMIC, "gather": _l.C8_SCATTER_GATHER}[mode]
        _l.check(self.L.c8_set_scatter_mode(self.h, m))

    @property
    def scatter(self):
        return {_l.C8_SCATTER_COLORED: "colored", _l.C8_SCATTER_ATOMIC: "atomic", _l.C8_SCATTER_GATHER: "gather"}[self.L.c8_get_scatter_mode(self.h)]

    def set_krylov_preconditioner(self, kind, sweeps=1):
        """Preconditioner of the device solves on this assembler: "jacobi" (node-block Jacobi, the default), "sgs"
        (`sweeps` symmetric multicolour node-block Gauss-Seidel sweeps) or "two_level" (a coarse correction with the
        rigid-body modes of node aggregates, then `sweeps` of those sweeps; one part only) or "multilevel" (the same
        construction repeated on the coarse matrix, `sweeps` per level, set_krylov_multilevel; one part only) or
        "two_level_parts" (the two-level kind over the parts of a multi-part mesh: part-local aggregates, one dense coarse
        problem over all parts replicated on every rank; "two_level" itself without a halo) or "multilevel_parts" (the
        multilevel kind over parts: the distributed level 0 of "two_level_parts" over block-sparse levels replicated on every
        rank, no cap on the mesh, set_krylov_multilevel; "multilevel" itself without a halo); c8_krylov_set_preconditioner."""
        kinds = {"jacobi": _l.C8_PRECOND_BLOCK_JACOBI, "sgs": _l.C8_PRECOND_BLOCK_SGS, "two_level": _l.C8_PRECOND_TWO_LEVEL,
                 "multilevel": _l.C8_PRECOND_MULTILEVEL, "two_level_parts": _l.C8_PRECOND_TWO_LEVEL_PARTS,
                 "multilevel_parts": _l.C8_PRECOND_MULTILEVEL_PARTS}
        if kind not in kinds:
            raise ValueError("preconditioner must be 'jacobi', 'sgs', 'two_level', 'multilevel', 'two_level_parts' or 'multilevel_parts', not %r" % (kind,))
        _l.check(self.L.c8_krylov_set_preconditioner(self.h, kinds[kind], int(sweeps)))

    @property
    def krylov_preconditioner(self):
        return {_l.C8_PRECOND_BLOCK_JACOBI: "jacobi", _l.C8_PRECOND_BLOCK_SGS: "sgs", _l.C8_PRECOND_TWO_LEVEL: "two_level",
                _l.C8_PRECOND_MULTILEVEL: "multilevel", _l.C8_PRECOND_TWO_LEVEL_PARTS: "two_level_parts",
                _l.C8_PRECOND_MULTILEVEL_PARTS: "multilevel_parts"}[_l.check(self.L.c8_krylov_get_preconditioner(self.h))]

    def set_krylov_multilevel(self, coarse_max=None, max_levels=None):
        """Settings of the "multilevel" and "multilevel_parts" preconditioners: another level is built while the coarsest one has more than
        `coarse_max` unknowns and fewer than `max_levels` levels exist (the system counts as one); None: the library's
        default.  The levels are rebuilt at the next solve; c8_krylov_set_multilevel."""
        _l.check(self.L.c8_krylov_set_multilevel(self.h, int(coarse_max or 0), int(max_levels or 0)))

    def set_assign_mode(self, on):
        """scatter='gather': Jacobian assemblies assign A and b (zero_all + assembly in one call) instead of adding"""
        _l.check(self.L.c8_set_assign_mode(self.h, int(bool(on))))

    def set_gather_early_nodes(self, node_begin, node_end):
        """scatter='gather' in two parts: Jacobian assemblies sum the rows of nodes [node_begin, node_end) only (the
        ghost rows of a mesh part); gather_finish() sums the rest, e.g. while those rows are being exchanged."""
        _l.check(self.L.c8_set_gather_early_nodes(self.h, int(node_begin), int(node_end)))

    def gather_finish(self):
        return self._rc(self.L.c8_gather_finish(self.h))

    def set_shape_cache(self, on):
        """cached shape tables of the hex8 wave kernels (default on; 1.7 KB per element)"""
        _l.check(self.L.c8_set_shape_cache(self.h, int(bool(on))))

    def set_stage_chunk(self, min_chunk):
        """scatter='gather': smallest chunk of elements staged at a time (default 8192)"""
        _l.check(self.L.c8_set_stage_chunk(self.h, int(min_chunk)))

    def set_stage_overlap(self, on):
        """scatter='gather' in several chunks: the row sums of a chunk beside the assembly of the next one (second stream)"""
        _l.check(self.L.c8_set_stage_overlap(self.h, int(bool(on))))

    def set_kernel(self, variant):
        """'auto' | 'slot' (one lane group per element) | 'wave' (one wavefront per hex8 element) | 'wave_ad' (the same with the
        iterated, automatically differentiated local solve also where a model has a closed form)"""
        v = {"auto": _l.C8_KERNEL_AUTO, "slot": _l.C8_KERNEL_SLOT, "wave": _l.C8_KERNEL_WAVE, "wave_ad": _l.C8_KERNEL_WAVE_AD, "node": _l.C8_KERNEL_NODE}[variant]
        _l.check(self.L.c8_set_kernel_variant(self.h, v))
        self.kernel = variant

    def set_async(self, flag):
        _l.check(self.L.c8_set_async(self.h, int(flag)))

    def use_current_stream(self):
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        _l.check(self.L.c8_set_stream(self.h, C.c_void_p(s)))

    def status(self):
        rc = self.L.c8_status(self.h)
        if rc < -1:
            _l.check(rc)
        return rc

    # ---- the hot path --------------------------------------------------------------------------
    @staticmethod
    def _state(u, p, u_prev, p_prev, xi_prev, xi):
        for t in (u, p, u_prev, p_prev, xi_prev, xi):
            assert t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch.float64"
        s = _l.State()
        s.x[0], s.x[1] = u.data_ptr(), p.data_ptr()
        s.x_prev[0], s.x_prev[1] = u_prev.data_ptr(), p_prev.data_ptr()
        s.xi_prev, s.xi = xi_prev.data_ptr(), xi.data_ptr()
        return s

    def _rc(self, rc):
        if rc < -1:
            _l.check(rc)
        return rc

    def forward_jacobian(self, u, p, u_prev, p_prev, xi_prev, xi, ls):
        """eval_forward_jacobian: returns 0, or -1 if a local Newton solve failed."""
        st, sy = self._state(u, p, u_prev, p_prev, xi_prev, xi), ls.c_struct()
        return self._rc(self.L.c8_assemble_forward_jacobian(self.h, C.byref(st), C.byref(sy)))

    def forward_jacobian_subset(self, u, p, u_prev, p_prev, xi_prev, xi, ls, elems):
        """eval_forward_jacobian over the elements listed in `elems` (int32 device tensor), atomic adds."""
        st, sy = self._state(u, p, u_prev, p_prev, xi_prev, xi), ls.c_struct()
        return self._rc(self.L.c8_assemble_forward_jacobian_subset(self.h, C.byref(st), C.byref(sy),
                                                                    C.c_void_p(elems.data_ptr()), int(elems.numel())))

    def global_residual(self, u, p, u_prev, p_prev, xi_prev, xi, ls):
        st, sy = self._state(u, p, u_prev, p_prev, xi_prev, xi), ls.c_struct()
        return self._rc(self.L.c8_assemble_residual(self.h, C.byref(st), C.byref(sy)))

    def adjoint_jacobian(self, u, p, u_prev, p_prev, xi_prev, xi, g, f, ls):
        st, sy = self._state(u, p, u_prev, p_prev, xi_prev, xi), ls.c_struct()
        return self._rc(self.L.c8_assemble_adjoint_jacobian(self.h, C.byref(st), C.c_void_p(g.data_ptr()),
                                                            C.c_void_p(f.data_ptr()), C.byref(sy)))

    def solve_adjoint_local(self, u, p, u_prev, p_prev, xi_prev, xi, z_u, z_p, phi, g, f):
        st = self._state(u, p, u_prev, p_prev, xi_prev, xi)
        z = (C.c_void_p * 2)(z_u.data_ptr(), z_p.data_ptr())
        return self._rc(self.L.c8_solve_adjoint_local(self.h, C.byref(st), z, C.c_void_p(phi.data_ptr()),
                                                      C.c_void_p(g.data_ptr()), C.c_void_p(f.data_ptr())))

    def qoi_gradient(self, u, p, u_prev, p_prev, xi_prev, xi, z_u, z_p, phi, grad):
        st = self._state(u, p, u_prev, p_prev, xi_prev, xi)
        z = (C.c_void_p * 2)(z_u.data_ptr(), z_p.data_ptr())
        return self._rc(self.L.c8_param_gradient(self.h, C.byref(st), z, C.c_void_p(phi.data_ptr()),
                                                 C.c_void_p(grad.data_ptr())))

    def cauchy(self, u, p, u_prev, p_prev, xi_prev, xi, out=None):
        """eval_cauchy: the Cauchy stress of the local model at every local-state point, from the stored state:
        [nelems, npts, 3, 3] float64 on the device (entries outside the ndims x ndims block are 0).  `out`, if given, is
        overwritten and returned."""
        torch = self.torch
        if out is None:
            out = torch.empty(self.nelems, self.npts, 3, 3, dtype=torch.float64, device=self.device)
        assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float64 and out.numel() == self.nelems * self.npts * 9
        st = self._state(u, p, u_prev, p_prev, xi_prev, xi)
        self._rc(self.L.c8_eval_cauchy(self.h, C.byref(st), C.c_void_p(out.data_ptr())))
        return out

    def _point_field(self, t, what):
        torch = self.torch
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64, what
        return t

    def spr_recover(self, ip_field, out=None):
        """spr_recovery (cspr.cpp): a point field [nelems, npts, ...] brought to the nodes [nnodes, ...] by superconvergent
        patch recovery (the trailing dimensions, at most 16 entries together, are the components).  `out`, if given, is
        overwritten and returned."""
        torch = self.torch
        self._point_field(ip_field, "ip_field")
        assert ip_field.dim() >= 2 and tuple(ip_field.shape[:2]) == (self.nelems, self.npts), tuple(ip_field.shape)
        comp = tuple(ip_field.shape[2:])
        ncomp = int(np.prod(comp)) if comp else 1
        if out is None:
            out = torch.empty((self.nnodes,) + comp, dtype=torch.float64, device=self.device)
        self._point_field(out, "out")
        assert out.numel() == self.nnodes * ncomp
        self._rc(self.L.c8_spr_recover(self.h, ncomp, C.c_void_p(ip_field.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def interpolate_to_points(self, nodal, out=None):
        """interpolate_to_cell_center at the local-state points: a nodal field [nnodes, ...] evaluated by the element's
        shape values, [nelems, npts, ...].  `out`, if given, is overwritten and returned."""
        torch = self.torch
        self._point_field(nodal, "nodal")
        assert nodal.dim() >= 1 and nodal.shape[0] == self.nnodes, tuple(nodal.shape)
        comp = tuple(nodal.shape[1:])
        ncomp = int(np.prod(comp)) if comp else 1
        if out is None:
            out = torch.empty((self.nelems, self.npts) + comp, dtype=torch.float64, device=self.device)
        self._point_field(out, "out")
        assert out.numel() == self.nelems * self.npts * ncomp
        self._rc(self.L.c8_interpolate_to_points(self.h, ncomp, C.c_void_p(nodal.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def spr_patches(self):
        """The recovery tables of this mesh as host arrays (copies): dict of patch_ptr [nnodes + 1], patch_elems, g
        [nnodes, ndims + 1], h [nnodes], stages [nnodes] and setup (ms device, ms host, ms upload, flagged nodes)."""
        kinds = (("patch_ptr", np.int64), ("patch_elems", np.int32), ("g", np.float64), ("h", np.float64),
                 ("stages", np.int32), ("setup", np.float64))
        out = {}
        for which, (name, dt) in enumerate(kinds):
            n, data = C.c_int64(), C.c_void_p()
            _l.check(self.L.c8_spr_table(self.h, which, C.byref(n), C.byref(data)))
            a = np.empty(n.value, dtype=dt)
            if n.value:
                C.memmove(a.ctypes.data, data, a.nbytes)
            out[name] = a
        out["g"] = out["g"].reshape(self.nnodes, self.ndims + 1)
        return out

    def error_contributions(self, u, p, u_prev, p_prev, xi_prev, xi, z_u, z_p, phi, E_R=None, E_C=None):
        """eval_error_contributions: (E_R, E_C), [nelems] float64 on the device: E_R[e] += z_e . R_e, E_C[e] += sum_pt phi_pt .
        C_pt at the stored state.  Allocated as zeros when not given, accumulated into when given."""
        torch = self.torch
        if E_R is None:
            E_R = torch.zeros(self.nelems, dtype=torch.float64, device=self.device)
        if E_C is None:
            E_C = torch.zeros(self.nelems, dtype=torch.float64, device=self.device)
        for t in (z_u, z_p, phi, E_R, E_C):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64
        assert E_R.numel() == self.nelems and E_C.numel() == self.nelems and phi.numel() == self.nelems * self.npts * self.nloc
        st = self._state(u, p, u_prev, p_prev, xi_prev, xi)
        z = (C.c_void_p * 2)(z_u.data_ptr(), z_p.data_ptr())
        self._rc(self.L.c8_eval_error_contributions(self.h, C.byref(st), z, C.c_void_p(phi.data_ptr()),
                                                    C.c_void_p(E_R.data_ptr()), C.c_void_p(E_C.data_ptr())))
        return E_R, E_C

    def _exact(self, fn, state, fine, z_u, z_p, phi, E_R, E_C):
        torch = self.torch
        if E_R is None:
            E_R = torch.zeros(self.nelems, dtype=torch.float64, device=self.device)
        if E_C is None:
            E_C = torch.zeros(self.nelems, dtype=torch.float64, device=self.device)
        for t in (z_u, z_p, phi, E_R, E_C):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float64
        assert E_R.numel() == self.nelems and E_C.numel() == self.nelems and phi.numel() == self.nelems * self.npts * self.nloc
        st, sf = self._state(*state), self._state(*fine)
        z = (C.c_void_p * 2)(z_u.data_ptr(), z_p.data_ptr())
        self._rc(fn(self.h, C.byref(st), C.byref(sf), z, C.c_void_p(phi.data_ptr()), C.c_void_p(E_R.data_ptr()),
                    C.c_void_p(E_C.data_ptr())))
        return E_R, E_C

    def exact_errors(self, state, fine, z_u, z_p, phi, E_R=None, E_C=None):
        """eval_exact_errors: (E_R, E_C), [nelems] float64 on the device, the derivative of the error contributions along
        fine - state:  E_R[e] += -z_e . (dR/dx dx + dR/dxi dxi),  E_C[e] += -sum_pt phi_pt . (dC/dx dx + dC/dxi dxi + dC/dx_prev
        dx_prev + dC/dxi_prev dxi_prev).  `state` and `fine` are (u, p, u_prev, p_prev, xi_prev, xi) device tensors; nothing
        of `fine` is written.  Outputs allocated as zeros when not given, accumulated into when given."""
        return self._exact(self.L.c8_eval_exact_errors, state, fine, z_u, z_p, phi, E_R, E_C)

    def linearization_errors(self, state, fine, z_u, z_p, phi, E_R=None, E_C=None):
        """eval_linearization_errors, per element: (E_lin_R, E_lin_C) = what exact_errors adds minus what error_contributions
        adds at `state`.  Arguments as exact_errors."""
        return self._exact(self.L.c8_eval_linearization_errors, state, fine, z_u, z_p, phi, E_R, E_C)

    # ---- virtual fields method (one-residual systems; calibr8_amd.vfm.VFMProblem drives these) ----------------------
    def vfm_set_virtual_field(self, w):
        """nodal virtual field [nnodes * ndims] (device tensor, kept by reference)"""
        self._vfm_w = w
        _l.check(self.L.c8_vfm_set_virtual_field(self.h, C.c_void_p(w.data_ptr())))

    def vfm_internal_power(self, u, p, u_prev, p_prev, xi_prev, xi, ivw, b=None):
        """eval_measured_residual: local solve with the measured u, u_prev into xi; ivw (device, one double) += w^T R;
        b (device [nnodes * ndims] or None) += R.  Returns 0, or -1 if a local solve failed."""
        st = self._state(u, p, u_prev, p_prev, xi_prev, xi)
        return self._rc(self.L.c8_vfm_internal_power(self.h, C.byref(st), None if b is None else C.c_void_p(b.data_ptr()),
                                                     C.c_void_p(ivw.data_ptr())))

    def vfm_forward_sens(self, u, p, u_prev, p_prev, xi_prev, xi, S_prev, S, ivw, divw):
        """eval_measured_residual_and_grad: as vfm_internal_power, S = local sensitivities [elems][pts][nloc][n_active]
        from S_prev (None = 0), divw [n_active] += d(w^T R)/dp.  Without active parameters S may be None."""
        st = self._state(u, p, u_prev, p_prev, xi_prev, xi)
        return self._rc(self.L.c8_vfm_forward_sens(self.h, C.byref(st), None if S_prev is None else C.c_void_p(S_prev.data_ptr()),
                                                   None if S is None else C.c_void_p(S.data_ptr()), C.c_void_p(ivw.data_ptr()),
                                                   C.c_void_p(divw.data_ptr())))

    def vfm_adjoint_step(self, u, p, u_prev, p_prev, xi_prev, xi, c, h, grad):
        """eval_vfm_adjoint_gradient at the stored state: h [elems][pts][nloc] updated in place, grad [n_active] +="""
        st = self._state(u, p, u_prev, p_prev, xi_prev, xi)
        return self._rc(self.L.c8_vfm_adjoint_step(self.h, C.byref(st), float(c), C.c_void_p(h.data_ptr()),
                                                   C.c_void_p(grad.data_ptr())))

    # ---- next to the hot path: boundary conditions on the device system, y = A x ----------------------
    def apply_dirichlet(self, dbcs, x_u, x_p, ls, is_adjoint=False):
        """dbcs: list of (resid, eq, nodes int32 device tensor, values float64 device tensor)."""
        d = (_l.Dbc * max(1, len(dbcs)))()
        for k, (resid, eq, nodes, vals) in enumerate(dbcs):
            d[k] = _l.Dbc(resid, eq, nodes.numel(), nodes.data_ptr(), vals.data_ptr())
        x = (C.c_void_p * 2)(x_u.data_ptr(), x_p.data_ptr())
        sy = ls.c_struct()
        return self._rc(self.L.c8_apply_dirichlet(self.h, len(dbcs), d, x, C.byref(sy), int(is_adjoint)))

    def apply_traction(self, tbcs, ls):
        """tbcs: list of (resid, faces int32 device tensor [n][3|4], traction float64 device tensor [n][pts][3])."""
        t = (_l.Tbc * max(1, len(tbcs)))()
        for k, (resid, faces, tr) in enumerate(tbcs):
            t[k] = _l.Tbc(resid, faces.shape[0], faces.shape[1], faces.data_ptr(), tr.data_ptr())
        sy = ls.c_struct()
        return self._rc(self.L.c8_apply_traction(self.h, len(tbcs), t, C.byref(sy)))

    def apply_A(self, ls, x_u, x_p, y_u, y_p):
        x = (C.c_void_p * 2)(x_u.data_ptr(), x_p.data_ptr())
        y = (C.c_void_p * 2)(y_u.data_ptr(), y_p.data_ptr())
        sy = ls.c_struct()
        return self._rc(self.L.c8_apply_A(self.h, C.byref(sy), x, y))

    # ---- objective ----
    def set_qoi_avg_disp(self):
        _l.check(self.L.c8_set_qoi_avg_disp(self.h))
        self.objective = ("avg_disp",)

    def set_qoi_calibration(self, faces, weights=(1.0, 1.0, 1.0), balance=1.0, coord_idx=1, coord_value=0.0,
                            coord_tol=1e-8, comp=1, dt_over_T=1.0):
        """Calibration objective (calibration.cpp): faces = node ids of the displacement side set [n][3|4] (host),
        load plane = nodes with |x[coord_idx] - coord_value| < coord_tol, reaction component comp."""
        f = np.ascontiguousarray(faces if faces is not None and len(faces) else np.zeros((0, 1)), dtype=np.int32)
        if f.ndim == 1:  # tri3 meshes: element ids of the displacement term (none = every element)
            f = f.reshape(-1, 1)
        d = _l.CalibrationDesc()
        d.num_faces, d.nodes_per_face, d.faces = f.shape[0], f.shape[1], f.ctypes.data
        for k in range(3):
            d.weights[k] = float(weights[k])
        d.balance_factor, d.coord_idx, d.coord_value, d.coord_tol = float(balance), int(coord_idx), float(coord_value), float(coord_tol)
        d.reaction_comp, d.dt_over_total_time = int(comp), float(dt_over_T)
        _l.check(self.L.c8_set_qoi_calibration(self.h, C.byref(d)))
        self.objective = ("calibration", f.tobytes(), f.shape, tuple(float(w) for w in weights), float(balance), int(coord_idx),
                          float(coord_value), float(coord_tol), int(comp), float(dt_over_T))

    def set_qoi_subdomain(self, kind, elem_set, index=0):
        """Subdomain objective over the elements of one element set (c8_set_qoi_subdomain): kind = "avg_stress" (the norm
        of the deviatoric Cauchy stress), "avg_local_var" (local dof `index`, a flat position in a point's local state or a
        name that local_dof() knows) or "disp_comp" (displacement component `index`), or the C8_QOI_* value.  Plain
        integrals, not divided by the volume."""
        kind = _l.C8_QOI_KINDS[kind] if isinstance(kind, str) else int(kind)
        if isinstance(index, str):
            index = local_dof(self.local_type, self.nloc, index)
        d = _l.SubdomainQoiDesc(kind, int(elem_set), int(index))
        _l.check(self.L.c8_set_qoi_subdomain(self.h, C.byref(d)))
        self.objective = ("subdomain", kind, int(elem_set), int(index) if kind != _l.C8_QOI_AVG_STRESS else 0)

    def set_qoi_reaction(self, coord_idx=1, coord_value=0.0, coord_tol=1e-8, comp=1):
        """Reaction objective (reaction.cpp without torque): the internal force component `comp` summed over the nodes with
        |x[coord_idx] - coord_value| < coord_tol.  On a multi-part mesh call set_allreduce first."""
        d = _l.ReactionDesc(int(coord_idx), float(coord_value), float(coord_tol), int(comp))
        _l.check(self.L.c8_set_qoi_reaction(self.h, C.byref(d)))
        self.objective = ("reaction", int(coord_idx), float(coord_value), float(coord_tol), int(comp))

    def set_allreduce(self, dist, num_parts):
        """Multi-part objective sums: `dist` = an initialised torch.distributed module (SUM all-reduce of host doubles)."""
        import torch

        def cb(_user, vals, n):
            t = torch.from_numpy(np.ctypeslib.as_array(vals, shape=(n,)))
            if dist.get_backend() == "nccl":
                d = t.to(self.device)
                dist.all_reduce(d, op=dist.ReduceOp.SUM)
                t.copy_(d.cpu())
            else:
                dist.all_reduce(t, op=dist.ReduceOp.SUM)

        self._allreduce_cb = _l.ALLREDUCE_FN(cb)  # keep the callback alive
        _l.check(self.L.c8_set_allreduce(self.h, self._allreduce_cb, None, int(num_parts)))

    def set_measured(self, u_meas, load_meas):
        """measured nodal displacements of the step (device tensor, kept by reference) and measured load"""
        self._u_meas = u_meas
        _l.check(self.L.c8_set_measured(self.h, C.c_void_p(u_meas.data_ptr()), float(load_meas)))

    def qoi_preprocess(self, u, p, u_prev, p_prev, xi_prev, xi):
        """preprocess_qoi: (side-set area, total load, load mismatch)"""
        st = self._state(u, p, u_prev, p_prev, xi_prev, xi)
        out = (C.c_double * 3)()
        _l.check(self.L.c8_qoi_preprocess(self.h, C.byref(st), out))
        return tuple(out)

    def eval_qoi(self, u, p, J, xi_prev=None, xi=None, u_prev=None, p_prev=None):
        """eval_qoi: J (1-element device tensor) += QoI value.  The local state is only needed by QoIs
        that read it ("average displacement" does not)."""
        s = _l.State()
        s.x[0], s.x[1] = u.data_ptr(), p.data_ptr()
        s.x_prev[0], s.x_prev[1] = (u_prev if u_prev is not None else u).data_ptr(), (p_prev if p_prev is not None else p).data_ptr()
        s.xi_prev = xi_prev.data_ptr() if xi_prev is not None else None
        s.xi = xi.data_ptr() if xi is not None else None
        return self._rc(self.L.c8_eval_qoi(self.h, C.byref(s), C.c_void_p(J.data_ptr())))
