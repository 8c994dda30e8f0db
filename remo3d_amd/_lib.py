"""ctypes binding of libremo3d_hip.so (include/remo3d_hip.h).

The library is the product: there is no Python / CPU fallback.  If the shared object is missing
the import of this module raises, and if no MI355X is visible ``Context()`` raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# REMO_LIB: another build of the same library (tools/: the -DREMO_PROBES build, compile-time variants); the product loads its own
LIB_PATH = os.environ.get("REMO_LIB") or os.path.join(_HERE, "libremo3d_hip.so")
REMO_MAX_RHS = 8


class RemoMesh(C.Structure):
    _fields_ = [("dim", C.c_int32), ("n_nodes", C.c_int64), ("coords", C.POINTER(C.c_double)),
                ("n_elems", C.c_int64), ("conn", C.POINTER(C.c_int32)), ("mat", C.POINTER(C.c_int32)),
                ("n_bfacets", C.c_int64), ("bconn", C.POINTER(C.c_int32)), ("bdirichlet", C.POINTER(C.c_uint8))]


class RemoOpts(C.Structure):
    _fields_ = [("preconditioner", C.c_int32), ("condense", C.c_int32), ("maxsteps", C.c_int32),
                ("check_every", C.c_int32), ("rtol", C.c_double), ("time_kernels", C.c_int32),
                ("coarse_degree", C.c_int32), ("coarse_ratio", C.c_int32), ("precision", C.c_int32), ("inner_digits", C.c_int32),
                ("serialize_solves", C.c_int32), ("op", C.c_int32), ("coarse", C.c_int32), ("assemble", C.c_int32), ("quadrature", C.c_int32)]


class RemoStats(C.Structure):
    _fields_ = [("n_dof", C.c_int64), ("n_free", C.c_int64), ("nnz", C.c_int64), ("n_edges", C.c_int64),
                ("n_faces", C.c_int64), ("n_rhs", C.c_int32), ("max_iterations", C.c_int32),
                ("iterations", C.c_int32 * REMO_MAX_RHS), ("relres", C.c_double * REMO_MAX_RHS),
                ("ms_symbolic", C.c_double), ("ms_h2d", C.c_double), ("ms_assemble", C.c_double),
                ("ms_solve", C.c_double), ("ms_eval", C.c_double), ("ms_total", C.c_double),
                ("spmv_ms", C.c_double), ("spmv_launches", C.c_int64), ("spmv_bytes", C.c_double),
                ("pcg_steps", C.c_int64), ("spmv_ms_raw", C.c_double), ("event_overhead_ms", C.c_double),
                ("refinement_cycles", C.c_int64), ("op_used", C.c_int32), ("coarse_used", C.c_int32),
                ("assembled", C.c_int32), ("patch_rounds", C.c_int32)]

    def as_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if hasattr(v, "__len__") else v
        return d


class RemoJob(C.Structure):
    """remo_job_t: the description of one batch for remo_solve_job / remo_batch_create_job (points are full coordinates)."""
    _dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    _fields_ = [("size", C.c_uint32), ("tensor", C.c_int32), ("n_mat", C.c_int32), ("sigma", _dp),
                ("n_rhs", C.c_int32), ("src_ptr", _ip), ("src_p", _dp), ("src_I", _dp),
                ("eval_ptr", _ip), ("eval_p", _dp), ("u_out", _dp),
                ("n_fun", C.c_int32), ("fun_rhs", _ip), ("fun_ptr", _ip), ("fun_p", _dp), ("fun_w", _dp), ("J_out", _dp), ("dJ_out", _dp),
                ("n_group", C.c_int32), ("group", _ip), ("dJg_out", _dp),
                ("warm", C.c_void_p),
                ("n_pts", C.c_int32), ("pts", _dp), ("n_frhs", C.c_int32), ("field_rhs", _ip), ("u_f", _dp), ("grad_f", _dp), ("J_f", _dp),
                ("elem_f", _ip)]


class RemoJobSecondary(C.Structure):
    """remo_job_secondary_t: a remo_job_t with the four members of the secondary-potential formulation behind it (the job's members
    are repeated here flat: the same bytes as the header's nested form, and they can be set by name like a RemoJob's)."""
    _fields_ = RemoJob._fields_ + [("secondary", C.c_int32), ("sec_quad", C.c_int32), ("sec_radius", C.c_double),
                                   ("sec_sigma0", C.POINTER(C.c_double))]


class RemoJobError(C.Structure):
    """remo_job_error_t: a remo_job_secondary_t with the five members of the error estimates behind it (flat, like RemoJobSecondary)."""
    _fields_ = RemoJobSecondary._fields_ + [("err", C.c_int32), ("err_n_group", C.c_int32), ("err_group", C.POINTER(C.c_int32)),
                                            ("err_out", C.POINTER(C.c_double)), ("errg_out", C.POINTER(C.c_double))]


class RemoJobPairs(C.Structure):
    """remo_job_pairs_t: a remo_job_error_t with the five members of the pair derivatives behind it (flat, like RemoJobSecondary)."""
    _fields_ = RemoJobError._fields_ + [("n_pair", C.c_int32), ("pair_reserved", C.c_int32), ("pair_a", C.POINTER(C.c_int32)),
                                        ("pair_b", C.POINTER(C.c_int32)), ("dP_out", C.POINTER(C.c_double))]


class RemoJobPairGroups(C.Structure):
    """remo_job_pair_groups_t: a remo_job_pairs_t with the four members of the pair derivatives per group of elements behind it (flat,
    like RemoJobSecondary)."""
    _fields_ = RemoJobPairs._fields_ + [("pair_n_group", C.c_int32), ("pair_group_reserved", C.c_int32), ("pair_group", C.POINTER(C.c_int32)),
                                        ("dPg_out", C.POINTER(C.c_double))]


# include/remo3d_hip.h: the drop-in boundary + inspection hooks of the parity tests
EXPORTS = ["remo_abi_version", "remo_opts_default", "remo_ctx_create", "remo_ctx_destroy", "remo_last_error",
           "remo_solve_batch", "remo_solve_batch_tensor", "remo_solve_batch_sens", "remo_solve_batch_sens_tensor", "remo_solve_batch_sens_groups", "remo_solve_batch_sens_groups_tensor",
           "remo_solve_batch_field", "remo_solve_batch_field_tensor", "remo_batch_field", "remo_host_field_element",
           "remo_warm_create", "remo_warm_destroy", "remo_warm_clear", "remo_warm_info", "remo_solve_batch_sens_warm", "remo_solve_batch_sens_warm_tensor", "remo_batch_create", "remo_batch_create_tensor", "remo_batch_run", "remo_batch_fetch", "remo_batch_destroy",
           "remo_batch_eval", "remo_batch_get_system", "remo_batch_get_vectors", "remo_batch_apply_coarse", "remo_batch_spmv",
           "remo_host_element_matrix", "remo_host_element_matrix_tensor", "remo_host_sens_element", "remo_host_factor_error", "remo_host_symbolic",
           "remo_solve_job", "remo_batch_create_job", "remo_host_point_shapes", "remo_host_secondary_element", "remo_host_error_facet", "remo_host_pair_element"]
# include/remo3d_hip_debug.h: probes and tuning knobs (tests, tools, bench.py's `box` record) - not part of the boundary
DEBUG_EXPORTS = ["remo_debug_stream", "remo_debug_clock", "remo_debug_device", "remo_debug_cache_gather", "remo_debug_xcc", "remo_debug_tune", "remo_debug_patch_phases", "remo_debug_patch_phases_p", "remo_debug_grid_barrier", "remo_debug_sens_timing", "remo_debug_sens_group_timing", "remo_debug_field_timing", "remo_debug_point_location", "remo_debug_secondary_timing", "remo_debug_direction_bytes", "remo_debug_pairs_timing", "remo_debug_pair_groups_timing",
                 "remo_debug_direction_forms", "remo_debug_vector_heads", "remo_debug_product", "remo_debug_row_ops"]

# The argument lists of the entries that take one (remo_solve_batch<kind>[_tensor], remo_batch_create[_tensor]) as members of
# RemoJob: ctx and mesh, JOB_HEAD, then the kind's members - for the solves followed by opts and stats.  load() derives the
# argtypes from this table and legacy_args() reads a call's arguments off a job, so a kind is spelled once.
JOB_HEAD = ["n_mat", "sigma", "n_rhs", "src_ptr", "src_p", "src_I", "eval_ptr", "eval_p"]
_SENS = ["u_out", "n_fun", "fun_rhs", "fun_ptr", "fun_p", "fun_w"]
LEGACY_MEMBERS = {"": ["u_out"],
                  "_sens": _SENS + ["J_out", "dJ_out"],
                  "_sens_warm": _SENS + ["J_out", "dJ_out", "warm"],
                  "_sens_groups": _SENS + ["n_group", "group", "J_out", "dJ_out", "dJg_out"],
                  "_field": ["u_out", "n_pts", "pts", "n_frhs", "field_rhs", "u_f", "grad_f", "J_f", "elem_f"]}


def legacy_args(job, kind=None):
    """The arguments behind (ctx, mesh) of remo_solve_batch<kind>[_tensor] - kind None: of remo_batch_create[_tensor] - read off a job."""
    return [getattr(job, name) for name in JOB_HEAD + (LEGACY_MEMBERS[kind] if kind is not None else [])]


_lib = None


def load():
    """Load libremo3d_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C remo3d_amd/csrc` "
                          "(or __graft_entry__.build()); remo3d_amd has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    dp, ip, i64p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    vp = C.c_void_p
    L.remo_abi_version.restype = C.c_int
    L.remo_opts_default.argtypes = [C.POINTER(RemoOpts)]
    L.remo_ctx_create.restype = vp
    L.remo_ctx_create.argtypes = [C.c_int]
    L.remo_ctx_destroy.argtypes = [vp]
    L.remo_last_error.restype = C.c_char_p
    L.remo_last_error.argtypes = [vp]
    member = dict(RemoJob._fields_)
    batch_args = [vp, C.POINTER(RemoMesh)] + [member[name] for name in JOB_HEAD]
    for kind, names in LEGACY_MEMBERS.items():
        for entry in (getattr(L, "remo_solve_batch" + kind), getattr(L, "remo_solve_batch" + kind + "_tensor")):
            entry.restype = C.c_int
            entry.argtypes = batch_args + [member[name] for name in names] + [C.POINTER(RemoOpts), C.POINTER(RemoStats)]
    L.remo_warm_create.restype = vp
    L.remo_warm_create.argtypes = [C.c_int]
    L.remo_warm_destroy.restype = None
    L.remo_warm_destroy.argtypes = [vp]
    L.remo_warm_clear.restype = None
    L.remo_warm_clear.argtypes = [vp]
    L.remo_warm_info.restype = C.c_int
    L.remo_warm_info.argtypes = [vp, i64p, ip, i64p, ip]
    L.remo_solve_job.restype = C.c_int
    L.remo_solve_job.argtypes = [vp, C.POINTER(RemoMesh), vp, C.POINTER(RemoOpts), C.POINTER(RemoStats)]     # the job: RemoJob, RemoJobSecondary, RemoJobError, RemoJobPairs or RemoJobPairGroups
    L.remo_batch_create_job.restype = C.c_int
    L.remo_batch_create_job.argtypes = [vp, C.POINTER(RemoMesh), vp, C.POINTER(vp)]
    L.remo_host_point_shapes.restype = C.c_int
    L.remo_host_point_shapes.argtypes = [C.c_int32, dp, dp, dp]
    L.remo_batch_field.restype = C.c_int
    L.remo_batch_field.argtypes = [vp, vp, C.c_int32, C.c_int32, dp, dp, dp, dp, ip]
    L.remo_host_field_element.restype = C.c_int
    L.remo_host_field_element.argtypes = [C.c_int32, dp, dp, C.c_double, dp, dp, dp]
    L.remo_debug_field_timing.restype = C.c_int
    L.remo_debug_field_timing.argtypes = [vp, dp]
    L.remo_debug_point_location.restype = C.c_int
    L.remo_debug_point_location.argtypes = [vp]
    L.remo_debug_direction_bytes.restype = C.c_int
    L.remo_debug_direction_bytes.argtypes = [vp]
    L.remo_host_secondary_element.restype = C.c_int
    L.remo_host_secondary_element.argtypes = [C.c_int32, dp, dp, C.c_double, C.c_double, C.c_double, dp, C.c_int32, dp]
    L.remo_host_error_facet.restype = C.c_int
    L.remo_host_error_facet.argtypes = [C.c_int32, C.c_int32, dp, dp, C.c_double, dp, dp, dp, C.c_double, dp, dp]
    L.remo_debug_secondary_timing.restype = C.c_int
    L.remo_debug_secondary_timing.argtypes = [vp, dp]
    L.remo_debug_sens_group_timing.restype = C.c_int
    L.remo_debug_sens_group_timing.argtypes = [vp, dp]
    L.remo_host_pair_element.restype = C.c_int
    L.remo_host_pair_element.argtypes = [C.c_int32, dp, C.c_int32, C.c_int32, dp, C.c_int32, ip, ip, dp]
    L.remo_debug_pairs_timing.restype = C.c_int
    L.remo_debug_pairs_timing.argtypes = [vp, dp]
    L.remo_debug_pair_groups_timing.restype = C.c_int
    L.remo_debug_pair_groups_timing.argtypes = [vp, dp]
    L.remo_host_sens_element.restype = C.c_int
    L.remo_host_sens_element.argtypes = [C.c_int32, dp, C.c_int32, dp, dp, dp]
    L.remo_debug_sens_timing.restype = C.c_int
    L.remo_debug_sens_timing.argtypes = [vp, dp]
    L.remo_batch_create.restype = C.c_int
    L.remo_batch_create.argtypes = batch_args + [C.POINTER(vp)]
    L.remo_batch_create_tensor.restype = C.c_int
    L.remo_batch_create_tensor.argtypes = batch_args + [C.POINTER(vp)]
    L.remo_batch_run.restype = C.c_int
    L.remo_batch_run.argtypes = [vp, vp, C.POINTER(RemoOpts), C.POINTER(RemoStats)]
    L.remo_batch_fetch.restype = C.c_int
    L.remo_batch_fetch.argtypes = [vp, vp, dp]
    L.remo_batch_destroy.argtypes = [vp, vp]
    L.remo_batch_eval.restype = C.c_int
    L.remo_batch_eval.argtypes = [vp, vp, C.c_int32, C.c_int32, dp, dp]
    L.remo_batch_get_system.restype = C.c_int
    L.remo_batch_get_system.argtypes = [vp, vp, ip, ip, dp, dp, ip]
    L.remo_batch_get_vectors.restype = C.c_int
    L.remo_batch_get_vectors.argtypes = [vp, vp, dp, dp, ip]
    L.remo_batch_apply_coarse.restype = C.c_int
    L.remo_batch_apply_coarse.argtypes = [vp, vp, C.c_int32, dp, dp, C.c_int32, i64p]
    L.remo_debug_patch_phases.restype = C.c_int
    L.remo_debug_patch_phases.argtypes = [vp, vp, C.c_int32, dp]
    L.remo_debug_patch_phases_p.restype = C.c_int
    L.remo_debug_patch_phases_p.argtypes = [vp, vp, C.c_int32, dp]
    L.remo_debug_grid_barrier.restype = C.c_int
    L.remo_debug_grid_barrier.argtypes = [vp, C.c_int32, C.c_int32, dp]
    L.remo_debug_xcc.restype = C.c_int
    L.remo_debug_xcc.argtypes = [vp, ip, C.c_int32]
    L.remo_debug_cache_gather.restype = C.c_int
    L.remo_debug_cache_gather.argtypes = [vp, C.c_int64, dp]
    L.remo_debug_device.restype = C.c_int
    L.remo_debug_device.argtypes = [vp, i64p]
    L.remo_debug_clock.restype = C.c_int
    L.remo_debug_clock.argtypes = [vp, dp]
    L.remo_debug_stream.restype = C.c_int
    L.remo_debug_stream.argtypes = [vp, C.c_int64, dp, dp]
    L.remo_batch_spmv.restype = C.c_int
    L.remo_batch_spmv.argtypes = [vp, vp, C.c_int32, dp, dp, C.c_int32, dp]
    L.remo_host_element_matrix.restype = C.c_int
    L.remo_host_element_matrix.argtypes = [C.c_int32, dp, C.c_double, dp]
    L.remo_host_element_matrix_tensor.restype = C.c_int
    L.remo_host_element_matrix_tensor.argtypes = [C.c_int32, dp, dp, dp]
    L.remo_host_factor_error.restype = C.c_double
    L.remo_host_symbolic.restype = C.c_int
    L.remo_host_symbolic.argtypes = [C.POINTER(RemoMesh), C.c_int32, i64p, ip, ip, ip]
    L.remo_debug_tune.restype = C.c_int
    L.remo_debug_tune.argtypes = [C.c_int32, C.c_int32]
    fp = C.POINTER(C.c_float)
    if hasattr(L, "remo_debug_direction_forms"):      # (REMO_LIB may name an older build, run beside this one for comparison)
        L.remo_debug_direction_forms.restype = C.c_int
        L.remo_debug_direction_forms.argtypes = [vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_double, dp, fp, dp, dp, dp, dp,
                                                 C.c_int32, dp, fp, fp, dp, dp]
        L.remo_debug_vector_heads.restype = C.c_int
        L.remo_debug_vector_heads.argtypes = [vp, C.c_int32, dp]
    if hasattr(L, "remo_debug_product"):
        L.remo_debug_product.restype = C.c_int
        L.remo_debug_product.argtypes = [vp, C.c_int32, C.c_int64, C.c_int64, ip, ip, dp, C.c_int64, ip, ip, dp, ip, ip, dp, ip]
    if hasattr(L, "remo_debug_row_ops"):
        L.remo_debug_row_ops.restype = C.c_int
        L.remo_debug_row_ops.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int32, ip, ip, dp, dp, C.c_double, dp, dp,
                                         C.c_int32, C.c_int32, vp, vp]
    _lib = L
    return L


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def mesh_struct(mesh):
    """RemoMesh view of a meshgen.Mesh-like object; returns (struct, keepalive)."""
    coords = np.ascontiguousarray(mesh.coords, dtype=np.float64)
    conn = np.ascontiguousarray(mesh.conn, dtype=np.int32)
    mat = np.ascontiguousarray(mesh.mat, dtype=np.int32)
    bconn = np.ascontiguousarray(mesh.bconn, dtype=np.int32).reshape(-1, mesh.dim)
    bdir = np.ascontiguousarray(mesh.bdirichlet, dtype=np.uint8)
    m = RemoMesh(int(mesh.dim), coords.shape[0], ptr(coords, C.c_double), conn.shape[0], ptr(conn, C.c_int32),
                 ptr(mat, C.c_int32), bconn.shape[0], ptr(bconn, C.c_int32), ptr(bdir, C.c_uint8))
    return m, (coords, conn, mat, bconn, bdir)
