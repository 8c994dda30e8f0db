"""Pair derivatives (remo_job_pairs_t) without a GPU: the struct behind the job and its binding, the refusal of a job without a
context, and the element arithmetic the pair kernel runs (remo_host_pair_element: moments of every column once, then an inner
product per pair) against remo_host_sens_element, which forms the same exact polynomial integrals from the two vectors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA3 = [1.0, 0.1, 0.02]


def test_struct_sizes_and_offsets():
    from remo3d_amd import _lib
    P = _lib.RemoJobPairs
    assert C.sizeof(P) == 320
    assert [getattr(P, n).offset for n in ("n_pair", "pair_reserved", "pair_a", "pair_b", "dP_out")] == [288, 292, 296, 304, 312]
    assert (C.sizeof(_lib.RemoJobError), C.sizeof(_lib.RemoJobSecondary), C.sizeof(_lib.RemoJob)) == (288, 256, 232)
    assert P._fields_[:len(_lib.RemoJobError._fields_)] == _lib.RemoJobError._fields_


def test_header_declares_the_struct_and_the_hook():
    from remo3d_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "remo3d_hip.h")).read()
    body = header[header.rindex("typedef struct {", 0, header.index("} remo_job_pairs_t;")):header.index("} remo_job_pairs_t;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [re.sub(r"\s+", " ", d.strip()) for d in body[body.index("{") + 1:].split(";") if d.strip()]
    assert decls == ["remo_job_error_t err", "int32_t n_pair", "int32_t pair_reserved", "const int32_t *pair_a, *pair_b", "double *dP_out"]
    assert "#define REMO_ABI_VERSION 7" in header
    assert "remo_host_pair_element(" in header and "remo_host_pair_element" in _lib.EXPORTS and L.remo_host_pair_element
    debug = open(os.path.join(ROOT, "include", "remo3d_hip_debug.h")).read()
    assert "remo_debug_pairs_timing(" in debug and "remo_debug_pairs_timing" in _lib.DEBUG_EXPORTS and L.remo_debug_pairs_timing


def test_batch_args_make_a_pairs_job_only_when_asked(mesh2d):
    from remo3d_amd import _lib, solver
    src, ev = [([0.0], [1.0]), ([0.1], [1.0]), ([0.4], [1.0])], [[0.1, 0.4], [0.0, 0.4], [0.0, 0.1]]
    assert type(solver._batch_args(None, mesh2d, SIGMA3, src, ev)[0][2]) is _lib.RemoJob
    assert type(solver._batch_args(None, mesh2d, SIGMA3, src, ev, job=True)[0][2]) is _lib.RemoJob
    assert type(solver._batch_args(None, mesh2d, SIGMA3, src, ev, secondary=dict(radius=5.0))[0][2]) is _lib.RemoJobSecondary
    assert type(solver._batch_args(None, mesh2d, SIGMA3, src, ev, error=True)[0][2]) is _lib.RemoJobError
    args, _, _, _, keep = solver._batch_args(None, mesh2d, SIGMA3, src, ev, pairs=[(0, 0), (2, 1), (0, 2)])
    j = args[2]
    assert type(j) is _lib.RemoJobPairs and j.size == 320 and (j.n_pair, j.pair_reserved, j.err, j.secondary) == (3, 0, 0, 0)
    assert [j.pair_a[i] for i in range(3)] == [0, 2, 0] and [j.pair_b[i] for i in range(3)] == [0, 1, 2] and not j.dP_out
    assert j.n_rhs == 3 and j.src_p[3] == 0.1      # points, as remo_solve_job reads them
    j = solver._batch_args(None, mesh2d, SIGMA3, src, ev, pairs=[])[0][2]
    assert type(j) is _lib.RemoJobPairs and j.n_pair == 0


def test_pairs_job_is_refused_without_a_context():
    from remo3d_amd import _lib
    L = _lib.load()
    a = np.zeros(1, dtype=np.int32)
    out = np.zeros(3)
    job = _lib.RemoJobPairs(size=C.sizeof(_lib.RemoJobPairs), n_pair=1, pair_a=_lib.ptr(a, C.c_int32), pair_b=_lib.ptr(a, C.c_int32),
                            dP_out=_lib.ptr(out, C.c_double))
    assert L.remo_solve_job(None, None, C.byref(job), None, None) == -1
    h = C.c_void_p()
    assert L.remo_batch_create_job(None, None, C.byref(job), C.byref(h)) == -1 and not h


def _sens_element(dim, X, tensor, xl, xu):
    from remo3d_amd import _lib
    L = _lib.load()
    out = np.zeros((3 if dim == 2 else 6) if tensor else 1)
    rc = L.remo_host_sens_element(dim, _lib.ptr(np.ascontiguousarray(X), C.c_double), int(tensor), _lib.ptr(np.ascontiguousarray(xl), C.c_double),
                                  _lib.ptr(np.ascontiguousarray(xu), C.c_double), _lib.ptr(out, C.c_double))
    assert rc == 0
    return out


PAIRS = [(a, b) for a in range(5) for b in range(a, 5)] + [(3, 1), (4, 0)]


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("tensor", [False, True])
def test_pair_element_is_the_sens_element_of_the_two_columns(dim, tensor):
    """Five random element vectors, all 15 pairs a <= b and two reversed ones: the value from the staged moments against
    remo_host_sens_element(x_a, x_b), to 1e-13 of the largest value - two orders of summation of the same exact integrals.  Scalar
    tables: x^T K_e x >= 0 on the diagonal."""
    from remo3d_amd import solver
    rng = np.random.default_rng(10 * dim + int(tensor))
    n = 10 if dim == 2 else 20
    for _ in range(4):
        X = rng.standard_normal((dim + 1, dim)) + (np.array([3.0, 0.0]) if dim == 2 else 0.0)
        x = rng.standard_normal((5, n))
        x[1, rng.integers(0, n, 3)] = 0.0      # constrained dofs read 0
        got = solver.host_pair_element(dim, X, x, PAIRS, tensor=tensor)
        ref = np.array([_sens_element(dim, X, tensor, x[a], x[b]) for a, b in PAIRS])
        assert got.shape == ref.shape == (17, (3 if dim == 2 else 6) if tensor else 1)
        assert np.max(np.abs(got - ref)) <= 1e-13 * np.max(np.abs(ref))
        if not tensor:
            assert all(got[i, 0] >= 0.0 for i, (a, b) in enumerate(PAIRS) if a == b)
    # (a, b) and (b, a): the tables are symmetric
    assert np.max(np.abs(got[PAIRS.index((1, 3))] - got[PAIRS.index((3, 1))])) <= 1e-13 * np.max(np.abs(ref))


def test_pair_element_refuses_bad_arguments():
    from remo3d_amd import solver
    X = np.array([[1.0, 0.0], [2.0, 0.0], [1.0, 1.0]])
    x = np.ones((2, 10))
    with pytest.raises(solver.RemoError):
        solver.host_pair_element(2, X, x, [(0, 2)])
    with pytest.raises(solver.RemoError):
        solver.host_pair_element(2, np.zeros((3, 2)), x, [(0, 1)])      # degenerate
    assert solver.host_pair_element(2, X, x, []).shape == (0, 1)
