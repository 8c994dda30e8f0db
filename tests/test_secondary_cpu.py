"""Secondary-potential formulation, the parts that need no GPU: the host copy of the element kernel's arithmetic
(remo_host_secondary_element) against the numpy restatement of tests/_secondary.py, the restatement itself against the CPU oracle's
primary solve and against the recorded fine-mesh values of the two-half-spaces case, and the keyword checks of the Python layer."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _secondary as S            # noqa: E402
from conftest import SIGMA3       # noqa: E402

R = 50.0
EVAL_Z = [0.4, 6.4, 2.0, 2.5, -0.3, 1.2]


def host_element(dim, X, sigma, sigma0, radius, src, n):
    """remo_host_secondary_element; sigma: a scalar or a symmetric dim x dim tensor."""
    from remo3d_amd import _lib
    from remo3d_amd._lib import ptr
    L = _lib.load()
    X = np.ascontiguousarray(X, dtype=float)
    src = np.ascontiguousarray(src, dtype=float)
    f = np.full(10 if dim == 2 else 20, np.nan)
    if np.ndim(sigma) == 0:
        rc = L.remo_host_secondary_element(dim, ptr(X, C.c_double), None, float(sigma), sigma0, radius, ptr(src, C.c_double), n, ptr(f, C.c_double))
    else:
        tri = np.ascontiguousarray(np.asarray(sigma, dtype=float)[np.triu_indices(dim)])
        rc = L.remo_host_secondary_element(dim, ptr(X, C.c_double), ptr(tri, C.c_double), 0.0, sigma0, radius, ptr(src, C.c_double), n, ptr(f, C.c_double))
    return rc, f


def _element(dim, src, diameters):
    """A fixed irregular element of diameter ~0.1, `diameters` of them away from src (2D: at r > 0)."""
    rng = np.random.default_rng(7 + dim)
    X = rng.random((dim + 1, dim)) * 0.1
    X -= X.mean(axis=0)
    away = np.full(dim, 1.0) / np.sqrt(dim) * 0.1 * diameters
    return X + np.asarray(src, dtype=float) + away


def _sigma(dim, tensor):
    if not tensor:
        return 0.1
    return np.diag([0.1, 0.2, 0.05][:dim]) + 0.01 * (np.ones((dim, dim)) - np.eye(dim))


SOURCES = {2: [(0.0, 0.0), (0.0, 3.0)], 3: [(0.0, 0.0, 0.0), (0.0, 0.0, 3.0), (0.05, 0.0, 0.1), (0.03, 0.02, 0.1)]}
CASES = [(dim, src, diam, tensor) for dim in (2, 3) for src in SOURCES[dim] for diam in (1, 10) for tensor in (False, True)]


@pytest.mark.parametrize("dim,src,diameters,tensor", CASES)
def test_host_element_matches_the_restatement(dim, src, diameters, tensor):
    """Element parity at the same n: origin, off-centre on the axis (image term), in 3D at x != 0 and at y > 0 (a source and its
    mirror image); elements one and ten diameters away; scalar and tensor conductivities.  1e-12 max|f_e|."""
    X, sig = _element(dim, src, diameters), _sigma(dim, tensor)
    D = (sig * np.eye(dim) if not tensor else sig) - 1.0 * np.eye(dim)
    for n in (3, 6):
        rc, f = host_element(dim, X, sig, 1.0, R, src, n)
        assert rc == 0
        ref = S.element_loads(dim, X[None], D[None], np.array([src], dtype=float), [1.0], 1.0, R, n)[0]
        assert np.max(np.abs(ref)) > 0
        assert np.max(np.abs(f - ref)) <= 1e-12 * np.max(np.abs(ref)), (n, f, ref)
    rc, f0 = host_element(dim, X, sig, 1.0, R, src, 0)       # 0: the default rule is one of the valid ones
    assert rc == 0 and np.all(np.isfinite(f0))


@pytest.mark.parametrize("dim", [2, 3])
def test_no_contrast_gives_exact_zeros_and_bad_arguments_are_refused(dim):
    X = _element(dim, SOURCES[dim][0], 1)
    for sig in (0.7, 0.7 * np.eye(dim)):
        rc, f = host_element(dim, X, sig, 0.7, R, SOURCES[dim][0], 6)
        assert rc == 0 and np.all(f == 0.0)
    assert host_element(dim, X, 0.1, 0.0, R, SOURCES[dim][0], 6)[0] == -1       # sigma0 must be positive
    assert host_element(dim, X, 0.1, 1.0, R, SOURCES[dim][0], 17)[0] == -1      # n_quad in [0, 16]
    assert host_element(dim, X, 0.1, 1.0, -1.0, SOURCES[dim][0], 6)[0] == -1
    assert host_element(dim, np.zeros((dim + 1, dim)), 0.1, 1.0, R, SOURCES[dim][0], 6)[0] == -3   # degenerate element


def test_rule_integrates_polynomials():
    """The restatement's conical rule: weights sum to 1, and - the Jacobian of the collapse is part of the integrand - monomials of
    the barycentrics are exact up to degree 2 n - 2 on the triangle and 2 n - 3 on the tetrahedron
    (int l_1^a l_2^b / |T| = 2 a! b! / (a + b + 2)!, int l_1^a l_2^b l_3^c / |T| = 6 a! b! c! / (a + b + c + 3)!)."""
    from math import factorial as fa
    for n in (2, 4, 6):
        l, w = S.conical_rule(2, n)
        assert abs(w.sum() - 1) < 1e-14 and np.all(l > 0)
        for a, b in ((1, 0), (0, 2), (n - 1, n - 1), (2 * n - 3, 1)):
            assert abs(np.sum(w * l[:, 1] ** a * l[:, 2] ** b) - 2 * fa(a) * fa(b) / fa(a + b + 2)) < 1e-14
        l, w = S.conical_rule(3, n)
        assert abs(w.sum() - 1) < 1e-14 and np.all(l > 0)
        for a, b, c in ((1, 0, 0), (0, 1, 0), (n - 2, n - 2, 1), (0, 0, 2 * n - 3)):
            assert abs(np.sum(w * l[:, 1] ** a * l[:, 2] ** b * l[:, 3] ** c) - 6 * fa(a) * fa(b) * fa(c) / fa(a + b + c + 3)) < 1e-14


@pytest.mark.parametrize("dim,bound", [(2, 1e-4), (3, 1e-3)])
def test_restatement_agrees_with_the_primary_solve(dim, bound, mesh2d, mesh3d):
    """On the suite's two-zone borehole meshes (sources in the mud, sigma0 = mud) primary and secondary differ by the primary's own
    mesh error: measured 3.2e-5 in 2D, 5.6e-4 in 3D."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle.fem_oracle import Oracle
    mesh = mesh2d if dim == 2 else mesh3d
    o = Oracle(mesh, SIGMA3, condense=False)

    def one(z):
        f, se, sf = o.rhs([z], [1.0])
        u, _, _, rc = o.pcg(f, 1e-12, 200000)
        assert rc == 0
        sec, _, _ = S.solve_secondary(mesh, o, SIGMA3, SIGMA3[0], S.axis_sources(dim, [z], [1.0]), EVAL_Z, R, 6)
        return np.max(np.abs(o.eval(u, EVAL_Z, (se, sf)) - sec) / np.abs(sec))
    with ThreadPoolExecutor(max_workers=2) as tp:      # the C calls release the GIL
        errs = list(tp.map(one, [0.0, 0.1]))
    print("primary vs secondary, dim", dim, errs)
    assert max(errs) <= bound, errs


def test_two_half_spaces_coarse_mesh_against_the_recorded_fine_values():
    """_two_half_spaces(4.0), 3.4 k triangles: the secondary solve is at least 5 x closer than the primary one to the recorded
    secondary values of scale 0.5 (measured 4.6e-3 against 3.2e-4: 14.6 x)."""
    zs, prim, sec = S.two_half_spaces(4.0)
    gz, gu = S.read_golden()
    assert np.array_equal(zs, gz)
    e_prim, e_sec = np.max(np.abs(prim - gu) / np.abs(gu)), np.max(np.abs(sec - gu) / np.abs(gu))
    print("two half spaces, scale 4: primary", e_prim, "secondary", e_sec)
    assert 5.0 * e_sec <= e_prim, (e_prim, e_sec)


# ---- the Python layer -------------------------------------------------------------------------------------------------------------
def test_job_struct_carries_the_new_members(mesh2d):
    """solver._batch_args with secondary=...: a job of the extended struct's size with the four members set; without it the job
    is the remo_job_t it was.  The header declares the extended struct with the job as its first member."""
    from remo3d_amd import _lib, solver
    src, ev = [([0.0], [1.0]), ([0.0, 0.1], [1.0, -1.0])], [EVAL_Z, EVAL_Z]
    args, _, tensor, eval_ptr, keep = solver._batch_args(None, mesh2d, SIGMA3, src, ev, secondary=dict(radius=R, sigma0=[1.0, 0.5], quad=5))
    j = args[2]
    J2 = _lib.RemoJobSecondary      # remo_job_secondary_t: the 232 bytes of a remo_job_t, then the four members
    assert isinstance(j, J2) and j.size == C.sizeof(J2) == 256 and C.sizeof(_lib.RemoJob) == 232
    assert J2.secondary.offset == 232 and J2.sec_quad.offset == 236 and J2.sec_radius.offset == 240 and J2.sec_sigma0.offset == 248
    assert all(getattr(J2, n).offset == getattr(_lib.RemoJob, n).offset for n, _ in _lib.RemoJob._fields_)
    assert (j.secondary, j.sec_quad, j.sec_radius) == (1, 5, R) and [j.sec_sigma0[0], j.sec_sigma0[1]] == [1.0, 0.5]
    assert j.n_rhs == 2 and not tensor and eval_ptr[-1] == 12
    j = solver._batch_args(None, mesh2d, SIGMA3, src, ev, secondary=dict(radius=R))[0][2]
    assert j.secondary == 1 and j.sec_quad == 0 and not j.sec_sigma0               # sigma0 left to the library: NULL
    j = solver._batch_args(None, mesh2d, SIGMA3, src, ev, job=True)[0][2]
    assert type(j) is _lib.RemoJob and j.size == 232        # without the keyword: the job as it was
    with pytest.raises(ValueError):
        solver._batch_args(None, mesh2d, SIGMA3, src, ev, secondary=dict(radius=R, sigma=1.0))
    header = open(os.path.join(ROOT, "include", "remo3d_hip.h")).read()
    ext = header[header.index("} remo_job_t;"):header.index("} remo_job_secondary_t;")]
    assert [ext.index(w) for w in ("remo_job_t job;", "int32_t secondary;", "int32_t sec_quad;", "sec_radius;", "*sec_sigma0;")] == sorted(
        ext.index(w) for w in ("remo_job_t job;", "int32_t secondary;", "int32_t sec_quad;", "sec_radius;", "*sec_sigma0;"))


def test_job_with_secondary_is_checked_without_a_device():
    """A NULL context is refused first; the host hook and the job entry are exported."""
    from remo3d_amd import _lib
    L = _lib.load()
    job = _lib.RemoJobSecondary(size=C.sizeof(_lib.RemoJobSecondary), secondary=1)
    assert L.remo_solve_job(None, None, C.byref(job), None, None) == -1
    assert "remo_host_secondary_element" in _lib.EXPORTS and L.remo_host_secondary_element


class _Context:
    """Stand-in solver context: records the keyword the sweep hands over, unit potentials."""
    calls = []

    def __init__(self, device):
        pass

    def close(self):
        pass

    def solve_batch(self, mesh, sigma, sources, evals, opts, secondary=None):
        _Context.calls.append(secondary)
        return [np.ones(len(e)) for e in evals], dict(pcg_steps=1), 0


def _model():
    from remo3d_amd.model import Model
    bm3 = os.path.join(ROOT, "tests", "golden", "examples", "Benchmark models", "Benchmark model 3")
    m = Model(["A0.4M6.0N", "A2.0M0.5N"])
    m.set_model_parameters(os.path.join(bm3, "Formation_BM3_00.txt"), os.path.join(bm3, "Borehole_BM3.txt"), dip=0)
    m.initialize_workers(cpu_workers=1, gpu_workers=1, context_factory=_Context)
    return m


def test_model_keyword_checks_and_hand_over():
    """formulation='secondary' with sensitivities, sensitivity_grid, field_grid, reuse, mixed precision or invert_logs: ValueError
    before any mesh is asked for; alone it reaches every batch's solve as secondary=dict(radius=domain_radius); 'primary' hands
    nothing over; model.formulation records the choice."""
    from remo3d_amd import inversion
    m = _model()
    seen = []

    def provider(dim, Rd, batch, fg, bh, dip):
        seen.append(dim)
        return types.SimpleNamespace(dim=dim, n_nodes=1000)
    depths = np.array([10.0, 10.5, 11.0])
    kw = dict(domain_radius=12.0, mesh_provider=provider, verbose=False)
    grid = dict(r=np.array([0.0, 0.5, 1.0]), z=np.array([9.0, 10.0, 11.0]))
    for bad in (dict(sensitivities=True), dict(sensitivity_grid=grid), dict(field_grid=grid), dict(reuse=inversion.SweepCache(warm=False)),
                dict(precision="mixed"), dict(solver_options=dict(precision="mixed"))):
        _Context.calls = []
        with pytest.raises(ValueError):
            m.simulate_logs(depths, formulation="secondary", **kw, **bad)
        assert not seen and not _Context.calls
    with pytest.raises(ValueError):
        m.invert_logs({t: np.ones(3) for t in m.tools}, depths, solver_kw=dict(formulation="secondary", **kw))
    assert not seen and not _Context.calls
    with pytest.raises(ValueError):
        m.simulate_logs(depths, formulation="tertiary", **kw)
    m.simulate_logs(depths, formulation="secondary", **kw)
    assert m.timing["failed_batches"] == 0, m.timing["first_error"]
    assert m.formulation == "secondary" and _Context.calls and all(c == dict(radius=12.0) for c in _Context.calls)
    _Context.calls = []
    m.simulate_logs(depths, **kw)
    assert m.formulation == "primary" and _Context.calls and all(c is None for c in _Context.calls)
