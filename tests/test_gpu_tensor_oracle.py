"""Conductivity tensors on the GPU against the oracle's tensor assembly (orc_create_tensor), entry by entry.

The mirror of test_gpu_parity.py for remo_batch_create_tensor: the assembled CSR system and its Jacobi diagonal, the CSR and patch
operator products, the vertex-block-only assembly, whole solves with their true residual, the multigrid cycle, the 2D degree-4
quadrature and one Model sweep.  The tensors differ per material (tests/_anisotropy.general_tensors: all six entries nonzero,
one material exactly sigma I) or have the shape Model gives them (model_tensors: TI layers with their own Rv / Rh beside isotropic
mud and flushed zone, on a conforming dipping mesh), so a layout or sign error in any entry shows."""
import os

import numpy as np
import pytest

from _anisotropy import MODEL_BH, MODEL_FG, general_tensors, model_tensors
from conftest import SIGMA3

pytestmark = pytest.mark.gpu

SRC = [([0.0], [1.0]), ([0.1], [1.0]), ([-0.1, 0.1], [1.0, -1.0])]
EVAL = [[0.4, 6.4, -2.0], [2.1, 2.6], [0.5, 3.0, 0.0]]
BM3 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Benchmark models", "Benchmark model 3")

_CACHE = {}       # meshes, oracles and reference potentials, shared by the parametrisations


def _dip_mesh(dip, scale):
    from remo3d_amd import meshgen
    snap = sorted({z for e in EVAL for z in e} - {0.0, 0.1, -0.1})
    return meshgen.make_mesh_3d_conforming(50.0, MODEL_FG, MODEL_BH, np.deg2rad(dip), sources_z=[0.0, 0.1, -0.1], snap_z=snap, scale=scale)


def _case(which, mesh2d, mesh3d):
    """(mesh, tensors) of a case.  "2d" / "3d": the conftest meshes with general_tensors; "dip30" / "dip60": Model-shaped
    tensors on a conforming dipping mesh; "*_coarse": the same on a coarser size field, for the solves (their reference is a
    sparse direct solve of the oracle's system)."""
    if which not in _CACHE:
        from remo3d_amd.meshgen import make_mesh
        from conftest import _two_zone
        if which == "2d":
            _CACHE[which] = (mesh2d, general_tensors(2))
        elif which == "3d":
            _CACHE[which] = (mesh3d, general_tensors(3))
        elif which == "3d_coarse":
            _CACHE[which] = (make_mesh(3, 50.0, [0.0, 0.1, -0.1], scale=16.0, material_fn=_two_zone(3), seed=0), general_tensors(3))
        else:
            dip = int(which[3:5])
            _CACHE[which] = (_dip_mesh(dip, 8.0 if which.endswith("_coarse") else 4.0), model_tensors(dip))
    return _CACHE[which]


def _oracle(which, mesh2d, mesh3d, condense=True, quadrature="exact", scalar=False):
    key = ("oracle", which, condense, quadrature, scalar)
    if key not in _CACHE:
        from oracle.fem_oracle import Oracle
        mesh, S = _case(which, mesh2d, mesh3d)
        _CACHE[key] = Oracle(mesh, SIGMA3 if scalar else S, condense=condense, quadrature=quadrature)
    return _CACHE[key]


def _reference(which, mesh2d, mesh3d):
    """The oracle's potentials of SRC / EVAL: its system, sources and evaluation, solved by a sparse direct factorisation."""
    key = ("ref", which)
    if key not in _CACHE:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
        o = _oracle(which, mesh2d, mesh3d)
        rp, col, val = o.csr()
        lu = spla.splu(sp.csr_matrix((val, col, rp), shape=(o.nfree, o.nfree)).tocsc(), permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0,
                       options=dict(SymmetricMode=True))
        ref = []
        for (z, I), ez in zip(SRC, EVAL):
            f, se, sf = o.rhs(z, I)
            ref.append(o.eval(lu.solve(f), ez, (se, sf)))
        _CACHE[key] = ref
    return _CACHE[key]


def _oracle_diag(o):
    rp, col, val = o.csr()
    rows = np.repeat(np.arange(o.nfree), np.diff(rp))
    return val[col == rows]


# The inspection tests run a batch only to assemble it (a short, loose PCG): what they assert is the system, not the solve.


def _check_system(b, o, label):
    """rowptr / col / freeid identical, values 1e-12 of the largest entry, Jacobi diagonal 1e-12."""
    rowptr, col, val, dinv, freeid = b.system()
    rp, oc, ov = o.csr()
    assert b.stats["n_free"] == o.nfree and b.stats["nnz"] == o.nnz
    assert np.array_equal(rowptr, rp) and np.array_equal(col, oc)
    assert np.array_equal(freeid, o.freeid())
    err = np.max(np.abs(val - ov)) / np.max(np.abs(ov))
    derr = np.max(np.abs(dinv * _oracle_diag(o) - 1.0))
    print("%s: CSR values %.2e of the largest entry, Jacobi diagonal %.2e" % (label, err, derr))
    assert err <= 1e-12
    assert derr <= 1e-12
    return val


@pytest.mark.parametrize("which,condense", [("2d", True), ("2d", False), ("3d", True), ("dip30", True), ("dip60", True)])
def test_tensor_system_matches_oracle(which, condense, mesh2d, mesh3d, gpu_ctx):
    from remo3d_amd import solver
    mesh, S = _case(which, mesh2d, mesh3d)
    o = _oracle(which, mesh2d, mesh3d, condense=condense)
    b = gpu_ctx.batch(mesh, S, SRC[:1], EVAL[:1])
    try:
        assert b.run(solver.make_opts(preconditioner="local", condense=condense, rtol=1e-2, op="csr")) >= 0, gpu_ctx.last_error()
        _check_system(b, o, "%s condense=%s" % (which, condense))
    finally:
        b.close()


@pytest.mark.parametrize("which", ["2d", "3d", "dip30"])
def test_tensor_spmv_matches_oracle(which, mesh2d, mesh3d, gpu_ctx):
    """The CSR product of a tensor batch, k = 1, 3, 5, 8 columns, against the oracle's: 5e-12 of the largest entry."""
    from remo3d_amd import solver
    mesh, S = _case(which, mesh2d, mesh3d)
    o = _oracle(which, mesh2d, mesh3d)
    b = gpu_ctx.batch(mesh, S, SRC[:1], EVAL[:1])
    try:
        assert b.run(solver.make_opts(preconditioner="local", rtol=1e-2, op="csr")) >= 0
        worst = 0.0
        for k in (1, 3, 5, 8):
            x = np.random.default_rng(k).standard_normal((o.nfree, k))
            y, _ = b.spmv(x if k > 1 else x[:, 0])
            y = y.reshape(o.nfree, k)
            yr = np.stack([o.spmv(x[:, c]) for c in range(k)], 1)
            err = np.max(np.abs(y - yr)) / np.max(np.abs(yr))
            worst = max(worst, err)
            assert err <= 5e-12, k
        print("%s: CSR product %.2e of the largest entry" % (which, worst))
    finally:
        b.close()


def _rhs_block(k):
    zs = np.linspace(-0.1, 0.1, k)
    return [([float(z)], [1.0]) for z in zs], [[float(z) + 0.4, float(z) + 6.4] for z in zs]


@pytest.mark.parametrize("which", ["3d", "dip30"])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_tensor_patch_operator_is_the_assembled_matrix(which, k, mesh2d, mesh3d, gpu_ctx):
    """The patch operator (factorised reference tensors contracted with the tensor metric terms) == the CSR product == the oracle's,
    5e-12 of the largest entry; also with fewer columns than the batch was laid out for."""
    from remo3d_amd import solver
    mesh, S = _case(which, mesh2d, mesh3d)
    o = _oracle(which, mesh2d, mesh3d)
    src, ev = _rhs_block(k)
    b = gpu_ctx.batch(mesh, S, src, ev)
    try:
        worst = 0.0
        for kk in sorted({k, max(1, k - 1), 1}):
            x = np.random.default_rng(10 * k + kk).standard_normal((o.nfree, kk))
            xx = x if kk > 1 else x[:, 0]
            ys = {}
            for op in ("csr", "patch"):
                assert b.run(solver.make_opts(preconditioner="local", rtol=1e-2, op=op)) >= 0
                assert b.stats["op_used"] == (3 if op == "patch" else 0)
                ys[op], _ = b.spmv(xx)
            yr = np.stack([o.spmv(x[:, c]) for c in range(kk)], 1).reshape(ys["csr"].shape)
            scale = np.max(np.abs(yr))
            worst = max(worst, np.max(np.abs(ys["patch"] - yr)) / scale)
            assert np.max(np.abs(ys["patch"] - yr)) <= 5e-12 * scale, (k, kk)
            assert np.max(np.abs(ys["patch"] - ys["csr"])) <= 5e-12 * scale, (k, kk)
        print("%s k=%d: patch operator %.2e of the largest entry" % (which, k, worst))
    finally:
        b.close()


@pytest.mark.parametrize("which", ["3d", "dip30"])
def test_tensor_patch_operator_without_the_assembled_matrix(which, mesh2d, mesh3d, gpu_ctx):
    """assemble="vertex_block": the Jacobi diagonal (every row) is the oracle's to 1e-12, the patch product the oracle's to 5e-12,
    and there is no matrix to show."""
    from remo3d_amd import solver
    mesh, S = _case(which, mesh2d, mesh3d)
    o = _oracle(which, mesh2d, mesh3d)
    b = gpu_ctx.batch(mesh, S, SRC, EVAL)
    try:
        assert b.run(solver.make_opts(rtol=1e-2, op="patch", assemble="vertex_block")) >= 0
        assert b.stats["op_used"] == 3 and b.stats["nnz"] == 0
        derr = np.max(np.abs(b.jacobi() * _oracle_diag(o) - 1.0))
        x = np.random.default_rng(0).standard_normal((o.nfree, 3))
        y, _ = b.spmv(x)
        yr = np.stack([o.spmv(x[:, c]) for c in range(3)], 1)
        err = np.max(np.abs(y - yr)) / np.max(np.abs(yr))
        print("%s vertex_block: Jacobi diagonal %.2e, patch product %.2e of the largest entry" % (which, derr, err))
        assert derr <= 1e-12
        assert err <= 5e-12
        with pytest.raises(solver.RemoError) as e:
            b.system()
        assert "assemble" in str(e.value)
    finally:
        b.close()


@pytest.mark.parametrize("which,op", [("2d", "csr"), ("3d_coarse", "csr"), ("3d_coarse", "patch"), ("dip30_coarse", "csr"),
                                      ("dip30_coarse", "patch"), ("dip60_coarse", "csr"), ("dip60_coarse", "patch")])
@pytest.mark.parametrize("coarse", ["chebyshev", "amg"])
@pytest.mark.parametrize("precision", ["fp64", "mixed"])
def test_tensor_solve_matches_oracle(which, op, coarse, precision, mesh2d, mesh3d, gpu_ctx):
    """Whole solves at rtol 1e-12: potentials within 1e-8 (relative to the largest) of the oracle's, the TRUE residual of the
    returned solution below 5e-11."""
    from remo3d_amd import solver
    mesh, S = _case(which, mesh2d, mesh3d)
    ref = _reference(which, mesh2d, mesh3d)
    b = gpu_ctx.batch(mesh, S, SRC, EVAL)
    try:
        rc = b.run(solver.make_opts(rtol=1e-12, maxsteps=20000, op=op, coarse=coarse, precision=precision))
        assert rc == 0, (rc, b.stats["pcg_steps"], gpu_ctx.last_error())
        assert b.stats["op_used"] == (3 if op == "patch" else 0) and b.stats["coarse_used"] == (1 if coarse == "chebyshev" else 2)
        err = 0.0
        for g, r in zip(b.fetch(), ref):
            assert np.all(np.isfinite(g))
            err = max(err, np.max(np.abs(g - r)) / np.max(np.abs(r)))
        tr = float(np.max(b.true_relres()))
        print("%s %s %s %s: steps %s, potentials %.2e, true relres %.2e" % (which, op, coarse, precision, b.stats["iterations"][:3], err, tr))
        assert err <= 1e-8
        assert tr < 5e-11
    finally:
        b.close()


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_multigrid_cycle_on_a_tensor_batch_is_symmetric_positive(which, mesh2d, mesh3d, gpu_ctx):
    """One cycle C of the hierarchy built on a tensor batch's P1 block: r1' C r2 = r2' C r1 to rounding, positive, and a convergent
    iteration for the block (energy norm of the error shrinks per cycle)."""
    import ctypes as C
    import scipy.sparse as sp
    from remo3d_amd import solver
    mesh, S = _case(which, mesh2d, mesh3d)
    b = gpu_ctx.batch(mesh, S, SRC, EVAL)
    try:
        assert b.run(solver.make_opts(rtol=1e-10, maxsteps=20000, op="csr", coarse="amg")) == 0
        assert b.stats["coarse_used"] == 2
        rowptr, col, val, dinv, freeid = b.system()
        n = len(rowptr) - 1
        nvc = C.c_int64(0)
        assert b._L.remo_batch_apply_coarse(b.ctx._h, b._h, 1, None, None, 0, C.byref(nvc)) == 0
        nv = nvc.value
        Avv = sp.csr_matrix((val, col, rowptr), shape=(n, n))[:nv, :nv].tocsr()
        rng = np.random.default_rng(7)
        R = rng.standard_normal((nv, 3))
        G = R.T @ b.apply_vertex_solver(R)
        sym = np.max(np.abs(G - G.T)) / np.max(np.abs(G))
        E = rng.standard_normal((nv, 3))
        E1 = E - b.apply_vertex_solver(Avv @ E)
        before = np.sqrt(np.einsum("ik,ik->k", E, Avv @ E))
        after = np.sqrt(np.einsum("ik,ik->k", E1, Avv @ E1))
        print("%s: cycle asymmetry %.2e, energy-norm contraction %s" % (which, sym, after / before))
        assert sym <= 1e-11
        assert np.all(np.diag(G) > 0)
        assert np.all(after < 0.9 * before)
    finally:
        b.close()


@pytest.mark.parametrize("scalar", [True, False])
@pytest.mark.parametrize("condense", [True, False])
def test_degree4_quadrature_matches_the_oracles_six_point_rule(scalar, condense, mesh2d, mesh3d, gpu_ctx):
    """2D quadrature="degree4" (remo_opts_t.quadrature = 1): the CSR system is the oracle's assembly with the 6-point rule to
    1e-12 of the largest entry, for scalar and tensor sigma, and differs from the exact-rule system by far more."""
    from remo3d_amd import solver
    mesh, S = _case("2d", mesh2d, mesh3d)
    o4 = _oracle("2d", mesh2d, mesh3d, condense=condense, quadrature="degree4", scalar=scalar)
    oe = _oracle("2d", mesh2d, mesh3d, condense=condense, scalar=scalar)
    b = gpu_ctx.batch(mesh, SIGMA3 if scalar else S, SRC[:1], EVAL[:1])
    try:
        assert b.run(solver.make_opts(preconditioner="local", condense=condense, rtol=1e-2, quadrature="degree4")) >= 0
        val = _check_system(b, o4, "degree4 scalar=%s condense=%s" % (scalar, condense))
        _, _, ve = oe.csr()
        d = np.max(np.abs(val - ve)) / np.max(np.abs(ve))
        print("degree4 vs exact rule: %.2e of the largest entry" % d)
        assert d > 1e-8
    finally:
        b.close()


def test_model_with_rvuz_matches_the_oracle_end_to_end():
    """Model on BM3 at dip 30 with RVUZ = 3 RTUZ in the outer layers only (the resistive bed stays isotropic), two depths in one
    batch, mesh_scale 8 (131 k unknowns): the GPU contexts and the oracle's systems (OracleDirectContext, sparse direct solve)
    give the same apparent resistivities to 1e-6 relative, both at rtol 1e-12."""
    import time
    from remo3d_amd.model import Model
    from oracle_backend import OracleDirectContext
    f = np.loadtxt(os.path.join(BM3, "Formation_BM3_30.txt"), skiprows=2)
    f6 = np.hstack([f, np.array([[3.0 * f[0, 4]], [np.nan], [3.0 * f[2, 4]]])])
    bore = os.path.join(BM3, "Borehole_BM3.txt")
    tools = ["A0.4M6.0N", "A2.0M0.5N"]
    depths = np.array([11.0, 13.0])
    kw = dict(mesh_scale=8.0, verbose=False, solver_options=dict(rtol=1e-12, maxsteps=20000))
    logs = {}
    for name, factory in (("gpu", None), ("oracle", OracleDirectContext)):
        m = Model(tools)
        m.set_model_parameters(f6, bore, dip=30)
        if factory is None:
            m.initialize_workers(cpu_workers=1, gpu_workers=1)
        else:
            m.initialize_workers(cpu_workers=1, gpu_workers=2, context_factory=factory)
        t0 = time.time()
        m.simulate_logs(depths, **kw)
        m.shutdown_workers()
        assert m.timing["failed_batches"] == 0 and m.timing["not_converged"] == 0, m.timing
        logs[name] = m.logs
        print("%s: %.1f s" % (name, time.time() - t0))
    worst = 0.0
    for t in tools:
        g, r = logs["gpu"][t][:, 1], logs["oracle"][t][:, 1]
        assert np.all(np.isfinite(g)) and np.all(np.isfinite(r))
        worst = max(worst, float(np.max(np.abs(g / r - 1.0))))
    print("apparent resistivity, GPU vs oracle: max rel difference %.2e" % worst)
    assert worst <= 1e-6
