"""Electrically anisotropic (TI) materials, host side: the tensor element matrix of the library (the code path the tensor
metric-terms kernel shares), its validation, the RVUZ column of the formation table and how Model hands tensors to the solver."""
import os
import types

import numpy as np
import pytest

from _anisotropy import general_tensors, mapping, ti_shape
from conftest import SIGMA3
from remo3d_amd import geometry, solver
from remo3d_amd.model import Model, default_mesh_provider

BM3 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Benchmark models", "Benchmark model 3")


def _elements(mesh, n=40):
    conn = np.sort(mesh.conn, axis=1)
    pick = np.linspace(0, len(conn) - 1, n).astype(int)
    return [(mesh.coords[conn[t]], SIGMA3[mesh.mat[t]]) for t in pick]


@pytest.mark.parametrize("dim", [2, 3])
def test_isotropic_tensor_is_bitwise_the_scalar_element_matrix(dim, mesh2d, mesh3d):
    for X, s in _elements(mesh2d if dim == 2 else mesh3d):
        K = solver.host_element_matrix(dim, X, s)
        Kt = solver.host_element_matrix(dim, X, s * np.eye(dim))
        assert np.array_equal(K, Kt)


@pytest.mark.parametrize("dim,dip", [(2, 0.0), (3, 30.0), (3, 60.0)])
def test_element_matrix_under_the_change_of_variables(dim, dip, mesh2d, mesh3d):
    """K_e(X; sigma S) == K_e(A X; sigma sqrt(det S)) (tests/_anisotropy.py), ratio 4, to 1e-13 of the largest entry."""
    S = np.diag([1.0, 0.25]) if dim == 2 else ti_shape(dip, 4.0)
    A, fac, _ = mapping(S)
    for X, s in _elements(mesh2d if dim == 2 else mesh3d):
        K = solver.host_element_matrix(dim, X, s * S)
        Km = solver.host_element_matrix(dim, X @ A.T, s * fac)
        assert np.max(np.abs(K - Km)) <= 1e-13 * np.max(np.abs(Km))
        assert not np.allclose(K, solver.host_element_matrix(dim, X, s), rtol=1e-3)    # the tensor does enter


@pytest.mark.parametrize("dim", [2, 3])
def test_tensor_element_matrices_match_oracle_quadrature(dim, mesh2d, mesh3d):
    """The tensor twin of test_reference_tensors_match_oracle_quadrature: the global matrix assembled from the library's tensor
    element matrices (remo_host_element_matrix_tensor, the host side of k_metric_terms_tensor) == the oracle's per-element
    quadrature of g_i^T S g_j with the FULL tensors (orc_create_tensor), 1e-13 of the largest entry.  One tensor per material,
    all different (tests/_anisotropy.general_tensors): every entry of the layout is nonzero somewhere, and material 0 is sigma I."""
    import scipy.sparse as sp
    from oracle.fem_oracle import Oracle
    mesh = mesh2d if dim == 2 else mesh3d
    S = general_tensors(dim)
    o = Oracle(mesh, S, condense=False)
    rp, col, val = o.csr()
    A = sp.csr_matrix((val, col, rp), shape=(o.nfree, o.nfree))
    conn = np.sort(mesh.conn, axis=1)
    eld, fid = o.eldof(), o.freeid()
    o.close()
    rows, cols, vals = [], [], []
    for t in range(len(conn)):
        K = solver.host_element_matrix(dim, mesh.coords[conn[t]], S[mesh.mat[t]])
        d = fid[eld[t]]
        ok = d >= 0
        rr, cc = np.meshgrid(d[ok], d[ok], indexing="ij")
        rows.append(rr.ravel()); cols.append(cc.ravel()); vals.append(K[np.ix_(ok, ok)].ravel())
    B = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=A.shape)
    err = abs(A - B).max() / abs(A).max()
    print("tensor element matrices vs oracle, %dD: %.2e of the largest entry" % (dim, err))
    assert err <= 1e-13
    assert set(np.unique(mesh.mat)) == {0, 1, 2}


def test_tensor_layout_off_diagonal_terms():
    """An off-diagonal entry enters with its sign: S and its mirror image in x (xz -> -xz) give different matrices, which equal
    each other's under x -> -x."""
    X = np.array([[0.1, 0.0, 0.0], [1.0, 0.2, 0.1], [0.2, 1.1, 0.3], [0.3, 0.1, 1.2]])
    S = ti_shape(30.0, 4.0)
    M = np.diag([-1.0, 1.0, 1.0])
    K1 = solver.host_element_matrix(3, X, S)
    K2 = solver.host_element_matrix(3, X, M @ S @ M)
    assert np.max(np.abs(K1 - K2)) > 1e-3 * np.max(np.abs(K1))
    K3 = solver.host_element_matrix(3, X @ M, M @ S @ M)     # mirrored element (negative orientation: |T| is taken)
    assert np.max(np.abs(K1 - K3)) <= 1e-13 * np.max(np.abs(K1))


@pytest.mark.parametrize("S", [
    [[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]],      # indefinite 2x2 minor
    [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]],     # negative determinant
    [[1.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 1.0]],      # singular
    [[-1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]],
    [[1.0, 0.0, 0.0], [0.0, np.nan, 0.0], [0.0, 0.0, 1.0]],
    [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, np.inf]],
    [[1.0, 0.5], [0.5, 0.2]],                                   # 2D, det < 0
    [[0.0, 0.0], [0.0, 1.0]],
    [[1.0, 0.0], [0.0, np.nan]],
])
def test_tensor_that_is_not_positive_definite_or_not_finite_is_rejected(S):
    S = np.asarray(S)
    dim = S.shape[0]
    X = np.eye(dim + 1, dim) + 0.5 if dim == 3 else np.array([[0.5, 0.0], [1.5, 0.0], [0.5, 1.0]])
    with pytest.raises(solver.RemoError) as ex:
        solver.host_element_matrix(dim, X, S)
    assert ex.value.code == solver.REMO_ERR_ARG


def test_sigma_table_layout_and_checks():
    S = np.array([[[1.0, 2.0, 3.0], [2.0, 4.0, 5.0], [3.0, 5.0, 6.0]]])
    t, tensor = solver.sigma_table(S, 3)
    assert tensor and t.tolist() == [[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]]
    t, tensor = solver.sigma_table(np.array([[[1.0, 2.0], [2.0, 3.0]]]), 2)
    assert tensor and t.tolist() == [[1.0, 2.0, 3.0]]
    t, tensor = solver.sigma_table([1.0, 0.1])
    assert not tensor and t.tolist() == [1.0, 0.1]
    with pytest.raises(ValueError):
        solver.sigma_table(np.array([[[1.0, 0.1], [0.0, 1.0]]]), 2)       # not symmetric
    with pytest.raises(ValueError):
        solver.sigma_table(np.eye(2)[None], 3)                            # 2x2 tensors for a 3D mesh


def test_ti_conductivity():
    S = geometry.ti_conductivity([0.1, 0.5], [0.025, 0.5], np.deg2rad(30.0), 3)
    n = np.array([np.sin(np.pi / 6), 0.0, np.cos(np.pi / 6)])
    assert np.allclose(S[0] @ n, 0.025 * n, rtol=1e-14)                  # the bedding normal carries sigma_v
    t = np.array([n[2], 0.0, -n[0]])
    assert np.allclose(S[0] @ t, 0.1 * t, rtol=1e-14) and np.allclose(S[0] @ [0, 1, 0], [0, 0.1, 0], rtol=1e-14)
    assert np.array_equal(S[1], 0.5 * np.eye(3))                          # isotropic: exactly sigma I
    assert np.array_equal(geometry.ti_conductivity([0.1], [0.3], 0.0, 2)[0], np.diag([0.1, 0.3]))


# ------------------------------------------------------------------------------------------------------------------------------
# formation table with RVUZ

def _write_table(path, rows, units=("M", "M", "M", "OHMM", "OHMM", "OHMM")):
    with open(path, "w") as f:
        f.write("TOP\tBOTTOM\tRDFZ\tRTFZ\tRTUZ\tRVUZ\n" + "\t".join(units) + "\n")
        for r in rows:
            f.write("\t".join("NaN" if np.isnan(v) else repr(float(v)) for v in r) + "\n")


def test_formation_table_with_rvuz_round_trip(tmp_path):
    rows = np.array([[0.0, 10.77, np.nan, np.nan, 10.0, 30.0], [10.77, 14.23, 0.5, 2.0, 100.0, np.nan], [14.23, 25.0, np.nan, np.nan, 10.0, 40.0]])
    p = tmp_path / "Formation.txt"
    _write_table(p, rows)
    m = Model(["A0.4M6.0N"])
    fp = m.load_formation_parameters(str(p))
    assert fp.shape == (3, 6)
    np.testing.assert_array_equal(fp, rows)
    # geometry units convert the first three columns only
    _write_table(p, rows, units=("DM", "DM", "DM", "OHMM", "OHMM", "OHMM"))
    fp = m.load_formation_parameters(str(p))
    np.testing.assert_allclose(fp[:, :3], rows[:, :3] * 0.1, rtol=1e-15)
    np.testing.assert_array_equal(fp[:, 3:], rows[:, 3:])


@pytest.mark.parametrize("bad", [0.0, -3.0])
def test_non_positive_rvuz_is_rejected(bad, tmp_path):
    rows = np.array([[0.0, 10.0, np.nan, np.nan, 10.0, 30.0], [10.0, 25.0, np.nan, np.nan, 10.0, bad]])
    with pytest.raises(ValueError):
        Model(["A0.4M6.0N"]).set_formation_parameters(rows)
    p = tmp_path / "Formation.txt"
    _write_table(p, rows)
    with pytest.raises(ValueError):
        Model(["A0.4M6.0N"]).load_formation_parameters(str(p))


# ------------------------------------------------------------------------------------------------------------------------------
# Model -> solver: what sigma reaches the context

class CapturingContext:
    """Stand-in for solver.Context: records the sigma of every batch (and, given `meshes`, the mesh with it), returns a unit
    potential."""

    def __init__(self, log, meshes=None):
        self.log = log
        self.meshes = meshes

    def solve_batch(self, mesh, sigma, sources, evals, opts):
        self.log.append((mesh.fg, sigma))
        if self.meshes is not None:
            self.meshes.append((mesh, sigma))
        return [np.ones(len(e)) for e in evals], {}, 0

    def close(self):
        pass


def _captured(formation, dip, depths, borehole=None, meshes=None, mesh_scale=None):
    """meshes: a list that receives (mesh, sigma) of every batch, the meshes then being the conforming meshes of the default
    provider at mesh_scale (otherwise stand-ins that carry the window only)."""
    log = []      # list.append is atomic: the contexts' host threads may share it
    m = Model(["A0.4M6.0N", "A2.0M0.5N"])
    bore = os.path.join(BM3, "Borehole_BM3.txt") if borehole is None else borehole
    m.set_model_parameters(formation, bore, dip=dip)
    m.initialize_workers(cpu_workers=1, gpu_workers=2, context_factory=lambda device: CapturingContext(log, meshes))
    real = default_mesh_provider(scale=mesh_scale) if meshes is not None else None

    def provider(dim, R, batch, fg, bh, dip_rad):
        if real is not None:
            mesh = real(dim, R, batch, fg, bh, dip_rad)
            mesh.fg = np.array(fg)
            return mesh
        return types.SimpleNamespace(dim=dim, n_nodes=10000, fg=np.array(fg))
    m.simulate_logs(np.asarray(depths, dtype=float), mesh_provider=provider, verbose=False)
    m.shutdown_workers()
    assert m.timing["failed_batches"] == 0, m.timing["first_error"]
    return list(log), m


BM3_FZ = np.array([[0.0, 10.77, np.nan, np.nan, 10.0], [10.77, 14.23, 0.5, 2.0, 100.0], [14.23, 25.0, np.nan, np.nan, 10.0]])


def _with_rvuz(f5, rv):
    return np.hstack([f5, np.asarray(rv, dtype=float)[:, None]])


@pytest.mark.parametrize("dip", [30, 0])
def test_model_passes_ti_tensors_per_material(dip):
    """BM3 with a flushed zone in the resistive bed, RVUZ = 3 RTUZ: every undisturbed-zone material carries
    ti_conductivity(sigma_h, sigma_h / 3) about n = (sin dip, 0, cos dip); mud and flushed zones are sigma I."""
    depths = np.linspace(8.0, 17.0, 10)
    log, _ = _captured(_with_rvuz(BM3_FZ, 3.0 * BM3_FZ[:, 4]), dip, depths)
    iso, _ = _captured(BM3_FZ, dip, depths)
    dim = 3 if dip else 2
    assert len(log) == len(iso) > 0
    by_window = {fg.tobytes(): np.asarray(s) for fg, s in iso}
    n = np.array([np.sin(np.deg2rad(dip)), 0.0, np.cos(np.deg2rad(dip))]) if dim == 3 else np.array([0.0, 1.0])
    n_aniso = 0
    for fg, S in log:
        assert S.ndim == 3 and S.shape[1:] == (dim, dim)
        sh = by_window[fg.tobytes()]                     # the isotropic model's sigma of the same window = sigma_h
        assert S.shape[0] == len(sh)
        # materials: mud, then per layer [flushed zone if any] + undisturbed zone
        uz = []
        k = 1
        for i in range(fg.shape[0]):
            if not np.isnan(fg[i, 2]):
                k += 1
            uz.append(k)
            k += 1
        assert k == len(sh)
        for j in range(len(sh)):
            if j in uz:
                assert np.array_equal(S[j], geometry.ti_conductivity([sh[j]], [sh[j] / 3.0], np.deg2rad(dip) if dim == 3 else 0.0, dim)[0])
                assert np.allclose(S[j] @ n, sh[j] / 3.0 * n, rtol=1e-14)
                n_aniso += 1
            else:
                assert np.array_equal(S[j], sh[j] * np.eye(dim))
    assert n_aniso > len(log)
    if dim == 3:
        _bedding_normal_is_the_mesh_normal(dip)


def _undisturbed_zones(fg):
    """Material numbers of the undisturbed zones of a window, layer by layer (meshgen.layered_material_fn)."""
    uz, k = [], 1
    for i in range(fg.shape[0]):
        k += 0 if np.isnan(fg[i, 2]) else 1
        uz.append(k)
        k += 1
    return uz


def _bedding_normal_is_the_mesh_normal(dip):
    """The same model on the conforming meshes the solver gets (coarse size field, two depths): on every face between the
    undisturbed zones of two adjacent layers, inside the part of the mesh whose dipping geometry is exact, the unit face normal m
    is an eigenvector of both tensors with eigenvalue sigma_v: |S m - sigma_v m| <= 1e-9 |S|.  This ties the bedding normal of
    geometry.ti_conductivity to the planes meshgen cuts the beds along; a mirrored normal misses by about sin(2 dip) |S| on
    every face.  On this coarse size field some elements within about a metre of the axis straddle a bed boundary (meshgen
    tolerates that for up to 1e-3 of the elements, test_meshgen.py): faces with a vertex within 1.5 m of the axis are left out."""
    meshes = []
    log, _ = _captured(_with_rvuz(BM3_FZ, 3.0 * BM3_FZ[:, 4]), dip, [11.0, 13.0], meshes=meshes, mesh_scale=8.0)
    assert meshes
    loc = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])
    n_faces = n_ok = 0
    for mesh, S in meshes:
        S = np.asarray(S)
        uz = _undisturbed_zones(mesh.fg)
        conn = np.asarray(mesh.conn)
        faces = np.sort(conn[:, loc].reshape(-1, 3), axis=1)
        owner = np.repeat(np.arange(len(conn)), 4)
        order = np.lexsort(faces.T[::-1])
        faces, owner = faces[order], owner[order]
        shared = np.nonzero(np.all(faces[1:] == faces[:-1], axis=1))[0]
        F, ma, mb = faces[shared], mesh.mat[owner[shared]], mesh.mat[owner[shared + 1]]
        X = mesh.coords[F]
        inside = np.all((np.linalg.norm(X, axis=2) < 0.95 * mesh.meta["exact_radius"]) & (np.hypot(X[..., 0], X[..., 1]) > 1.5), axis=1)
        for a, b in zip(uz[:-1], uz[1:]):
            sel = inside & (((ma == a) & (mb == b)) | ((ma == b) & (mb == a)))
            if not np.any(sel):
                continue
            m = np.cross(X[sel, 1] - X[sel, 0], X[sel, 2] - X[sel, 0])
            m /= np.linalg.norm(m, axis=1)[:, None]
            ok = np.ones(len(m), bool)
            for j in (a, b):
                sv = np.linalg.eigvalsh(S[j])[0]                     # sigma_v < sigma_h here (Rv = 3 Rh)
                ok &= np.linalg.norm(m @ S[j] - sv * m, axis=1) <= 1e-9 * np.max(np.abs(S[j]))
            n_faces += len(m)
            n_ok += int(ok.sum())
    print("faces between adjacent beds: %d, normal an eigenvector of both tensors (sigma_v): %d" % (n_faces, n_ok))
    assert n_faces > 30 and n_ok == n_faces


@pytest.mark.parametrize("dip", [30, 0])
def test_isotropic_rvuz_passes_todays_scalar_sigma(dip):
    depths = np.linspace(8.0, 17.0, 10)
    base, _ = _captured(BM3_FZ, dip, depths)
    for rv in (np.full(3, np.nan), BM3_FZ[:, 4].copy(), np.array([np.nan, 100.0, 10.0])):
        log, _ = _captured(_with_rvuz(BM3_FZ, rv), dip, depths)
        got = {fg.tobytes(): s for fg, s in log}
        for fg, s in base:
            g = got[fg.tobytes()]
            assert isinstance(g, list) and np.asarray(g).ndim == 1
            assert np.array_equal(np.asarray(g), np.asarray(s))


def test_dropped_flushed_zone_window_is_isotropic():
    """Dip 30, R = 50: a bed whose top lies 53 m below the window centre (45.9 m perpendicular to the bedding) is in the window,
    its 0.5 m flushed zone is not; the windowing then gives the bed RTFZ (geometry.window_formation), in the RVUZ copy alike: the
    material is isotropic at 1 / RTFZ."""
    f5 = np.array([[0.0, 113.0, np.nan, np.nan, 10.0], [113.0, 200.0, 0.5, 2.0, 20.0], [200.0, 300.0, np.nan, np.nan, 5.0]])
    bore = np.array([[0.0, 0.2, 1.0], [300.0, 0.2, 1.0]])
    log, _ = _captured(_with_rvuz(f5, [30.0, 60.0, 15.0]), 30, [60.0], borehole=bore)
    assert len(log) == 1
    fg, S = log[0]
    assert fg.shape[0] == 2 and np.isnan(fg[1, 2])                   # bed 2 kept, its flushed zone dropped
    assert S.shape == (3, 3, 3)                                       # mud, bed 1, bed 2
    assert np.array_equal(S[2], 0.5 * np.eye(3))                      # 1 / RTFZ, isotropic
    assert np.array_equal(S[1], geometry.ti_conductivity([0.1], [1.0 / 30.0], np.deg2rad(30.0), 3)[0])


def test_plot_accepts_the_six_column_model(tmp_path):
    log, m = _captured(_with_rvuz(BM3_FZ, 3.0 * BM3_FZ[:, 4]), 0, np.linspace(8.0, 17.0, 5))
    written = m.save_results(str(tmp_path))
    assert any(w.endswith("Results_plot.png") for w in written)
