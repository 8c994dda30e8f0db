"""CPU side of the sensitivity maps (remo_solve_batch_sens_groups): geometry.sensitivity_cells on hand-made meshes - every element in
the cell of its centroid, compact material-pure ids, the rest pseudo-cell, the absolute-depth offset, both lateral axes in 3D - and
the binding's declarations of the two entries."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT


def _mesh2d():
    """A 4 x 3 lattice of unit squares over r in [0, 4], z in [-1, 2], each cut into two triangles; material = column parity."""
    xs, zs = np.arange(5.0), np.arange(-1.0, 3.0)
    P = np.array([[x, z] for z in zs for x in xs])
    idx = lambda i, k: k * 5 + i
    conn, mat = [], []
    for k in range(3):
        for i in range(4):
            a, b, c, d = idx(i, k), idx(i + 1, k), idx(i + 1, k + 1), idx(i, k + 1)
            conn += [[a, b, c], [a, c, d]]
            mat += [i % 2, i % 2]
    return types.SimpleNamespace(dim=2, coords=P, conn=np.array(conn, dtype=np.int32), mat=np.array(mat, dtype=np.int32))


def _mesh3d():
    """Eight small tetrahedra, one around each of eight chosen centroids (x, y, z); materials 0 / 1 by the sign of x."""
    cents = np.array([[0.5, 0.0, 0.5], [-0.5, 0.0, 0.5], [0.0, 1.5, 0.5], [0.0, -1.5, 1.5], [1.2, 1.2, 1.5], [-1.6, 0.2, -0.5],
                      [0.3, 0.4, 2.5], [3.0, 3.0, 0.5]])
    tet = 0.05 * np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])      # centroid 0
    P = np.vstack([c + tet for c in cents])
    conn = np.arange(32, dtype=np.int32).reshape(8, 4)
    return types.SimpleNamespace(dim=3, coords=P, conn=conn, mat=(cents[:, 0] < 0).astype(np.int32)), cents


def _check_tables(group, gmat, gcell, mat, cell):
    assert group.dtype == np.int32 and group.shape == mat.shape
    n_group = len(gmat)
    assert len(gcell) == n_group and np.array_equal(np.unique(group), np.arange(n_group))      # compact
    assert np.array_equal(gmat[group], mat)                                                   # material-pure
    assert np.array_equal(gcell[group], cell)                                                 # every element in its cell
    assert len(set(zip(gmat.tolist(), gcell.tolist()))) == n_group                            # one group per pair


def test_cells_2d():
    from remo3d_amd import geometry
    m = _mesh2d()
    grid = dict(r=[0.0, 1.0, 2.0, 3.0], z=[-1.0, 0.0, 1.0])          # r in [3, 4) and z in [1, 2) are outside
    group, gmat, gcell = geometry.sensitivity_cells(m, m.mat, grid, 0.0)
    cen = m.coords[m.conn].mean(axis=1)
    ir, iz = np.floor(cen[:, 0]).astype(int), np.floor(cen[:, 1] + 1.0).astype(int)
    cell = np.where((ir < 3) & (iz < 2), iz * 3 + ir, 6)
    _check_tables(group, gmat, gcell, m.mat, cell)
    assert np.sum(cell == 6) == 12 and set(gmat[gcell == 6]) == {0, 1}      # the rest cell: one group per material in it
    # mat = None reads mesh.mat; another material array regroups
    assert np.array_equal(geometry.sensitivity_cells(m, None, grid, 0.0)[0], group)
    one = geometry.sensitivity_cells(m, np.zeros_like(m.mat), grid, 0.0)
    assert len(one[1]) == 7 and np.all(one[1] == 0)


def test_absolute_depth_offset():
    """The mesh is centred on its batch: the same grid in absolute depth finds the same cells when the offset moves with it."""
    from remo3d_amd import geometry
    m = _mesh2d()
    base = geometry.sensitivity_cells(m, m.mat, dict(r=[0.0, 2.0, 4.0], z=[-1.0, 0.5, 2.0]), 0.0)
    moved = geometry.sensitivity_cells(m, m.mat, dict(r=[0.0, 2.0, 4.0], z=[99.0, 100.5, 102.0]), 100.0)
    for a, b in zip(base, moved):
        assert np.array_equal(a, b)
    assert 4 not in base[2]                                          # the grid covers the mesh: no rest cell
    away = geometry.sensitivity_cells(m, m.mat, dict(r=[0.0, 2.0, 4.0], z=[-1.0, 0.5, 2.0]), 100.0)
    assert np.all(away[2] == 4) and len(away[1]) == 2                # everything in the rest cell, one group per material


def test_cells_3d_r_and_x_axes():
    from remo3d_amd import geometry
    m, cents = _mesh3d()
    z_edges = [0.0, 1.0, 2.0]
    # r = hypot(x, y): 0.5, 0.5, 1.5, 1.5, 1.697, 1.612, 0.5 (z outside), 4.24 (outside)
    group, gmat, gcell = geometry.sensitivity_cells(m, m.mat, dict(r=[0.0, 1.0, 2.0], z=z_edges), 0.0)
    _check_tables(group, gmat, gcell, m.mat, np.array([0, 0, 1, 3, 3, 4, 4, 4]))
    assert group[0] != group[1]                                      # the same cell, two materials
    # signed x in the dip plane, y summed: x = 0.5, -0.5, 0, 0, 1.2, -1.6, 0.3 (z outside), 3 (outside)
    group, gmat, gcell = geometry.sensitivity_cells(m, m.mat, dict(x=[-2.0, 0.0, 2.0], z=z_edges), 0.0)
    _check_tables(group, gmat, gcell, m.mat, np.array([1, 0, 1, 3, 3, 4, 4, 4]))
    with pytest.raises(ValueError):
        geometry.sensitivity_cells(_mesh2d(), None, dict(x=[-2.0, 2.0], z=z_edges), 0.0)
    with pytest.raises(ValueError):
        geometry.sensitivity_cells(m, m.mat, dict(r=[0.0, 1.0]), 0.0)


def test_group_entries_are_declared_with_the_documented_arguments():
    from remo3d_amd import _lib
    from remo3d_amd._lib import RemoMesh, RemoOpts, RemoStats
    header = open(os.path.join(ROOT, "include", "remo3d_hip.h")).read()
    L = _lib.load()
    dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_void_p
    want = [vp, C.POINTER(RemoMesh), C.c_int32, dp, C.c_int32, ip, dp, dp, ip, dp,      # ctx, mesh, n_mat, sigma, n_rhs, src_ptr, src_z, src_I, eval_ptr, eval_z
            dp, C.c_int32, ip, ip, dp, dp,                                              # u_out, n_fun, fun_rhs, fun_ptr, fun_z, fun_w
            C.c_int32, ip, dp, dp, dp,                                                  # n_group, group, J_out, dJ_out, dJg_out
            C.POINTER(RemoOpts), C.POINTER(RemoStats)]
    for name in ("remo_solve_batch_sens_groups", "remo_solve_batch_sens_groups_tensor"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == want
        decl = re.search(r"int %s\((.*?)\);" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S)
        assert decl, name
        args = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
        assert len(args) == len(want)
        assert args[16:21] == ["n_group", "group", "J_out", "dJ_out", "dJg_out"] and args[-2:] == ["opts", "stats"]
    assert L.remo_abi_version() == 7
