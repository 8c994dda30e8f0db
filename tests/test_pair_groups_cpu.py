"""Pair derivatives per group of elements (remo_job_pair_groups_t) without a GPU: the struct behind the pairs job and its binding, the
refusal of a job without a context, the far-field constant's derivative per group, and Model.simulate_array_logs(sensitivity_grid=...)
through a stand-in context whose group derivatives add up to its material derivatives, so that the maps follow by hand."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA3 = [1.0, 0.1, 0.02]


def test_struct_sizes_and_offsets():
    from remo3d_amd import _lib
    G = _lib.RemoJobPairGroups
    assert C.sizeof(G) == 344
    assert [getattr(G, n).offset for n in ("pair_n_group", "pair_group_reserved", "pair_group", "dPg_out")] == [320, 324, 328, 336]
    assert C.sizeof(_lib.RemoJobPairs) == 320
    assert G._fields_[:len(_lib.RemoJobPairs._fields_)] == _lib.RemoJobPairs._fields_


def test_header_declares_the_struct_and_the_hook():
    from remo3d_amd import _lib
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "remo3d_hip.h")).read()
    end = header.index("} remo_job_pair_groups_t;")
    body = re.sub(r"/\*.*?\*/", "", header[header.rindex("typedef struct {", 0, end):end], flags=re.S)
    decls = [re.sub(r"\s+", " ", d.strip()) for d in body[body.index("{") + 1:].split(";") if d.strip()]
    assert decls == ["remo_job_pairs_t pairs", "int32_t pair_n_group", "int32_t pair_group_reserved", "const int32_t *pair_group", "double *dPg_out"]
    assert "#define REMO_ABI_VERSION 7" in header
    debug = open(os.path.join(ROOT, "include", "remo3d_hip_debug.h")).read()
    assert "remo_debug_pair_groups_timing(" in debug and "remo_debug_pair_groups_timing" in _lib.DEBUG_EXPORTS and L.remo_debug_pair_groups_timing


def test_batch_args_make_a_pair_groups_job_only_when_asked(mesh2d):
    from remo3d_amd import _lib, solver
    src, ev = [([0.0], [1.0]), ([0.1], [1.0]), ([0.4], [1.0])], [[0.1, 0.4], [0.0, 0.4], [0.0, 0.1]]
    pairs = [(0, 0), (2, 1), (0, 2)]
    j = solver._batch_args(None, mesh2d, SIGMA3, src, ev, pairs=pairs)[0][2]
    assert type(j) is _lib.RemoJobPairs and j.size == 320
    n_elems = np.asarray(mesh2d.conn).shape[0]
    group = (np.arange(n_elems) % 5 - 1).astype(np.int64)
    args, _, _, _, keep = solver._batch_args(None, mesh2d, SIGMA3, src, ev, pairs=pairs, pair_groups=(group, None))
    j = args[2]
    assert type(j) is _lib.RemoJobPairGroups and j.size == 344 and (j.n_pair, j.pair_n_group, j.pair_group_reserved) == (3, 4, 0)
    assert [j.pair_group[i] for i in range(6)] == [-1, 0, 1, 2, 3, -1] and not j.dPg_out and not j.dP_out
    assert solver._batch_args(None, mesh2d, SIGMA3, src, ev, pairs=pairs, pair_groups=(group, 9))[0][2].pair_n_group == 9
    with pytest.raises(ValueError):
        solver._batch_args(None, mesh2d, SIGMA3, src, ev, pairs=pairs, pair_groups=(group[:-1], None))
    with pytest.raises(ValueError):
        solver._batch_args(None, mesh2d, SIGMA3, src, ev, pair_groups=(group, None))


def test_pair_groups_job_is_refused_without_a_context():
    from remo3d_amd import _lib
    L = _lib.load()
    a = np.zeros(1, dtype=np.int32)
    out, outg = np.zeros(3), np.zeros(2)
    job = _lib.RemoJobPairGroups(size=C.sizeof(_lib.RemoJobPairGroups), n_pair=1, pair_a=_lib.ptr(a, C.c_int32), pair_b=_lib.ptr(a, C.c_int32),
                                 dP_out=_lib.ptr(out, C.c_double), pair_n_group=2, pair_group=_lib.ptr(a, C.c_int32), dPg_out=_lib.ptr(outg, C.c_double))
    assert L.remo_solve_job(None, None, C.byref(job), None, None) == -1
    h = C.c_void_p()
    assert L.remo_batch_create_job(None, None, C.byref(job), C.byref(h)) == -1 and not h


# ---- the far-field constant per group ----------------------------------------------------------------------------------------------------
def _bins(mesh, n_bins):
    """Material-pure groups: (material, bin of the centroid's polar angle), and the material of every group."""
    d = int(mesh.dim)
    cen = np.asarray(mesh.coords)[np.asarray(mesh.conn)].mean(axis=1)
    rho = np.abs(cen[:, 0]) if d == 2 else np.hypot(cen[:, 0], cen[:, 1])
    b = np.minimum((np.arctan2(rho, cen[:, d - 1]) / np.pi * n_bins).astype(np.int64), n_bins - 1)
    return np.asarray(mesh.mat).astype(np.int64) * n_bins + b, np.repeat(np.arange(3), n_bins), b


@pytest.mark.parametrize("tensor", [False, True])
def test_far_field_reference_per_group(mesh2d, mesh3d, tensor):
    """dcg added over the groups of each material is dc (1e-14 of the largest entry: the same terms in another order); with a band of
    elements in no group the other groups keep their values and exactly the band's facets are missing."""
    from remo3d_amd import solver
    for mesh in (mesh2d, mesh3d):
        d = int(mesh.dim)
        sig = np.array(SIGMA3)
        if tensor:
            rng = np.random.default_rng(d)
            Q = rng.standard_normal((3, d, d))
            sig = sig[:, None, None] * (np.eye(d)[None] + 0.1 * (Q + np.swapaxes(Q, 1, 2)))
        group, gmat, b = _bins(mesh, 6)
        assert len(solver.far_field_reference(mesh, sig, 50.0)) == 2
        c, dc, dcg = solver.far_field_reference(mesh, sig, 50.0, group, 18)
        c0, dc0 = solver.far_field_reference(mesh, sig, 50.0)
        assert c == c0 and np.array_equal(dc, dc0) and dcg.shape == (18,) + dc.shape[1:]
        back = np.zeros_like(dc)
        np.add.at(back, gmat, dcg)
        assert np.max(np.abs(back - dc)) <= 1e-14 * np.max(np.abs(dc))
        assert np.count_nonzero(np.abs(dcg).reshape(18, -1).max(axis=1)) >= 4      # the surface is shared among the bins
        # the bins 2 and 3 (around the horizontal) in no group
        band = (b == 2) | (b == 3)
        cut = np.where(band, -1, group)
        cb, dcb, dcgb = solver.far_field_reference(mesh, sig, 50.0, cut, 18)
        assert cb == c and np.array_equal(dcb, dc)
        in_band = np.isin(np.arange(18) % 6, (2, 3))
        assert np.array_equal(dcgb[~in_band], dcg[~in_band]) and np.all(dcgb[in_band] == 0.0) and np.any(dcg[in_band] != 0.0)
        assert solver.far_field_reference(mesh, sig, 50.0, cut)[2].shape[0] == int(cut.max()) + 1
        with pytest.raises(ValueError):
            solver.far_field_reference(mesh, sig, 50.0, group[:-1])


# ---- Model.simulate_array_logs(sensitivity_grid=...) through a stand-in context -----------------------------------------------------------
FORMATION = np.array([[0.0, 12.0, np.nan, np.nan, 7.0], [12.0, 13.5, 0.6, 2.0, 30.0], [13.5, 60.0, np.nan, np.nan, 4.0]])
BOREHOLE = np.array([[0.0, 0.2, 0.5], [60.0, 0.2, 0.5]])
DEPTHS = np.array([11.0, 12.5, 14.0])
R_SPACE = 2.5
GRID = dict(r=[0.0, 0.3, 1.0, 4.0], z=[9.0, 11.5, 12.5, 13.0, 16.0])
_MESHES = {}


class _FullSpaceGroups:
    """Full-space potentials I R / (4 pi |z - a|) whatever the mesh, pair derivatives dP[p, k] = -(1 + p) (1 + k), and per group
    dPg[p, g] = dP[p, material of g] * (elements of g) / (elements of its material): the groups of a material add up to dP.  Records
    every call."""
    calls = []

    def __init__(self, device):
        pass

    def close(self):
        pass

    def solve_batch_pairs(self, mesh, sigma, sources, evals, pairs, opts, far_field=None, groups=None, n_group=None):
        assert far_field == 50.0
        outs = [sum(I * R_SPACE / (4.0 * np.pi * np.abs(np.asarray(e, dtype=float) - a)) for a, I in zip(np.atleast_1d(z), np.atleast_1d(cur)))
                for (z, cur), e in zip(sources, evals)]
        dP = -np.outer(1.0 + np.arange(len(pairs)), 1.0 + np.arange(len(sigma)))
        rec = dict(n_rhs=len(sources), pairs=list(pairs), sigma=np.array(sigma, dtype=float), groups=groups, n_group=n_group)
        _FullSpaceGroups.calls.append(rec)
        if groups is None:
            return outs, dP, dict(pcg_steps=1), 0
        groups, mat = np.asarray(groups), np.asarray(mesh.mat)
        assert groups.shape == mat.shape and groups.min() >= 0 and groups.max() == n_group - 1
        gmat = np.zeros(n_group, dtype=np.int64)
        gmat[groups] = mat
        assert np.array_equal(gmat[groups], mat)      # material-pure
        share = np.bincount(groups, minlength=n_group) / np.bincount(mat, minlength=len(sigma))[gmat]
        rec["gmat"] = gmat
        return outs, dP, dP[:, gmat] * share[None], dict(pcg_steps=1), 0


def _sweep(fail=None, drawn=None, **kw):
    from remo3d_amd import arrays
    from remo3d_amd.model import Model, default_mesh_provider
    inner = default_mesh_provider(scale=3.0)

    def provider(dim, R, batch, fg, bh, dip):
        if drawn is not None:
            drawn.append(batch.index)
        if fail is not None and batch.index == fail:
            raise RuntimeError("injected into batch %d" % batch.index)
        if batch.index not in _MESHES:
            _MESHES[batch.index] = inner(dim, R, batch, fg, bh, dip)
        return _MESHES[batch.index]
    m = Model(["A0.4M6.0N"])
    m.set_model_parameters(FORMATION, BOREHOLE)
    m.initialize_workers(cpu_workers=1, gpu_workers=1, context_factory=_FullSpaceGroups)
    _FullSpaceGroups.calls = []
    m.simulate_array_logs(arrays.laterolog7(), DEPTHS, domain_radius=50.0, batch_size=1, mesh_provider=provider, verbose=False, **kw)
    return m


@pytest.mark.parametrize("sensitivities", [False, True])
def test_array_maps_follow_from_the_group_derivatives(sensitivities):
    from remo3d_amd import arrays
    m = _sweep(sensitivity_grid=GRID, sensitivities=sensitivities)
    assert m.timing["failed_batches"] == 0, m.timing["first_error"]
    arr = m.array
    assert (m.array_sensitivities is not None) == sensitivities
    assert set(m.sensitivity_grid) == {"r", "z"} and np.array_equal(m.sensitivity_grid["z"], GRID["z"])
    # the right-hand sides and pairs of sensitivities=True, whether it was given or not
    assert [(c["n_rhs"], len(c["pairs"])) for c in _FullSpaceGroups.calls] == [(7, 12)] * 3
    assert all(c["groups"] is not None and c["n_group"] == len(c["gmat"]) for c in _FullSpaceGroups.calls)
    pot, cur = np.flatnonzero(arr.potential_electrodes), np.flatnonzero(arr.current_electrodes)
    for mode in ("LL7", "A0"):
        maps, rest = m.array_sensitivity_maps[mode], m.array_sensitivity_map_rest[mode]
        assert maps.shape == (3, 4, 3) and rest.shape == (3,) and np.all(np.isfinite(maps)) and np.all(np.isfinite(rest))
        mm = arr.matrices(mode)
        for di, call in enumerate(_FullSpaceGroups.calls):
            I, _, y, w_hat = arrays.focus(m.array_impedances[di], mm)
            # G_k = sum_ij w_hat_i I_j dP[(i, j), k] with pair p = (position of i among the monitors) * 3 + (position of j among the current electrodes)
            G = sum(w_hat[i] * I[j] * -(1.0 + (a * 3 + b)) * (1.0 + np.arange(len(call["sigma"]))) for a, i in enumerate(pot) for b, j in enumerate(cur))
            Ra = abs(mm.K * y / mm.I0)
            assert Ra == pytest.approx(m.array_logs[mode][di, 1], rel=1e-13)
            by_hand = -(np.sign(mm.K * y / mm.I0) * mm.K / mm.I0 / Ra) * float(call["sigma"] @ G)
            assert maps[di].sum() + rest[di] == pytest.approx(by_hand, rel=1e-12)
            assert np.count_nonzero(maps[di]) >= 6 and rest[di] != 0.0


def test_array_maps_store_with_tensors():
    """_ArrayMaps.store alone, tensor tables: the cell value is -(scale / Ra) * sum over the cell's groups of sigma_g : Gg."""
    from remo3d_amd import arrays
    from remo3d_amd.model import _ArrayMaps
    arr = arrays.laterolog7()
    plan = types.SimpleNamespace(dim=3, array=arr, depths=np.array([5.0]), slab=lambda *t: np.zeros((1, 2) + t))
    out = _ArrayMaps(plan, dict(x=[-1.0, 0.0, 1.0], z=[0.0, 1.0]))
    rng = np.random.default_rng(3)
    Q = rng.standard_normal((2, 3, 3))
    sigma = np.eye(3)[None] * np.array([1.0, 0.2])[:, None, None] + 0.02 * (Q + np.swapaxes(Q, 1, 2))
    gmat, gcell = np.array([0, 1, 1, 0]), np.array([0, 0, 1, 2])
    Z = np.nan_to_num(arr.full_space_impedances(2.0), nan=7.0)
    pot, cur = np.flatnonzero(arr.potential_electrodes), np.flatnonzero(arr.current_electrodes)
    dZg = {(i, j): rng.standard_normal((4, 3, 3)) for i in pot for j in cur}
    dZg = {k: v + np.swapaxes(v, 1, 2) for k, v in dZg.items()}
    out.store(types.SimpleNamespace(sigma=sigma, group_mat=gmat, group_cell=gcell, depth_index=[0], Z=[Z], dZg=[dZg]))
    for k, mode in enumerate(arr.modes):
        mm = arr.matrices(mode)
        I, _, y, w_hat = arrays.focus(Z, mm)
        Gg = sum(w_hat[i] * I[j] * dZg[(i, j)] for i in pot for j in cur)
        per_group = np.einsum("gab,gab->g", sigma[gmat], Gg)
        expect = -(1.0 / y) * np.array([per_group[0] + per_group[1], per_group[2], per_group[3]])      # scale / Ra = sign * (K / I0) / |K y / I0| = 1 / y
        assert np.allclose(out.slabs[0][0, k], expect, rtol=1e-12, atol=0.0)


def test_array_maps_failed_batch_is_nan():
    m = _sweep(fail=1, sensitivity_grid=GRID)
    assert m.timing["failed_batches"] == 1 and "injected" in m.timing["first_error"]
    failed = np.array([False, True, False])
    for mode in ("LL7", "A0"):
        assert np.array_equal(np.isnan(m.array_sensitivity_maps[mode]).all(axis=(1, 2)), failed)
        assert np.array_equal(np.isnan(m.array_sensitivity_maps[mode]).any(axis=(1, 2)), failed)
        assert np.array_equal(np.isnan(m.array_sensitivity_map_rest[mode]), failed)
        assert np.array_equal(np.isnan(m.array_logs[mode][:, 1]), failed)


def test_attributes_stay_none_without_the_keyword_and_a_bad_grid_raises_before_any_batch():
    from remo3d_amd import arrays
    m = _sweep(sensitivities=True)
    assert m.array_sensitivity_maps is None and m.array_sensitivity_map_rest is None and m.sensitivity_grid is None
    assert all(c["groups"] is None for c in _FullSpaceGroups.calls) and m.array_sensitivities is not None
    bad = [dict(z=[0.0, 1.0]), dict(r=[0.0, 1.0]), dict(r=[0.0, 1.0], x=[0.0, 1.0], z=[0.0, 1.0]), dict(r=[0.0, 1.0], z=[1.0]),
           dict(r=[0.0, 1.0, 1.0], z=[0.0, 1.0]), dict(r=[[0.0, 1.0]], z=[0.0, 1.0]), dict(x=[-1.0, 1.0], z=[0.0, 1.0]), "rz"]
    for grid in bad:
        drawn = []
        with pytest.raises(ValueError):
            _sweep(drawn=drawn, sensitivity_grid=grid)
        assert drawn == [] and _FullSpaceGroups.calls == []
    # a sweep without the keyword clears what the one before published
    m = _sweep(sensitivity_grid=GRID)
    assert m.array_sensitivity_maps is not None
    _FullSpaceGroups.calls = []
    m.simulate_array_logs(arrays.laterolog7(), DEPTHS, domain_radius=50.0, batch_size=1, mesh_provider=lambda *a: _MESHES[a[2].index], verbose=False)
    assert m.array_sensitivity_maps is None and m.array_sensitivity_map_rest is None and m.array_logs is not None
