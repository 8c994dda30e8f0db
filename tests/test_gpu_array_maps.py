"""Model.simulate_array_logs(sensitivity_grid=...) on the GPU: d ln Ra / d ln R per grid cell of both laterolog modes, from the pair
derivatives per group of elements (remo_job_pair_groups_t).

Cases of tests/test_gpu_arrays.py: Example_01 in 2D (two depths) and Benchmark model 3 at dip 30 in 3D (one depth), domain_radius 12,
mesh scale 2.5, rtol 1e-12, the CSR product (its solves repeat bit for bit, so a sweep with the grid can be compared with one without).
Ra is homogeneous of degree one in the resistivities, the far-field constant included: the cells and the rest sum to 1, within the
1e-8 tests/test_gpu_sensitivity_maps.py asserts for the tools.
"""
import copy
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EX1 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Example_01", "Input")
BM3 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Benchmark models", "Benchmark model 3")
TIGHT = dict(rtol=1e-12, maxsteps=20000)
SUM_BOUND = 1e-8
RADIUS = 12.0
_CASES = {}


def _tables(which):
    if which == "2d":
        f = np.loadtxt(os.path.join(EX1, "Formation.txt"), skiprows=2)
        b = np.loadtxt(os.path.join(EX1, "Borehole.txt"), skiprows=2)
        dip, depths = 0, np.array([8.3, 12.45])
        grid = dict(r=[0.0, 0.15, 0.4, 1.0, 2.5, 6.0], z=[4.0, 7.0, 8.0, 8.6, 10.0, 12.0, 12.9, 15.0])
    else:
        f = np.loadtxt(os.path.join(BM3, "Formation_BM3_30.txt"), skiprows=2)
        b = np.loadtxt(os.path.join(BM3, "Borehole_BM3.txt"), skiprows=2)
        dip, depths = 30, np.array([6.0])
        grid = dict(x=[-6.0, -1.0, -0.3, 0.0, 0.3, 1.0, 6.0], z=[2.0, 5.0, 5.7, 6.3, 7.0, 10.0])
    b[:, 1] *= 1e-3      # CALM in mm
    return f, b, dip, depths, grid


def _case(which):
    """The sweeps of a case, run once: with the full grid and sensitivities (through a context that records what the solver was given
    and returned), without the grid, with a one-cell grid that holds the whole mesh, and with a part of the full grid."""
    if which in _CASES:
        return _CASES[which]
    from remo3d_amd import arrays, solver
    from remo3d_amd.model import Model, default_mesh_provider
    f, b, dip, depths, grid = _tables(which)
    inner, cache, seen = default_mesh_provider(scale=2.5), {}, []

    def provider(dim, R, batch, fg, bh, dip_rad):
        key = (batch.index, batch.electrodes.tobytes())
        if key not in cache:
            cache[key] = inner(dim, R, batch, fg, bh, dip_rad)
        return cache[key]

    class Recording(solver.Context):
        def solve_batch_pairs(self, mesh, sigma, sources, evals, pairs, opts=None, **kw):
            out = super().solve_batch_pairs(mesh, sigma, sources, evals, pairs, opts, **kw)
            seen.append(dict(mesh=mesh, sigma=np.array(sigma, dtype=float), pairs=list(pairs), kw=kw, out=out))
            return out

    arr = arrays.laterolog7()
    lateral = "x" if "x" in grid else "r"
    part = {lateral: grid[lateral][1:-1], "z": grid["z"][1:-2]}
    whole = dict(r=[0.0, 2.0 * RADIUS], z=[float(depths.min()) - 2.0 * RADIUS, float(depths.max()) + 2.0 * RADIUS])
    sweeps = [("full", dict(sensitivity_grid=grid, sensitivities=True)), ("none", dict(sensitivities=True)), ("whole", dict(sensitivity_grid=whole)),
              ("part", dict(sensitivity_grid=part))]
    if which == "2d":
        sweeps.append(("grid only", dict(sensitivity_grid=grid)))
    runs = {}
    m = Model(["A0.4M6.0N"])      # one model and context for all sweeps; a sweep publishes new arrays, so a shallow copy keeps the ones before
    m.set_model_parameters(f, b, borehole_geometry_type="diameter", dip=dip)
    m.initialize_workers(cpu_workers=1, gpu_workers=1, context_factory=Recording)
    try:
        for name, more in sweeps:
            m.simulate_array_logs(arr, depths, domain_radius=RADIUS, batch_size=1, mesh_provider=provider, verbose=False, solver_options=dict(op="csr"),
                                  **dict(TIGHT, **more))
            assert m.timing["failed_batches"] == 0, (name, m.timing["first_error"])
            runs[name] = copy.copy(m)
    finally:
        m.shutdown_workers()
    seen[:] = seen[:len(depths)]      # the calls of the first sweep
    _CASES[which] = dict(runs=runs, seen=seen, grid=grid, part=part, arr=arr, f=f, depths=depths, dim=3 if dip else 2)
    return _CASES[which]


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_cells_and_rest_sum_to_one(which):
    c = _case(which)
    m, grid = c["runs"]["full"], c["grid"]
    lateral = "x" if "x" in grid else "r"
    assert set(m.sensitivity_grid) == {lateral, "z"}
    for mode in ("LL7", "A0"):
        maps, rest = m.array_sensitivity_maps[mode], m.array_sensitivity_map_rest[mode]
        assert maps.shape == (len(c["depths"]), len(grid["z"]) - 1, len(grid[lateral]) - 1) and rest.shape == (len(c["depths"]),)
        total = maps.sum(axis=(1, 2)) + rest
        print("ARRAY MAPS %s %s: cells + rest - 1 = %s, largest cell %s, rest %s" % (which, mode, total - 1.0, np.max(np.abs(maps), axis=(1, 2)), rest))
        assert np.max(np.abs(total - 1.0)) <= SUM_BOUND
        assert np.all(np.max(np.abs(maps), axis=(1, 2)) > 1e-3)
        # a grid of one cell that holds the whole mesh reads 1, and nothing is left for the rest
        one = c["runs"]["whole"]
        assert one.array_sensitivity_maps[mode].shape == (len(c["depths"]), 1, 1)
        assert np.max(np.abs(one.array_sensitivity_maps[mode][:, 0, 0] - 1.0)) <= SUM_BOUND and np.all(one.array_sensitivity_map_rest[mode] == 0.0)
        # a part of the grid: the same cells, the rest takes the difference
        p = c["runs"]["part"]
        pm, pr = p.array_sensitivity_maps[mode], p.array_sensitivity_map_rest[mode]
        assert pm.shape == (maps.shape[0], maps.shape[1] - 3, maps.shape[2] - 2)
        assert np.max(np.abs(pm - maps[:, 1:-2, 1:-1])) <= SUM_BOUND
        assert np.max(np.abs(pr - (rest + maps.sum(axis=(1, 2)) - pm.sum(axis=(1, 2))))) <= SUM_BOUND


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_the_grid_leaves_the_other_outputs_alone(which):
    """Logs, currents, impedances and sensitivities with and without the grid: the same bits (CSR product); without the grid the new
    attributes stay None; the grid alone implies the right-hand sides of sensitivities=True."""
    c = _case(which)
    a, b, g = c["runs"]["full"], c["runs"]["none"], c["runs"].get("grid only")
    assert b.array_sensitivity_maps is None and b.array_sensitivity_map_rest is None and (g is None or g.array_sensitivities is None)
    for mode in ("LL7", "A0"):
        assert np.array_equal(a.array_logs[mode], b.array_logs[mode]) and np.array_equal(a.array_currents[mode], b.array_currents[mode])
        assert np.array_equal(a.array_sensitivities[mode], b.array_sensitivities[mode], equal_nan=True)
        assert np.array_equal(a.array_mud_sensitivity[mode], b.array_mud_sensitivity[mode])
        if g is not None:      # (2D)
            assert np.array_equal(a.array_logs[mode], g.array_logs[mode])
            assert np.array_equal(a.array_sensitivity_maps[mode], g.array_sensitivity_maps[mode])
    assert np.array_equal(a.array_impedances, b.array_impedances, equal_nan=True) and (g is None or np.array_equal(a.array_impedances, g.array_impedances, equal_nan=True))


@pytest.mark.parametrize("which", ["2d", "3d"])
def test_groups_summed_by_table_entry_are_the_layer_sensitivities(which):
    """The group derivatives the solver returned, focused as the maps are and added by material: the mud's against array_mud_sensitivity
    and, for every table entry whose resistivity no other entry shares and whose materials are isotropic, the materials of that
    resistivity against array_sensitivities - both as d ln Ra / d ln R = (dRa / dR) R / Ra."""
    from remo3d_amd import arrays
    c = _case(which)
    m, arr, f = c["runs"]["full"], c["arr"], c["f"]
    half = 0.5 if c["dim"] == 3 else 1.0
    pot, cur = np.flatnonzero(arr.potential_electrodes), np.flatnonzero(arr.current_electrodes)
    assert len(c["seen"]) == len(c["depths"])
    checked = 0
    for di, call in enumerate(c["seen"]):
        sigma, mat, groups = call["sigma"], np.asarray(call["mesh"].mat), np.asarray(call["kw"]["groups"])
        outs, dP, dPg, st, rc = call["out"]
        assert len(call["pairs"]) == len(pot) * len(cur) and dPg.shape[:2] == (len(call["pairs"]), call["kw"]["n_group"])
        gmat = np.zeros(call["kw"]["n_group"], dtype=np.int64)
        gmat[groups] = mat
        assert np.array_equal(gmat[groups], mat)
        iso = sigma if sigma.ndim == 1 else np.array([s[0, 0] if np.allclose(s, s[0, 0] * np.eye(s.shape[0]), rtol=1e-13, atol=0.0) else np.nan for s in sigma])
        for mode in ("LL7", "A0"):
            mm = arr.matrices(mode)
            I, _, y, w_hat = arrays.focus(m.array_impedances[di], mm)
            Gg = sum(w_hat[i] * I[j] * half * dPg[a * len(cur) + b] for a, i in enumerate(pot) for b, j in enumerate(cur))
            Ra = m.array_logs[mode][di, 1]
            w = sigma[gmat] * Gg if sigma.ndim == 1 else np.sum(sigma[gmat] * Gg, axis=(1, 2))
            by_mat = -(np.sign(mm.K * y / mm.I0) * mm.K / mm.I0 / Ra) * np.bincount(gmat, weights=w, minlength=len(sigma))
            mud = m.array_mud_sensitivity[mode][di] / iso[0] / Ra
            worst = abs(by_mat[0] - mud)
            s = m.array_sensitivities[mode][di]
            R_all = f[:, 3:5][np.isfinite(f[:, 3:5])]
            for layer in range(f.shape[0]):
                for col in (3, 4):
                    R = f[layer, col]
                    aniso = col == 4 and f.shape[1] >= 6 and np.isfinite(f[layer, 5])
                    if not np.isfinite(R) or aniso or np.sum(R_all == R) != 1 or abs(1.0 / R - iso[0]) <= 1e-9 * iso[0]:
                        continue
                    ks = [k for k in range(1, len(sigma)) if np.isfinite(iso[k]) and abs(iso[k] * R - 1.0) <= 1e-12]
                    if not ks or s[layer, col - 2] == 0.0:
                        continue
                    worst = max(worst, abs(by_mat[ks].sum() - s[layer, col - 2] * R / Ra))
                    checked += 1
            print("ARRAY MAPS %s %s depth %d: groups by table entry against the layer sensitivities %.2e" % (which, mode, di, worst))
            assert worst <= SUM_BOUND
    assert checked >= 2


def test_plot_array_sensitivity_map_writes_a_picture(tmp_path):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from remo3d_amd import plotting
    m = _case("2d")["runs"]["full"]
    path = str(tmp_path / "ll7.png")
    fig = plotting.plot_array_sensitivity_map(m, "LL7", 1, path)
    plt.close(fig)
    assert os.path.getsize(path) > 1000
