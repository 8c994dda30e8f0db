"""Model.simulate_logs(sensitivity_grid=...) end to end on the GPU: maps of d ln Ra / d ln R on an (r, z) grid, on two depths each
of Example_01 (2D) and of BM3 at 30 degrees of dip with one TI layer (3D) - the models of the end-to-end tests of
test_gpu_sensitivity.py.  Ra is homogeneous of degree one in the resistivities, so the cells and the rest sum to 1."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BM3 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Benchmark models", "Benchmark model 3")
EX1 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Example_01", "Input")
TOOLS = ["A0.4M6.0N", "A2.0M0.5N"]
_CACHE = {}


def _cached_provider(scale):
    from remo3d_amd.model import default_mesh_provider
    inner, cache = default_mesh_provider(scale=scale), {}

    def provider(dim, R, batch, fg, bh, dip):      # the meshes depend on geometry only: every run of a case shares them
        if batch.index not in cache:
            cache[batch.index] = inner(dim, R, batch, fg, bh, dip)
        return cache[batch.index]
    return provider


def _case(which):
    if which == "2D":
        f = np.loadtxt(os.path.join(EX1, "Formation.txt"), skiprows=2)
        b = np.loadtxt(os.path.join(EX1, "Borehole.txt"), skiprows=2)
        b[:, 1] *= 1e-3
        # the batches are centred near 8 - 13 m and reach 50 m from there
        full = dict(r=np.array([0.0, 0.1, 0.3, 1.0, 3.0, 10.0, 51.0]), z=np.concatenate([[-45.0], np.linspace(0.0, 20.0, 11), [70.0]]))
        part = dict(r=full["r"][:4], z=full["z"][1:8])
        return dict(f=f, b=b, dip=0, depths=np.array([8.3, 12.45]), radius=50.0, scale=1.0, full=full, part=part, part_slice=(slice(1, 7), slice(0, 3)))
    f = np.loadtxt(os.path.join(BM3, "Formation_BM3_30.txt"), skiprows=2)
    f = np.vstack([f[:2], [14.23, 40.0, np.nan, np.nan, 10.0], [40.0, 60.0, np.nan, np.nan, 30.0]])
    f6 = np.hstack([f, np.full((4, 1), np.nan)])
    f6[1, 5] = 2.0 * f6[1, 4]
    b = np.loadtxt(os.path.join(BM3, "Borehole_BM3.txt"), skiprows=2)
    b[:, 1] *= 1e-3
    full = dict(x=np.array([-13.0, -3.0, -0.5, 0.0, 0.5, 3.0, 13.0]), z=np.concatenate([[-10.0], np.linspace(2.0, 10.0, 5), [20.0]]))
    part = dict(x=full["x"][1:5], z=full["z"][2:5])
    return dict(f=f6, b=b, dip=30, depths=np.array([6.0, 7.0]), radius=12.0, scale=2.5, full=full, part=part, part_slice=(slice(2, 4), slice(1, 4)))


def _run(which, grid=None, sensitivities=False):
    key = (which, None if grid is None else grid, sensitivities)
    if key not in _CACHE:
        from remo3d_amd.model import Model
        c = _CACHE.setdefault(("case", which), _case(which))
        provider = _CACHE.setdefault(("provider", which), _cached_provider(c["scale"]))
        kw = dict(dip=c["dip"], domain_radius=c["radius"], verbose=False, mesh_provider=provider, gpu_workers=1,
                  solver_options=dict(rtol=1e-12, maxsteps=20000, op="csr"), sensitivities=sensitivities)
        if grid is not None:
            kw["sensitivity_grid"] = c[grid] if grid in ("full", "part") else dict(r=[0.0, 1000.0], z=[-1000.0, 1000.0])
        m = Model.compute_synthetic_logs(TOOLS, c["depths"], c["f"], c["b"], borehole_geometry_type="diameter", **kw)
        assert m.timing["failed_batches"] == 0, m.timing["first_error"]
        _CACHE[key] = m
    return _CACHE[key]


@pytest.mark.parametrize("which", ["2D", "3D"])
def test_cells_and_rest_sum_to_one(which):
    c = _CACHE.setdefault(("case", which), _case(which))
    m = _run(which, "full", sensitivities=True)
    lateral = "x" if "x" in c["full"] else "r"
    for name in TOOLS:
        maps, rest = m.sensitivity_maps[name], m.sensitivity_map_rest[name]
        assert maps.shape == (2, len(c["full"]["z"]) - 1, len(c["full"][lateral]) - 1) and rest.shape == (2,)
        assert np.all(np.isfinite(maps)) and np.all(np.isfinite(rest))
        total = maps.sum(axis=(1, 2)) + rest
        print("MAPS %s %s: cells %s rest %s  sum - 1 = %s" % (which, name, maps.sum(axis=(1, 2)), rest, total - 1.0))
        assert np.all(np.abs(total - 1.0) <= 1e-8)
        assert np.all(np.abs(maps).max(axis=(1, 2)) > 1e-3)      # the tool does see the grid


@pytest.mark.parametrize("which", ["2D", "3D"])
def test_partial_grid_and_one_cell(which):
    c = _CACHE.setdefault(("case", which), _case(which))
    full, part, one = _run(which, "full", sensitivities=True), _run(which, "part"), _run(which, "one")
    assert part.sensitivities is None and one.sensitivities is None
    sz, sh = c["part_slice"]
    for name in TOOLS:
        fm, fr = full.sensitivity_maps[name], full.sensitivity_map_rest[name]
        pm, pr = part.sensitivity_maps[name], part.sensitivity_map_rest[name]
        assert np.all(np.abs(pm.sum(axis=(1, 2)) + pr - 1.0) <= 1e-8)
        # the partial grid's cells are cells of the full grid: the same values, and the rest takes up every other cell
        np.testing.assert_allclose(pm, fm[:, sz, sh], rtol=0, atol=1e-8)
        np.testing.assert_allclose(pr, fr + fm.sum(axis=(1, 2)) - fm[:, sz, sh].sum(axis=(1, 2)), rtol=0, atol=1e-8)
        assert np.all(np.abs(pr - fr) > 1e-6)
        assert one.sensitivity_maps[name].shape == (2, 1, 1)
        assert np.all(np.abs(one.sensitivity_maps[name][:, 0, 0] - 1.0) <= 1e-8)
        assert np.all(one.sensitivity_map_rest[name] == 0.0)


@pytest.mark.parametrize("which", ["2D", "3D"])
def test_logs_and_sensitivities_do_not_change_with_the_grid(which):
    with_grid, without = _run(which, "full", sensitivities=True), _run(which, None, sensitivities=True)
    assert without.sensitivity_maps is None and without.sensitivity_map_rest is None
    for name in TOOLS:
        np.testing.assert_array_equal(with_grid.logs[name], without.logs[name])
        np.testing.assert_array_equal(with_grid.sensitivities[name], without.sensitivities[name])
        np.testing.assert_array_equal(with_grid.mud_sensitivity[name], without.mud_sensitivity[name])


@pytest.mark.parametrize("which", ["2D", "3D"])
def test_plot_sensitivity_map_writes_a_picture(which, tmp_path):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from remo3d_amd import plotting
    m = _run(which, "full", sensitivities=True)
    path = str(tmp_path / "map.png")
    fig = plotting.plot_sensitivity_map(m, TOOLS[0], 1, path)
    plt.close(fig)
    assert os.path.getsize(path) > 1000
