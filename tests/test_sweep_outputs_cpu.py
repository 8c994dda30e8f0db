"""What Model.simulate_logs publishes, per output (logs, layer and mud sensitivities, maps), with a stand-in solver of closed-form
J_j = 1 + j, dJ_j/dsigma_m = (1 + j)(1 + m), dJ_j/dp_g = (1 + j)(1 + g) on real coarse 2D meshes: the maps alone and beside the
sensitivities, a failed batch in every output, the reset of what a later sweep does not ask for, and a programming error in a batch."""
import numpy as np
import pytest

TOOLS = ["A0.4M6.0N", "A2.0M0.5N"]
FORMATION = np.array([[0.0, 12.0, np.nan, np.nan, 7.0], [12.0, 13.5, 0.6, 2.0, 30.0], [13.5, 60.0, np.nan, np.nan, 4.0]])
BOREHOLE = np.array([[0.0, 0.2, 0.5], [60.0, 0.2, 0.5]])
DEPTHS = np.array([11.0, 12.5, 14.0])
GRID = dict(r=np.array([0.0, 0.3, 2.0, 20.0]), z=np.array([5.0, 11.0, 12.0, 13.5, 20.0]))
RADIUS, BATCH_SIZE = 50.0, 2
_MESHES = {}        # batch index -> mesh: they depend on geometry only, every run shares them


class _Context:
    """J_j = 1 + j, dJ[j, m] = (1 + j)(1 + m), dJg[j, g] = (1 + j)(1 + g); potentials with u_N - u_M = J (or u_M = J)."""
    calls = None     # per sweep: id(mesh) -> (sigma, groups, n_group) of the last call with groups

    def __init__(self, device):
        pass

    def close(self):
        pass

    @staticmethod
    def _J(n):
        return 1.0 + np.arange(n)

    def _potentials(self, evals, functionals):
        outs = [np.zeros(len(e)) for e in evals]
        for j, (rhs, z, w) in enumerate(functionals):
            outs[rhs][np.flatnonzero(np.isclose(evals[rhs], z[-1]))] = 1.0 + j
        return outs

    def solve_batch(self, mesh, sigma, sources, evals, opts):
        return [np.ones(len(e)) for e in evals], dict(pcg_steps=1), 0

    def solve_batch_sens(self, mesh, sigma, sources, evals, functionals, opts):
        J = self._J(len(functionals))
        return self._potentials(evals, functionals), J, np.outer(J, 1.0 + np.arange(len(sigma))), dict(pcg_steps=1), 0

    def solve_batch_sens_groups(self, mesh, sigma, sources, evals, functionals, groups, n_group, opts):
        J = self._J(len(functionals))
        _Context.calls[id(mesh)] = (np.array(sigma), np.array(groups), n_group)
        return (self._potentials(evals, functionals), J, np.outer(J, 1.0 + np.arange(len(sigma))), np.outer(J, 1.0 + np.arange(n_group)),
                dict(pcg_steps=1), 0)


def _sweep(model=None, fail=None, n_ctx=1, **kw):
    """One sweep; fail = (batch index, exception type): the provider raises in that batch."""
    from remo3d_amd.model import Model, default_mesh_provider
    inner = default_mesh_provider(scale=3.0)

    def provider(dim, R, batch, fg, bh, dip):
        if fail is not None and batch.index == fail[0]:
            raise fail[1]("injected into batch %d" % batch.index)
        if batch.index not in _MESHES:
            _MESHES[batch.index] = inner(dim, R, batch, fg, bh, dip)
        return _MESHES[batch.index]

    if model is None:
        model = Model(TOOLS)
        model.set_model_parameters(FORMATION, BOREHOLE)
        model.initialize_workers(cpu_workers=1, gpu_workers=n_ctx, context_factory=_Context)
    _Context.calls = {}
    model.simulate_logs(DEPTHS, domain_radius=RADIUS, batch_size=BATCH_SIZE, mesh_provider=provider, verbose=False, **kw)
    model.calls = _Context.calls
    return model


@pytest.fixture(scope="module")
def runs():
    both = _sweep(sensitivities=True, sensitivity_grid=GRID)
    return dict(both=both, maps=_sweep(sensitivity_grid=GRID), sens=_sweep(sensitivities=True))


def _batches(model):
    sim, batches = model._prepare_simulation_depths_and_tasks(DEPTHS, BATCH_SIZE)
    assert len(batches) >= 2
    return sim, batches


def _rows(batch):
    return [(r.depth_index, r.tool_index) for s in batch.solves for r in s.records]


def test_maps_alone_and_beside_the_sensitivities(runs):
    """Shapes; the maps against -(scale / Ra) bincount(group_cell, sigma[group_mat] dJg) of the closed form, computed here from the
    batch's own mesh; logs and sensitivities bit for bit the same with and without the grid."""
    from remo3d_amd import geometry, tasks
    both, maps, sens = runs["both"], runs["maps"], runs["sens"]
    n_z, n_r = len(GRID["z"]) - 1, len(GRID["r"]) - 1
    assert maps.sensitivities is None and maps.mud_sensitivity is None
    assert sens.sensitivity_maps is None and sens.sensitivity_map_rest is None and sens.sensitivity_grid is None
    sim, batches = _batches(both)
    for m in (both, maps):
        assert m.timing["failed_batches"] == 0, m.timing["first_error"]
        assert sorted(m.sensitivity_grid) == ["r", "z"] and np.array_equal(m.sensitivity_grid["z"], GRID["z"])
        want = {name: np.full((len(DEPTHS), n_z * n_r + 1), np.nan) for name in TOOLS}
        for batch in batches:
            mesh = _MESHES[batch.index]
            sigma, groups, n_group = m.calls[id(mesh)]
            g, group_mat, group_cell = geometry.sensitivity_cells(mesh, None, GRID, sim[batch.index])
            assert np.array_equal(groups, g) and n_group == len(group_mat) and sigma.ndim == 1
            assert len(np.unique(group_cell)) > 3          # the grid does cut the mesh into several cells
            for j, (di, ti, K) in enumerate(tasks.batch_functionals(batch, m.tools)[1]):
                J = 1.0 + j
                scale, Ra = np.sign(K * J) * K, abs(K * J)
                dJg = J * (1.0 + np.arange(n_group))
                want[TOOLS[ti]][di] = -(scale / Ra) * np.bincount(group_cell, weights=sigma[group_mat] * dJg, minlength=n_z * n_r + 1)
        for name in TOOLS:
            assert m.sensitivity_maps[name].shape == (len(DEPTHS), n_z, n_r) and m.sensitivity_map_rest[name].shape == (len(DEPTHS),)
            assert np.all(np.isfinite(want[name]))
            np.testing.assert_allclose(m.sensitivity_maps[name].reshape(len(DEPTHS), -1), want[name][:, :-1], rtol=1e-13, atol=0)
            np.testing.assert_allclose(m.sensitivity_map_rest[name], want[name][:, -1], rtol=1e-13, atol=0)
    for name in TOOLS:
        assert both.sensitivities[name].shape == (len(DEPTHS), 3, 3) and both.mud_sensitivity[name].shape == (len(DEPTHS),)
        np.testing.assert_array_equal(both.sensitivity_maps[name], maps.sensitivity_maps[name])
        np.testing.assert_array_equal(both.sensitivity_map_rest[name], maps.sensitivity_map_rest[name])
        np.testing.assert_array_equal(both.logs[name], sens.logs[name])
        np.testing.assert_array_equal(both.logs[name], maps.logs[name])
        np.testing.assert_array_equal(both.sensitivities[name], sens.sensitivities[name])
        np.testing.assert_array_equal(both.mud_sensitivity[name], sens.mud_sensitivity[name])
        assert np.all(both.logs[name][:, 1] > 0) and np.all(both.mud_sensitivity[name] != 0)


def test_a_failed_batch_is_nan_in_every_output_and_nowhere_else(runs):
    good = runs["both"]
    _, batches = _batches(good)
    k = 1
    bad = _sweep(fail=(k, RuntimeError), n_ctx=2, sensitivities=True, sensitivity_grid=GRID)
    assert bad.timing["failed_batches"] == 1 and bad.timing["first_error"].startswith("batch %d: RuntimeError: injected" % k)
    failed = np.zeros((len(DEPTHS), len(TOOLS)), dtype=bool)
    for di, ti in _rows(batches[k]):
        failed[di, ti] = True
    assert failed.any() and not failed.all()
    for ti, name in enumerate(TOOLS):
        f = failed[:, ti]
        for got, ref in ((bad.logs[name][:, 1], good.logs[name][:, 1]), (bad.sensitivities[name], good.sensitivities[name]),
                         (bad.mud_sensitivity[name], good.mud_sensitivity[name]), (bad.sensitivity_maps[name], good.sensitivity_maps[name]),
                         (bad.sensitivity_map_rest[name], good.sensitivity_map_rest[name])):
            assert np.all(np.isnan(got[f]))
            np.testing.assert_array_equal(got[~f], ref[~f])      # NaN there only where the table has none (RDFZ, RTFZ of two layers)
        for ref in (good.logs[name], good.mud_sensitivity[name], good.sensitivity_maps[name], good.sensitivity_map_rest[name], good.sensitivities[name][:, :, 2]):
            assert np.all(np.isfinite(ref))
        np.testing.assert_array_equal(bad.logs[name][:, 0], DEPTHS)


def test_a_plain_sweep_resets_what_it_was_not_asked_for(runs):
    m = _sweep(sensitivities=True, sensitivity_grid=GRID)
    assert all(getattr(m, a) is not None for a in ("sensitivities", "mud_sensitivity", "sensitivity_maps", "sensitivity_map_rest", "sensitivity_grid"))
    _sweep(model=m)
    assert all(getattr(m, a) is None for a in ("sensitivities", "mud_sensitivity", "sensitivity_maps", "sensitivity_map_rest", "sensitivity_grid"))
    for name in TOOLS:
        assert m.logs[name].shape == (len(DEPTHS), 2) and np.all(np.isfinite(m.logs[name]))


def test_a_programming_error_in_a_batch_is_raised_after_the_sweep_is_published(runs):
    from remo3d_amd.model import Model
    _, batches = _batches(runs["both"])
    m = Model(TOOLS)
    m.set_model_parameters(FORMATION, BOREHOLE)
    m.initialize_workers(cpu_workers=1, gpu_workers=1, context_factory=_Context)
    assert m.logs is None and m.timing == {}
    with pytest.raises(TypeError, match="injected into batch 0"):
        _sweep(model=m, fail=(0, TypeError), sensitivities=True)
    assert m.timing["failed_batches"] == 1 and m.timing["first_error"].startswith("batch 0: TypeError")
    assert m.timing["batches"] == len(batches) and m.timing["points"] == len(DEPTHS) * len(TOOLS) - len(_rows(batches[0]))
    for ti, name in enumerate(TOOLS):
        nan = np.isnan(m.logs[name][:, 1])
        assert sorted(np.flatnonzero(nan)) == sorted(di for di, t in _rows(batches[0]) if t == ti)
        assert np.array_equal(np.isnan(m.mud_sensitivity[name]), nan)
