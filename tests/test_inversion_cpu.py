"""The inversion without a GPU: the damped step and the loop on analytic problems, Model.invert_logs and the sweep cache with an
analytic stand-in for the solver context, and two gloo ranks against one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from remo3d_amd import inversion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- lm_step --------------------------------------------------------------------------------------------------------------------
def _linear(seed=0, n_data=12, n=4):
    rng = np.random.default_rng(seed)
    J = rng.standard_normal((n_data, n))
    m = rng.standard_normal(n)
    truth = rng.standard_normal(n)
    w = rng.uniform(0.5, 2.0, n_data)
    noise = 0.1 * rng.standard_normal(n_data)
    r = J @ (m - truth) + noise           # residual of the linear forward J m against data J truth - noise
    return J, m, w, r


def test_lm_step_solves_a_linear_problem_in_one_step():
    J, m, w, r = _linear()
    d = inversion.lm_step(r, J, w, 0.0, None, 0.0, m, None, 0.0, -np.inf, np.inf, None)
    sw = np.sqrt(w)
    ref = np.linalg.lstsq(sw[:, None] * J, -sw * r, rcond=None)[0]
    np.testing.assert_allclose(d, ref, rtol=1e-12, atol=1e-14)
    assert np.max(np.abs(J.T @ (w * (r + J @ d)))) <= 1e-12 * np.max(np.abs(J.T @ (w * r)))      # the gradient vanishes


def test_lm_step_is_clipped_by_max_step_and_bounds():
    J, m, w, r = _linear()
    free = inversion.lm_step(r, J, w, 0.0, None, 0.0, m, None, 0.0, -np.inf, np.inf, None)
    assert np.max(np.abs(free)) > 0.2
    d = inversion.lm_step(r, J, w, 0.0, None, 0.0, m, None, 0.0, -np.inf, np.inf, 0.2)
    np.testing.assert_array_equal(d, np.clip(free, -0.2, 0.2))
    lo, hi = m - 0.05, m + 0.01
    d = inversion.lm_step(r, J, w, 0.0, None, 0.0, m, None, 0.0, lo, hi, None)
    np.testing.assert_allclose(m + d, np.clip(m + free, lo, hi), rtol=0, atol=1e-15)
    assert np.all(m + d >= lo - 1e-15) and np.all(m + d <= hi + 1e-15)


def test_lm_step_minimises_the_regularised_objective():
    """beta, beta_ref and mu > 0: the residual of the stated normal equations vanishes, and the step is a minimum of the (quadratic)
    objective with the damping term."""
    J, m, w, r = _linear(1)
    mask = np.ones((4, 1), bool)
    L = inversion.first_differences(mask)
    assert L.shape == (3, 4) and np.array_equal(L[0], [-1.0, 1.0, 0.0, 0.0])
    m_ref = np.zeros(4)
    beta, beta_ref, mu = 0.7, 0.3, 0.05
    d = inversion.lm_step(r, J, w, mu, L, beta, m, m_ref, beta_ref, -np.inf, np.inf, None)
    H = J.T @ (w[:, None] * J)
    lhs = H + mu * np.diag(np.diag(H)) + beta * L.T @ L + beta_ref * np.eye(4)
    g = J.T @ (w * r) + beta * L.T @ (L @ m) + beta_ref * (m - m_ref)
    assert np.max(np.abs(lhs @ d + g)) <= 1e-12 * np.max(np.abs(g))
    d0 = inversion.lm_step(r, J, w, 0.0, L, beta, m, m_ref, beta_ref, -np.inf, np.inf, None)
    phi = lambda x: inversion.objective(r + J @ (x - m), w, L, beta, x, m_ref, beta_ref)
    rng = np.random.default_rng(3)
    assert all(phi(m + d0) <= phi(m + d0 + 1e-3 * rng.standard_normal(4)) for _ in range(20))


def test_lm_step_leaves_an_unseen_parameter_alone():
    J, m, w, r = _linear()
    J[:, 2] = 0.0
    d = inversion.lm_step(r, J, w, 1e-2, None, 0.0, m, None, 0.0, -np.inf, np.inf, None)
    assert d[2] == 0.0 and np.all(d[[0, 1, 3]] != 0.0)
    sv, std, res = inversion.posterior(J, w)
    assert np.isnan(std[2]) and np.all(np.isfinite(std[[0, 1, 3]]))
    np.testing.assert_allclose(res, [1.0, 1.0, 0.0, 1.0], atol=1e-12)
    H = (J[:, [0, 1, 3]].T * w) @ J[:, [0, 1, 3]]
    np.testing.assert_allclose(std[[0, 1, 3]], np.sqrt(np.diag(np.linalg.inv(H))), rtol=1e-10)


# ---- the loop on an analytic nonlinear forward: Ra_i = sum_j w_ij R_j^p_ij -------------------------------------------------------
class _Power:
    def __init__(self, seed=0, n_data=10, n=3):
        rng = np.random.default_rng(seed)
        self.W = rng.uniform(0.1, 1.0, (n_data, n))
        self.P = rng.uniform(0.3, 1.2, (n_data, n))
        self.truth = np.log(np.array([2.0, 30.0, 8.0])[:n])
        self.obs = self.ra(self.truth)
        self.calls = 0

    def ra(self, m):
        return np.sum(self.W * np.exp(m)[None, :] ** self.P, axis=1)

    def __call__(self, m):
        self.calls += 1
        terms = self.W * np.exp(m)[None, :] ** self.P
        ra = terms.sum(1)
        return np.log(ra) - np.log(self.obs), self.P * terms / ra[:, None]      # d ln Ra / d ln R


def test_loop_reaches_the_truth_and_accepted_objectives_never_increase():
    f = _Power()
    m0 = f.truth + np.log([2.0, 0.5, 1.5])
    res = inversion.lm_loop(f, m0, np.full(10, 1.0 / 0.05 ** 2), max_iterations=30, ftol=1e-12, xtol=1e-12)
    np.testing.assert_allclose(res.m, f.truth, rtol=0, atol=1e-8)
    assert len(res.history) == f.calls
    acc = [h["objective"] for h in res.history if h["accepted"]]
    assert all(b < a for a, b in zip(acc, acc[1:])) and acc[-1] < 1e-12 * acc[0]
    assert res.history[0]["accepted"] and all(h["excluded"] == 0 for h in res.history)


def test_a_rejected_step_restores_the_table_and_raises_mu():
    """An evaluate whose second call returns a worse residual than its Jacobian promised: the step is rejected, on_reject gets the
    accepted point, mu grows tenfold and the next trial starts from the accepted residual (no second evaluation of it)."""
    f = _Power()
    m0 = f.truth + np.log([2.0, 0.5, 1.5])
    seen, restored = [], []

    def evaluate(m):
        seen.append(np.array(m))
        r, J = f(m)
        return (r + 50.0, J) if len(seen) == 2 else (r, J)

    res = inversion.lm_loop(evaluate, m0, np.full(10, 400.0), max_iterations=30, ftol=1e-12, xtol=1e-12, on_reject=lambda m: restored.append(np.array(m)))
    h = res.history
    assert h[0]["accepted"] and not h[1]["accepted"] and h[2]["accepted"]
    assert len(restored) >= 1 and np.array_equal(restored[0], m0)
    assert h[2]["mu"] == pytest.approx(10.0 * h[1]["mu"])
    assert len(seen) == len(h)                                   # the accepted point was not evaluated again
    np.testing.assert_allclose(res.m, f.truth, rtol=0, atol=1e-8)


def test_loop_leaves_out_and_counts_records_without_a_datum():
    f = _Power()

    def evaluate(m):
        r, J = f(m)
        r[3] = np.nan
        return r, J
    res = inversion.lm_loop(evaluate, f.truth + 0.3, np.full(10, 400.0), max_iterations=30, ftol=1e-12, xtol=1e-12)
    assert all(h["excluded"] == 1 for h in res.history) and res.weights[3] == 0.0
    np.testing.assert_allclose(res.m, f.truth, rtol=0, atol=1e-8)
    res = inversion.lm_loop(f, f.truth + 0.3, np.full(10, 400.0), target_rms=0.5)
    assert res.stop == "target_rms" and res.rms <= 0.5


# ---- Model.invert_logs with a stand-in context -------------------------------------------------------------------------------------
from _inversion_standin import StandInWarm, example_model, provider, TOOLS      # noqa: E402


def _truth_logs(model, depths, **kw):
    model.simulate_logs(depths, verbose=False, sensitivities=True, **kw)
    assert model.timing["failed_batches"] == 0, model.timing["first_error"]
    return {t: model.logs[t][:, 1].copy() for t in TOOLS}


SIM = dict(domain_radius=12.0, batch_size=5, mesh_provider=provider)


def test_invert_logs_recovers_the_truth_and_keeps_frozen_entries():
    depths = np.arange(3.0, 11.0, 1.0)
    m = example_model()
    truth = m.formation_model.copy()
    obs = _truth_logs(m, depths, **SIM)
    obs[TOOLS[0]][2] = np.nan                                    # no datum
    m.ctx.sweeps.clear()
    free = np.zeros((truth.shape[0], 2), bool)
    free[[0, 1, 2], 1] = True                                    # RTUZ of the three layers the depths see
    m.formation_model[[0, 1, 2], 4] *= [2.0, 0.5, 1.5]
    frozen = m.formation_model[~np.pad(free, ((0, 0), (3, 0)))].copy()
    inv = m.invert_logs(obs, depths, free=free, solver_kw=SIM, max_iterations=30, ftol=1e-14, xtol=1e-12, warm_start=False)
    assert inv is m.inversion
    np.testing.assert_allclose(m.formation_model[[0, 1, 2], 4], truth[[0, 1, 2], 4], rtol=1e-8)
    assert np.array_equal(m.formation_model[~np.pad(free, ((0, 0), (3, 0)))], frozen, equal_nan=True)      # bit for bit
    assert np.array_equal(inv.final_table, m.formation_model, equal_nan=True) and inv.start_table[0, 4] == pytest.approx(2 * truth[0, 4])
    assert all(h["excluded"] == 1 for h in inv.history)
    assert len(inv.history) == len(m.ctx.sweeps)                 # one record per sweep
    assert all(k in inv.history[0] for k in ("objective", "rms", "mu", "accepted", "excluded", "seconds", "pcg_steps", "warm_hits"))
    assert np.all(np.isfinite(inv.parameter_std)) and inv.unseen == [] and inv.singular_values.shape == (3,)
    np.testing.assert_allclose(inv.resolution, 1.0, atol=1e-9)
    # logs and sensitivities are those of the accepted table
    logs = {t: m.logs[t][:, 1].copy() for t in TOOLS}
    m.simulate_logs(depths, verbose=False, sensitivities=True, **SIM)
    for t in TOOLS:
        np.testing.assert_array_equal(m.logs[t][:, 1], logs[t])


def test_invert_logs_reports_an_unseen_layer_and_rejects_a_free_nan():
    depths = np.arange(3.0, 8.0, 1.0)
    m = example_model()
    obs = _truth_logs(m, depths, **SIM)
    m.formation_model[[0, 1], 4] *= [1.5, 0.7]
    start_far = m.formation_model[3, 4]
    inv = m.invert_logs(obs, depths, free="RTUZ", solver_kw=SIM, max_iterations=20, ftol=1e-14, xtol=1e-12, warm_start=False)
    far = [i for i, e in enumerate(inv.free_entries) if e == (3, 4)][0]      # the layer below 40 m: outside every 12 m window
    assert np.isnan(inv.parameter_std[far]) and (3, 1) in inv.unseen and inv.resolution[far] == pytest.approx(0.0, abs=1e-12)
    assert m.formation_model[3, 4] == start_far
    assert np.all(np.isfinite(np.delete(inv.parameter_std, far)))
    mask = np.zeros((4, 2), bool)
    mask[0, 0] = True                                            # RTFZ of layer 0 is NaN in the table
    with pytest.raises(ValueError, match="NaN"):
        m.invert_logs(obs, depths, free=mask, solver_kw=SIM)
    with pytest.raises(ValueError):
        m.invert_logs({"nope": obs[TOOLS[0]]}, depths, solver_kw=SIM)


def test_meshes_are_reused_between_the_sweeps_of_an_inversion():
    depths = np.arange(3.0, 8.0, 1.0)
    for reuse in (True, False):
        m = example_model()
        obs = _truth_logs(m, depths, **SIM)
        m.ctx.sweeps.clear()
        m.formation_model[[0, 1], 4] *= [1.5, 0.7]
        inv = m.invert_logs(obs, depths, free="RTUZ", solver_kw=SIM, max_iterations=4, reuse_meshes=reuse, warm_start=False)
        sweeps = m.ctx.sweeps
        assert len(sweeps) == len(inv.history) >= 3
        for bi in sweeps[0]:
            ids = [id(s[bi]) for s in sweeps]
            assert (len(set(ids)) == 1) if reuse else (len(set(ids)) == len(ids))
        assert [h["mesh_hits"] for h in inv.history][1:] == [len(sweeps[0]) if reuse else 0] * (len(sweeps) - 1)


def test_warm_states_follow_the_batches_up_to_the_cap():
    depths = np.arange(3.0, 13.0, 1.0)
    m = example_model()
    n_batches = None
    with inversion.SweepCache(warm_bytes=10 ** 9, warm_factory=StandInWarm) as cache:
        for k in range(3):
            m.simulate_logs(depths, verbose=False, sensitivities=True, reuse=cache, **SIM)
            n_batches = m.timing["batches"]
            assert m.timing["warm_hits"] == (0 if k == 0 else n_batches) and m.timing["mesh_hits"] == (0 if k == 0 else n_batches)
        assert n_batches >= 2 and len(cache.states) == n_batches
        states = list(cache.states.values())
    assert all(s.closed for s in states)
    with inversion.SweepCache(warm_bytes=StandInWarm.BYTES + 1, warm_factory=StandInWarm) as cache:      # room for one state
        for k in range(2):
            m.simulate_logs(depths, verbose=False, sensitivities=True, reuse=cache, **SIM)
        assert len(cache.states) == 1 and m.timing["warm_hits"] == 1 and m.timing["failed_batches"] == 0
    m.simulate_logs(depths, verbose=False, sensitivities=True, **SIM)       # reuse=None: the stand-in is called without `warm`
    assert "warm_hits" not in m.timing


def test_sweep_cache_is_cleared_by_geometry_and_tools_but_not_by_resistivities():
    from remo3d_amd.model import Model
    depths = np.arange(3.0, 8.0, 1.0)
    m = example_model()
    with inversion.SweepCache(warm_bytes=10 ** 9, warm_factory=StandInWarm) as cache:
        m.simulate_logs(depths, verbose=False, sensitivities=True, reuse=cache, **SIM)
        first = dict(cache.meshes)
        m.formation_model[:, 4] *= 1.3                            # resistivities only
        m.borehole_model[:, 2] *= 0.9
        m.simulate_logs(depths, verbose=False, sensitivities=True, reuse=cache, **SIM)
        assert cache.cleared == 0 and all(cache.meshes[bi] is first[bi] for bi in first) and m.timing["warm_hits"] == len(first)
        m.formation_model[0, 1] += 0.25                           # a boundary depth
        m.formation_model[1, 0] += 0.25
        m.simulate_logs(depths, verbose=False, sensitivities=True, reuse=cache, **SIM)
        assert cache.cleared == 1 and m.timing["mesh_hits"] == 0 and m.timing["warm_hits"] == 0
        assert all(cache.meshes[bi] is not first[bi] for bi in first)
        second = dict(cache.meshes)
        m2 = example_model(tools=TOOLS[:1])                       # another tool list
        m2.formation_model[:] = m.formation_model
        m2.simulate_logs(depths, verbose=False, sensitivities=True, reuse=cache, **SIM)
        assert cache.cleared == 2 and m2.timing["mesh_hits"] == 0
        assert all(cache.meshes[bi] is not second.get(bi) for bi in cache.meshes)


def test_plot_inversion_writes_a_picture(tmp_path):
    from remo3d_amd import plotting
    import matplotlib.pyplot as plt
    depths = np.arange(3.0, 8.0, 1.0)
    m = example_model()
    obs = _truth_logs(m, depths, **SIM)
    truth = m.formation_model.copy()
    m.formation_model[[0, 1], 4] *= [1.5, 0.7]
    m.invert_logs(obs, depths, solver_kw=SIM, max_iterations=3)
    path = str(tmp_path / "inversion.png")
    fig = plotting.plot_inversion(m, path, true_table=truth)
    assert len(fig.axes) == 1 + len(TOOLS) and os.path.getsize(path) > 10000
    plt.close(fig)


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_gloo_ranks_end_with_the_table_of_one(tmp_path):
    worker = os.path.join(ROOT, "tests", "_inversion_worker.py")
    env = dict(os.environ, OMP_NUM_THREADS="1", REMO_DIST_BACKEND="gloo")
    one = str(tmp_path / "one")
    r = subprocess.run([sys.executable, worker, one], env={k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")},
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    two = str(tmp_path / "two")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), worker, two]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    ref = json.load(open(one + ".0"))
    got = [json.load(open("{}.{}".format(two, k))) for k in range(2)]
    assert ref["world"] == 1 and [g["world"] for g in got] == [2, 2]
    for g in got:
        assert g["table"] == ref["table"]                         # hex strings of the doubles: bit for bit
        assert g["accepted"] == ref["accepted"]
    assert sum(g["my_batches"] for g in got) == ref["my_batches"] and all(g["my_batches"] > 0 for g in got)
