"""Shared by tests/test_inversion_cpu.py and its two-rank worker: an analytic stand-in for the solver context
(Model.initialize_workers(context_factory=...)) whose readings depend on every material of the batch's window,
    J_j = sum_m a_jm / sigma_m,   a_jm = 1 + (7 j + 3 m) mod 5,   dJ_j/dsigma_m = -a_jm / sigma_m^2,
a stand-in for solver.WarmState, and the model they are used with."""
import types

import numpy as np

TOOLS = ["A0.4M6.0N", "A2.0M0.5N"]


class StandInWarm:
    BYTES = 1000

    def __init__(self, device):
        self.filled, self.used_last, self.closed = False, 0, False

    def info(self):
        return dict(n_free=10 if self.filled else 0, n_cols=1 if self.filled else 0, bytes=self.BYTES, used_last=self.used_last)

    def clear(self):
        self.filled, self.used_last = False, 0

    def close(self):
        self.closed = True


class StandInContext:
    def __init__(self, device):
        self.device_id = device
        self.sweeps = []          # per sweep: batch index -> the mesh object the context was given

    def close(self):
        pass

    def _note(self, mesh):
        if not self.sweeps or mesh.bi in self.sweeps[-1]:
            self.sweeps.append({})
        self.sweeps[-1][mesh.bi] = mesh

    @staticmethod
    def _readings(sigma, functionals):
        sigma = np.asarray(sigma, float)
        a = np.array([[1.0 + (7 * j + 3 * m) % 5 for m in range(len(sigma))] for j in range(len(functionals))]).reshape(len(functionals), len(sigma))
        return a @ (1.0 / sigma), -a / sigma[None, :] ** 2

    def solve_batch_sens(self, mesh, sigma, sources, evals, functionals, opts, warm=None):
        self._note(mesh)
        if warm is not None:
            warm.used_last, warm.filled = int(warm.filled), True
        J, dJ = self._readings(sigma, functionals)
        outs = [np.zeros(len(e)) for e in evals]
        at = [0] * len(evals)
        for j, (rhs, z, w) in enumerate(functionals):      # potentials consistent with J: 0 at the first point of a record, J at the last
            outs[rhs][at[rhs] + len(z) - 1] = J[j]
            at[rhs] += len(z)
        return outs, J, dJ, dict(pcg_steps=len(functionals)), 0

    def solve_batch(self, mesh, sigma, sources, evals, opts):
        from remo3d_amd import tasks
        raise NotImplementedError("the stand-in answers through solve_batch_sens")


def provider(dim, R, batch, fg, bh, dip):
    return types.SimpleNamespace(dim=dim, n_nodes=10, bi=batch.index)


def example_model(tools=TOOLS):
    """Four isotropic layers, the last one below every 12 m window of the depths the tests use; 2D."""
    from remo3d_amd.model import Model
    nan = np.nan
    form = np.array([[0.0, 5.0, nan, nan, 10.0], [5.0, 9.0, nan, nan, 100.0], [9.0, 40.0, nan, nan, 20.0], [40.0, 60.0, nan, nan, 30.0]])
    bore = np.array([[0.0, 0.2, 1.0], [60.0, 0.2, 1.0]])
    m = Model(list(tools))
    m.set_model_parameters(form, bore)
    m.initialize_workers(cpu_workers=1, gpu_workers=1, context_factory=StandInContext)
    return m
