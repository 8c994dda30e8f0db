"""Inversion of measured logs for the resistivities of the formation table (Model.invert_logs), and what one sweep of a model can
hand the next (SweepCache: the batch meshes, which depend on geometry only, and per batch the solutions of the previous sweep,
solver.WarmState, from which the next sweep's solves start).

Three layers, each usable without the one above: lm_step - one damped Gauss-Newton step, a pure function of arrays; lm_loop -
Levenberg-Marquardt around a callable evaluate(m) -> (residual, jacobian); invert_model - the loop with a Model's sweep as evaluate.
The unknowns are m = ln R of the free table entries; nothing here differentiates: the Jacobian is (R / Ra) dRa/dR of
Model.sensitivities (adjoint solves, remo_solve_batch_sens).
"""
from __future__ import annotations

import threading
import time
import types
from typing import Callable, Optional

import numpy as np

LN3 = float(np.log(3.0))


# ---- one damped step ----------------------------------------------------------------------------------------------------------
def _stacked(residual, jacobian, weights, mu, L, beta, m, m_ref, beta_ref):
    """Rows and right-hand side of the least-squares problem whose normal equations are
    (J^T W J + mu diag(J^T W J) + beta L^T L + beta_ref I) d = -(J^T W r + beta L^T L m + beta_ref (m - m_ref))."""
    r, J, w = np.asarray(residual, float), np.asarray(jacobian, float), np.asarray(weights, float)
    m = np.asarray(m, float)
    n = m.size
    sw = np.sqrt(w)
    rows, rhs = [sw[:, None] * J], [-sw * r]
    if mu > 0.0:
        rows.append(np.diag(np.sqrt(mu * np.sum(w[:, None] * J * J, axis=0))))
        rhs.append(np.zeros(n))
    if beta > 0.0 and L is not None and len(L):
        L = np.asarray(L, float)
        rows.append(np.sqrt(beta) * L)
        rhs.append(-np.sqrt(beta) * (L @ m))
    if beta_ref > 0.0 and m_ref is not None:
        rows.append(np.sqrt(beta_ref) * np.eye(n))
        rhs.append(-np.sqrt(beta_ref) * (m - np.asarray(m_ref, float)))
    return np.vstack(rows), np.concatenate(rhs)


def lm_step(residual, jacobian, weights, mu, L, beta, m, m_ref, beta_ref, lower, upper, max_step):
    """The step d of Levenberg-Marquardt for the objective
        phi(m) = sum_i w_i r_i(m)^2 + beta |L m|^2 + beta_ref |m - m_ref|^2,    r(m + d) ~ r + J d,
    i.e. the solution of (J^T W J + mu diag(J^T W J) + beta L^T L + beta_ref I) d = -(J^T W r + beta L^T L m + beta_ref (m - m_ref)),
    solved in its stacked least-squares form (the condition of J, not of J^T J; a parameter no datum sees - a zero column - gets
    d = 0: the minimum-norm solution, not a regularised one).  Then every component is clipped to +-max_step and m + d to
    [lower, upper].  residual [n_data], jacobian [n_data, n], weights [n_data] (the diagonal of W), L [n_rows, n] or None."""
    m = np.asarray(m, float)
    A, b = _stacked(residual, jacobian, weights, mu, L, beta, m, m_ref, beta_ref)
    d = np.linalg.lstsq(A, b, rcond=None)[0]
    if max_step is not None:
        d = np.clip(d, -max_step, max_step)
    md = m + d
    return np.where((md < lower) | (md > upper), np.clip(md, lower, upper) - m, d)


def objective(residual, weights, L, beta, m, m_ref, beta_ref):
    r, w = np.asarray(residual, float), np.asarray(weights, float)
    phi = float(np.sum(w * r * r))
    if beta > 0.0 and L is not None and len(L):
        phi += beta * float(np.sum((np.asarray(L, float) @ m) ** 2))
    if beta_ref > 0.0 and m_ref is not None:
        phi += beta_ref * float(np.sum((m - np.asarray(m_ref, float)) ** 2))
    return phi


# ---- the loop -----------------------------------------------------------------------------------------------------------------
def lm_loop(evaluate: Callable, m0, weights, L=None, beta=0.0, m_ref=None, beta_ref=0.0, lower=-np.inf, upper=np.inf, max_step=LN3,
            mu=1e-2, mu_up=10.0, mu_down=0.1, mu_min=1e-9, max_iterations=15, ftol=1e-3, xtol=1e-5, target_rms=None,
            on_accept: Optional[Callable] = None, on_reject: Optional[Callable] = None):
    """Levenberg-Marquardt.  evaluate(m) -> (residual, jacobian) or (residual, jacobian, info dict); records whose residual or
    Jacobian row is not finite are left out of that evaluation (weight 0) and counted.  A trial point that does not lower the
    objective is rejected: mu grows by mu_up, on_reject(m_accepted) is called (the caller restores its state) and the accepted
    residual and Jacobian are kept - no second evaluation.  max_iterations counts the trial evaluations after the first.
    Stops: max_iterations; relative decrease of the objective of an accepted step below ftol; largest |d| of a step below xtol;
    weighted rms below target_rms.  Returns a namespace: m, residual, jacobian, weights (those used: 0 where left out), objective,
    rms, mu, stop, history (one record per evaluation: objective, rms, mu, accepted, excluded, seconds + the info of evaluate)."""
    w_all = np.asarray(weights, float)
    history = []

    def run(m, mu_now):
        t0 = time.time()
        out = evaluate(m)
        r, J = np.asarray(out[0], float), np.asarray(out[1], float)
        info = dict(out[2]) if len(out) > 2 else {}
        bad = ~(np.isfinite(r) & np.all(np.isfinite(J), axis=1))
        w = np.where(bad, 0.0, w_all)
        r, J = np.where(bad, 0.0, r), np.where(bad[:, None], 0.0, J)
        phi = objective(r, w, L, beta, m, m_ref, beta_ref)
        n_ok = int(np.count_nonzero(w > 0.0))
        rms = float(np.sqrt(np.sum(w * r * r) / max(n_ok, 1)))
        history.append(dict(info, objective=phi, rms=rms, mu=mu_now, accepted=False, excluded=int(np.count_nonzero(bad)), seconds=time.time() - t0))
        return types.SimpleNamespace(m=np.array(m, float), residual=r, jacobian=J, weights=w, objective=phi, rms=rms)

    cur = run(np.asarray(m0, float), mu)
    history[-1]["accepted"] = True
    if on_accept:
        on_accept(cur.m)
    stop = "max_iterations"
    for _ in range(int(max_iterations)):
        if target_rms is not None and cur.rms <= target_rms:
            stop = "target_rms"
            break
        if cur.objective == 0.0:
            stop = "ftol"
            break
        d = lm_step(cur.residual, cur.jacobian, cur.weights, mu, L, beta, cur.m, m_ref, beta_ref, lower, upper, max_step)
        if np.max(np.abs(d), initial=0.0) < xtol:
            stop = "xtol"
            break
        trial = run(cur.m + d, mu)
        if trial.objective < cur.objective and np.isfinite(trial.objective):
            decrease = (cur.objective - trial.objective) / cur.objective
            history[-1]["accepted"] = True
            cur = trial
            mu = max(mu * mu_down, mu_min)
            if on_accept:
                on_accept(cur.m)
            if decrease < ftol:
                stop = "ftol"
                break
        else:
            mu *= mu_up
            if on_reject:
                on_reject(cur.m)
    else:
        if target_rms is not None and cur.rms <= target_rms:
            stop = "target_rms"
    return types.SimpleNamespace(m=cur.m, residual=cur.residual, jacobian=cur.jacobian, weights=cur.weights, objective=cur.objective,
                                 rms=cur.rms, mu=mu, stop=stop, history=history)


def first_differences(mask):
    """L of the smoothness term: one row per pair of vertically adjacent free entries of one column, -1 / +1 on their unknowns
    (the unknowns are numbered like np.argwhere(mask): row-major)."""
    mask = np.asarray(mask, bool)
    number = -np.ones(mask.shape, dtype=int)
    number[mask] = np.arange(int(mask.sum()))
    rows = []
    for c in range(mask.shape[1]):
        for l in range(mask.shape[0] - 1):
            if mask[l, c] and mask[l + 1, c]:
                row = np.zeros(int(mask.sum()))
                row[number[l, c]], row[number[l + 1, c]] = -1.0, 1.0
                rows.append(row)
    return np.array(rows).reshape(len(rows), int(mask.sum()))


def posterior(jacobian, weights, L=None, beta=0.0, beta_ref=0.0):
    """(singular values of W^1/2 J, parameter_std, resolution).  parameter_std = sqrt(diag((J^T W J)^-1)) - NaN for a parameter no
    datum sees (a zero column: reported, never regularised away), inf along directions the data leave undetermined; resolution = the
    diagonal of (J^T W J + beta L^T L + beta_ref I)^+ J^T W J."""
    A = np.sqrt(np.asarray(weights, float))[:, None] * np.asarray(jacobian, float)
    n = A.shape[1]
    seen = np.any(A != 0.0, axis=0)
    std = np.full(n, np.nan)
    sv = np.linalg.svd(A, compute_uv=False) if A.size else np.zeros(0)
    if np.any(seen):     # eigenvectors of J^T W J on the seen parameters: std_i^2 = sum_k Q_ik^2 / lambda_k
        lam, Q = np.linalg.eigh(A[:, seen].T @ A[:, seen])
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(lam > 1e-13 * max(float(lam.max()), 1e-300), 1.0 / lam, np.inf)
            std[seen] = np.sqrt(np.sum(np.where(Q ** 2 > 1e-30, Q ** 2 * inv[None, :], 0.0), axis=1))
    H = A.T @ A
    reg = np.zeros((n, n))
    if beta > 0.0 and L is not None and len(L):
        reg += beta * (np.asarray(L, float).T @ np.asarray(L, float))
    if beta_ref > 0.0:
        reg += beta_ref * np.eye(n)
    resolution = np.diag(np.linalg.pinv(H + reg) @ H) if n else np.zeros(0)
    return sv, std, resolution


# ---- what a sweep hands the next ----------------------------------------------------------------------------------------------
def sweep_signature(plan) -> tuple:
    """Everything the batches' meshes and the sizes of their systems depend on: depths, batch size (through the batches), domain
    radius, dip and the tool's eccentricity; the tools; the mesh settings; the geometric columns of both tables (TOP, BOTTOM, RDFZ;
    depth and caliper).  Resistivities are not in it."""
    model = plan.model
    def raw(a):
        return np.ascontiguousarray(np.asarray(a, dtype=float)).tobytes()
    tools = tuple((name, raw(t)) for name, t in model.tools.items())
    batches = tuple(raw(b.electrodes) for b in plan.batches)
    return (raw(plan.depths), raw(plan.simulation_depths), batches, float(plan.domain_radius), float(model.dip_deg), float(getattr(plan, "eccentricity", 0.0)), tools,
            plan.mesh_scale, bool(plan.netgen_path), None if plan.default_provider else id(plan.provider),
            raw(model.formation_model[:, :3]), raw(model.borehole_model[:, :2]))


def _device_memory(device):
    """(bytes of the device's memory, who said so): torch.cuda.mem_get_info where torch sees the device; else the HIP runtime the
    library is linked against, asked directly (a process whose torch cannot initialise its own context still solves on the device,
    and its warm states must not silently fall to a cap of 0); (0, why) when neither sees a device."""
    why = []
    try:
        import torch
        if torch.cuda.is_available():
            return int(torch.cuda.mem_get_info(device)[1]), "torch"
        why.append("torch sees no device")
    except Exception as ex:
        why.append("torch: {}: {}".format(type(ex).__name__, ex))
    try:
        import ctypes as C
        from . import _lib
        L = _lib.load()      # (its handle resolves the symbols of the HIP runtime it depends on)
        free, total, count = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
        if L.hipGetDeviceCount(C.byref(count)) == 0 and 0 <= device < count.value and L.hipSetDevice(int(device)) == 0 \
                and L.hipMemGetInfo(C.byref(free), C.byref(total)) == 0:
            return int(total.value), "hip"
        why.append("the HIP runtime sees no device {}".format(device))
    except Exception as ex:
        why.append("hip: {}: {}".format(type(ex).__name__, ex))
    return 0, "no device: " + "; ".join(why)


class SweepCache:
    """Pass as Model.simulate_logs(..., reuse=cache): the mesh of every batch index is kept, and per batch index a solver.WarmState
    up to warm_bytes of device memory (default: a quarter of the device's memory as torch.cuda.mem_get_info reports it at creation;
    0 without a device); batches beyond the cap run cold.  A sweep whose signature (sweep_signature) differs clears the cache first.
    Under several ranks a warm state helps where the same rank draws the same batch again (schedule="static"); a miss is a cold
    solve, never an error.  close() frees the device memory."""

    def __init__(self, meshes: bool = True, warm: bool = True, warm_bytes: Optional[int] = None, device: int = 0,
                 warm_factory: Optional[Callable] = None):
        self.keep_meshes, self.keep_warm, self.device = bool(meshes), bool(warm), int(device)
        self.warm_bytes_from = "caller"      # where the cap came from: "caller", "torch", "hip" or "no device: <why>"
        if warm_bytes is None:
            warm_bytes, self.warm_bytes_from = (_device_memory(self.device) if self.keep_warm else (0, "warm=False"))
            warm_bytes //= 4
        self.warm_bytes = int(warm_bytes)
        self.warm_factory = warm_factory
        self.signature = None
        self.meshes, self.states, self.cold = {}, {}, set()
        self.lock = threading.Lock()
        self.mesh_hits = self.warm_hits = self.sweeps = self.cleared = 0

    def begin(self, signature):
        """Start of a sweep: another signature than the last sweep's clears everything; the hit counters start at 0."""
        if self.signature is not None and signature != self.signature:
            self.clear()
            self.cleared += 1
        self.signature = signature
        self.mesh_hits = self.warm_hits = 0
        self.sweeps += 1

    def clear(self):
        with self.lock:
            for s in self.states.values():
                s.close()
            self.meshes, self.states, self.cold = {}, {}, set()

    def close(self):
        self.clear()
        self.signature = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def mesh(self, bi):
        with self.lock:
            mesh = self.meshes.get(bi) if self.keep_meshes else None
            self.mesh_hits += int(mesh is not None)
            return mesh

    def has_mesh(self, bi):
        return self.keep_meshes and bi in self.meshes

    def store_mesh(self, bi, mesh):
        if self.keep_meshes:
            with self.lock:
                self.meshes[bi] = mesh

    def bytes_held(self):
        return sum(int(s.info()["bytes"]) for s in self.states.values())

    def warm_state(self, bi):
        """The batch's state, made on first use while the cap allows another one of the largest size seen so far; else None."""
        if not self.keep_warm or self.warm_bytes <= 0:
            return None
        with self.lock:
            if bi in self.states:
                return self.states[bi]
            if bi in self.cold:
                return None
            sizes = [int(s.info()["bytes"]) for s in self.states.values()]
            if sum(sizes) + max(sizes, default=0) > self.warm_bytes:
                self.cold.add(bi)
                return None
            if self.warm_factory is None:
                from . import solver
                self.warm_factory = solver.WarmState
            self.states[bi] = self.warm_factory(self.device)
            return self.states[bi]

    def after_solve(self, bi, state):
        """Count the hit; a state that took the total past the cap is given up again (its batch runs cold from then on)."""
        with self.lock:
            self.warm_hits += int(state.info()["used_last"] == 1)
            if self.bytes_held() > self.warm_bytes:
                self.states.pop(bi).close()
                self.cold.add(bi)


# ---- Model.invert_logs --------------------------------------------------------------------------------------------------------
def free_mask(formation_model, free) -> np.ndarray:
    """Boolean [n_layers, n_cols] over the resistivity columns of the table (RTFZ, RTUZ and, when present, RVUZ)."""
    fm = np.asarray(formation_model, float)
    res = fm[:, 3:]
    finite = np.isfinite(res)
    if isinstance(free, str):
        names = {"RTFZ": 0, "RTUZ": 1, "RVUZ": 2}
        cols = list(range(res.shape[1])) if free == "all" else [names.get(p.strip().upper(), -1) for p in free.split("+")]
        if any(c < 0 or c >= res.shape[1] for c in cols):
            raise ValueError("free has to be 'all' or a '+'-joined choice of RTFZ, RTUZ and RVUZ (columns the table has), or a mask")
        mask = np.zeros(res.shape, bool)
        mask[:, cols] = finite[:, cols]
        return mask
    mask = np.asarray(free, bool)
    if mask.ndim != 2 or mask.shape[0] != res.shape[0] or mask.shape[1] > 3 or (mask.shape[1] > res.shape[1] and mask[:, res.shape[1]:].any()):
        raise ValueError("the free mask has to be [n_layers, n_cols] over RTFZ, RTUZ, RVUZ")
    full = np.zeros(res.shape, bool)
    k = min(mask.shape[1], res.shape[1])
    full[:, :k] = mask[:, :k]
    if np.any(full & ~finite):
        raise ValueError("a free entry is NaN in the formation table: layers {}".format(sorted(set(np.argwhere(full & ~finite)[:, 0].tolist()))))
    return full


def invert_model(model, observed, measurement_depths, free="RTUZ", data_std=0.05, beta=0.0, reference=None, beta_ref=0.0,
                 bounds=(0.01, 1e5), max_step=LN3, max_iterations=15, ftol=1e-3, xtol=1e-5, target_rms=None, mu=1e-2,
                 reuse_meshes=True, warm_start=False, warm_bytes=None, solver_kw=None, cache: Optional[SweepCache] = None):
    """Model.invert_logs (documented there)."""
    from . import sweep
    depths = np.asarray(measurement_depths, float)
    tools = [t for t in model.tools if t in observed]
    if not tools or set(observed) - set(model.tools):
        raise ValueError("observed has to hold logs of the model's tools: {}".format(list(model.tools)))
    obs = []
    for t in tools:
        o = np.asarray(observed[t], float)
        o = o[:, 1] if o.ndim == 2 else o
        if o.shape != depths.shape:
            raise ValueError("observed['{}'] has to hold one value per measurement depth".format(t))
        obs.append(o)
    obs = np.concatenate(obs)
    std = np.concatenate([np.full(depths.size, float(data_std[t] if isinstance(data_std, dict) else data_std)) for t in tools])
    if np.any(std <= 0.0):
        raise ValueError("data_std has to be positive")
    start = np.array(model.formation_model, copy=True)
    mask = free_mask(start, free)
    at = np.argwhere(mask)                                # (layer, resistivity column): table column 3 + c, sensitivity column 1 + c
    if not len(at):
        raise ValueError("no free entry")
    m0 = np.log(start[at[:, 0], 3 + at[:, 1]])
    m_ref = None
    if reference is not None:
        ref = np.asarray(reference, float)
        m_ref = np.log(ref[at[:, 0], 3 + at[:, 1]])
        if not np.all(np.isfinite(m_ref)):
            raise ValueError("the reference table has no positive value for a free entry")
    L = first_differences(mask)
    own_cache = cache is None and (reuse_meshes or warm_start)
    if own_cache:
        cache = SweepCache(meshes=reuse_meshes, warm=warm_start, warm_bytes=warm_bytes, device=int(getattr(model.ctx, "device_id", 0) or 0))
    sim_kw = dict(solver_kw or {})
    sim_kw.setdefault("verbose", False)
    snapshot = {}

    r0 = start[at[:, 0], 3 + at[:, 1]]

    def set_table(m):      # (an unknown that never moved keeps the bits of its table entry: exp(ln R) is not R)
        model.formation_model[at[:, 0], 3 + at[:, 1]] = np.where(m == m0, r0, np.exp(m))

    def evaluate(m):
        set_table(m)
        model.simulate_logs(depths, sensitivities=True, reuse=cache, **sim_kw)
        R = model.formation_model[at[:, 0], 3 + at[:, 1]]
        sim = np.concatenate([model.logs[t][:, 1] for t in tools])
        with np.errstate(divide="ignore", invalid="ignore"):
            ok = np.isfinite(sim) & np.isfinite(obs) & (sim > 0.0) & (obs > 0.0)
            r = np.where(ok, np.log(np.where(ok, sim, 1.0)) - np.log(np.where(ok, obs, 1.0)), np.nan)
            J = np.vstack([model.sensitivities[t][:, at[:, 0], 1 + at[:, 1]] for t in tools]) * R[None, :] / sim[:, None]
        J = np.where(ok[:, None], J, np.nan)
        snapshot["trial"] = (model.logs, model.sensitivities, model.mud_sensitivity, dict(model.timing))
        tm = model.timing
        return r, J, dict(pcg_steps=int(tm.get("pcg_steps", 0)), warm_hits=int(tm.get("warm_hits", 0)), mesh_hits=int(tm.get("mesh_hits", 0)),
                          failed_batches=int(tm.get("failed_batches", 0)), mesh_s=float(tm.get("mesh_s", 0.0)), solve_s=float(tm.get("solve_s", 0.0)),
                          sweep_s=float(tm.get("total_s", 0.0)))

    def accept(m):
        snapshot["accepted"] = snapshot["trial"]

    cache_info = dict(warm_bytes=cache.warm_bytes, warm_bytes_from=cache.warm_bytes_from, meshes=cache.keep_meshes, warm=cache.keep_warm) if cache is not None else None
    try:
        res = lm_loop(evaluate, m0, 1.0 / std ** 2, L=L, beta=beta, m_ref=m_ref, beta_ref=beta_ref, lower=float(np.log(bounds[0])),
                      upper=float(np.log(bounds[1])), max_step=max_step, mu=mu, max_iterations=max_iterations, ftol=ftol, xtol=xtol,
                      target_rms=target_rms, on_accept=accept, on_reject=set_table)
    finally:
        if cache is not None:
            cache_info.update(warm_states=len(cache.states), cold_batches=len(cache.cold))
        if own_cache:
            cache.close()
    set_table(res.m)
    model.logs, model.sensitivities, model.mud_sensitivity, model.timing = snapshot["accepted"]
    sv, pstd, resolution = posterior(res.jacobian, res.weights, L, beta, beta_ref)
    unseen = [tuple(int(v) for v in at[i]) for i in np.flatnonzero(np.isnan(pstd))]
    model.inversion = types.SimpleNamespace(
        start_table=start, final_table=np.array(model.formation_model, copy=True), free=mask, free_entries=[(int(l), int(3 + c)) for l, c in at],
        tools=tools, jacobian=res.jacobian, residual=res.residual, weights=res.weights, singular_values=sv, parameter_std=pstd,
        resolution=resolution, unseen=unseen, history=res.history, objective=res.objective, rms=res.rms, stop=res.stop, cache_info=cache_info, observed={t: np.asarray(observed[t], float) for t in tools},
        depths=depths)
    if unseen and sim_kw.get("verbose") and sweep.rank() == 0:
        print("invert_logs: no datum sees the free entries (layer, resistivity column) {}: left at their start values".format(unseen))
    return model.inversion
