"""`Model`: the public face of ReMo3D (remo3d/remo3d.py class Model, lines 23-1147) on top of the
MI355X library.  Same constructor, same `compute_synthetic_logs(...)` keyword arguments and
defaults, same `logs` dictionary (tool -> [n_depths, 2] array of depth and apparent resistivity),
same `Results_<n>.txt` layout.

What differs, by design:
  * the MPI worker farm (remo3d.py:552-599, 809-865) is gone: one process drives one GPU; under
    `torchrun` every rank takes a block-cyclic share of the batches and the logs are combined
    with one RCCL all-reduce of the [n_depths, n_tools] slab (sweep.py);
  * Gmsh / Netgen are not available: batch meshes come from `mesh_provider` (default: the seeded
    in-repo mesher, meshgen.make_mesh, with the reference's size field); a provider that reads
    real MSH 2.2 files can be plugged in;
  * there is no CPU solver behind it: without libremo3d_hip.so and a GPU, construction of the
    solver context raises.
"""
from __future__ import annotations

import collections
import datetime
import multiprocessing
import os
import queue
import sys
import threading
import time
import types
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor
from typing import Callable, Dict, Optional

import numpy as np

from . import arrays, geometry, meshgen, solver, sweep, tasks, tools as tools_mod

CONVERSION = {"M": 1.0, "DM": 0.1, "CM": 0.01, "MM": 0.001, "IN": 0.0254, "FT": 0.3048}


# Default multiplier on the reference's size field.  2D: 0.35 - the value at which the complete Example_01 of the reference
# (1506 points) sits within p99 8e-4 / max 2.2e-3 of the reference's committed log (scale 1.0: 7.7e-3 / 2.5e-2, 0.5: 3.6e-3 /
# 9.4e-3; profiles/r02_example01_scales.log): short lateral spacings read potential differences of a few per cent of the
# potential, next to a borehole wall with a kink every 0.1 m.  3D: 1.0 (the reference's field as it is).
DEFAULT_SCALE = {2: 0.35, 3: 1.0}

# Contexts (HIP stream + arena + host thread) per GPU when the caller does not say (gpu_workers = 0).  bench.py, size L, same box,
# points/s on SURVEY 8d's span: 1 context 91-101, 2: 109.7-110.3 / 115.3-115.9, 3: 113.3-113.4 / 117.2, 4: 110.1
# (profiles/r04_i_bench_streams*.json, r04_c_bench_streams*.json) - all with the HIP runtime's default of four hardware queues,
# where the fourth context shares a queue with another stream of the process.  With eight (remo3d_amd/__init__.py), end of round 4,
# alternating runs on one box: 3 contexts 159.9-160.0, 4: 157.9-160.6, 5: 168.1-168.3, 6: 165.7-166.5, 8: 163.8-165.2
# (profiles/r04_bl_hw_queues_and_contexts.json).
DEFAULT_CONTEXTS = 5
MAX_CONTEXTS = 8


def lattice_mesh_key(dim, domain_radius, batch, scale, seed=0) -> tuple:
    """What a lattice mesh depends on: the electrode pattern of the batch in its own frame, size multiplier and seed - not the
    depth (the 40 batches of the bench's 100-depth sweep share six meshes).  Key of the provider's caches, in memory and on disk."""
    cur = batch.electrodes[0, batch.electrodes[1, :] != 0]
    pot = batch.electrodes[0, batch.electrodes[1, :] == 0]
    return (int(dim), float(domain_radius), tuple(float(v) for v in np.round(cur, 4)), tuple(float(v) for v in np.round(pot, 4)), float(scale), int(seed))


def tuned_coarse_for_conforming(n_nodes: int) -> dict:
    """Solver of the P1 block for the revolved conforming 3D meshes.  Graded and sheared, they want more of it than isotropic meshes
    of the same vertex count: one multigrid cycle where its hierarchy can be built (GPU scan at 64 k vertices, tools/scan_conforming.py,
    profiles/r04_p_scan_conforming_vertex_solver.log: 62.4 ms of solve per batch and 187 steps against 69.5 ms / 198 steps with the best
    polynomial; Model end to end 63 against 54 points/s), else a Chebyshev polynomial of higher degree on a wider interval than the
    library's default (tools/scan_coarse3d.py: 8 / 300 at 19 k vertices, 14 / 400 at 51 k)."""
    rel = max(int(n_nodes), 1) / 12600.0
    return dict(coarse="amg_or_chebyshev", coarse_degree=int(min(16, max(6, round(7.0 * rel ** 0.5)))),
                coarse_ratio=int(min(1200, max(150, round(220.0 * rel ** (2.0 / 3.0))))))


def vertex_solver_options(dim: int, n_nodes: int, conforming: bool, n_contexts: int) -> dict:
    """The solver of the P1 block `Model` asks for when the caller did not choose one (keywords of solver.make_opts).
    2D: the library's default (one multigrid cycle).  3D, interface-conforming meshes of the default provider: the cycle with the tuned
    polynomial behind it (tuned_coarse_for_conforming).  3D, any other mesh: the cycle (polynomial if its hierarchy cannot be built)
    WHEN SEVERAL CONTEXTS SHARE THE GPU - its set-up waits for the host once per level and its twelve launches per step are latency,
    which other batches' kernels fill: bench.py on three contexts, points/s with the cycle against the polynomial: size S 434 / 410,
    M 253 / 222, L 131 / 122, L mixed 187 / 177, XL 37.0 / 33.9, XL mixed 54.6 / 49.3 (profiles/r04_s_*, r04_u_*, r04_x_*, r04_y_*); on ONE context the polynomial (the library's default in 3D)
    is ahead: L 93 / 87, S 252 / 205 (profiles/r04_t_*)."""
    if dim != 3:
        return {}
    if conforming:
        return tuned_coarse_for_conforming(n_nodes)
    return dict(coarse="amg_or_chebyshev") if n_contexts >= 2 else {}


def default_mesh_provider(scale: Optional[float] = None, seed: int = 0, mesh_3d: str = "conforming", sectors: int = 6) -> Callable:
    """Batch mesh factory.  scale: multiplier on the reference's size field (None: DEFAULT_SCALE by dimension).  2D: interface-conforming half-disc meshes built per batch.
    3D, mesh_3d = "conforming" (default): the 2D conforming mesh of the window revolved in the sheared
    frame of the dipping layers (meshgen.make_mesh_3d_conforming: every interface of the reference's
    OpenCASCADE geometry is a union of element faces); "lattice": seeded graded half-ball meshes cached on
    the electrode pattern, materials by element centroid (the bench's synthetic meshes)."""
    if mesh_3d not in ("conforming", "lattice"):
        raise ValueError("mesh_3d must be 'conforming' or 'lattice'")
    cache: Dict[tuple, meshgen.Mesh] = {}

    scale_arg = scale

    def provider(dim, domain_radius, batch, local_formation_geometry, local_borehole_geometry, dip_rad):
        scale = DEFAULT_SCALE[dim] if scale_arg is None else scale_arg
        cur = batch.electrodes[0, batch.electrodes[1, :] != 0]
        pot = batch.electrodes[0, batch.electrodes[1, :] == 0]
        fn = meshgen.layered_material_fn(dim, local_formation_geometry, local_borehole_geometry, dip_rad)
        if dim == 2:
            # axisymmetric models get meshes that CONFORM to the borehole wall, the layer boundaries and
            # the flushed-zone radii (like the reference's Netgen / Gmsh geometry); they depend on the
            # depth window, so there is nothing to cache
            # and are refined around measuring electrodes as well as current electrodes: a potential
            # difference read next to a layer boundary needs it (max deviation from the reference's
            # Example_01 log 7e-2 -> 5e-3, median 9e-4 -> 3e-4; it costs 2.5x the triangles, which is cheap in 2D)
            polys = meshgen.layer_interfaces_2d(local_formation_geometry, local_borehole_geometry, domain_radius)
            inside = [z for z in list(cur) + list(pot) if abs(z) < domain_radius]
            fg = np.asarray(local_formation_geometry, dtype=float)
            cap = meshgen.LayerCap(np.concatenate([fg[:1, 0], fg[:, 1]]))     # thin beds bound the element size
            return meshgen.make_mesh(2, domain_radius, sources_z=inside, scale=scale, seed=seed, interfaces=polys, material_fn=fn,
                                     layer_cap=cap)
        if mesh_3d == "conforming":
            fg = np.asarray(local_formation_geometry, dtype=float)
            cap = meshgen.LayerCap(np.concatenate([fg[:1, 0], fg[:, 1]]))
            return meshgen.make_mesh_3d_conforming(domain_radius, local_formation_geometry, local_borehole_geometry, dip_rad,
                                                   sources_z=list(cur), snap_z=list(pot), scale=scale, seed=seed, layer_cap=cap, sectors=sectors,
                                                   source_x=float(getattr(batch, "lateral", 0.0)))     # an eccentred tool: refined where it is
        key = lattice_mesh_key(dim, domain_radius, batch, scale, seed)
        base = cache.get(key)
        if base is None:
            # (also kept on disk, meshgen.cached_mesh: every batch of a tool, every rank and every rerun share it)
            base = meshgen.cached_mesh(("lattice",) + key, lambda: meshgen.make_mesh(
                dim, domain_radius, sources_z=list(cur), scale=scale, seed=seed, snap_z=[z for z in pot if abs(z) < domain_radius]))
            if len(cache) > 64:
                cache.clear()
            cache[key] = base
        mat = fn(base.coords[base.conn].mean(1)).astype(np.int32)
        return meshgen.Mesh(dim, base.coords, base.conn, mat, base.bconn, base.bdirichlet, base.meta)

    return provider


# mesh generation ahead of the solver, in spawned processes (numpy / scipy only: they never touch the GPU)
_WORKER_PROVIDER = None


def _mesh_worker_init(provider_kwargs):
    global _WORKER_PROVIDER
    _WORKER_PROVIDER = default_mesh_provider(**provider_kwargs)


def _mesh_worker_run(job):
    dim, domain_radius, electrodes, fg, bh, dip_rad, lateral = job
    return _WORKER_PROVIDER(dim, domain_radius, types.SimpleNamespace(electrodes=electrodes, lateral=lateral), fg, bh, dip_rad)


# -- the stages of Model.simulate_logs, in the order a sweep goes through them ---------------------------
class _Plan:
    """Stage 1, before any batch is drawn: the arguments checked, the batches, the solver options."""

    def __init__(self, model, measurement_depths, domain_radius, batch_size, mesh_generator, mesh_provider, mesh_scale, solver_kw,
                 solver_options, verbose, eccentricity=0.0):
        extra = dict(solver_options or {})
        # the tool's displacement from the borehole axis, along x of the mesh frame: checked before any batch is drawn
        if not np.isfinite(eccentricity):
            raise ValueError("eccentricity has to be a finite number of metres")
        self.eccentricity = float(eccentricity)
        if self.eccentricity != 0.0:
            if abs(self.eccentricity) >= float(np.min(model.borehole_model[:, 1])):
                raise ValueError("eccentricity has to be smaller than the smallest borehole radius: the tool is in the mud")
            if mesh_generator == "netgen":
                raise ValueError("An eccentred tool is a 3D model: the only mesh generator supported in 3D models is gmsh")
        self.model, self.domain_radius, self.mesh_scale = model, domain_radius, mesh_scale
        self.depths = np.asarray(measurement_depths, dtype=float)
        alert = False
        for far in self._reaches():
            if far > domain_radius:
                raise ValueError("Some electrodes are locate outside the simulation domain. Domain size have to be increased")
            alert |= far > 0.75 * domain_radius
        if alert and verbose:
            print("Some electrodes are located close to the boundary of the simulation domain. This may cause problems during simulation. "
                  "Consider increase of the domain size")
        if mesh_generator not in ("auto", "gmsh", "netgen"):
            raise ValueError("mesh_generator has to be 'auto', 'gmsh' or 'netgen'")
        dipping = not np.isclose(model.dip_deg, 0)
        is3d = dipping or self.eccentricity != 0.0      # an eccentred tool breaks the axial symmetry also between flat beds
        if is3d and mesh_generator == "netgen":
            raise ValueError("The only mesh generator supported in 3D models is gmsh")
        if solver_kw["preconditioner"] not in ("local", "multigrid"):
            raise ValueError("preconditioner has to be 'local' or 'multigrid'")
        if model.ctx is None:
            raise RuntimeError("initialize_workers() has to be called before simulate_logs()")
        if model.dip_deg != 0 or self.eccentricity != 0.0:
            model.borehole_model = model._add_points_to_borehole()
        self.dim, self.window_dip = (3, model.dip_rad if dipping else 0.0) if is3d else (2, 0.0)
        self.mesh_dip = self.window_dip                 # what the mesher is given: exactly 0 for flat beds
        self.netgen_path = (not is3d) and mesh_generator in ("auto", "netgen")
        self.default_provider = mesh_provider is None     # its 3D meshes are the conforming revolved ones; only it runs in the mesh pool
        self.provider = mesh_provider or default_mesh_provider(scale=mesh_scale)
        self.simulation_depths, self.batches = self._draw_batches(batch_size)
        for b in self.batches:
            b.lateral = self.eccentricity
        self.borehole_geometry = np.ascontiguousarray(model.borehole_model[:, :2])
        self.mud = np.interp(self.simulation_depths, model.borehole_model[:, 0], model.borehole_model[:, 2])
        if verbose and sweep.rank() == 0:
            print("{} simulation tasks prepared".format(len(self.batches)))
        # ONE dictionary of solver keywords: the explicit arguments, over-ridden by solver_options (a key given in both places used
        # to raise "multiple values" inside every batch, i.e. a sweep of NaNs); unknown keys fail here, before any batch is drawn,
        # on every rank alike
        self.base_kw = dict(solver_kw, **extra)
        self.opts = solver.make_opts(**self.base_kw)
        # the solver of the P1 block follows the mesh kind and the number of contexts (vertex_solver_options) unless the caller chose one
        self.tuned_coarse = self.base_kw["preconditioner"] == "multigrid" and not any(k in extra for k in ("coarse", "coarse_degree", "coarse_ratio"))
        self.contexts = [model.ctx] + list(getattr(model, "extra_ctx", []))
        self.share_len = len(list(sweep.my_share(len(self.batches))))
        self.secondary = None      # simulate_logs(formulation="secondary"): the keyword every batch's solve is given

    def _reaches(self):
        """How far from a batch's centre the electrodes of every tool lie."""
        return [float(np.max(np.abs(t[0, :3]))) for t in self.model.tools.values()]

    def _draw_batches(self, batch_size):
        return self.model._prepare_simulation_depths_and_tasks(self.depths, batch_size)

    def batch_opts(self, mesh):
        if self.tuned_coarse and getattr(mesh, "dim", 0) == 3:
            vs = vertex_solver_options(3, mesh.n_nodes, self.default_provider, len(self.contexts))
            if vs:
                return solver.make_opts(**dict(self.base_kw, **vs))
        return self.opts

    def slab(self, *tail):
        """Zeros per (depth, tool): every rank fills its own records and sweep.combine sums over the ranks."""
        return np.zeros((len(self.depths), len(self.model.tools)) + tail)


class _Windowing:
    """Stage 2: the part of the model a batch sees."""

    def __init__(self, plan):
        self.plan, fm = plan, plan.model.formation_model
        self.formation_h, self.formation_v, self.formation_ids = fm[:, :5], plan.model._vertical_formation_model(), geometry.entry_id_table(fm)
        self.ti_table = fm.shape[1] >= 6 and bool(np.any(~np.isnan(fm[:, 5])))

    def _of(self, formation, bi):
        p = self.plan
        if p.netgen_path:   # the reference's default 2D windowing (remo3d.py:776-779, worker.py:94)
            return geometry.select_netgen_data_range(p.borehole_geometry, formation, p.mud[bi], p.simulation_depths[bi], p.domain_radius)
        # Gmsh-path windowing (worker.py:84), the only one for dipping models
        return geometry.select_data_range(p.borehole_geometry, formation, p.window_dip, p.mud[bi], p.simulation_depths[bi], p.domain_radius)

    def window(self, bi):
        """(geometry, borehole, sigma): sigma is 1-D as in the reference unless a material of the window is anisotropic; then
        [n_mat, dim, dim] TI tensors.  The vertical conductivities come from windowing the RVUZ copy of the table the same way,
        so that every quirk of the windowing (e.g. a dropped flushed zone: the layer takes RTFZ) applies to both alike."""
        fg, bh, sigma = self._of(self.formation_h, bi)
        if self.formation_v is None:
            return fg, bh, sigma
        sigma_v = self._of(self.formation_v, bi)[2]
        if len(sigma_v) != len(sigma):
            raise RuntimeError("windowing of RTUZ and RVUZ gave different materials")
        if np.array_equal(np.asarray(sigma_v), np.asarray(sigma)):
            return fg, bh, sigma
        return fg, bh, geometry.ti_conductivity(sigma, sigma_v, self.plan.window_dip, self.plan.dim)

    def entries(self, bi, sigma):
        """For the layer sensitivities: (the table entry behind every material - the identifier table through the same windowing -,
        sigma as TI tensors when the table has an RVUZ: dRa/dRTUZ and dRa/dRVUZ apart need the tensor derivative, also where the
        window is isotropic)."""
        entries = geometry.material_entries(self._of(self.formation_ids, bi)[2])
        if len(entries) != len(sigma):
            raise RuntimeError("windowing of the entry identifiers gave different materials")
        if self.ti_table and np.ndim(sigma) == 1:
            sigma = geometry.ti_conductivity(sigma, sigma, self.plan.window_dip, self.plan.dim)
        return entries, sigma


class _MeshAhead:
    """Stage 3: which batches this rank takes - its block-cyclic share ("static"), or whatever it draws from the shared counter while
    it is free ("dynamic", the reference's pull scheduling, remo3d.py:843-860; sweep.BatchQueue) - and their meshes.  mesh_workers > 0:
    the default mesher runs ahead of the solver in that many spawned processes (the reference meshes inside its MPI workers, i.e. in
    parallel too: worker.py:84-97), on batches drawn ahead: the whole share at once when it is fixed anyway, a few (they are OWNED once
    drawn) under the pull schedule."""

    def __init__(self, plan, windowing, bq, schedule, mesh_workers, cache=None):
        self.plan, self.windowing, self.bq, self.schedule = plan, windowing, bq, schedule
        self.pool, self.pending, self.ahead = None, {}, collections.deque()
        self.cache = cache      # inversion.SweepCache (simulate_logs(reuse=...)): the meshes of an earlier sweep of the same geometry
        if cache is not None and cache.keep_meshes and cache.meshes and all(cache.has_mesh(bi) for bi in sweep.my_share(len(plan.batches))):
            mesh_workers = 0    # nothing to mesh: no worker pool
        if mesh_workers is None:    # default: the reference's cpu_workers mesh (and solve) in parallel; here they mesh, for sweeps long
            mesh_workers = min(int(plan.model.cpu_workers or 0), 8) if (plan.default_provider and plan.share_len >= 16) else 0   # enough to pay for the start-up
        if mesh_workers > 0 and plan.default_provider and plan.share_len > 1:
            self.pool = self._start_pool(int(mesh_workers), plan.mesh_scale)
        self.depth = 1 if self.pool is None else (plan.share_len if schedule == "static" else int(mesh_workers) + len(plan.contexts))
        self.draw, self.lock = iter(bq), threading.Lock()

    @staticmethod
    def _start_pool(n, mesh_scale):
        main_mod = sys.modules.get("__main__")
        hidden = {}
        try:
            # spawned children re-import the caller's __main__ (and would re-run a script without an
            # `if __name__ == "__main__"` guard, GPU contexts and all): hide its path while the workers start -
            # the worker functions live in this module, nothing of __main__ is needed over there
            for attr in ("__file__", "__spec__"):
                if main_mod is not None and getattr(main_mod, attr, None) is not None:
                    hidden[attr] = getattr(main_mod, attr)
                    setattr(main_mod, attr, None)
            pool = ProcessPoolExecutor(max_workers=n, mp_context=multiprocessing.get_context("spawn"),
                                       initializer=_mesh_worker_init, initargs=(dict(scale=mesh_scale),))
            # the executor starts a process per submit while none is idle: start them ALL here, while __main__ is hidden
            for fut in [pool.submit(time.sleep, 0.25) for _ in range(n)]:
                fut.result()
            return pool
        except Exception:     # no worker processes here: mesh inline
            return None
        finally:
            for attr, v in hidden.items():
                setattr(main_mod, attr, v)

    def next_batch(self):
        p = self.plan
        with self.lock:
            # under the pull schedule a drawn batch is OWNED: near the end of the sweep a rank must not sit on a queue of
            # batches the other ranks are idle for - draw ahead no further than its fair part of what is left
            cap = self.depth if self.schedule == "static" else max(1, min(self.depth, 1 + self.bq.remaining_hint() // (2 * max(1, sweep.world_size()))))
            while len(self.ahead) < cap:
                try:
                    bi = next(self.draw)
                except StopIteration:
                    break
                if self.pool is not None and not (self.cache is not None and self.cache.has_mesh(bi)):
                    try:
                        fg, bh, _ = self.windowing.window(bi)
                        self.pending[bi] = self.pool.submit(_mesh_worker_run, (p.dim, p.domain_radius, p.batches[bi].electrodes, fg, bh, p.mesh_dip, p.eccentricity))
                    except Exception:
                        pass      # reported when the batch's turn comes
                self.ahead.append(bi)
            return self.ahead.popleft() if self.ahead else None

    def mesh(self, bi, fg, bh):
        if self.cache is not None:      # a hit is served without the worker pool; a miss is meshed as ever and kept
            mesh = self.cache.mesh(bi)
            if mesh is None:
                mesh = self._make(bi, fg, bh)
                self.cache.store_mesh(bi, mesh)
            return mesh
        return self._make(bi, fg, bh)

    def _make(self, bi, fg, bh):
        p, mesh = self.plan, None
        if bi in self.pending:
            try:
                mesh = self.pending.pop(bi).result()
            except Exception:     # a worker process died: mesh this batch here
                mesh = None
        return mesh if mesh is not None else p.provider(p.dim, p.domain_radius, p.batches[bi], fg, bh, p.mesh_dip)

    def shutdown(self):
        if self.pool is not None:     # whatever happened in the sweep, the mesh processes do not outlive it
            self.pool.shutdown(wait=False, cancel_futures=True)


def _ra_scale(K, J, dim):
    """Ra = |K J| (/ 2 in 3D, where a half-space is meshed), so dRa = scale * dJ with scale = sign(K J) K (/ 2)."""
    return np.sign(K * J) * K / (2.0 if dim == 3 else 1.0)


class _Output:
    """Stage 4: one thing a sweep produces.  Its slabs (_Plan.slab) are written by several host threads at disjoint (depth, tool)
    rows without a lock.  A new output is a subclass listed in Model.simulate_logs, with store(job) - after the solve: the records of the
    job's batch into the slabs - and publish(model) - the combined slabs as attributes of the model, one array per tool; if it needs more of
    the solver than potentials, also adjoint = True and a prepare."""
    adjoint = False     # needs the functionals of the records and J, dJ of the adjoint solves

    def prepare(self, job):
        """Before the solve: add to the job what this output needs the solver to be given (it may replace job.sigma)."""

    def fail(self, rows):
        for slab in self.slabs:
            for di, ti in rows:
                slab[di, ti] = np.nan

    def combine(self):
        self.slabs = [sweep.combine(slab) for slab in self.slabs]


def _per_tool(model, of):
    return {name: of(i) for i, name in enumerate(model.tools.keys())}


class _Logs(_Output):
    def __init__(self, plan):
        self.plan, self.slabs = plan, [plan.slab()]

    def store(self, job):
        for u, rd in zip(job.outs, job.readers):
            for (di, ti, K, o, m) in rd:
                self.slabs[0][di, ti] = tasks.apparent_resistivity(u[o:o + m], m, K, self.plan.dim)

    def publish(self, model):
        model.logs = _per_tool(model, lambda i: np.vstack([self.plan.depths, self.slabs[0][:, i]]).T)


class _LayerSensitivities(_Output):
    """dRa/dR of every entry of the formation table and dRa/dRm: Ra = |K J| (/ 2 in 3D), dRa/dR = sign(K J) K (/ 2) * dJ/dsigma * (-1 / R^2)."""
    adjoint = True

    def __init__(self, plan, windowing):
        fm = plan.model.formation_model
        self.plan, self.windowing = plan, windowing
        self.slabs = [plan.slab(fm.shape[0], fm.shape[1] - 2), plan.slab()]
        dip = plan.model.dip_rad
        self.ti_normal = np.array([np.sin(dip), 0.0, np.cos(dip)]) if plan.dim == 3 else np.array([0.0, 1.0])   # geometry.ti_conductivity

    def prepare(self, job):
        job.entries, job.sigma = self.windowing.entries(job.bi, job.sigma)

    def store(self, job):
        p = self.plan
        for j, (di, ti, K) in enumerate(job.fun_readers):
            self.slabs[0][di, ti], dmud = geometry.resistivity_sensitivity(job.dJ[j], job.entries, p.model.formation_model,
                                                                           _ra_scale(K, job.J[j], p.dim), self.ti_normal)
            self.slabs[1][di, ti] = dmud * (-1.0 / p.mud[job.bi] ** 2)

    def publish(self, model):
        model.sensitivities = _per_tool(model, lambda i: self.slabs[0][:, i])
        model.mud_sensitivity = _per_tool(model, lambda i: self.slabs[1][:, i])


class _Maps(_Output):
    """d ln Ra / d ln R of every cell of the grid - every sigma inside it scaled by 1 / s, d sigma / d ln s = -sigma - and of the
    rest pseudo-cell, the last entry of a record."""
    adjoint = True

    def __init__(self, plan, grid):
        self.plan, self.grid = plan, grid
        self.lateral = "x" if "x" in grid else "r"
        self.n_cells = (len(grid["z"]) - 1) * (len(grid[self.lateral]) - 1)
        self.slabs = [plan.slab(self.n_cells + 1)]

    def prepare(self, job):
        job.groups, job.group_mat, job.group_cell = geometry.sensitivity_cells(job.mesh, None, self.grid, self.plan.simulation_depths[job.bi])

    def store(self, job):
        half = 2.0 if self.plan.dim == 3 else 1.0
        sig = np.asarray(job.sigma, dtype=float)
        for j, (di, ti, K) in enumerate(job.fun_readers):
            Ra = abs(K * job.J[j]) / half
            w = sig[job.group_mat] * job.dJg[j] if sig.ndim == 1 else np.sum(sig[job.group_mat] * job.dJg[j], axis=(1, 2))
            self.slabs[0][di, ti] = -(_ra_scale(K, job.J[j], self.plan.dim) / Ra) * np.bincount(job.group_cell, weights=w, minlength=self.n_cells + 1)

    def publish(self, model):
        n = self.n_cells
        shape = (len(self.plan.depths), len(self.grid["z"]) - 1, len(self.grid[self.lateral]) - 1)
        model.sensitivity_maps = _per_tool(model, lambda i: self.slabs[0][:, i, :n].reshape(shape))
        model.sensitivity_map_rest = _per_tool(model, lambda i: self.slabs[0][:, i, n])
        model.sensitivity_grid = {k: np.asarray(v, dtype=float) for k, v in self.grid.items()}


class _ErrorEstimates(_Output):
    """The estimated relative discretisation error E / |J| of every reading (remo_job_error_t: the facet jumps of the forward and the
    adjoint solution, element by element) and, with a grid, the share of E made in every cell and in the rest pseudo-cell."""
    adjoint = True

    def __init__(self, plan, grid):
        self.plan, self.grid = plan, grid
        self.slabs = [plan.slab()]
        if grid is not None:
            self.lateral = "x" if "x" in grid else "r"
            self.n_cells = (len(grid["z"]) - 1) * (len(grid[self.lateral]) - 1)
            self.slabs.append(plan.slab(self.n_cells + 1))

    def prepare(self, job):
        job.error = True
        if self.grid is not None:     # one group per cell: an element belongs to the cell of geometry.sensitivity_cells, whatever its material
            group, _, group_cell = geometry.sensitivity_cells(job.mesh, None, self.grid, self.plan.simulation_depths[job.bi])
            job.error = dict(n_group=self.n_cells + 1, group=np.asarray(group_cell)[group].astype(np.int32))

    def store(self, job):
        for j, (di, ti, K) in enumerate(job.fun_readers):
            Jj, E = job.J[j], job.E[j]
            self.slabs[0][di, ti] = E / abs(Jj) if Jj != 0 else np.nan
            if self.grid is not None:
                self.slabs[1][di, ti] = job.Eg[j] / E if E != 0 else np.nan

    def publish(self, model):
        model.error_estimates = _per_tool(model, lambda i: self.slabs[0][:, i])
        if self.grid is not None:
            n = self.n_cells
            shape = (len(self.plan.depths), len(self.grid["z"]) - 1, len(self.grid[self.lateral]) - 1)
            model.error_maps = _per_tool(model, lambda i: self.slabs[1][:, i, :n].reshape(shape))
            model.error_map_rest = _per_tool(model, lambda i: self.slabs[1][:, i, n])
            model.error_grid = {k: np.asarray(v, dtype=float) for k, v in self.grid.items()}


class _FieldSections(_Output):
    """The potential and the current density of the right-hand side behind a record - the electrode configuration actually
    energised - on a section grid of points: physical values (3D: the half-space FE field halved, as tasks.apparent_resistivity
    halves its potentials).  Only the records of the kept measurement depths are stored; a batch that holds none takes the plain
    solver entry."""
    MAX_SOURCES = 4     # point sources of one right-hand side

    def __init__(self, plan, grid, depths):
        self.plan, self.grid = plan, grid
        self.lateral = "x" if "x" in grid else "r"
        geometry.field_points(grid, plan.dim, 0.0)     # a malformed grid fails here, before any batch is drawn
        kept = np.arange(len(plan.depths)) if depths is None else np.asarray(depths, dtype=int).ravel()
        if kept.size != np.unique(kept).size or np.any(kept < 0) or np.any(kept >= len(plan.depths)):
            raise ValueError("field_depths must be distinct indices into measurement_depths")
        self.kept, self.slot = kept, {int(d): i for i, d in enumerate(kept)}
        self.n_z, self.n_h = len(grid["z"]), len(grid[self.lateral])
        n_tools, n_pts = len(plan.model.tools), self.n_z * self.n_h
        self.slabs = [np.zeros((kept.size, n_tools, n_pts)), np.zeros((kept.size, n_tools, n_pts, plan.dim)),
                      np.zeros((kept.size, n_tools, 1 + 2 * self.MAX_SOURCES))]

    def prepare(self, job):
        solves = self.plan.batches[job.bi].solves
        rhs = [k for k, s in enumerate(solves) if any(r.depth_index in self.slot for r in s.records)]
        if rhs:
            job.field_rhs = rhs
            job.field_points = geometry.field_points(self.grid, self.plan.dim, self.plan.simulation_depths[job.bi])

    def store(self, job):
        if job.field_rhs is None:
            return
        half = 0.5 if self.plan.dim == 3 else 1.0
        for j, k in enumerate(job.field_rhs):
            z, I = job.sources[k]
            z = np.asarray(z, dtype=float)
            z = z[:, -1] if z.ndim == 2 else z      # an eccentred tool: points (e, 0, z); x is the plan's eccentricity for all
            if len(z) > self.MAX_SOURCES:
                raise ValueError("a right-hand side with more than {} point sources".format(self.MAX_SOURCES))
            src = np.zeros(1 + 2 * self.MAX_SOURCES)
            src[0] = len(z)
            src[1:1 + len(z)] = np.asarray(z) + self.plan.simulation_depths[job.bi]
            src[1 + self.MAX_SOURCES:1 + self.MAX_SOURCES + len(z)] = I
            for (di, ti, K, o, m) in job.readers[k]:
                if di in self.slot:
                    i = self.slot[di]
                    self.slabs[0][i, ti] = half * job.field["u"][j]
                    self.slabs[1][i, ti] = half * job.field["J"][j]
                    self.slabs[2][i, ti] = src

    def fail(self, rows):
        for slab in self.slabs:
            for di, ti in rows:
                if di in self.slot:
                    slab[self.slot[di], ti] = np.nan

    def publish(self, model):
        shape = (self.kept.size, self.n_z, self.n_h)
        model.field_sections = _per_tool(model, lambda i: dict(u=self.slabs[0][:, i].reshape(shape), J=self.slabs[1][:, i].reshape(shape + (self.plan.dim,))))

        def sources(i):
            out = []
            for rec in self.slabs[2][:, i]:
                n = 0 if np.isnan(rec[0]) else int(rec[0])
                out.append((rec[1:1 + n].copy(), rec[1 + self.MAX_SOURCES:1 + self.MAX_SOURCES + n].copy()))
            return out
        model.field_sources = _per_tool(model, sources)
        model.field_source_x = _per_tool(model, lambda i: [np.full(len(zs), self.plan.eccentricity) for zs, _ in sources(i)])
        model.field_grid = {k: np.asarray(v, dtype=float) for k, v in self.grid.items()}
        model.field_depth_index = self.kept.copy()


class _BatchRunner:
    """Stages 5 and 6: one batch from its window to every output, and the host threads that do so batch after batch."""

    def __init__(self, plan, windowing, meshes, outputs, cache=None):
        self.plan, self.windowing, self.meshes, self.outputs, self.cache = plan, windowing, meshes, outputs, cache
        self.free_ctx = queue.Queue()
        for c in plan.contexts:
            self.free_ctx.put(c)
        self.acc = dict(mesh=0.0, solve=0.0, points=0, failed_batches=0, not_converged=0, first_error=None, pcg_steps=0, programming_error=None)
        self.lock = threading.Lock()     # of acc

    def run_batch(self, bi):
        p, acc = self.plan, self.acc
        batch = p.batches[bi]
        try:
            t0 = time.time()
            fg, bh, sigma = self.windowing.window(bi)
            job = types.SimpleNamespace(bi=bi, sigma=sigma, mesh=self.meshes.mesh(bi, fg, bh), groups=None, functionals=None,
                                        field_rhs=None, field_points=None, error=None)
            sources, evals, job.readers = tasks.batch_rhs(batch, p.model.tools, p.eccentricity)
            job.sources = sources
            t1 = time.time()
            opts = p.batch_opts(job.mesh)
            if any(o.adjoint for o in self.outputs):
                job.functionals, job.fun_readers = tasks.batch_functionals(batch, p.model.tools, p.eccentricity)
            for o in self.outputs:
                o.prepare(job)
            est = {} if job.error is None else dict(error=job.error)     # the keyword only where an output asked for it

            def adjoint(res, *names):     # (potentials, J, dJ, [dJg,] [E, [Eg],] stats, rc) of the adjoint entries into the job
                for name, value in zip(names, res):
                    setattr(job, name, value)
                job.E, job.Eg = (tuple(res[len(names):-2]) + (None, None))[:2]
                return res[-2], res[-1]
            c = self.free_ctx.get()
            try:     # the solver entry follows from what the outputs asked for
                if job.groups is not None:
                    st, rc = adjoint(c.solve_batch_sens_groups(job.mesh, job.sigma, sources, evals, job.functionals, job.groups, len(job.group_mat), opts, **est),
                                     "outs", "J", "dJ", "dJg")
                elif job.functionals is not None:
                    warm = self.cache.warm_state(bi) if self.cache is not None else None      # the batch's solutions of the previous sweep
                    if warm is not None:
                        try:
                            st, rc = adjoint(c.solve_batch_sens(job.mesh, job.sigma, sources, evals, job.functionals, opts, warm=warm, **est), "outs", "J", "dJ")
                        finally:
                            self.cache.after_solve(bi, warm)
                    else:
                        st, rc = adjoint(c.solve_batch_sens(job.mesh, job.sigma, sources, evals, job.functionals, opts, **est), "outs", "J", "dJ")
                elif job.field_rhs is not None:
                    job.outs, job.field, st, rc = c.solve_batch_field(job.mesh, job.sigma, sources, evals, job.field_points, job.field_rhs, opts)
                elif p.secondary is not None:
                    job.outs, st, rc = c.solve_batch(job.mesh, job.sigma, sources, evals, opts, secondary=p.secondary)
                else:
                    job.outs, st, rc = c.solve_batch(job.mesh, job.sigma, sources, evals, opts)
            finally:
                self.free_ctx.put(c)
            t2 = time.time()
            for o in self.outputs:
                o.store(job)
            n = sum(len(rd) for _, rd in zip(job.outs, job.readers))
            with self.lock:
                acc["mesh"] += t1 - t0; acc["solve"] += t2 - t1; acc["points"] += n
                acc["not_converged"] += int(rc == solver.REMO_NOT_CONVERGED); acc["pcg_steps"] += int(st.get("pcg_steps", 0))
        except Exception as ex:
            rows = [(r.depth_index, r.tool_index) for s in batch.solves for r in s.records]
            for o in self.outputs:      # any failure in a batch -> NaN for its records (worker.py:135-138: a bare except)
                o.fail(rows)
            with self.lock:             # ... but not silently: the reference's worker at least shows it on stderr
                acc["failed_batches"] += 1
                if acc["first_error"] is None:
                    acc["first_error"] = "batch {}: {}: {}".format(bi, type(ex).__name__, ex)
                # a programming error (e.g. in a custom mesh_provider) is recorded like any other failure HERE - a rank that
                # raised now would miss the collectives of the report and leave the other ranks waiting in the all-reduce - and is
                # raised once they are through
                if isinstance(ex, (TypeError, AttributeError, NameError)) and acc["programming_error"] is None:
                    acc["programming_error"] = ex

    def _drive(self):
        for bi in iter(self.meshes.next_batch, None):
            self.run_batch(bi)

    def drive(self):
        """One host thread per context (ctypes calls release the GIL) when there is more than one of both, contexts and batches."""
        n = len(self.plan.contexts)
        if n > 1 and self.plan.share_len > 1:
            with ThreadPoolExecutor(max_workers=n) as tp:
                for fut in [tp.submit(self._drive) for _ in range(n)]:
                    fut.result()
        else:
            self._drive()


# -- the stages of Model.simulate_array_logs: a plan, outputs and a batch of their own; windowing, meshes and threads are the tools' ----
class _ArrayPlan(_Plan):
    """Stage 1 for an electrode array (arrays.ElectrodeArray): batches of consecutive depths; slabs per (depth, mode)."""

    def __init__(self, model, array, sensitivities, *args):
        self.array, self.sensitivities = array, bool(sensitivities)
        super().__init__(model, *args)

    def _reaches(self):
        a = self.array
        return [float(np.max(np.abs(a.offsets - np.mean(a.offsets[a.current_electrodes]))))]

    def _draw_batches(self, batch_size):
        return arrays.build_batches(self.array, self.depths, batch_size)

    def slab(self, *tail):
        return np.zeros((len(self.depths), len(self.array.modes)) + tail)


class _ArrayOutput(_Output):
    def fail(self, rows):
        for slab in self.slabs:
            for di, _ in rows:
                slab[di] = np.nan


class _ArrayLogs(_ArrayOutput):
    """Ra and the currents of every mode, and the impedances they were formed from (physical values; NaN where not measured)."""

    def __init__(self, plan):
        m = len(plan.array.names)
        self.plan, self.slabs = plan, [plan.slab(), plan.slab(m), np.zeros((len(plan.depths), m, m))]

    def store(self, job):
        for di, Z in zip(job.depth_index, job.Z):
            self.slabs[2][di] = Z
            for k, mode in enumerate(self.plan.array.modes):
                self.slabs[0][di, k], self.slabs[1][di, k], _ = self.plan.array.apparent_resistivity(mode, Z)

    def publish(self, model):
        modes = list(self.plan.array.modes)
        model.array = self.plan.array
        model.array_logs = {mode: np.vstack([self.plan.depths, self.slabs[0][:, k]]).T for k, mode in enumerate(modes)}
        model.array_currents = {mode: self.slabs[1][:, k] for k, mode in enumerate(modes)}
        model.array_impedances = self.slabs[2]


class _ArraySensitivities(_ArrayOutput):
    """dRa/dR of every table entry and dRa/dRm per mode: dy = sum_ij w_hat_i I_j dZ_ij (arrays.focus) with dZ_ij the pair derivative of
    the right-hand sides of electrodes i and j, Ra = |K y / I0|; the table entries through geometry.resistivity_sensitivity as for the tools."""

    def __init__(self, plan, windowing):
        fm = plan.model.formation_model
        self.plan, self.windowing = plan, windowing
        self.slabs = [plan.slab(fm.shape[0], fm.shape[1] - 2), plan.slab()]
        dip = plan.model.dip_rad
        self.ti_normal = np.array([np.sin(dip), 0.0, np.cos(dip)]) if plan.dim == 3 else np.array([0.0, 1.0])   # geometry.ti_conductivity

    def prepare(self, job):
        job.entries, job.sigma = self.windowing.entries(job.bi, job.sigma)

    def store(self, job):
        p = self.plan
        for di, Z, dZ in zip(job.depth_index, job.Z, job.dZ):
            for k, mode in enumerate(p.array.modes):
                mm = p.array.matrices(mode)
                I, _, y, w_hat = arrays.focus(Z, mm)
                G = sum(w_hat[i] * I[j] * d for (i, j), d in dZ.items() if w_hat[i] != 0.0 and I[j] != 0.0)
                scale = np.sign(mm.K * y / mm.I0) * mm.K / mm.I0
                self.slabs[0][di, k], dmud = geometry.resistivity_sensitivity(G, job.entries, p.model.formation_model, scale, self.ti_normal)
                self.slabs[1][di, k] = dmud * (-1.0 / p.mud[job.bi] ** 2)

    def publish(self, model):
        modes = list(self.plan.array.modes)
        model.array_sensitivities = {mode: self.slabs[0][:, k] for k, mode in enumerate(modes)}
        model.array_mud_sensitivity = {mode: self.slabs[1][:, k] for k, mode in enumerate(modes)}


class _ArrayMaps(_ArrayOutput):
    """d ln Ra / d ln R per mode of every cell of the grid and of the rest pseudo-cell, as _Maps forms them for the tools: per group of
    elements Gg = sum_ij w_hat_i I_j dZg_ij (arrays.focus; dZg the pair derivatives per group), the cell value
    -(scale / Ra) * sum over the groups of the cell of sigma_g * Gg (tensors: sigma : Gg) with scale = sign(K y / I0) K / I0."""

    @staticmethod
    def lateral_axis(grid):
        """'r' or 'x' of a well-formed grid (geometry.sensitivity_cells' rules; Model.simulate_array_logs asks before any batch is drawn)."""
        lateral = [k for k in ("r", "x") if k in grid] if isinstance(grid, dict) else []
        if len(lateral) != 1 or "z" not in grid:
            raise ValueError("sensitivity_grid must hold the edges of 'z' and of one of 'r' and 'x'")
        for e in (grid["z"], grid[lateral[0]]):
            if np.ndim(e) != 1 or len(e) < 2 or np.any(np.diff(np.asarray(e, dtype=float)) <= 0):
                raise ValueError("sensitivity_grid edges must be increasing, two at least")
        return lateral[0]

    def __init__(self, plan, grid):
        self.plan, self.grid, self.lateral = plan, grid, self.lateral_axis(grid)
        if self.lateral == "x" and plan.dim != 3:
            raise ValueError("the 'x' axis exists in 3D only")
        self.n_cells = (len(grid["z"]) - 1) * (len(grid[self.lateral]) - 1)
        self.slabs = [plan.slab(self.n_cells + 1)]

    def prepare(self, job):
        job.groups, job.group_mat, job.group_cell = geometry.sensitivity_cells(job.mesh, None, self.grid, self.plan.simulation_depths[job.bi])

    def store(self, job):
        p = self.plan
        sig = np.asarray(job.sigma, dtype=float)[job.group_mat]
        for di, Z, dZg in zip(job.depth_index, job.Z, job.dZg):
            for k, mode in enumerate(p.array.modes):
                mm = p.array.matrices(mode)
                I, _, y, w_hat = arrays.focus(Z, mm)
                Gg = sum(w_hat[i] * I[j] * d for (i, j), d in dZg.items() if w_hat[i] != 0.0 and I[j] != 0.0)
                Ra = abs(mm.K * y / mm.I0)
                scale = np.sign(mm.K * y / mm.I0) * mm.K / mm.I0
                w = sig * Gg if sig.ndim == 1 else np.sum(sig * Gg, axis=(1, 2))
                self.slabs[0][di, k] = -(scale / Ra) * np.bincount(job.group_cell, weights=w, minlength=self.n_cells + 1)

    def publish(self, model):
        n, modes = self.n_cells, list(self.plan.array.modes)
        shape = (len(self.plan.depths), len(self.grid["z"]) - 1, len(self.grid[self.lateral]) - 1)
        model.array_sensitivity_maps = {mode: self.slabs[0][:, k, :n].reshape(shape) for k, mode in enumerate(modes)}
        model.array_sensitivity_map_rest = {mode: self.slabs[0][:, k, n] for k, mode in enumerate(modes)}
        model.sensitivity_grid = {k: np.asarray(v, dtype=float) for k, v in self.grid.items()}


class _ArrayRunner(_BatchRunner):
    """Stage 5 for an array: per depth of the batch one right-hand side of unit current per electrode that some mode makes carry
    current - with sensitivities also per read / null electrode: by reciprocity their solutions are the adjoint ones - each read at all
    other electrodes of its depth; the pairs (read / null electrode, current electrode) give dZ (Context.solve_batch_pairs), and with
    the groups an output asked for (_ArrayMaps) also dZg per group of elements."""

    def run_batch(self, bi):
        p, acc = self.plan, self.acc
        batch, arr = p.batches[bi], p.array
        try:
            t0 = time.time()
            fg, bh, sigma = self.windowing.window(bi)
            job = types.SimpleNamespace(bi=bi, sigma=sigma, mesh=self.meshes.mesh(bi, fg, bh), depth_index=[s.records[0].depth_index for s in batch.solves],
                                        groups=None)
            m = len(arr.names)
            cur, pot = np.flatnonzero(arr.current_electrodes), np.flatnonzero(arr.potential_electrodes)
            active = sorted(set(cur) | (set(pot) if p.sensitivities else set()))
            sources, evals, rhs_of = [], [], {}
            for s, solve in enumerate(batch.solves):
                z = solve.electrodes[0]
                for i in active:
                    rhs_of[(s, i)] = len(sources)
                    sources.append((np.array([z[i]]), np.array([1.0])))
                    evals.append(np.array([z[k] for k in range(m) if k != i]))
            t1 = time.time()
            opts = p.batch_opts(job.mesh)
            for o in self.outputs:
                o.prepare(job)
            pairs = [(rhs_of[(s, i)], rhs_of[(s, j)]) for s in range(len(batch.solves)) for i in pot for j in cur] if p.sensitivities else []
            c = self.free_ctx.get()
            try:      # an array reads potentials, not differences: against infinity, not against the grounded surface of the batch mesh
                if job.groups is not None:
                    outs, dP, dPg, st, rc = c.solve_batch_pairs(job.mesh, job.sigma, sources, evals, pairs, opts, far_field=float(p.domain_radius),
                                                                groups=job.groups, n_group=len(job.group_mat))
                else:
                    outs, dP, st, rc = c.solve_batch_pairs(job.mesh, job.sigma, sources, evals, pairs, opts, far_field=float(p.domain_radius))
            finally:
                self.free_ctx.put(c)
            t2 = time.time()
            half = 0.5 if p.dim == 3 else 1.0      # the half ball with its sources in the symmetry plane: the potentials of 2 I
            job.Z, job.dZ, job.dZg = [], [], []
            for s in range(len(batch.solves)):
                Z = np.full((m, m), np.nan)
                for i in active:
                    Z[[k for k in range(m) if k != i], i] = half * np.asarray(outs[rhs_of[(s, i)]])
                job.Z.append(Z)
                job.dZ.append({(i, j): half * dP[pairs.index((rhs_of[(s, i)], rhs_of[(s, j)]))] for i in pot for j in cur} if pairs else {})
                if job.groups is not None:
                    job.dZg.append({(i, j): half * dPg[pairs.index((rhs_of[(s, i)], rhs_of[(s, j)]))] for i in pot for j in cur})
            for o in self.outputs:
                o.store(job)
            with self.lock:
                acc["mesh"] += t1 - t0; acc["solve"] += t2 - t1; acc["points"] += len(batch.solves) * len(arr.modes)
                acc["not_converged"] += int(rc == solver.REMO_NOT_CONVERGED); acc["pcg_steps"] += int(st.get("pcg_steps", 0))
        except Exception as ex:
            for o in self.outputs:      # any failure in a batch -> NaN for its depths
                o.fail([(r.depth_index, r.tool_index) for s in batch.solves for r in s.records])
            with self.lock:
                acc["failed_batches"] += 1
                if acc["first_error"] is None:
                    acc["first_error"] = "batch {}: {}: {}".format(bi, type(ex).__name__, ex)
                if isinstance(ex, (TypeError, AttributeError, NameError)) and acc["programming_error"] is None:
                    acc["programming_error"] = ex


class Model:
    conversion_table = CONVERSION

    def __init__(self, tools, force_single_electrode_configuration=True):
        self.tools, self.sec = self.set_tools_parameters(tools, force_single_electrode_configuration=force_single_electrode_configuration)
        self.formation_model = None
        self.borehole_model = None
        self.dip_deg = None
        self.dip_rad = None
        self.cpu_workers = None
        self.gpu_workers = None
        self.ctx = None
        self.extra_ctx = []
        self.logs = None
        self.sensitivities = None      # simulate_logs(sensitivities=True): per tool dRa/dR [n_depths, n_layers, n_cols]
        self.mud_sensitivity = None    # ... and dRa/dRm [n_depths]
        self.sensitivity_maps = None   # simulate_logs(sensitivity_grid=...): per tool d ln Ra / d ln R of every grid cell [n_depths, n_z, n_r]
        self.sensitivity_map_rest = None   # ... and of everything outside the grid [n_depths]
        self.sensitivity_grid = None   # the grid of the last maps
        self.field_sections = None     # simulate_logs(field_grid=...): per tool dict(u [n_kept, n_z, n_h] in V, J [n_kept, n_z, n_h, dim] in A/m2)
        self.field_sources = None      # ... per tool and kept record the energised point sources (absolute z, I)
        self.field_source_x = None     # ... and their x in the mesh frame (the eccentricity of the sweep; 0 for a centred tool)
        self.error_estimates = None    # simulate_logs(error_estimate=True): per tool the estimated relative error of the apparent resistivity [n_depths]
        self.error_maps = None         # simulate_logs(error_grid=...): per tool the share of that estimate made in every grid cell [n_depths, n_z, n_r]
        self.error_map_rest = None     # ... and outside the grid [n_depths]; the cells and the rest sum to 1
        self.error_grid = None         # the grid of the last error maps
        self.formulation = None        # "primary" or "secondary": how the last sweep treated the point sources (simulate_logs)
        self.eccentricity = None       # the displacement of the tool from the borehole axis in the last sweep, metres along x
        self.field_grid = None         # the grid of the last sections
        self.field_depth_index = None  # ... and the indices into measurement_depths they were kept for
        self.inversion = None          # invert_logs: what the last inversion found (inversion.invert_model)
        self.array = None              # simulate_array_logs: the arrays.ElectrodeArray of the last array sweep
        self.array_logs = None         # ... per mode [n_depths, 2] (depth, Ra)
        self.array_currents = None     # ... per mode the electrode currents [n_depths, m]
        self.array_impedances = None   # ... the transfer impedances [n_depths, m, m] in V / A, NaN where not measured
        self.array_sensitivities = None    # simulate_array_logs(sensitivities=True): per mode dRa/dR [n_depths, n_layers, n_cols]
        self.array_mud_sensitivity = None  # ... and dRa/dRm [n_depths]
        self.array_sensitivity_maps = None      # simulate_array_logs(sensitivity_grid=...): per mode d ln Ra / d ln R of every grid cell [n_depths, n_z, n_r]
        self.array_sensitivity_map_rest = None  # ... and of everything outside the grid [n_depths]; the grid is self.sensitivity_grid
        self.timing = {}

    # -- complete procedure (remo3d.py:65-174) ---------------------------------------------------
    @classmethod
    def compute_synthetic_logs(cls, tools, measurement_depths, formation_model, borehole_model,
                               force_single_electrode_configuration=True, formation_units=["M", "M", "M"],
                               borehole_geometry_type="diameter", borehole_units=["M", "M"], dip=0, cpu_workers=4,
                               gpu_workers=0, domain_radius=50, batch_size=5, mesh_generator="auto",
                               preconditioner="multigrid", condense=True, **extensions):
        model = cls(tools, force_single_electrode_configuration=force_single_electrode_configuration)
        model.set_model_parameters(formation_model, borehole_model, borehole_geometry_type=borehole_geometry_type, dip=dip)
        model.initialize_workers(cpu_workers=cpu_workers, gpu_workers=gpu_workers)
        model.simulate_logs(measurement_depths, domain_radius=domain_radius, batch_size=batch_size, mesh_generator=mesh_generator,
                            preconditioner=preconditioner, condense=condense, **extensions)
        model.shutdown_workers()
        return model

    # -- tools (remo3d.py:178-321) ---------------------------------------------------------------
    def set_tools_parameters(self, tools, force_single_electrode_configuration=True):
        return tools_mod.tool_tables(tools, force_single_electrode_configuration)

    # -- model (remo3d.py:344-548) ---------------------------------------------------------------
    def set_model_parameters(self, formation_model, borehole_model, borehole_geometry_type="diameter", dip=0):
        """Formation and borehole model from table files (paths) or from arrays in metres (remo3d.py:344-377: same argument
        meaning; an argument of any other type is ignored there and is a TypeError here)."""
        def model_from(source, from_file, from_array, what):
            if isinstance(source, (str, os.PathLike)):
                return from_file(os.fspath(source))
            if isinstance(source, np.ndarray):
                return from_array(source)
            raise TypeError("{} model has to be a file name or a numpy array, not {}".format(what, type(source).__name__))
        self.formation_model = model_from(formation_model, self.load_formation_parameters, self.set_formation_parameters, "formation")
        self.borehole_model = model_from(borehole_model, lambda f: self.load_borehole_parameters(f, borehole_geometry_type),
                                         lambda a: self.set_borehole_parameters(a, borehole_geometry_type), "borehole")
        self.dip_deg, self.dip_rad = self.set_dip(dip)
        self._check_model_geometry()

    @staticmethod
    def _read_table(path):
        """Tab-separated table with a name row and a unit row (remo3d.py:395-398, 459-462)."""
        with open(path) as f:
            lines = f.read().splitlines()
        units = lines[1].split()
        rows = [ln.split("\t") for ln in lines[2:] if ln.strip()]
        data = np.array([[float(v) for v in r if v.strip() != ""] for r in rows], dtype=float)
        return np.atleast_2d(data), units

    def load_formation_parameters(self, formation_model_file):
        data, units = self._read_table(formation_model_file)
        return self.set_formation_parameters(data, units[:3])     # the geometry columns; resistivities (2 or 3 columns) are in ohm m

    def set_formation_parameters(self, formation_parameters, formation_units=["M", "M", "M"]):
        fp = np.array(formation_parameters, dtype=float)   # a copy (the reference converts the caller's array in place, remo3d.py:427)
        for i, u in enumerate(formation_units):
            if u not in CONVERSION:
                raise ValueError("{} unit in formation model file not recognized. Allowed units: M, DM, CM, MM, IN, FT".format(u))
            fp[:, i] *= CONVERSION[u]
        if (np.diff(fp[:, :2], axis=0) <= 0.0).any() or (fp[1:, 0] != fp[:-1, 1]).any():
            raise ValueError("Uncorrect formation model geometry")
        if np.nanmin(fp[:, [3, 4]]) <= 0.0:
            raise ValueError("Formation resistivies have to be higher than 0 ohmm")
        if fp.shape[1] > 6:
            raise ValueError("Formation model has at most 6 columns: TOP, BOTTOM, RDFZ, RTFZ, RTUZ and RVUZ")
        if fp.shape[1] == 6:     # RVUZ: vertical resistivity of the undisturbed zone (RTUZ is then the horizontal one); NaN = isotropic
            rv = fp[:, 5]
            if np.any(rv[~np.isnan(rv)] <= 0.0):
                raise ValueError("Vertical resistivities (RVUZ) have to be higher than 0 ohmm")
        return fp

    def _vertical_formation_model(self):
        """The 5-column formation table with RTUZ replaced by RVUZ (NaN -> RTUZ), or None when the model is isotropic (no RVUZ
        column, or RVUZ equal to RTUZ wherever it is given).  Windowed like the model itself, it gives the vertical conductivity
        of every material in the same order (simulate_logs)."""
        fm = self.formation_model
        if fm is None or fm.shape[1] < 6:
            return None
        rv = np.where(np.isnan(fm[:, 5]), fm[:, 4], fm[:, 5])
        if np.array_equal(rv, fm[:, 4]):
            return None
        fv = np.array(fm[:, :5], copy=True)
        fv[:, 4] = rv
        return fv

    def load_borehole_parameters(self, borehole_model_file, borehole_geometry_type="diameter"):
        data, units = self._read_table(borehole_model_file)
        return self.set_borehole_parameters(data, borehole_geometry_type=borehole_geometry_type, borehole_units=units[:-1])

    def set_borehole_parameters(self, borehole_parameters, borehole_geometry_type="diameter", borehole_units=["M", "M"]):
        bp = np.array(borehole_parameters, dtype=float)   # a copy: the caller's array is not converted in place
        if np.shape(bp)[0] < 2:
            raise ValueError("Borehole paramaters have to be defined for at least two depths")
        for i, u in enumerate(borehole_units):
            if u not in CONVERSION:
                raise ValueError("{} unit in borehole model file not recognized. Allowed units: M, DM, CM, MM, IN, FT".format(u))
            bp[:, i] *= CONVERSION[u]
        if (np.diff(bp[:, 0], axis=0) <= 0.0).any() or (bp[:, 1] <= 0.0).any():
            raise ValueError("Uncorrect borehole model geometry")
        if borehole_geometry_type == "diameter":
            bp[:, 1] /= 2
        elif borehole_geometry_type != "radius":
            raise ValueError("Uncorrect borehole geometry type - use 'diameter' or 'radius' to specify borehole geometry")
        if np.nanmin(bp[:, 2]) <= 0.0:
            raise ValueError("Drilling mud resistivies have to be higher than 0 ohmm")
        return bp

    def set_dip(self, dip):
        if dip < 0 or dip >= 90:
            raise ValueError("Uncorrect dip angle")
        return dip, dip * np.pi / 180

    def _check_model_geometry(self):
        for i in range(np.shape(self.formation_model)[0]):
            inside = (self.borehole_model[:, 0] >= self.formation_model[i, 0]) & (self.borehole_model[:, 0] <= self.formation_model[i, 1])
            if np.any(self.borehole_model[inside, 1] >= self.formation_model[i, 2]):
                raise ValueError("Borehole radius have to be smaller than the extend of the filtration zone")

    def _add_points_to_borehole(self, maximal_distance=0.15):
        """Densify the borehole polyline for 3D models (remo3d.py:694-720).  Unlike the reference
        (Appendix A of SURVEY.md: unbound variable) an already dense model is returned unchanged."""
        bm = self.borehole_model
        depths = [bm[0, 0]]
        for i in range(1, bm.shape[0]):
            gap = bm[i, 0] - bm[i - 1, 0]
            if gap > maximal_distance:
                depths += list(np.linspace(bm[i - 1, 0], bm[i, 0], np.max([3, int(gap * 10 + 1)]))[1:])
            else:
                depths.append(bm[i, 0])
        depths = np.asarray(depths)
        if depths.shape[0] > bm.shape[0]:
            return np.vstack([depths, np.interp(depths, bm[:, 0], bm[:, 1]), np.interp(depths, bm[:, 0], bm[:, 2])]).T
        return bm

    # -- workers (remo3d.py:552-599, 887-899) ------------------------------------------------------
    def initialize_workers(self, cpu_workers=4, gpu_workers=0, context_factory: Optional[Callable] = None):
        """The reference spawns MPI workers here (remo3d.py:552-599); this build opens GPU contexts in the
        calling process (device = LOCAL_RANK under torchrun): `gpu_workers` of them (0, the default, = DEFAULT_CONTEXTS), each
        with its own HIP stream and arena and driven by its own host thread in simulate_logs, so batches
        overlap on the GPU the way the reference's GPU workers overlap (they fill the launch-latency gaps of
        one another: +40 % in 3D at five, more in 2D).  Parallelism ACROSS GPUs comes from the launcher (one rank per GPU);
        cpu_workers is validated like the reference and sizes the pool of mesh-generating processes (there is no CPU
        solver).  Under torchrun this is also where the rank joins the process group (sweep.init_from_env)."""
        if type(cpu_workers) != int or type(gpu_workers) != int:
            raise ValueError("The number of processes have to be an intager")
        if cpu_workers < 1:
            raise ValueError("Minimal number of cpu workers is 1")
        if gpu_workers < 0:
            raise ValueError("Minimal number of gpu workers is 0")
        self.cpu_workers, self.gpu_workers = cpu_workers, gpu_workers
        # under torchrun (WORLD_SIZE > 1) the ranks share the sweep: join the process group here, as the reference
        # brings its farm up in initialize_workers (remo3d.py:592-599); without it every rank would compute every batch
        sweep.init_from_env()
        self.world_size = sweep.world_size()
        device = int(os.environ.get("REMO_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        make = context_factory or solver.Context     # context_factory(device): a stand-in solver for the CPU tests of the sweep
        self.ctx = make(device)
        # contexts on this GPU: gpu_workers of them (at most MAX_CONTEXTS); the reference's default gpu_workers = 0 means "no GPU worker"
        # there and "the build's default" here: DEFAULT_CONTEXTS - the launch-latency-bound quarter of one batch's PCG step (the
        # chain of small launches on the vertex block) is filled by the other batches' kernels
        n_ctx = DEFAULT_CONTEXTS if gpu_workers == 0 else min(gpu_workers, MAX_CONTEXTS)
        self.extra_ctx = [make(device) for _ in range(n_ctx - 1)]

    def shutdown_workers(self):
        for c in getattr(self, "extra_ctx", []):
            c.close()
        self.extra_ctx = []
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None

    # -- tasks (remo3d.py:602-692) -----------------------------------------------------------------
    def _prepare_simulation_depths_and_tasks(self, measurement_depths, batch_size):
        return tasks.build_batches(self.tools, self.sec, measurement_depths, batch_size)

    # -- the sweep (remo3d.py:723-884 + workers/worker.py:74-142) ----------------------------------
    def simulate_logs(self, measurement_depths, domain_radius=50, batch_size=5, mesh_generator="auto", preconditioner="multigrid",
                      condense=True, mesh_provider: Optional[Callable] = None, mesh_scale: Optional[float] = None, rtol: float = 1e-8,
                      maxsteps: int = 1000, verbose: bool = True, mesh_workers: Optional[int] = None, precision: str = "fp64",
                      schedule: str = "static", solver_options: Optional[dict] = None, sensitivities: bool = False,
                      sensitivity_grid: Optional[dict] = None, reuse=None, field_grid: Optional[dict] = None,
                      field_depths=None, eccentricity: float = 0.0, formulation: str = "primary", error_estimate: bool = False,
                      error_grid: Optional[dict] = None):
        """error_estimate: also fill self.error_estimates[tool] [n_depths] with E / |J| of the record's reading, the estimated relative
        discretisation error of the apparent resistivity on the batch mesh the sweep drew (mesh_scale): the goal-oriented estimate
        from the facet jumps of the normal current density of the forward and the adjoint solution (remo_job_error_t; dimensionless,
        NaN where J = 0 or the batch failed).  Implies the adjoint solves; about what the sensitivities cost.  The constant is the
        conventional one, not a sharp one: DESIGN.md section 3.8 states how the estimate compares with the true error.
        error_grid: dict(r=edges, z=edges[, x=edges]), cells as sensitivity_grid defines them: also fill self.error_maps[tool]
        [n_depths, n_z, n_r] and self.error_map_rest[tool] [n_depths] with the share of the estimate made in every cell and outside the
        grid (they sum to 1) - where a size field should be tightened -, and self.error_grid.  Implies error_estimate.  Both work with
        sensitivities, sensitivity_grid, eccentricity, anisotropic tables and reuse; not with formulation="secondary",
        precision="mixed" or field_grid: a ValueError before any batch is drawn.
        formulation: "primary" (default) - every point source goes into the load vector, as without the keyword - or "secondary":
        every batch is solved for the smooth remainder u_s of u = u_p + u_s, u_p the closed-form potential of the batch's sources in
        homogeneous mud inside a grounded sphere of radius domain_radius (remo_job_secondary_t.secondary; sigma0 is left to the library: the
        conductivity at the source), so the elements around the electrodes no longer resolve a 1 / r singularity.  Works with
        eccentricity, with anisotropic tables and with any mesh_scale; not (yet) with sensitivities, sensitivity_grid, field_grid,
        reuse, precision="mixed" or invert_logs: a ValueError before any batch is drawn.  self.formulation records the choice.
        eccentricity: signed displacement in metres of the WHOLE tool from the borehole axis, along x of the mesh frame - the dip
        plane y = 0.  The bedding planes are z + x tan(dip) = const with z growing downwards (meshgen.layered_material_fn), so a bed
        boundary lies shallower at +x: +x is UP-dip, a negative value moves the tool down-dip; with dip 0 the direction is immaterial.
        A non-zero value selects the 3D model also between flat beds (dim 3, dip exactly 0), sends every batch through
        remo_solve_job with its electrodes at (eccentricity, 0, z), and refines the batch meshes around them; it has to be smaller
        than the smallest borehole radius (the tool is in the mud) and cannot be combined with mesh_generator="netgen".  A
        displacement OUT of the dip plane would break the mirror symmetry in y = 0 that the half-ball model rests on: it is not
        offered.  0.0 (default): the centred tool, exactly as without the keyword.  self.eccentricity records the value.
        solver_options: further keywords of solver.make_opts for every batch (op, coarse, quadrature, assemble, ...).
        sensitivities: also fill self.sensitivities[tool] = dRa/dR in ohm m per ohm m, [n_depths, n_layers, n_cols] with the
        columns of the formation table from column 2 on (RDFZ - a radius, always NaN -, RTFZ, RTUZ, and RVUZ when present; 0 where
        the batch's window does not hold the entry, NaN where the table has NaN or the batch failed), and self.mud_sensitivity[tool]
        = dRa/dRm [n_depths] (Rm: the mud resistivity of the record's batch), by adjoint solves (remo_solve_batch_sens: about twice
        the solves of the plain sweep); fp64 only.
        sensitivity_grid: dict(r=edges, z=edges) in metres (3D also x=edges instead of r; z: absolute depth along the borehole axis;
        geometry.sensitivity_cells): also fill self.sensitivity_maps[tool] [n_depths, n_z, n_r] with the dimensionless
        d ln Ra / d ln R of every cell - every resistivity inside the cell (mud, flushed zones, Rh and Rv alike) scaled by a common
        factor - and self.sensitivity_map_rest[tool] [n_depths] with the same for everything outside the grid (the two sum to 1);
        NaN where the batch failed.  Implies the adjoint solves (remo_solve_batch_sens_groups); may be combined with sensitivities.
        field_grid: dict(r=coordinates, z=coordinates) in metres (3D also x= instead of r: the signed x of the dip plane y = 0; r
        there means x >= 0; z: absolute depth along the borehole axis; geometry.field_points): also fill
        self.field_sections[tool] = dict(u [n_kept, n_z, n_r] in V, J [n_kept, n_z, n_r, dim] in A/m2) with the potential and the
        current density J = -Sigma grad u of the right-hand side the record's reading comes from (remo_solve_batch_field) -
        physical values: in 3D the half-space FE field halved -, self.field_sources[tool] with that right-hand side's point sources
        (absolute z, I) per kept record (with a reciprocal configuration: the electrode actually energised), self.field_grid and
        self.field_depth_index.  NaN outside the batch's mesh and where the batch failed.  field_depths: the indices into
        measurement_depths for which sections are kept (default: all).  fp64 only; not together with sensitivities,
        sensitivity_grid or reuse (there are no field variants of the adjoint entries).
        reuse: an inversion.SweepCache shared by sweeps of one geometry (the iterations of invert_logs): the batch meshes come from it
        after the first sweep, and with sensitivities=True every batch's solves start from its solutions of the previous sweep
        (solver.WarmState); self.timing then also reports mesh_hits and warm_hits.  None (default): nothing is kept."""
        start = time.time()
        if formulation not in ("primary", "secondary"):
            raise ValueError("formulation has to be 'primary' or 'secondary'")
        if formulation == "secondary":
            if sensitivities or sensitivity_grid is not None or field_grid is not None or reuse is not None:
                raise ValueError("formulation='secondary' cannot be combined with sensitivities, sensitivity_grid, field_grid or an inversion's "
                                 "sweeps (reuse, invert_logs): the adjoint and field entries read the finite-element potential alone")
            if precision != "fp64" or (solver_options or {}).get("precision", "fp64") != "fp64":
                raise ValueError("formulation='secondary' is fp64: precision has to be 'fp64'")
        error_estimate = bool(error_estimate) or error_grid is not None
        if error_estimate:
            if formulation == "secondary":
                raise ValueError("error estimates cannot be combined with formulation='secondary': the indicator reads the finite-element potential alone")
            if precision != "fp64" or (solver_options or {}).get("precision", "fp64") != "fp64":
                raise ValueError("error estimates are formed from fp64 solutions: precision has to be 'fp64'")
            if field_grid is not None:
                raise ValueError("error estimates cannot be combined with field_grid: there are no field sections with the adjoint solver entries")
            if error_grid is not None:     # a malformed grid fails here, before any batch is drawn
                lateral = [k for k in ("r", "x") if k in error_grid]
                if len(lateral) != 1 or "z" not in error_grid:
                    raise ValueError("error_grid must hold the edges of 'z' and of one of 'r' and 'x'")
                for e in (error_grid["z"], error_grid[lateral[0]]):
                    if np.ndim(e) != 1 or len(e) < 2 or np.any(np.diff(np.asarray(e, dtype=float)) <= 0):
                        raise ValueError("error_grid edges must be increasing, two at least")
        if field_grid is not None:
            if sensitivities or sensitivity_grid is not None or reuse is not None:
                raise ValueError("field_grid cannot be combined with sensitivities, sensitivity_grid or an inversion's sweeps: "
                                 "there are no field sections with the adjoint solver entries")
            if precision != "fp64" or (solver_options or {}).get("precision", "fp64") != "fp64":
                raise ValueError("field sections are formed from the fp64 solution: precision has to be 'fp64'")
        elif field_depths is not None:
            raise ValueError("field_depths needs a field_grid")
        plan = _Plan(self, measurement_depths, domain_radius, batch_size, mesh_generator, mesh_provider, mesh_scale,
                     dict(preconditioner=preconditioner, condense=condense, rtol=rtol, maxsteps=maxsteps, precision=precision),
                     solver_options, verbose, eccentricity)
        plan.secondary = dict(radius=float(domain_radius)) if formulation == "secondary" else None
        self.eccentricity = plan.eccentricity
        self.formulation = formulation
        windowing = _Windowing(plan)
        outputs = [_Logs(plan)]     # the ONE place where the keywords of the further outputs are looked at
        if sensitivities:
            outputs.append(_LayerSensitivities(plan, windowing))
        if sensitivity_grid is not None:
            outputs.append(_Maps(plan, sensitivity_grid))
        if field_grid is not None:
            outputs.append(_FieldSections(plan, field_grid, field_depths))
        if error_estimate:
            outputs.append(_ErrorEstimates(plan, error_grid))
        bq = sweep.BatchQueue(len(plan.batches), schedule)
        if reuse is not None:
            from . import inversion
            reuse.begin(inversion.sweep_signature(plan))
        meshes = _MeshAhead(plan, windowing, bq, schedule, mesh_workers, reuse)
        runner = _BatchRunner(plan, windowing, meshes, outputs, reuse)

        def reset():
            self.sensitivities = self.mud_sensitivity = self.sensitivity_maps = self.sensitivity_map_rest = self.sensitivity_grid = None
            self.field_sections = self.field_sources = self.field_source_x = self.field_grid = self.field_depth_index = None
            self.error_estimates = self.error_maps = self.error_map_rest = self.error_grid = None
        self._drive_and_report(plan, bq, meshes, runner, outputs, reset, schedule, start, verbose, reuse)

    def _drive_and_report(self, plan, bq, meshes, runner, outputs, reset, schedule, start, verbose, reuse=None):
        """The end of every sweep: the host threads, then - collectives, in this order on every rank - the slabs combined and
        published (reset() clears what an earlier sweep of the same kind published) and self.timing."""
        t_busy = time.time()
        try:
            runner.drive()
        finally:
            meshes.shutdown()
        t_busy = time.time() - t_busy
        # the report.  Collectives, in this order on every rank - also one that drew nothing or whose batches failed
        acc = runner.acc
        bq.check_complete()          # every batch was taken exactly once over the ranks
        for o in outputs:            # the same pattern for every slab: every rank has zeros outside its own records
            o.combine()
        reset()
        for o in outputs:
            o.publish(self)
        self.timing = dict(total_s=time.time() - start, mesh_s=acc["mesh"], solve_s=acc["solve"], points=acc["points"], batches=len(plan.batches),
                           my_batches=len(bq.taken), world_size=sweep.world_size(), schedule=schedule, busy_s=t_busy,
                           busy_s_per_rank=[b[0] for b in sweep.gather_floats([t_busy])], failed_batches=acc["failed_batches"],
                           not_converged=acc["not_converged"], first_error=acc["first_error"], pcg_steps=acc["pcg_steps"])
        if reuse is not None:
            self.timing.update(mesh_hits=reuse.mesh_hits, warm_hits=reuse.warm_hits)
        if acc["programming_error"] is not None:     # every rank is through the collectives: now it may raise
            raise acc["programming_error"]
        if verbose and acc["failed_batches"]:
            print("rank {}: {} of {} batches failed (NaN in the logs); first: {}".format(sweep.rank(), acc["failed_batches"], len(bq.taken), acc["first_error"]))
        if verbose and acc["not_converged"]:
            print("rank {}: PCG stopped at maxsteps in {} batches".format(sweep.rank(), acc["not_converged"]))
        if verbose and sweep.rank() == 0:
            print("\nProcessed in: ", datetime.timedelta(seconds=self.timing["total_s"]))

    # -- electrode arrays and focused logs (no counterpart in the reference) -------------------------
    def simulate_array_logs(self, array, measurement_depths, domain_radius=50, batch_size=1, preconditioner="multigrid", condense=True,
                            mesh_provider: Optional[Callable] = None, mesh_scale: Optional[float] = None, rtol: float = 1e-8,
                            maxsteps: int = 1000, verbose: bool = True, solver_options: Optional[dict] = None, sensitivities: bool = False,
                            sensitivity_grid: Optional[dict] = None):
        """The logs of a multi-electrode array (arrays.ElectrodeArray; arrays.laterolog7() is the seven-electrode laterolog) in the
        model of simulate_logs: 2D for dip 0, 3D otherwise; windowing, meshes, contexts, the NaN of a failed batch and self.timing as
        there.  A batch holds batch_size consecutive depths; per depth every electrode that some mode makes carry current is one
        right-hand side of unit current, read at all other electrodes: the transfer impedances, from which every mode's bucking
        currents and reading follow (arrays.focus).  Fills self.array, self.array_logs[mode] [n_depths, 2] (depth, Ra),
        self.array_currents[mode] [n_depths, m] and self.array_impedances [n_depths, m, m] (V / A, physical values against infinity -
        solver.far_field_reference adds what the grounded surface of the batch mesh at domain_radius takes -, NaN where not measured).  sensitivities: also self.array_sensitivities[mode] [n_depths, n_layers, n_cols] and
        self.array_mud_sensitivity[mode] [n_depths], with the meaning, units and NaN / 0 conventions of self.sensitivities and
        self.mud_sensitivity - by reciprocity, from the pair derivatives of the forward solutions (the read / null electrodes become
        right-hand sides too; no adjoint solves).  sensitivity_grid: dict(r=edges, z=edges), in 3D also x=edges instead of r, with the
        meaning of simulate_logs' keyword: also self.array_sensitivity_maps[mode] [n_depths, n_z, n_r], d ln Ra / d ln R of every cell -
        what the focused reading sees where -, self.array_sensitivity_map_rest[mode] [n_depths] for everything outside the grid (cells
        and rest sum to 1) and self.sensitivity_grid; from the pair derivatives per group of elements (remo_job_pair_groups_t), with the
        right-hand sides sensitivities=True adds, with or without that flag.  fp64 only.  Beyond self.sensitivity_grid nothing
        simulate_logs publishes is touched, and the other way round."""
        start = time.time()
        if not isinstance(array, arrays.ElectrodeArray):
            raise ValueError("array has to be an arrays.ElectrodeArray")
        if (solver_options or {}).get("precision", "fp64") != "fp64":
            raise ValueError("array logs are formed from fp64 solutions: precision has to be 'fp64'")
        if sensitivity_grid is not None:
            _ArrayMaps.lateral_axis(sensitivity_grid)
        plan = _ArrayPlan(self, array, sensitivities or sensitivity_grid is not None, measurement_depths, domain_radius, batch_size, "auto", mesh_provider, mesh_scale,
                          dict(preconditioner=preconditioner, condense=condense, rtol=rtol, maxsteps=maxsteps, precision="fp64"),
                          solver_options, verbose)
        windowing = _Windowing(plan)
        outputs = [_ArrayLogs(plan)]
        if sensitivities:
            outputs.append(_ArraySensitivities(plan, windowing))
        if sensitivity_grid is not None:
            outputs.append(_ArrayMaps(plan, sensitivity_grid))
        bq = sweep.BatchQueue(len(plan.batches), "static")
        meshes = _MeshAhead(plan, windowing, bq, "static", None)
        runner = _ArrayRunner(plan, windowing, meshes, outputs)

        def reset():
            self.array_sensitivities = self.array_mud_sensitivity = self.array_sensitivity_maps = self.array_sensitivity_map_rest = None
            if sensitivity_grid is not None:
                self.sensitivity_grid = None
        self._drive_and_report(plan, bq, meshes, runner, outputs, reset, "static", start, verbose)

    # -- inversion (no counterpart in the reference) -----------------------------------------------
    def invert_logs(self, observed, measurement_depths, free="RTUZ", **kw):
        """Fit the resistivities of the formation table to observed apparent resistivities.  observed: dict tool -> [n_depths] in
        ohm m on the grid of measurement_depths (or the [n_depths, 2] arrays of self.logs); NaN = no datum.  Unknowns: ln R of the
        free table entries - free = "RTUZ" (default: every finite RTUZ), "RTUZ+RTFZ", "all", or a boolean mask [n_layers, n_cols]
        over RTFZ, RTUZ, RVUZ; radii and boundaries are never free, a free NaN entry is an error.  Residuals ln Ra_sim - ln Ra_obs
        weighted by 1 / data_std (relative standard deviation, a scalar or a dict per tool, default 0.05); records where either value
        is NaN or not positive are left out of that evaluation and counted.  Levenberg-Marquardt (inversion.lm_loop) with
        J^T W J + mu diag(J^T W J) + beta L^T L (L: first differences of ln R between vertically adjacent free entries of a column;
        beta default 0) and an optional pull beta_ref toward a `reference` table; steps clipped to bounds = (0.01, 1e5) ohm m and to
        max_step = ln 3.  Every evaluation is one simulate_logs(sensitivities=True) sweep at the trial table.  Stops: max_iterations
        (15), ftol, xtol, target_rms.  Further keywords: mu, reuse_meshes (default True: the meshes of the first sweep serve all),
        warm_start (default False; True: every batch's solves start from its solutions of the previous sweep - about half the PCG steps
        over an inversion, but on the short 3D span measured the solve time of sweeps two onward did not beat cached meshes alone:
        DESIGN.md section 3.4), warm_bytes, and solver_kw: a dict of
        simulate_logs keywords (domain_radius, batch_size, rtol, mesh_scale, solver_options, ...).
        On return the formation table holds the result, self.logs / self.sensitivities are those of the accepted table and
        self.inversion (also returned) holds start_table, final_table, free, jacobian, singular_values, parameter_std (ln units; NaN
        for an entry no datum sees, listed in `unseen`), resolution, history (one record per sweep: objective, rms, mu, accepted,
        excluded, seconds, pcg_steps, warm_hits, mesh_hits, ...) and stop."""
        from . import inversion
        return inversion.invert_model(self, observed, measurement_depths, free=free, **kw)

    # -- results (remo3d.py:902-1147): Results_<n>.txt per group of logs on one depth grid + Results_plot.png ------------------
    def save_results(self, output_folder=None, measurements_to_save="auto", plot_layout="auto", plot_depth_lim="auto", plot_aspect_ratio="auto",
                     model_rad_lim="auto", model_res_lim="auto", logs_res_lim="auto", logs_at_nan="break", logs_interpolation_factor=1,
                     logs_colours="auto", plot=True):
        """Same keywords as the reference (remo3d.py:902-903).  plot=False (this build's addition) skips the picture; without an
        output folder the reference only shows the figure (a notebook feature): here the figure is returned."""
        plot_kw = dict(plot_layout=plot_layout, plot_depth_lim=plot_depth_lim, plot_aspect_ratio=plot_aspect_ratio, model_rad_lim=model_rad_lim,
                       model_res_lim=model_res_lim, logs_res_lim=logs_res_lim, logs_at_nan=logs_at_nan,
                       logs_interpolation_factor=logs_interpolation_factor, logs_colours=logs_colours)
        if output_folder is None:
            if plot and self.logs and self.formation_model is not None:
                from . import plotting
                return plotting.plot_results(self, None, **plot_kw)
            return None
        sub = os.path.join(output_folder, "Results_{}/".format(datetime.datetime.now().strftime("%Y_%m_%d__%H_%M_%S")))
        os.makedirs(sub, exist_ok=True)
        pending = list(self.logs.keys()) if measurements_to_save == "auto" else list(measurements_to_save)
        n = 1
        written = []
        while pending:
            head = pending[0]
            group = [head] + [k for k in pending[1:] if self.logs[k].shape[0] == self.logs[head].shape[0]
                              and np.all(np.isclose(self.logs[head][:, 0], self.logs[k][:, 0]))]
            pending = [k for k in pending if k not in group]
            table = np.hstack([self.logs[head]] + [self.logs[k][:, 1:2] for k in group[1:]])
            header = "\t".join(["DEPTH"] + group) + "\n" + "\t".join(["M"] + ["OHMM"] * len(group))
            path = sub + "Results_{}.txt".format(n)
            np.savetxt(path, table, fmt="%.4f", delimiter="\t", header=header, comments="")
            written.append(path)
            n += 1
        if plot and self.logs and self.formation_model is not None:     # (no picture of a model that was never set)
            from . import plotting
            import matplotlib.pyplot as plt
            fig = plotting.plot_results(self, sub + "Results_plot.png", **plot_kw)
            plt.close(fig)
            written.append(sub + "Results_plot.png")
        return written
