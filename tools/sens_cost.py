"""Cost of remo_solve_batch_sens on headline-size batches: two batches of the bench's size L (five right-hand sides, one functional
each, one context), the sensitivity entry against remo_solve_batch on the same build, and the contraction's HIP-event time beside
its algorithmic bytes (remo_debug_sens_timing).  Prints one JSON line per batch.  With --groups N also the group entry
(remo_solve_batch_sens_groups) with an N-cell (r, z) grid and with group = arange(n_elems): the call against the sensitivity
entry, and - from runs with time_kernels, which synchronise after every functional - the group order per batch and the material
pass, the per-element pass and the group sums per functional (remo_debug_sens_group_timing).

    python tools/sens_cost.py [--size L] [--batches 0 20] [--reps 3] [--groups 8192]

Each GPU step runs in a child process under its own time limit; a step that fails ends the script."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(size, bi, reps, n_cells=0):
    import time
    import numpy as np
    import bench
    from remo3d_amd import solver
    w = bench._build_some((100, bench.SIZES[size], "lattice", [bi]))[0]
    mesh, sigma, src, ev = w["mesh"], w["sigma"], w["sources"], w["evals"]
    fun = []
    for k, e in enumerate(ev):      # the functional of the record: u_N - u_M, or u_M
        e = np.asarray(e, dtype=float)
        fun.append((k, e[:2], np.array([-1.0, 1.0])) if e.size >= 2 else (k, e[:1], np.array([1.0])))
    o = solver.make_opts()
    out = dict(size=size, batch=bi, n_rhs=len(src), n_fun=len(fun), elements=int(mesh.conn.shape[0]))
    with solver.Context(0) as ctx:
        ctx.solve_batch(mesh, sigma, src, ev, o)      # warm-up: arena, code objects
        ctx.solve_batch_sens(mesh, sigma, src, ev, fun, o)
        t_plain, t_sens, k_ms = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter(); _, st, rc = ctx.solve_batch(mesh, sigma, src, ev, o); t_plain.append(time.perf_counter() - t0)
            assert rc == 0
            t0 = time.perf_counter(); _, J, dJ, st2, rc = ctx.solve_batch_sens(mesh, sigma, src, ev, fun, o); t_sens.append(time.perf_counter() - t0)
            assert rc == 0 and np.all(np.isfinite(dJ))
            k_ms.append(ctx.sens_timing())
        ms, nbytes = min(k_ms)
        out.update(rows=int(st["n_free"]), plain_ms=1e3 * min(t_plain), sens_ms=1e3 * min(t_sens), ratio=min(t_sens) / min(t_plain),
                   plain_pcg_steps=int(st["pcg_steps"]), sens_pcg_steps=int(st2["pcg_steps"]), plain_solve_ms=st["ms_solve"], sens_solve_ms=st2["ms_solve"],
                   contraction_ms=ms, contraction_bytes=nbytes, contraction_gbs=nbytes / ms / 1e6 if ms > 0 else None,
                   op_bytes=st["spmv_bytes"])
        if n_cells > 0:
            from remo3d_amd import geometry
            nz = max(1, int(round((2 * n_cells) ** 0.5)))
            nr = max(1, n_cells // nz)
            c = mesh.coords[mesh.conn].mean(axis=1)
            rho = np.abs(c[:, 0]) if mesh.dim == 2 else np.hypot(c[:, 0], c[:, 1])
            grid = dict(r=np.linspace(0.0, 0.5 * float(rho.max()), nr + 1), z=np.linspace(float(c[:, -1].min()), float(c[:, -1].max()) + 1e-9, nz + 1))
            cells = geometry.sensitivity_cells(mesh, None, grid, 0.0)
            ot = solver.make_opts(time_kernels=True)
            for label, group, ng in (("grid", cells[0], len(cells[1])), ("arange", np.arange(len(mesh.mat), dtype=np.int32), len(mesh.mat))):
                ctx.solve_batch_sens_groups(mesh, sigma, src, ev, fun, group, ng, o)      # warm-up (the arena grows)
                t_g, parts = [], []
                for _ in range(reps):
                    t0 = time.perf_counter(); r = ctx.solve_batch_sens_groups(mesh, sigma, src, ev, fun, group, ng, o); t_g.append(time.perf_counter() - t0)
                    assert r[5] == 0 and np.all(np.isfinite(r[3]))
                    r = ctx.solve_batch_sens_groups(mesh, sigma, src, ev, fun, group, ng, ot)
                    parts.append(ctx.sens_group_timing())
                best = np.min(np.array(parts), axis=0)
                out[label] = dict(n_group=int(ng), call_ms=1e3 * min(t_g), ratio_to_sens=min(t_g) / min(t_sens), order_ms=best[0],
                                  material_ms_per_fun=best[1] / len(fun), per_element_ms_per_fun=best[2] / len(fun), group_sum_ms_per_fun=best[3] / len(fun))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="L")
    ap.add_argument("--batches", type=int, nargs="+", default=[0, 20])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--groups", type=int, default=0, help="cells of the (r, z) grid of the group entry (0: not measured)")
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds per batch")
    a = ap.parse_args()
    if a.child is not None:
        measure(a.size, a.child, a.reps, a.groups)
        return 0
    for bi in a.batches:
        rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--size", a.size, "--reps", str(a.reps),
                              "--groups", str(a.groups), "--child", str(bi)])
        if rc != 0:
            print("batch %d: exit status %d - stopping" % (bi, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
