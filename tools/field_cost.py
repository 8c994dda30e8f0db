"""Cost of remo_solve_batch_field on a headline-size batch: a batch of the bench's size L (five right-hand sides, one context),
remo_solve_batch against remo_solve_batch_field with an n x n section in the plane y = 0 for all five columns, best of --reps;
the location of the points and the evaluation launches by HIP events (remo_debug_field_timing); and the PCG step counts of both,
which must be equal - what the field entry adds to the solve is the direction launch that forms the whole x instead of the
evaluated rows.  Prints one JSON line per batch.

    python tools/field_cost.py [--size L] [--batches 20] [--reps 3] [--n 256]

Each GPU step runs in a child process under its own time limit; a step that fails ends the script."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(size, bi, reps, n):
    import time
    import numpy as np
    import bench
    from remo3d_amd import geometry, solver
    w = bench._build_some((100, bench.SIZES[size], "lattice", [bi]))[0]
    mesh, sigma, src, ev = w["mesh"], w["sigma"], w["sources"], w["evals"]
    dim = int(mesh.dim)
    span = 10.0     # metres across and along: borehole, beds and the near far field
    grid = dict(z=np.linspace(-span, span, n))
    grid["x" if dim == 3 else "r"] = np.linspace(-span, span, n) if dim == 3 else np.linspace(0.0, span, n)
    pts = geometry.field_points(grid, dim, 0.0)
    o = solver.make_opts()
    out = dict(size=size, batch=bi, n_rhs=len(src), elements=int(mesh.conn.shape[0]), points=int(pts.shape[0]))
    with solver.Context(0) as ctx:
        ctx.solve_batch(mesh, sigma, src, ev, o)      # warm-up: arena, code objects
        ctx.solve_batch_field(mesh, sigma, src, ev, pts, None, o)
        t_plain, t_field, k_ms = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter(); _, st, rc = ctx.solve_batch(mesh, sigma, src, ev, o); t_plain.append(time.perf_counter() - t0)
            assert rc == 0
            t0 = time.perf_counter(); _, f, st2, rc = ctx.solve_batch_field(mesh, sigma, src, ev, pts, None, o); t_field.append(time.perf_counter() - t0)
            assert rc == 0
            k_ms.append(ctx.field_timing())
        assert int(st["pcg_steps"]) == int(st2["pcg_steps"]), (st["pcg_steps"], st2["pcg_steps"])
        inside = f["elem"] >= 0
        assert np.all(np.isfinite(f["J"][:, inside]))
        best = np.min(np.array(k_ms), axis=0)
        out.update(rows=int(st["n_free"]), inside=int(inside.sum()), plain_ms=1e3 * min(t_plain), field_ms=1e3 * min(t_field), ratio=min(t_field) / min(t_plain),
                   plain_pcg_steps=int(st["pcg_steps"]), field_pcg_steps=int(st2["pcg_steps"]), plain_solve_ms=st["ms_solve"], field_solve_ms=st2["ms_solve"],
                   locate_ms=float(best[0]), eval_ms=float(best[1]))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="L")
    ap.add_argument("--batches", type=int, nargs="+", default=[20])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=256, help="points along each axis of the section")
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds per batch")
    a = ap.parse_args()
    if a.child is not None:
        measure(a.size, a.child, a.reps, a.n)
        return 0
    for bi in a.batches:
        rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--size", a.size, "--reps", str(a.reps),
                              "--n", str(a.n), "--child", str(bi)])
        if rc != 0:
            print("batch %d: exit status %d - stopping" % (bi, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
