"""Cost of remo_solve_batch_sens on headline-size batches: two batches of the bench's size L (five right-hand sides, one functional
each, one context), the sensitivity entry against remo_solve_batch on the same build, and the contraction's HIP-event time beside
its algorithmic bytes (remo_debug_sens_timing).  Prints one JSON line per batch.

    python tools/sens_cost.py [--size L] [--batches 0 20] [--reps 3]

Each GPU step runs in a child process under its own time limit; a step that fails ends the script."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(size, bi, reps):
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
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="L")
    ap.add_argument("--batches", type=int, nargs="+", default=[0, 20])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", type=int, default=None)
    ap.add_argument("--limit", type=int, default=420, help="seconds per batch")
    a = ap.parse_args()
    if a.child is not None:
        measure(a.size, a.child, a.reps)
        return 0
    for bi in a.batches:
        rc = subprocess.call(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--size", a.size, "--reps", str(a.reps),
                              "--child", str(bi)])
        if rc != 0:
            print("batch %d: exit status %d - stopping" % (bi, rc), file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
