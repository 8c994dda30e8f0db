"""Whether the fused pair pass pays: a batch of the bench's size L (batch 20) with the seven electrodes of arrays.laterolog7() as
unit right-hand sides around the batch's first source, and the 28 pairs a <= b.
  (a) the fused pass (k_pair_contract: one launch), HIP-event time of remo_debug_pairs_timing;
  (b) the same 28 values by 28 launches of k_sens_contract with both columns forward (remo_debug_tune key 42 = 0);
  (c) the whole call, seven solves + the pass, against remo_solve_batch_sens with the 12 functionals of the LL7 - the four monitors
      read under each of the three current electrodes: three forward and twelve adjoint solves, twelve contraction launches.
Writes profiles/pairs_cost.json and prints it.

    python tools/pairs_cost.py [--size L] [--batch 20] [--reps 3]

The GPU work runs in a child process under its own time limit."""
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
    from remo3d_amd import arrays, solver
    w = bench._build_some((100, bench.SIZES[size], "lattice", [bi]))[0]
    mesh, sigma = w["mesh"], w["sigma"]
    arr = arrays.laterolog7()
    z0 = float(np.atleast_1d(np.asarray(w["sources"][0][0], dtype=float))[0])
    z = z0 + arr.offsets
    m = len(z)
    src = [([z[i]], [1.0]) for i in range(m)]
    ev = [[z[k] for k in range(m) if k != i] for i in range(m)]
    pairs = [(a, b) for a in range(m) for b in range(a, m)]
    cur = [i for i in range(m) if arr.current_electrodes[i]]
    mon = [i for i in range(m) if arr.potential_electrodes[i]]
    src3 = [src[i] for i in cur]
    ev3 = [[z[k] for k in mon] for _ in cur]
    fun = [(c, [z[k]], [1.0]) for c in range(len(cur)) for k in mon]
    o = solver.make_opts()
    out = dict(size=size, batch=bi, elements=int(mesh.conn.shape[0]), n_rhs=m, n_pair=len(pairs), n_fun=len(fun), n_mat=int(np.asarray(sigma).shape[0]))
    L = solver._lib.load()
    with solver.Context(0) as ctx:
        ctx.solve_batch_pairs(mesh, sigma, src, ev, pairs, o)      # warm-up: arena, code objects
        ctx.solve_batch_sens(mesh, sigma, src3, ev3, fun, o)
        fused, single, t_pairs, t_sens, sens_ms = [], [], [], [], []
        for _ in range(reps):
            t0 = time.perf_counter(); r = ctx.solve_batch_pairs(mesh, sigma, src, ev, pairs, o); t_pairs.append(time.perf_counter() - t0)
            assert r[-1] == 0 and np.all(np.isfinite(r[1]))
            fused.append(ctx.pairs_timing()[0])
            dP = r[1]
            t0 = time.perf_counter(); s = ctx.solve_batch_sens(mesh, sigma, src3, ev3, fun, o); t_sens.append(time.perf_counter() - t0)
            assert s[-1] == 0 and np.all(np.isfinite(s[2]))
            sens_ms.append(ctx.sens_timing()[0])
            L.remo_debug_tune(42, 0)
            try:
                r0 = ctx.solve_batch_pairs(mesh, sigma, src, ev, pairs, o)
            finally:
                L.remo_debug_tune(42, 1)
            assert r0[-1] == 0 and ctx.pairs_timing()[1] == len(pairs)
            single.append(ctx.pairs_timing()[0])
        out.update(rows=int(r[2]["n_free"]), fused_ms=min(fused), per_pair_launches_ms=min(single), speedup=min(single) / min(fused),
                   fused_vs_single_max_rel=float(np.max(np.abs(r0[1] - dP)) / np.max(np.abs(dP))),
                   pairs_call_ms=1e3 * min(t_pairs), sens_call_ms=1e3 * min(t_sens), call_ratio=min(t_pairs) / min(t_sens),
                   pairs_pcg_steps=int(r[2]["pcg_steps"]), sens_pcg_steps=int(s[3]["pcg_steps"]), sens_contraction_ms=min(sens_ms))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="L")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--limit", type=int, default=420, help="seconds for the measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairs_cost.json"))
    a = ap.parse_args()
    if a.child:
        measure(a.size, a.batch, a.reps)
        return 0
    p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--size", a.size, "--batch", str(a.batch),
                        "--reps", str(a.reps), "--child"], stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        print("measurement: exit status %d" % p.returncode, file=sys.stderr)
        return p.returncode
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
