"""Whether the fused pair pass pays: a batch of the bench's size L (batch 20) with the seven electrodes of arrays.laterolog7() as
unit right-hand sides around the batch's first source, and the 28 pairs a <= b.
  (a) the fused pass (k_pair_contract: one launch), HIP-event time of remo_debug_pairs_timing;
  (b) the same 28 values by 28 launches of k_sens_contract with both columns forward (remo_debug_tune key 42 = 0);
  (c) the whole call, seven solves + the pass, against remo_solve_batch_sens with the 12 functionals of the LL7 - the four monitors
      read under each of the three current electrodes: three forward and twelve adjoint solves, twelve contraction launches.
Writes profiles/pairs_cost.json and prints it.

    python tools/pairs_cost.py [--size L] [--batch 20] [--reps 3]

--groups: what the pair derivatives per group of elements (remo_job_pair_groups_t) cost on the same batch instead - the seven
electrodes, the 12 pairs (monitor, current electrode) Model.simulate_array_logs asks for, and two groupings: the (material, cell)
groups of an 8192-cell grid (geometry.sensitivity_cells, 128 z x 64 r) and group = arange(n_elems), the per-element map.  Per
grouping the ordering by group, the per-element launches and the group sums (HIP events of remo_debug_pair_groups_timing, from
calls with time_kernels) and the whole call (host clock around the call, calls without time_kernels) against the same call
without groups, alternating.  Writes profiles/pair_groups_cost.json.

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


def measure_groups(size, bi, reps):
    import time
    import numpy as np
    import bench
    from remo3d_amd import arrays, geometry, solver
    w = bench._build_some((100, bench.SIZES[size], "lattice", [bi]))[0]
    mesh, sigma = w["mesh"], w["sigma"]
    arr = arrays.laterolog7()
    z0 = float(np.atleast_1d(np.asarray(w["sources"][0][0], dtype=float))[0])
    z = z0 + arr.offsets
    m = len(z)
    src = [([z[i]], [1.0]) for i in range(m)]
    ev = [[z[k] for k in range(m) if k != i] for i in range(m)]
    pairs = [(i, j) for i in np.flatnonzero(arr.potential_electrodes) for j in np.flatnonzero(arr.current_electrodes)]
    n = int(mesh.conn.shape[0])
    grid = dict(z=np.linspace(z0 - 16.0, z0 + 16.0, 129), r=np.concatenate([[0.0], np.geomspace(0.05, 50.0, 64)]))
    cells, gmat, _ = geometry.sensitivity_cells(mesh, None, grid)
    groupings = {"grid_8192_cells": (cells, len(gmat)), "per_element": (np.arange(n, dtype=np.int32), n)}
    o, ot = solver.make_opts(), solver.make_opts(time_kernels=True)
    out = dict(size=size, batch=bi, elements=n, n_rhs=m, n_pair=len(pairs), n_mat=int(np.asarray(sigma).shape[0]), reps=reps)
    with solver.Context(0) as ctx:
        ctx.solve_batch_pairs(mesh, sigma, src, ev, pairs, o)      # warm-up: arena, code objects
        for name, (group, n_group) in groupings.items():
            ctx.solve_batch_pairs(mesh, sigma, src, ev, pairs, o, groups=group, n_group=n_group)      # ... of the group path, at this size
            plain, grouped, parts, pass_ms = [], [], [], []
            for _ in range(reps):
                t0 = time.perf_counter(); r0 = ctx.solve_batch_pairs(mesh, sigma, src, ev, pairs, o); plain.append(time.perf_counter() - t0)
                pass_ms.append(ctx.pairs_timing()[0])
                t0 = time.perf_counter(); r = ctx.solve_batch_pairs(mesh, sigma, src, ev, pairs, o, groups=group, n_group=n_group); grouped.append(time.perf_counter() - t0)
                assert r0[-1] == 0 and r[-1] == 0 and np.all(np.isfinite(r[2]))
                both = ctx.pair_groups_timing()
                rt = ctx.solve_batch_pairs(mesh, sigma, src, ev, pairs, ot, groups=group, n_group=n_group)
                assert rt[-1] == 0
                parts.append(ctx.pair_groups_timing() + (both[1],))
            best = min(parts, key=lambda p: p[0] + p[1] + p[2])
            out[name] = dict(n_group=int(n_group), order_ms=best[0], per_element_launches_ms=best[1], group_sums_ms=best[2], slices=best[3],
                             launches_and_sums_unsplit_ms=min(p[4] for p in parts), material_pass_ms=min(pass_ms),
                             call_ms=1e3 * min(grouped), call_without_groups_ms=1e3 * min(plain), call_ratio=min(grouped) / min(plain),
                             call_ms_all=[1e3 * t for t in grouped], call_without_groups_ms_all=[1e3 * t for t in plain],
                             dPg_bytes=int(r[2].nbytes), pcg_steps=int(r[3]["pcg_steps"]))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="L")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--groups", action="store_true", help="the cost of the pair derivatives per group of elements instead")
    ap.add_argument("--limit", type=int, default=420, help="seconds for the measurement")
    ap.add_argument("--out", default=None, help="default: profiles/pairs_cost.json, with --groups profiles/pair_groups_cost.json")
    a = ap.parse_args()
    if a.child:
        (measure_groups if a.groups else measure)(a.size, a.batch, a.reps)
        return 0
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "pair_groups_cost.json" if a.groups else "pairs_cost.json")
    p = subprocess.run(["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--size", a.size, "--batch", str(a.batch),
                        "--reps", str(a.reps), "--child"] + (["--groups"] if a.groups else []), stdout=subprocess.PIPE, text=True)
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
