"""What the secondary-potential formulation (remo_job_secondary_t.secondary) costs and buys, measured on the device.  Three legs:

  cost   a batch of the bench's size L (five right-hand sides, one context): remo_solve_batch against the same batch with
         secondary=dict(radius=R), best of --reps; the load-vector launches by HIP events (remo_debug_secondary_timing); the PCG
         step counts of both.
  quad   the rule order: on the GPU test cases (the suite's two-zone 2D / 3D meshes, scalar and tensor, and the two half spaces) the
         largest relative change of any potential when n points per direction become n + 3, for n = 2 .. 9.  The default is the
         smallest n whose change is at most 1e-7 in every case.
  logs   Model on benchmark model 1 (2D) and benchmark model 3 at dip 30 (3D): the logs at mesh_scale x {1, 1.5, 2} in both
         formulations against the secondary logs at mesh_scale x 0.5.

    python tools/secondary_cost.py [--legs cost quad logs] [--size L] [--batch 20] [--reps 3] [--out profiles/secondary_cost.json]

Each leg runs in a child process under its own time limit; a leg that fails ends the script.  Records, sets no threshold."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
R = 50.0


def leg_cost(args):
    import time
    import bench
    from remo3d_amd import solver
    w = bench._build_some((100, bench.SIZES[args.size], "lattice", [args.batch]))[0]
    mesh, sigma, src, ev = w["mesh"], w["sigma"], w["sources"], w["evals"]
    o = solver.make_opts()
    sec = dict(radius=R)
    out = dict(size=args.size, batch=args.batch, n_rhs=len(src), elements=int(mesh.conn.shape[0]))
    with solver.Context(0) as ctx:
        ctx.solve_batch(mesh, sigma, src, ev, o)      # warm-up: arena, code objects
        ctx.solve_batch(mesh, sigma, src, ev, o, secondary=sec)
        t_plain, t_sec, k_ms = [], [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); a, st, rc = ctx.solve_batch(mesh, sigma, src, ev, o); t_plain.append(time.perf_counter() - t0)
            assert rc == 0
            t0 = time.perf_counter(); b, st2, rc = ctx.solve_batch(mesh, sigma, src, ev, o, secondary=sec); t_sec.append(time.perf_counter() - t0)
            assert rc == 0
            k_ms.append(ctx.secondary_timing())
        import numpy as np
        diff = max(float(np.max(np.abs(x - y) / np.abs(y))) for x, y in zip(a, b) if len(y))
        out.update(rows=int(st["n_free"]), plain_ms=1e3 * min(t_plain), secondary_ms=1e3 * min(t_sec), ratio=min(t_sec) / min(t_plain),
                   load_vector_ms=min(k_ms), plain_pcg_steps=int(st["pcg_steps"]), secondary_pcg_steps=int(st2["pcg_steps"]),
                   plain_solve_ms=st["ms_solve"], secondary_solve_ms=st2["ms_solve"], max_rel_difference_of_potentials=diff)
    return out


def leg_quad(args):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import SIGMA3, _two_zone
    from test_oracle import _two_half_spaces
    from remo3d_amd import geometry, solver
    from remo3d_amd.meshgen import make_mesh
    ev = [0.4, 6.4, 2.0, 2.5, -0.3, 1.2]
    rhs = [([0.0], [1.0]), ([0.1], [1.0]), ([0.0, 0.1], [1.0, -1.0])]
    m2 = make_mesh(2, R, [0.0, 0.1, -0.1], scale=2.0, material_fn=_two_zone(2), seed=0)
    m3 = make_mesh(3, R, [0.0, 0.1, -0.1], scale=8.0, material_fn=_two_zone(3), seed=0)
    ti = np.stack([np.eye(3), geometry.ti_conductivity(0.1, 0.025, np.deg2rad(30.0), 3)[0], 0.02 * np.eye(3)])
    cases = {"2d": (m2, SIGMA3, rhs, [ev] * 3), "3d": (m3, SIGMA3, rhs, [ev] * 3), "3d_tensor": (m3, ti, rhs, [ev] * 3)}
    for scale in (4.0, 1.0):
        mesh, sigma, zs, _ = _two_half_spaces(scale)
        cases["two_half_spaces_%g" % scale] = (mesh, sigma, [([0.0], [1.0])], [list(zs)])
    o = solver.make_opts(rtol=1e-13, maxsteps=100000, op="csr")
    out = {}
    with solver.Context(0) as ctx:
        for name, (mesh, sigma, src, evs) in cases.items():
            u = {}
            for n in range(2, 13):
                outs, _, rc = ctx.solve_batch(mesh, sigma, src, evs, o, secondary=dict(radius=R, quad=n))
                assert rc == 0
                u[n] = np.concatenate(outs)
            out[name] = {str(n): float(np.max(np.abs(u[n] - u[n + 3]) / np.abs(u[n + 3]))) for n in range(2, 10)}
    worst = {str(n): max(c[str(n)] for c in out.values()) for n in range(2, 10)}
    return dict(change_when_n_becomes_n_plus_3=out, worst=worst, smallest_n_within_1e_7=min(int(n) for n, v in worst.items() if v <= 1e-7))


def leg_logs(args):
    import time
    import numpy as np
    from remo3d_amd.model import Model
    bm = os.path.join(ROOT, "tests", "golden", "examples", "Benchmark models")
    tools = ["A0.4M6.0N", "A2.0M0.5N"]
    which = {"bm1": (os.path.join(bm, "Benchmark model 1", "Formation_BM1.txt"), os.path.join(bm, "Benchmark model 1", "Borehole_BM1.txt"), 0,
                     np.array([8.0, 9.0, 10.0, 11.0, 12.0]), args.base_2d),
             "bm3_dip30": (os.path.join(bm, "Benchmark model 3", "Formation_BM3_30.txt"), os.path.join(bm, "Benchmark model 3", "Borehole_BM3.txt"), 30,
                           np.array([6.0, 6.5]), args.base_3d)}
    out = {}
    for name in args.models:
        f, b, dip, depths, base = which[name]

        def run(scale, formulation):
            t0 = time.perf_counter()
            m = Model.compute_synthetic_logs(tools, depths, f, b, dip=dip, domain_radius=R, mesh_scale=scale, verbose=False, gpu_workers=1,
                                             solver_options=dict(rtol=1e-10, maxsteps=20000), formulation=formulation)
            assert m.timing["failed_batches"] == 0, m.timing["first_error"]
            return np.concatenate([m.logs[t][:, 1] for t in tools]), int(m.timing["pcg_steps"]), time.perf_counter() - t0
        ref, steps, secs = run(0.5 * base, "secondary")
        rec = dict(base_mesh_scale=base, depths=[float(d) for d in depths], reference=dict(mesh_scale=0.5 * base, pcg_steps=steps, seconds=secs), runs=[])
        for mult in (1.0, 1.5, 2.0):
            for formulation in ("primary", "secondary"):
                ra, steps, secs = run(mult * base, formulation)
                rec["runs"].append(dict(mesh_scale=mult * base, formulation=formulation, pcg_steps=steps, seconds=secs,
                                        max_rel_error=float(np.max(np.abs(ra - ref) / np.abs(ref)))))
        out[name] = rec
    return out


LEGS = dict(cost=(leg_cost, 600), quad=(leg_quad, 600), logs=(leg_logs, 1100))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["cost", "quad", "logs"], choices=list(LEGS))
    ap.add_argument("--size", default="L")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--models", nargs="+", default=["bm1", "bm3_dip30"])
    ap.add_argument("--base-2d", type=float, default=1.0, help="the mesh_scale that counts as x 1 on benchmark model 1")
    ap.add_argument("--base-3d", type=float, default=1.0, help="... and on benchmark model 3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "secondary_cost.json"))
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(LEGS[args.child][0](args)), flush=True)
        return
    result = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            result = json.load(fh)
    for leg in args.legs:      # a fresh process per leg, each under its own time limit; the first failure ends the script
        cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--size", args.size, "--batch", str(args.batch), "--reps", str(args.reps),
               "--base-2d", str(args.base_2d), "--base-3d", str(args.base_3d), "--models"] + args.models
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LEGS[leg][1])
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit("leg {} failed with exit status {}".format(leg, p.returncode))
        result[leg] = json.loads(lines[-1][7:])
        print(leg, json.dumps(result[leg]), flush=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
