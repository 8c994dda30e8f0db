"""What the goal-oriented error estimates (remo_job_error_t.err) cost and how they compare with the true error, measured on the device.

  cost         one batch of the bench's size L (five right-hand sides, one functional each, one context): remo_solve_batch_sens
               against the same job with error=True and with a per-element grouping, alternating, best of --reps; and, with
               --parent-tree, remo_solve_batch_sens of the package and built library in that checkout (the parent commit's) in a
               process of its own, the two processes alternating --rounds times.
  effectivity  Model on the reference's Example_01 (2D, six tools): error_estimates at mesh_scale 2, 1 and 0.5 beside the true
               relative change of Ra against a run at mesh_scale 0.25; median and extreme ratio estimate / true.

    python tools/error_estimate_study.py [--legs cost effectivity] [--parent-tree DIR] [--size L] [--batch 20] [--reps 3] [--rounds 2]
                                         [--scales 2 1 0.5] [--truth 0.25] [--stride 1] [--out profiles/error_estimate_study.json]

One GPU process at a time: each step runs in a child process under its own time limit, and a step that fails ends the script.
Records, sets no threshold."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOOLS = ["B5.7A0.4M", "B4.48A1.62M", "M1.0A0.1B", "A2.0M0.5N", "N0.5M2.0A", "M4.0A0.5B"]


def _batch(args):
    import numpy as np
    import bench
    w = bench._build_some((100, bench.SIZES[args.size], "lattice", [args.batch]))[0]
    fun = []
    for k, e in enumerate(w["evals"]):      # the functional of the record: u_N - u_M, or u_M
        e = np.asarray(e, dtype=float)
        fun.append((k, e[:2], np.array([-1.0, 1.0])) if e.size >= 2 else (k, e[:1], np.array([1.0])))
    return w["mesh"], w["sigma"], w["sources"], w["evals"], fun


def leg_cost(args):
    """This build: the sensitivity entry, the same with the estimates, and with the per-element map."""
    import time
    import numpy as np
    from remo3d_amd import solver
    mesh, sigma, src, ev, fun = _batch(args)
    n = int(mesh.conn.shape[0])
    each = dict(n_group=n, group=np.arange(n, dtype=np.int32))
    o = solver.make_opts()
    out = dict(size=args.size, batch=args.batch, n_rhs=len(src), n_fun=len(fun), elements=n)
    with solver.Context(0) as ctx:
        for kw in (dict(), dict(error=True), dict(error=each)):      # warm-up: arena, code objects
            ctx.solve_batch_sens(mesh, sigma, src, ev, fun, o, **kw)
        t = dict(sens=[], err=[], err_map=[])
        for _ in range(args.reps):
            for name, kw in (("sens", dict()), ("err", dict(error=True)), ("err_map", dict(error=each))):
                t0 = time.perf_counter(); r = ctx.solve_batch_sens(mesh, sigma, src, ev, fun, o, **kw); t[name].append(time.perf_counter() - t0)
                assert r[-1] == 0
        E, J = r[3], r[1]
        out.update(rows=int(r[-2]["n_free"]), sens_ms=1e3 * min(t["sens"]), err_ms=1e3 * min(t["err"]), err_map_ms=1e3 * min(t["err_map"]),
                   ratio_err=min(t["err"]) / min(t["sens"]), ratio_err_map=min(t["err_map"]) / min(t["sens"]),
                   estimated_relative_error=(E / np.abs(J)).tolist())
    return out


def leg_parent(args):
    """Another checkout (--parent-tree, first on sys.path of this child): the sensitivity entry alone."""
    import time
    from remo3d_amd import _lib, solver
    mesh, sigma, src, ev, fun = _batch(args)
    o = solver.make_opts()
    with solver.Context(0) as ctx:
        ctx.solve_batch_sens(mesh, sigma, src, ev, fun, o)
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter(); r = ctx.solve_batch_sens(mesh, sigma, src, ev, fun, o); t.append(time.perf_counter() - t0)
            assert r[-1] == 0
    return dict(lib=_lib.LIB_PATH, sens_ms=1e3 * min(t))


def leg_effectivity(args):
    import time
    import numpy as np
    from remo3d_amd.model import Model
    ex = os.path.join(ROOT, "tests", "golden", "examples", "Example_01", "Input")
    depths = np.arange(0, 25.1, 0.1)[::args.stride]

    def run(scale, est):
        t0 = time.time()
        m = Model.compute_synthetic_logs(TOOLS, depths, os.path.join(ex, "Formation.txt"), os.path.join(ex, "Borehole.txt"), gpu_workers=1,
                                         verbose=False, mesh_scale=scale, mesh_workers=12, error_estimate=est)
        assert m.timing["failed_batches"] == 0, m.timing["first_error"]
        return m, time.time() - t0
    truth, s = run(args.truth, False)
    ra0 = np.array([truth.logs[t][:, 1] for t in TOOLS])
    out = dict(depths=int(depths.size), tools=TOOLS, truth_scale=args.truth, truth_seconds=s, scales={})
    for scale in args.scales:
        plain, s0 = run(scale, False)
        m, s1 = run(scale, True)
        ra = np.array([m.logs[t][:, 1] for t in TOOLS])
        est = np.array([m.error_estimates[t] for t in TOOLS])
        true = np.abs(ra - ra0) / ra0
        ok = (true > 0) & np.isfinite(est) & (est > 0)      # (a reading that does not change at all has no ratio)
        ratio = est[ok] / true[ok]
        out["scales"][str(scale)] = dict(
            seconds_plain=s0, seconds_with_estimates=s1, solve_s_plain=plain.timing["solve_s"], solve_s_with_estimates=m.timing["solve_s"],
            true_median=float(np.median(true)), true_max=float(np.max(true)), estimate_median=float(np.median(est)), estimate_max=float(np.max(est)),
            ratio_median=float(np.median(ratio)), ratio_min=float(np.min(ratio)), ratio_max=float(np.max(ratio)),
            fraction_bounded=float(np.mean(est >= true)), correlation_of_logs=float(np.corrcoef(np.log(est[ok]), np.log(true[ok]))[0, 1]),
            estimate_by_tool=np.median(est, axis=1).tolist(), true_by_tool=np.median(true, axis=1).tolist())
        print("scale %g: true median %.2e max %.2e | estimate median %.2e | estimate / true median %.1f min %.2f max %.1f | bounded %.0f %%" % (
            scale, np.median(true), np.max(true), np.median(est), np.median(ratio), np.min(ratio), np.max(ratio), 100 * np.mean(est >= true)),
            file=sys.stderr, flush=True)
    return out


LEGS = dict(cost=(leg_cost, 420), parent=(leg_parent, 300), effectivity=(leg_effectivity, 900))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="+", default=["cost", "effectivity"], choices=["cost", "effectivity"])
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built (cost leg)")
    ap.add_argument("--size", default="L")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="alternations of the two builds")
    ap.add_argument("--scales", type=float, nargs="+", default=[2.0, 1.0, 0.5])
    ap.add_argument("--truth", type=float, default=0.25)
    ap.add_argument("--stride", type=int, default=1, help="every stride-th of Example_01's 251 depths")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child is not None:
        if a.child == "parent":      # that checkout's package, library and bench.py instead of this one's
            sys.path.insert(0, os.path.abspath(a.parent_tree))
        print(json.dumps(LEGS[a.child][0](a)), flush=True)
        return 0
    passed = ["--size", a.size, "--batch", str(a.batch), "--reps", str(a.reps), "--truth", str(a.truth), "--stride", str(a.stride),
              "--scales"] + [str(s) for s in a.scales]

    def child(leg, extra=()):
        cmd = ["timeout", "-k", "10", str(LEGS[leg][1]), sys.executable, os.path.abspath(__file__), "--child", leg] + passed + list(extra)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print("leg %s: exit status %d - stopping" % (leg, p.returncode), file=sys.stderr)
            sys.exit(p.returncode)
        return json.loads(p.stdout.strip().splitlines()[-1])
    result = {}
    if "cost" in a.legs:
        own, parent = [], []
        for _ in range(a.rounds if a.parent_tree else 1):
            if a.parent_tree:
                parent.append(child("parent", ["--parent-tree", a.parent_tree]))
            own.append(child("cost"))
        best = min(own, key=lambda r: r["sens_ms"])
        result["cost"] = dict(best, rounds=own)
        if parent:
            p_ms = min(r["sens_ms"] for r in parent)
            result["cost"].update(parent_sens_ms=p_ms, parent_rounds=parent, sens_to_parent=best["sens_ms"] / p_ms,
                                  err_to_parent=min(r["err_ms"] for r in own) / p_ms)
    if "effectivity" in a.legs:
        result["effectivity"] = child("effectivity")
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
