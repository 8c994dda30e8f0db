#!/usr/bin/env python3
"""Offline (CPU, scipy) emulation of the fp32 search direction of the one-shot fp64 solves (PcgBuffersT::p32, remo_debug_tune key 41):
a multi-column PCG on the oracle's matrix with C = blockdiag(exact solve of the P1 vertex block, Jacobi), frozen converged columns and
the product's stopping test, run once as it is and once with the direction rounded to fp32 after p0 and after every direction update
(everything else - q = A p, x += alpha p, r -= alpha q, every sum - stays fp64 and uses the ROUNDED p, as the kernels do).  Prints,
for both runs, the steps per column, the true relative residual and the largest relative difference of x.

  python tools/study_direction_fp32.py [S|M|L|fixture] [rtol] [columns]

S / M / L: one batch of the bench sweep (tools/precond_study.py's set-up).  fixture: the 3D lattice mesh of the tests (tests/conftest.py
mesh3d) with the right-hand sides of tests/test_gpu_direction_fp32.py - the check that the step-count cap of that test is not what
hides a failure."""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.fem_oracle import Oracle  # noqa: E402

FIXTURE_SRC = [([0.0], [1.0]), ([0.1], [1.0]), ([-0.1, 0.1], [1.0, -1.0]), ([0.0], [2.0]), ([0.1], [0.5]), ([-0.1], [1.0]),
               ([0.0, 0.1], [1.0, 1.0]), ([0.1], [3.0])]


def block_pcg(A, F, C, rtol, maxit, round_p):
    """Columns of F solved side by side with per-column step lengths; a column whose <Cr, r> has dropped below rtol^2 <Cr0, r0> is
    frozen (alpha = beta = 0).  -> x, steps per column"""
    rnd = (lambda P: P.astype(np.float32).astype(np.float64)) if round_p else (lambda P: P)
    X = np.zeros_like(F)
    R = F.copy()
    Z = C(R)
    P = rnd(Z.copy())
    rz = np.einsum("ij,ij->j", R, Z)
    rz0 = rz.copy()
    steps = np.zeros(F.shape[1], dtype=int)
    for it in range(1, maxit + 1):
        live = rz > rtol * rtol * rz0
        if not live.any():
            break
        Q = A @ P
        pq = np.einsum("ij,ij->j", P, Q)
        alpha = np.where(live & (pq > 0), rz / np.where(pq > 0, pq, 1.0), 0.0)
        X += alpha * P
        R -= alpha * Q
        Z = C(R)
        rzn = np.einsum("ij,ij->j", R, Z)
        beta = np.where(live, rzn / np.where(rz > 0, rz, 1.0), 0.0)
        P = rnd(Z + beta * P)
        steps[live] = it
        rz = np.where(live, rzn, rz)
    return X, steps


def study(mesh, sigma, sources, rtol, log=print):
    o = Oracle(mesh, sigma, condense=True)
    rp, col, val = o.csr()
    n = o.nfree
    A = sp.csr_matrix((val, col, rp), shape=(n, n))
    fid = o.freeid()
    nvf = int((fid[:o.nv] >= 0).sum())
    F = np.stack([o.rhs(z, I)[0] for z, I in sources], axis=1)
    dinv = 1.0 / A.diagonal()
    lu = spla.splu(A[:nvf, :nvf].tocsc())

    def C(R):
        Z = dinv[:, None] * R
        Z[:nvf] = lu.solve(R[:nvf])
        return Z
    log(f"T={o.nt} n={n} nv_free={nvf} columns={F.shape[1]} rtol={rtol:g}")
    out = {}
    for name, rounded in (("fp64 p", False), ("fp32 p", True)):
        t = time.time()
        X, steps = block_pcg(A, F, C, rtol, 5000, rounded)
        true = np.linalg.norm(F - A @ X, axis=0) / np.linalg.norm(F, axis=0)
        out[name] = (X, steps)
        log(f"{name}: steps per column {steps.tolist()}  largest {steps.max()}  true relres max {true.max():.3e}  ({time.time() - t:.1f}s)")
    (X0, s0), (X1, s1) = out["fp64 p"], out["fp32 p"]
    log(f"max rel diff of x: {np.max(np.abs(X1 - X0)) / np.max(np.abs(X0)):.2e}   steps {s0.max()} -> {s1.max()}")
    return s0, s1


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "S"
    rtol = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-8
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    if which == "fixture":
        from remo3d_amd.meshgen import make_mesh

        def zones(c):
            m = np.where(c[:, 2] > 1.0, 2, 1)
            m[np.hypot(c[:, 0], c[:, 1]) < 0.1] = 0
            return m.astype(np.int32)
        mesh = make_mesh(3, 50.0, [0.0, 0.1, -0.1], scale=8.0, material_fn=zones, seed=0)
        study(mesh, [1.0, 0.1, 0.02], FIXTURE_SRC[:k], rtol)
        return
    import bench
    w = bench.build_workload(0, 1, k, bench.SIZES[which])["work"][0]
    study(w["mesh"], np.asarray(w["sigma"], float), w["sources"][:k], rtol)


if __name__ == "__main__":
    main()
