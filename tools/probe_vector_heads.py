#!/usr/bin/env python3
"""How long a workgroup of the PCG's two vector launches (k_pcg_direction_flat, k_pcg_update_tile) spends on its scalars before its
first stored value: clocks of wave 0 of every workgroup (remo_debug_vector_heads), on one-shot solves of headline batches.
Needs the probes build: make -C remo3d_amd/csrc probes; REMO_LIB=remo3d_amd/libremo3d_hip_probes.so
   python tools/probe_vector_heads.py [SIZE [BATCHES]]      (default L 2)"""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench


def main():
    size = sys.argv[1] if len(sys.argv) > 1 else "L"
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    t0 = time.time()
    work = bench.build_workload(0, 1, 100, bench.SIZES[size], max_batches=nb)["work"]
    print("%d batches of size %s built in %.1f s" % (len(work), size, time.time() - t0), flush=True)
    from remo3d_amd import _lib, solver
    L = _lib.load()
    with solver.Context(0) as ctx:
        for bi, w in enumerate(work):
            for rep in range(2):
                assert L.remo_debug_vector_heads(ctx._h, 1, None) == 0, ctx.last_error()
                _, st, rc = ctx.solve_batch(w["mesh"], w["sigma"], w["sources"], w["evals"], solver.make_opts(rtol=1e-8, maxsteps=1000))
                out = (C.c_double * 8)()
                assert L.remo_debug_vector_heads(ctx._h, 0, out) == 0, ctx.last_error()
                print("batch %d run %d: rc %d, %d steps, direction bytes %d, n %d" % (bi, rep, rc, st["pcg_steps"], ctx.direction_bytes(), st["n_free"]))
                for name, o in (("direction", 0), ("update", 4)):
                    print("   %-9s head %8.0f ticks of %8.0f per workgroup (wave 0), mean share %.3f, %d workgroups" %
                          (name, out[o], out[o + 1], out[o + 2], int(out[o + 3])), flush=True)


if __name__ == "__main__":
    main()
