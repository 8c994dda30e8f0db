"""Worker of tests/test_inversion_cpu.py: one inversion with the analytic stand-in context, alone or as one of two gloo ranks under
torchrun; writes the final table (hex: bit for bit), the accepted / rejected sequence and its share of the batches."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from remo3d_amd import sweep  # noqa: E402
from _inversion_standin import TOOLS, example_model, provider  # noqa: E402


def main():
    out_path = sys.argv[1]
    depths = np.arange(3.0, 13.0, 1.0)
    sim = dict(domain_radius=12.0, batch_size=5, mesh_provider=provider)
    m = example_model()          # initialize_workers joins the process group under torchrun (REMO_DIST_BACKEND=gloo)
    m.simulate_logs(depths, verbose=False, sensitivities=True, **sim)
    obs = {t: m.logs[t][:, 1].copy() for t in TOOLS}
    m.formation_model[[0, 1, 2], 4] *= [2.0, 0.5, 1.5]
    inv = m.invert_logs(obs, depths, free="RTUZ", solver_kw=sim, max_iterations=12, warm_start=False)
    res = dict(rank=sweep.rank(), world=sweep.world_size(), table=[float(v).hex() for v in m.formation_model.ravel()],
               accepted=[bool(h["accepted"]) for h in inv.history], my_batches=int(m.timing["my_batches"]))
    with open("{}.{}".format(out_path, sweep.rank()), "w") as f:
        json.dump(res, f)
    sweep.barrier()


if __name__ == "__main__":
    main()
