"""CPU-side checks of the C-ABI library: it loads without a GPU, exports every symbol the header
declares, fails cleanly when no device exists, and its host-side pieces (reference tensors, dof
numbering / CSR pattern) agree with the oracle.  No GPU compute is attempted here."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, SIGMA3


def _declared(header_name):
    header = open(os.path.join(ROOT, "include", header_name)).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    return set(re.findall(r"\b(remo_[a-z_]+)\s*\(", header))


def test_library_exports_every_declared_symbol():
    """The public header holds the boundary + the inspection hooks and NO debug probes; those live in their own
    header.  The library exports everything either header declares."""
    from remo3d_amd import _lib
    declared, debug = _declared("remo3d_hip.h"), _declared("remo3d_hip_debug.h")
    assert declared and debug, "no declarations parsed"
    assert not any(n.startswith("remo_debug") for n in declared), "debug probes belong in include/remo3d_hip_debug.h"
    assert all(n.startswith("remo_debug") for n in debug)
    L = _lib.load()
    for name in declared | debug:
        assert hasattr(L, name), f"{name} declared in include/ but not exported"
    assert set(_lib.EXPORTS) == declared
    assert set(_lib.DEBUG_EXPORTS) == debug
    assert L.remo_abi_version() == 7


def test_options_defaults_follow_reference():
    from remo3d_amd import solver
    o = solver.make_opts()
    assert o.maxsteps == 1000 and o.condense == 1 and o.preconditioner == 1     # ngsolve_functions.py:50, remo3d.py:82-83
    assert abs(o.rtol - 1e-8) < 1e-20
    with pytest.raises(ValueError):
        solver.make_opts(preconditioner="ilu")


def test_context_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from remo3d_amd import solver
    with pytest.raises(solver.RemoError) as e:
        solver.Context(0)
    assert "HIP device" in str(e.value) or "device" in str(e.value)


@pytest.mark.parametrize("dim", [2, 3])
def test_reference_tensors_match_oracle_quadrature(dim, mesh2d, mesh3d):
    """Global matrix assembled from the library's exactly integrated reference tensors (host code
    path shared with the kernels) == the oracle's per-element quadrature: two independent routes,
    1e-13 of the largest entry."""
    import scipy.sparse as sp
    from oracle.fem_oracle import Oracle
    from remo3d_amd import solver
    mesh = mesh2d if dim == 2 else mesh3d
    o = Oracle(mesh, SIGMA3, condense=False)
    rp, col, val = o.csr()
    A = sp.csr_matrix((val, col, rp), shape=(o.nfree, o.nfree))
    conn = np.sort(mesh.conn, axis=1)
    eld, fid = o.eldof(), o.freeid()
    rows, cols, vals = [], [], []
    for t in range(len(conn)):
        K = solver.host_element_matrix(dim, mesh.coords[conn[t]], SIGMA3[mesh.mat[t]])
        d = fid[eld[t]]
        ok = d >= 0
        rr, cc = np.meshgrid(d[ok], d[ok], indexing="ij")
        rows.append(rr.ravel()); cols.append(cc.ravel()); vals.append(K[np.ix_(ok, ok)].ravel())
    B = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=A.shape)
    assert abs(A - B).max() <= 1e-13 * abs(A).max()


@pytest.mark.parametrize("which,condense", [("2d", True), ("2d", False), ("3d", True)])
def test_host_symbolic_matches_oracle(which, condense, mesh2d, mesh3d):
    from oracle.fem_oracle import Oracle
    from remo3d_amd import solver
    mesh = mesh2d if which == "2d" else mesh3d
    sy = solver.host_symbolic(mesh, condense)
    o = Oracle(mesh, SIGMA3, condense=condense)
    rp, col, _ = o.csr()
    assert sy["n_free"] == o.nfree and sy["nnz"] == o.nnz and sy["n_edges"] == o.ne and sy["n_faces"] == o.nf
    assert np.array_equal(sy["rowptr"], rp) and np.array_equal(sy["col"], col)
    assert np.array_equal(sy["freeid"], o.freeid())


def test_probe_keys_are_not_in_the_product_library():
    """remo_debug_tune: the keys that force one of the product's own paths are always there (return 0); the keys of rejected
    experiments and ablations - some give wrong results on purpose - exist only in the -DREMO_PROBES build and return -1 here."""
    from remo3d_amd import _lib
    L = _lib.load()
    for key, default in ((3, -1), (6, 1), (9, 1), (13, 1), (15, 1), (16, 0), (17, 1), (18, 1), (22, 1), (24, 1), (25, 1), (29, 1), (30, 1), (31, 1), (39, 1), (40, 2), (41, 1), (42, 1), (43, 0)):
        assert L.remo_debug_tune(key, default) == 0, key
    for key in (0, 1, 2, 4, 5, 7, 8, 19, 20, 21, 23, 26, 27, 28, 32, 33, 34, 35, 36, 37, 38, 99):
        assert L.remo_debug_tune(key, 0) == -1, key


def test_no_kernel_of_the_library_uses_scratch_memory():
    """Every kernel of ours in the BUILT library keeps its data in registers and LDS (private segment = 0 bytes in the code objects'
    metadata): round 4 found k_patch_apply storing 48 bytes per lane to scratch - an array of K sums chosen by a run-time index,
    not a spill, so the compiler's summary said "vgpr-spill 0" - which cost 13 % of the operator's time.  rocPRIM's radix sort
    (a library kernel of the numbering phase) is the one exception."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import code_objects
    from remo3d_amd import _lib
    if not os.path.exists(code_objects.READELF):
        pytest.skip("llvm-readelf not in this image")
    ks = code_objects.kernels(_lib.LIB_PATH)
    names = code_objects.demangle([k["name"] for k in ks])
    ours = [(k, d) for k, d in zip(ks, names) if d.startswith("remo::")]
    assert len(ours) > 100, len(ours)
    assert any("k_patch_apply<double, 5" in d for _, d in ours)
    # one kernel per form of the PCG step's update and direction launches (pcg_kernels.hip)
    for form in ("k_pcg_update<double, 5, true", "k_pcg_update<double, 5, false", "k_pcg_update_tile<double, 5", "k_pcg_update_folded<double, 5",
                 "k_pcg_update_x<float, 5", "k_pcg_direction_flat<double, 5", "k_pcg_direction_row<double, 5"):
        assert any(form in d for _, d in ours), form
    bad = ["%s: %d bytes per lane" % (d, k["scratch"]) for k, d in ours if k["scratch"] != 0]
    assert not bad, bad
