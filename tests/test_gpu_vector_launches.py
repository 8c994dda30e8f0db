"""The direction launch beside an fp32 search direction, flat form (k_pcg_direction_flat<double, K, float>: two consecutive values per
lane and access, whole lines of r and p per wave instruction, the first loads requested before the scalars are reduced) against the
row form (k_pcg_direction_row<double, K, float>).

First through remo_debug_direction_forms: ONE launch of each form on the same synthetic vectors, partial sums and scalar block.  No
solve is involved - none of the patch operator's unordered LDS additions - so p and the forwarded scalars are compared BIT FOR BIT.
One input set (drawn once, sliced per case).  A workgroup of the flat form takes 256 values per wave and load set, 16 values per lane
and pass of its loop, so the sizes below end inside a lane's two values, inside a wave, inside a workgroup's pass and behind a
wrapped grid-stride loop.  n K itself is a multiple of K: where a size of the list is none, the next multiple is taken, and a
residue of n K mod 4 that K cannot reach (K = 2: only 0 and 2; K = 8: only 0) is left out.

Then whole solves on the suite's 3D mesh with the flat (key 30 = 1) and the row form (key 30 = 0) of the direction launch, and with the
tile form of the update launch (key 31 = 1: beside an fp32 direction it requests its first tile before it reduces its scalars) and its
row form (key 31 = 0): the patch operator's sums are not bit-reproducible, so these are held to the bounds
tests/test_gpu_direction_fp32.py uses for two runs of this path."""
import ctypes as C

import numpy as np
import pytest

from conftest import SIGMA3

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 5, 8]
TOL2 = 1e-24
NMAX = 20000          # rows of the input set
_IN = {}


def _inputs():
    if not _IN:
        rng = np.random.default_rng(20251)
        _IN["r"] = rng.standard_normal(NMAX * 8)
        _IN["z"] = rng.standard_normal(NMAX * 8)
        _IN["p"] = rng.standard_normal(NMAX * 8).astype(np.float32)
        _IN["dinv"] = rng.uniform(0.2, 3.0, NMAX)
        _IN["part"] = rng.uniform(0.5, 1.5, (2, 1024 * 8)) * 1e-3
        _IN["pq"] = rng.uniform(1.0, 2.0, 8)
        _IN["rz"] = rng.uniform(0.1, 1.0, (2, 8))
    return _IN


def _run(ctx, n, nv, k, grid, step=3, nb_rz=37, done=0, frozen=None):
    """Both forms of one direction launch of `step`; returns (p_in, p_flat, p_row, scal_in, scal_flat, scal_row, zi, beta)."""
    from remo3d_amd import _lib
    L = _lib.load()
    d = _inputs()
    N, NV = n * k, nv * k
    r, z, p, dinv = d["r"][:N].copy(), d["z"][:max(NV, 1)].copy(), d["p"][:N].copy(), d["dinv"][:n].copy()
    part = [d["part"][s][:max(nb_rz, 1) * k].copy() for s in (0, 1)]
    scal = np.zeros(48)
    scal[0:8] = 1e3 * np.arange(1, 9)                 # <Cr0, r0>
    scal[8:16] = d["pq"]
    scal[16:24], scal[24:32] = d["rz"][0], d["rz"][1]  # <Cr, r> of even / odd steps: the launch of `step` reads the set of step & 1
    if frozen is not None:
        scal[16 + 8 * (step & 1) + frozen] = 0.5 * TOL2 * scal[frozen]
    scal[32:33].view(np.int32)[0] = done
    out = [np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(48), np.zeros(48)]
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    rc = L.remo_debug_direction_forms(ctx._h, n, nv, k, grid, step, TOL2, _lib.ptr(r, C.c_double), _lib.ptr(p, C.c_float), _lib.ptr(z, C.c_double),
                                      _lib.ptr(dinv, C.c_double), _lib.ptr(part[0], C.c_double), _lib.ptr(part[1], C.c_double), nb_rz,
                                      _lib.ptr(scal, C.c_double), out[0].ctypes.data_as(fp), out[1].ctypes.data_as(fp),
                                      out[2].ctypes.data_as(dp), out[3].ctypes.data_as(dp))
    assert rc == 0, ctx.last_error()
    zsel = r.copy()
    zsel[:NV] = z[:NV]
    zi = np.repeat(dinv, k) * zsel
    rzn = part[(step + 1) & 1][:nb_rz * k].reshape(nb_rz, k).sum(axis=0)
    rzo = scal[16 + 8 * (step & 1):][:k]
    beta = np.where(rzo > TOL2 * scal[:k], rzn / rzo, 0.0)
    return p, out[0], out[1], scal, out[2], out[3], zi, beta


def _check(res, k, step=3):
    p, pf, pr, scal, sf, sr, zi, beta = res
    assert pf.tobytes() == pr.tobytes(), "p: flat and row form differ in %d of %d values" % (np.count_nonzero(pf.view(np.uint32) != pr.view(np.uint32)), pf.size)
    assert sf.tobytes() == sr.tobytes(), (sf, sr)
    # both forms against the restatement in numpy (the sums of beta in another order: to fp32 rounding, not bit for bit)
    ref = zi + np.tile(beta, pf.size // k) * p.astype(np.float64)
    assert np.all(np.abs(pf - ref) <= 2.0 ** -22 * (np.abs(zi) + np.abs(np.tile(beta, pf.size // k) * p) + 1e-300)), np.max(np.abs(pf - ref))
    # the new <Cr, r> is forwarded to the set of the next step, nothing else in the block moves
    nxt = 16 + 8 * ((step + 1) & 1)
    same = np.ones(48, bool)
    same[nxt:nxt + k] = False
    assert sf[same].tobytes() == scal[same].tobytes()
    assert len(set(np.round(beta, 12))) == k, beta          # beta differs column by column


def _sizes(k):
    """n for the sizes of the list (the next multiple of k at or above each) and one n per reachable residue of n k mod 4."""
    ns = sorted({max(1, -(-t // k)) for t in (1, 3, 255, 257, 1023, 1025)})
    for res in (1, 2, 3):
        hit = [n for n in range(301, 301 + 8) if (n * k) % 4 == res]
        if hit:
            ns.append(hit[0])
    return sorted(set(ns))


@pytest.mark.parametrize("k", KS)
def test_flat_equals_row_small_sizes(k, gpu_ctx):
    """Sizes that end inside a lane's values and inside a wave; vertex rows up to about a third (the z / r boundary inside the launch)."""
    for n in _sizes(k):
        nv = n // 3
        _check(_run(gpu_ctx, n, nv, k, grid=(n + 255) // 256), k)


@pytest.mark.parametrize("k", KS)
def test_grid_stride_wraps_twice_and_ends_ragged(k, gpu_ctx):
    """Two workgroups, n k = 2 * 256 * 4 * 4 * 2 + 3 (k = 1; else the next multiple of k): two full passes of the loop and a ragged third."""
    n = -(-(2 * 256 * 4 * 4 * 2 + 3) // k)
    assert n * k >= 16387 and n * k % 16 != 0
    _check(_run(gpu_ctx, n, n // 5, k, grid=2), k)


@pytest.mark.parametrize("k", KS)
def test_vertex_row_boundary(k, gpu_ctx):
    """nv = 0, nv = n, and nv k = 1, 2, 3 mod 4 where k reaches it: the boundary between z and r inside one lane's two values; with 700
    rows some waves lie wholly below it (z loaded), one across, the rest above (the z load skipped as a whole wave instruction)."""
    n = 700
    nvs = [0, n] + [next(nv for nv in range(101, 109) if (nv * k) % 4 == res) for res in (1, 2, 3) if any((nv * k) % 4 == res for nv in range(101, 109))]
    for nv in nvs:
        _check(_run(gpu_ctx, n, nv, k, grid=3), k)


@pytest.mark.parametrize("nb_rz", [1, 255, 256, 257, 700, 1024])
def test_partial_rows(nb_rz, gpu_ctx):
    """The partial sums of the update launch, 1 to 1024 rows: one to four rows per thread of the head, the last round partly empty."""
    _check(_run(gpu_ctx, 1000, 300, 5, grid=4, nb_rz=nb_rz), 5)
    _check(_run(gpu_ctx, 1000, 300, 5, grid=4, nb_rz=nb_rz, step=4), 5, step=4)


@pytest.mark.parametrize("k", KS)
def test_frozen_column(k, gpu_ctx):
    """<Cr, r> of the last column below tol^2 <Cr0, r0>: beta = 0 there, and its p is float(d z) exactly."""
    res = _run(gpu_ctx, 1000, 300, k, grid=4, frozen=k - 1)
    p, pf, pr, scal, sf, sr, zi, beta = res
    assert pf.tobytes() == pr.tobytes() and sf.tobytes() == sr.tobytes()
    assert beta[k - 1] == 0.0
    assert pf[k - 1::k].tobytes() == zi[k - 1::k].astype(np.float32).tobytes()
    if k > 1:
        assert np.any(pf[0::k] != zi[0::k].astype(np.float32))


@pytest.mark.parametrize("done", [1, 3])
def test_finished_solve_stores_nothing(done, gpu_ctx):
    """Done word set to a step <= the launch's (3): p and the scalar block come back byte for byte; 4 (a later step) does not stop it."""
    p, pf, pr, scal, sf, sr, _, _ = _run(gpu_ctx, 1000, 300, 5, grid=4, done=done)
    assert pf.tobytes() == p.tobytes() and pr.tobytes() == p.tobytes()
    assert sf.tobytes() == scal.tobytes() and sr.tobytes() == scal.tobytes()
    p, pf, pr, scal, sf, sr, _, _ = _run(gpu_ctx, 1000, 300, 5, grid=4, done=4)
    assert pf.tobytes() == pr.tobytes() and pf.tobytes() != p.tobytes()


@pytest.fixture(scope="module")
def tune():
    """remo_debug_tune for the solves: key 9 = 0 (the first Chebyshev step as a launch of its own: with it folded into the update launch
    a vertex block this small keeps the fp64 direction); every key back to the product's default at the end."""
    from remo3d_amd import _lib
    L = _lib.load()
    assert L.remo_debug_tune(9, 0) == 0
    try:
        yield L.remo_debug_tune
    finally:
        for key, default in ((9, 1), (30, 1), (31, 1)):
            L.remo_debug_tune(key, default)


SRC = [([0.0], [1.0]), ([0.1], [1.0]), ([-0.1, 0.1], [1.0, -1.0]), ([0.0], [2.0]), ([0.1], [0.5])]
EVAL = [[0.4, 6.4, -2.0], [2.1, 2.6], [0.5, 3.0, 0.0], [0.4], [1.0, 2.0]]


@pytest.mark.parametrize("key", [30, 31])
@pytest.mark.parametrize("k", [5, 3])
def test_solves_with_either_form_agree(k, key, mesh3d, gpu_ctx, tune):
    """The 3D fixture (28 298 tetrahedra), patch operator, rtol 1e-12: the direction launch's flat (key 30 = 1) against its row form
    (key 30 = 0), and the update launch's tile form - first loads requested before the scalars - (key 31 = 1) against its row form
    (key 31 = 0): step counts within max(3, 3 %) of each other, potentials within 1e-9 of the largest, the direction in fp32 in both."""
    from remo3d_amd import solver
    runs = {}
    try:
        for flat in (1, 0):
            assert tune(key, flat) == 0
            o, st, rc = gpu_ctx.solve_batch(mesh3d, SIGMA3, SRC[:k], EVAL[:k], solver.make_opts(rtol=1e-12, maxsteps=20000, op="patch"))
            assert rc == 0, gpu_ctx.last_error()
            assert st["op_used"] == 3 and gpu_ctx.direction_bytes() == 4
            runs[flat] = (o, st["pcg_steps"])
    finally:
        tune(key, 1)
    (new, s1), (old, s0) = runs[1], runs[0]
    scale = max(np.max(np.abs(b)) for b in old)
    diff = max(np.max(np.abs(a - b)) for a, b in zip(new, old))
    print("k=%d key %d: steps %d, with the row form %d; max difference %.2e of the largest potential" % (k, key, s1, s0, diff / scale))
    assert all(np.all(np.isfinite(a)) for a in new)
    assert abs(s1 - s0) <= max(3.0, 0.03 * s0), (s1, s0)
    assert diff <= 1e-9 * scale, (diff, scale)
