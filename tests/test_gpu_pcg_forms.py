"""Every form of the PCG step's update and direction launches (pcg_kernels.hip), forced by its remo_debug_tune keys on meshes small
enough for a test: the same potentials, true residuals and step counts as the same batch solved with the CSR product."""
import numpy as np
import pytest

from conftest import SIGMA3
from test_gpu_parity import EVAL, SRC, _hub_mesh

# update launch: key 9 = first Chebyshev step inside it (the folded form), 31 = tile form, 29 = masked slab loads of the row form
UPDATE_FORMS = {"folded": {}, "tile": {9: 0}, "row_masked": {9: 0, 31: 0}, "row_unmasked": {9: 0, 31: 0, 29: 0}}
KEYS = (9, 29, 30, 31)      # 30: direction launch, flat (1) or row (0) form; every default is 1


def _rhs(k):
    """k right-hand sides: SRC / EVAL of the parity tests, then single sources along the axis"""
    zs = np.linspace(-0.3, 0.3, max(k - len(SRC), 0))
    src = list(SRC) + [([float(z)], [1.0]) for z in zs]
    ev = list(EVAL) + [[float(z) + 0.4, float(z) + 6.4] for z in zs]
    return src[:k], ev[:k]


@pytest.fixture(scope="module")
def resident(gpu_ctx, mesh3d):
    """(batch, potentials and step count of the CSR product) per (k, precision): made once, left unchanged"""
    from remo3d_amd import solver
    made = {}

    def get(k, precision):
        if (k, precision) not in made:
            src, ev = _rhs(k)
            b = gpu_ctx.batch(mesh3d, SIGMA3, src, ev)
            assert b.run(solver.make_opts(rtol=1e-11, maxsteps=5000, precision=precision, op="csr")) == 0 and b.stats["op_used"] == 0
            made[(k, precision)] = (b, np.concatenate(b.fetch()), b.stats["pcg_steps"])
        return made[(k, precision)]
    yield get
    for b, _, _ in made.values():
        b.close()


def _run_form(b, ref, ref_steps, precision, update, flat):
    from remo3d_amd import _lib, solver
    L = _lib.load()
    try:
        for key in KEYS:      # a product build that lacks a key fails here instead of running the default
            assert L.remo_debug_tune(key, {30: flat}.get(key, UPDATE_FORMS[update].get(key, 1))) == 0, key
        assert b.run(solver.make_opts(rtol=1e-11, maxsteps=5000, precision=precision, op="patch")) == 0
        assert b.stats["op_used"] == 3
        u, steps = np.concatenate(b.fetch()), b.stats["pcg_steps"]
        relres = np.max(b.true_relres())
    finally:
        for key in KEYS:
            L.remo_debug_tune(key, 1)
    print(update, "flat" if flat else "row", precision, "max rel diff %.3e" % np.max(np.abs(u - ref) / np.maximum(np.abs(ref), 1e-300)), "relres %.3e" % relres,
          "steps", steps, ref_steps)
    assert np.allclose(u, ref, rtol=1e-8, atol=0)
    assert relres < 5e-11
    assert abs(steps - ref_steps) <= max(3, ref_steps // 20), (steps, ref_steps)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("flat", [1, 0])
@pytest.mark.parametrize("update,precision", [(u, "fp64") for u in UPDATE_FORMS] + [("row_masked", "mixed"), ("row_unmasked", "mixed")])
def test_update_and_direction_forms_solve_like_the_csr_path(update, precision, flat, k, resident):
    """The update launch's folded, tile and row (masked / unmasked) kernels, crossed with the direction launch's flat and row
    kernels and 1, 5 and 8 right-hand sides; fp32 storage always takes the row form, so the mixed mode runs those."""
    b, ref, ref_steps = resident(k, precision)
    _run_form(b, ref, ref_steps, precision, update, flat)


@pytest.mark.gpu
@pytest.mark.parametrize("update", ["tile", "row_masked"])
def test_row_of_five_or_more_patches(update, gpu_ctx):
    """8 right-hand sides: 32 elements per patch.  A hub vertex in more than 4 * 32 tetrahedra has its row in at least five patches
    however the elements are ordered: the slots beyond the fourth are the tile form's `more` path and the row form's tail loop."""
    from remo3d_amd import solver
    mesh = _hub_mesh(80)
    assert np.bincount(mesh.conn.ravel()).max() > 4 * (256 // 8)
    zs = np.linspace(-1.4, 1.6, 8)
    b = gpu_ctx.batch(mesh, [0.5, 0.05], [([float(z)], [1.0]) for z in zs], [[float(z) + 0.7, 0.05] for z in zs])
    try:
        assert b.run(solver.make_opts(rtol=1e-11, maxsteps=5000, op="csr")) == 0 and b.stats["op_used"] == 0
        ref, ref_steps = np.concatenate(b.fetch()), b.stats["pcg_steps"]
        _run_form(b, ref, ref_steps, "fp64", update, 1)
    finally:
        b.close()
