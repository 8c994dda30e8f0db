"""Model.simulate_array_logs on the GPU: a three-electrode array is the lateral tool; the focusing condition holds through the
solver; the sensitivities of both laterolog modes against central differences of their logs.

Measured on MI355X (the tests print every figure before they assert):
  focusing, Example_01, two depths, rtol 1e-12: potentials of the focused currents against Z I 5.07e-13 / 8.09e-13, null condition
    1.32e-13 / 2.33e-14 (bound: ten times the largest);
  homogeneous 1 ohm m copy against 1 ohm m (bound: twice the tool's error): tool A0.4M6.0N 3.82e-05, LL7 5.97e-05, A0 5.43e-05;
  sensitivities against central differences at +-0.1 % (bound 1e-5), worst over LL7 and A0: 2D RTFZ 6.82e-08, RTUZ 1.94e-07, mud
    1.19e-07; 3D RTUZ 4.12e-09, mud 6.23e-08.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EX1 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Example_01", "Input")
BM3 = os.path.join(os.path.dirname(__file__), "golden", "examples", "Benchmark models", "Benchmark model 3")
TOOL = "A0.4M6.0N"
STEP = 1e-3          # +-0.1 % of the entry
SENS_BOUND = 1e-5    # measure and bound of the Model test in tests/test_gpu_sensitivity.py (same solver settings)
FOCUS_BOUND = 8.1e-12   # 10 x the largest measured value (8.09e-13); the starting bound was the project's 1e-6 bar for a potential
TIGHT = dict(rtol=1e-12, maxsteps=20000)


def _example01():
    f = np.loadtxt(os.path.join(EX1, "Formation.txt"), skiprows=2)
    b = np.loadtxt(os.path.join(EX1, "Borehole.txt"), skiprows=2)
    b[:, 1] *= 1e-3      # CALM in mm
    return f, b


def _cached_provider(scale):
    """The meshes depend on geometry and electrodes only: every run of a case shares them."""
    from remo3d_amd.model import default_mesh_provider
    inner, cache = default_mesh_provider(scale=scale), {}

    def provider(dim, R, batch, fg, bh, dip):
        key = (batch.index, batch.electrodes.tobytes())
        if key not in cache:
            cache[key] = inner(dim, R, batch, fg, bh, dip)
        return cache[key]
    return provider


def _model(f, b, dip=0, factory=None):
    from remo3d_amd.model import Model
    m = Model([TOOL])
    m.set_model_parameters(f, b, borehole_geometry_type="diameter", dip=dip)
    m.initialize_workers(cpu_workers=1, gpu_workers=1, context_factory=factory)
    return m


def test_a_three_electrode_array_is_the_lateral_tool():
    """The array with the electrodes of tools.tool_table("A0.4M6.0N") at depth + shift + table[0, :3], inject A, read N - M,
    K = table[0, 3]: the same electrodes and flags in every batch, hence the same mesh, window and right-hand side as simulate_logs
    with batch_size = 1, and the same log to 1e-12 relative (2D, CSR product)."""
    from remo3d_amd import arrays, tools
    f, b = _example01()
    t = tools.tool_table(TOOL)
    names = []
    for s in t[1, :3]:
        names.append("A" if s != 0 else ("M" if "M" not in names else "N"))
    arr = arrays.ElectrodeArray({n: float(t[1, 3] + z) for n, z in zip(names, t[0, :3])},
                                {"lateral": dict(inject={"A": 1.0}, read={"N": 1.0, "M": -1.0}, K=float(t[0, 3]))})
    depths = np.array([8.3, 12.45])
    m = _model(f, b)
    try:
        kw = dict(batch_size=1, mesh_provider=_cached_provider(1.0), verbose=False, solver_options=dict(op="csr"))
        m.simulate_logs(depths, **kw)
        assert m.timing["failed_batches"] == 0, m.timing["first_error"]
        m.simulate_array_logs(arr, depths, **kw)
        assert m.timing["failed_batches"] == 0, m.timing["first_error"]
    finally:
        m.shutdown_workers()
    tool, got = m.logs[TOOL], m.array_logs["lateral"]
    print("ARRAYS lateral: tool %s array %s" % (tool[:, 1], got[:, 1]))
    assert np.array_equal(got[:, 0], tool[:, 0]) and np.all(tool[:, 1] > 0)
    assert np.max(np.abs(got[:, 1] / tool[:, 1] - 1.0)) <= 1e-12


def test_focusing_holds_through_the_solver():
    """laterolog7 on Example_01, two depths, rtol 1e-12.  Per depth one further solve on the batch's mesh with ALL current electrodes at
    the currents the focusing found, read at the four monitors, against Z I from array_impedances, relative to the largest monitor
    potential; the null condition of LL7 then holds in that solve.  Measured: 8.09e-13 (potentials), 1.32e-13 (null condition)."""
    from remo3d_amd import arrays, solver
    seen = []

    class Recording(solver.Context):
        def solve_batch_pairs(self, mesh, sigma, sources, evals, pairs, opts=None, **kw):
            seen.append((mesh, sigma))
            return super().solve_batch_pairs(mesh, sigma, sources, evals, pairs, opts, **kw)

    f, b = _example01()
    arr = arrays.laterolog7()
    depths = np.array([8.3, 12.45])
    kw = dict(batch_size=1, mesh_provider=_cached_provider(1.0), verbose=False, **TIGHT)
    m = _model(f, b, factory=Recording)
    try:
        m.simulate_array_logs(arr, depths, **kw)
        assert m.timing["failed_batches"] == 0, m.timing["first_error"]
        assert len(seen) == 2
        cur, mon = np.flatnonzero(arr.current_electrodes), np.flatnonzero(arr.potential_electrodes)
        batches = arrays.build_batches(arr, depths, 1)[1]
        worst = 0.0
        for di, (mesh, sigma) in enumerate(list(seen)):
            z = batches[di].solves[0].electrodes[0]
            I = m.array_currents["LL7"][di]
            outs, _, st, rc = m.ctx.solve_batch_pairs(mesh, sigma, [(z[cur], I[cur])], [z[mon]], [], solver.make_opts(**TIGHT), far_field=50.0)
            assert rc == 0
            V = np.nan_to_num(m.array_impedances[di]) @ I
            err = float(np.max(np.abs(outs[0] - V[mon])) / np.max(np.abs(V[mon])))
            null = abs(arr.matrices("LL7").N[0, mon] @ outs[0]) / np.max(np.abs(outs[0]))
            print("ARRAYS focusing depth %.2f: currents %s  potentials vs Z I %.2e  null condition %.2e  Ra LL7 %.4f A0 %.4f"
                  % (depths[di], I[cur], err, null, m.array_logs["LL7"][di, 1], m.array_logs["A0"][di, 1]))
            worst = max(worst, err, float(null))
        assert worst <= FOCUS_BOUND
    finally:
        m.shutdown_workers()


_HOMOGENEOUS = {}


def _homogeneous():
    """Example_01 with every resistivity 1 ohm m, mud included, two depths: (error of the tool A0.4M6.0N against 1 ohm m, the array
    logs per mode, the array) on the same sweep settings."""
    if not _HOMOGENEOUS:
        from remo3d_amd import arrays
        f, b = _example01()
        f[:, 3:] = np.where(np.isnan(f[:, 3:]), np.nan, 1.0)
        b[:, 2] = 1.0
        arr = arrays.laterolog7()
        depths = np.array([8.3, 12.45])
        m = _model(f, b)
        try:
            kw = dict(batch_size=1, mesh_provider=_cached_provider(1.0), verbose=False, **TIGHT)
            m.simulate_logs(depths, **kw)
            assert m.timing["failed_batches"] == 0, m.timing["first_error"]
            m.simulate_array_logs(arr, depths, **kw)
            assert m.timing["failed_batches"] == 0, m.timing["first_error"]
        finally:
            m.shutdown_workers()
        _HOMOGENEOUS.update(e_tool=float(np.max(np.abs(m.logs[TOOL][:, 1] - 1.0))), logs={k: v[:, 1] for k, v in m.array_logs.items()}, arr=arr)
    return _HOMOGENEOUS["e_tool"], _HOMOGENEOUS["logs"], _HOMOGENEOUS["arr"]


def test_homogeneous_model_reads_one_ohm_m_within_twice_the_tools_error():
    """In a homogeneous 1 ohm m copy of the model both modes read 1 ohm m within twice the error of the plain tool A0.4M6.0N on the
    same sweep settings (the factor is slack for the different electrode spacings).  The array reads potentials, not differences:
    what makes this hold is that they are taken against infinity (solver.far_field_reference), not against the grounded surface of
    the batch mesh at 50 m - against that surface LL7 and A0 were 1.42e-02 and 8.13e-03 off (I_total / (4 pi 50 m)), the tool, whose
    difference u_N - u_M cancels the constant, 3.82e-05."""
    e_tool, logs, _ = _homogeneous()
    e_ll7, e_a0 = float(np.max(np.abs(logs["LL7"] - 1.0))), float(np.max(np.abs(logs["A0"] - 1.0)))
    print("ARRAYS homogeneous 1 ohm m: tool %s %.2e  LL7 %.2e  A0 %.2e" % (TOOL, e_tool, e_ll7, e_a0))
    assert e_ll7 <= 2.0 * e_tool and e_a0 <= 2.0 * e_tool


def _sensitivity_case(label, f, b, dip, depths, radius, scale, entries):
    """array_sensitivities / array_mud_sensitivity of both modes against central differences of array_logs at +-0.1 % of the table
    entries `entries` and of the mud; the difference relative to the record's largest |R dRa/dR|."""
    from remo3d_amd import arrays
    arr = arrays.laterolog7()
    provider = _cached_provider(scale)
    kw = dict(domain_radius=radius, batch_size=1, mesh_provider=provider, verbose=False, **TIGHT)

    def run(ff, bb, **more):
        m = _model(ff, bb, dip=dip)
        try:
            m.simulate_array_logs(arr, depths, **dict(kw, **more))
        finally:
            m.shutdown_workers()
        assert m.timing["failed_batches"] == 0, m.timing["first_error"]
        return m
    base = run(f, b, sensitivities=True)
    plain = run(f, b)
    mud = np.interp(depths, base.borehole_model[:, 0], base.borehole_model[:, 2])      # batch_size 1, symmetric array: the batch centre is the depth
    worst = 0.0
    for mode in arr.modes:
        assert np.allclose(base.array_logs[mode], plain.array_logs[mode], rtol=1e-9, atol=0.0)
    for what in list(entries) + ["mud"]:
        runs = []
        for sgn in (1, -1):
            ff, bb = f.copy(), b.copy()
            if what == "mud":
                bb[:, 2] *= 1 + sgn * STEP
            else:
                ff[what[0], what[1]] *= 1 + sgn * STEP
            runs.append(run(ff, bb))
        for mode in arr.modes:
            fd = (runs[0].array_logs[mode][:, 1] - runs[1].array_logs[mode][:, 1]) / (2 * STEP)      # R dRa/dR
            s = base.array_sensitivities[mode]
            scale_rec = np.maximum(np.max(np.abs(np.nan_to_num(s[:, :, 1:] * f[None, :, 3:])), axis=(1, 2)), 1e-300)
            if what == "mud":
                got = base.array_mud_sensitivity[mode] * mud
                scale_rec = np.maximum(scale_rec, np.abs(got))
            else:
                got = s[:, what[0], what[1] - 2] * f[what[0], what[1]]
            err = float(np.max(np.abs(got - fd) / scale_rec))
            print("ARRAYS %s %s entry %s: reciprocity %s  differences %s  -> %.2e" % (label, mode, what, got, fd, err))
            worst = max(worst, err)
    return base, worst


def test_array_sensitivities_2d_against_central_differences():
    """Example_01, two depths: dRa/dRTFZ of layer 1, dRa/dRTUZ of layer 3 and dRa/dRm of LL7 and A0."""
    f, b = _example01()
    base, worst = _sensitivity_case("2D", f, b, 0, np.array([8.3, 12.45]), 50.0, 1.0, [(1, 3), (3, 4)])
    print("ARRAYS 2D worst %.2e" % worst)
    for mode in ("LL7", "A0"):
        assert base.array_sensitivities[mode].shape == (2, f.shape[0], 3)
    assert worst <= SENS_BOUND


def test_array_sensitivities_3d_against_central_differences():
    """Benchmark model 3 at dip 30, one depth, domain_radius 12, mesh_scale 2.5: dRa/dRTUZ of the resistive bed and dRa/dRm."""
    f = np.loadtxt(os.path.join(BM3, "Formation_BM3_30.txt"), skiprows=2)
    b = np.loadtxt(os.path.join(BM3, "Borehole_BM3.txt"), skiprows=2)
    b[:, 1] *= 1e-3
    base, worst = _sensitivity_case("3D", f, b, 30, np.array([6.0]), 12.0, 2.5, [(1, 4)])
    print("ARRAYS 3D worst %.2e" % worst)
    assert base.array_sensitivities["LL7"].shape == (1, f.shape[0], f.shape[1] - 2)
    assert worst <= SENS_BOUND
