"""Multi-electrode arrays and focused readings: the algebra between the matrix of transfer impedances and a log.

A galvanic array of m point electrodes is described by Z [m, m], Z_ij the potential at electrode i per unit current at electrode j.
A MODE of the array says which electrodes inject fixed currents, which carry bucking currents that a focusing condition determines,
which potential combinations that condition nulls, and which combination is read:

    mode = dict(inject={name: I}, bucking=[{name: share}, ...], null=[{name: weight}, ...], read={name: weight}, K=None)

With I_f [m] the injected currents, S [m, n_b] the share columns (one bucking unknown each), N [n_b, m] the null conditions,
w [m] the read weights and I0 = sum(inject):

    M = N Z S,   c = -M^-1 N Z I_f,   I = I_f + S c,   V = Z I,   y = w . V,   Ra = |K y / I0|.

The derivative of y needs no differentiation of the small solve: dy = w_hat^T dZ I with w_hat = w - N^T M^-T S^T Z^T w.
Only entries Z_ij with i a read / null electrode and j a current electrode of the mode are ever used - a point electrode has no
potential of its own, so a read or null electrode that carries current in the same mode is refused.
K = None is the factor that makes Ra = R in a homogeneous full space: the same algebra on Z0_ij = 1 / (4 pi |z_i - z_j|).
"""
from __future__ import annotations

import numpy as np

_MODE_KEYS = {"inject", "bucking", "null", "read", "K"}


class ModeMatrices:
    """I_f [m], S [m, n_b], N [n_b, m], w [m], I0 and K of one mode; rows / cols: the electrodes whose potentials / currents it uses."""

    def __init__(self, I_f, S, N, w, K):
        self.I_f, self.S, self.N, self.w, self.K = I_f, S, N, w, K
        self.I0 = float(np.sum(I_f))
        self.cols = (I_f != 0.0) | np.any(S != 0.0, axis=1)
        self.rows = (w != 0.0) | np.any(N != 0.0, axis=0)


def focus(Z, mm: ModeMatrices):
    """(I [m], V [m], y, w_hat [m]) of one mode on the impedances Z [m, m]: the bucking currents that null the mode's conditions, the
    potentials V = Z I (meaningful at the mode's read / null electrodes), the reading y = w . V and the weights of its derivative,
    dy = w_hat^T dZ I.  Entries of Z the mode does not use may be anything (NaN included).  A singular focusing system is a ValueError."""
    Z = np.where(mm.rows[:, None] & mm.cols[None, :], np.asarray(Z, dtype=np.float64), 0.0)
    n_b = mm.S.shape[1]
    I = mm.I_f.copy()
    w_hat = mm.w.copy()
    if n_b > 0:
        M = mm.N @ Z @ mm.S
        scale = np.max(np.abs(M))
        if not np.all(np.isfinite(M)) or scale == 0.0 or np.linalg.cond(M) > 1e12:
            raise ValueError("the focusing conditions do not determine the bucking currents (singular N Z S)")
        c = -np.linalg.solve(M, mm.N @ Z @ mm.I_f)
        I = I + mm.S @ c
        w_hat = w_hat - mm.N.T @ np.linalg.solve(M.T, mm.S.T @ (Z.T @ mm.w))
    V = Z @ I
    return I, V, float(mm.w @ V), w_hat


class ElectrodeArray:
    """electrodes: dict name -> offset [m] from the record point, positive downwards; modes: dict name -> mode (see the module)."""

    def __init__(self, electrodes, modes):
        self.names = list(electrodes)
        self.offsets = np.array([float(electrodes[n]) for n in self.names])
        m = len(self.names)
        if m < 2:
            raise ValueError("an array needs at least two electrodes")
        if not np.all(np.isfinite(self.offsets)) or len(np.unique(self.offsets)) != m:
            raise ValueError("electrode offsets must be finite and distinct (coinciding electrodes)")
        if not modes:
            raise ValueError("an array needs at least one mode")
        self.modes = {name: dict(mode) for name, mode in modes.items()}
        self._matrices = {name: self._build(name, mode) for name, mode in self.modes.items()}
        for name, mm in self._matrices.items():      # K = None: Ra = R in a homogeneous full space
            if mm.K is None:
                y0 = focus(self.full_space_impedances(1.0), mm)[2]
                if y0 == 0.0 or not np.isfinite(y0):
                    raise ValueError("mode {!r} reads nothing in a homogeneous full space: give K".format(name))
                mm.K = abs(mm.I0 / y0)

    def _vector(self, mode_name, what, d):
        v = np.zeros(len(self.names))
        for n, x in dict(d).items():
            if n not in self.names:
                raise ValueError("mode {!r}: {} names the unknown electrode {!r}".format(mode_name, what, n))
            v[self.names.index(n)] += float(x)
        return v

    def _build(self, name, mode):
        unknown = set(mode) - _MODE_KEYS
        if unknown:
            raise ValueError("mode {!r}: unknown keys {}".format(name, sorted(unknown)))
        m = len(self.names)
        I_f = self._vector(name, "inject", mode.get("inject") or {})
        bucking, null = list(mode.get("bucking") or []), list(mode.get("null") or [])
        if len(bucking) != len(null):
            raise ValueError("mode {!r}: {} bucking unknowns need as many null conditions, not {}".format(name, len(bucking), len(null)))
        S = np.array([self._vector(name, "bucking", b) for b in bucking]).reshape(len(bucking), m).T
        N = np.array([self._vector(name, "null", c) for c in null]).reshape(len(null), m)
        w = self._vector(name, "read", mode.get("read") or {})
        mm = ModeMatrices(I_f, S, N, w, None if mode.get("K") is None else float(mode["K"]))
        if mm.I0 == 0.0:
            raise ValueError("mode {!r}: the injected currents sum to zero (I0 = 0)".format(name))
        if not np.any(w != 0.0):
            raise ValueError("mode {!r} reads no electrode".format(name))
        both = mm.rows & mm.cols
        if np.any(both):
            raise ValueError("mode {!r}: electrode {!r} is read or nulled and carries current - a point electrode has no potential of its own"
                             .format(name, self.names[int(np.argmax(both))]))
        return mm

    def matrices(self, mode) -> ModeMatrices:
        return self._matrices[mode]

    @property
    def current_electrodes(self):
        """Mask [m]: the electrodes some mode makes carry current."""
        return np.any([mm.cols for mm in self._matrices.values()], axis=0)

    @property
    def potential_electrodes(self):
        """Mask [m]: the electrodes some mode reads or nulls."""
        return np.any([mm.rows for mm in self._matrices.values()], axis=0)

    def full_space_impedances(self, R=1.0):
        """Z0_ij = R / (4 pi |z_i - z_j|) of point electrodes in a homogeneous full space of resistivity R; the diagonal is NaN."""
        d = np.abs(self.offsets[:, None] - self.offsets[None, :])
        with np.errstate(divide="ignore"):
            Z0 = float(R) / (4.0 * np.pi * d)
        Z0[np.diag_indices_from(Z0)] = np.nan
        return Z0

    def apparent_resistivity(self, mode, Z, half=False):
        """(Ra, I [m], w_hat [m]) of one mode on Z.  half: the potentials are those of twice the current (the 3D half ball with its
        sources in the symmetry plane), so y is halved."""
        mm = self._matrices[mode]
        I, _, y, w_hat = focus(Z, mm)
        return abs(mm.K * (0.5 * y if half else y) / mm.I0), I, w_hat


def build_batches(array: ElectrodeArray, measurement_depths, batch_size: int):
    """(combined_depths [n_batches], batches): batch_size consecutive depths per batch, as tasks.build_batches lays out the tools'.
    A batch is centred, like a tool's, on its current electrodes: the simulated depth of a record is its measurement depth plus the
    mean offset of the array's current electrodes.  Every depth is one tasks.Solve whose electrodes [2, m] are the array's, in
    the array's order, in the batch frame, with the current flags of the modes; batch.electrodes is their union (tasks._merge)."""
    from . import tasks
    md = np.asarray(measurement_depths, dtype=float)
    flags = array.current_electrodes.astype(float)
    centre = float(np.mean(array.offsets[array.current_electrodes]))
    sim = np.round(md + centre, decimals=4)
    nb = int(np.ceil(sim.size / batch_size))
    grid = np.pad(sim, (0, nb * batch_size - sim.size), mode="constant", constant_values=np.nan).reshape(nb, batch_size)
    combined = np.round(np.nanmean(grid, axis=1), decimals=4)
    offsets = np.round(grid - combined[:, None], decimals=4)
    batches = []
    for bi in range(nb):
        batch = tasks.Batch(bi, float(combined[bi]), np.zeros((2, 0)))
        cur, pot = [], []
        for di in range(batch_size):
            if np.isnan(grid[bi, di]):
                break
            off = float(offsets[bi, di])
            el = np.round(np.vstack([array.offsets - centre + off, flags]), 4)
            cur += list(el[0, el[1] != 0]); pot += list(el[0, el[1] == 0])
            batch.solves.append(tasks.Solve(bi * batch_size + di, el, [tasks.Record(bi * batch_size + di, 0, off)]))
        batch.electrodes = tasks._merge(pot, cur)
        batches.append(batch)
    return combined, batches


def laterolog7(a0m1=0.36, a0m2=0.46, a0a1=1.0) -> ElectrodeArray:
    """The symmetric seven-electrode sonde A1' M2' M1' A0 M1 M2 A1 (offsets in metres from A0).  Mode "LL7": A0 injects 1, one bucking
    unknown shared half and half by the guards A1 and A1', found from (M1 + M1') / 2 = (M2 + M2') / 2; the reading is the mean of the
    four monitors.  Mode "A0": the same reading with no bucking current, the unfocused curve."""
    if not 0.0 < a0m1 < a0m2 < a0a1:
        raise ValueError("laterolog7 needs 0 < a0m1 < a0m2 < a0a1")
    electrodes = {"A1'": -a0a1, "M2'": -a0m2, "M1'": -a0m1, "A0": 0.0, "M1": a0m1, "M2": a0m2, "A1": a0a1}
    read = {"M1": 0.25, "M1'": 0.25, "M2": 0.25, "M2'": 0.25}
    modes = {"LL7": dict(inject={"A0": 1.0}, bucking=[{"A1": 0.5, "A1'": 0.5}], null=[{"M1": 0.5, "M1'": 0.5, "M2": -0.5, "M2'": -0.5}], read=read),
             "A0": dict(inject={"A0": 1.0}, read=read)}
    return ElectrodeArray(electrodes, modes)
