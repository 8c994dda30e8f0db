"""Windowing of the global borehole / formation model to the simulation sphere of one batch:
the build's own restatement of remo3d/gmsh_functions.py:10-174 (SelectGmshDataRange and its two
helpers).  Output frame: depth relative to the batch's combined depth, z positive downwards.

Quirks of the reference that are kept because they define its results (pinned by
tests/golden/windows_*.json, generated from the reference in this container):
  * the borehole polyline keeps one extra sample on each side of the window (3-tap dilation);
  * in dipping models the borehole window is a slab |z| < R, not a sphere;
  * layers are kept when either boundary is closer than 0.99 R to the window centre, measured
    perpendicular to the (dipping) boundary; flushed zones that do not reach into that radius are
    merged into the undisturbed zone;
  * the first / last layer is stretched to +-1.01 R (times sqrt(1 + tan^2 dip) when dipping).
"""
from __future__ import annotations

import numpy as np


def _segment_circle_hit(p1, p2, radius):
    """Intersection of segment p1->p2 (rows are (z, r)) with the circle z^2 + r^2 = radius^2 that
    lies strictly inside the segment (gmsh_functions.py:12-25)."""
    x1, y1 = p1[1], p1[0]
    x2, y2 = p2[1], p2[0]
    dx, dy = x2 - x1, y2 - y1
    dr2 = dx * dx + dy * dy
    D = x1 * y2 - x2 * y1
    disc = radius ** 2 * dr2 - D ** 2
    for sign in (-1, 1):
        x = (D * dy + sign * np.sign(dy) * dx * np.sqrt(disc)) / dr2
        y = (-D * dx + sign * np.abs(dy) * np.sqrt(disc)) / dr2
        p = np.array([y, x])
        t = np.dot(p1 - p2, p1 - p)
        if 0 < t < np.dot(p1 - p2, p1 - p2):
            return p
    return None


def window_borehole(borehole_geometry, dip, depth, R):
    """Local borehole wall polyline [(z, radius)] clipped to the domain (gmsh_functions.py:10-90)."""
    bg = np.asarray(borehole_geometry, dtype=float)
    if bg.shape[0] == 2:
        loc = bg.copy()
    else:
        if dip == 0:
            inside = (bg[:, 0] - depth) ** 2 + bg[:, 1] ** 2 < R ** 2
        else:
            inside = np.abs(bg[:, 0] - depth) < R
        grown = inside.copy()
        grown[:-1] |= inside[1:]
        grown[1:] |= inside[:-1]
        loc = bg[grown, :].copy()
    loc[:, 0] -= depth

    def on_or_in(z, r):
        if dip == 0:
            q = z * z + r * r
            return (q == R * R), (q < R * R)
        return (abs(z) == R), (abs(z) < R)

    for end in (0, -1):
        nxt = 1 if end == 0 else -2
        z, r = loc[end]
        on, inn = on_or_in(z, r)
        sgn = -1.0 if end == 0 else 1.0
        if on:
            continue
        if inn:  # extend straight up / down to the domain boundary at the same radius
            if dip == 0:
                omega = np.arccos(r / R)
                new = np.array([sgn * np.sin(omega) * R, r])
            else:
                new = np.array([sgn * R, r])
            loc = np.vstack((new, loc)) if end == 0 else np.vstack((loc, new))
        else:    # pull the outside point back onto the boundary
            if dip == 0:
                loc[end, :] = _segment_circle_hit(loc[end, :], loc[nxt, :], R)
            else:
                a = abs(loc[end, 0]) - R
                b = R - sgn * loc[nxt, 0]
                loc[end, :] = [sgn * R, (b * loc[end, 1] + a * loc[nxt, 1]) / (a + b)]
    return loc


def window_formation(formation_parameters, dip, depth, R, active_geometry_window=0.99):
    """Local layer table [(top, bottom, fz_radius)] and the resistivity list in material order
    (gmsh_functions.py:92-165)."""
    fp = np.asarray(formation_parameters, dtype=float)
    active = R * active_geometry_window
    loc = fp.copy()
    loc[:, :2] -= depth
    if dip == 0:
        a = 0.0
        dist = np.abs(loc[:, :2])
    else:
        a = np.tan(dip)
        dist = np.abs(loc[:, :2]) / np.sqrt(a * a + 1.0)
    layers = loc[np.any(dist < active, axis=1), :]

    has_fz = ~np.isnan(layers[:, 2])
    if dip == 0:
        xs = np.repeat(layers[has_fz, 2][:, None], 2, axis=1)
        ys = layers[has_fz, :2]
    else:
        xs = np.repeat(layers[has_fz, 2][:, None], 4, axis=1)
        xs[:, :2] *= -1
        ys = a * xs + np.hstack([layers[has_fz, :2], layers[has_fz, :2]])
    reach = np.any(np.sqrt(xs ** 2 + ys ** 2) < active, axis=1)
    drop = has_fz.copy()
    drop[has_fz] = ~reach

    model = layers.copy()
    with_res = fp.shape[1] == 5
    if with_res:
        model[drop, 4] = model[drop, 3]
        model[drop, 2:4] = np.nan
    else:
        model[drop, 2] = np.nan
    stretch = R * 1.01 if dip == 0 else R * np.sqrt(a * a + 1.0) * 1.01
    if model[0, 0] > -stretch:
        model[0, 0] = -stretch
    if model[-1, 1] < stretch:
        model[-1, 1] = stretch
    if not with_res:
        return model
    res = model[:, 3:5].ravel()
    return model[:, :3], res[~np.isnan(res)]


def select_data_range(borehole_geometry, formation_parameters, dip, mud_resistivity, depth, R, active_geometry_window=0.99):
    """(local_formation_geometry, local_borehole_geometry, sigma) with sigma = [1/Rm] + 1/R_zones
    (gmsh_functions.py:168-174); the order of sigma is the material numbering of the mesh."""
    bh = window_borehole(borehole_geometry, dip, depth, R)
    fg, res = window_formation(formation_parameters, dip, depth, R, active_geometry_window)
    sigma = [1.0 / mud_resistivity] + list(1.0 / res)
    return fg, bh, sigma


def ti_conductivity(sigma_h, sigma_v, dip_rad, dim):
    """[n, dim, dim] conductivity tensors of transversely isotropic materials: Sigma = sigma_h I + (sigma_v - sigma_h) n n^T with
    n the bedding normal.  3D local frame: the bedding planes are z + x tan(dip) = const (meshgen.layered_material_fn), so
    n = (sin dip, 0, cos dip); 2D (r, z), dip 0: diag(sigma_h, sigma_v).  A material with sigma_v == sigma_h is exactly sigma_h I."""
    sh = np.atleast_1d(np.asarray(sigma_h, dtype=float))
    sv = np.atleast_1d(np.asarray(sigma_v, dtype=float))
    if sh.shape != sv.shape:
        raise ValueError("sigma_h and sigma_v differ in length")
    if dim == 2:
        if dip_rad != 0:
            raise ValueError("the axisymmetric (2D) model has no dip")
        n = np.array([0.0, 1.0])
    elif dim == 3:
        n = np.array([np.sin(dip_rad), 0.0, np.cos(dip_rad)])
    else:
        raise ValueError("dim must be 2 or 3")
    P = np.outer(n, n)
    # sigma_h (I - n n^T) + sigma_v n n^T: the same tensor, with the principal values exact when the normal is a coordinate axis
    S = sh[:, None, None] * (np.eye(dim) - P) + sv[:, None, None] * P
    iso = sh == sv
    S[iso] = sh[iso, None, None] * np.eye(dim)
    return S


# ---------------------------------------------------------------------------------------------
# Materials of a window <-> entries of the formation table (sensitivities, Model.simulate_logs)


def entry_id_table(formation_parameters):
    """5-column copy of the formation table whose resistivity columns hold entry identifiers 1 + 2 * layer (RTFZ) and
    2 + 2 * layer (RTUZ) instead of resistivities, NaN kept where the table has NaN.  Windowed like the table itself
    (select_data_range / select_netgen_data_range) it names the table entry behind every material: see material_entries."""
    fp = np.asarray(formation_parameters, dtype=float)
    ids = np.array(fp[:, :5], copy=True)
    layer = np.arange(fp.shape[0], dtype=float)
    for c in (3, 4):
        ids[:, c] = np.where(np.isnan(fp[:, c]), np.nan, 1.0 + 2.0 * layer + (c - 3))
    return ids


def material_entries(sigma_of_ids):
    """(layer, table column) of every material, from the `sigma` list a windowing function returned for entry_id_table(...):
    None for the mud (material 0), else (layer, 3) for RTFZ or (layer, 4) for RTUZ.  Every quirk of the windowing applies to the
    identifiers as it does to the resistivities (a dropped flushed zone: the layer's one material is its RTFZ entry)."""
    out = [None]
    for s in list(sigma_of_ids)[1:]:
        k = int(round(1.0 / float(s))) - 1
        out.append((k // 2, 3 + k % 2))
    return out


def resistivity_sensitivity(dJ, entries, formation_parameters, scale, normal=None):
    """Chain rule from dJ/dsigma of the materials of one window to the table's resistivities, for one functional:
    returns (dRa/dR [n_layers, n_cols], dRa/dRm) with dRa/dR = scale * sum_{materials of the entry} dJ/dsigma * (-1 / R^2) and
    scale = sign(K J) K (/ 2 in 3D).  The columns follow the table from column 2 on (RDFZ, RTFZ, RTUZ, and RVUZ when present): RDFZ
    is a radius, not a resistivity, and stays NaN; entries no material of the window holds are 0, NaN where the table has NaN.
    dJ: [n_mat] (scalar sigma) or [n_mat, dim, dim] symmetric G with dJ = G : dSigma (tensor sigma).  For a tensor material
    dJ/dsigma_h = G : (I - n n^T) and dJ/dsigma_v = G : n n^T with `normal` the bedding normal of ti_conductivity; with an RVUZ
    column the undisturbed zone's sigma_h = 1 / RTUZ and sigma_v = 1 / RVUZ (RVUZ NaN: isotropic, all of it goes to RTUZ)."""
    fp = np.asarray(formation_parameters, dtype=float)
    dJ = np.asarray(dJ, dtype=float)
    out = np.where(np.isnan(fp[:, 2:]), np.nan, 0.0)
    out[:, 0] = np.nan
    has_rv = fp.shape[1] >= 6

    def parts(g):
        if g.ndim == 0:
            return float(g), 0.0, float(g)     # (d/dsigma_h, d/dsigma_v, d/dsigma of an isotropic material)
        n = np.asarray(normal, dtype=float)
        P = np.outer(n, n)
        gv = float(np.sum(g * P))
        return float(np.trace(g)) - gv, gv, float(np.trace(g))

    mud = scale * parts(dJ[0])[2]              # d/dsigma_mud; the caller applies -1 / Rm^2
    for m, e in enumerate(entries):
        if e is None:
            continue
        layer, col = e
        gh, gv, giso = parts(dJ[m])
        R = fp[layer, col]
        if col == 4 and has_rv and not np.isnan(fp[layer, 5]):
            out[layer, 2] += scale * gh * (-1.0 / R ** 2)
            out[layer, 3] += scale * gv * (-1.0 / fp[layer, 5] ** 2)
        else:
            out[layer, col - 2] += scale * giso * (-1.0 / R ** 2)
    return out, mud


# ---------------------------------------------------------------------------------------------
# Sensitivity maps: the elements of a batch's mesh binned on an (r, z) grid (Model.simulate_logs(sensitivity_grid=...))


def sensitivity_cells(mesh, mat, grid, z_offset=0.0):
    """Groups of elements for Context.solve_batch_sens_groups: one group per (material, grid cell) pair that occurs.
    grid: dict with the edges, in metres, of the depth axis `z` and of one lateral axis: `r`, the distance from the borehole axis
    (2D: the mesh's r; 3D: hypot(x, y)), or in 3D `x`, the signed x of the dip plane (y summed).  z is absolute depth in the
    formation table's sense, measured along the borehole axis: the mesh lives in the frame of its batch (depth relative to the
    batch's combined depth), and z_offset - that combined depth - undoes it, so one grid serves every batch of a sweep.
    An element belongs to the cell that holds its centroid (cells are half-open, [lo, hi)); elements whose centroid lies outside
    the grid go to one "rest" pseudo-cell with index n_z * n_r.  mat: the material of every element (None: mesh.mat).
    Returns (group [n_elems] int32 - compact ids 0 .. n_group - 1 -, group_material [n_group], group_cell [n_group]) with
    cell = iz * n_r + ir; every group is material-pure."""
    coords = np.asarray(mesh.coords, dtype=float)
    conn = np.asarray(mesh.conn)
    mat = np.asarray(mesh.mat if mat is None else mat, dtype=np.int64)
    dim = coords.shape[1]
    if mat.shape != (conn.shape[0],):
        raise ValueError("mat must hold one material per element")
    lateral = [k for k in ("r", "x") if k in grid]
    if len(lateral) != 1 or "z" not in grid:
        raise ValueError("grid must hold the edges of 'z' and of one of 'r' and 'x'")
    if lateral[0] == "x" and dim != 3:
        raise ValueError("the 'x' axis exists in 3D only")
    ez = np.asarray(grid["z"], dtype=float)
    eh = np.asarray(grid[lateral[0]], dtype=float)
    for e in (ez, eh):
        if e.ndim != 1 or e.size < 2 or np.any(np.diff(e) <= 0):
            raise ValueError("grid edges must be increasing, two at least")
    cen = coords[conn].mean(axis=1)
    z = cen[:, dim - 1] + float(z_offset)
    if lateral[0] == "x":
        h = cen[:, 0]
    else:
        h = np.abs(cen[:, 0]) if dim == 2 else np.hypot(cen[:, 0], cen[:, 1])
    n_z, n_h = ez.size - 1, eh.size - 1
    iz = np.searchsorted(ez, z, side="right") - 1
    ih = np.searchsorted(eh, h, side="right") - 1
    inside = (iz >= 0) & (iz < n_z) & (ih >= 0) & (ih < n_h)
    cell = np.where(inside, iz * n_h + ih, n_z * n_h)
    pair, group = np.unique(mat * (n_z * n_h + 1) + cell, return_inverse=True)
    return group.astype(np.int32).ravel(), pair // (n_z * n_h + 1), pair % (n_z * n_h + 1)


def field_points(grid, dim, z_offset=0.0):
    """Points of a section for Context.solve_batch_field, in the frame of a batch.  grid: dict with the point COORDINATES (not edges),
    in metres, of the depth axis `z` and of one lateral axis: `r` (2D: the mesh's r; 3D: x >= 0 in the dip plane y = 0) or in 3D `x`,
    the signed x of the dip plane.  z is absolute depth along the borehole axis as in sensitivity_cells; z_offset - the batch's
    combined depth - takes it to the batch's frame.  Returns [n_z * n_h, dim], z outermost: point iz * n_h + ih."""
    if dim not in (2, 3):
        raise ValueError("dim must be 2 or 3")
    lateral = [k for k in ("r", "x") if k in grid]
    if len(lateral) != 1 or "z" not in grid:
        raise ValueError("grid must hold the coordinates of 'z' and of one of 'r' and 'x'")
    if lateral[0] == "x" and dim != 3:
        raise ValueError("the 'x' axis exists in 3D only")
    z = np.asarray(grid["z"], dtype=float)
    h = np.asarray(grid[lateral[0]], dtype=float)
    for c in (z, h):
        if c.ndim != 1 or c.size < 1 or not np.all(np.isfinite(c)):
            raise ValueError("grid coordinates must be finite 1-D arrays, one point at least")
    if lateral[0] == "r" and np.any(h < 0):
        raise ValueError("'r' is a distance from the borehole axis: it cannot be negative")
    pts = np.zeros((z.size, h.size, dim))
    pts[:, :, 0] = h[None, :]
    pts[:, :, dim - 1] = (z - float(z_offset))[:, None]
    return pts.reshape(-1, dim)


# ---------------------------------------------------------------------------------------------
# Netgen path (2D only): remo3d/netgen_functions.py:12-118


def _segment_circle_hit_side(p1, p2, radius, side):
    """Like _segment_circle_hit, restricted to the upper (z < 0) or lower (z > 0) half
    (netgen_functions.py:14-29)."""
    x1, y1 = p1[1], p1[0]
    x2, y2 = p2[1], p2[0]
    dx, dy = x2 - x1, y2 - y1
    dr2 = dx * dx + dy * dy
    D = x1 * y2 - x2 * y1
    disc = radius ** 2 * dr2 - D ** 2
    for sign in (-1, 1):
        x = (D * dy + sign * np.sign(dy) * dx * np.sqrt(disc)) / dr2
        y = (-D * dx + sign * np.abs(dy) * np.sqrt(disc)) / dr2
        p = np.array([y, x])
        t = np.dot(p1 - p2, p1 - p)
        if ((side == "top" and y < 0) or (side == "bottom" and y > 0)) and 0 < t < np.dot(p1 - p2, p1 - p2):
            return p
    return None


def select_netgen_data_range(borehole_geometry, formation_parameters, mud_resistivity, depth, R, active_geometry_window=0.999):
    """Windowing of the reference's default 2D path (mesh_generator "netgen", remo3d.py:776-779):
    returns (local_formation_geometry [L, 5] = top, bottom, fz_radius, region numbers left / right,
    local_borehole_geometry [B, 2], sigma).  Quirks kept because they define the reference's inputs:
    the position of the borehole end points relative to the domain is tested with z^2 + r (radius NOT
    squared, netgen_functions.py:43-62); the active radius is 0.999 R; a flushed zone is dropped only if
    both inner corners AND the connecting line lie outside the active radius; the first / last layer is
    cut at the borehole polyline's end points instead of being stretched."""
    bg = np.asarray(borehole_geometry, dtype=float)
    fp = np.asarray(formation_parameters, dtype=float)
    if bg.shape[0] == 2:
        loc = bg.copy()
    else:
        inside = (bg[:, 0] - depth) ** 2 + bg[:, 1] ** 2 < R ** 2
        grown = inside.copy()
        grown[:-1] |= inside[1:]
        grown[1:] |= inside[:-1]
        loc = bg[grown, :].copy()
    loc[:, 0] -= depth
    for end, side in ((0, "top"), (-1, "bottom")):
        nxt = 1 if end == 0 else -2
        sgn = -1.0 if end == 0 else 1.0
        q = loc[end, 0] ** 2 + loc[end, 1]          # sic: radius not squared
        if np.isclose(q, R ** 2):
            continue
        if q < R ** 2:
            omega = np.arccos(loc[end, 1] / R)
            new = np.array([sgn * np.sin(omega) * R, loc[end, 1]])
            loc = np.vstack((new, loc)) if end == 0 else np.vstack((loc, new))
        else:
            loc[end, :] = _segment_circle_hit_side(loc[end, :], loc[nxt, :], R, side)

    active = R * active_geometry_window
    rel = fp[:, :2] - depth
    point_within = np.any(rel ** 2 <= active ** 2, axis=1)
    line_across = np.all(rel ** 2 > active ** 2, axis=1) & (fp[:, 0] < depth) & (fp[:, 1] > depth)
    model = fp[point_within | line_across, :].copy()
    model[:, :2] -= depth
    has_fz = ~np.isnan(model[:, 2])
    top_out = model[:, 0] ** 2 + model[:, 2] ** 2 >= active ** 2
    bot_out = model[:, 1] ** 2 + model[:, 2] ** 2 >= active ** 2
    line_out = ~((model[:, 0] < 0) & (model[:, 1] > 0) & (model[:, 2] < active))
    drop = has_fz & top_out & bot_out & line_out
    model[drop, 2] = np.nan
    model[drop, 4] = model[drop, 3]
    model[drop, 3] = np.nan
    if model[0, 0] != loc[0, 0]:
        model[0, 0] = loc[0, 0]
    if model[-1, 1] != loc[-1, 0]:
        model[-1, 1] = loc[-1, 0]
    grid = np.empty((model.shape[0], 2))
    region = 2
    for i in range(model.shape[0]):
        if np.isnan(model[i, 3]):
            grid[i, :] = region
            region += 1
        else:
            grid[i, 0] = region
            grid[i, 1] = region + 1
            region += 2
    res = model[:, 3:5].ravel()
    res = res[~np.isnan(res)]
    sigma = [1.0 / mud_resistivity] + list(1.0 / res)
    return np.hstack((model[:, :3], grid)), loc, sigma
