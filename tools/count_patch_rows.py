#!/usr/bin/env python3
"""Distinct free rows per patch of the patch operator, counted on the CPU for patches of E and 2 E elements.

The element list is cut in the device's order (symbolic_gpu.hip: vertices of an element ascending, elements by a stable sort on
(smallest vertex, second smallest vertex)) into patches of E consecutive elements.  A patch's rows are its distinct free dofs:
one per vertex, two per edge, one per face (P3); a dof on a Dirichlet boundary face has no row.

    python tools/count_patch_rows.py [--batch 0] [--size L] [--elements 51,102]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def entity_rows(mesh):
    """[T, 20] distinct row labels per element dof (-1 = constrained), in the device's element order."""
    conn = np.sort(np.asarray(mesh.conn, dtype=np.int64), axis=1)
    nv = int(mesh.coords.shape[0])
    order = np.lexsort((conn[:, 1], conn[:, 0]))      # stable: ties keep the caller's order
    conn = conn[order]
    T = conn.shape[0]
    ea, eb = np.array([0, 0, 0, 1, 1, 2]), np.array([1, 2, 3, 2, 3, 3])
    fa, fb, fc = np.array([0, 0, 0, 1]), np.array([1, 1, 2, 2]), np.array([2, 3, 3, 3])
    ekey = (conn[:, ea] * nv + conn[:, eb]).ravel()
    fkey = ((conn[:, fa] * nv + conn[:, fb]) * nv + conn[:, fc]).ravel()
    eu, eid = np.unique(ekey, return_inverse=True)
    fu, fid = np.unique(fkey, return_inverse=True)
    ne = eu.size
    # Dirichlet: every vertex, edge and face of a boundary face that carries the flag
    b = np.sort(np.asarray(mesh.bconn, dtype=np.int64)[np.asarray(mesh.bdirichlet).astype(bool)], axis=1)
    vcons = np.zeros(nv, dtype=bool); vcons[b.ravel()] = True
    bek = np.concatenate([b[:, 0] * nv + b[:, 1], b[:, 0] * nv + b[:, 2], b[:, 1] * nv + b[:, 2]])
    econs = np.isin(eu, bek)
    fcons = np.isin(fu, (b[:, 0] * nv + b[:, 1]) * nv + b[:, 2])
    eid, fid = eid.reshape(T, 6), fid.reshape(T, 4)
    rows = np.empty((T, 20), dtype=np.int64)
    rows[:, 0:4] = np.where(vcons[conn], -1, conn)
    e0 = np.where(econs[eid], -1, nv + 2 * eid)
    rows[:, 4:16:2] = e0
    rows[:, 5:16:2] = np.where(e0 < 0, -1, e0 + 1)
    rows[:, 16:20] = np.where(fcons[fid], -1, nv + 2 * ne + fid)
    n_rows = int((~vcons).sum() + 2 * (~econs).sum() + (~fcons).sum())
    return rows, n_rows


def count(rows, n_rows, E):
    T = rows.shape[0]
    npatch = (T + E - 1) // E
    patch = np.repeat(np.arange(T) // E, 20)
    r = rows.ravel()
    keep = r >= 0
    pairs = np.unique(patch[keep] * (n_rows + rows.max() + 2) + r[keep])      # distinct (patch, row)
    per_patch = np.bincount(pairs // (n_rows + rows.max() + 2), minlength=npatch)
    slots = np.bincount(np.unique(pairs % (n_rows + rows.max() + 2), return_inverse=True)[1])
    return dict(E=E, T=T, patches=npatch, patch_rows=int(per_patch.sum()), rows_per_element=per_patch.sum() / T,
                mean=per_patch.mean(), max=int(per_patch.max()), rows=int(slots.size), slots_per_row=per_patch.sum() / slots.size,
                rows_with_5_or_more_slots=int((slots >= 5).sum()), rows_of_one_patch=int((slots == 1).sum()),
                padded_to_16=int(((per_patch + 15) // 16 * 16).sum()),
                over_612=int((per_patch > 612).sum()), over_1226=int((per_patch > 1226).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--size", default="L")
    ap.add_argument("--elements", default="51,102")
    a = ap.parse_args()
    import bench
    w = bench._build_some((100, bench.SIZES[a.size], "lattice", [a.batch]))[0]
    rows, n_rows = entity_rows(w["mesh"])
    print("bench sweep batch %d, size %s: T = %d, free rows = %d" % (a.batch, a.size, rows.shape[0], n_rows))
    for E in (int(v) for v in a.elements.split(",")):
        c = count(rows, n_rows, E)
        print("E = %(E)3d: %(patches)d patches, %(patch_rows)d patch rows = %(rows_per_element).3f per element, %(slots_per_row).3f per matrix row; "
              "per patch mean %(mean).1f max %(max)d; padded to 16: %(padded_to_16)d; rows of one patch alone %(rows_of_one_patch)d, "
              "with 5 or more slots %(rows_with_5_or_more_slots)d; patches over 612 rows %(over_612)d, over 1226 %(over_1226)d" % c)


if __name__ == "__main__":
    main()
