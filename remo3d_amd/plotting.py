"""Picture of a model and its synthetic logs: what the reference draws at the end of `save_results` (remo3d.py:993-1147) - the
formation as resistivity-coloured polygons (dipping layers, invasion zones, the borehole with its caliper) beside one or more
tracks of apparent-resistivity logs, saved as `Results_plot.png`.  Same keywords and defaults as the reference; unlike it this
module neither changes `Model.logs` (the reference overwrites them with the smoothed curves) nor the formation table (the reference
stretches its first and last row in place).  matplotlib is imported on first use, with a non-interactive backend if none is set."""
import os

import numpy as np


def _limits_of_logs(curves):
    """The reference's automatic resistivity range (remo3d.py:1015-1024): the extremes of everything in the log tables, rounded
    outwards to two significant digits of the maximum.  (Its scan runs over whole tables, depth column included; kept.)"""
    hi = max(float(np.nanmax(c)) for c in curves)
    lo = min(float(np.nanmin(c)) for c in curves)
    unit = 10.0 ** (np.floor(np.log10(hi)) - 1)
    return [float(np.floor(lo / unit) * unit), float(np.ceil(hi / unit) * unit)]


def model_polygons(formation, borehole, dip_deg, depth_lim, rad_lim):
    """(polygons, resistivities): one quadrilateral per layer spanning the picture, sheared by the dip; on top of it the invaded
    zone of a layer that has one (columns of the formation table: top, bottom, invasion radius, flushed-zone and virgin
    resistivity - remo3d.py:344-548); last the borehole between the mirrored caliper curves, coloured by its mean mud resistivity.
    The first and last layer are extended so that the sheared picture is filled (remo3d.py:1031-1032).  An optional sixth column
    (RVUZ, the vertical resistivity of an anisotropic layer) is not drawn: the virgin zone shows RTUZ."""
    f = np.array(np.asarray(formation, dtype=float)[:, :5], dtype=float, copy=True)
    slope = np.tan(np.deg2rad(dip_deg))
    f[0, 0] -= slope * rad_lim[1]
    f[-1, 1] += slope * rad_lim[1]
    polys, res = [], []

    def sheared(r0, r1, top, bottom):
        return np.array([[r0, top + slope * r0], [r0, bottom + slope * r0], [r1, bottom + slope * r1], [r1, top + slope * r1]])
    for top, bottom, r_inv, *rho in f:
        rho = [v for v in rho if not np.isnan(v)]
        polys.append(sheared(rad_lim[0], rad_lim[1], top, bottom))
        res.append(rho[-1])                                   # virgin zone (the table's last resistivity)
        if not np.isnan(r_inv):
            polys.append(sheared(-r_inv, r_inv, top, bottom))
            res.append(rho[0])                                # flushed zone
    if borehole is not None:
        b = np.asarray(borehole, dtype=float)
        polys.append(np.vstack([np.column_stack([-b[:, 1], b[:, 0]]), np.column_stack([b[:, 1], b[:, 0]])[::-1]]))
        res.append(float(np.mean(b[:, 2])))
    return polys, np.asarray(res)


def smoothed(log, factor):
    """Cubic resampling of one (depth, value) table to `factor` times its points (display only)."""
    if factor <= 1:
        return log
    from scipy.interpolate import interp1d
    z = np.linspace(log[:, 0].min(), log[:, 0].max(), int(log.shape[0] * factor))
    return np.column_stack([z, interp1d(log[:, 0], log[:, 1], kind="cubic")(z)])


def plot_results(model, path=None, plot_layout="auto", plot_depth_lim="auto", plot_aspect_ratio="auto", model_rad_lim="auto",
                 model_res_lim="auto", logs_res_lim="auto", logs_at_nan="break", logs_interpolation_factor=1, logs_colours="auto"):
    """Draws `model` (a remo3d_amd.Model with logs) and returns the matplotlib figure; `path`: also written there as PNG."""
    if logs_at_nan not in ("break", "continue"):
        raise ValueError('logs_at_nan paramater has to be set to "break" or "continue"')
    import matplotlib
    if not os.environ.get("MPLBACKEND") and not os.environ.get("DISPLAY"):
        matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt
    from matplotlib import ticker
    from matplotlib.collections import PatchCollection
    from matplotlib.patches import Polygon

    formation, borehole = model.formation_model, model.borehole_model
    logs = {k: smoothed(np.asarray(v, dtype=float), logs_interpolation_factor) for k, v in model.logs.items()}
    if plot_depth_lim == "auto":
        plot_depth_lim = [float(np.nanmin(formation[:, :2])), float(np.nanmax(formation[:, :2]))]
    if model_rad_lim == "auto":
        if np.all(np.isnan(formation[:, 2])):
            reach = 10.0 * float(np.nanmax(borehole[:, 1]))
        else:
            reach = 2.0 * float(np.nanmax(formation[:, 2]))
        model_rad_lim = [-reach, reach]
    if logs_res_lim == "auto":
        logs_res_lim = _limits_of_logs(list(logs.values()))
    if plot_aspect_ratio == "auto":
        plot_aspect_ratio = (plot_depth_lim[1] - plot_depth_lim[0]) / 25.0 * 1.25
    tracks = [list(logs.keys())] if plot_layout == "auto" else [list(t) for t in plot_layout]

    polys, res = model_polygons(formation, borehole, model.dip_deg, plot_depth_lim, model_rad_lim)
    width = 5 + 5 * len(tracks)
    style = {"font.size": 14, "axes.labelsize": 14, "axes.titlesize": 14, "xtick.labelsize": 14, "ytick.labelsize": 14, "axes.titlepad": 14,
             "xtick.major.size": 10, "xtick.minor.size": 5, "ytick.major.size": 10, "ytick.minor.size": 5}
    with plt.rc_context(style):
        fig, axes = plt.subplots(1, 1 + len(tracks), sharey=True, figsize=[width, width * plot_aspect_ratio], facecolor="white")
        picture = PatchCollection([Polygon(p, closed=True) for p in polys], cmap=matplotlib.colormaps["viridis"])
        picture.set_array(res)
        if model_res_lim != "auto":
            picture.set_clim(model_res_lim)
        left = axes[0]
        left.add_collection(picture)
        left.plot([0, 0], plot_depth_lim, color="black")
        left.margins(x=0, y=0)
        left.set_xlim(model_rad_lim)
        left.set_ylim(plot_depth_lim)
        left.invert_yaxis()
        left.minorticks_on()
        left.set_title("Formation model\ndip = %s\N{DEGREE SIGN}\n" % model.dip_deg)
        left.set_xlabel("Radial distance [m]", labelpad=10)
        left.set_ylabel("Depth [m]", labelpad=10)
        marks = left.get_xticks()
        left.xaxis.set_major_locator(ticker.FixedLocator(marks))
        left.set_xticklabels(["%.2f" % abs(t) for t in marks])
        left.xaxis.set_ticks_position("top")
        left.xaxis.set_label_position("top")
        cycle = plt.rcParams["axes.prop_cycle"].by_key()["color"]
        for t, names in enumerate(tracks):
            colours = cycle if logs_colours == "auto" else logs_colours[t]
            base = axes[1 + t]
            for i, name in enumerate(names):
                ax = base if i == 0 else base.twiny()
                curve = logs[name]
                if logs_at_nan == "continue":
                    curve = curve[~np.isnan(curve[:, 1])]
                colour = colours[i % len(colours)]
                ax.plot(curve[:, 1], curve[:, 0], color=colour)
                ax.set_xlabel(name + "\n[ohmm]", color=colour, labelpad=-8)
                ax.spines["top"].set_color(colour)
                ax.spines["top"].set_position(("outward", i * 55 + 10))
                ax.set_xticks(logs_res_lim)
                ax.tick_params(axis="x", color=colour)
                ax.set_xlim(logs_res_lim)
                ax.xaxis.set_label_position("top")
                ax.xaxis.set_ticks_position("top")
            base.grid(True)
            base.margins(x=0, y=0)
        bar = fig.colorbar(picture, ax=axes, location="bottom", orientation="horizontal", pad=0.05, label="Resistivity [ohmm]",
                           shrink=min(1.0, plot_aspect_ratio))
        bar.ax.minorticks_on()
        if path is not None:
            fig.savefig(path, bbox_inches="tight")
    return fig


def plot_sensitivity_map(model, tool, depth_index, path=None):
    """One picture of model.sensitivity_maps[tool][depth_index] (Model.simulate_logs(sensitivity_grid=...)): d ln Ra / d ln R per
    cell as a pcolormesh on a symmetric-log colour scale, depth downwards, with the bed boundaries and the borehole wall drawn
    over it.  Returns the figure; `path`: also written there."""
    return _draw_sensitivity_map(model, model.sensitivity_maps[tool][depth_index], tool, float(model.logs[tool][depth_index, 0]), path)


def plot_array_sensitivity_map(model, mode, depth_index, path=None):
    """The same picture of model.array_sensitivity_maps[mode][depth_index] (Model.simulate_array_logs(sensitivity_grid=...)): what the
    mode of the array - a focused laterolog, say - sees where."""
    return _draw_sensitivity_map(model, model.array_sensitivity_maps[mode][depth_index], mode, float(model.array_logs[mode][depth_index, 0]), path)


def _draw_sensitivity_map(model, cells, name, depth, path):
    import matplotlib
    if not os.environ.get("MPLBACKEND") and not os.environ.get("DISPLAY"):
        matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt
    from matplotlib.colors import SymLogNorm
    grid = model.sensitivity_grid
    lateral = "x" if "x" in grid else "r"
    m = np.asarray(cells, dtype=float)
    top = float(np.nanmax(np.abs(m))) if np.any(np.isfinite(m)) else 1.0
    top = top if top > 0 else 1.0
    fig, ax = plt.subplots(figsize=(5, 7))
    mesh = ax.pcolormesh(grid[lateral], grid["z"], m, cmap="RdBu_r", norm=SymLogNorm(linthresh=1e-4 * top, vmin=-top, vmax=top), shading="flat")
    slope = np.tan(np.deg2rad(model.dip_deg)) if lateral == "x" else 0.0
    h = np.array([grid[lateral][0], grid[lateral][-1]])
    for z in np.unique(np.asarray(model.formation_model, dtype=float)[:, :2]):      # bed boundaries (sheared by the dip in the x view)
        ax.plot(h, z + slope * h, color="k", lw=0.6)
    bh = np.asarray(model.borehole_model, dtype=float)
    for sgn in ((1.0, -1.0) if h[0] < 0 else (1.0,)):
        ax.plot(sgn * bh[:, 1], bh[:, 0], color="k", lw=0.9)
    ax.set_xlim(h[0], h[1])
    ax.set_ylim(grid["z"][-1], grid["z"][0])
    ax.set_xlabel("{} [m]".format(lateral))
    ax.set_ylabel("depth [m]")
    ax.set_title("{} at {:.2f} m: d ln Ra / d ln R".format(name, depth))
    fig.colorbar(mesh, ax=ax)
    if path is not None:
        fig.savefig(path, dpi=120)
    return fig


def plot_error_map(model, tool, depth_index, path=None):
    """One picture of model.error_maps[tool][depth_index] (Model.simulate_logs(error_grid=...)): the share of the reading's error
    estimate made in every cell as a pcolormesh on a logarithmic colour scale, depth downwards, with the bed boundaries and the
    borehole wall drawn over it; the title carries the estimated relative error.  Returns the figure; `path`: also written there."""
    import matplotlib
    if not os.environ.get("MPLBACKEND") and not os.environ.get("DISPLAY"):
        matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt
    from matplotlib.colors import LogNorm
    grid = model.error_grid
    lateral = "x" if "x" in grid else "r"
    m = np.asarray(model.error_maps[tool][depth_index], dtype=float)
    top = float(np.nanmax(m)) if np.any(np.isfinite(m)) else 1.0
    top = top if top > 0 else 1.0
    fig, ax = plt.subplots(figsize=(5, 7))
    mesh = ax.pcolormesh(grid[lateral], grid["z"], np.where(m > 0, m, np.nan), cmap="magma", norm=LogNorm(vmin=1e-6 * top, vmax=top), shading="flat")
    slope = np.tan(np.deg2rad(model.dip_deg)) if lateral == "x" else 0.0
    h = np.array([grid[lateral][0], grid[lateral][-1]])
    for z in np.unique(np.asarray(model.formation_model, dtype=float)[:, :2]):      # bed boundaries (sheared by the dip in the x view)
        ax.plot(h, z + slope * h, color="w", lw=0.6)
    bh = np.asarray(model.borehole_model, dtype=float)
    for sgn in ((1.0, -1.0) if h[0] < 0 else (1.0,)):
        ax.plot(sgn * bh[:, 1], bh[:, 0], color="w", lw=0.9)
    ax.set_xlim(h[0], h[1])
    ax.set_ylim(grid["z"][-1], grid["z"][0])
    ax.set_xlabel("{} [m]".format(lateral))
    ax.set_ylabel("depth [m]")
    ax.set_title("{} at {:.2f} m: share of the estimate {:.2e}".format(tool, float(model.logs[tool][depth_index, 0]),
                                                                      float(model.error_estimates[tool][depth_index])))
    fig.colorbar(mesh, ax=ax)
    if path is not None:
        fig.savefig(path, dpi=120)
    return fig


def _uniform_axis(c):
    c = np.asarray(c, dtype=float)
    return c.size < 3 or np.allclose(np.diff(c), (c[-1] - c[0]) / (c.size - 1), rtol=1e-6, atol=0.0)


def _resample(values, src, dst, axis):
    """Linear interpolation of `values` along `axis` from the coordinates src to dst (NaN stays NaN where it is met)."""
    moved = np.moveaxis(values, axis, -1)
    out = np.empty(moved.shape[:-1] + (dst.size,))
    for idx in np.ndindex(moved.shape[:-1]):
        out[idx] = np.interp(dst, src, moved[idx])
    return np.moveaxis(out, -1, axis)


def plot_field_section(model, tool, depth_index, path=None):
    """One picture of model.field_sections[tool] for the record at measurement depth `depth_index`
    (Model.simulate_logs(field_grid=...)): filled contours of log10 |u| and the streamlines of the current density J over the
    resistivity model (model_polygons), the energised electrodes marked.  matplotlib's streamplot needs an evenly spaced grid: a
    section on other coordinates (e.g. geometric in r) is resampled linearly to as many evenly spaced points for the streamlines.
    Returns the figure; `path`: also written there."""
    import matplotlib
    if not os.environ.get("MPLBACKEND") and not os.environ.get("DISPLAY"):
        matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt
    from matplotlib.collections import PolyCollection
    from matplotlib.colors import LogNorm
    if getattr(model, "field_sections", None) is None:
        raise ValueError("the model holds no field sections: run simulate_logs(field_grid=...) first")
    kept = [int(i) for i in model.field_depth_index]
    if int(depth_index) not in kept:
        raise ValueError("no field section was kept for depth index {} (field_depths = {})".format(depth_index, kept))
    k = kept.index(int(depth_index))
    grid = model.field_grid
    lateral = "x" if "x" in grid else "r"
    h, z = np.asarray(grid[lateral], dtype=float), np.asarray(grid["z"], dtype=float)
    if h.size < 2 or z.size < 2 or np.any(np.diff(h) <= 0) or np.any(np.diff(z) <= 0):
        raise ValueError("a picture needs increasing grid coordinates, two at least along both axes")
    u = np.asarray(model.field_sections[tool]["u"][k], dtype=float)
    J = np.asarray(model.field_sections[tool]["J"][k], dtype=float)
    dim = J.shape[-1]
    fig, ax = plt.subplots(figsize=(5, 7))
    polys, res = model_polygons(model.formation_model, model.borehole_model, model.dip_deg if lateral == "x" else 0.0, (z[0], z[-1]), (h[0], h[-1]))
    ax.add_collection(PolyCollection(polys, array=res, cmap="Greys", norm=LogNorm(vmin=max(res.min(), 1e-3) / 2, vmax=res.max() * 2), alpha=0.35, edgecolors="k",
                                     linewidths=0.4))
    lu = np.ma.masked_invalid(np.log10(np.where(np.abs(u) > 0, np.abs(u), np.nan)))
    cs = ax.contourf(h, z, lu, levels=20, cmap="viridis", alpha=0.75)
    Jh, Jz = J[..., 0], J[..., dim - 1]
    hs, zs = h, z
    if not _uniform_axis(h):
        hs = np.linspace(h[0], h[-1], h.size)
        Jh, Jz = _resample(Jh, h, hs, 1), _resample(Jz, h, hs, 1)
    if not _uniform_axis(z):
        zs = np.linspace(z[0], z[-1], z.size)
        Jh, Jz = _resample(Jh, z, zs, 0), _resample(Jz, z, zs, 0)
    if np.any(np.isfinite(Jh) & np.isfinite(Jz)):
        ax.streamplot(hs, zs, np.ma.masked_invalid(Jh), np.ma.masked_invalid(Jz), color="w", linewidth=0.7, density=1.2, arrowsize=0.7)
    src_z, src_I = model.field_sources[tool][k]
    src_x = getattr(model, "field_source_x", None)      # an eccentred tool: the electrodes at x = e of the dip plane
    src_x = np.zeros(np.size(src_z)) if src_x is None else np.atleast_1d(src_x[tool][k])
    for zq, Iq, xq in zip(np.atleast_1d(src_z), np.atleast_1d(src_I), src_x):
        ax.plot([xq if lateral == "x" else abs(xq)], [zq], marker="o" if Iq > 0 else "s", color="r" if Iq > 0 else "b", ms=6, mec="k", zorder=5)
    ax.set_xlim(h[0], h[-1])
    ax.set_ylim(z[-1], z[0])
    ax.set_xlabel("{} [m]".format(lateral))
    ax.set_ylabel("depth [m]")
    ax.set_title("{} at {:.2f} m: log10 |u / V|, streamlines of J".format(tool, float(model.logs[tool][int(depth_index), 0])))
    fig.colorbar(cs, ax=ax)
    if path is not None:
        fig.savefig(path, dpi=120)
    return fig


def plot_inversion(model, path=None, true_table=None):
    """One picture of model.inversion (Model.invert_logs): the resistivity columns of the start, final and - if given - true
    formation table against depth (one panel per column with a free entry), and beside them the observed and the fitted logs per
    tool.  Returns the figure; `path`: also written there."""
    import matplotlib
    if not os.environ.get("MPLBACKEND") and not os.environ.get("DISPLAY"):
        matplotlib.use("Agg", force=False)
    import matplotlib.pyplot as plt
    inv = model.inversion
    names = ["RTFZ", "RTUZ", "RVUZ"]
    cols = [c for c in range(inv.free.shape[1]) if inv.free[:, c].any()]
    fig, axes = plt.subplots(1, len(cols) + len(inv.tools), figsize=(3.2 * (len(cols) + len(inv.tools)), 7), sharey=True, squeeze=False)
    axes = axes[0]

    def stairs(ax, table, c, **kw):
        t = np.asarray(table, dtype=float)
        z = np.column_stack([t[:, 0], t[:, 1]]).ravel()
        ax.plot(np.repeat(t[:, 3 + c], 2), z, **kw)
    for ax, c in zip(axes, cols):
        stairs(ax, inv.start_table, c, color="0.6", lw=1.0, label="start")
        if true_table is not None:
            stairs(ax, true_table, c, color="k", lw=2.2, alpha=0.5, label="true")
        stairs(ax, inv.final_table, c, color="C3", lw=1.2, label="final")
        ax.set_xscale("log")
        ax.set_xlabel("{} [ohmm]".format(names[c]))
        ax.grid(True, which="both", lw=0.3)
        ax.legend(loc="lower right", fontsize=8)
    for ax, tool in zip(axes[len(cols):], inv.tools):
        obs = np.asarray(inv.observed[tool], dtype=float)
        obs = obs[:, 1] if obs.ndim == 2 else obs
        ax.plot(obs, inv.depths, "k.", ms=4, label="observed")
        ax.plot(model.logs[tool][:, 1], model.logs[tool][:, 0], color="C3", lw=1.0, label="fitted")
        ax.set_xscale("log")
        ax.set_xlabel("{} [ohmm]".format(tool))
        ax.grid(True, which="both", lw=0.3)
        ax.legend(loc="lower right", fontsize=8)
    lo, hi = float(np.min(inv.depths)), float(np.max(inv.depths))
    pad = 0.1 * max(hi - lo, 1.0)
    axes[0].set_ylim(hi + pad, lo - pad)
    axes[0].set_ylabel("depth [m]")
    fig.suptitle("inversion: rms {:.3g} after {} sweeps ({})".format(inv.rms, len(inv.history), inv.stop))
    if path is not None:
        fig.savefig(path, dpi=120)
    return fig
