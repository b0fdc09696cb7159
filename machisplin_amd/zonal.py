"""Zonal statistics on the device: a layer's statistics per zone of an integer zone plane, and those statistics on the cells.

What the reference's users run ``terra::zonal`` for: basin mean elevation, a cell's height relative to its basin, the mean
elevation of a lake or a plateau patch.  A zone plane is a ``label`` or ``id`` plane of :func:`patches.patches`, the ``index``
plane of :func:`flowpath.flowpath` with ``where="outlet"`` (drainage basins), or a land-cover or administrative raster.
include/machisplin_hip.h, section "zonal", states the rule: the values are quantised to integers ``q = rint(v / quantum)`` with
``quantum`` a power of two, and every accumulator -- cells, n, sum q, sum q^2 in two words, min, max -- is an exact integer, so
no result depends on the order of addition and every table and plane equals a numpy and Python-int restatement bit for bit.
All work on the cells runs in libmachisplin_hip.so (csrc/zonal.hip); this module only marshals arguments.

The classes of a CATEGORICAL layer per zone -- counts, fractions, the mode -- are :func:`classes.crosstab`.

Out of scope: median and mode per zone, zones given as floats, more than 2^31 - 1 cells, weights (a cell's area on a lon/lat
grid).
"""
from __future__ import annotations

import ctypes as C
import math

from . import _lib

STATS = ("count", "sum", "mean", "sd", "min", "max", "range", "minus_mean", "above_min", "below_max", "dev", "cells")   # bit k of the header
TABLE_STATS = STATS[:7] + ("cells",)                                           # what a table can hold; bits 7 .. 10 exist only as planes
TABLES = ("dense", "present", None)
NO_STRIP = 1                                                                   # MHS_ZONAL_NO_STRIP
INT32_MAX = 2 ** 31 - 1
_INT = ("count", "cells")


def _names(what, names, allowed):
    names = (names,) if isinstance(names, str) else tuple(names)
    for n in names:
        if n not in allowed:
            raise ValueError(f"unknown statistic {n!r} in {what}: one of {', '.join(allowed)}")
    if len(set(names)) != len(names):
        raise ValueError(f"{what} must name each statistic once")
    return names


def _check(stack, zones, layer, stats, planes, n_zones, table, quantum, out_dtype):
    """every argument check of :func:`zonal`, before any device call: (stats, planes, n_zones, quantum)"""
    import torch
    if table not in TABLES:
        raise ValueError(f"unknown table {table!r}: one of 'dense', 'present' or None")
    stats = _names("stats", stats, TABLE_STATS) if table is not None else ()
    planes = _names("planes", planes, STATS)
    if table is not None and not stats:
        raise ValueError("no output: a table needs at least one statistic in stats (or table=None)")
    if not stats and not planes:
        raise ValueError("no output: stats (with a table) and planes are both empty")
    if not isinstance(zones, torch.Tensor) or zones.dim() != 2 or zones.dtype.is_floating_point or zones.dtype.is_complex or zones.dtype == torch.bool:
        raise ValueError("zones must be a 2-D integer tensor (zones given as floats are out of scope)")
    g = stack.geom
    if not 0 <= int(layer) < stack.n_layers:
        raise ValueError(f"layer {layer} is not one of the stack's {stack.n_layers} layers")
    if g.nrow < 1 or g.ncol < 1:
        raise ValueError("the grid has no cell (nrow, ncol)")
    if g.nrow * g.ncol > INT32_MAX:
        raise ValueError(f"grid too large: nrow * ncol = {g.nrow * g.ncol} passes 2^31 - 1")
    if tuple(zones.shape) != (g.nrow, g.ncol):
        raise ValueError(f"shape mismatch: zones is {tuple(zones.shape)}, the stack's grid ({g.nrow}, {g.ncol})")
    if n_zones is not None:
        n_zones = int(n_zones)
        if not 1 <= n_zones <= INT32_MAX:
            raise ValueError(f"n_zones must be in 1 .. 2^31 - 1 (a zone is an int32), not {n_zones}")
    if quantum is not None:
        quantum = float(quantum)
        if not (2.0 ** -1022 <= quantum <= 2.0 ** 1023) or math.frexp(quantum)[0] != 0.5:
            raise ValueError(f"quantum must be a power of two in 2^-1022 .. 2^1023, not {quantum!r}")
    if out_dtype not in (None, torch.float64, torch.float32):
        raise ValueError("out_dtype must be torch.float64 or torch.float32")
    return stats, planes, n_zones, quantum


def zonal(stack, zones, layer=0, stats=("mean",), planes=(), n_zones=None, table="dense", quantum=None, out_dtype=None, stream=None, strip=True):
    """The statistics of layer ``layer`` inside each zone of ``zones`` (include/machisplin_hip.h, section "zonal").  ``zones`` is
    a 2-D integer tensor of the stack's ``nrow x ncol`` (other widths than int32 are converted by torch); a cell belongs to zone
    ``z`` when ``0 <= z < n_zones``, a negative zone is "no zone", and a zone ``>= n_zones`` is refused.  ``n_zones`` None: the
    library measures ``max(zone) + 1`` (for a dense table in a first call of its own, which sizes the table).  A cell
    contributes when it has a zone and its value is valid and finite.

    Statistics are those of ``q = rint(v / quantum)``; ``quantum`` None: the smallest power of two with ``max|v| <= 2^30 *
    quantum`` over the layer (1 for int16).  ``info["n_inexact"]`` counts the contributing cells with ``q * quantum != v``: when
    it is 0 the statistics are those of the input itself.

    ``stats`` names the table's statistics, some of :data:`TABLE_STATS` (``count sum mean sd min max range cells``);
    ``table="dense"`` gives arrays of length ``n_zones``, ``"present"`` only the zones that have a cell, in increasing zone
    number, with their numbers under ``"zone"`` (the form for cell-number labels), None no table.  ``planes`` names some of
    :data:`STATS`: each cell receives its zone's statistic, or -- ``minus_mean above_min below_max dev`` -- its own value
    against it; float planes are ``out_dtype`` (float64 unless given), ``count`` and ``cells`` int32; a cell without a zone gets
    NaN (0).  ``strip=False`` flushes the accumulate kernel's LDS table after every tile (a diagnostic: the results are the same).

    Returns ``(table, planes, info)``: two dicts of device tensors by name (``table`` None without one; float64, ``count`` and
    ``cells`` int64) and a dict of the fields of mhs_zonal_info (n_zones, n_present, n_cells_in_zones, n_contributing,
    n_nonfinite, n_inexact, quantum, scratch_bytes)."""
    import torch
    stats, planes, n_zones, quantum = _check(stack, zones, layer, stats, planes, n_zones, table, quantum, out_dtype)
    out_dtype = out_dtype or torch.float64
    g = stack.geom
    src = stack.planes
    dev = src.device
    if zones.device != dev or zones.dtype != torch.int32 or zones.stride(1) != 1:
        zones = zones.to(device=dev, dtype=torch.int32).contiguous()
    cg = g.c_struct()
    dt = {torch.float64: _lib.F64, torch.float32: _lib.F32, torch.int16: _lib.I16}[src.dtype]
    cs = _lib.Stack(src.data_ptr(), src.shape[0], dt, src.stride(0), src.stride(1), stack.nodata)
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    flags = 0 if strip else NO_STRIP
    info = _lib.ZonalInfo()

    def call(tab, pl, nz, q):
        _lib.check(_lib.lib().mhs_zonal_dev(C.byref(cg), C.byref(cs), int(layer), zones.data_ptr(), zones.stride(0), nz or 0, q or 0.0, flags,
                                            C.byref(tab) if tab is not None else None, C.byref(pl) if pl is not None else None, st, C.byref(info)))

    if table == "dense" and n_zones is None:                    # the library measures n_zones (and the quantum) before the table is sized
        call(None, None, None, quantum)
        n_zones, quantum = info.n_zones, info.quantum
    tab = tab_out = None
    if table is not None:
        rows = n_zones if table == "dense" else min(n_zones or g.nrow * g.ncol, g.nrow * g.ncol)
        tab_out = {n: torch.empty(rows, dtype=torch.int64 if n in _INT else torch.float64, device=dev) for n in stats}
        zone = torch.empty(rows, dtype=torch.int32, device=dev) if table == "present" else None
        tab = _lib.ZonalTable(rows, zone.data_ptr() if zone is not None else None,
                              *[tab_out[n].data_ptr() if n in tab_out else None for n in TABLE_STATS])
    pl = pl_out = None
    pl_out = {n: torch.empty((g.nrow, g.ncol), dtype=torch.int32 if n in _INT else out_dtype, device=dev) for n in planes}
    if planes:
        pl = _lib.ZonalPlanes()
        for n in planes:
            pl.plane[STATS.index(n)] = pl_out[n].data_ptr()
            pl.ld[STATS.index(n)] = g.ncol
        pl.dtype = _lib.F64 if out_dtype == torch.float64 else _lib.F32
    call(tab, pl, n_zones, quantum)
    info = {k: getattr(info, k) for k, _ in _lib.ZonalInfo._fields_}
    if table == "present":
        k = info["n_present"]
        tab_out = {"zone": zone[:k], **{n: v[:k] for n, v in tab_out.items()}}
    return tab_out, pl_out, info
