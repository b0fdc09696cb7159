"""Zonal statistics on the device: a layer's statistics per zone of an integer zone plane, and those statistics on the cells.

What the reference's users run ``terra::zonal`` for: basin mean elevation, a cell's height relative to its basin, the mean
elevation of a lake or a plateau patch.  A zone plane is a ``label`` or ``id`` plane of :func:`patches.patches`, the ``index``
plane of :func:`flowpath.flowpath` with ``where="outlet"`` (drainage basins), or a land-cover or administrative raster.
include/machisplin_hip.h, section "zonal", states the rule: the values are quantised to integers ``q = rint(v / quantum)`` with
``quantum`` a power of two, and every accumulator -- cells, n, sum q, sum q^2 in two words, min, max -- is an exact integer, so
no result depends on the order of addition and every table and plane equals a numpy and Python-int restatement bit for bit.
All work on the cells runs in libmachisplin_hip.so (csrc/zonal.hip); this module only marshals arguments.

The classes of a CATEGORICAL layer per zone -- counts, fractions, the mode -- are :func:`classes.crosstab`.

ORDER STATISTICS -- the median or any quantile per zone, per coarse cell (:func:`aggregate_quantile`) or of the whole layer, and a
cell's rank inside its zone -- are :func:`quantile` (section "zonal quantiles", csrc/quantile.hip): the cells' (zone, q) keys go
through the library's deterministic radix sort (:func:`sort_keys`, csrc/sort_keys.hip), and every quantile is a look-up.

Out of scope: the mode per zone here (:func:`classes.crosstab` has it), zones given as floats, more than 2^31 - 1 cells, weights (a
cell's area on a lon/lat grid); for quantiles also window medians, types other than 7, mid-rank percentiles, more than 16
probabilities per call.
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


QUANTILE_PLANES = ("q", "below", "frac_below")
MAX_PROBS = 16


def _check_quantile(stack, zones, probs, layer, planes, n_zones, table, quantum, out_dtype, target=None):
    """every argument check of :func:`quantile` and :func:`aggregate_quantile`, before any device call: (probs, planes, n_zones, quantum)"""
    import torch
    if table not in TABLES:
        raise ValueError(f"unknown table {table!r}: one of 'dense', 'present' or None")
    try:
        probs = tuple(float(p) for p in ((probs,) if isinstance(probs, (int, float)) else probs))
    except (TypeError, ValueError):
        raise ValueError("probs must be a sequence of numbers in [0, 1]") from None
    if not 1 <= len(probs) <= MAX_PROBS:
        raise ValueError(f"probs must hold 1 .. {MAX_PROBS} probabilities, not {len(probs)}")
    for p in probs:
        if not 0.0 <= p <= 1.0:                                            # NaN fails both comparisons
            raise ValueError(f"probs: {p!r} is not in [0, 1]")
    planes = _names("planes", planes, QUANTILE_PLANES)
    if table is None and not planes:
        raise ValueError("no output: table is None and planes is empty")
    if zones is not None and target is not None:
        raise ValueError("zones and a target grid are both given: a cell's zone is one or the other")
    g = stack.geom
    if zones is not None and (not isinstance(zones, torch.Tensor) or zones.dim() != 2 or zones.dtype.is_floating_point or zones.dtype.is_complex
                              or zones.dtype == torch.bool):
        raise ValueError("zones must be a 2-D integer tensor or None (zones given as floats are out of scope)")
    if not 0 <= int(layer) < stack.n_layers:
        raise ValueError(f"layer {layer} is not one of the stack's {stack.n_layers} layers")
    if g.nrow < 1 or g.ncol < 1:
        raise ValueError("the grid has no cell (nrow, ncol)")
    if g.nrow * g.ncol > INT32_MAX:
        raise ValueError(f"grid too large: nrow * ncol = {g.nrow * g.ncol} passes 2^31 - 1")
    if zones is not None and tuple(zones.shape) != (g.nrow, g.ncol):
        raise ValueError(f"shape mismatch: zones is {tuple(zones.shape)}, the stack's grid ({g.nrow}, {g.ncol})")
    if target is not None and (target.nrow < 1 or target.ncol < 1 or target.nrow * target.ncol > INT32_MAX or not target.xres > 0 or not target.yres > 0):
        raise ValueError("geom: the target grid needs 1 .. 2^31 - 1 cells and positive resolutions")
    if n_zones is not None:
        if zones is None:
            raise ValueError("n_zones goes with a zone plane: without one it follows from the target grid, or is 1")
        n_zones = int(n_zones)
        if not 1 <= n_zones <= INT32_MAX:
            raise ValueError(f"n_zones must be in 1 .. 2^31 - 1 (a zone is an int32), not {n_zones}")
    if quantum is not None:
        quantum = float(quantum)
        if not (2.0 ** -1022 <= quantum <= 2.0 ** 1023) or math.frexp(quantum)[0] != 0.5:
            raise ValueError(f"quantum must be a power of two in 2^-1022 .. 2^1023, not {quantum!r}")
    if out_dtype not in (None, torch.float64, torch.float32):
        raise ValueError("out_dtype must be torch.float64 or torch.float32")
    return probs, planes, n_zones, quantum


def _quantile(stack, zones, probs, layer, planes, n_zones, table, quantum, out_dtype, stream, target):
    import torch
    out_dtype = out_dtype or torch.float64
    g = stack.geom
    src = stack.planes
    dev = src.device
    if zones is not None and (zones.device != dev or zones.dtype != torch.int32 or zones.stride(1) != 1):
        zones = zones.to(device=dev, dtype=torch.int32).contiguous()
    cg = g.c_struct()
    ct = target.c_struct() if target is not None else None
    dt = {torch.float64: _lib.F64, torch.float32: _lib.F32, torch.int16: _lib.I16}[src.dtype]
    cs = _lib.Stack(src.data_ptr(), src.shape[0], dt, src.stride(0), src.stride(1), stack.nodata)
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    cp = (C.c_double * len(probs))(*probs)
    info = _lib.QuantileInfo()

    def call(tab, pl, nz, q):
        _lib.check(_lib.lib().mhs_zonal_quantile_dev(C.byref(cg), C.byref(cs), int(layer), zones.data_ptr() if zones is not None else None,
                                                     zones.stride(0) if zones is not None else 0, nz or 0, q or 0.0, 0, cp, len(probs),
                                                     C.byref(ct) if ct is not None else None, C.byref(tab) if tab is not None else None,
                                                     C.byref(pl) if pl is not None else None, st, C.byref(info)))

    if zones is None:
        rows_dense = target.nrow * target.ncol if target is not None else 1
    elif table == "dense" and n_zones is None:                   # the library measures n_zones (and the quantum) before the table is sized
        call(None, None, None, quantum)
        n_zones, quantum = info.n_zones, info.quantum
        rows_dense = n_zones
    else:
        rows_dense = n_zones
    tab = tab_out = zone = None
    if table is not None:
        rows = rows_dense if table == "dense" else min(rows_dense or g.nrow * g.ncol, g.nrow * g.ncol)
        tab_out = {"q": torch.empty((rows, len(probs)), dtype=torch.float64, device=dev), "count": torch.empty(rows, dtype=torch.int64, device=dev)}
        zone = torch.empty(rows, dtype=torch.int32, device=dev) if table == "present" else None
        tab = _lib.QuantileTable(rows, zone.data_ptr() if zone is not None else None, tab_out["count"].data_ptr(), tab_out["q"].data_ptr())
    pl = None
    pl_out = {}
    if planes:
        pl = _lib.QuantilePlanes()
        pl.dtype = _lib.F64 if out_dtype == torch.float64 else _lib.F32
        if "q" in planes:
            pl_out["q"] = torch.empty((len(probs), g.nrow, g.ncol), dtype=out_dtype, device=dev)
            for j in range(len(probs)):
                pl.q[j], pl.ld_q[j] = pl_out["q"][j].data_ptr(), g.ncol
        if "below" in planes:
            pl_out["below"] = torch.empty((g.nrow, g.ncol), dtype=torch.int32, device=dev)
            pl.below, pl.ld_below = pl_out["below"].data_ptr(), g.ncol
        if "frac_below" in planes:
            pl_out["frac_below"] = torch.empty((g.nrow, g.ncol), dtype=out_dtype, device=dev)
            pl.frac_below, pl.ld_frac_below = pl_out["frac_below"].data_ptr(), g.ncol
        pl_out = {n: pl_out[n] for n in planes}
    call(tab, pl, n_zones if zones is not None else None, quantum)
    info = {k: getattr(info, k) for k, _ in _lib.QuantileInfo._fields_}
    if table == "present":
        k = info["n_present"]
        tab_out = {"zone": zone[:k], "q": tab_out["q"][:k], "count": tab_out["count"][:k]}
    return tab_out, pl_out, info


def quantile(stack, zones=None, probs=(0.5,), layer=0, planes=(), n_zones=None, table="dense", quantum=None, out_dtype=None, stream=None):
    """The quantiles ``probs`` (1 .. 16 probabilities in [0, 1]; R's type 7, numpy's ``linear``) of layer ``layer`` inside each zone
    of ``zones`` (include/machisplin_hip.h, section "zonal quantiles"); ``zones=None``: the whole layer is zone 0.  Membership,
    NA, ``n_zones``, ``quantum`` and ``info["n_inexact"]`` are :func:`zonal`'s: the quantiles are those of ``q = rint(v /
    quantum)``, ``p = 0`` and ``p = 1`` equal ``zonal``'s ``min`` and ``max`` bit for bit, and with ``n_inexact == 0`` the median
    equals ``numpy.median`` of the zone's values bit for bit.

    ``table="dense"`` gives ``{"q": [n_zones, n_probs] float64, "count": [n_zones] int64}``; ``"present"`` only the zones with a
    contributing cell, ascending, with ``"zone"`` -- it allocates nothing proportional to ``n_zones``, the form for cell-number
    labels --; None no table.  ``planes`` names some of :data:`QUANTILE_PLANES`: ``q`` (``[n_probs, nrow, ncol]``: each cell
    receives its zone's quantiles, NaN without a zone), ``below`` (int32: the contributing cells of the cell's zone with a smaller
    value, -1 where the cell does not contribute) and ``frac_below`` (``below / n``, NaN likewise); float planes are ``out_dtype``.

    Returns ``(table, planes, info)``; ``info`` has the fields of mhs_quantile_info (zonal's, ``n_present`` counting the zones with
    a contributing cell, and ``passes_run``, ``scratch_bytes``)."""
    probs, planes, n_zones, quantum = _check_quantile(stack, zones, probs, layer, planes, n_zones, table, quantum, out_dtype)
    return _quantile(stack, zones, probs, layer, planes, n_zones, table, quantum, out_dtype, stream, None)


def aggregate_quantile(stack, geom, probs=(0.5,), layer=0, quantum=None, out_dtype=None, stream=None):
    """``terra::aggregate(fun = median)`` and its quantiles: layer ``layer`` on the grid ``geom`` (same coordinate system, any
    resolution, origin and extent), a target cell taking the source cells whose centre lies in it -- the footprints of
    ``resample.resample``'s aggregates, so ``p = 0``, ``p = 1`` and the count equal its ``min``, ``max`` and ``count``.

    Returns ``(planes [n_probs, geom.nrow, geom.ncol], count plane [geom.nrow, geom.ncol] int64, info)``; a target cell without a
    contributing source cell holds NaN and count 0."""
    import torch
    probs, _, _, quantum = _check_quantile(stack, None, probs, layer, (), None, "dense", quantum, out_dtype, target=geom)
    table, _, info = _quantile(stack, None, probs, layer, (), None, "dense", quantum, None, stream, geom)
    q = table["q"].t().contiguous().reshape(len(probs), geom.nrow, geom.ncol)
    if out_dtype == torch.float32:
        q = q.to(torch.float32)
    return q, table["count"].reshape(geom.nrow, geom.ncol), info


def sort_keys(keys, bit_lo=0, bit_hi=64, stream=None):
    """Sort a 1-D uint64 (or int64, read as uint64) device tensor ascending IN PLACE by its bits ``bit_lo .. bit_hi - 1`` with the
    library's deterministic radix sort (include/machisplin_hip.h, section "sort"); the caller guarantees that the keys agree
    outside that window.  Returns ``{"passes_run", "scratch_bytes"}``."""
    import torch
    if not isinstance(keys, torch.Tensor) or keys.dim() != 1 or keys.dtype not in (torch.uint64, torch.int64):
        raise ValueError("keys must be a 1-D uint64 or int64 tensor")
    if keys.numel() > 1 and keys.stride(0) != 1:
        raise ValueError("keys must be contiguous")
    if keys.numel() > INT32_MAX:
        raise ValueError("keys: more than 2^31 - 1 keys")
    if not 0 <= int(bit_lo) <= int(bit_hi) <= 64:
        raise ValueError("bit_lo, bit_hi: the window needs 0 <= bit_lo <= bit_hi <= 64")
    if not keys.is_cuda:
        raise ValueError("keys must be a device tensor")
    st = stream if stream is not None else torch.cuda.current_stream(keys.device).cuda_stream
    info = _lib.SortInfo()
    _lib.check(_lib.lib().mhs_sort_keys_dev(keys.data_ptr() if keys.numel() else None, keys.numel(), int(bit_lo), int(bit_hi), st, C.byref(info)))
    return {"passes_run": info.passes_run, "scratch_bytes": info.scratch_bytes}
