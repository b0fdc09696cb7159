"""Rasters onto one grid: resample, aggregate, extract at points, align.

The reference package's README says "All rasters must be the same: resolution, projection and extent" and sends its users to
``terra::crop`` and ``terra::extract`` for the rest.  This module brings stacks in the same coordinate system -- they may differ
in resolution, origin and extent -- onto one grid: :func:`resample` (nearest, bilinear, cubic; the aggregates mean, min, max,
sum, count for a coarser target), :func:`extract` at points and :func:`align`, which makes one float32 stack, ready for
``mltps`` and ``Mess``, from several.  Another coordinate system is ``project``'s part.  A CATEGORICAL raster onto a coarser
grid -- the mode, or the share of each class in the target cell -- is :func:`classes.aggregate`, over the same footprints.
include/machisplin_hip.h, section "resample", states the rules.  All arithmetic on the cells runs in libmachisplin_hip.so
(csrc/resample.hip); this module only marshals arguments.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .raster import Geometry, RasterStack

METHODS = ("near", "bilinear", "cubic", "mean", "min", "max", "sum", "count")      # the MHS_RS_* of the header, in its order
EXTRACT = {"simple": 0, "near": 0, "bilinear": 1, "cubic": 2}


def _method(method) -> int:
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}: one of {', '.join(METHODS)}")
    return METHODS.index(method)


def resample(stack: RasterStack, geom: Geometry, method="bilinear", out_dtype=None, window=None, out=None, stream=None) -> RasterStack:
    """Every layer of ``stack`` on the grid ``geom`` (same coordinate system, any resolution, origin and extent), in one
    launch: ``method`` is one of :data:`METHODS` -- ``near``, ``bilinear`` and ``cubic`` interpolate at the target cells'
    centres; ``mean``, ``min``, ``max``, ``sum`` and ``count`` take the source cells whose centre lies in the target cell
    (how a 30 m product becomes a 1 km one).  Returns a RasterStack whose nodata is NaN: float32 planes unless the source is
    float64 or ``out_dtype`` says otherwise (a float32 value is the float64 result rounded once).  NaN where the centre is
    outside the source, where every tap is NA, and for mean / min / max of no valid cell; ``count`` and ``sum`` are 0 there.
    ``window`` = (r0, r1, c0, c1) of ``geom`` gives those cells of the whole-grid result bit for bit, on the window's
    geometry.  ``out``: a pre-allocated device tensor (layers, rows, cols) with unit column stride."""
    import torch
    code = _method(method)
    r0, r1, c0, c1 = (int(x) for x in window) if window is not None else (0, geom.nrow, 0, geom.ncol)
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else torch.float64 if stack.planes.dtype == torch.float64 else torch.float32
    if out_dtype not in (torch.float64, torch.float32):
        raise ValueError("out_dtype must be torch.float64 or torch.float32")
    shape = (stack.n_layers, r1 - r0, c1 - c0)
    if out is None:
        out = torch.empty(shape, dtype=out_dtype, device=stack.planes.device)
    if out.dtype != out_dtype or not out.is_cuda or out.dim() != 3 or tuple(out.shape) != shape or (out.numel() and out.stride(2) != 1):
        raise ValueError("out must be a device tensor (layers, rows, cols) of out_dtype with unit column stride")
    st = stream if stream is not None else torch.cuda.current_stream(stack.planes.device).cuda_stream
    sg, ss, tg = stack.geom.c_struct(), stack.c_struct(), geom.c_struct()
    _lib.check(_lib.lib().mhs_resample_dev(C.byref(sg), C.byref(ss), C.byref(tg), r0, r1, c0, c1, code, out.data_ptr(), out.stride(1),
                                           out.stride(0), _lib.F64 if out_dtype == torch.float64 else _lib.F32, st))
    res = RasterStack.__new__(RasterStack)          # keeps `out` as it is: RasterStack() would copy a padded tensor
    res.planes, res.geom, res.nodata = out, geom.window(r0, r1, c0, c1) if window is not None else geom, float("nan")
    return res


def extract(stack: RasterStack, xy, method="simple") -> np.ndarray:
    """terra::extract(stack, xy, method=): the layers' values at the points ``xy`` (n x 2: x, y), an (n, C) float64 array.
    ``"simple"`` is the value of the cell that holds the point (what ``mltps.station_predictors`` looks up), ``"bilinear"``
    and ``"cubic"`` interpolate between the cell centres.  NaN outside the raster and where the method gives NA."""
    import torch
    if method not in EXTRACT:
        raise ValueError(f"unknown method {method!r}: one of {', '.join(EXTRACT)}")
    xy = np.asarray(xy, dtype=np.float64)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError("xy must be n x 2")
    n = xy.shape[0]
    dev = stack.planes.device
    pts = torch.from_numpy(np.ascontiguousarray(xy.T)).to(dev)                  # column-major n x 2
    out = torch.empty((stack.n_layers, n), dtype=torch.float64, device=dev)
    sg, ss = stack.geom.c_struct(), stack.c_struct()
    _lib.check(_lib.lib().mhs_extract_points_dev(C.byref(sg), C.byref(ss), pts.data_ptr(), n, EXTRACT[method], out.data_ptr(),
                                                 torch.cuda.current_stream(dev).cuda_stream))
    return np.ascontiguousarray(out.cpu().numpy().T)


def align(stacks, geom: Geometry | None = None, methods="bilinear") -> RasterStack:
    """One float32 RasterStack on ``geom`` (default: the first stack's grid) from several stacks on different grids, all
    layers concatenated in order, nodata NaN: ready for ``mltps``, ``covariates`` and ``Mess``.  ``methods``: one of
    :data:`METHODS` for all, or one per stack.  A stack that is on ``geom`` already is passed through by a plain conversion
    (its NA cells become NaN), not through the kernel."""
    import torch
    stacks = list(stacks)
    if not stacks:
        raise ValueError("no stack to align")
    geom = geom or stacks[0].geom
    methods = [methods] * len(stacks) if isinstance(methods, str) else list(methods)
    if len(methods) != len(stacks):
        raise ValueError("give one method, or one per stack")
    for m in methods:
        _method(m)
    dev = stacks[0].planes.device
    planes = torch.empty((sum(s.n_layers for s in stacks), geom.nrow, geom.ncol), dtype=torch.float32, device=dev)
    k = 0
    for s, m in zip(stacks, methods):
        dst = planes[k:k + s.n_layers]
        if s.geom == geom:
            dst.copy_(s.planes)
            if not np.isnan(s.nodata):
                dst[s.planes == s.nodata] = float("nan")
        else:
            resample(s, geom, m, out=dst)
        k += s.n_layers
    return RasterStack(geom, planes, float("nan"))
