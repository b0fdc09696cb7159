"""MESS, the multivariate environmental similarity surface (Elith, Kearney & Phillips 2010):

``Mess(ref).grid(stack)`` <-> ``dismo::mess(covar.ras, dat_tps[[i]][, 1:n.covars], full = TRUE)``

For every cell and every variable the cell's value is placed in the empirical distribution of the reference rows (the
stations' covariates); the worst variable is the cell's MESS and its index the "most dissimilar variable" (MoD).  A negative
MESS marks a cell where at least one covariate lies outside the stations' range -- where the six learners extrapolate.
include/machisplin_hip.h states the rule.  All arithmetic runs in libmachisplin_hip.so; this module only marshals arguments.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .raster import RasterStack


class Mess:
    """The reference table of a MESS: ``ref`` is n_ref x n_vars (one row per station, one column per variable, every value
    finite, no constant column).  ``n_vars`` is the number of layers of the stack it will be asked about, or two more:
    the last two columns are then LONG and LAT of the stations' cell centres (the ``X`` of
    :func:`mltps.station_predictors`)."""

    def __init__(self, ref):
        ref = np.asarray(ref, dtype=np.float64)
        if ref.ndim != 2:
            raise ValueError("ref must be an n_ref x n_vars table")
        cm = np.asfortranarray(ref)          # column-major, as R hands a matrix over
        h = C.c_void_p()
        _lib.check(_lib.lib().mhs_mess_create(cm.ctypes.data, ref.shape[0], ref.shape[1], C.byref(h)))
        self._h = h
        self.n_ref, self.n_vars = int(ref.shape[0]), int(ref.shape[1])

    def grid(self, stack: RasterStack, window=None, out=None, mod=False, stream=None):
        """The MESS plane of ``stack`` (or of its window (r0, r1, c0, c1)): a float64 device tensor, NaN where any
        variable is NA.  ``mod=True`` also returns the MoD plane (int32, 0-based variable, -1 at NA cells): the result
        is then the pair ``(mess, mod)``.  ``out`` / ``mod`` may be pre-allocated 2-D device tensors of the window's
        shape with unit column stride.  The call only enqueues on ``stream`` (default: torch's current stream)."""
        import torch
        geom = stack.geom
        r0, r1, c0, c1 = window if window is not None else (0, geom.nrow, 0, geom.ncol)
        dev = stack.planes.device
        shape = (r1 - r0, c1 - c0)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=dev)
        if out.dtype != torch.float64 or not out.is_cuda or out.dim() != 2 or out.stride(1) != 1 or tuple(out.shape) != shape:
            raise ValueError("out must be a float64 device tensor of the window's shape with unit column stride")
        want_mod = mod is not False and mod is not None
        if want_mod:
            if mod is True:
                mod = torch.empty(shape, dtype=torch.int32, device=dev)
            if mod.dtype != torch.int32 or not mod.is_cuda or mod.dim() != 2 or mod.stride(1) != 1 or tuple(mod.shape) != shape:
                raise ValueError("mod must be an int32 device tensor of the window's shape with unit column stride")
        g, s = geom.c_struct(), stack.c_struct()
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.lib().mhs_mess_grid_dev(self._h, C.byref(g), C.byref(s), r0, r1, c0, c1, out.data_ptr(), out.stride(0),
                                                mod.data_ptr() if want_mod else None, mod.stride(0) if want_mod else 0, st))
        return (out, mod) if want_mod else out

    def points(self, X):
        """MESS and MoD of the rows of ``X`` (n x n_vars: the stations themselves, hold-out rows): ``(mess, mod)`` as
        numpy arrays (float64, int32)."""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] != self.n_vars:
            raise ValueError(f"X must be n x {self.n_vars}")
        cm = np.asfortranarray(X)
        out, mod = np.empty(X.shape[0]), np.empty(X.shape[0], dtype=np.int32)
        _lib.check(_lib.lib().mhs_mess_points(self._h, cm.ctypes.data, X.shape[0], out.ctypes.data, mod.ctypes.data))
        return out, mod

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib._lib is not None:
            _lib._lib.mhs_mess_free(h)
            self._h = None
