"""Connected patches of a mask on the device: label, size, sieve.

Which cells of a mask belong together -- what the reference's users run ``terra::patches`` (``raster::clump``) and a size
filter for (the "sieve" of GDAL and SAGA) before ``terra::distance``: a void of three cells on a mountain is no coast, one
stray cell below a threshold no lake.  include/machisplin_hip.h, section "patches", states the rule: every product is an
integer, so every plane equals a numpy restatement bit for bit.  All work on the cells runs in libmachisplin_hip.so
(csrc/patches.hip, a block-based union-find); this module only marshals arguments.  A ``keep`` plane goes straight into
:func:`proximity.proximity`, which takes a 2-D integer tensor of feature flags.

Out of scope: patches of equal value (``terra::patches(values=TRUE)``), wrap-around at the date line, more than 2^31 - 1
cells.  The statistics of another layer per patch are :func:`zonal.zonal`: a ``label`` or ``id`` plane is a zone plane.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from .proximity import WHERE, INT32_MAX, _Plane

PRODUCTS = ("label", "id", "size", "edge", "keep")                              # the planes of mhs_patches_out, in its order
EDGE = ("any", "touching", "interior")                                         # the MHS_PATCH_EDGE_* of the header, in its order


class PatchesResult(dict):
    """what :func:`patches` returns for several products: the planes by name, and ``.info``"""
    info = None


def _check(stack, layer, where, threshold, connectivity, products, min_size, max_size, edge):
    """every argument check of :func:`patches`, before any device call"""
    import torch
    if isinstance(stack, torch.Tensor):
        if stack.dim() != 2 or stack.dtype.is_floating_point or stack.dtype.is_complex:
            raise ValueError("stack must be a RasterStack or a 2-D bool or integer tensor of feature flags")
        if where != "valid" or threshold is not None or layer != 0:
            raise ValueError("a tensor of feature flags takes no layer, where or threshold: every nonzero cell is a feature")
        stack, where, threshold = _Plane(stack), "ne", 0.0
    if where not in WHERE:
        raise ValueError(f"unknown where {where!r}: one of {', '.join(WHERE)}")
    code = WHERE.index(where)
    if code >= 2:
        if threshold is None:
            raise ValueError(f"where={where!r} needs a threshold")
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("threshold must not be NaN")
    else:
        threshold = 0.0
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, not {connectivity!r}")
    one = isinstance(products, str)
    names = (products,) if one else tuple(products)
    for n in names:
        if n not in PRODUCTS:
            raise ValueError(f"unknown product {n!r}: one of {', '.join(PRODUCTS)}")
    if not names or len(set(names)) != len(names):
        raise ValueError("products must name at least one product, each once")
    min_size = int(min_size)
    if min_size < 1:
        raise ValueError("min_size must be at least 1")
    max_size = 2 ** 63 - 1 if max_size is None else int(max_size)
    if max_size < min_size:
        raise ValueError(f"max_size {max_size} is below min_size {min_size}")
    if edge not in EDGE:
        raise ValueError(f"unknown edge {edge!r}: one of {', '.join(EDGE)}")
    g = stack.geom
    if not 0 <= int(layer) < stack.n_layers:
        raise ValueError(f"layer {layer} is not one of the stack's {stack.n_layers} layers")
    if g.nrow < 1 or g.ncol < 1:
        raise ValueError("the grid has no cell (nrow, ncol)")
    if g.nrow * g.ncol > INT32_MAX:
        raise ValueError(f"grid too large: nrow * ncol = {g.nrow * g.ncol} passes 2^31 - 1 (label is an int32)")
    return stack, code, threshold, one, names, min_size, min(max_size, 2 ** 63 - 1), EDGE.index(edge)


def patches(stack, layer=0, where="valid", threshold=None, connectivity=8, products=("label",), min_size=1, max_size=None, edge="any",
            stream=None):
    """The connected patches of the feature cells of layer ``layer`` (include/machisplin_hip.h, section "patches").  A cell is
    a feature when it satisfies ``where``, one of :data:`proximity.WHERE`: ``na``, ``valid``, or ``lt le gt ge eq ne`` against
    ``threshold``.  Two feature cells are neighbours under ``connectivity`` 4 (N, S, E, W) or 8 (plus the diagonals).
    ``products`` names some of :data:`PRODUCTS`: ``label`` (int32, the smallest cell number row * ncol + col of the cell's
    patch), ``id`` (int32, 1 .. K in increasing order of label: the numbering of ``terra::patches`` and
    ``scipy.ndimage.label``), ``size`` (int32, the patch's cells), ``edge`` (uint8, 1 where the patch has a cell in the first
    or last row or column) and ``keep`` (uint8, 1 where ``min_size <= size <= max_size`` -- ``max_size`` None: no limit -- and
    the patch meets ``edge``: ``any``, ``touching`` or ``interior``; this is the sieve).  On a non-feature cell label is -1
    and every other product 0.

    Always the whole plane: there is no window.  A 2-D bool or integer tensor may stand in place of ``stack``: every nonzero
    cell is a feature.

    Returns ``(planes, info)``: a dict of device tensors by name (``.info`` too) -- or the single tensor when ``products`` is
    one name -- and a dict of the fields of mhs_patches_info (n_features, n_patches, n_kept_patches, n_kept_cells, max_size,
    scratch_bytes)."""
    import torch
    stack, code, threshold, one, names, min_size, max_size, edge_rule = _check(stack, layer, where, threshold, connectivity, products, min_size,
                                                                               max_size, edge)
    g = stack.geom
    src = stack.planes
    planes = {n: torch.empty((g.nrow, g.ncol), dtype=torch.uint8 if n in ("edge", "keep") else torch.int32, device=src.device) for n in names}
    out = _lib.PatchesOut(*[planes[n].data_ptr() if n in planes else None for n in PRODUCTS])
    info = _lib.PatchesInfo()
    cg = g.c_struct()
    dt = {torch.float64: _lib.F64, torch.float32: _lib.F32, torch.int16: _lib.I16}[src.dtype]
    cs = _lib.Stack(src.data_ptr(), src.shape[0], dt, src.stride(0), src.stride(1), stack.nodata)
    st = stream if stream is not None else torch.cuda.current_stream(src.device).cuda_stream
    _lib.check(_lib.lib().mhs_patches_dev(C.byref(cg), C.byref(cs), int(layer), code, threshold, int(connectivity), min_size, max_size, edge_rule,
                                          C.byref(out), g.ncol, st, C.byref(info)))
    info = {k: getattr(info, k) for k, _ in _lib.PatchesInfo._fields_}
    if one:
        return planes[names[0]], info
    res = PatchesResult(planes)
    res.info = info
    return res, info


def sieve(stack, layer=0, where="valid", threshold=None, connectivity=8, min_size=1, max_size=None, edge="any", stream=None):
    """The ``keep`` plane of :func:`patches` alone: a uint8 device tensor, 1 at the cells of the patches that pass the filter --
    a mask of feature flags for :func:`proximity.proximity`."""
    return patches(stack, layer, where, threshold, connectivity, "keep", min_size, max_size, edge, stream)[0]
