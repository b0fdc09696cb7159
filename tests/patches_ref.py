"""numpy restatements of the patches rule (include/machisplin_hip.h, section "patches"), independent of the library and of scipy.

Two of them: :func:`flood` is a breadth-first flood fill from each unlabelled feature cell in row-major order -- the cell it
starts from is the smallest cell number of its patch, and the order of the starts is the id numbering --, :func:`propagate`
replaces every feature cell's label by the minimum over its neighbourhood until nothing changes (small grids: a serpentine takes
as many rounds as it is long).  Both return the label plane as int64; :func:`products` makes every plane of the rule from it.
"""
import numpy as np

from proximity_ref import WHERE, features  # noqa: F401  (the predicates are proximity's)

EDGE = ("any", "touching", "interior")
PRODUCTS = ("label", "id", "size", "edge", "keep")
OFFSETS = {4: ((-1, 0), (1, 0), (0, -1), (0, 1)),
           8: ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))}


def flood(mask, connectivity=8):
    """label by flood fill: int64, -1 at a non-feature cell"""
    mask = np.asarray(mask, dtype=bool)
    nrow, ncol = mask.shape
    pad = np.zeros((nrow + 2, ncol + 2), dtype=bool)                # a frame of non-features: no bounds test in the loop
    pad[1:-1, 1:-1] = mask
    w = ncol + 2
    todo = pad.ravel().tolist()
    steps = [dr * w + dc for dr, dc in OFFSETS[connectivity]]
    label = np.full((nrow + 2) * w, -1, dtype=np.int64)
    for start in np.flatnonzero(pad.ravel()).tolist():             # row-major
        if not todo[start]:
            continue
        name = (start // w - 1) * ncol + start % w - 1
        todo[start] = False
        front, members = [start], [start]
        while front:
            nxt = []
            for p in front:
                for s in steps:
                    q = p + s
                    if todo[q]:
                        todo[q] = False
                        nxt.append(q)
            members.extend(nxt)
            front = nxt
        label[members] = name
    return label.reshape(nrow + 2, w)[1:-1, 1:-1].copy()


def propagate(mask, connectivity=8):
    """label by iterated minimum propagation: int64, -1 at a non-feature cell"""
    mask = np.asarray(mask, dtype=bool)
    nrow, ncol = mask.shape
    big = np.int64(nrow * ncol)
    lab = np.full((nrow + 2, ncol + 2), big, dtype=np.int64)
    lab[1:-1, 1:-1] = np.where(mask, np.arange(nrow * ncol, dtype=np.int64).reshape(nrow, ncol), big)
    while True:
        new = lab[1:-1, 1:-1].copy()
        for dr, dc in OFFSETS[connectivity]:
            np.minimum(new, lab[1 + dr:nrow + 1 + dr, 1 + dc:ncol + 1 + dc], out=new)
        new[~mask] = big
        if np.array_equal(new, lab[1:-1, 1:-1]):
            break
        lab[1:-1, 1:-1] = new
    return np.where(mask, lab[1:-1, 1:-1], -1)


def products(label, min_size=1, max_size=None, edge="any"):
    """the five planes of the rule from the label plane, and the info's counts: (dict of planes, dict of counts)"""
    label = np.asarray(label, dtype=np.int64)
    nrow, ncol = label.shape
    feat = label >= 0
    roots = np.unique(label[feat])                                  # ascending: the order of the ids
    idx = np.searchsorted(roots, np.where(feat, label, 0))          # per cell, the rank of its patch
    sizes = np.bincount(idx[feat], minlength=roots.size).astype(np.int64)
    border = np.zeros((nrow, ncol), dtype=bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    touches = np.zeros(roots.size, dtype=bool)
    touches[idx[feat & border]] = True
    passes = (sizes >= min_size) & (sizes <= (max_size if max_size is not None else nrow * ncol))
    passes &= {"any": np.ones(roots.size, dtype=bool), "touching": touches, "interior": ~touches}[edge]
    planes = {"label": label.astype(np.int32),
              "id": np.where(feat, idx + 1, 0).astype(np.int32),
              "size": np.where(feat, sizes[idx] if roots.size else 0, 0).astype(np.int32),
              "edge": np.where(feat, touches[idx] if roots.size else False, False).astype(np.uint8),
              "keep": np.where(feat, passes[idx] if roots.size else False, False).astype(np.uint8)}
    info = {"n_features": int(feat.sum()), "n_patches": int(roots.size), "n_kept_patches": int(passes.sum()),
            "n_kept_cells": int(sizes[passes].sum()), "max_size": int(sizes.max()) if roots.size else 0}
    return planes, info


def patches(mask, connectivity=8, min_size=1, max_size=None, edge="any", search=flood):
    """every plane of the rule for the feature mask, and the counts"""
    return products(search(mask, connectivity), min_size, max_size, edge)
