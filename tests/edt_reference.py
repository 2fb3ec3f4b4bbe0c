"""Brute-force definition of the map's distance fields (GridMap::updateESDF, grid_map.cpp:125-521), in plain numpy.

The reference builds every field from two Euclidean distance transforms of a binary grid: the distance to the nearest
occupied cell (`pos`) and the distance to the nearest free cell (`neg`).  It computes them by the separable
lower-envelope construction; this module states what that construction computes and evaluates the statement directly:
the squared index distance from a cell to its nearest seed is the minimum over ALL seed cells of the grid of
dx^2 + dy^2 (+ dz^2), an exact small integer.  There is no per-axis pass, no envelope and no intermediate buffer here,
so nothing in this file can share a mistake with a kernel or with harness/workload.hpp (fillESDF).

From the integers the reference's floating-point steps follow one by one, and each of them is correctly rounded in IEEE
double, so the result is defined to the bit:
    pos = res * sqrt(d2(occupied))          "no occupied cell anywhere": sqrt(numeric_limits<double>::max())
    neg = res * sqrt(d2(free))              likewise
    out = pos;  if (neg > 0) out += (-neg + res)            (grid_map.cpp:200-207)

The five fields (the occupancy grids hold 0 or 1; index order x, y, z with z fastest):
    esdf3d            from occ3d                                         (425-521)
    esdf2d            from occ2d                                         (125-207)
    critical          from the critical grid (the caller's, or "any occupied voxel in the column")   (211-279)
    critical_inflate  from the grid  critical < chassis_colli_radius     (283-351; the reference keeps it in esdf_buffer_2d_critical)
    inflate           from the grid  esdf2d   < chassis_colli_radius     (355-423)
"""
import numpy as np

DMAX = np.finfo(np.float64).max
NONE = -1   # sq_dist: there is no seed in the grid


def sq_dist(seeds, pairs_per_chunk=1 << 22):
    """Squared index distance from every cell to the nearest seed cell, int64, by global brute force: every cell against
    every seed of the whole 2-D or 3-D grid.  NONE everywhere when the grid has no seed.

    A seed cell is its own nearest seed (0), so only the other cells are searched: `pos` costs free x occupied pairs and
    `neg` occupied x free.  The pairs are walked in chunks of the smaller of the two sets."""
    seeds = np.asarray(seeds, dtype=bool)
    out = np.zeros(seeds.shape, dtype=np.int64)
    if not seeds.any():
        out[...] = NONE
        return out
    if seeds.all():
        return out
    s = np.argwhere(seeds).astype(np.int64)      # [k, nd]
    t = np.argwhere(~seeds).astype(np.int64)     # [m, nd]
    best = np.full(len(t), np.iinfo(np.int64).max, dtype=np.int64)
    if len(s) <= len(t):                          # few seeds: a chunk of seeds against all cells
        step = max(1, pairs_per_chunk // len(t))
        for a in range(0, len(s), step):
            d2 = np.zeros((len(t), len(s[a:a + step])), dtype=np.int64)
            for ax in range(seeds.ndim):
                d = t[:, None, ax] - s[None, a:a + step, ax]
                d2 += d * d
            np.minimum(best, d2.min(axis=1), out=best)
    else:                                         # few cells: a chunk of cells against all seeds
        step = max(1, pairs_per_chunk // len(s))
        for a in range(0, len(t), step):
            d2 = np.zeros((len(t[a:a + step]), len(s)), dtype=np.int64)
            for ax in range(seeds.ndim):
                d = t[a:a + step, None, ax] - s[None, :, ax]
                d2 += d * d
            best[a:a + step] = d2.min(axis=1)
    out[~seeds] = best
    return out


def _metres(d2, res):
    return res * np.sqrt(np.where(d2 == NONE, DMAX, d2.astype(np.float64)))


def signed_field(occupied, res):
    """The signed field of a boolean grid (True = occupied), in the reference's operation order."""
    occupied = np.asarray(occupied, dtype=bool)
    pos = _metres(sq_dist(occupied), res)
    neg = _metres(sq_dist(~occupied), res)
    out = pos.copy()
    m = neg > 0.0
    out[m] = out[m] + (-neg[m] + res)
    return out


def fields(occ2d, occ3d, dims, res, radius, occ2d_critical=None):
    """dict of the five fields, flat arrays in the library's index order.  occ*: 0/1 grids, flat or shaped."""
    nx, ny, nz = (int(v) for v in dims)
    o3 = np.asarray(occ3d).reshape(nx, ny, nz) == 1
    o2 = np.asarray(occ2d).reshape(nx, ny) == 1
    oc = o3.any(axis=2) if occ2d_critical is None else np.asarray(occ2d_critical).reshape(nx, ny) == 1
    esdf2d = signed_field(o2, res)
    critical = signed_field(oc, res)
    return dict(esdf3d=signed_field(o3, res).ravel(), esdf2d=esdf2d.ravel(), critical=critical.ravel(),
                inflate=signed_field(esdf2d < radius, res).ravel(),
                critical_inflate=signed_field(critical < radius, res).ravel())
