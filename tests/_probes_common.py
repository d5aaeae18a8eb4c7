"""Probe layouts shared by the GPU probe tests and their 2-rank worker."""
import numpy as np

from open_ludwig_amd import probes as pm


def tunnel_points(grids):
    """points on every level of a cases.tunnel_with_sphere hierarchy (sphere of radius 6.8 about (19.2, 16, 16) in level-1 cells):
    interior ones, ones at a refinement edge, at the domain's faces and next to the sphere (corners replaced by the base cell)"""
    cand = [[27.1, 16.1, 16.2], [27.95, 15.1, 14.2], [10.3, 20.1, 20.2], [47.9, 2.1, 2.2], [3.1, 31.8, 31.9], [13.9, 12.1, 12.3],
            [31.9, 22.3, 9.4], [5.37, 7.71, 29.05], [23.6, 9.9, 19.75], [35.2, 16.0, 16.0]]
    ok = []
    for q in cand:
        try:
            pm.plan_probes([q], grids)
            ok.append(q)
        except ValueError:
            pass
    for x in np.arange(11.0, 16.0, 0.05):                    # upstream of the sphere on the finest level: +x corners in the body
        try:
            pl = pm.plan_probes([[x, 16.05, 16.05]], grids)
        except ValueError:
            continue
        if pl.level[0] == len(grids) - 1 and pl.replaced[0].any():
            ok.append([x, 16.05, 16.05])
            break
    return pm.plan_probes(ok, grids)


def straddling_points(grids, owners, per_level=6, others=2):
    """points whose stencil reaches blocks of two owners (a face, edge or corner of the cut), on every level, and on every level
    `others` more whose base block another rank owns (so that every rank samples some)"""
    pts = []
    for li, g in enumerate(grids):
        own = np.asarray(owners[li])
        found = 0
        rest = {}
        for b, (bx, by, bz) in enumerate(g.active_block_coords):
            if found >= per_level and all(v >= others for v in rest.values()) and len(rest) == len(set(own.tolist())):
                break
            # the block's +x+y+z corner: the stencil of a point just below it spans the 8 blocks around that corner
            q = (np.array([bx, by, bz], float) * 8 - 0.5 + np.array([0.3, 0.45, 0.2])) * g.dx
            try:
                pl = pm.plan_probes([q], grids)
            except ValueError:
                continue
            if pl.level[0] != li:
                continue
            if found < per_level and len(set(own[pl.blocks[0]].tolist())) > 1:
                pts.append(q)
                found += 1
                rest.setdefault(int(own[pl.blocks[0, 0]]), 0)
            elif rest.get(int(own[pl.blocks[0, 0]]), 0) < others:
                pts.append(q)
                rest[int(own[pl.blocks[0, 0]])] = rest.get(int(own[pl.blocks[0, 0]]), 0) + 1
    return pm.plan_probes(pts, grids)
