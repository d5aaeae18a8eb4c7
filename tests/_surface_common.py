"""Shared by the surface-statistics tests: a triangulated sphere matching cases.add_sphere, the physical scales a synthetic tunnel
lacks, and a reader of uncompressed VTU cell data and FieldData."""
import base64
import re
from types import SimpleNamespace

import numpy as np

from open_ludwig_amd.preprocess import SolverMesh

_NP = {"Float32": np.float32, "Float64": np.float64, "Int64": np.int64, "UInt8": np.uint8, "Int32": np.int32}


def sphere_mesh(center, radius, subdivisions=3, inside=True):
    """an icosphere (outward normals) about `center`; inside=True adds two tiny triangles at the centre, deep in the body (no search
    of radius 5 maps them to a fluid cell on a level whose sphere is more than 5 sqrt(3) cells in radius)"""
    t = (1.0 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
         [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    tris = np.array([[v[i] for i in tri] for tri in f], dtype=np.float64)
    tris /= np.linalg.norm(tris, axis=2, keepdims=True)
    for _ in range(subdivisions):
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ab, bc, ca = [(x + y) / np.linalg.norm(x + y, axis=1, keepdims=True) for x, y in ((a, b), (b, c), (c, a))]
        tris = np.concatenate([np.stack(q, axis=1) for q in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    tris = tris * radius + np.asarray(center, dtype=np.float64)
    if inside:
        c = np.asarray(center, dtype=np.float64)
        tiny = np.array([[[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]], [[0, 0, 0.05], [0, 0.1, 0.05], [0.1, 0, 0.05]]], dtype=np.float64)
        tris = np.concatenate([tris, tiny + c])
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    cp = np.cross(e1, e2)
    area = 0.5 * np.linalg.norm(cp, axis=1)
    flat = tris.reshape(-1, 3)
    return SolverMesh(tris, flat.min(axis=0), flat.max(axis=0), cp / (2.0 * area)[:, None], area, tris.mean(axis=1))


def tunnel_sphere_mesh(grids, subdivisions=3):
    """the sphere of cases.tunnel_with_sphere (centre and radius in level-1 cells, dx = 1 on level 1)"""
    g = grids[0]
    nbx, nby, nbz = g.grid_dim_x, g.grid_dim_y, g.grid_dim_z
    center = np.array([nbx * 8 * 0.4, nby * 8 * 0.5, nbz * 8 * 0.5])
    radius = 0.9 * 8 * min(nby, nbz) / 6.0 + 2.0
    return sphere_mesh(center, radius, subdivisions), center, radius


def tunnel_params(center, radius):
    """the physical scales forces.stress_from_cells / finish_forces read, for a synthetic tunnel in lattice units"""
    return SimpleNamespace(mesh_offset=np.zeros(3), rho_physical=1.225, velocity_scale=40.0, u_physical=2.0,
                           reference_area=float(np.pi * radius * radius), reference_chord=float(2 * radius),
                           moment_center=tuple(float(x) for x in center), time_scale=0.01)


def read_vtu(path):
    """{'n_cells', 'cells': {name: array}, 'fields': {name: array}, 'types': {name: VTK type}} of an uncompressed VTU"""
    txt = open(path).read()
    assert "compressor=" not in txt

    def dec(payload, dtype):
        n = int(np.frombuffer(base64.b64decode(payload[:12]), dtype=np.uint64)[0])
        return np.frombuffer(base64.b64decode(payload[12:])[:n], dtype=dtype)
    out = {"n_cells": int(re.search(r'NumberOfCells="(\d+)"', txt).group(1)), "cells": {}, "fields": {}, "types": {}}
    fd = re.search(r"<FieldData>(.*?)</FieldData>", txt, re.S)
    if fd:
        for m in re.finditer(r'<DataArray type="(\w+)" Name="(\w+)" NumberOfTuples="(\d+)" format="binary">([^<]*)</DataArray>', fd.group(1)):
            out["fields"][m.group(2)] = dec(m.group(4), _NP[m.group(1)])
            out["types"][m.group(2)] = m.group(1)
    cd = re.search(r"<CellData>(.*?)</CellData>", txt, re.S).group(1)
    for m in re.finditer(r'<DataArray type="(\w+)" Name="(\w+)"( NumberOfComponents="(\d+)")? format="binary">([^<]*)</DataArray>', cd):
        a = dec(m.group(5), _NP[m.group(1)])
        k = int(m.group(4) or 1)
        out["cells"][m.group(2)] = a.reshape(-1, k) if k > 1 else a
        out["types"][m.group(2)] = m.group(1)
    return out
