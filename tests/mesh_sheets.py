"""Flat sheets: the meshes on which EVERY 1-ring covariance of the ARAP local step has rank 2 (a ground plane, a wall), which the
closed smooth surfaces of the rest of the suite never produce.  tests/test_valence_meshes.py checks the builder and the CPU
references on them, tests/test_gpu_valence.py runs the solvers.

A planar grid with alternating diagonals (valence 8 and 4 inside), its interior vertices jittered in the plane by +-0.25 cell,
scaled by 0.05.  Axis-aligned, z = 0 makes the third row and column of every covariance exactly zero; tilted by a random
rotation, the smallest singular value is rounding noise of either sign.  The jitter makes many angles obtuse: real edges whose two
cotangents are both clamped have weight exactly 0.0, the kernels' padding sentinel.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from multiviewstitch_amd import scene as S

SEED = 4171
CELL = 0.05
SIZES = {"small": (21, 17), "large": (56, 40)}              # large: >= 2048 vertices, MVS_SOLVER_AUTO takes the patch solver
CASES = ("small_flat", "small_tilted", "large_flat", "large_tilted")
NODE_STEP = 13


@dataclasses.dataclass(frozen=True)
class Sheet:
    name: str
    pts: np.ndarray             # (V, 3)
    normals: np.ndarray         # (V, 3)
    faces: np.ndarray           # (F, 3) int32
    Q: np.ndarray               # plane coordinates -> world (identity for the flat sheets)
    nodes: np.ndarray           # every NODE_STEP-th vertex, int32
    targets: np.ndarray         # (len(nodes), 3)

    @property
    def n(self):
        """the plane's unit normal"""
        return self.Q[:, 2]

    @property
    def extent(self):
        return float(np.abs(self.pts).max())

    @property
    def expect(self):
        return ("patch", 8) if len(self.pts) >= 2048 else ("cg", 0)


def _deform(p):
    """in the plane: a rotation by 0.4 rad, a shear and a ripple; z stays 0"""
    c, s = np.cos(0.4), np.sin(0.4)
    M = np.array([[c, -s], [s, c]]) @ np.array([[1.0, 0.15], [0.0, 1.0]])
    q = p[:, :2] @ M.T + 0.01 * np.sin(9 * p[:, :2])
    return np.concatenate([q, np.zeros((len(p), 1))], axis=1)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Sheet:
    size, kind = name.split("_")
    nx, ny = SIZES[size]
    rng = np.random.default_rng(SEED + nx)
    j, i = np.mgrid[0:ny, 0:nx]
    xy = np.stack([i, j], axis=-1).astype(np.float64)
    xy[1:-1, 1:-1] += rng.uniform(-0.25, 0.25, size=(ny - 2, nx - 2, 2))
    plane = np.concatenate([xy.reshape(-1, 2) * CELL, np.zeros((nx * ny, 1))], axis=1)
    faces = []
    for b in range(ny - 1):
        for a in range(nx - 1):
            v00, v10, v01, v11 = b * nx + a, b * nx + a + 1, (b + 1) * nx + a, (b + 1) * nx + a + 1
            if (a + b) % 2 == 0:
                faces += [(v00, v10, v11), (v00, v11, v01)]
            else:
                faces += [(v00, v10, v01), (v10, v11, v01)]
    faces = np.array(faces, np.int32)
    Q = np.eye(3)
    if kind == "tilted":
        Q, r = np.linalg.qr(np.random.default_rng(SEED + 1).normal(size=(3, 3)))
        Q = Q * np.sign(np.diag(r))
        if np.linalg.det(Q) < 0:
            Q[:, 2] = -Q[:, 2]
    pts = plane @ Q.T
    nodes = np.arange(0, len(pts), NODE_STEP, dtype=np.int32)
    targets = _deform(plane[nodes]) @ Q.T
    normals = S.vertex_normals_plyobj(pts, faces)
    for a in (pts, normals, faces, Q, nodes, targets):
        a.setflags(write=False)
    return Sheet(name, pts, normals, faces, Q, nodes, targets)


# (energy rel., vertex RMS / extent, rotation RMS) oracle.arap and ref_numpy.arap were measured to differ by at SEED, rounded up
# (tests/test_valence_meshes.py asserts that it still holds); the GPU tolerance is max(project figure, ten times this)
# largest measured: energy 9.6e-14 (large_flat), vertex RMS / extent 6.2e-15 (large_flat), rotation RMS 1.3e-13 (large_tilted)
CPU_DISAGREEMENT = {c: (2e-13, 1e-14, 3e-13) for c in CASES}
# real edges of weight exactly 0.0 (directed count) the oracle's cotangent weights hold at SEED: 146 of 1992, 938 of 13058
ZERO_WEIGHT_EDGES = {"small": 146, "large": 938}
