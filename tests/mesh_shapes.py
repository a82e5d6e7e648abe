"""Closed triangle meshes generated for the mesh tests (test_mesh_cpu.py,
test_mesh_gpu.py), and STL writers in both forms."""

import math
import struct

import numpy as np


def cube(lo, hi):
    """12 triangles, outward normals."""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    v = [[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0], [x0, y0, z1], [x1, y0, z1], [x1, y1, z1],
         [x0, y1, z1]]
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (3, 0, 4, 7)]
    t = []
    for a, b, c, d in quads:
        t += [[a, b, c], [a, c, d]]
    return v, t


def octahedron(c, r):
    """|x - c| + |y - c| + |z - c| = r: 8 triangles, outward normals."""
    v = [[c[0] + r, c[1], c[2]], [c[0] - r, c[1], c[2]], [c[0], c[1] + r, c[2]], [c[0], c[1] - r, c[2]],
         [c[0], c[1], c[2] + r], [c[0], c[1], c[2] - r]]
    t = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return v, t


def icosphere(c, r, subdivisions):
    """20 * 4^subdivisions triangles, every vertex at distance r from c (up to
    rounding), outward normals."""
    g = (1 + math.sqrt(5)) / 2
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / math.sqrt(1 + g * g) for p in v]
    for _ in range(subdivisions):
        mid, nt = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c_ in t:
            ab, bc, ca = m(a, b), m(b, c_), m(c_, a)
            nt += [(a, ab, ca), (b, bc, ab), (c_, ca, bc), (ab, bc, ca)]
        t = nt
    verts = [[float(c[a] + r * p[a]) for a in range(3)] for p in v]
    return verts, [list(x) for x in t]


def as_float32(vertices):
    """The vertices rounded to float32 (what a binary STL stores)."""
    return np.asarray(vertices, dtype=np.float32).astype(np.float64).tolist()


def write_binary_stl(path, vertices, triangles):
    v = np.asarray(vertices, dtype=np.float32)
    with open(path, "wb") as f:
        f.write(b"binary stl".ljust(80, b" "))
        f.write(struct.pack("<I", len(triangles)))
        for t in triangles:
            f.write(struct.pack("<12fH", 0.0, 0.0, 0.0, *[float(x) for i in t for x in v[i]], 0))


def write_ascii_stl(path, vertices, triangles):
    v = np.asarray(vertices, dtype=np.float32)
    with open(path, "w") as f:
        f.write("solid test\n")
        for t in triangles:
            f.write(" facet normal 0 0 0\n  outer loop\n")
            for i in t:
                f.write("   vertex %.17g %.17g %.17g\n" % tuple(float(x) for x in v[i]))
            f.write("  endloop\n endfacet\n")
        f.write("endsolid test\n")
