"""Unstructured meshes for the parity tests (TET4: tests/test_unstructured_meshes.py on the CPU, tests/test_gpu_unstructured.py
on the GPU; HEX8: tests/test_host_cl.py, tests/test_gpu_parity.py).  The Kuhn meshes of the other tests have valence 14 and
structured hexahedra rows of 27 node blocks; these reach the paths a real mesh takes:

  hydrogel   tests/golden/solid_hydrogel_tension_model.msh read as a plain TET4 mesh (5,504 tets, valence 31)
  delaunay   scipy Delaunay of a jittered 30^3 grid (179,455 tets, valence > 16: more workgroups than CUs)
  hub        a Kuhn mesh plus a hub of tetrahedra that share one vertex: a row longer than a row-gather workgroup's LDS
             budget, so that SCATTER_AUTO resolves to COLOURED
  over256    the same hub with more than 256 tetrahedra at one vertex: more colours than the colouring allows
  hex_fan    hexahedra around an axis (51 nodes, 16 elements): a row of 51 node blocks for the HEX8 cluster kernels

Fields are generated from the coordinates normalised to the unit cube (synth.*_fields expect [0, 1]^3)."""
from pathlib import Path

import numpy as np

from rdcfes_amd import synth

GOLDEN = Path(__file__).resolve().parent / "golden"
LDS_BUDGET = 50 * 1024                     # rdc_mesh_upload's row-gather budget on a 160 KB-LDS device
HUB_TETS = {5: 120, 3: 245}                # hub sizes that turn rowgather_ok off (5 unknowns: 80..90, 3 unknowns: 230..240)


def orient(conn, xyz):
    """swap two vertices of every negatively oriented tet"""
    conn = np.array(conn, dtype=np.uint32)
    X = xyz[conn.astype(np.int64)]
    v = np.einsum("ij,ij->i", np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), X[:, 3] - X[:, 0])
    neg = v < 0
    conn[neg, 2], conn[neg, 3] = conn[neg, 3].copy(), conn[neg, 2].copy()
    return np.ascontiguousarray(conn)


def unit_cube(xyz):
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    return (xyz - lo) / (hi - lo)


def hydrogel():
    from rdcfes_amd import gmsh
    m = gmsh.read_msh2(GOLDEN / "solid_hydrogel_tension_model.msh")
    assert m.elem_type == 4
    xyz = np.ascontiguousarray(m.xyz, dtype=np.float64)
    return orient(m.conn, xyz), xyz


def delaunay(n=30, seed=11):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*(np.arange(n),) * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    xyz = (g + rng.uniform(-0.3, 0.3, g.shape)) / (n - 1)       # jitter breaks the co-spherical ties of a grid
    tets = Delaunay(xyz).simplices.astype(np.uint32)
    X = xyz[tets.astype(np.int64)]
    v = np.einsum("ij,ij->i", np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), X[:, 3] - X[:, 0])
    tets = tets[np.abs(v) > 1e-9]                                # drop slivers (test_host_highvalence.py)
    perm = rng.permutation(tets.shape[0])                        # element order of a mesh file, not of the sweep
    return orient(tets[perm], xyz), np.ascontiguousarray(xyz)


def hub(n_hub, k=6):
    """Kuhn K(k) (random order) and a hub of n_hub tets that share only one vertex h, a corner of the cube: each hub tet
    brings three new nodes, so h has 3 n_hub new neighbours (a row of 3 n_hub + 1 + its Kuhn blocks) and n_hub new elements.
    The hub tets are thin cones along directions spread over a cap around the outward diagonal of the corner."""
    conn, xyz = synth.kuhn_tet_mesh(k, order="random")
    nn = xyz.shape[0]
    corner = np.flatnonzero(np.all((np.abs(xyz) < 1e-12) | (np.abs(xyz - 1.0) < 1e-12), axis=1))
    h = int(corner[np.argmin(elems_per_node(conn, nn)[corner])])
    out = (xyz[h] - 0.5) / np.linalg.norm(xyz[h] - 0.5)
    # Fibonacci points on the cap of half-angle 50 degrees around `out`
    i = np.arange(n_hub) + 0.5
    cos_t = 1.0 - (1.0 - np.cos(np.radians(50.0))) * i / n_hub
    phi = np.pi * (1.0 + 5.0 ** 0.5) * i
    e1 = np.cross(out, [1.0, 0.0, 0.0] if abs(out[0]) < 0.9 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(out, e1)
    sin_t = np.sqrt(1.0 - cos_t ** 2)
    d = cos_t[:, None] * out + sin_t[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    a1 = np.cross(d, e2 if abs(np.dot(out, e2)) < 0.9 else e1)
    a1 /= np.linalg.norm(a1, axis=1)[:, None]
    a2 = np.cross(d, a1)
    L, s = 0.5, 0.012
    tip = xyz[h] + L * d
    new = np.stack([tip + s * (np.cos(w) * a1 + np.sin(w) * a2) for w in (0.0, 2.0 * np.pi / 3.0, 4.0 * np.pi / 3.0)], axis=1)
    ids = nn + np.arange(3 * n_hub).reshape(n_hub, 3)
    star = np.column_stack([np.full(n_hub, h), ids])
    xyz2 = np.vstack([xyz, new.reshape(-1, 3)])
    return orient(np.vstack([conn, star]), xyz2), np.ascontiguousarray(xyz2)


def hex_fan(n_sectors=8, n_layers=2, seed=5):
    """Unstructured HEX8: per layer n_sectors hexahedra around the z axis, each with the bottom face (axis node, spoke node at
    radius 1 and angle t_s, outer node at radius 1.3 and t_s + pi / n, spoke node at t_(s+1)) and the same nodes one level up
    as its top face; nodes permuted and jittered by 0.03.  Every element touches the axis, so the middle axis node of two
    layers has every node of the mesh in its row: with 8 sectors 51 node blocks (a structured mesh has at most 27), which
    is what reaches the later passes of the cluster kernels' copy-out and long image segments of odd phase."""
    rng = np.random.default_rng(seed)
    t = 2.0 * np.pi * np.arange(n_sectors) / n_sectors
    ring = np.concatenate([[[0.0, 0.0]], np.column_stack([np.cos(t), np.sin(t)]),
                           1.3 * np.column_stack([np.cos(t + np.pi / n_sectors), np.sin(t + np.pi / n_sectors)])])
    per = ring.shape[0]                                          # axis, spokes 1 .. n, outer n + 1 .. 2 n
    xyz = np.concatenate([np.column_stack([ring, np.full(per, 0.6 * z)]) for z in range(n_layers + 1)])
    s = np.arange(n_sectors)
    bottom = np.column_stack([np.zeros_like(s), 1 + s, 1 + n_sectors + s, 1 + (s + 1) % n_sectors])
    conn = np.concatenate([np.column_stack([bottom + per * z, bottom + per * (z + 1)]) for z in range(n_layers)])
    xyz = xyz + rng.uniform(-0.03, 0.03, xyz.shape)
    pn = rng.permutation(xyz.shape[0])                           # new id of old node
    inv = np.empty_like(pn)
    inv[pn] = np.arange(pn.size)
    return np.ascontiguousarray(pn[conn], dtype=np.uint32), np.ascontiguousarray(xyz[inv])


def valence(conn, n_node):
    """number of distinct neighbours of every node"""
    c = conn.astype(np.int64)
    pairs = np.unique(np.concatenate([c[:, a] * n_node + c[:, b] for a in range(4) for b in range(4) if a != b]))
    return np.bincount(pairs // n_node, minlength=n_node)


def elems_per_node(conn, n_node):
    return np.bincount(conn.astype(np.int64).ravel(), minlength=n_node)
