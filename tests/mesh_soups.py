"""Open and broken triangle meshes for the winding-number sign (PBF_MESH_SIGN_WINDING, pbf_mesh_winding): seven soups built from
tests/mesh_shapes.py that pbf_mesh_records refuses and pbf_mesh_soup_records accepts, each (vertices (nv, 3) float64, triangles
(nt, 3) uint32), plus the five closed shapes under the names the tests share."""
import numpy as np

import mesh_shapes as MS

CLOSED = ["box", "tetra", "torus", "ico2", "ico3"]
SOUPS = ["open1", "bowl", "cap3", "flipped", "dup", "slit", "twoboxes"]
ALL = SOUPS + CLOSED
SECOND_BOX = ((500.0, 400.0, 500.0), (800.0, 760.0, 900.0))


def _centroids(v, t):
    return v[t.astype(np.int64)].mean(axis=1)


def soup(name):
    if name == "open1":                                  # one face missing
        v, t = MS.shape("ico2")
        return v, t[:-1].copy()
    if name == "bowl":                                   # a sphere cut open at the top: a third of it missing
        v, t = MS.shape("ico2")
        return v, t[_centroids(v, t)[:, 2] < MS.CENTRE[2] + 60.0].copy()
    if name == "cap3":
        v, t = MS.shape("ico3")
        return v, t[_centroids(v, t)[:, 0] < MS.CENTRE[0] + 100.0].copy()
    if name == "flipped":                                # one face inside out
        v, t = MS.shape("ico2")
        t = t.copy()
        t[7] = t[7, ::-1]
        return v, t
    if name == "dup":                                    # one face twice
        v, t = MS.shape("ico2")
        return v, np.concatenate([t, t[5:6]])
    if name == "slit":                                   # a torus with one ring segment of its tube missing
        v, t = MS.shape("torus")
        return v, t[24:].copy()
    if name == "twoboxes":                               # two watertight parts pushed through each other
        v1, t1 = MS.box()
        v2, t2 = MS.box(*SECOND_BOX)
        return np.concatenate([v1, v2]), np.concatenate([t1, t2 + np.uint32(len(v1))])
    raise KeyError(name)


TETRA_3X5X4 = (313.0, 290.0, 333.0)     # mesh_shapes' tetra moved by 3 along x: its face x = 310 held a node of 3x5x4


def mesh(name, lattice=None):
    """a soup or a closed shape by name; on the tie lattice the box is the one whose faces pass through nodes (the case
    that lattice is for), and on 3x5x4 the tetra is shifted off the one node that lay on it (no node of 2x2x2, 3x5x4 or A
    may be nearer to a mesh than the value check allows: tests/test_mesh_winding_cpu.py asserts it)"""
    if name in SOUPS:
        return soup(name)
    if name == "box" and lattice == "ties":
        return MS.box(*MS.TIE_BOX)
    if name == "tetra" and lattice == "3x5x4":
        return MS.tetra(TETRA_3X5X4)
    return MS.shape(name)
