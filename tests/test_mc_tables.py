"""The generated marching-cubes tables (tools/gen_mc_tables.py -> csrc/mc_tables.hpp, oracle/mc_tables.h).

The reference's tables (src/mc_constants.h) are data we may not copy, so ours are derived from first
principles; these tests pin the properties that make them a valid marching-cubes table set:
combinatorially watertight and consistently oriented on random fields, EdgeTable == crossed edges,
NumVerts == row length, complement cases cross the same edges, the two copies are identical and
reproducible from the generator."""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
EDGES = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]


def load(path):
    txt = open(path).read()

    def arr(name):
        body = re.search(name + r"\[256\](?:\[16\])? = \{(.*?)\};", txt, re.S).group(1)
        return [int(v, 0) for v in re.findall(r"0x[0-9a-fA-F]+|\d+", body)]

    edge, nv = arr("kMcEdgeTable"), arr("kMcNumVerts")
    tri = np.array(arr("kMcTriTable")).reshape(256, 16)
    return edge, nv, tri


def test_tables_consistent_and_reproducible(tmp_path):
    a = open(os.path.join(ROOT, "pbf-sph_amd", "csrc", "mc_tables.hpp")).read()
    b = open(os.path.join(ROOT, "oracle", "mc_tables.h")).read()
    strip = lambda s: re.sub(r"PBF_(ORACLE_)?MC_TABLES_H(PP)?", "G", s)  # noqa: E731
    assert strip(a) == strip(b)
    edge, nv, tri = load(os.path.join(ROOT, "oracle", "mc_tables.h"))
    for ci in range(256):
        row = [v for v in tri[ci] if v != 255]
        assert len(row) == nv[ci] and nv[ci] % 3 == 0 and tri[ci][len(row)] == 255
        crossed = sum(1 << i for i, (p, q) in enumerate(EDGES) if ((ci >> p) & 1) != ((ci >> q) & 1))
        assert edge[ci] == crossed
        assert sum(1 << e for e in set(row)) == crossed  # every crossed edge is used, nothing else
        assert edge[255 - ci] == edge[ci]
    assert nv[0] == nv[255] == 0 and all(nv[1 << k] == 3 for k in range(8))
    # the classic EdgeTable values for the single-corner cases (public knowledge, also SURVEY's edge numbering)
    assert [edge[1], edge[2], edge[4], edge[8]] == [0x109, 0x203, 0x406, 0x80c]


def test_watertight_and_oriented_on_random_fields():
    """Every interior mesh edge is shared by exactly two triangles with opposite direction."""
    _, _, tri = load(os.path.join(ROOT, "oracle", "mc_tables.h"))
    rng = np.random.default_rng(7)
    n = 10
    for trial in range(6):
        f = rng.random((n, n, n))  # white noise: hits every ambiguous configuration
        inside = f < 0.5
        node = lambda x, y, z: (x * n + y) * n + z  # noqa: E731
        directed = {}
        seen_cases = set()
        for x in range(n - 1):
            for y in range(n - 1):
                for z in range(n - 1):
                    ids = [node(x + c[0], y + c[1], z + c[2]) for c in CORNERS]
                    ci = sum(1 << k for k, c in enumerate(CORNERS) if inside[x + c[0], y + c[1], z + c[2]])
                    seen_cases.add(ci)
                    row = [e for e in tri[ci] if e != 255]
                    for t in range(0, len(row), 3):
                        vs = [tuple(sorted((ids[EDGES[e][0]], ids[EDGES[e][1]]))) for e in row[t:t + 3]]
                        assert len(set(vs)) == 3
                        for k in range(3):
                            key = (vs[k], vs[(k + 1) % 3])
                            directed[key] = directed.get(key, 0) + 1
        assert len(seen_cases) > 200
        # boundary of the sampled block: mesh edges lying in a boundary face are open by construction
        def on_boundary(v):
            (a, b) = v
            ca, cb = np.unravel_index(a, (n, n, n)), np.unravel_index(b, (n, n, n))
            return any((ca[k] == cb[k]) and ca[k] in (0, n - 1) for k in range(3))
        bad = 0
        for (u, v), cnt in directed.items():
            if on_boundary(u) and on_boundary(v):
                continue
            if cnt != 1 or directed.get((v, u), 0) != 1:
                bad += 1
        assert bad == 0, bad


# ---- pinned against the REFERENCE's tables (src/mc_constants.h:4,23,154) -------------------------------------------
def _digests():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.mc_case_digests


def test_tables_vs_reference_digest():
    """tests/golden/ref_mc_digest.npz was generated from the reference's mc_constants.h compiled where it lies
    (tests/golden/make_golden.py ref_mc): EdgeTable and NumVertsTable as numbers, TriTable as per-case digests.
    Ours: EdgeTable equal, NumVertsTable equal (=> the same triangle count per cube, hence the same 'Final Vertex
    count' for the same field), the polygons each case is tiled into equal — as oriented loops — in all 256 cases;
    how a polygon with more than three corners is split into triangles is NOT derivable from first principles (the
    classic table inherits it from hand-made base cases and their rotations): the triangle sets agree in exactly 98
    cases, the other 158 tile the same polygons with other diagonals."""
    S = np.load(os.path.join(ROOT, "tests", "golden", "ref_mc_digest.npz"))
    edge, nv, tri = load(os.path.join(ROOT, "oracle", "mc_tables.h"))
    assert np.array_equal(np.array(edge, np.uint32), S["edge"])
    assert np.array_equal(np.array(nv, np.uint32), S["numverts"])
    loops_crc, tris_crc = _digests()(tri)
    assert np.array_equal(loops_crc, S["loops_crc"])           # same polygons, same orientation: 256 / 256
    same = int((tris_crc == S["tris_crc"]).sum())
    assert same == 98, same
    # every case made of triangles only (no polygon to split) must agree exactly
    for ci in range(256):
        row = [v for v in tri[ci] if v != 255]
        tris = [tuple(row[i:i + 3]) for i in range(0, len(row), 3)]
        directed = {e for a, b, c in tris for e in ((a, b), (b, c), (c, a))}
        if all((b, a) not in directed for a, b in directed):   # no interior diagonal at all
            assert tris_crc[ci] == S["tris_crc"][ci], ci


def test_tables_vs_reference_live():
    """The same comparison against the reference header itself where oracle/_ref/libref_mc.so was built from it;
    elsewhere the reference side is the committed digest of that header's tables."""
    import ctypes as C
    so = os.path.join(ROOT, "oracle", "_ref", "libref_mc.so")
    S = np.load(os.path.join(ROOT, "tests", "golden", "ref_mc_digest.npz"))
    edge, nv, tri = load(os.path.join(ROOT, "oracle", "mc_tables.h"))
    if os.path.exists(so):
        R = C.CDLL(so)
        for f in (R.ref_mc_edge, R.ref_mc_numverts, R.ref_mc_tri):
            f.restype = C.c_uint32
        ref_edge = [R.ref_mc_edge(ci) for ci in range(256)]
        ref_nv = [R.ref_mc_numverts(ci) for ci in range(256)]
        la, ta = _digests()([[R.ref_mc_tri(ci, j) for j in range(16)] for ci in range(256)])
    else:
        ref_edge, ref_nv, la, ta = list(S["edge"]), list(S["numverts"]), S["loops_crc"], S["tris_crc"]
    assert ref_edge == list(edge)
    assert ref_nv == list(nv)
    lb, tb = _digests()(tri)
    assert np.array_equal(la, lb) and int((ta == tb).sum()) == 98
    assert np.array_equal(la, S["loops_crc"]) and np.array_equal(ta, S["tris_crc"])   # the fixture is current
