#!/usr/bin/env python3
"""Derives the marching-cubes table of bodyfit_volume_surface_* (include/bodyfit.h states the rule) and writes it as
3dbodyanimation_amd/csrc/mc_table_inl.h.  Nothing here is recalled from a published table: the 256 rows follow from the rule.

    corner c of a cell          (i + (c & 1), j + (c >> 1 & 1), k + (c >> 2 & 1)); bit c of the case: corner c is INSIDE
    edge e = 4 axis + r         joins the r-th corner (ascending) whose `axis` bit is clear to that corner with the bit set
    on each of the six faces    the crossed face edges are joined by segments: two crossings, one segment; four crossings (the
                                ambiguous face), two segments that each cut off ONE INSIDE corner (both cells that share the face
                                see the same four signs and draw the same segments)
    direction                   one handedness for every segment: seen from outside the cube, the inside corners a segment cuts
                                off lie on its right; it makes case 1 the triangle (0, 4, 8), normal away from corner 0
    loops                       following the directed segments closes loops; they are taken in ascending order of their smallest
                                edge, each from that edge in its direction
    fan                         a loop of length L gives L - 2 triangles (a, v_i, v_i+1) from an apex a: the first rotation of the
                                loop none of whose fan diagonals joins two edges of one cube face (such a diagonal lies in the face
                                and would collide with the neighbouring cell's)

    python3 tools/gen_mc_table.py            # rewrites csrc/mc_table_inl.h
    python3 tools/gen_mc_table.py --check    # exit status 1 unless the committed header holds exactly these numbers
"""
import os
import sys

import numpy as np

MAX_TRI = 5
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3dbodyanimation_amd", "csrc", "mc_table_inl.h")


def corner_xyz(c):
    return np.array([c & 1, c >> 1 & 1, c >> 2 & 1], np.int64)


def edge_corners(e):
    """the two corners of edge e = 4 axis + r: (the corner with the axis bit clear, the one with it set)"""
    axis, r = divmod(e, 4)
    low = [c for c in range(8) if not c >> axis & 1][r]
    return low, low | 1 << axis


EDGE_OF = {frozenset(edge_corners(e)): e for e in range(12)}


def edge_faces(e):
    """the two cube faces (axis, value) that hold edge e"""
    axis = e // 4
    a = edge_corners(e)[0]
    return {(b, a >> b & 1) for b in range(3) if b != axis}


def midpoint(e):
    a, b = edge_corners(e)
    return (corner_xyz(a) + corner_xyz(b)) / 2.0


def face_cycle(axis, value):
    """the four corners of face (axis, value) in cyclic order"""
    b, c = [x for x in range(3) if x != axis]
    base = value << axis
    return [base, base | 1 << b, base | 1 << b | 1 << c, base | 1 << c]


def directed(p, q, cut_off, axis, value):
    """the segment between the face edges p and q of face (axis, value), directed so that the inside corners `cut_off` lie on its
    right for a viewer outside the cube"""
    n = np.zeros(3)
    n[axis] = 1.0 if value else -1.0
    centre = np.mean([corner_xyz(c) for c in cut_off], axis=0)
    side = float(n @ np.cross(midpoint(q) - midpoint(p), centre - midpoint(p)))
    assert side != 0.0
    return (p, q) if side < 0.0 else (q, p)


def segments(case):
    out = []
    for axis in range(3):
        for value in (0, 1):
            cyc = face_cycle(axis, value)
            ins = [bool(case >> c & 1) for c in cyc]
            crossed = [m for m in range(4) if ins[m] != ins[(m + 1) % 4]]        # face edge m joins cyc[m] and cyc[m + 1]
            edge = [EDGE_OF[frozenset((cyc[m], cyc[(m + 1) % 4]))] for m in range(4)]
            if len(crossed) == 2:
                out.append(directed(edge[crossed[0]], edge[crossed[1]], [c for c, s in zip(cyc, ins) if s], axis, value))
            elif len(crossed) == 4:
                for m in range(4):
                    if ins[m]:                                                   # the two face edges at the inside corner cyc[m]
                        out.append(directed(edge[(m - 1) % 4], edge[m], [cyc[m]], axis, value))
    return out


def loops(case):
    nxt = {}
    for p, q in segments(case):
        assert p not in nxt, (case, p)
        nxt[p] = q
    assert sorted(nxt) == sorted(nxt.values())                                   # one segment in, one out, at every crossed edge
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3
        out.append(loop)
    return out


def fan(loop):
    L = len(loop)
    for r in range(L):
        v = loop[r:] + loop[:r]
        if all(not (edge_faces(v[0]) & edge_faces(v[m])) for m in range(2, L - 1)):
            return [(v[0], v[m], v[m + 1]) for m in range(1, L - 1)]
    raise AssertionError(f"no apex for the loop {loop}")


def case_triangles(case):
    return [t for loop in loops(case) for t in fan(loop)]


def table():
    """(n_tri u8 [256], tri u8 [256][16]: the 3 n_tri edge ids of the case's triangles, then 255)"""
    n_tri = np.zeros(256, np.uint8)
    tri = np.full((256, 16), 255, np.uint8)
    for case in range(256):
        tris = case_triangles(case)
        assert len(tris) <= MAX_TRI
        n_tri[case] = len(tris)
        tri[case, :3 * len(tris)] = np.asarray(tris, np.uint8).reshape(-1)
    return n_tri, tri


def header_text():
    n_tri, tri = table()
    rows = ["// GENERATED by tools/gen_mc_table.py (the rule: include/bodyfit.h, SURFACE EXTRACTION): do not edit.",
            "// MC_N_TRI[case]: the triangles of the case; MC_TRI[case]: their 3 n edge ids (e = 4 axis + r) in order, then 255.",
            "// MC_TABLE_STORAGE: where the two arrays live (a HIP unit defines it as __constant__ before the include).",
            "#pragma once",
            "#ifndef MC_TABLE_STORAGE",
            "#define MC_TABLE_STORAGE static const",
            "#endif",
            f"#define MC_MAX_TRI {MAX_TRI}",
            "MC_TABLE_STORAGE unsigned char MC_N_TRI[256] = {"]
    for a in range(0, 256, 32):
        rows.append("  " + ", ".join(str(int(x)) for x in n_tri[a:a + 32]) + ",")
    rows.append("};")
    rows.append("alignas(16) MC_TABLE_STORAGE unsigned char MC_TRI[256][16] = {")
    for case in range(256):
        rows.append("  {" + ", ".join(f"{int(x):3d}" for x in tri[case]) + "},")
    rows.append("};")
    return "\n".join(rows) + "\n"


def parse_header(text):
    """the numbers of a header written by header_text: (n_tri [256], tri [256][16])"""
    import re
    body = re.sub(r"//[^\n]*", "", text)
    first = re.search(r"MC_N_TRI\[256\] = \{(.*?)\};", body, re.S).group(1)
    second = re.search(r"MC_TRI\[256\]\[16\] = \{(.*)\};", body, re.S).group(1)
    return (np.array(re.findall(r"\d+", first), np.int64).astype(np.uint8),
            np.array(re.findall(r"\d+", second), np.int64).astype(np.uint8).reshape(256, 16))


if __name__ == "__main__":
    text = header_text()
    if "--check" in sys.argv[1:]:
        sys.exit(0 if os.path.exists(HEADER) and open(HEADER).read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    n_tri, _ = table()
    print(f"{HEADER}: {int(n_tri.sum())} triangles, at most {int(n_tri.max())} in a row, "
          f"histogram {np.bincount(n_tri, minlength=MAX_TRI + 1).tolist()}")
