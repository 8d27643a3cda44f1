"""The reconcile step in plain Python: the canonical preference order of decoded records and the overlap rule that removes duplicates.

Written from the wording of DESIGN.md section 2 ("detections reconciled in the order (family, id, hamming, -margin, corners)") and of
the oracle's header: records are sorted by family, id, lower hamming, higher decision margin, then the eight corner coordinates
p[0][0], p[0][1], p[1][0] ... ascending; walking that order, a record is dropped when a record already KEPT with the same family and
id overlaps it.  Two quads overlap when a side of one meets a side of the other -- a proper crossing, or an end point that lies on
the other side (collinear and within its bounding box) -- or when the first corner of one lies inside the other by the even-odd
rule of a ray towards -x.  Python floats are IEEE doubles, and every expression below applies the operations in the order the
definition states them, so the decisions are the definition's, bit for bit.  Nothing here sorts by rank, tracks runs or knows lanes."""


def order_key(rec):
    """The canonical preference order as a tuple Python compares lexicographically.  -margin is exact (a sign flip)."""
    return (int(rec["family"]), int(rec["id"]), int(rec["hamming"]), -float(rec["decision_margin"])) + \
        tuple(float(rec["p"][i][k]) for i in range(4) for k in range(2))


def _side_of(a, b, c):
    """> 0, < 0 or == 0: on which side of the line a -> b the point c lies."""
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def _in_box(a, b, c):
    return min(a[0], b[0]) <= c[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= c[1] <= max(a[1], b[1])


def _opposite(u, v):
    return (u > 0 and v < 0) or (u < 0 and v > 0)


def sides_meet(p1, p2, q1, q2):
    d1, d2 = _side_of(q1, q2, p1), _side_of(q1, q2, p2)
    d3, d4 = _side_of(p1, p2, q1), _side_of(p1, p2, q2)
    if _opposite(d1, d2) and _opposite(d3, d4):   # the ends of each side lie strictly on either side of the other: a proper crossing
        return True
    return (d1 == 0 and _in_box(q1, q2, p1)) or (d2 == 0 and _in_box(q1, q2, p2)) or \
        (d3 == 0 and _in_box(p1, p2, q1)) or (d4 == 0 and _in_box(p1, p2, q2))


def corner_inside(poly, q):
    inside = False
    for i in range(4):
        a, b = poly[i], poly[i - 1]
        if (a[1] > q[1]) != (b[1] > q[1]) and q[0] < (b[0] - a[0]) * (q[1] - a[1]) / (b[1] - a[1]) + a[0]:
            inside = not inside
    return inside


def quads_overlap(a, b):
    for i in range(4):
        for j in range(4):
            if sides_meet(a[i], a[(i + 1) % 4], b[j], b[(j + 1) % 4]):
                return True
    return corner_inside(a, b[0]) or corner_inside(b, a[0])


def _quad(rec):
    return [(float(rec["p"][i][0]), float(rec["p"][i][1])) for i in range(4)]


def reconcile(records):
    """Indices into `records` of the kept ones, in their final order."""
    order = sorted(range(len(records)), key=lambda i: order_key(records[i]))   # (stable: exact duplicates stay in input order)
    kept = []
    for i in order:
        ri, qi = records[i], _quad(records[i])
        if not any(records[j]["family"] == ri["family"] and records[j]["id"] == ri["id"] and quads_overlap(_quad(records[j]), qi)
                   for j in kept):
            kept.append(i)
    return kept
