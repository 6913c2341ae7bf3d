"""Host half of ``rs features``: boundary edges -> rings -> simplified, georeferenced GeoJSON polygons (numpy + stdlib only;
the reference uses OpenCV contours, shapely and geojson: ``robosat/features/core.py``, ``robosat/features/parking.py``).

Vertices are pixel corners, integer (x, y) in [0, W] x [0, H], y down.  An edge row is ``(tile, label, x, y, dir)``: the
pixel (x, y) of component ``label`` walked round with the pixel on the right -- dir 0 top (x,y)->(x+1,y), 1 right
(x+1,y)->(x+1,y+1), 2 bottom (x+1,y+1)->(x,y+1), 3 left (x,y+1)->(x,y).  With that orientation the shoelace area of a
component's outer ring is positive, its holes' negative, and the areas of its rings sum to its pixel count.

``--geometry centerline`` has its own half at the end of the file: skeleton links -> lines -> pruned, simplified LineStrings."""

import json
import math
import sys

import numpy as np

from robosat_amd.tiles import Tile, pixel_to_location, tile_bounds

_SX = np.array([0, 1, 1, 0], dtype=np.int64)  # start corner of an edge, relative to its pixel
_SY = np.array([0, 0, 1, 1], dtype=np.int64)
_DX = np.array([1, 0, -1, 0], dtype=np.int64)  # heading
_DY = np.array([0, 1, 0, -1], dtype=np.int64)


def signed_area(ring):
    """Shoelace area of an open ring [[x, y], ...] (positive for the outer rings ``link_rings`` returns); exact for integers."""

    ring = np.asarray(ring)
    x, y = ring[:, 0], ring[:, 1]
    twice = np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)
    return twice / 2 if twice % 2 else twice // 2


def _rotate_to_smallest(ring):
    start = np.lexsort((ring[:, 1], ring[:, 0]))[0]
    return np.roll(ring, -start, axis=0)


def _link(group, x, y, d, bits, turns):
    """The linking itself: edges (pixel x, y, dir d) of int64 ``group`` ids, vertices below 2^bits -> [(first edge, ring), ...] in
    the order of the sort key (group, y, x, dir) of each ring's smallest edge; ``(group << 2 * bits + 2)`` must fit an int64."""

    n = len(group)
    sx, sy = x + _SX[d], y + _SY[d]
    ex, ey = sx + _DX[d], sy + _DY[d]

    def key(g, vx, vy, direction):
        return ((g << 2 * bits | vy << bits | vx) << 2) | direction

    out_key = key(group, sx, sy, d)
    order = np.argsort(out_key, kind="stable")
    sorted_keys = out_key[order]
    assert n == 1 or (np.diff(sorted_keys) > 0).all(), "duplicate edges"
    nxt = np.full(n, -1, dtype=np.int64)
    for turn in turns:  # left, straight, right
        want = key(group, ex, ey, (d + turn) & 3)
        pos = np.minimum(np.searchsorted(sorted_keys, want), n - 1)
        hit = (sorted_keys[pos] == want) & (nxt < 0)
        nxt[hit] = order[pos[hit]]
    assert (nxt >= 0).all(), "an edge without a successor: the edge list is not the boundary of a label image"

    nxt_l, order_l = nxt.tolist(), order.tolist()
    seen = bytearray(n)
    rings = []
    for start in order_l:
        if seen[start]:
            continue
        idx = []
        cur = start
        while not seen[cur]:
            seen[cur] = 1
            idx.append(cur)
            cur = nxt_l[cur]
        assert cur == start, "edges do not close into a ring"
        idx = np.array(idx)
        rings.append((start, _rotate_to_smallest(np.stack([sx[idx], sy[idx]], axis=1))))
    return rings


def _ring_order(ring):
    return signed_area(ring) < 0, int(ring[0, 0]), int(ring[0, 1])


def link_rings(edges, turns=(3, 0, 1)):
    """Edge rows int [E, 5] in any order -> ``{(tile, label): [ring, ...]}``; a ring is an int64 array [k, 2] of unit-step
    vertices, not closed, started at its lexicographically smallest (x, y); the component's outer ring first, then its holes
    ordered by their first vertex.

    Edges of one label link head to tail.  Where a vertex has two outgoing edges of the label (two of its pixels meeting
    only at that corner) the walk takes the LEFT turn, onto the diagonally opposite pixel's edge: rings then never touch
    themselves, and every component has exactly one ring of positive area.  ``turns`` is that preference (left, straight, right as
    dir + 3, + 0, + 1); the tests pass the right turn first to show what it does."""

    e = np.asarray(edges, dtype=np.int64).reshape(-1, 5)
    n = len(e)
    if n == 0:
        return {}
    tile, label, x, y, d = e.T
    assert tile.min() >= 0 and tile.max() < 1024 and label.min() >= 1 and label.max() <= 1 << 24, "tile < 1024, label <= 2^24"
    assert x.min() >= 0 and y.min() >= 0 and max(x.max(), y.max()) < 4096 and d.min() >= 0 and d.max() <= 3
    rings = {}
    for start, ring in _link(tile << 25 | label, x, y, d, 13, turns):
        rings.setdefault((int(tile[start]), int(label[start])), []).append(ring)
    for group_rings in rings.values():
        group_rings.sort(key=_ring_order)
    return rings


MOSAIC_SIDE = 1 << 16  # pixels per side a stitched component may span (17-bit vertex coordinates in the linking key)
MOSAIC_COMPONENTS = 1 << 27  # components per call (the rest of the 63 key bits)


def link_rings_mosaic(edges, turns=(3, 0, 1)):
    """``link_rings`` for stitched edge rows int [E, 4] = (label, X, Y, dir) in mosaic pixels -> ``{label: [ring, ...]}`` with
    the rings in mosaic pixels.  Labels (up to 2^29) are ranked densely and every component is linked relative to the corner
    of its own bounding box, so what must fit the key is a component's extent (at most 2^16 pixels a side, whatever the
    mosaic's) and the number of components (below 2^27); beyond either: ValueError."""

    e = np.asarray(edges, dtype=np.int64).reshape(-1, 4)
    if len(e) == 0:
        return {}
    label, x, y, d = e.T
    if label.min() < 1 or x.min() < 0 or y.min() < 0 or d.min() < 0 or d.max() > 3:
        raise ValueError("edge rows are (label >= 1, X >= 0, Y >= 0, dir 0..3)")
    labels, rank = np.unique(label, return_inverse=True)
    rank = rank.reshape(-1).astype(np.int64)
    if len(labels) >= MOSAIC_COMPONENTS:
        raise ValueError("{} components in one call: ring linking takes fewer than 2^27".format(len(labels)))
    x0 = np.full(len(labels), np.iinfo(np.int64).max)
    y0 = x0.copy()
    np.minimum.at(x0, rank, x)
    np.minimum.at(y0, rank, y)
    rx, ry = x - x0[rank], y - y0[rank]
    if max(rx.max(), ry.max()) >= MOSAIC_SIDE:
        raise ValueError("a stitched component spans {} pixels: ring linking takes at most 2^16 a side".format(int(max(rx.max(), ry.max())) + 1))
    rings = {}
    for start, ring in _link(rank, rx, ry, d, 17, turns):
        rings.setdefault(int(label[start]), []).append(ring + np.array([x0[rank[start]], y0[rank[start]]]))
    for group_rings in rings.values():
        group_rings.sort(key=_ring_order)
    return rings


def drop_collinear(ring):
    """The ring without the vertices at which it does not turn."""

    ring = np.asarray(ring)
    a, b = ring - np.roll(ring, 1, axis=0), np.roll(ring, -1, axis=0) - ring
    turn = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return ring[turn != 0]


def perimeter(ring):
    ring = np.asarray(ring, dtype=np.float64)
    return float(np.sqrt(((np.roll(ring, -1, axis=0) - ring) ** 2).sum(axis=1)).sum())


def _line_distance(points, a, b):
    ab = b - a
    norm = np.hypot(ab[0], ab[1])
    if norm == 0:
        return np.hypot(points[:, 0] - a[0], points[:, 1] - a[1])
    return np.abs(ab[0] * (points[:, 1] - a[1]) - ab[1] * (points[:, 0] - a[0])) / norm


def simplify_ring(ring, simplify):
    """Collinear vertices dropped, then (simplify > 0) Douglas-Peucker with epsilon = simplify * perimeter of the ring
    (``robosat/features/core.py:123``) in its closed-ring form: the ring is started at its lexicographically smallest vertex
    v0 and split at the vertex farthest from v0 (the first such), and each half is reduced as an open line, keeping a vertex
    where the largest distance to the chord exceeds epsilon.  Returns an open ring, possibly with fewer than 3 vertices."""

    ring = drop_collinear(ring)
    if simplify <= 0 or len(ring) < 3:
        return ring
    ring = _rotate_to_smallest(ring)
    epsilon = simplify * perimeter(ring)
    pts = np.concatenate([ring, ring[:1]]).astype(np.float64)
    n = len(ring)
    far = int(np.argmax(np.hypot(pts[:n, 0] - pts[0, 0], pts[:n, 1] - pts[0, 1])))
    keep = np.zeros(n + 1, dtype=bool)
    keep[[0, far, n]] = True
    stack = [(0, far), (far, n)]
    while stack:
        lo, hi = stack.pop()
        if hi - lo < 2:
            continue
        dist = _line_distance(pts[lo + 1:hi], pts[lo], pts[hi])
        k = int(np.argmax(dist))
        if dist[k] > epsilon:
            mid = lo + 1 + k
            keep[mid] = True
            stack += [(lo, mid), (mid, hi)]
    keep[n] = False
    if far == 0 or not np.hypot(*(pts[far] - pts[0])) > epsilon:  # the whole ring lies within epsilon of one point
        return ring[:1]
    return ring[keep[:n]]


def polygon_is_valid(rings):
    """False where any two segments of the polygon's rings cross properly (their interiors meet in one point).  Plain
    O(n^2) orientation tests, exact for integer vertices."""

    seg_a, seg_b = [], []
    for ring in rings:
        ring = np.asarray(ring, dtype=np.int64)
        seg_a.append(ring)
        seg_b.append(np.roll(ring, -1, axis=0))
    a, b = np.concatenate(seg_a), np.concatenate(seg_b)

    def orient(p, q, r):  # sign of (q - p) x (r - p), broadcast
        return np.sign((q[..., 0] - p[..., 0]) * (r[..., 1] - p[..., 1]) - (q[..., 1] - p[..., 1]) * (r[..., 0] - p[..., 0]))

    for start in range(0, len(a), 256):
        p, q = a[start:start + 256, None, :], b[start:start + 256, None, :]
        r, s = a[None, :, :], b[None, :, :]
        if ((orient(p, q, r) * orient(p, q, s) < 0) & (orient(r, s, p) * orient(r, s, q) < 0)).any():
            return False
    return True


def featurize(edges, table, tiles, shape, simplify=0.01, warn=sys.stderr, iou=None, score=None):
    """Edge rows + component table rows (tile, label, area, ...) of one batch -> GeoJSON features.  ``tiles[i]`` is the
    ``Tile`` of batch index i, ``shape`` = (H, W).  Rings are simplified, checked, reversed to RFC 7946 winding (outer ring
    counter-clockwise, holes clockwise in lon / lat), closed and georeferenced from pixel corners.  Plain GeoJSON Feature
    dicts, ordered by (batch index, label).  ``iou`` (``--dedupe``): {(batch index, label): float}, added as the property
    ``iou``; ``score`` (``--score``): the same keys, added as the property ``score``."""

    h, w = shape
    area = {(int(r[0]), int(r[1])): int(r[2]) for r in np.asarray(table).reshape(-1, 7)}
    features = []
    for (index, label), rings in sorted(link_rings(edges).items()):
        tile = tiles[index]
        outer = simplify_ring(rings[0], simplify)
        if len(outer) < 3:
            print("Warning: simplified feature no longer valid polygon, skipping", file=warn)
            continue
        kept = [outer] + [r for r in (simplify_ring(hole, simplify) for hole in rings[1:]) if len(r) >= 3]
        if simplify > 0 and not polygon_is_valid(kept):
            print("Warning: extracted feature is not valid, skipping", file=warn)
            continue
        coordinates = []
        for ring in kept:
            ring = ring[::-1]  # y points down in the tile and up on the map
            closed = [pixel_to_location(tile, int(px) / w, int(py) / h) for px, py in ring]
            coordinates.append([[lon, lat] for lon, lat in closed + closed[:1]])
        features.append({
            "type": "Feature",
            "geometry": {"type": "Polygon", "coordinates": coordinates},
            "properties": {"tile": [int(tile.x), int(tile.y), int(tile.z)], "area_px": area[(index, label)]},
        })
        if iou is not None:
            features[-1]["properties"]["iou"] = float(iou[(index, label)])
        if score is not None:
            features[-1]["properties"]["score"] = float(score[(index, label)])
    return features


class FeatureWriter:
    """Collects features and writes one FeatureCollection ordered by (z, x, y, label): two runs over the same masks give
    byte-identical files (floats are printed by ``repr``).  The features of a tile arrive in label order from one
    ``featurize`` call, so a stable sort by the tile is that order."""

    def __init__(self):
        self.features = []

    def add(self, features):
        self.features.extend(features)

    def save(self, out):
        def by_tile(feature):
            x, y, z = feature["properties"]["tile"]
            return z, x, y

        collection = {"type": "FeatureCollection", "features": sorted(self.features, key=by_tile)}
        with open(out, "w") as fp:
            json.dump(collection, fp)


# ---- rs features --stitch: the tiles of a zoom level as one sparse raster -------------------------------------------------
NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))  # (dx, dy) of NW N NE W E SW S SE
CALL_PIXELS = (1 << 29) - 1  # the library takes T*H*W < 2^29 per call
CALL_TILES = 65535


def group_clusters(tiles):
    """Tiles -> their 8-connected clusters within each zoom level (the halo crosses diagonals): a list of lists of ``Tile``,
    each sorted by (z, x, y), the clusters ordered by their first tile."""

    todo = {Tile(int(t.x), int(t.y), int(t.z)) for t in tiles}
    clusters = []
    for seed in sorted(todo, key=lambda t: (t.z, t.x, t.y)):
        if seed not in todo:
            continue
        todo.discard(seed)
        cluster, stack = [], [seed]
        while stack:
            t = stack.pop()
            cluster.append(t)
            for dx, dy in NEIGHBOURS:
                n = Tile(t.x + dx, t.y + dy, t.z)
                if n in todo:
                    todo.discard(n)
                    stack.append(n)
        clusters.append(sorted(cluster, key=lambda t: (t.z, t.x, t.y)))
    return clusters


def pack_clusters(clusters, tile_pixels, side=4096, limit=CALL_PIXELS, max_tiles=CALL_TILES):
    """Whole clusters of one zoom level -> calls (lists of tiles sorted by (z, x, y)), greedily in order, never splitting a
    cluster: a call holds at most ``limit`` pixels at ``tile_pixels`` per tile (the padded tile where there is an apron), at
    most ``max_tiles`` tiles, and spans less than 2^31 mosaic pixels (``side`` = the longer tile side).  A single cluster
    beyond that: ValueError."""

    span = ((1 << 31) - 1) // side

    def fits(tiles):
        xs, ys = [t.x for t in tiles], [t.y for t in tiles]
        return (len(tiles) * tile_pixels <= limit and len(tiles) <= max_tiles and max(xs) - min(xs) < span and max(ys) - min(ys) < span
                and len({t.z for t in tiles}) == 1)

    calls, current = [], []
    for cluster in clusters:
        if not fits(cluster):
            raise ValueError("a cluster of {} connected tiles ({} pixels each) around {}/{}/{} exceeds one device call ({} pixels, {} "
                             "tiles) and cannot be split".format(len(cluster), tile_pixels, cluster[0].z, cluster[0].x, cluster[0].y, limit,
                                                                 max_tiles))
        if current and not fits(current + cluster):
            calls.append(current)
            current = []
        current = current + cluster
    if current:
        calls.append(current)
    return [sorted(call, key=lambda t: (t.z, t.x, t.y)) for call in calls]


def stitch_tables(tiles, shape):
    """The tiles of one call, sorted by (z, x, y) (a tile's slot is its position) -> (nbr int32 [T, 8]: the slot of each
    neighbour in ``NEIGHBOURS`` order or -1; origin int32 [T, 2]: the tile's (X, Y) in mosaic pixels from the call's smallest x
    and y; (x_min, y_min) in tiles)."""

    h, w = shape
    assert list(tiles) == sorted(tiles, key=lambda t: (t.z, t.x, t.y)) and len({t.z for t in tiles}) == 1, "one zoom level, sorted"
    slot = {(t.x, t.y): i for i, t in enumerate(tiles)}
    assert len(slot) == len(tiles), "duplicate tiles"
    x_min, y_min = min(t.x for t in tiles), min(t.y for t in tiles)
    nbr = np.array([[slot.get((t.x + dx, t.y + dy), -1) for dx, dy in NEIGHBOURS] for t in tiles], dtype=np.int32).reshape(-1, 8)
    origin = np.array([[(t.x - x_min) * w, (t.y - y_min) * h] for t in tiles], dtype=np.int64).reshape(-1, 2)
    assert origin.max() + max(h, w) < 1 << 31, "the call spans 2^31 mosaic pixels"
    return nbr, origin.astype(np.int32), (x_min, y_min)


def mosaic_location(z, gx, gy, shape):
    """``(lon, lat)`` of the pixel corner (gx, gy) of zoom level z's whole raster (gx = tile x * W + pixel x), through the tile it
    falls in: ``pixel_to_location`` there, except that a corner on the tile's east / south edge takes that edge's own
    longitude / latitude.  A tile's east edge is computed as its neighbour's west edge is, so a vertex on a seam gets the same
    floats from either tile."""

    h, w = shape
    last = (1 << z) - 1
    tile = Tile(min(gx // w, last), min(gy // h, last), z)
    return tile_vertex_location(tile, gx - tile.x * w, gy - tile.y * h, shape)


def tile_vertex_location(tile, px, py, shape):
    h, w = shape
    west, south, east, north = tile_bounds(tile)
    lon, lat = pixel_to_location(tile, px / w, py / h)
    return east if px == w else lon, south if py == h else lat


def featurize_stitched(edges, table, tiles, shape, simplify=0.01, warn=sys.stderr, georeference=True, iou=None, score=None):
    """``featurize`` for one stitched call: edge rows (label, X, Y, dir) + table rows (label, area, X0, Y0, X1, Y1) in
    mosaic pixels, ``tiles`` the call's tiles in slot order.  A feature's ``tile`` is the tile holding its canonical pixel (the
    one its label names: label - 1 = slot * H * W + y * W + x), ``area_px`` the area of the whole component; features come in
    label order, which is (slot, label).  ``georeference=False`` leaves the vertices as mosaic pixel corners [X, Y].  ``iou``
    (``--dedupe``): {label: float}, added as the property ``iou``; ``score`` (``--score``): the same keys, the property ``score``."""

    h, w = shape
    x_min, y_min = min(t.x for t in tiles), min(t.y for t in tiles)
    area = {int(r[0]): int(r[1]) for r in np.asarray(table).reshape(-1, 6)}
    features = []
    for label, rings in sorted(link_rings_mosaic(edges).items()):
        tile = tiles[(label - 1) // (h * w)]
        outer = simplify_ring(rings[0], simplify)
        if len(outer) < 3:
            print("Warning: simplified feature no longer valid polygon, skipping", file=warn)
            continue
        kept = [outer] + [r for r in (simplify_ring(hole, simplify) for hole in rings[1:]) if len(r) >= 3]
        if simplify > 0 and not polygon_is_valid(kept):
            print("Warning: extracted feature is not valid, skipping", file=warn)
            continue
        coordinates = []
        for ring in kept:
            ring = ring[::-1]  # y points down in the raster and up on the map
            if georeference:
                closed = [list(mosaic_location(tile.z, x_min * w + int(px), y_min * h + int(py), shape)) for px, py in ring]
            else:
                closed = [[int(px), int(py)] for px, py in ring]
            coordinates.append(closed + closed[:1])
        features.append({
            "type": "Feature",
            "geometry": {"type": "Polygon", "coordinates": coordinates},
            "properties": {"tile": [int(tile.x), int(tile.y), int(tile.z)], "area_px": area[label], "stitched": True},
        })
        if iou is not None:
            features[-1]["properties"]["iou"] = float(iou[label])
        if score is not None:
            features[-1]["properties"]["score"] = float(score[label])
    return features


# ---- rs features --dedupe: which predicted components the reference labels already map ---------------------------------------
def dedupe_keep(table, ref_table, pairs, threshold):
    """``robosat/tools/dedupe.py`` restated on rasters.  ``table``: rows of the predicted components, ``ref_table``: of the
    reference's, both per tile (rows of 7: tile, label, area, ...) or both stitched (rows of 6: label, area, ...); ``pairs``: the
    overlap table, rows (raster, label of the predicted, label of the reference, shared pixels), raster = the tile, or 0 for
    stitched tables.  For a predicted component P, N(P) = the reference components that share a pixel with it,
    inter = the pixels it shares with them and union = area(P) + sum of area(Q) over N(P) - inter.  P is kept iff N(P) is
    empty (IoU 0.0) or ``inter < threshold * union`` (Python floats; strict, as the reference's ``iou(...) < threshold``).
    Returns (keep bool [N], iou float64 [N]) in the order of ``table``'s rows."""

    table, ref_table = np.asarray(table), np.asarray(ref_table)
    if table.ndim != 2 or table.shape[1] not in (6, 7) or ref_table.ndim != 2 or ref_table.shape[1] != table.shape[1]:
        raise ValueError("tables are [N, 7] (per tile) or [N, 6] (stitched), both alike; got {} and {}".format(table.shape, ref_table.shape))
    per_tile = table.shape[1] == 7

    def keys(raster, label):  # (tiles per call <= 65535, labels < 2^29)
        return np.asarray(raster, dtype=np.int64) << 31 | np.asarray(label, dtype=np.int64)

    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 4)
    keep = np.ones(len(table), dtype=bool)
    iou = np.zeros(len(table), dtype=np.float64)
    if len(pairs) == 0 or len(table) == 0:
        return keep, iou
    # the reference's areas are looked up for the pairs alone: unopened reference masks can hold tens of thousands of components
    ref_key = keys(ref_table[:, 0], ref_table[:, 1]) if per_tile else keys(0, ref_table[:, 0])
    order = np.argsort(ref_key, kind="stable")
    at = np.searchsorted(ref_key[order], keys(pairs[:, 0], pairs[:, 2]))
    if len(order) == 0 or at.max() >= len(order) or (ref_key[order][at] != keys(pairs[:, 0], pairs[:, 2])).any():
        raise ValueError("a pair names a reference component that is not in ref_table")
    ref_area = ref_table[:, 2 if per_tile else 1].astype(np.int64)[order][at]
    touched, group = np.unique(keys(pairs[:, 0], pairs[:, 1]), return_inverse=True)
    inter, others = np.zeros(len(touched), dtype=np.int64), np.zeros(len(touched), dtype=np.int64)
    np.add.at(inter, group.reshape(-1), pairs[:, 3])
    np.add.at(others, group.reshape(-1), ref_area)
    own = keys(table[:, 0], table[:, 1]) if per_tile else keys(0, table[:, 0])
    hit = np.minimum(np.searchsorted(touched, own), len(touched) - 1)
    area = table[:, 2 if per_tile else 1].tolist()
    for i in np.nonzero(touched[hit] == own)[0].tolist():  # (plain Python numbers from here: the rule as it is written)
        shared = int(inter[hit[i]])
        union = area[i] + int(others[hit[i]]) - shared
        keep[i] = shared < float(threshold) * union
        iou[i] = shared / union
    return keep, iou


# ---- rs features --score: a polygon's confidence from the sums of its pixels' probability bytes ---------------------------------
def scores_from_sums(sums, areas, weights=None):
    """``sums`` int [N, K] (``ops.component_scores``: per component and model, the sum of the quantised probability bytes over its
    pixels), ``areas`` int [N] (the component table's) and K weights (unset: all 1) -> float64 [N]:
    ``sum_k w_k * sums[c][k] / (255 * area_c * sum_k w_k)`` in Python floats -- the mean over the component's pixels of the
    probability ``rs masks`` votes with, ``np.average(linspace(0, 1, 256)[q], axis=0, weights=w)``."""

    sums = np.asarray(sums)
    if sums.ndim != 2 or sums.shape[1] < 1:
        raise ValueError("sums are [N, K] with K >= 1, got {}".format(sums.shape))
    areas = np.asarray(areas).reshape(-1)
    if len(areas) != len(sums):
        raise ValueError("{} areas for {} rows of sums".format(len(areas), len(sums)))
    weights = [1.0] * sums.shape[1] if weights is None else [float(w) for w in weights]
    if len(weights) != sums.shape[1]:
        raise ValueError("{} weights for {} models".format(len(weights), sums.shape[1]))
    total = sum(weights)
    if not (all(0 <= w < float("inf") for w in weights) and total > 0):
        raise ValueError("weights are finite, not negative and not all 0, got {}".format(weights))
    if len(areas) and int(areas.min()) < 1:
        raise ValueError("a component has at least one pixel, got an area of {}".format(int(areas.min())))
    out = np.zeros(len(sums), dtype=np.float64)
    for i, (row, area) in enumerate(zip(sums.tolist(), areas.tolist())):  # (plain Python numbers: the formula as it is written)
        out[i] = sum(w * n for w, n in zip(weights, row)) / (255 * area * total)
    return out


# ---- rs features --geometry centerline: skeleton links -> lines ----------------------------------------------------------------
# A link row is (tile, label, x, y, dir): skeleton pixel (x, y) joined to (x + 1, y) for dir 0 (E), (x + 1, y + 1) for 1 (SE),
# (x, y + 1) for 2 (S), (x - 1, y + 1) for 3 (SW); dir -1 is a skeleton pixel without links.  Vertices are PIXELS (their centres
# on the map), unlike the polygon half's corners.  A line is (tile, label, points int64 [k, 2]); it is closed where k > 1 and
# its first point is its last.
_LINK_STEP = ((1, 0), (1, 1), (0, 1), (-1, 1))


def _link_key(a, b):
    return (a, b) if a < b else (b, a)


def link_lines(rows):
    """Link rows int [N, 5] (or [N, 4] = (label, X, Y, dir) of a stitched call, taken as tile 0) in any order -> the lines of the
    link graph, a list of (tile, label, points).  The degree of a pixel is the number of its links; pixels of degree != 2 are
    nodes.  A line is a maximal chain of links whose interior pixels have degree 2: it runs from node to node (back to the same
    node for a loop hanging on a junction), or it is a node-free cycle, closed, started at its lexicographically smallest (x, y)
    and walked towards the smaller of that pixel's two neighbours.  A pixel without links is a line of one point.  The output is
    canonical whatever the order of the rows: every line is the smaller of its two readings (an open line starts at its smaller
    end), and the lines are sorted by (tile, points).  A line's label is the smallest label among its links' rows."""

    r = np.asarray(rows, dtype=np.int64)
    if r.ndim == 2 and r.shape[1] == 4:
        r = np.concatenate([np.zeros((len(r), 1), dtype=np.int64), r], axis=1)
    r = r.reshape(-1, 5)
    by_tile = {}
    for tile, label, x, y, d in r.tolist():
        adj, labels, lone = by_tile.setdefault(tile, ({}, {}, {}))
        a = (x, y)
        if d < 0:
            lone[a] = label
            continue
        assert d <= 3, "dir is -1..3"
        b = (x + _LINK_STEP[d][0], y + _LINK_STEP[d][1])
        key = _link_key(a, b)
        assert key not in labels, "duplicate link"
        labels[key] = label
        adj.setdefault(a, set()).add(b)
        adj.setdefault(b, set()).add(a)

    lines = []
    for tile in sorted(by_tile):
        adj, labels, lone = by_tile[tile]
        used = set()

        def walk(a, b, stop):
            points = [a, b]
            used.add(_link_key(a, b))
            while b != stop and len(adj[b]) == 2:
                first, second = adj[b]
                nxt = second if first == points[-2] else first
                used.add(_link_key(b, nxt))
                points.append(nxt)
                b = nxt
            return points

        found = [[p] for p in lone if p not in adj]
        for a in sorted(p for p in adj if len(adj[p]) != 2):
            for b in sorted(adj[a]):
                if _link_key(a, b) not in used:
                    points = walk(a, b, None)
                    found.append(min(points, points[::-1]))
        for a in sorted(adj):  # what is left: cycles without a node
            b = min(adj[a])
            if _link_key(a, b) not in used:
                found.append(walk(a, b, a))
        for points in sorted(found):
            if len(points) == 1:
                label = lone[points[0]]
            else:
                label = min(labels[_link_key(a, b)] for a, b in zip(points, points[1:]))
            lines.append((tile, label, np.array(points, dtype=np.int64).reshape(-1, 2)))
    return lines


def line_length(points):
    """Length in pixels: a link counts 1 or sqrt(2)."""

    d = np.diff(np.asarray(points, dtype=np.int64), axis=0)
    return float(np.hypot(d[:, 0], d[:, 1]).sum())


def _line_rows(lines):
    """Lines -> the link rows they came from (each link under its line's label)."""

    step = {s: d for d, s in enumerate(_LINK_STEP)}
    rows = []
    for tile, label, points in lines:
        points = np.asarray(points).tolist()
        if len(points) == 1:
            rows.append((tile, label, points[0][0], points[0][1], -1))
        for (ax, ay), (bx, by) in zip(points, points[1:]):
            if (bx - ax, by - ay) not in step:
                ax, ay, bx, by = bx, by, ax, ay
            rows.append((tile, label, ax, ay, step[(bx - ax, by - ay)]))
    return np.array(rows, dtype=np.int64).reshape(-1, 5)


def prune_lines(lines, prune):
    """Removes spurs from the lines of ``link_lines``.  A spur is an open line from an end of degree 1 to a junction (a pixel
    where three or more line ends meet) whose length (``line_length``) is below ``prune``.  Removal goes in rounds.  In a round
    every junction drops its spurs, shortest first (ties in the lines' canonical order), but keeps at least two of its line
    ends; then the remaining links are linked afresh (``link_lines``: two lines left at a former junction become one), and the
    next round looks at the new lines, until a round finds nothing to remove.  A line between two ends of degree 1, a line between
    two junctions and a cycle are never spurs, and a junction never loses all its lines: no component vanishes or falls apart.
    The result depends on the set of links alone, pruning it again changes nothing, and ``prune`` = 0 returns the lines as they
    are."""

    lines = list(lines)
    while prune > 0:
        ends = {}
        for tile, _, points in lines:
            if len(points) > 1:
                for p in (points[0], points[-1]):
                    key = (tile, int(p[0]), int(p[1]))
                    ends[key] = ends.get(key, 0) + 1
        spurs = {}
        for i, (tile, _, points) in enumerate(lines):
            if len(points) < 2:
                continue
            a, b = (tile, int(points[0][0]), int(points[0][1])), (tile, int(points[-1][0]), int(points[-1][1]))
            if a == b:
                continue
            for end, junction in ((a, b), (b, a)):
                if ends[end] == 1 and ends[junction] >= 3:
                    length = line_length(points)
                    if length < prune:
                        spurs.setdefault(junction, []).append((length, points.tolist(), i))
        drop = set()
        for junction, candidates in spurs.items():
            candidates.sort()
            drop.update(i for _, _, i in candidates[:ends[junction] - 2])
        if not drop:
            break
        lines = link_lines(_line_rows([line for i, line in enumerate(lines) if i not in drop]))
    return lines


def simplify_line(points, tolerance):
    """Douglas-Peucker on a polyline [[x, y], ...] with ``tolerance`` in pixels: between two kept vertices the vertex farthest from
    their chord is kept where that distance exceeds the tolerance.  Both ends are kept; a closed line (first point = last) keeps
    its start vertex, the distance to the zero-length chord being the distance to that point.  Tolerance 0 drops only vertices
    that lie on the chord of their kept neighbours."""

    points = np.asarray(points)
    n = len(points)
    if n < 3:
        return points
    pts = points.astype(np.float64)
    keep = np.zeros(n, dtype=bool)
    keep[[0, n - 1]] = True
    stack = [(0, n - 1)]
    while stack:
        lo, hi = stack.pop()
        if hi - lo < 2:
            continue
        dist = _line_distance(pts[lo + 1:hi], pts[lo], pts[hi])
        k = int(np.argmax(dist))
        if dist[k] > tolerance:
            mid = lo + 1 + k
            keep[mid] = True
            stack += [(lo, mid), (mid, hi)]
    return points[keep]


def line_width(d2_values, radius):
    """The width properties of one line from the capped squared distances (``ops.distance_transform`` with ``radius``) at the pixels
    of its chain, after pruning and before simplification.  The width at a pixel is ``2 * sqrt(d2) - 1``: the pixel itself plus what
    lies either side of it up to the nearest non-road pixel.  ``width_px`` is the median over the chain (junction pixels read wide,
    spur stubs narrow), ``width_min_px`` / ``width_max_px`` the extremes, all rounded to 3 decimals; ``width_capped`` is True where
    any pixel sits at ``radius^2`` (no non-road pixel within reach: the true width is larger), and absent otherwise.  The estimator is
    biased, knowingly: an axis-parallel road of odd width w gives exactly w, one of even width w - 1, its skeleton running on one of
    the two middle rows."""

    d2 = np.asarray(d2_values, dtype=np.int64).reshape(-1)
    if len(d2) == 0 or d2.min() < 0 or d2.max() > radius * radius:
        raise ValueError("a line has at least one pixel and its squared distances lie in 0..{}".format(radius * radius))
    width = 2.0 * np.sqrt(d2.astype(np.float64)) - 1.0
    properties = {"width_px": round(float(np.median(width)), 3), "width_min_px": round(float(width.min()), 3),
                  "width_max_px": round(float(width.max()), 3)}
    if (d2 == radius * radius).any():
        properties["width_capped"] = True
    return properties


EARTH_RADIUS = 6378137.0  # metres, the sphere of the web mercator


def ground_resolution(lat, z, width):
    """Metres per pixel at latitude ``lat`` (degrees) in a zoom level ``z`` of tiles ``width`` pixels wide."""

    return 2.0 * math.pi * EARTH_RADIUS * math.cos(math.radians(lat)) / (2 ** z * width)


class Widths:
    """The ``widths=`` of ``centerlines`` / ``centerlines_stitched``: ``sample(coords)`` takes int32 [N, 3] rows (slot, y, x) and
    returns the N values of the batch's or call's distance transform there (one call per batch: two small transfers, no raster
    comes back); ``radius`` is the transform's."""

    def __init__(self, sample, radius):
        self.sample, self.radius = sample, int(radius)

    def of_lines(self, coords, lengths):
        """Rows (slot, y, x) of all lines' chains, concatenated -> one ``line_width`` dict per line."""

        values = np.asarray(self.sample(np.ascontiguousarray(coords, dtype=np.int32)), dtype=np.int64).reshape(-1)
        assert len(values) == len(coords) == sum(lengths), "one value per chain pixel"
        ends = np.cumsum(lengths)
        return [line_width(values[end - n:end], self.radius) for n, end in zip(lengths, ends)]


def _line_feature(tile, label, points, locate, area, prune_length, tolerance, stitched):
    kept = simplify_line(points, tolerance)
    coordinates = [list(locate(int(px), int(py))) for px, py in kept]
    if len(coordinates) == 1:  # a skeleton of one pixel: a LineString takes two positions
        coordinates = coordinates * 2
    properties = {"tile": [int(tile.x), int(tile.y), int(tile.z)], "component": int(label), "length_px": round(prune_length, 3),
                  "area_px": area}
    if stitched:
        properties["stitched"] = True
    return {"type": "Feature", "geometry": {"type": "LineString", "coordinates": coordinates}, "properties": properties}


def _add_widths(feature, width, lat, z, tile_width):
    """``line_width``'s properties and ``width_m`` = ``width_px`` times the ground resolution at ``lat``, the latitude of the centre
    of the chain's middle pixel (index len // 2)."""

    feature["properties"].update(width)
    feature["properties"]["width_m"] = width["width_px"] * ground_resolution(lat, z, tile_width)


def centerlines(links, table, tiles, shape, prune=20, tolerance=1.5, widths=None):
    """Link rows (tile, label, x, y, dir) + component table rows (tile, label, area, ...) of one batch -> one GeoJSON Feature per
    line (``link_lines``, ``prune_lines``, ``simplify_line``): a LineString whose vertices are PIXEL CENTRES (x + 0.5, y + 0.5)
    georeferenced in their tile; properties ``tile``, ``component`` (the label), ``length_px`` (before simplification) and
    ``area_px`` (of the component).  Ordered by (batch index, points).  ``widths`` (``--width``): a ``Widths`` over the batch's
    distance transform; every feature gains ``line_width``'s properties and ``width_m``."""

    h, w = shape
    area = {(int(r[0]), int(r[1])): int(r[2]) for r in np.asarray(table).reshape(-1, 7)}
    lines = prune_lines(link_lines(np.asarray(links).reshape(-1, 5)), prune)
    features = []
    for index, label, points in lines:
        tile = tiles[index]

        def locate(px, py, tile=tile):
            return pixel_to_location(tile, (px + 0.5) / w, (py + 0.5) / h)

        features.append(_line_feature(tile, label, points, locate, area[(index, label)], line_length(points), tolerance, False))
    if widths is not None and lines:
        coords = np.concatenate([np.stack([np.full(len(p), index), p[:, 1], p[:, 0]], axis=1) for index, _, p in lines])
        for feature, (index, _, points), width in zip(features, lines, widths.of_lines(coords, [len(p) for _, _, p in lines])):
            px, py = points[len(points) // 2]
            lat = pixel_to_location(tiles[index], (int(px) + 0.5) / w, (int(py) + 0.5) / h)[1]
            _add_widths(feature, width, lat, tiles[index].z, w)
    return features


def mosaic_centre_location(z, gx, gy, shape):
    """``(lon, lat)`` of the centre of pixel (gx, gy) of zoom level z's whole raster, through the tile it falls in (present or not):
    the floats ``centerlines`` gives the same pixel from that tile's side."""

    h, w = shape
    tile = Tile(gx // w, gy // h, z)
    return pixel_to_location(tile, (gx - tile.x * w + 0.5) / w, (gy - tile.y * h + 0.5) / h)


def mosaic_slots(tiles, points, shape):
    """Mosaic pixels int [N, 2] = (X, Y) of one stitched call -> int64 [N, 3] rows (slot, y, x) through the call's tiles (in slot
    order); a pixel that no tile of the call covers: ValueError."""

    h, w = shape
    points = np.asarray(points, dtype=np.int64).reshape(-1, 2)
    x_min, y_min = min(t.x for t in tiles), min(t.y for t in tiles)
    nx, ny = max(t.x for t in tiles) - x_min + 1, max(t.y for t in tiles) - y_min + 1
    slots = np.full(nx * ny, -1, dtype=np.int64)
    slots[[(t.y - y_min) * nx + (t.x - x_min) for t in tiles]] = np.arange(len(tiles))
    tx, ty = points[:, 0] // w, points[:, 1] // h
    if len(points) and (tx.min() < 0 or ty.min() < 0 or tx.max() >= nx or ty.max() >= ny or (slots[ty * nx + tx] < 0).any()):
        raise ValueError("a mosaic pixel outside the tiles of the call")
    return np.stack([slots[ty * nx + tx], points[:, 1] - ty * h, points[:, 0] - tx * w], axis=1)


def centerlines_stitched(links, table, tiles, shape, prune=20, tolerance=1.5, georeference=True, widths=None):
    """``centerlines`` for one stitched call: link rows (label, X, Y, dir) + table rows (label, area, ...) in mosaic pixels,
    ``tiles`` the call's tiles in slot order.  A feature's ``tile`` is the tile holding its component's canonical pixel,
    ``"stitched": true`` marks it; ordered by (label, points).  ``georeference=False`` leaves the vertices as mosaic pixels
    [X, Y].  ``widths``: as in ``centerlines``, over the call's distance transform (a chain's mosaic pixels go through
    ``mosaic_slots``)."""

    h, w = shape
    x_min, y_min = min(t.x for t in tiles), min(t.y for t in tiles)
    z = tiles[0].z
    area = {int(r[0]): int(r[1]) for r in np.asarray(table).reshape(-1, 6)}

    def locate(px, py):
        return mosaic_centre_location(z, x_min * w + px, y_min * h + py, shape) if georeference else (px, py)

    lines = sorted(prune_lines(link_lines(np.asarray(links).reshape(-1, 4)), prune), key=lambda line: (line[1], line[2].tolist()))
    features = []
    for _, label, points in lines:
        tile = tiles[(label - 1) // (h * w)]
        features.append(_line_feature(tile, label, points, locate, area[label], line_length(points), tolerance, True))
    if widths is not None and lines:
        coords = mosaic_slots(tiles, np.concatenate([p for _, _, p in lines]), shape)
        for feature, (_, _, points), width in zip(features, lines, widths.of_lines(coords, [len(p) for _, _, p in lines])):
            px, py = points[len(points) // 2]
            lat = mosaic_centre_location(z, x_min * w + int(px), y_min * h + int(py), shape)[1]
            _add_widths(feature, width, lat, z, w)
    return features
