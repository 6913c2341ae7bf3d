"""What the ``rs features --stitch`` tests share: a tile grid pasted into one zero canvas, on which the per-tile restatements of
``features_ref`` ARE the stitched definitions (include/robosat_hip.h).  Not a test module.

The canvas has a margin on every side, so the restatement's own border rule (erode reads outside as 1) cannot reach the content:
``margin(eps_open, eps_close)`` = 2 * (eps_open + eps_close) + 2.  Slots follow the host's order: tiles sorted by (x, y)."""

import numpy as np

import features_ref as R


def margin(eps_open=0, eps_close=0):
    return 2 * (eps_open + eps_close) + 2


class Grid:
    """``tiles``: {(tx, ty): array [H, W]} of the PRESENT tiles (any integer tile coordinates)."""

    def __init__(self, tiles, pad):
        self.coords = sorted(tiles)  # slot order: x, then y
        self.h, self.w = tiles[self.coords[0]].shape
        self.pad = pad
        self.x_min, self.y_min = min(x for x, _ in self.coords), min(y for _, y in self.coords)
        self.nx, self.ny = max(x for x, _ in self.coords) - self.x_min + 1, max(y for _, y in self.coords) - self.y_min + 1
        self.stack = np.stack([tiles[c] for c in self.coords])
        self.canvas = self.paste(self.stack)
        # global index slot * H * W + y * W + x of every canvas pixel, -1 where no tile is
        index = np.arange(len(self.coords) * self.h * self.w, dtype=np.int64).reshape(len(self.coords), self.h, self.w)
        self.index = self.paste(index, fill=-1)

    def corner(self, slot):
        """Canvas (row, column) of the tile's first pixel."""
        tx, ty = self.coords[slot]
        return self.pad + (ty - self.y_min) * self.h, self.pad + (tx - self.x_min) * self.w

    def paste(self, stack, fill=0):
        out = np.full((self.ny * self.h + 2 * self.pad, self.nx * self.w + 2 * self.pad), fill, dtype=np.asarray(stack).dtype)
        for slot, plane in enumerate(stack):
            r, c = self.corner(slot)
            out[r:r + self.h, c:c + self.w] = plane
        return out

    def cut(self, canvas, apron=0):
        """The tiles' planes of a canvas-sized array, with ``apron`` more pixels on every side."""
        planes = []
        for slot in range(len(self.coords)):
            r, c = self.corner(slot)
            planes.append(canvas[r - apron:r + self.h + apron, c - apron:c + self.w + apron])
        return np.stack(planes)

    def tables(self):
        """(nbr int32 [T, 8] in the order NW N NE W E SW S SE, origin int32 [T, 2]) written out independently of the host code."""
        slot = {c: i for i, c in enumerate(self.coords)}
        order = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
        nbr = np.array([[slot.get((x + dx, y + dy), -1) for dx, dy in order] for x, y in self.coords], dtype=np.int32)
        origin = np.array([[(x - self.x_min) * self.w, (y - self.y_min) * self.h] for x, y in self.coords], dtype=np.int32)
        return nbr, origin

    def global_labels(self, mask_canvas):
        """Canvas labels by the stitched rule: the restated 4-connected components, each named 1 + its smallest global index."""
        ref = R.label(mask_canvas)
        out = np.zeros(ref.shape, dtype=np.int32)
        fg = ref != 0
        assert (self.index[fg] >= 0).all(), "foreground outside the tiles"
        if fg.any():
            smallest = np.full(int(ref.max()) + 1, np.iinfo(np.int64).max)
            np.minimum.at(smallest, ref[fg], self.index[fg])
            out[fg] = smallest[ref[fg]] + 1
        return out

    def table(self, labels_canvas, min_area=0):
        """Rows (label, area, X0, Y0, X1, Y1) in mosaic pixels, sorted by label."""
        rows = R.table(labels_canvas, min_area)[:, 1:].astype(np.int64)
        rows[:, 2:] -= self.pad
        return rows

    def edges(self, labels_canvas):
        """Sorted rows (label, X, Y, dir) in mosaic pixels."""
        rows = R.edges(labels_canvas)[:, 1:].astype(np.int64)
        rows[:, 1:3] -= self.pad
        return R.sort_rows(rows)


def split(image, h, w, absent=(), x0=0, y0=0):
    """An image cut into h x w tiles -> {(tx, ty): tile}, without the ``absent`` (column, row) positions."""

    rows, cols = image.shape[0] // h, image.shape[1] // w
    assert rows * h == image.shape[0] and cols * w == image.shape[1]
    return {(x0 + c, y0 + r): np.ascontiguousarray(image[r * h:(r + 1) * h, c * w:(c + 1) * w])
            for r in range(rows) for c in range(cols) if (c, r) not in absent}
