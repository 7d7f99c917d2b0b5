"""Shared by tests/test_region_cpu.py and tests/test_gpu_region.py: the
geometries of tests/test_gpu_reader.py restated, and the regions and frame
ranges a region read is checked with.  TEST INFRASTRUCTURE ONLY."""
from oracle_bindings import CHANNEL, SPACE, TIME

GEOMETRIES = {
    # the 16-byte path; a non-identity shard order
    "aligned": [(TIME, 0, 2, 1), (SPACE, 64, 32, 1), (SPACE, 64, 32, 2)],
    # ragged tiles in y and x
    "ragged": [(TIME, 0, 3, 1), (SPACE, 45, 16, 2), (SPACE, 70, 32, 1)],
    # unaligned chunk rows
    "odd": [(TIME, 0, 2, 1), (SPACE, 17, 17, 1), (SPACE, 33, 33, 1)],
    # tile_group_offset and chunk_internal_offset both vary inside a layer; ragged c and z
    "5d": [(TIME, 0, 2, 1), (CHANNEL, 3, 2, 1), (SPACE, 5, 2, 2), (SPACE, 20, 8, 1),
           (SPACE, 24, 16, 1)],
    # tiles taller than one 64-row slab of the kernel's walk, the last slab cut twice
    "tall": [(TIME, 0, 1, 1), (SPACE, 150, 100, 1), (SPACE, 40, 24, 1)],
    # three tile rows of two slabs: rows 60-70 of tile row 1 exist, and a region over
    # all three rows walks a whole interior tile row
    "taller": [(TIME, 0, 1, 1), (SPACE, 250, 100, 1), (SPACE, 40, 24, 1)],
}
PERMUTED = (GEOMETRIES["5d"], [0, 2, 1, 3, 4])     # the frame-permuting storage order
XY_SHAPES = [(64, 64, 32, 32), (45, 70, 16, 32)]  # H, W, th, tw in acquisition orientation
SLAB = 64                                         # rows of a tile one work item moves


def xy_dims(shape):
    H, W, th, tw = shape
    return [(TIME, 0, 2, 1), (CHANNEL, 2, 1, 1), (SPACE, H, th, 1), (SPACE, W, tw, 1)]


XY_ORDER = [0, 1, 3, 2]


def _odd_below(v):
    if v < 3:
        return 1
    return v - 1 if (v - 1) % 2 else v - 2


def regions_of(dims, tall_rows_along="y"):
    """{name: (x0, y0, width, height)} for frames of dims[-2] x dims[-1] pixels in
    tiles of the dims' chunk sizes, all in the orientation of the frames handed
    back.  tall_rows_along: the axis the storage rows run along ("y", or "x" for an
    XY-swapped storage order): tiles longer than a slab on it add the slab cases."""
    H, th = dims[-2][1], dims[-2][2]
    W, tw = dims[-1][1], dims[-1][2]
    ntx, nty = -(-W // tw), -(-H // th)
    out = {
        "whole": (0, 0, W, H),
        "first-pixel": (0, 0, 1, 1),
        "last-pixel": (W - 1, H - 1, 1, 1),
        "inside-a-tile": (1, 1, max(min(tw, W) - 2, 1), max(min(th, H) - 2, 1)),
        "row": (0, H // 2, W, 1),
        "column": (W // 2, 0, 1, H),
        "last-tile": ((ntx - 1) * tw, (nty - 1) * th, W - (ntx - 1) * tw, H - (nty - 1) * th),
    }
    # the four-tile corner at (tw, th): odd origin, odd width and height
    x0, y0 = min(_odd_below(tw), _odd_below(W)), min(_odd_below(th), _odd_below(H))
    w, h = 5, 7
    while w > 1 and x0 + w > W:
        w -= 2
    while h > 1 and y0 + h > H:
        h -= 2
    out["corner"] = (x0, y0, w, h)
    n, t = (H, th) if tall_rows_along == "y" else (W, tw)
    if t > SLAB:
        other = W if tall_rows_along == "y" else H
        o0 = 3 if other > 3 else 0
        on = min(other - o0, 9)

        def rows(name, r0, nr):
            if r0 + nr <= n:
                out[name] = (o0, r0, on, nr) if tall_rows_along == "y" else (r0, o0, nr, on)

        rows("rows-60-70", 60, 11)                      # they cross a slab boundary
        if n > t + 70:
            rows("rows-60-70-of-tile-1", t + 60, 11)
        cut0 = (t - 1) // SLAB * SLAB
        rows("cut-last-slab", cut0 + 1, min(t, n) - cut0 - 1)
        rows("last-rows", n - 3, 3)
    return out


def frame_ranges(F):
    """the whole layer, a single middle frame, the last frame"""
    return sorted({(0, F), (F // 2, 1), (F - 1, 1)})
