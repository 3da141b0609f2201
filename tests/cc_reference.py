"""Connected components restated in plain numpy / Python (what tests/test_gpu_cc.py holds include/pea_cc.h to, and what
tests/test_cc_host.py holds to scipy.ndimage.label and to hand-written expectations), and the table of named cases that both files use.

The rule is written down directly: walk the pixels in flat order; an unlabelled non-zero pixel is the FIRST pixel of a new component,
which gets the next number and is filled by an iterative flood fill over the explicit neighbour list of (ndim, connectivity), joining
neighbours of the same value.  Then the sizes, min_size (a component of fewer pixels is dropped) and the renumbering 1 .. n_kept in the
order of the first pixels.

Case sizing.  The kernel's tile is 32 x 32 pixels of one plane (csrc/pea_k_cc.hip: kTile) and its flat passes take 1024 pixels per
workgroup and 256 per wave.  The 2D cases are 70 x 150 (3 x 5 tiles, remainders 6 and 22, 10.3 flat runs), the 3D cases 5 x 37 x 70
(2 x 3 tiles per plane, remainders 5 and 6): at least two whole tiles and a ragged one along every tiled axis."""
import functools

import numpy as np

N2_1 = [(-1, 0), (0, -1), (0, 1), (1, 0)]
N2_2 = N2_1 + [(-1, -1), (-1, 1), (1, -1), (1, 1)]
N3_1 = [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0)]
N3_2 = N3_1 + [(-1, -1, 0), (-1, 1, 0), (-1, 0, -1), (-1, 0, 1), (0, -1, -1), (0, -1, 1), (0, 1, -1), (0, 1, 1), (1, -1, 0), (1, 1, 0),
               (1, 0, -1), (1, 0, 1)]
N3_3 = N3_2 + [(-1, -1, -1), (-1, -1, 1), (-1, 1, -1), (-1, 1, 1), (1, -1, -1), (1, -1, 1), (1, 1, -1), (1, 1, 1)]
NEIGHBOURS = {(2, 1): N2_1, (2, 2): N2_2, (3, 1): N3_1, (3, 2): N3_2, (3, 3): N3_3}
assert [len(NEIGHBOURS[k]) for k in sorted(NEIGHBOURS)] == [4, 8, 6, 18, 26]
assert all(len(set(v)) == len(v) and all(tuple(-c for c in o) in v for o in v) for v in NEIGHBOURS.values())

H2, W2 = 70, 150
Z3, H3, W3 = 5, 37, 70


def cc_reference(x, connectivity, min_size=0):
    """one image [Y, X] or [Z, Y, X] of any integer / bool dtype -> (labels int32 of x's shape, (found, kept))"""
    x = np.asarray(x)
    offs = NEIGHBOURS[(x.ndim, connectivity)]
    pad = np.zeros(tuple(s + 2 for s in x.shape), np.int64)
    pad[tuple(slice(1, -1) for _ in x.shape)] = x
    strides = [int(np.prod(pad.shape[a + 1:])) for a in range(x.ndim)]
    deltas = [sum(o * s for o, s in zip(off, strides)) for off in offs]
    val = pad.ravel().tolist()
    lab = [0] * len(val)
    sizes = [0]
    for p in np.flatnonzero(pad.ravel()).tolist():  # increasing: the flat order of the image
        if lab[p]:
            continue
        n, v, count, stack = len(sizes), val[p], 0, [p]
        lab[p] = n
        while stack:
            q = stack.pop()
            count += 1
            for d in deltas:
                r = q + d
                if val[r] == v and not lab[r]:
                    lab[r] = n
                    stack.append(r)
        sizes.append(count)
    sizes = np.asarray(sizes, np.int64)
    keep = sizes >= min_size
    keep[0] = False
    new = np.where(keep, np.cumsum(keep), 0)
    full = np.asarray(lab, np.int64).reshape(pad.shape)[tuple(slice(1, -1) for _ in x.shape)]
    return new[full].astype(np.int32), (len(sizes) - 1, int(keep.sum()))


def cc_reference_batch(x, connectivity, min_size=0):
    """[B, ...] -> (labels int32 [B, ...], counts int32 [B, 2])"""
    res = [cc_reference(img, connectivity, min_size) for img in x]
    return np.stack([r[0] for r in res]), np.asarray([r[1] for r in res], np.int32)


# ---- the named cases ------------------------------------------------------------------------------------------------------------------------
def serpentine(h=H2, w=W2):
    """a one-pixel-wide chain: every other row whole, joined at alternating ends -- it crosses every vertical tile border in every
    other row"""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    m[1::4, w - 1] = 1
    m[3::4, 0] = 1
    return m


def spiral(h=H2, w=W2):
    """a one-pixel-wide square spiral with one-pixel gaps between its windings, wound inwards from (0, 0)"""
    m = np.zeros((h, w), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    free = lambda yy, xx: 0 <= yy < h and 0 <= xx < w and not m[yy, xx]
    m[0, 0] = 1
    turns = 0
    while turns < 2:
        ny, nx = y + dy, x + dx
        ay, ax = ny + dy, nx + dx  # the pixel after the next must be free too, or the arm would touch the previous winding
        if free(ny, nx) and (not (0 <= ay < h and 0 <= ax < w) or not m[ay, ax]):
            y, x, turns = ny, nx, 0
            m[y, x] = 1
        else:
            dy, dx = dx, -dy
            turns += 1
    return m


def rings(h=H2, w=W2):
    yy, xx = np.mgrid[0:h, 0:w]
    return (np.maximum(np.abs(yy - h // 2), np.abs(xx - w // 2)) % 3 == 0).astype(np.uint8)


def comb(h=H2, w=W2):
    """teeth in every other column that join only in the last row: the root (0, 0) lies far from most pixels"""
    m = np.zeros((h, w), np.uint8)
    m[:, 0::2] = 1
    m[h - 1] = 1
    return m


def u_shape(h=H2, w=W2):
    """a U whose first pixel is on the right arm, in another tile than its bulk"""
    m = np.zeros((h, w), np.uint8)
    m[2:61, w - 10] = 1
    m[40:61, 5] = 1
    m[60, 5:w - 9] = 1
    return m


def random_mask(seed, density, shape):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def helix(z=Z3, h=H3, w=W3):
    """the sides of a rectangle, one per plane, consecutive sides sharing their corner pixel: connected through z faces only"""
    m = np.zeros((z, h, w), np.uint8)
    y0, y1, x0, x1 = 3, h - 3, 4, w - 5
    for k in range(z):
        side = k % 4
        if side == 0: m[k, y0, x0:x1 + 1] = 1
        elif side == 1: m[k, y0:y1 + 1, x1] = 1
        elif side == 2: m[k, y1, x0:x1 + 1] = 1
        else: m[k, y0:y1 + 1, x0] = 1
    return m


def two_blobs(offset):
    """two 2 x 4 x 4 blobs of which the second begins at `offset` from the first one's last pixel, across the tile border at 32"""
    m = np.zeros((Z3, H3, W3), np.uint8)
    m[0:2, 28:32, 28:32] = 1
    z, y, x = 1 + offset[0], 31 + offset[1], 31 + offset[2]
    m[z:z + 2, y:y + 4, x:x + 4] = 1
    return m


def blocky_ids(seed=77, shape=(H2, W2), block=7):
    """an int32 id map of few ids, so that every id occurs in several disconnected places and different ids are adjacent; negative ids
    and 2^30 among them"""
    rng = np.random.default_rng(seed)
    ids = np.array([0, 0, 1, 2, 3, -1, -3, 2 ** 30], np.int32)
    cy, cx = (shape[0] + block - 1) // block, (shape[1] + block - 1) // block
    coarse = ids[rng.integers(0, len(ids), (cy, cx))]
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, block, axis=0), block, axis=1)[:shape[0], :shape[1]])


def sized_components():
    """components of 26, 24 and 25 pixels in that raster order (and a fourth of 40): min_size = 25 drops the second"""
    m = np.zeros((H2, W2), np.uint8)
    m[1:3, 100:113] = 1    # 26, inside one tile
    m[30:34, 30:36] = 1    # 24, across the tile borders at 32 in both axes
    m[50:55, 62:67] = 1    # 25, across the tile border at 64
    m[60:64, 120:130] = 1  # 40, across the tile border at 128
    return m


@functools.lru_cache(maxsize=None)
def cases_2d():
    """name -> uint8 mask [Y, X] (never modified: copy first)"""
    c = {
        "one_pixel": np.ones((1, 1), np.uint8),
        "row_1x150": random_mask(11, 0.7, (1, 150)),
        "col_150x1": random_mask(12, 0.7, (150, 1)),
        "all_background": np.zeros((H2, W2), np.uint8),
        "all_foreground": np.ones((H2, W2), np.uint8),
        "checkerboard": (np.indices((H2, W2)).sum(axis=0) % 2 == 0).astype(np.uint8),
        "serpentine": serpentine(),
        "serpentine_t": np.ascontiguousarray(serpentine(W2, H2).T),
        "spiral": spiral(),
        "rings": rings(),
        "comb": comb(),
        "u_shape": u_shape(),
        "random_0.3": random_mask(21, 0.3, (H2, W2)),
        "random_0.59": random_mask(22, 0.59, (H2, W2)),
        "random_0.8": random_mask(23, 0.8, (H2, W2)),
        "sized": sized_components(),
    }
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def cases_3d():
    """name -> uint8 mask [Z, Y, X]"""
    c = {
        "helix": helix(),
        "edge_touch": two_blobs((1, 1, -3)),     # the blobs share x, differ by one step in z and y: an edge
        "corner_touch": two_blobs((1, 1, 1)),
        "random3d_0.3": random_mask(31, 0.3, (Z3, H3, W3)),
    }
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def cases_ids():
    """name -> int32 label image"""
    c = {"blocky_ids": blocky_ids(), "blocky_ids_3d": blocky_ids(78, (Z3 * H3, W3), 5).reshape(Z3, H3, W3)}
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(group, name, connectivity, min_size=0):
    """the restatement's answer for a named case, computed once: (labels [1, ...], counts [1, 2])"""
    img = {"2d": cases_2d, "3d": cases_3d, "ids": cases_ids}[group]()[name]
    lab, cnt = cc_reference_batch(img[None], connectivity, min_size)
    lab.setflags(write=False)
    return lab, cnt
