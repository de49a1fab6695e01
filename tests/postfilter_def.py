"""The scalar definition of the disparity post-filter (include/jn_postfilter.h) restated: the checker of tests/test_gpu_postfilter.py and
tests/test_postfilter_api.py.  TEST INFRASTRUCTURE.  `segments_literal` is the header's graph handed to a plain union-find, pixel by
pixel; `segments` hands the same graph (the same edge list) to scipy's connected_components where scipy is present, because the literal
loop takes seconds per 1280x720 frame — tests/test_postfilter_api.py holds the two against each other.  The median is a literal sort."""
import numpy as np

I16, I16_SUB = 1, 2
MARKERS = {I16: -1, I16_SUB: -16}


def to_q(m, fmt):
    """-> (q int64, valid bool): valid iff v >= 0; q = 16 v (I16) or v (I16_SUB)."""
    m = np.asarray(m, np.int16).astype(np.int64)
    return m * (16 if fmt == I16 else 1), m >= 0


def _edges(q, valid, range_q):
    """The graph's edges of one map as pairs of flat pixel indices: 4-neighbours, both valid, |q - q'| <= range_q."""
    H, W = q.shape
    idx = np.arange(H * W).reshape(H, W)
    eh = valid[:, 1:] & valid[:, :-1] & (np.abs(q[:, 1:] - q[:, :-1]) <= range_q)
    ev = valid[1:, :] & valid[:-1, :] & (np.abs(q[1:, :] - q[:-1, :]) <= range_q)
    a = np.concatenate([idx[:, 1:][eh], idx[1:, :][ev]])
    b = np.concatenate([idx[:, :-1][eh], idx[:-1, :][ev]])
    return a, b


def segments_literal(q, valid, range_q):
    """-> sizes [H][W] int64: the number of pixels of the segment each valid pixel belongs to (0 at invalid pixels), the number of
    segments, and a map of segment identifiers (meaningful at valid pixels).  A plain union-find over the edges, one at a time."""
    H, W = q.shape
    parent = list(range(H * W))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    a, b = _edges(q, valid, range_q)
    for x, y in zip(a.tolist(), b.tolist()):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    roots = np.array([find(x) for x in range(H * W)]).reshape(H, W)
    count = np.bincount(roots[valid], minlength=H * W)
    return np.where(valid, count[roots], 0), int((count > 0).sum()), roots


def segments(q, valid, range_q):
    """segments_literal's results, through scipy's connected components when it is there and the map is not tiny."""
    H, W = q.shape
    if H * W < 4096:
        return segments_literal(q, valid, range_q)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return segments_literal(q, valid, range_q)
    a, b = _edges(q, valid, range_q)
    g = coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(H * W, H * W))
    _, lab = connected_components(g, directed=False)
    lab = lab.reshape(H, W)
    count = np.bincount(lab[valid], minlength=H * W)
    return np.where(valid, count[lab], 0), int((count > 0).sum()), lab


def median3(m):
    """Stage 2 on one map (int64, valid iff >= 0): the lower median of the valid pixels of the clipped 3x3 window, at valid pixels."""
    H, W = m.shape
    out = m.copy()
    if H * W <= 4096:                                            # literally
        for y in range(H):
            for x in range(W):
                if m[y, x] < 0:
                    continue
                win = sorted(int(v) for v in m[max(0, y - 1):y + 2, max(0, x - 1):x + 2].ravel() if v >= 0)
                out[y, x] = win[(len(win) - 1) // 2]
        return out
    big = np.iinfo(np.int64).max                                  # the same, all pixels at once: invalid values sort last
    p = np.full((H + 2, W + 2), big)
    p[1:-1, 1:-1] = np.where(m >= 0, m, big)
    stack = np.sort(np.stack([p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)]), axis=0)
    k = (stack != big).sum(axis=0)
    med = np.take_along_axis(stack, np.maximum(k - 1, 0)[None] // 2, axis=0)[0]
    return np.where(m >= 0, med, m)


def apply(maps, fmt, speckle_size=200, speckle_range_q=16, median=0, seg=segments):
    """maps [n][H][W] int16 -> (filtered maps int16, stats [n][4] uint32: valid on input, segments, speckle segments, pixels removed)."""
    maps = np.asarray(maps, np.int16)
    out = np.empty_like(maps)
    stats = np.zeros((maps.shape[0], 4), np.uint32)
    for f in range(maps.shape[0]):
        q, valid = to_q(maps[f], fmt)
        m = maps[f].astype(np.int64)
        stats[f, 0] = valid.sum()
        if speckle_size >= 1:
            size, nseg, ident = seg(q, valid, speckle_range_q)
            speckle = valid & (size < speckle_size)
            stats[f, 1] = nseg
            stats[f, 2] = np.unique(ident[speckle]).size
            stats[f, 3] = speckle.sum()
            m = np.where(speckle, MARKERS[fmt], m)
        if median:
            m = median3(m)
        out[f] = m.astype(np.int16)
    return out, stats


# ---- the longest chains a frame can hold: test and measurement inputs (tests/test_gpu_postfilter.py, scripts/postfilter_rate.py) ----

def spiral(H, W):
    """A one-pixel-wide rectangular spiral from the corner to the centre: one chain through the whole frame.  A walk that goes straight
    while the cell after the next one is free, and turns right otherwise."""
    m = [[-1] * W for _ in range(H)]
    y = x = 0
    dy, dx = 0, 1
    m[0][0] = 5

    def free(yy, xx):
        return not (0 <= yy < H and 0 <= xx < W) or m[yy][xx] < 0
    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and m[ny][nx] < 0 and free(ny + dy, nx + dx):
                break
            dy, dx = dx, -dy
        else:
            break
        y, x = ny, nx
        m[y][x] = 5
    return np.array(m, np.int16)


def serpentine(H, W):
    """Rows 0, 2, 4, ... full, joined alternately at the right and the left end: one chain, crossing every tile border both ways."""
    m = np.full((H, W), -1, np.int16)
    m[0::2, :] = 9
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 9
    return m
