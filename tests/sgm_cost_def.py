"""The scalar definition of the SGM mode over a cost volume (include/jn_sgm_cost.h) restated in numpy: the checker of
tests/test_sgm_cost_api.py and tests/test_gpu_sgm_cost.py.  TEST INFRASTRUCTURE.  Everything is integer arithmetic.  The restatement is
anchored in test_sgm_cost_api.py: `aggregate` over `sad3_volume` equals oracle/sgm_oracle.cpp bit for bit, `ssd_volume` equals a literal
triple loop (`ssd_literal`)."""
import numpy as np

SAD3, BLOCK_SSD, EXTERNAL = 0, 1, 2
PATHS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (-1, 1), (1, -1))


def prefilter(I, cap):
    """g = clamp(Sobel_x, -cap, cap) + cap with replicated borders (jn_sgm.h)."""
    I = np.asarray(I, np.int64)
    H, W = I.shape
    P = np.pad(I, 1, mode="edge")
    h = P[:, 2:] - P[:, :-2]                                   # [H+2][W]: I(x+1) - I(x-1) of the rows y-1 .. y+1
    sx = h[:-2] + 2 * h[1:-1] + h[2:]
    return np.clip(sx, -cap, cap) + cap


def sad3_volume(gL, gR, D):
    """jn_sgm.h's cost: C(x,y,d) = sum_{i=-1..1} |gL(cl(x+i), y) - gR(cl(x+i-d), y)| -> [H][W][D]."""
    H, W = gL.shape
    x = np.arange(W)
    C = np.zeros((H, W, D), np.int64)
    for d in range(D):
        for i in (-1, 0, 1):
            C[:, :, d] += np.abs(gL[:, np.clip(x + i, 0, W - 1)] - gR[:, np.clip(x + i - d, 0, W - 1)])
    return C


def ssd_volume(gL, gR, D, r):
    """SSD_r(x,y,d) = sum_{j,i=-r..r} (gL(cl(x+i), cr(y+j)) - gR(cl(x+i-d), cr(y+j)))^2 -> [H][W][D]."""
    H, W = gL.shape
    x, y = np.arange(W), np.arange(H)
    out = np.zeros((H, W, D), np.int64)
    for d in range(D):
        hs = np.zeros((H, W), np.int64)
        for i in range(-r, r + 1):
            e = gL[:, np.clip(x + i, 0, W - 1)] - gR[:, np.clip(x + i - d, 0, W - 1)]
            hs += e * e
        for j in range(-r, r + 1):
            out[:, :, d] += hs[np.clip(y + j, 0, H - 1)]
    return out


def ssd_literal(gL, gR, D, r):
    """The same, one term at a time."""
    H, W = gL.shape
    cl = lambda v, hi: min(max(v, 0), hi)
    out = np.zeros((H, W, D), np.int64)
    for y in range(H):
        for x in range(W):
            for d in range(D):
                s = 0
                for j in range(-r, r + 1):
                    for i in range(-r, r + 1):
                        e = int(gL[cl(y + j, H - 1), cl(x + i, W - 1)]) - int(gR[cl(y + j, H - 1), cl(x + i - d, W - 1)])
                        s += e * e
                out[y, x, d] = s
    return out


def block_cost(L, R, D, cap, r, cost_shift, cost_max):
    """C = min(SSD_r >> cost_shift, cost_max) of a u8 pair -> [H][W][D] uint8."""
    ssd = ssd_volume(prefilter(L, cap), prefilter(R, cap), D, r)
    return np.minimum(ssd >> cost_shift, cost_max).astype(np.uint8)


def _step(C, prev, ok, P1, P2):
    """One pixel of every line at once.  C, prev [N][D]; ok [N]: the predecessor exists (otherwise L = C)."""
    big = 1 << 30
    m = prev.min(axis=1, keepdims=True)
    lo = np.full_like(prev, big); lo[:, 1:] = prev[:, :-1] + P1
    hi = np.full_like(prev, big); hi[:, :-1] = prev[:, 1:] + P1
    L = C + np.minimum(np.minimum(prev, lo), np.minimum(hi, m + P2)) - m
    return np.where(ok[:, None], L, C)


def path(C, dx, dy, P1, P2):
    """L_r of one direction r = (dx, dy) over the volume C [H][W][D] (int64)."""
    H, W, D = C.shape
    L = np.zeros_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        prev = None
        for x in xs:
            L[:, x] = C[:, x] if prev is None else _step(C[:, x], prev, np.ones(H, bool), P1, P2)
            prev = L[:, x]
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    prev = None
    cols = np.arange(W)
    for y in ys:
        if prev is None:
            L[y] = C[y]
        else:
            src = cols - dx
            ok = (src >= 0) & (src < W)
            L[y] = _step(C[y], prev[np.clip(src, 0, W - 1)], ok, P1, P2)
        prev = L[y]
    return L


def aggregate(C, P1, P2, lr_max_diff, subpixel):
    """jn_sgm.h from `paths` on, over the volume C [H][W][D]: -> int16 map [H][W]."""
    C = np.asarray(C).astype(np.int64)
    H, W, D = C.shape
    S = np.zeros_like(C)
    for dx, dy in PATHS:
        S += path(C, dx, dy, P1, P2)
    dL = S.argmin(axis=2)                                      # the smallest d of the minimum
    big = 1 << 40
    SR = np.full((H, W, D), big, np.int64)                     # SR(x, y, d) = S(x + d, y, d) over x + d < W
    for d in range(D):
        if d < W:
            SR[:, :W - d, d] = S[:, d:, d]
    dR = SR.argmin(axis=2)
    x = np.arange(W)[None, :].repeat(H, 0)
    xr = x - dL
    ok = np.ones((H, W), bool)
    if lr_max_diff >= 0:
        ok = (xr >= 0) & (np.abs(dL - np.take_along_axis(dR, np.clip(xr, 0, W - 1), axis=1)) <= lr_max_diff)
    if not subpixel:
        return np.where(ok, dL, -1).astype(np.int16)
    d16 = 16 * dL
    inner = (dL > 0) & (dL < D - 1)
    pick = lambda dd: np.take_along_axis(S, np.clip(dd, 0, D - 1)[:, :, None], axis=2)[:, :, 0]
    sm, sc, sp = pick(dL - 1), pick(dL), pick(dL + 1)
    den = np.maximum(sm + sp - 2 * sc, 1)
    num = 16 * (sm - sp) + den
    q = np.sign(num) * (np.abs(num) // (2 * den))              # C division: towards zero
    d16 = np.where(inner, d16 + q, d16)
    return np.where(ok, d16, -16).astype(np.int16)


def process(L, R, D, P1, P2, cap, lr_max_diff, subpixel, r, cost_shift, cost_max):
    """The BLOCK_SSD mode end to end on a u8 pair."""
    return aggregate(block_cost(L, R, D, cap, r, cost_shift, cost_max), P1, P2, lr_max_diff, subpixel)
