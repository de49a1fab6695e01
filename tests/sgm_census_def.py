"""The census / Hamming cost of the SGM mode (include/jn_sgm_cost.h, JN_SGM_COST_CENSUS) restated in numpy: the checker of
tests/test_sgm_census_api.py and tests/test_gpu_sgm_census.py.  TEST INFRASTRUCTURE.  Everything is integer arithmetic.  Signatures are
boolean stacks, deliberately not packed the way the kernel packs them: only Hamming distances are compared.  The aggregation is
tests/sgm_cost_def.py's; the restatement is anchored in test_sgm_census_api.py to a literal loop (`census_volume_literal`)."""
import numpy as np

import sgm_cost_def as cd

CENSUS = 4


def window(r):
    """(rx, ry) of block_radius r: 5x5, 7x7, 9x7."""
    return r, min(r, 3)


def bits(r):
    rx, ry = window(r)
    return (2 * rx + 1) * (2 * ry + 1) - 1


def census(I, rx, ry):
    """cen_I as a boolean stack [H][W][bits]: neighbour (i, j) != (0, 0) of the replicated-border image strictly less than the centre."""
    I = np.asarray(I, np.int64)
    H, W = I.shape
    x, y = np.arange(W), np.arange(H)
    out = []
    for j in range(-ry, ry + 1):
        for i in range(-rx, rx + 1):
            if i == 0 and j == 0:
                continue
            out.append(I[np.clip(y + j, 0, H - 1)][:, np.clip(x + i, 0, W - 1)] < I)
    return np.stack(out, axis=2)


def census_volume(L, R, D, r, cost_max):
    """C(x,y,d) = min(|cen_L(x,y) ^ cen_R(cl(x-d), y)|, cost_max) -> [H][W][D] uint8."""
    rx, ry = window(r)
    cl_, cr_ = census(L, rx, ry), census(R, rx, ry)
    H, W, _ = cl_.shape
    x = np.arange(W)
    C = np.zeros((H, W, D), np.int64)
    for d in range(D):
        C[:, :, d] = (cl_ != cr_[:, np.clip(x - d, 0, W - 1)]).sum(axis=2)
    return np.minimum(C, cost_max).astype(np.uint8)


def census_volume_literal(L, R, D, r, cost_max):
    """The same, one comparison at a time."""
    rx, ry = window(r)
    H, W = L.shape
    cl = lambda v, hi: min(max(v, 0), hi)
    out = np.zeros((H, W, D), np.uint8)
    for y in range(H):
        for x in range(W):
            for d in range(D):
                xr = cl(x - d, W - 1)
                hm = 0
                for j in range(-ry, ry + 1):
                    for i in range(-rx, rx + 1):
                        if i == 0 and j == 0:
                            continue
                        a = int(L[cl(y + j, H - 1), cl(x + i, W - 1)]) < int(L[y, x])
                        b = int(R[cl(y + j, H - 1), cl(xr + i, W - 1)]) < int(R[y, xr])
                        hm += a != b
                out[y, x, d] = min(hm, cost_max)
    return out


def process(L, R, D, P1, P2, lr_max_diff, subpixel, r, cost_max):
    """The CENSUS mode end to end on a u8 pair."""
    return cd.aggregate(census_volume(L, R, D, r, cost_max), P1, P2, lr_max_diff, subpixel)


def increasing_tables():
    """Strictly increasing maps of the 7-bit grey values [0, 127] into u8, for the invariance tests: a gain with an offset, and a gamma
    curve (exponent 0.6) forced strictly increasing."""
    v = np.arange(128)
    gamma = np.floor(255.0 * (v / 127.0) ** 0.6).astype(np.int64)
    for k in range(1, 128):
        gamma[k] = max(gamma[k], gamma[k - 1] + 1)
    assert gamma[-1] <= 255
    return {"gain": (2 * v + 1).astype(np.uint8), "gamma": gamma.astype(np.uint8)}
