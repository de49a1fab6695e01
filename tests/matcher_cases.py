"""The case table of the three matchers the reference does not have (SGM, block matching with SAD and with SSD on the matrix cores), shared by
tests/test_gpu_matcher_matrix.py (every case against the scalar definition on the GPU), tests/test_matcher_matrix.py (the table covers every
kernel instantiation in the binary; the checker at the same parameter edges) and scripts/sgm_debug.py.  Plain data and numpy: nothing here
touches a GPU.

A case is (W, H, D, scene, n, kw, layout, edge, why):
  scene    an int: the survey's plane-and-box pair of that disparity range (Oracle.synth_pair); or a generator of PAIRS below
  kw       parameters that differ from the mode's defaults
  layout   how the caller's images lie in memory: pad (pitch = W + pad), gap (rows between two images of the batch), extra (max_batch = n + extra),
           smaller_first (a batch of n - 1 of the same frames first, on the same handle)
  edge     (SGM only) what the oracle's path values must show for the case to count: see sgm_edges()
  why      one line: the edge the case is there for (it is printed when the case fails)"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "W H D scene n kw layout edge why")


def case(W, H, D, scene, n, kw, why, layout=None, edge=()):
    return Case(W, H, D, scene, n, dict(kw), dict(layout or {}), tuple(edge), why)


def case_id(c):
    return "%dx%d-D%d-%s-n%d-%s%s" % (c.W, c.H, c.D, c.scene, c.n, "-".join("%s%s" % (k[:3], v) for k, v in sorted(c.kw.items())) or "defaults",
                                      "-" + "-".join("%s%s" % (k, v) for k, v in sorted(c.layout.items())) if c.layout else "")


# ------------------------------------------------------------------ images ------------------------------------------------------------------
def _bits(W, H, seed):
    """0/255 noise, the left image the right one moved by five columns: both prefiltered images sit at 0 and 2 cap almost everywhere, the
    true disparity keeps one path value low while the others climb to the recurrence's limit"""
    t = (np.random.default_rng(seed).integers(0, 2, (H, W + 5)) * 255).astype(np.uint8)
    return t[:, :W].copy(), t[:, 5:].copy()


def _noise(W, H, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W)).astype(np.uint8), rng.integers(0, 256, (H, W)).astype(np.uint8)


def _saw(W, H, seed):
    """Opposed ramps, 8 grey levels per column (W <= 32): Sobel_x is >= +31 in every left pixel and <= -31 in every right pixel, borders
    included, so with cap = 31 the prefiltered images are 62 and 0 everywhere: every |a - b| = 2 cap, every candidate's cost is the largest
    a block can have, every candidate ties."""
    assert W <= 32
    x = np.arange(W)
    return np.tile((8 * x).astype(np.uint8), (H, 1)), np.tile((248 - 8 * x).astype(np.uint8), (H, 1))


def _peak(W, H, seed):
    """The mirror of _saw: the left image the same ramp, the right one falling by 12 a column except for ten steps of +4 from column 12 on,
    which make its prefiltered image 62 in the nine columns 13..21 and 0 elsewhere: for x >= 17 exactly ONE candidate (d = x - 17) has cost 0
    with a 9x9 block, its neighbours cost one column of the block, everything further away the largest cost"""
    assert 24 <= W <= 32
    steps = np.full(W - 1, -12)
    steps[12:22] = 4
    r = 252 + np.concatenate([[0], np.cumsum(steps)])
    assert r.min() >= 0
    return np.tile((8 * np.arange(W)).astype(np.uint8), (H, 1)), np.tile(r.astype(np.uint8), (H, 1))


def _flat(W, H, seed):
    return np.full((H, W), 77, np.uint8), np.full((H, W), 77, np.uint8)


PAIRS = {"bits": _bits, "noise": _noise, "saw": _saw, "peak": _peak, "flat": _flat}


def images(c, oracle):
    """(Ls, Rs) [n][H][W] uint8 of a case; frame b is drawn with seed 700 + b"""
    pairs = [PAIRS[c.scene](c.W, c.H, 700 + b) if c.scene in PAIRS else oracle.synth_pair(c.W, c.H, c.scene, 700 + b) for b in range(c.n)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


# ------------------------------------------------------------------ SGM ------------------------------------------------------------------
# The row sweeps come in a byte form and a 16-bit form (WIDE: 3 P2 > 255, the three-path volume is u16); strips of 16 pixels (8 at D = 256), four to
# a block: 64 (32) columns of the sheared frame, NB = ceil((W + H - 1) / 64 (32)) blocks.
_EDGE_PARAMS = [
    ({"P1": 10, "P2": 85, "prefilter_cap": 20}, ("top", "byte"), 96, 24, 2, "3 P2 = 255: the largest P2 of the byte form, the three-path byte reaches 255"),
    ({"P1": 10, "P2": 86, "prefilter_cap": 20, "subpixel": 1}, ("top", "wide"), 96, 24, 2, "3 P2 = 258: the first P2 of the 16-bit form, same images and cap as P2 = 85"),
    ({"P1": 20, "P2": 249, "prefilter_cap": 1}, ("top", "wide"), 200, 48, 1, "the largest P2 the ABI accepts (cap = 1): path values reach 255, three-path sums 747"),
    ({"P1": 7, "P2": 69, "prefilter_cap": 31, "subpixel": 1}, ("top", "byte"), 96, 24, 2, "6 cap + P2 = 255 with the largest cap: a path value reaches the top of a byte"),
    ({"P1": 20, "P2": 64, "prefilter_cap": 31}, ("top", "byte"), 64, 16, 1, "P2 = 64: the first value past six bits"),
    ({"P1": 0, "P2": 60}, ("byte",), 80, 20, 1, "P1 = 0: a step of one disparity is free"),
    ({"P1": 60, "P2": 60, "subpixel": 1}, ("top", "byte"), 80, 20, 1, "P1 = P2: the neighbours' term never wins over the jump term"),
    ({"P1": 100, "P2": 100, "prefilter_cap": 20, "lr_max_diff": 0}, ("top", "wide"), 80, 20, 1, "P1 = P2 in the 16-bit form, exact L/R agreement"),
]
SGM_CASES = [case(W, H, D, "bits", n, kw, why, edge=edge) for D in (64, 128, 256) for kw, edge, W, H, n, why in _EDGE_PARAMS]
SGM_CASES += [
    case(8, 8, 64, "noise", 2, {}, "the smallest frame jn_sgm_create accepts"),
    case(8, 8, 128, "noise", 1, {"P2": 90, "prefilter_cap": 20, "subpixel": 1}, "8x8 in the 16-bit form, 1/16 pixel"),
    case(8, 8, 256, "noise", 1, {}, "8x8 with eight lanes per pixel: one strip"),
    case(9, 8, 64, "noise", 1, {"P2": 120, "prefilter_cap": 20}, "one column more than a multiple of 8, 16-bit form"),
    case(9, 8, 256, "noise", 2, {"subpixel": 1}, "9x8: the second strip of 8 pixels holds one column"),
    case(17, 9, 128, "noise", 2, {"lr_max_diff": 3}, "17x9: one pixel in the second strip of 16, wide L/R tolerance"),
    case(17, 9, 64, "noise", 1, {"lr_max_diff": -1, "subpixel": 1}, "17x9 without the L/R check"),
    case(40, 12, 64, 12, 1, {}, "narrower than one block of four strips (W < 64)"),
    case(40, 12, 128, 12, 1, {"P2": 86, "prefilter_cap": 20}, "narrower than one block, 16-bit form"),
    case(20, 12, 256, 12, 1, {"lr_max_diff": 0}, "narrower than one block of four strips of 8 (W < 32)"),
    case(56, 9, 64, 16, 1, {"lr_max_diff": 3}, "W + H - 1 = 64: exactly one block"),
    case(57, 9, 64, 16, 1, {"lr_max_diff": 3}, "W + H - 1 = 65: the second block holds one column of the sheared frame"),
    case(57, 9, 128, 16, 1, {"P2": 100, "prefilter_cap": 20, "subpixel": 1}, "W + H - 1 = 65 in the 16-bit form"),
    case(24, 9, 256, 8, 1, {"lr_max_diff": -1}, "W + H - 1 = 32: exactly one block of strips of 8, no L/R check"),
    case(25, 9, 256, 8, 1, {"lr_max_diff": -1, "P2": 86, "prefilter_cap": 20}, "W + H - 1 = 33, 16-bit form, no L/R check"),
    case(150, 40, 64, 40, 3, {"P2": 86, "prefilter_cap": 20}, "pitch = W + 8, gap rows, max_batch = n + 2, n - 1 first; 16-bit form",
         layout={"pad": 8, "gap": 3, "extra": 2, "smaller_first": True}),
    case(150, 40, 128, 40, 2, {"subpixel": 1}, "odd pitch (W + 13): every row but the first starts at an odd address",
         layout={"pad": 13, "gap": 1, "extra": 2, "smaller_first": True}),
    case(93, 31, 256, 30, 2, {"P2": 120, "prefilter_cap": 15, "subpixel": 1}, "odd pitch and gap rows at D = 256, 16-bit form",
         layout={"pad": 13, "gap": 2, "extra": 2, "smaller_first": True}),
]

# strips per block (JN_SGM_NS) and four lanes per pixel at D = 256 (JN_SGM_LQ) exist in the hooks build only: (environment, case)
_HOOK_BYTE = {"P1": 7, "P2": 69, "prefilter_cap": 31, "subpixel": 1}
_HOOK_WIDE = {"P1": 10, "P2": 86, "prefilter_cap": 20}
SGM_HOOKS_CASES = [(env, case(W, 24, D, "bits", 2, kw, why, edge=edge))
                   for env, D, W in (({"JN_SGM_NS": "2"}, 64, 96), ({"JN_SGM_NS": "8"}, 64, 200), ({"JN_SGM_NS": "2"}, 128, 96), ({"JN_SGM_NS": "8"}, 128, 200),
                                     ({"JN_SGM_LQ": "4"}, 256, 96))
                   for kw, edge, why in ((_HOOK_BYTE, ("top", "byte"), "byte form, 6 cap + P2 = 255"), (_HOOK_WIDE, ("top", "wide"), "16-bit form, 3 P2 = 258"))]

# The sweeps over a cost volume (include/jn_sgm_cost.h: k_swc_h, k_sw_w<..., true>; four strips and the default lanes per pixel only).  They run in
# tests/test_gpu_sgm_cost.py's anchor: jn_sgm.h's own cost as an EXTERNAL volume must give the plain handle's map, so the parameters lie inside both
# handles' ranges (6 cap + P2 <= 255 is also "every byte of the volume <= 255 - P2").  The scene is the anchor's plane-and-box pair.
_WIDE_VOL = {"P1": 7, "P2": 100, "prefilter_cap": 20}
SGM_VOLUME_CASES = [case(W, H, D, min(D - 16, 48), 2, kw, why) for W, H, D, kw, why in (
    (150, 60, 64, {}, "byte form, D = 64"),
    (190, 45, 128, {"subpixel": 1}, "byte form, D = 128, 1/16 pixel"),
    (300, 40, 256, {"subpixel": 1, "lr_max_diff": 2}, "byte form, eight lanes per pixel, 1/16 pixel"),
    (141, 52, 64, _WIDE_VOL, "3 P2 > 255: the 16-bit three-path volume, D = 64"),
    (333, 37, 128, {"lr_max_diff": -1}, "no L/R check"),
    (222, 43, 128, _WIDE_VOL, "16-bit form, D = 128"),
    (260, 36, 256, _WIDE_VOL, "16-bit form, eight lanes per pixel"))]

DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (-1, 1), (1, -1))
DOWN, UP = ((0, 1), (1, 1), (-1, 1)), ((0, -1), (-1, -1), (1, -1))


def cost_volume(gL, gR, D):
    """C(x, y, d) of include/jn_sgm.h: three columns of absolute differences, clamped at the image border.  [H][W][D] int32"""
    H, W = gL.shape
    Cv = np.zeros((H, W, D), np.int32)
    xs = np.arange(W)
    for d in range(D):
        for i in (-1, 0, 1):
            xl = np.clip(xs + i, 0, W - 1); xr = np.clip(xs + i - d, 0, W - 1)
            Cv[:, :, d] += np.abs(gL[:, xl].astype(np.int32) - gR[:, xr].astype(np.int32))
    return Cv


def path_excess(sgm, L, R, D, kw):
    """{direction: L_r - C} of one pair by the oracle (int32, [H][W][D]), the cost volume, and the largest L_r of any direction"""
    p = sgm.params(D, **kw)
    gL, gR = sgm.prefilter(L, p.prefilter_cap), sgm.prefilter(R, p.prefilter_cap)
    Cv = cost_volume(gL, gR, D)
    paths = {dxy: sgm.path(gL, gR, D, p.P1, p.P2, *dxy).astype(np.int32) for dxy in DIRECTIONS}
    return {dxy: v - Cv for dxy, v in paths.items()}, Cv, max(int(v.max()) for v in paths.values())


def sgm_edges(c, m, top):
    """What a case's `edge` names, read off the oracle's path values of one frame; returns the names that were NOT reached.
      top   some L_r = 6 cap + P2, the largest value the recurrence can give (255 when the parameters sit on the ABI's limit)
      byte  3 P2 <= 255 and the three-path volume's stored value 3 P2 - sum(L_r - C) takes both 0 and 3 P2
      wide  3 P2 > 255, some three-path sum of L_r - C is above 255 and some stored value 3 P2 - sum is (neither fits a byte)"""
    P2, cap = c.kw.get("P2", 60), c.kw.get("prefilter_cap", 31)
    sums = [sum(m[d] for d in trio) for trio in (DOWN, UP)]
    lo, hi = min(int(s.min()) for s in sums), max(int(s.max()) for s in sums)
    reached = {"top": top == 6 * cap + P2,
               "byte": 3 * P2 <= 255 and lo == 0 and hi == 3 * P2,
               "wide": 3 * P2 > 255 and hi > 255 and 3 * P2 - lo > 255}
    return [e for e in c.edge if not reached[e]]


def volume_order(D, wide, lq=None):
    """d of every stored element of a pixel in the sweeps' volumes (sgm_sweep.hip VOLUME LAYOUT / REGISTER LAYOUT): lq lanes share a pixel (8 at
    D = 256 in the release library, else 4), a lane holds D / lq disparities as NR pairs (j, j + NR), 16-byte pieces of the lanes interleave"""
    lq = lq or (8 if D == 256 else 4)
    DPL = D // lq
    NR = DPL // 2
    out = np.zeros(D, np.int64)
    for e in range(D):
        if wide:                                              # u16 elements: a piece holds registers 4c .. 4c+3 as they are
            c, q, w = e // (8 * lq), (e % (8 * lq)) // 8, e % 8
            r, half = 4 * c + w // 2, w % 2
        else:                                                 # bytes: a piece holds registers 8c .. 8c+7, packed in pairs
            c, q, b = e // (16 * lq), (e % (16 * lq)) // 16, e % 16
            r, half = 8 * c + 2 * (b // 4) + ((b % 4) >> 1), b & 1
        out[e] = DPL * q + r + half * NR
    return out


# ------------------------------------------------------------------ block matching ------------------------------------------------------------------
# SSD (cost_function 1, bm_mfma.hip): k_bmq_match<NT, R, SIDE>, NT = D / 32 + 1 tiles of 32 candidate columns; a wave takes 32 columns, the launch
# picks 12 rows per band for a lone small pair.  100x40: a last tile of 4 columns and a last band of 4 rows.
_BM_LAYOUT = {"pad": 13, "gap": 2, "extra": 2, "smaller_first": True}
BM_SSD_CASES = [case(100, 40, D, 24, 1, {"block_radius": r, "cost_function": 1, "subpixel": (D // 32 + r) & 1},
                     "NT = %d, R = %d: both sides, last tile of 4 columns, last band of 4 rows" % (D // 32 + 1, r))
                for D in range(32, 257, 32) for r in (2, 3, 4)]
BM_SSD_CASES += [
    case(64, 24, 256, 24, 2, {"block_radius": 4, "cost_function": 1, "subpixel": 1}, "NT = 9, R = 4 (the largest LDS request) on whole tiles and whole bands"),
    case(64, 24, 256, 24, 2, {"block_radius": 3, "cost_function": 1}, "NT = 9, R = 3 on whole tiles and whole bands"),
    case(64, 24, 224, 24, 2, {"block_radius": 4, "cost_function": 1}, "NT = 8, R = 4 on whole tiles and whole bands"),
    case(32, 20, 256, "saw", 1, {"block_radius": 4, "cost_function": 1, "subpixel": 1}, "every candidate costs 81 x 62^2: all ties, the smallest d must win"),
    case(32, 20, 256, "peak", 1, {"block_radius": 4, "cost_function": 1, "subpixel": 1, "lr_max_diff": -1}, "one candidate at cost 0 among candidates at the largest cost"),
    case(32, 20, 32, "saw", 2, {"block_radius": 4, "cost_function": 1}, "all ties at the largest cost, two tiles"),
] + [case(32, 20, D, "saw", 1, {"block_radius": 2 + D // 32 % 3, "cost_function": 1}, "all ties under NT = %d: the smallest d must win in every tile walk" % (D // 32 + 1))
     for D in range(64, 256, 32)] + [
    case(64, 24, 128, "flat", 1, {"block_radius": 2, "cost_function": 1, "subpixel": 1}, "every candidate costs 0"),
    case(100, 40, 160, 24, 1, {"block_radius": 3, "cost_function": 1, "lr_max_diff": -1}, "no right-referenced pass"),
    case(8, 8, 32, "noise", 2, {"block_radius": 4, "cost_function": 1}, "the smallest frame jn_bm_create accepts: the block is higher and wider than the image"),
    case(8, 8, 256, "noise", 1, {"block_radius": 2, "cost_function": 1, "subpixel": 1}, "8x8 under nine tiles of candidates"),
    case(27, 11, 64, "noise", 1, {"block_radius": 3, "cost_function": 1, "lr_max_diff": 0}, "narrower than one tile of 32 columns"),
    case(150, 40, 96, 40, 3, {"block_radius": 3, "cost_function": 1, "subpixel": 1}, "pitch = W + 8, gap rows, max_batch = n + 2, n - 1 first",
         layout={"pad": 8, "gap": 3, "extra": 2, "smaller_first": True}),
    case(93, 31, 192, 30, 2, {"block_radius": 4, "cost_function": 1}, "odd pitch (W + 13), gap rows", layout=_BM_LAYOUT),
]

# SAD (cost_function 0, bm.hip): k_bm<R, SIDE>; chunks of 16 disparities go round the four waves, the last chunk holds 8 when D is an odd multiple
# of 8.  D -> chunks per wave: 8, 16: 1 0 0 0 | 24: 1 1 0 0 | 40: 1 1 1 0 | 56: 1 1 1 1 | 72: 2 1 1 1 | 88: 2 2 1 1 | 104: 2 2 2 1 | 136: 3 2 2 2 |
# 200: 4 3 3 3 | 248, 256: 4 4 4 4.  70x20: a second column group of 6 pixels.
BM_SAD_DS = (8, 16, 24, 40, 56, 72, 88, 104, 136, 200, 248, 256)
BM_SAD_CASES = [case(70, 20, D, 16, 1, {"block_radius": r, "subpixel": (i + r) & 1, "lr_max_diff": -1 if (i + r) % 5 == 0 else 1},
                     "%d chunks of 16 over four waves%s, R = %d" % ((D + 15) // 16, ", the last one half full" if D & 8 else "", r))
                for i, D in enumerate(BM_SAD_DS) for r in (2, 3, 4)]
BM_SAD_CASES += [
    case(32, 20, 256, "saw", 1, {"block_radius": 4, "subpixel": 1}, "every candidate costs 81 x 62: packed 16-bit sums at 4 x 81 x 62 + 3, all ties"),
    case(32, 20, 256, "peak", 1, {"block_radius": 4, "subpixel": 1, "lr_max_diff": -1}, "one candidate at cost 0 among candidates at the largest cost"),
    case(32, 20, 8, "saw", 2, {"block_radius": 4}, "all ties at the largest cost, half a chunk"),
    case(8, 8, 8, "noise", 2, {"block_radius": 4}, "the smallest frame and the smallest range"),
    case(8, 8, 256, "noise", 1, {"block_radius": 2, "subpixel": 1}, "8x8 under the largest range"),
    case(27, 11, 40, "noise", 1, {"block_radius": 3, "lr_max_diff": 0}, "narrower than 32 columns"),
    case(150, 40, 72, 40, 3, {"block_radius": 2, "subpixel": 1}, "pitch = W + 8, gap rows, max_batch = n + 2, n - 1 first",
         layout={"pad": 8, "gap": 3, "extra": 2, "smaller_first": True}),
    case(93, 31, 200, 30, 2, {"block_radius": 3}, "odd pitch (W + 13), gap rows", layout=_BM_LAYOUT),
]
BM_CASES = BM_SSD_CASES + BM_SAD_CASES


# ------------------------------------------------------------------ dispatch, restated ------------------------------------------------------------------
MATCHER_FAMILIES = ("k_sw_w", "k_sw_h", "k_swc_h", "k_bm", "k_bm_finish_sub", "k_bmq_match", "k_bmq_box", "k_bmq_finish")


def sgm_instantiations(c, env=None, volume=False):
    """The k_sw_w and k_sw_h / k_swc_h instantiations a batch of the SGM case launches (sgm_sweep.hip sweep_run / sweep_run_cost, run_sweeps,
    launch_w), named as c++filt prints them.  volume: the costs are read from a volume (the last argument of k_sw_w).
    env: the hooks build's JN_SGM_NS / JN_SGM_LQ; the release library ignores both, and so does the volume path of either build."""
    env = {} if volume or not env else env
    ns = int(env.get("JN_SGM_NS", 4))
    ns = ns if c.D != 256 and ns in (2, 8) else 4
    lq = 4 if c.D != 256 or env.get("JN_SGM_LQ") == "4" else 8
    nr = c.D // (2 * lq)                                      # disparity pairs per lane
    ring = 8 if nr <= 16 and lq == 4 else 4
    wide = "true" if 3 * c.kw.get("P2", 60) > 255 else "false"
    return {"%s<%d, %d>" % ("k_swc_h" if volume else "k_sw_h", nr, lq)} | {
        "k_sw_w<%d, %d, %d, %s, %s, %d, %s>" % (nr, ns, ring, final, wide, lq, "true" if volume else "false") for final in ("false", "true")}


def bm_instantiations(c):
    """The matching and finishing kernels a batch of the block-matching case launches (bm.hip bm_submit, bm_mfma.hip run)"""
    r, sides = c.kw.get("block_radius", 4), (0, 1) if c.kw.get("lr_max_diff", 1) >= 0 else (0,)
    if c.kw.get("cost_function", 0) == 1:
        return {"k_bmq_box<%d>" % r, "k_bmq_finish<%d>" % r} | {"k_bmq_match<%d, %d, %d>" % (c.D // 32 + 1, r, s) for s in sides}
    return {"k_bm<%d, %d>" % (r, s) for s in sides} | ({"k_bm_finish_sub<%d>" % r} if c.kw.get("subpixel", 0) else set())


def table_instantiations():
    out = set()
    for c in SGM_CASES:
        out |= sgm_instantiations(c)
    for env, c in SGM_HOOKS_CASES:
        out |= sgm_instantiations(c, env)
    for c in SGM_VOLUME_CASES:
        out |= sgm_instantiations(c, volume=True)
    for c in BM_CASES:
        out |= bm_instantiations(c)
    return out
