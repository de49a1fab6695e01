"""The case table of the ELAS path and its dispatch, restated: shared by tests/test_gpu_elas_matrix.py (every case bit for bit against the CPU
oracle on the GPU), tests/test_elas_matrix.py (the table launches every ELAS kernel instantiation the two libraries hold; every case gives the
status it declares on the CPU) and tests/mocks/elas_route_worker.py (the cases whose switches are read once per process).  Plain data and
numpy: nothing here touches a GPU.

A case is (W, H, sd, disp_max, seed, n, kw, env, hooks, why, flow, run):
  sd, seed  the survey's plane-and-box pair of that disparity range (Oracle.synth_pair); frame b is drawn with seed + b
  n         pairs.  n == 1: a latency handle (max_batch 1) through jn_elas_process, host pointers; n > 1: a batch handle (max_batch n)
            through jn_elas_submit, device pointers
  kw        parameters that differ from the ROBOTICS defaults
  env       environment switches of the case, on top of BASE_ENV; a case of a child takes the child's (CHILDREN)
  hooks     the case needs the hooks build (csrc/hooks.h)
  why       one line: what the case is there for
  flow      "plane" or "desc": what jn_elas_route_stats must report (declared here, NOT computed: test_elas_matrix.py checks the restated
            dispatch against it, the GPU test the library)
  run       host_threads (always explicit: the pool's size decides routes), slots (the batch goes out on every slot at once), pad (pitch = W + pad),
            noise (index of a frame of pure noise: too few support points), gpu_dt (jn_elas_route_stats says the HANDLE triangulates
            on the GPU), child (name in CHILDREN: the case runs in that fresh process)"""
import math
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "W H sd disp_max seed n kw env hooks why flow run")

# what tests/conftest.py puts into the environment of the pytest process (the GPU test sets it per case, a child gets it from the parent)
BASE_ENV = {"JN_POST_FUSED_MIN_PIXELS": "0"}
UNFUSED = {"JN_POST_FUSED_MIN_PIXELS": "10000000"}          # the library's own default: small batches take the four short kernels

# Switches that a `static` in a launcher reads once per process: fresh child processes (tests/mocks/elas_route_worker.py), one per line.
# name: (hooks build, environment)
CHILDREN = {
    "lr_ccl_split": (False, {"JN_LR_CCL_FUSED": "0"}),
    "grid_late": (False, {"JN_GRID_EARLY": "0"}),
    "wavefront": (False, {"JN_FILTER_WAVEFRONT": "1", "JN_HOST_FILTERS": "0"}),      # (the wavefront form alone is not "fast": lone pairs would filter on the host)
    "sgm_tail3": (False, {"JN_SGM_TAIL": "3"}),
    "hooks_a": (True, {"JN_SUPPORT_SEGMENTS": "1", "JN_FUSE_LIST": "0", "JN_BIN_SETUP": "0", "JN_DENSE_XCD_ORDER": "0", "JN_POST_BAND": "8",
                       "JN_DT_DUMMY": "1", "JN_DT_DUMMY_US": "1"}),
    "hooks_b": (True, {"JN_BIN_SETUP": "1", "JN_POST_BAND": "24"}),
    "hooks_c": (True, {"JN_POST_BAND": "1000"}),
}
SGM_TAIL_ID = "sgm-tail3"            # the one entry of a child that is not an ELAS case (elas_route_worker.py)
SGM_TAIL_FRAME = (150, 40, 64, 2)    # W, H, num_disparities, pairs of that entry


def case(W, H, sd, disp_max, seed, n, kw, why, flow="plane", env=None, hooks=False, **run):
    run.setdefault("host_threads", 8 if n == 1 else 2)
    run.setdefault("slots", 1)
    if run.get("child"):
        hooks, env = CHILDREN[run["child"]][0], dict(CHILDREN[run["child"]][1], **(env or {}))
    return Case(W, H, sd, disp_max, seed, n, dict(kw), dict(env or {}), hooks, why, flow, run)


def case_id(c):
    return "%dx%d-d%d-s%d-n%d-%s%s%s" % (c.W, c.H, c.disp_max, c.seed, c.n, "-".join("%s%s" % (k.replace("_", "")[:12], v) for k, v in sorted(c.kw.items())) or "defaults",
                                        "".join("-%s%s" % (k[3:], v) for k, v in sorted(c.env.items())),
                                        "".join("-%s%s" % (k, v) for k, v in sorted(c.run.items()) if (k, v) not in (("slots", 1),) and k != "child"))


def images(c, oracle):
    """(Ls, Rs) [n][H][W] uint8 of a case"""
    pairs = [oracle.synth_pair(c.W, c.H, c.sd, c.seed + b) for b in range(c.n)]
    if "noise" in c.run:
        rng = np.random.default_rng(c.seed)
        pairs[c.run["noise"]] = tuple(rng.integers(0, 255, (c.H, c.W)).astype(np.uint8) for _ in range(2))
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def effective_env(c):
    return dict(BASE_ENV, **c.env)


# ------------------------------------------------------------------ parameters, restated ------------------------------------------------------------------
DEFAULTS = dict(disp_min=0, support_threshold=0.85, support_texture=10, candidate_stepsize=5, incon_window_size=5, incon_threshold=5,
                incon_min_support=5, add_corners=0, grid_size=20, beta=0.02, gamma=3.0, sigma=1.0, sradius=2.0, match_texture=1, lr_threshold=2,
                speckle_sim_threshold=1.0, speckle_size=200, ipol_gap_width=3, filter_median=0, filter_adaptive_mean=1, postprocess_only_left=1,
                subsampling=0)
F = np.float32


def params(c):
    p = dict(DEFAULTS, disp_max=c.disp_max)
    assert set(c.kw) <= set(p), sorted(set(c.kw) - set(p))
    p.update(c.kw)
    return p


def radius_of(p):
    return int(max(F(math.ceil(float(F(p["sigma"]) * F(p["sradius"])))), F(2.0)))


def priors(p):
    """P[0..radius] of jn_elas_create (elas.cpp:802-805) in its float arithmetic"""
    gamma, beta, two_sigma_sq = F(p["gamma"]), F(p["beta"]), F(2) * F(p["sigma"]) * F(p["sigma"])
    with np.errstate(over="ignore"):
        return [int((-np.log(gamma + np.exp(F(-dd * dd) / two_sigma_sq)) + np.log(gamma)) / beta) for dd in range(radius_of(p) + 1)]


PRIOR_LIMIT = 1 << 19          # cost + prior in 24 bits of k_dense's keys, bias 2^20
CELL_PRIOR_MAX = 8000          # kCellPriorMax: the 16-bit cost field of k_dense_row's keys


def create_status(c):
    """jn_elas_create's range checks: 0 accepted, 2 JN_ERR_UNSUPPORTED, 3 JN_ERR_INVALID"""
    p = params(c)
    if c.W < 32 or c.H < 32 or c.W > 8192 or c.H > 8192 or c.n < 1 or c.run["slots"] < 1:
        return 3
    if ((p["subsampling"] and ((c.W | c.H) & 1)) or p["disp_max"] > 255 or p["disp_max"] < 10 or p["disp_min"] > p["disp_max"] or p["ipol_gap_width"] < 0 or
            p["candidate_stepsize"] < 1 or p["grid_size"] < 1 or radius_of(p) > 7 or p["incon_window_size"] < 0):
        return 2
    return 2 if any(abs(v) >= PRIOR_LIMIT for v in priors(p)) else 0


def prior_edge_betas(gamma=3.0):
    """(accepted, refused): float32 betas that put |P[0]| one part in 10^4 below and above 2^19 (far more than logf's last bit)"""
    p0 = float(np.log(F(gamma) + F(1)) - np.log(F(gamma)))
    return float(F(p0 / PRIOR_LIMIT * (1 + 1e-4))), float(F(p0 / PRIOR_LIMIT * (1 - 1e-4)))


# ------------------------------------------------------------------ dispatch, restated ------------------------------------------------------------------
# Only what decides WHICH kernel runs (csrc/kernels.hip launchers, csrc/elas_batch.cpp plan_batch / queue_stage_a / queue_post_processing /
# queue_stage_b, csrc/delaunay_gpu.hip launch_delaunay), for the FIRST batch of a fresh handle, every frame of which finds support points.
DT_WHOLE = (152 * 1024 - 64) // 32          # delaunay_gpu_capacity(152 KB): vertices of a side one workgroup's LDS holds
STRIP_W, TILE_H = 128, 8


def lattice(c):
    p = params(c)
    step = p["candidate_stepsize"] + (p["candidate_stepsize"] % 2 if p["subsampling"] else 0)
    return step, -(-c.W // step), -(-c.H // step)


def _knob(c, env, name, hook):
    """the value of a switch as the case's library sees it: the release library has no JN_HOOK_ENV names"""
    return env.get(name) if (c.hooks or not hook) else None


def support_route(c, env=None):
    """(pitch bucket, segments) of k_support_lds, or None: no bucket holds the window (k_support, materialised descriptors only)"""
    env = effective_env(c) if env is None else env
    step, cw, _ = lattice(c)

    def bucket(nseg):
        win = c.W if nseg == 1 else -(-cw // nseg) * step + 2 * c.disp_max + 8
        return next((b for b in (320, 640, 1280, 2560) if win <= b), None)
    split = int(_knob(c, env, "JN_SUPPORT_SPLIT", True) or 0)
    if split >= 1 and bucket(split):
        return bucket(split), split
    per = 64 if 2 * c.disp_max + 8 <= 64 * step else 128
    max_seg = max(1, int(_knob(c, env, "JN_SUPPORT_SEGMENTS", True) or 8))
    for nseg in range(min(max(1, -(-cw // per)), max_seg), max_seg + 1):
        if bucket(nseg):
            return bucket(nseg), nseg
    return (bucket(1), 1) if bucket(1) else None


def dense_row_applies(c):
    p = params(c)
    return p["grid_size"] >= 8 and all(abs(v) <= CELL_PRIOR_MAX for v in priors(p))


def plane_flow(c, env=None):
    env = effective_env(c) if env is None else env
    nbx, nby = -(-c.W // STRIP_W), -(-c.H // TILE_H)
    magic_ok = nbx * nby * c.n * max(nbx, nby) < (1 << 32)
    return support_route(c, env) is not None and dense_row_applies(c) and magic_ok and env.get("JN_DESC_FLOW") != "desc"


def filter_form(c, env=None):
    """support_filters_form: 2 lattice and codes in LDS (k_filter_resolve), 1 the codes only (k_filter_resolve_big), 0 the wavefront alone"""
    env = effective_env(c) if env is None else env
    p = params(c)
    _, cw, ch = lattice(c)
    budget = int(_knob(c, env, "JN_FILTER_LDS_KB", True) or 150) * 1024
    if p["incon_window_size"] != 5 or int(env.get("JN_FILTER_WAVEFRONT") or 0) or not 1 <= p["incon_min_support"] <= 254:
        return 0
    return 2 if (cw + 10) * (ch + 10) * 2 + cw * ch <= budget else (1 if cw * ch <= budget else 0)


def _gap(W, gap_width, corners):
    if corners or gap_width > 64:
        return {"k_gap_rows_any", "k_gap_cols_any"}
    return {"k_gap4<true>", "k_gap4<false>"} if W % 4 == 0 else {"k_gap<true>", "k_gap<false>"}


CCL = {"k_ccl_rows", "k_ccl_merge", "k_ccl_count", "k_ccl_apply"}


def elas_instantiations(c, env=None):
    """The kernels of kernels.hip and delaunay_gpu.hip that the case's batch launches, named as c++filt prints them"""
    env = effective_env(c) if env is None else env
    p = params(c)
    n, W, H = c.n, c.W, c.H
    step, cw, ch = lattice(c)
    knob = lambda name, hook=True: _knob(c, env, name, hook)
    on = lambda name, default, hook=False: int(knob(name, hook)) != 0 if knob(name, hook) is not None else default
    out = set()
    # ---- stage A ----
    plane = plane_flow(c, env)
    out.add("k_sobel_planes" if plane else "k_descriptor_fused")
    route = support_route(c, env)
    out.add("k_support_lds<4, %d, %s>" % (route[0], "true" if plane else "false") if route else "k_support")
    nthreads = min(c.run["host_threads"], max(1, 8 * n * c.run["slots"]))
    form = filter_form(c, env)
    min_batch = nthreads + 1 if knob("JN_HOST_FILTERS", False) is None else ((1 << 30) if int(knob("JN_HOST_FILTERS", False)) else 1)
    filtered = (n >= min_batch or (min_batch < (1 << 30) and form != 0)) and p["incon_window_size"] == 5
    listed = False
    if filtered and form == 2:
        out |= {"k_filter_classify<5>", "k_filter_resolve<5>"}
        listed = on("JN_FUSE_LIST", True, hook=True)
    elif filtered:
        budget = int(knob("JN_FILTER_LDS_KB") or 150) * 1024 // 2
        if (cw + 10) * (ch + 10) > budget and (budget // (ch + 10) - 10 < 8 or budget // (cw + 10) < 1):
            filtered = False
        points = (ch + 5) // 6
        lanes = 16 if points <= 32 else (8 if points <= 64 else 0)
        filtered = filtered and lanes != 0
        if filtered:
            if form == 1:
                out |= {"k_filter_classify<5>", "k_filter_resolve_big<5>"}
            out.add("k_support_filters<5, %d>" % lanes)
    corners = bool(p["add_corners"])
    gpu_arrange = not corners and on("JN_GPU_ARRANGE", True)
    own_stream_a = on("JN_STAGE_A_PRIORITY", False)                     # stage A on a stream of its own (a device with more than one priority)
    gpu_dt = False
    if filtered:
        if not listed:
            out.add("k_support_list")
        # (explicit host_threads below 14: the handle takes the GPU triangulation whatever the machine's cores)
        assert 1 <= c.run["host_threads"] < 14
        gpu_delaunay = on("JN_GPU_DELAUNAY", True) and n > 1 and gpu_arrange and form != 0
        arr_cap = min(cw * ch, 8192)
        arr_stride = min(cw * ch, 16384) if on("JN_ARRANGE_GLOBAL", False, hook=True) else arr_cap
        if gpu_delaunay and cw * ch > DT_WHOLE:
            arr_stride = max(arr_stride, min(cw * ch, 16384))
        gpu_dt = gpu_delaunay and not own_stream_a
        parts = (4 if nthreads >= 8 * n else (2 if nthreads >= 4 * n else 1)) if on("JN_SPLIT_DELAUNAY", True) else 1
        if gpu_arrange and (gpu_dt or parts == 1):
            out.add("k_arrange<1>")
            if arr_stride > arr_cap:                                  # the slot's first batch: the larger forms are launched whatever the sides hold
                done_to = arr_cap
                if arr_cap < 12288:
                    out.add("k_arrange<2>")
                    done_to = min(arr_stride, 12288)
                if arr_stride > done_to:
                    out.add("k_arrange<0>")
            if gpu_dt:
                wide = "true" if W >= 2048 or H >= 2048 else "false"
                out |= {"k_delaunay<%s>" % wide} if cw * ch <= DT_WHOLE else {"k_delaunay_sub<%s>" % wide, "k_delaunay_top<%s>" % wide}
                if int(knob("JN_DT_DUMMY") or 0) in (1, 2, 3, 4):
                    out.add("k_dt_dummy")
    grid_early = filtered and on("JN_GRID_EARLY", True) and not corners and not own_stream_a
    out |= {"k_grid_mark_list" if grid_early else "k_grid_mark", "k_grid_dilate"}
    # ---- stage B ----
    fuse_bin = on("JN_BIN_SETUP", n <= 2, hook=True)
    out |= {"k_bin<true>"} if fuse_bin else {"k_tri_setup", "k_bin<false>"}
    out |= {"k_owner", "k_dense_row<%d>" % (4 if c.disp_max < 128 else 8)} if plane else {"k_dense"}
    both, mean = not p["postprocess_only_left"], bool(p["filter_adaptive_mean"])
    lr = {"k_lr_ccl_rows"} | CCL - {"k_ccl_rows"} if on("JN_LR_CCL_FUSED", True) else {"k_lr"} | CCL
    if p["subsampling"]:
        out |= {"k_lr_sub"} | CCL | _gap(W // 2, p["ipol_gap_width"] // 2 + 1, corners)
        out |= {"k_adaptive_mean_sub<false>", "k_adaptive_mean_sub<true>"} if mean else set()
    else:
        fusable = (on("JN_POST_FUSED", True) and not corners and p["ipol_gap_width"] <= 3 and W >= 16 and H >= 16 and
                   n * W * H >= int(env.get("JN_POST_FUSED_MIN_PIXELS", 10000000)))
        out |= lr
        if fusable and (W * H) & 3 == 0:
            out |= {"k_gap_mean_fused"} | (CCL | {"k_copy_ok"} if both else set())
        else:
            out |= (CCL if both else set()) | _gap(W, p["ipol_gap_width"], corners)
            out |= {"k_adaptive_mean_h4" if W % 4 == 0 else "k_adaptive_mean_h", "k_adaptive_mean_v"} if mean else set()
    if p["filter_median"]:
        out |= {"k_median<true>", "k_median<false>"}
    return out


# ------------------------------------------------------------------ the cases ------------------------------------------------------------------
_B, _BE = prior_edge_betas()
_SMALL = (160, 120, 30, 63, 7)
_NODE = (320, 180, 48, 95, 11)
_BOTH = {"postprocess_only_left": 0}

# the fall-back flow as the parameters choose it: a lone pair on a latency handle, three pairs with both maps on a batch handle
FALLBACK = [(kw, why) for kw, why in (
    ({"grid_size": 1}, "grid_size 1: grid_magic = 0, the kernels divide"),
    ({"grid_size": 4}, "grid_size 4 < 8"),
    ({"grid_size": 7}, "grid_size 7: the largest grid the plane flow refuses"),
    ({"beta": 3e-5}, "beta 3e-5: a prior beyond kCellPriorMax"),
    ({"beta": _B}, "|P[0]| just below 2^19: cost + prior next to the ends of the 24-bit key field"))]
RELEASE_CASES = [case(*_SMALL, 1, kw, "fall-back flow, lone pair; " + why, flow="desc") for kw, why in FALLBACK]
RELEASE_CASES += [case(*_NODE, 3, dict(kw, **_BOTH), "fall-back flow, batch of 3, both maps; " + why, flow="desc", gpu_dt=True) for kw, why in FALLBACK]

_DESC = {"JN_DESC_FLOW": "desc"}
RELEASE_CASES += [case(320, 240, 40, 79, 21, 1, kw, "JN_DESC_FLOW=desc: k_dense under " + why, flow="desc", env=_DESC) for kw, why in (
    ({"disp_min": 6}, "disp_min 6"), ({"disp_min": -5}, "a negative disp_min"), ({"match_texture": 5, "lr_threshold": 1}, "match_texture 5"),
    ({"grid_size": 16, "sradius": 3.0}, "radius 3 on a grid of 16"))]
RELEASE_CASES += [
    case(320, 240, 40, 79, 21, 1, {"subsampling": 1}, "JN_DESC_FLOW=desc with subsampling: k_lr_sub and the half-size passes", flow="desc", env=_DESC),
    case(320, 180, 48, 127, 3, 1, {}, "JN_DESC_FLOW=desc at disp_max 127", flow="desc", env=_DESC),
    case(320, 180, 48, 255, 12345, 1, {}, "JN_DESC_FLOW=desc at disp_max 255: the widest LDS rows of k_dense", flow="desc", env=_DESC),
    case(333, 201, 30, 95, 5, 1, _BOTH, "JN_DESC_FLOW=desc on a ragged frame, two segments in the 640 bucket; odd W * H: the unfused passes, k_gap / k_adaptive_mean_h",
         flow="desc", env=_DESC),
    case(300, 160, 30, 63, 4, 1, {}, "JN_DESC_FLOW=desc, pitch 352 > width 300", flow="desc", env=_DESC, pad=52),
    case(*_NODE, 4, _BOTH, "JN_DESC_FLOW=desc, frame 2 of 4 fails: k_dense meets info.ok == 0", flow="desc", env=_DESC, noise=2, gpu_dt=True),
    case(*_NODE, 3, {"grid_size": 4}, "the parameter-chosen fall-back with a failing frame on the host route", flow="desc", env={"JN_GPU_DELAUNAY": "0"}, noise=0),
]

# create-time and per-batch switches, in-process
RELEASE_CASES += [
    case(*_NODE, 1, _BOTH, "JN_POST_FUSED=0 on a lone pair: k_gap4, k_adaptive_mean_h4", env={"JN_POST_FUSED": "0"}),
    case(*_NODE, 3, _BOTH, "JN_POST_FUSED=0 on a batch", env={"JN_POST_FUSED": "0"}, gpu_dt=True),
    case(*_NODE, 1, {}, "JN_SPLIT_DELAUNAY=0 with 2 pool threads: k_arrange feeds the host", env={"JN_SPLIT_DELAUNAY": "0"}, host_threads=2),
    case(*_NODE, 1, {}, "JN_SPLIT_DELAUNAY=0 with 8 pool threads (4 parts by default)", env={"JN_SPLIT_DELAUNAY": "0"}, host_threads=8),
    case(*_NODE, 1, {}, "8 pool threads: every side in 4 parts, no device arrangement", host_threads=8),
    case(*_NODE, 1, {}, "4 pool threads: every side in 2 parts", host_threads=4),
    case(*_NODE, 1, {}, "JN_ZERO_COPY=0 on a latency handle: payload copied, stage B not gated", env={"JN_ZERO_COPY": "0"}),
    case(*_NODE, 3, _BOTH, "JN_ZERO_COPY=1 on a batch handle, host route", env={"JN_ZERO_COPY": "1", "JN_GPU_DELAUNAY": "0"}),
    case(*_NODE, 3, {}, "JN_ZERO_COPY=1 on a batch handle, GPU triangulation", env={"JN_ZERO_COPY": "1"}, gpu_dt=True),
    case(*_NODE, 3, {}, "JN_STAGE_EVENTS=0 on a batch handle", env={"JN_STAGE_EVENTS": "0"}, gpu_dt=True),
    case(*_NODE, 1, {}, "JN_STAGE_EVENTS=1 on a latency handle", env={"JN_STAGE_EVENTS": "1"}),
    case(*_NODE, 3, _BOTH, "JN_STAGE_A_PRIORITY=1, two slots in flight: stage A on its own stream, host route, grid in stage B",
         env={"JN_STAGE_A_PRIORITY": "1"}, slots=2, gpu_dt=True),      # (the handle would triangulate on the GPU; a batch whose stage A has its own stream does not)
    case(*_NODE, 1, {}, "JN_WAIT_SPIN_US=0 and JN_POOL_SPIN_US=0 on a latency handle", env={"JN_WAIT_SPIN_US": "0", "JN_POOL_SPIN_US": "0"}),
    case(*_NODE, 3, {}, "JN_WAIT_SPIN_US=0 and JN_POOL_SPIN_US=0 on the host route of a batch handle",
         env={"JN_WAIT_SPIN_US": "0", "JN_POOL_SPIN_US": "0", "JN_GPU_DELAUNAY": "0"}),
    case(*_NODE, 1, {}, "JN_GATE_STAGE_B=0: stage B queued after the host stage", env={"JN_GATE_STAGE_B": "0"}),
    case(*_NODE, 1, {}, "JN_HOST_FILTERS=1: filters and list on the host pool, k_grid_mark", env={"JN_HOST_FILTERS": "1"}),
    case(*_NODE, 1, {}, "JN_GPU_ARRANGE=0 with one task per side", env={"JN_GPU_ARRANGE": "0"}, host_threads=2),
]

# the parameter-driven forms
RELEASE_CASES += [
    case(*_SMALL, 1, {}, "320 bucket, one segment; k_dense_row<4>, k_bin<true>"),
    case(*_SMALL, 3, _BOTH, "batch of 3: k_tri_setup + k_bin<false>, k_delaunay<false>, k_copy_ok", gpu_dt=True),
    case(333, 201, 30, 95, 5, 2, {}, "640 bucket, two segments, plane flow; a batch of 2 keeps k_bin<true>", gpu_dt=True),
    case(1300, 48, 40, 255, 9, 1, {}, "1280 bucket, three segments of 87 candidates; k_dense_row<8>"),
    case(1300, 48, 40, 255, 9, 1, {}, "1280 bucket, materialised descriptors", flow="desc", env=_DESC),
    case(1300, 100, 40, 255, 9, 1, {"candidate_stepsize": 21}, "2560 bucket: 62 candidates a row in one segment, window = W = 1300"),
    case(1300, 100, 40, 255, 9, 1, {"candidate_stepsize": 21}, "2560 bucket, materialised descriptors", flow="desc", env=_DESC),
    case(2600, 40, 40, 63, 3, 1, {}, "2600 columns: eight segments of 65 candidates in the 640 bucket"),
    case(2600, 40, 40, 63, 3, 2, {}, "2600 columns on a batch handle: k_delaunay<true> (integer predicates from 2048 columns on)", gpu_dt=True),
    case(2600, 64, 40, 63, 3, 2, {}, "2600x64: 6760 lattice points a side, k_delaunay_sub<true> + k_delaunay_top<true>", gpu_dt=True),
    case(*_NODE, 2, {"candidate_stepsize": 3}, "lattice of 6420 points: k_delaunay_sub<false> + k_delaunay_top<false>", gpu_dt=True),
    case(*_NODE, 2, {"candidate_stepsize": 2}, "lattice of 14400 points: the first batch launches k_arrange<2> and k_arrange<0>", gpu_dt=True),
    case(320, 180, 48, 63, 11, 1, {"candidate_stepsize": 1}, "lattice 320x180: the codes fit the LDS, the lattice does not: k_filter_resolve_big, k_support_filters<5, 16>"),
    case(256, 200, 40, 63, 11, 1, {"candidate_stepsize": 1}, "lattice 256x200: k_filter_resolve_big, 34 points a wavefront step: k_support_filters<5, 8>"),
    case(*_NODE, 1, {"incon_min_support": 0}, "min_support 0: outside what classification takes, the wavefront kernel alone (JN_HOST_FILTERS=0 keeps a lone pair on the GPU)",
         env={"JN_HOST_FILTERS": "0"}),
    case(*_NODE, 1, {"incon_window_size": 3, "incon_min_support": 3}, "a window the kernels do not take: host filters"),
    case(322, 180, 48, 95, 11, 1, _BOTH, "W % 4 != 0 under the library's own threshold: k_gap, k_adaptive_mean_h", env=UNFUSED),
    case(*_NODE, 1, _BOTH, "W % 4 == 0 under the library's own threshold: k_gap4, k_adaptive_mean_h4", env=UNFUSED),
    case(161, 121, 30, 63, 7, 3, _BOTH, "odd W * H: no fused pass, no k_copy_ok, whatever the threshold", gpu_dt=True),
    case(*_NODE, 1, dict(_BOTH, ipol_gap_width=100), "ipol_gap_width 100 without corners: k_gap_rows_any, k_gap_cols_any"),
    case(*_NODE, 1, dict(_BOTH, ipol_gap_width=7, filter_adaptive_mean=0, filter_median=1), "gap width 7: not fusable; median instead of the mean"),
    case(*_NODE, 1, {"add_corners": 1}, "corner points: host arrangement, k_grid_mark, k_gap_rows_any"),
    case(*_NODE, 1, {"subsampling": 1}, "subsampling: k_lr_sub, k_adaptive_mean_sub, half-size gap"),
    case(324, 180, 48, 95, 11, 1, dict(_BOTH, subsampling=1, filter_median=1), "subsampling, half width 162: k_gap on the half-size maps, median"),
]

# switches read once per process: fresh children of the release library
RELEASE_CASES += [
    case(*_NODE, 1, _BOTH, "JN_LR_CCL_FUSED=0: k_lr + k_ccl_rows, fused pass behind", child="lr_ccl_split"),
    case(*_NODE, 3, _BOTH, "JN_LR_CCL_FUSED=0 on a batch, unfused passes behind", env=UNFUSED, child="lr_ccl_split", gpu_dt=True),
    case(*_NODE, 1, {}, "JN_GRID_EARLY=0 on a lone pair: the grid from the host stage's payload", child="grid_late"),
    case(*_NODE, 3, _BOTH, "JN_GRID_EARLY=0 on the GPU route: the grid from k_delaunay's payload", child="grid_late", gpu_dt=True),
    case(*_NODE, 1, {}, "JN_FILTER_WAVEFRONT=1: k_support_filters<5, 16> sweeps and removes", child="wavefront"),
    case(*_NODE, 3, _BOTH, "JN_FILTER_WAVEFRONT=1 on a batch: no GPU triangulation without the fast filters", child="wavefront"),
]

HOOKS_CASES = [case(*_NODE, 1, {}, "JN_SUPPORT_SPLIT=%d" % k, env={"JN_SUPPORT_SPLIT": str(k)}, hooks=True) for k in (1, 2, 5)]
HOOKS_CASES += [
    case(*_NODE, 3, _BOTH, "JN_SUPPORT_SPLIT=5 on a batch", env={"JN_SUPPORT_SPLIT": "5"}, hooks=True, gpu_dt=True),
    case(1300, 48, 40, 255, 9, 1, {}, "JN_SUPPORT_SPLIT=1 at 1300 columns: the 2560 bucket holds the whole row", env={"JN_SUPPORT_SPLIT": "1"}, hooks=True),
    case(*_NODE, 1, {"candidate_stepsize": 2}, "JN_ARRANGE_GLOBAL=1 on the host route: lattice of 14400, one task per side", env={"JN_ARRANGE_GLOBAL": "1"}, hooks=True,
         host_threads=2),
    case(2600, 40, 40, 63, 3, 1, {}, "JN_SUPPORT_SEGMENTS=1 at 2600 columns: no bucket, materialised descriptors, k_support", flow="desc", child="hooks_a"),
    case(*_NODE, 1, _BOTH, "JN_FUSE_LIST=0, JN_BIN_SETUP=0 at n = 1, JN_DENSE_XCD_ORDER=0, JN_POST_BAND=8: 23 bands, the last of 4 rows", child="hooks_a"),
    case(*_NODE, 3, _BOTH, "the same at n = 3, behind k_dt_dummy", child="hooks_a", gpu_dt=True),
    case(*_NODE, 3, {"grid_size": 4}, "JN_DENSE_XCD_ORDER=0 under k_dense", flow="desc", child="hooks_a", gpu_dt=True),
    case(*_NODE, 1, _BOTH, "JN_BIN_SETUP=1 at n = 1, JN_POST_BAND=24: 8 bands of 24 rows, the last of 12", child="hooks_b"),
    case(*_NODE, 3, _BOTH, "JN_BIN_SETUP=1 at n = 3: k_bin<true> on a batch", child="hooks_b", gpu_dt=True),
    case(*_NODE, 3, _BOTH, "JN_POST_BAND=1000: one band", child="hooks_c", gpu_dt=True),
]
ALL_CASES = RELEASE_CASES + HOOKS_CASES
BY_ID = {case_id(c): c for c in ALL_CASES}

# In the release binary, reachable through no parameter set or shipped switch of the release library.  name: reason
UNREACHABLE_IN_RELEASE = {
    "k_support": "needs candidate_stepsize > 2042 on a frame wider than 2560 columns (five lattice columns at most: support points enough only on frames of "
                 "tens of megapixels); otherwise up to eight segments always fit a bucket, and only the hooks build's JN_SUPPORT_SEGMENTS caps them",
}


def table_instantiations(cases):
    return set().union(*(elas_instantiations(c) for c in cases))
