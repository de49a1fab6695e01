"""One case of tests/elas_cases.py through the package, as tests/test_gpu_elas_matrix.py and tests/mocks/elas_route_worker.py run it: the caller has
the case's environment and library in place.  Outputs are pre-filled with FILL, so a frame the library leaves alone shows."""
import ctypes as C

import numpy as np

FILL = -7.0


def parameters(jn, c):
    return jn.Elas.parameters(0, disp_max=c.disp_max, **c.kw)


def run_case(jn, c, Ls, Rs):
    """-> (status [n], outs: per slot (D1 [n][H][W], D2), route_stats of slot 0 after the batch)"""
    from jackal_navigation_amd.device import DeviceArray
    n, H, W = Ls.shape
    p, slots = parameters(jn, c), c.run["slots"]
    if n == 1:
        pitch = W + c.run.get("pad", 0)
        Lp, Rp = np.full((H, pitch), 200, np.uint8), np.full((H, pitch), 17, np.uint8)        # garbage in the padding must not matter
        Lp[:, :W], Rp[:, :W] = Ls[0], Rs[0]
        D1, D2 = np.full((1, H, W), FILL, np.float32), np.full((1, H, W), FILL, np.float32)
        with jn.Elas(p, W, H, host_threads=c.run["host_threads"]) as e:
            st = e.process(Lp, Rp, D1[0], D2[0], (W, H, pitch))
            return [st], [(D1, D2)], e.route_stats(0)
    dL, dR = DeviceArray.from_numpy(Ls), DeviceArray.from_numpy(Rs)
    fill = np.full((n, H, W), FILL, np.float32)
    bufs = [(DeviceArray.from_numpy(fill), DeviceArray.from_numpy(fill), (C.c_int32 * n)()) for _ in range(slots)]
    try:
        with jn.Elas(p, W, H, max_batch=n, host_threads=c.run["host_threads"], slots=slots) as e:
            for s, (d1, d2, st) in enumerate(bufs):
                e.submit(s, n, dL.ptr, dR.ptr, W, H * W, d1.ptr, d2.ptr, st)
            for s in range(slots):
                e.wait(s)
            stats = e.route_stats(0)
        assert all(list(st) == list(bufs[0][2]) for _, _, st in bufs), "the slots disagree about the frames' status"
        return list(bufs[0][2]), [(d1.numpy(), d2.numpy()) for d1, d2, _ in bufs], stats
    finally:
        for a in [dL, dR] + [b for d1, d2, _ in bufs for b in (d1, d2)]:
            a.free()


def expected(oracle, c, Ls, Rs):
    """-> (status [n], D1 [n][H][W], D2) of the CPU oracle, in the layout the library writes: a failed frame keeps FILL, a half-size map (subsampling)
    lies at the start of its frame's buffer"""
    n, H, W = Ls.shape
    po = oracle.params(0, disp_max=c.disp_max, **c.kw)
    st, D1, D2 = [], np.full((n, H, W), FILL, np.float32), np.full((n, H, W), FILL, np.float32)
    for b in range(n):
        s, a1, a2 = oracle.process(po, Ls[b], Rs[b], fill=FILL)
        st.append(int(s))
        if s == 0:
            D1[b].reshape(-1)[:a1.size] = a1.reshape(-1)
            D2[b].reshape(-1)[:a2.size] = a2.reshape(-1)
    return st, D1, D2
