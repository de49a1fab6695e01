"""Create / use / destroy handles (ELAS, then SGM and block matching with all their slots) repeatedly and from several threads; device memory
must come back."""
import os, sys, threading
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jackal_navigation_amd as jn
import torch

def free_mb():
    f, t = torch.cuda.mem_get_info(0)
    return f / 2**20

W, H = 640, 360
L, R = jn.node.synth_pair(W, H, 64, 5)
base = None
for it in range(25):
    D1 = np.zeros((H, W), np.float32); D2 = np.zeros((H, W), np.float32)
    with jn.Elas(jn.Elas.parameters(0, disp_max=95), W, H, max_batch=4, slots=3, host_threads=4) as e:
        assert e.process(L, R, D1, D2, (W, H, W)) == 0
    if it == 2:
        base = free_mb()
print("free MB after 3 cycles %.0f, after 25 cycles %.0f" % (base, free_mb()))
assert abs(free_mb() - base) < 64, "device memory leak"
ref = D1.copy()

def worker(k, out):
    Da = np.zeros((H, W), np.float32); Db = np.zeros((H, W), np.float32)
    with jn.Elas(jn.Elas.parameters(0, disp_max=95), W, H, max_batch=2, slots=2, host_threads=2) as e:
        for _ in range(10):
            assert e.process(L, R, Da, Db, (W, H, W)) == 0
    out[k] = np.array_equal(Da, ref)

res = {}
ths = [threading.Thread(target=worker, args=(k, res)) for k in range(4)]
[t.start() for t in ths]; [t.join() for t in ths]
print("4 handles used from 4 threads concurrently:", res)
assert all(res.values())
# The same for the SGM handle, plain and with the census cost (its slots also own a cost volume and signatures): a scan batch on every slot
# (the slots beyond 0 are made when they are first used), then destroy.
from jackal_navigation_amd.device import DeviceArray
sp = jn.node.scan_params(W, H)
lut = jn.node.build_valid_disp_lut(sp, W, H)
dL = DeviceArray.from_numpy(L[None]); dR = DeviceArray.from_numpy(R[None])
S = 8
dd = [DeviceArray((1, H, W), np.int16) for _ in range(S)]; u8 = [DeviceArray((1, H, W), np.uint8) for _ in range(S)]
bins = [DeviceArray((1, sp.bins), np.float64) for _ in range(S)]; meta = [DeviceArray((1, 4), np.float64) for _ in range(S)]
from jackal_navigation_amd import sgm as _sgm
for cost, name in ((None, "SGM"), (jn.Sgm.cost_parameters(cost_function=_sgm.SGM_COST_CENSUS, block_radius=4), "SGM census")):
    base = None
    for it in range(25):
        with jn.Sgm(jn.Sgm.parameters(num_disparities=64), W, H, max_batch=1, cost=cost) as m:
            for s in range(S):
                m.submit_scan(s, 1, dL.ptr, dR.ptr, W, H * W, dd[s].ptr, sp, lut.ptr, u8[s].ptr, bins[s].ptr, meta[s].ptr)
            for s in range(S):
                m.wait(s)
        if it == 2:
            base = free_mb()
            ref_sgm = dd[0].numpy().copy()
    print("%s, 8 slots: free MB after 3 cycles %.0f, after 25 cycles %.0f" % (name, base, free_mb()))
    assert abs(free_mb() - base) < 64, "device memory leak (%s)" % name
    assert all(np.array_equal(d.numpy(), ref_sgm) for d in dd), "%s slots disagree" % name
# And the block-matching handle, the sum of absolute differences and the matrix cores' squared differences: its six slots.
S = 6
for cost, name in ((0, "SAD"), (1, "SSD")):
    base = None
    for it in range(25):
        with jn.Bm(jn.Bm.parameters(num_disparities=64, cost_function=cost), W, H, max_batch=1) as m:
            for s in range(S):
                m.submit_scan(s, 1, dL.ptr, dR.ptr, W, H * W, dd[s].ptr, sp, lut.ptr, u8[s].ptr, bins[s].ptr, meta[s].ptr)
            for s in range(S):
                m.wait(s)
        if it == 2:
            base = free_mb()
            ref_bm = dd[0].numpy().copy()
    print("BM %s, 6 slots: free MB after 3 cycles %.0f, after 25 cycles %.0f" % (name, base, free_mb()))
    assert abs(free_mb() - base) < 64, "device memory leak (BM %s)" % name
    assert all(np.array_equal(d.numpy(), ref_bm) for d in dd[:S]), "BM slots disagree"
print("lifecycle OK")
