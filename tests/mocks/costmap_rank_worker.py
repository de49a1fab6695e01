"""One rank of tests/test_gpu_costmap.py::test_two_ranks_merge_their_grids (TEST INFRASTRUCTURE).  Builds the costmap of ITS OWN two
frames (jn_obstacle_costmap on maps only this rank has), then merges scan and grid across the ranks with the one-call forms
(jn_scan_allreduce, jn_costmap_allreduce) and leaves what it saw in out_dir.
    python costmap_rank_worker.py <rank> <world> <out_dir>
JN_RCCL_LIB points at tests/mocks/fake_rccl.cpp's library: both ranks share device 0."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
rank, world, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
W, H, N = 320, 180, 2
CP = dict(cells_x=64, cells_y=64, resolution=0.1, origin_x=0.0, origin_y=-3.2, min_hits=2, from_cloud=0)    # N * 64 * 64 = 8192 elements


def main():
    import jackal_navigation_amd as jn
    from jackal_navigation_amd import costmap, node, parallel
    from jackal_navigation_amd.device import DeviceArray
    jn.load()
    sp = node.scan_params(W, H)
    lut = node.build_valid_disp_lut(sp, W, H)
    cp = costmap.costmap_params(**CP)
    rng = np.random.default_rng(100 + rank)
    maps = rng.integers(0, 40, (N, H, W)).astype(np.uint8)
    for f in range(N):
        for _ in range(10):                                      # faces at one depth: the cells that get many hits
            x0, y0 = int(rng.integers(0, W - 40)), int(rng.integers(0, H - 30))
            maps[f, y0:y0 + 30, x0:x0 + 40] = rng.integers(8, 60)
    dD = DeviceArray.from_numpy(maps)
    bins = DeviceArray((N, sp.bins), np.float64); meta = DeviceArray((N, 4), np.float64)
    node.obstacle_scan(sp, N, dD.ptr, lut.ptr, W, H, bins.ptr, meta.ptr)
    hits = DeviceArray((N, cp.cells_y, cp.cells_x), np.uint16); grid = DeviceArray((N, cp.cells_y, cp.cells_x), np.int8)
    costmap.obstacle_costmap(sp, cp, N, dD.ptr, lut.ptr, W, H, bins.ptr, hits.ptr, grid.ptr)
    for name, a in (("local_hits", hits), ("local_grid", grid), ("local_bins", bins)):
        np.save(os.path.join(out_dir, "%s%d.npy" % (name, rank)), a.numpy())

    def id_exchange(raw):
        path = os.path.join(out_dir, "comm_id.bin")
        if raw is not None:
            with open(path + ".tmp", "wb") as f:
                f.write(raw)
            os.replace(path + ".tmp", path)
            return raw
        t0 = time.time()
        while not os.path.exists(path):
            if time.time() - t0 > 60:
                raise RuntimeError("rank 0 never wrote the communicator id")
            time.sleep(0.01)
        return open(path, "rb").read()

    comm = parallel.ScanComm(rank, world, 0, id_exchange)
    info = comm.info()
    comm.merge(N, sp.bins, bins.ptr, meta.ptr)                   # the robot-level scan first: the grid's free cells come from it
    costmap.allreduce(comm, sp, cp, N, bins.ptr, hits.ptr, grid.ptr)
    comm.close()
    for name, a in (("merged_hits", hits), ("merged_grid", grid), ("merged_bins", bins)):
        np.save(os.path.join(out_dir, "%s%d.npy" % (name, rank)), a.numpy())
    json.dump({"info": list(info), "size": [W, H], "cp": CP}, open(os.path.join(out_dir, "report%d.json" % rank), "w"))


main()
