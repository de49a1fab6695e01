"""tests/scan_def.py (the mono8 node tail in numpy, what tests/test_gpu_rigs.py checks the kernels with) pinned to oracle/node_oracle.cpp
(the restatement read against point_cloud.cpp) under every rig of tests/rigs.py: the u8 map, the valid-disparity table and the cloud bit for
bit, the bins equal wherever no bearing sits on a bin edge, the extrema within SCAN_TOL.  CPU only."""
import numpy as np
import pytest

import rigs
import scan_def as sdef
from subpix_check import MARGIN, SCAN_TOL          # the project's scan tolerance and bin-edge margin: one definition

SHAPES = [(200, 37), (321, 49), (257, 17), (1, 33), (513, 1)]
N = 3


def test_to_u8_on_the_values_that_decide_it(oracle):
    v = rigs.decisive_floats()
    got = sdef.to_u8(v)
    assert np.array_equal(got, oracle.to_u8(v))
    by = dict(zip(v.tolist(), got.tolist()))
    assert [by[x] for x in (0.5, 1.5, 2.5, 254.5, 255.5, -0.5, 256.0, 1e9, -1e9, -10.0)] == [0, 2, 2, 254, 255, 0, 255, 255, 0, 0]
    assert by[float(np.float32(255.49998))] == 255 and by[float(np.float32(1 - 2.0 ** -10))] == 1 and by[float(np.float32(0.5 + 2.0 ** -10))] == 1
    assert sdef.to_u8(np.array([np.inf, -np.inf], np.float32)).tolist() == [255, 0]


@pytest.mark.parametrize("name", rigs.NAMES)
def test_the_definition_equals_the_oracle(oracle, same, name):
    left_out = frames = 0
    reached = None
    for W, H in SHAPES:
        rng = np.random.default_rng(1000 + 7 * W + H)
        sp = rigs.apply(name, oracle.scan_params(W, H), W, H)
        D = rigs.float_maps(rng, N, H, W)
        u8 = sdef.to_u8(D)
        assert same(u8, oracle.to_u8(D)), (name, W, H)
        lut = sdef.valid_lut(sp, W, H)
        assert same(lut, oracle.valid_lut(sp, W, H)), (name, W, H)
        for f in range(N):
            want = oracle.point_cloud(sp, u8[f])
            got, nz = sdef.cloud(sp, u8[f]), sdef.cloud_w_nonzero(sp, u8[f])
            assert got.shape == (int((u8[f] >= 2).sum()), 3) and same(got[nz], want), (name, W, H, f)        # the oracle leaves the w = 0 pixels out
            assert not got[~nz].any(), (name, W, H, f)
            for flavour, mine, theirs in (("lut", sdef.scan(sp, u8[f], lut), oracle.scan(sp, u8[f], lut)),
                                          ("cloud", sdef.scan_cloud(sp, u8[f]), oracle.scan_cloud(sp, u8[f]))):
                bins, meta, edge = mine
                frames += 1
                if edge > MARGIN:
                    assert np.array_equal(bins < sdef.EMPTY - 1, theirs[0] < sdef.EMPTY - 1), (name, W, H, f, flavour)
                    assert np.allclose(bins, theirs[0], rtol=0, atol=SCAN_TOL), (name, W, H, f, flavour)
                else:
                    left_out += 1
                assert np.allclose(meta, theirs[1], rtol=0, atol=SCAN_TOL), (name, W, H, f, flavour)
        if (W, H) == SHAPES[0]:
            reached = rigs.facts(sp, u8, lut)
    assert 20 * left_out <= frames, (left_out, frames)
    assert rigs.REACHES[name](reached), {k: v for k, v in reached.items() if k != "bins_hit"}


def test_the_rigs_differ_and_the_table_wraps_where_the_row_says(oracle):
    """No two rigs give the same table and scan; the 256 -> 0 wrap and the Z < 0 rejection fire under rigs other than the default one."""
    W, H = 200, 37
    rng = np.random.default_rng(5)
    u8 = rigs.u8_maps(rng, 1, H, W)
    seen = {}
    for name in rigs.NAMES:
        sp = rigs.apply(name, oracle.scan_params(W, H), W, H)
        lut = sdef.valid_lut(sp, W, H)
        bins, meta, _ = sdef.scan_cloud(sp, u8[0])
        seen[name] = (lut.tobytes(), bins.tobytes(), meta.tobytes())
        f = rigs.facts(sp, u8, lut)
        if name == "gp_steep":
            assert (lut[H - 8:, :, 0] == 0).all()
        if name in ("rear_fov360", "rolled90"):
            assert 0 < f["lut_z_negative"] != rigs.facts(rigs.apply("default", oracle.scan_params(W, H), W, H), u8, lut)["lut_z_negative"], name
    assert len(set(seen.values())) == len(rigs.NAMES)
