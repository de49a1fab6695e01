"""The camera-to-robot transform XR / XT of a rig from a few frames of flat floor — the replacement of the reference README's step 3
(identity and zero, `point_cloud -g -m`, six rqt_reconfigure sliders turned until the ground lines up in rviz):

    python3 scripts/ground_calibrate.py rig.yml --left l0.npy l1.npy --right r0.npy r1.npy [--rectified] [--size 640x360] [--write out.yml]
    python3 scripts/ground_calibrate.py rig.yml --disparity d0.npy d1.npy [--write out.yml]

rig.yml is the OpenCV calibration file the reference reads (K1, K2, D1, D2, R, T and, optionally, XR, XT; include/jn_calib.h).  Frames are
grey images ([H][W] uint8 .npy, or .jpg / .jpeg); raw frames at the calibrated size are undistorted and rectified to --size first, --rectified
says they already are at --size.  --disparity takes float32 maps of the rectified left image instead (pixels, invalid < 0).
Frames -> ELAS -> jn_ground_estimate (a plane fit per frame, on the GPU) -> jn_ground_extrinsics (the joint fit next to a prior).
The prior: the file's XR / XT with --prior file; by default the nominal forward-looking camera (jn_ground_nominal_prior) when the file has
no XR / XT or has the README's identity / zero, else the file's.  A floor fixes roll, pitch and height: yaw and XT.x / XT.y stay the prior's.
Prints one JSON line (XR, XT, tilt from the prior, height, inlier share and rms per frame); --write saves the calibration with the new XR / XT."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import jackal_navigation_amd as jn  # noqa: E402
from jackal_navigation_amd import calib, ground, node  # noqa: E402
from jackal_navigation_amd.device import DeviceArray  # noqa: E402


def load_grey(path):
    """-> DeviceArray [H][W] uint8."""
    if path.lower().endswith((".jpg", ".jpeg")):
        return node.imdecode_gray(open(path, "rb").read())
    a = np.load(path)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise SystemExit("%s: expected a [H][W] uint8 array, got %s %s" % (path, a.shape, a.dtype))
    return DeviceArray.from_numpy(a)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("calibration")
    ap.add_argument("--left", nargs="+", default=[])
    ap.add_argument("--right", nargs="+", default=[])
    ap.add_argument("--disparity", nargs="+", default=[])
    ap.add_argument("--rectified", action="store_true")
    ap.add_argument("--calib-size", default="640x360", help="the size the rig was calibrated at (not in the file)")
    ap.add_argument("--size", default=None, help="working size WxH (default: the calibrated size)")
    ap.add_argument("--prior", choices=("auto", "file", "nominal"), default="auto")
    ap.add_argument("--max-tilt", type=float, default=30.0)
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--disp-max", type=int, default=255)
    ap.add_argument("--write", default=None)
    a = ap.parse_args()
    if bool(a.disparity) == bool(a.left) or len(a.left) != len(a.right):
        raise SystemExit("give --left and --right (as many of each), or --disparity")
    cw, ch = (int(v) for v in a.calib_size.split("x"))
    W, H = (int(v) for v in (a.size or a.calib_size).split("x"))
    c, XR_file, XT_file, present = jn.load_calibration(a.calibration, cw, ch)
    has_extrinsics = bool(present & calib.XR) and not (np.array_equal(XR_file, np.eye(3)) and not XT_file.any())
    use_file = a.prior == "file" or (a.prior == "auto" and has_extrinsics)
    XR0, XT0 = (XR_file, XT_file) if use_file else ground.nominal_prior()
    rect = node.stereo_rectify(c, W, H)
    sp = node.scan_params(W, H)
    sp.Q[:] = list(rect.Q)
    sp.XR[:] = np.asarray(XR0).reshape(-1).tolist()
    sp.XT[:] = np.asarray(XT0).tolist()
    if a.disparity:
        maps = np.stack([np.load(p).astype(np.float32) for p in a.disparity])
        if maps.shape[1:] != (H, W):
            raise SystemExit("the disparity maps are %s, --size says %dx%d" % (maps.shape[1:], W, H))
    else:
        remaps = None
        if not a.rectified:
            remaps = [node.init_undistort_rectify_map(list(K), list(D), list(Rr), list(P), W, H)
                      for K, D, Rr, P in ((c.K1, c.D1, rect.R1, rect.P1), (c.K2, c.D2, rect.R2, rect.P2))]
        maps = np.zeros((len(a.left), H, W), np.float32)
        D2 = np.zeros((H, W), np.float32)
        with jn.Elas(jn.Elas.parameters(jn.Elas.ROBOTICS, disp_max=a.disp_max), W, H) as e:
            for i, (pl, pr) in enumerate(zip(a.left, a.right)):
                eyes = []
                for eye, path in enumerate((pl, pr)):
                    raw = load_grey(path)
                    if a.rectified:
                        if raw.shape != (H, W):
                            raise SystemExit("%s is %s, --size says %dx%d" % (path, raw.shape, W, H))
                        eyes.append(raw.numpy())
                    else:
                        out = DeviceArray((H, W), np.uint8)
                        sh, sw = raw.shape
                        node.remap(1, raw.ptr, sw, sh, sw, sw * sh, remaps[eye][0].ptr, remaps[eye][1].ptr, out.ptr, W, H, W, W * H)
                        eyes.append(out.numpy())
                st = e.process(eyes[0], eyes[1], maps[i], D2, (W, H, W))
                if st != 0:
                    maps[i] = -10.0                              # too few support points: the frame has no floor to offer
    gp = ground.ground_params(W, H, hypotheses=a.hypotheses)
    d = DeviceArray.from_numpy(maps)
    planes = ground.estimate(sp, gp, maps.shape[0], d.ptr, ground.F32, W, H)
    frames = [{"status": p.status, "inlier_share": round(p.inliers / max(1, p.valid), 4), "rms_px": round(p.rms, 4),
               "height_m": round(p.height_m, 5), "plane_px": [p.a, p.b, p.c]} for p in planes]
    try:
        XR, XT, tilt = ground.extrinsics(planes, sp, a.max_tilt)
    except jn.JnError as err:
        print(json.dumps({"script": "scripts/ground_calibrate.py", "error": str(err), "frames": frames}))
        raise SystemExit(2)
    line = {"script": "scripts/ground_calibrate.py", "size": [W, H], "prior": "file" if use_file else "nominal", "frames_ok": sum(1 for p in planes if p.status == 0),
            "XR": XR.reshape(-1).tolist(), "XT": XT.tolist(), "tilt_from_prior_deg": round(tilt, 4), "height_m": round(float(XT[2]), 5), "frames": frames}
    if a.write:
        jn.save_calibration(a.write, c, XR, XT)
        line["written"] = a.write
    print(json.dumps(line))


if __name__ == "__main__":
    main()
