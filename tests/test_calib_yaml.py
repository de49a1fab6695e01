"""The calibration file (include/jn_calib.h): the OpenCV FileStorage YAML subset, read and written without OpenCV.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("K1", "K2", "D1", "D2", "R", "T")


def _matrix(name, rows, cols, vals, per_line=3, dt="d"):
    body = ""
    for i, v in enumerate(vals):
        body += repr(float(v)) + (", " if i + 1 < len(vals) else " ")
        if i % per_line == per_line - 1 and i + 1 < len(vals):
            body += "\n       "
    return "%s: !!opencv-matrix\n   rows: %d\n   cols: %d\n   dt: %s\n   data: [ %s]\n" % (name, rows, cols, dt, body)


def _text(c, XR=None, XT=None, per_line=3, **replace):
    parts = {"K1": _matrix("K1", 3, 3, c.K1, per_line), "K2": _matrix("K2", 3, 3, c.K2, per_line), "D1": _matrix("D1", 1, 5, c.D1, per_line),
             "D2": _matrix("D2", 1, 5, c.D2, per_line), "R": _matrix("R", 3, 3, c.R, per_line), "T": _matrix("T", 3, 1, c.T, per_line)}
    if XR is not None:
        parts["XR"] = _matrix("XR", 3, 3, XR, per_line)
    if XT is not None:
        parts["XT"] = _matrix("XT", 3, 1, XT, per_line)
    parts.update(replace)
    return "%YAML:1.0\n" + "".join(v for v in parts.values() if v)


def _same(a, b):
    return all(bytes(getattr(a, k)) == bytes(getattr(b, k)) for k in FIELDS)


def test_header_symbols_are_exported_by_both_libraries(jn):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "jn_calib.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(jn_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(jn.CALIB_EXPORTS) == ["jn_calib_load_yaml", "jn_calib_save_yaml"]
    lib = jn.load()
    assert not [n for n in declared if not hasattr(lib, n)]
    with jn.hooks_library() as hooks:
        assert not [n for n in declared if not hasattr(hooks, n)]
    from jackal_navigation_amd import calib
    hdr = open(os.path.join(ROOT, "include", "jn_calib.h")).read()
    for name in ("K1", "K2", "D1", "D2", "R", "T", "XR", "XT", "STEREO"):
        assert int(re.search(r"#define JN_CALIB_%s (\d+)" % name, hdr).group(1)) == getattr(calib, name)


def test_a_text_written_from_the_defaults_loads_back_bit_for_bit(jn, tmp_path):
    from jackal_navigation_amd import node, calib
    d = node.stereo_calib()
    sp = node.scan_params(640, 360)
    p = tmp_path / "rig.yml"
    p.write_text(_text(d, sp.XR, sp.XT))
    c, XR, XT, present = jn.load_calibration(str(p), 1280, 720)
    assert _same(c, d) and present == 255
    assert (c.calib_width, c.calib_height) == (1280, 720)                # not in the file: the caller's
    assert XR.tobytes() == bytes(sp.XR) and XT.tobytes() == bytes(sp.XT)
    # data wrapped one value per line, and all on one line
    for per_line in (1, 100):
        p.write_text(_text(d, sp.XR, sp.XT, per_line=per_line))
        c, XR, XT, present = jn.load_calibration(str(p))
        assert _same(c, d) and XR.tobytes() == bytes(sp.XR) and present == 255


def test_the_shipped_rig_file_loads_to_the_compiled_in_defaults(jn):
    from jackal_navigation_amd import node
    c, XR, XT, present = jn.load_calibration(os.path.join(ROOT, "tests", "golden", "amrl_jackal_webcam_stereo.yml"))
    assert present == 255 and _same(c, node.stereo_calib())             # its T is a plain sequence, the rest !!opencv-matrix
    sp = node.scan_params(640, 360)
    assert XR.tobytes() == bytes(sp.XR) and XT.tobytes() == bytes(sp.XT)


def test_xr_xt_absent_is_identity_and_zero(jn, tmp_path):
    from jackal_navigation_amd import node, calib
    p = tmp_path / "rig.yml"
    p.write_text(_text(node.stereo_calib()) + "# a comment\nnote: 3\n")
    c, XR, XT, present = jn.load_calibration(str(p))
    assert present == calib.STEREO == 63 and np.array_equal(XR, np.eye(3)) and np.array_equal(XT, np.zeros(3))
    p.write_text(_text(node.stereo_calib(), XT=[0.1, 0.2, 0.3]))
    c, XR, XT, present = jn.load_calibration(str(p))
    assert present == 63 | calib.XT and np.array_equal(XR, np.eye(3)) and XT.tolist() == [0.1, 0.2, 0.3]


def test_save_load_round_trip_is_bit_exact(jn, tmp_path):
    from jackal_navigation_amd import _lib
    rng = np.random.default_rng(5)
    p = str(tmp_path / "rt.yml")
    for trial in range(20):
        c = _lib.StereoCalib()
        vals = rng.standard_normal(43) * 10.0 ** rng.integers(-300, 300, 43)
        vals[:6] = [-0.0, 0.0, 5e-324, -2.2250738585072009e-308, 1.7976931348623157e308, 1.0]      # negative zero, denormals, the largest double
        rng.shuffle(vals)
        for name, (a, b) in zip(("K1", "D1", "K2", "D2", "R", "T"), ((0, 9), (9, 14), (14, 23), (23, 28), (28, 37), (37, 40))):
            getattr(c, name)[:] = vals[a:b].tolist()
        XR, XT = rng.standard_normal(9) * 1e-7, vals[40:43]
        jn.save_calibration(p, c, XR, XT)
        c2, XR2, XT2, present = jn.load_calibration(p)
        assert present == 255 and _same(c, c2), trial
        assert XR2.tobytes() == XR.tobytes() and XT2.tobytes() == XT.tobytes(), trial
    assert open(p).read().startswith("%YAML:1.0\nK1: !!opencv-matrix\n   rows: 3\n   cols: 3\n   dt: d\n   data: [ ")
    c.K1[4] = float("nan")
    with pytest.raises(_lib.JnError) as e:
        jn.save_calibration(p, c, XR, XT)
    assert e.value.status == _lib.JN_ERR_INVALID
    c.K1[4] = 1.0
    with pytest.raises(_lib.JnError):
        jn.save_calibration(str(tmp_path / "no_such_dir" / "x.yml"), c, XR, XT)


def test_malformed_files_are_refused_and_leave_the_outputs_untouched(jn, tmp_path):
    from jackal_navigation_amd import node, calib, _lib
    L = calib._bind()
    d = node.stereo_calib()
    good = _text(d, np.eye(3).reshape(-1), [0, 0, 0.3])
    cases = {
        "no header": good.replace("%YAML:1.0\n", ""),
        "truncated data": _text(d, K1=_matrix("K1", 3, 3, list(d.K1)[:8])),
        "truncated file": good[:good.index("data: [") + 30],
        "too long": _text(d, K1=_matrix("K1", 3, 3, list(d.K1) + [1.0])),
        "wrong shape": _text(d, K1=_matrix("K1", 1, 9, d.K1)),
        "wrong shape D": _text(d, D1=_matrix("D1", 5, 5, list(d.D1) * 5)),
        "dt u": _text(d, R=_matrix("R", 3, 3, d.R, dt="u")),
        "dt i": _text(d, R=_matrix("R", 3, 3, d.R, dt="i")),
        "not a number": good.replace(repr(float(d.K2[0])), "abc"),
        "nan": good.replace(repr(float(d.K2[0])), "nan"),
        "missing T": _text(d, T=""),
        "twice": good + _matrix("K1", 3, 3, d.K1),
        "xr shape": _text(d) + _matrix("XR", 3, 3, [1.0] * 9).replace("cols: 3", "cols: 2"),
        "no colon": good.replace("K2:", "K2"),
    }
    p = tmp_path / "bad.yml"
    for what, text in cases.items():
        p.write_text(text)
        c = _lib.StereoCalib()
        C.memset(C.byref(c), 0x5a, C.sizeof(c))
        before = bytes(c)
        XR, XT, present = np.full(9, 7.0), np.full(3, 8.0), C.c_int32(-5)
        st = L.jn_calib_load_yaml(str(p).encode(), C.byref(c), XR.ctypes.data, XT.ctypes.data, C.byref(present))
        assert st == _lib.JN_ERR_INVALID, what
        assert bytes(c) == before and (XR == 7.0).all() and (XT == 8.0).all() and present.value == -5, what
    p.write_text(good)                                                    # dt f and a plain sequence for a 3-vector are legal
    assert L.jn_calib_load_yaml(str(p).encode(), C.byref(_lib.StereoCalib()), np.zeros(9).ctypes.data, np.zeros(3).ctypes.data, None) == _lib.JN_OK
    p.write_text(_text(d, R=_matrix("R", 3, 3, d.R, dt="f"), T="T: [ 1.5, -2.,\n   3e-1 ]\n"))
    c, XR, XT, present = jn.load_calibration(str(p))
    assert list(c.T) == [1.5, -2.0, 0.3] and present == 63
    # a missing file, NULL arguments
    c = _lib.StereoCalib()
    z9, z3 = np.zeros(9), np.zeros(3)
    assert L.jn_calib_load_yaml(str(tmp_path / "none.yml").encode(), C.byref(c), z9.ctypes.data, z3.ctypes.data, None) == _lib.JN_ERR_INVALID
    assert L.jn_calib_load_yaml(None, C.byref(c), z9.ctypes.data, z3.ctypes.data, None) == _lib.JN_ERR_INVALID
    assert L.jn_calib_load_yaml(str(p).encode(), None, z9.ctypes.data, z3.ctypes.data, None) == _lib.JN_ERR_INVALID
    assert L.jn_calib_load_yaml(str(p).encode(), C.byref(c), None, z3.ctypes.data, None) == _lib.JN_ERR_INVALID
    assert L.jn_calib_load_yaml(str(p).encode(), C.byref(c), z9.ctypes.data, None, None) == _lib.JN_ERR_INVALID
    assert L.jn_calib_save_yaml(None, C.byref(c), z9.ctypes.data, z3.ctypes.data) == _lib.JN_ERR_INVALID
    assert L.jn_calib_save_yaml(str(p).encode(), None, z9.ctypes.data, z3.ctypes.data) == _lib.JN_ERR_INVALID
    with pytest.raises(_lib.JnError):
        jn.load_calibration(str(tmp_path / "none.yml"))
