"""K26 (csrc/clc_boardorder.hpp: the chessboard ordering on the device) without a GPU: the kernel header compiled with g++
(tests/shim/boardorder_shim.cpp, the lanes a loop) against the yardstick, the product library's host clc_chessboard_order, on every
case of tests/boardorder_cases.py — index, status and n_labelings equal, worst within 16 eps; its hull and quadrilateral against
tests/chess_ref.py exactly; what the cases are built to show and the margins of their decisions, on the restatement alone; the new
symbols and every refusal of the three new calls (they need no handle); a stand-alone AddressSanitizer / UBSan program."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import boardorder_cases as bc  # noqa: E402
import chess_ref as ref  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402

V = bc.V
NEW = ("clc_chessboard_order_device", "clc_find_chessboard_device", "clc_find_chessboard_gpu")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return bc.build_shim(str(tmp_path_factory.mktemp("bo") / "libboardorder_shim.so"))


def test_what_the_cases_are_built_to_show():
    """On the restatement alone.  No pass's ratio in [0.9 tol, 1.1 tol]; in every pass that the ratio gate lets through every node's
    second-nearest candidate position is at least (1 + 1e-6) x as far (squared) as its nearest (a pass beyond 1.1 tol is rejected
    whatever it matched: the exact lattice's quarter turns put nodes midway between candidates there).  As measured: the smallest such
    margin 11.5 (jitter), the largest valid ratio 0.24."""
    hulls = {}
    for name in bc.NAMES:
        rs = bc.restated(name)
        passes = [p for r in rs for p in r["passes"]]
        near = [p[0] for p in passes if 0.9 * bc.TOL <= p[0] <= 1.1 * bc.TOL]
        margin = min([p[1] for p in passes if p[0] <= bc.TOL], default=np.inf)
        hulls[name] = [len(r["hull"]) for r in rs]
        print(name, "status", [r["status"] for r in rs], "hull", hulls[name], "ties", [r["ties"] for r in rs], "labelings",
              [r["n_labelings"] for r in rs], "smallest margin", margin, "largest valid ratio", max([p[0] for p in passes if p[0] <= bc.TOL], default=None))
        assert not near, (name, near)
        assert margin >= 1.0 + 1e-6, (name, margin)
    st = lambda name: [r["status"] for r in bc.restated(name)]
    for name in ("scenes", "tilted_9x6", "tilted_6x6", "jitter", "lattice", "grid_2x2", "grid_2x7", "grid_32x32", "half", "count_gt", "stride_gt"):
        assert set(st(name)) == {ref.FOUND}, name
    for name in ("scenes", "tilted_9x6", "tilted_6x6"):
        assert all(6 <= h <= 10 for h in hulls[name]), (name, hulls[name])
    assert {r["n_labelings"] for r in bc.restated("tilted_9x6")} == {2} and {r["n_labelings"] for r in bc.restated("tilted_6x6")} == {4}
    assert hulls["lattice"] == [4] and hulls["lattice_dup"] == [4] and st("lattice_dup") == [ref.NO_GRID]
    lat = bc.restated("lattice")[0]
    assert all(p[0] < 1e-9 for p in lat["passes"] if p[0] <= bc.TOL)  # every predicted node lands on a candidate
    assert min(hulls["jitter"]) >= 7
    assert hulls["circle_20"] == [20] and hulls["circle_64"] == [64] and st("circle_20") == st("circle_64") == [ref.NO_GRID]
    assert hulls["octagon"] == [8] and bc.restated("octagon")[0]["ties"] > 1
    assert bc.cases()["grid_32x32"]["xy"].shape[1] == 1024 and bc.cases()["grid_2x2"]["xy"].shape[1] == 4
    c = bc.cases()["half"]["xy"]
    frac = np.abs(c - np.trunc(c))
    assert (frac == 0.5).any() and (c[0][frac[0] == 0.5] > 0).any() and (c[1][frac[1] == 0.5] < 0).any() and (c < 0).any()
    assert (bc.round_away(c) != np.rint(c)).any()  # half to even would give other pixels
    assert (bc.cases()["count_gt"]["count"] > 20).all() and bc.cases()["stride_gt"]["xy"].shape[1] == 256
    assert st("refusals") == bc.REFUSALS_STATUS
    moved = bc.restated("refusals")[2]
    assert len(moved["hull"]) >= 4 and moved["passes"] and min(p[0] for p in moved["passes"]) > 1.1 * bc.TOL  # refused by the tol gate


@pytest.mark.parametrize("name", bc.NAMES)
def test_shim_against_the_yardstick(shim, name):
    """The kernel header on the host against clc_chessboard_order; the hull (candidate slots, from the vertex smallest in (x, y)) and
    the quadrilateral (hull positions) against tests/chess_ref.py, exactly.  As measured: worst differs by at most 1.05 eps."""
    c = bc.cases()[name]
    want = bc.host_order(c)
    got = bc.shim_order(shim, c)
    print(name, "status", want["status"], "labelings", want["n_labelings"], "hull sizes", got["nh"])
    bc.assert_same_order(got, want, name)
    assert [r["status"] for r in bc.restated(name)] == list(want["status"])
    n = c["cols"] * c["rows"]
    for k in range(len(c["xy"])):
        if c["status"][k] == ref.OVERFLOW or c["count"][k] < n or not (np.abs(c["xy"][k, :n]) <= 2.0 ** 24).all():
            assert got["nh"][k] == 0
            continue
        P = bc.round_away(c["xy"][k, :n])
        hv = ref.hull(P)
        assert list(got["hull"][k, :got["nh"][k]]) == list(hv), (name, k)
        if len(hv) >= 4:
            assert list(got["quad"][k]) == list(ref.largest_quad(P, np.array(hv))), (name, k)
    # an image alone gives its row of the batch, and the nullable outputs may be left out
    one = {key: (v[:1] if isinstance(v, np.ndarray) else v) for key, v in c.items()}
    alone = bc.shim_order(shim, one)
    assert np.array_equal(alone["index"][0], got["index"][0]) and alone["status"][0] == got["status"][0]
    assert np.array_equal(alone["worst"].view(np.uint64), got["worst"][:1].view(np.uint64))


def test_shim_gather(shim):
    c = bc.cases()["refusals"]
    both = {key: (np.concatenate([v, bc.cases()["scenes"][key][:3]]) if isinstance(v, np.ndarray) else v) for key, v in c.items()}
    o = bc.shim_order(shim, both)
    k, n = len(both["xy"]), 20
    starts = np.full((k, n, 2), -7.0, np.float32); found = np.full(k, -7, np.int32); offsets = np.full(k + 1, -7, np.int64)
    strength = np.full((k, n), -7.0)
    shim.shim_board_gather(V(both["xy"]), V(o["index"]), V(o["status"]), C.c_longlong(20), C.c_longlong(k), C.c_int32(n), V(starts), V(found),
                           V(offsets), V(strength))
    assert list(found) == [0] * 7 + [1] * 3 and list(offsets) == [20 * i for i in range(k + 1)] and np.isnan(strength).all()
    assert np.isnan(starts[:7]).all()
    for i in range(7, 10):
        assert np.array_equal(starts[i], both["xy"][i, o["index"][i]])
    assert shim.shim_board_lds_bytes(1024) == 56 * 1024 + 2784 <= 64 * 1024


def test_symbols_and_version():
    header = open(os.path.join(ROOT, "include", "clc.h")).read()
    L = _capi.lib()
    for n in NEW:
        assert re.search(r"\b%s\(" % n, header) and n in _capi.EXPORTED and hasattr(L, n), n
    assert L.clc_version() == 210
    from camlasercalibratool_amd import Solver, _build
    assert all(hasattr(Solver, m) for m in ("chessboard_order_device", "find_chessboard_device"))
    assert "clc_boardorder.hpp" in _build.SIDE_HEADERS and "clc_boardorder.hpp" not in _build.HEADERS + _build.HOST_HEADERS
    with pytest.raises(ValueError):
        Solver.find_chessboard(None, np.zeros((1, 16, 16), np.uint8), 5, 4, ordering="somewhere")


def test_order_device_refusals():
    """What clc_chessboard_order refuses, in its order, under the new name; the NULL handle last."""
    L = _capi.lib()
    xy = np.zeros((1, 20, 2), np.float32); count = np.array([20], np.int32); index = np.zeros(20, np.int32); status = np.ones(1, np.int32)
    bad = lambda **kw: _capi.ChessOrderOptions(**{**dict(tol=0.3, reserved=0, reserved2=0), **kw})
    for args, text in [((xy, count, 20, 1, 5, 4, bad(tol=0.0), index, status), "tol"), ((xy, count, 20, 1, 5, 4, bad(tol=0.51), index, status), "tol"),
                       ((xy, count, 20, 1, 5, 4, bad(tol=float("nan")), index, status), "tol"), ((xy, count, 20, 1, 5, 4, bad(reserved=1), index, status), "reserved"),
                       ((xy, count, 20, 1, 5, 4, bad(reserved2=1), index, status), "reserved"), ((xy, count, 20, 1, 1, 20, None, index, status), "cols and rows"),
                       ((xy, count, 20, 1, 33, 32, None, index, status), "cols and rows"), ((xy, count, 20, 2 ** 31, 5, 4, None, index, status), "too many images"),
                       ((xy, count, 19, 1, 5, 4, None, index, status), "stride"), ((None, count, 20, 1, 5, 4, None, index, status), "bad argument"),
                       ((xy, None, 20, 1, 5, 4, None, index, status), "bad argument"), ((xy, count, 20, 1, 5, 4, None, None, status), "bad argument"),
                       ((xy, count, 20, 1, 5, 4, None, index, None), "bad argument"),
                       ((xy, count, 20, 1, 5, 4, None, index, status), "bad argument"),   # nothing wrong but the NULL handle
                       ((None, None, 20, 0, 5, 4, None, None, None), "bad argument")]:    # (no image: the handle is still asked for)
        a, cnt, stride, n, cols, rows, o, ix, st = args
        code = L.clc_chessboard_order_device(None, V(a), V(cnt), stride, n, cols, rows, None if o is None else C.byref(o), V(ix), V(st), None, None)
        msg = L.clc_last_error().decode()
        assert code == -1 and msg.startswith("clc_chessboard_order_device:") and text in msg, (code, msg, text)
    # a refusal of the options comes before the stride, the stride before the handle
    code = L.clc_chessboard_order_device(None, V(xy), V(count), 19, 1, 5, 4, C.byref(bad(tol=0.0)), V(index), V(status), None, None)
    assert code == -1 and "tol" in L.clc_last_error().decode()


@pytest.mark.parametrize("name", ["clc_find_chessboard_device", "clc_find_chessboard_gpu"])
def test_find_refusals(name):
    """The refusals of clc_find_chessboard, in its order, under the new names; all without a handle."""
    L = _capi.lib()
    f = getattr(L, name)
    img = np.zeros((1, 16, 16), np.uint8); found = np.zeros(1, np.int32); corners = np.zeros((20, 2), np.float32)
    ref_ = lambda o: None if o is None else C.byref(o)
    def call(co, oo, so, im, w, cols, rows, cr, fd, height=16, pitch=16, n=1):
        code = f(None, ref_(co), ref_(oo), ref_(so), V(im), w, height, pitch, n, cols, rows, V(cr), V(fd), None)
        return code, L.clc_last_error().decode()
    for change, text in [(dict(threshold=0), "threshold"), (dict(nms_radius=8), "nms_radius"), (dict(rel_permille=1001), "rel_permille"),
                         (dict(max_per_image=0), "max_per_image"), (dict(max_per_image=1025), "max_per_image"), (dict(reserved=1), "reserved")]:
        o = _capi.default_chess_options()
        for k, v in change.items():
            setattr(o, k, v)
        code, msg = call(o, None, None, img, 16, 5, 4, corners, found)
        assert code == -1 and msg.startswith(name + ":") and text in msg, (code, msg)
    small = _capi.default_chess_options(); small.max_per_image = 19
    bad_order = _capi.ChessOrderOptions(0.7, 0, 0)
    bad_subpix = _capi.default_subpix_options(11); bad_subpix.win_x = 16
    for args, kw, text in [((small, None, None, img, 16, 5, 4, corners, found), {}, "max_per_image must be >= cols x rows"),
                           ((None, bad_order, None, img, 16, 5, 4, corners, found), {}, "tol"),
                           ((None, None, bad_subpix, img, 16, 5, 4, corners, found), {}, "refinement"),
                           ((None, None, None, img, 16, 1, 4, corners, found), {}, "cols and rows"),
                           ((None, None, None, img, 0, 5, 4, corners, found), {}, "width and height"),
                           ((None, None, None, img, 16, 5, 4, corners, found), dict(pitch=15), "pitch"),
                           ((None, None, None, img, 16, 5, 4, corners, found), dict(n=2 ** 31), "too many images"),
                           ((None, None, None, None, 16, 5, 4, corners, found), {}, "bad argument"),
                           ((None, None, None, img, 16, 5, 4, None, found), {}, "bad argument"),
                           ((None, None, None, img, 16, 5, 4, corners, None), {}, "bad argument"),
                           ((None, None, None, img, 16, 5, 4, corners, found), {}, "bad argument")]:  # the last: the NULL handle alone
        code, msg = call(*args, **kw)
        assert code == -1 and msg.startswith(name + ":") and text in msg, (code, msg, text)
    # the detection's refusal comes before the ordering's, that before the refinement's
    code, msg = call(small, bad_order, bad_subpix, img, 0, 5, 4, corners, found)
    assert "width and height" in msg
    code, msg = call(small, bad_order, bad_subpix, img, 16, 5, 4, corners, found)
    assert "tol" in msg
    # every field of the refinement options, the order of two refusals, the corner count: the rows all composite forms share
    import imagecall_refusals
    imagecall_refusals.check_composite_refusals(L, name)


def test_sanitized_standalone_program(tmp_path):
    """tests/shim/boardorder_main.cpp, built with -fsanitize=address,undefined and run as an ordinary process: the kernel header beside
    the host ordering on every case above and on grids from 2 x 2 to 32 x 32, every array and the LDS block allocated exactly."""
    exe, data = str(tmp_path / "boardorder_main"), str(tmp_path / "cases.bin")
    bc.write_cases(data)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "shim", "boardorder_main.cpp"), "-o", exe])
    p = subprocess.run([exe, data], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    print(p.stdout)
    assert "shapes ok" in p.stdout and "cases %d " % len(bc.NAMES) in p.stdout, p.stdout
    m = re.search(r"grids (\d+) found (\d+)", p.stdout)
    assert m and int(m.group(1)) == 45 and int(m.group(2)) > 0, p.stdout  # (as measured: 44 of the 45 jittered grids are found, by both)
