"""Chessboard corners from images (K25) on the GPU: clc_chess_corners(_device) against the host build of the same header
(tests/shim/chess_shim.cpp), the same bits on x, y, R5, count, count_raw and status — every value is an integer, so there is no tolerance —
on the cases of tests/chess_cases.py (images from 10 x 30 to 640 x 400, pitches that leave no row aligned, corners on both sides of every
tile edge, exact ties, more raw candidates than the cap, every gate at its ends), for an image alone and in batches of 0, 1 and 257
images (two launches of 170 and 87), through both forms, on the product library, twice in a row; then calib.FindChessboardCorners end to
end against the truth and against the existing route from the truth's rounded corners."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import campose_ref  # noqa: E402
import chess_cases as cases  # noqa: E402
import chess_ref as ref  # noqa: E402
import subpix_cases as sp  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sv():
    from camlasercalibratool_amd import Solver
    with Solver() as s:
        yield s


@pytest.fixture(scope="module")
def prod():
    import camlasercalibratool_amd as clc
    from camlasercalibratool_amd import _build
    with clc.Solver(0, library=_build.PRODUCT_LIB_PATH) as s:
        yield s


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return cases.build_shim(str(tmp_path_factory.mktemp("ch") / "libchess_shim.so"))


def host_form(sv, images, width, o):
    return sv.chess_corners(images, cases.options_c(o), width=width)


def device_form(sv, images, width, o):
    """clc_chess_corners_device on torch tensors -> the dict of Solver.chess_corners."""
    import torch
    dev = torch.device("cuda", sv.device)
    img = torch.from_numpy(np.ascontiguousarray(images)).to(dev)
    r = {k: torch.from_numpy(v).to(dev) for k, v in cases.empty_result(img.shape[0], o.max_per_image).items()}
    torch.cuda.synchronize()
    sv.chess_corners_device(img.data_ptr(), width, img.shape[1], img.shape[2], img.shape[0], r["xy"].data_ptr(), r["count"].data_ptr(),
                            r["status"].data_ptr(), r["r5"].data_ptr(), r["count_raw"].data_ptr(), cases.options_c(o))
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("name", cases.NAMES)
def test_cases_bit_for_bit(sv, prod, shim, name):
    """Both forms and the product library against the host build; a second call the same bits; each of the first images alone."""
    c = cases.cases()[name]
    images, width, o = c["images"], c["width"], c["options"]
    want = cases.shim_detect(shim, images, width, o)
    cases.assert_same_bits(want, cases.reference(name), name + ": the host build against the restatement")
    got = host_form(sv, images, width, o)
    print(name, "count", got["count"][:12], "raw", got["count_raw"][:12], "status", got["status"][:12])
    cases.assert_same_bits(got, want, name + ", host form")
    cases.assert_same_bits(device_form(sv, images, width, o), want, name + ", device form")
    cases.assert_same_bits(host_form(prod, images, width, o), want, name + ", product library")
    cases.assert_same_bits(host_form(prod, images, width, o), want, name + ", product library, a second call")
    cases.assert_same_bits(device_form(prod, images, width, o), want, name + ", product library, device form")
    for k in range(min(len(images), 2)):
        one = host_form(sv, images[k:k + 1], width, o)
        for key in cases.KEYS:
            assert np.array_equal(one[key][0], want[key][k], equal_nan=True), (name, k, key)


@pytest.mark.parametrize("count", cases.COUNTS)
def test_batches_bit_for_bit(prod, shim, count):
    """0, 1 and 257 images of 160 x 120 (257: two launches on one stream) on the product library, both forms, twice in a row."""
    images, o = cases.batch(count), ref.Options()
    want = cases.shim_detect(shim, images, sp.BOARD_W, o)
    if count:
        assert (want["count"] == 20).all() and np.array_equal(want["xy"][-1], cases.reference("scenes")["xy"][(count - 1) % 12], equal_nan=True)
    for again in range(2):
        cases.assert_same_bits(host_form(prod, images, sp.BOARD_W, o), want, f"{count} images, host form, call {again}")
        cases.assert_same_bits(device_form(prod, images, sp.BOARD_W, o), want, f"{count} images, device form, call {again}")


def test_optional_outputs_left_out(sv, shim):
    import ctypes as C
    c = cases.cases()["scenes"]
    want = cases.shim_detect(shim, c["images"], c["width"], c["options"])
    r = cases.empty_result(len(c["images"]), c["options"].max_per_image)
    V = lambda a: a.ctypes.data_as(C.c_void_p)
    img = np.ascontiguousarray(c["images"])
    code = sv._L.clc_chess_corners(sv._h, None, V(img), c["width"], img.shape[1], img.shape[2], img.shape[0], V(r["xy"]), None, V(r["count"]), None,
                                   V(r["status"]))
    assert code == 0
    for k in ("xy", "count", "status"):
        assert np.array_equal(r[k].view(np.uint8), want[k].view(np.uint8)), k
    assert (r["r5"] == -7).all() and (r["count_raw"] == -7).all()


def pose_error(q_wxyz, t, s):
    R = campose_ref.quat_wxyz_to_R(q_wxyz)
    return float(np.linalg.norm(t - s["t"])), float(np.degrees(np.arccos(np.clip((np.trace(R.T @ s["R"]) - 1) / 2, -1, 1))))


def test_find_chessboard_end_to_end(sv):
    """calib.FindChessboardCorners on the four accuracy scenes of K24 (eps 0.01, half-windows 3 and 5): every board found; the RMS of
    its refined corners to the truth at most 1.25 x what the existing route reaches from the truth's rounded corners on the same image
    and window (the starts differ by up to one pixel while the iteration runs to the same stopping rule; on the numpy restatements the
    ratio is 0.998-1.001: tests/test_chess_host.py); CalcCamPoses from the result (half-window 3) no farther from the true pose than
    1.25 x the same route's, in translation and in rotation.  refine_win 0 returns the detector's integer pixels; an image without a
    board has NaN corners and found = 0 and does not fail the call."""
    import camlasercalibratool_amd as clc
    scenes = [sp.board_scene(seed) for seed in sp.BOARD_SEEDS]
    images = np.stack([s["image"] for s in scenes] + [np.full((sp.BOARD_H, sp.BOARD_W), 128, np.uint8)])
    cols, rows = sp.INNER
    det = sv.chess_corners(images)
    pixels, board0, found0 = clc.FindChessboardCorners(images, sp.INNER, sp.SQUARE, refine_win=0, solver=sv)
    assert list(found0) == [True] * 4 + [False] and np.isnan(pixels[4]).all()
    relabelled = [cases.relabel_truth(s["truth"], cols, rows, det["xy"][k, :cols * rows].astype(float), True) for k, s in enumerate(scenes)]
    for k in range(4):
        assert np.array_equal(pixels[k], np.rint(pixels[k])) and sp.rms(pixels[k], relabelled[k][0]) <= 1.0
    refined3 = baseline3 = None
    for w in (3, 5):
        corners, board, found = clc.FindChessboardCorners(images, sp.INNER, sp.SQUARE, refine_win=w, eps=0.01, solver=sv)
        assert list(found) == [True] * 4 + [False] and np.isnan(corners[4]).all()
        starts = [np.rint(t).astype(np.float32) for t, _ in relabelled]
        baseline, _, _ = clc.CornerSubPix(images[:4], starts, win=w, eps=0.01, solver=sv)
        for k in range(4):
            r1, r0 = sp.rms(corners[k], relabelled[k][0]), sp.rms(baseline[k], relabelled[k][0])
            print("seed", sp.BOARD_SEEDS[k], "half-window", w, "rms to the truth: from the detector", r1, "from the rounded truth", r0, "ratio", r1 / r0)
            assert r1 <= 1.25 * r0
            assert np.allclose(board[k], scenes[k]["board_xy"])
        if w == 3:
            refined3, baseline3 = corners, baseline
    # the corners back in the truth's order (a half turn of the labeling is a half turn of the board frame), then the poses
    cam = clc.Camera.pinhole(*sp.PROJ, width=sp.BOARD_W, height=sp.BOARD_H)
    board = [s["board_xy"] for s in scenes]
    def truth_order(per_image):
        out = []
        for k in range(4):
            a = np.empty_like(per_image[k])
            a[relabelled[k][1]] = per_image[k]
            out.append(a)
        return out
    q1, t1, st1, _ = clc.CalcCamPoses(cam, truth_order(refined3), board, solver=sv)
    q0, t0, st0, _ = clc.CalcCamPoses(cam, truth_order(baseline3), board, solver=sv)
    assert (st0 == 1).all() and (st1 == 1).all()
    for k, s in enumerate(scenes):
        e1, e0 = pose_error(q1[k], t1[k], s), pose_error(q0[k], t0[k], s)
        print("seed", sp.BOARD_SEEDS[k], "from the detector: t %.5f m, %.3f deg; from the rounded truth: t %.5f m, %.3f deg" % (e1 + e0))
        assert e1[0] <= 1.25 * e0[0] and e1[1] <= 1.25 * e0[1]
