"""Sub-pixel corner refinement (K24) on the GPU: clc_corner_subpix(_device) and calib.CornerSubPix against the host build of the same
header (tests/shim/subpix_shim.cpp), bit for bit on corners, status, iterations and strength, on the smallest shapes at which the kernel
can go wrong: images of 33 x 21 (pitch 40) and 61 x 47, half-windows from 1 (9 of 64 lanes) to 15 (16 window pixels per lane, a window
larger than the small image), a zero zone, 3 images holding 0, 1 and 257 corners, offsets[0] > 0, in place; every status on an edge
case; the accuracy against the rendered truth and what it buys clc_board_poses."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import campose_ref  # noqa: E402
import subpix_cases as cases  # noqa: E402
import subpix_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sv():
    from camlasercalibratool_amd import Solver
    with Solver() as s:
        yield s


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return cases.build_shim(str(tmp_path_factory.mktemp("sp") / "libsubpix_shim.so"))


def host_form(sv, b, o):
    return sv.corner_subpix(b["images"], b["corners"], b["offsets"], cases.options_c(o), width=b["width"])


def device_form(sv, b, o, in_place=False):
    """clc_corner_subpix_device on torch tensors -> the dict of Solver.corner_subpix."""
    import torch
    dev = torch.device("cuda", sv.device)
    img = torch.from_numpy(np.ascontiguousarray(b["images"])).to(dev)
    cin = torch.from_numpy(np.ascontiguousarray(b["corners"], dtype=np.float32)).to(dev)
    off = torch.from_numpy(np.ascontiguousarray(b["offsets"], dtype=np.int64)).to(dev)
    out = cin if in_place else cin.clone()
    m = cin.shape[0]
    st = torch.full((m,), -99, dtype=torch.int32, device=dev)
    it = torch.zeros((m,), dtype=torch.int32, device=dev)
    lam = torch.full((m,), float("nan"), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    sv.corner_subpix_device(img.data_ptr(), b["width"], img.shape[1], img.shape[2], img.shape[0], cin.data_ptr(), off.data_ptr(), out.data_ptr(),
                            st.data_ptr(), it.data_ptr(), lam.data_ptr(), cases.options_c(o))
    return dict(corners=out.cpu().numpy(), status=st.cpu().numpy(), iterations=it.cpu().numpy(), strength=lam.cpu().numpy())


def assert_same_bits(got, want, what):
    for k in cases.KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        bad = np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))
        assert len(bad) == 0, (what, k, bad[:8], a[bad[:8]], b[bad[:8]])


@pytest.mark.parametrize("size", range(len(cases.SIZES)))
def test_batches_bit_for_bit(sv, shim, size):
    """Every window on the batch of 0, 1 and 257 corners with offsets[0] = 5: the host-array form, the device form and the device form in
    place against the host build, bit for bit; the rows outside the offsets untouched; a second call the same bits."""
    b = cases.batch(size)
    for win, o in enumerate(cases.WINDOWS):
        want = cases.shim_refine(shim, b["images"], b["width"], b["corners"], b["offsets"], o)
        got = host_form(sv, b, o)
        assert_same_bits(got, want, f"host form, size {size} window {win}")
        assert_same_bits(device_form(sv, b, o), want, f"device form, size {size} window {win}")
        if win in (1, 4):
            assert_same_bits(device_form(sv, b, o, in_place=True), want, f"device form in place, size {size} window {win}")
            assert_same_bits(host_form(sv, b, o), got, "a second call")
        hist = dict(zip(*np.unique(got["status"][cases.FIRST:cases.FIRST + sum(cases.COUNTS)], return_counts=True)))
        print("size", size, "window", win, "status", hist, "iterations up to", int(got["iterations"].max()))


def test_product_library_and_optional_outputs(sv, shim):
    """The product library gives the hooks build's bits; corners_out alone (status, iterations and strength NULL); host form in place."""
    import ctypes as C
    import camlasercalibratool_amd as clc
    from camlasercalibratool_amd import _build
    b, o = cases.batch(0), cases.WINDOWS[2]
    want = cases.shim_refine(shim, b["images"], b["width"], b["corners"], b["offsets"], o)
    with clc.Solver(0, library=_build.PRODUCT_LIB_PATH) as prod:
        assert_same_bits(host_form(prod, b, o), want, "product library")
    V = lambda a: a.ctypes.data_as(C.c_void_p)
    img, off = np.ascontiguousarray(b["images"]), np.ascontiguousarray(b["offsets"], dtype=np.int64)
    io = np.array(b["corners"], dtype=np.float32)
    oc = cases.options_c(o)
    code = sv._L.clc_corner_subpix(sv._h, C.byref(oc), V(img), b["width"], img.shape[1], img.shape[2], img.shape[0], V(io), V(off), V(io), None, None,
                                   None)
    assert code == 0 and np.array_equal(io.view(np.uint32), want["corners"].view(np.uint32))


def test_empty_calls(sv):
    o = cases.options_c(ref.Options(3, 3))
    img = np.zeros((2, 8, 8), np.uint8)
    r = sv.corner_subpix(img, np.zeros((0, 2), np.float32), [0, 0, 0], o)
    assert r["corners"].shape == (0, 2)
    r = sv.corner_subpix(img[:0], np.full((3, 2), 2.5, np.float32), [0], o)
    assert (r["status"] == -99).all() and np.array_equal(r["corners"], np.full((3, 2), 2.5, np.float32))
    # images without a corner between images with some, and a corner array that begins behind offsets[0]
    r = sv.corner_subpix(img, np.full((3, 2), 2.5, np.float32), [1, 1, 2], o)
    assert list(r["status"]) == [-99, ref.SINGULAR, -99]


@pytest.mark.parametrize("name", ["flat", "max_iter_1", "converged", "nan", "inf", "outside", "outside_far", "at_width", "leaving"])
def test_edge_statuses(sv, shim, name):
    c = cases.edge_cases()[name]
    want = cases.shim_refine(shim, c["images"], c["width"], c["corners"], c["offsets"], c["options"])
    assert want["status"][0] == c["expect"]
    got = host_form(sv, c, c["options"])
    print(name, {k: got[k] for k in cases.KEYS})
    assert_same_bits(got, want, name)
    assert_same_bits(device_form(sv, c, c["options"]), want, name + " (device form)")


def test_ell_corners_revert_by_themselves(sv, shim):
    e = cases.ell_corners()
    want = cases.shim_refine(shim, e["images"], e["width"], e["corners"], e["offsets"], e["options"])
    got = host_form(sv, e, e["options"])
    assert_same_bits(got, want, "L-corners")
    rev = got["status"] == ref.REVERTED
    assert rev.sum() >= 1 and np.array_equal(got["corners"][rev], e["corners"][rev])


def test_a_corner_alone_and_in_the_batch(sv):
    b, o = cases.batch(1), cases.WINDOWS[3]
    whole = host_form(sv, b, o)
    rows = [cases.FIRST + 1, cases.FIRST + 64, cases.FIRST + 257]
    for c in rows:
        one = sv.corner_subpix(b["images"][2:3], b["corners"][c:c + 1], [0, 1], cases.options_c(o), width=b["width"])
        for k in cases.KEYS:
            assert np.array_equal(one[k][0], whole[k][c], equal_nan=True), (c, k)


def pose_error(q_wxyz, t, s):
    R = campose_ref.quat_wxyz_to_R(q_wxyz)
    return float(np.linalg.norm(t - s["t"])), float(np.degrees(np.arccos(np.clip((np.trace(R.T @ s["R"]) - 1) / 2, -1, 1))))


def test_accuracy_and_the_pose_it_feeds(sv, shim):
    """The four rendered boards in one call (calib.CornerSubPix, lists per image, starts = the true corners rounded to integers, eps
    0.01): the device's corners are the host build's bits, so the gate tests/test_subpix_host.py holds on the restatement (refined RMS <=
    0.25 x start RMS at half-windows 3 and 5) is asserted on them as they are; and clc_board_poses from the refined corners (half-window
    3) ends closer to the true pose than from the rounded ones, in translation and in rotation."""
    import camlasercalibratool_amd as clc
    scenes = [cases.board_scene(seed) for seed in cases.BOARD_SEEDS]
    images = np.stack([s["image"] for s in scenes])
    starts = [np.rint(s["truth"]).astype(np.float32) for s in scenes]
    off = np.arange(len(scenes) + 1) * len(starts[0])
    refined3 = None
    for w in (3, 5):
        refined, status, strength = clc.CornerSubPix(images, starts, win=w, eps=0.01, solver=sv)
        want = cases.shim_refine(shim, images, cases.BOARD_W, np.concatenate(starts), off, ref.Options(w, w, eps=0.01))
        assert np.array_equal(np.concatenate(refined).view(np.uint32), want["corners"].view(np.uint32))
        assert np.array_equal(np.concatenate(status), want["status"]) and np.array_equal(np.concatenate(strength), want["strength"])
        for s, st, r in zip(scenes, starts, refined):
            r0, r1 = cases.rms(st, s["truth"]), cases.rms(r, s["truth"])
            print("half-window", w, "start rms", r0, "refined rms", r1, "ratio", r1 / r0)
            assert r1 <= 0.25 * r0
        assert all((x == ref.CONVERGED).all() for x in status) and all((x > 0).all() for x in strength)
        if w == 3:
            refined3 = refined
    cam = clc.Camera.pinhole(*cases.PROJ, width=cases.BOARD_W, height=cases.BOARD_H)
    board = [s["board_xy"] for s in scenes]
    q0, t0, st0, _ = clc.CalcCamPoses(cam, starts, board, solver=sv)
    q1, t1, st1, _ = clc.CalcCamPoses(cam, refined3, board, solver=sv)
    assert (st0 == 1).all() and (st1 == 1).all()
    for k, s in enumerate(scenes):
        e0, e1 = pose_error(q0[k], t0[k], s), pose_error(q1[k], t1[k], s)
        print("seed", cases.BOARD_SEEDS[k], "rounded: t %.5f m, %.3f deg; refined: t %.5f m, %.3f deg" % (e0 + e1))
        assert e1[0] < e0[0] and e1[1] < e0[1]
