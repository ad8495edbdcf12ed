"""Tag-grid corners from images (K27) on the GPU: clc_tag_grid, clc_tag_grid_device and clc_tag_grid_points_device against the host build
of the same header (tests/shim/tags_shim.cpp behind tests/shim/chess_shim.cpp), the same bits on every output — every value is an integer
or a NaN, so there is no tolerance — on the scenes of tests/tags_cases.py, each alone and in batches of 0, 1 and 257 images of 160 x 120
(two launches of 170 and 87), through every form, on the hooks build and on the product library, twice in a row; then
calib.FindTagGridCorners end to end against the truth and against the existing route from the truth's rounded corners."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import campose_ref  # noqa: E402
import subpix_cases as sp  # noqa: E402
import tags_cases as cases  # noqa: E402
import tags_ref as ref  # noqa: E402

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
def shims(tmp_path_factory):
    return cases.build_shims(str(tmp_path_factory.mktemp("tags")))


def host_form(sv, images, width, fam, cols, rows, o=ref.Options()):
    return sv.tag_grid(images, fam, cols, rows, cases.options_c(o), width=width)


def device_form(sv, images, width, fam, cols, rows, o=ref.Options(), points=None):
    """clc_tag_grid_device on torch tensors -> the dict of Solver.tag_grid; points = (tag_size, tag_spacing): clc_tag_grid_points_device on
    the result as well -> (dict, (corners_px, board_xy, offsets))."""
    import torch
    dev = torch.device("cuda", sv.device)
    img = torch.from_numpy(np.ascontiguousarray(images)).to(dev)
    n, T = img.shape[0], cols * rows
    r = {k: torch.from_numpy(v).to(dev) for k, v in cases.empty_result(n, T).items()}
    torch.cuda.synchronize()
    sv.tag_grid_device(img.data_ptr(), width, img.shape[1], img.shape[2], n, fam, cols, rows, r["corners"].data_ptr(), r["hamming"].data_ptr(),
                       r["count"].data_ptr(), r["status"].data_ptr(), r["n_quads"].data_ptr(), r["n_foreign"].data_ptr(),
                       r["n_edges_dropped"].data_ptr(), r["strength"].data_ptr(), cases.options_c(o))
    out = {k: v.cpu().numpy() for k, v in r.items()}
    if points is None:
        return out
    px = torch.full((max(n * 4 * T, 1), 2), -7.0, dtype=torch.float32, device=dev)
    bd = torch.full((max(n * 4 * T, 1), 2), -7.0, dtype=torch.float32, device=dev)
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    sv.tag_grid_points_device(r["corners"].data_ptr(), r["hamming"].data_ptr(), n, cols, rows, points[0], points[1], px.data_ptr(), bd.data_ptr(),
                              off.data_ptr())
    return out, (px.cpu().numpy()[:n * 4 * T], bd.cpu().numpy()[:n * 4 * T], off.cpu().numpy())


@pytest.mark.parametrize("name", cases.NAMES)
def test_scenes_bit_for_bit(sv, prod, shims, name):
    """Every form, the hooks build and the product library, against the host build; a second call the same bits."""
    s = cases.scene(name)
    cols, rows = s["grid"]
    img, width, fam = s["image"][None], s["width"], s["family"]
    want = cases.shim_tag_grid(shims, img, width, fam, cols, rows)
    cases.assert_same_bits(want, cases.reference(name), name + ": the host build against the restatement")
    got = host_form(sv, img, width, fam, cols, rows)
    print(name, "count", got["count"], "quads", got["n_quads"], "foreign", got["n_foreign"], "hamming", got["hamming"][0])
    cases.assert_same_bits(got, want, name + ", host form")
    cases.assert_same_bits(device_form(sv, img, width, fam, cols, rows), want, name + ", device form")
    cases.assert_same_bits(host_form(prod, img, width, fam, cols, rows), want, name + ", product library")
    cases.assert_same_bits(host_form(prod, img, width, fam, cols, rows), want, name + ", product library, a second call")
    got, pts = device_form(prod, sp.padded(img, width + 3, fill=201), width, fam, cols, rows, points=(0.055, 0.3))
    cases.assert_same_bits(got, want, name + ", product library, device form, another pitch")
    wpts = cases.shim_points(shims, want["corners"], want["hamming"], cols, rows, 0.055, 0.3)
    for a, b, what in zip(pts, wpts, ("corners_px", "board_xy", "offsets")):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, what)


@pytest.mark.parametrize("count", (0, 1, 257))
def test_batches_bit_for_bit(prod, shims, count):
    """0, 1 and 257 images of 160 x 120 (257: two launches on one stream) on the product library, every form, twice in a row."""
    images, fam = cases.batch(count), cases.scene("small_2x2_d4_b2")["family"]
    want = cases.shim_tag_grid(shims, images, 160, fam, 2, 2)
    wpts = cases.shim_points(shims, want["corners"], want["hamming"], 2, 2, 0.05, 0.3)
    if count:
        assert list(want["count"][:2]) == [4, 0][:count] and want["count"].sum() == 4 * ((count + 1) // 2)
        assert np.array_equal(want["corners"][-1], cases.reference("small_2x2_d4_b2")["corners"][0], equal_nan=True)
    for again in range(2):
        cases.assert_same_bits(host_form(prod, images, 160, fam, 2, 2), want, f"{count} images, host form, call {again}")
        got, pts = device_form(prod, images, 160, fam, 2, 2, points=(0.05, 0.3))
        cases.assert_same_bits(got, want, f"{count} images, device form, call {again}")
        for a, b, what in zip(pts, wpts, ("corners_px", "board_xy", "offsets")):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (count, what)
        assert pts[2][0] == 0 and pts[2][-1] == 4 * want["count"].sum()


def test_options_and_optional_outputs(sv, shims):
    """max_quads 1, a full edge list, a contrast above the image's range; the nullable outputs left out."""
    import ctypes as C
    s = cases.scene("big_3x2_d6_b2")
    img, fam = s["image"][None], s["family"]
    for o in (ref.Options(max_quads=1), ref.Options(contrast=255), ref.Options(max_border_errors=8)):
        cases.assert_same_bits(host_form(sv, img, 320, fam, 3, 2, o), cases.shim_tag_grid(shims, img, 320, fam, 3, 2, o), str(o))
    fimg, ffam, fo = cases.fence()
    got = host_form(sv, fimg, 300, ffam, 1, 1, fo)
    assert got["n_edges_dropped"][0] > 0
    cases.assert_same_bits(got, cases.shim_tag_grid(shims, fimg, 300, ffam, 1, 1, fo), "fence")
    want = cases.shim_tag_grid(shims, img, 320, fam, 3, 2)
    r = cases.empty_result(1, 6)
    V = lambda a: a.ctypes.data_as(C.c_void_p)
    fc = fam.c_struct()
    code = sv._L.clc_tag_grid(sv._h, C.byref(fc), None, None, None, V(np.ascontiguousarray(img)), 320, 240, 320, 1, 3, 2, V(r["corners"]), V(r["hamming"]),
                              V(r["count"]), V(r["status"]), None, None, None, None)
    assert code == 0
    cases.assert_same_bits(r, want, "optional outputs left out", keys=("corners", "hamming", "count", "status"))
    assert (r["n_quads"] == -7).all() and (r["strength"] == -7).all()


def pose_error(q_wxyz, t, s):
    R = campose_ref.quat_wxyz_to_R(q_wxyz)
    return float(np.linalg.norm(t - s["t"])), float(np.degrees(np.arccos(np.clip((np.trace(R.T @ s["R"]) - 1) / 2, -1, 1))))


def test_find_tag_grid_end_to_end(sv):
    """calib.FindTagGridCorners on the six accuracy scenes (half-window 3, eps 0.01): every tag found, in id order; the RMS of its refined
    corners to the truth at most 1.25 x what the existing route (CornerSubPix, K24) reaches from the truth's rounded corners on the same
    image (the starts differ by up to a pixel and a half while the iteration runs to the same stopping rule); CalcCamPoses from the
    result no farther from the true pose than 1.25 x the same route's, in translation and in rotation.  refine_win 0 returns the
    decoder's integer pixels.  Measured ratios: DESIGN.md K27."""
    import camlasercalibratool_amd as clc
    for name in cases.GRID_SCENES:
        s = cases.scene(name)
        cols, rows = s["grid"]
        img = s["image"][None]
        px, board, ids = clc.FindTagGridCorners(img, s["grid"], cases.TAG_SIZE, cases.SPACING, s["family"], refine_win=0, solver=sv)
        assert list(ids[0]) == list(range(cols * rows)) and np.array_equal(px[0], np.rint(px[0]))
        assert np.array_equal(px[0], cases.reference(name)["corners"][0].reshape(-1, 2))
        corners, board, ids = clc.FindTagGridCorners(img, s["grid"], cases.TAG_SIZE, cases.SPACING, s["family"], refine_win=3, eps=0.01, solver=sv)
        truth = s["truth"].reshape(-1, 2)
        baseline, _, _ = clc.CornerSubPix(img, [np.rint(truth).astype(np.float32)], win=3, eps=0.01, solver=sv)
        r1, r0 = sp.rms(corners[0], truth), sp.rms(baseline[0], truth)
        print(name, "rms to the truth: from the decoder", r1, "from the rounded truth", r0, "ratio", r1 / r0)
        assert r1 <= 1.25 * r0
        cam = clc.Camera.pinhole(*s["proj"], width=s["width"], height=s["height"])
        q1, t1, st1, _ = clc.CalcCamPoses(cam, corners, board, solver=sv)
        q0, t0, st0, _ = clc.CalcCamPoses(cam, baseline, board, solver=sv)
        assert st0[0] == 1 and st1[0] == 1
        e1, e0 = pose_error(q1[0], t1[0], s), pose_error(q0[0], t0[0], s)
        print(name, "from the decoder: t %.5f m, %.3f deg; from the rounded truth: t %.5f m, %.3f deg" % (e1 + e0))
        assert e1[0] <= 1.25 * e0[0] and e1[1] <= 1.25 * e0[1]


def test_cut_off_board_gives_a_pose(sv):
    """The scene whose last column of tags is cut by the image border: the five tags in view give a pose (the true one to the accuracy
    of the whole boards above) where FindChessboardCorners on the tags' corner grid finds no board."""
    import camlasercalibratool_amd as clc
    s = cases.scene("cut_off")
    img = s["image"][None]
    corners, board, ids = clc.FindTagGridCorners(img, s["grid"], cases.TAG_SIZE, cases.SPACING, s["family"], solver=sv)
    assert list(ids[0]) == [0, 1, 2, 3, 4] and len(corners[0]) == 20 and np.isfinite(corners[0]).all()
    cam = clc.Camera.pinhole(*s["proj"], width=s["width"], height=s["height"])
    q, t, st, rms = clc.CalcCamPoses(cam, corners, board, solver=sv)
    e = pose_error(q[0], t[0], s)
    print("cut-off board: t %.5f m, %.3f deg, rms %.3f px" % (e + (float(rms[0]),)))
    # a wrong corner order or id is not a small error: a tag's corners a quarter turn on turn the board by 90 degrees, an id one column
    # off moves it by 65 mm; 10 mm (2.4 % of the depth of 0.42 m) and 2 degrees separate a right pose from either
    assert st[0] == 1 and e[0] <= 0.01 and e[1] <= 2.0
    for grid in ((6, 4), (4, 6)):
        _, _, found = clc.FindChessboardCorners(img, grid, cases.TAG_SIZE, chess_options=clc.ChessOptions(500, 3, 250, 1024, 0), solver=sv)
        assert not found[0]
