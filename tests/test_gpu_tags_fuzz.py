"""K27 on the GPU at the sizes its loops and packed keys are written for: clc_tag_grid, clc_tag_grid_device and
clc_tag_grid_points_device against the host build of the same header (tests/shim/tags_shim.cpp behind tests/shim/chess_shim.cpp), the
same bits on every output, on the cases of tests/tags_fuzz_cases.py — boards of more than 64 tags, the payload sides 3, 5 and 7, ids and
code tables up to their ends, a board inside a texture of hundreds of candidates and quads with the quad list cut at every place that
matters, 172 unlike images in two launches, the compaction alone on synthetic arrays, and the refinement behind a grid of 72 tags —
through every form, on the hooks build and on the product library, a second call the same.

The restatement does not run here: tests/test_tags_fuzz_cases.py holds the host build to it on every one of these cases, and asserts
what each case is required to show."""
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import chess_cases  # noqa: E402
import subpix_cases as sp  # noqa: E402
import subpix_ref  # noqa: E402
import tags_cases as cases  # noqa: E402
import tags_fuzz_cases as F  # noqa: E402
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
    return cases.build_shims(str(tmp_path_factory.mktemp("tagsfuzz")))


@pytest.fixture(autouse=True)
def wall_time(request):
    t = time.perf_counter()
    yield
    print("%s: %.2f s" % (request.node.name, time.perf_counter() - t))


def host_form(solver, c, images=None, subpix=None):
    img = c["images"] if images is None else images
    return solver.tag_grid(img, c["family"], c["grid"][0], c["grid"][1], cases.options_c(c["options"]), chess_cases.options_c(c["chess"]), subpix,
                           width=c["width"])


def device_form(solver, c, images=None, points=False):
    """clc_tag_grid_device on torch tensors -> the dict of Solver.tag_grid; points: clc_tag_grid_points_device on the result as well ->
    (dict, (corners_px, board_xy, offsets))."""
    import torch
    dev = torch.device("cuda", solver.device)
    img = torch.from_numpy(np.ascontiguousarray(c["images"] if images is None else images)).to(dev)
    cols, rows = c["grid"]
    n, T = img.shape[0], cols * rows
    r = {k: torch.from_numpy(v).to(dev) for k, v in cases.empty_result(n, T).items()}
    torch.cuda.synchronize()
    solver.tag_grid_device(img.data_ptr(), c["width"], img.shape[1], img.shape[2], n, c["family"], cols, rows, r["corners"].data_ptr(),
                           r["hamming"].data_ptr(), r["count"].data_ptr(), r["status"].data_ptr(), r["n_quads"].data_ptr(), r["n_foreign"].data_ptr(),
                           r["n_edges_dropped"].data_ptr(), r["strength"].data_ptr(), cases.options_c(c["options"]), chess_cases.options_c(c["chess"]))
    out = {k: v.cpu().numpy() for k, v in r.items()}
    if not points:
        return out
    return out, device_points(solver, r["corners"], r["hamming"], n, cols, rows)


def device_points(solver, corners, hamming, n, cols, rows):
    """clc_tag_grid_points_device on the device tensors corners and hamming -> (corners_px, board_xy, offsets), the capacity whole."""
    import torch
    T = cols * rows
    px = torch.full((max(n * 4 * T, 1), 2), -7.0, dtype=torch.float32, device=corners.device)
    bd = torch.full((max(n * 4 * T, 1), 2), -7.0, dtype=torch.float32, device=corners.device)
    off = torch.full((n + 1,), -7, dtype=torch.int64, device=corners.device)
    torch.cuda.synchronize()
    solver.tag_grid_points_device(corners.data_ptr(), hamming.data_ptr(), n, cols, rows, F.TAG_SIZE, F.TAG_SPACING, px.data_ptr(), bd.data_ptr(),
                                  off.data_ptr())
    return px.cpu().numpy()[:n * 4 * T], bd.cpu().numpy()[:n * 4 * T], off.cpu().numpy()


def same_points(got, want, what):
    for a, b, which in zip(got, want, ("corners_px", "board_xy", "offsets")):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, which)


def every_form(sv, prod, shims, c, what):
    """Every form on the hooks build and on the product library against the host build; a second call; another pitch; the compaction
    of the result -> the host build's result."""
    want = F.host(shims, c)
    got = host_form(sv, c)
    print(what, "count", got["count"], "quads", got["n_quads"], "foreign", got["n_foreign"], "edges dropped", got["n_edges_dropped"])
    cases.assert_same_bits(got, want, what + ", host form")
    cases.assert_same_bits(device_form(sv, c), want, what + ", device form")
    cases.assert_same_bits(host_form(prod, c), want, what + ", product library")
    cases.assert_same_bits(host_form(prod, c), want, what + ", product library, a second call")
    got, pts = device_form(prod, c, sp.padded(c["images"], c["width"] + 3, fill=201), points=True)
    cases.assert_same_bits(got, want, what + ", product library, device form, another pitch")
    same_points(pts, cases.shim_points(shims, want["corners"], want["hamming"], c["grid"][0], c["grid"][1], F.TAG_SIZE, F.TAG_SPACING), what)
    return want


@pytest.mark.parametrize("name", F.BOARDS)
def test_boards_bit_for_bit(sv, prod, shims, name):
    """More than 64 tags and more than 256 candidates (the 9 x 8 board: 70 tags seen among 502 candidates), and the payload sides 3, 5
    and 7 under both borders (25, 81, 121 and 81 cells)."""
    c = F.board(name)
    want = every_form(sv, prod, shims, c, name)
    if name in F.WIDE_BOARDS:
        assert want["count"][0] >= 57 and (want["hamming"][0, 64:] >= 0).any() == (name == "wide_9x8_d4_b1")
    else:
        assert want["count"][0] == c["grid"][0] * c["grid"][1]


@pytest.mark.parametrize("name", F.SPARSE)
def test_sparse_ids_bit_for_bit(sv, prod, shims, name):
    """Six drawn tags in grids of 65, 128 and 1024 tags, decoded with tables of 1, 17, 1000 and 4096 codes; the planted ties."""
    want = every_form(sv, prod, shims, F.sparse_case(name), name)
    assert want["count"][0] + want["n_foreign"][0] >= 1 and want["n_quads"][0] == 6


@pytest.mark.parametrize("name", F.CROWDS)
def test_crowds_bit_for_bit(sv, prod, shims, name):
    """Hundreds of candidates, of quads and of dropped edges; tags accepted at ranks beyond 256 and 512; every candidate slot taken."""
    want = every_form(sv, prod, shims, F.crowd(name), name)
    assert want["count"][0] == 4 and want["n_quads"][0] > 256


def test_crowd_quad_list_cut_anywhere(sv, prod, shims):
    """max_quads on either side of every tag's rank in crowd_9_cut (253 .. 256), its default, and in the middle of the paths of one p0
    in crowd_10."""
    seen = []
    for max_quads in F.MAX_QUADS:
        c = F.crowd("crowd_9_cut", max_quads or ref.Options().max_quads)
        want = F.host(shims, c)
        seen.append(int(want["count"][0]))
        for solver in (sv, prod):
            cases.assert_same_bits(host_form(solver, c), want, "crowd_9_cut at max_quads %d" % max_quads)
        cases.assert_same_bits(device_form(prod, c), want, "crowd_9_cut at max_quads %d, device form" % max_quads)
    assert seen == [0, 1, 2, 3, 4, 3]
    full = F.host(shims, F.crowd("crowd_10"))
    for max_quads in F.CAP_INSIDE:
        c = F.crowd("crowd_10", max_quads)
        want = F.host(shims, c)
        assert want["n_quads"][0] == full["n_quads"][0] > 1024
        for solver in (sv, prod):
            cases.assert_same_bits(host_form(solver, c), want, "crowd_10 at max_quads %d" % max_quads)
    c = F.crowd("crowd_10", 1024, shifted=True)  # the list full with more quads behind it, and the ids 0 .. 3 not in the image
    want = F.host(shims, c)
    assert list(np.flatnonzero(want["hamming"][0] >= 0)) == [4, 5, 6, 7]
    for solver in (sv, prod):
        cases.assert_same_bits(host_form(solver, c), want, "crowd_10, the ids 4 .. 7")
        cases.assert_same_bits(device_form(solver, c), want, "crowd_10, the ids 4 .. 7, device form")


def test_batch_of_unlike_images(sv, prod, shims):
    """172 images of 320 x 240 — crowded ones, boards, a blank one, one and three candidates, a detection overflow — in an order that puts
    a crowded image and a nearly empty one into the same slot of the two launches: the whole result against the host build's on both
    forms, twice; the first image, the overflow, its neighbours and the last two against the call on that image alone; another pitch."""
    order = F.batch_order()
    c = F.batch_case()
    images = np.ascontiguousarray(c["images"][order])
    want = F.host(shims, c, images)
    o = F.OVERFLOW_AT
    assert want["status"][o] == ref.OVERFLOW and want["count"][o] == 0 and want["n_quads"][o] == 0 and np.isnan(want["corners"][o]).all()
    assert (np.delete(want["status"], o) == ref.OK).all() and want["count"][o - 1] == 4 and want["count"][o + 1] == 4
    wpts = cases.shim_points(shims, want["corners"], want["hamming"], 2, 2, F.TAG_SIZE, F.TAG_SPACING)
    for again in range(2):
        cases.assert_same_bits(host_form(prod, c, images), want, "172 images, host form, call %d" % again)
        got, pts = device_form(prod, c, images, points=True)
        cases.assert_same_bits(got, want, "172 images, device form, call %d" % again)
        same_points(pts, wpts, "172 images")
    cases.assert_same_bits(host_form(sv, c, images), want, "172 images, hooks build")
    cases.assert_same_bits(device_form(sv, c, sp.padded(images, c["width"] + 3, fill=201)), want, "172 images, pitch 323")
    for i in (0, o - 1, o, o + 1, F.BATCH_N - 2, F.BATCH_N - 1):
        alone = device_form(prod, c, images[i:i + 1])
        cases.assert_same_bits(alone, {k: v[i:i + 1] for k, v in got.items()}, "image %d alone" % i)


@pytest.mark.parametrize("n_tags,cols,n_images,pattern", F.COMPACTIONS)
def test_compaction_bit_for_bit(sv, prod, shims, n_tags, cols, n_images, pattern):
    """clc_tag_grid_points_device on synthetic arrays against the host build: the same bytes in all three outputs and nothing written
    behind the last point, on both builds, twice."""
    import torch
    corners, hamming = F.compaction(n_tags, cols, n_images, pattern)
    want = cases.shim_points(shims, corners, hamming, cols, n_tags // cols, F.TAG_SIZE, F.TAG_SPACING)
    assert want[2][-1] == 4 * (hamming >= 0).sum()
    for solver in (sv, prod, prod):
        dev = torch.device("cuda", solver.device)
        # (an empty tensor has no address to hand over: one unused row)
        cd = torch.from_numpy(corners if n_images else np.zeros((1, n_tags, 4, 2), np.float32)).to(dev)
        hd = torch.from_numpy(hamming if n_images else np.zeros((1, n_tags), np.int32)).to(dev)
        same_points(device_points(solver, cd, hd, n_images, cols, n_tags // cols), want, (n_tags, cols, n_images, pattern))


def test_refinement_behind_a_large_grid(sv, prod):
    """clc_tag_grid with the refinement on the 9 x 8 board = clc_tag_grid without it, then clc_corner_subpix on those corners: the same
    bits in the corners and the strengths of all 72 tags (the offsets i 4 T with T > 64); a tag not seen keeps its NaN."""
    c = F.board("wide_9x8_d4_b1")
    T = c["grid"][0] * c["grid"][1]
    o = sp.options_c(subpix_ref.Options(3, 3, -1, -1, 30, 0.01))
    for solver in (sv, prod):
        plain = host_form(solver, c)
        refined = host_form(solver, c, subpix=o)
        two = solver.corner_subpix(c["images"], plain["corners"].reshape(-1, 2), np.array([0, 4 * T], np.int64), o)
        seen = plain["hamming"][0] >= 0
        assert seen.sum() >= 65 and seen[64:].any() and not seen.all()
        cases.assert_same_bits(refined, plain, "what the refinement leaves alone", keys=("hamming", "count", "status", "n_quads", "n_foreign", "n_edges_dropped"))
        assert np.array_equal(refined["corners"].reshape(-1, 2).view(np.uint8), two["corners"].view(np.uint8))
        assert np.array_equal(refined["strength"].reshape(-1).view(np.uint8), two["strength"].view(np.uint8))
        assert np.isnan(refined["corners"][0][~seen]).all() and np.isfinite(refined["corners"][0][seen]).all()
        moved = np.abs(refined["corners"][0][seen] - plain["corners"][0][seen]).max()
        assert moved > 0.0
        # two images, so that the second one's rows begin at 4 T
        both = solver.tag_grid(np.concatenate([c["images"][:, ::-1].copy(), c["images"]]), c["family"], c["grid"][0], c["grid"][1],
                               cases.options_c(c["options"]), chess_cases.options_c(c["chess"]), o, width=c["width"])
        assert np.array_equal(both["corners"][1].view(np.uint8), refined["corners"][0].view(np.uint8))
        assert np.array_equal(both["strength"][1].view(np.uint8), refined["strength"][0].view(np.uint8))
