"""The chessboard ordering on the device (K26) on the GPU.  clc_chessboard_order_device against the yardstick, the product library's
host clc_chessboard_order, on every case of tests/boardorder_cases.py: index, status and n_labelings equal, worst within 16 eps (the
spacing is sqrt(dx dx + dy dy) against hypot), on the hooks and the product library, a second call the first one's bits, an image alone
its row of the batch, the nullable outputs left out, batches of 0, 1 and 257 images.  clc_find_chessboard_device and
clc_find_chessboard_gpu against clc_find_chessboard bit for bit (the starts are the same integer pixels once index is equal, and the
refinement is deterministic), with and without the refinement; calib.FindChessboardCorners(ordering="device") against its default."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import boardorder_cases as bc  # noqa: E402
import chess_cases  # noqa: E402
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


_YARD = {}  # the yardstick of a case, computed once and left unchanged


def yardstick(name):
    if name not in _YARD:
        _YARD[name] = bc.host_order(bc.cases()[name])
    return _YARD[name]


def device_order(sv, c, optional=True):
    """clc_chessboard_order_device on torch tensors -> host_order's dict (n_labelings and worst None where left out)."""
    import torch
    dev = torch.device("cuda", sv.device)
    k, n = len(c["xy"]), c["cols"] * c["rows"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xy, count, status = up(c["xy"]), up(c["count"]), up(c["status"])
    e = bc.empty_out(k, n, optional)
    index = up(e["index"])
    lab = up(e["n_labelings"]) if optional else None
    worst = up(e["worst"]) if optional else None
    torch.cuda.synchronize()
    sv.chessboard_order_device(xy.data_ptr(), count.data_ptr(), c["xy"].shape[1], k, c["cols"], c["rows"], index.data_ptr(), status.data_ptr(),
                               lab.data_ptr() if optional else 0, worst.data_ptr() if optional else 0)
    return dict(index=index.cpu().numpy(), status=status.cpu().numpy(), n_labelings=lab.cpu().numpy() if optional else None,
                worst=worst.cpu().numpy() if optional else None)


@pytest.mark.parametrize("name", bc.NAMES)
def test_order_device_against_the_yardstick(sv, prod, name):
    c = bc.cases()[name]
    want = yardstick(name)
    got = device_order(sv, c)
    print(name, "status", got["status"], "labelings", got["n_labelings"])
    bc.assert_same_order(got, want, name + ", hooks library")
    bc.assert_same_order(device_order(sv, c), got, name + ", a second call", worst_exact=True)
    first = device_order(prod, c)
    bc.assert_same_order(first, want, name + ", product library")
    bc.assert_same_order(first, got, name + ", product against hooks library", worst_exact=True)
    for k in range(min(len(c["xy"]), 2)):  # each of the first images alone
        one = {key: (v[k:k + 1] if isinstance(v, np.ndarray) else v) for key, v in c.items()}
        alone = device_order(prod, one)
        bc.assert_same_order(alone, {key: v[k:k + 1] for key, v in got.items()}, f"{name}, image {k} alone", worst_exact=True)


def test_nullable_outputs_left_out(prod):
    """index and status inside one sentinel-filled device buffer, n_labelings and worst left out: the results are there and every other
    word of the buffer is untouched."""
    import torch
    c = bc.cases()["refusals"]
    want = yardstick("refusals")
    dev = torch.device("cuda", prod.device)
    k, n, guard = len(c["xy"]), 20, 64
    arena = torch.full((guard + k * n + guard + k + guard,), -77, dtype=torch.int32, device=dev)
    arena[guard + k * n + guard:guard + k * n + guard + k] = torch.from_numpy(c["status"]).to(dev)
    xy, count = torch.from_numpy(c["xy"]).to(dev), torch.from_numpy(c["count"]).to(dev)
    torch.cuda.synchronize()
    base = arena.data_ptr()
    prod.chessboard_order_device(xy.data_ptr(), count.data_ptr(), 20, k, 5, 4, base + 4 * guard, base + 4 * (guard + k * n + guard))
    a = arena.cpu().numpy()
    assert np.array_equal(a[guard:guard + k * n], want["index"].reshape(-1))
    assert np.array_equal(a[guard + k * n + guard:guard + k * n + guard + k], want["status"])
    assert (a[:guard] == -77).all() and (a[guard + k * n:guard + k * n + guard] == -77).all() and (a[-guard:] == -77).all()
    c2 = bc.cases()["scenes"]
    got = device_order(prod, c2, optional=False)
    assert np.array_equal(got["index"], yardstick("scenes")["index"]) and np.array_equal(got["status"], yardstick("scenes")["status"])


@pytest.mark.parametrize("count", (0, 1, 257))
def test_order_device_batches(prod, count):
    c = bc.batch(count)
    want = bc.host_order(c)
    for again in range(2):
        bc.assert_same_order(device_order(prod, c), want, f"{count} images, call {again}")
    if count:
        assert (want["status"] == ref.FOUND).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# Images in, ordered corners out
# ---------------------------------------------------------------------------------------------------------------------------------
def find_device(sv, images, cols, rows, so):
    """clc_find_chessboard_device on torch tensors -> the dict of Solver.find_chessboard."""
    import torch
    dev = torch.device("cuda", sv.device)
    img = torch.from_numpy(np.ascontiguousarray(images)).to(dev)
    n, per = img.shape[0], cols * rows
    corners = torch.full((n, per, 2), -7.0, dtype=torch.float32, device=dev)
    found = torch.full((n,), -7, dtype=torch.int32, device=dev)
    lam = torch.full((n, per), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    sv.find_chessboard_device(img.data_ptr(), img.shape[2], img.shape[1], img.shape[2], n, cols, rows, corners.data_ptr(), found.data_ptr(),
                              lam.data_ptr(), subpix_options=so)
    return dict(corners=corners.cpu().numpy(), found=found.cpu().numpy().astype(bool), strength=lam.cpu().numpy())


def same_bits(a, b, what):
    for key in ("corners", "found", "strength"):
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, key, x.shape, y.shape, x.dtype, y.dtype)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (what, key, x.reshape(-1)[:8], y.reshape(-1)[:8])


@pytest.mark.parametrize("win", (0, 3))
@pytest.mark.parametrize("which", ("accuracy", "batch257"))
def test_find_chessboard_on_the_device_bit_for_bit(sv, prod, which, win):
    from camlasercalibratool_amd import _capi
    if which == "accuracy":
        images = np.stack([sp.board_scene(seed)["image"] for seed in sp.BOARD_SEEDS] + [np.full((sp.BOARD_H, sp.BOARD_W), 128, np.uint8)])
    else:
        images = chess_cases.batch(257)  # 160 x 120, two detection chunks
    cols, rows = sp.INNER
    so = _capi.SubpixOptions(win, win, -1, -1, 30, 0, 0.01) if win else None
    want = prod.find_chessboard(images, cols, rows, subpix_options=so)
    if which == "accuracy":
        assert list(want["found"]) == [True] * 4 + [False] and np.isnan(want["corners"][4]).all() and not np.isnan(want["corners"][:4]).any()
    else:
        assert want["found"].all()
    assert np.isnan(want["strength"]).all() if not win else not np.isnan(want["strength"][want["found"]]).any()
    for s, lib in ((prod, "product"), (sv, "hooks")):
        same_bits(s.find_chessboard(images, cols, rows, subpix_options=so, ordering="device"), want, f"{which} win {win}: clc_find_chessboard_gpu, {lib}")
        same_bits(find_device(s, images, cols, rows, so), want, f"{which} win {win}: clc_find_chessboard_device, {lib}")


def test_find_chessboard_corners_with_device_ordering(sv):
    import camlasercalibratool_amd as clc
    images = np.stack([sp.board_scene(seed)["image"] for seed in sp.BOARD_SEEDS] + [np.full((sp.BOARD_H, sp.BOARD_W), 128, np.uint8)])
    for win in (0, 3, 11):
        a = clc.FindChessboardCorners(images, sp.INNER, sp.SQUARE, refine_win=win, solver=sv)
        b = clc.FindChessboardCorners(images, sp.INNER, sp.SQUARE, refine_win=win, solver=sv, ordering="device")
        assert list(a[2]) == list(b[2]) == [True] * 4 + [False]
        for k in range(5):
            assert np.array_equal(a[0][k].view(np.uint32), b[0][k].view(np.uint32)) and np.array_equal(a[1][k], b[1][k]), (win, k)
