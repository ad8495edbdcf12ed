"""K17 on the MI355X: clc_board_poses_alternate against the host build of the same code (tests/shim/altpose_shim.cpp), scipy and the
restatement (tests/altpose_ref.py) on one batch per camera model sized to go wrong at the lane and slot edges; the images next to a
CLC_ALT_NONE one; clc_board_poses and clc_board_poses_robust before and after on the same handle; the device form behind
offsets_dev[0] > 0; n_images = 0; the Python front end and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import altpose_cases as cases  # noqa: E402
import robustpose_cases as rcases  # noqa: E402
import test_altpose_host as AH  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu
CAMS = AH.CAMS  # both camera models
REAL = ("rms", "cost_in", "cost_alt", "ratio", "rot_angle", "normal_angle")
# The device's costs against the restatement: measured on these batches 1.4e-13 at most (K10's device-side FMA contraction puts
# the device's pose 4e-9 from the host's at most here; at a minimum the cost moves with the square of that: 3.5e-14 relative
# between device and host), asserted at the host test's bound, one decade over it
GPU_COST_GAP_BOUND = AH.COST_GAP_BOUND


@pytest.fixture(scope="module")
def sv():
    with clc.Solver(0) as s:
        yield s


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return AH.build_shim(str(tmp_path_factory.mktemp("apg") / "libaltpose_shim.so"))


@pytest.fixture(scope="module")
def batch(shim):
    """Per camera: the edge shapes plus a few seeded views as ONE batch of at most 40 images (every image under a mask), the input poses
    by the shim's K10, the shim's result and the restatement — computed once."""
    out = {}
    for name in CAMS:
        e = AH.edge_batch(shim, name)
        cam = e["cam"]
        extra = [i for kind, n in (("far", 4), ("block4", 4), ("tag1", 2), ("near", 2)) for i in cases.view(name, kind, n)]
        c2, b2, o2 = rcases.csr([(i[0], i[1]) for i in extra])
        q2, t2, _, st2, _ = AH.H.shim_board_poses(shim, cam, c2, b2, o2)
        assert np.all(st2 == 1)
        e["corners"], e["board"] = np.concatenate([e["corners"], c2]), np.concatenate([e["board"], b2])
        e["off"] = np.concatenate([e["off"], e["off"][-1] + o2[1:]])
        e["mask"] = np.concatenate([e["mask"], np.ones(len(c2), bool)])
        e["q"], e["t"], e["st"] = np.concatenate([e["q"], q2]), np.concatenate([e["t"], t2]), np.concatenate([e["st"], st2]).astype(np.int32)
        assert len(e["off"]) - 1 <= 40
        e["ao"] = AH.shim_options(shim)
        e["s"], e["lifted"], e["rs"] = AH.run_both(shim, e, e["ao"])
        AH.assert_input_condition(e["rs"], e["ao"])
        out[name] = e
    return out


def device(sv, e, sel=None):
    """The host form on the batch (sel: a subset of its images, in order)."""
    off = e["off"]
    if sel is None:
        return sv.board_poses_alternate(e["cam"], e["corners"], e["board"], off, e["q"], e["t"], e["st"], inlier=e["mask"], want_summaries=True)
    idx = np.concatenate([np.arange(off[k], off[k + 1]) for k in sel]) if len(sel) else np.zeros(0, int)
    o = np.concatenate([[0], np.cumsum([off[k + 1] - off[k] for k in sel])]).astype(np.int64)
    return sv.board_poses_alternate(e["cam"], e["corners"][idx], e["board"][idx], o, e["q"][sel], e["t"][sel], e["st"][sel],
                                    inlier=e["mask"][idx], want_summaries=True)


def same_bits(a, b, ia=None, ib=None):
    ia = slice(None) if ia is None else ia
    ib = slice(None) if ib is None else ib
    for key in ("q", "t", "kind", "ambiguous", "better"):
        assert np.array_equal(a[key][ia], b[key][ib]), key
    for key in REAL:
        assert np.array_equal(a[key][ia], b[key][ib], equal_nan=True), key


@pytest.mark.parametrize("name", CAMS)
def test_batch_matches_shim_scipy_and_restatement(sv, batch, name):
    e = batch[name]
    d, s = device(sv, e), e["s"]
    # kind and both flags: the host shim's, the restatement's
    for key in ("kind", "ambiguous", "better"):
        assert np.array_equal(d[key], s[key]), (key, d[key], s[key])
    AH.assert_edge_kinds(d["kind"], e["notes"])
    assert set(d["kind"]) == {0, 1, 2} and d["ambiguous"].any()
    # poses by the two-tier rule against scipy started from the device's answer, costs against the restatement
    gap = AH.assert_matches_restatement(d, e["rs"], e["lifted"], e["board"], e["off"], e["mask"])
    ok = d["kind"] != 0
    dq, dt = np.abs(d["q"] - s["q"]).max(1), np.abs(d["t"] - s["t"]).max(1)
    print("%s: largest relative cost gap to the restatement %.2e; device against host shim: q %.2e t %.2e cost_alt %.2e (relative)"
          % (name, gap, dq[ok].max(), dt[ok].max(), (np.abs(d["cost_alt"] - s["cost_alt"])[ok] / s["cost_alt"][ok]).max()))
    assert gap <= GPU_COST_GAP_BOUND
    # device against host: K10's tolerance (test_gpu_board_poses_robust)
    assert np.all(dq[ok] <= 1e-7) and np.all(dt[ok] <= 1e-7)
    # an image without an alternate: the defined outputs, empty summaries
    for k in np.flatnonzero(~ok):
        sm = d["summaries"][k]
        assert (sm.termination, sm.num_iterations, sm.num_evaluations, sm.final_cost) == (0, 0, 0, 0.0), k
    # a second run gives the same bits
    same_bits(device(sv, e), d)


@pytest.mark.parametrize("name", CAMS)
def test_images_next_to_a_none_image_are_unaffected(sv, batch, name):
    e = batch[name]
    d = device(sv, e)
    keep = np.flatnonzero(d["kind"] != 0)
    assert len(keep) < len(d["kind"])
    same_bits(device(sv, e, keep), d, None, keep)


def test_earlier_calls_keep_their_bits(sv, batch):
    e = batch["radtan"]
    cam = e["cam"]
    imgs = cases.dirty("radtan", 3) + [(i[0], i[1]) for i in cases.view("radtan", "far", 3)]
    corners, board, off = rcases.csr([(i[0], i[1]) for i in imgs])
    before = sv.board_poses(cam, corners, board, off), sv.board_poses_robust(cam, corners, board, off)
    q, t, _, st, _, inl = before[1][:6]
    a = sv.board_poses_alternate(cam, corners, board, off, q, t, st, inlier=inl)
    assert np.all(a["kind"] != 0)
    device(sv, e)
    after = sv.board_poses(cam, corners, board, off), sv.board_poses_robust(cam, corners, board, off)
    for x, y in zip(before[0][:4] + before[1][:4] + before[1][5:], after[0][:4] + after[1][:4] + after[1][5:]):
        assert np.array_equal(x, y, equal_nan=True)


def test_device_form_behind_an_offset_and_zero_images(sv, batch):
    import torch
    e = batch["kb"]
    cam, off = e["cam"], e["off"]
    n, M = len(off) - 1, len(e["corners"])
    a = device(sv, e)
    pad = 7  # 7 corners that belong to no image: offsets_dev[0] = 7
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    dc = up(np.concatenate([np.full((pad, 2), 1e6, np.float32), e["corners"]]))
    db = up(np.concatenate([np.full((pad, 2), -3.0, np.float32), e["board"]]))
    dm = up(np.concatenate([np.ones(pad, np.uint8), e["mask"].astype(np.uint8)]))
    do, dqi, dti, dsi = up(off + pad), up(e["q"]), up(e["t"]), up(e["st"])
    f64 = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=dev)
    out = {k: f64(n) for k in REAL}
    dq, dt = f64(n, 4), f64(n, 3)
    dk = torch.full((n,), -7, dtype=torch.int32, device=dev)
    da, dbt = (torch.full((n,), 9, dtype=torch.uint8, device=dev) for _ in range(2))
    dsm = torch.zeros(n * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sv.board_poses_alternate_device(cam, dc.data_ptr(), db.data_ptr(), do.data_ptr(), n, dqi.data_ptr(), dti.data_ptr(), dsi.data_ptr(),
                                    dk.data_ptr(), inlier_ptr=dm.data_ptr(), q_ptr=dq.data_ptr(), t_ptr=dt.data_ptr(),
                                    rms_ptr=out["rms"].data_ptr(), cost_in_ptr=out["cost_in"].data_ptr(), cost_alt_ptr=out["cost_alt"].data_ptr(),
                                    ratio_ptr=out["ratio"].data_ptr(), rot_angle_ptr=out["rot_angle"].data_ptr(),
                                    normal_angle_ptr=out["normal_angle"].data_ptr(), ambiguous_ptr=da.data_ptr(), better_ptr=dbt.data_ptr(),
                                    summaries_ptr=dsm.data_ptr())
    c = dict({k: v.cpu().numpy() for k, v in out.items()}, q=dq.cpu().numpy(), t=dt.cpu().numpy(), kind=dk.cpu().numpy(),
             ambiguous=da.cpu().numpy().astype(bool), better=dbt.cpu().numpy().astype(bool))
    same_bits(a, c)
    sm = (_capi.Summary * n).from_buffer_copy(dsm.cpu().numpy().tobytes())
    assert all(sm[k].final_cost == a["summaries"][k].final_cost and sm[k].num_iterations == a["summaries"][k].num_iterations for k in range(n))
    # the inputs are left as they were
    assert np.array_equal(dm.cpu().numpy()[pad:].astype(bool), e["mask"]) and np.array_equal(dqi.cpu().numpy(), e["q"])
    # kind alone, and no mask: the images whose mask is all ones give the same kinds
    dk2 = torch.full((n,), -7, dtype=torch.int32, device=dev)
    sv.board_poses_alternate_device(cam, dc.data_ptr(), db.data_ptr(), do.data_ptr(), n, dqi.data_ptr(), dti.data_ptr(), dsi.data_ptr(), dk2.data_ptr())
    full = np.array([e["mask"][off[k]:off[k + 1]].all() for k in range(n)])
    assert np.array_equal(dk2.cpu().numpy()[full], a["kind"][full])
    # zero images: nothing to do, nothing written
    sv.board_poses_alternate_device(cam, dc.data_ptr(), db.data_ptr(), do.data_ptr(), 0, dqi.data_ptr(), dti.data_ptr(), dsi.data_ptr(), dk2.data_ptr())
    z = sv.board_poses_alternate(cam, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.array([0], dtype=np.int64),
                                 np.zeros((0, 4)), np.zeros((0, 3)), np.zeros(0, np.int32))
    assert z["kind"].shape == (0,) and z["q"].shape == (0, 4)


def test_python_front_end(sv):
    cam = cases.CAMERAS["radtan"]
    imgs = cases.dirty("radtan", 2) + [(i[0], i[1]) for i in cases.view("radtan", "far", 3)] + [(i[0], i[1]) for i in cases.view("radtan", "near", 2)]
    corners, board, off = rcases.csr([(i[0], i[1]) for i in imgs])
    q, t, st, keep, table = clc.BoardPosesChecked(cam, corners, board, off, solver=sv)  # robust: the contaminated boards are unambiguous
    assert q.shape == (7, 4) and t.shape == (7, 3) and np.all(st == 1) and "inlier" in table
    assert np.array_equal(keep, ~table["ambiguous"]) and np.array_equal(keep, [True, True, False, False, False, True, True])
    assert np.array_equal(table["kind"][2:5], [2, 2, 2]) and np.array_equal(table["n_inliers"][:2], [123, 123])
    # the plain fit on the clean images: the same poses (every corner an inlier), the same table
    c5 = corners[off[2]:]
    q5, t5, st5, keep5, table5 = clc.BoardPosesChecked(cam, c5, board[off[2]:], off[2:] - off[2], robust=False, solver=sv)
    assert "inlier" not in table5 and np.array_equal(keep5, keep[2:]) and np.array_equal(q5, q[2:]) and np.array_equal(t5, t[2:])
    assert np.array_equal(table5["ratio"], table["ratio"][2:])
    # a gate of 1 keeps every image whose input is the lower minimum
    _, _, _, keep1, table1 = clc.BoardPosesChecked(cam, corners, board, off, ratio_gate=1.0, solver=sv)
    assert np.array_equal(keep1, ~table1["better"])


def test_refusals_come_back_through_the_c_abi(sv):
    cam = cases.CAMERAS["radtan"]
    px, b = rcases.board()[:8] * 100 + 50, rcases.board()[:8]
    off = np.array([0, 8], dtype=np.int64)
    args = (cam, px, b, off, np.array([[1.0, 0, 0, 0]]), np.array([[0.0, 0, 1]]), np.array([1], np.int32))
    for kw, msg in [(dict(same_angle=float("nan")), "same_angle must be finite and > 0"), (dict(same_angle=0.0), "same_angle must be finite and > 0"),
                    (dict(ratio_gate=0.5), "ratio_gate must be finite and >= 1"), (dict(ratio_gate=float("inf")), "ratio_gate must be finite and >= 1")]:
        ao = _capi.default_alt_pose_options()
        for k, v in kw.items():
            setattr(ao, k, v)
        with pytest.raises(clc.ClcError) as ei:
            sv.board_poses_alternate(*args, alt=ao)
        assert ei.value.code == -1 and msg in str(ei.value), str(ei.value)
    with pytest.raises(clc.ClcError) as ei:
        sv.board_poses_alternate(cam, px, b, np.array([0, 8, 4], dtype=np.int64), np.tile([1.0, 0, 0, 0], (2, 1)), np.zeros((2, 3)), np.ones(2, np.int32))
    assert ei.value.code == -1 and "offsets not monotone" in str(ei.value)
    o = _capi.default_pose_options()
    o.use_loss = 1
    with pytest.raises(clc.ClcError) as ei:
        sv.board_poses_alternate(*args, options=o)
    assert ei.value.code == -1
