"""K16 on the MI355X: clc_board_poses_robust against the host build of the same code (tests/shim/robustpose_shim.cpp) and the
sequential restatement (tests/robustpose_ref.py) over the edge shapes; bit for bit against clc_board_poses on clean images and on
the clean corners of contaminated ones; the host form, the device form (offsets_dev[0] > 0) and a second run; and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import robustpose_cases as cases  # noqa: E402
import test_campose_host as H  # noqa: E402
import test_robustpose_host as RH  # noqa: E402

import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu
CAMS = ["radtan", "kb"]  # both camera models


@pytest.fixture(scope="module")
def sv():
    with clc.Solver(0) as s:
        yield s


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return RH.build_shim(str(tmp_path_factory.mktemp("rpg") / "librobustpose_shim.so"))


def device(sv, cam, corners, board, off, ro=None):
    q, t, rms, st, sm, inl, ni, bg, nf = sv.board_poses_robust(cam, corners, board, off, robust=ro, want_summaries=True)
    return {"q": q, "t": t, "rms": rms, "status": st, "sm": sm, "inlier": inl, "n_inliers": ni, "best_group": bg, "n_fits": nf}


def summary_fields(sm, k):
    s = sm[k]
    return (s.termination, s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps, s.num_evaluations, s.initial_cost, s.final_cost)


def same_bits(a, b, n):
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["q"], b["q"]) and np.array_equal(a["t"], b["t"])
    assert np.array_equal(a["rms"], b["rms"], equal_nan=True)
    for key in ("inlier", "n_inliers", "best_group", "n_fits"):
        assert np.array_equal(a[key], b[key]), key
    for k in range(n):
        assert summary_fields(a["sm"], k) == summary_fields(b["sm"], k), k


@pytest.fixture(scope="module")
def edge(shim):
    """Per camera: the edge shapes, the shim's result at max_fits 4 and 1, and the restatement — computed once."""
    out = {}
    for name in CAMS:
        cam = H.CAMERAS[name]
        seq, notes = cases.edge_shapes(cam)
        corners, board, off = cases.csr(seq)
        ro, ro1 = RH.shim_options(shim, cam), RH.shim_options(shim, cam, max_fits=1)
        lifted, rs = RH.restate(shim, cam, corners, board, off, ro)
        RH.assert_input_condition(rs, ro)
        out[name] = dict(shim=shim, cam=cam, seq=seq, notes=notes, corners=corners, board=board, off=off, ro=ro, ro1=ro1,
                         s=RH.shim_robust(shim, cam, corners, board, off, ro), s1=RH.shim_robust(shim, cam, corners, board, off, ro1), rs=rs)
    return out


@pytest.mark.parametrize("name", CAMS)
def test_edge_shapes_match_shim_and_restatement(sv, edge, name):
    e = edge[name]
    cam, corners, board, off, notes = e["cam"], e["corners"], e["board"], e["off"], e["notes"]
    n = len(off) - 1
    d, d1 = device(sv, cam, corners, board, off, e["ro"]), device(sv, cam, corners, board, off, e["ro1"])
    s, s1, rs = e["s"], e["s1"], e["rs"]
    # max_fits = 1: the mask is the winner's first set and n_inliers its count — counts, winner and first masks, exactly
    for key in ("status", "best_group", "n_fits", "n_inliers", "inlier"):
        assert np.array_equal(d1[key], s1[key]), (key, d1[key], s1[key])
        assert np.array_equal(d[key], s[key]), (key, d[key], s[key])
    assert np.all(d1["n_fits"][d1["status"] == 1] == 1)
    # min_inliers = 8: a lone tag's own four corners are no consensus (the consensus kernel's own refusal)
    ro8 = _capi.RobustPoseOptions(e["ro"].hyp_threshold, e["ro"].threshold, 8, 4)
    d8, s8 = device(sv, cam, corners, board, off, ro8), RH.shim_robust(e["shim"], cam, corners, board, off, ro8)
    for key in ("status", "best_group", "n_fits", "n_inliers", "inlier"):
        assert np.array_equal(d8[key], s8[key]), (key, d8[key], s8[key])
    assert d8["status"][notes["n4"]] == -3 and d8["best_group"][notes["n4"]] == -1 and d8["n_fits"][notes["n4"]] == 0
    for k, r in enumerate(rs):
        sl = slice(off[k], off[k + 1])
        assert d["best_group"][k] == r["best_group"] and d["n_fits"][k] == r["n_fits"] and d["status"][k] == r["status"], k
        assert np.array_equal(d["inlier"][sl], r["mask"]) and np.array_equal(d1["inlier"][sl], r["first_mask"] & (d1["status"][k] == 1)), k
        if r["winner"] >= 0 and d1["status"][k] == 1:
            assert d1["n_inliers"][k] == r["counts"][r["winner"]], k
    st = {k: d["status"][v] for k, v in notes.items()}
    assert st["n0"] == st["n3"] == st["all_outliers"] == -3, st
    assert d["best_group"][notes["best_last"]] == 63 and d["best_group"][notes["best_second_chunk"]] == 64
    assert d["best_group"][notes["two_tags_tie"]] == int(np.argmin(s["costs"][notes["two_tags_tie"]]))
    assert d["n_inliers"][notes["nan_corner"]] == 143 and d["n_inliers"][notes["stray"]] == 4
    # poses: K10's device-versus-host tolerance (test_gpu_board_poses: the controller is built with FMA contraction on the device)
    ok = d["status"] == 1
    dq, dt = np.abs(d["q"] - s["q"]).max(1), np.abs(d["t"] - s["t"]).max(1)
    for k in np.flatnonzero(ok & ~((dq <= 1e-12) & (dt <= 1e-12))):
        assert dq[k] <= 1e-7 and dt[k] <= 1e-7, (k, dq[k], dt[k])
        assert abs(d["sm"][k].final_cost - s["sm"][k].final_cost) <= 1e-10 * s["sm"][k].final_cost, k
    assert np.all(np.abs(d["rms"][ok] - s["rms"][ok]) <= 1e-10 * s["rms"][ok] + 1e-15)
    bad = ~ok
    assert np.all(d["q"][bad] == [1, 0, 0, 0]) and np.all(d["t"][bad] == 0) and np.all(np.isnan(d["rms"][bad]))
    assert np.all(d["n_inliers"][bad] == 0) and not any(d["inlier"][off[k]:off[k + 1]].any() for k in np.flatnonzero(bad))
    # the neighbours of the images that end without a pose: the bits they give alone
    for k in sorted({j for b in np.flatnonzero(bad) for j in (b - 1, b + 1) if 0 <= j < n and ok[j]}):
        a = device(sv, cam, e["seq"][k][0], e["seq"][k][1], np.array([0, len(e["seq"][k][0])], dtype=np.int64), e["ro"])
        assert np.array_equal(a["q"][0], d["q"][k]) and np.array_equal(a["t"][0], d["t"][k]) and a["rms"][0] == d["rms"][k], k
        assert np.array_equal(a["inlier"], d["inlier"][off[k]:off[k + 1]])


@pytest.mark.parametrize("name", CAMS)
def test_clean_images_are_bit_identical_to_board_poses(sv, shim, name):
    cam = H.CAMERAS[name]
    rng = np.random.default_rng(41)
    b = cases.board()
    seq = []
    for _ in range(24):
        R, t = cases.pose(rng)
        seq.append((cases.project(cam, b, R, t, rng, noise=0.1), b))
    corners, board, off = cases.csr(seq)
    n = len(seq)
    ro = RH.shim_options(shim, cam)
    s = RH.shim_robust(shim, cam, corners, board, off, ro)
    assert s["first"].all() and s["inlier"].all()  # the premise: every corner an inlier at both stages
    q0, t0, r0, st0, sm0 = sv.board_poses(cam, corners, board, off, want_summaries=True)
    d = device(sv, cam, corners, board, off, ro)
    assert d["inlier"].all() and np.all(d["n_fits"] == 1) and np.all(d["n_inliers"] == 144) and np.all(d["status"] == 1)
    assert np.array_equal(d["q"], q0) and np.array_equal(d["t"], t0) and np.array_equal(d["rms"], r0) and np.array_equal(d["status"], st0)
    for k in range(n):
        assert summary_fields(d["sm"], k) == summary_fields(sm0, k), k
    # clc_board_poses on the same handle afterwards: the same bits as before
    q1, t1, r1, st1, _ = sv.board_poses(cam, corners, board, off)
    assert np.array_equal(q1, q0) and np.array_equal(t1, t0) and np.array_equal(r1, r0) and np.array_equal(st1, st0)


@pytest.mark.parametrize("name", CAMS)
def test_contaminated_images_equal_board_poses_on_the_clean_corners(sv, name):
    cam = H.CAMERAS[name]
    imgs = cases.contaminated_set(cam, 16, 1) + cases.swapped_far_set(cam, 8)
    corners, board, off = cases.csr([(i[0], i[1]) for i in imgs])
    clean = np.concatenate([i[2] for i in imgs])
    coff = np.concatenate([[0], np.cumsum([i[2].sum() for i in imgs])]).astype(np.int64)
    d = device(sv, cam, corners, board, off)  # the default options
    assert np.array_equal(d["inlier"], clean) and np.all(d["status"] == 1)
    assert np.array_equal(d["n_inliers"], np.diff(coff)) and set(d["n_fits"]) <= {1, 2, 3}
    qc, tc, rc, stc, smc = sv.board_poses(cam, corners[clean], board[clean], coff, want_summaries=True)
    assert np.all(stc == 1)
    assert np.array_equal(d["q"], qc) and np.array_equal(d["t"], tc) and np.array_equal(d["rms"], rc)
    for k in range(len(imgs)):
        assert summary_fields(d["sm"], k) == summary_fields(smc, k), k
    # the plain fit on all corners is what the consensus protects from
    q0, t0, _, st0, _ = sv.board_poses(cam, corners, board, off)
    for k in range(16, len(imgs)):  # the swapped-id images
        _, b, _, R, t = imgs[k]
        assert RH.board_distance(b, q0[k], t0[k], R, t) > 10 * RH.board_distance(b, d["q"][k], d["t"][k], R, t), k


def test_host_form_device_form_and_second_run_give_the_same_bits(sv, edge):
    import torch
    e = edge["radtan"]
    cam, off = e["cam"], e["off"]
    n, M = len(off) - 1, len(e["corners"])
    a = device(sv, cam, e["corners"], e["board"], off, e["ro"])
    b = device(sv, cam, e["corners"], e["board"], off, e["ro"])
    same_bits(a, b, n)
    # the device form behind 7 corners that belong to no image: offsets_dev[0] = 7
    pad = 7
    dev = torch.device("cuda:0")
    pc = np.concatenate([np.full((pad, 2), 1e6, np.float32), e["corners"]])
    pb = np.concatenate([np.full((pad, 2), -3.0, np.float32), e["board"]])
    dc, db, do = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pc, pb, off + pad))
    f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
    i32 = lambda: torch.empty(n, dtype=torch.int32, device=dev)
    dq, dt, dr, ds, dni, dbg, dnf = f64(n, 4), f64(n, 3), f64(n), i32(), i32(), i32(), i32()
    dm = torch.full((M + pad,), 9, dtype=torch.uint8, device=dev)
    dsm = torch.empty(n * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for rep in range(2):
        sv.board_poses_robust_device(cam, dc.data_ptr(), db.data_ptr(), do.data_ptr(), n, dq.data_ptr(), dt.data_ptr(), dr.data_ptr(),
                                     ds.data_ptr(), dsm.data_ptr(), dm.data_ptr(), dni.data_ptr(), dbg.data_ptr(), dnf.data_ptr(), robust=e["ro"])
        m = dm.cpu().numpy()
        assert np.all(m[:pad] == 9)  # nothing written in front of the first image
        sm = (_capi.Summary * n).from_buffer_copy(dsm.cpu().numpy().tobytes())
        c = {"q": dq.cpu().numpy(), "t": dt.cpu().numpy(), "rms": dr.cpu().numpy(), "status": ds.cpu().numpy(), "sm": sm,
             "inlier": m[pad:].astype(bool), "n_inliers": dni.cpu().numpy(), "best_group": dbg.cpu().numpy(), "n_fits": dnf.cpu().numpy()}
        same_bits(a, c, n)
    # the nullable outputs left out
    dq2, dt2, ds2 = f64(n, 4), f64(n, 3), i32()
    sv.board_poses_robust_device(cam, dc.data_ptr(), db.data_ptr(), do.data_ptr(), n, dq2.data_ptr(), dt2.data_ptr(), 0, ds2.data_ptr(), 0,
                                 dm.data_ptr(), robust=e["ro"])
    assert np.array_equal(dq2.cpu().numpy(), a["q"]) and np.array_equal(dt2.cpu().numpy(), a["t"]) and np.array_equal(ds2.cpu().numpy(), a["status"])
    assert np.array_equal(dm.cpu().numpy()[pad:].astype(bool), a["inlier"])


def test_python_front_end(sv):
    cam = H.CAMERAS["radtan"]
    imgs = cases.contaminated_set(cam, 3, 1)
    q, t, st, rms, masks, info = clc.CalcCamPosesRobust(cam, [i[0] for i in imgs], [i[1] for i in imgs], solver=sv)
    assert np.all(st == 1) and all(np.array_equal(m, i[2]) for m, i in zip(masks, imgs))
    assert np.array_equal(info["n_inliers"], [123] * 3) and np.all(info["best_group"] >= 0) and np.all(info["n_fits"] >= 1)
    assert q.shape == (3, 4) and t.shape == (3, 3) and np.all(np.isfinite(rms))


def test_refusals_come_back_through_the_c_abi(sv):
    cam = H.CAMERAS["radtan"]
    px, b = cases.board()[:8] * 100 + 50, cases.board()[:8]
    off = np.array([0, 8], dtype=np.int64)
    base = _capi.default_robust_pose_options(cam)
    for kw, msg in [(dict(threshold=float("nan")), "the gates must be finite and > 0"), (dict(hyp_threshold=0.0), "the gates must be finite and > 0"),
                    (dict(hyp_threshold=base.threshold / 2), "hyp_threshold < threshold"), (dict(min_inliers=3), "min_inliers < 4"),
                    (dict(max_fits=0), "max_fits outside 1..8"), (dict(max_fits=9), "max_fits outside 1..8")]:
        ro = _capi.RobustPoseOptions(base.hyp_threshold, base.threshold, base.min_inliers, base.max_fits)
        for k, v in kw.items():
            setattr(ro, k, v)
        with pytest.raises(clc.ClcError) as ei:
            sv.board_poses_robust(cam, px, b, off, robust=ro)
        assert ei.value.code == -1 and msg in str(ei.value), str(ei.value)
    with pytest.raises(clc.ClcError) as ei:
        sv.board_poses_robust(cam, px, b, np.array([0, 8, 4], dtype=np.int64))
    assert ei.value.code == -1 and "offsets not monotone" in str(ei.value)
    o = _capi.default_pose_options()
    o.use_loss = 1
    with pytest.raises(clc.ClcError) as ei:
        sv.board_poses_robust(cam, px, b, off, options=o)
    assert ei.value.code == -1
    # zero images: nothing to do
    q, t, rms, st, _, inl, ni, bg, nf = sv.board_poses_robust(cam, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32), np.array([0], dtype=np.int64))
    assert q.shape == (0, 4) and inl.shape == (0,)
