"""The host-array forms of K10 and K16-K20 (clc_board_poses, _robust, _alternate, clc_joint_refine, clc_camera_guess,
clc_camera_calibrate, clc_score_board_poses, clc_select_board_poses) and of the offline flow (clc_assemble_observations, _stations,
_interpolated, clc_clock_offset_sweep) with their nullable arrays given and NULL, with the arrays
starting at 0 and behind spare elements, and their _device forms on the same data: every run of a call compared with the other runs
of that call BIT FOR BIT.  No fit has to be well posed and nothing has a tolerance: what is held is the host code's staging (which
array goes up, which comes back, from and to which element), the lines of csrc/abi_campose.hip, abi_joint.hip, abi_camcal.hip,
abi_guidance.hip and abi_frontend.hip that the Python wrappers, which always pass every output, do not reach.

The variants of a host form: A every nullable array given, offsets from 0; B every nullable OUTPUT NULL; C as A with spare elements
in front of the CSR arrays and a first offset > 0; D the _device form on C's arrays (K18, K19: with the
status rows of the images outside every problem filled in by the caller, which the host forms do themselves).  Held: the mandatory outputs are the same in A-D,
the optional ones of C and D are A's, and around every host output the sentinels stand: in front of the first offset (the arrays
indexed by the absolute offsets) and in one guard row behind.

On the hooks-free product library, through ctypes with every argument spelt out, as tests/test_gpu_abi_refusals.py.  The shapes are
the smallest at which the arithmetic of the staging can go wrong: an empty last image (two equal offsets at the end), images in front
of the first problem and behind the last, fewer candidates than k."""
import ctypes as C

import numpy as np
import pytest

import camcal_cases as ccases
import guidance_cases as gcases
import joint_cases as jcases
import test_guidance_host as GH
import camlasercalibratool_amd as clc
from camlasercalibratool_amd import _build, _capi, simdata as sd
from camlasercalibratool_amd.camera import ClcCamera

pytestmark = pytest.mark.gpu

Z = C.c_size_t
SENTINEL = {np.dtype(np.float32): -777.25, np.dtype(np.float64): -777.25, np.dtype(np.int32): -777, np.dtype(np.int64): -777,
            np.dtype(np.uint8): 0xAB}
SUMMARY = C.sizeof(_capi.Summary)
# compared of a summary: termination ... final_cost.  Behind them stand solve_ms (the host's wall clock) and eval_kernel_ms /
# eval_kernel_launches, which the board-pose kernels' LM summary does not set (they differ from run to run of the same call)
TIMES = slice(_capi.Summary.solve_ms.offset, SUMMARY)
NAME = "radtan"
SPARE_C, SPARE_P = 4, 3  # spare corners / laser points in front (variant C)


def P(a, first=0):
    """The address of row `first` of a numpy array or of a torch tensor; None: NULL."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return C.c_void_p(a.ctypes.data + first * a.strides[0])
    return C.c_void_p(a.data_ptr() + first * a.stride(0) * a.element_size())


def ref(x):
    return None if x is None else C.byref(x)


class Out:
    """A host output of `count` rows of `width`: `front` sentinel rows in front (an array indexed by the absolute offsets; the call
    gets the address of row 0), one guard row behind.  dtype "summary": rows of clc_summary as bytes."""

    def __init__(self, dtype, count, width=1, front=0):
        if dtype == "summary":
            dtype, width = np.uint8, SUMMARY
        self.front, self.count = front, count
        self.a = np.full((front + count + 1, width), SENTINEL[np.dtype(dtype)], dtype=dtype)

    def get(self):
        s = SENTINEL[self.a.dtype]
        assert np.all(self.a[:self.front] == s), "written in front of the first offset"
        assert np.all(self.a[self.front + self.count:] == s), "written behind the last row"
        return self.a[self.front:self.front + self.count].copy()


def spare(a, front):
    """`front` rows of a value no call should read in front of the rows of a."""
    return np.ascontiguousarray(np.concatenate([np.full((front,) + a.shape[1:], 99, dtype=a.dtype), a]))


def collect(outs, form):
    """{name: Out | tensor | None} -> {name: rows as numpy}; of the summaries the fields a kernel computes."""
    r = {}
    for k, o in outs.items():
        if o is None:
            continue
        v = o.get() if isinstance(o, Out) else o.cpu().numpy()[getattr(o, "front_rows", 0):]
        if v.dtype == np.uint8 and v.ndim == 2 and v.shape[1] == SUMMARY:
            v[:, TIMES] = 0
        r[k] = v
    return r


def same(x, y, keys, what):
    for k in keys:
        assert x[k].tobytes() == y[k].tobytes(), (what, k)


def check_variants(runs, mandatory, optional):
    """runs: {"A": .., "B": .., "C": .., "D": ..} (D optional)."""
    for v in ("B", "C", "D"):
        if v in runs:
            same(runs[v], runs["A"], mandatory, v)
    assert not set(optional) & set(runs["B"])
    for v in ("C", "D"):
        if v in runs:
            same(runs[v], runs["A"], optional, v)


class Env:
    def __init__(self):
        import torch
        self.torch = torch
        self.sv = clc.Solver(0, library=_build.PRODUCT_LIB_PATH)
        assert not self.sv._L.has_hooks
        self.L = C.CDLL(_build.PRODUCT_LIB_PATH)  # the same loaded library, no argument types attached: every call spells its own
        self.L.clc_last_error.restype = C.c_char_p
        self.h = self.sv._h
        self.cam = ccases.CAMERAS[NAME]
        self.ccam = self.cam.to_c()
        self.popt = _capi.Options()
        self.L.clc_pose_options_default(C.byref(self.popt))

    def close(self):
        self.sv.close()

    def ok(self, rc):
        assert rc == 0, self.L.clc_last_error().decode("utf-8", "replace")

    def dev(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        self.torch.cuda.synchronize()
        return t

    def dout(self, dtype, count, width=1, front=0):
        """A device output, filled like an Out (no guard is read back); `front` rows in front are dropped by collect()."""
        if dtype == "summary":
            dtype, width = np.uint8, SUMMARY
        t = self.dev(np.full((front + count, width), SENTINEL[np.dtype(dtype)], dtype=dtype))
        t.front_rows = front
        return t


@pytest.fixture(scope="module")
def e():
    env = Env()
    yield env
    env.close()


# ---- K10, K16, K17: 3 images of 8, 12 and 0 corners (whole tags of four), the empty one last ----
def pose_images():
    imgs = [ccases.images(NAME, 501, 1, ids=(0, 35))[0], ccases.images(NAME, 502, 1, ids=(0, 5, 30))[0]]
    corners = np.concatenate([i[0] for i in imgs]).astype(np.float32)
    board = np.concatenate([i[1] for i in imgs]).astype(np.float32)
    assert corners.shape == (20, 2)
    return corners, board, np.array([0, 8, 20, 20], dtype=np.int64)


def pose_inputs(e, form):
    """-> corners, board, offsets (host arrays, or device tensors for D), first offset, M, n."""
    corners, board, off = pose_images()
    first = 0 if form in "AB" else SPARE_C
    if first:
        corners, board, off = spare(corners, first), spare(board, first), off + first
    if form == "D":
        corners, board, off = e.dev(corners), e.dev(board), e.dev(off)
    return corners, board, off, first, 20, 3


def make(e, form, dtype, count, width=1, front=0, given=True):
    if not given:
        return None
    return e.dout(dtype, count, width, front) if form == "D" else Out(dtype, count, width, front)


def board_poses(e, form):
    corners, board, off, first, M, n = pose_inputs(e, form)
    opt = form != "B"
    o = dict(q=make(e, form, np.float64, n, 4), t=make(e, form, np.float64, n, 3), status=make(e, form, np.int32, n),
             rms=make(e, form, np.float64, n, given=opt), summaries=make(e, form, "summary", n, given=opt))
    f = e.L.clc_board_poses_device if form == "D" else e.L.clc_board_poses
    g = lambda k: P(o[k] if o[k] is None or form == "D" else o[k].a)
    e.ok(f(e.h, ref(e.ccam), ref(e.popt), P(corners), P(board), P(off), Z(n), g("q"), g("t"), g("rms"), g("status"), g("summaries")))
    return collect(o, form)


def test_board_poses_variants(e):
    runs = {v: board_poses(e, v) for v in "ABCD"}
    check_variants(runs, ("q", "t", "status"), ("rms", "summaries"))
    assert list(runs["A"]["status"][:, 0]) == [_capi.POSE_OK, _capi.POSE_OK, _capi.POSE_TOO_FEW]


def board_poses_robust(e, form):
    corners, board, off, first, M, n = pose_inputs(e, form)
    opt = form != "B"
    o = dict(q=make(e, form, np.float64, n, 4), t=make(e, form, np.float64, n, 3), status=make(e, form, np.int32, n),
             inlier=make(e, form, np.uint8, M, front=first),
             rms=make(e, form, np.float64, n, given=opt), summaries=make(e, form, "summary", n, given=opt),
             n_inliers=make(e, form, np.int32, n, given=opt), best_group=make(e, form, np.int32, n, given=opt),
             n_fits=make(e, form, np.int32, n, given=opt))
    f = e.L.clc_board_poses_robust_device if form == "D" else e.L.clc_board_poses_robust
    g = lambda k: P(o[k] if o[k] is None or form == "D" else o[k].a)
    e.ok(f(e.h, ref(e.ccam), ref(e.popt), None, P(corners), P(board), P(off), Z(n), g("q"), g("t"), g("rms"), g("status"),
           g("summaries"), g("inlier"), g("n_inliers"), g("best_group"), g("n_fits")))
    return collect(o, form)


def test_board_poses_robust_variants(e):
    runs = {v: board_poses_robust(e, v) for v in "ABCD"}
    check_variants(runs, ("q", "t", "status", "inlier"), ("rms", "summaries", "n_inliers", "best_group", "n_fits"))
    assert list(runs["A"]["status"][:2, 0]) == [_capi.POSE_OK, _capi.POSE_OK] and runs["A"]["inlier"].sum() > 0


ALT_OPTIONAL = ("q_alt", "t_alt", "rms_alt", "cost_in", "cost_alt", "ratio", "rot_angle", "normal_angle", "ambiguous", "better",
                "summaries")


def board_poses_alternate(e, form, mask, start):
    corners, board, off, first, M, n = pose_inputs(e, form)
    inlier = None if mask is None else spare(mask, first)
    q_in, t_in, st_in = start["q"], start["t"], start["status"]
    if form == "D":
        inlier, q_in, t_in, st_in = (None if inlier is None else e.dev(inlier)), e.dev(q_in), e.dev(t_in), e.dev(st_in)
    opt = form != "B"
    mk = lambda dtype, width=1: make(e, form, dtype, n, width, given=opt)
    o = dict(kind=make(e, form, np.int32, n), q_alt=mk(np.float64, 4), t_alt=mk(np.float64, 3), rms_alt=mk(np.float64),
             cost_in=mk(np.float64), cost_alt=mk(np.float64), ratio=mk(np.float64), rot_angle=mk(np.float64),
             normal_angle=mk(np.float64), ambiguous=mk(np.uint8), better=mk(np.uint8), summaries=mk("summary"))
    f = e.L.clc_board_poses_alternate_device if form == "D" else e.L.clc_board_poses_alternate
    g = lambda k: P(o[k] if o[k] is None or form == "D" else o[k].a)
    e.ok(f(e.h, ref(e.ccam), ref(e.popt), None, P(corners), P(board), P(off), Z(n), P(inlier), P(q_in), P(t_in), P(st_in),
           g("q_alt"), g("t_alt"), g("rms_alt"), g("cost_in"), g("cost_alt"), g("ratio"), g("rot_angle"), g("normal_angle"), g("kind"),
           g("ambiguous"), g("better"), g("summaries")))
    return collect(o, form)


@pytest.mark.parametrize("with_inlier", [False, True])
def test_board_poses_alternate_variants(e, with_inlier):
    start = board_poses(e, "A")
    mask = None
    if with_inlier:  # image 1 without its middle tag
        mask = np.ones((20, 1), dtype=np.uint8)
        mask[12:16] = 0
    runs = {v: board_poses_alternate(e, v, mask, start) for v in "ABCD"}
    check_variants(runs, ("kind",), ALT_OPTIONAL)
    assert np.any(runs["A"]["kind"] != _capi.ALT_NONE)
    if with_inlier:
        assert runs["A"]["cost_in"].tobytes() != board_poses_alternate(e, "A", None, start)["cost_in"].tobytes()


# ---- K18: 2 problems x 2 images of 4 corners and 2 laser points, one image in front of the first problem and one behind the last ----
def joint_inputs():
    p = [jcases.problem(NAME, 511 + k, 2, 4, 2, spread4=True) for k in range(3)]
    loose = [dict(p[2], images=p[2]["images"][:1]), dict(p[2], images=p[2]["images"][1:])]
    a = jcases.arrays([loose[0], p[0], p[1], loose[1]])
    a["prob_off"] = np.array([1, 3, 5], dtype=np.int64)
    a["poses_cl0"] = np.ascontiguousarray(a["poses_cl0"][1:3])
    return a


def joint_refine(e, form, a, start, keep=None, prob_off=True, npr=2):
    n = 6
    first_c, first_p = (0, 0) if form in "AB" else (SPARE_C, SPARE_P)
    corners, board, pts = spare(a["corners"], first_c), spare(a["board"], first_c), spare(a["pts"], first_p)
    coff, poff, proff = a["coff"] + first_c, a["poff"] + first_p, (a["prob_off"] if prob_off else None)
    opt = form != "B"
    if form == "D":
        corners, board, pts, coff, poff = (e.dev(x) for x in (corners, board, pts, coff, poff))
        proff, keep = (None if proff is None else e.dev(proff)), (None if keep is None else e.dev(keep))
        o = dict(q=e.dev(start["q"]), t=e.dev(start["t"]), poses_cl=e.dev(a["poses_cl0"][:npr]))
    else:
        o = dict(q=Out(np.float64, n, 4), t=Out(np.float64, n, 3), poses_cl=Out(np.float64, npr, 7))
        o["q"].a[:n], o["t"].a[:n], o["poses_cl"].a[:npr] = start["q"], start["t"], a["poses_cl0"][:npr]
    o.update(summaries=make(e, form, "summary", npr), status=make(e, form, np.int32, n),
             H_cl=make(e, form, np.float64, npr, 36, given=opt), cost_parts=make(e, form, np.float64, npr, 2, given=opt))
    f = e.L.clc_joint_refine_device if form == "D" else e.L.clc_joint_refine
    g = lambda k: P(o[k] if o[k] is None or form == "D" else o[k].a)
    if form == "D":
        n = device_images(o, n, a["prob_off"] if prob_off else None)
    e.ok(f(e.h, ref(e.ccam), ref(e.popt), None, P(corners), P(board), P(coff), P(pts), P(poff), P(keep), Z(n), P(proff), Z(npr),
           g("q"), g("t"), g("poses_cl"), g("summaries"), g("H_cl"), g("cost_parts"), g("status")))
    return collect(o, form)


def device_images(o, n, prob_off):
    """The _device forms cover the images from problem_offsets[0] on and write no status for an image outside every problem (the
    host forms fill those rows with NOT_KEPT themselves): the status rows start as NOT_KEPT -> the n_images of the call."""
    o["status"].fill_(_capi.JOINT_NOT_KEPT)
    return n - (0 if prob_off is None else int(prob_off[0]))


@pytest.fixture(scope="module")
def joint(e):
    a = joint_inputs()
    o = dict(q=Out(np.float64, 6, 4), t=Out(np.float64, 6, 3), status=Out(np.int32, 6))
    e.ok(e.L.clc_board_poses(e.h, ref(e.ccam), ref(e.popt), P(a["corners"]), P(a["board"]), P(a["coff"]), Z(6), P(o["q"].a), P(o["t"].a),
                             None, P(o["status"].a), None))
    start = collect(o, "A")
    assert np.all(start["status"] == _capi.POSE_OK)
    return a, start


JOINT_MANDATORY = ("q", "t", "poses_cl", "summaries", "status")


@pytest.mark.parametrize("with_keep", [False, True])
def test_joint_refine_variants(e, joint, with_keep):
    a, start = joint
    keep = None
    if with_keep:  # problem 1 without its second image; the images outside the problems stay outside whatever keep says
        keep = np.ones(6, dtype=np.uint8)
        keep[4] = 0
    runs = {v: joint_refine(e, v, a, start, keep) for v in "ABCD"}
    check_variants(runs, JOINT_MANDATORY, ("H_cl", "cost_parts"))
    st = runs["A"]["status"][:, 0]
    assert st[0] == st[5] == _capi.JOINT_NOT_KEPT and np.all(st[1:4] != _capi.JOINT_NOT_KEPT) and (st[4] == _capi.JOINT_NOT_KEPT) == with_keep
    for k in ("q", "t"):  # the images outside the problems keep their start
        assert runs["A"][k][[0, 5]].tobytes() == start[k][[0, 5]].tobytes()
    if with_keep:
        assert runs["A"]["poses_cl"].tobytes() != joint_refine(e, "A", a, start)["poses_cl"].tobytes()


def test_joint_refine_without_problem_offsets(e, joint):
    """problem_offsets = NULL: one problem of all the images, the same as the offsets [0, n] spelt out (run A)."""
    a, start = joint
    one = dict(a, prob_off=np.array([0, 6], dtype=np.int64))
    runs = {v: joint_refine(e, v, one, start, prob_off=(v == "A"), npr=1) for v in "ABCD"}
    check_variants(runs, JOINT_MANDATORY, ("H_cl", "cost_parts"))
    assert np.all(runs["A"]["status"] != _capi.JOINT_NOT_KEPT)


# ---- K19: 2 problems x 2 images x 16 corners behind one image that belongs to no problem, the distortion held ----
CAM_BYTES = C.sizeof(ClcCamera)


@pytest.fixture(scope="module")
def camcal(e):
    imgs = [ccases.images(NAME, 521 + k, 1 if k == 0 else 2, ids=ccases.CORNER_TAGS) for k in range(3)]
    a = ccases.arrays(imgs)
    a["prob_off"] = np.array([1, 3, 5], dtype=np.int64)
    assert list(a["coff"]) == [0, 16, 32, 48, 64, 80]
    start_cam = ccases.start_camera(e.cam).to_c()
    o = dict(q=Out(np.float64, 5, 4), t=Out(np.float64, 5, 3), status=Out(np.int32, 5))
    e.ok(e.L.clc_board_poses(e.h, ref(start_cam), ref(e.popt), P(a["corners"]), P(a["board"]), P(a["coff"]), Z(5), P(o["q"].a), P(o["t"].a),
                             None, P(o["status"].a), None))
    start = collect(o, "A")
    assert np.all(start["status"] == _capi.POSE_OK)
    start["cams"] = np.tile(np.frombuffer(bytes(start_cam), dtype=np.uint8), (2, 1))
    return a, start


def camera_calibrate(e, form, a, start, keep=None):
    n, npr = 5, 2
    first = 0 if form in "AB" else SPARE_C
    corners, board, coff, proff = spare(a["corners"], first), spare(a["board"], first), a["coff"] + first, a["prob_off"]
    co = _capi.CamcalOptions()
    e.L.clc_camcal_options_default(C.byref(co), C.c_int32(e.cam.model))
    co.hold_mask |= 0xF0
    opt = form != "B"
    if form == "D":
        corners, board, coff, proff = (e.dev(x) for x in (corners, board, coff, proff))
        keep = None if keep is None else e.dev(keep)
        o = dict(q=e.dev(start["q"]), t=e.dev(start["t"]), cams=e.dev(start["cams"]))
    else:
        o = dict(q=Out(np.float64, n, 4), t=Out(np.float64, n, 3), cams=Out(np.uint8, npr, CAM_BYTES))
        o["q"].a[:n], o["t"].a[:n], o["cams"].a[:npr] = start["q"], start["t"], start["cams"]
    o.update(summaries=make(e, form, "summary", npr), status=make(e, form, np.int32, n),
             H_cam=make(e, form, np.float64, npr, 64, given=opt), rms_px=make(e, form, np.float64, npr, given=opt))
    f = e.L.clc_camera_calibrate_device if form == "D" else e.L.clc_camera_calibrate
    g = lambda k: P(o[k] if o[k] is None or form == "D" else o[k].a)
    if form == "D":
        n = device_images(o, n, a["prob_off"])
    e.ok(f(e.h, ref(e.popt), ref(co), P(corners), P(board), P(coff), P(keep), Z(n), P(proff), Z(npr), g("cams"), g("q"), g("t"),
           g("summaries"), g("H_cam"), g("rms_px"), g("status")))
    return collect(o, form)


@pytest.mark.parametrize("with_keep", [False, True])
def test_camera_calibrate_variants(e, camcal, with_keep):
    a, start = camcal
    keep = None
    if with_keep:  # problem 1 without its second image
        keep = np.ones(5, dtype=np.uint8)
        keep[4] = 0
    runs = {v: camera_calibrate(e, v, a, start, keep) for v in "ABCD"}
    check_variants(runs, ("q", "t", "cams", "summaries", "status"), ("H_cam", "rms_px"))
    st = runs["A"]["status"][:, 0]
    assert st[0] == _capi.CAMCAL_NOT_KEPT and np.all(st[1:4] != _capi.CAMCAL_NOT_KEPT) and (st[4] == _capi.CAMCAL_NOT_KEPT) == with_keep
    assert runs["A"]["q"][0].tobytes() == start["q"][0].tobytes() and runs["A"]["cams"].tobytes() != start["cams"].tobytes()


def camera_guess(e, form, a):
    first = 0 if form in "AB" else SPARE_C
    corners, board, off = spare(a["corners"], first), spare(a["board"], first), a["coff"] + first
    if form == "D":
        corners, board, off = (e.dev(x) for x in (corners, board, off))
    cam_out, n_used = ClcCamera(), C.c_int32(-777)
    f = e.L.clc_camera_guess_device if form == "D" else e.L.clc_camera_guess
    rc = f(e.h, C.c_int32(e.cam.model), C.c_int32(640), C.c_int32(480), P(corners), P(board), P(off), Z(5), C.byref(cam_out),
           None if form == "B" else C.byref(n_used))
    return rc, bytes(cam_out), n_used.value


def test_camera_guess_variants(e, camcal):
    a, _ = camcal
    runs = {v: camera_guess(e, v, a) for v in "ABCD"}
    for v in "BCD":
        assert runs[v][:2] == runs["A"][:2], v
    assert runs["B"][2] == -777 and runs["C"][2] == runs["D"][2] == runs["A"][2] and 0 <= runs["A"][2] <= 5


# ---- K20: 3 candidates, 65 rays ----
SCORE_KEYS = (("n_hits", np.int32, 1), ("H_add", np.float64, 36), ("sv", np.float64, 6), ("score", np.float64, 1))


def guidance_model(c):
    """T_cl and H0 (None: NULL) as arrays that the caller holds for the length of the call."""
    return np.ascontiguousarray(c["pose_cl"], dtype=np.float64), None if c["H0"] is None else np.ascontiguousarray(c["H0"], dtype=np.float64)


def score(e, c, device, wanted):
    n = 3
    q, t = np.ascontiguousarray(c["q"]), np.ascontiguousarray(c["t"])
    if device:
        q, t = e.dev(q), e.dev(t)
    form = "D" if device else "A"
    o = {k: make(e, form, dt, n, w, given=k in wanted) for k, dt, w in SCORE_KEYS}
    f = e.L.clc_score_board_poses_device if device else e.L.clc_score_board_poses
    g = lambda k: P(o[k] if o[k] is None or device else o[k].a)
    pose_cl, H0 = guidance_model(c)
    e.ok(f(e.h, ref(GH.options_of(c["model"])), P(pose_cl), P(H0), Z(n), P(q), P(t), g("n_hits"), g("H_add"), g("sv"), g("score")))
    return collect(o, form)


def test_score_board_poses_each_output_alone(e):
    c = gcases.shape(65, 3)
    keys = [k for k, _, _ in SCORE_KEYS]
    whole = score(e, c, False, keys)
    assert whole["n_hits"].sum() > 0
    same(score(e, c, True, keys), whole, keys, "device")
    for k in keys:
        for device in (False, True):
            alone = score(e, c, device, [k])
            assert list(alone) == [k]
            same(alone, whole, [k], (k, device))


def select(e, c, device, k, extras):
    q, t = np.ascontiguousarray(c["q"]), np.ascontiguousarray(c["t"])
    if device:
        q, t = e.dev(q), e.dev(t)
    o = dict(chosen=Out(np.int64, k), sv_after=Out(np.float64, k, 6) if extras else None, score_after=Out(np.float64, k) if extras else None,
             H_after=Out(np.float64, 1, 36) if extras else None, n_chosen=Out(np.int32, 1) if extras else None)
    f = e.L.clc_select_board_poses_device if device else e.L.clc_select_board_poses
    g = lambda key: None if o[key] is None else P(o[key].a)
    pose_cl, H0 = guidance_model(c)
    e.ok(f(e.h, ref(GH.options_of(c["model"])), P(pose_cl), P(H0), Z(3), P(q), P(t), Z(k), g("chosen"), g("sv_after"), g("score_after"),
           g("H_after"), g("n_chosen")))
    return collect(o, "A")


@pytest.mark.parametrize("k", [2, 5])
def test_select_board_poses_variants(e, k):
    c = gcases.shape(65, 3)
    extras = ("sv_after", "score_after", "H_after", "n_chosen")
    runs = {"A": select(e, c, False, k, True), "B": select(e, c, False, k, False), "D": select(e, c, True, k, True),
            "C": select(e, c, True, k, False)}  # (C here: the _device form without the optional outputs)
    for v in "BCD":
        same(runs[v], runs["A"], ("chosen",), v)
    same(runs["D"], runs["A"], extras, "D")
    assert not set(extras) & (set(runs["B"]) | set(runs["C"]))
    chosen = runs["A"]["chosen"][:, 0]
    assert runs["A"]["n_chosen"][0, 0] == np.count_nonzero(chosen >= 0) >= 1 and np.all(chosen[3:] == -1)
    assert np.all(np.isnan(runs["A"]["score_after"][3:])) and np.all(np.isnan(runs["A"]["sv_after"][3:]))


# ---- the assemble forms and the clock sweep: 3 scans x 16 rays behind 16 spare rays (no scan that short holds a board segment, so
# the calls agree on "no segment"), and 3 simulated scans of 1 081 rays with a board, where what the call reads as ranges decides the
# stored observations ----
SPARE_R = 16
POSE_STAMP = np.array([0.0, 0.1, 0.2, 0.3, 1.0, 1.1, 1.2, 1.3])  # two stations of four poses, 1 m apart: two key frames
POSE_Q = np.tile([1.0, 0.0, 0.0, 0.0], (8, 1))
POSE_T = np.array([[0.0, 0, 1]] * 4 + [[1.0, 0, 1]] * 4)
SCAN_STAMP = np.array([0.05, 0.15, 1.05])
STORED = ("tag_q", "tag_t", "pts_off", "pts", "ptl_off", "ptl")


def scans_of(shape):
    if shape == 16:
        rng = np.random.default_rng(5)
        return dict(ranges=rng.uniform(1.0, 3.0, 48).astype(np.float32), offsets=np.array([0, 16, 32, 48], dtype=np.int64),
                    angle_min=np.full(3, -0.5, dtype=np.float32), angle_increment=np.full(3, 0.01, dtype=np.float32),
                    range_min=np.full(3, 0.1, dtype=np.float32))
    return sd.sim_laser_scans(7, 3, board_prob=1.0)


def scan_arguments(e, form, scans):
    """The thirteen leading arguments after the options: poses, ranges, offsets, (n_rays,) scan geometry, scan stamps; and what holds
    them alive."""
    r, off = np.ascontiguousarray(scans["ranges"], dtype=np.float32), np.ascontiguousarray(scans["offsets"], dtype=np.int64)
    n_rays = int(off[-1] - off[0])
    if form == "C":
        r, off = spare(r, SPARE_R), off + SPARE_R
    a = [POSE_STAMP, POSE_Q, POSE_T, r, off] + [np.ascontiguousarray(scans[k], dtype=np.float32) for k in ("angle_min", "angle_increment", "range_min")] + [SCAN_STAMP]
    if form == "D":
        a = [e.dev(x) for x in a]
    p = [P(x) for x in a]
    return [Z(8)] + p[:5] + [Z(3)] + ([Z(n_rays)] if form == "D" else []) + p[5:], a


def options_of(e, name):
    o = {"clc_assemble_observations": _capi.AssembleOptions, "clc_assemble_stations": _capi.StationOptions,
         "clc_assemble_interpolated": _capi.InterpOptions, "clc_clock_offset_sweep": _capi.TimeOffsetOptions}[name]()
    getattr(e.L, {"clc_assemble_observations": "clc_assemble_options_default", "clc_assemble_stations": "clc_station_options_default",
                  "clc_assemble_interpolated": "clc_interp_options_default", "clc_clock_offset_sweep": "clc_clock_offset_options_default"}[name])(C.byref(o))
    if name == "clc_assemble_observations":
        o.max_dt = 0.2
    elif name == "clc_assemble_stations":
        o.center_dist_max, o.min_members, o.close_last_run = 0.01, 2, 1
    elif name == "clc_assemble_interpolated":
        o.max_gap = 0.5
    else:
        o.n_offsets, o.interp.max_gap = 3, 0.5
    return o


ASSEMBLE = {"clc_assemble_observations": ((("scan_pose", np.int32),), _capi.AssembleInfo),
            "clc_assemble_stations": ((("scan_station", np.int32),), _capi.StationInfo),
            "clc_assemble_interpolated": ((("scan_bracket", np.int32), ("scan_u", np.float64)), _capi.AssembleInfo)}


def assemble(e, name, form, scans):
    outs, info_type = ASSEMBLE[name]
    args, alive = scan_arguments(e, form, scans)
    given = form != "B"
    o = {k: make(e, form, dt, 3, given=given) for k, dt in outs}
    info = info_type() if given else None
    opt = options_of(e, name)
    g = lambda k: P(o[k] if o[k] is None or form == "D" else o[k].a)
    e.ok(getattr(e.L, name + ("_device" if form == "D" else ""))(e.h, ref(opt), *args, *[g(k) for k, _ in outs], ref(info)))
    r = collect(o, form)
    if given:
        r["info"] = np.frombuffer(bytes(info), dtype=np.uint8).copy()
    stored = e.sv.stored_observations()
    for k in STORED:
        r[k] = np.ascontiguousarray(getattr(stored, k))
    del alive
    return r, info


@pytest.mark.parametrize("shape", [16, 1081])
@pytest.mark.parametrize("name", sorted(ASSEMBLE))
def test_assemble_variants(e, name, shape):
    scans = scans_of(shape)
    runs, infos = {}, {}
    for v in "ABCD":
        runs[v], infos[v] = assemble(e, name, v, scans)
    check_variants(runs, STORED, [k for k, _ in ASSEMBLE[name][0]] + ["info"])
    if shape == 1081:
        assert infos["A"].n_segments >= 1


def clock_sweep(e, form, scans):
    args, alive = scan_arguments(e, form, scans)
    given = form != "B"
    o = dict(offsets=Out(np.float64, 3) if given else None, final_cost=Out(np.float64, 3) if given else None,
             poses=Out(np.float64, 3, 7) if given else None, summaries=Out("summary", 3) if given else None)
    result, opt, pose7 = _capi.TimeOffsetResult(), options_of(e, "clc_clock_offset_sweep"), np.ascontiguousarray(jcases.POSE_CL_TRUE)
    g = lambda k: None if o[k] is None else P(o[k].a)
    f = e.L.clc_clock_offset_sweep_device if form == "D" else e.L.clc_clock_offset_sweep
    e.ok(f(e.h, ref(opt), *args, P(pose7), g("offsets"), g("final_cost"), g("poses"), g("summaries"), ref(result)))
    r = collect(o, "A")
    r["result"] = np.frombuffer(bytes(result), dtype=np.uint8).copy()
    del alive
    return r, result


@pytest.mark.parametrize("shape", [16, 1081])
def test_clock_offset_sweep_variants(e, shape):
    scans = scans_of(shape)
    runs, results = {}, {}
    for v in "ABCD":
        runs[v], results[v] = clock_sweep(e, v, scans)
    check_variants(runs, ("result",), ("offsets", "final_cost", "poses", "summaries"))
    assert list(runs["A"]["offsets"][:, 0]) == [-0.02, 0.0, 0.02]
    assert (results["A"].n_scans_used >= 1) == (shape == 1081)
