"""What the calls on a batch of one (clc_solve_multistart, clc_solve_subsets, clc_score_blocks) and the front-end calls
(clc_line_fit_batched(_device), clc_scan_to_points, clc_board_segments, clc_assemble_observations, clc_keyframes, clc_board_poses)
answer to ONE deliberately bad input each: the return code and the beginning of clc_last_error, and for pairs of faults which of the
two is reported.  A record of the host code's behaviour in csrc/abi_batched.hip, abi_frontend.hip and abi_campose.hip, taken from
reading that code: it holds the refusals, their texts and their order still while the host code around them is rearranged.

On the hooks-free product library, through ctypes with every argument spelt out (NULL pointers and zero counts included).  One tiny
upload serves the rows: a batch of ONE problem of 3 poses x 8 points (blocks = poses), a 3-scan ray set of 16 rays each, 2 images x 4
corners; `two` is the same records as a batch of two problems.  At 24 records every lane holds one record, so no block boundary can
fall inside a lane there: the one row that needs a boundary inside a scan's lane uploads 3 poses x 100 points (2 records per lane).

Negative first offset: refused by clc_assemble_observations and clc_board_poses; NOT refused by clc_line_fit_batched,
clc_scan_to_points and clc_board_segments, which take it as the start of the range inside the caller's arrays (the rows pass pointers
16 elements into larger arrays and get the results of the same call with offsets from 0).  clc_line_fit_batched_device and
clc_keyframes see no host offsets.  No timing is asserted."""
import ctypes as C

import numpy as np
import pytest

import camlasercalibratool_amd as clc
import resident_plan_ref as R
from camlasercalibratool_amd import _build, _capi, camera as cam_mod, simdata as sd

pytestmark = pytest.mark.gpu

OK, INVALID, NONFINITE, NO_DATA = 0, -1, -3, -5
Z = C.c_size_t
DEFAULT_FLAGS = 2 | 16 | 32 | 128 | 256 | 512     # kDefaultLaunchFlags (csrc/abi_paths.hpp)
NO_RESIDENT = DEFAULT_FLAGS | 4096                # set after the upload: the lane layout exists, the launch flags rule its kernel out
FAILURE = {v: k for k, v in _capi.TERMINATION.items()}["FAILURE"]

ONE_TEXT = ": the shared observations must be uploaded as a batch of ONE problem (clc_upload_batched, n_problems = 1)"
OFFS_TEXT = ": block_offsets must start at 0 and end at the problem's record count"
WG_TEXT = ": the problem is not held by one workgroup (clc_path_info.batched_resident == 0, or the launch flags rule the resident kernel out): "
SCAN_TEXT = ": a block boundary falls inside a scan (consecutive records of one plane): a block must hold whole scans"


def P(a, first=0):
    """The address of element `first` (along axis 0) of a numpy array; None: NULL."""
    return None if a is None else C.c_void_p(a.ctypes.data + first * a.strides[0])


def ref(x):
    return None if x is None else C.byref(x)


def _records(seed, n_poses, pts):
    rec = clc.flatten_observations(sd.sim_fixed_count(seed, n_poses, pts, noise_sigma=0.01), False, False)
    assert [list(l) for l in R.scan_lengths(rec, [0, rec.shape[0]])] == [[pts] * n_poses]
    return rec


class Env:
    def __init__(self):
        self.sv = clc.Solver(0, library=_build.PRODUCT_LIB_PATH)
        assert not self.sv._L.has_hooks
        self.L = C.CDLL(_build.PRODUCT_LIB_PATH)     # the same loaded library, no argument types attached: every row spells its own
        self.L.clc_last_error.restype = C.c_char_p
        self.h = self.sv._h
        self.state = None
        rng = np.random.default_rng(5)
        self.rec = _records(11, 3, 8)
        self.rec_cut = _records(12, 3, 100)
        assert R.plan(self.rec, [0, 24]).path_info()[:3] == (1, 256, 1) and R.plan(self.rec_cut, [0, 300]).path_info()[:3] == (1, 256, 2)
        self.x = sd.pose7_from_T(sd.tlc_to_tcl(sd.GT_RLC, sd.GT_TLC))
        # front end: 3 scans x 16 rays, every host array with 16 spare elements in front (the negative-first-offset rows)
        self.ranges = rng.uniform(1.0, 3.0, 64).astype(np.float32)
        self.am = np.full(3, -0.5, dtype=np.float32)
        self.ai = np.full(3, 0.01, dtype=np.float32)
        self.rm = np.full(3, 0.1, dtype=np.float32)
        self.points = rng.uniform(-1.0, 1.0, (64, 3))
        self.points[:, 2] = 0.0
        t = rng.uniform(-1.0, 1.0, 64)
        self.xy = np.stack([t, 0.3 * t + 0.5 + rng.normal(size=64) * 0.002], axis=1)
        # 2 images x 4 corners
        self.camera = cam_mod.Camera.pinhole(500.0, 500.0, 320.0, 240.0).to_c()
        self.board = np.array([[0, 0], [.1, 0], [.1, .1], [0, .1]] * 2, dtype=np.float32)
        self.corners = (np.array([[300, 220], [350, 222], [348, 272], [298, 270]] * 2) + rng.normal(size=(8, 2))).astype(np.float32)

    def close(self):
        self.sv.set_launch(0, -1)
        self.sv.close()

    def ensure(self, upload, flags=-1):
        if self.state != (upload, flags):
            self.sv.set_launch(0, -1)
            rec = {"one": self.rec, "two": np.tile(self.rec, (2, 1)), "cut": self.rec_cut}[upload]
            n = rec.shape[0]
            self.sv.upload_batched(rec, np.array([0, n], dtype=np.int64) if upload != "two" else np.array([0, n // 2, n], dtype=np.int64))
            assert self.sv.path_info().batched_resident == 1
            self.sv.set_launch(0, flags)
            self.state = (upload, flags)

    def error(self):
        return self.L.clc_last_error().decode("utf-8", "replace")

    def opt(self, default="clc_options_default", **kw):
        o = _capi.Options()
        getattr(self.L, default)(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def aopt(self, line0=None, **kw):
        o = _capi.AssembleOptions()
        self.L.clc_assemble_options_default(C.byref(o))
        for k, v in kw.items():
            setattr(o.line, k, v)
        if line0 is not None:
            o.line0[0], o.line0[1] = line0
        return o

    def starts(self, n, bad=None):
        p = np.tile(self.x, (n, 1))
        p[:, 0] += 0.01 * np.arange(n)
        if bad is not None:
            p[n - 1, 4] = bad
        return p


# ---- the calls: every argument a keyword with a good default; -> (return code, the arguments used) ----
def multistart(e, **kw):
    a = dict(h=e.h, opt=e.opt(), n=2, poses=e.starts(2), sms=(_capi.Summary * 2)())
    a.update(kw)
    return e.L.clc_solve_multistart(a["h"], ref(a["opt"]), Z(a["n"]), P(a["poses"]), ref(a["sms"])), a


def _blocks(kw, n_rec):
    off = np.asarray(kw.pop("off", [0, n_rec // 3, 2 * (n_rec // 3), n_rec]), dtype=np.int64)
    return off, kw.pop("nb", off.size - 1)


def subsets(e, n_rec=24, **kw):
    off, nb = _blocks(kw, n_rec)
    a = dict(h=e.h, opt=e.opt(), nb=nb, off=off, ns=2, w=np.ones((2, max(off.size - 1, 1)), dtype=np.uint8), poses=e.starts(2),
             sms=(_capi.Summary * 2)())
    a.update(kw)
    return e.L.clc_solve_subsets(a["h"], ref(a["opt"]), Z(a["nb"]), P(a["off"]), Z(a["ns"]), P(a["w"]), P(a["poses"]), ref(a["sms"])), a


def scores(e, n_rec=24, **kw):
    off, nb = _blocks(kw, n_rec)
    cells = 2 * max(off.size - 1, 1)
    a = dict(h=e.h, opt=e.opt(), nb=nb, off=off, ns=2, poses=e.starts(2), tau=0.03, ssq=np.full(cells, -7.0), cost=np.full(cells, -7.0),
             inl=np.full(cells, -7, dtype=np.int32))
    a.update(kw)
    return e.L.clc_score_blocks(a["h"], ref(a["opt"]), Z(a["nb"]), P(a["off"]), Z(a["ns"]), P(a["poses"]), C.c_double(a["tau"]),
                                P(a["ssq"]), P(a["cost"]), P(a["inl"])), a


OFF16 = np.array([0, 16, 32, 48], dtype=np.int64)


def line_fit(e, first=0, **kw):
    a = dict(h=e.h, opt=e.opt("clc_line_options_default"), xy=e.xy, off=OFF16 - first, n=3, lines=np.zeros((3, 2)), sms=(_capi.Summary * 3)())
    a.update(kw)
    return e.L.clc_line_fit_batched(a["h"], ref(a["opt"]), P(a["xy"], first), P(a["off"]), Z(a["n"]), P(a["lines"]), ref(a["sms"])), a


def line_fit_device(e, **kw):
    import torch
    dev = torch.device("cuda", 0)
    a = dict(h=e.h, opt=e.opt("clc_line_options_default"), n=3, xy=torch.from_numpy(e.xy[:48]).to(dev), off=torch.from_numpy(OFF16).to(dev),
             lines=torch.zeros((3, 2), dtype=torch.float64, device=dev))
    a.update(kw)
    torch.cuda.synchronize()
    d = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = e.L.clc_line_fit_batched_device(a["h"], ref(a["opt"]), d(a["xy"]), d(a["off"]), Z(a["n"]), d(a["lines"]), None)
    a["lines_host"] = None if a["lines"] is None else a["lines"].cpu().numpy()
    return rc, a


def scan_points(e, first=0, **kw):
    a = dict(h=e.h, ranges=e.ranges, off=OFF16 - first, n=3, am=e.am, ai=e.ai, rm=e.rm, points=np.full((64, 3), -7.0))
    a.update(kw)
    return e.L.clc_scan_to_points(a["h"], P(a["ranges"], first), P(a["off"]), Z(a["n"]), P(a["am"]), P(a["ai"]), P(a["rm"]),
                                  P(a["points"], first)), a


def segments(e, first=0, **kw):
    a = dict(h=e.h, points=e.points, off=OFF16 - first, n=3, seg=np.full((3, 2), -7, dtype=np.int64), status=np.full(3, -7, dtype=np.int32))
    a.update(kw)
    return e.L.clc_board_segments(a["h"], P(a["points"], first), P(a["off"]), Z(a["n"]), P(a["seg"]), P(a["status"])), a


def assemble(e, **kw):
    q = np.tile([1.0, 0.0, 0.0, 0.0], (2, 1))
    a = dict(h=e.h, opt=e.aopt(), np_=2, stamp=np.array([0.0, 1.0]), q=q, t=np.array([[0.0, 0, 1], [0.5, 0, 1]]), ranges=e.ranges, off=OFF16.copy(),
             n=3, am=e.am, ai=e.ai, rm=e.rm, sstamp=np.array([0.0, 0.5, 1.0]), scan_pose=np.full(3, -7, dtype=np.int32), info=_capi.AssembleInfo())
    a.update(kw)
    return e.L.clc_assemble_observations(a["h"], ref(a["opt"]), Z(a["np_"]), P(a["stamp"]), P(a["q"]), P(a["t"]), P(a["ranges"]), P(a["off"]),
                                         Z(a["n"]), P(a["am"]), P(a["ai"]), P(a["rm"]), P(a["sstamp"]), P(a["scan_pose"]), ref(a["info"])), a


def keyframes(e, **kw):
    a = dict(h=e.h, opt=e.aopt(), n=2, q=np.tile([1.0, 0.0, 0.0, 0.0], (2, 1)), t=np.array([[0.0, 0, 1], [0.5, 0, 1]]),
             keep=np.full(2, 7, dtype=np.uint8), kept=C.c_int64(-7))
    a.update(kw)
    return e.L.clc_keyframes(a["h"], ref(a["opt"]), Z(a["n"]), P(a["q"]), P(a["t"]), P(a["keep"]), ref(a["kept"])), a


def board_poses(e, **kw):
    a = dict(h=e.h, cam=e.camera, opt=e.opt("clc_pose_options_default"), corners=e.corners, board=e.board, off=np.array([0, 4, 8], dtype=np.int64),
             n=2, q=np.full((2, 4), -7.0), t=np.full((2, 3), -7.0), rms=np.full(2, -7.0), status=np.full(2, -7, dtype=np.int32))
    a.update(kw)
    if isinstance(a["cam"], int):
        c = cam_mod.ClcCamera.from_buffer_copy(e.camera)
        c.model = a["cam"]
        a["cam"] = c
    return e.L.clc_board_poses(a["h"], ref(a["cam"]), ref(a["opt"]), P(a["corners"]), P(a["board"]), P(a["off"]), Z(a["n"]), P(a["q"]), P(a["t"]),
                               P(a["rms"]), P(a["status"]), None), a


I64 = lambda *v: np.array(v, dtype=np.int64)
BIG = 1 << 31
NOLOSS0 = dict(use_loss=1, loss_scale_factor=0.0)

# (id, upload, launch flags, call, return code, beginning of clc_last_error)
ROWS = []


def row(name, call, code, text, upload="one", flags=-1):
    ROWS.append(pytest.param(upload, flags, call, code, text, id=name))


def _null_offsets(e, f):
    """(the wrappers size their arrays by the offsets: NULL offsets are passed beside arrays made for three blocks)"""
    if f is subsets:
        return e.L.clc_solve_subsets(e.h, None, Z(3), None, Z(2), P(np.ones((2, 3), dtype=np.uint8)), P(e.starts(2)), ref((_capi.Summary * 2)())), {}
    return e.L.clc_score_blocks(e.h, None, Z(3), None, Z(2), P(e.starts(2)), C.c_double(0.03), P(np.zeros(6)), P(np.zeros(6)),
                                P(np.zeros(6, dtype=np.int32))), {}


for who, f in (("clc_solve_multistart", multistart), ("clc_solve_subsets", subsets), ("clc_score_blocks", scores)):
    s = who[4:]
    blocked = f is not multistart
    count = "n" if f is multistart else "ns"
    row(f"{s}-null-handle", lambda e, f=f: f(e, h=None), INVALID, who + ": bad argument")
    row(f"{s}-null-poses", lambda e, f=f: f(e, poses=None), INVALID, who + ": bad argument")
    row(f"{s}-zero-count", lambda e, f=f, c=count: f(e, **{c: 0}), INVALID, who + ": bad argument")
    row(f"{s}-batch-of-two", lambda e, f=f: f(e), NO_DATA, who + ONE_TEXT, upload="two")
    row(f"{s}-iterations", lambda e, f=f: f(e, opt=e.opt(max_num_iterations=-1)), INVALID, who + ": max_num_iterations < 0")
    row(f"{s}-loss-scale", lambda e, f=f: f(e, opt=e.opt(**NOLOSS0)), INVALID, who + ": loss_scale_factor must be > 0")
    row(f"{s}-default-options", lambda e, f=f: f(e, opt=None), OK, None)
    # two faults: NULL / zero before NO_DATA; NO_DATA before the options; the iteration count before the loss scale
    row(f"{s}-zero-count+batch-of-two", lambda e, f=f, c=count: f(e, **{c: 0}), INVALID, who + ": bad argument", upload="two")
    row(f"{s}-batch-of-two+iterations", lambda e, f=f: f(e, opt=e.opt(max_num_iterations=-1)), NO_DATA, who + ONE_TEXT, upload="two")
    row(f"{s}-iterations+loss-scale", lambda e, f=f: f(e, opt=e.opt(max_num_iterations=-1, **NOLOSS0)), INVALID, who + ": max_num_iterations < 0")
    if not blocked:
        row(f"{s}-null-summaries", lambda e: multistart(e, sms=None), INVALID, who + ": bad argument")
        row(f"{s}-nan-start", lambda e: multistart(e, poses=e.starts(2, np.nan)), NONFINITE, who + ": non-finite initial pose")
        row(f"{s}-iterations+nan-start", lambda e: multistart(e, opt=e.opt(max_num_iterations=-1), poses=e.starts(2, np.inf)), INVALID,
            who + ": max_num_iterations < 0")
        continue
    many = "subsets" if f is subsets else "poses"
    row(f"{s}-null-offsets", lambda e, f=f: _null_offsets(e, f), INVALID, who + ": bad argument")
    row(f"{s}-zero-blocks", lambda e, f=f: f(e, nb=0), INVALID, who + ": bad argument")
    row(f"{s}-too-many", lambda e, f=f: f(e, ns=BIG), INVALID, f"{who}: too many {many}")
    row(f"{s}-too-many-blocks", lambda e, f=f: f(e, nb=BIG), INVALID, who + ": too many blocks")
    row(f"{s}-offsets-start", lambda e, f=f: f(e, off=I64(1, 8, 16, 24)), INVALID, who + OFFS_TEXT)
    row(f"{s}-offsets-end", lambda e, f=f: f(e, off=I64(0, 8, 16, 23)), INVALID, who + OFFS_TEXT)
    row(f"{s}-offsets-monotone", lambda e, f=f: f(e, off=I64(0, 16, 8, 24)), INVALID, who + ": block_offsets not monotone")
    row(f"{s}-not-resident", lambda e, f=f: f(e), INVALID, who + WG_TEXT, flags=NO_RESIDENT)
    row(f"{s}-boundary-in-a-scan", lambda e, f=f: f(e, n_rec=300, off=I64(0, 1, 100, 200, 300)), INVALID, who + SCAN_TEXT, upload="cut")
    row(f"{s}-boundary-on-a-lane-cut", lambda e, f=f: f(e, n_rec=300, off=I64(0, 2, 100, 200, 300)), OK, None, upload="cut")
    # two faults, in the order the call reports them
    row(f"{s}-batch-of-two+too-many", lambda e, f=f: f(e, ns=BIG), NO_DATA, who + ONE_TEXT, upload="two")
    row(f"{s}-too-many+offsets", lambda e, f=f: f(e, ns=BIG, off=I64(1, 8, 16, 24)), INVALID, f"{who}: too many {many}")
    row(f"{s}-start+monotone", lambda e, f=f: f(e, off=I64(1, 16, 8, 24)), INVALID, who + OFFS_TEXT)
    row(f"{s}-offsets+iterations", lambda e, f=f: f(e, off=I64(0, 16, 8, 24), opt=e.opt(max_num_iterations=-1)), INVALID,
        who + ": block_offsets not monotone")
    row(f"{s}-iterations+not-resident", lambda e, f=f: f(e, opt=e.opt(max_num_iterations=-1)), INVALID, who + ": max_num_iterations < 0",
        flags=NO_RESIDENT)
    row(f"{s}-not-resident+boundary", lambda e, f=f: f(e, n_rec=300, off=I64(0, 1, 100, 200, 300)), INVALID, who + WG_TEXT, upload="cut",
        flags=NO_RESIDENT)
    if f is subsets:
        row(f"{s}-null-weights", lambda e: subsets(e, w=None), INVALID, who + ": bad argument")
        row(f"{s}-null-summaries", lambda e: subsets(e, sms=None), INVALID, who + ": bad argument")
        row(f"{s}-nan-start", lambda e: subsets(e, poses=e.starts(2, np.nan)), NONFINITE, who + ": non-finite initial pose")
        row(f"{s}-loss-scale+nan-start", lambda e: subsets(e, opt=e.opt(**NOLOSS0), poses=e.starts(2, -np.inf)), INVALID,
            who + ": loss_scale_factor must be > 0")
        row(f"{s}-nan-start+not-resident", lambda e: subsets(e, poses=e.starts(2, np.nan)), NONFINITE, who + ": non-finite initial pose",
            flags=NO_RESIDENT)
    else:
        row(f"{s}-nan-tau", lambda e: scores(e, tau=float("nan")), INVALID, who + ": bad argument")
        row(f"{s}-nan-pose+not-resident", lambda e: scores(e, poses=e.starts(2, np.nan)), INVALID, who + WG_TEXT, flags=NO_RESIDENT)


LF = "clc_line_fit_batched"
row("line_fit-null-handle", lambda e: line_fit(e, h=None), INVALID, LF + ": bad argument")
row("line_fit-null-lines", lambda e: line_fit(e, lines=None), INVALID, LF + ": bad argument")
row("line_fit-null-xy", lambda e: line_fit(e, xy=None), INVALID, LF + ": bad argument")
row("line_fit-iterations", lambda e: line_fit(e, opt=e.opt("clc_line_options_default", max_num_iterations=-1)), INVALID, LF + ": max_num_iterations < 0")
row("line_fit-loss-scale", lambda e: line_fit(e, opt=e.opt("clc_line_options_default", **NOLOSS0)), INVALID, LF + ": loss_scale_factor must be > 0")
row("line_fit-monotone", lambda e: line_fit(e, off=I64(0, 32, 16, 48)), INVALID, LF + ": offsets not monotone")
row("line_fit-nan-line", lambda e: line_fit(e, lines=np.array([[0, 0], [np.nan, 0], [0, 0.0]])), NONFINITE, LF + ": non-finite initial line")
row("line_fit-zero-scans+iterations", lambda e: line_fit(e, n=0, opt=e.opt("clc_line_options_default", max_num_iterations=-1)), INVALID,
    LF + ": max_num_iterations < 0")
row("line_fit-iterations+monotone", lambda e: line_fit(e, off=I64(0, 32, 16, 48), opt=e.opt("clc_line_options_default", max_num_iterations=-1)),
    INVALID, LF + ": max_num_iterations < 0")
row("line_fit-monotone+nan-line", lambda e: line_fit(e, off=I64(0, 32, 16, 48), lines=np.full((3, 2), np.nan)), INVALID, LF + ": offsets not monotone")
LFD = LF + "_device"
row("line_fit_device-null-handle", lambda e: line_fit_device(e, h=None), INVALID, LFD + ": bad argument")
row("line_fit_device-null-lines", lambda e: line_fit_device(e, lines=None), INVALID, LFD + ": bad argument")
row("line_fit_device-iterations", lambda e: line_fit_device(e, opt=e.opt("clc_line_options_default", max_num_iterations=-1)), INVALID,
    LFD + ": max_num_iterations < 0")
row("line_fit_device-loss-scale", lambda e: line_fit_device(e, opt=e.opt("clc_line_options_default", **NOLOSS0)), INVALID,
    LFD + ": loss_scale_factor must be > 0")
row("line_fit_device-zero-scans+iterations", lambda e: line_fit_device(e, n=0, opt=e.opt("clc_line_options_default", max_num_iterations=-1)), INVALID,
    LFD + ": max_num_iterations < 0")
SP = "clc_scan_to_points"
row("scan_to_points-null-handle", lambda e: scan_points(e, h=None), INVALID, SP + ": bad argument")
row("scan_to_points-null-angles", lambda e: scan_points(e, am=None), INVALID, SP + ": bad argument")
row("scan_to_points-null-ranges", lambda e: scan_points(e, ranges=None), INVALID, SP + ": bad argument")
row("scan_to_points-too-many", lambda e: scan_points(e, n=65536), INVALID, SP + ": at most 65535 scans per call")
row("scan_to_points-monotone", lambda e: scan_points(e, off=I64(0, 32, 16, 48)), INVALID, SP + ": offsets not monotone")
row("scan_to_points-monotone+null-ranges", lambda e: scan_points(e, off=I64(0, 32, 16, 48), ranges=None), INVALID, SP + ": offsets not monotone")
BS = "clc_board_segments"
row("board_segments-null-handle", lambda e: segments(e, h=None), INVALID, BS + ": bad argument")
row("board_segments-null-seg", lambda e: segments(e, seg=None), INVALID, BS + ": bad argument")
row("board_segments-null-points", lambda e: segments(e, points=None), INVALID, BS + ": bad argument")
row("board_segments-too-many", lambda e: segments(e, n=0x1FFFFFFF1), INVALID, BS + ": too many scans")
row("board_segments-monotone", lambda e: segments(e, off=I64(0, 32, 16, 48)), INVALID, BS + ": offsets not monotone")
row("board_segments-monotone+null-points", lambda e: segments(e, off=I64(0, 32, 16, 48), points=None), INVALID, BS + ": offsets not monotone")
AO = "clc_assemble_observations"
row("assemble-null-handle", lambda e: assemble(e, h=None), INVALID, AO + ": bad argument")
row("assemble-null-stamps", lambda e: assemble(e, sstamp=None), INVALID, AO + ": bad argument")
row("assemble-iterations", lambda e: assemble(e, opt=e.aopt(max_num_iterations=-1)), INVALID, AO + ": bad options")
row("assemble-loss-scale", lambda e: assemble(e, opt=e.aopt(**NOLOSS0)), INVALID, AO + ": bad options")
row("assemble-nan-line", lambda e: assemble(e, opt=e.aopt(line0=(0.0, np.nan))), NONFINITE, AO + ": bad options")
row("assemble-negative-offset", lambda e: assemble(e, off=I64(-16, 0, 16, 32)), INVALID, AO + ": negative offset")
row("assemble-monotone", lambda e: assemble(e, off=I64(0, 32, 16, 48)), INVALID, AO + ": offsets not monotone")
row("assemble-null-ranges", lambda e: assemble(e, ranges=None), INVALID, AO + ": NULL ranges")
row("assemble-iterations+negative-offset", lambda e: assemble(e, opt=e.aopt(max_num_iterations=-1), off=I64(-16, 0, 16, 32)), INVALID, AO + ": bad options")
row("assemble-negative-offset+monotone", lambda e: assemble(e, off=I64(-1, 32, 16, 48)), INVALID, AO + ": negative offset")
row("assemble-monotone+null-ranges", lambda e: assemble(e, off=I64(0, 32, 16, 48), ranges=None), INVALID, AO + ": offsets not monotone")
KF = "clc_keyframes"
row("keyframes-null-handle", lambda e: keyframes(e, h=None), INVALID, KF + ": bad argument")
row("keyframes-null-translations", lambda e: keyframes(e, t=None), INVALID, KF + ": bad argument")
row("keyframes-iterations", lambda e: keyframes(e, opt=e.aopt(max_num_iterations=-1)), INVALID, KF + ": bad options")
row("keyframes-loss-scale", lambda e: keyframes(e, opt=e.aopt(**NOLOSS0)), INVALID, KF + ": bad options")
row("keyframes-nan-line", lambda e: keyframes(e, opt=e.aopt(line0=(np.inf, 0.0))), NONFINITE, KF + ": bad options")
BP = "clc_board_poses"
row("board_poses-null-handle", lambda e: board_poses(e, h=None), INVALID, BP + ": bad argument")
row("board_poses-null-status", lambda e: board_poses(e, status=None), INVALID, BP + ": bad argument")
row("board_poses-camera", lambda e: board_poses(e, cam=7), INVALID, BP + ": unknown camera model")
row("board_poses-iterations", lambda e: board_poses(e, opt=e.opt("clc_pose_options_default", max_num_iterations=-1)), INVALID, BP + ": max_num_iterations < 0")
row("board_poses-loss", lambda e: board_poses(e, opt=e.opt("clc_pose_options_default", use_loss=1)), INVALID,
    BP + ": the pose refinement has no loss (use_loss must be 0)")
row("board_poses-too-many", lambda e: board_poses(e, n=BIG), INVALID, BP + ": too many images")
row("board_poses-negative-offset", lambda e: board_poses(e, off=I64(-4, 0, 4)), INVALID, BP + ": negative offset")
row("board_poses-monotone", lambda e: board_poses(e, off=I64(0, 8, 4)), INVALID, BP + ": offsets not monotone")
row("board_poses-null-corners", lambda e: board_poses(e, corners=None), INVALID, BP + ": bad argument")
row("board_poses-camera+iterations", lambda e: board_poses(e, cam=7, opt=e.opt("clc_pose_options_default", max_num_iterations=-1)), INVALID,
    BP + ": unknown camera model")
row("board_poses-zero-images+loss", lambda e: board_poses(e, n=0, opt=e.opt("clc_pose_options_default", use_loss=1)), INVALID,
    BP + ": the pose refinement has no loss (use_loss must be 0)")
row("board_poses-loss+negative-offset", lambda e: board_poses(e, opt=e.opt("clc_pose_options_default", use_loss=1), off=I64(-4, 0, 4)), INVALID,
    BP + ": the pose refinement has no loss (use_loss must be 0)")
row("board_poses-negative-offset+monotone", lambda e: board_poses(e, off=I64(-1, 8, 4)), INVALID, BP + ": negative offset")
row("board_poses-default-options", lambda e: board_poses(e, opt=None), OK, None)


ROWS.sort(key=lambda p: (p.values[0], p.values[1]))     # (stable: one upload per group of rows)


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


@pytest.mark.parametrize("upload,flags,call,code,text", ROWS)
def test_one_bad_input(env, upload, flags, call, code, text):
    env.ensure(upload, flags)
    rc, _ = call(env)
    print(rc, env.error() if rc != OK else "")
    assert rc == code
    if code != OK:
        assert env.error().startswith(text), env.error()


def test_the_refusal_texts_in_full(env):
    """The long texts to their last character (the table compares their beginnings)."""
    env.ensure("one", NO_RESIDENT)
    assert subsets(env)[0] == INVALID
    assert env.error() == "clc_solve_subsets" + WG_TEXT + "materialise the subsets and use clc_solve_batched"
    assert scores(env)[0] == INVALID
    assert env.error() == "clc_score_blocks" + WG_TEXT + "score the poses one by one with clc_factor_evaluate"
    env.ensure("two")
    for who, f in (("clc_solve_multistart", multistart), ("clc_solve_subsets", subsets), ("clc_score_blocks", scores)):
        assert f(env)[0] == NO_DATA and env.error() == who + ONE_TEXT
    env.ensure("cut")
    assert subsets(env, n_rec=300, off=I64(0, 1, 100, 200, 300))[0] == INVALID and env.error() == "clc_solve_subsets" + SCAN_TEXT


def _key(s):
    return (s.termination, s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps, s.num_evaluations, s.initial_cost, s.final_cost)


def test_multistart_without_the_resident_kernel_solves_start_after_start(env):
    """Launch flags that rule the resident kernel out: clc_solve_multistart is not refused — every start is clc_solve_batched of the
    one problem under the same flags, bit for bit (the suite holds that call to the oracle), and ends as the one launch does."""
    env.ensure("one")
    rc, on_chip = multistart(env)
    assert rc == OK
    env.ensure("one", NO_RESIDENT)
    rc, a = multistart(env)
    assert rc == OK
    for k in range(2):
        p, s = env.sv.solve_batched(env.starts(2)[k:k + 1])
        assert np.array_equal(a["poses"][k], p[0]) and _key(a["sms"][k]) == _key(s[0]), k
        assert a["sms"][k].termination not in (0, FAILURE) and a["sms"][k].final_cost <= a["sms"][k].initial_cost
        assert a["sms"][k].termination == on_chip["sms"][k].termination


def test_what_is_accepted(env):
    """The other side of the table: a non-finite pose is a row of NaN / NaN / 0 for clc_score_blocks; a failed refusal leaves the
    handle serving; an empty subset is its own failure."""
    env.ensure("one")
    rc, a = scores(env, poses=env.starts(2, np.nan))
    assert rc == OK
    ssq, cost, inl = (a[k].reshape(2, 3) for k in ("ssq", "cost", "inl"))
    assert np.isnan(ssq[1]).all() and np.isnan(cost[1]).all() and not inl[1].any()
    assert np.all(ssq[0] > 0) and np.all(cost[0] > 0) and np.all((inl[0] >= 0) & (inl[0] <= 8))
    rc, b = scores(env, ssq=None, inl=None)          # optional tables
    assert rc == OK and np.array_equal(b["cost"].reshape(2, 3)[0], cost[0])
    w = np.array([[1, 1, 1], [0, 0, 0]], dtype=np.uint8)
    rc, c = subsets(env, w=w)
    assert rc == OK and c["sms"][1].termination == FAILURE and np.array_equal(c["poses"][1], env.starts(2)[1])
    rc, m = multistart(env)
    assert rc == OK and np.array_equal(c["poses"][0], m["poses"][0]) and _key(c["sms"][0]) == _key(m["sms"][0])


def test_nothing_to_do_touches_nothing(env):
    """n = 0: CLC_OK, every output as it was."""
    rc, a = line_fit(env, n=0, lines=np.full((3, 2), -7.0))
    assert rc == OK and np.all(a["lines"] == -7.0) and all(s.num_iterations == 0 and s.final_cost == 0.0 for s in a["sms"])
    rc, a = line_fit_device(env, n=0)
    assert rc == OK and not a["lines_host"].any()
    rc, a = line_fit_device(env, n=0, xy=None, off=None, lines=None)
    assert rc == OK
    rc, a = scan_points(env, n=0)
    assert rc == OK and np.all(a["points"] == -7.0)
    rc, a = scan_points(env, off=I64(5, 5, 5, 5), ranges=None, points=None)      # scans, but no rays
    assert rc == OK
    rc, a = segments(env, n=0)
    assert rc == OK and np.all(a["seg"] == -7) and np.all(a["status"] == -7)
    rc, a = segments(env, n=0, off=None, seg=None, status=None)
    assert rc == OK
    rc, a = board_poses(env, n=0)
    assert rc == OK and all(np.all(a[k] == -7) for k in ("q", "t", "rms", "status"))
    rc, a = keyframes(env, n=0, q=None, t=None)
    assert rc == OK and a["kept"].value == 0 and np.all(a["keep"] == 7)
    rc, a = assemble(env, n=0, off=I64(0), am=None, ai=None, rm=None, sstamp=None, ranges=None)
    assert rc == OK and np.all(a["scan_pose"] == -7) and a["info"].n_observations == 0


def test_a_negative_first_offset_where_it_is_not_refused(env):
    """clc_line_fit_batched, clc_scan_to_points, clc_board_segments: offsets [-16, 0, 16, 32] on pointers 16 elements into the arrays are
    the call with offsets [0, 16, 32, 48] on the arrays themselves."""
    rc, a = line_fit(env)
    rc2, b = line_fit(env, first=16)
    assert rc == OK and rc2 == OK and b["off"][0] == -16
    assert np.array_equal(a["lines"], b["lines"]) and [_key(s) for s in a["sms"]] == [_key(s) for s in b["sms"]]
    assert np.abs(a["lines"]).max() > 0
    rc, a = scan_points(env)
    rc2, b = scan_points(env, first=16)
    assert rc == OK and rc2 == OK and np.array_equal(a["points"], b["points"])
    assert np.all(a["points"][:48] != -7.0) and np.all(a["points"][48:] == -7.0)
    rc, a = segments(env)
    rc2, b = segments(env, first=16)
    assert rc == OK and rc2 == OK and np.array_equal(a["status"], b["status"]) and np.all(a["status"] != -7)
    assert np.array_equal(a["seg"], b["seg"])      # (indices within a scan: the same whatever the first offset)
