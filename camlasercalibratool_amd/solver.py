"""Solver: thin object wrapper over one clc_handle (include/clc.h)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _capi, resample
from ._capi import AltPoseOptions, CamcalOptions, ChessOptions, ChessOrderOptions, FullOptions, GuidanceOptions, Iteration, JointLossOptions, JointOptions, Options, RangeOptions, RobustPoseOptions, SubpixOptions, Summary, TagFamilyC, TagOptions, TERMINATION, check, default_line_options, default_options, dptr, iptr


_Pose7 = C.c_double * 7


@dataclass
class SolveResult:
    pose: np.ndarray  # [tx,ty,tz,qx,qy,qz,qw]
    summary: Summary
    trace: List[Iteration]

    @property
    def termination(self) -> str:
        return TERMINATION.get(self.summary.termination, "?")


def flatten_observations(obs_set, use_linefitting_data: bool = True, use_boundary_constraint: bool = False) -> np.ndarray:
    """Residual-block construction of CamLaserCalibration (src/LaseCamCalCeres.cpp:222-295)
    -> records [N,8] = {n(3), d, p(3), scale}.  Host-side; does not need a GPU."""
    L = _capi.lib()
    n = C.c_int64()
    args = (C.c_int(obs_set.n_poses), dptr(np.ascontiguousarray(obs_set.tag_q, dtype=np.float64)),
            dptr(np.ascontiguousarray(obs_set.tag_t, dtype=np.float64)), iptr(obs_set.pts_off), dptr(obs_set.pts),
            iptr(obs_set.ptl_off), dptr(obs_set.ptl), C.c_int(int(use_linefitting_data)),
            C.c_int(int(use_boundary_constraint)))
    check(L.clc_flatten_observations(*args, None, C.byref(n)), "clc_flatten_observations")
    rec = np.empty((n.value, 8))
    check(L.clc_flatten_observations(*args, dptr(rec), C.byref(n)), "clc_flatten_observations")
    return rec


RESULT_RECORD = 12  # doubles per clc_result_record: pose[7], final_cost, initial_cost, iterations, termination, global index
COMM_ID_BYTES = 128


class TagFamily:
    """The code table of a tag family (clc_tag_family, K27): `codes` [n] uint64 words of side x side payload bits, bit side side - 1 the
    cell (row 0, col 0) of the upright tag, row-major, top row first (the order of the published AprilTag tables); `border` black cells
    around the payload; a decode is accepted at a Hamming distance <= max_hamming.  This package ships no table: a Kalibr board's
    36h11 comes from the user's AprilTag install, TagFamily.generate makes seeded families for tests and printed boards of one's own."""

    def __init__(self, codes, side: int, border: int, max_hamming: int = 1):
        self.codes = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1)
        self.side, self.border, self.max_hamming = int(side), int(border), int(max_hamming)

    def c_struct(self) -> TagFamilyC:
        """clc_tag_family over this object's table (which has to outlive the call)."""
        return TagFamilyC(self.side, self.border, len(self.codes), self.max_hamming, self.codes.ctypes.data)

    @staticmethod
    def cells(word: int, side: int) -> np.ndarray:
        """The payload [side, side] of a word: 1 white, row 0 the top row of the upright tag."""
        n = side * side
        return np.array([(int(word) >> (n - 1 - k)) & 1 for k in range(n)], dtype=np.uint8).reshape(side, side)

    @staticmethod
    def word(cells) -> int:
        w = 0
        for v in np.asarray(cells).reshape(-1):
            w = (w << 1) | int(v)
        return w

    @staticmethod
    def rotations(word: int, side: int):
        """The word as read from each of the tag's four corners in turn (quarter turns of the payload)."""
        m = TagFamily.cells(word, side)
        return [TagFamily.word(np.rot90(m, k)) for k in range(4)]

    @classmethod
    def generate(cls, side: int, n: int, min_hamming: int, seed: int, border: int = 2, max_hamming: int = 1) -> "TagFamily":
        """A seeded greedy search: draw a word, keep it if it is at least min_hamming from every rotation of every kept word and from its
        own three rotations.  Deterministic in (side, n, min_hamming, seed)."""
        if not 3 <= side <= 7:
            raise ValueError("TagFamily.generate: side must be in [3, 7]")
        rng = np.random.default_rng(seed)
        ham = lambda a, b: bin(a ^ b).count("1")
        kept, kept_rot = [], []
        for _ in range(200000):
            if len(kept) == n:
                break
            w = int(rng.integers(0, 1 << (side * side), dtype=np.uint64))
            rot = cls.rotations(w, side)
            if min(ham(w, r) for r in rot[1:]) < min_hamming or any(ham(w, r) < min_hamming for r in kept_rot):
                continue
            kept.append(w); kept_rot += rot
        if len(kept) < n:
            raise ValueError("TagFamily.generate: no %d codes of %d bits at distance %d" % (n, side * side, min_hamming))
        return cls(kept, side, border, max_hamming)


def _images_arg(who: str, images: np.ndarray, width: Optional[int]):
    """The images of a host-array call of the image front end -> (the uint8 array [n, height, pitch], its four C arguments: the pointer,
    width (the pitch unless given), height, pitch)."""
    img = np.ascontiguousarray(images, dtype=np.uint8)
    if img.ndim != 3:
        raise ValueError("%s: images must be [n, height, pitch]" % who)
    return img, (img.ctypes.data_as(C.c_void_p), C.c_int32(img.shape[2] if width is None else width), C.c_int32(img.shape[1]),
                 C.c_int64(img.shape[2]))


def chessboard_order(cand_xy: np.ndarray, count: np.ndarray, cols: int, rows: int, status: Optional[np.ndarray] = None,
                     options: Optional[ChessOrderOptions] = None) -> dict:
    """clc_chessboard_order (K25; host code: no Solver, no device): cand_xy [n, stride, 2] and count [n] as Solver.chess_corners returns
    them (status: its status, -2 passes through) -> dict(index [n, rows, cols] int32: the candidate slot of node (j, i) at [i, j], -1
    where no grid was found; status [n]: 1 found, 0 too few candidates, -1 no grid, -2 overflow; n_labelings [n]; worst [n])."""
    xy = np.ascontiguousarray(cand_xy, dtype=np.float32)
    if xy.ndim != 3 or xy.shape[2] != 2:
        raise ValueError("chessboard_order: cand_xy must be [n, stride, 2]")
    n, stride = xy.shape[0], xy.shape[1]
    cnt = np.ascontiguousarray(count, dtype=np.int32)
    if cnt.shape != (n,):
        raise ValueError("chessboard_order: count needs one entry per image")
    st = np.ones(n, np.int32) if status is None else np.array(status, dtype=np.int32).reshape(n)
    per = max(int(cols) * int(rows), 1)
    index = np.full((n, per), -1, np.int32); lab = np.zeros(n, np.int32); worst = np.full(n, np.nan)
    V = lambda a: a.ctypes.data_as(C.c_void_p)
    o = C.byref(options) if options is not None else None
    check(_capi.lib().clc_chessboard_order(V(xy), V(cnt), C.c_int64(stride), C.c_size_t(n), C.c_int32(cols), C.c_int32(rows), o, V(index), V(st),
                                           V(lab), V(worst)), "clc_chessboard_order")
    return dict(index=index.reshape(n, rows, cols) if per == cols * rows else index, status=st, n_labelings=lab, worst=worst)


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the C-ABI: called by ONE rank, distributed to the others out of band."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    check(_capi.lib().clc_comm_unique_id(buf), "clc_comm_unique_id")
    return buf.raw


class Comm:
    """RCCL communicator bound to one Solver (clc_comm): collectives run on the solver's stream.
    Creating it is a collective call — every rank of the job must do so with the same id."""

    def __init__(self, solver: "Solver", uid: Optional[bytes], rank: int, world: int):
        """uid None (hooks build only, tests): a communicator laid out as `rank` of `world` without RCCL behind it — its all-gather
        moves this rank's segment into place and nothing else (clc_debug_comm_create_layout)."""
        self._L = solver._L
        self._c = C.c_void_p()
        self._solver = solver  # keep the handle alive
        if uid is None:
            check(solver._hook("clc_debug_comm_create_layout")(C.byref(self._c), solver._h, C.c_int(rank), C.c_int(world)), "clc_debug_comm_create_layout")
        else:
            assert len(uid) == COMM_ID_BYTES
            check(self._L.clc_comm_create(C.byref(self._c), solver._h, C.c_char_p(uid), C.c_int(rank), C.c_int(world)),
                  "clc_comm_create")
        self.rank, self.world = rank, world

    @property
    def library(self) -> str:
        return self._L.clc_comm_library().decode()

    @property
    def rccl_ranks(self) -> int:
        """Size of the communicator as RCCL reports it (ncclCommCount)."""
        return int(self._L.clc_comm_world(self._c))

    def gather_results(self, first_global_index: int, cap_per_rank: int, copy: bool = True) -> np.ndarray:
        """ncclAllGather of the result records of the solver's last solve_batched -> [world*cap_per_rank, 12]
        (rank-major; padding records have global index -1).  copy=False returns a view of the communicator's
        pinned host buffer (valid until the next gather) instead of a fresh array."""
        n = self.world * cap_per_rank
        if copy:
            out = np.empty((n, RESULT_RECORD))
            check(self._L.clc_gather_results(self._c, C.c_int64(first_global_index), C.c_size_t(cap_per_rank), dptr(out)),
                  "clc_gather_results")
            return out
        check(self._L.clc_gather_results(self._c, C.c_int64(first_global_index), C.c_size_t(cap_per_rank), None),
              "clc_gather_results")
        return np.ctypeslib.as_array(self._L.clc_comm_records(self._c), shape=(n, RESULT_RECORD))

    def solve_gather(self, poses0: np.ndarray, first_global_index: int, cap_per_rank: int, options: Optional[Options] = None,
                     copy: bool = True):
        """clc_solve_batched_gather: the solver's uploaded shard solved by ONE launch whose epilogue writes the result records into
        the gather buffer, all-gather in place, one copy to the host -> (records [world*cap_per_rank, 12], BatchStats of the local
        shard).  poses0: [P_local, 7] start poses (None: the handle's pinned buffer, batched_buffers()[0], already filled).
        copy=False: `records` is a view of the communicator's pinned host buffer (valid until the next gather)."""
        n = self.world * cap_per_rank
        st = _capi.BatchStats()
        o = options or default_options()
        if poses0 is None:
            pp = C.POINTER(C.c_double)()
            if self._solver.num_problems > 0:
                check(self._L.clc_batched_host_buffers(self._solver._h, C.byref(pp), None), "clc_batched_host_buffers")
            p_arg = C.cast(pp, C.c_void_p)
        else:
            poses = np.ascontiguousarray(poses0, dtype=np.float64)
            assert poses.size == 7 * self._solver.num_problems, "one start pose per local problem"
            p_arg = C.cast(dptr(poses), C.c_void_p)
        out = np.empty((n, RESULT_RECORD)) if copy else None
        check(self._L.clc_solve_batched_gather(self._c, C.byref(o), p_arg, C.c_int64(first_global_index), C.c_size_t(cap_per_rank),
                                               dptr(out) if copy else None, C.byref(st)), "clc_solve_batched_gather")
        if not copy:
            out = np.ctypeslib.as_array(self._L.clc_comm_records(self._c), shape=(n, RESULT_RECORD))
        return out, st

    def set_root(self, root: int = -1):
        """clc_comm_set_root: -1 = every rank receives (and copies to its host) every record; r >= 0 = only rank r does (ncclGather to r),
        the other ranks keep their own segment only.  Every rank must choose the same root."""
        check(self._L.clc_comm_set_root(self._c, C.c_int(root)), "clc_comm_set_root")

    def info(self) -> "_capi.CommInfo":
        ci = _capi.CommInfo()
        check(self._L.clc_comm_get_info(self._c, C.byref(ci)), "clc_comm_get_info")
        return ci

    def _records_view(self, ptr, n):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(n, RESULT_RECORD))

    def solve_gather_pipelined(self, poses0: np.ndarray, first_global_index: int, cap_per_rank: int, options: Optional[Options] = None):
        """clc_solve_batched_gather_pipelined: enqueue THIS step, get the PREVIOUS step's (records view [world*cap_per_rank, 12], BatchStats)
        — (None, None) on the first call.  The view stays valid until the NEXT pipelined call / flush; flush() returns the last step's."""
        n = self.world * cap_per_rank
        st = _capi.BatchStats()
        o = options or default_options()
        if poses0 is None:
            pp = C.POINTER(C.c_double)()
            if self._solver.num_problems > 0:
                check(self._L.clc_batched_host_buffers(self._solver._h, C.byref(pp), None), "clc_batched_host_buffers")
            p_arg = C.cast(pp, C.c_void_p)
        else:
            poses = np.ascontiguousarray(poses0, dtype=np.float64)
            assert poses.size == 7 * self._solver.num_problems, "one start pose per local problem"
            p_arg = C.cast(dptr(poses), C.c_void_p)
        prev = C.c_void_p()
        check(self._L.clc_solve_batched_gather_pipelined(self._c, C.byref(o), p_arg, C.c_int64(first_global_index), C.c_size_t(cap_per_rank),
                                                         C.byref(prev), C.byref(st)), "clc_solve_batched_gather_pipelined")
        if not prev.value:
            return None, None
        return self._records_view(prev, n), st

    def flush(self, cap_per_rank: int):
        """clc_gather_flush: complete the step in flight -> (records view, BatchStats), or (None, None) when none is."""
        st = _capi.BatchStats()
        rec = C.c_void_p()
        check(self._L.clc_gather_flush(self._c, C.byref(rec), C.byref(st)), "clc_gather_flush")
        if not rec.value:
            return None, None
        return self._records_view(rec, self.world * cap_per_rank), st

    def close(self):
        if getattr(self, "_c", None) is not None and self._c:
            self._L.clc_comm_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Solver:
    """One solver context on one GPU (one HIP stream).  Not thread-safe per instance.
    library: None = the build the package runs on (the product library unless CLC_LIBRARY names another), "hooks" = the
    -DCLC_TEST_HOOKS build (the debug_* / time_* methods other than the layout reports need it), or a path."""

    def __init__(self, device: int = 0, library: Optional[str] = None):
        self._L = _capi.lib() if library is None else (_capi.hooks_lib() if library == "hooks" else _capi.load(library))
        self._h = C.c_void_p()
        check(self._L.clc_create(C.byref(self._h), C.c_int(device)), "clc_create")
        self.device = device

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.clc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- configuration ----
    def set_stream(self, hip_stream: Optional[int]):
        check(self._L.clc_set_stream(self._h, C.c_void_p(hip_stream or 0)), "clc_set_stream")

    def set_auto_paths(self, disable_mask: int = 0):
        """clc_set_auto_paths: 1 = no cooperative one-launch solve, 2 = no single-workgroup on-chip solve, 8 = (at upload) not the
        32-workgroup one-hop form; 0 = library default.  Every bit disables a path."""
        check(self._L.clc_set_auto_paths(self._h, C.c_int(disable_mask)), "clc_set_auto_paths")

    def set_small_on_coop(self, enable: bool = True):
        """clc_set_small_on_coop (at upload): problems one workgroup holds also get the cooperative layout and run on 32 workgroups first."""
        check(self._L.clc_set_small_on_coop(self._h, C.c_int(int(enable))), "clc_set_small_on_coop")

    def debug_fast_small(self, enable: Optional[bool] = None) -> int:
        """Test hook: switch the host-planned upload of small problems on / off (None: leave it) -> uploads that took it so far."""
        n = C.c_longlong()
        check(self._hook("clc_debug_fast_small")(self._h, C.c_int(-1 if enable is None else int(enable)), C.byref(n)), "clc_debug_fast_small")
        return n.value

    def debug_single_controller(self, cooperative_kernels: bool):
        """Test hook: the single-workgroup solve runs the cooperative kernel's register-state LM controller instead of its own."""
        check(self._hook("clc_debug_single_controller")(self._h, C.c_int(int(cooperative_kernels))), "clc_debug_single_controller")

    def set_launch(self, grid_blocks: int = 0, flags: int = 0):
        check(self._L.clc_set_launch(self._h, C.c_int(grid_blocks), C.c_int(flags)), "clc_set_launch")

    def device_info(self) -> Tuple[str, int]:
        buf = C.create_string_buffer(256)
        n = C.c_int()
        check(self._L.clc_device_info(self._h, buf, C.c_int(256), C.byref(n)), "clc_device_info")
        return buf.value.decode(), n.value

    # ---- data ----
    def upload(self, records: np.ndarray):
        records = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 8)
        check(self._L.clc_upload(self._h, dptr(records), C.c_size_t(records.shape[0])), "clc_upload")

    def upload_device(self, device_ptr: int, n: int):
        """records already in HBM as an [n,8] float64 AoS array (e.g. torch tensor .data_ptr())."""
        check(self._L.clc_upload_device(self._h, C.c_void_p(device_ptr), C.c_size_t(n)), "clc_upload_device")

    @property
    def num_observations(self) -> int:
        return int(self._L.clc_num_observations(self._h))

    # ---- resident scans: problem assembly on the device ----
    def store_observations(self, obs_set):
        """Upload the pose-major form of std::vector<Oberserve> (tag poses + scan points, 24 B per point) once; it stays
        resident for any number of select_observations calls."""
        S = obs_set
        check(self._L.clc_store_observations(self._h, C.c_int(S.n_poses), dptr(np.ascontiguousarray(S.tag_q, dtype=np.float64)),
                                             dptr(np.ascontiguousarray(S.tag_t, dtype=np.float64)), iptr(S.pts_off), dptr(S.pts),
                                             iptr(S.ptl_off), dptr(S.ptl)), "clc_store_observations")

    @property
    def store_generation(self) -> int:
        """Stamp of the scans currently stored on this handle (bumped by every store_observations)."""
        return int(self._L.clc_store_generation(self._h))

    def select_observations(self, use_linefitting_data: bool = True, use_boundary_constraint: bool = False) -> int:
        """Build the residual blocks of the selection on the device (src/LaseCamCalCeres.cpp:222-295) and make them the
        handle's observation array (as upload() would) -> number of records."""
        n = C.c_int64()
        check(self._L.clc_select_observations(self._h, C.c_int(int(use_linefitting_data)), C.c_int(int(use_boundary_constraint)),
                                              C.byref(n)), "clc_select_observations")
        return n.value

    def debug_flatten_device(self, use_linefitting_data: bool = True, use_boundary_constraint: bool = False) -> np.ndarray:
        """The device-built records of a selection, copied back (test hook)."""
        n = C.c_int64()
        check(self._hook("clc_debug_flatten_device")(self._h, C.c_int(int(use_linefitting_data)), C.c_int(int(use_boundary_constraint)),
                                               None, C.c_int64(0), C.byref(n)), "clc_debug_flatten_device")
        rec = np.empty((n.value, 8))
        if n.value:
            check(self._hook("clc_debug_flatten_device")(self._h, C.c_int(int(use_linefitting_data)), C.c_int(int(use_boundary_constraint)),
                                                   dptr(rec), C.c_int64(n.value), C.byref(n)), "clc_debug_flatten_device")
        return rec

    # ---- plug-in level ----
    def factor_evaluate(self, pose: np.ndarray, want_jacobian: bool = True):
        n = self.num_observations
        r = np.empty(n)
        j = np.empty((n, 7)) if want_jacobian else None
        check(self._L.clc_factor_evaluate(self._h, dptr(np.ascontiguousarray(pose, dtype=np.float64)), dptr(r), dptr(j)),
              "clc_factor_evaluate")
        return r, j

    def pose_plus(self, x: np.ndarray, delta: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 7)
        delta = np.ascontiguousarray(delta, dtype=np.float64).reshape(-1, 6)
        out = np.empty_like(x)
        check(self._L.clc_pose_plus(self._h, dptr(x), dptr(delta), dptr(out), C.c_size_t(x.shape[0])), "clc_pose_plus")
        return out

    # ---- evaluation / solve ----
    def eval(self, pose: np.ndarray, with_loss: bool = True, loss_scale_factor: float = 0.05, want_jacobian: bool = True):
        """-> (cost, g[6], H[21])  (g, H None for a cost-only pass)."""
        cost = C.c_double()
        g = np.empty(6) if want_jacobian else None
        H = np.empty(21) if want_jacobian else None
        check(self._L.clc_eval(self._h, dptr(np.ascontiguousarray(pose, dtype=np.float64)), C.c_int(int(with_loss)),
                               C.c_double(loss_scale_factor), C.byref(cost), dptr(g), dptr(H)), "clc_eval")
        return cost.value, g, H

    def solve(self, pose0: np.ndarray, options: Optional[Options] = None, trace_cap: int = 256) -> SolveResult:
        pose = np.array(pose0, dtype=np.float64).reshape(7)  # (a copy: in/out)
        s = Summary()
        tr = (Iteration * trace_cap)() if trace_cap > 0 else None
        o = options or default_options()
        # (a ctypes view of the array's buffer: numpy's .ctypes.data_as() costs 2.7 us per call, 3 % of a C2 solve)
        check(self._L.clc_solve(self._h, C.byref(o), _Pose7.from_buffer(pose), C.byref(s), tr, trace_cap), "clc_solve")
        n = max(0, min(trace_cap, s.num_iterations + 1))
        return SolveResult(pose, s, [tr[i] for i in range(n)])

    def information(self, pose: np.ndarray):
        """Analysis pass (src/LaseCamCalCeres.cpp:316-381) -> (H[6,6], b[6], chi2, sv[6], V[6,6], n_null)."""
        H = np.empty(36); b = np.empty(6); chi = C.c_double(); sv = np.empty(6); V = np.empty(36); nn = C.c_int()
        check(self._L.clc_information(self._h, dptr(np.ascontiguousarray(pose, dtype=np.float64)), dptr(H), dptr(b),
                                      C.byref(chi), dptr(sv), dptr(V), C.byref(nn)), "clc_information")
        return H.reshape(6, 6), b, chi.value, sv, V.reshape(6, 6), nn.value

    def closed_form(self):
        """CamLaserCalClosedSolution on the uploaded records -> (Tlc[4,4], unobservable, sv9)."""
        T = np.empty(16); un = C.c_int(); sv = np.empty(9)
        check(self._L.clc_closed_form(self._h, dptr(T), C.byref(un), dptr(sv)), "clc_closed_form")
        return T.reshape(4, 4), bool(un.value), sv

    # ---- batched ----
    def upload_batched(self, records: np.ndarray, offsets: np.ndarray):
        records = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        check(self._L.clc_upload_batched(self._h, dptr(records), iptr(offsets), C.c_size_t(len(offsets) - 1)),
              "clc_upload_batched")

    def upload_batched_device(self, device_ptr: int, offsets: np.ndarray):
        """records already in HBM as an [N,8] float64 AoS array (ready on the solver's stream); offsets on the host."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        check(self._L.clc_upload_batched_device(self._h, C.c_void_p(device_ptr), iptr(offsets), C.c_size_t(len(offsets) - 1)),
              "clc_upload_batched_device")

    @property
    def num_problems(self) -> int:
        return int(self._L.clc_num_problems(self._h))

    def batched_buffers(self):
        """The handle's own pinned host arrays of the uploaded batch -> (poses [P,7] float64 view, summaries: ctypes array
        view of P Summary records).  Fill `poses` with the start poses and call solve_batched_inplace(): no staging copies."""
        P = self.num_problems
        pp, ps = C.POINTER(C.c_double)(), C.POINTER(Summary)()
        check(self._L.clc_batched_host_buffers(self._h, C.byref(pp), C.byref(ps)), "clc_batched_host_buffers")
        poses = np.ctypeslib.as_array(pp, shape=(P, 7))
        sms = C.cast(ps, C.POINTER(Summary * P)).contents
        return poses, sms

    def solve_batched_inplace(self, options: Optional[Options] = None):
        """clc_solve_batched on the handle's own buffers (batched_buffers()): start poses in, results out, in place."""
        P = self.num_problems
        pp, ps = C.POINTER(C.c_double)(), C.POINTER(Summary)()
        check(self._L.clc_batched_host_buffers(self._h, C.byref(pp), C.byref(ps)), "clc_batched_host_buffers")
        o = options or default_options()
        check(self._L.clc_solve_batched(self._h, C.byref(o), pp, ps), "clc_solve_batched")
        return np.ctypeslib.as_array(pp, shape=(P, 7)), C.cast(ps, C.POINTER(Summary * P)).contents

    def solve_batched(self, poses0: np.ndarray, options: Optional[Options] = None):
        """-> (poses[P,7], summaries[P])"""
        P = self.num_problems
        poses = np.ascontiguousarray(np.array(poses0, dtype=np.float64).reshape(P, 7)).copy()
        sm = (Summary * P)()
        o = options or default_options()
        check(self._L.clc_solve_batched(self._h, C.byref(o), dptr(poses), sm), "clc_solve_batched")
        return poses, sm

    def closed_form_batched(self, poses_out: Optional[np.ndarray] = None):
        """clc_closed_form_batched: CamLaserCalClosedSolution of every uploaded problem (its records taken as points_on_line records)
        -> (Tlc [P,4,4], unobservable [P] bool, sv9 [P,9], status [P] int32, poses [P,7]).  poses: the start pose Tcl = Tlc^-1 of
        every problem with status CLC_OK, written into poses_out when given (e.g. the pose view of batched_buffers(), ready for
        solve_batched_inplace); other rows are left as they were (NaN in a new array)."""
        P = self.num_problems
        T = np.full((P, 16), np.nan); sv9 = np.full((P, 9), np.nan)
        un = np.zeros(P, dtype=np.int32); st = np.zeros(P, dtype=np.int32)
        if poses_out is None:
            poses = np.full((P, 7), np.nan)
        else:
            poses = poses_out
            assert poses.shape == (P, 7) and poses.dtype == np.float64 and poses.flags["C_CONTIGUOUS"], "poses_out: C-contiguous [P,7] float64"
        i32 = C.POINTER(C.c_int32)
        check(self._L.clc_closed_form_batched(self._h, poses.ctypes.data_as(C.POINTER(C.c_double)), dptr(T), un.ctypes.data_as(i32),
                                              dptr(sv9), st.ctypes.data_as(i32)), "clc_closed_form_batched")
        return T.reshape(P, 4, 4), un.astype(bool), sv9, st, poses

    def information_batched(self, poses: np.ndarray):
        """clc_information_batched: the analysis pass of every uploaded problem at poses [P,7] (may be the pose view of
        batched_buffers()) -> (H [P,6,6], b [P,6], chi2 [P], sv [P,6], V [P,6,6], n_null [P])."""
        P = self.num_problems
        if not (isinstance(poses, np.ndarray) and poses.dtype == np.float64 and poses.flags["C_CONTIGUOUS"]):
            poses = np.ascontiguousarray(poses, dtype=np.float64)
        assert poses.size == 7 * P, "poses: [P,7]"
        H = np.empty((P, 36)); b = np.empty((P, 6)); chi = np.empty(P); sv = np.empty((P, 6)); V = np.empty((P, 36))
        nn = np.empty(P, dtype=np.int32)
        check(self._L.clc_information_batched(self._h, poses.ctypes.data_as(C.POINTER(C.c_double)), dptr(H), dptr(b), dptr(chi), dptr(sv),
                                              dptr(V), nn.ctypes.data_as(C.POINTER(C.c_int32))), "clc_information_batched")
        return H.reshape(P, 6, 6), b, chi, sv, V.reshape(P, 6, 6), nn

    def solve_multistart(self, poses0: np.ndarray, options: Optional[Options] = None):
        """clc_solve_multistart: S independent LM solves from S start poses [S, 7] on the ONE problem uploaded as a batch of one
        (upload_batched(records, [0, n])) — one copy of the observations on the device -> (poses [S, 7], summaries [S])."""
        poses = np.ascontiguousarray(np.array(poses0, dtype=np.float64).reshape(-1, 7)).copy()
        S = poses.shape[0]
        sm = (Summary * S)()
        o = options or default_options()
        check(self._L.clc_solve_multistart(self._h, C.byref(o), C.c_size_t(S), dptr(poses), sm), "clc_solve_multistart")
        return poses, sm

    def solve_subsets(self, block_offsets: np.ndarray, weights: np.ndarray, poses0: np.ndarray, options: Optional[Options] = None):
        """clc_solve_subsets: S resampled solves on the ONE problem uploaded as a batch of one (upload_batched(records, [0, n])).
        block_offsets [B + 1] cuts the records into consecutive blocks (one per pose), weights [S, B] uint8 says how many times subset k
        takes block b (0: left out; resample.jackknife_weights / bootstrap_weights / random_subset_weights) — [S, B] or one row [B], whole
        numbers 0..255 (resample.as_weight_rows: ValueError otherwise, also for a flat [S * B] vector, which used to be accepted) —, poses0 [S, 7] or [7] (every
        subset from the same start) -> (poses [S, 7], summaries [S]).  An empty or non-finite subset: termination FAILURE, pose kept."""
        off = np.ascontiguousarray(block_offsets, dtype=np.int64).reshape(-1)
        B = off.size - 1
        assert B >= 1, "block_offsets: [B + 1]"
        w = resample.as_weight_rows(weights, B)   # (ValueError for 256, -1, 0.5: a plain cast to uint8 would wrap or truncate them)
        S = w.shape[0]
        p0 = np.asarray(poses0, dtype=np.float64)
        poses = np.ascontiguousarray(np.broadcast_to(p0.reshape(-1, 7), (S, 7))).copy()
        sm = (Summary * S)()
        o = options or default_options()
        check(self._L.clc_solve_subsets(self._h, C.byref(o), B, off.ctypes.data_as(C.POINTER(C.c_int64)), S,
                                        w.ctypes.data_as(C.POINTER(C.c_uint8)), dptr(poses), sm), "clc_solve_subsets")
        return poses, sm

    def score_blocks(self, block_offsets: np.ndarray, poses: np.ndarray, tau: float, options: Optional[Options] = None):
        """clc_score_blocks: S candidate poses [S, 7] judged against every block (block_offsets [B + 1], one block per recorded pose) of
        the ONE problem uploaded as a batch of one -> (ssq [S, B] sum of squared residuals without the loss, cost [S, B] robust cost under
        `options`, inliers [S, B] int32: records within tau of their plane).  One launch, a workgroup per pose, on the upload that
        solve_multistart / solve_subsets use; a non-finite pose: NaN / NaN / 0 in its row."""
        off = np.ascontiguousarray(block_offsets, dtype=np.int64).reshape(-1)
        B = off.size - 1
        x = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 7))
        S = x.shape[0]
        assert B >= 1 and S >= 1, "block_offsets: [B + 1], poses: [S, 7]"
        ssq = np.empty((S, B))
        cost = np.empty((S, B))
        inl = np.empty((S, B), dtype=np.int32)
        o = options or default_options()
        check(self._L.clc_score_blocks(self._h, C.byref(o), B, off.ctypes.data_as(C.POINTER(C.c_int64)), S, dptr(x), C.c_double(tau),
                                       dptr(ssq), dptr(cost), inl.ctypes.data_as(C.POINTER(C.c_int32))), "clc_score_blocks")
        return ssq, cost, inl

    # ---- scan line fitting ----
    def line_fit_batched(self, xy: np.ndarray, offsets: np.ndarray, lines0: np.ndarray,
                         options: Optional[Options] = None, want_summaries: bool = True):
        """LineFittingCeres for many scans: xy [M,2], CSR offsets [S+1], lines0 [S,2] -> (lines [S,2], summaries)."""
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        S = len(offsets) - 1
        lines = np.ascontiguousarray(np.array(lines0, dtype=np.float64).reshape(S, 2)).copy()
        sm = (Summary * S)() if want_summaries and S > 0 else None
        o = options or default_line_options()
        check(self._L.clc_line_fit_batched(self._h, C.byref(o), dptr(xy), iptr(offsets), C.c_size_t(S), dptr(lines), sm),
              "clc_line_fit_batched")
        return lines, sm

    def line_fit_batched_device(self, xy_ptr: int, offsets_ptr: int, n_scans: int, lines_ptr: int, summaries_ptr: int = 0,
                                options: Optional[Options] = None):
        """LineFittingCeres on device-resident arrays (data_ptr()s; ready on the solver's stream)."""
        o = options or default_line_options()
        check(self._L.clc_line_fit_batched_device(self._h, C.byref(o), C.c_void_p(xy_ptr), C.c_void_p(offsets_ptr), C.c_size_t(n_scans),
                                                  C.c_void_p(lines_ptr), C.c_void_p(summaries_ptr or 0)), "clc_line_fit_batched_device")

    def scan_to_points_device(self, ranges_ptr: int, offsets_ptr: int, n_scans: int, n_rays: int, angle_min_ptr: int,
                              angle_increment_ptr: int, range_min_ptr: int, points_ptr: int):
        """TranScanToPoints on device-resident arrays (data_ptr()s; ready on the solver's stream)."""
        check(self._L.clc_scan_to_points_device(self._h, C.c_void_p(ranges_ptr), C.c_void_p(offsets_ptr), C.c_size_t(n_scans),
                                                C.c_size_t(n_rays), C.c_void_p(angle_min_ptr), C.c_void_p(angle_increment_ptr),
                                                C.c_void_p(range_min_ptr), C.c_void_p(points_ptr)), "clc_scan_to_points_device")

    def scan_to_points(self, ranges: np.ndarray, offsets: np.ndarray, angle_min, angle_increment, range_min) -> np.ndarray:
        """TranScanToPoints (src/utilities.cpp:181-215) for many scans: ranges float32 [M], CSR offsets [S+1],
        per-scan angle_min / angle_increment / range_min -> points [M,3]."""
        r = np.ascontiguousarray(ranges, dtype=np.float32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        S = len(offsets) - 1
        f = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (S,)))
        am, ai, rm = f(angle_min), f(angle_increment), f(range_min)
        pts = np.empty((r.shape[0], 3))
        fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        check(self._L.clc_scan_to_points(self._h, fp(r), iptr(offsets), C.c_size_t(S), fp(am), fp(ai), fp(rm), dptr(pts)),
              "clc_scan_to_points")
        return pts

    # ---- camera models and board poses (K10) ----
    def camera_lift(self, camera, px: np.ndarray) -> np.ndarray:
        """liftProjective of pixels px [n, 2] (float32) -> x/z, y/z [n, 2] (unrounded)."""
        p = np.ascontiguousarray(px, dtype=np.float32).reshape(-1, 2)
        out = np.empty((p.shape[0], 2))
        c = camera.to_c()
        check(self._L.clc_camera_lift(self._h, C.byref(c), p.ctypes.data_as(C.c_void_p), C.c_size_t(p.shape[0]), dptr(out)), "clc_camera_lift")
        return out

    def camera_project(self, camera, pts: np.ndarray, pose7: Optional[np.ndarray] = None) -> np.ndarray:
        """spaceToPlane of pts [n, 3] after p_c = R p + t of pose7 = T_cl [t, qx, qy, qz, qw] (None: identity) -> pixels [n, 2]."""
        P = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        out = np.empty((P.shape[0], 2))
        c = camera.to_c()
        pp = None if pose7 is None else dptr(np.ascontiguousarray(pose7, dtype=np.float64).reshape(7))
        check(self._L.clc_camera_project(self._h, C.byref(c), pp, dptr(P), C.c_size_t(P.shape[0]), dptr(out)), "clc_camera_project")
        return out

    def board_poses(self, camera, corners_px: np.ndarray, board_xy: np.ndarray, offsets: np.ndarray,
                    options: Optional[Options] = None, want_summaries: bool = False):
        """One board pose per image (CamPoseEst::calcCamPose): corners_px [M, 2] float32 pixels, board_xy [M, 2] float32 board-plane
        points, CSR offsets [n+1] -> (q_ca_wxyz [n, 4], t_ca [n, 3], rms [n], status [n] int32, summaries or None)."""
        cp = np.ascontiguousarray(corners_px, dtype=np.float32).reshape(-1, 2)
        bx = np.ascontiguousarray(board_xy, dtype=np.float32).reshape(-1, 2)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        q = np.empty((n, 4)); t = np.empty((n, 3)); rms = np.empty(n); st = np.empty(n, dtype=np.int32)
        sm = (Summary * n)() if want_summaries and n > 0 else None
        c = camera.to_c()
        o = C.byref(options) if options is not None else None
        check(self._L.clc_board_poses(self._h, C.byref(c), o, cp.ctypes.data_as(C.c_void_p), bx.ctypes.data_as(C.c_void_p), iptr(offsets),
                                      C.c_size_t(n), dptr(q), dptr(t), dptr(rms), st.ctypes.data_as(C.c_void_p), sm), "clc_board_poses")
        return q, t, rms, st, sm

    def board_poses_device(self, camera, corners_ptr: int, board_ptr: int, offsets_ptr: int, n_images: int, q_ptr: int, t_ptr: int,
                           rms_ptr: int = 0, status_ptr: int = 0, summaries_ptr: int = 0, options: Optional[Options] = None):
        """clc_board_poses_device on device-resident arrays (data_ptr()s; ready on the solver's stream)."""
        c = camera.to_c()
        o = C.byref(options) if options is not None else None
        check(self._L.clc_board_poses_device(self._h, C.byref(c), o, C.c_void_p(corners_ptr), C.c_void_p(board_ptr), C.c_void_p(offsets_ptr),
                                             C.c_size_t(n_images), C.c_void_p(q_ptr), C.c_void_p(t_ptr), C.c_void_p(rms_ptr or 0),
                                             C.c_void_p(status_ptr), C.c_void_p(summaries_ptr or 0)), "clc_board_poses_device")

    def board_poses_robust(self, camera, corners_px: np.ndarray, board_xy: np.ndarray, offsets: np.ndarray,
                           options: Optional[Options] = None, robust: Optional[RobustPoseOptions] = None, want_summaries: bool = False):
        """clc_board_poses_robust (K16): per image a consensus over its tags (groups of four corners), the K10 fit on the consensus set,
        re-gate and refit until the set stops changing.  Arrays as board_poses -> (q_ca_wxyz [n, 4], t_ca [n, 3], rms [n], status [n]
        (CLC_POSE_*, -3 = no consensus), summaries or None, inlier [M] bool, n_inliers [n], best_group [n], n_fits [n])."""
        cp = np.ascontiguousarray(corners_px, dtype=np.float32).reshape(-1, 2)
        bx = np.ascontiguousarray(board_xy, dtype=np.float32).reshape(-1, 2)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        q = np.empty((n, 4)); t = np.empty((n, 3)); rms = np.empty(n); st = np.empty(n, dtype=np.int32)
        inl = np.zeros(cp.shape[0], dtype=np.uint8)
        ni = np.empty(n, dtype=np.int32); bg = np.empty(n, dtype=np.int32); nf = np.empty(n, dtype=np.int32)
        sm = (Summary * n)() if want_summaries and n > 0 else None
        c = camera.to_c()
        o = C.byref(options) if options is not None else None
        ro = C.byref(robust) if robust is not None else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self._L.clc_board_poses_robust(self._h, C.byref(c), o, ro, vp(cp), vp(bx), vp(offsets), C.c_size_t(n), vp(q), vp(t), vp(rms),
                                             vp(st), sm, vp(inl), vp(ni), vp(bg), vp(nf)), "clc_board_poses_robust")
        return q, t, rms, st, sm, inl.astype(bool), ni, bg, nf

    def board_poses_robust_device(self, camera, corners_ptr: int, board_ptr: int, offsets_ptr: int, n_images: int, q_ptr: int, t_ptr: int,
                                  rms_ptr: int = 0, status_ptr: int = 0, summaries_ptr: int = 0, inlier_ptr: int = 0,
                                  n_inliers_ptr: int = 0, best_group_ptr: int = 0, n_fits_ptr: int = 0,
                                  options: Optional[Options] = None, robust: Optional[RobustPoseOptions] = None):
        """clc_board_poses_robust_device on device-resident arrays (data_ptr()s; ready on the solver's stream); inlier: uint8,
        indexed like the corners."""
        c = camera.to_c()
        o = C.byref(options) if options is not None else None
        ro = C.byref(robust) if robust is not None else None
        V = C.c_void_p
        check(self._L.clc_board_poses_robust_device(self._h, C.byref(c), o, ro, V(corners_ptr), V(board_ptr), V(offsets_ptr),
                                                    C.c_size_t(n_images), V(q_ptr), V(t_ptr), V(rms_ptr or 0), V(status_ptr),
                                                    V(summaries_ptr or 0), V(inlier_ptr), V(n_inliers_ptr or 0), V(best_group_ptr or 0),
                                                    V(n_fits_ptr or 0)), "clc_board_poses_robust_device")

    def board_poses_alternate(self, camera, corners_px: np.ndarray, board_xy: np.ndarray, offsets: np.ndarray, q_in_wxyz: np.ndarray,
                              t_in: np.ndarray, status_in: np.ndarray, inlier: Optional[np.ndarray] = None,
                              options: Optional[Options] = None, alt: Optional[AltPoseOptions] = None, want_summaries: bool = False):
        """clc_board_poses_alternate (K17): per image the other minimum of the planar fit, from the mirror of the input pose about the
        line of sight, and how ambiguous the choice is.  Arrays as board_poses; (q_in_wxyz [n, 4], t_in [n, 3], status_in [n]) from
        board_poses / board_poses_robust, inlier [M] (bool / uint8, None: every corner) the robust call's mask -> dict: q [n, 4], t
        [n, 3], rms, cost_in, cost_alt, ratio, rot_angle, normal_angle [n], kind [n] int32 (CLC_ALT_*: 0 none, 1 same, 2 distinct),
        ambiguous, better [n] bool, summaries (or None)."""
        cp = np.ascontiguousarray(corners_px, dtype=np.float32).reshape(-1, 2)
        bx = np.ascontiguousarray(board_xy, dtype=np.float32).reshape(-1, 2)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        qi = np.ascontiguousarray(q_in_wxyz, dtype=np.float64).reshape(n, 4)
        ti = np.ascontiguousarray(t_in, dtype=np.float64).reshape(n, 3)
        si = np.ascontiguousarray(status_in, dtype=np.int32).reshape(n)
        m = None if inlier is None else np.ascontiguousarray(np.asarray(inlier).astype(np.uint8)).reshape(cp.shape[0])
        real = {k: np.empty(n) for k in ("rms", "cost_in", "cost_alt", "ratio", "rot_angle", "normal_angle")}
        q = np.empty((n, 4)); t = np.empty((n, 3)); kind = np.empty(n, dtype=np.int32)
        amb = np.zeros(n, dtype=np.uint8); bet = np.zeros(n, dtype=np.uint8)
        sm = (Summary * n)() if want_summaries and n > 0 else None
        c = camera.to_c()
        o = C.byref(options) if options is not None else None
        ao = C.byref(alt) if alt is not None else None
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(self._L.clc_board_poses_alternate(self._h, C.byref(c), o, ao, vp(cp), vp(bx), vp(offsets), C.c_size_t(n), vp(m), vp(qi), vp(ti),
                                                vp(si), vp(q), vp(t), vp(real["rms"]), vp(real["cost_in"]), vp(real["cost_alt"]),
                                                vp(real["ratio"]), vp(real["rot_angle"]), vp(real["normal_angle"]), vp(kind), vp(amb),
                                                vp(bet), sm), "clc_board_poses_alternate")
        return dict(real, q=q, t=t, kind=kind, ambiguous=amb.astype(bool), better=bet.astype(bool), summaries=sm)

    def board_poses_alternate_device(self, camera, corners_ptr: int, board_ptr: int, offsets_ptr: int, n_images: int, q_in_ptr: int,
                                     t_in_ptr: int, status_in_ptr: int, kind_ptr: int, inlier_ptr: int = 0, q_ptr: int = 0, t_ptr: int = 0,
                                     rms_ptr: int = 0, cost_in_ptr: int = 0, cost_alt_ptr: int = 0, ratio_ptr: int = 0,
                                     rot_angle_ptr: int = 0, normal_angle_ptr: int = 0, ambiguous_ptr: int = 0, better_ptr: int = 0,
                                     summaries_ptr: int = 0, options: Optional[Options] = None, alt: Optional[AltPoseOptions] = None):
        """clc_board_poses_alternate_device on device-resident arrays (data_ptr()s; ready on the solver's stream); inlier, ambiguous,
        better: uint8; kind is required, a zero pointer leaves any other output out."""
        c = camera.to_c()
        o = C.byref(options) if options is not None else None
        ao = C.byref(alt) if alt is not None else None
        V = lambda p: C.c_void_p(p or 0)
        check(self._L.clc_board_poses_alternate_device(self._h, C.byref(c), o, ao, V(corners_ptr), V(board_ptr), V(offsets_ptr),
                                                       C.c_size_t(n_images), V(inlier_ptr), V(q_in_ptr), V(t_in_ptr), V(status_in_ptr),
                                                       V(q_ptr), V(t_ptr), V(rms_ptr), V(cost_in_ptr), V(cost_alt_ptr), V(ratio_ptr),
                                                       V(rot_angle_ptr), V(normal_angle_ptr), V(kind_ptr), V(ambiguous_ptr),
                                                       V(better_ptr), V(summaries_ptr)), "clc_board_poses_alternate_device")

    # ---- joint refinement (K18) ----
    def joint_refine(self, camera, corners_px: np.ndarray, board_xy: np.ndarray, corner_offsets: np.ndarray, pts: np.ndarray,
                     pts_offsets: np.ndarray, q_ca_wxyz: np.ndarray, t_ca: np.ndarray, poses_cl: np.ndarray,
                     problem_offsets: Optional[np.ndarray] = None, keep: Optional[np.ndarray] = None, options: Optional[Options] = None,
                     joint: Optional[JointOptions] = None) -> dict:
        """clc_joint_refine (K18): one cost over T_cl and every board pose of a problem — corner reprojection over sigma_corner plus laser
        point-to-board-plane distance over sigma_laser.  Image i owns corners [corner_offsets[i], corner_offsets[i+1]) and laser points
        [pts_offsets[i], pts_offsets[i+1]); problem k owns images [problem_offsets[k], problem_offsets[k+1]) (None: one problem).
        q_ca_wxyz [n, 4], t_ca [n, 3], poses_cl [n_problems, 7] are the start poses (not modified).
        -> dict(q [n, 4], t [n, 3], poses_cl [n_problems, 7], summaries, H_cl [n_problems, 6, 6], cost_parts [n_problems, 2] (corner,
        laser), status [n] int32 (CLC_JOINT_*))."""
        cp = np.ascontiguousarray(corners_px, dtype=np.float32).reshape(-1, 2)
        bx = np.ascontiguousarray(board_xy, dtype=np.float32).reshape(-1, 2)
        co = np.ascontiguousarray(corner_offsets, dtype=np.int64)
        P = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        po = np.ascontiguousarray(pts_offsets, dtype=np.int64)
        n = len(co) - 1
        if n < 0 or len(po) != n + 1:
            raise ValueError("joint_refine: corner_offsets and pts_offsets need one entry per image plus one")
        if n > 0 and (co[-1] > len(cp) or co[-1] > len(bx) or po[-1] > len(P) or co[0] < 0 or po[0] < 0):
            raise ValueError("joint_refine: offsets run past corners_px, board_xy or pts")
        pr = None if problem_offsets is None else np.ascontiguousarray(problem_offsets, dtype=np.int64)
        npb = 1 if pr is None else len(pr) - 1
        q = np.array(q_ca_wxyz, dtype=np.float64, order="C").reshape(n, 4)
        t = np.array(t_ca, dtype=np.float64, order="C").reshape(n, 3)
        cl = np.array(poses_cl, dtype=np.float64, order="C").reshape(npb, 7)
        kp = None if keep is None else np.ascontiguousarray(np.asarray(keep).astype(np.uint8))
        if kp is not None and kp.shape != (n,):
            raise ValueError("joint_refine: keep needs one entry per image")
        if pr is not None and (len(pr) < 1 or (len(pr) > 1 and pr[-1] > n)):
            raise ValueError("joint_refine: problem_offsets run past the images")
        sm = (Summary * max(npb, 1))()
        H = np.empty((npb, 6, 6)); parts = np.empty((npb, 2)); st = np.empty(n, dtype=np.int32)
        c = camera.to_c()
        V = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(self._L.clc_joint_refine(self._h, C.byref(c), C.byref(options) if options is not None else None,
                                       C.byref(joint) if joint is not None else None, V(cp), V(bx), V(co), V(P), V(po), V(kp), C.c_size_t(n),
                                       V(pr), C.c_size_t(npb), V(q), V(t), V(cl), sm, V(H), V(parts), V(st)), "clc_joint_refine")
        return dict(q=q, t=t, poses_cl=cl, summaries=sm, H_cl=H, cost_parts=parts, status=st)

    def joint_refine_device(self, camera, corners_ptr: int, board_ptr: int, corner_offsets_ptr: int, pts_ptr: int, pts_offsets_ptr: int,
                            n_images: int, n_problems: int, q_ptr: int, t_ptr: int, poses_cl_ptr: int, summaries_ptr: int, status_ptr: int,
                            problem_offsets_ptr: int = 0, keep_ptr: int = 0, H_cl_ptr: int = 0, cost_parts_ptr: int = 0,
                            options: Optional[Options] = None, joint: Optional[JointOptions] = None):
        """clc_joint_refine_device on device-resident arrays (data_ptr()s; ready on the solver's stream): the per-image arrays are
        indexed by the absolute image index, the call covers n_images images from problem_offsets[0] on; q, t, poses_cl in / out."""
        c = camera.to_c()
        V = lambda p: C.c_void_p(p or 0)
        check(self._L.clc_joint_refine_device(self._h, C.byref(c), C.byref(options) if options is not None else None,
                                              C.byref(joint) if joint is not None else None, V(corners_ptr), V(board_ptr),
                                              V(corner_offsets_ptr), V(pts_ptr), V(pts_offsets_ptr), V(keep_ptr), C.c_size_t(n_images),
                                              V(problem_offsets_ptr), C.c_size_t(n_problems), V(q_ptr), V(t_ptr), V(poses_cl_ptr),
                                              V(summaries_ptr), V(H_cl_ptr), V(cost_parts_ptr), V(status_ptr)), "clc_joint_refine_device")

    # ---- robust joint refinement: a Cauchy loss per corner and per laser point (K22) ----
    def joint_refine_robust(self, camera, corners_px: np.ndarray, board_xy: np.ndarray, corner_offsets: np.ndarray, pts: np.ndarray,
                            pts_offsets: np.ndarray, q_ca_wxyz: np.ndarray, t_ca: np.ndarray, poses_cl: np.ndarray,
                            problem_offsets: Optional[np.ndarray] = None, keep: Optional[np.ndarray] = None,
                            options: Optional[Options] = None, joint: Optional[JointOptions] = None,
                            loss: Optional[JointLossOptions] = None) -> dict:
        """clc_joint_refine_robust (K22): joint_refine's arguments and cost with a Cauchy loss on every corner (scale loss.loss_corner,
        in units of sigma_corner) and on every laser point (loss.loss_laser, in units of sigma_laser); loss None: the defaults, a
        scale 0: no loss on that term.
        -> joint_refine's dict (final_cost and cost_parts are the robust cost and its shares) and w_corner [len(corners_px)],
        w_laser [len(pts)]: rho' of every observation at the returned poses (1 where the term has no loss, NaN for an image that
        takes no part or a problem that ended CLC_FAILURE; w >= 0.5: |residual| <= scale * sigma)."""
        cp = np.ascontiguousarray(corners_px, dtype=np.float32).reshape(-1, 2)
        bx = np.ascontiguousarray(board_xy, dtype=np.float32).reshape(-1, 2)
        co = np.ascontiguousarray(corner_offsets, dtype=np.int64)
        P = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        po = np.ascontiguousarray(pts_offsets, dtype=np.int64)
        n = len(co) - 1
        if n < 0 or len(po) != n + 1:
            raise ValueError("joint_refine_robust: corner_offsets and pts_offsets need one entry per image plus one")
        if n > 0 and (co[-1] > len(cp) or co[-1] > len(bx) or po[-1] > len(P) or co[0] < 0 or po[0] < 0):
            raise ValueError("joint_refine_robust: offsets run past corners_px, board_xy or pts")
        pr = None if problem_offsets is None else np.ascontiguousarray(problem_offsets, dtype=np.int64)
        npb = 1 if pr is None else len(pr) - 1
        q = np.array(q_ca_wxyz, dtype=np.float64, order="C").reshape(n, 4)
        t = np.array(t_ca, dtype=np.float64, order="C").reshape(n, 3)
        cl = np.array(poses_cl, dtype=np.float64, order="C").reshape(npb, 7)
        kp = None if keep is None else np.ascontiguousarray(np.asarray(keep).astype(np.uint8))
        if kp is not None and kp.shape != (n,):
            raise ValueError("joint_refine_robust: keep needs one entry per image")
        if pr is not None and (len(pr) < 1 or (len(pr) > 1 and pr[-1] > n)):
            raise ValueError("joint_refine_robust: problem_offsets run past the images")
        sm = (Summary * max(npb, 1))()
        H = np.empty((npb, 6, 6)); parts = np.empty((npb, 2)); st = np.empty(n, dtype=np.int32)
        wc, wl = np.full(len(cp), np.nan), np.full(len(P), np.nan)
        c = camera.to_c()
        V = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(self._L.clc_joint_refine_robust(self._h, C.byref(c), C.byref(options) if options is not None else None,
                                              C.byref(joint) if joint is not None else None, C.byref(loss) if loss is not None else None,
                                              V(cp), V(bx), V(co), V(P), V(po), V(kp), C.c_size_t(n), V(pr), C.c_size_t(npb), V(q), V(t), V(cl),
                                              sm, V(H), V(parts), V(st), V(wc), V(wl)), "clc_joint_refine_robust")
        return dict(q=q, t=t, poses_cl=cl, summaries=sm, H_cl=H, cost_parts=parts, status=st, w_corner=wc, w_laser=wl)

    def joint_refine_robust_device(self, camera, corners_ptr: int, board_ptr: int, corner_offsets_ptr: int, pts_ptr: int,
                                   pts_offsets_ptr: int, n_images: int, n_problems: int, q_ptr: int, t_ptr: int, poses_cl_ptr: int,
                                   summaries_ptr: int, status_ptr: int, problem_offsets_ptr: int = 0, keep_ptr: int = 0, H_cl_ptr: int = 0,
                                   cost_parts_ptr: int = 0, w_corner_ptr: int = 0, w_laser_ptr: int = 0, options: Optional[Options] = None,
                                   joint: Optional[JointOptions] = None, loss: Optional[JointLossOptions] = None):
        """clc_joint_refine_robust_device on device-resident arrays (data_ptr()s; ready on the solver's stream): joint_refine_device's
        conventions; w_corner, w_laser (float64) are indexed by the absolute corner / point offsets."""
        c = camera.to_c()
        V = lambda p: C.c_void_p(p or 0)
        check(self._L.clc_joint_refine_robust_device(self._h, C.byref(c), C.byref(options) if options is not None else None,
                                                     C.byref(joint) if joint is not None else None,
                                                     C.byref(loss) if loss is not None else None, V(corners_ptr), V(board_ptr),
                                                     V(corner_offsets_ptr), V(pts_ptr), V(pts_offsets_ptr), V(keep_ptr), C.c_size_t(n_images),
                                                     V(problem_offsets_ptr), C.c_size_t(n_problems), V(q_ptr), V(t_ptr), V(poses_cl_ptr),
                                                     V(summaries_ptr), V(H_cl_ptr), V(cost_parts_ptr), V(status_ptr), V(w_corner_ptr),
                                                     V(w_laser_ptr)), "clc_joint_refine_robust_device")

    # ---- joint refinement with the scanner's range offset and scale (K21) ----
    def joint_refine_range(self, camera, corners_px, board_xy, corner_offsets, pts: np.ndarray, pts_offsets: np.ndarray,
                           q_ca_wxyz: np.ndarray, t_ca: np.ndarray, poses_cl: np.ndarray, range0: Optional[np.ndarray] = None,
                           problem_offsets: Optional[np.ndarray] = None, keep: Optional[np.ndarray] = None,
                           options: Optional[Options] = None, range_options: Optional[RangeOptions] = None) -> dict:
        """clc_joint_refine_range (K21): joint_refine's cost with the laser points corrected along their rays,
        p' = (1 + kappa + b / |p|) p, and b (range offset, metres) and kappa (range scale) in the shared block beside T_cl.
        range0 [n_problems, 2]: the start (None: zeros; a held parameter keeps its value and is still applied).  With
        range_options.hold_board_poses the camera and the three corner arrays may be None.
        -> dict(q, t, poses_cl, range [n_problems, 2], summaries, H_cr [n_problems, 8, 8] (the information on [T_cl tangent, b,
        kappa], board poses marginalised), cost_parts, status)."""
        P = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        po = np.ascontiguousarray(pts_offsets, dtype=np.int64)
        n = len(po) - 1
        cp = bx = co = None
        if corner_offsets is not None:
            cp = np.ascontiguousarray(corners_px, dtype=np.float32).reshape(-1, 2)
            bx = np.ascontiguousarray(board_xy, dtype=np.float32).reshape(-1, 2)
            co = np.ascontiguousarray(corner_offsets, dtype=np.int64)
            if len(co) != n + 1:
                raise ValueError("joint_refine_range: corner_offsets and pts_offsets need one entry per image plus one")
            if n > 0 and (co[-1] > len(cp) or co[-1] > len(bx) or co[0] < 0):
                raise ValueError("joint_refine_range: offsets run past corners_px or board_xy")
        if n < 0 or (n > 0 and (po[-1] > len(P) or po[0] < 0)):
            raise ValueError("joint_refine_range: offsets run past pts")
        pr = None if problem_offsets is None else np.ascontiguousarray(problem_offsets, dtype=np.int64)
        npb = 1 if pr is None else len(pr) - 1
        q = np.array(q_ca_wxyz, dtype=np.float64, order="C").reshape(n, 4)
        t = np.array(t_ca, dtype=np.float64, order="C").reshape(n, 3)
        cl = np.array(poses_cl, dtype=np.float64, order="C").reshape(npb, 7)
        rg = np.zeros((npb, 2)) if range0 is None else np.array(range0, dtype=np.float64, order="C").reshape(npb, 2)
        kp = None if keep is None else np.ascontiguousarray(np.asarray(keep).astype(np.uint8))
        if kp is not None and kp.shape != (n,):
            raise ValueError("joint_refine_range: keep needs one entry per image")
        if pr is not None and (len(pr) < 1 or (len(pr) > 1 and pr[-1] > n)):
            raise ValueError("joint_refine_range: problem_offsets run past the images")
        sm = (Summary * max(npb, 1))()
        H = np.empty((npb, 8, 8)); parts = np.empty((npb, 2)); st = np.empty(n, dtype=np.int32)
        c = camera.to_c() if camera is not None else None
        V = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(self._L.clc_joint_refine_range(self._h, C.byref(c) if c is not None else None, C.byref(options) if options is not None else None,
                                             C.byref(range_options) if range_options is not None else None, V(cp), V(bx), V(co), V(P), V(po),
                                             V(kp), C.c_size_t(n), V(pr), C.c_size_t(npb), V(q), V(t), V(cl), V(rg), sm, V(H), V(parts), V(st)),
              "clc_joint_refine_range")
        return dict(q=q, t=t, poses_cl=cl, range=rg, summaries=sm, H_cr=H, cost_parts=parts, status=st)

    def joint_refine_range_device(self, camera, corners_ptr: int, board_ptr: int, corner_offsets_ptr: int, pts_ptr: int, pts_offsets_ptr: int,
                                  n_images: int, n_problems: int, q_ptr: int, t_ptr: int, poses_cl_ptr: int, range_ptr: int,
                                  summaries_ptr: int, status_ptr: int, problem_offsets_ptr: int = 0, keep_ptr: int = 0, H_cr_ptr: int = 0,
                                  cost_parts_ptr: int = 0, options: Optional[Options] = None, range_options: Optional[RangeOptions] = None):
        """clc_joint_refine_range_device on device-resident arrays (data_ptr()s; ready on the solver's stream): the conventions of
        joint_refine_device; q, t, poses_cl and range in / out."""
        c = camera.to_c() if camera is not None else None
        V = lambda p: C.c_void_p(p or 0)
        check(self._L.clc_joint_refine_range_device(self._h, C.byref(c) if c is not None else None,
                                                    C.byref(options) if options is not None else None,
                                                    C.byref(range_options) if range_options is not None else None, V(corners_ptr),
                                                    V(board_ptr), V(corner_offsets_ptr), V(pts_ptr), V(pts_offsets_ptr), V(keep_ptr),
                                                    C.c_size_t(n_images), V(problem_offsets_ptr), C.c_size_t(n_problems), V(q_ptr), V(t_ptr),
                                                    V(poses_cl_ptr), V(range_ptr), V(summaries_ptr), V(H_cr_ptr), V(cost_parts_ptr),
                                                    V(status_ptr)), "clc_joint_refine_range_device")

    def range_correct(self, pts: np.ndarray, offset: float, scale: float) -> np.ndarray:
        """clc_range_correct: p' = (1 + scale + offset / |p|) p of pts [N, 3]; NaN for a point that is non-finite or at the origin."""
        P = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        out = np.empty_like(P)
        rg = np.array([offset, scale], dtype=np.float64)
        V = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self._L.clc_range_correct(self._h, V(rg), V(P), C.c_size_t(len(P)), V(out)), "clc_range_correct")
        return out

    def range_correct_device(self, pts_ptr: int, n: int, out_ptr: int, offset: float, scale: float):
        """clc_range_correct_device on device-resident arrays (data_ptr()s; out may be pts)."""
        rg = np.array([offset, scale], dtype=np.float64)
        check(self._L.clc_range_correct_device(self._h, rg.ctypes.data_as(C.c_void_p), C.c_void_p(pts_ptr or 0), C.c_size_t(n),
                                               C.c_void_p(out_ptr or 0)), "clc_range_correct_device")

    # ---- pose guidance (K20) ----
    @staticmethod
    def _guidance_args(pose_cl, H0, options):
        pose = np.ascontiguousarray(pose_cl, dtype=np.float64).reshape(7)
        H = None if H0 is None else np.ascontiguousarray(H0, dtype=np.float64).reshape(36)
        return pose, H, (C.byref(options) if options is not None else None)

    def score_board_poses(self, pose_cl: np.ndarray, q_ca_wxyz: np.ndarray, t_ca: np.ndarray, H0: Optional[np.ndarray] = None,
                          options: Optional[GuidanceOptions] = None) -> dict:
        """clc_score_board_poses (K20): for every candidate board pose (q_ca_wxyz [n, 4], t_ca [n, 3], the board in the camera frame)
        the scanner's rays are cast through T_cl = pose_cl onto the board; H_add is the information clc_information's H would gain if
        the pose were recorded, sv the eigenvalues of H0 + H_add (descending), score the criterion of `options` (None: the defaults).
        H0 [6, 6] or None (zeros).  -> dict(n_hits [n] int32 (-1: a non-finite candidate), H_add [n, 6, 6], sv [n, 6], score [n])."""
        q = np.ascontiguousarray(q_ca_wxyz, dtype=np.float64).reshape(-1, 4)
        t = np.ascontiguousarray(t_ca, dtype=np.float64).reshape(-1, 3)
        if q.shape[0] != t.shape[0]:
            raise ValueError("score_board_poses: q_ca_wxyz and t_ca need one row per candidate")
        n = q.shape[0]
        pose, H, o = self._guidance_args(pose_cl, H0, options)
        nh = np.empty(n, dtype=np.int32); Ha = np.empty((n, 6, 6)); sv = np.empty((n, 6)); sc = np.empty(n)
        V = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(self._L.clc_score_board_poses(self._h, o, V(pose), V(H), C.c_size_t(n), V(q), V(t), V(nh), V(Ha), V(sv), V(sc)),
              "clc_score_board_poses")
        return dict(n_hits=nh, H_add=Ha, sv=sv, score=sc)

    def score_board_poses_device(self, pose_cl: np.ndarray, n_cand: int, q_ptr: int, t_ptr: int, n_hits_ptr: int = 0, H_add_ptr: int = 0,
                                 sv_ptr: int = 0, score_ptr: int = 0, H0: Optional[np.ndarray] = None,
                                 options: Optional[GuidanceOptions] = None):
        """clc_score_board_poses_device: the candidates and the per-candidate outputs (each optional) are device arrays (data_ptr()s;
        ready on the solver's stream); pose_cl, H0 and the options on the host."""
        pose, H, o = self._guidance_args(pose_cl, H0, options)
        V = lambda p: C.c_void_p(p or 0)
        A = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(self._L.clc_score_board_poses_device(self._h, o, A(pose), A(H), C.c_size_t(n_cand), V(q_ptr), V(t_ptr), V(n_hits_ptr),
                                                   V(H_add_ptr), V(sv_ptr), V(score_ptr)), "clc_score_board_poses_device")

    def _select_board_poses(self, name: str, pose_cl, H0, options, n: int, q, t, k: int) -> dict:
        pose, H, o = self._guidance_args(pose_cl, H0, options)
        kk = max(int(k), 0)
        ch = np.full(kk, -1, dtype=np.int64); sva = np.full((kk, 6), np.nan); sca = np.full(kk, np.nan)
        Hf = np.zeros((6, 6)) if H is None else H.reshape(6, 6).copy()
        nc = C.c_int32(0)
        A = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(getattr(self._L, name)(self._h, o, A(pose), A(H), C.c_size_t(n), q, t, C.c_size_t(kk), A(ch) if kk else None, A(sva), A(sca),
                                     A(Hf), C.byref(nc)), name)
        return dict(chosen=ch, sv_after=sva, score_after=sca, H_after=Hf, n_chosen=nc.value)

    def select_board_poses(self, pose_cl: np.ndarray, q_ca_wxyz: np.ndarray, t_ca: np.ndarray, k: int, H0: Optional[np.ndarray] = None,
                           options: Optional[GuidanceOptions] = None) -> dict:
        """clc_select_board_poses (K20): a greedy choice of k candidates without replacement — every round picks the seen candidate not
        yet chosen with the largest score of M + H_add (ties: the lowest index), then M += H_add[chosen]; M starts at H0.
        -> dict(chosen [k] int64 in order, -1 padded; sv_after [k, 6] and score_after [k] of M after each round (NaN in the padding);
        H_after [6, 6]; n_chosen)."""
        q = np.ascontiguousarray(q_ca_wxyz, dtype=np.float64).reshape(-1, 4)
        t = np.ascontiguousarray(t_ca, dtype=np.float64).reshape(-1, 3)
        if q.shape[0] != t.shape[0]:
            raise ValueError("select_board_poses: q_ca_wxyz and t_ca need one row per candidate")
        return self._select_board_poses("clc_select_board_poses", pose_cl, H0, options, q.shape[0], q.ctypes.data_as(C.c_void_p),
                                        t.ctypes.data_as(C.c_void_p), k)

    def select_board_poses_device(self, pose_cl: np.ndarray, n_cand: int, q_ptr: int, t_ptr: int, k: int, H0: Optional[np.ndarray] = None,
                                  options: Optional[GuidanceOptions] = None) -> dict:
        """clc_select_board_poses_device: the candidates are device arrays (data_ptr()s; ready on the solver's stream); the results
        come back to the host as select_board_poses' do."""
        return self._select_board_poses("clc_select_board_poses_device", pose_cl, H0, options, n_cand, C.c_void_p(q_ptr or 0),
                                        C.c_void_p(t_ptr or 0), k)

    # ---- sub-pixel corner refinement (K24) ----
    def corner_subpix(self, images: np.ndarray, corners_px: np.ndarray, offsets: np.ndarray, options: Optional[SubpixOptions] = None,
                      width: Optional[int] = None) -> dict:
        """clc_corner_subpix (K24, cv::cornerSubPix restated): images uint8 [n, H, W], or [n, H, pitch] with width= given; corners_px
        [M, 2] float32 start pixels grouped per image by the CSR offsets [n + 1] (absolute rows of corners_px).
        -> dict(corners [M, 2] float32, status [M] int32 (CLC_SUBPIX_*), iterations [M] int32, strength [M]); rows outside
        [offsets[0], offsets[n]) come back as they went in, with status -99, iterations 0 and strength NaN."""
        img, img_args = _images_arg("corner_subpix", images, width)
        cp = np.ascontiguousarray(corners_px, dtype=np.float32).reshape(-1, 2)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(off) - 1
        if n != img.shape[0] or (n > 0 and (off[0] < 0 or off[-1] > len(cp))):
            raise ValueError("corner_subpix: offsets need one entry per image and one more, inside corners_px")
        out = cp.copy()
        st = np.full(len(cp), -99, dtype=np.int32); it = np.zeros(len(cp), dtype=np.int32); lam = np.full(len(cp), np.nan)
        V = lambda a: a.ctypes.data_as(C.c_void_p)
        o = C.byref(options) if options is not None else None
        check(self._L.clc_corner_subpix(self._h, o, *img_args, C.c_size_t(n), V(cp), V(off), V(out), V(st), V(it), V(lam)), "clc_corner_subpix")
        return dict(corners=out, status=st, iterations=it, strength=lam)

    def corner_subpix_device(self, images_ptr: int, width: int, height: int, pitch: int, n_images: int, corners_ptr: int, offsets_ptr: int,
                             out_ptr: int, status_ptr: int = 0, iterations_ptr: int = 0, strength_ptr: int = 0,
                             options: Optional[SubpixOptions] = None):
        """clc_corner_subpix_device on device-resident arrays (data_ptr()s; ready on the solver's stream); out_ptr may be corners_ptr."""
        V = lambda p: C.c_void_p(p or 0)
        o = C.byref(options) if options is not None else None
        check(self._L.clc_corner_subpix_device(self._h, o, V(images_ptr), C.c_int32(width), C.c_int32(height), C.c_int64(pitch),
                                               C.c_size_t(n_images), V(corners_ptr), V(offsets_ptr), V(out_ptr), V(status_ptr),
                                               V(iterations_ptr), V(strength_ptr)), "clc_corner_subpix_device")

    # ---- chessboard corners from images (K25) ----
    def chess_corners(self, images: np.ndarray, options: Optional[ChessOptions] = None, width: Optional[int] = None) -> dict:
        """clc_chess_corners (K25): images uint8 [n, H, W], or [n, H, pitch] with width= given -> dict(xy [n, stride, 2] float32 integer
        pixels ordered by (-R5, y, x), NaN in the unused slots; r5 [n, stride] int32; count [n]; count_raw [n]; status [n]: 1, or -2
        where the image has more than 4096 raw candidates), stride = options.max_per_image."""
        img, img_args = _images_arg("chess_corners", images, width)
        o = options if options is not None else _capi.default_chess_options()
        n, stride = img.shape[0], max(int(o.max_per_image), 1)
        xy = np.full((n, stride, 2), -7.0, np.float32); r5 = np.full((n, stride), -7, np.int32)
        cnt = np.full(n, -7, np.int32); raw = np.full(n, -7, np.int32); st = np.full(n, -99, np.int32)
        V = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self._L.clc_chess_corners(self._h, C.byref(o), *img_args, C.c_size_t(n), V(xy), V(r5), V(cnt), V(raw), V(st)), "clc_chess_corners")
        return dict(xy=xy, r5=r5, count=cnt, count_raw=raw, status=st)

    def chess_corners_device(self, images_ptr: int, width: int, height: int, pitch: int, n_images: int, xy_ptr: int, count_ptr: int,
                             status_ptr: int, r5_ptr: int = 0, count_raw_ptr: int = 0, options: Optional[ChessOptions] = None):
        """clc_chess_corners_device on device-resident arrays (data_ptr()s; ready on the solver's stream)."""
        V = lambda p: C.c_void_p(p or 0)
        o = C.byref(options) if options is not None else None
        check(self._L.clc_chess_corners_device(self._h, o, V(images_ptr), C.c_int32(width), C.c_int32(height), C.c_int64(pitch),
                                               C.c_size_t(n_images), V(xy_ptr), V(r5_ptr), V(count_ptr), V(count_raw_ptr), V(status_ptr)),
              "clc_chess_corners_device")

    def find_chessboard(self, images: np.ndarray, cols: int, rows: int, chess_options: Optional[ChessOptions] = None,
                        order_options: Optional[ChessOrderOptions] = None, subpix_options: Optional[SubpixOptions] = None,
                        width: Optional[int] = None, ordering: str = "host") -> dict:
        """clc_find_chessboard (K25): detection on the device, ordering into the cols x rows grid on the host, and with subpix_options
        the refinement (K24) -> dict(corners [n, cols rows, 2] float32, row i cols + j = node (j, i), NaN where no board was found;
        found [n] bool; strength [n, cols rows]).  ordering="device": clc_find_chessboard_gpu (K26), the ordering on the device too
        and nothing read back between the stages; the same results."""
        if ordering not in ("host", "device"):
            raise ValueError("find_chessboard: ordering must be 'host' or 'device'")
        img, img_args = _images_arg("find_chessboard", images, width)
        n, per = img.shape[0], max(int(cols) * int(rows), 1)
        corners = np.full((n, per, 2), np.nan, np.float32); found = np.zeros(n, np.int32); lam = np.full((n, per), np.nan)
        V = lambda a: a.ctypes.data_as(C.c_void_p)
        ref = lambda o: C.byref(o) if o is not None else None
        name = "clc_find_chessboard" if ordering == "host" else "clc_find_chessboard_gpu"
        check(getattr(self._L, name)(self._h, ref(chess_options), ref(order_options), ref(subpix_options), *img_args,
                                     C.c_size_t(n), C.c_int32(cols), C.c_int32(rows), V(corners), V(found), V(lam)), name)
        return dict(corners=corners, found=found.astype(bool), strength=lam)

    # ---- the ordering on the device (K26) ----
    def chessboard_order_device(self, cand_xy_ptr: int, count_ptr: int, stride: int, n_images: int, cols: int, rows: int, index_ptr: int,
                                status_ptr: int, n_labelings_ptr: int = 0, worst_ptr: int = 0, options: Optional[ChessOrderOptions] = None):
        """clc_chessboard_order_device on device-resident arrays (data_ptr()s; ready on the solver's stream): cand_xy [n, stride, 2]
        float32 and count [n] int32 as chess_corners_device wrote them, status [n] int32 read and written, index [n, cols rows] int32;
        n_labelings [n] int32 and worst [n] float64 may be left out."""
        V = lambda p: C.c_void_p(p or 0)
        o = C.byref(options) if options is not None else None
        check(self._L.clc_chessboard_order_device(self._h, V(cand_xy_ptr), V(count_ptr), C.c_int64(stride), C.c_size_t(n_images), C.c_int32(cols),
                                                  C.c_int32(rows), o, V(index_ptr), V(status_ptr), V(n_labelings_ptr), V(worst_ptr)),
              "clc_chessboard_order_device")

    def find_chessboard_device(self, images_ptr: int, width: int, height: int, pitch: int, n_images: int, cols: int, rows: int, corners_ptr: int,
                               found_ptr: int, strength_ptr: int = 0, chess_options: Optional[ChessOptions] = None,
                               order_options: Optional[ChessOrderOptions] = None, subpix_options: Optional[SubpixOptions] = None):
        """clc_find_chessboard_device on device-resident arrays (data_ptr()s; ready on the solver's stream): images uint8, corners
        [n, cols rows, 2] float32, found [n] int32, strength [n, cols rows] float64 (may be left out)."""
        V = lambda p: C.c_void_p(p or 0)
        ref = lambda o: C.byref(o) if o is not None else None
        check(self._L.clc_find_chessboard_device(self._h, ref(chess_options), ref(order_options), ref(subpix_options), V(images_ptr),
                                                 C.c_int32(width), C.c_int32(height), C.c_int64(pitch), C.c_size_t(n_images), C.c_int32(cols),
                                                 C.c_int32(rows), V(corners_ptr), V(found_ptr), V(strength_ptr)), "clc_find_chessboard_device")

    # ---- tag-grid corners from images (K27) ----
    def tag_grid(self, images: np.ndarray, family: "TagFamily", cols: int, rows: int, tag_options: Optional[TagOptions] = None,
                 chess_options: Optional[ChessOptions] = None, subpix_options: Optional[SubpixOptions] = None,
                 width: Optional[int] = None) -> dict:
        """clc_tag_grid (K27): images uint8 [n, H, W], or [n, H, pitch] with width= given; a cols x rows grid of tags of `family`, tag
        id = row cols + col -> dict(corners [n, cols rows, 4, 2] float32, NaN for a tag not seen, integer pixels or with subpix_options
        refined (K24); hamming [n, cols rows], -1 not seen; count [n]; status [n]: 1, or -2 where the detection overflowed; n_quads,
        n_foreign, n_edges_dropped [n]; strength [n, cols rows, 4])."""
        img, img_args = _images_arg("tag_grid", images, width)
        n, T = img.shape[0], max(int(cols) * int(rows), 1)
        r = dict(corners=np.full((n, T, 4, 2), -7.0, np.float32), hamming=np.full((n, T), -7, np.int32), count=np.full(n, -7, np.int32),
                 status=np.full(n, -99, np.int32), n_quads=np.full(n, -7, np.int32), n_foreign=np.full(n, -7, np.int32),
                 n_edges_dropped=np.full(n, -7, np.int32), strength=np.full((n, T, 4), -7.0))
        V = lambda a: a.ctypes.data_as(C.c_void_p)
        ref = lambda o: C.byref(o) if o is not None else None
        fam = family.c_struct()
        check(self._L.clc_tag_grid(self._h, C.byref(fam), ref(tag_options), ref(chess_options), ref(subpix_options), *img_args,
                                   C.c_size_t(n), C.c_int32(cols), C.c_int32(rows), V(r["corners"]), V(r["hamming"]), V(r["count"]), V(r["status"]),
                                   V(r["n_quads"]), V(r["n_foreign"]), V(r["n_edges_dropped"]), V(r["strength"])), "clc_tag_grid")
        return r

    def tag_grid_device(self, images_ptr: int, width: int, height: int, pitch: int, n_images: int, family: "TagFamily", cols: int, rows: int,
                        corners_ptr: int, hamming_ptr: int, count_ptr: int, status_ptr: int, n_quads_ptr: int = 0, n_foreign_ptr: int = 0,
                        n_edges_dropped_ptr: int = 0, strength_ptr: int = 0, tag_options: Optional[TagOptions] = None,
                        chess_options: Optional[ChessOptions] = None, subpix_options: Optional[SubpixOptions] = None):
        """clc_tag_grid_device on device-resident arrays (data_ptr()s; ready on the solver's stream): images uint8, corners
        [n, cols rows, 4, 2] float32, hamming [n, cols rows] int32, count and status [n] int32; the others may be left out."""
        V = lambda p: C.c_void_p(p or 0)
        ref = lambda o: C.byref(o) if o is not None else None
        fam = family.c_struct()
        check(self._L.clc_tag_grid_device(self._h, C.byref(fam), ref(tag_options), ref(chess_options), ref(subpix_options), V(images_ptr),
                                          C.c_int32(width), C.c_int32(height), C.c_int64(pitch), C.c_size_t(n_images), C.c_int32(cols),
                                          C.c_int32(rows), V(corners_ptr), V(hamming_ptr), V(count_ptr), V(status_ptr), V(n_quads_ptr),
                                          V(n_foreign_ptr), V(n_edges_dropped_ptr), V(strength_ptr)), "clc_tag_grid_device")

    def tag_grid_points_device(self, corners_ptr: int, hamming_ptr: int, n_images: int, cols: int, rows: int, tag_size: float,
                               tag_spacing: float, corners_px_ptr: int, board_xy_ptr: int, offsets_ptr: int):
        """clc_tag_grid_points_device: the seen tags of tag_grid_device's result, image by image in id order, as board_poses_device takes
        them: corners_px and board_xy [n 4 cols rows, 2] float32 (the capacity), offsets [n + 1] int64."""
        V = lambda p: C.c_void_p(p or 0)
        check(self._L.clc_tag_grid_points_device(self._h, V(corners_ptr), V(hamming_ptr), C.c_size_t(n_images), C.c_int32(cols), C.c_int32(rows),
                                                 C.c_double(tag_size), C.c_double(tag_spacing), V(corners_px_ptr), V(board_xy_ptr),
                                                 V(offsets_ptr)), "clc_tag_grid_points_device")

    # ---- camera intrinsics from the board images (K19) ----
    def camera_guess(self, model: int, width: int, height: int, corners_px: np.ndarray, board_xy: np.ndarray, offsets: np.ndarray):
        """clc_camera_guess: the closed-form start -> (Camera with fx = fy, the principal point at the image centre and zero distortion,
        n_used).  Raises ClcError where the images give no focal length."""
        from .camera import Camera, ClcCamera
        cp = np.ascontiguousarray(corners_px, dtype=np.float32).reshape(-1, 2)
        bx = np.ascontiguousarray(board_xy, dtype=np.float32).reshape(-1, 2)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(off) - 1
        if n < 0 or (n > 0 and (off[0] < 0 or off[-1] > len(cp) or off[-1] > len(bx))):
            raise ValueError("camera_guess: offsets run past corners_px or board_xy")
        c, used = ClcCamera(), C.c_int32(0)
        V = lambda a: a.ctypes.data_as(C.c_void_p)
        check(self._L.clc_camera_guess(self._h, C.c_int32(model), C.c_int32(width), C.c_int32(height), V(cp), V(bx), V(off), C.c_size_t(n),
                                       C.byref(c), C.byref(used)), "clc_camera_guess")
        return Camera(c.model, tuple(c.proj), tuple(c.dist), int(width), int(height)), used.value

    def camera_guess_device(self, model: int, width: int, height: int, corners_ptr: int, board_ptr: int, offsets_ptr: int, n_images: int):
        """clc_camera_guess_device on device-resident corners, board points and offsets (data_ptr()s) -> (Camera, n_used)."""
        from .camera import Camera, ClcCamera
        c, used = ClcCamera(), C.c_int32(0)
        V = lambda p: C.c_void_p(p or 0)
        check(self._L.clc_camera_guess_device(self._h, C.c_int32(model), C.c_int32(width), C.c_int32(height), V(corners_ptr), V(board_ptr),
                                              V(offsets_ptr), C.c_size_t(n_images), C.byref(c), C.byref(used)), "clc_camera_guess_device")
        return Camera(c.model, tuple(c.proj), tuple(c.dist), int(width), int(height)), used.value

    def camera_calibrate(self, cameras, corners_px: np.ndarray, board_xy: np.ndarray, corner_offsets: np.ndarray, q_ca_wxyz: np.ndarray,
                         t_ca: np.ndarray, problem_offsets: Optional[np.ndarray] = None, keep: Optional[np.ndarray] = None,
                         options: Optional[Options] = None, camcal: Optional[CamcalOptions] = None) -> dict:
        """clc_camera_calibrate (K19): per problem the reprojection error in pixels over sigma_px, minimised over the free intrinsics and
        every board pose.  cameras: one Camera (one problem) or a sequence, one per problem: the starts.  Image i owns corners
        [corner_offsets[i], corner_offsets[i+1]); problem k owns images [problem_offsets[k], problem_offsets[k+1]) (None: one problem).
        q_ca_wxyz [n, 4], t_ca [n, 3]: the start poses (not modified).
        -> dict(cameras [list of Camera], q [n, 4], t [n, 3], summaries, H_cam [n_problems, 8, 8], rms_px [n_problems], status [n] int32
        (CLC_CAMCAL_*))."""
        from .camera import Camera, ClcCamera
        cams_in = [cameras] if isinstance(cameras, Camera) else list(cameras)
        cp = np.ascontiguousarray(corners_px, dtype=np.float32).reshape(-1, 2)
        bx = np.ascontiguousarray(board_xy, dtype=np.float32).reshape(-1, 2)
        co = np.ascontiguousarray(corner_offsets, dtype=np.int64)
        n = len(co) - 1
        if n < 0 or (n > 0 and (co[-1] > len(cp) or co[-1] > len(bx) or co[0] < 0)):
            raise ValueError("camera_calibrate: offsets run past corners_px or board_xy")
        pr = None if problem_offsets is None else np.ascontiguousarray(problem_offsets, dtype=np.int64)
        npb = 1 if pr is None else len(pr) - 1
        if len(cams_in) != npb:
            raise ValueError("camera_calibrate: one camera per problem")
        if pr is not None and (len(pr) < 1 or (len(pr) > 1 and pr[-1] > n)):
            raise ValueError("camera_calibrate: problem_offsets run past the images")
        q = np.array(q_ca_wxyz, dtype=np.float64, order="C").reshape(n, 4)
        t = np.array(t_ca, dtype=np.float64, order="C").reshape(n, 3)
        kp = None if keep is None else np.ascontiguousarray(np.asarray(keep).astype(np.uint8))
        if kp is not None and kp.shape != (n,):
            raise ValueError("camera_calibrate: keep needs one entry per image")
        cams = (ClcCamera * max(npb, 1))(*[c.to_c() for c in cams_in])
        sm = (Summary * max(npb, 1))()
        H = np.empty((npb, 8, 8)); rms = np.empty(npb); st = np.empty(n, dtype=np.int32)
        V = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(self._L.clc_camera_calibrate(self._h, C.byref(options) if options is not None else None,
                                           C.byref(camcal) if camcal is not None else None, V(cp), V(bx), V(co), V(kp), C.c_size_t(n), V(pr),
                                           C.c_size_t(npb), cams, V(q), V(t), sm, V(H), V(rms), V(st)), "clc_camera_calibrate")
        out = [Camera(cams[k].model, tuple(cams[k].proj), tuple(cams[k].dist), cams_in[k].width, cams_in[k].height) for k in range(npb)]
        return dict(cameras=out, q=q, t=t, summaries=sm, H_cam=H, rms_px=rms, status=st)

    def camera_calibrate_device(self, corners_ptr: int, board_ptr: int, corner_offsets_ptr: int, n_images: int, n_problems: int,
                                cameras_ptr: int, q_ptr: int, t_ptr: int, summaries_ptr: int, status_ptr: int, problem_offsets_ptr: int = 0,
                                keep_ptr: int = 0, H_cam_ptr: int = 0, rms_ptr: int = 0, options: Optional[Options] = None,
                                camcal: Optional[CamcalOptions] = None):
        """clc_camera_calibrate_device on device-resident arrays (data_ptr()s; ready on the solver's stream): cameras as clc_camera
        records (72 bytes each), in / out like q and t; the per-image arrays are indexed by the absolute image index."""
        V = lambda p: C.c_void_p(p or 0)
        check(self._L.clc_camera_calibrate_device(self._h, C.byref(options) if options is not None else None,
                                                  C.byref(camcal) if camcal is not None else None, V(corners_ptr), V(board_ptr),
                                                  V(corner_offsets_ptr), V(keep_ptr), C.c_size_t(n_images), V(problem_offsets_ptr),
                                                  C.c_size_t(n_problems), V(cameras_ptr), V(q_ptr), V(t_ptr), V(summaries_ptr), V(H_cam_ptr),
                                                  V(rms_ptr), V(status_ptr)), "clc_camera_calibrate_device")

    # ---- one robust cost over intrinsics, board poses, T_cl and range (K23) ----
    def calibrate_full(self, cameras, corners_px, board_xy, corner_offsets, pts: np.ndarray, pts_offsets: np.ndarray,
                       q_ca_wxyz: np.ndarray, t_ca: np.ndarray, poses_cl: np.ndarray, range0: Optional[np.ndarray] = None,
                       problem_offsets: Optional[np.ndarray] = None, keep: Optional[np.ndarray] = None,
                       options: Optional[Options] = None, full: Optional[FullOptions] = None) -> dict:
        """clc_calibrate_full (K23): per problem the pixel reprojection error of the corners and the point-to-plane error of the
        range-corrected laser points under one Cauchy cost, minimised over the free members of [T_cl, b, kappa, the 8 intrinsics] and
        every board pose.  cameras: one Camera (one problem) or one per problem: the starts.  The other arguments are
        joint_refine_range's; corners_px, board_xy and corner_offsets may be None where full holds the board poses and all 8
        intrinsics.  full None: clc_full_options_default of the first camera's model.
        -> dict(cameras [list of Camera], q [n, 4], t [n, 3], poses_cl [n_problems, 7], range [n_problems, 2], summaries, H_full
        [n_problems, 16, 16] (order: dt_cl, dtheta_cl, b, kappa, proj[0..3], dist[0..3]), cost_parts [n_problems, 2], rms_px
        [n_problems], status [n] int32 (CLC_JOINT_*), w_corner [len(corners_px)], w_laser [len(pts)]: rho' of every observation at
        the returned point, NaN for an image that takes no part)."""
        from .camera import Camera, ClcCamera
        cams_in = [cameras] if isinstance(cameras, Camera) else list(cameras)
        P = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        po = np.ascontiguousarray(pts_offsets, dtype=np.int64)
        n = len(po) - 1
        cp = bx = co = None
        if corner_offsets is not None:
            cp = np.ascontiguousarray(corners_px, dtype=np.float32).reshape(-1, 2)
            bx = np.ascontiguousarray(board_xy, dtype=np.float32).reshape(-1, 2)
            co = np.ascontiguousarray(corner_offsets, dtype=np.int64)
            if len(co) != n + 1:
                raise ValueError("calibrate_full: corner_offsets and pts_offsets need one entry per image plus one")
            if n > 0 and (co[-1] > len(cp) or co[-1] > len(bx) or co[0] < 0):
                raise ValueError("calibrate_full: offsets run past corners_px or board_xy")
        if n < 0 or (n > 0 and (po[-1] > len(P) or po[0] < 0)):
            raise ValueError("calibrate_full: offsets run past pts")
        pr = None if problem_offsets is None else np.ascontiguousarray(problem_offsets, dtype=np.int64)
        npb = 1 if pr is None else len(pr) - 1
        if len(cams_in) != npb:
            raise ValueError("calibrate_full: one camera per problem")
        if pr is not None and (len(pr) < 1 or (len(pr) > 1 and pr[-1] > n)):
            raise ValueError("calibrate_full: problem_offsets run past the images")
        q = np.array(q_ca_wxyz, dtype=np.float64, order="C").reshape(n, 4)
        t = np.array(t_ca, dtype=np.float64, order="C").reshape(n, 3)
        cl = np.array(poses_cl, dtype=np.float64, order="C").reshape(npb, 7)
        rg = np.zeros((npb, 2)) if range0 is None else np.array(range0, dtype=np.float64, order="C").reshape(npb, 2)
        kp = None if keep is None else np.ascontiguousarray(np.asarray(keep).astype(np.uint8))
        if kp is not None and kp.shape != (n,):
            raise ValueError("calibrate_full: keep needs one entry per image")
        cams = (ClcCamera * max(npb, 1))(*[c.to_c() for c in cams_in])
        sm = (Summary * max(npb, 1))()
        H = np.empty((npb, 16, 16)); parts = np.empty((npb, 2)); rms = np.empty(npb); st = np.empty(n, dtype=np.int32)
        wc = None if cp is None else np.full(len(cp), np.nan)
        wl = np.full(len(P), np.nan)
        V = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        check(self._L.clc_calibrate_full(self._h, cams, C.byref(options) if options is not None else None,
                                         C.byref(full) if full is not None else None, V(cp), V(bx), V(co), V(P), V(po), V(kp), C.c_size_t(n),
                                         V(pr), C.c_size_t(npb), V(q), V(t), V(cl), V(rg), sm, V(H), V(parts), V(rms), V(st), V(wc), V(wl)),
              "clc_calibrate_full")
        out = [Camera(cams[k].model, tuple(cams[k].proj), tuple(cams[k].dist), cams_in[k].width, cams_in[k].height) for k in range(npb)]
        return dict(cameras=out, q=q, t=t, poses_cl=cl, range=rg, summaries=sm, H_full=H, cost_parts=parts, rms_px=rms, status=st,
                    w_corner=wc, w_laser=wl)

    def calibrate_full_device(self, cameras_ptr: int, corners_ptr: int, board_ptr: int, corner_offsets_ptr: int, pts_ptr: int,
                              pts_offsets_ptr: int, n_images: int, n_problems: int, q_ptr: int, t_ptr: int, poses_cl_ptr: int,
                              range_ptr: int, summaries_ptr: int, status_ptr: int, problem_offsets_ptr: int = 0, keep_ptr: int = 0,
                              H_full_ptr: int = 0, cost_parts_ptr: int = 0, rms_ptr: int = 0, w_corner_ptr: int = 0, w_laser_ptr: int = 0,
                              options: Optional[Options] = None, full: Optional[FullOptions] = None):
        """clc_calibrate_full_device on device-resident arrays (data_ptr()s; ready on the solver's stream): joint_refine_device's
        conventions, cameras as clc_camera records (72 bytes each) in / out as in camera_calibrate_device; w_corner, w_laser
        (float64) are indexed by the absolute corner / point offsets.  Nothing is read back ahead of the enqueue."""
        V = lambda p: C.c_void_p(p or 0)
        check(self._L.clc_calibrate_full_device(self._h, V(cameras_ptr), C.byref(options) if options is not None else None,
                                                C.byref(full) if full is not None else None, V(corners_ptr), V(board_ptr),
                                                V(corner_offsets_ptr), V(pts_ptr), V(pts_offsets_ptr), V(keep_ptr), C.c_size_t(n_images),
                                                V(problem_offsets_ptr), C.c_size_t(n_problems), V(q_ptr), V(t_ptr), V(poses_cl_ptr),
                                                V(range_ptr), V(summaries_ptr), V(H_full_ptr), V(cost_parts_ptr), V(rms_ptr), V(status_ptr),
                                                V(w_corner_ptr), V(w_laser_ptr)), "clc_calibrate_full_device")

    # ---- board-segment detection ----
    def board_segments(self, points: np.ndarray, offsets: np.ndarray):
        """AutoGetLinePts (src/selectScanPoints.cpp:17-190) for many scans: points [M,3], CSR offsets [S+1] ->
        (seg [S,2] int64: first, last index of the board's segment in its scan, inclusive, or -1, -1;
        status [S] int32: CLC_SEG_FOUND 1, CLC_SEG_NONE 0, CLC_SEG_REF_THROWS -1 where the reference raises)."""
        P = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        S = len(offsets) - 1
        seg = np.empty((max(S, 0), 2), dtype=np.int64)
        status = np.empty(max(S, 0), dtype=np.int32)
        check(self._L.clc_board_segments(self._h, dptr(P) if P.size else None, iptr(offsets), C.c_size_t(S),
                                         seg.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)), "clc_board_segments")
        return seg, status

    def board_segments_device(self, points_ptr: int, offsets_ptr: int, n_scans: int, seg_ptr: int, status_ptr: int = 0):
        """AutoGetLinePts on device-resident arrays (data_ptr()s; ready on the solver's stream): points [M,3] float64,
        offsets [S+1] int64, seg [S,2] int64 out, status [S] int32 out (0: not written)."""
        check(self._L.clc_board_segments_device(self._h, C.c_void_p(points_ptr), C.c_void_p(offsets_ptr), C.c_size_t(n_scans),
                                                C.c_void_p(seg_ptr), C.c_void_p(status_ptr or 0)), "clc_board_segments_device")

    # ---- the offline flow: stamped tag poses + raw scans -> stored observations (K13) ----
    def keyframes(self, q_wc: np.ndarray, t_wc: np.ndarray, options: Optional["_capi.AssembleOptions"] = None) -> np.ndarray:
        """The key-frame filter of main/calibr_offline.cpp:62-78 on tag poses q_wc [n, 4] (w, x, y, z), t_wc [n, 3] -> keep [n] bool."""
        q = np.ascontiguousarray(q_wc, dtype=np.float64).reshape(-1, 4)
        t = np.ascontiguousarray(t_wc, dtype=np.float64).reshape(-1, 3)
        assert q.shape[0] == t.shape[0], "one translation per quaternion"
        keep = np.zeros(q.shape[0], dtype=np.uint8)
        n = C.c_int64()
        o = options or _capi.default_assemble_options()
        check(self._L.clc_keyframes(self._h, C.byref(o), q.shape[0], q.ctypes.data, t.ctypes.data, keep.ctypes.data, C.byref(n)), "clc_keyframes")
        assert n.value == int(keep.sum())
        return keep.astype(bool)

    def assemble_observations(self, pose_stamp, q_wc, t_wc, scans: dict, scan_stamp, options: Optional["_capi.AssembleOptions"] = None):
        """main/calibr_offline.cpp:62-155 in one call: stamped tag poses (pose_stamp [n], q_wc [n, 4] (w, x, y, z), t_wc [n, 3]) and
        raw scans (`scans` as simdata.sim_laser_scans returns them: ranges, offsets, angle_min, angle_increment, range_min;
        scan_stamp [S]) -> (AssembleInfo, scan_pose [S] int32).  The observations are left stored on the handle
        (select_observations, closed_form, solve, information follow; stored_observations() copies them back)."""
        ps = np.ascontiguousarray(pose_stamp, dtype=np.float64).reshape(-1)
        q = np.ascontiguousarray(q_wc, dtype=np.float64).reshape(-1, 4)
        t = np.ascontiguousarray(t_wc, dtype=np.float64).reshape(-1, 3)
        assert q.shape[0] == t.shape[0] == ps.shape[0], "one stamp, quaternion and translation per pose"
        r = np.ascontiguousarray(scans["ranges"], dtype=np.float32)
        off = np.ascontiguousarray(scans["offsets"], dtype=np.int64)
        S = len(off) - 1
        f = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (S,)))
        am, ai, rm = f(scans["angle_min"]), f(scans["angle_increment"]), f(scans["range_min"])
        ss = np.ascontiguousarray(scan_stamp, dtype=np.float64).reshape(-1)
        assert ss.shape[0] == S, "one stamp per scan"
        scan_pose = np.zeros(S, dtype=np.int32)
        info = _capi.AssembleInfo()
        o = options or _capi.default_assemble_options()
        check(self._L.clc_assemble_observations(self._h, C.byref(o), ps.shape[0], ps.ctypes.data, q.ctypes.data, t.ctypes.data, r.ctypes.data,
                                                off.ctypes.data, S, am.ctypes.data, ai.ctypes.data, rm.ctypes.data, ss.ctypes.data,
                                                scan_pose.ctypes.data, C.byref(info)), "clc_assemble_observations")
        return info, scan_pose

    def assemble_observations_device(self, n_poses: int, pose_stamp_ptr: int, q_wc_ptr: int, t_wc_ptr: int, ranges_ptr: int, offsets_ptr: int,
                                     n_scans: int, n_rays: int, angle_min_ptr: int, angle_increment_ptr: int, range_min_ptr: int,
                                     scan_stamp_ptr: int, scan_pose_ptr: int = 0, options: Optional["_capi.AssembleOptions"] = None):
        """clc_assemble_observations_device on device-resident arrays (data_ptr()s; ready on the solver's stream) -> AssembleInfo."""
        info = _capi.AssembleInfo()
        o = options or _capi.default_assemble_options()
        check(self._L.clc_assemble_observations_device(self._h, C.byref(o), n_poses, pose_stamp_ptr or None, q_wc_ptr or None, t_wc_ptr or None,
                                                       ranges_ptr or None, offsets_ptr or None, n_scans, n_rays, angle_min_ptr or None,
                                                       angle_increment_ptr or None, range_min_ptr or None, scan_stamp_ptr or None,
                                                       scan_pose_ptr or None, C.byref(info)), "clc_assemble_observations_device")
        return info

    # ---- static stations: averaged tag poses and station-mode assembly (K14) ----
    def static_poses(self, pose_stamp, q_wc, t_wc, options: Optional["_capi.StationOptions"] = None, cap_stations: Optional[int] = None) -> dict:
        """GetStaticPose (src/utilities.cpp:86-155) on stamped tag poses (pose_stamp [n] or None: the stamps come back 0; q_wc [n, 4]
        (w, x, y, z), t_wc [n, 3]) -> {"n_stations" (the true count), "first", "last" [k] int64 (pose indices of the first and the
        last member), "start_time", "end_time" [k], "q" [k, 4], "t" [k, 3], "status" [k] int32 (CLC_STATION_*)}; k = n_stations, or
        at most cap_stations when given (0: the count alone)."""
        q = np.ascontiguousarray(q_wc, dtype=np.float64).reshape(-1, 4)
        t = np.ascontiguousarray(t_wc, dtype=np.float64).reshape(-1, 3)
        ps = None if pose_stamp is None else np.ascontiguousarray(pose_stamp, dtype=np.float64).reshape(-1)
        assert q.shape[0] == t.shape[0] and (ps is None or ps.shape[0] == q.shape[0]), "one stamp, quaternion and translation per pose"
        o = options or _capi.default_station_options()
        n = C.c_int64()
        args = (self._h, C.byref(o), q.shape[0], None if ps is None else ps.ctypes.data, q.ctypes.data, t.ctypes.data)
        if cap_stations is None:
            check(self._L.clc_static_poses(*args, 0, None, None, None, None, None, None, None, C.byref(n)), "clc_static_poses")
            cap_stations = n.value
        k = int(cap_stations)
        out = {"first": np.zeros(k, np.int64), "last": np.zeros(k, np.int64), "start_time": np.zeros(k), "end_time": np.zeros(k),
               "q": np.zeros((k, 4)), "t": np.zeros((k, 3)), "status": np.zeros(k, np.int32)}
        ptr = lambda a: a.ctypes.data if k > 0 else None
        check(self._L.clc_static_poses(*args, k, ptr(out["first"]), ptr(out["last"]), ptr(out["start_time"]), ptr(out["end_time"]), ptr(out["q"]),
                                       ptr(out["t"]), ptr(out["status"]), C.byref(n)), "clc_static_poses")
        out["n_stations"] = n.value
        return out

    def assemble_stations(self, pose_stamp, q_wc, t_wc, scans: dict, scan_stamp, options: Optional["_capi.StationOptions"] = None):
        """assemble_observations in station mode: the stamped tag poses are averaged per static station (static_poses) and every scan
        with a board segment whose stamp lies in a station's [start_time, end_time] becomes one observation with that station's
        averaged pose -> (StationInfo, scan_station [S] int32).  The observations are left stored on the handle."""
        ps = np.ascontiguousarray(pose_stamp, dtype=np.float64).reshape(-1)
        q = np.ascontiguousarray(q_wc, dtype=np.float64).reshape(-1, 4)
        t = np.ascontiguousarray(t_wc, dtype=np.float64).reshape(-1, 3)
        assert q.shape[0] == t.shape[0] == ps.shape[0], "one stamp, quaternion and translation per pose"
        r = np.ascontiguousarray(scans["ranges"], dtype=np.float32)
        off = np.ascontiguousarray(scans["offsets"], dtype=np.int64)
        S = len(off) - 1
        f = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (S,)))
        am, ai, rm = f(scans["angle_min"]), f(scans["angle_increment"]), f(scans["range_min"])
        ss = np.ascontiguousarray(scan_stamp, dtype=np.float64).reshape(-1)
        assert ss.shape[0] == S, "one stamp per scan"
        scan_station = np.zeros(S, dtype=np.int32)
        info = _capi.StationInfo()
        o = options or _capi.default_station_options()
        check(self._L.clc_assemble_stations(self._h, C.byref(o), ps.shape[0], ps.ctypes.data, q.ctypes.data, t.ctypes.data, r.ctypes.data,
                                            off.ctypes.data, S, am.ctypes.data, ai.ctypes.data, rm.ctypes.data, ss.ctypes.data,
                                            scan_station.ctypes.data, C.byref(info)), "clc_assemble_stations")
        return info, scan_station

    def assemble_stations_device(self, n_poses: int, pose_stamp_ptr: int, q_wc_ptr: int, t_wc_ptr: int, ranges_ptr: int, offsets_ptr: int,
                                 n_scans: int, n_rays: int, angle_min_ptr: int, angle_increment_ptr: int, range_min_ptr: int,
                                 scan_stamp_ptr: int, scan_station_ptr: int = 0, options: Optional["_capi.StationOptions"] = None):
        """clc_assemble_stations_device on device-resident arrays (data_ptr()s; ready on the solver's stream) -> StationInfo."""
        info = _capi.StationInfo()
        o = options or _capi.default_station_options()
        check(self._L.clc_assemble_stations_device(self._h, C.byref(o), n_poses, pose_stamp_ptr or None, q_wc_ptr or None, t_wc_ptr or None,
                                                   ranges_ptr or None, offsets_ptr or None, n_scans, n_rays, angle_min_ptr or None,
                                                   angle_increment_ptr or None, range_min_ptr or None, scan_stamp_ptr or None,
                                                   scan_station_ptr or None, C.byref(info)), "clc_assemble_stations_device")
        return info

    # ---- interpolated tag poses: one observation per scan, the pose interpolated at the scan's stamp (K15) ----
    def interpolate_poses(self, pose_stamp, q_wc, t_wc, query_stamp, options: Optional["_capi.InterpOptions"] = None) -> dict:
        """The tag pose at every query stamp (+ options.time_offset), between the two stamped poses that bracket it (pose_stamp [n],
        q_wc [n, 4] (w, x, y, z), t_wc [n, 3] in file order; include/clc.h states the rule) -> {"bracket" [m] int32 (the index of the
        bracket's first pose, or SCAN_NO_POSE), "u" [m], "q" [m, 4] (unit), "t" [m, 3]}."""
        ps = np.ascontiguousarray(pose_stamp, dtype=np.float64).reshape(-1)
        q = np.ascontiguousarray(q_wc, dtype=np.float64).reshape(-1, 4)
        t = np.ascontiguousarray(t_wc, dtype=np.float64).reshape(-1, 3)
        assert q.shape[0] == t.shape[0] == ps.shape[0], "one stamp, quaternion and translation per pose"
        x = np.ascontiguousarray(query_stamp, dtype=np.float64).reshape(-1)
        m = x.shape[0]
        out = {"bracket": np.zeros(m, np.int32), "u": np.zeros(m), "q": np.zeros((m, 4)), "t": np.zeros((m, 3))}
        o = options or _capi.default_interp_options()
        check(self._L.clc_interpolate_poses(self._h, C.byref(o), ps.shape[0], ps.ctypes.data, q.ctypes.data, t.ctypes.data, m, x.ctypes.data,
                                            out["bracket"].ctypes.data, out["u"].ctypes.data, out["q"].ctypes.data, out["t"].ctypes.data),
              "clc_interpolate_poses")
        return out

    def assemble_interpolated(self, pose_stamp, q_wc, t_wc, scans: dict, scan_stamp, options: Optional["_capi.InterpOptions"] = None):
        """assemble_observations with the tag pose interpolated at every scan's stamp (+ options.time_offset): every scan with a board
        segment and a bracket becomes one observation -> (AssembleInfo, scan_bracket [S] int32, scan_u [S]).  The observations are
        left stored on the handle."""
        ps = np.ascontiguousarray(pose_stamp, dtype=np.float64).reshape(-1)
        q = np.ascontiguousarray(q_wc, dtype=np.float64).reshape(-1, 4)
        t = np.ascontiguousarray(t_wc, dtype=np.float64).reshape(-1, 3)
        assert q.shape[0] == t.shape[0] == ps.shape[0], "one stamp, quaternion and translation per pose"
        r = np.ascontiguousarray(scans["ranges"], dtype=np.float32)
        off = np.ascontiguousarray(scans["offsets"], dtype=np.int64)
        S = len(off) - 1
        f = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (S,)))
        am, ai, rm = f(scans["angle_min"]), f(scans["angle_increment"]), f(scans["range_min"])
        ss = np.ascontiguousarray(scan_stamp, dtype=np.float64).reshape(-1)
        assert ss.shape[0] == S, "one stamp per scan"
        scan_bracket = np.zeros(S, dtype=np.int32)
        scan_u = np.zeros(S)
        info = _capi.AssembleInfo()
        o = options or _capi.default_interp_options()
        check(self._L.clc_assemble_interpolated(self._h, C.byref(o), ps.shape[0], ps.ctypes.data, q.ctypes.data, t.ctypes.data, r.ctypes.data,
                                                off.ctypes.data, S, am.ctypes.data, ai.ctypes.data, rm.ctypes.data, ss.ctypes.data,
                                                scan_bracket.ctypes.data, scan_u.ctypes.data, C.byref(info)), "clc_assemble_interpolated")
        return info, scan_bracket, scan_u

    def assemble_interpolated_device(self, n_poses: int, pose_stamp_ptr: int, q_wc_ptr: int, t_wc_ptr: int, ranges_ptr: int, offsets_ptr: int,
                                     n_scans: int, n_rays: int, angle_min_ptr: int, angle_increment_ptr: int, range_min_ptr: int,
                                     scan_stamp_ptr: int, scan_bracket_ptr: int = 0, scan_u_ptr: int = 0,
                                     options: Optional["_capi.InterpOptions"] = None):
        """clc_assemble_interpolated_device on device-resident arrays (data_ptr()s; ready on the solver's stream) -> AssembleInfo."""
        info = _capi.AssembleInfo()
        o = options or _capi.default_interp_options()
        check(self._L.clc_assemble_interpolated_device(self._h, C.byref(o), n_poses, pose_stamp_ptr or None, q_wc_ptr or None, t_wc_ptr or None,
                                                       ranges_ptr or None, offsets_ptr or None, n_scans, n_rays, angle_min_ptr or None,
                                                       angle_increment_ptr or None, range_min_ptr or None, scan_stamp_ptr or None,
                                                       scan_bracket_ptr or None, scan_u_ptr or None, C.byref(info)),
              "clc_assemble_interpolated_device")
        return info

    def time_offset_sweep(self, pose_stamp, q_wc, t_wc, scans: dict, scan_stamp, pose0: np.ndarray,
                          options: Optional["_capi.TimeOffsetOptions"] = None) -> dict:
        """The camera-laser clock sweep (include/clc.h, K15): one calibration problem per candidate offset on the same scans and points,
        the tag poses interpolated at scan_stamp + offset, solved as one batch from pose0 (T_cl, [tx, ty, tz, qx, qy, qz, qw]) ->
        {"offsets" [n], "final_cost" [n], "poses" [n, 7], "summaries" (Summary array [n]), "n_scans_used", "records_per_problem",
        "best_index", "best_offset", "at_edge"}.  The handle's batch is the sweep's afterwards; the stored observations are untouched."""
        ps = np.ascontiguousarray(pose_stamp, dtype=np.float64).reshape(-1)
        q = np.ascontiguousarray(q_wc, dtype=np.float64).reshape(-1, 4)
        t = np.ascontiguousarray(t_wc, dtype=np.float64).reshape(-1, 3)
        assert q.shape[0] == t.shape[0] == ps.shape[0], "one stamp, quaternion and translation per pose"
        r = np.ascontiguousarray(scans["ranges"], dtype=np.float32)
        off = np.ascontiguousarray(scans["offsets"], dtype=np.int64)
        S = len(off) - 1
        f = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (S,)))
        am, ai, rm = f(scans["angle_min"]), f(scans["angle_increment"]), f(scans["range_min"])
        ss = np.ascontiguousarray(scan_stamp, dtype=np.float64).reshape(-1)
        assert ss.shape[0] == S, "one stamp per scan"
        p0 = np.ascontiguousarray(pose0, dtype=np.float64).reshape(7)
        o = options or _capi.default_time_offset_options()
        n = max(int(o.n_offsets), 0)
        out = {"offsets": np.zeros(n), "final_cost": np.full(n, np.nan), "poses": np.tile(p0, (n, 1)), "summaries": (Summary * n)()}
        res = _capi.TimeOffsetResult()
        check(self._L.clc_clock_offset_sweep(self._h, C.byref(o), ps.shape[0], ps.ctypes.data, q.ctypes.data, t.ctypes.data, r.ctypes.data,
                                            off.ctypes.data, S, am.ctypes.data, ai.ctypes.data, rm.ctypes.data, ss.ctypes.data, p0.ctypes.data,
                                            out["offsets"].ctypes.data, out["final_cost"].ctypes.data, out["poses"].ctypes.data,
                                            C.byref(out["summaries"]), C.byref(res)), "clc_clock_offset_sweep")
        out.update({k: getattr(res, k) for k, _ in res._fields_})
        return out

    def time_offset_sweep_device(self, n_poses: int, pose_stamp_ptr: int, q_wc_ptr: int, t_wc_ptr: int, ranges_ptr: int, offsets_ptr: int,
                                 n_scans: int, n_rays: int, angle_min_ptr: int, angle_increment_ptr: int, range_min_ptr: int,
                                 scan_stamp_ptr: int, pose0: np.ndarray, options: Optional["_capi.TimeOffsetOptions"] = None) -> dict:
        """clc_clock_offset_sweep_device on a device-resident recording (data_ptr()s; ready on the solver's stream) -> time_offset_sweep's dict."""
        p0 = np.ascontiguousarray(pose0, dtype=np.float64).reshape(7)
        o = options or _capi.default_time_offset_options()
        n = max(int(o.n_offsets), 0)
        out = {"offsets": np.zeros(n), "final_cost": np.full(n, np.nan), "poses": np.tile(p0, (n, 1)), "summaries": (Summary * n)()}
        res = _capi.TimeOffsetResult()
        check(self._L.clc_clock_offset_sweep_device(self._h, C.byref(o), n_poses, pose_stamp_ptr or None, q_wc_ptr or None, t_wc_ptr or None,
                                                   ranges_ptr or None, offsets_ptr or None, n_scans, n_rays, angle_min_ptr or None,
                                                   angle_increment_ptr or None, range_min_ptr or None, scan_stamp_ptr or None, p0.ctypes.data,
                                                   out["offsets"].ctypes.data, out["final_cost"].ctypes.data, out["poses"].ctypes.data,
                                                   C.byref(out["summaries"]), C.byref(res)), "clc_clock_offset_sweep_device")
        out.update({k: getattr(res, k) for k, _ in res._fields_})
        return out

    def debug_sweep_records(self) -> np.ndarray:
        """Test hook: the records [n_offsets * records_per_problem, 8] the last time_offset_sweep[_device] of this process uploaded."""
        n = C.c_int64()
        f = self._hook("clc_debug_sweep_records")
        check(f(None, C.c_int64(0), C.byref(n)), "clc_debug_sweep_records")
        out = np.zeros((n.value // 8, 8))
        check(f(out.ctypes.data_as(C.c_void_p), C.c_int64(n.value), C.byref(n)), "clc_debug_sweep_records")
        return out

    def debug_station_walk(self, t_wc, options: Optional["_capi.StationOptions"] = None) -> dict:
        """Test hook: the walk of static_poses alone -> {"first", "last", "members" [k] int64, "n_stations", "n_runs"}."""
        t = np.ascontiguousarray(t_wc, dtype=np.float64).reshape(-1, 3)
        o = options or _capi.default_station_options()
        f = self._hook("clc_debug_station_walk")
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        ns, nr = C.c_int64(), C.c_int64()
        check(f(self._h, C.byref(o), t.shape[0], t.ctypes.data, 0, None, None, None, C.byref(ns), C.byref(nr)), "clc_debug_station_walk")
        k = ns.value
        out = {"first": np.zeros(k, np.int64), "last": np.zeros(k, np.int64), "members": np.zeros(k, np.int64)}
        if k > 0:
            check(f(self._h, C.byref(o), t.shape[0], t.ctypes.data, k, out["first"].ctypes.data, out["last"].ctypes.data,
                    out["members"].ctypes.data, C.byref(ns), C.byref(nr)), "clc_debug_station_walk")
        out["n_stations"], out["n_runs"] = ns.value, nr.value
        return out

    def stored_observations(self):
        """The scans stored on the handle (store_observations / assemble_observations), copied back -> simdata.ObservationSet."""
        from .simdata import ObservationSet
        n = C.c_int()
        check(self._L.clc_stored_observations(self._h, C.byref(n), None, None, None, None, None, None, None), "clc_stored_observations")
        P = n.value
        pts_off = np.zeros(P + 1, dtype=np.int64); ptl_off = np.zeros(P + 1, dtype=np.int64)
        check(self._L.clc_stored_observations(self._h, None, None, None, pts_off.ctypes.data, None, ptl_off.ctypes.data, None),
              "clc_stored_observations")
        tq = np.zeros((P, 4)); tt = np.zeros((P, 3)); pts = np.zeros((int(pts_off[P]), 3)); ptl = np.zeros((int(ptl_off[P]), 3))
        check(self._L.clc_stored_observations(self._h, None, tq.ctypes.data, tt.ctypes.data, None, pts.ctypes.data, None, ptl.ctypes.data),
              "clc_stored_observations")
        return ObservationSet(tq, tt, pts_off, pts, ptl_off, ptl)

    def debug_assemble_lines(self) -> np.ndarray:
        """Test hook: the fitted lines [P, 2] the last assemble_observations[_device] of this process computed its end points from."""
        n = C.c_int64()
        f = self._hook("clc_debug_assemble_lines")
        check(f(None, C.c_int64(0), C.byref(n)), "clc_debug_assemble_lines")
        out = np.zeros((n.value, 2))
        check(f(out.ctypes.data_as(C.c_void_p), C.c_int64(n.value), C.byref(n)), "clc_debug_assemble_lines")
        return out

    # ---- test / profiling hooks ----
    def debug_math(self, op: int, x: np.ndarray) -> np.ndarray:
        """Device branch of a scalar helper, element-wise (hooks build): 0 rsqrt_pos, 1 rcp_pos, 2 rcp_pos_safe, 3 sqrt_pos, 4 rcp_ge1,
        5 rcp_ge1_weight, 6 log via frexp_pos + log_mant_exp."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        out = np.empty_like(x)
        f = self._hook("clc_debug_math")
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong]
        check(f(self._h, op, x.ctypes.data, out.ctypes.data, x.shape[0]), "clc_debug_math")
        return out

    def debug_wave_reduce(self, lanes: np.ndarray, reduce_mode: int) -> np.ndarray:
        lanes = np.ascontiguousarray(lanes, dtype=np.float64).reshape(64, 28)
        out = np.empty(28)
        check(self._hook("clc_debug_wave_reduce")(self._h, dptr(lanes), dptr(out), C.c_int(reduce_mode)), "clc_debug_wave_reduce")
        return out

    def _hook(self, name: str):
        f = getattr(self._L, name, None)
        if f is None:
            raise RuntimeError(f"{name} is a test hook: not in the product library — create the solver with library=\"hooks\" "
                               "(csrc/libclc_hip_hooks.so) or run with CLC_LIBRARY set to a hooks build")
        return f

    def path_info(self) -> "_capi.PathInfo":
        """clc_get_path_info: which layouts the last uploads built and how the cooperative path is doing."""
        pi = _capi.PathInfo()
        check(self._L.clc_get_path_info(self._h, C.byref(pi)), "clc_get_path_info")
        return pi

    def debug_rows(self):
        """Row layout report -> (rows_ok, n_rows, batched_rows_ok, batched_n_rows)."""
        pi = self.path_info()
        return bool(pi.rows_layout), pi.n_rows, bool(pi.batched_rows_layout), pi.batched_n_rows

    def rows_carry_z(self):
        """(single-problem rows, batched rows) carry z: some uploaded record has p.z != 0, so the rows are the 24-byte form
        (64 z after the 64 (x, y) pairs of every row, 14 moments per scan) instead of the 16-byte one."""
        pi = self.path_info()
        return pi.rows_layout == 2, pi.batched_rows_layout == 2

    def debug_resident(self):
        """Resident ("lane") layout report of the uploaded batch -> (built, lanes per problem, largest points per lane,
        j-rows in all); built = the batched solver keeps every problem on chip for its whole solve (clc_resident.hpp)."""
        pi = self.path_info()
        return bool(pi.batched_resident), pi.batched_lanes, pi.batched_points_per_lane, pi.batched_lane_rows

    def debug_resident_single(self):
        """Lane layout of the single-problem array -> (built, lanes, points per lane); built = clc_solve with the default
        flags runs the whole LM solve in ONE single-workgroup launch (problems of at most 512 x 22 points)."""
        pi = self.path_info()
        return bool(pi.single_resident), pi.single_lanes, pi.single_points_per_lane

    def debug_coop(self):
        """Cooperative whole-GPU solve of the single-problem array (csrc/clc_coop.hpp) -> (layout built, largest points per
        lane, solves run on it, launches that timed out, resting on this handle)."""
        pi = self.path_info()
        return bool(pi.coop_resident), pi.coop_points_per_lane, pi.coop_solves, pi.coop_timeouts, bool(pi.coop_resting)

    def debug_coop_control(self, drop_next: int = 0, reenable: bool = False):
        """Test hook: launch the next cooperative solve `drop_next` workgroups short (it must time out and fall back); clear the
        disabled state."""
        check(self._hook("clc_debug_coop_control")(self._h, C.c_int(drop_next), C.c_int(int(reenable))), "clc_debug_coop_control")

    def debug_coop_set_tag(self, tag: int):
        """Test hook: first pass tag of the next cooperative solve (32-bit; exercises the wrap)."""
        check(self._hook("clc_debug_coop_set_tag")(self._h, C.c_uint(tag)), "clc_debug_coop_set_tag")

    def debug_wave_split(self, grid: int):
        """Wave split table of the row layout for `grid` workgroups -> (split[grid * 8 + 1], first[n_rows])."""
        n_rows = self.debug_rows()[1]
        split = np.zeros(grid * 8 + 1, dtype=np.int32)
        first = np.zeros(max(n_rows, 1), dtype=np.int32)
        self._hook("clc_debug_wave_split").argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        check(self._hook("clc_debug_wave_split")(self._h, C.c_int(grid), split.ctypes.data, first.ctypes.data), "clc_debug_wave_split")
        return split, first[:n_rows]

    def time_steps(self, pose: np.ndarray, first: int, last: int) -> Tuple[float, int]:
        """Mean period [ms] of the step_kernel launches first..last of one default solve (HIP events on the handle's
        stream right before launch `first` and right after launch `last`) and the solve's number of passes."""
        ms = C.c_double()
        n = C.c_int()
        check(self._hook("clc_time_steps")(self._h, dptr(np.ascontiguousarray(pose, dtype=np.float64)), C.c_int(first), C.c_int(last),
                                     C.byref(ms), C.byref(n)), "clc_time_steps")
        return ms.value, n.value

    def time_batched_eval(self, poses: np.ndarray, reps: int = 20) -> float:
        """Mean duration [ms] of `reps` back-to-back batched_eval_kernel launches over all uploaded problems at `poses`."""
        ms = C.c_double()
        P = self.num_problems
        poses = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(P, 7))
        check(self._hook("clc_time_batched_eval")(self._h, dptr(poses), C.c_int(reps), C.byref(ms)), "clc_time_batched_eval")
        return ms.value

    def time_eval(self, pose: np.ndarray, reps: int = 20, with_loss: bool = True, loss_scale_factor: float = 0.05,
                  with_jacobian: bool = True) -> float:
        """Mean duration [ms] of `reps` back-to-back evaluation-kernel launches (HIP events on the
        handle's stream)."""
        ms = C.c_double()
        check(self._hook("clc_time_eval")(self._h, dptr(np.ascontiguousarray(pose, dtype=np.float64)), C.c_int(int(with_loss)),
                                    C.c_double(loss_scale_factor), C.c_int(int(with_jacobian)), C.c_int(reps), C.byref(ms)),
              "clc_time_eval")
        return ms.value
