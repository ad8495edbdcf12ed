"""Pure-Python restatement of the batched lane planner (res_plan_kernel in csrc/clc_resident.hpp, build_resident and its
caller emit_rows_and_lanes in csrc/abi_layouts.hip) for the tests of clc_solve_batched: what clc_get_path_info reports
after clc_upload_batched.  A test helper only — the package plans on the device.

  * scans: runs of records whose (n, d, scale) are bitwise equal (scan_flag_kernel), cut at every problem start
    (mark_problem_starts_kernel);
  * a problem's points per lane: the smallest c >= max(1, ceil(n_p / NL)) with sum_s ceil(c_s / c) <= NL, at most the
    form's capacity (PR + PL); a problem with more scans than lanes, or none such c, does not fit; an empty problem: 0;
  * forms: 256 lanes (capacity 42), then 512 (capacity 22) for the whole batch when some problem does not fit 256;
    straight to 512 under flag 8192; records with p.z != 0: only the 512-lane z form (capacity 22);
  * flag 4096 at upload, or no records at all: no lane layout;
  * the lane deal (res_build_kernel): scan s with c records takes Ls = ceil(c / ppl) lanes, lane i of them q + (i < r) records
    (q, r = divmod(c, Ls)) from record s0 + i q + min(i, r); the lanes past the total are idle (lane_cuts)."""
import numpy as np

FLAG_NO_RESIDENT = 4096
FLAG_RESIDENT_WG512 = 8192

CAP = {256: 23 + 19, 512: 4 + 18, "z": 10 + 12}   # PR + PL of the three instantiations (clc_abi_internal.hpp kResPR* / kResPL*)
GRP = {256: 3, 512: 2, "z": 2}                    # points per group of the kernel's point loop (clc_resident.hpp GRP)


def scan_lengths(records, offsets):
    """-> list over problems of the scan lengths (np.int64 arrays) the device planner sees."""
    rec = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, 8)
    off = np.asarray(offsets, dtype=np.int64)
    n = rec.shape[0]
    key = rec.view(np.uint64)[:, [0, 1, 2, 3, 7]]
    new = np.ones(n, dtype=bool)
    if n > 1:
        new[1:] = (key[1:] != key[:-1]).any(axis=1)
    starts_p = off[:-1][off[:-1] < n]
    new[starts_p] = True
    first = np.flatnonzero(new)
    out = []
    for p in range(len(off) - 1):
        r0, r1 = int(off[p]), int(off[p + 1])
        if r1 <= r0:
            out.append(np.zeros(0, dtype=np.int64))
            continue
        f = first[(first >= r0) & (first < r1)]
        out.append(np.diff(np.append(f, r1)).astype(np.int64))
    return out


def problem_ppl(lens, n_lanes, cap):
    """Points per lane of one problem (0: empty), or None when it does not fit."""
    lens = np.asarray(lens, dtype=np.int64)
    n_p = int(lens.sum())
    if n_p == 0:
        return 0
    if len(lens) > n_lanes:
        return None
    for c in range(max(1, -(-n_p // n_lanes)), cap + 1):
        if int(((lens + c - 1) // c).sum()) <= n_lanes:
            return c
    return None


def lane_cuts(lens, nl, ppl):
    """The lane deal of one problem at `ppl` points per lane on `nl` lanes, as res_build_kernel writes the lane descriptors:
    -> (scan [nl], first_record [nl], cnt [nl]) np.int64; an idle lane has scan -1, cnt 0 and first_record = the record count."""
    lens = np.asarray(lens, dtype=np.int64)
    scan = np.full(nl, -1, dtype=np.int64)
    first = np.full(nl, int(lens.sum()), dtype=np.int64)
    cnt = np.zeros(nl, dtype=np.int64)
    t, s0 = 0, 0
    for s, c in enumerate(lens):
        c = int(c)
        Ls = -(-c // ppl)
        q, r = divmod(c, Ls) if Ls else (0, 0)
        for i in range(Ls):
            assert t < nl, "the problem does not fit the workgroup at this many points per lane"
            scan[t], first[t], cnt[t] = s, s0 + i * q + min(i, r), q + (1 if i < r else 0)
            t += 1
        s0 += c
    return scan, first, cnt


class Plan:
    """What clc_get_path_info should say about the batched lane layout, plus the per-problem points per lane."""

    def __init__(self, lanes, with_z, ppl):
        self.lanes = lanes                      # 0 (no lane layout), 256 or 512
        self.with_z = with_z
        self.ppl = ppl                          # per problem (empty: 0); None without a layout
        self.resident = lanes != 0

    @property
    def form(self):
        """256, 512 or 'z' (None without a layout): which instantiation of resident_solve_kernel runs."""
        if not self.resident:
            return None
        return "z" if self.with_z else self.lanes

    @property
    def max_ppl(self):
        return max(self.ppl) if self.resident and self.ppl else 0

    @property
    def lane_rows(self):
        return sum(self.ppl) if self.resident else 0

    @property
    def uniform(self):
        return self.resident and all(c == self.ppl[0] for c in self.ppl)

    def path_info(self):
        """(batched_resident, batched_lanes, batched_points_per_lane, batched_lane_rows, batched_points_carry_z)"""
        return (int(self.resident), self.lanes, self.max_ppl, self.lane_rows, int(self.resident and self.with_z))


def plan_lens(lens_per_problem, flags=0, any_z=False):
    """The plan of a batch given its scan lengths per problem (as scan_lengths returns them)."""
    if (flags & FLAG_NO_RESIDENT) or sum(int(np.sum(l)) for l in lens_per_problem) == 0:
        return Plan(0, False, None)
    if any_z:
        tries = [(512, CAP["z"])]
    elif flags & FLAG_RESIDENT_WG512:
        tries = [(512, CAP[512])]
    else:
        tries = [(256, CAP[256]), (512, CAP[512])]
    for nl, cap in tries:
        ppl = [problem_ppl(l, nl, cap) for l in lens_per_problem]
        if all(c is not None for c in ppl):
            return Plan(nl, any_z, ppl)
    return Plan(0, False, None)


def plan(records, offsets, flags=0):
    """The plan of clc_upload_batched(records, offsets) under launch flags `flags` (0: the library's defaults)."""
    rec = np.asarray(records, dtype=np.float64).reshape(-1, 8)
    any_z = bool(np.any(rec[:, 6] != 0.0))
    return plan_lens(scan_lengths(rec, offsets), flags, any_z)
