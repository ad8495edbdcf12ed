"""Edge and shape fuzz of the kernels in front of the solve (csrc/clc_frontend.hpp) against the oracle and the high-precision references of
tests/test_scan_frontend_host.py, which also holds the input generators and shows that the oracle alone meets the gates on them.

  * line_fit_kernel (four scans per wave, a 16-lane DPP row each): parity with oracle.line_fit on every scan of every kind, loss on and
    off, at batch sizes that give every count of live rows in the last wave; bitwise independence of a scan from its neighbours, its
    position and its batch; base offsets in both forms; a NaN point in one scan of a wave; options and refused inputs.
    Gates (those of test_gpu_parity.py): equal termination and num_iterations, line within 1e-9 max(1, |line|), final cost within 1e-12.
  * scan_to_points_kernel / scan_to_points_flat_kernel: ragged and empty scans, the grid-stride loop, the range edges, theta beyond
    2 pi; x, y within 5 * 2^-53 * r of the extended-precision restatement (OpenCL's 4 ulp for fp64 sin / cos, which the device library
    follows, plus the product's rounding).  Measured on the MI355X: kernel 1.598e-16 of r (1.44 x 2^-53); oracle the same 1.598e-16.
  * K5 (normal9_kernel, normal9_rows_kernel at both strides, reduce9_kernel): n on the tile, row and partial-row edges under forced
    grids of 1, 2, 3, 7 and the default, on every layout, against the exact sums.  Gate: 8 x the oracle's own worst distance from the
    exact reference over the same case list, floored at 64 * 2^-53.  Measured on the MI355X, relative to sv9[0] / max|Tlc|: kernel sv9
    1.84e-15, Tlc 6.03e-13; oracle sv9 3.34e-14, Tlc 4.27e-12 (gates 2.67e-13 and 3.42e-11); 8 row and 5 row-z layouts built.
    The `k0 + 1 < n` guard of normal9_kernel cannot be observed through results: retile_kernel zero-fills a tile's padding, and a zero
    record adds nothing to any of the 45 sums — the guard is a second line of defence, not what keeps the sums right.
  * line fit parity measured on the MI355X: 13 211 scans, worst line 1.33e-11, worst cost 3.02e-14; module 3 s.
  * one chain on device pointers only: ranges -> points -> board segments -> line fit, bit for bit the host chain."""
import ctypes as C
import time

import numpy as np
import pytest

import camlasercalibratool_amd as clc
import test_scan_frontend_host as H
from camlasercalibratool_amd import _capi

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 3, 4, 5, 31, 32, 33, 63, 1027)
SPENT = [0.0]


@pytest.fixture(scope="module")
def sv():
    s = clc.Solver(0)
    yield s
    s.close()
    print(f"scan front end: {SPENT[0]:.1f} s in the tests of this module")
    assert SPENT[0] < 60.0, SPENT[0]


@pytest.fixture(autouse=True)
def _clock():
    t = time.perf_counter()
    yield
    SPENT[0] += time.perf_counter() - t


def _sm(s):
    """A summary as comparable bits, solve_ms excluded."""
    return (s.termination, s.num_iterations, s.num_successful_steps, s.num_unsuccessful_steps, s.num_evaluations,
            float(s.initial_cost).hex(), float(s.final_cost).hex(), float(s.eval_kernel_ms).hex(), s.eval_kernel_launches)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _options(use_loss=1, max_it=None, a=None):
    o = H.line_options(clc, use_loss, max_it)
    if a is not None:
        o.loss_scale_factor = a
    return o


def _check_parity(oracle_mod, xy, off, l0, lines, sms, tag, use_loss=1, loss_a=0.05, max_it=None):
    refs = H.oracle_line_fits(oracle_mod, xy, off, l0, use_loss, loss_a, max_it)
    worst_l, worst_c = 0.0, 0.0
    for k, ref in enumerate(refs):
        t = tag + (k, int(off[k + 1] - off[k]))
        assert sms[k].termination == ref.summary.termination, t
        assert sms[k].num_iterations == ref.summary.num_iterations, t
        dl = np.abs(lines[k] - ref.pose).max() / max(1.0, np.abs(ref.pose).max())
        dc = abs(sms[k].final_cost - ref.summary.final_cost)
        assert dl <= 1e-9, t + (dl,)
        assert dc <= 1e-12, t + (dc,)
        worst_l, worst_c = max(worst_l, dl), max(worst_c, dc)
    return worst_l, worst_c


def _mixed(seed, per_kind):
    """A batch of mixed kinds -> xy, off, lines0."""
    parts = [H.fuzz_scans(seed + i, per_kind[i], kind) for i, kind in enumerate(H.ALL_KINDS) if per_kind[i]]
    xy = np.concatenate([p[0] for p in parts])
    lens = np.concatenate([np.diff(p[1]) for p in parts])
    off = np.zeros(lens.size + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    return xy, off, np.concatenate([p[2] for p in parts])


def _take(xy, off, l0, order):
    lens = np.diff(off)[order]
    o2 = np.zeros(len(order) + 1, dtype=np.int64)
    o2[1:] = np.cumsum(lens)
    x2 = np.concatenate([xy[off[k]:off[k + 1]] for k in order]).reshape(-1, 2)
    return x2, o2, l0[order]


def _device_line_fit(sv, xy, off, l0, options=None, summaries=True):
    import torch
    dev = torch.device("cuda:0")
    S = len(off) - 1
    d_xy = torch.from_numpy(np.ascontiguousarray(xy)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(off)).to(dev)
    d_l = torch.from_numpy(np.ascontiguousarray(l0).copy()).to(dev)
    d_sm = torch.zeros(S * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sv.line_fit_batched_device(d_xy.data_ptr(), d_off.data_ptr(), S, d_l.data_ptr(), d_sm.data_ptr() if summaries else 0, options)
    sms = (_capi.Summary * S).from_buffer_copy(d_sm.cpu().numpy().tobytes()) if summaries else None
    return d_l.cpu().numpy(), sms


# ---- line fit ----------------------------------------------------------------------------------------------------------------------
def test_line_fit_parity_fuzz_every_kind_and_last_wave_shape(sv, oracle_mod):
    """12 000 scans and more: six kinds (sentinel_skew with the loss only) x loss on / off x ten batch sizes, every scan checked."""
    t0 = time.perf_counter()
    total, worst = 0, (0.0, 0.0)
    for ki, kind in enumerate(H.ALL_KINDS):
        for use_loss in ((1,) if kind == "sentinel_skew" else (1, 0)):
            for S in BATCHES:
                xy, off, l0, _ = H.fuzz_scans(1000 * ki + S, S, kind)
                lines, sms = sv.line_fit_batched(xy, off, l0, _options(use_loss))
                w = _check_parity(oracle_mod, xy, off, l0, lines, sms, (kind, use_loss, S), use_loss)
                worst = (max(worst[0], w[0]), max(worst[1], w[1]))
                total += S
    print(f"line fit parity: {total} scans, worst line {worst[0]:.2e}, worst cost {worst[1]:.2e}, {time.perf_counter() - t0:.1f} s")
    assert total >= 4000


def test_line_fit_scan_is_independent_of_neighbours_position_and_batch(sv):
    """257 scans of mixed kinds as given, in a seeded random order, and 40 of them alone: line and summary bitwise the same.  A DPP
    read that leaks between the four rows of a wave, or any use of the wave / block index, shows here."""
    xy, off, l0 = _mixed(7, (60, 60, 17, 40, 40, 40))
    S = len(off) - 1
    assert S == 257
    lines, sms = sv.line_fit_batched(xy, off, l0)
    rng = np.random.default_rng(123)
    order = rng.permutation(S)
    x2, o2, l2 = _take(xy, off, l0, order)
    lines2, sms2 = sv.line_fit_batched(x2, o2, l2)
    for j, k in enumerate(order):
        assert np.array_equal(_bits(lines2[j]), _bits(lines[k])) and _sm(sms2[j]) == _sm(sms[k]), (j, k)
    for k in rng.choice(S, 40, replace=False):
        x1, o1, l1 = _take(xy, off, l0, [k])
        la, sa = sv.line_fit_batched(x1, o1, l1)
        assert np.array_equal(_bits(la[0]), _bits(lines[k])) and _sm(sa[0]) == _sm(sms[k]), k


def test_line_fit_base_offsets_host_and_device(sv):
    xy, off, l0 = _mixed(11, (20, 9, 3, 5, 5, 5))
    S = len(off) - 1
    lines, sms = sv.line_fit_batched(xy, off, l0)
    pad = np.full((1000, 2), 123.0)
    tail = np.full((7, 2), -5.0)
    big = np.concatenate([pad, xy, tail])
    lb, sb = sv.line_fit_batched(big, off + 1000, l0)  # host form: offsets[0] = 1000 into a longer xy
    assert np.array_equal(_bits(lb), _bits(lines)) and [_sm(s) for s in sb] == [_sm(s) for s in sms]
    ld, sd_ = _device_line_fit(sv, big, off + 1000, l0)  # device form: absolute offsets with a base
    assert np.array_equal(_bits(ld), _bits(lines)) and [_sm(s) for s in sd_] == [_sm(s) for s in sms]
    ln, _ = _device_line_fit(sv, big, off + 1000, l0, summaries=False)  # summaries NULL
    assert np.array_equal(_bits(ln), _bits(lines))
    l0_, s0_ = _device_line_fit(sv, xy, off, l0)
    assert np.array_equal(_bits(l0_), _bits(lines)) and [_sm(s) for s in s0_] == [_sm(s) for s in sms]
    assert S == 47


def test_line_fit_nan_point_in_one_scan_of_a_wave(sv, oracle_mod):
    """A non-finite cost at iteration 0 is Ceres' FAILURE with the line left as it was (include/clc.h); the three other scans of the
    wave return the bits they return without it."""
    xy, off, l0, _ = H.fuzz_scans(31, 8, "start")
    clean, sm_clean = sv.line_fit_batched(xy, off, l0)
    for row in range(4):
        bad = xy.copy()
        k = 4 + row  # the second wave's row
        bad[off[k] + (off[k + 1] - off[k]) // 2, row % 2] = np.nan
        lines, sms = sv.line_fit_batched(bad, off, l0)
        for j in range(8):
            if j != k:
                assert np.array_equal(_bits(lines[j]), _bits(clean[j])) and _sm(sms[j]) == _sm(sm_clean[j]), (row, j)
        ref = oracle_mod.line_fit(bad[off[k]:off[k + 1]], l0[k], options=H.line_options(oracle_mod), linear_solver="qr")
        assert ref.summary.termination == 6 and np.array_equal(ref.pose, l0[k])  # FAILURE, line unchanged
        assert sms[k].termination == ref.summary.termination
        assert np.array_equal(_bits(lines[k]), _bits(ref.pose))


@pytest.mark.parametrize("case", ["max_it_0", "max_it_1", "loss_a_0.5", "sentinel_no_loss"])
def test_line_fit_options_against_the_oracle(sv, oracle_mod, case):
    S = 67
    if case.startswith("max_it"):
        m = int(case[-1])
        for kind in ("mid", "start", "short"):
            xy, off, l0, _ = H.fuzz_scans(41, S, kind)
            lines, sms = sv.line_fit_batched(xy, off, l0, _options(1, m))
            _check_parity(oracle_mod, xy, off, l0, lines, sms, (case, kind), 1, 0.05, m)
            assert max(s.num_iterations for s in sms) <= m
            if m == 0:
                assert np.array_equal(lines, l0)
    elif case == "loss_a_0.5":
        for kind in ("mid", "start"):
            xy, off, l0, _ = H.fuzz_scans(42, S, kind)
            lines, sms = sv.line_fit_batched(xy, off, l0, _options(1, None, 0.5))
            _check_parity(oracle_mod, xy, off, l0, lines, sms, (case, kind), 1, 0.5)
            base, _ = sv.line_fit_batched(xy, off, l0)
            assert not np.array_equal(lines, base)  # the factor is used
    else:
        xy, off, l0, _ = H.fuzz_scans(43, S, "sentinel")
        lines, sms = sv.line_fit_batched(xy, off, l0, _options(0))
        _check_parity(oracle_mod, xy, off, l0, lines, sms, (case,), 0)


def test_line_fit_refused_inputs(sv):
    xy, off, l0, _ = H.fuzz_scans(51, 6, "mid")
    for a in (0.0, -0.05, float("nan")):
        with pytest.raises(clc.ClcError) as e:
            sv.line_fit_batched(xy, off, l0, _options(1, None, a))
        assert e.value.code == -1  # CLC_ERR_INVALID_ARG
    sv.line_fit_batched(xy, off, l0, _options(0, None, 0.0))  # without the loss the factor is not read
    with pytest.raises(clc.ClcError) as e:
        sv.line_fit_batched(xy, off, l0, _options(1, -1))
    assert e.value.code == -1
    bad = l0.copy()
    bad[3, 1] = np.nan
    with pytest.raises(clc.ClcError) as e:
        sv.line_fit_batched(xy, off, bad)
    assert e.value.code == -3  # CLC_ERR_NONFINITE
    o2 = off.copy()
    o2[3] = o2[2] - 1
    with pytest.raises(clc.ClcError) as e:
        sv.line_fit_batched(xy, o2, l0)
    assert e.value.code == -1
    lines, sms = sv.line_fit_batched(xy, off, l0)  # and the handle still works
    assert all(s.termination in (1, 2, 3, 4, 5) for s in sms)


# ---- scan conversion ---------------------------------------------------------------------------------------------------------------
def _device_scan_to_points(sv, c):
    import torch
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    S, n = len(c["offsets"]) - 1, int(c["offsets"][-1])
    d = [t(c[k]) for k in ("ranges", "offsets", "angle_min", "angle_increment", "range_min")]
    d_p = torch.full((n, 3), -7.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    sv.scan_to_points_device(d[0].data_ptr(), d[1].data_ptr(), S, n, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d_p.data_ptr())
    return d_p.cpu().numpy()


def test_scan_to_points_case_list_both_forms(sv, oracle_mod):
    c = H.scan_cases()
    off = c["offsets"]
    host = sv.scan_to_points(c["ranges"], off, c["angle_min"], c["angle_increment"], c["range_min"])
    devp = _device_scan_to_points(sv, c)
    assert np.array_equal(_bits(host), _bits(devp))  # the 2-D kernel and the flat kernel, bit for bit
    ref = np.concatenate([oracle_mod.scan_to_points(c["ranges"][off[k]:off[k + 1]], c["angle_min"][k], c["angle_increment"][k], c["range_min"][k])
                          for k in range(len(off) - 1)])
    assert np.array_equal(host == 1000.0, ref == 1000.0)
    assert np.array_equal(_bits(host[:, 2]), _bits(ref[:, 2])) and not host[:, 2].any()
    worst, mask = H.scan_error(host, c)
    worst_o, _ = H.scan_error(ref, c)
    print(f"scan_to_points vs extended precision: kernel {worst:.3e} of r ({worst * 2 ** 53:.2f} x 2^-53), oracle {worst_o:.3e} ({worst_o * 2 ** 53:.2f} x 2^-53)")
    assert np.array_equal((host[:, :2] == 1000.0).all(1), mask)
    assert np.isfinite(host).all()
    assert worst <= 5 * 2.0 ** -53
    assert mask.sum() > 100 and (~mask).sum() > 50000


def test_scan_to_points_arguments(sv):
    c = H.scan_cases()
    off = c["offsets"]
    want = sv.scan_to_points(c["ranges"], off, c["angle_min"], c["angle_increment"], c["range_min"])
    # a base offset in the host form: points[3 * offsets[0]:] is written, the rest is left alone
    base, n = 37, int(off[-1])
    r = np.concatenate([np.full(base, 5.0, dtype=np.float32), c["ranges"], np.full(11, 5.0, dtype=np.float32)])
    pts = np.full((base + n + 11, 3), -7.0)
    o2 = np.ascontiguousarray(off + base)
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    rc = sv._L.clc_scan_to_points(sv._h, fp(r), o2.ctypes.data_as(C.POINTER(C.c_int64)), C.c_size_t(len(off) - 1), fp(c["angle_min"]),
                                  fp(c["angle_increment"]), fp(c["range_min"]), pts.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
    assert np.array_equal(_bits(pts[base:base + n]), _bits(want)) and (pts[:base] == -7.0).all() and (pts[base + n:] == -7.0).all()
    # 65 535 scans of one ray are accepted, 65 536 refused; no scans: nothing to do
    for S, ok in ((65535, True), (65536, False)):
        rr = np.full(S, 2.0, dtype=np.float32)
        oo = np.arange(S + 1, dtype=np.int64)
        am = np.linspace(-3.0, 3.0, S).astype(np.float32)
        if ok:
            p = sv.scan_to_points(rr, oo, am, np.float32(0.01), np.float32(0.1))
            assert np.abs(p[:, 0] - 2.0 * np.cos(am.astype(np.float64))).max() <= 2e-15 and np.abs(p[:, 1] - 2.0 * np.sin(am.astype(np.float64))).max() <= 2e-15
        else:
            with pytest.raises(clc.ClcError) as e:
                sv.scan_to_points(rr, oo, am, np.float32(0.01), np.float32(0.1))
            assert e.value.code == -1
    assert sv.scan_to_points(np.zeros(0, dtype=np.float32), np.zeros(1, dtype=np.int64), 0.0, 0.0, 0.0).shape == (0, 3)


# ---- closed form (K5) --------------------------------------------------------------------------------------------------------------
TILES, ROWS = 2 | 32, 2 | 32 | 256
GRIDS = (0, 1, 2, 3, 7)


def test_closed_form_on_the_tile_row_and_grid_edges(sv, oracle_mod):
    """Every case x {tiles, rows (the z cases: the ROW_DOUBLES_Z stride), default} x grid {default, 1, 2, 3, 7}: `unobservable` as the
    oracle's; sv9 and Tlc within 8 x the oracle's own worst distance from the exact sums (floor 64 * 2^-53) of the exact reference;
    rank-deficient cases: sv9 and `unobservable` only.  Repeats are bitwise equal; layouts and grids agree to the same gate."""
    cases = H.closed_form_cases()
    o_sv, o_T, exact = H.oracle_closed_form_yardstick(oracle_mod, cases)
    floor = 64 * 2.0 ** -53
    g_sv, g_T = max(8 * o_sv, floor), max(8 * o_T, floor)
    k_sv, k_T, n_rows_z, n_rows = 0.0, 0.0, 0, 0
    try:
        for (label, rec, rd), ex in zip(cases, exact):
            with_z = bool(rec[:, 6].any())
            results = {}
            for flags in (TILES, ROWS, -1):
                sv.set_launch(0, flags)
                sv.upload(rec)
                pi = sv.path_info()
                if flags == ROWS and rec.shape[0] >= 4:  # (fewer than 4 records per scan: no streaming layouts are built)
                    assert pi.rows_layout == (2 if with_z else 1) and pi.n_rows >= (rec.shape[0] + 63) // 64, (label, pi.rows_layout)
                    n_rows_z += with_z
                    n_rows += not with_z
                if flags == -1 and rec.shape[0] >= 200000:
                    assert pi.rows_layout == 1, label  # the default route of a large array is the row layout
                for grid in GRIDS:
                    sv.set_launch(grid, flags)
                    T, un, s9 = sv.closed_form()
                    T2, un2, s92 = sv.closed_form()
                    tag = (label, flags, grid)
                    assert np.array_equal(_bits(T), _bits(T2)) and np.array_equal(_bits(s9), _bits(s92)) and un == un2, tag
                    assert un == ex[1], tag
                    dsv, dT = H.closed_form_distance(ex, T, un, s9, rd)
                    assert dsv <= g_sv, tag + (dsv, g_sv)
                    k_sv = max(k_sv, dsv)
                    if not rd:
                        assert dT <= g_T, tag + (dT, g_T)
                        k_T = max(k_T, dT)
                    results[(flags, grid)] = (T, s9)
            if not rd:  # layouts and grids against each other
                Ts = np.stack([r[0] for r in results.values()])
                ss = np.stack([r[1] for r in results.values()])
                assert np.ptp(Ts, axis=0).max() <= g_T * np.abs(ex[2]).max(), label
                assert np.ptp(ss, axis=0).max() <= g_sv * ex[0][0], label
    finally:
        sv.set_launch(0, -1)
    print(f"closed form vs exact sums: kernel sv9 {k_sv:.2e} Tlc {k_T:.2e}; oracle sv9 {o_sv:.2e} Tlc {o_T:.2e}; gates {g_sv:.2e} {g_T:.2e}; "
          f"{n_rows} row and {n_rows_z} row-z layouts")
    assert n_rows >= 5 and n_rows_z >= 4


# ---- chain -------------------------------------------------------------------------------------------------------------------------
def test_device_chain_ranges_to_fitted_lines(sv):
    """float32 ranges -> scan_to_points_device -> board_segments_device -> line_fit_batched_device on the segments, on device pointers
    only (the segments are gathered with torch on the device), against the same chain through the host forms: bit for bit."""
    import torch
    from camlasercalibratool_amd import simdata as sd
    rng = np.random.default_rng(9)
    lens = rng.integers(700, 1300, 33)
    parts = [sd.sim_laser_scans(900 + k, 1, n_rays=int(n)) for k, n in enumerate(lens)]
    S = 33
    off = np.zeros(S + 1, dtype=np.int64)
    off[1:] = np.cumsum(lens)
    c = dict(ranges=np.concatenate([p["ranges"] for p in parts]), offsets=off, angle_min=np.concatenate([p["angle_min"] for p in parts]),
             angle_increment=np.concatenate([p["angle_increment"] for p in parts]), range_min=np.concatenate([p["range_min"] for p in parts]))
    # host chain
    pts = sv.scan_to_points(c["ranges"], off, c["angle_min"], c["angle_increment"], c["range_min"])
    seg, st = sv.board_segments(pts, off)
    n_seg = np.where(seg[:, 0] >= 0, seg[:, 1] - seg[:, 0] + 1, 0)
    assert (st == 1).sum() >= 10
    loff = np.zeros(S + 1, dtype=np.int64)
    loff[1:] = np.cumsum(n_seg)
    xy = np.concatenate([pts[off[k] + seg[k, 0]:off[k] + seg[k, 1] + 1, :2] if n_seg[k] else np.zeros((0, 2)) for k in range(S)])
    lines, sms = sv.line_fit_batched(xy, loff, np.zeros((S, 2)))
    # device chain
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_r, d_off, d_am, d_ai, d_rm = (t(c[k]) for k in ("ranges", "offsets", "angle_min", "angle_increment", "range_min"))
    n = int(off[-1])
    d_pts = torch.empty((n, 3), dtype=torch.float64, device=dev)
    d_seg = torch.empty((S, 2), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    sv.scan_to_points_device(d_r.data_ptr(), d_off.data_ptr(), S, n, d_am.data_ptr(), d_ai.data_ptr(), d_rm.data_ptr(), d_pts.data_ptr())
    sv.board_segments_device(d_pts.data_ptr(), d_off.data_ptr(), S, d_seg.data_ptr(), 0)
    d_n = torch.where(d_seg[:, 0] >= 0, d_seg[:, 1] - d_seg[:, 0] + 1, torch.zeros_like(d_seg[:, 0]))
    d_loff = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    d_loff[1:] = torch.cumsum(d_n, 0)
    M = int(d_loff[-1].item())
    scan_of = torch.repeat_interleave(torch.arange(S, device=dev), d_n)
    idx = d_off[scan_of] + d_seg[scan_of, 0] + (torch.arange(M, device=dev) - d_loff[scan_of])
    d_xy = d_pts[idx, :2].contiguous()
    d_lines = torch.zeros((S, 2), dtype=torch.float64, device=dev)
    d_sm = torch.zeros(S * C.sizeof(_capi.Summary), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sv.line_fit_batched_device(d_xy.data_ptr(), d_loff.data_ptr(), S, d_lines.data_ptr(), d_sm.data_ptr())
    assert np.array_equal(d_seg.cpu().numpy(), seg) and np.array_equal(_bits(d_xy.cpu().numpy()), _bits(xy))
    assert np.array_equal(_bits(d_lines.cpu().numpy()), _bits(lines))
    dsm = (_capi.Summary * S).from_buffer_copy(d_sm.cpu().numpy().tobytes())
    assert [_sm(s) for s in dsm] == [_sm(s) for s in sms]
    assert sum(s.termination in (1, 2, 3) for s in sms) >= 10
