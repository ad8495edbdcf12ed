"""The launch-path resolver (camlasercalibratool_amd/csrc/abi_paths.hpp, compiled for the host with g++ by tests/shim/paths_shim.cpp)
against the launchers' rules as they stood before it gathered them (tests/launch_paths_ref.py): for every flag value of
clc_set_launch (-1 and 0 .. 16383), sizes on both sides of every threshold, the layouts an upload may have built, profile_events,
the auto-path mask and the grid override, the plans pick the kernels, template arguments and grids the launchers picked."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import launch_paths_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "camlasercalibratool_amd", "csrc")
FLAGS = np.arange(-1, 16384, dtype=np.int32)
NF = len(FLAGS)
CACHE = R.CACHE
# observations: the single-workgroup capacity (512 x 22), the auto row cut, the cooperative capacity, both cache thresholds of the
# compact layout (28 B per observation), the step chain's int limit, and the 2-workgroups-per-CU grid of 256 CUs
N_OBS = sorted({0, 1, 127, 128, 129, 11264, 199999, 200000, 200001, 2_600_000, 32768 * 128, 32768 * 128 + 1,
                CACHE // 28, CACHE // 28 + 1, (CACHE + CACHE // 2) // 28, (CACHE + CACHE // 2) // 28 + 1, 0x7FFFFFFE, 0x7FFFFFFF})
# rows: the equal-shares cut (16 x 8 rows per workgroup of a 256-workgroup grid), the 1.5x-cache threshold of rows with and without z
N_ROWS = sorted({0, 1, 16 * 8 * 256, 16 * 8 * 256 + 1, (CACHE + CACHE // 2) // 1088, (CACHE + CACHE // 2) // 1088 + 1,
                 (CACHE + CACHE // 2) // 1600, (CACHE + CACHE // 2) // 1600 + 1})


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(HERE, "shim", "paths_shim.cpp")
    out = os.path.join(HERE, "shim", "libpaths_shim.so")
    deps = [src] + [os.path.join(CSRC, f) for f in ("abi_paths.hpp", "clc_rows.hpp", "clc_math.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", out])
    L = C.CDLL(out)
    ull, ll = C.c_ulonglong, C.c_longlong
    L.shim_plan_stream.argtypes = [C.c_void_p, C.c_long, C.c_int, ull, ll, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.shim_plan_solve.argtypes = [C.c_void_p, C.c_long, C.c_int, ull, ll, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_int] * 5 + [C.c_void_p]
    L.shim_plan_batched.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.shim_plan_upload.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p]
    return L


def _table(fn, width, *args, dtype=np.int32):
    out = np.empty((NF, width), dtype=dtype)
    fn(FLAGS.ctypes.data, NF, *args, out.ctypes.data)
    return out


def _same(got, want, case, name, mask=None):
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    bad = got != want if mask is None else (got != want) & mask
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        pytest.fail(f"{name}: flags {int(FLAGS[i])} {case}: plan {got[i]}, launchers {want[i]} ({int(bad.sum())} flag values differ)")


def test_stream_plan(shim):
    n = 0
    for go, ncu, n_obs, n_rows, rows_ok, rows_z, compact_ok in itertools.product((0, 1, 300), (256, 80), N_OBS, N_ROWS, (0, 1), (0, 1),
                                                                                     (0, 1)):
        if rows_z and not rows_ok:
            continue
        case = dict(go=go, ncu=ncu, n_obs=n_obs, n_rows=n_rows, rows_ok=rows_ok, rows_z=rows_z, compact_ok=compact_ok)
        t = _table(shim.shim_plan_stream, 8, go, n_obs, n_rows, rows_ok, rows_z, compact_ok, ncu)
        r = R.stream(FLAGS, go, n_obs, n_rows, rows_ok, rows_z, compact_ok, ncu)
        layout, rows = t[:, 0], t[:, 0] >= R.ROWS
        _same(layout, r["layout"], case, "layout")
        _same(t[:, 1], r["threads"], case, "threads")
        _same(t[:, 2], r["grid"], case, "grid")
        _same(t[:, 3], r["pf"], case, "prefetch", mask=~rows)
        _same(t[:, 4], r["nt"], case, "nt")
        _same(np.where(rows, t[:, 4], t[:, 5]), r["step_nt"], case, "step chain nt")
        _same(t[:, 6], r["eval_eq"], case, "eval_equal")
        _same(t[:, 7], r["step_eq"], case, "step_equal")
        n += 1
    assert n > 1000


def test_solve_plan(shim):
    sizes = [(5_000, 80), (150_000, 2_400), (250_000, 4_000), (0x7FFFFFFF, 1 << 25)]
    for (n_obs, n_rows), go, layouts, sres_ok, cres_ok, soc, ad, pe in itertools.product(
            sizes, (0, 7), itertools.product((0, 1), (0, 1)), (0, 1), (0, 1), (0, 1), (0, 1, 2, 3, 8, 11), (0, 1, 2)):
        rows_ok, compact_ok = layouts
        case = dict(n_obs=n_obs, go=go, rows_ok=rows_ok, compact_ok=compact_ok, sres=sres_ok, cres=cres_ok, soc=soc, ad=ad, pe=pe)
        t = _table(shim.shim_plan_solve, 3, go, n_obs, n_rows, rows_ok, 0, compact_ok, 256, sres_ok, cres_ok, soc, ad, pe)
        r = R.solve(FLAGS, go, n_obs, n_rows, rows_ok, 0, compact_ok, 256, sres_ok, cres_ok, soc, ad, pe)
        single, coop, step = t[:, 0] != 0, t[:, 1] != 0, t[:, 2] != 0
        # clc_solve: `if (single && !coop)` the single-workgroup solve; `if (coop && ++eligible > retry_at)` the cooperative one;
        # `if (single)`; the step chain; the launch pair
        _same(coop & ~(single & ~coop), r["tries_coop"], case, "cooperative tried")
        _same(single, r["single"], case, "single-workgroup")
        _same(step, r["step"], case, "step chain")


def test_batched_plan(shim):
    ctile = R.CTILE_DOUBLES * 8
    tiles = ((1, 1), (80, 10), (CACHE // ctile, 300), (CACHE // ctile + 1, 300), ((CACHE + CACHE // 2) // ctile + 1, 20000))
    rows = (0, 1 << 20, (CACHE + CACHE // 2) // 1088 + 1, (1 << 30) // 1088, (1 << 30) // 1088 + 1)
    res = ((0, 0, 0, 0), (1, 0, 42, 256), (1, 1, 22, 512), (1, 0, 98304, 256), (1, 0, 98305, 256))  # (the last: past 1.5x the cache)
    # 25 shapes, a Latin square over (tiles, rows, lane layout)
    shapes = [(tiles[i % 5], rows[i // 5], (1024, 1025)[(i + i // 5) % 2], res[(i + i // 5) % 5]) for i in range(25)]
    for go, ncu, P, lay, shape in itertools.product((0, 5, 5000), (256, 80), (1, 4, 24, 1024, 2048, 8192, 8193),
                                                    ((0, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 0)), shapes):
        (total_tiles, max_tiles), n_rows, max_rows, (res_ok, res_z, res_rows, res_lanes) = shape
        compact_ok, rows_ok, rows_z = lay
        case = dict(go=go, ncu=ncu, P=P, lay=lay, shape=shape)
        b = np.array([P, total_tiles, max_tiles, n_rows, max_rows, compact_ok, rows_ok, rows_z, res_ok, res_z, res_rows, res_lanes],
                     dtype=np.int64)
        out = np.empty((NF, 14), dtype=np.int64)
        shim.shim_plan_batched(FLAGS.ctypes.data, NF, go, ncu, b.ctypes.data, out.ctypes.data)
        r = R.batched(FLAGS, go, ncu, P, total_tiles, max_tiles, n_rows, max_rows, compact_ok, rows_ok, rows_z, res_ok, res_z, res_rows,
                      res_lanes)
        for k, name in enumerate(R.BATCHED_FIELDS):
            _same(out[:, k], r[name], case, name)


def test_upload_plan(shim):
    for ad, batch in itertools.product(range(12), (0, 1)):
        t = _table(shim.shim_plan_upload, 3, ad, batch)
        r = R.upload(FLAGS, ad, bool(batch))
        for k, name in enumerate(("resident", "first_lanes", "one_hop")):
            _same(t[:, k], r[name], dict(ad=ad, batch=batch), name)


def test_flow_blocks_per_problem():
    """The restatement of abi_batchflow.hip's flow_blocks_per_problem that tests/batched_flow_cases.py plans its batches with: values
    worked out by hand from the rule (four workgroups per CU over the batch, at least eight units per workgroup, at least one)."""
    f = R.flow_blocks_per_problem
    for b in (1, 7, 8, 9, 15, 16, 17):                      # a few problems on 256 CUs: the longest problem's units decide
        assert f(256, 4, 8 * b) == b and f(256, 4, 8 * b + 7) == b
    assert f(256, 5, 63) == 7 and f(256, 3, 127) == 15 and f(256, 3, 7) == 1 and f(256, 3, 0) == 1
    assert f(256, 1, 10**6 // 64) == 1024 and f(256, 1024, 10**6) == 1      # the batch size decides
    assert f(256, 512, 24) == 2 and f(256, 513, 24) == 2 and f(256, 1023, 24) == 2 and f(256, 1024, 24) == 1 and f(256, 511, 24) == 3
    assert f(80, 160, 24) == 2 and f(80, 320, 24) == 1 and f(0, 3, 800) == 2
