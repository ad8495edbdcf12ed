"""Pure-Python restatement of which kernels the launchers pick (csrc/abi_solve.hip launch_eval / solve_stepped / clc_solve,
abi_frontend.hip clc_closed_form, abi_batched.hip batched_launch_setup, abi_layouts.hip's upload choices), written from the
launchers as they stood before csrc/abi_paths.hpp gathered the rules, for tests/test_launch_paths.py (and, flow_blocks_per_problem,
abi_batchflow.hip's workgroups per problem, for tests/batched_flow_cases.py).  Every other function takes
`flags` as an np.int64 array (each -1 .. 16383, clc_set_launch) and evaluates all of them at once; the other inputs are scalars.

  * flags = -1: the defaults (2|16|32|128|256|512), and the size-dependent choices ("auto");
  * the Infinity Cache is 256 MiB: beyond it (auto) the compact layout gets the deep pipeline; beyond 1.5x (auto) streamed loads
    are non-temporal; the compact layout counts 28 B per observation, rows 64 B of descriptor + 128 (z: 192) doubles each;
  * auto keeps arrays below 2x10^5 observations on the compact layout when it exists."""
import numpy as np

FLAG_PREFETCH, FLAG_NONTEMPORAL, FLAG_COMPACT, FLAG_WG512, FLAG_DEEP = 2, 4, 16, 32, 64
FLAG_STEP, FLAG_ROWS, FLAG_EQUAL_WAVES, FLAG_BATCHED_WG256, FLAG_BATCHED_LOCKSTEP = 128, 256, 512, 1024, 2048
FLAG_NO_RESIDENT, FLAG_RESIDENT_WG512 = 4096, 8192
DEFAULT_FLAGS = 2 | 16 | 32 | 128 | 256 | 512
CACHE = 256 << 20
TILE, BLOCK, CTILE_DOUBLES, ROW_DOUBLES, ROW_DOUBLES_Z, ROWDESC_BYTES = 128, 256, 448, 128, 192, 64
TILES, COMPACT, ROWS, ROWS_Z = 0, 1, 2, 3


def _decode(flags):
    flags = np.asarray(flags, dtype=np.int64)
    auto = flags < 0
    fl = np.where(auto, DEFAULT_FLAGS, flags)
    return auto, (lambda b: (fl & b) != 0)


def _row_bytes(n_rows, z):
    return n_rows * ((ROW_DOUBLES_Z if z else ROW_DOUBLES) * 8 + ROWDESC_BYTES)


def _rows_nontemporal(auto, bit, n_rows, z):
    return bit(FLAG_NONTEMPORAL) | (auto & (_row_bytes(n_rows, z) > CACHE + CACHE // 2))


def _use_rows(auto, bit, n_obs, rows_ok, compact_ok):
    return bit(FLAG_ROWS) & bool(rows_ok) & (~auto | (not compact_ok) | (n_obs >= 200000))


def _eval_grid(bit, grid_override, n, num_cus):
    tiles = (n + TILE - 1) // TILE
    big = bit(FLAG_WG512)
    per_cu = np.where(~big & (tiles >= 16 * (BLOCK // 64) * 2 * num_cus), 2, 1)
    cap = grid_override if grid_override > 0 else per_cu * num_cus
    return np.minimum(max(tiles, 1), cap) * np.ones_like(per_cu)


def stream(flags, grid_override, n_obs, n_rows, rows_ok, rows_z, compact_ok, num_cus):
    """-> dict of arrays: what clc_eval (K1), the step chain and clc_closed_form launch.
    layout (TILES / COMPACT / ROWS / ROWS_Z), threads and grid of K1, pf (K1's PF template argument; -1 on rows), nt (K1's NT;
    the closed form's and the step chain's on rows), step_nt (the step chain's NT), eval_eq (K1's EQ on rows), step_eq (the step
    chain's EQ on rows; the wave split table is built where eval_eq / step_eq hold)."""
    auto, bit = _decode(flags)
    rows = _use_rows(auto, bit, n_obs, rows_ok, compact_ok)
    cp = bit(FLAG_COMPACT) & bool(compact_ok)
    big = bit(FLAG_WG512)
    grid = _eval_grid(bit, grid_override, n_obs, num_cus)
    rnt = _rows_nontemporal(auto, bit, n_rows, rows_z)
    deep = bit(FLAG_DEEP) | (auto & (n_obs * 28 > CACHE))
    cnt = bit(FLAG_NONTEMPORAL) | (auto & (n_obs * 28 > CACHE + CACHE // 2))
    eq = bit(FLAG_EQUAL_WAVES) & ~(auto & (n_rows > 16 * 8 * grid))
    layout = np.where(rows, ROWS_Z if rows_z else ROWS, np.where(cp, COMPACT, TILES))
    pf = np.where(rows, -1, np.where(cp, deep, big | bit(FLAG_PREFETCH))).astype(np.int64)
    nt = np.where(rows, rnt, np.where(cp, cnt, bit(FLAG_NONTEMPORAL)))
    rows_eq = bit(FLAG_EQUAL_WAVES) & (not rows_z)
    return {"layout": layout, "threads": np.where(big, 512, 256), "grid": grid, "pf": pf, "nt": nt,
            "step_nt": np.where(rows, rnt, deep), "eval_eq": rows & (not rows_z) & big & eq, "step_eq": rows & rows_eq}


def solve(flags, grid_override, n_obs, n_rows, rows_ok, rows_z, compact_ok, num_cus, sres_ok, cres_ok, small_on_coop, auto_disable,
          profile_events):
    """-> dict of arrays, what clc_solve does: tries_coop (the back-off count is taken and, where it allows, the cooperative solve
    made), single (the single-workgroup solve runs where the cooperative one is not tried, rests or times out), step (otherwise the
    step chain rather than the [eval, lm] launch pair)."""
    auto, bit = _decode(flags)
    go0 = grid_override == 0
    single_ok = bool(sres_ok) & auto & ((auto_disable & 2) == 0) & go0 & (profile_events != 1)
    single_first = single_ok & (not (cres_ok and small_on_coop))
    coop_gate = bool(cres_ok) & auto & ((auto_disable & 1) == 0) & go0 & (profile_events != 1)
    rows = _use_rows(auto, bit, n_obs, rows_ok, compact_ok)
    step = (bit(FLAG_STEP) & ((bit(FLAG_COMPACT) & bool(compact_ok)) | rows) & bit(FLAG_WG512) & (n_obs < 0x7FFFFFFF)
            & (profile_events != 1))
    return {"tries_coop": ~single_first & coop_gate, "single": single_ok, "step": step * np.ones_like(auto)}


BATCHED_FIELDS = ["bpp", "n_blocks", "lm_threads", "lm_blocks", "compact", "deep", "nt", "rows", "rows_nt", "rows_wave", "one_wave",
                  "whole_solve", "resident", "res_nt"]


def batched(flags, grid_override, num_cus, problems, total_tiles, max_tiles, n_rows, max_rows, compact_ok, rows_ok, rows_z, res_ok,
            res_z, res_rows, res_lanes):
    """-> dict of arrays: the BatchedLaunch fields of batched_launch_setup."""
    auto, bit = _decode(flags)
    P = problems
    rows = bit(FLAG_ROWS) & bool(rows_ok)
    rows_wave = rows & ~bit(FLAG_BATCHED_WG256) & (~auto | (P >= 8 * num_cus))
    target = grid_override if grid_override > 0 else 4 * num_cus
    bpp = (target + P - 1) // P
    bpp = max(1, min(bpp, max(1, max_tiles // 4)))
    bpp = min(bpp, 16)
    one_wave = rows_wave & (bpp == 1) & (P >= 32 * num_cus)
    bpp = np.where(rows_wave & ~one_wave, bpp * (BLOCK // 64), bpp)
    compact = bit(FLAG_COMPACT) & bool(compact_ok)
    cbytes = total_tiles * CTILE_DOUBLES * 8
    nt = bit(FLAG_NONTEMPORAL) | (compact & auto & (cbytes > CACHE + CACHE // 2))
    deep = bit(FLAG_DEEP) | (auto & (cbytes > CACHE))
    rows_nt = rows & _rows_nontemporal(auto, bit, n_rows, rows_z)
    whole = rows & (not rows_z) & ~bit(FLAG_BATCHED_LOCKSTEP) & (_row_bytes(n_rows, rows_z) <= (1 << 30)) & (max_rows <= 1024)
    resident = bool(res_ok) & ((np.where(auto, DEFAULT_FLAGS, flags) & (FLAG_NO_RESIDENT | FLAG_BATCHED_LOCKSTEP)) == 0)
    res_bytes = res_rows * res_lanes * (3 if res_z else 2) * 8
    res_nt = bit(FLAG_NONTEMPORAL) | (auto & (res_bytes > CACHE + CACHE // 2))
    one = np.ones_like(auto, dtype=np.int64)
    return {"bpp": bpp * one, "n_blocks": P * bpp * one, "lm_threads": 64 * one, "lm_blocks": (P + 63) // 64 * one, "compact": compact,
            "deep": deep, "nt": nt, "rows": rows, "rows_nt": rows_nt, "rows_wave": rows_wave, "one_wave": one_wave, "whole_solve": whole,
            "resident": resident, "res_nt": res_nt}


def flow_blocks_per_problem(num_cus, problems, units):
    """Workgroups per problem of clc_closed_form_batched / clc_information_batched (abi_batchflow.hip flow_blocks_per_problem): four
    workgroups per CU over the whole batch, never fewer than eight streaming units per workgroup.  units: the longest problem's rows
    (row layout: batch_max_rows) or 128-point tiles (tile layout: batch_max_tiles).  Neither the flags nor the grid override enter."""
    want = 4 * max(1, int(num_cus))
    bpp = (want + int(problems) - 1) // int(problems)
    return max(1, min(bpp, max(1, int(units) // 8)))


def upload(flags, auto_disable, batch):
    """-> dict of arrays: resident (lane layouts built at all), first_lanes (the lane count tried first), one_hop (the cooperative
    layout's 32-workgroup form may be tried)."""
    auto, bit = _decode(flags)
    one = np.ones_like(auto)
    return {"resident": ~bit(FLAG_NO_RESIDENT), "first_lanes": np.where((not batch) | bit(FLAG_RESIDENT_WG512), 512, 256),
            "one_hop": ((auto_disable & 8) == 0) & one}
