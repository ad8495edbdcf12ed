"""Resampling over poses (pure numpy; needs no GPU): weight rows for Solver.solve_subsets / clc_solve_subsets, the definition of a
weighted subset as a materialised problem, the covariance estimates that the resampled solutions give, and the selection rule of the
consensus calibration (consensus_select, on the block scores of Solver.score_blocks / clc_score_blocks).

A weight row holds one unsigned 8-bit multiplicity per block of records (one block per pose): subset k is the problem in which every
record of block b appears w[k, b] times.  Poses are [p(3), q(x, y, z, w)], as everywhere in this package; their differences are taken
in the 6-dimensional local coordinates of the reference's PoseLocalParameterization (pose_plus)."""
import numpy as np


def jackknife_weights(n_blocks: int) -> np.ndarray:
    """Leave-one-out: [P, P], row k leaves block k out."""
    return (1 - np.eye(int(n_blocks), dtype=np.uint8)).astype(np.uint8)


def bootstrap_weights(n_blocks: int, n_subsets: int, seed: int = 0) -> np.ndarray:
    """Bootstrap over blocks: [S, P], row k = the multiplicities of P draws with replacement (default_rng(seed))."""
    P, S = int(n_blocks), int(n_subsets)
    rng = np.random.default_rng(seed)
    w = np.zeros((S, P), dtype=np.int64)
    for k in range(S):
        w[k] = np.bincount(rng.integers(0, P, P), minlength=P)
    if w.size and w.max() > 255:
        raise ValueError("a multiplicity beyond 255 does not fit a weight")
    return w.astype(np.uint8)


def random_subset_weights(n_blocks: int, n_subsets: int, m: int, seed: int = 0) -> np.ndarray:
    """Random m-of-P subsets without replacement: [S, P] of 0 / 1 (default_rng(seed))."""
    P, S, m = int(n_blocks), int(n_subsets), int(m)
    if not 0 <= m <= P:
        raise ValueError("m must be in [0, n_blocks]")
    rng = np.random.default_rng(seed)
    w = np.zeros((S, P), dtype=np.uint8)
    for k in range(S):
        w[k, rng.choice(P, m, replace=False)] = 1
    return w


def as_weight_rows(w, n_blocks: int) -> np.ndarray:
    """Weight rows as clc_solve_subsets reads them: [S, n_blocks] uint8, C-contiguous.  Accepts [S, n_blocks] or one row [n_blocks] of
    integers, booleans or integral floats in 0..255.  ValueError for a value outside 0..255 (a cast to uint8 would wrap 256 to 0: a
    block silently left out), for a non-integral or non-finite float, for a non-numeric array and for any other shape."""
    B = int(n_blocks)
    a = np.asarray(w)
    if B < 1 or a.ndim not in (1, 2) or a.shape[-1] != B or a.size == 0:
        raise ValueError(f"weights: [S, {B}] or [{B}], got {a.shape}")
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if a.dtype.kind == "f":
        if not np.all(np.isfinite(a)) or np.any(a != np.floor(a)):
            raise ValueError("weights: whole numbers only (a weight is a multiplicity)")
    elif a.dtype.kind not in "iu":
        raise ValueError(f"weights: integers, got {a.dtype}")
    if np.any(a < 0) or np.any(a > 255):
        raise ValueError("weights: multiplicities in 0..255")
    return np.ascontiguousarray(a.reshape(-1, B), dtype=np.uint8)


def materialize(records: np.ndarray, block_offsets, w) -> np.ndarray:
    """The definition of a weighted subset: the records of block b, w[b] times in a row, block after block.  For the oracle, for
    clc_solve_batched, and for problems that one workgroup does not hold."""
    rec = np.asarray(records)
    off = np.asarray(block_offsets, dtype=np.int64).reshape(-1)
    w = np.asarray(w).reshape(-1)
    if off.size != w.size + 1 or off[0] != 0 or off[-1] != rec.shape[0] or np.any(np.diff(off) < 0):
        raise ValueError("block_offsets: [len(w) + 1], from 0 to the record count, non-decreasing")
    parts = [np.tile(rec[off[b]:off[b + 1]], (int(w[b]),) + (1,) * (rec.ndim - 1)) for b in range(w.size) if w[b] > 0]
    return np.concatenate(parts) if parts else rec[:0].copy()


def _quat_mul(a, b):  # Hamilton product, (x, y, z, w)
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def local_delta(x_ref, x) -> np.ndarray:
    """The d with pose_plus(x_ref, d) = x, exactly: pose_plus sets p = p_ref + dp and q = normalised(q_ref * [1, dtheta / 2]), so
    dp = p - p_ref and dtheta = 2 vec(q_rel) / w(q_rel), q_rel = q_ref^-1 * q (the normalisation cancels in the ratio)."""
    x_ref = np.asarray(x_ref, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    qr = x_ref[3:7]
    q_rel = _quat_mul(np.array([-qr[0], -qr[1], -qr[2], qr[3]]), x[3:7])
    return np.concatenate([x[0:3] - x_ref[0:3], 2.0 * q_rel[0:3] / q_rel[3]])


def local_deltas(x_ref, X) -> np.ndarray:
    return np.stack([local_delta(x_ref, x) for x in np.asarray(X, dtype=np.float64).reshape(-1, 7)])


def jackknife_covariance(x_full, X) -> np.ndarray:
    """(P - 1) / P * sum_k (d_k - mean d)(d_k - mean d)^T over the P leave-one-out solutions X [P, 7], d_k = local_delta(x_full, X[k])."""
    D = local_deltas(x_full, X)
    P = D.shape[0]
    E = D - D.mean(axis=0)
    return (P - 1.0) / P * (E.T @ E)


def bootstrap_covariance(x_full, X) -> np.ndarray:
    """1 / (S - 1) * sum_k (d_k - mean d)(d_k - mean d)^T over the S bootstrap solutions X [S, 7], d_k = local_delta(x_full, X[k])."""
    D = local_deltas(x_full, X)
    S = D.shape[0]
    E = D - D.mean(axis=0)
    return (E.T @ E) / max(S - 1, 1)


def consensus_select(ssq, rms_max: float):
    """The consensus rule on a table of block scores ssq [S, B] (Solver.score_blocks: per candidate k and block b the sum of squared
    residuals; with one block per pose and point rows, sqrt(ssq) is that pose's RMS point-to-plane distance).  Block b SUPPORTS
    candidate k when sqrt(ssq[k, b]) <= rms_max (NaN supports nothing).  The candidate with the largest support wins; ties go to the
    smaller sum of ssq over the supporting blocks, then to the lower index.
    -> (best_index, inlier_mask [B] bool: the winner's supporting blocks, sizes [S]: every candidate's support).  No candidate has any
    support (or S = 0): best_index = -1 and an all-False mask."""
    q = np.asarray(ssq, dtype=np.float64)
    if q.ndim != 2:
        raise ValueError("ssq: [S, B]")
    S, B = q.shape
    with np.errstate(invalid="ignore"):
        sup = np.sqrt(q) <= float(rms_max)   # (NaN, and the square root of a negative number, compare False)
    sizes = sup.sum(axis=1).astype(np.int64)
    if S == 0 or sizes.max() == 0:
        return -1, np.zeros(B, dtype=bool), sizes
    total = np.where(sup, q, 0.0).sum(axis=1)
    best = -1
    for k in range(S):   # (the documented order, written out: support, then sum, then index)
        if sizes[k] == 0:
            continue
        if best < 0 or sizes[k] > sizes[best] or (sizes[k] == sizes[best] and total[k] < total[best]):
            best = k
    return int(best), sup[best].copy(), sizes
