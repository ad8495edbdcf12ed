"""clc_solve_subsets and camlasercalibratool_amd.resample without a GPU: the symbol is declared, exported and bound; the definition
of a weighted subset (resample.materialize); seeded weight generators; local coordinates and covariance estimates against a direct
numpy computation on poses the oracle produced for materialised subsets."""
import ctypes as C
import os
import re

import numpy as np

from camlasercalibratool_amd import _build, _capi, resample, simdata as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solve_subsets_is_declared_exported_and_refuses_a_null_handle():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clc.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+clc_solve_subsets\s*\(\s*clc_handle\s*\*", hdr)
    assert "clc_solve_subsets" in _capi.EXPORTED
    off = (C.c_int64 * 2)(0, 1)
    w = (C.c_uint8 * 1)(1)
    pose = (C.c_double * 7)(0, 0, 0, 0, 0, 0, 1)
    sm = _capi.Summary()
    for path in (_build.PRODUCT_LIB_PATH, _build.HOOKS_LIB_PATH):
        L = _capi.load(path)
        assert L.clc_version() == 210
        rc = L.clc_solve_subsets(None, None, 1, off, 1, w, pose, C.byref(sm))
        assert rc == -1 and _capi.ERRORS[rc] == "CLC_ERR_INVALID_ARG"
        assert L.clc_last_error().decode().startswith("clc_solve_subsets")
        assert list(pose) == [0, 0, 0, 0, 0, 0, 1]


def test_materialize_is_the_definition():
    rec = np.arange(7 * 8, dtype=np.float64).reshape(7, 8)
    off = [0, 2, 2, 5, 7]   # blocks of 2, 0, 3, 2 records
    got = resample.materialize(rec, off, [2, 3, 0, 1])
    assert np.array_equal(got, rec[[0, 1, 0, 1, 5, 6]])
    assert np.array_equal(resample.materialize(rec, off, [1, 1, 1, 1]), rec)
    assert resample.materialize(rec, off, [0, 0, 0, 0]).shape == (0, 8)
    assert np.array_equal(resample.materialize(rec, off, np.array([0, 0, 3, 0], dtype=np.uint8)), rec[[2, 3, 4] * 3])
    for bad in ([0, 2, 5, 7], [1, 2, 2, 5, 7], [0, 2, 2, 5, 6], [0, 3, 2, 5, 7]):
        try:
            resample.materialize(rec, bad, [1, 1, 1, 1])
        except ValueError:
            continue
        raise AssertionError(bad)


def test_weight_generators_are_seeded_and_well_formed():
    J = resample.jackknife_weights(6)
    assert J.dtype == np.uint8 and J.shape == (6, 6) and np.array_equal(J, 1 - np.eye(6, dtype=np.uint8))
    B = resample.bootstrap_weights(50, 60, 3)
    assert B.dtype == np.uint8 and B.shape == (60, 50) and np.all(B.sum(axis=1) == 50) and B.max() > 1
    assert np.array_equal(B, resample.bootstrap_weights(50, 60, 3)) and not np.array_equal(B, resample.bootstrap_weights(50, 60, 4))
    # the documented stream: P draws with replacement per row from default_rng(seed)
    rng = np.random.default_rng(3)
    assert np.array_equal(B[0], np.bincount(rng.integers(0, 50, 50), minlength=50))
    R = resample.random_subset_weights(50, 20, 8, 5)
    assert R.dtype == np.uint8 and R.shape == (20, 50) and np.all(R.sum(axis=1) == 8) and R.max() == 1
    assert np.array_equal(R, resample.random_subset_weights(50, 20, 8, 5)) and not np.array_equal(R, resample.random_subset_weights(50, 20, 8, 6))
    assert len({r.tobytes() for r in R}) > 1


def test_local_delta_inverts_pose_plus(oracle_mod):
    rng = np.random.default_rng(0)
    x = sd.pose7_from_T(sd.tlc_to_tcl(sd.GT_RLC, sd.GT_TLC))
    worst = 0.0
    for k in range(200):
        d = rng.uniform(-1, 1, 6)
        d *= rng.uniform(0, 0.1) / np.abs(d).max()
        xk = oracle_mod.pose_plus(x, d)
        worst = max(worst, np.abs(resample.local_delta(x, xk) - d).max())
        x = xk if k % 10 == 9 else x   # (walk the reference pose too)
    assert worst <= 1e-12, worst
    assert np.array_equal(resample.local_delta(x, x)[:3], np.zeros(3)) and np.abs(resample.local_delta(x, x)).max() <= 1e-16
    # q and -q are the same rotation
    y = oracle_mod.pose_plus(x, np.array([0, 0, 0, .05, -.02, .01]))
    y2 = y.copy()
    y2[3:] = -y2[3:]
    assert np.allclose(resample.local_delta(x, y), resample.local_delta(x, y2), rtol=0, atol=1e-15)


def test_covariances_against_numpy_on_oracle_solutions_of_materialised_subsets(oracle_mod):
    """12 poses x 40 points: the oracle solves every leave-one-out problem and 16 bootstrap problems; the module's estimates against
    the textbook formulas written out with numpy on the same poses."""
    import oracle
    S = sd.sim_fixed_count(21, 12, 40, noise_sigma=0.01)
    rec = oracle.flatten(S, False, False)
    off = np.arange(13, dtype=np.int64) * 40
    x0 = oracle_mod.pose_plus(sd.pose7_from_T(sd.tlc_to_tcl(sd.GT_RLC, sd.GT_TLC)), np.array([.01, -.01, .02, .01, .01, -.02]))
    full = oracle_mod.solve(rec, x0, linear_solver="qr").pose

    def deltas(W):
        X = np.stack([oracle_mod.solve(resample.materialize(rec, off, w), full, linear_solver="qr").pose for w in W])
        D = np.empty((len(W), 6))
        for k, xk in enumerate(X):   # written out: dp, and dtheta from the relative rotation R_full^T R_k = I + [dtheta]x + O(dtheta^2)
            D[k, :3] = xk[:3] - full[:3]
            Rrel = sd.T_from_pose7(full)[:3, :3].T @ sd.T_from_pose7(xk)[:3, :3]
            D[k, 3:] = [Rrel[2, 1] - Rrel[1, 2], Rrel[0, 2] - Rrel[2, 0], Rrel[1, 0] - Rrel[0, 1]]
            D[k, 3:] /= 1.0 + np.trace(Rrel)   # 2 vec(q) / w(q) = (R - R^T)^vee / (1 + tr R), exactly
            D[k, 3:] *= 2.0
        return X, D

    X, D = deltas(resample.jackknife_weights(12))
    assert np.abs(resample.local_deltas(full, X) - D).max() <= 1e-12
    E = D - D.mean(axis=0)
    want = 11.0 / 12.0 * sum(np.outer(e, e) for e in E)
    got = resample.jackknife_covariance(full, X)
    assert got.shape == (6, 6) and np.allclose(got, got.T, rtol=0, atol=0) and np.all(np.diag(got) > 0)
    # (deltas agree to 1e-12 absolute on values of ~1e-3: products of two of them to ~1e-9 relative)
    assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max()
    Xb, Db = deltas(resample.bootstrap_weights(12, 16, 1))
    Eb = Db - Db.mean(axis=0)
    wantb = sum(np.outer(e, e) for e in Eb) / 15.0
    assert np.abs(resample.bootstrap_covariance(full, Xb) - wantb).max() <= 1e-8 * np.abs(wantb).max()


def test_as_weight_rows_refuses_what_a_cast_to_uint8_would_hide():
    """Solver.solve_subsets converts its weights with resample.as_weight_rows: 256 must not become 0 (the block left out), -1 not 255,
    2.5 not 2."""
    B = 5
    ok = resample.as_weight_rows([[0, 1, 2, 254, 255], [1, 1, 1, 1, 1]], B)
    assert ok.dtype == np.uint8 and ok.shape == (2, B) and ok.flags["C_CONTIGUOUS"] and ok[0].tolist() == [0, 1, 2, 254, 255]
    one = resample.as_weight_rows(np.array([0, 3, 0, 255, 1], dtype=np.int64), B)          # one row
    assert one.shape == (1, B) and one.tolist() == [[0, 3, 0, 255, 1]]
    assert resample.as_weight_rows(np.array([[0.0, 1.0, 2.0, 255.0, 7.0]]), B).tolist() == [[0, 1, 2, 255, 7]]   # integral floats
    assert resample.as_weight_rows(np.array([[True, False, True, True, False]]), B).tolist() == [[1, 0, 1, 1, 0]]
    sliced = np.arange(20, dtype=np.int32).reshape(2, 10)[:, ::2]                            # not contiguous
    assert np.array_equal(resample.as_weight_rows(sliced, B), sliced) and resample.as_weight_rows(sliced, B).flags["C_CONTIGUOUS"]
    u8 = resample.jackknife_weights(B)
    assert np.array_equal(resample.as_weight_rows(u8, B), u8)
    bad = [np.array([[0, 1, 2, 3, 256]]), np.array([[0, 1, 2, 3, -1]]), np.array([[0, 1, 2, 3, 2.5]]), np.array([[0, 1, 2, 3, np.nan]]),
           np.array([[0, 1, 2, 3, np.inf]]), np.array([[0, 1, 2, 3, 1e3]]), np.zeros((2, 4), dtype=np.uint8), np.zeros((2, 6), dtype=np.uint8),
           np.zeros(10, dtype=np.uint8), np.zeros((1, 2, B), dtype=np.uint8), np.zeros((0, B), dtype=np.uint8), np.uint8(1),
           np.array([["1"] * B]), np.array([[1 + 0j] * B])]
    for w in bad:
        try:
            resample.as_weight_rows(w, B)
        except ValueError:
            continue
        raise AssertionError(w)
    # what the plain cast did
    assert np.ascontiguousarray(np.array([256, -1]), dtype=np.uint8).tolist() == [0, 255]
    # Solver.solve_subsets converts before it touches the library: a Solver without a handle gets as far as the refusal
    from camlasercalibratool_amd import solver
    s = solver.Solver.__new__(solver.Solver)
    for w in (np.array([[1, 1, 256, 1, 1]]), np.array([[1, 1, -1, 1, 1]]), np.array([[1, 1, 2.5, 1, 1]]), np.ones(2 * B, dtype=np.uint8)):
        try:
            s.solve_subsets(np.arange(B + 1), w, np.array([0, 0, 0, 0, 0, 0, 1.0]))
        except ValueError:
            continue
        raise AssertionError(w)
