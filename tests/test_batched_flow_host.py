"""The dense back end of the batched closed form and analysis pass (csrc/clc_batchflow.hpp), compiled for the host with g++
(tests/shim/batchflow_shim.cpp): the one-row-per-lane Jacobi sweeps, the pivoted LDL^T solve, U V^T and the closed-form back end
against the host back end they restate (clc_host.hpp) and numpy — on seeded SPD matrices and on the rank-deficient normal
equations of sim_degenerate (exact zero pivots: "parallel_boards"; near-singular: "only_pitch").  Same compiler, same flags:
the restatement must agree with clc_host.hpp bit for bit here.  And the new kernels must not spill."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "camlasercalibratool_amd", "csrc")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bf") / "libbatchflow_shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                           os.path.join(HERE, "shim", "batchflow_shim.cpp"), "-o", out])
    return C.CDLL(out)


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _eig(shim, A, which):
    n = A.shape[0]
    A = np.ascontiguousarray(A, dtype=np.float64)
    w = np.empty(n); V = np.empty((n, n))
    if which == "bf":
        assert shim.shim_bf_eig(_p(A), n, _p(w), _p(V)) == 0
    else:
        shim.shim_host_eig(_p(A), n, _p(w), _p(V))
    return w, V


def _closed_form(shim, AtA, Atb, which):
    AtA = np.ascontiguousarray(AtA, dtype=np.float64); Atb = np.ascontiguousarray(Atb, dtype=np.float64)
    T = np.empty(16); un = C.c_int(); sv9 = np.empty(9); pose = np.empty(7)
    if which == "bf":
        rc = shim.shim_bf_closed_form(_p(AtA), _p(Atb), _p(T), C.byref(un), _p(sv9), _p(pose))
        return rc, T.reshape(4, 4), un.value, sv9, pose
    rc = shim.shim_host_closed_form(_p(AtA), _p(Atb), _p(T), C.byref(un), _p(sv9))
    return rc, T.reshape(4, 4), un.value, sv9, None


def _normal9(rec):
    """A^T A, A^T b of CamLaserCalClosedSolution (src/LaseCamCalCeres.cpp:144-161): row kron([x, y, 1], n), b = -d."""
    n = rec[:, 0:3]; d = rec[:, 3]
    bar = np.stack([rec[:, 4], rec[:, 5], np.ones(len(rec))], 1)
    A = (bar[:, :, None] * n[:, None, :]).reshape(-1, 9)
    return A.T @ A, A.T @ (-d)


def _acc45(rec):
    """The 45 accumulators of K5: [bb(6) x nn(6)] then A^T b (9, b-major)."""
    nx, ny, nz, d, x, y = (rec[:, i] for i in range(6))
    nn = np.stack([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz], 1)
    bb = np.stack([x * x, x * y, x, y * y, y, np.ones_like(x)], 1)
    bv = np.stack([x, y, np.ones_like(x)], 1); nv = np.stack([nx, ny, nz], 1)
    return np.concatenate([(bb[:, :, None] * nn[:, None, :]).reshape(-1, 36).sum(0),
                           ((bv[:, :, None] * nv[:, None, :]).reshape(-1, 9) * (-d)[:, None]).sum(0)])


def _spd(rng, n, cond=1e6):
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = np.exp(rng.uniform(0, np.log(cond), n))
    return (Q * ev) @ Q.T


@pytest.mark.parametrize("n", [3, 6, 9])
def test_jacobi_rows_matches_host_and_numpy(shim, n):
    rng = np.random.default_rng(100 + n)
    for _ in range(20):
        A = _spd(rng, n)
        A = 0.5 * (A + A.T)
        w, V = _eig(shim, A, "bf")
        w0, V0 = _eig(shim, A, "host")
        assert np.array_equal(w, w0) and np.array_equal(V, V0)
        ref = np.sort(np.linalg.eigvalsh(A))[::-1]
        assert np.allclose(w, ref, rtol=1e-10, atol=1e-12 * ref[0])
        assert np.abs(A @ V - V * w).max() <= 1e-9 * ref[0]
        assert np.all(np.diff(w) <= 0)


def test_jacobi_rows_ties_keep_the_host_order(shim):
    """Repeated eigenvalues (a diagonal matrix with ties: no rotation at all) — the columns come out in std::sort's order."""
    A = np.diag([2.0, 5.0, 2.0, 5.0, 1.0, 2.0])
    w, V = _eig(shim, A, "bf")
    w0, V0 = _eig(shim, A, "host")
    assert np.array_equal(w, w0) and np.array_equal(V, V0)


def test_ldlt9_matches_host_on_spd_and_exact_zero_pivots(shim):
    rng = np.random.default_rng(7)
    for k in range(20):
        A = _spd(rng, 9, 1e8)
        if k % 2:  # exact zero rows / columns (the parallel_boards pattern): zero pivots, pseudo-inverse of D
            z = rng.choice(9, size=3, replace=False)
            A[z, :] = 0.0; A[:, z] = 0.0
        b = rng.normal(size=9)
        x = np.empty(9); x0 = np.empty(9)
        Ac = np.ascontiguousarray(A)
        shim.shim_bf_ldlt9(_p(Ac), _p(b), _p(x))
        shim.shim_host_ldlt9(_p(Ac), _p(b), _p(x0))
        assert np.array_equal(x, x0)
        if k % 2 == 0:
            assert np.allclose(A @ x, b, rtol=0, atol=1e-6 * np.abs(b).max())


def test_nearest_orthogonal3_matches_host(shim):
    rng = np.random.default_rng(11)
    cases = [rng.normal(size=(3, 3)) for _ in range(20)]
    cases += [np.outer(rng.normal(size=3), rng.normal(size=3)), np.zeros((3, 3))]  # rank 1 and 0: completed U
    for M in cases:
        M = np.ascontiguousarray(M)
        Q = np.empty(9); Q0 = np.empty(9)
        shim.shim_bf_orth3(_p(M), _p(Q))
        shim.shim_host_orth3(_p(M), _p(Q0))
        assert np.array_equal(Q, Q0)
        Q = Q.reshape(3, 3)
        assert np.abs(Q @ Q.T - np.eye(3)).max() < 1e-12


def _check_closed_form(shim, AtA, Atb):
    from camlasercalibratool_amd import simdata as sd
    rc, T, un, sv9, pose = _closed_form(shim, AtA, Atb, "bf")
    rc0, T0, un0, sv90, _ = _closed_form(shim, AtA, Atb, "host")
    assert rc == rc0 and un == un0 and np.array_equal(sv9, sv90)
    assert np.array_equal(T, T0) or (np.isnan(T).any() and np.isnan(T0).any())
    if rc == 0:
        assert np.abs(pose - sd.pose7_from_T(np.linalg.inv(T))).max() <= 1e-12
    return rc, T, un, sv9


def test_closed_form_back_end_on_noisy_batches(shim, oracle_mod):
    from camlasercalibratool_amd import simdata as sd
    probs, _ = sd.sim_batch(5, 6, 20, 100, 0.01)
    for S in probs:
        rec = oracle_mod.flatten(S, True, False)
        AtA, Atb = _normal9(rec)
        rc, T, un, sv9 = _check_closed_form(shim, AtA, Atb)
        T_or, un_or, sv9_or = oracle_mod.closed_form(rec)
        assert rc == 0 and un == un_or == 0
        assert np.abs(T - T_or).max() < 1e-9 and np.allclose(sv9, sv9_or, rtol=1e-9)


@pytest.mark.parametrize("kind", ["parallel_boards", "only_pitch"])
def test_closed_form_back_end_on_unobservable_systems(shim, oracle_mod, kind):
    from camlasercalibratool_amd import simdata as sd
    rec = oracle_mod.flatten(sd.sim_degenerate(kind), True, False)
    AtA, Atb = _normal9(rec)
    rc, T, un, sv9 = _check_closed_form(shim, AtA, Atb)
    T_or, un_or, sv9_or = oracle_mod.closed_form(rec)
    assert un == un_or == 1 and rc == 0 and np.isfinite(T).all()
    assert np.abs(sv9 - sv9_or).max() <= 1e-9 * sv9_or[0]
    ref = np.sort(np.linalg.eigvalsh(AtA))[::-1]
    assert np.abs(sv9 - ref).max() <= 1e-9 * ref[0]


def test_accumulator_expansion_is_the_normal_equation(shim, oracle_mod):
    from camlasercalibratool_amd import simdata as sd
    probs, _ = sd.sim_batch(9, 1, 10, 50, 0.01)
    rec = oracle_mod.flatten(probs[0], True, False)
    acc = _acc45(rec)
    AtA = np.empty(81)
    shim.shim_bf_expand45(_p(acc), _p(AtA))
    AtA0, Atb0 = _normal9(rec)
    assert np.allclose(AtA.reshape(9, 9), AtA0, rtol=1e-12, atol=1e-12 * np.abs(AtA0).max())
    assert np.allclose(acc[36:], Atb0, rtol=1e-12, atol=1e-12 * np.abs(Atb0).max())


def test_batched_flow_kernels_do_not_spill():
    import sys
    sys.path.insert(0, ROOT)
    from camlasercalibratool_amd import _build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc] + _build.HIPCC_FLAGS + ["-c", os.path.join(CSRC, "abi_batchflow.hip"), "-o", os.path.join(tmp, "bf.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    res, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            res[cur][m.group(1).strip()] = int(m.group(2))
    names = [k for k in res if "bf_" in k]
    for frag in ("bf_normal9_rows_kernel", "bf_normal9_tiles_kernel", "bf_closed_form_kernel", "bf_info_rows_kernel",
                 "bf_info_tiles_kernel", "bf_info_kernel"):
        assert any(frag in k for k in names), frag
    for k in names:
        u = res[k]
        assert u["ScratchSize"] == 0 and u.get("SGPRs Spill", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (k, u)
        assert u["VGPRs"] <= 256, (k, u)
