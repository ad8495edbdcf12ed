"""Near ties of the LM controller's decisions (csrc/clc_lm.hpp, the oracle's lm_minimize) — a test helper.

Two solvers that sum in different orders (a GPU kernel and the oracle, or two GPU forms) take the same decisions in every
iteration of the LM loop unless one of them sits right on its threshold.  The four decisions:
  * ParameterToleranceReached: step_norm <= ptol * (|x| + ptol)
  * FunctionToleranceReached:  |cost_change| <= ftol * cost
  * IsStepSuccessful:          relative_decrease > min_relative_decrease
  * after a successful step:   gradient_max_norm <= gtol
A difference in iteration count or termination is accepted only when the oracle's own trace shows one of them within
TIE_REL (relative) of its threshold, at or before the iteration where the earlier of the two solves stopped.

The oracle's trace leaves out the iteration that a parameter or function test ends.  The helper therefore solves again with
the three tolerances at zero (they decide termination only, so the iterations up to there are the same) and reads that
iteration from the longer trace; the |x| of iteration k's parameter test is the pose after iteration k - 1, which a solve
with max_num_iterations = k - 1 returns."""
import numpy as np

TIE_REL = 1e-8
PARAMETER, FUNCTION = 2, 3   # CLC_CONVERGENCE_PARAMETER / _FUNCTION (include/clc.h) = the oracle's codes


def _close(v, thr):
    return thr != 0.0 and abs(v - thr) <= TIE_REL * abs(thr)


def _stop_iteration(termination, num_iterations):
    """The iteration whose tests ended a solve: the parameter and function tests run before the iteration is recorded."""
    return num_iterations + 1 if termination in (PARAMETER, FUNCTION) else num_iterations


def near_tie(oracle_mod, records, x0, options, a, b):
    """options: the oracle's Options both solves ran with; a, b: (termination, num_iterations) of the two solves.
    -> None, or a description of the first decision within TIE_REL of its threshold up to the earlier stop."""
    o = options
    k_stop = min(_stop_iteration(*a[:2]), _stop_iteration(*b[:2]))
    full_o = oracle_mod.Options.from_buffer_copy(o)
    full_o.function_tolerance = full_o.gradient_tolerance = full_o.parameter_tolerance = 0.0
    full_o.max_num_iterations = max(k_stop, 0)
    full = oracle_mod.solve(records, x0, full_o, linear_solver="qr", trace_cap=k_stop + 2).trace
    if _close(full[0].gradient_max_norm, o.gradient_tolerance):
        return f"iteration 0: gradient test, gradient_max_norm {full[0].gradient_max_norm!r} vs {o.gradient_tolerance!r}"
    x_cost = full[0].cost
    x_norm0 = float(np.linalg.norm(np.asarray(x0, dtype=np.float64)))
    for k in range(1, min(k_stop, len(full) - 1) + 1):
        it = full[k]
        if it.step_is_valid:
            thr = o.parameter_tolerance * (x_norm0 + o.parameter_tolerance)
            if abs(it.step_norm - thr) <= 0.5 * thr:  # |x| moves little: only then is the exact |x| worth a solve
                part = oracle_mod.Options.from_buffer_copy(full_o)
                part.max_num_iterations = k - 1
                xk = oracle_mod.solve(records, x0, part, linear_solver="qr", trace_cap=k + 1).pose
                thr = o.parameter_tolerance * (float(np.linalg.norm(xk)) + o.parameter_tolerance)
                if _close(it.step_norm, thr):
                    return f"iteration {k}: parameter test, step_norm {it.step_norm!r} vs {thr!r}"
            if _close(abs(it.cost_change), o.function_tolerance * x_cost):
                return f"iteration {k}: function test, |cost_change| {abs(it.cost_change)!r} vs {o.function_tolerance * x_cost!r}"
            if _close(it.relative_decrease, o.min_relative_decrease):
                return f"iteration {k}: step test, relative_decrease {it.relative_decrease!r} vs {o.min_relative_decrease!r}"
        if it.step_is_successful:
            if _close(it.gradient_max_norm, o.gradient_tolerance):
                return f"iteration {k}: gradient test, gradient_max_norm {it.gradient_max_norm!r} vs {o.gradient_tolerance!r}"
            x_cost = it.cost
    return None


def require_near_tie(oracle_mod, records, x0, options, got, ref, label):
    """got / ref: (termination, num_iterations, final_cost) of two solves that took different decisions somewhere; options: the
    oracle's Options of both.  Requires a near tie in the oracle's trace and final costs within ftol * cost; prints the exemption."""
    assert records.shape[0] > 0, (label, "an empty problem has no decision to tie")
    why = near_tie(oracle_mod, records, x0, options, got, ref)
    assert why is not None, (label, "the solves' decisions differ without a near tie", tuple(got), tuple(ref))
    assert abs(got[2] - ref[2]) <= options.function_tolerance * abs(ref[2]), (label, why, tuple(got), tuple(ref))
    print(f"near-tie exemption {label}: {tuple(got)} vs {tuple(ref)}: {why}")


def check_flip(oracle_mod, records, x0, options, got, ref, label):
    """got / ref as above.  Same termination and iteration count -> 0; otherwise require_near_tie, -> 1."""
    if tuple(got[:2]) == tuple(ref[:2]):
        return 0
    require_near_tie(oracle_mod, records, x0, options, got, ref, label)
    return 1
