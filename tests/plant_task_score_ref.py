"""CPU restatement of the task score of the resident plant (include/ilqr_hip.h ilqr_hip_plant_set_task_score), in NumPy on top of
al_task_ref.points / rows_off: the nine points of a state row of the history ring against one row of the task window, a foot's rows off
where the schedule row has it in stance.

For one interval: v_i = max(0, p_i - hi_i, lo_i - p_i) (an infinite side never counts; a switched-off row gives 0), V_g the maximum of v_i
over the group g = CoM, left foot, right foot.  The record, eight doubles per rollout: 0..2 the maximum of V_g over the scored intervals
(0 before the first), 3..5 the number of intervals with V_g > tol, 6 the sum of v_i^2 over intervals and coordinates, 7 the intervals scored.
An interval with a non-finite point adds NaN to slot 6, counts in slot 7 and is left out of slots 0..5.  No GPU."""
import numpy as np

import al_task_ref as tr

COORDS, TERMS = tr.COORDS, 8
GROUP_OF = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2])
# the points are held to what the task tests hold them to (test_gpu_al_task.py: |got - want| <= 1e-12 on every coordinate)
POINT_TOL = 1e-12


def violations(P, win, stance):
    """v [..., 9] of points P [..., 9] against window rows win [..., 18] under stance flags [..., 2]; a non-finite point gives NaN in v"""
    P, win = np.asarray(P, dtype=np.float64), np.asarray(win, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        v = np.maximum(0.0, np.maximum(P - win[..., COORDS:], win[..., :COORDS] - P))
    v = np.where(tr.rows_off(stance), 0.0, v)
    return np.where(np.isfinite(P), v, np.nan)


def interval_terms(P, win, stance, tol):
    """term rows [..., 8] of one interval per leading index"""
    v = violations(P, win, stance)
    bad = ~np.isfinite(np.asarray(P, dtype=np.float64)).all(axis=-1)
    out = np.zeros(v.shape[:-1] + (TERMS,))
    for g in range(3):
        V = np.where(bad, 0.0, np.nan_to_num(v[..., GROUP_OF == g]).max(axis=-1))
        out[..., g] = V
        out[..., 3 + g] = np.where(bad, 0.0, (V > tol).astype(np.float64))
    out[..., 6] = np.where(bad, np.nan, np.nan_to_num(v ** 2).sum(axis=-1))
    out[..., 7] = 1.0
    return out


def fold(record, terms):
    """the record [B, 8] with the term rows [m, B, 8] folded in, in interval order"""
    rec = np.array(record, dtype=np.float64)
    for t in terms:
        rec[:, :3] = np.maximum(rec[:, :3], t[:, :3])
        rec[:, 3:] = rec[:, 3:] + t[:, 3:]
    return rec


def expected_record(hx, win_rows, stance_rows, tol, points=None):
    """record [B, 8] of ring rows hx [m, B, 51] against window rows win_rows [m, B, 18] and schedule rows stance_rows [m, B, 2]"""
    P = tr.points(hx) if points is None else points
    return fold(np.zeros((hx.shape[1], TERMS)), interval_terms(P, win_rows, stance_rows, tol))


def margins(P, win, stance, tol):
    """(side, decision): how far the inputs are from an equality the comparison with the device could trip over -- the smallest
    |p - bound| over the finite sides of rows that are on, and the smallest |V_g - tol| over the groups with a violation (finite points only)"""
    P, win = np.asarray(P, dtype=np.float64), np.asarray(win, dtype=np.float64)
    on = ~tr.rows_off(stance) & np.isfinite(P)
    bounds = np.stack([win[..., :COORDS], win[..., COORDS:]], axis=-1)
    with np.errstate(invalid="ignore"):
        d = np.abs(P[..., None] - bounds)
    fin = np.isfinite(bounds) & on[..., None]
    side = d[fin].min() if fin.any() else np.inf
    t = interval_terms(P, win, stance, tol)
    # (a group without a live violated side has V_g = 0 exactly, on the device too while `side` holds: V_g > tol is then false whatever tol >= 0 is)
    V = t[..., :3][np.isfinite(t[..., 6])]
    V = V[V > 0.0]
    decision = np.abs(V - tol).min() if V.size else np.inf
    return float(side), float(decision)


def close_enough(got, want):
    """the comparison of the GPU tests: the points-derived slots 0..2 to POINT_TOL absolute, slot 6 to POINT_TOL scaled by its own (squared)
    magnitude where that exceeds 1, slots 3..5 and 7 exact; NaN must meet NaN"""
    got, want = np.asarray(got), np.asarray(want)
    ok = (np.abs(got[:, :3] - want[:, :3]) <= POINT_TOL).all(axis=1)
    ok &= (got[:, 3:6] == want[:, 3:6]).all(axis=1) & (got[:, 7] == want[:, 7])
    nan = np.isnan(want[:, 6])
    with np.errstate(invalid="ignore"):
        ok &= np.where(nan, np.isnan(got[:, 6]), np.abs(got[:, 6] - want[:, 6]) <= POINT_TOL * np.maximum(1.0, np.abs(want[:, 6])))
    return ok
