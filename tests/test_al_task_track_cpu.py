"""CPU side of the task family's bounds track and of the plant's task score (include/ilqr_hip.h ilqr_hip_set_al_task_bounds_track,
ilqr_hip_plant_set_task_score): the footstep helper of scenario.py on a hand-written schedule, the NumPy score reference
(tests/plant_task_score_ref.py) and the proof, on the reference alone, that the case set of the GPU tests discriminates and stays away
from every equality a comparison could trip over; the exported symbols.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import al_task_ref as tr
import al_task_track_cases as tc
import plant_task_score_ref as pts
from conftest import load_package

pkg = load_package()
sc = pkg.scenario
INF = np.inf
ERR_ARG = 1


def _track(**kw):
    args = dict(half_size=tc.HALF, land_rows=2, clearance=tc.CLEARANCE, clearance_margin_rows=1)
    args.update(kw)
    return sc.al_task_track_from_footsteps(tc.SCHEDULE, tc.FOOTSTEPS, **args)


def test_swing_phases_of_the_hand_written_schedule():
    assert sc.swing_phases(tc.SCHEDULE[:, 0]) == tc.PHASES["left"]
    assert sc.swing_phases(tc.SCHEDULE[:, 1]) == tc.PHASES["right"]          # the second phase reaches the last row
    assert sc.swing_phases(np.ones(5, dtype=int)) == [] and sc.swing_phases(np.zeros(3, dtype=int)) == [(0, 3)]


def test_track_from_footsteps_row_by_row():
    t = _track()
    assert t.shape == (12, 18)
    want = np.tile(tr.NO_BOUNDS, (12, 1))
    hx, hy = tc.HALF
    # landing rows: the last two rows of each phase, x and y only
    for k0, rows, (cx, cy) in ((3, (4, 5), tc.FOOTSTEPS["left"][0]), (6, (0, 1), tc.FOOTSTEPS["right"][0]), (6, (10, 11), tc.FOOTSTEPS["right"][1])):
        for r in rows:
            want[r, k0:k0 + 2] = (cx - hx, cy - hy); want[r, 9 + k0:9 + k0 + 2] = (cx + hx, cy + hy)
    # clearance rows: at least one row from both ends of the phase -- left [2, 6): 3, 4; right [0, 2): none; right [8, 12): 9, 10
    want[[3, 4], 5] = tc.CLEARANCE
    want[[9, 10], 8] = tc.CLEARANCE
    assert np.array_equal(t, want)
    assert np.all(t[:, [0, 1, 2]] == -INF) and np.all(t[:, [9, 10, 11]] == INF)      # the CoM is never bounded
    assert np.all(t[:, 9 + 5] == INF) and np.all(t[:, 9 + 8] == INF)                 # z has no upper bound
    # the defaults: land_rows = 2, no clearance; a margin of 2 leaves no row of a four-row phase
    assert np.array_equal(sc.al_task_track_from_footsteps(tc.SCHEDULE, tc.FOOTSTEPS, tc.HALF)[:, [5, 8]], np.full((12, 2), -INF))
    assert np.all(_track(clearance_margin_rows=2)[:, [5, 8]] == -INF)
    assert np.array_equal(np.isfinite(_track(clearance_margin_rows=0)[:, 8]), tc.SCHEDULE[:, 1] == 0)
    # land_rows beyond the phase: the whole phase, not a row before it
    long = _track(land_rows=9)
    assert np.array_equal(np.isfinite(long[:, 3]), tc.SCHEDULE[:, 0] == 0) and np.array_equal(np.isfinite(long[:, 6]), tc.SCHEDULE[:, 1] == 0)
    # a scalar half size serves both axes
    one = _track(half_size=0.04)
    assert one[5, 3] == tc.FOOTSTEPS["left"][0][0] - 0.04 and one[5, 9 + 4] == tc.FOOTSTEPS["left"][0][1] + 0.04


def test_track_from_footsteps_passes_the_stackers_validation_and_is_its_track():
    t = _track()
    lo, hi = t[:, :9], t[:, 9:]
    assert not np.isnan(t).any() and (lo <= hi).all() and not (lo == INF).any() and not (hi == -INF).any()
    # stack_al_task_bounds as a track builder: N + 1 = rows, one record
    rows = t.shape[0]
    again = sc.stack_al_task_bounds(dict(left_foot=(t[:, 3:6], t[:, 12:15]), right_foot=(t[:, 6:9], t[:, 15:18])), 1, rows - 1)
    assert again.shape == (1, rows, 18) and np.array_equal(again[0], t)


def test_track_from_footsteps_refuses():
    good = dict(stance=tc.SCHEDULE, footsteps=tc.FOOTSTEPS, half_size=tc.HALF)
    for bad in (dict(footsteps={"left": [], "right": tc.FOOTSTEPS["right"]}),                       # a footstep too few
                dict(footsteps={"left": tc.FOOTSTEPS["left"], "right": tc.FOOTSTEPS["right"] + [(0.0, 0.0)]}),      # one too many
                dict(footsteps={"left": tc.FOOTSTEPS["left"]}), dict(footsteps=[(0.0, 0.0)]),
                dict(footsteps={"left": [(0.3, 0.2, 0.1)], "right": tc.FOOTSTEPS["right"]}),
                dict(stance=tc.SCHEDULE[:, :1]), dict(stance=tc.SCHEDULE.reshape(-1)), dict(stance=np.zeros((0, 2), dtype=int)),
                dict(half_size=(0.1, 0.1, 0.1)), dict(half_size=-0.1), dict(land_rows=-1), dict(clearance_margin_rows=-1), dict(clearance=(0.1, 0.2))):
        with pytest.raises(ValueError):
            sc.al_task_track_from_footsteps(**dict(good, **bad))
    assert sc.al_task_track_from_footsteps(**good).shape == (12, 18)


# ---------------------------------------------------------------------------------------------------------------------- the score reference
def test_reference_by_hand():
    P = np.array([0.0, 0.0, 1.0, 0.1, 0.2, 0.05, 0.1, -0.2, 0.30])
    win = np.tile(tr.NO_BOUNDS, 1).copy()
    win[2] = 1.02; win[9 + 2] = 2.0             # CoM z 2 cm below its floor
    win[5] = 0.08                               # left foot 3 cm below its floor
    win[9 + 8] = 0.25                           # right foot 5 cm above its ceiling
    t = pts.interval_terms(P, win, np.array([0, 0]), 0.025)
    assert np.allclose(t[:3], [0.02, 0.03, 0.05], atol=1e-15) and t[3:6].tolist() == [0.0, 1.0, 1.0] and t[7] == 1.0
    assert abs(t[6] - (0.02 ** 2 + 0.03 ** 2 + 0.05 ** 2)) < 1e-15
    # the left foot stands: its rows are off, the right foot's are not
    t = pts.interval_terms(P, win, np.array([1, 0]), 0.025)
    assert t[1] == 0.0 and t[4] == 0.0 and t[2] > 0.0 and abs(t[6] - (0.02 ** 2 + 0.05 ** 2)) < 1e-15
    # a non-finite point: NaN in slot 6, counted, left out of the rest
    Pn = P.copy(); Pn[4] = np.nan
    t = pts.interval_terms(Pn, win, np.array([0, 0]), 0.025)
    assert np.isnan(t[6]) and t[7] == 1.0 and np.all(t[:6] == 0.0)
    # the fold: maxima and sums, in order
    rec = pts.fold(np.zeros((1, 8)), np.array([[[0.01, 0, 0.03, 0, 0, 1, 1e-3, 1]], [[0.02, 0, 0.01, 1, 0, 0, 2e-3, 1]]]))
    assert rec[0].tolist() == [0.02, 0.0, 0.03, 1.0, 0.0, 1.0, 1e-3 + 2e-3, 2.0]


def _static_rows(m=3):
    """the case set as the CPU knows it: the plant's initial points against the rows 0..m-1 of window and schedule"""
    prob, x0, ui, win, P0, excited = tc.score_case()
    P = np.tile(P0, (m, 1, 1))
    return P, np.moveaxis(win[:, :m], 1, 0), np.moveaxis(prob["stance"][:, :m], 1, 0), excited


def test_the_score_case_set_discriminates_and_keeps_its_distance():
    P, w, st, excited = _static_rows()
    B = P.shape[1]
    assert B == tc.B_WAVE and len(excited) == B
    v = pts.violations(P, w, st)                                   # [3, B, 9]
    # each of the 18 sides is violated somewhere, with a size below and a size above the tolerance
    for k in range(9):
        for side in range(2):
            sizes = {size for b, (k_, s_, size) in enumerate(excited) if (k_, s_) == (k, side) and b not in tc.INF_ROLLOUTS and v[:, b, k].max() > 0.0}
            assert sizes == {tc.SMALL, tc.LARGE}, (k, side, sizes)
    for b, (k, side, size) in enumerate(excited):
        d = (P[:, b, k] - w[:, b, 9 + k]) if side else (w[:, b, k] - P[:, b, k])
        if b in tc.INF_ROLLOUTS:
            assert np.all(d == -INF) and np.all(v[:, b] == 0.0)            # an infinite side never counts
        else:
            assert np.allclose(d, size + 1e-3 * np.arange(3), atol=1e-12)   # the designed distance, another one per knot
    # a stance-foot row that would be violated but for the stance rule -- and the record differs without the rule
    free = pts.violations(P, w, np.zeros_like(st))
    hidden = (free > 1e-6) & (v == 0.0)
    assert hidden.any() and hidden[..., :3].sum() == 0
    rec = pts.fold(np.zeros((B, 8)), pts.interval_terms(P, w, st, tc.TOL))
    rec_free = pts.fold(np.zeros((B, 8)), pts.interval_terms(P, w, np.zeros_like(st), tc.TOL))
    assert not np.array_equal(rec, rec_free)
    # tol above and below a violation: counts of both kinds, and another tolerance gives other counts
    assert (rec[:, 3:6].sum(axis=1) > 0).any() and ((rec[:, :3].max(axis=1) > 0) & (rec[:, 3:6].sum(axis=1) == 0)).any()
    assert not np.array_equal(rec[:, 3:6], pts.fold(np.zeros((B, 8)), pts.interval_terms(P, w, st, 0.5 * tc.SMALL))[:, 3:6])
    # every group has a violation and a count somewhere; rows differ from knot to knot (another row's bounds give another record)
    assert np.all((rec[:, :3] > 0).sum(axis=0) > 0) and np.all(rec[:, 3:6].sum(axis=0) > 0) and np.all(rec[:, 7] == 3.0)
    assert not np.allclose(rec[:, 6], pts.fold(np.zeros((B, 8)), pts.interval_terms(P, np.roll(w, 1, axis=0), st, tc.TOL))[:, 6], atol=1e-9)
    # the distance from every equality: 1e-6 at the least (the GPU tests repeat this on the rows their plant produced)
    side, decision = pts.margins(P, w, st, tc.TOL)
    print("smallest |p - bound| over the live finite sides %.3e m, smallest |V_g - tol| %.3e m" % (side, decision))
    assert side >= 1e-6 and decision >= 1e-6


def test_exported_symbols():
    import __graft_entry__ as ge
    ge.build_library()
    from mpc_ilqr_mujoco_amd import solver as sv
    L = sv.load_library()
    legacy = C.CDLL(sv.LEGACY_LIB_PATH)
    names = ("ilqr_hip_set_al_task_bounds_track", "ilqr_hip_clear_al_task_bounds_track", "ilqr_hip_al_task_bounds_track_rows",
             "ilqr_hip_plant_set_task_score", "ilqr_hip_plant_clear_task_score", "ilqr_hip_plant_get_task_score", "ilqr_hip_plant_task_score_device")
    for name in names:
        assert hasattr(L, name) and hasattr(legacy, name), name
    # null handles are refused before anything is touched
    assert L.ilqr_hip_set_al_task_bounds_track(None, 1, None) == ERR_ARG and L.ilqr_hip_clear_al_task_bounds_track(None) == ERR_ARG
    assert L.ilqr_hip_al_task_bounds_track_rows(None) == -1 and L.ilqr_hip_al_bounds_track_rows(None) == -1
    assert L.ilqr_hip_plant_set_task_score(None, C.c_double(0.0)) == ERR_ARG and L.ilqr_hip_plant_clear_task_score(None) == ERR_ARG
    assert L.ilqr_hip_plant_get_task_score(None, None) == ERR_ARG and L.ilqr_hip_plant_task_score_device(None, None) == ERR_ARG
    assert len(sv.PLANT_TASK_SCORE_TERMS) == 8
    # the kernels live in the per-knot module
    M = C.CDLL(os.path.join(os.path.dirname(sv.LIB_PATH), "libilqr_hip_alknot.so"))
    assert hasattr(M, "ilqr_alknot_module") and hasattr(M, "ilqr_alknot_module_plant_task_score") and hasattr(M, "ilqr_alknot_module_window_from_track")
