"""The window rule of the reference track on the CPU (references.ReferenceData.problem_at_starts; include/ilqr_hip.h
ilqr_hip_window_from_track applies the same rule on the device, tests/test_gpu_reference_track.py).

Yardstick: ReferenceData.problem_at, one rollout at a time -- the loader the repository already tests against the reference's files
(tests/test_references.py).  problem_at_starts moves rows and compares nothing numerically: every comparison is bit for bit."""
import os
import re

import numpy as np
import pytest

import reference_track_cases as rc
from conftest import ROOT, load_package

pkg = load_package()
T, N, B, KEYS = rc.T, rc.N, rc.B, rc.KEYS


def _stacked(rd, starts, step, base, follow):
    """problem_at(start + step) rollout by rollout, the six items stacked"""
    probs = [rd.problem_at(int(s) + step, N, base, follow_schedule=follow) for s in starts]
    return {k: np.concatenate([p[k] for p in probs], axis=0) for k in KEYS}


@pytest.mark.parametrize("contact_rows", [None, rc.CONTACT_ROWS, 0])
@pytest.mark.parametrize("follow", [False, True])
def test_problem_at_starts_is_problem_at_rollout_by_rollout(follow, contact_rows):
    rd, base = rc.track(contact_rows), rc.base_problem()
    rng = np.random.default_rng(7)
    hi = T - N if follow else T + 40      # follow: the last row stays inside the track; else starts past its end too
    for step in (0, 1, 3, 11):
        starts = rng.integers(0, hi - step, size=B)
        starts[:3] = (0, hi - step - 1, 101)
        got = rd.problem_at_starts(starts, step, N, base, follow_schedule=follow)
        want = _stacked(rd, starts, step, base, follow)
        for k in KEYS:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (k, step)
        assert got["N"] == N and got["Q"] is base["Q"] and got["gravity"] == base["gravity"]
        if not follow:
            assert ((starts + step + N) > T - 1).any()      # some windows clamp at row T - 1 ...
            b = int(np.argmax(starts))
            assert np.array_equal(got["x_ref"][b, -1], rd.x_ref[T - 1]) and np.array_equal(got["com_ref"][b, -1], rd.com_ref[T - 1])
    one = rd.problem_at_starts([5], 2, N, base, follow_schedule=follow)      # one entry: one set
    assert all(one[k].shape[0] == 1 and np.array_equal(one[k], rd.problem_at(7, N, base, follow_schedule=follow)[k]) for k in KEYS)


def test_the_shared_inputs_reach_the_edges():
    """what tests/test_gpu_reference_track.py asserts before it touches the GPU, checked where no GPU is needed too"""
    rd = rc.track(rc.CONTACT_ROWS)
    for follow in (False, True):
        st = rc.starts_for(follow)
        rc.check_starts_reach_the_edges(rd, st, follow)
        for step in rc.STEPS:
            p = rd.problem_at_starts(st, step, N, rc.base_problem(), follow_schedule=follow)
            if follow:      # a flag past the cut table reads 1 where the full table holds 0
                full = rc.track().problem_at_starts(st, step, N, rc.base_problem(), follow_schedule=True)
                assert ((p["stance"] == 1) & (full["stance"] == 0)).any() and (p["stance"] == 0).any()
            else:
                assert any(np.array_equal(p["x_ref"][b, -1], p["x_ref"][b, -2]) for b in range(B))


def test_index_errors_where_the_reference_throws():
    rd, base = rc.track(), rc.base_problem()
    with pytest.raises(IndexError):
        rd.problem_at_starts([0, -1], 0, N, base)
    with pytest.raises(IndexError):
        rd.problem_at_starts([0, 1], -1, N, base)
    # follow_schedule: the foot / CoM-velocity rows have no clamp -- exactly where problem_at raises
    for s in range(T - N - 4, T + 2):
        for step in (0, 2):
            try:
                rd.problem_at(s + step, N, base, follow_schedule=True); ok = True
            except IndexError:
                ok = False
            assert ok == (s + step + N < T)
            if ok:
                rd.problem_at_starts([3, s], step, N, base, follow_schedule=True)
            else:
                with pytest.raises(IndexError):
                    rd.problem_at_starts([3, s], step, N, base, follow_schedule=True)
            rd.problem_at_starts([3, s], step, N, base)      # horizon-local rows 0..N: any start will do
    # a track shorter than the horizon: the horizon-local rows already pass it
    short = rc.track()
    short.x_ref, short.u_ref, short.com_ref, short.ee_ref, short.com_vel_ref = (a[:N] for a in (rd.x_ref, rd.u_ref, rd.com_ref, rd.ee_ref, rd.com_vel_ref))
    with pytest.raises(IndexError):
        short.problem_at(0, N, base)
    with pytest.raises(IndexError):
        short.problem_at_starts([0], 0, N, base)


def test_the_new_entry_points_are_exported_and_validate_their_arguments():
    import __graft_entry__ as ge
    ge.build_library()
    from mpc_ilqr_mujoco_amd import solver as sv
    L = sv.load_library()
    names = ("ilqr_hip_set_reference_track", "ilqr_hip_clear_reference_track", "ilqr_hip_reference_track_rows", "ilqr_hip_set_track_starts",
             "ilqr_hip_window_from_track", "ilqr_hip_get_reference_windows")
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    for name in names:
        assert name in sv.EXPORTS and hasattr(L, name) and re.search(r"\bint %s\s*\(" % name, hdr), name
    assert L.ilqr_hip_reference_track_rows(None) == -1
    assert L.ilqr_hip_set_reference_track(None, 1, None, None, None, None, None, None, 0) == 1      # ILQR_ERR_ARG
    assert L.ilqr_hip_clear_reference_track(None) == 1 and L.ilqr_hip_set_track_starts(None, None, 1) == 1
    assert L.ilqr_hip_window_from_track(None, 0, 0) == 1 and L.ilqr_hip_get_reference_windows(None, None, None, None, None, None, None) == 1
    for method in ("set_reference_track", "clear_reference_track", "set_track_starts", "window_from_track", "reference_windows"):
        assert callable(getattr(sv.BatchedILQR, method))


def test_runner_refuses_device_refs_without_the_resident_plant():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml

    class Handle:
        N = N

        def enable_profiling(self, on):
            pass
    rd, base = rc.track(), rc.base_problem()
    with pytest.raises(ValueError):
        ml.MPCRunner(Handle(), rd, base, device_refs=True)
    with pytest.raises(ValueError):
        ml.MPCRunner(Handle(), rd, base, resident=True, track_starts=[0])
    run = ml.MPCRunner(Handle(), rd, base, resident=True, device_refs=True, track_starts=np.arange(4))
    assert run.device_refs and np.array_equal(run.track_starts, np.arange(4))
    assert np.array_equal(ml.MPCRunner(Handle(), rd, base, resident=True, device_refs=True).track_starts, [0])
