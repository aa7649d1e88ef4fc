"""The builders of the handle walks (handle_walk_cases.py) on the CPU: they guard test_gpu_handle_walk.py against vacuity.

  * coverage:        every transition of the table is visited by the directed sequences and the seeded walks between them, every two-valued
                     one in both directions, every observation kind is used, and every sequence replays as legal -- computed from the sequences.
  * discrimination:  with the oracle alone.  For every transition that is meant to change the result and that oracle_lib can state, the
                     oracle's cold solve from the walk's start under the configuration before and after differs in final cost by more than
                     1e-6 relative (DISCRIMINATION_MARGIN: a condition on the inputs, far above the 1e-9 .. 1e-13 at which the device matches
                     the oracle) in EVERY one of the six sampled rollouts, two per k_control workgroup (odd rollouts, which start past a
                     joint limit, and none a multiple of three, whose references and schedule are the same in one set and in B sets).
                     Where a transition did not reach the margin the inputs were changed: forward differences at 1e-2, the wide tolerance
                     at 500, the iteration-control transitions held at contact mode 2 under the low gravity, where the rollouts keep improving.
  * recipe:          the setter sequence that brings a fresh handle to a configuration holds one set_problem and one call per field that
                     differs from what ilqr_hip_create leaves, nothing else -- on the call lists of a recording stand-in for BatchedILQR."""
import numpy as np
import pytest

import handle_walk_cases as hw


class _CRecorder:
    """stand-in for the ctypes library of a handle: every entry point answers ILQR_OK"""

    def __init__(self, calls):
        self._calls = calls

    def __getattr__(self, name):
        def call(*a):
            self._calls.append((name, a))
            return 0
        return call


class _Recorder:
    """stand-in for solver.BatchedILQR: records every call; the getters whose results a transition hands on answer with arrays of the right count"""

    def __init__(self, nb):
        self.calls, self.B, self.N, self.h = [], nb, hw.N, None
        self.L = _CRecorder(self.calls)

    def _chk(self, rc):
        assert rc == 0

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def call(*a, **k):
            self.calls.append((name, a, k))
            return {"linearization": (np.zeros(1), np.zeros(1)), "quadratics": (np.zeros(1),) * 4}.get(name)
        return call

    def names(self):
        return [c[0] for c in self.calls]


def test_every_transition_is_visited_in_both_directions_and_every_sequence_is_legal():
    seqs = hw.all_sequences()
    got, need = hw.covered_labels(seqs), hw.required_labels()         # (replay asserts the legality of every step)
    assert not need - got, sorted(map(str, need - got))
    # every transition of the table by name as well, and nothing in a sequence that the table does not hold
    used = {step[1] for seq in seqs for step in seq if step[0] == "T"}
    assert used == set(hw.TRANSITIONS), sorted(set(hw.TRANSITIONS) ^ used)
    kinds = {step[1] for seq in seqs for step in seq if step[0] == "O"} | {"b" for seq in seqs for step in seq if step[0] == "B0"}
    assert kinds == set(hw.KINDS)
    # the directed list names every family of facts, and every name once
    fams = [f for f, _, _ in hw.directed()]
    assert set(fams) == {"cold_start_aside", "layouts", "buffers", "installed_removed", "side_work"}
    assert len({(f, n) for f, n, _ in hw.directed()}) == len(hw.directed())
    # between initialize and solve(): exactly one change in each cold-start sequence but the control
    for f, n, seq in hw.directed():
        if f == "cold_start_aside":
            i0, i1 = seq.index(("B0",)), seq.index(("B1",))
            assert i1 - i0 == (1 if n.startswith("nothing") else 2), n      # (the two controls: an empty block)
    # ... and the caller's own trajectory is among them, given to the WALKED handle between initialize and solve()
    assert any(f == "cold_start_aside" and ("T", "side:set_trajectory") in seq[seq.index(("B0",)):seq.index(("B1",))] for f, n, seq in hw.directed())
    # the backward pass alone runs directly behind a getter that converted a layout, in both layouts' getters
    for getter in ("read:quadratics", "read:linearization"):
        assert any(seq[i:i + 2] == [("T", getter), ("T", "side:stage_backward_pass")] for f, n, seq in hw.directed() if f == "layouts" for i in range(len(seq))), getter


def test_seeded_walks_are_reproducible_legal_and_observe_after_every_second_transition():
    walks = hw.random_walks()
    assert walks == hw.random_walks() and list(walks) == list(hw.WALK_SEEDS) and len(walks) == 6
    assert len({str(w) for w in walks.values()}) == len(walks)
    for seed, seq in walks.items():
        hw.replay(seq)
        assert sum(step[0] == "T" for step in seq) == hw.WALK_TRANSITIONS, seed
        # T T O  or  B0 T T B1
        run = 0
        for step in seq:
            if step[0] == "T":
                run += 1
            elif step[0] in ("O", "B1"):
                assert run == 2, (seed, step); run = 0
        assert run == 0


def test_no_sequence_holds_a_refused_combination():
    """the combinations the library refuses (test 3 of the GPU file calls them on purpose) never occur in a configuration a sequence reaches"""
    for seq in hw.all_sequences():
        for step, old, new, label in hw.replay(seq):
            assert not (new["al"] is not None and new["wsets"]), step
            assert new["mode"] != 1, step
            assert new["jac"] in (0, 1) and new["max_iter"] in hw.MAX_ITERS + (hw.ITERS,)
            if new["track"] is not None:
                stp, follow = new["track"]
                assert (hw.track_starts(hw.B).max() + stp if follow else 0) + hw.N < hw.walking_track().x_ref.shape[0]


@pytest.mark.parametrize("name", sorted(hw.DISCRIMINATING))
def test_oracle_tells_the_configurations_of_a_transition_apart(name):
    before, after = hw.discriminating_pair(name)
    assert hw.result_key(before) != hw.result_key(after)
    ca = np.array([hw.oracle_cost(before, b) for b in hw.ORACLE_ROLLOUTS])
    cb = np.array([hw.oracle_cost(after, b) for b in hw.ORACLE_ROLLOUTS])
    assert np.all(np.isfinite(ca)) and np.all(np.isfinite(cb))
    d = np.abs(ca - cb) / np.abs(ca)
    print(name, d)
    assert (d > hw.DISCRIMINATION_MARGIN).all(), (name, d)


def test_every_result_changing_transition_has_a_discriminating_base():
    """what is meant to change the result: every transition that moves result_key at some base; each has a base in DISCRIMINATING (the
    oracle states it) or GPU_ONLY_DISCRIMINATING (stance geometry and the augmented Lagrangian: fresh handles alone tell them apart)"""
    have = set(hw.DISCRIMINATING) | set(hw.GPU_ONLY_DISCRIMINATING)
    for name in have:
        a, b = hw.discriminating_pair(name)
        assert hw.result_key(a) != hw.result_key(b), name
    fields = {n.split(":")[0] for n in have}
    for name, t in hw.TRANSITIONS.items():
        f = name.split(":")[0]
        if t.step is None or f in hw.ORDER_FIELDS:
            assert f not in fields, name
        else:
            assert f in fields, name                                  # one direction of the field is held to the margin
    # the order switches leave result_key alone at every base
    for f in hw.ORDER_FIELDS:
        for name in (n for n in hw.TRANSITIONS if n.split(":")[0] == f):
            new = hw.TRANSITIONS[name].step(hw.START)
            assert new is None or hw.result_key(new) == hw.result_key(hw.START), name


def _configurations():
    """every configuration an observation of a sequence is made in, once"""
    seen = {}
    for seq in hw.all_sequences():
        cfg = None
        for step, old, new, label in hw.replay(seq):
            if step[0] in ("O", "B1"):
                seen[str(sorted(new.items(), key=str))] = new
    return list(seen.values())


def test_fresh_handle_recipe_is_the_shortest():
    cfgs = _configurations()
    assert len(cfgs) > 60
    for cfg in cfgs:
        for nb in (hw.B, hw.B_SMALL):
            r = _Recorder(nb)
            hw.recipe(r, cfg, nb)
            assert r.names() == hw.recipe_calls(cfg), (cfg, r.names())
            assert len(set(r.names())) == len(r.names())              # no call twice
    # ... and recipe_calls is minimal: one call per field that differs from the handle's defaults (grouped where one setter carries two fields)
    groups = [("mode", "soft"), ("jac", "early_exit")]
    for cfg in cfgs:
        differs = {f for f in hw.HANDLE_DEFAULT if cfg[f] != hw.HANDLE_DEFAULT[f]}
        for g in groups:
            if differs & set(g):
                differs = (differs - set(g)) | {g[0]}
        calls = hw.recipe_calls(cfg)
        n = 1                                                           # set_problem: gravity, weights, weight sets, references, schedule
        differs -= {"gravity", "refs_var", "refs_sets", "sched_var", "sched_sets", "weights", "wsets"}
        if "track" in differs:
            n += 3; differs.discard("track")
        if "al" in differs:
            al = cfg["al"]
            n += 1 + {None: 0, "table": 1, "window": 1, "cut": 3}[al["jc"]] + (al["st"] is not None) + bool(al["tk"]); differs.discard("al")
        assert len(calls) == n + len(differs), (cfg, calls)
    # the default configuration takes set_problem and the iteration count alone
    r = _Recorder(hw.B); hw.recipe(r, hw.START, hw.B)
    assert r.names() == ["set_problem", "set_max_iterations"]


def test_transitions_call_what_they_are_named_after():
    """each transition's calls on the recording stand-in: a field transition calls setters only, side work never touches a setter of the table"""
    setters = set()
    for cfg in _configurations():
        setters |= set(hw.recipe_calls(cfg))
    D = dict(hw.inputs(hw.B_SMALL), pack=(1, 2, 3))
    for seq in hw.all_sequences():
        for step, old, new, label in hw.replay(seq):
            if step[0] != "T":
                continue
            r = _Recorder(hw.B_SMALL)
            hw.TRANSITIONS[step[1]].apply(r, old, new, D)
            names = [n for n in r.names() if not n.startswith("ilqr_hip_")]
            assert r.calls, step
            if hw.TRANSITIONS[step[1]].step is None:
                assert not set(names) & setters, (step, names)


def test_start_inputs():
    D = hw.inputs(hw.B)
    assert D["x0"].shape == (40, 51) and D["ui"].shape == (40, 6, 19) and hw.inputs(hw.B_SMALL)["x0"].shape == (5, 51)
    assert np.array_equal(hw.inputs(hw.B_SMALL)["x0"], D["x0"][:5])
    assert len({r.tobytes() for r in D["x0"]}) == 40                    # no two rollouts alike
    jr = hw.ol.joint_ranges()
    th = D["x0"][:, 7:26]
    assert ((th > jr[:, 1]).any(axis=1) | (th < jr[:, 0]).any(axis=1)).sum() >= 20      # the joint-limit rows carry weight
    for sched in hw.SCHEDULES.values():
        assert sched.shape == (7, 2) and 0 < (sched == 0).sum() and (sched.sum(axis=1) > 0).all()      # swing phases, never both feet up
