"""Solve groups without a GPU (include/ilqr_hip.h ilqr_hip_set_groups ...): the NumPy restatement of the selection rule and of the perturbation
(tests/group_ref.py) on constructed inputs, the scenario helpers, the refusals of MPCRunner, the boundary (header, exports, documents, build
rules) -- and the inputs of the GPU tests of the incumbent and of the adoption (tests/test_gpu_groups.py), whose winners the CPU oracle fixes here
with a margin no GPU rounding reaches."""
import os
import re
import subprocess

import numpy as np
import pytest

import group_cases as gc
import group_ref as gr
import observation_cases as oc
from conftest import ROOT, load_package

pkg = load_package()
sc = pkg.scenario
NU = 19
NAMES = ("ilqr_hip_set_groups", "ilqr_hip_num_groups", "ilqr_hip_group_set_perturbation", "ilqr_hip_group_clear_perturbation", "ilqr_hip_group_draws",
         "ilqr_hip_group_perturb", "ilqr_hip_group_select", "ilqr_hip_group_get_winners", "ilqr_hip_group_winners_device", "ilqr_hip_group_adopt")


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- the selection rule
@pytest.mark.parametrize("G", [1, 2, 3, 5, 8, 64, 70])
def test_select_rule_on_constructed_keys(G):
    cases = dict(gc.select_cases(G))
    base = cases["distinct"]
    for name, k in cases.items():
        (w,), (rec,) = gr.select(k, G)
        fin = np.isfinite(k)
        # the rule, stated independently of gr.select: no finite key -> member 0; else the first position of the smallest finite key
        want = 0 if not fin.any() else int(np.flatnonzero(fin & (k == k[fin].min()))[0])
        assert w == want, (G, name)
        assert _same(rec, [k[want], k[0], fin.sum(), k[fin].max() if fin.any() else np.nan]), (G, name)
    assert gr.select(cases["tie_all"], G)[0][0] == 0 and gr.select(cases["all_nan"], G)[0][0] == 0 and gr.select(cases["no_finite_key_mixed"], G)[0][0] == 0
    assert np.isnan(gr.select(cases["all_nan"], G)[1][0, 3]) and gr.select(cases["all_nan"], G)[1][0, 2] == 0
    if G >= 2:
        assert gr.select(cases["tie_first_last"], G)[0][0] == 0 and gr.select(cases["tie_last_two"], G)[0][0] == G - 2
        assert gr.select(cases["one_finite_key_last"], G)[0][0] == G - 1                       # -inf never wins
        assert gr.select(cases["signed_zeros_tie"], G)[0][0] == 0                              # 0.0 == -0.0: the lower member
        for p in range(G):                                                                       # a NaN in every position: never the winner, never counted
            (w,), (rec,) = gr.select(cases["nan_at_%d" % p], G)
            assert w != p and rec[2] == G - 1
        lo = int(np.argmin(base))
        assert gr.select(cases["nan_on_the_minimum"], G)[0][0] == int(np.argsort(base)[1]) != lo
    if G >= 3:
        assert gr.select(cases["tie_middle"], G)[0][0] == G // 2
    # groups are independent and the winner is a GLOBAL index: the cases side by side
    keys = np.concatenate([k for k in cases.values()])
    w, rec = gr.select(keys, G)
    for i, k in enumerate(cases.values()):
        (w1,), (r1,) = gr.select(k, G)
        assert w[i] == i * G + w1 and _same(rec[i], r1)
    # every batch of the GPU test holds whole cases
    for B, Gs in gc.SHAPES:
        if Gs == G:
            bs = gc.select_batches(B, G)
            assert all(b.shape == (B,) for b in bs) and len(bs) * (B // G) >= len(cases)


# ---- the perturbation
def test_perturbation_restatement():
    assert all(np.array_equal(oc.philox4x32_10(np.array(c), np.array(k)), np.array(w)) for c, k, w in oc.KNOWN_ANSWERS)      # (the generator it rests on)
    B, N, G, seed, stream0 = 24, 7, 4, 0xA5A5_0000_1234_5678, (1 << 33) + 5
    sigma = sc.stack_group_sigma(G, np.linspace(0.5, 2.0, NU))
    d0 = gr.perturbation(B, N, G, sigma, 1, seed, stream0, 0)
    assert d0.shape == (B, N, NU) and np.all(d0[0::G] == 0.0) and np.all(d0[np.arange(B) % G != 0] != 0.0)      # member 0 untouched, every other entry moved
    # the layout of the sequence: normal i = (t // hold) 19 + j of stream stream0 + b under the draw counter, z[2k], z[2k + 1] from block k
    z = gr.normals(B, N * NU, seed, stream0, 0)
    b, t, j = 5, 3, 11
    assert d0[b, t, j] == sigma[b % G, j] * z[b, t * NU + j]
    s = stream0 + b
    blk = (t * NU + j) // 2
    words = oc.philox4x32_10(np.array([s & 0xFFFFFFFF, s >> 32, 0, blk]), np.array([seed & 0xFFFFFFFF, seed >> 32]))
    u1, u2 = oc.uniforms(words)
    pair = np.sqrt(-2.0 * np.log(u1)) * np.array([np.cos(oc.TWO_PI * u2), np.sin(oc.TWO_PI * u2)])
    assert z[b, t * NU + j] == pair[(t * NU + j) % 2]
    # the observation model's stream with the draw counter in the interval's place: the same normals where both define them
    assert np.array_equal(gr.normals(B, 50, seed, stream0, 3), oc.normals(seed, stream0 + np.arange(B), [3])[0])
    # hold repeats a segment's draw; the last segment may be short
    d3 = gr.perturbation(B, N, G, sigma, 3, seed, stream0, 0)
    assert np.array_equal(d3[:, 0], d3[:, 1]) and np.array_equal(d3[:, 1], d3[:, 2]) and np.array_equal(d3[:, 3], d3[:, 5]) and not np.array_equal(d3[:, 2], d3[:, 3])
    assert np.array_equal(d3[:, 0], d0[:, 0]) and np.array_equal(d3[:, 3], d0[:, 1]) and np.array_equal(d3[:, 6], d0[:, 2])
    # two calls differ and are reproducible from the draw counter
    d1 = gr.perturbation(B, N, G, sigma, 1, seed, stream0, 1)
    assert not np.array_equal(d1, d0) and np.array_equal(d1, gr.perturbation(B, N, G, sigma, 1, seed, stream0, 1))
    u = np.random.default_rng(3).uniform(-50, 50, (B, N, NU))
    twice = gr.perturbed(gr.perturbed(u, G, sigma, 1, seed, stream0, 0), G, sigma, 1, seed, stream0, 1)
    assert np.array_equal(twice, (u + d0) + d1) and np.array_equal(twice[0::G], u[0::G])
    # one row serves every member g >= 1; the streams still differ per rollout
    one = gr.perturbation(B, N, G, sigma[1:2], 1, seed, stream0, 0)
    assert np.array_equal(one[1::G], d0[1::G]) and np.all(one[0::G] == 0.0) and not np.array_equal(one[1], one[2])
    # a batch is its halves with stream0 moved on: G divides the split
    assert np.array_equal(gr.perturbation(B // 2, N, G, sigma, 1, seed, stream0 + B // 2, 0), d0[B // 2:])
    # unit variance, roughly: 24 x 7 x 19 x 3 / 4 draws
    zz = gr.normals(64, 400, seed, 0, 0)
    assert abs(zz.mean()) < 0.03 and abs(zz.std() - 1.0) < 0.03


def test_stack_group_sigma_and_repeat_for_groups():
    s = sc.stack_group_sigma(5, 0.5)
    assert s.shape == (5, NU) and np.all(s[0] == 0.0) and np.array_equal(s[1:, 0], 0.5 * 2.0 ** np.arange(4))      # geometric by default
    base = np.linspace(0.1, 1.9, NU)
    s = sc.stack_group_sigma(4, base, ladder=[1.0, 3.0, 0.0])
    assert np.all(s[0] == 0.0) and np.array_equal(s[1], base) and np.array_equal(s[2], 3.0 * base) and np.all(s[3] == 0.0)
    assert sc.stack_group_sigma(1, 2.0).shape == (1, NU) and np.all(sc.stack_group_sigma(1, 2.0) == 0.0)
    for bad in (dict(G=0, base=1.0), dict(G=3, base=1.0, ladder=[1.0]), dict(G=3, base=-1.0), dict(G=2, base=np.nan)):
        with pytest.raises(ValueError):
            sc.stack_group_sigma(**bad)
    table = np.arange(3 * 7, dtype=np.float64).reshape(3, 7)                                   # a per-rollout table
    r = sc.repeat_for_groups(table, 4)
    assert r.shape == (12, 7) and r.flags["C_CONTIGUOUS"] and all(np.array_equal(r[m * 4 + g], table[m]) for m in range(3) for g in range(4))
    window = np.random.default_rng(0).uniform(-1, 1, (2, 6, 2, 3))                              # a stacked window (foot references)
    r = sc.repeat_for_groups(window, 3)
    assert r.shape == (6, 6, 2, 3) and np.array_equal(r[0], r[2]) and np.array_equal(r[3], window[1]) and not np.array_equal(r[2], r[3])
    st = np.array([[[1, 1], [1, 0]], [[0, 1], [1, 1]]], dtype=np.int32)
    assert sc.repeat_for_groups(st, 2).dtype == np.int32 and np.array_equal(sc.repeat_for_groups(st, 1), st)
    with pytest.raises(ValueError):
        sc.repeat_for_groups(table, 0)


# ---- the runner
class _Handle:
    """what MPCRunner's constructor reads of a solver"""
    B, N = 8, 6

    def enable_profiling(self, on):
        pass


def test_mpc_runner_refuses_starts_where_the_members_of_a_group_would_differ():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    base = dict(dt=0.02)
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(_Handle(), None, base, starts=4, start_sigma=0.0)                          # the host-plant path
    for table in (dict(plant_observation=np.zeros((1, 100))), dict(plant_actuator=np.zeros((1, 39)))):
        with pytest.raises(ValueError, match="per rollout"):
            ml.MPCRunner(_Handle(), None, base, resident=True, starts=4, start_sigma=0.0, **table)
    for bad in (dict(starts=3, start_sigma=0.0), dict(starts=0), dict(starts=4), dict(starts=4, start_sigma=np.zeros((3, NU))), dict(starts=4, start_sigma=1.0, start_hold=0)):
        with pytest.raises(ValueError):
            ml.MPCRunner(_Handle(), None, base, resident=True, **bad)
    r = ml.MPCRunner(_Handle(), None, base, resident=True, starts=4, start_sigma=0.5, start_hold=2, start_seed=9)
    assert r.starts == 4 and r.start_sigma.shape == (1, NU) and np.all(r.start_sigma == 0.5) and (r.start_hold, r.start_seed) == (2, 9) and r.winners is None
    r = ml.MPCRunner(_Handle(), None, base, resident=True, starts=4, start_sigma=sc.stack_group_sigma(4, 0.5))
    assert r.start_sigma.shape == (4, NU)
    r = ml.MPCRunner(_Handle(), None, base, plant_observation=None)                           # starts absent: nothing asked, nothing refused
    assert r.starts == 1 and r.start_sigma is None
    # starts = 1 or absent: exactly the calls of a runner without it
    from test_plant_cpu import NX, _base, _Recorder, _Refs
    calls = []
    for kw in (dict(), dict(starts=1), dict(starts=1, start_sigma=2.0)):
        rec = _Recorder(3, 25)
        run = ml.MPCRunner(rec, _Refs(25), _base(25), resident=True, **kw)
        run.run(np.zeros((3, NX)), 3)
        assert run.winners is None and not any("group" in c for c in rec.calls)
        calls.append(rec.calls)
    assert calls[0] == calls[1] == calls[2] and calls[0].count("plant_advance") == 3


# ---- the inputs of the GPU tests, fixed on the oracle
def test_oracle_fixes_the_winners_of_the_gpu_tests():
    """GPU test 3 (perturbed starts, tests/group_cases.py incumbent_*) and GPU test 4 (designed starts, adopt_*), N = 6 and N = 5: on the oracle at
    least one group's winner is not member 0 and at least one group's is, and within every group the best and the second-best key differ by more
    than 1e-6 relative -- here by more than gc.MARGIN = 1e-3, so that no GPU rounding changes a winner."""
    keys = gc.incumbent_oracle_keys()
    w, rec = gr.select(keys, gc.INC_G)
    member = w - np.arange(len(w)) * gc.INC_G
    print("incumbent case: winners' members %s, margins %s" % (member, gc.margins(keys, gc.INC_G)))
    assert np.all(np.isfinite(keys)) and (member != 0).any() and (member == 0).any()
    assert gc.margins(keys, gc.INC_G).min() > gc.MARGIN > 1e-6
    assert np.all(rec[:, 0] <= rec[:, 1])
    for N in gc.HORIZONS:
        keys = gc.adopt_oracle_keys(N)
        w, _ = gr.select(keys, gc.ADOPT_G)
        member = w - np.arange(len(w)) * gc.ADOPT_G
        print("adopt case N = %d: winners' members %s, margins %s" % (N, member, gc.margins(keys, gc.ADOPT_G)))
        assert np.array_equal(member, [gc.good_member(m) for m in range(len(w))])               # the designed start wins, at another member in every group
        assert np.all(np.isfinite(keys)) and (member != 0).any() and (member == 0).any() and len(set(member)) == len(member)
        assert gc.margins(keys, gc.ADOPT_G).min() > gc.MARGIN > 1e-6
        x0, ui = gc.adopt_starts(N)
        xg = gc.adopt_trajectory(N)                                                              # what set_trajectory is given: the rollout of the controls
        assert xg.shape == (gc.ADOPT_B, N + 1, 51) and np.all(np.isfinite(xg)) and np.array_equal(xg[:, 0], x0) and not np.array_equal(xg[:, 1], xg[:, 0])
        assert all(np.array_equal(x0[m * gc.ADOPT_G + g], x0[m * gc.ADOPT_G]) for m in range(len(w)) for g in range(gc.ADOPT_G))      # one x0 per group


# ---- the boundary
def test_groups_are_declared_exported_documented_and_built():
    from mpc_ilqr_mujoco_amd import solver as sv
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    for n in NAMES:
        assert re.search(r"^(int|long) %s\(" % n, hdr, re.M), n
        assert n in sv.EXPORTS, n
    assert "int ilqr_hip_group_set_perturbation(ilqr_hip_ctx* ctx, int n_sets, const double* sigma /*[n_sets][19]*/, int hold, unsigned long long seed, unsigned long long stream0);" in hdr
    for m in ("set_groups", "num_groups", "group_set_perturbation", "group_clear_perturbation", "group_draws", "group_perturb", "group_select", "group_winners", "group_adopt"):
        assert callable(getattr(sv.BatchedILQR, m)), m
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(n in integ for n in NAMES)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert all(k in design for k in ("k_group_adopt", "k_group_select", "k_group_perturb", "ilqr_hip_group_adopt", "xbar_rolled", "lxx_layout", "ab_packed"))
    assert "ilqr_hip_set_groups" in open(os.path.join(ROOT, "README.md")).read()
    assert os.path.exists(os.path.join(ROOT, "docs", "KERNEL_RESOURCES_GROUPS.md"))
    # a dry run (nothing is compiled): the module is built from group_kernels.hip alone, beside the library, and belongs to the default target
    csrc = os.path.join(ROOT, "mpc-ilqr-mujoco_amd", "csrc")
    dry = subprocess.run(["make", "-n", "-B", "-C", csrc, "../lib/libilqr_hip_groups.so"], capture_output=True, text=True).stdout
    assert "-c group_kernels.hip" in dry and "-ffp-contract=on" in dry and "libilqr_hip_groups.so" in dry and "ilqr_kernels.hip" not in dry
    assert "libilqr_hip_groups.so" in subprocess.run(["make", "-n", "-B", "-C", csrc], capture_output=True, text=True).stdout
