"""The actuator model of the resident plant without a GPU (include/ilqr_hip.h ilqr_hip_plant_set_actuator and companions): the NumPy
restatement of the draws and of the chain delay line -> lag -> noise (tests/actuator_cases.py), the golden the GPU test reads, known
answers of the chain, the fitness of the GPU test's inputs shown on the restatement alone, the entry points' argument checks, the Python
mirrors and the runner's call order.

Bounds: the integer part exactly; moments of n = 48 640 normals |mean| < 4 / sqrt(n), |std - 1| < 4 / sqrt(2 n) (four standard errors);
the golden against the restatement that wrote it 1e-14 absolute on the draws (another libm may differ by an ulp of log / cos / sin at
r <= 8.7) and 1e-13 on the applied torque (sigma <= 2 times that, through a lag that does not amplify); the lag against 1 - exp(-k h / tau)
1e-15 (k <= 40 steps of a recursion that loses at most an ulp of a value <= 1 each).
A mutant of the chain has to move the applied torque by 1e3 x the GPU test's torque bound, 1e-12 x max(1, |t|), so by 1e-9 x max(1, |t|)."""
import ctypes as C
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import actuator_cases as ac
import observation_cases as oc
from conftest import load_package
from test_plant_cpu import NX, _base, _Recorder, _Refs

pkg = load_package()
sc = pkg.scenario
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
NAMES = ("ilqr_hip_plant_set_actuator", "ilqr_hip_plant_clear_actuator", "ilqr_hip_plant_num_actuator_sets", "ilqr_hip_plant_get_actuator",
         "ilqr_hip_plant_get_actuator_blend", "ilqr_hip_plant_actuator_draws", "ilqr_hip_plant_get_applied")
GPU_TORQUE_TOL = 1e-12
B, SUB, COUNT = ac.GOLDEN_B, ac.GOLDEN_SUBSTEPS, ac.GOLDEN_COUNT
H = ac.GOLDEN_DT / SUB


def _lib():
    import __graft_entry__ as ge
    ge.build_library()
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv, sv.load_library()


# ---- the draws
def test_draws_use_the_blocks_behind_the_observations():
    seed = ac.GOLDEN_SEED
    w = ac.words(seed, np.arange(5), np.arange(3))
    assert w.shape == (3, 5, 10, 4)
    # the same generator, the same counter form: block 32 + q of the actuator is what the observation's layout would draw at k = 32 + q
    s, i, k = np.broadcast_arrays(np.arange(5, dtype=np.uint64)[None, :, None], np.arange(3, dtype=np.uint64)[:, None, None], (32 + np.arange(10, dtype=np.uint64))[None, None, :])
    counter = np.stack([s, np.zeros_like(s), i, k], axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64), counter.shape[:-1] + (2,))
    assert np.array_equal(w, oc.philox4x32_10(counter, key))
    # disjoint from the observation's blocks 0..24 under the same seed: no normal in common
    z, zo = ac.normals(seed, np.arange(5), np.arange(3)), oc.normals(seed, np.arange(5), np.arange(3))
    assert z.shape == (3, 5, 19) and zo.shape == (3, 5, 50)
    assert not np.isin(z.ravel(), zo.ravel()).any()
    assert abs(float(np.corrcoef(z[..., :19].ravel(), zo[..., :19].ravel())[0, 1])) < 4.0 / np.sqrt(z.size)
    # joints 2q, 2q + 1 from block 32 + q; the twentieth normal is dropped
    u1, u2 = oc.uniforms(w)
    r = np.sqrt(-2.0 * np.log(u1))
    assert np.array_equal(z[..., 0::2], (r * np.cos(oc.TWO_PI * u2))) and np.array_equal(z[..., 1::2], (r * np.sin(oc.TWO_PI * u2))[..., :9])


def test_moments_of_the_normals():
    z = ac.normals(4321, np.arange(64), np.arange(40))
    n = z.size
    assert z.shape == (40, 64, 19) and n == 48640
    mean, std = float(z.mean()), float(z.std())
    print("normals: mean %.4f, std %.4f, largest |z| %.2f" % (mean, std, np.abs(z).max()))
    assert abs(mean) < 4.0 / np.sqrt(n) and abs(std - 1.0) < 4.0 / np.sqrt(2.0 * n)
    # a shard that starts at rollout 20 draws what the global batch draws; intervals likewise; another seed does not
    assert np.array_equal(ac.normals(4321, 20 + np.arange(17), np.arange(3)), z[:3, 20:37])
    assert np.array_equal(ac.draws(4321, 20, 7, 2, 17), z[7:9, 20:37])
    assert not np.array_equal(ac.normals(4322, np.arange(4), np.arange(2)), z[:2, :4])


def test_golden_is_the_restatement():
    g = ac.golden()
    rec = g["records"]
    assert rec.shape == (B, 39) and np.array_equal(rec, ac.golden_records())
    assert int(g["seed"]) == ac.GOLDEN_SEED and int(g["stream0"]) == 0 and int(g["interval0"]) == 0 and int(g["count"]) == COUNT and int(g["substeps"]) == SUB
    # what the issue asks of the records: delays below, at and above an interval; the four time constants mixed per joint; sigma 0 up to 2
    assert set(rec[:, 0]) == {0.0, 1.0, 2.0, 3.0, 4.0, 8.0} and set(np.unique(rec[:, 1:20])) == {0.0, 0.005, 0.02, 0.08}
    assert rec[:, 20:].min() == 0.0 and rec[:, 20:].max() == 2.0 and ((rec[:, 1:20] > 0).any(axis=1) & (rec[:, 1:20] == 0).any(axis=1)).sum() >= 20
    assert np.array_equal(ac.words(ac.GOLDEN_SEED, np.arange(B), [0])[0], g["words0"].astype(np.uint64))      # the integer part: exactly
    z = ac.draws(ac.GOLDEN_SEED, 0, 0, COUNT, B)
    beta = ac.blend(rec, H)
    t = ac.run_chain(rec, beta, g["commands"], g["z"], SUB)
    print("golden against this machine's restatement: z %.2e, beta %.2e, applied %.2e" % (np.abs(z - g["z"]).max(), np.abs(beta - g["beta"]).max(), np.abs(t - g["applied"]).max()))
    assert np.abs(z - g["z"]).max() < 1e-14 and np.abs(beta - g["beta"]).max() < 1e-15 and np.abs(t - g["applied"]).max() < 1e-13
    assert np.array_equal(g["commands"], ac.synthetic_commands(COUNT * SUB, B))


# ---- known answers of the chain
def test_a_zero_record_maps_a_command_sequence_to_itself_bit_for_bit():
    c = ac.synthetic_commands(27, B)
    z = ac.draws(5, 0, 0, 9, B)
    for rec in (np.zeros((1, 39)), np.zeros((B, 39))):
        with warnings.catch_warnings():
            warnings.simplefilter("error")                                  # beta for tau = 0 is never computed: no division by zero
            beta = ac.blend(rec, H)
        assert np.all(beta == 1.0)
        assert np.array_equal(ac.run_chain(rec, beta, c, z, 3), c)
    # ... whatever the beta row holds: the chain selects, it does not multiply
    assert np.array_equal(ac.run_chain(np.zeros((1, 39)), np.full((1, 19), np.nan), c, z, 3), c)
    # the guard acts in front of the delay line: a command with one non-finite entry enters as zeros, and comes out as zeros `delay` substeps later
    rec = np.zeros((1, 39)); rec[0, 0] = 2.0
    cb = c.copy(); cb[4, 7, 3] = np.inf; cb[5, 9, 0] = np.nan
    t = ac.run_chain(rec, ac.blend(rec, H), cb, z, 3)
    assert np.all(t[6, 7] == 0.0) and np.all(t[7, 9] == 0.0) and np.all(np.isfinite(t))
    keep = np.ones((27, B), dtype=bool); keep[6, 7] = keep[7, 9] = False
    want = np.concatenate([np.repeat(c[:1], 2, axis=0), c[:-2]])           # primed with c_0: the first two substeps still apply it
    assert np.array_equal(t[keep], want[keep])


def test_a_constant_command_is_a_fixed_point_without_noise():
    rec = ac.golden_records(); rec[:, 20:] = 0.0
    c = np.repeat(ac.synthetic_commands(1, B), 30, axis=0)
    t = ac.run_chain(rec, ac.blend(rec, H), c, np.zeros((10, B, 19)), 3)
    assert np.array_equal(t, c)                                             # primed with c_0: delay line, lag and output hold it exactly
    # with noise the output is the command plus sigma z of the interval, held over its substeps
    rec = ac.golden_records()
    z = ac.draws(9, 0, 0, 10, B)
    t = ac.run_chain(rec, ac.blend(rec, H), c, z, 3)
    assert np.array_equal(t, c + np.repeat(rec[None, :, 20:] * z, 3, axis=0)) and np.array_equal(t[0], t[2]) and not np.array_equal(t[2], t[3])


def test_the_lag_follows_the_exponential_against_a_step_command():
    taus = np.array([0.005, 0.02, 0.08])
    rec = np.zeros((3, 39)); rec[:, 1:20] = taus[:, None]
    c = np.zeros((41, 3, 19)); c[1:] = 1.0                                  # primed at 0, then a unit step
    t = ac.run_chain(rec, ac.blend(rec, H), c, np.zeros((14, 3, 19)), 3)
    k = np.arange(41)[:, None, None]
    want = -np.expm1(-k * H / taus[None, :, None])
    err = float(np.abs(t - want).max())
    print("lag against 1 - exp(-k h / tau): worst error %.2e (bound 1e-15)" % err)
    assert err < 1e-15
    # a delay shifts the response by whole substeps
    rec[:, 0] = 4.0
    td = ac.run_chain(rec, ac.blend(rec, H), c, np.zeros((14, 3, 19)), 3)
    assert np.array_equal(td[4:], t[:-4]) and np.all(td[:5] == 0.0)


# ---- fitness of the GPU test's inputs, on the restatement alone
@pytest.mark.parametrize("hold", [1, SUB])
def test_every_mutant_of_the_chain_moves_the_applied_torque_of_the_gpu_records(hold):
    """The records of the GPU test (golden_records), six intervals of three substeps, under a synthetic command that changes in every substep
    (feedback mode 1) or in every interval (mode 0): each wrong chain moves at least 25 of the 37 rollouts, one in every group of four."""
    rec = ac.golden_records()
    beta = ac.blend(rec, H)
    c = ac.synthetic_commands(COUNT * SUB, B, hold=hold)
    z = ac.draws(ac.GOLDEN_SEED, 0, 0, COUNT, B)
    t = ac.run_chain(rec, beta, c, z, SUB)
    smallest = np.inf
    for mutant in ac.MUTANTS:
        tm = ac.run_chain(rec, beta, c, z, SUB, mutant=mutant, seed=ac.GOLDEN_SEED)
        factor = (np.abs(tm - t) / (GPU_TORQUE_TOL * np.maximum(1.0, np.abs(t)))).max(axis=(0, 2))      # per rollout, in units of the GPU bound
        moved = factor >= 1e3
        groups = [bool(moved[k:k + 4].any()) for k in range(0, B, 4)]
        print("hold %d, %-18s moves %2d rollouts, smallest factor among them %.2e" % (hold, mutant, moved.sum(), factor[moved].min()))
        assert moved.sum() >= 25 and all(groups), (mutant, int(moved.sum()), groups)
        smallest = min(smallest, float(factor[moved].min()))
    print("hold %d: smallest factor over all mutants %.2e x the GPU torque bound" % (hold, smallest))


# ---- host logic
def test_stack_plant_actuator_broadcasts_and_validates():
    a = sc.stack_plant_actuator(4)
    assert a.shape == (4, 39) and a.dtype == np.float64 and np.array_equal(a, np.zeros((4, 39)))
    a = sc.stack_plant_actuator(4, delay=[0, 1, 2, 8], tau=0.02, sigma=np.arange(19) * 0.1)
    assert np.array_equal(a[:, 0], (0, 1, 2, 8)) and np.all(a[:, 1:20] == 0.02) and np.array_equal(a[:, 20:], np.tile(np.arange(19) * 0.1, (4, 1)))
    a = sc.stack_plant_actuator(4, delay=3, tau=[0.0, 0.005, 0.02, 0.08], sigma=np.full((4, 19), 0.5))
    assert np.all(a[:, 0] == 3) and np.array_equal(a[:, 1:20], np.repeat([[0.0], [0.005], [0.02], [0.08]], 19, axis=1)) and np.all(a[:, 20:] == 0.5)
    assert sc.stack_plant_actuator(19, tau=np.arange(19.0))[3, 1:20].tolist() == list(range(19))      # B == 19: a vector is read per joint
    for kw in (dict(delay=9), dict(delay=1.5), dict(delay=-1), dict(delay=[0, 1]), dict(tau=-1e-9), dict(sigma=-0.1), dict(tau=np.nan), dict(sigma=np.inf), dict(delay=np.nan),
               dict(tau=np.zeros(3)), dict(sigma=np.zeros((3, 19))), dict(tau=np.zeros((4, 19, 1)))):
        with pytest.raises(ValueError):
            sc.stack_plant_actuator(4, **kw)
    with pytest.raises(ValueError):
        sc.stack_plant_actuator(0)


def test_actuator_entry_points_refuse_bad_arguments_before_they_touch_the_handle():
    sv, L = _lib()
    good = [0.0] * 39
    for fn in NAMES:
        assert hasattr(L, fn)
    rec = (C.c_double * 39)(*good)
    buf = (C.c_double * (39 * 37))()
    seed, s0 = C.c_ulonglong(1), C.c_ulonglong(0)
    assert L.ilqr_hip_plant_set_actuator(None, rec, 1, seed, s0) == ERR_ARG
    assert L.ilqr_hip_plant_clear_actuator(None) == ERR_ARG
    assert L.ilqr_hip_plant_num_actuator_sets(None) == -1
    assert L.ilqr_hip_plant_get_actuator(None, buf, None, None) == ERR_ARG
    assert L.ilqr_hip_plant_get_actuator_blend(None, buf) == ERR_ARG
    assert L.ilqr_hip_plant_actuator_draws(None, C.c_long(0), 1, buf) == ERR_ARG
    assert L.ilqr_hip_plant_get_applied(None, buf) == ERR_ARG
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    assert L.ilqr_hip_plant_set_actuator(h, None, 1, seed, s0) == ERR_ARG
    for n_sets in (0, -1, 2, 37):                                           # neither 1 nor the batch (0 on this handle, and 0 sets is no table)
        assert L.ilqr_hip_plant_set_actuator(h, buf, n_sets, seed, s0) == ERR_ARG, n_sets
    # a delay that is no integer in 0..8, a negative tau or sigma, a non-finite entry anywhere
    for col, v in ((0, 9.0), (0, 1.5), (0, -1.0), (0, np.nan), (0, np.inf), (1, -1e-300), (19, -0.02), (20, -1e-300), (38, -2.0), (7, np.nan), (30, np.inf), (38, -np.inf)):
        r = list(good); r[col] = v
        assert L.ilqr_hip_plant_set_actuator(h, (C.c_double * 39)(*r), 1, seed, s0) == ERR_ARG, (col, v)
    assert L.ilqr_hip_plant_get_actuator(h, None, None, None) == ERR_ARG
    assert L.ilqr_hip_plant_get_actuator_blend(h, None) == ERR_ARG
    assert L.ilqr_hip_plant_num_actuator_sets(h) == 0                       # no table on the zeroed handle
    for i0, count, out in ((0, 0, buf), (0, -2, buf), (-1, 1, buf), (0, 1, None), (0, 1, buf)):      # (the zeroed handle has N = 0: every count exceeds it)
        assert L.ilqr_hip_plant_actuator_draws(h, C.c_long(i0), count, out) == ERR_ARG, (i0, count)
    assert L.ilqr_hip_plant_get_applied(h, None) == ERR_ARG


def test_header_and_wrappers_declare_the_feature():
    from mpc_ilqr_mujoco_amd import solver as sv
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\s*\(", hdr, re.M), name
    assert all(name in sv.EXPORTS for name in NAMES)
    assert re.search(r"^#define\s+ILQR_PLANT_ACTUATOR\s+39\b", hdr, re.M) and sv.PLANT_ACTUATOR == 39
    assert re.search(r"^#define\s+ILQR_PLANT_ACTUATOR_MAX_DELAY\s+8\b", hdr, re.M) and sv.PLANT_ACTUATOR_MAX_DELAY == 8 == ac.MAX_DELAY
    hpp = open(os.path.join(ROOT, "include", "ilqr_hip.hpp")).read()
    assert all(m in hpp for m in ("plantSetActuator", "plantClearActuator", "plantNumActuatorSets", "plantActuator", "plantActuatorBlend", "plantActuatorDraws", "plantApplied"))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integ for name in NAMES)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ilqr_hip_plant_set_actuator" in design and "k_plant_follow_a" in design and "k_actuator_draw" in design
    # a dry run (nothing is compiled): what builds the module compiles plant_kernels.hip with the module's macro
    mk = subprocess.run(["make", "-n", "-B", "../lib/libilqr_hip_actuator.so"], cwd=os.path.join(ROOT, "mpc-ilqr-mujoco_amd", "csrc"), capture_output=True, text=True)
    assert mk.returncode == 0, mk.stderr
    assert any("plant_kernels.hip" in line and "-DPLANT_ACTUATOR_MODULE" in line for line in mk.stdout.splitlines()), mk.stdout
    s = sv.BatchedILQR.__new__(sv.BatchedILQR)      # no handle: the shape checks fail before the library is reached
    s.B, s.N, s.h = 3, 25, None
    for bad in (np.ones(38), np.ones((2, 39)), np.ones((3, 40)), np.ones((1, 3, 39))):
        with pytest.raises(ValueError):
            s.plant_set_actuator(bad)
    for seed, stream0 in ((-1, 0), (1 << 64, 0), (0, -1), (0, 1 << 64)):
        with pytest.raises(ValueError):
            s.plant_set_actuator(np.zeros((3, 39)), seed=seed, stream0=stream0)
    for i0, count in ((-1, 1), (0, 0), (0, 26)):
        with pytest.raises(ValueError):
            s.plant_actuator_draws(i0, count)


def test_the_built_modules_export_their_entry_points():
    sv, L = _lib()
    path = os.path.join(os.path.dirname(sv.LIB_PATH), "libilqr_hip_actuator.so")
    assert os.path.exists(path), path
    M = C.CDLL(path)
    for name in ("ilqr_actuator_module_set_attr", "ilqr_actuator_module_follow", "ilqr_actuator_module_draw"):
        assert hasattr(M, name), name


class _ActuatorRecorder(_Recorder):
    def plant_set_observation(self, observation, seed=0, stream0=0):
        self._rec("plant_set_observation(%d,%d,%d)" % (len(observation), seed, stream0))

    def plant_get_observed(self):
        self._rec("plant_get_observed")
        return np.zeros((self.B, NX))

    def plant_set_actuator(self, actuator, seed=0, stream0=0):
        self._rec("plant_set_actuator(%d,%d,%d)" % (len(actuator), seed, stream0))


def test_runner_refuses_without_the_resident_plant_and_installs_in_order():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    Bn, Nn = 3, 25
    a = sc.stack_plant_actuator(Bn, delay=[0, 2, 4], tau=0.02)
    o = sc.stack_plant_observation(Bn, joints_noise=0.002)
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(_ActuatorRecorder(Bn, Nn), _Refs(Nn), _base(Nn), plant_actuator=a)
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(_ActuatorRecorder(Bn, Nn), _Refs(Nn), _base(Nn), plant_actuator=a, resident=False)
    for bad in (np.ones((2, 39)), np.ones((Bn, 38)), np.ones((1, Bn, 39))):
        with pytest.raises(ValueError):
            ml.MPCRunner(_ActuatorRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_actuator=bad)
    s = _ActuatorRecorder(Bn, Nn)
    run = ml.MPCRunner(s, _Refs(Nn), _base(Nn), resident=True, substeps=3, plant_observation=o, observation_seed=7, plant_actuator=a, actuator_seed=77, actuator_stream0=5)
    run.run(np.zeros((Bn, NX)), 2)
    head = ["plant_configure(3,0,schedule)", "plant_set_observation(3,7,0)", "plant_set_actuator(3,77,5)", "plant_set_history(2)", "plant_reset"]
    assert s.calls[:5] == head, s.calls
    assert s.calls.count("plant_advance") == 2
    s = _ActuatorRecorder(Bn, Nn)
    ml.MPCRunner(s, _Refs(Nn), _base(Nn), resident=True).run(np.zeros((Bn, NX)), 2)
    assert not any(c.startswith("plant_set_actuator") for c in s.calls)
    one = ml.MPCRunner(_ActuatorRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_actuator=a[1])      # one record, given as a vector
    assert one.plant_actuator.shape == (1, 39)
