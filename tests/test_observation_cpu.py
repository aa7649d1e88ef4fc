"""The observation model of the resident plant without a GPU (include/ilqr_hip.h ilqr_hip_plant_set_observation and companions): the NumPy
restatement of the generator (tests/observation_cases.py) against the published Philox4x32-10 vectors, the moments of its normals, the
structure of the error rows, the golden the GPU test reads, the entry points' argument checks, the Python mirrors and the runner's call
order.

Bounds: the integer part exactly; moments of n = 128 000 normals |mean| < 4 / sqrt(n), |std - 1| < 4 / sqrt(2 n) (four standard errors);
delta.quat unit to 1e-15; the golden against the restatement that wrote it 1e-14 absolute (another libm may differ by an ulp of log / cos /
sin at r <= 8.7)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import observation_cases as oc
from conftest import load_package
from test_plant_cpu import NX, _base, _Recorder, _Refs

pkg = load_package()
sc = pkg.scenario
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
NAMES = ("ilqr_hip_plant_set_observation", "ilqr_hip_plant_clear_observation", "ilqr_hip_plant_num_observation_sets", "ilqr_hip_plant_get_observation",
         "ilqr_hip_plant_observation_errors", "ilqr_hip_plant_get_observed")


def _lib():
    import __graft_entry__ as ge
    ge.build_library()
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv, sv.load_library()


# ---- the generator
def test_restatement_reproduces_the_published_philox_vectors():
    for counter, key, want in oc.KNOWN_ANSWERS:
        got = oc.philox4x32_10(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert [int(w) for w in got] == list(want), (counter, key, [hex(int(w)) for w in got])
    # vectorised over leading axes as the draws use it: the same words
    cs = np.array([k[0] for k in oc.KNOWN_ANSWERS], dtype=np.uint64)
    ks = np.array([k[1] for k in oc.KNOWN_ANSWERS], dtype=np.uint64)
    assert np.array_equal(oc.philox4x32_10(cs, ks), np.array([k[2] for k in oc.KNOWN_ANSWERS], dtype=np.uint64))


def test_uniforms_stay_inside_the_open_interval_and_are_exact():
    w = np.array([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF], [0, 0x800, 0x40000000, 0]], dtype=np.uint64)
    u1, u2 = oc.uniforms(w)
    assert u1[0] == 2.0 ** -54 and u1[1] == 1.5 * 2.0 ** -53 and u2[1] == 0.25 + 2.0 ** -54
    assert 0.0 < u1.min() and u2[0] <= 1.0 and np.isfinite(np.sqrt(-2.0 * np.log(u2[0])))        # the largest word pair: log(u) is 0, not positive


def test_moments_of_the_normals():
    z = oc.normals(1234, np.arange(64), np.arange(40))
    n = z.size
    assert z.shape == (40, 64, 50) and n == 128000
    mean, std = float(z.mean()), float(z.std())
    print("normals: mean %.4f, std %.4f, largest |z| %.2f" % (mean, std, np.abs(z).max()))
    assert abs(mean) < 4.0 / np.sqrt(n) and abs(std - 1.0) < 4.0 / np.sqrt(2.0 * n)
    # streams and intervals are independent coordinates of the counter: a shard that starts at rollout 20 draws what the global batch draws
    assert np.array_equal(oc.normals(1234, 20 + np.arange(17), np.arange(3)), z[:3, 20:37])
    assert np.array_equal(oc.normals(1234, np.arange(4), 7 + np.arange(2)), z[7:9, :4])
    assert not np.array_equal(oc.normals(1235, np.arange(4), np.arange(2)), z[:2, :4])
    # a stream index beyond 32 bits reaches the second counter word
    hi = oc.normals(1234, np.array([1 << 32, 0], dtype=np.uint64), [0])
    assert np.array_equal(hi[0, 1], z[0, 0]) and not np.array_equal(hi[0, 0], z[0, 0])


# ---- structure of the error rows
def test_error_rows_and_boxplus():
    rng = np.random.default_rng(3)
    rec = oc.golden_records()
    d = oc.errors(rec, 99, 0, 0, 4)
    assert d.shape == (4, oc.GOLDEN_B, NX)
    assert np.abs(np.linalg.norm(d[..., 3:7], axis=-1) - 1.0).max() < 1e-15                     # delta.quat is a unit quaternion
    x = rng.normal(size=(oc.GOLDEN_B, NX)); x[:, 3:7] /= np.linalg.norm(x[:, 3:7], axis=1, keepdims=True)
    zero = np.arange(oc.GOLDEN_B) % 4 == 3
    assert zero.sum() >= 4 and np.all(d[:, zero, 3] == 1.0) and np.all(np.delete(d[:, zero], 3, axis=-1) == 0.0)
    assert np.array_equal(oc.boxplus(x, d[0])[zero], x[zero])                                    # a zero record: x [+] delta == x
    bias_only = np.flatnonzero(np.arange(oc.GOLDEN_B) % 4 == 1)
    other = oc.errors(rec, 7, 5, 11, 4)
    assert np.array_equal(d[:, bias_only], other[:, bias_only]) and np.array_equal(d[0, bias_only], d[3, bias_only])      # pure bias: no seed, no interval
    assert not np.array_equal(d[0, 0], d[1, 0]) and not np.array_equal(d[:, 0], other[:, 0])     # noise: both
    assert np.array_equal(oc.errors(rec[:1], 99, 0, 0, 2, B=3)[:, 0], d[:2, 0])                  # one record for all: rollout 0 as before
    # the rotation: delta.quat is exp of the rotation vector, and [+] composes it on the right (body frame)
    e = np.zeros(50); e[3:6] = (0.0, 0.0, 0.2)
    row = oc.error_rows(e)
    assert np.allclose(row[3:7], (np.cos(0.1), 0.0, 0.0, np.sin(0.1)), atol=1e-16)
    xq = np.zeros(NX); xq[3] = 1.0
    assert np.array_equal(oc.boxplus(xq, row)[3:7], row[3:7])
    e = np.zeros(50); e[0:3] = (0.1, -0.2, 0.3); e[6] = 0.5; e[25] = -1.0; e[49] = 2.0
    row = oc.error_rows(e)
    assert np.array_equal(row[:3], e[:3]) and np.array_equal(row[3:7], (1.0, 0.0, 0.0, 0.0)) and np.array_equal(row[7:], e[6:])


def test_golden_is_the_restatement():
    g = oc.golden()
    rec = g["records"]
    assert rec.shape == (oc.GOLDEN_B, 100) and np.abs(rec).max() <= 1.0 and rec[:, 50:].min() >= 0.0 and np.array_equal(rec, oc.golden_records())
    assert int(g["seed"]) == oc.GOLDEN_SEED and int(g["stream0"]) == 0 and int(g["interval0"]) == oc.GOLDEN_INTERVAL0 and int(g["count"]) == oc.GOLDEN_COUNT
    kinds = np.arange(oc.GOLDEN_B) % 4
    assert all((kinds == k).sum() >= 8 for k in range(4)) and np.abs(rec[4]).min() == 1.0        # the four kinds of record, one at the bounds
    b, k = np.broadcast_arrays(np.arange(oc.GOLDEN_B, dtype=np.uint64)[:, None], np.arange(25, dtype=np.uint64)[None, :])
    counter = np.stack([b, np.zeros_like(b), np.zeros_like(b), k], axis=-1)
    key = np.broadcast_to(np.array([oc.GOLDEN_SEED & 0xFFFFFFFF, oc.GOLDEN_SEED >> 32], dtype=np.uint64), counter.shape[:-1] + (2,))
    assert np.array_equal(oc.philox4x32_10(counter, key), g["words0"].astype(np.uint64))         # the integer part: exactly
    z = oc.normals(oc.GOLDEN_SEED, np.arange(oc.GOLDEN_B), np.arange(oc.GOLDEN_COUNT))
    d = oc.errors(rec, oc.GOLDEN_SEED, 0, 0, oc.GOLDEN_COUNT)
    print("golden against this machine's restatement: z %.2e, delta %.2e" % (np.abs(z - g["z"]).max(), np.abs(d - g["delta"]).max()))
    assert np.abs(z - g["z"]).max() < 1e-14 and np.abs(d - g["delta"]).max() < 1e-14


# ---- host logic
def test_stack_plant_observation_broadcasts_and_validates():
    o = sc.stack_plant_observation(4)
    assert o.shape == (4, 100) and o.dtype == np.float64 and np.array_equal(o, np.zeros((4, 100)))
    o = sc.stack_plant_observation(4, position_bias=(0.01, 0.0, -0.02), orientation_noise=0.02, joints_noise=np.arange(19) * 1e-3, linear_velocity_bias=[0.1, 0.2, 0.3, 0.4],
                                   angular_velocity_noise=np.full((4, 3), 0.05), joint_velocities_bias=np.ones((4, 19)))
    assert np.array_equal(o[:, 0:3], np.tile((0.01, 0.0, -0.02), (4, 1))) and np.all(o[:, 53:56] == 0.02) and np.array_equal(o[:, 56:75], np.tile(np.arange(19) * 1e-3, (4, 1)))
    assert np.array_equal(o[:, 25:28], np.repeat([[0.1], [0.2], [0.3], [0.4]], 3, axis=1)) and np.all(o[:, 78:81] == 0.05) and np.all(o[:, 31:50] == 1.0)
    untouched = np.ones(100, dtype=bool)
    for a, b in ((0, 3), (53, 56), (56, 75), (25, 28), (78, 81), (31, 50)):
        untouched[a:b] = False
    assert np.all(o[:, untouched] == 0.0)
    from mpc_ilqr_mujoco_amd import solver as sv
    assert [(g, f, w) for g, f, w in sv.PLANT_OBSERVATION_GROUPS] == [(g, f, w) for g, f, w in sc._OBSERVATION_GROUPS] and sum(w for _, _, w in sv.PLANT_OBSERVATION_GROUPS) == 50
    for kw in (dict(pelvis_bias=0.1), dict(position_bias=(0.1, 0.2)), dict(joints_noise=np.zeros(3)), dict(position_bias=np.zeros((3, 3))), dict(position_noise=-0.01),
               dict(joints_noise=[0.0] * 18 + [-1e-9]), dict(orientation_bias=np.nan), dict(angular_velocity_noise=np.inf), dict(joint_velocities_bias=np.zeros((4, 19, 1)))):
        with pytest.raises(ValueError):
            sc.stack_plant_observation(4, **kw)
    with pytest.raises(ValueError):
        sc.stack_plant_observation(0)
    assert sc.stack_plant_observation(4, position_bias=-0.5)[0, 0] == -0.5                      # a bias may be negative


def test_observation_entry_points_refuse_bad_arguments_before_they_touch_the_handle():
    sv, L = _lib()
    good = [0.0] * 100
    for fn in NAMES:
        assert hasattr(L, fn)
    rec = (C.c_double * 100)(*good)
    buf = (C.c_double * (100 * 37))()
    seed, s0 = C.c_ulonglong(1), C.c_ulonglong(0)
    assert L.ilqr_hip_plant_set_observation(None, rec, 1, seed, s0) == ERR_ARG
    assert L.ilqr_hip_plant_clear_observation(None) == ERR_ARG
    assert L.ilqr_hip_plant_num_observation_sets(None) == -1
    assert L.ilqr_hip_plant_get_observation(None, buf, None, None) == ERR_ARG
    assert L.ilqr_hip_plant_observation_errors(None, C.c_long(0), 1, buf) == ERR_ARG
    assert L.ilqr_hip_plant_get_observed(None, buf) == ERR_ARG
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    assert L.ilqr_hip_plant_set_observation(h, None, 1, seed, s0) == ERR_ARG
    for n_sets in (0, -1, 2, 37):                                           # neither 1 nor the batch (0 on this handle, and 0 sets is no table)
        assert L.ilqr_hip_plant_set_observation(h, buf, n_sets, seed, s0) == ERR_ARG, n_sets
    for col, v in ((0, np.nan), (49, np.inf), (50, np.nan), (99, -np.inf), (50, -1e-300), (74, -1.0), (99, -0.5)):      # non-finite anywhere, a negative sigma
        r = list(good); r[col] = v
        assert L.ilqr_hip_plant_set_observation(h, (C.c_double * 100)(*r), 1, seed, s0) == ERR_ARG, (col, v)
    assert L.ilqr_hip_plant_get_observation(h, None, None, None) == ERR_ARG
    assert L.ilqr_hip_plant_num_observation_sets(h) == 0                    # no table on the zeroed handle
    for i0, count, out in ((0, 0, buf), (0, -2, buf), (-1, 1, buf), (0, 1, None), (0, 1, buf)):      # (the zeroed handle has N = 0: every count exceeds it)
        assert L.ilqr_hip_plant_observation_errors(h, C.c_long(i0), count, out) == ERR_ARG, (i0, count)
    assert L.ilqr_hip_plant_get_observed(h, None) == ERR_ARG


def test_header_and_wrappers_declare_the_feature():
    from mpc_ilqr_mujoco_amd import solver as sv
    hdr = open(os.path.join(ROOT, "include", "ilqr_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int " + name + r"\s*\(", hdr, re.M), name
    assert all(name in sv.EXPORTS for name in NAMES)
    assert re.search(r"^#define\s+ILQR_PLANT_OBSERVATION\s+100\b", hdr, re.M) and sv.PLANT_OBSERVATION == 100
    hpp = open(os.path.join(ROOT, "include", "ilqr_hip.hpp")).read()
    assert all(m in hpp for m in ("plantSetObservation", "plantClearObservation", "plantNumObservationSets", "plantObservation", "plantObservationErrors", "plantObserved"))
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integ for name in NAMES)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "ilqr_hip_plant_set_observation" in design and "k_plant_follow_o" in design and "k_observation_draw" in design
    # a dry run (nothing is compiled): what builds the module compiles plant_kernels.hip with the module's macro
    mk = subprocess.run(["make", "-n", "-B", "../lib/libilqr_hip_observe.so"], cwd=os.path.join(ROOT, "mpc-ilqr-mujoco_amd", "csrc"), capture_output=True, text=True)
    assert mk.returncode == 0, mk.stderr
    assert any("plant_kernels.hip" in line and "-DPLANT_OBSERVE_MODULE" in line for line in mk.stdout.splitlines()), mk.stdout
    s = sv.BatchedILQR.__new__(sv.BatchedILQR)      # no handle: the shape checks fail before the library is reached
    s.B, s.N, s.h = 3, 25, None
    for bad in (np.ones(99), np.ones((2, 100)), np.ones((3, 101)), np.ones((1, 3, 100))):
        with pytest.raises(ValueError):
            s.plant_set_observation(bad)
    for seed, stream0 in ((-1, 0), (1 << 64, 0), (0, -1), (0, 1 << 64)):
        with pytest.raises(ValueError):
            s.plant_set_observation(np.zeros((3, 100)), seed=seed, stream0=stream0)
    for i0, count in ((-1, 1), (0, 0), (0, 26)):
        with pytest.raises(ValueError):
            s.plant_observation_errors(i0, count)


class _ObservationRecorder(_Recorder):
    def plant_set_payload(self, payload):
        self._rec("plant_set_payload(%d)" % len(payload))

    def plant_set_observation(self, observation, seed=0, stream0=0):
        self._rec("plant_set_observation(%d,%d,%d)" % (len(observation), seed, stream0))

    def plant_get_observed(self):
        self._rec("plant_get_observed")
        return np.zeros((self.B, NX))


def test_runner_refuses_without_the_resident_plant_and_installs_in_order():
    from mpc_ilqr_mujoco_amd import mpc_loop as ml
    Bn, Nn = 3, 25
    o = sc.stack_plant_observation(Bn, position_bias=[0.0, 0.01, 0.02], joints_noise=0.002)
    m = sc.stack_plant_payload(Bn, [0.0, 5.0, 15.0])
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(_ObservationRecorder(Bn, Nn), _Refs(Nn), _base(Nn), plant_observation=o)
    with pytest.raises(ValueError, match="resident"):
        ml.MPCRunner(_ObservationRecorder(Bn, Nn), _Refs(Nn), _base(Nn), plant_observation=o, resident=False)
    for bad in (np.ones((2, 100)), np.ones((Bn, 99)), np.ones((1, Bn, 100))):
        with pytest.raises(ValueError):
            ml.MPCRunner(_ObservationRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_observation=bad)
    s = _ObservationRecorder(Bn, Nn)
    run = ml.MPCRunner(s, _Refs(Nn), _base(Nn), resident=True, plant_payload=m, plant_observation=o, observation_seed=77, observation_stream0=5)
    run.run(np.zeros((Bn, NX)), 2)
    head = ["plant_configure(1,0,schedule)", "plant_set_payload(3)", "plant_set_observation(3,77,5)", "plant_set_history(2)", "plant_reset"]
    assert s.calls[:5] == head, s.calls
    # the cold first step initialises from the measurement, the warm one on the device
    rest = s.calls[5:]
    assert rest.index("plant_get_observed") < rest.index("initialize") and rest.count("plant_get_observed") == 1 and rest.count("initialize_warm_from_plant") == 1
    assert s.calls.count("plant_advance") == 2
    s = _ObservationRecorder(Bn, Nn)
    ml.MPCRunner(s, _Refs(Nn), _base(Nn), resident=True).run(np.zeros((Bn, NX)), 2)
    assert not any(c.startswith("plant_set_observation") or c == "plant_get_observed" for c in s.calls)
    one = ml.MPCRunner(_ObservationRecorder(Bn, Nn), _Refs(Nn), _base(Nn), resident=True, plant_observation=o[1])      # one record, given as a vector
    assert one.plant_observation.shape == (1, 100)
