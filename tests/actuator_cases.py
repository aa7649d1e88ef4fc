"""The actuator model of the resident plant (include/ilqr_hip.h ilqr_hip_plant_set_actuator) restated in NumPy: the normals of the torque
noise -- the generator of tests/observation_cases.py in the blocks 32..41 -- and the chain command -> delay line -> first-order lag -> noise,
with the priming rule.  The integer part of the draws is exact, so the device's differ from these by the libm of log / cos / sin alone; the
chain is additions, one product rounded on its own per stage and selections, so given the device's beta and draws it is the device's
arithmetic.

Shared by tests/test_actuator_cpu.py, tests/test_gpu_actuator.py and tests/golden/gen_actuator_golden.py."""
import os

import numpy as np

from observation_cases import MASK, TWO_PI, philox4x32_10, uniforms

NU, REC, SLOTS, MAX_DELAY = 19, 39, 9, 8
BLOCK0, BLOCKS = 32, 10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actuator_golden.npz")
MUTANTS = ("delay_off_by_one", "lag_dropped", "noise_dropped", "primed_with_zeros", "noise_per_substep")


def words(seed, streams, intervals):
    """output words [len(intervals), len(streams), 10, 4] of the blocks 32..41"""
    seed = int(seed)
    s = np.asarray(streams, dtype=np.uint64)[None, :, None]
    i = np.asarray(intervals, dtype=np.uint64)[:, None, None]
    k = (BLOCK0 + np.arange(BLOCKS, dtype=np.uint64))[None, None, :]
    s, i, k = np.broadcast_arrays(s, i, k)
    counter = np.stack([s & MASK, s >> np.uint64(32), i & MASK, k], axis=-1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    return philox4x32_10(counter, np.broadcast_to(key, counter.shape[:-1] + (2,)))


def normals(seed, streams, intervals):
    """z [len(intervals), len(streams), 19]: block 32 + q gives joints 2q and 2q + 1; the second normal of block 41 is discarded"""
    u1, u2 = uniforms(words(seed, streams, intervals))
    r = np.sqrt(-2.0 * np.log(u1))
    ang = TWO_PI * u2
    z = np.empty(u1.shape[:-1] + (2 * BLOCKS,))
    z[..., 0::2] = r * np.cos(ang)
    z[..., 1::2] = r * np.sin(ang)
    return z[..., :NU]


def draws(seed, stream0, interval0, count, B):
    """z [count, B, 19]: what ilqr_hip_plant_actuator_draws returns"""
    return normals(seed, int(stream0) + np.arange(int(B)), int(interval0) + np.arange(int(count)))


def blend(records, h):
    """beta [n, 19] = -expm1(-h / tau); 1 where tau == 0, which is never computed (and never used: the chain selects)"""
    tau = np.atleast_2d(np.asarray(records, dtype=np.float64))[:, 1:1 + NU]
    beta = np.ones_like(tau)
    lag = tau != 0.0
    beta[lag] = -np.expm1(-h / tau[lag])
    return beta


def guard(c):
    """main/humanoid_mpc.cpp:162-165: a command with a non-finite entry is zero, all of it"""
    c = np.array(c, dtype=np.float64)
    c[~np.isfinite(c).all(axis=-1)] = 0.0
    return c


class Chain:
    """The actuator state of B rollouts: n substeps since the priming, the delay line [B, 9, 19], the lag output y [B, 19].
    records [1 or B, 39], beta [1 or B, 19] (the device's, or blend(records, h)).  mutant: one of MUTANTS -- a WRONG chain, for the tests that
    show the inputs of the GPU tests can tell."""

    def __init__(self, records, beta, B=None, mutant=None):
        records = np.atleast_2d(np.asarray(records, dtype=np.float64))
        self.B = records.shape[0] if B is None else int(B)
        rec = np.broadcast_to(records, (self.B, REC))
        self.delay = rec[:, 0].astype(np.int64)
        self.tau, self.sigma = rec[:, 1:1 + NU].copy(), rec[:, 1 + NU:].copy()
        self.beta = np.broadcast_to(np.atleast_2d(np.asarray(beta, dtype=np.float64)), (self.B, NU)).copy()
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant
        if mutant == "delay_off_by_one":
            self.delay = np.where(self.delay == MAX_DELAY, MAX_DELAY - 1, self.delay + 1)
        self.prime()

    def prime(self):
        self.n = 0
        self.fifo = np.zeros((self.B, SLOTS, NU))
        self.y = np.zeros((self.B, NU))

    def substep(self, command, z):
        """command [B, 19] (the law's output, in front of the guard), z [B, 19] (the interval's normals) -> the applied torque [B, 19]"""
        c = guard(command)
        rows = np.arange(self.B)
        if self.n == 0:
            first = np.zeros_like(c) if self.mutant == "primed_with_zeros" else c
            self.fifo[:] = first[:, None, :]
            self.y = first.copy()
        self.fifo[:, self.n % SLOTS] = c
        a = self.fifo[rows, (self.n - self.delay) % SLOTS]
        if self.n > 0 or self.mutant == "primed_with_zeros":
            d = self.beta * (a - self.y)
            lagged = self.y + d
            self.y = a.copy() if self.mutant == "lag_dropped" else np.where(self.tau == 0.0, a, lagged)
        s = self.sigma * z
        t = self.y.copy() if self.mutant == "noise_dropped" else np.where(self.sigma == 0.0, self.y, self.y + s)
        self.n += 1
        return t

    def copy(self):
        other = Chain.__new__(Chain)
        other.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()})
        return other


def run_chain(records, beta, commands, z, substeps, mutant=None, seed=None):
    """commands [n_sub, B, 19], z [intervals, B, 19], interval of substep n = n // substeps -> applied [n_sub, B, 19].  The mutant
    noise_per_substep reads another draw in every substep (the normals of `seed` at interval n in the place of n // substeps)."""
    commands = np.asarray(commands, dtype=np.float64)
    ch = Chain(records, beta, B=commands.shape[1], mutant=mutant)
    if mutant == "noise_per_substep":
        zs = draws(seed, 0, 0, commands.shape[0], commands.shape[1])
        return np.stack([ch.substep(commands[n], zs[n]) for n in range(commands.shape[0])])
    return np.stack([ch.substep(commands[n], z[n // substeps]) for n in range(commands.shape[0])])


# ---- the records of the golden and of the GPU tests: B = 37, six intervals of three substeps
GOLDEN_B, GOLDEN_SEED, GOLDEN_INTERVAL0, GOLDEN_COUNT, GOLDEN_SUBSTEPS, GOLDEN_DT = 37, 0x0FED_CBA9_8765_4321, 0, 6, 3, 0.02
DELAYS = (0, 1, 2, 3, 4, 8)
TAUS = (0.0, 0.005, 0.02, 0.08)


def golden_records(B=GOLDEN_B, seed=23):
    """rollout b: delay DELAYS[b % 6] (below, at and above an interval of three substeps); tau per joint one of TAUS, all zero where
    b % 4 == 3; sigma per joint zero or up to 2 N m, all zero where b % 4 == 2.  No rollout has a zero record."""
    rng = np.random.default_rng(seed)
    b = np.arange(B)
    rec = np.zeros((B, REC))
    rec[:, 0] = np.asarray(DELAYS, dtype=np.float64)[b % len(DELAYS)]
    tau = np.asarray(TAUS)[rng.integers(0, len(TAUS), (B, NU))]
    tau[:, 0] = TAUS[2]                                                 # (at least one lagged joint per record, whatever was drawn)
    rec[:, 1:1 + NU] = np.where((b % 4 == 3)[:, None], 0.0, tau)
    sigma = np.where(rng.random((B, NU)) < 0.25, 0.0, rng.uniform(0.0, 2.0, (B, NU)))
    sigma[:, 1] = 2.0                                                   # (the upper bound, and at least one noisy joint per record)
    rec[:, 1 + NU:] = np.where((b % 4 == 2)[:, None], 0.0, sigma)
    return rec


def synthetic_commands(n_sub, B=GOLDEN_B, hold=1, seed=29):
    """[n_sub, B, 19]: torques of some tens of N m that change in every `hold`-th substep (hold = substeps: feedback mode 0)"""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-40.0, 40.0, (1, B, NU))
    steps = rng.uniform(-3.0, 3.0, (-(-n_sub // hold), B, NU))
    return np.repeat(base + np.cumsum(steps, axis=0), hold, axis=0)[:n_sub]


def golden():
    return np.load(GOLDEN)
