"""Inputs of the solve-group tests (test_groups_cpu.py, test_gpu_groups.py): the constructed keys of the selection rule, the batches of groups
and the designed starts whose winners the CPU oracle fixes.  NumPy, the CPU oracle and the host-only helpers; no GPU code.

Shapes: (B, G) in SHAPES -- 8 and 64 divide the wave (several groups per wave, one per wave), 5 and 3 do not (one group per wave, idle lanes;
B = 39: a last workgroup that is not full); N = 6 and N = 5 -- a rollout's xbar, ubar and gains have an odd number of doubles at one of them
and an even number at the other (357 / 306, 114 / 95, 5814 / 4845), which is the 8-byte and the 16-byte path of k_group_adopt.
Problems: the shipped cost, constraint-free dynamics, dt = 0.02.  Group m of a batch takes the state and the controls of rollout
POOL_ROWS[m % 7] of the handle-walk pool (handle_walk_cases.inputs: mid-envelope states with seeded offsets) -- the even rollouts, whose cost after
a few iterations answers to the start by several per cent (the odd ones sit past a joint limit and end at the same cost from any start)."""
import functools

import numpy as np

import dynamics_envelope_cases as dc
import group_ref as gr
import handle_walk_cases as hw
import oracle_lib as ol
from conftest import load_package

pkg = load_package()
sc = pkg.scenario
NX, NU = 51, 19
DT = dc.H
SHAPES = ((40, 8), (40, 5), (128, 64), (39, 3))
HORIZONS = (6, 5)
POOL = 40
POOL_ROWS = (4, 2, 6, 8, 10, 12, 0)
MARGIN = 1e-3                      # the winners' margin asked of the oracle's keys, relative (far above what GPU rounding moves a cost by)


# ---- the selection rule on constructed keys
def select_cases(G):
    """[(name, keys [G])]: distinct keys; ties of the minimum at several positions; a NaN in every position, alone and on the minimum; +inf and
    -inf; groups without a finite key; signed zeros"""
    rng = np.random.default_rng(1000 + G)
    base = rng.uniform(1.0, 9.0, G)
    out = [("distinct", base.copy()), ("descending", np.sort(base)[::-1].copy()), ("ascending", np.sort(base))]
    lo = 0.5
    for name, pos in (("first_last", (0, G - 1)), ("last_two", (G - 2, G - 1)), ("middle", (G // 2, G // 2 + 1)), ("all", tuple(range(G)))):
        pos = sorted(set(p for p in pos if 0 <= p < G))
        k = base.copy(); k[pos] = lo
        out.append(("tie_" + name, k))
    for p in range(G):
        k = base.copy(); k[p] = np.nan
        out.append(("nan_at_%d" % p, k))
    k = base.copy(); k[int(np.argmin(base))] = np.nan
    out.append(("nan_on_the_minimum", k))
    for p in (0, G // 2, G - 1):
        k = base.copy(); k[p] = -np.inf
        out.append(("minus_inf_at_%d" % p, k))
        k = base.copy(); k[p] = np.inf
        out.append(("plus_inf_at_%d" % p, k))
    k = np.full(G, -np.inf); k[G - 1] = 7.0
    out.append(("one_finite_key_last", k))
    out.append(("all_nan", np.full(G, np.nan)))
    k = np.where(np.arange(G) % 3 == 0, np.nan, np.where(np.arange(G) % 3 == 1, np.inf, -np.inf))
    out.append(("no_finite_key_mixed", k))
    k = base.copy(); k[G - 1] = -0.0; k[0] = 0.0
    out.append(("signed_zeros_tie", k))
    k = -base
    out.append(("negative", k))
    return out


def select_batches(B, G):
    """the cases of select_cases(G) as key arrays [B], M = B / G cases per array, the last array filled up with the first cases again"""
    cases = [k for _, k in select_cases(G)]
    M = B // G
    out = []
    for a in range(0, len(cases), M):
        chunk = cases[a:a + M]
        chunk = chunk + cases[:M - len(chunk)]
        out.append(np.concatenate(chunk))
    return out


# ---- batches of groups
@functools.lru_cache(maxsize=None)
def problem(N):
    prob = sc.make_problem(ol.reference_kinematics, N=N)
    prob["dt"] = DT
    return prob


def oracle(N, max_iter):
    o = ol.Oracle(N, DT)
    o.set_problem(problem(N))
    o.set_options(lam=hw.LAMBDA0, max_iter=max_iter, early_exit=0)
    return o


def group_inputs(M, G, N):
    """(x0 [M G, 51], ui [M G, N, 19]): group m repeats rollout POOL_ROWS[m % 7] of the pool, member-minor"""
    D = hw.inputs(POOL)
    idx = np.array(POOL_ROWS)[np.arange(M) % len(POOL_ROWS)]
    return sc.repeat_for_groups(D["x0"][idx], G), sc.repeat_for_groups(D["ui"][idx, :N], G)


# ---- GPU test 3 (the incumbent): perturbed starts
INC_B, INC_G, INC_N, INC_ITERS = 40, 8, 6, 3
INC_HOLD, INC_SEED, INC_STREAM0 = 2, 1, 7
INC_BASE = 2.0


def incumbent_sigma():
    return sc.stack_group_sigma(INC_G, INC_BASE, ladder=np.linspace(0.5, 4.0, INC_G - 1))


@functools.lru_cache(maxsize=None)
def incumbent_starts():
    """(x0 [B, 51], ui [B, N, 19]) before the perturbation: the pool's controls in the even groups; in the odd groups the whole group starts
    from controls damaged by seeded noise of 20 Nm, a start that a perturbed member can beat"""
    M = INC_B // INC_G
    x0, ui = group_inputs(M, INC_G, INC_N)
    u = ui[::INC_G].copy()
    rng = np.random.default_rng(77)
    u[1::2] = np.clip(u[1::2] + rng.uniform(-1.0, 1.0, u[1::2].shape) * 20.0, -0.8 * sc.CTRLRANGE, 0.8 * sc.CTRLRANGE)
    ui = sc.repeat_for_groups(u, INC_G)
    x0.setflags(write=False); ui.setflags(write=False)
    return x0, ui


@functools.lru_cache(maxsize=None)
def incumbent_oracle_keys():
    """the oracle's cost of every member after INC_ITERS iterations from the perturbed start [B]"""
    x0, ui = incumbent_starts()
    up = gr.perturbed(ui, INC_G, incumbent_sigma(), INC_HOLD, INC_SEED, INC_STREAM0, 0)
    return oracle(INC_N, INC_ITERS).batch_solve(x0, up)[1]


# ---- GPU test 4 (adopt): designed starts, the good one at another member in every group
ADOPT_B, ADOPT_G, ADOPT_ITERS = 40, 8, 2


def good_member(m):
    return (3 * m) % ADOPT_G      # 0, 3, 6, 1, 4: group 0's winner is its member 0


@functools.lru_cache(maxsize=None)
def adopt_starts(N):
    """(x0 [B, 51], ui [B, N, 19]): member good_member(m) of group m starts from the pool's controls, the others from
    the pool's controls plus seeded noise of 8 .. 30 Nm (clipped to 0.8 of the control range), which two iterations do not repair"""
    M = ADOPT_B // ADOPT_G
    x0, ui = group_inputs(M, ADOPT_G, N)
    ui = ui.copy()
    rng = np.random.default_rng(4100 + N)
    noise = rng.uniform(-1.0, 1.0, ui.shape) * rng.uniform(8.0, 30.0, (ADOPT_B, 1, 1))
    ui = np.clip(ui + noise, -0.8 * sc.CTRLRANGE, 0.8 * sc.CTRLRANGE)
    for m in range(M):
        b = m * ADOPT_G + good_member(m)
        ui[b] = hw.inputs(POOL)["ui"][POOL_ROWS[m % len(POOL_ROWS)], :N]
    x0.setflags(write=False); ui.setflags(write=False)
    return x0, ui


@functools.lru_cache(maxsize=None)
def adopt_oracle_keys(N):
    x0, ui = adopt_starts(N)
    return oracle(N, ADOPT_ITERS).batch_solve(x0, ui)[1]


def margins(keys, G):
    """per group (second-best key - best key) / |best key| over the finite keys"""
    k = np.sort(np.asarray(keys).reshape(-1, G), axis=1)
    return (k[:, 1] - k[:, 0]) / np.abs(k[:, 0])


@functools.lru_cache(maxsize=None)
def adopt_trajectory(N):
    """xbar [B, N + 1, 51] that goes with adopt_starts(N) through set_trajectory: the oracle's rollout of every member's controls from its x0 --
    what the oracle's keys were computed from.  (A solve reports the cost of the trajectory it is GIVEN for a rollout that accepts no step,
    ilqr.cpp:540, and the designed start of some groups accepts none in two iterations: the trajectory has to be the rollout of the controls.)"""
    x0, ui = adopt_starts(N)
    o = oracle(N, ADOPT_ITERS)
    out = np.zeros((x0.shape[0], N + 1, NX))
    for b in range(x0.shape[0]):
        o.initialize(x0[b], ui[b])
        out[b] = o.get("xbar")
    assert np.array_equal(out[:, 0], x0)
    out.setflags(write=False)
    return out
