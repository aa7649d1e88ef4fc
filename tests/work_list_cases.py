"""Cases of the work-list tests (test_work_lists_cpu.py, test_gpu_work_lists.py, golden/gen_work_list_golden.py): batches wider than one
k_control workgroup (16 rollouts), so that the lists of the linearisation cache and of the first-pass skip (DevState::chg, chg_f, order) are
assembled from several workgroups, each with one atomicAdd per list.

The reference is the CPU oracle (oracle_lib.Oracle), one handle per rollout.  It is too slow to solve 40 rollouts inside a GPU test, so
golden/work_list_traces.npz keeps, per case and solve, what decides every list -- iteration count, cost / alpha / lambda trace and final
lambda of every rollout -- and predicted_counts() turns alpha traces into the list lengths and the two counters a device run must report.

NumPy, the oracle and the host kinematics of the product library; no GPU."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import conftest
import oracle_lib as ol

pkg = conftest.load_package()
sc = pkg.scenario
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(G, "work_list_traces.npz")
N, NX, NU = 25, 51, 19
GROUP = 16                                      # rollouts per k_control workgroup (CTRL_WAVES)
MAX_THREADS = 16
SEEDS = range(16)
MODE_CASES = ("contact2", "contact3", "contact4", "joint_limits", "walking50", "weight_sets")
MODE_B = 24                                     # two workgroups, the second half full
TRACE_KEYS = ("it", "cost", "alpha", "lam", "lam_final")
# the solves of standing40 the fixture holds: three initialize(x0, ui) + solve on one handle (lambda carries over), a convergence-exit solve,
# steps 2 and 3 of the warm-started chains with a shift of 1 and of 2 (step 1 of either is fixed0), and of a chain with a shift of 1 whose
# plant is disturbed between the solves: the undisturbed chains start every later solve converged and accept nothing in it
STANDING_RUNS = ("fixed0", "fixed1", "fixed2", "exit", "warm1_1", "warm1_2", "warm2_1", "warm2_2", "kick1_1", "kick1_2")
CHAINS = dict(warm1=(1, False), warm2=(2, False), kick1=(1, True))      # name: (shift, the plant is kicked between the solves)
CHAIN_STEPS = 3


class Case:
    def __init__(self, name, prob, x0, ui, iters, plant=None, seed=None):
        self.name, self.prob, self.x0, self.ui, self.iters, self.plant, self.seed = name, prob, x0, ui, iters, dict(plant or {}), seed
        self.B = len(x0)

    def configure(self, h):
        """contact mode, friction, joint-limit rows and stiffness on an oracle or a solver handle (the setters share their names)"""
        p = self.plant
        if "contact" in p:
            h.set_contact_mode(p["contact"])
        if "friction" in p:
            h.set_friction(p["friction"])
        if "limits" in p:
            h.set_joint_limits(True)
            h.set_joint_limit_stiffness(p["limits"])

    def problem_of(self, b):
        """the problem of rollout b with 1-D weights, for Oracle.set_problem(p, b)"""
        prob = self.prob
        if np.ndim(prob["Q"]) == 1:
            return prob
        p = dict(prob)
        for k in ("Q", "R", "Qf"):
            p[k] = np.array(prob[k][b])
        p["task_weights"] = tuple(float(v) for v in prob["task_weights"][b])
        p["w_joint"], p["w_ctrl"] = float(prob["w_joint"][b]), float(prob["w_ctrl"][b])
        return p

    def oracle(self, b, early_exit=False):
        o = ol.Oracle(self.prob["N"], self.prob["dt"])
        o.set_problem(self.problem_of(b), b)
        o.set_options(jac_mode=0, early_exit=int(early_exit), max_iter=self.iters)
        self.configure(o)
        return o


def _sv():
    from mpc_ilqr_mujoco_amd import solver as sv
    return sv


def _standing(B, seed, gravity=None):
    sv = _sv()
    prob = sc.make_problem(sv.reference_kinematics, N=N, gravity=gravity)
    ug = sv.gravity_compensation(sc.standing_state(), prob["gravity"])
    x0, ui = sc.synthetic_batch(B, N, seed, ug)
    return prob, x0, ui


def standing40():
    """synthetic_batch(40, 25, 53, grav_comp) on the shipped problem, 10 fixed iterations: three workgroups of 16 / 16 / 8"""
    return Case("standing40", *_standing(40, 53), iters=10, seed=53)


EARTH = (0.0, 0.0, -9.81)


def mode_case(name, seed):
    B = MODE_B
    if name in ("contact2", "contact3", "contact4"):
        plant = dict(contact=int(name[-1]))
        if name != "contact2":
            plant["friction"] = 0.7 if name == "contact3" else 0.4
        return Case(name, *_standing(B, seed, EARTH), iters=6, plant=plant, seed=seed)
    if name == "joint_limits":
        # every other rollout starts with the left knee (hinge 3) past its upper limit and moving out, every fourth also with the right elbow
        # (hinge 18) past its lower limit: the stop and its restoring term act in both workgroups
        prob, x0, ui = _standing(B, seed)
        x0 = x0.copy()
        x0[1::2, 7 + 3] = 2.09; x0[1::2, 32 + 3] = 1.5
        x0[3::4, 7 + 18] = -1.29; x0[3::4, 32 + 18] = 0.1
        k = float(np.load(os.path.join(G, "joint_limit_stiffness_golden.npz"))["stiffness"])
        return Case(name, prob, x0, ui, iters=6, plant=dict(limits=k), seed=seed)
    if name == "walking50":
        from mpc_ilqr_mujoco_amd import references as rf
        prob, x0, ui, _ = sc.walking_batch(B, 50, seed, os.path.join(G, "refdata_golden.npz"), _sv(), rf)
        return Case(name, prob, x0, ui, iters=6, plant=dict(contact=2), seed=seed)
    if name == "weight_sets":
        prob, x0, ui = _standing(B, seed)
        scale = (1.0, 1.5, 0.6)
        prob = sc.stack_weight_sets(prob, [dict(Q=prob["Q"] * scale[b % 3], Qf=prob["Qf"] * scale[b % 3]) for b in range(B)])
        return Case(name, prob, x0, ui, iters=10, seed=seed)
    raise KeyError(name)


# ---- oracle solves ---------------------------------------------------------------------------------------------------------------------
def record(o, iters):
    it, cost, alpha, lam = o.trace()
    assert cost.shape == (iters + 1,) and alpha.shape == (iters,)
    return dict(it=np.int64(it), cost=cost, alpha=alpha, lam=lam, lam_final=np.float64(o.get_lambda()))


def solve_fixed(case, b, f=1.0, early_exit=False):
    """one cold solve of rollout b from f * x0"""
    o = case.oracle(b, early_exit)
    x = case.x0[b] * f
    o.initialize(x, case.ui[b]); o.solve(x)
    return record(o, case.iters)


def warm_start(o, x, shift):
    """The resident solution of `o` shifted by `shift` knots behind the state x (ilqr.cpp:68-80 for a shift of 1, which the oracle's own
    initialize does; a longer shift repeats the last control and re-rolls the knots the shift leaves open)."""
    pxb, pub = o.get("xbar"), o.get("ubar")
    if shift == 1:
        o.initialize(x, None, pxb, pub)
        return
    n = pub.shape[0]
    ub = pub[np.minimum(np.arange(n) + shift, n - 1)]
    xb = np.empty_like(pxb)
    xb[0] = x
    xb[1:n - shift + 1] = pxb[1 + shift:]
    for t in range(n - shift, n):
        xb[t + 1] = o.step(xb[t], ub[t])
    o.set_trajectory(xb, ub)


def advance(o, x, shift):
    """the state `shift` oracle steps along the control law of the solution `o` holds (compute_control at knot 0, u_t + K_t (x - x_t) after it)"""
    x = o.step(x, o.compute_control(x))
    if shift > 1:
        xb, ub, K = o.get("xbar"), o.get("ubar"), o.get("K")
        for t in range(1, shift):
            x = o.step(x, ub[t] + K[t] @ (x - xb[t]))
    return x


KICK = 0.1


def kick_of(b, step):
    """the disturbance of rollout b ahead of solve `step`: every velocity moved by up to 0.1 (the spread of synthetic_batch's initial ones)"""
    return KICK * np.random.default_rng([53, b, step]).uniform(-1.0, 1.0, NX - 26)


def solve_chain(case, b, shift, f=1.0, kick=False):
    """MPC steps on one oracle handle: a cold solve from f * x0, then CHAIN_STEPS - 1 times advance (and kick), warm start, solve.
    -> ([record per step], states [CHAIN_STEPS, 51])"""
    o = case.oracle(b)
    x = case.x0[b] * f
    o.initialize(x, case.ui[b]); o.solve(x)
    recs, xs = [record(o, case.iters)], [x]
    for k in range(1, CHAIN_STEPS):
        x = advance(o, x, shift)
        if kick:
            x = x.copy(); x[26:] += kick_of(b, k)
        warm_start(o, x, shift); o.solve(x)
        recs.append(record(o, case.iters)); xs.append(x)
    return recs, np.array(xs)


def standing_runs(case, b, f=1.0):
    """every solve of STANDING_RUNS for rollout b -> ({run: record}, {chain: states})"""
    out, xs = {}, {}
    o = case.oracle(b)
    x = case.x0[b] * f
    for k in range(CHAIN_STEPS):
        o.initialize(x, case.ui[b]); o.solve(x)
        out["fixed%d" % k] = record(o, case.iters)
    out["exit"] = solve_fixed(case, b, f, early_exit=True)
    for chain, (shift, kick) in CHAINS.items():
        recs, xs[chain] = solve_chain(case, b, shift, f, kick)
        assert np.array_equal(recs[0]["alpha"], out["fixed0"]["alpha"], equal_nan=True)
        for k in range(1, CHAIN_STEPS):
            out["%s_%d" % (chain, k)] = recs[k]
    return out, xs


def mode_runs(case, b, f=1.0):
    return {"fixed0": solve_fixed(case, b, f)}, {}


def runs_of(case):
    return standing_runs if case.name == "standing40" else mode_runs


def same_decisions(a, b):
    """two {run: record}: iteration counts and alpha traces equal"""
    return all(int(a[r]["it"]) == int(b[r]["it"]) and np.array_equal(a[r]["alpha"], b[r]["alpha"], equal_nan=True) for r in a)


def tie_free(case, b, base=None):
    """no accept decision of rollout b sits on a tie: x0 scaled by (1 +- 1e-9) leaves every iteration count and alpha trace as it was"""
    fn = runs_of(case)
    base = fn(case, b)[0] if base is None else base
    return all(same_decisions(base, fn(case, b, f)[0]) for f in (1.0 + 1e-9, 1.0 - 1e-9))


def threads():
    return max(1, min(MAX_THREADS, os.cpu_count() or 1))


def pool_map(fn, items):
    """fn over items on at most 16 threads (the oracle's calls release the interpreter lock; every call has a handle of its own)"""
    with ThreadPoolExecutor(max_workers=threads()) as ex:
        return list(ex.map(fn, items))


def stack(per_rollout):
    """[{run: record}] over the rollouts -> {run: {key: array with a leading rollout axis}}"""
    return {run: {k: np.array([r[run][k] for r in per_rollout]) for k in TRACE_KEYS} for run in per_rollout[0]}


# ---- the fixture -----------------------------------------------------------------------------------------------------------------------
def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def fixture_run(fx, case, run="fixed0"):
    return {k: fx["%s/%s/%s" % (case, run, k)] for k in TRACE_KEYS}


def fixture_cases(fx):
    """the mode cases the fixture holds, with their seeds"""
    return {c: int(fx[c + "/seed"]) for c in MODE_CASES if c + "/seed" in fx}


# ---- from traces to lists --------------------------------------------------------------------------------------------------------------
def predicted_counts(alpha, iterations, early_exit):
    """What the lists of a solve hold, from its alpha traces [B, n] (NaN behind a rollout's last iteration) and iteration counts [B]:
    (first-pass rollouts with the skip, without it, linearised rollouts with the cache, without it, list length per iteration).

    A rollout is active in iteration i while it has a trace entry there.  Iteration 0 takes every rollout; the list of iteration i >= 1
    holds the active rollouts whose iteration i - 1 accepted a candidate (alpha != 0), in the first-pass skip and in the cache alike;
    without either the pass takes every active rollout.  Without the convergence exit every rollout runs all n iterations."""
    alpha, iterations = np.asarray(alpha, dtype=np.float64), np.asarray(iterations)
    B, n = alpha.shape
    assert iterations.shape == (B,)
    if not early_exit:
        assert (iterations == n).all(), "fixed iterations: every rollout runs all of them"
    lists, active = [B], [B]
    for i in range(1, n):
        act = iterations > i
        assert not np.isnan(alpha[act, i - 1]).any(), "an active rollout has a trace entry in the previous iteration"
        lists.append(int((act & (alpha[:, i - 1] != 0.0)).sum()))
        active.append(int(act.sum()))
    return sum(lists), sum(active), sum(lists), sum(active), lists


def list_members(alpha, iterations, i):
    """the rollouts on the list of iteration i >= 1"""
    alpha, iterations = np.asarray(alpha), np.asarray(iterations)
    return np.flatnonzero((iterations > i) & (alpha[:, i - 1] != 0.0))


def occurrence(alpha, iterations):
    """(iterations >= 1 that hold both listed and skipped rollouts, iterations >= 1 whose list has entries from more than one workgroup)
    -- a case of these tests needs one of each"""
    iterations = np.asarray(iterations)
    mixed, spread = [], []
    for i in range(1, np.asarray(alpha).shape[1]):
        m = list_members(alpha, iterations, i)
        if 0 < len(m) < int((iterations > i).sum()):
            mixed.append(i)
        if len(set(int(b) // GROUP for b in m)) > 1:
            spread.append(i)
    return mixed, spread


def per_group(alpha, iterations, i):
    """list entries of iteration i per workgroup"""
    m = list_members(alpha, iterations, i)
    return [int((m // GROUP == g).sum()) for g in range((len(iterations) + GROUP - 1) // GROUP)]
