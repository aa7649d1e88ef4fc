"""Input builders for the cost-path tests (test_cost_envelope_cpu.py, test_gpu_cost_envelope.py, test_oracle_golden.py): problem
DATA the cost kernels read -- weights, references, stance rows, the soft-limit tables -- in shapes that a kernel reading the wrong
entry cannot survive.  NumPy and the oracle's host kinematics only; no GPU.

  * golden_problem(): one task term alone, tracking and penalties off (the problems of the torch-autograd golden).
  * single_term_problems(): those problems with the references and stance rows of tests/golden/cost_golden.npz.
  * scrambled_problem(): per-rollout reference sets in which no two entries of a block are equal.
  * limit_sweep(): one rollout per (hinge or actuator, side), each inside the 10 % soft margin at one knot.
  * pen() / pen_grad() / pen_hess(): the soft limit penalty in closed form (robot_utils.cpp:615-778).
"""
import os

import numpy as np

import oracle_lib as ol
from conftest import load_package

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sc = load_package().scenario
NX, NU, NQ = 51, 19, 26
TASK_KEYS = ("W_com_pos", "W_com_vel", "W_foot", "W_foot_vel", "W_upright", "w_balance")      # order of prob["task_weights"]
STANCE_ROWS = np.array([[1, 1], [1, 0], [0, 1], [0, 0]], dtype=np.int32)


def cost_golden():
    return np.load(os.path.join(G, "cost_golden.npz"))


def golden_problem(c, N=25, **weights):
    # (`c`, the loaded golden, is not read: kept for the call sites of test_oracle_golden.py)
    cfg = dict(sc.SHIPPED_CONFIG)
    cfg.update(W_com_pos=0.0, W_com_vel=0.0, W_foot=0.0, W_foot_vel=0.0, W_upright=0.0, w_balance=0.0)
    cfg.update(weights)
    prob = sc.make_problem(ol.reference_kinematics, N=N, cfg=cfg)
    # zero out tracking so only the task term remains
    prob["Q"] = np.zeros(51); prob["Qf"] = np.zeros(51); prob["R"] = np.zeros(19)
    prob["w_joint"] = 0.0; prob["w_ctrl"] = 0.0
    return prob


def single_term_problems(c, N=4):
    """[(label, problem, golden term names)]: each of the six task terms alone with the golden's own weight, references and stance
    rows, and the foot-velocity term once more with the right foot in swing.  The summed grad_* / hess_* of the names is the gradient
    and Hessian of the problem's stage cost at the golden states, at every knot t < N."""
    out = []
    p = golden_problem(c, N=N, W_com_pos=float(c["w_com"]))
    p["com_ref"][:] = c["ref_com"]
    out.append(("com", p, ["com"]))
    p = golden_problem(c, N=N, W_com_vel=float(c["w_comvel"]))
    p["com_vel_ref"][:] = c["ref_comvel"]
    out.append(("comvel", p, ["comvel"]))
    p = golden_problem(c, N=N, W_foot=float(c["w_eepos"]))
    p["stance"][:] = 0
    p["ee_ref"][0, :, 0] = c["ref_ee"]
    p["ee_ref"][0, :, 1] = c["ref_ee"] * np.array([1, -1, 1])
    out.append(("eepos", p, ["eepos_L", "eepos_R"]))
    p = golden_problem(c, N=N, W_foot_vel=float(c["w_eevel"]))
    out.append(("eevel", p, ["eevel_L", "eevel_R"]))
    p = golden_problem(c, N=N, W_foot_vel=float(c["w_eevel"]))
    p["stance"][0, :, 1] = 0
    out.append(("eevel_right_swing", p, ["eevel_L"]))
    p = golden_problem(c, N=N, W_upright=float(c["w_upright"]))
    out.append(("upright", p, ["upright"]))
    p = golden_problem(c, N=N, w_balance=float(c["w_balance"]))
    # support point = mean of the foot refs (both stance)
    p["ee_ref"][0, :, 0, :2] = c["ref_ps"] + np.array([0.0, 0.1])
    p["ee_ref"][0, :, 1, :2] = c["ref_ps"] - np.array([0.0, 0.1])
    out.append(("balance", p, ["balance"]))
    return out


def scrambled_problem(B, N, seed, gravity=None):
    """Problem with per-rollout reference sets (n_sets == B) in which nothing is uniform: every entry its own draw around the shipped
    value, so an index, a stride or a set that is off by one reads a different number."""
    rng = np.random.default_rng(seed)
    cfg = dict(sc.SHIPPED_CONFIG)
    prob = sc.make_problem(ol.reference_kinematics, N=N, cfg=cfg, gravity=gravity)
    Q, R, Qf = sc.build_cost_matrices(cfg)
    prob["Q"] = Q * np.exp(rng.uniform(-0.9, 0.9, NX))                           # each entry within a factor 2.5 of the shipped one
    prob["R"] = R * np.exp(rng.uniform(-0.9, 0.9, NU))
    prob["Qf"] = Qf * np.exp(rng.uniform(-0.9, 0.9, NX))
    shipped = np.array([cfg[k] for k in TASK_KEYS]); shipped[1] = 3.0          # (W_com_vel ships as 0: the value the parity tests switch it on with)
    prob["task_weights"] = tuple(float(v) for v in shipped * rng.uniform(0.7, 1.3, 6))
    prob["w_joint"] = float(cfg["joint_limit_weight"] * rng.uniform(0.7, 0.95))
    prob["w_ctrl"] = float(cfg["torque_limit_weight"] * rng.uniform(1.05, 1.3))
    # an entry with a heavier weight has its reference further out (rank of the weight in its block -> amplitude): replacing the weights
    # of a block by their mean then moves every rollout's cost the same way, instead of 19 signed terms that may cancel in one of them
    rank_R = np.argsort(np.argsort(prob["R"])) / (NU - 1.0)
    rank_Q = np.argsort(np.argsort(prob["Q"][7:NQ])) / (NQ - 8.0)
    prob["u_ref"] = sc.CTRLRANGE * (0.06 + 0.22 * rank_R) * rng.uniform(0.8, 1.0, (B, N, NU)) * rng.choice([-1.0, 1.0], (B, N, NU))
    x_ref = np.tile(sc.standing_state(), (B, N + 1, 1))
    x_ref[..., 0:3] += rng.uniform(-0.03, 0.03, (B, N + 1, 3))
    x_ref[..., 3:7] = sc._axis_angle_quat(rng.uniform(-0.1, 0.1, (B, N + 1, 3)))
    x_ref[..., 7:NQ] += (0.04 + 0.16 * rank_Q) * rng.uniform(0.6, 1.0, (B, N + 1, NQ - 7)) * rng.choice([-1.0, 1.0], (B, N + 1, NQ - 7))
    x_ref[..., NQ:] += rng.uniform(-0.2, 0.2, (B, N + 1, NX - NQ))
    x_ref[..., 3:7] /= np.linalg.norm(x_ref[..., 3:7], axis=-1, keepdims=True)
    prob["x_ref"] = x_ref
    com_ref, ee_ref = np.zeros((B, N + 1, 3)), np.zeros((B, N + 1, 2, 3))
    for b in range(B):
        for t in range(N + 1):
            com_ref[b, t], ee_ref[b, t] = ol.reference_kinematics(x_ref[b, t])
    prob["com_ref"] = com_ref + rng.uniform(-0.02, 0.02, com_ref.shape)
    prob["ee_ref"] = ee_ref + rng.uniform(-0.02, 0.02, ee_ref.shape)
    prob["com_vel_ref"] = rng.uniform(-0.1, 0.1, (B, N + 1, 3))
    # rows 11 / 10 / 01 / 00: rollout b starts at row b and walks the list with a stride of its own
    b_, t_ = np.arange(B)[:, None], np.arange(N + 1)[None, :]
    prob["stance"] = np.ascontiguousarray(STANCE_ROWS[(b_ + t_ * (1 + (b_ // 4) % 3)) % 4])
    return prob


def tracking_only(prob):
    """The same problem with every task term and both penalties off: lx = Q (x - x_ref), lu = R (u - u_ref), lxx = diag Q, luu = R."""
    p = dict(prob)
    p["task_weights"] = (0.0,) * 6
    p["w_joint"] = 0.0; p["w_ctrl"] = 0.0
    return p


def tracking_closed_form(prob, b, xs, us):
    """(lx [N+1,51], lu [N,19], lxx [N+1,51,51], luu [N,19], total cost) of tracking_only(prob) for reference set b, in plain NumPy."""
    N = prob["N"]
    Qd = np.tile(prob["Q"], (N + 1, 1)); Qd[N] = prob["Qf"]
    ex, eu = xs - prob["x_ref"][b], us - prob["u_ref"][b]
    lxx = np.zeros((N + 1, NX, NX)); lxx[:, np.arange(NX), np.arange(NX)] = Qd
    cost = 0.5 * (ex * Qd * ex).sum() + 0.5 * (eu * prob["R"] * eu).sum()
    return Qd * ex, prob["R"] * eu, lxx, np.tile(prob["R"], (N, 1)), cost


def _soft_bounds(rng_):
    lo = rng_[:, 0] + 0.1 * (rng_[:, 1] - rng_[:, 0]); hi = rng_[:, 1] - 0.1 * (rng_[:, 1] - rng_[:, 0])
    return lo, hi


def pen(val, rng_, w):
    lo, hi = _soft_bounds(rng_)
    return w * (np.maximum(val - hi, 0) ** 2 + np.maximum(lo - val, 0) ** 2).sum()


def pen_grad(val, rng_, w):
    lo, hi = _soft_bounds(rng_)
    return 2.0 * w * (np.maximum(val - hi, 0) - np.maximum(lo - val, 0))


def pen_hess(val, rng_, w):
    """diagonal of the Hessian: 2 w where the penalty is active"""
    lo, hi = _soft_bounds(rng_)
    return 2.0 * w * ((val > hi) | (val < lo))


def sweep_base_state():
    """The standing state, except that the two shoulder-roll hinges -- whose standing angle 0 lies 0.005 rad INSIDE their soft margin
    (ranges -0.34 .. 3.11 and -3.11 .. 0.34) -- are moved to 1 % of their range past its edge: no penalty entry is active."""
    jr = cost_golden()["jrange"]
    lo, hi = _soft_bounds(jr)
    x = sc.standing_state()
    x[7:NQ] = np.clip(x[7:NQ], lo + 0.01 * (jr[:, 1] - jr[:, 0]), hi - 0.01 * (jr[:, 1] - jr[:, 0]))
    return x


def limit_sweep(N, knot=1):
    """(X [76,N+1,51], U [76,N,19], cases): rollout 2 j + side puts hinge j (rollouts 0..37) or actuator j (38..75) 3 % of its range
    inside the lower (side 0) or upper (side 1) end at knot `knot` -- within the 10 % soft margin; everything else is
    sweep_base_state() under its gravity-compensation controls (shipped gravity).  cases[r] = (kind, j, side, value)."""
    c = cost_golden()
    prob = sc.make_problem(ol.reference_kinematics, N=N)
    o = ol.Oracle(N, prob["dt"]); o.set_problem(prob)
    X = np.tile(sweep_base_state(), (76, N + 1, 1))
    U = np.tile(o.grav_comp(sweep_base_state()), (76, N, 1))
    cases = []
    for kind, table, base in (("joint", c["jrange"], 0), ("ctrl", c["ctrlrange"], 38)):
        for j in range(19):
            lo, hi = table[j]
            for side, v in enumerate((lo + 0.03 * (hi - lo), hi - 0.03 * (hi - lo))):
                r = base + 2 * j + side
                if kind == "joint":
                    X[r, knot, 7 + j] = v
                else:
                    U[r, knot, j] = v
                cases.append((kind, j, side, float(v)))
    return X, U, cases
