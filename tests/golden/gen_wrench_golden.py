#!/usr/bin/env python3
"""wrench_golden.npz: single plant steps under an external wrench on the pelvis (include/ilqr_hip.h ilqr_hip_plant_set_wrench), in all six
step kinds -- contact modes 0-4, each without and with joint-limit rows.

The NumPy Kane / KKT restatement of gen_golden.py is reused unchanged, by import.  For the duration of a call gen_golden.kane_eval_c is
replaced by a wrapper that subtracts the generalized force of the wrench,
    Wg = [F ; R0^T T + r x (R0^T F)]      (F, T world frame, r pelvis frame, R0 the pelvis rotation; conjugate to qvel[0:6]),
from the first six entries of the generalized force it returns.  kane_step_c builds M = cols - bias (the wrench cancels: M is unaffected)
and rhs = tau - D v - bias (gains + Wg), and kane_step_c / kane_step_lim then solve every mode -- stance rows, unilateral release, Coulomb
check, kinetic friction, joint-limit rows -- with it.

Every case is kept only if each decision of its step is taken with a margin, the margins of gen_friction / gen_limits: a normal force
below 1 N (the unilateral release and the cone check), a foot within 5 % of the cone's surface, a limit decision with |v_i+| < 0.05 rad/s
reject the draw.  Contact mode 1 is bilateral and has no active set; in modes 2, 3 and 4 at least one case stands on another active set
(feet released / sliding) than the same state without the wrench.

   python tests/golden/gen_wrench_golden.py
"""
import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg      # noqa: E402

F_MAX, T_MAX = 150.0, 40.0
TRIES = 6000


def generalized_force(q, F, T, r):
    R0 = gg.q2R_c(q[3:7])
    Fb = R0.T @ F
    return np.concatenate([F, R0.T @ T + np.cross(r, Fb)])


@contextlib.contextmanager
def wrench_applied(F, T, r):
    """gen_golden.kane_eval_c returns its generalized force less Wg on the base rows while the context is open"""
    orig = gg.kane_eval_c

    def with_wrench(bodies, q, v, qacc, grav, armature):
        Fg, feet = orig(bodies, q, v, qacc, grav, armature)
        Fg = Fg.copy()
        Fg[0:6] = Fg[0:6] - generalized_force(q, F, T, r)
        return Fg, feet

    gg.kane_eval_c = with_wrench
    try:
        yield
    finally:
        gg.kane_eval_c = orig


def contact_margins_ok(bodies, ctrl, x, u, h, grav, stance, mode, mu, lock, lock_acc):
    """the decisions kane_step_c takes in `mode` with the hinges `lock` prescribed: the unilateral check reads the rigid solution (mode 1),
    the Coulomb check the solution behind the release (mode 2)"""
    if mode < 2:
        return True
    _, feet0 = gg.kane_eval_c(bodies, x[:26], x[26:], np.zeros(25), grav, 0.1)
    kw = dict(stance=stance, want=True, lock=lock, lock_acc=lock_acc)
    _, _, _, lam1, act1, _ = gg.kane_step_c(bodies, ctrl, x, u, h, grav, contact=1, **kw)
    for f in range(2):
        if act1[f] and abs(feet0[f]["up"] @ lam1[6 * f + 3:6 * f + 6]) < 1.0:
            return False
    if mode >= 3:
        _, _, _, lam2, act2, _ = gg.kane_step_c(bodies, ctrl, x, u, h, grav, contact=2, **kw)
        for f in range(2):
            if not act2[f]:
                continue
            fo = lam2[6 * f + 3:6 * f + 6]; fn = feet0[f]["up"] @ fo; ft = np.sqrt(max(fo @ fo - fn * fn, 0.0))
            if fn < 1.0 or abs(ft / (mu * fn) - 1.0) < 0.05:
                return False
    return True


def step_case(bodies, ctrl, rngj, x, u, h, grav, stance, mode, limits, mu):
    """(x_next, signature, ok): the step under whatever wrench is applied, its active set (stance feet, sliding feet, stopped hinges), and
    whether every decision kept its margin"""
    kw = dict(stance=stance, contact=mode, mu=mu)
    ok = contact_margins_ok(bodies, ctrl, x, u, h, grav, stance, mode, mu, (), None)
    lock = []
    if limits:
        xn, lock, _, margin = gg.kane_step_lim(bodies, ctrl, x, u, h, grav, **kw)
        ok = ok and margin >= 0.05
        if lock:
            ok = ok and contact_margins_ok(bodies, ctrl, x, u, h, grav, stance, mode, mu, tuple(lock), None)
    _, _, _, _, act, slide = gg.kane_step_c(bodies, ctrl, x, u, h, grav, want=True, lock=tuple(lock), **kw)
    if not limits:
        xn = gg.kane_step_c(bodies, ctrl, x, u, h, grav, **kw)
    sig = (tuple(int(a) for a in act), tuple(int(s) for s in slide), tuple(int(i) for i in lock))
    return xn, sig, bool(ok and np.all(np.isfinite(xn)))


# one slot per case: contact mode, joint-limit rows, stance, what the wrench consists of, r != 0, a tilted pelvis, the active set must differ
# from the no-wrench twin's (contact part), at least one hinge must be stopped
def slots():
    S = []

    def add(mode, limits, stance, kind, r=False, tilt=False, change=False, locked=False):
        S.append(dict(mode=mode, limits=limits, stance=stance, kind=kind, r=r, tilt=tilt, change=change, locked=locked))

    add(0, 0, (1, 1), "zero"); add(0, 0, (1, 1), "force"); add(0, 0, (1, 1), "torque"); add(0, 0, (1, 1), "both", r=True); add(0, 0, (1, 1), "both", r=True, tilt=True)
    add(0, 1, (1, 1), "zero", locked=True); add(0, 1, (1, 1), "force", r=True, locked=True); add(0, 1, (1, 1), "both", tilt=True, locked=True); add(0, 1, (1, 1), "torque")
    add(1, 0, (1, 1), "zero"); add(1, 0, (1, 0), "force", r=True); add(1, 0, (0, 1), "both"); add(1, 0, (1, 1), "torque", tilt=True)
    add(2, 0, (1, 1), "zero"); add(2, 0, (1, 1), "both", change=True); add(2, 0, (1, 0), "force")
    add(3, 0, (1, 1), "zero"); add(3, 0, (1, 1), "both", r=True, change=True); add(3, 0, (0, 1), "torque")
    add(4, 0, (1, 1), "zero"); add(4, 0, (1, 1), "both", change=True); add(4, 0, (1, 0), "force", r=True, tilt=True); add(4, 0, (0, 1), "torque")
    add(1, 1, (1, 1), "force", locked=True)
    add(2, 1, (1, 1), "zero", locked=True); add(2, 1, (1, 1), "both", r=True, locked=True); add(2, 1, (1, 0), "force")
    add(3, 1, (1, 1), "both", locked=True)
    add(4, 1, (1, 1), "zero", locked=True); add(4, 1, (1, 1), "both", locked=True); add(4, 1, (0, 1), "force", r=True); add(4, 1, (1, 0), "torque", tilt=True)
    return S


def draw(rng, rngj, s, tries):
    x = np.zeros(51); x[2] = 1.0432; x[3] = 1.0
    x[0:3] += rng.uniform(-0.02, 0.02, 3)
    amp = 0.4 if s["tilt"] else 0.05
    aa = rng.uniform(-amp, amp, 3); ang = np.linalg.norm(aa); x[3] = np.cos(ang / 2); x[4:7] = np.sin(ang / 2) / ang * aa
    x[7:26] = rng.uniform(-0.15, 0.15, 19)
    x[26:] = rng.uniform(-0.4, 0.4, 25)
    if s["limits"]:
        for i in rng.choice(19, size=int(rng.integers(1, 4)), replace=False):
            up = rng.random() < 0.5
            x[7 + i] = rngj[i, 1] + rng.uniform(0.01, 0.08) if up else rngj[i, 0] - rng.uniform(0.01, 0.08)
            x[32 + i] = rng.uniform(0.3, 2.0) * (1 if up else -1) * (1 if rng.random() < 0.75 else -1)
    u = rng.uniform(-20, 20, 19)
    F, T, r = np.zeros(3), np.zeros(3), np.zeros(3)
    if s["kind"] in ("force", "both"):
        d = rng.normal(size=3); F = d / np.linalg.norm(d) * rng.uniform(50.0, F_MAX)
    if s["kind"] in ("torque", "both"):
        d = rng.normal(size=3); T = d / np.linalg.norm(d) * rng.uniform(10.0, T_MAX)
    if s["r"]:
        r = rng.uniform(-0.15, 0.15, 3)
    mu = [1.0, 0.6, 0.3][tries % 3]
    return x, u, F, T, r, mu


def main():
    bodies, ctrl = gg.load_mjcf()
    rngj = np.array([b["rng"] for b in bodies if b["rng"] is not None])
    rng = np.random.default_rng(2032)
    h, grav = 0.02, np.array([0.0, 0.0, -9.81])
    out = dict(x=[], u=[], stance=[], contact=[], limits=[], mu=[], wrench=[], x_next=[], x_next_nowrench=[], act=[], slide=[], lock=[], changed=[])
    tries = 0
    for s in slots():
        found = False
        while not found and tries < TRIES:
            tries += 1
            x, u, F, T, r, mu = draw(rng, rngj, s, tries)
            xn0, sig0, ok0 = step_case(bodies, ctrl, rngj, x, u, h, grav, s["stance"], s["mode"], s["limits"], mu)
            if s["kind"] == "zero":
                xn, sig, ok = xn0, sig0, ok0
            else:
                with wrench_applied(F, T, r):
                    xn, sig, ok = step_case(bodies, ctrl, rngj, x, u, h, grav, s["stance"], s["mode"], s["limits"], mu)
            if not ok or (s["locked"] and not sig[2]) or (s["change"] and sig[:2] == sig0[:2]):
                continue
            if s["kind"] != "zero" and not np.abs(xn - xn0).max() > 1e-6:
                continue
            found = True
            lk = np.zeros(19, dtype=int); lk[list(sig[2])] = 1
            for k, val in (("x", x), ("u", u), ("stance", np.array(s["stance"])), ("contact", s["mode"]), ("limits", s["limits"]), ("mu", mu),
                           ("wrench", np.concatenate([F, T, r])), ("x_next", xn), ("x_next_nowrench", xn0), ("act", np.array(sig[0])), ("slide", np.array(sig[1])),
                           ("lock", lk), ("changed", int(sig != sig0))):
                out[k].append(val)
        assert found, ("pattern not found within the try budget", s, tries)
    n = len(out["x"])
    assert n <= 40
    contact, changed, W = np.array(out["contact"]), np.array(out["changed"]), np.array(out["wrench"])
    for mode in range(5):
        assert (np.abs(W[contact == mode]).max(axis=1) == 0).any(), ("no zero-wrench case in mode", mode)
    for mode in (2, 3, 4):
        assert changed[contact == mode].any(), ("no changed active set in mode", mode)
    np.savez(os.path.join(HERE, "wrench_golden.npz"), h=h, gravity=grav, soft=1e-5, pelvis_com=bodies[0]["c"], **{k: np.array(v) for k, v in out.items()})
    print("wrench golden:", n, "cases in", tries, "draws; changed active sets:", changed.tolist())


if __name__ == "__main__":
    main()
