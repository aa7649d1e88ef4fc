#!/usr/bin/env python3
"""payload_golden.npz: single plant steps of a robot whose pelvis carries a rigid payload (include/ilqr_hip.h ilqr_hip_plant_set_payload), in
all six step kinds -- contact modes 0-4, each without and with joint-limit rows.

The NumPy Kane / KKT restatement of gen_golden.py is reused unchanged, by import: the payload is MERGED INTO BODY 0 of the `bodies` list by
the parallel-axis theorem,
    m' = m + mp        c' = (m c + mp cp) / m'        I' = I + m P(c - c') + Ic + mp P(cp - c'),    P(r) = |r|^2 E - r r^T,
and kane_step_c / kane_step_lim run on that list as they are -- one composite rigid body through Kane's equations.  The kernels add a
spatial inertia to an articulated one in the pelvis frame; the two share no code path.  A wrench beside the payload goes through
gen_wrench_golden.wrench_applied, by import as well.

Every case is kept only if each decision of its step is taken with a margin, the margins of gen_wrench_golden.py: a normal force below
1 N (the unilateral release and the cone check), a foot within 5 % of the cone's surface, a limit decision with |v_i+| < 0.05 rad/s reject
the draw.  In modes 2, 3 and 4 at least one case stands on another active set (feet released / sliding / hinges stopped apart) than the
same state without the payload; main() asserts it, so the draw budget yielded one for each of the three modes.

   python tests/golden/gen_payload_golden.py
"""
import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg            # noqa: E402
import gen_wrench_golden as gw     # noqa: E402

TRIES = 8000
PELVIS_MASS = 5.39


def inertia_matrix(i6):
    xx, yy, zz, xy, xz, yz = i6
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def par(r):
    return (r @ r) * np.eye(3) - np.outer(r, r)


def with_payload(bodies, pl):
    """the list with the payload pl [10] merged into body 0 (the pelvis): a composite rigid body"""
    mp, cp, Ic = float(pl[0]), np.asarray(pl[1:4], dtype=np.float64), inertia_matrix(pl[4:10])
    b0 = dict(bodies[0])
    m, c, I = b0["m"], b0["c"], b0["I"]
    m2 = m + mp
    c2 = (m * c + mp * cp) / m2
    b0.update(m=m2, c=c2, I=I + m * par(c - c2) + Ic + mp * par(cp - c2))
    return [b0] + list(bodies[1:])


def random_inertia(rng, scale):
    A = rng.normal(size=(3, 3))
    I = scale * (A @ A.T / 3.0 + 0.05 * np.eye(3))
    return np.array([I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]])


# one slot per case: contact mode, joint-limit rows, stance, the payload's kind, a wrench beside it, a tilted pelvis, the active set must
# differ from the unloaded twin's, at least one hinge must be stopped
def slots():
    S = []

    def add(mode, limits, stance, kind, wrench=False, tilt=False, change=False, locked=False):
        S.append(dict(mode=mode, limits=limits, stance=stance, kind=kind, wrench=wrench, tilt=tilt, change=change, locked=locked))

    add(0, 0, (1, 1), "zero"); add(0, 0, (1, 1), "point0"); add(0, 0, (1, 1), "point"); add(0, 0, (1, 1), "inertia"); add(0, 0, (1, 1), "heavy", tilt=True)
    add(0, 0, (1, 1), "inertia", wrench=True)
    add(0, 1, (1, 1), "zero", locked=True); add(0, 1, (1, 1), "point", locked=True); add(0, 1, (1, 1), "heavy", tilt=True, locked=True); add(0, 1, (1, 1), "inertia", wrench=True)
    add(1, 0, (1, 1), "zero"); add(1, 0, (1, 0), "point"); add(1, 0, (0, 1), "heavy"); add(1, 0, (1, 1), "inertia", tilt=True)
    add(2, 0, (1, 1), "zero"); add(2, 0, (1, 1), "heavy", change=True); add(2, 0, (1, 0), "point0")
    add(3, 0, (1, 1), "zero"); add(3, 0, (1, 1), "heavy", change=True); add(3, 0, (0, 1), "inertia", wrench=True)
    add(4, 0, (1, 1), "zero"); add(4, 0, (1, 1), "heavy", change=True); add(4, 0, (1, 0), "point", tilt=True); add(4, 0, (0, 1), "inertia")
    add(1, 1, (1, 1), "point", locked=True)
    add(2, 1, (1, 1), "zero", locked=True); add(2, 1, (1, 1), "inertia", locked=True); add(2, 1, (1, 0), "heavy")
    add(3, 1, (1, 1), "heavy", wrench=True, locked=True)
    add(4, 1, (1, 1), "zero", locked=True); add(4, 1, (1, 1), "inertia", locked=True); add(4, 1, (0, 1), "heavy", tilt=True)
    return S


def draw_payload(rng, kind):
    pl = np.zeros(10)
    if kind == "zero":
        return pl
    if kind == "heavy":
        pl[0] = 20.0                                               # against the pelvis' 5.39 kg
        pl[1:4] = np.array([-0.1, 0.0, 0.3]) + rng.uniform(-0.08, 0.08, 3)      # a backpack at torso height, off the midline
        pl[4:10] = random_inertia(rng, 0.4)
        return pl
    pl[0] = rng.uniform(2.0, 12.0)
    if kind in ("point", "inertia"):
        pl[1:4] = rng.uniform(-0.3, 0.3, 3)
    if kind == "inertia":
        pl[4:10] = random_inertia(rng, rng.uniform(0.05, 0.3))
    return pl


def main():
    bodies, ctrl = gg.load_mjcf()
    assert abs(bodies[0]["m"] - PELVIS_MASS) < 1e-9
    rngj = np.array([b["rng"] for b in bodies if b["rng"] is not None])
    rng = np.random.default_rng(2033)
    h, grav = 0.02, np.array([0.0, 0.0, -9.81])
    out = dict(x=[], u=[], stance=[], contact=[], limits=[], mu=[], payload=[], wrench=[], x_next=[], x_next_nopayload=[], act=[], slide=[], lock=[], changed=[])
    tries = 0
    for s in slots():
        found = False
        ws = dict(s, kind="both" if s["wrench"] else "zero", r=s["wrench"])      # the draw of gen_wrench_golden: state, control, wrench, friction
        while not found and tries < TRIES:
            tries += 1
            x, u, F, T, r, mu = gw.draw(rng, rngj, ws, tries)
            pl = draw_payload(rng, s["kind"])
            ctx = gw.wrench_applied(F, T, r) if s["wrench"] else contextlib.nullcontext()
            with ctx:
                xn0, sig0, ok0 = gw.step_case(bodies, ctrl, rngj, x, u, h, grav, s["stance"], s["mode"], s["limits"], mu)
                if s["kind"] == "zero":
                    xn, sig, ok = xn0, sig0, ok0
                else:
                    xn, sig, ok = gw.step_case(with_payload(bodies, pl), ctrl, rngj, x, u, h, grav, s["stance"], s["mode"], s["limits"], mu)
            if not ok or (s["locked"] and not sig[2]) or (s["change"] and sig[:2] == sig0[:2]):
                continue
            if s["kind"] != "zero" and not np.abs(xn - xn0).max() > 1e-6:
                continue
            found = True
            lk = np.zeros(19, dtype=int); lk[list(sig[2])] = 1
            for k, val in (("x", x), ("u", u), ("stance", np.array(s["stance"])), ("contact", s["mode"]), ("limits", s["limits"]), ("mu", mu), ("payload", pl),
                           ("wrench", np.concatenate([F, T, r])), ("x_next", xn), ("x_next_nopayload", xn0), ("act", np.array(sig[0])), ("slide", np.array(sig[1])),
                           ("lock", lk), ("changed", int(sig != sig0))):
                out[k].append(val)
        assert found, ("pattern not found within the try budget", s, tries)
    n = len(out["x"])
    assert n <= 40
    contact, changed, PL = np.array(out["contact"]), np.array(out["changed"]), np.array(out["payload"])
    for mode in range(5):
        assert (np.abs(PL[contact == mode]).max(axis=1) == 0).any(), ("no zero-payload case in mode", mode)
    for mode in (2, 3, 4):
        assert changed[contact == mode].any(), ("no changed active set in mode", mode)
    np.savez(os.path.join(HERE, "payload_golden.npz"), h=h, gravity=grav, soft=1e-5, pelvis_mass=bodies[0]["m"], **{k: np.array(v) for k, v in out.items()})
    print("payload golden:", n, "cases in", tries, "draws; changed active sets:", changed.tolist())


if __name__ == "__main__":
    main()
