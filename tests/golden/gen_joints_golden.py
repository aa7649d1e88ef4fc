#!/usr/bin/env python3
"""joints_golden.npz: single plant steps of a robot whose joints are not the model's (include/ilqr_hip.h ilqr_hip_plant_set_joints) -- a record
of gain g[19], range scale s[19], damping d[19] and armature a[19] -- in all six step kinds: contact modes 0-4, each without and with
joint-limit rows.

The NumPy Kane / KKT restatement of gen_golden.py is reused unchanged, by import: kane_step_c / kane_step_lim take per-joint vectors as they
are, and a step under a record is their step with
    ctrlrange * s[:, None],   g * u,   damping = d,   armature = a.
gen_wrench_golden.step_case (the step with its active set and decision margins) does not hand damping and armature on, so for the duration
of a call gen_golden.kane_step_c is replaced by a wrapper that passes the two (joints_applied), in the way gen_wrench_golden.wrench_applied
replaces kane_eval_c.  A wrench beside the record goes through that context, a payload through gen_payload_golden.with_payload.

Every case is kept only if each decision of its step is taken with a margin, the margins of gen_wrench_golden.py.  In modes 2, 3 and 4 and
among the cases with joint-limit rows at least one case stands on another active set (feet released / sliding, hinges stopped) than the
same state under the nominal record; main() asserts it.

Beside x_next the file keeps, per case: x_next_nominal (the same state and control under the model's joints, scalar arguments),
x_next_nominal_vectors (the nominal record given as four 19-vectors: main() asserts that it equals the former to 0.0), and x_next_mutant
[5]: the step of five WRONG readings of the record (MUTANTS).  main() asserts that every mutant misses x_next, in at least one case, by
1000 times the bound the GPU step is held to (1e-10 absolute in mode 0 without rows, 1e-9 relative to max(1, max |x_next|) otherwise), so
the cases tell the readings apart before any kernel runs.

   python tests/golden/gen_joints_golden.py
"""
import contextlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg             # noqa: E402
import gen_payload_golden as gp     # noqa: E402
import gen_wrench_golden as gw      # noqa: E402

TRIES = 12000
NOMINAL = np.concatenate([np.ones(57), 0.1 * np.ones(19)])
KNEE = 3                            # left knee, in the order of u
MUTANTS = ("gain_behind_clamp", "scale_ignored", "damping_not_in_armature", "mean_armature", "legs_swapped")
SWAP = np.concatenate([np.arange(5, 10), np.arange(0, 5), np.arange(10, 19)])
FREE_TOL, STEP_TOL = 1e-10, 1e-9    # the GPU step's bounds (tests/test_gpu_payload.py)


def fields(rec):
    return rec[0:19], rec[19:38], rec[38:57], rec[57:76]


@contextlib.contextmanager
def joints_applied(d, a):
    """gen_golden.kane_step_c takes damping d and armature a (scalars or 19-vectors) while the context is open"""
    orig = gg.kane_step_c

    def with_joints(*args, **kw):
        kw["damping"], kw["armature"] = d, a
        return orig(*args, **kw)

    gg.kane_step_c = with_joints
    try:
        yield
    finally:
        gg.kane_step_c = orig


def step_arguments(ctrl, u, rec, h, mutant=None):
    """(ctrlrange, u, damping, armature) of the step under rec; mutant: one of the wrong readings instead"""
    g, s, d, a = fields(rec)
    if mutant == "gain_behind_clamp":           # g clamp(u, s R): clamp(g u, g s R) for g > 0, 0 for g = 0
        return ctrl * (s * g)[:, None], g * u, d, a
    if mutant == "scale_ignored":
        return ctrl, g * u, d, a
    if mutant == "damping_not_in_armature":     # effective armature a + h DAMPING: kane_step_c adds h d itself
        return ctrl * s[:, None], g * u, d, a + h * (1.0 - d)
    if mutant == "mean_armature":
        return ctrl * s[:, None], g * u, d, np.full(19, a.mean())
    if mutant == "legs_swapped":
        return step_arguments(ctrl, u, np.concatenate([f[SWAP] for f in fields(rec)]), h)
    assert mutant is None, mutant
    return ctrl * s[:, None], g * u, d, a


def step_under(bodies, ctrl, rngj, x, u, h, grav, s, mu, rec, mutant=None):
    c2, u2, d, a = step_arguments(ctrl, u, rec, h, mutant)
    with joints_applied(d, a):
        return gw.step_case(bodies, c2, rngj, x, u2, h, grav, s["stance"], s["mode"], s["limits"], mu)


# one slot per case: contact mode, joint-limit rows, stance, the record's kind, a wrench / a payload beside it, a tilted pelvis, the active set
# must differ from the nominal twin's (contact part / stopped hinges), at least one hinge must be stopped
def slots():
    S = []

    def add(mode, limits, stance, kind, wrench=False, payload=False, tilt=False, change=False, lock_change=False, locked=False):
        S.append(dict(mode=mode, limits=limits, stance=stance, kind=kind, wrench=wrench, payload=payload, tilt=tilt, change=change, lock_change=lock_change, locked=locked))

    add(0, 0, (1, 1), "nominal"); add(0, 0, (1, 1), "gain"); add(0, 0, (1, 1), "scale"); add(0, 0, (1, 1), "damping"); add(0, 0, (1, 1), "armature")
    add(0, 0, (1, 1), "all", tilt=True); add(0, 0, (1, 1), "dead_knee"); add(0, 0, (1, 1), "gain_clamped"); add(0, 0, (1, 1), "scale_clamped")
    add(0, 0, (1, 1), "all", wrench=True); add(0, 0, (1, 1), "all", payload=True, tilt=True); add(0, 0, (1, 1), "damping", wrench=True, payload=True)
    add(0, 1, (1, 1), "nominal", locked=True); add(0, 1, (1, 1), "all", locked=True); add(0, 1, (1, 1), "big", lock_change=True); add(0, 1, (1, 1), "armature", wrench=True, locked=True)
    add(1, 0, (1, 1), "nominal"); add(1, 0, (1, 0), "all"); add(1, 0, (0, 1), "dead_knee", payload=True); add(1, 0, (1, 1), "gain_clamped", tilt=True)
    add(2, 0, (1, 1), "nominal"); add(2, 0, (1, 1), "big", change=True); add(2, 0, (1, 0), "scale_clamped")
    add(3, 0, (1, 1), "nominal"); add(3, 0, (1, 1), "big", change=True); add(3, 0, (0, 1), "damping", wrench=True)
    add(4, 0, (1, 1), "nominal"); add(4, 0, (1, 1), "big", change=True); add(4, 0, (1, 0), "all", tilt=True); add(4, 0, (0, 1), "armature", payload=True)
    add(1, 1, (1, 1), "all", locked=True)
    add(2, 1, (1, 1), "nominal", locked=True); add(2, 1, (1, 1), "gain", locked=True); add(2, 1, (1, 0), "big")
    add(3, 1, (1, 1), "all", wrench=True, locked=True)
    add(4, 1, (1, 1), "nominal", locked=True); add(4, 1, (1, 1), "big", locked=True); add(4, 1, (0, 1), "scale", tilt=True)
    return S


def draw_record(rng, kind, u, ctrl):
    """(record [76], u): the kinds that need a particular control change it"""
    rec, u = NOMINAL.copy(), u.copy()
    R = ctrl[:, 1]
    if kind in ("gain", "all", "big"):
        rec[0:19] = rng.uniform(0.5, 1.5, 19)
    if kind in ("scale", "all", "big", "scale_clamped"):
        rec[19:38] = rng.uniform(0.02, 0.6, 19)
    if kind in ("damping", "all", "big"):
        rec[38:57] = rng.uniform(0.3, 3.0, 19)
    if kind in ("armature", "all", "big"):
        rec[57:76] = rng.uniform(0.03, 0.3, 19)
    if kind == "big":                             # torques of the size of the ranges: the record decides which feet hold
        u = rng.uniform(-1.0, 1.0, 19) * R
    if kind == "dead_knee":
        rec[19 + KNEE] = 0.0
        u[KNEE] = rng.choice([-1.0, 1.0]) * rng.uniform(10.0, 20.0)
    if kind == "gain_clamped":                    # g u beyond the range on three of the small motors, u inside it
        for i in rng.choice(np.flatnonzero(R <= 40.0), size=3, replace=False):
            u[i] = rng.choice([-1.0, 1.0]) * rng.uniform(5.0, 15.0)
            rec[i] = 1.3 * R[i] / abs(u[i])
    return rec, u


def bound_units(got, want, free):
    """the error in units of the bound the GPU step is held to"""
    if free:
        return float(np.abs(got - want).max()) / FREE_TOL
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max())) / STEP_TOL


def main():
    bodies, ctrl = gg.load_mjcf()
    rngj = np.array([b["rng"] for b in bodies if b["rng"] is not None])
    rng = np.random.default_rng(2036)
    h, grav = 0.02, np.array([0.0, 0.0, -9.81])
    keys = ("x", "u", "stance", "contact", "limits", "mu", "joints", "wrench", "payload", "x_next", "x_next_nominal", "x_next_nominal_vectors", "x_next_mutant", "act", "slide", "lock",
            "changed", "kind")
    out = {k: [] for k in keys}
    tries = 0
    for s in slots():
        found = False
        ws = dict(s, kind="both" if s["wrench"] else "zero", r=s["wrench"])      # the draw of gen_wrench_golden: state, control, wrench, friction
        while not found and tries < TRIES:
            tries += 1
            x, u, F, T, r, mu = gw.draw(rng, rngj, ws, tries)
            pl = gp.draw_payload(rng, "inertia") if s["payload"] else np.zeros(10)
            rec, u = draw_record(rng, s["kind"], u, ctrl)
            bl = gp.with_payload(bodies, pl) if s["payload"] else bodies
            with (gw.wrench_applied(F, T, r) if s["wrench"] else contextlib.nullcontext()):
                xn0, sig0, ok0 = gw.step_case(bl, ctrl, rngj, x, u, h, grav, s["stance"], s["mode"], s["limits"], mu)
                if s["kind"] == "nominal":
                    xn, sig, ok = xn0, sig0, ok0
                else:
                    xn, sig, ok = step_under(bl, ctrl, rngj, x, u, h, grav, s, mu, rec)
                if not ok or (s["locked"] and not sig[2]) or (s["change"] and sig[:2] == sig0[:2]) or (s["lock_change"] and sig[2] == sig0[2]):
                    continue
                if s["kind"] != "nominal" and not np.abs(xn - xn0).max() > 1e-6:
                    continue
                g_, s_, _, _ = fields(rec)
                R = ctrl[:, 1]
                if s["kind"] == "gain_clamped" and not ((np.abs(u) < R) & (np.abs(g_ * u) > s_ * R)).any():
                    continue
                if s["kind"] == "scale_clamped" and not ((np.abs(u) < R) & (np.abs(u) > s_ * R)).any():
                    continue
                xnv, sigv, _ = step_under(bl, ctrl, rngj, x, u, h, grav, s, mu, NOMINAL)
                assert np.array_equal(xnv, xn0) and sigv == sig0, "the nominal record as vectors is the scalar step, to 0.0"
                muts = [step_under(bl, ctrl, rngj, x, u, h, grav, s, mu, rec, m)[0] for m in MUTANTS]
            found = True
            lk = np.zeros(19, dtype=int); lk[list(sig[2])] = 1
            for k, val in (("x", x), ("u", u), ("stance", np.array(s["stance"])), ("contact", s["mode"]), ("limits", s["limits"]), ("mu", mu), ("joints", rec),
                           ("wrench", np.concatenate([F, T, r])), ("payload", pl), ("x_next", xn), ("x_next_nominal", xn0), ("x_next_nominal_vectors", xnv),
                           ("x_next_mutant", np.array(muts)), ("act", np.array(sig[0])), ("slide", np.array(sig[1])), ("lock", lk), ("changed", int(sig != sig0)),
                           ("kind", s["kind"])):
                out[k].append(val)
        assert found, ("pattern not found within the try budget", s, tries)
    n = len(out["x"])
    assert n <= 40
    contact, limits, changed = np.array(out["contact"]), np.array(out["limits"]), np.array(out["changed"])
    for mode in range(5):
        assert (np.array(out["kind"])[contact == mode] == "nominal").any(), ("no nominal case in mode", mode)
    for mode in (2, 3, 4):
        assert changed[contact == mode].any(), ("no changed active set in mode", mode)
    assert changed[limits == 1].any(), "no changed active set under joint-limit rows"
    X, XM = np.array(out["x_next"]), np.array(out["x_next_mutant"])
    miss = {m: max(bound_units(XM[i, k], X[i], contact[i] == 0 and not limits[i]) for i in range(n)) for k, m in enumerate(MUTANTS)}
    assert min(miss.values()) >= 1000.0, miss
    np.savez_compressed(os.path.join(HERE, "joints_golden.npz"), h=h, gravity=grav, soft=1e-5, ctrlrange=ctrl[:, 1], mutants=np.array(MUTANTS),
                        **{k: np.array(v) for k, v in out.items()})
    print("joints golden:", n, "cases in", tries, "draws; changed active sets:", changed.tolist())
    print("mutants miss x_next by (units of the GPU step bound):", {m: "%.2e" % v for m, v in miss.items()})


if __name__ == "__main__":
    main()
