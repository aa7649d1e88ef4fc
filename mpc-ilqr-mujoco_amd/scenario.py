"""Problem data and synthetic batches for the H1 iLQR hot path (host-side, numpy only).

Mirrors the reference's configuration rules:
  * Config::buildCostMatrices      /root/reference/src/common/config.cpp:66-122 (diagonal Q, R, Qf)
  * shipped weights                /root/reference/config.yaml:24-58
  * standing pose                  /root/reference/src/common/robot_utils.cpp:567-583, data/q_standing.csv
  * reference construction         /root/reference/src/common/robot_utils.cpp:355-413 (com / foot refs by FK)
  * synthetic batch distributions  SURVEY.md section 8(d)
"""
import numpy as np

NQ, NV, NX, NU = 26, 25, 51, 19

# /root/reference/config.yaml:24-58 (as shipped)
SHIPPED_CONFIG = dict(
    Q_position_x=200.0, Q_position_y=50.0, Q_position_z=200.0, Q_quat_w=50.0, Q_quat_xyz=(50.0, 50.0, 50.0),
    Q_joint_pos=50.0, Q_vel_x=150.0, Q_vel_y=50.0, Q_vel_z=150.0, Q_ang_vel=75.0, Q_joint_vel=75.0,
    R_control=0.001, Qf_multiplier=2.0, Qf_position_x=5.0, Qf_position_y=2.0, Qf_position_z=5.0, Qf_vel_z=4.0,
    W_com_pos=100.0, W_com_vel=0.0, W_foot=400.0, W_foot_vel=400.0, W_upright=20.0, w_balance=30.0,
    joint_limit_weight=1500.0, torque_limit_weight=1500.0,
    gravity=(0.0, 0.0, -1.0), horizon=25, dt=0.02,
)

# /root/reference/robots/h1_description/mjcf/h1.xml:191-209
CTRLRANGE = np.array([200, 200, 200, 300, 40, 200, 200, 200, 300, 40, 200, 40, 40, 18, 18, 40, 40, 18, 18], dtype=np.float64)


def build_cost_matrices(cfg=SHIPPED_CONFIG):
    """Diagonals of Q, R, Qf exactly as Config::buildCostMatrices (config.cpp:66-122)."""
    Q = np.ones(NX)
    Q[0], Q[1], Q[2] = cfg["Q_position_x"], cfg["Q_position_y"], cfg["Q_position_z"]
    Q[3] = cfg["Q_quat_w"]
    Q[4:7] = cfg["Q_quat_xyz"]
    Q[7:NQ] = cfg["Q_joint_pos"]
    Q[NQ + 0], Q[NQ + 1], Q[NQ + 2] = cfg["Q_vel_x"], cfg["Q_vel_y"], cfg["Q_vel_z"]
    Q[NQ + 3:NQ + 6] = cfg["Q_ang_vel"]
    Q[NQ + 6:] = cfg["Q_joint_vel"]
    R = np.ones(NU) * cfg["R_control"]
    Qf = Q * cfg["Qf_multiplier"]
    Qf[0] *= cfg["Qf_position_x"]
    Qf[1] *= cfg["Qf_position_y"]
    Qf[2] *= cfg["Qf_position_z"]
    Qf[NQ + 2] *= cfg["Qf_vel_z"]
    return Q, R, Qf


def standing_state():
    x = np.zeros(NX)
    x[2] = 1.0432
    x[3] = 1.0
    return x


def make_problem(kin, N=25, cfg=SHIPPED_CONFIG, x_ref=None, stance=None, gravity=None):
    """Shared-reference problem dict. `kin(x) -> (com[3], ee[2,3])` supplies the FK used by
    loadReferences (robot_utils.cpp:369-403). x_ref: [N+1,51] (default: standing row repeated)."""
    Q, R, Qf = build_cost_matrices(cfg)
    if x_ref is None:
        x_ref = np.tile(standing_state(), (N + 1, 1))
    x_ref = np.asarray(x_ref, dtype=np.float64).reshape(1, N + 1, NX)
    com_ref = np.zeros((1, N + 1, 3))
    ee_ref = np.zeros((1, N + 1, 2, 3))
    for t in range(N + 1):
        com_ref[0, t], ee_ref[0, t] = kin(x_ref[0, t])
    if stance is None:
        stance = np.ones((N + 1, 2), dtype=np.int32)
    return dict(
        N=N, dt=cfg["dt"], Q=Q, R=R, Qf=Qf,
        task_weights=(cfg["W_com_pos"], cfg["W_com_vel"], cfg["W_foot"], cfg["W_foot_vel"], cfg["W_upright"], cfg["w_balance"]),
        w_joint=cfg["joint_limit_weight"], w_ctrl=cfg["torque_limit_weight"],
        gravity=tuple(cfg["gravity"] if gravity is None else gravity),
        x_ref=x_ref, u_ref=np.zeros((1, N, NU)), com_ref=com_ref,
        stance=np.asarray(stance, dtype=np.int32).reshape(1, N + 1, 2), ee_ref=ee_ref,
        com_vel_ref=np.zeros((1, N + 1, 3)),
    )


WEIGHT_KEYS = ("Q", "R", "Qf", "task_weights", "w_joint", "w_ctrl")


def stack_weight_sets(problem, sets):
    """Problem dict for a weight sweep: rollout b solves `problem` under the weights of sets[b], a dict that overrides any of Q, R, Qf,
    task_weights, w_joint, w_ctrl (what it leaves out keeps the base value).  The six items come back stacked on a leading axis of
    len(sets) -- Q [B,51], R [B,19], Qf [B,51], task_weights [B,6], w_joint [B], w_ctrl [B] -- which BatchedILQR.set_problem installs as
    per-rollout weight sets; everything else is shared with `problem`."""
    for b, ov in enumerate(sets):
        bad = set(ov) - set(WEIGHT_KEYS)
        if bad:
            raise KeyError("set %d overrides %s: only %s vary per rollout" % (b, sorted(bad), ", ".join(WEIGHT_KEYS)))
    out = dict(problem)
    for k in WEIGHT_KEYS:
        out[k] = np.stack([np.asarray(ov.get(k, problem[k]), dtype=np.float64) for ov in sets])
    return out


# what a solver handle holds before any setter is called (ilqr_hip_create): gravity, friction coefficient, contact softness, joint-limit stiffness
PLANT_PARAM_DEFAULTS = dict(gravity=(0.0, 0.0, -9.81), friction=1.0, softness=1e-5, limit_stiffness=0.0, torque_gain=1.0)


def stack_plant_params(B, gravity=None, friction=None, softness=None, limit_stiffness=None, torque_gain=None):
    """Plant parameter sets [B, 7] for BatchedILQR.plant_set_params / MPCRunner(plant_params=...): columns gravity x, y, z, friction
    coefficient, contact softness, joint-limit stiffness, torque gain.  Each argument is one value for all rollouts (gravity: 3 values) or
    one per rollout (gravity [B, 3], the others [B]); None is the handle's default (PLANT_PARAM_DEFAULTS).  Raises ValueError for a shape
    that is neither, a non-finite entry, friction < 0, softness <= 0, limit_stiffness < 0 or torque_gain < 0."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be positive")
    d = PLANT_PARAM_DEFAULTS
    out = np.empty((B, 7))
    g = np.asarray(d["gravity"] if gravity is None else gravity, dtype=np.float64)
    if g.shape not in ((3,), (B, 3)):
        raise ValueError("gravity must be [3] or [B, 3]")
    out[:, 0:3] = g
    for col, name, val in ((3, "friction", friction), (4, "softness", softness), (5, "limit_stiffness", limit_stiffness), (6, "torque_gain", torque_gain)):
        v = np.asarray(d[name] if val is None else val, dtype=np.float64)
        if v.shape not in ((), (B,)):
            raise ValueError("%s must be a scalar or [B]" % name)
        out[:, col] = v
    if not np.isfinite(out).all():
        raise ValueError("plant parameters must be finite")
    if (out[:, 3] < 0).any() or (out[:, 4] <= 0).any() or (out[:, 5] < 0).any() or (out[:, 6] < 0).any():
        raise ValueError("friction >= 0, softness > 0, limit_stiffness >= 0 and torque_gain >= 0 are required")
    return out


def stack_plant_wrench(B, force=None, torque=None, point=None, first=0, end=np.inf):
    """External wrenches on the pelvis [B, 11] for BatchedILQR.plant_set_wrench / MPCRunner(plant_wrench=...): columns force x, y, z (world
    frame, N), torque x, y, z (world frame, N m), point of application x, y, z (pelvis frame, m; solver.pelvis_inertial_offset() is
    MuJoCo's xfrc_applied), first and end of the window of plant intervals the wrench acts in (first <= i < end, counted from plant_reset).
    Each vector is [3] for all rollouts or [B, 3], None is zero; first / end are a scalar or [B], end may be inf.  Raises ValueError for a
    shape that is neither, a non-finite entry other than end = inf, a negative or non-integral first / end, or end < first."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be positive")
    out = np.empty((B, 11))
    for col, name, val in ((0, "force", force), (3, "torque", torque), (6, "point", point)):
        v = np.zeros(3) if val is None else np.asarray(val, dtype=np.float64)
        if v.shape not in ((3,), (B, 3)):
            raise ValueError("%s must be [3] or [B, 3]" % name)
        out[:, col:col + 3] = v
    for col, name, val in ((9, "first", first), (10, "end", end)):
        v = np.asarray(val, dtype=np.float64)
        if v.shape not in ((), (B,)):
            raise ValueError("%s must be a scalar or [B]" % name)
        out[:, col] = v
    if not np.isfinite(out[:, :10]).all() or np.isnan(out[:, 10]).any() or (out[:, 10] == -np.inf).any():
        raise ValueError("plant wrenches must be finite (end may be inf)")
    fin_end = np.where(np.isfinite(out[:, 10]), out[:, 10], 0.0)
    if (out[:, 9] < 0).any() or (out[:, 10] < 0).any() or (out[:, 9] != np.floor(out[:, 9])).any() or (fin_end != np.floor(fin_end)).any():
        raise ValueError("first and end must be non-negative integers")
    if (out[:, 10] < out[:, 9]).any():
        raise ValueError("end >= first is required")
    return out


def stack_plant_payload(B, mass, com=None, inertia=None):
    """Rigid payloads on the pelvis [B, 10] for BatchedILQR.plant_set_payload / MPCRunner(plant_payload=...): columns mass (kg), centre of
    mass x, y, z (pelvis frame, m), Ixx, Iyy, Izz, Ixy, Ixz, Iyz of the rotational inertia about the payload's own centre of mass (pelvis
    axes, kg m^2).  mass is a scalar or [B]; com [3] or [B, 3], None the pelvis origin; inertia [6] or [B, 6], None a point mass.  Raises
    ValueError for a shape that is neither, a non-finite entry, a negative mass or an inertia that is not positive semidefinite -- what
    ilqr_hip_plant_set_payload refuses."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be positive")
    out = np.empty((B, 10))
    m = np.asarray(mass, dtype=np.float64)
    if m.shape not in ((), (B,)):
        raise ValueError("mass must be a scalar or [B]")
    out[:, 0] = m
    for col, n, name, val in ((1, 3, "com", com), (4, 6, "inertia", inertia)):
        v = np.zeros(n) if val is None else np.asarray(val, dtype=np.float64)
        if v.shape not in ((n,), (B, n)):
            raise ValueError("%s must be [%d] or [B, %d]" % (name, n, n))
        out[:, col:col + n] = v
    if not np.isfinite(out).all():
        raise ValueError("plant payloads must be finite")
    if (out[:, 0] < 0).any():
        raise ValueError("mass >= 0 is required")
    xx, yy, zz, xy, xz, yz = (out[:, 4 + k] for k in range(6))
    eps = 1e-12
    det = xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz)
    mag = np.abs(xx * yy * zz) + np.abs(xx * yz * yz) + np.abs(xy * xy * zz) + 2.0 * np.abs(xy * yz * xz) + np.abs(yy * xz * xz)
    bad = (xx < 0) | (yy < 0) | (zz < 0) | (xx * yy - xy * xy < -eps * (xx * yy + xy * xy)) | (xx * zz - xz * xz < -eps * (xx * zz + xz * xz)) \
        | (yy * zz - yz * yz < -eps * (yy * zz + yz * yz)) | (det < -eps * mag)
    if bad.any():
        raise ValueError("the rotational inertia must be positive semidefinite")
    return out


# groups of an observation record in tangent order: argument stem, first coordinate, width (solver.PLANT_OBSERVATION_GROUPS)
_OBSERVATION_GROUPS = (("position", 0, 3), ("orientation", 3, 3), ("joints", 6, 19), ("linear_velocity", 25, 3), ("angular_velocity", 28, 3), ("joint_velocities", 31, 19))


def stack_plant_observation(B, **groups):
    """Observation models [B, 100] for BatchedILQR.plant_set_observation / MPCRunner(plant_observation=...): bias[50] then sigma[50] in the
    tangent order of the Jacobians.  Keywords, each `<group>_bias` or `<group>_noise` with group one of position (m, world), orientation
    (rotation vector, body frame, rad), joints (rad), linear_velocity (m/s, world), angular_velocity (rad/s, body), joint_velocities
    (rad/s); a value is a scalar, a vector of the group's width (3 or 19), [B] (one scalar per rollout) or [B, width]; what is not given is
    zero.  Raises ValueError for an unknown keyword, a shape that is none of these, a non-finite entry or a negative noise level -- what
    ilqr_hip_plant_set_observation refuses."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be positive")
    out = np.zeros((B, 100))
    known = {g + suffix: (first + half, width) for g, first, width in _OBSERVATION_GROUPS for suffix, half in (("_bias", 0), ("_noise", 50))}
    for name, val in groups.items():
        if name not in known:
            raise ValueError("unknown observation group %r (known: %s)" % (name, ", ".join(sorted(known))))
        first, width = known[name]
        v = np.asarray(val, dtype=np.float64)
        if v.shape == (B,) and B != width:      # (B == width: a vector is read per coordinate; [B, 1] says per rollout)
            v = v[:, None]
        if v.shape not in ((), (width,), (1, width), (B, 1), (B, width)):
            raise ValueError("%s must be a scalar, [%d], [B] or [B, %d]" % (name, width, width))
        out[:, first:first + width] = v
    if not np.isfinite(out).all():
        raise ValueError("plant observation records must be finite")
    if (out[:, 50:] < 0).any():
        raise ValueError("noise levels >= 0 are required")
    return out


def stack_plant_actuator(B, delay=0, tau=0.0, sigma=0.0):
    """Actuator models [B, 39] for BatchedILQR.plant_set_actuator / MPCRunner(plant_actuator=...): delay, tau[19], sigma[19].  delay (plant
    substeps, an integer 0..8) is a scalar or [B]; tau (s, the time constant of a first-order lag, 0: none) and sigma (N m, torque noise) are
    each a scalar, a vector per joint [19], [B] (one scalar per rollout) or [B, 19].  Raises ValueError for a shape that is none of these, a
    non-finite entry, a negative tau or sigma or a delay that is not an integer in 0..8 -- what ilqr_hip_plant_set_actuator refuses."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be positive")
    out = np.zeros((B, 39))
    d = np.asarray(delay, dtype=np.float64)
    if d.shape not in ((), (1,), (B,)):
        raise ValueError("delay must be a scalar or [B]")
    out[:, 0] = d
    for name, val, first in (("tau", tau, 1), ("sigma", sigma, 20)):
        v = np.asarray(val, dtype=np.float64)
        if v.shape == (B,) and B != 19:      # (B == 19: a vector is read per joint; [B, 1] says per rollout)
            v = v[:, None]
        if v.shape not in ((), (19,), (1, 19), (B, 1), (B, 19)):
            raise ValueError("%s must be a scalar, [19], [B] or [B, 19]" % name)
        out[:, first:first + 19] = v
    if not np.isfinite(out).all():
        raise ValueError("plant actuator records must be finite")
    if (out[:, 1:] < 0).any():
        raise ValueError("tau >= 0 and sigma >= 0 are required")
    if (out[:, 0] < 0).any() or (out[:, 0] > 8).any() or (out[:, 0] != np.floor(out[:, 0])).any():
        raise ValueError("delay must be an integer in 0..8 (plant substeps)")
    return out


# fields of a joint record in record order with their nominal values (solver.PLANT_JOINT_FIELDS)
_JOINT_FIELDS = (("gain", 1.0), ("range_scale", 1.0), ("damping", 1.0), ("armature", 0.1))


def stack_plant_joints(records, B):
    """Joint records [B, 76] for BatchedILQR.plant_set_joints / MPCRunner(plant_joints=...): gain[19], range_scale[19], damping[19],
    armature[19] in the order of u.  records is one dict (every rollout) or a sequence of B dicts; a dict holds any of "gain", "range_scale",
    "damping", "armature", each a scalar (every joint) or a vector per joint [19]; what it leaves out is nominal (1, 1, 1, 0.1), so {} is the
    model's joints.  Raises ValueError for another key, a shape that is neither, a sequence that is not B long, a non-finite or a negative
    entry -- what ilqr_hip_plant_set_joints refuses."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be positive")
    if isinstance(records, dict):
        records = [records] * B
    records = list(records)
    if len(records) != B:
        raise ValueError("records must be one dict or B of them")
    out = np.empty((B, 76))
    names = [f for f, _ in _JOINT_FIELDS]
    for b, rec in enumerate(records):
        if not isinstance(rec, dict):
            raise ValueError("a joint record is a dict")
        extra = set(rec) - set(names)
        if extra:
            raise ValueError("unknown joint field(s) %s: a record has %s" % (sorted(extra), names))
        for k, (name, nominal) in enumerate(_JOINT_FIELDS):
            v = np.asarray(rec.get(name, nominal), dtype=np.float64)
            if v.shape not in ((), (19,)):
                raise ValueError("%s must be a scalar or [19]" % name)
            out[b, 19 * k:19 * (k + 1)] = v
    if not np.isfinite(out).all():
        raise ValueError("plant joint records must be finite")
    if (out < 0).any():
        raise ValueError("gain, range_scale, damping and armature must be >= 0")
    return out


_AL_BOUND_FIELDS = ("joint_lo", "joint_hi", "ctrl_lo", "ctrl_hi")


def _check_al_bounds(out):
    """what ilqr_hip_set_al_bounds refuses"""
    lo, hi = out.reshape(-1, 2, 2, 19)[:, :, 0], out.reshape(-1, 2, 2, 19)[:, :, 1]
    if np.isnan(out).any() or (lo > hi).any() or (lo == np.inf).any() or (hi == -np.inf).any():
        raise ValueError("bounds: no NaN, lo <= hi, lo < +inf, hi > -inf")
    return out


def stack_al_bounds(records, B, margin=0.0):
    """Bounds table [n, 76] for BatchedILQR.set_al_bounds: joint_lo[19], joint_hi[19] (hinges in the order of the state slots 7..25),
    ctrl_lo[19], ctrl_hi[19] (order of u).  records is one dict (n = 1: every rollout reads it) or a sequence of B dicts (n = B).  Every key
    is optional: "joint_lo", "joint_hi", "ctrl_lo", "ctrl_hi", each a [19] array or a dict {index: value} that overrides single
    coordinates, and "torque_scale", a scalar or [19], which scales both ends of the model's control bound at `margin` as the `scale` of
    plant_joints scales the plant's clamp (0: a dead motor, lo = hi = 0); "ctrl_lo" / "ctrl_hi" are applied after it.  A key left out gives
    the default bound at `margin` (solver.al_default_bounds).  -inf / +inf switch a side off.  Raises ValueError for another key, a wrong
    shape or index, a sequence that is not B long, or a record ilqr_hip_set_al_bounds refuses (a NaN, lo > hi, lo = +inf, hi = -inf)."""
    from . import solver
    B = int(B)
    if B < 1:
        raise ValueError("B must be positive")
    if isinstance(records, dict):
        records = [records]
    else:
        records = list(records)
        if len(records) != B:
            raise ValueError("records must be one dict or B of them")
    default = solver.al_default_bounds(margin)
    out = np.tile(default, (len(records), 1))
    for b, rec in enumerate(records):
        if not isinstance(rec, dict):
            raise ValueError("a bounds record is a dict")
        extra = set(rec) - set(_AL_BOUND_FIELDS) - {"torque_scale"}
        if extra:
            raise ValueError("unknown bounds field(s) %s: a record has %s and torque_scale" % (sorted(extra), list(_AL_BOUND_FIELDS)))
        if "torque_scale" in rec:
            sc_ = np.asarray(rec["torque_scale"], dtype=np.float64)
            if sc_.shape not in ((), (19,)) or not np.isfinite(sc_).all() or (sc_ < 0).any():
                raise ValueError("torque_scale must be a finite scalar or [19], >= 0")
            out[b, 38:57] = sc_ * default[38:57]; out[b, 57:76] = sc_ * default[57:76]
        for k, name in enumerate(_AL_BOUND_FIELDS):
            v = rec.get(name)
            if v is None:
                continue
            if isinstance(v, dict):
                for i, val in v.items():
                    if not (isinstance(i, (int, np.integer)) and 0 <= i < 19):
                        raise ValueError("%s: index %r is not in 0..18" % (name, i))
                    out[b, 19 * k + int(i)] = float(val)
            else:
                v = np.asarray(v, dtype=np.float64)
                if v.shape != (19,):
                    raise ValueError("%s must be [19] or {index: value}" % name)
                out[b, 19 * k:19 * (k + 1)] = v
    return _check_al_bounds(out)


# keys of a state-bounds record: name -> (first box coordinate, length); box coordinates in the order of ilqr_hip_set_al_state_bounds
_AL_STATE_FIELDS = {"pelvis_pos": (0, 3), "pelvis_lin_vel": (3, 3), "pelvis_ang_vel": (6, 3), "joint_vel": (9, 19)}


def stack_al_state_bounds(records, B):
    """State-bounds table [n, 56] for BatchedILQR.set_al_state_bounds: lo[28], hi[28] over the box coordinates pelvis position (3, world),
    pelvis linear velocity (3, world), pelvis angular velocity (3, body), joint velocities (19, order of u).  records is one dict (n = 1:
    every rollout reads it) or a sequence of B dicts (n = B).  Every key is optional and takes a pair (lo, hi), each a scalar or a vector of
    the key's length: "pelvis_pos", "pelvis_lin_vel", "pelvis_ang_vel", "joint_vel"; and the shorthands "pelvis_z": (lo, hi) of the
    pelvis height alone, and "joint_speed": v, a scalar or [19], for the symmetric joint_vel bound (-v, +v).  A shorthand is applied after
    the key it refines.  A key left out gives -inf / +inf: no bound.  Raises ValueError for another key, a wrong shape, a sequence that is
    not B long, or a record ilqr_hip_set_al_state_bounds refuses (a NaN, lo > hi, lo = +inf, hi = -inf)."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be positive")
    if isinstance(records, dict):
        records = [records]
    else:
        records = list(records)
        if len(records) != B:
            raise ValueError("records must be one dict or B of them")
    out = np.empty((len(records), 56))
    out[:, :28] = -np.inf; out[:, 28:] = np.inf

    def pair(name, v, n):
        try:
            lo, hi = v
        except (TypeError, ValueError):
            raise ValueError("%s takes a pair (lo, hi)" % name)
        lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        if lo.shape not in ((), (n,)) or hi.shape not in ((), (n,)):
            raise ValueError("%s: lo and hi are scalars or [%d]" % (name, n))
        return lo, hi

    for b, rec in enumerate(records):
        if not isinstance(rec, dict):
            raise ValueError("a state-bounds record is a dict")
        extra = set(rec) - set(_AL_STATE_FIELDS) - {"pelvis_z", "joint_speed"}
        if extra:
            raise ValueError("unknown state-bounds field(s) %s: a record has %s, pelvis_z and joint_speed" % (sorted(extra), list(_AL_STATE_FIELDS)))
        for name, (k0, n) in _AL_STATE_FIELDS.items():
            if rec.get(name) is not None:
                out[b, k0:k0 + n], out[b, 28 + k0:28 + k0 + n] = pair(name, rec[name], n)
        if rec.get("pelvis_z") is not None:
            out[b, 2], out[b, 28 + 2] = (float(v.reshape(-1)[0]) for v in pair("pelvis_z", rec["pelvis_z"], 1))
        if rec.get("joint_speed") is not None:
            v = np.asarray(rec["joint_speed"], dtype=np.float64)
            if v.shape not in ((), (19,)) or np.isnan(v).any() or (v < 0).any():
                raise ValueError("joint_speed must be a scalar or [19], >= 0")
            out[b, 9:28], out[b, 28 + 9:56] = -v, v
    lo, hi = out[:, :28], out[:, 28:]
    if np.isnan(out).any() or (lo > hi).any() or (lo == np.inf).any() or (hi == -np.inf).any():
        raise ValueError("state bounds: no NaN, lo <= hi, lo < +inf, hi > -inf")
    return out


def _is_knot_triple(v):
    return (isinstance(v, (tuple, list)) and len(v) == 3 and all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in v[:2]))


def _knot_records(records, B, N):
    """records of the knot stackers -> per record the N + 1 plain dicts of its knots: a value that is a triple (first_knot, end_knot, value)
    or a list of triples holds at the knots first_knot <= t < end_knot (a later triple overrides an earlier one) and is left out elsewhere"""
    B, N = int(B), int(N)
    if B < 1 or N < 1:
        raise ValueError("B and N must be positive")
    if isinstance(records, dict):
        records = [records]
    else:
        records = list(records)
        if len(records) != B:
            raise ValueError("records must be one dict or B of them")
    out = []
    for rec in records:
        if not isinstance(rec, dict):
            raise ValueError("a bounds record is a dict")
        knots = [dict() for _ in range(N + 1)]
        for key, v in rec.items():
            if _is_knot_triple(v):
                v = [v]
            if isinstance(v, list) and len(v) > 0 and all(_is_knot_triple(e) for e in v):
                for first, end, val in v:
                    if not 0 <= first <= end <= N + 1:
                        raise ValueError("%s: knots (%r, %r) are not 0 <= first_knot <= end_knot <= N + 1" % (key, first, end))
                    for t in range(int(first), int(end)):
                        knots[t][key] = val
            else:
                for k in knots:
                    k[key] = v
        out.append(knots)
    return out


def stack_al_knot_bounds(records, B, N, margin=0.0):
    """Bounds windows [n, N+1, 76] for BatchedILQR.set_al_knot_bounds (and, with N + 1 = rows, tracks for set_al_bounds_track): row t holds
    knot t's joint_lo[19], joint_hi[19], ctrl_lo[19], ctrl_hi[19].  records is one dict (n = 1) or a sequence of B dicts (n = B) with the
    keys and values of stack_al_bounds; every value may also be a triple (first_knot, end_knot, value) -- the value holds at the knots
    first_knot <= t < end_knot -- or a list of such triples.  Knots outside every triple get the default: the model's bound at `margin`.
    Raises ValueError where stack_al_bounds does, and for knots outside 0 <= first_knot <= end_knot <= N + 1."""
    per = _knot_records(records, B, N)
    return np.stack([np.concatenate([stack_al_bounds(k, 1, margin) for k in knots]) for knots in per])


def stack_al_state_knot_bounds(records, B, N):
    """State-bounds windows [n, N+1, 56] for BatchedILQR.set_al_state_knot_bounds: row t holds knot t's lo[28], hi[28].  records as for
    stack_al_state_bounds; every value may also be a triple (first_knot, end_knot, value) or a list of such triples, as in
    stack_al_knot_bounds.  Knots outside every triple get -inf / +inf: no bound."""
    per = _knot_records(records, B, N)
    return np.stack([np.concatenate([stack_al_state_bounds(k, 1) for k in knots]) for knots in per])


# keys of a task-bounds record: name -> first task coordinate (three each), in the order of ilqr_hip_set_al_task_bounds
_AL_TASK_FIELDS = {"com": 0, "left_foot": 3, "right_foot": 6}


def stack_al_task_bounds(records, B, N):
    """Task-bounds windows [n, N+1, 18] for BatchedILQR.set_al_task_bounds (and, with N + 1 = rows and one record, out[0] is a track for
    set_al_task_bounds_track): row t holds knot t's lo[9], hi[9] over the task coordinates CoM
    x, y, z, left ankle origin x, y, z, right ankle origin x, y, z (world frame).  records is one dict (n = 1: every rollout reads the
    window) or a sequence of B dicts (n = B).  Every key is optional: "com", "left_foot", "right_foot" take a pair (lo, hi), each a scalar,
    [3] (the whole horizon) or [N+1, 3] (one row per knot); the shorthands "swing_clearance": z_min sets z >= z_min on both feet (the
    solver ignores a foot's rows at its stance knots, so this bounds the swing phases) and "com_xy": ((x0, y0), (x1, y1)) the box
    x0 <= x <= x1, y0 <= y <= y1 of the CoM.  A shorthand is applied after the key it refines.  A key left out gives -inf / +inf: no bound.
    Raises ValueError for another key, a wrong shape, a sequence that is not B long, or a window ilqr_hip_set_al_task_bounds refuses (a NaN,
    lo > hi, lo = +inf, hi = -inf)."""
    B, N = int(B), int(N)
    if B < 1 or N < 1:
        raise ValueError("B and N must be positive")
    if isinstance(records, dict):
        records = [records]
    else:
        records = list(records)
        if len(records) != B:
            raise ValueError("records must be one dict or B of them")
    out = np.empty((len(records), N + 1, 18))
    out[:, :, :9] = -np.inf; out[:, :, 9:] = np.inf

    def rows(name, v):
        v = np.asarray(v, dtype=np.float64)
        if v.shape not in ((), (3,), (N + 1, 3)):
            raise ValueError("%s: lo and hi are scalars, [3] or [N+1, 3]" % name)
        return np.broadcast_to(v, (N + 1, 3))

    for b, rec in enumerate(records):
        if not isinstance(rec, dict):
            raise ValueError("a task-bounds record is a dict")
        extra = set(rec) - set(_AL_TASK_FIELDS) - {"swing_clearance", "com_xy"}
        if extra:
            raise ValueError("unknown task-bounds field(s) %s: a record has %s, swing_clearance and com_xy" % (sorted(extra), list(_AL_TASK_FIELDS)))
        for name, k0 in _AL_TASK_FIELDS.items():
            if rec.get(name) is not None:
                try:
                    lo, hi = rec[name]
                except (TypeError, ValueError):
                    raise ValueError("%s takes a pair (lo, hi)" % name)
                out[b, :, k0:k0 + 3], out[b, :, 9 + k0:9 + k0 + 3] = rows(name, lo), rows(name, hi)
        if rec.get("swing_clearance") is not None:
            z = np.asarray(rec["swing_clearance"], dtype=np.float64)
            if z.shape != ():
                raise ValueError("swing_clearance is one height")
            out[b, :, 5] = out[b, :, 8] = float(z)
        if rec.get("com_xy") is not None:
            c = np.asarray(rec["com_xy"], dtype=np.float64)
            if c.shape != (2, 2):
                raise ValueError("com_xy is ((x0, y0), (x1, y1))")
            out[b, :, 0:2], out[b, :, 9:11] = c[0], c[1]
    lo, hi = out[..., :9], out[..., 9:]
    if np.isnan(out).any() or (lo > hi).any() or (lo == np.inf).any() or (hi == -np.inf).any():
        raise ValueError("task bounds: no NaN, lo <= hi, lo < +inf, hi > -inf")
    return out


def swing_phases(flags):
    """The swing phases of one foot of a contact schedule: flags [rows] (1 stance, 0 swing) -> [(first, end)], the maximal runs of rows with
    flag 0 as half-open ranges, in order; a run reaching the last row counts."""
    flags = np.asarray(flags)
    phases, first = [], None
    for r, f in enumerate(flags):
        if f == 0 and first is None:
            first = r
        if f != 0 and first is not None:
            phases.append((first, r)); first = None
    if first is not None:
        phases.append((first, len(flags)))
    return phases


def al_task_track_from_footsteps(stance, footsteps, half_size, land_rows=2, clearance=None, clearance_margin_rows=2):
    """A task bounds track [rows, 18] (BatchedILQR.set_al_task_bounds_track) from a footstep plan.  stance [rows, 2] is the contact schedule
    on the loop's timeline (1 stance, 0 swing; column 0 the left foot); footsteps = {"left": [(x, y), ...], "right": [...]} has one landing
    centre per swing phase of that foot, in order (a swing phase: a maximal run of rows with flag 0, swing_phases; a run reaching the last
    row counts).  On the last `land_rows` rows of each phase the foot's x and y are bounded to centre +- half_size ("land inside this
    stone"); with `clearance`, z >= clearance holds on the rows of a phase at least `clearance_margin_rows` from both of its ends (row r of
    a phase [first, end): first + margin <= r < end - margin).  Everything else is -inf / +inf.  Raises ValueError when a foot's footstep
    count differs from its phase count or a shape is wrong."""
    stance = np.asarray(stance)
    if stance.ndim != 2 or stance.shape[1] != 2 or stance.shape[0] < 1:
        raise ValueError("stance is the contact schedule [rows, 2]")
    if not isinstance(footsteps, dict) or set(footsteps) != {"left", "right"}:
        raise ValueError('footsteps is {"left": [(x, y), ...], "right": [(x, y), ...]}')
    half = np.asarray(half_size, dtype=np.float64)
    if half.shape not in ((), (2,)) or not (half >= 0.0).all():
        raise ValueError("half_size is one non-negative length or (half_x, half_y)")
    half = np.broadcast_to(half, (2,))
    land_rows, margin = int(land_rows), int(clearance_margin_rows)
    if land_rows < 0 or margin < 0:
        raise ValueError("land_rows and clearance_margin_rows are non-negative")
    if clearance is not None and np.asarray(clearance, dtype=np.float64).shape != ():
        raise ValueError("clearance is one height")
    rows = stance.shape[0]
    out = np.empty((rows, 18))
    out[:, :9] = -np.inf; out[:, 9:] = np.inf
    for e, name in enumerate(("left", "right")):
        k0 = _AL_TASK_FIELDS[name + "_foot"]
        try:
            steps = np.asarray(footsteps[name], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("footsteps[%r] is a list of (x, y)" % name)
        if steps.size == 0:
            steps = np.zeros((0, 2))
        if steps.ndim != 2 or steps.shape[1] != 2:
            raise ValueError("footsteps[%r] is a list of (x, y)" % name)
        phases = swing_phases(stance[:, e])
        if len(phases) != len(steps):
            raise ValueError("%s foot: %d footsteps for %d swing phases" % (name, len(steps), len(phases)))
        for (first, end), centre in zip(phases, steps):
            land = slice(max(first, end - land_rows), end)
            out[land, k0:k0 + 2], out[land, 9 + k0:9 + k0 + 2] = centre - half, centre + half
            if clearance is not None and first + margin < end - margin:
                out[first + margin:end - margin, k0 + 2] = float(clearance)
    lo, hi = out[:, :9], out[:, 9:]
    if np.isnan(out).any() or (lo > hi).any() or (lo == np.inf).any() or (hi == -np.inf).any():
        raise ValueError("task bounds: no NaN, lo <= hi, lo < +inf, hi > -inf")
    return out


def al_bounds_from_plant_joints(joints, margin=0.0):
    """The bounds table [n, 76] in which the solver knows each rollout's torque range of stack_plant_joints' records `joints` [n, 76]:
    ctrl_lo, ctrl_hi = range_scale_i * the default control bound of actuator i at `margin` (range_scale = 0, a dead motor: lo = hi = 0);
    the joint bounds are the default.  The per-joint `gain` of the records is NOT folded in: the plant multiplies the commanded torque by it
    ahead of its clamp, so the command that saturates is hi / gain, which this table does not express; neither are damping and armature."""
    from . import solver
    j = np.asarray(joints, dtype=np.float64)
    if j.ndim == 1:
        j = j[None]
    if j.ndim != 2 or j.shape[1] != 76:
        raise ValueError("joints must be [n, 76] (stack_plant_joints)")
    scale = j[:, 19:38]
    if not np.isfinite(scale).all() or (scale < 0).any():
        raise ValueError("range_scale must be finite and >= 0")
    default = solver.al_default_bounds(margin)
    out = np.tile(default, (j.shape[0], 1))
    out[:, 38:57] = scale * default[38:57]; out[:, 57:76] = scale * default[57:76]
    return _check_al_bounds(out)


# fields of a terrain record in record order with their flat defaults (solver.PLANT_TERRAIN): the solver's ground, everywhere, always
_TERRAIN_FIELDS = (("z_left", 0.0), ("z_right", 0.0), ("edge_x", -np.inf), ("first", 0.0), ("end", np.inf))


def stack_plant_terrain(records, B):
    """Floors [B, 5] for BatchedILQR.plant_set_terrain / MPCRunner(plant_terrain=...): z_left, z_right (floor height under the left / right
    foot, m), edge_x (the height holds for a foot whose ankle is at world x >= edge_x, m; -inf: everywhere), first and end of the window of
    plant intervals the record acts in (first <= i < end, counted from plant_reset).  records is one dict (every rollout) or a sequence of B
    dicts; a dict holds any of these five scalars, what it leaves out is flat (0, 0, -inf, 0, inf), so {} is the solver's ground.  Raises
    ValueError for another key, a value that is no scalar, a sequence that is not B long, a non-finite height, an edge that is neither finite
    nor -inf, a negative or non-integral first / end (end may be inf) or end < first -- what ilqr_hip_plant_set_terrain refuses."""
    B = int(B)
    if B < 1:
        raise ValueError("B must be positive")
    if isinstance(records, dict):
        records = [records] * B
    records = list(records)
    if len(records) != B:
        raise ValueError("records must be one dict or B of them")
    out = np.empty((B, 5))
    names = [f for f, _ in _TERRAIN_FIELDS]
    for b, rec in enumerate(records):
        if not isinstance(rec, dict):
            raise ValueError("a terrain record is a dict")
        extra = set(rec) - set(names)
        if extra:
            raise ValueError("unknown terrain field(s) %s: a record has %s" % (sorted(extra), names))
        for k, (name, flat) in enumerate(_TERRAIN_FIELDS):
            v = np.asarray(rec.get(name, flat), dtype=np.float64)
            if v.shape != ():
                raise ValueError("%s must be a scalar" % name)
            out[b, k] = v
    if not np.isfinite(out[:, :2]).all():
        raise ValueError("floor heights must be finite")
    if np.isnan(out[:, 2]).any() or (out[:, 2] == np.inf).any():
        raise ValueError("edge_x must be finite or -inf")
    if not np.isfinite(out[:, 3]).all() or np.isnan(out[:, 4]).any() or (out[:, 4] == -np.inf).any():
        raise ValueError("first must be finite, end finite or inf")
    fin_end = np.where(np.isfinite(out[:, 4]), out[:, 4], 0.0)
    if (out[:, 3] < 0).any() or (out[:, 4] < 0).any() or (out[:, 3] != np.floor(out[:, 3])).any() or (fin_end != np.floor(fin_end)).any():
        raise ValueError("first and end must be non-negative integers")
    if (out[:, 4] < out[:, 3]).any():
        raise ValueError("end >= first is required")
    return out


def repeat_for_groups(table, G):
    """A per-problem table or stacked window [M, ...] repeated for solve groups of G members, member-minor: [M G, ...] whose rows m G .. m G + G - 1
    are row m (BatchedILQR.set_groups: the members of a group share x0, references, schedule and plant tables)."""
    G = int(G)
    if G < 1:
        raise ValueError("G must be >= 1")
    table = np.asarray(table)
    if table.ndim < 1:
        raise ValueError("a table has a leading axis of problems")
    return np.ascontiguousarray(np.repeat(table, G, axis=0))


def stack_group_sigma(G, base, ladder=None):
    """The perturbation table [G, 19] of BatchedILQR.group_set_perturbation: row 0 zeros (the incumbent), row g = base * ladder[g - 1].
    base: a scalar or [19] standard deviations per actuator (Nm); ladder [G - 1] factors, by default geometric, 2 ** (g - 1): each member
    searches twice as far from the incumbent as the one before it."""
    G = int(G)
    if G < 1:
        raise ValueError("G must be >= 1")
    base = np.broadcast_to(np.asarray(base, dtype=np.float64), (19,))
    ladder = 2.0 ** np.arange(G - 1) if ladder is None else np.asarray(ladder, dtype=np.float64)
    if ladder.shape != (G - 1,):
        raise ValueError("ladder must have G - 1 entries")
    out = np.zeros((G, 19))
    out[1:] = ladder[:, None] * base[None, :]
    if not np.all(np.isfinite(out)) or np.any(out < 0.0):
        raise ValueError("sigmas must be finite and >= 0")
    return out


def _axis_angle_quat(w):
    ang = np.linalg.norm(w, axis=-1, keepdims=True)
    half = 0.5 * ang
    s = np.where(ang > 1e-12, np.sin(half) / np.maximum(ang, 1e-300), 0.5)
    return np.concatenate([np.cos(half), s * w], axis=-1)


def synthetic_batch(B, N, seed, u_gravcomp):
    """Seeded standing-balance batch: x0 = x_stand + delta, u_init = u_gravcomp + U(-1,1)
    clipped to 80 % of ctrlrange. Returns x0 [B,51], u_init [B,N,19]."""
    rng = np.random.default_rng(seed)
    x0 = np.tile(standing_state(), (B, 1))
    x0[:, 0:3] += rng.uniform(-0.02, 0.02, size=(B, 3))
    x0[:, 3:7] = _axis_angle_quat(rng.uniform(-0.05, 0.05, size=(B, 3)))
    x0[:, 7:NQ] += rng.uniform(-0.05, 0.05, size=(B, NQ - 7))
    x0[:, NQ:] += rng.uniform(-0.1, 0.1, size=(B, NV))
    u = np.asarray(u_gravcomp, dtype=np.float64)[None, None, :] + rng.uniform(-1.0, 1.0, size=(B, N, NU))
    u = np.clip(u, -0.8 * CTRLRANGE, 0.8 * CTRLRANGE)
    return x0, u


def walking_batch(B, N, seed, refdata_npz, sv, rf):
    """BASELINE.json configs[4]: B receding-horizon windows of the H1 walking reference (data/h1_walking_pin.csv rows, shipped as
    the fixture tests/golden/refdata_golden.npz), each with its own references and contact schedule: offline preparation as
    references.prepare_reference does it (Pinocchio -> MuJoCo quaternion order, velocities, stance flags from the foot hull),
    window start t0 drawn per rollout, initial state = the reference row perturbed, gravity-compensation controls + noise.
    `sv` = the solver module (host kinematics), `rf` = the references module.  Returns (problem with per-rollout sets, x0, u_init, t0)."""
    r = np.load(refdata_npz)
    q_mj = rf.pinocchio_to_mujoco(r["walking_pin_rows"])
    v = rf.differentiate_positions(q_mj, float(r["dt"]))
    flags = rf.contact_schedule(q_mj, sv.foot_clearance)
    rd = rf.ReferenceData(sv.reference_kinematics, sv.reference_com_velocity)
    rd.set_states(np.concatenate([q_mj, v], axis=1)); rd.contact = flags
    T = q_mj.shape[0]
    base = make_problem(sv.reference_kinematics, N=N, gravity=(0.0, 0.0, -1.0))
    rng = np.random.default_rng(seed)
    t0 = rng.integers(0, T - N - 1, size=B)
    probs = {}
    keys = ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref")
    stacks = {k: [] for k in keys}
    for b in range(B):
        if int(t0[b]) not in probs:
            probs[int(t0[b])] = rd.problem_at(int(t0[b]), N, base, follow_schedule=True)
        for k in keys:
            stacks[k].append(probs[int(t0[b])][k][0])
    prob = dict(base); prob["N"] = N
    for k in keys:
        prob[k] = np.stack(stacks[k])
    x0 = rd.x_ref[t0].copy()
    x0[:, 7:26] += rng.uniform(-0.02, 0.02, (B, 19)); x0[:, 0:3] += rng.uniform(-0.01, 0.01, (B, 3)); x0[:, 26:] *= 0.5
    ug = sv.gravity_compensation(standing_state(), prob["gravity"])
    ui = np.tile(ug, (B, N, 1)) + rng.uniform(-0.5, 0.5, (B, N, 19))
    return prob, x0, ui, t0
