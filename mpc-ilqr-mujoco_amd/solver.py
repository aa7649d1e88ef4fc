"""Host-side Python mirror of the reference's solver interface over the C-ABI HIP library.

`BatchedILQR` mirrors `iLQR` (reference include/ilqr/ilqr.hpp:17-45) for a batch of B independent
rollouts; `BatchedMPC` mirrors `MPC::stepOnce` (reference include/ilqr/mpc.hpp:18-47,
src/ilqr/mpc.cpp:40-127).  All compute happens in libilqr_hip.so (hand-written HIP kernels for
gfx950); there is no CPU fallback -- constructing a solver without the library or without a GPU
raises.
"""
import ctypes as C
import os

import numpy as np

NX, NU, NQ, NV = 51, 19, 26, 25
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ILQR_HIP_LIB", os.path.join(_HERE, "lib", "libilqr_hip.so"))
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

STATUS = {0: "ILQR_OK", 1: "ILQR_ERR_ARG", 2: "ILQR_ERR_HIP", 3: "ILQR_ERR_NO_DEVICE", 4: "ILQR_ERR_STATE", 5: "ILQR_ERR_UNSUPPORTED"}
JAC_ANALYTIC, JAC_FD_FORWARD = 0, 1

# every symbol include/ilqr_hip.h declares (checked by the CPU test-suite against the built library)
EXPORTS = [
    "ilqr_hip_create", "ilqr_hip_destroy", "ilqr_hip_last_error", "ilqr_hip_batch", "ilqr_hip_horizon", "ilqr_hip_num_slices", "ilqr_hip_reload_environment", "ilqr_hip_set_dedup_saturated_retry",
    "ilqr_hip_set_cost_weights", "ilqr_hip_set_task_weights", "ilqr_hip_set_constraint_weights", "ilqr_hip_set_gravity",
    "ilqr_hip_set_weight_sets", "ilqr_hip_clear_weight_sets", "ilqr_hip_num_weight_sets",
    "ilqr_hip_set_augmented_lagrangian", "ilqr_hip_clear_augmented_lagrangian", "ilqr_hip_augmented_lagrangian_rounds",
    "ilqr_hip_get_al_multipliers", "ilqr_hip_set_al_multipliers", "ilqr_hip_get_al_penalties", "ilqr_hip_get_al_violation", "ilqr_hip_get_al_trace",
    "ilqr_hip_al_update",
    "ilqr_hip_set_al_bounds", "ilqr_hip_clear_al_bounds", "ilqr_hip_num_al_bound_sets", "ilqr_hip_get_al_bounds", "ilqr_hip_al_default_bounds",
    "ilqr_hip_set_al_state_bounds", "ilqr_hip_clear_al_state_bounds", "ilqr_hip_num_al_state_bound_sets", "ilqr_hip_get_al_state_bounds",
    "ilqr_hip_get_al_state_multipliers", "ilqr_hip_set_al_state_multipliers", "ilqr_hip_get_al_state_penalties", "ilqr_hip_get_al_state_violation",
    "ilqr_hip_get_al_state_trace", "ilqr_hip_al_state_slot",
    "ilqr_hip_set_al_knot_bounds", "ilqr_hip_set_al_state_knot_bounds", "ilqr_hip_get_al_knot_bounds", "ilqr_hip_al_bounds_per_knot",
    "ilqr_hip_set_al_bounds_track", "ilqr_hip_clear_al_bounds_track", "ilqr_hip_al_bounds_track_rows", "ilqr_hip_set_al_bounds_track_starts",
    "ilqr_hip_al_bounds_window_from_track",
    "ilqr_hip_set_al_task_bounds", "ilqr_hip_clear_al_task_bounds", "ilqr_hip_num_al_task_bound_sets", "ilqr_hip_get_al_task_bounds",
    "ilqr_hip_get_al_task_multipliers", "ilqr_hip_set_al_task_multipliers", "ilqr_hip_get_al_task_penalties", "ilqr_hip_get_al_task_violation",
    "ilqr_hip_get_al_task_trace", "ilqr_hip_get_al_task_points", "ilqr_hip_get_al_task_velocities",
    "ilqr_hip_set_al_task_bounds_track", "ilqr_hip_clear_al_task_bounds_track", "ilqr_hip_al_task_bounds_track_rows",
    "ilqr_hip_set_contact_schedule", "ilqr_hip_set_ee_references", "ilqr_hip_set_references",
    "ilqr_hip_set_regularization", "ilqr_hip_set_max_iterations", "ilqr_hip_set_tolerance", "ilqr_hip_set_options", "ilqr_hip_set_early_exit_gate",
    "ilqr_hip_initialize", "ilqr_hip_initialize_warm_resident", "ilqr_hip_initialize_device",
    "ilqr_hip_solve", "ilqr_hip_solve_async", "ilqr_hip_synchronize",
    "ilqr_hip_get_xbar", "ilqr_hip_get_ubar", "ilqr_hip_get_gains_K", "ilqr_hip_get_gains_kff", "ilqr_hip_get_cost",
    "ilqr_hip_get_iterations", "ilqr_hip_get_lambda", "ilqr_hip_get_trace", "ilqr_hip_first_knot_device", "ilqr_hip_pack_first_knot_device",
    "ilqr_hip_compute_control",
    "ilqr_hip_set_trajectory", "ilqr_hip_stage_rollout", "ilqr_hip_stage_linearize", "ilqr_hip_stage_cost_quadratics",
    "ilqr_hip_stage_backward_pass", "ilqr_hip_stage_line_search", "ilqr_hip_stage_total_cost",
    "ilqr_hip_get_linearization", "ilqr_hip_set_linearization", "ilqr_hip_get_quadratics", "ilqr_hip_set_quadratics",
    "ilqr_hip_get_value_function", "ilqr_hip_step", "ilqr_hip_step_stance", "ilqr_hip_set_stance_source", "ilqr_hip_step_geometry", "ilqr_hip_get_stance", "ilqr_hip_set_contact_mode", "ilqr_hip_set_friction", "ilqr_hip_set_joint_limits", "ilqr_hip_set_joint_limit_stiffness", "ilqr_hip_enable_profiling", "ilqr_hip_get_stage_ms", "ilqr_hip_get_adopt_mismatches", "ilqr_hip_get_iterations_enqueued", "ilqr_hip_get_speculative_iterations", "ilqr_hip_get_split_iterations", "ilqr_hip_set_profiled_stages",
    "ilqr_hip_payload_width", "ilqr_hip_comm_available", "ilqr_hip_comm_get_unique_id", "ilqr_hip_comm_init", "ilqr_hip_comm_destroy", "ilqr_hip_comm_world", "ilqr_hip_comm_rank",
    "ilqr_hip_gather_first_knot",
    "ilqr_hip_reference_kinematics", "ilqr_hip_reference_com_velocity", "ilqr_hip_foot_clearance", "ilqr_hip_gravity_compensation", "ilqr_hip_stream",
    "ilqr_hip_plant_reset", "ilqr_hip_plant_configure", "ilqr_hip_plant_kick", "ilqr_hip_plant_advance", "ilqr_hip_initialize_warm_from_plant",
    "ilqr_hip_plant_set_history", "ilqr_hip_plant_get_history", "ilqr_hip_plant_get_state", "ilqr_hip_plant_get_control", "ilqr_hip_plant_get_stance",
    "ilqr_hip_plant_get_alive", "ilqr_hip_plant_state_device",
    "ilqr_hip_plant_follow", "ilqr_hip_initialize_warm_from_plant_shifted", "ilqr_hip_initialize_warm_resident_shifted", "ilqr_hip_compute_control_at",
    "ilqr_hip_set_relinearize_unchanged", "ilqr_hip_get_linearized_rollouts", "ilqr_hip_set_repeat_first_pass", "ilqr_hip_get_first_pass_rollouts",
    "ilqr_hip_get_retry_pass_rollouts", "ilqr_hip_set_reroll_nominal", "ilqr_hip_get_nominal_rollouts",
    "ilqr_hip_set_listed_spec", "ilqr_hip_get_listed_spec_iterations", "ilqr_hip_get_iteration_orders", "ilqr_hip_get_iteration_lists",
    "ilqr_hip_plant_set_score", "ilqr_hip_plant_clear_score", "ilqr_hip_plant_get_score", "ilqr_hip_plant_score_device",
    "ilqr_hip_plant_set_task_score", "ilqr_hip_plant_clear_task_score", "ilqr_hip_plant_get_task_score", "ilqr_hip_plant_task_score_device",
    "ilqr_hip_set_reference_track", "ilqr_hip_clear_reference_track", "ilqr_hip_reference_track_rows", "ilqr_hip_set_track_starts",
    "ilqr_hip_window_from_track", "ilqr_hip_get_reference_windows",
    "ilqr_hip_plant_set_model", "ilqr_hip_plant_set_params", "ilqr_hip_plant_clear_params", "ilqr_hip_plant_num_param_sets", "ilqr_hip_plant_get_params",
    "ilqr_hip_plant_set_wrench", "ilqr_hip_plant_clear_wrench", "ilqr_hip_plant_num_wrench_sets", "ilqr_hip_plant_get_wrench", "ilqr_hip_plant_intervals",
    "ilqr_hip_step_wrench", "ilqr_hip_pelvis_inertial_offset",
    "ilqr_hip_plant_set_payload", "ilqr_hip_plant_clear_payload", "ilqr_hip_plant_num_payload_sets", "ilqr_hip_plant_get_payload", "ilqr_hip_step_payload",
    "ilqr_hip_plant_set_observation", "ilqr_hip_plant_clear_observation", "ilqr_hip_plant_num_observation_sets", "ilqr_hip_plant_get_observation",
    "ilqr_hip_plant_observation_errors", "ilqr_hip_plant_get_observed",
    "ilqr_hip_plant_set_actuator", "ilqr_hip_plant_clear_actuator", "ilqr_hip_plant_num_actuator_sets", "ilqr_hip_plant_get_actuator",
    "ilqr_hip_plant_get_actuator_blend", "ilqr_hip_plant_actuator_draws", "ilqr_hip_plant_get_applied",
    "ilqr_hip_plant_set_joints", "ilqr_hip_plant_get_joints", "ilqr_hip_step_joints",
    "ilqr_hip_plant_set_terrain", "ilqr_hip_plant_clear_terrain", "ilqr_hip_plant_num_terrain_sets", "ilqr_hip_plant_get_terrain", "ilqr_hip_step_terrain",
    "ilqr_hip_terrain_stance",
    "ilqr_hip_set_groups", "ilqr_hip_num_groups", "ilqr_hip_group_set_perturbation", "ilqr_hip_group_clear_perturbation", "ilqr_hip_group_draws",
    "ilqr_hip_group_perturb", "ilqr_hip_group_select", "ilqr_hip_group_get_winners", "ilqr_hip_group_winners_device", "ilqr_hip_group_copy_winners_device", "ilqr_hip_group_adopt",
]
# slots of a group record (include/ilqr_hip.h ilqr_hip_group_select)
GROUP_RECORD = ("winner_key", "incumbent_key", "finite_keys", "largest_finite_key")
# the items of a problem dict that are reference windows (one set, or one per rollout)
REFERENCE_KEYS = ("x_ref", "u_ref", "com_ref", "stance", "ee_ref", "com_vel_ref")
# slots of the closed-loop score record (include/ilqr_hip.h ILQR_PLANT_SCORE_TERMS)
PLANT_SCORE_TERMS = ("state", "control", "upright", "balance", "joint_limits", "control_limits", "min_pelvis_height", "intervals")
# slots of the task score record (include/ilqr_hip.h ILQR_PLANT_TASK_SCORE_TERMS): per group (CoM, left foot, right foot) the largest
# violation in metres and the number of intervals above the tolerance; the sum of squared violations; the number of intervals scored
PLANT_TASK_SCORE_TERMS = ("max_com", "max_left", "max_right", "over_com", "over_left", "over_right", "sum_squares", "intervals")
# columns of a plant parameter set (include/ilqr_hip.h ILQR_PLANT_PARAMS)
PLANT_PARAMS = ("gravity_x", "gravity_y", "gravity_z", "friction", "softness", "limit_stiffness", "torque_gain")
# columns of a plant wrench record (include/ilqr_hip.h ILQR_PLANT_WRENCH)
PLANT_WRENCH = ("force_x", "force_y", "force_z", "torque_x", "torque_y", "torque_z", "point_x", "point_y", "point_z", "first", "end")
# columns of a plant payload record (include/ilqr_hip.h ILQR_PLANT_PAYLOAD)
PLANT_PAYLOAD = ("mass", "com_x", "com_y", "com_z", "Ixx", "Iyy", "Izz", "Ixy", "Ixz", "Iyz")
# groups of a plant observation record (include/ilqr_hip.h ILQR_PLANT_OBSERVATION): name, first tangent coordinate, width; the record is
# bias[50] then sigma[50] in this order
PLANT_OBSERVATION_GROUPS = (("position", 0, 3), ("orientation", 3, 3), ("joints", 6, 19), ("linear_velocity", 25, 3), ("angular_velocity", 28, 3), ("joint_velocities", 31, 19))
PLANT_OBSERVATION = 100
# a plant actuator record (include/ilqr_hip.h ILQR_PLANT_ACTUATOR): delay (plant substeps, an integer 0..PLANT_ACTUATOR_MAX_DELAY), tau[19], sigma[19]
PLANT_ACTUATOR = 39
PLANT_ACTUATOR_MAX_DELAY = 8
# fields of a plant joint record (include/ilqr_hip.h ILQR_PLANT_JOINTS), 19 values each in the order of u, with their nominal values
PLANT_JOINT_FIELDS = (("gain", 1.0), ("range_scale", 1.0), ("damping", 1.0), ("armature", 0.1))
PLANT_JOINTS = 76
# one record of the bounds table of the augmented-Lagrangian limits (ILQR_AL_BOUNDS): joint_lo[19], joint_hi[19], ctrl_lo[19], ctrl_hi[19]
AL_BOUNDS = 76
# one record of the state bounds of the augmented Lagrangian (ILQR_AL_STATE_BOUNDS): lo[28], hi[28] over the box coordinates -- pelvis
# position (3), pelvis linear velocity (3), pelvis angular velocity (3), joint velocities (19); al_state_slot(k) is coordinate k's state slot
AL_STATE_COORDS = 28
AL_STATE_BOUNDS = 56
# one row of a window of task bounds of the augmented Lagrangian (ILQR_AL_TASK_BOUNDS): lo[9], hi[9] over the task coordinates -- CoM x, y, z,
# left ankle origin x, y, z, right ankle origin x, y, z, world frame
AL_TASK_COORDS = 9
AL_TASK_BOUNDS = 18
# the velocities of those coordinates (ILQR_AL_TASK_VEL_COORDS): of the CoM, the left ankle origin and the right ankle origin, world frame, m/s
AL_TASK_VEL_COORDS = 9
# columns of a plant terrain record (include/ilqr_hip.h ILQR_PLANT_TERRAIN)
PLANT_TERRAIN = ("z_left", "z_right", "edge_x", "first", "end")



class ILQRError(RuntimeError):
    pass


_libs = {}
# test library with every cross-check kernel family compiled in (csrc/Makefile, -DILQR_LEGACY_KERNELS); the product library
# holds the default family only and refuses a handle whose environment selects another
LEGACY_LIB_PATH = os.path.join(_HERE, "lib", "libilqr_hip_legacy.so")


def load_library(path=None):
    """Load libilqr_hip.so (or the library at `path`); fails loudly when the HIP extension has not been built."""
    path = LIB_PATH if path is None else path
    lib = _libs.get(path)
    if lib is None:
        if not os.path.exists(path):
            raise ILQRError("HIP extension missing: %s (run __graft_entry__.build())" % path)
        lib = C.CDLL(path)
        lib.ilqr_hip_last_error.restype = C.c_char_p
        lib.ilqr_hip_stream.restype = C.c_void_p
        _libs[path] = lib
    return lib


def _c64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _table(a, B, width, what):
    """a per-rollout table as [n_sets, width] doubles, n_sets 1 or B (one record may come one-dimensional); `what` names it in the error"""
    a = _c64(a)
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2 or a.shape[1] != width or a.shape[0] not in (1, B):
        raise ValueError("plant %s must be [1, %d] or [B, %d]" % (what, width, width))
    return a


def _rows(a, count, width, what):
    """an optional per-item array of the single-step calls as [count, width] doubles; None stays None"""
    if a is None:
        return None
    a = _c64(a)
    if a.shape != (count, width):
        raise ValueError("%s must be [count, %d]" % (what, width))
    return a


def reference_kinematics(x):
    """(com[3], ee[2,3]) as RobotUtils::loadReferences computes them (robot_utils.cpp:369-403)."""
    L = load_library()
    x = _c64(x)
    com, ee = np.zeros(3), np.zeros((2, 3))
    rc = L.ilqr_hip_reference_kinematics(_p(x), _p(com), _p(ee))
    if rc:
        raise ILQRError(STATUS.get(rc, str(rc)))
    return com, ee


def reference_com_velocity(x):
    """CoM-velocity reference J_com(q) qvel as RobotUtils::loadReferences computes it (robot_utils.cpp:383-391)."""
    L = load_library()
    x = _c64(x)
    cv = np.zeros(3)
    rc = L.ilqr_hip_reference_com_velocity(_p(x), _p(cv))
    if rc:
        raise ILQRError(STATUS.get(rc, str(rc)))
    return cv


def terrain_stance(qpos, terrain, interval=0):
    """(stance[2], floor[2]) of qpos[26] on the floor of the record terrain[5] (columns PLANT_TERRAIN) in plant interval `interval`: foot f
    touches iff foot_clearance(qpos)[f] < floor[f], floor[f] = z_f while the window holds the interval and the foot's ankle-link origin is at
    world x >= edge_x, else 0 (ilqr_hip_terrain_stance: the rule of the plant under plant_set_terrain, on the host)."""
    L = load_library()
    q, t = _c64(qpos), _c64(terrain)
    if q.shape != (26,) or t.shape != (len(PLANT_TERRAIN),):
        raise ValueError("qpos must have 26 entries (MuJoCo order), terrain 5")
    st, fl = np.zeros(2, dtype=np.int32), np.zeros(2)
    rc = L.ilqr_hip_terrain_stance(_p(q), _p(t), C.c_long(int(interval)), st.ctypes.data_as(C.POINTER(C.c_int)), _p(fl))
    if rc:
        raise ILQRError(STATUS.get(rc, str(rc)))
    return st, fl


def foot_clearance(qpos):
    """Height of the lowest point of each foot's collision hull above the floor (get_contacts.py:96-147); [left, right]."""
    L = load_library()
    q = _c64(qpos)
    if q.shape != (26,):
        raise ValueError("qpos must have 26 entries (MuJoCo order)")
    clr = np.zeros(2)
    rc = L.ilqr_hip_foot_clearance(_p(q), _p(clr))
    if rc:
        raise ILQRError(STATUS.get(rc, str(rc)))
    return clr


def pelvis_inertial_offset():
    """Centre of mass of the pelvis body in the pelvis frame [3]: a wrench applied at this point is MuJoCo's xfrc_applied (host only)."""
    r = np.zeros(3)
    fn = load_library().ilqr_hip_pelvis_inertial_offset
    fn.restype = None
    fn(_p(r))
    return r


def gravity_compensation(x, gravity):
    """qfrc_bias[6+i] at zero velocity (RobotUtils::computeGravComp, robot_utils.cpp:844-866)."""
    L = load_library()
    x, g = _c64(x), _c64(gravity)
    u = np.zeros(NU)
    rc = L.ilqr_hip_gravity_compensation(_p(x), _p(g), _p(u))
    if rc:
        raise ILQRError(STATUS.get(rc, str(rc)))
    return u


def al_state_slot(k):
    """State slot of box coordinate k of the state bounds (ilqr_hip_al_state_slot; host only); -1 outside 0..27."""
    return int(load_library().ilqr_hip_al_state_slot(int(k)))


def al_default_bounds(margin=0.0):
    """The bounds set_augmented_lagrangian(margin=...) enforces without a table, as one record [AL_BOUNDS] = joint_lo[19], joint_hi[19],
    ctrl_lo[19], ctrl_hi[19]; margin = 0: the model's joint and control ranges (ilqr_hip_al_default_bounds; host only)."""
    out = np.zeros(AL_BOUNDS)
    rc = load_library().ilqr_hip_al_default_bounds(C.c_double(float(margin)), _p(out))
    if rc:
        raise ILQRError(STATUS.get(rc, str(rc)))
    return out


def weight_sets_of(prob, B):
    """The per-rollout weight table a problem dict asks for, or None: a table is wanted when any of Q / R / Qf is 2-D or task_weights /
    w_joint / w_ctrl has a leading axis of length B; the items that are still shared are broadcast to every set.
    Returns (Q [B,51], R [B,19], Qf [B,51], task [B,6], constraint [B,2])."""
    Q, R, Qf = (np.asarray(prob[k], dtype=np.float64) for k in ("Q", "R", "Qf"))
    task = np.asarray(prob["task_weights"], dtype=np.float64)
    wj, wc = np.asarray(prob["w_joint"], dtype=np.float64), np.asarray(prob["w_ctrl"], dtype=np.float64)
    if not (Q.ndim == 2 or R.ndim == 2 or Qf.ndim == 2 or task.ndim == 2 or wj.ndim == 1 or wc.ndim == 1):
        return None
    for name, a, shape in (("Q", Q, (NX,)), ("R", R, (NU,)), ("Qf", Qf, (NX,)), ("task_weights", task, (6,)), ("w_joint", wj, ()), ("w_ctrl", wc, ())):
        if a.shape != shape and a.shape != (B,) + shape:
            raise ValueError("%s: shape %s is neither %s (shared) nor %s (one per rollout)" % (name, a.shape, shape, (B,) + shape))
    bc = lambda a, shape: np.ascontiguousarray(np.broadcast_to(a, (B,) + shape))
    return bc(Q, (NX,)), bc(R, (NU,)), bc(Qf, (NX,)), bc(task, (6,)), np.ascontiguousarray(np.stack([np.broadcast_to(wj, (B,)), np.broadcast_to(wc, (B,))], axis=1))


class BatchedILQR:
    """iLQR for B independent rollouts on one GPU (reference include/ilqr/ilqr.hpp:17-45)."""

    def __init__(self, batch, N=25, dt=0.02, device=0, lib_path=None):
        self.L = load_library(lib_path)
        self.B, self.N, self.dt, self.device = int(batch), int(N), float(dt), int(device)
        self.max_iter = 10
        h = C.c_void_p()
        rc = self.L.ilqr_hip_create(C.byref(h), int(device), self.B, self.N, C.c_double(self.dt))
        self.h = h
        if rc:
            msg = self.L.ilqr_hip_last_error(h).decode() if h else ""
            self.close()
            raise ILQRError("ilqr_hip_create failed: %s %s" % (STATUS.get(rc, rc), msg))

    def set_dedup_saturated_retry(self, on=True):
        """Skip lambda retries whose lambda is already saturated (bit-identical repeats of the pass that has just failed); on by default,
        False restores the full retry (as ILQR_DEDUP_RETRY=0)."""
        self._chk(self.L.ilqr_hip_set_dedup_saturated_retry(self.h, int(bool(on))))

    def retry_pass_rollouts(self):
        """Rollouts whose lambda retry ran, summed over the iterations of the last solve (ilqr_hip_get_retry_pass_rollouts)."""
        fn = self.L.ilqr_hip_get_retry_pass_rollouts
        fn.restype = C.c_longlong
        n = int(fn(self.h))
        if n < 0:
            raise ILQRError("ilqr_hip_get_retry_pass_rollouts: %s" % self.L.ilqr_hip_last_error(self.h).decode())
        return n

    def set_relinearize_unchanged(self, on=True):
        """Re-linearise every rollout in every iteration (comparison, profiling); off by default: an iteration linearises only the rollouts
        whose nominal trajectory the previous one changed (ilqr_hip_set_relinearize_unchanged)."""
        self._chk(self.L.ilqr_hip_set_relinearize_unchanged(self.h, int(bool(on))))

    def linearized_rollouts(self):
        """Rollouts whose linearisation and cost quadratics ran, summed over the iterations of the last solve."""
        fn = self.L.ilqr_hip_get_linearized_rollouts
        fn.restype = C.c_longlong
        n = int(fn(self.h))
        if n < 0:
            raise ILQRError("ilqr_hip_get_linearized_rollouts: %s" % self.L.ilqr_hip_last_error(self.h).decode())
        return n

    def set_repeat_first_pass(self, on=True):
        """Run the first backward pass, line search and candidate costs of every iteration for every active rollout (comparison, profiling);
        off by default: from iteration 1 on they run only for the rollouts that accepted a candidate in the previous iteration
        (ilqr_hip_set_repeat_first_pass)."""
        self._chk(self.L.ilqr_hip_set_repeat_first_pass(self.h, int(bool(on))))

    def first_pass_rollouts(self):
        """Rollouts whose first pass ran, summed over the iterations of the last solve."""
        fn = self.L.ilqr_hip_get_first_pass_rollouts
        fn.restype = C.c_longlong
        n = int(fn(self.h))
        if n < 0:
            raise ILQRError("ilqr_hip_get_first_pass_rollouts: %s" % self.L.ilqr_hip_last_error(self.h).decode())
        return n

    def set_reroll_nominal(self, on=True):
        """Run every nominal rollout the reference executes, beside the linearisation with adoption and mismatch count (verification);
        off by default: a rollout whose result the buffers already hold -- iterations >= 1, iteration 0 behind a cold start -- is not
        launched (ilqr_hip_set_reroll_nominal; as ILQR_REUSE_ROLLOUT=0)."""
        self._chk(self.L.ilqr_hip_set_reroll_nominal(self.h, int(bool(on))))

    def nominal_rollouts(self):
        """Rollouts the nominal-rollout launches of the last solve were enqueued for (ilqr_hip_get_nominal_rollouts)."""
        fn = self.L.ilqr_hip_get_nominal_rollouts
        fn.restype = C.c_longlong
        n = int(fn(self.h))
        if n < 0:
            raise ILQRError("ilqr_hip_get_nominal_rollouts: null handle")
        return n

    def reload_environment(self):
        """Re-read the diagnostic environment switches (read once, at creation) for this handle."""
        self._chk(self.L.ilqr_hip_reload_environment(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.ilqr_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise ILQRError("%s: %s" % (STATUS.get(rc, rc), self.L.ilqr_hip_last_error(self.h).decode()))

    # ---- problem data (RobotUtils setters)
    def set_problem(self, prob):
        L, h = self.L, self.h
        self.set_problem_constants(prob)
        st = np.ascontiguousarray(prob["stance"], dtype=np.int32)
        self._chk(L.ilqr_hip_set_contact_schedule(h, st.ctypes.data_as(_ip), int(st.shape[0])))
        ee, cv = _c64(prob["ee_ref"]), _c64(prob["com_vel_ref"])
        self._chk(L.ilqr_hip_set_ee_references(h, _p(ee), _p(cv), int(ee.shape[0])))
        self.set_references(prob["x_ref"], prob["u_ref"], prob["com_ref"])

    def set_problem_constants(self, prob):
        """The items of a problem dict that are not reference windows: weights (or per-rollout weight sets) and gravity."""
        L, h = self.L, self.h
        sets = weight_sets_of(prob, self.B)
        if sets is not None:
            # per-rollout weights: the table carries every weight (shared items broadcast); the shared setters keep what they hold
            self.set_weight_sets(*sets)
        else:
            self._chk(L.ilqr_hip_set_cost_weights(h, _p(_c64(prob["Q"])), _p(_c64(prob["R"])), _p(_c64(prob["Qf"]))))
            self._chk(L.ilqr_hip_set_task_weights(h, *[C.c_double(float(v)) for v in prob["task_weights"]]))
            self._chk(L.ilqr_hip_set_constraint_weights(h, C.c_double(prob["w_joint"]), C.c_double(prob["w_ctrl"])))
            if self.num_weight_sets():
                self.clear_weight_sets()
        g = prob["gravity"]
        self.gravity = np.array(g, dtype=np.float64)
        self._chk(L.ilqr_hip_set_gravity(h, C.c_double(g[0]), C.c_double(g[1]), C.c_double(g[2])))

    def set_weight_sets(self, Q, R, Qf, task_weights, constraint_weights):
        """One set of cost weights per rollout (ilqr_hip_set_weight_sets): Q [n,51], R [n,19], Qf [n,51], task_weights [n,6] in the order of
        prob["task_weights"], constraint_weights [n,2] = (w_joint, w_ctrl); n = 1 or B.  Takes precedence over the shared weights until
        clear_weight_sets()."""
        Q, R, Qf, tw, cw = (np.atleast_2d(_c64(a)) for a in (Q, R, Qf, task_weights, constraint_weights))
        n = Q.shape[0]
        if Q.shape != (n, NX) or R.shape != (n, NU) or Qf.shape != (n, NX) or tw.shape != (n, 6) or cw.shape != (n, 2):
            raise ValueError("weight sets: Q [n,51], R [n,19], Qf [n,51], task_weights [n,6], constraint_weights [n,2] with one n")
        self._chk(self.L.ilqr_hip_set_weight_sets(self.h, _p(Q), _p(R), _p(Qf), _p(tw), _p(cw), int(n)))

    def clear_weight_sets(self):
        """Back to the shared weights the handle holds."""
        self._chk(self.L.ilqr_hip_clear_weight_sets(self.h))

    def num_weight_sets(self):
        """0: shared weights; else the number of sets of the installed table (1 or B)."""
        return int(self.L.ilqr_hip_num_weight_sets(self.h))

    # ---- augmented-Lagrangian joint and torque limits (include/ilqr_hip.h ilqr_hip_set_augmented_lagrangian)
    def set_augmented_lagrangian(self, rounds, rho_joint0, rho_ctrl0, growth=10.0, rho_max_factor=1e4, margin=0.0, tol_joint=1e-3, tol_ctrl=1e-2):
        """Enforce the joint and torque ranges (shrunk by `margin` of their width on each side) by up to `rounds` rounds of solve + multiplier
        update in every solve(); replaces the plain penalties w_joint / w_ctrl until clear_augmented_lagrangian()."""
        self._chk(self.L.ilqr_hip_set_augmented_lagrangian(self.h, int(rounds), *[C.c_double(float(v)) for v in (rho_joint0, rho_ctrl0, growth, rho_max_factor, margin, tol_joint, tol_ctrl)]))

    def clear_augmented_lagrangian(self):
        """Back to the plain penalties the handle holds."""
        self._chk(self.L.ilqr_hip_clear_augmented_lagrangian(self.h))

    def augmented_lagrangian_rounds(self):
        """0: not installed; else the rounds it was installed with."""
        return int(self.L.ilqr_hip_augmented_lagrangian_rounds(self.h))

    def al_multipliers(self):
        """(joint [B,N+1,19,2], ctrl [B,N,19,2]): the multipliers of the (lower, upper) bounds."""
        joint, ctrl = np.zeros((self.B, self.N + 1, NU, 2)), np.zeros((self.B, self.N, NU, 2))
        self._chk(self.L.ilqr_hip_get_al_multipliers(self.h, _p(joint), _p(ctrl)))
        return joint, ctrl

    def set_al_multipliers(self, joint=None, ctrl=None, rho=None):
        """Install multipliers (shapes of al_multipliers) and / or the penalties rho [B,2] = (joint, ctrl); None leaves that part as it is."""
        joint, ctrl, rho = (None if a is None else _c64(a) for a in (joint, ctrl, rho))
        if (joint is not None and joint.shape != (self.B, self.N + 1, NU, 2)) or (ctrl is not None and ctrl.shape != (self.B, self.N, NU, 2)) or (rho is not None and rho.shape != (self.B, 2)):
            raise ValueError("multipliers: joint [B,N+1,19,2], ctrl [B,N,19,2], rho [B,2]")
        self._chk(self.L.ilqr_hip_set_al_multipliers(self.h, _p(joint), _p(ctrl), _p(rho)))

    def al_penalties(self):
        """rho [B,2] = (joint, ctrl) as the store holds them."""
        return self._get("ilqr_hip_get_al_penalties", (self.B, 2))

    def al_violation(self):
        """(viol [B,2] = (joint, ctrl), done [B]) of the last update."""
        viol, done = np.zeros((self.B, 2)), np.zeros(self.B, dtype=np.int32)
        self._chk(self.L.ilqr_hip_get_al_violation(self.h, _p(viol), done.ctypes.data_as(_ip)))
        return viol, done

    def al_trace(self):
        """[rounds, B, 5]: joint violation, control violation, rho_joint, rho_ctrl, inner iterations of every round of the last solve (NaN: not run)."""
        return self._get("ilqr_hip_get_al_trace", (self.augmented_lagrangian_rounds(), self.B, 5))

    def al_update(self, round=0):
        """Stage call: the multiplier update on the resident nominal trajectory, into row `round` of the trace."""
        self._chk(self.L.ilqr_hip_al_update(self.h, int(round)))

    def set_al_bounds(self, bounds):
        """One table of bounds per rollout for the augmented-Lagrangian limits: [AL_BOUNDS] / [1, AL_BOUNDS] (every rollout) or
        [B, AL_BOUNDS] (rollout b reads row b); columns joint_lo[19], joint_hi[19], ctrl_lo[19], ctrl_hi[19] (al_default_bounds,
        scenario.stack_al_bounds).  The table holds the final bounds: the installed margin is not applied to it.  -inf / +inf switch a side
        off.  Acts on the cost only; stays until clear_al_bounds() or clear_augmented_lagrangian()."""
        b = _c64(bounds)
        if b.ndim == 1:
            b = b[None]
        if b.ndim != 2 or b.shape[1] != AL_BOUNDS:
            raise ValueError("bounds must be [%d], [1, %d] or [B, %d]" % (AL_BOUNDS, AL_BOUNDS, AL_BOUNDS))
        self._chk(self.L.ilqr_hip_set_al_bounds(self.h, _p(b), int(b.shape[0])))

    def clear_al_bounds(self):
        """Back to the model's ranges at the installed margin."""
        self._chk(self.L.ilqr_hip_clear_al_bounds(self.h))

    def num_al_bound_sets(self):
        """0: no table; else the number of records of the installed table (1 or B)."""
        return int(self.L.ilqr_hip_num_al_bound_sets(self.h))

    def al_bounds(self):
        """[B, AL_BOUNDS]: the record each rollout is solved with (without a table: the model's bounds at the installed margin)."""
        return self._get("ilqr_hip_get_al_bounds", (self.B, AL_BOUNDS))

    # ---- augmented-Lagrangian bounds on pelvis position, pelvis velocity and joint velocities (include/ilqr_hip.h ilqr_hip_set_al_state_bounds)
    def set_al_state_bounds(self, bounds, rho_state0, tol_state=1e-3):
        """Bounds on the 28 box coordinates, enforced as a third family of the installed augmented Lagrangian: [AL_STATE_BOUNDS] /
        [1, AL_STATE_BOUNDS] (every rollout) or [B, AL_STATE_BOUNDS] (rollout b reads row b); columns lo[28], hi[28]
        (scenario.stack_al_state_bounds).  -inf / +inf switch a side off.  rho_state0: the initial penalty of the family; a rollout is done
        only when its state violation is <= tol_state as well.  Acts on the cost only; stays until clear_al_state_bounds() or
        clear_augmented_lagrangian()."""
        b = _c64(bounds)
        if b.ndim == 1:
            b = b[None]
        if b.ndim != 2 or b.shape[1] != AL_STATE_BOUNDS:
            raise ValueError("bounds must be [%d], [1, %d] or [B, %d]" % (AL_STATE_BOUNDS, AL_STATE_BOUNDS, AL_STATE_BOUNDS))
        self._chk(self.L.ilqr_hip_set_al_state_bounds(self.h, _p(b), int(b.shape[0]), C.c_double(float(rho_state0)), C.c_double(float(tol_state))))

    def clear_al_state_bounds(self):
        """No state bounds any more."""
        self._chk(self.L.ilqr_hip_clear_al_state_bounds(self.h))

    def num_al_state_bound_sets(self):
        """0: no table; else the number of records of the installed table (1 or B)."""
        return int(self.L.ilqr_hip_num_al_state_bound_sets(self.h))

    def al_state_bounds(self):
        """[B, AL_STATE_BOUNDS]: the record each rollout is solved with (without a table: -inf / +inf)."""
        return self._get("ilqr_hip_get_al_state_bounds", (self.B, AL_STATE_BOUNDS))

    def al_state_multipliers(self):
        """[B,N+1,28,2]: the multipliers of the (lower, upper) bounds of the box coordinates."""
        return self._get("ilqr_hip_get_al_state_multipliers", (self.B, self.N + 1, AL_STATE_COORDS, 2))

    def set_al_state_multipliers(self, mu=None, rho=None):
        """Install state multipliers [B,N+1,28,2] and / or the penalties rho_state [B]; None leaves that part as it is."""
        mu, rho = (None if a is None else _c64(a) for a in (mu, rho))
        if (mu is not None and mu.shape != (self.B, self.N + 1, AL_STATE_COORDS, 2)) or (rho is not None and rho.shape != (self.B,)):
            raise ValueError("state multipliers: mu [B,N+1,28,2], rho [B]")
        self._chk(self.L.ilqr_hip_set_al_state_multipliers(self.h, _p(mu), _p(rho)))

    def al_state_penalties(self):
        """rho_state [B] as the store holds it."""
        return self._get("ilqr_hip_get_al_state_penalties", (self.B,))

    def al_state_violation(self):
        """viol_state [B] of the last update (the done flags: al_violation)."""
        return self._get("ilqr_hip_get_al_state_violation", (self.B,))

    def al_state_trace(self):
        """[rounds, B, 2]: state violation and rho_state of every round of the last solve (NaN: not run)."""
        return self._get("ilqr_hip_get_al_state_trace", (self.augmented_lagrangian_rounds(), self.B, 2))

    # ---- augmented-Lagrangian bounds on the centre of mass and the two ankle origins (include/ilqr_hip.h ilqr_hip_set_al_task_bounds)
    def set_al_task_bounds(self, win, rho_task0, tol_task=1e-3):
        """A window of bounds on the nine task coordinates (CoM, left ankle origin, right ankle origin; world frame), enforced as a fourth
        family of the installed augmented Lagrangian: [N+1, AL_TASK_BOUNDS] / [1, N+1, AL_TASK_BOUNDS] (every rollout) or
        [B, N+1, AL_TASK_BOUNDS]; row t holds knot t's lo[9], hi[9] (scenario.stack_al_task_bounds).  -inf / +inf switch a side off; a
        foot's rows are off at the knots where the contact schedule has it in stance.  rho_task0: the initial penalty of the family; a
        rollout is done only when its task violation (metres) is <= tol_task as well.  Acts on the cost only; horizon-local (a warm start
        shifts the multipliers, not the window); stays until clear_al_task_bounds() or clear_augmented_lagrangian()."""
        b = self._knot_window(win, AL_TASK_BOUNDS, "task bounds")
        self._chk(self.L.ilqr_hip_set_al_task_bounds(self.h, _p(b), int(b.shape[0]), C.c_double(float(rho_task0)), C.c_double(float(tol_task))))

    def clear_al_task_bounds(self):
        """No task bounds any more."""
        self._chk(self.L.ilqr_hip_clear_al_task_bounds(self.h))

    def num_al_task_bound_sets(self):
        """0: no window; else the number of windows installed (1 or B)."""
        return int(self.L.ilqr_hip_num_al_task_bound_sets(self.h))

    def al_task_bounds(self):
        """[B, N+1, AL_TASK_BOUNDS]: the window each rollout is solved with (without one: -inf / +inf)."""
        return self._get("ilqr_hip_get_al_task_bounds", (self.B, self.N + 1, AL_TASK_BOUNDS))

    def al_task_multipliers(self):
        """[B,N+1,9,2]: the multipliers of the (lower, upper) bounds of the task coordinates."""
        return self._get("ilqr_hip_get_al_task_multipliers", (self.B, self.N + 1, AL_TASK_COORDS, 2))

    def set_al_task_multipliers(self, mu=None, rho=None):
        """Install task multipliers [B,N+1,9,2] and / or the penalties rho_task [B]; None leaves that part as it is."""
        mu, rho = (None if a is None else _c64(a) for a in (mu, rho))
        if (mu is not None and mu.shape != (self.B, self.N + 1, AL_TASK_COORDS, 2)) or (rho is not None and rho.shape != (self.B,)):
            raise ValueError("task multipliers: mu [B,N+1,9,2], rho [B]")
        self._chk(self.L.ilqr_hip_set_al_task_multipliers(self.h, _p(mu), _p(rho)))

    def al_task_penalties(self):
        """rho_task [B] as the store holds it."""
        return self._get("ilqr_hip_get_al_task_penalties", (self.B,))

    def al_task_violation(self):
        """viol_task [B] of the last update, metres (the done flags: al_violation)."""
        return self._get("ilqr_hip_get_al_task_violation", (self.B,))

    def al_task_trace(self):
        """[rounds, B, 2]: task violation and rho_task of every round of the last solve (NaN: not run)."""
        return self._get("ilqr_hip_get_al_task_trace", (self.augmented_lagrangian_rounds(), self.B, 2))

    def al_task_points(self):
        """[B, N+1, 9]: the task coordinates of the resident nominal trajectory as the kernels compute them."""
        return self._get("ilqr_hip_get_al_task_points", (self.B, self.N + 1, AL_TASK_COORDS))

    def al_task_velocities(self):
        """[B, N+1, 9]: the velocities (m/s, world frame) of the task coordinates -- CoM, left ankle origin, right ankle origin -- at every knot
        of the resident nominal trajectory, in the convention of the cost's velocity terms.  Needs an installed augmented Lagrangian and an
        initialised trajectory."""
        return self._get("ilqr_hip_get_al_task_velocities", (self.B, self.N + 1, AL_TASK_VEL_COORDS))

    # ---- bounds that change from knot to knot (include/ilqr_hip.h ilqr_hip_set_al_knot_bounds)
    def _knot_window(self, bounds, width, what):
        """a window of bounds as [n_sets, N+1, width] doubles (one window may come two-dimensional)"""
        b = _c64(bounds)
        if b.ndim == 2:
            b = b[None]
        if b.ndim != 3 or b.shape[1:] != (self.N + 1, width):
            raise ValueError("%s must be [N+1, %d], [1, N+1, %d] or [B, N+1, %d]" % (what, width, width, width))
        return b

    def set_al_knot_bounds(self, bounds):
        """A window of joint / torque bounds per rollout in place of one record: [N+1, AL_BOUNDS] / [1, N+1, AL_BOUNDS] (every rollout) or
        [B, N+1, AL_BOUNDS]; row t holds knot t's bounds in the columns of set_al_bounds (scenario.stack_al_knot_bounds).  The torque
        columns of row N are checked and never read.  Replaces a table of set_al_bounds, keeps the multipliers; horizon-local (a warm start
        does not move it).  Stays until set_al_bounds(), clear_al_bounds() or clear_augmented_lagrangian()."""
        b = self._knot_window(bounds, AL_BOUNDS, "knot bounds")
        self._chk(self.L.ilqr_hip_set_al_knot_bounds(self.h, _p(b), int(b.shape[0])))

    def set_al_state_knot_bounds(self, bounds, rho_state0, tol_state=1e-3):
        """A window of state bounds per rollout: [N+1, AL_STATE_BOUNDS] / [1, N+1, AL_STATE_BOUNDS] or [B, N+1, AL_STATE_BOUNDS]; row t holds
        knot t's lo[28], hi[28] (scenario.stack_al_state_knot_bounds).  rho_state0 and tol_state as in set_al_state_bounds, which it replaces
        (and which replaces it)."""
        b = self._knot_window(bounds, AL_STATE_BOUNDS, "state knot bounds")
        self._chk(self.L.ilqr_hip_set_al_state_knot_bounds(self.h, _p(b), int(b.shape[0]), C.c_double(float(rho_state0)), C.c_double(float(tol_state))))

    def al_knot_bounds(self):
        """(joint_ctrl [B, N+1, AL_BOUNDS], state [B, N+1, AL_STATE_BOUNDS]): what each rollout is solved with at each knot, whoever wrote it --
        a window, a track cut, a table's record repeated over the knots, or the model's bounds at the installed margin and -inf / +inf."""
        jc, st = np.zeros((self.B, self.N + 1, AL_BOUNDS)), np.zeros((self.B, self.N + 1, AL_STATE_BOUNDS))
        self._chk(self.L.ilqr_hip_get_al_knot_bounds(self.h, _p(jc), _p(st)))
        return jc, st

    def al_bounds_per_knot(self):
        """Bit 0: the joint / torque bounds are a window; bit 1: the state bounds are one."""
        return int(self.L.ilqr_hip_al_bounds_per_knot(self.h))

    def set_al_bounds_track(self, joint_ctrl=None, state=None):
        """Upload a bounds track once: joint_ctrl [rows, AL_BOUNDS] and / or state [rows, AL_STATE_BOUNDS] on the loop's timeline (a state part
        needs installed state bounds, which supply rho_state0 and tol_state).  The start rows become one shared start of 0; a second call
        replaces the track."""
        jc, st = (None if a is None else _c64(a) for a in (joint_ctrl, state))
        if jc is None and st is None:
            raise ValueError("bounds track: joint_ctrl [rows, %d] and / or state [rows, %d]" % (AL_BOUNDS, AL_STATE_BOUNDS))
        rows = (jc if jc is not None else st).shape[0]
        if (jc is not None and jc.shape != (rows, AL_BOUNDS)) or (st is not None and st.shape != (rows, AL_STATE_BOUNDS)):
            raise ValueError("bounds track: joint_ctrl [rows, %d] and / or state [rows, %d] with one number of rows" % (AL_BOUNDS, AL_STATE_BOUNDS))
        self._chk(self.L.ilqr_hip_set_al_bounds_track(self.h, int(rows), _p(jc), _p(st)))

    def clear_al_bounds_track(self):
        """Free the bounds track; the windows last written stay installed."""
        self._chk(self.L.ilqr_hip_clear_al_bounds_track(self.h))

    def al_bounds_track_rows(self):
        """0 without a bounds track, else its rows."""
        return int(self.L.ilqr_hip_al_bounds_track_rows(self.h))

    def set_al_bounds_track_starts(self, starts):
        """One start row of the bounds track per rollout (B entries) or one shared start (one entry); every start >= 0."""
        st = np.ascontiguousarray(np.atleast_1d(starts), dtype=np.int32)
        if st.ndim != 1:
            raise ValueError("starts must be one-dimensional (one entry, or one per rollout)")
        self._chk(self.L.ilqr_hip_set_al_bounds_track_starts(self.h, st.ctypes.data_as(_ip), int(st.shape[0])))

    def set_al_task_bounds_track(self, task):
        """Upload the task family's bounds track once: task [rows, AL_TASK_BOUNDS], rows lo[9], hi[9] on the loop's timeline
        (scenario.stack_al_task_bounds, scenario.al_task_track_from_footsteps).  Needs installed task bounds (set_al_task_bounds), which
        supply rho_task0 and tol_task.  Its row count is its own, independent of set_al_bounds_track's; the start rows are shared with that
        track and become one shared start of 0.  A second call replaces the track."""
        tk = _c64(task)
        if tk.ndim != 2 or tk.shape[1] != AL_TASK_BOUNDS:
            raise ValueError("task bounds track: [rows, %d]" % AL_TASK_BOUNDS)
        self._chk(self.L.ilqr_hip_set_al_task_bounds_track(self.h, int(tk.shape[0]), _p(tk)))

    def clear_al_task_bounds_track(self):
        """Free the task bounds track; the window last written stays installed."""
        self._chk(self.L.ilqr_hip_clear_al_task_bounds_track(self.h))

    def al_task_bounds_track_rows(self):
        """0 without a task bounds track, else its rows."""
        return int(self.L.ilqr_hip_al_task_bounds_track_rows(self.h))

    def al_bounds_window_from_track(self, step):
        """Enqueue the ONE kernel that writes the bounds windows of MPC step `step` from every installed track (rollout b, knot t: track row
        min(start[b] + step + t, rows - 1), each track clamped to its own last row); uploads nothing and does not synchronise."""
        self._chk(self.L.ilqr_hip_al_bounds_window_from_track(self.h, int(step)))

    def set_references(self, x_ref, u_ref, com_ref):
        x_ref, u_ref, com_ref = _c64(x_ref), _c64(u_ref), _c64(com_ref)
        if x_ref.shape[1:] != (self.N + 1, NX) or u_ref.shape[1:] != (self.N, NU) or com_ref.shape[1:] != (self.N + 1, 3):
            raise ILQRError("reference size mismatch")  # iLQR::solve returns false (ilqr.cpp:526-532)
        self._chk(self.L.ilqr_hip_set_references(self.h, _p(x_ref), _p(u_ref), _p(com_ref), int(x_ref.shape[0])))

    # ---- reference windows from a track on the device (include/ilqr_hip.h "reference windows from a track")
    def set_reference_track(self, refdata):
        """Upload the full-length arrays of a references.ReferenceData (x_ref, u_ref, com_ref, ee_ref, com_vel_ref, contact) once; the start
        rows become one shared start of 0.  A second call replaces the track."""
        x, u, com, ee, cv = (_c64(a) for a in (refdata.x_ref, refdata.u_ref, refdata.com_ref, refdata.ee_ref, refdata.com_vel_ref))
        T = x.shape[0]
        if x.shape != (T, NX) or u.shape != (T, NU) or com.shape != (T, 3) or ee.shape != (T, 2, 3) or cv.shape != (T, 3):
            raise ValueError("reference track: x_ref [T,51], u_ref [T,19], com_ref [T,3], ee_ref [T,2,3], com_vel_ref [T,3] with one T")
        ct = np.ascontiguousarray(refdata.contact, dtype=np.int32)
        if ct.shape[0] and ct.shape[1:] != (2,):
            raise ValueError("reference track: contact [Tc,2]")
        self._chk(self.L.ilqr_hip_set_reference_track(self.h, int(T), _p(x), _p(u), _p(com), _p(ee), _p(cv), ct.ctypes.data_as(_ip) if ct.shape[0] else None, int(ct.shape[0])))

    def clear_reference_track(self):
        """Free the track; the windows last written stay installed."""
        self._chk(self.L.ilqr_hip_clear_reference_track(self.h))

    def reference_track_rows(self):
        """0 without a track, else its rows."""
        return int(self.L.ilqr_hip_reference_track_rows(self.h))

    def set_track_starts(self, starts):
        """One start row of the track per rollout (B entries) or one shared start (one entry); every start >= 0."""
        st = np.ascontiguousarray(np.atleast_1d(starts), dtype=np.int32)
        if st.ndim != 1:
            raise ValueError("starts must be one-dimensional (one entry, or one per rollout)")
        self._chk(self.L.ilqr_hip_set_track_starts(self.h, st.ctypes.data_as(_ip), int(st.shape[0])))

    def window_from_track(self, step, follow_schedule=False):
        """Enqueue the kernel that writes the reference windows of MPC step `step` (rollout b: track rows from start[b] + step on, the rule
        of ReferenceData.problem_at_starts) into the buffers the solver reads; uploads nothing and does not synchronise."""
        self._chk(self.L.ilqr_hip_window_from_track(self.h, int(step), int(bool(follow_schedule))))

    def reference_windows(self):
        """The reference windows the solver currently reads, one per rollout whoever wrote them: a dict with the six keys REFERENCE_KEYS."""
        B, n1 = self.B, self.N + 1
        out = dict(x_ref=np.zeros((B, n1, NX)), u_ref=np.zeros((B, self.N, NU)), com_ref=np.zeros((B, n1, 3)), ee_ref=np.zeros((B, n1, 2, 3)),
                   com_vel_ref=np.zeros((B, n1, 3)), stance=np.zeros((B, n1, 2), dtype=np.int32))
        self._chk(self.L.ilqr_hip_get_reference_windows(self.h, _p(out["x_ref"]), _p(out["u_ref"]), _p(out["com_ref"]), _p(out["ee_ref"]), _p(out["com_vel_ref"]),
                                                        out["stance"].ctypes.data_as(_ip)))
        return out

    # ---- options (ilqr.hpp:22-24)
    def set_regularization(self, lam):
        self._chk(self.L.ilqr_hip_set_regularization(self.h, C.c_double(lam)))

    def set_max_iterations(self, n):
        self._chk(self.L.ilqr_hip_set_max_iterations(self.h, int(n)))
        self.max_iter = int(n)

    def set_tolerance(self, tol):
        self._chk(self.L.ilqr_hip_set_tolerance(self.h, C.c_double(tol)))

    def set_options(self, jacobian_mode=JAC_ANALYTIC, fd_eps=1e-5, early_exit=True):
        self._chk(self.L.ilqr_hip_set_options(self.h, int(jacobian_mode), C.c_double(fd_eps), int(bool(early_exit))))

    def set_early_exit_gate(self, on=True):
        """Per-handle switch of the early-exit gate: off = solve_async enqueues all iterations at once and never blocks the host."""
        self._chk(self.L.ilqr_hip_set_early_exit_gate(self.h, int(bool(on))))

    # ---- initializeWithReference / solve
    def initialize(self, x0, u_init=None, prev_xbar=None, prev_ubar=None):
        ks = [_c64(x0), None if u_init is None else _c64(u_init), None if prev_xbar is None else _c64(prev_xbar), None if prev_ubar is None else _c64(prev_ubar)]
        self._chk(self.L.ilqr_hip_initialize(self.h, *[_p(k) for k in ks]))

    def _check_shift(self, shift):
        shift = int(shift)
        if not 1 <= shift <= self.N - 1:
            raise ValueError("shift must be in 1 .. N - 1")
        return shift

    def initialize_warm_resident(self, x0, shift=1):
        """Warm start from the resident solution shifted by `shift` knots (the knots applied since the last solve; 1: the reference's)."""
        shift, x0 = self._check_shift(shift), _c64(x0)
        if x0.shape != (self.B, NX):
            raise ValueError("x0 must be [B, 51]")
        if shift == 1:
            self._chk(self.L.ilqr_hip_initialize_warm_resident(self.h, _p(x0)))
        else:
            self._chk(self.L.ilqr_hip_initialize_warm_resident_shifted(self.h, _p(x0), shift))

    def initialize_device(self, x0_ptr, u_init_ptr):
        self._chk(self.L.ilqr_hip_initialize_device(self.h, C.c_void_p(x0_ptr), C.c_void_p(u_init_ptr)))

    def solve(self, x0=None):
        cost = np.zeros(self.B)
        x0 = None if x0 is None else _c64(x0)
        self._chk(self.L.ilqr_hip_solve(self.h, _p(x0), _p(cost)))
        return cost

    def solve_async(self):
        self._chk(self.L.ilqr_hip_solve_async(self.h))

    def synchronize(self):
        self._chk(self.L.ilqr_hip_synchronize(self.h))

    # ---- accessors (ilqr.hpp:34-37)
    def _get(self, fn, shape, dtype=np.float64):
        out = np.zeros(shape, dtype=dtype)
        ptr = out.ctypes.data_as(_dp if dtype == np.float64 else _ip)
        self._chk(getattr(self.L, fn)(self.h, ptr))
        return out

    def xbar(self):
        return self._get("ilqr_hip_get_xbar", (self.B, self.N + 1, NX))

    def ubar(self):
        return self._get("ilqr_hip_get_ubar", (self.B, self.N, NU))

    def gains_K(self):
        return self._get("ilqr_hip_get_gains_K", (self.B, self.N, NU, NX))

    def gains_kff(self):
        return self._get("ilqr_hip_get_gains_kff", (self.B, self.N, NU))

    def cost(self):
        return self._get("ilqr_hip_get_cost", (self.B,))

    def iterations(self):
        return self._get("ilqr_hip_get_iterations", (self.B,), np.int32)

    def lambdas(self):
        return self._get("ilqr_hip_get_lambda", (self.B,))

    def trace(self):
        cost = np.zeros((self.B, self.max_iter + 1))
        alpha = np.zeros((self.B, self.max_iter))
        lam = np.zeros((self.B, self.max_iter))
        self._chk(self.L.ilqr_hip_get_trace(self.h, _p(cost), _p(alpha), _p(lam)))
        return cost, alpha, lam

    def first_knot_device(self):
        """Device pointers (u0[B][19], K0[B][19][51], cost[B]) -- the payload of the per-step gather."""
        u0, K0, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self.L.ilqr_hip_first_knot_device(self.h, C.byref(u0), C.byref(K0), C.byref(c)))
        return u0.value, K0.value, c.value

    def pack_first_knot_device(self, u0_ptr, K0_ptr=None, cost_ptr=None):
        """Write u0[B][19] (+ K0[B][19][51], cost[B]) into caller-owned device buffers (gather payload)."""
        self._chk(self.L.ilqr_hip_pack_first_knot_device(self.h, C.c_void_p(u0_ptr), C.c_void_p(K0_ptr), C.c_void_p(cost_ptr)))

    # ---- multi-GPU: RCCL behind the C ABI (include/ilqr_hip.h "multi-GPU")
    @staticmethod
    def comm_available():
        """True if librccl can be opened with every entry point the gather needs (check on EVERY rank before comm_init(world > 1))."""
        return bool(load_library().ilqr_hip_comm_available())

    @staticmethod
    def comm_unique_id():
        """128-byte RCCL id (rank 0 creates it and hands it to every rank)."""
        L = load_library()
        buf = C.create_string_buffer(128)
        rc = L.ilqr_hip_comm_get_unique_id(buf)
        if rc:
            raise ILQRError("ilqr_hip_comm_get_unique_id: %s" % STATUS.get(rc, rc))
        return buf.raw

    def comm_init(self, world, rank, unique_id=None):
        self._chk(self.L.ilqr_hip_comm_init(self.h, int(world), int(rank), unique_id))

    def comm_destroy(self):
        self._chk(self.L.ilqr_hip_comm_destroy(self.h))

    def gather_first_knot(self, recv_ptr, root=0, with_gains=False):
        """Enqueue the per-step gather of [u0 | cost | (K0)] rows to `root` (recv_ptr: device buffer there, None elsewhere)."""
        self._chk(self.L.ilqr_hip_gather_first_knot(self.h, int(root), int(bool(with_gains)), C.c_void_p(recv_ptr)))

    def compute_control(self, x_measured, knot=0):
        """u = ubar_knot + K_knot (x - xbar_knot) [B,19]; knot 0 is MPC::stepOnce's law, later knots serve a caller that solves every m-th interval."""
        knot, x = int(knot), _c64(x_measured)
        if not 0 <= knot < self.N:
            raise ValueError("knot must be in 0 .. N - 1")
        if x.shape != (self.B, NX):
            raise ValueError("x_measured must be [B, 51]")
        u = np.zeros((self.B, NU))
        if knot == 0:
            self._chk(self.L.ilqr_hip_compute_control(self.h, _p(x), _p(u)))
        else:
            self._chk(self.L.ilqr_hip_compute_control_at(self.h, knot, _p(x), _p(u)))
        return u

    # ---- stage entry points
    def set_trajectory(self, xbar, ubar):
        self._chk(self.L.ilqr_hip_set_trajectory(self.h, _p(_c64(xbar)), _p(_c64(ubar))))

    def stage_rollout(self):
        self._chk(self.L.ilqr_hip_stage_rollout(self.h))

    def stage_linearize(self):
        self._chk(self.L.ilqr_hip_stage_linearize(self.h))

    def stage_cost_quadratics(self):
        self._chk(self.L.ilqr_hip_stage_cost_quadratics(self.h))

    def stage_backward_pass(self):
        self._chk(self.L.ilqr_hip_stage_backward_pass(self.h))

    def stage_line_search(self):
        imp = np.zeros(self.B, dtype=np.int32)
        cost, alpha = np.zeros(self.B), np.zeros(self.B)
        self._chk(self.L.ilqr_hip_stage_line_search(self.h, imp.ctypes.data_as(_ip), _p(cost), _p(alpha)))
        return imp.astype(bool), cost, alpha

    def stage_total_cost(self):
        cost = np.zeros(self.B)
        self._chk(self.L.ilqr_hip_stage_total_cost(self.h, _p(cost)))
        return cost

    def linearization(self):
        A = np.zeros((self.B, self.N, NX, NX))
        Bm = np.zeros((self.B, self.N, NX, NU))
        self._chk(self.L.ilqr_hip_get_linearization(self.h, _p(A), _p(Bm)))
        return A, Bm

    def set_linearization(self, A, Bm):
        self._chk(self.L.ilqr_hip_set_linearization(self.h, _p(_c64(A)), _p(_c64(Bm))))

    def quadratics(self):
        lx, lu = np.zeros((self.B, self.N + 1, NX)), np.zeros((self.B, self.N, NU))
        lxx, luu = np.zeros((self.B, self.N + 1, NX, NX)), np.zeros((self.B, self.N, NU))
        self._chk(self.L.ilqr_hip_get_quadratics(self.h, _p(lx), _p(lu), _p(lxx), _p(luu)))
        return lx, lu, lxx, luu

    def set_quadratics(self, lx, lu, lxx, luu):
        self._chk(self.L.ilqr_hip_set_quadratics(self.h, _p(_c64(lx)), _p(_c64(lu)), _p(_c64(lxx)), _p(_c64(luu))))

    def value_function(self):
        Vx, Vxx = np.zeros((self.B, NX)), np.zeros((self.B, NX, NX))
        self._chk(self.L.ilqr_hip_get_value_function(self.h, _p(Vx), _p(Vxx)))
        return Vx, Vxx

    def step(self, x, u):
        x, u = _c64(x), _c64(u)
        xn = np.zeros_like(x)
        self._chk(self.L.ilqr_hip_step(self.h, int(x.shape[0]), _p(x), _p(u), _p(xn)))
        return xn

    def step_stance(self, x, u, stance_left, stance_right):
        """One step with explicit stance flags (they matter in contact mode only)."""
        x, u = _c64(x), _c64(u)
        xn = np.zeros_like(x)
        self._chk(self.L.ilqr_hip_step_stance(self.h, int(x.shape[0]), _p(x), _p(u), int(stance_left), int(stance_right), _p(xn)))
        return xn

    def step_wrench(self, x, u, stance_left, stance_right, wrench):
        """step_stance with one external wrench on the pelvis per item: wrench [count, 9] = force, torque (world frame) and point of
        application (pelvis frame); always the two-lane step (ilqr_hip_step_wrench)."""
        x, u = _c64(x), _c64(u)
        wrench = _rows(_c64(wrench), x.shape[0], 9, "wrench")
        xn = np.zeros_like(x)
        self._chk(self.L.ilqr_hip_step_wrench(self.h, int(x.shape[0]), _p(x), _p(u), int(stance_left), int(stance_right), _p(wrench), _p(xn)))
        return xn

    def step_payload(self, x, u, stance_left, stance_right, payload, wrench=None):
        """step_wrench with one rigid payload on the pelvis per item as well: payload [count, 10] (columns PLANT_PAYLOAD), wrench [count, 9]
        or None for none; always the two-lane step (ilqr_hip_step_payload)."""
        x, u = _c64(x), _c64(u)
        payload = _rows(_c64(payload), x.shape[0], len(PLANT_PAYLOAD), "payload")
        wrench = _rows(wrench, x.shape[0], 9, "wrench")
        xn = np.zeros_like(x)
        self._chk(self.L.ilqr_hip_step_payload(self.h, int(x.shape[0]), _p(x), _p(u), int(stance_left), int(stance_right), _p(wrench), _p(payload), _p(xn)))
        return xn

    def step_joints(self, x, u, stance_left, stance_right, joints, wrench=None, payload=None):
        """step_payload with one joint record per item: joints [count, 76] (gain, range scale, damping, armature of the 19 joints;
        scenario.stack_plant_joints builds them), wrench [count, 9] and payload [count, 10] each or None for none; always the two-lane step
        (ilqr_hip_step_joints)."""
        x, u = _c64(x), _c64(u)
        joints = _rows(_c64(joints), x.shape[0], PLANT_JOINTS, "joints")
        wrench = _rows(wrench, x.shape[0], 9, "wrench")
        payload = _rows(payload, x.shape[0], len(PLANT_PAYLOAD), "payload")
        xn = np.zeros_like(x)
        self._chk(self.L.ilqr_hip_step_joints(self.h, int(x.shape[0]), _p(x), _p(u), int(stance_left), int(stance_right), _p(wrench), _p(payload), _p(joints), _p(xn)))
        return xn

    def step_terrain(self, x, u, terrain):
        """(x_next, stance [count, 2]): one step per item under the flags its own feet give on the floor terrain[i] = z_left, z_right, edge_x
        (terrain_stance with the window open), decided on the device; contact modes 2-4, always the two-lane step (ilqr_hip_step_terrain)."""
        x, u = _c64(x), _c64(u)
        terrain = _rows(_c64(terrain), x.shape[0], 3, "terrain")
        xn, st = np.zeros_like(x), np.zeros((x.shape[0], 2), dtype=np.int32)
        self._chk(self.L.ilqr_hip_step_terrain(self.h, int(x.shape[0]), _p(x), _p(u), _p(terrain), _p(xn), st.ctypes.data_as(C.POINTER(C.c_int))))
        return xn, st

    def set_stance_source(self, source):
        """Stance source of the dynamics (include/ilqr_hip.h): "schedule" (default) or "geometry" -- every step takes the stance flags from
        its own feet (a foot touches iff its ankle-link hull reaches the floor, foot_clearance < 0); the cost keeps the schedule."""
        code = {"schedule": 0, "geometry": 1}.get(source)
        if code is None:
            raise ValueError("stance source must be 'schedule' or 'geometry'")
        self._chk(self.L.ilqr_hip_set_stance_source(self.h, code))
        self.stance_source = source

    def step_geometry(self, x, u):
        """Plant step with contacts from geometry: (x_next [count,51], stance [count,2]) -- the flags each item decided from its own x."""
        x, u = _c64(x), _c64(u)
        xn = np.zeros_like(x)
        st = np.zeros((x.shape[0], 2), dtype=np.int32)
        self._chk(self.L.ilqr_hip_step_geometry(self.h, int(x.shape[0]), _p(x), _p(u), _p(xn), st.ctypes.data_as(_ip)))
        return xn, st

    def stance(self):
        """[B,N,2] stance flags the dynamics use for steps t = 0..N-1 of the current nominal trajectories."""
        st = np.zeros((self.B, self.N, 2), dtype=np.int32)
        self._chk(self.L.ilqr_hip_get_stance(self.h, st.ctypes.data_as(_ip)))
        return st

    def set_contact_mode(self, mode, softness=0.0):
        """0: constraint-free step; 1: rigid stance constraints on the feet the contact schedule marks;
        2: unilateral; 3: unilateral + Coulomb limit (set_friction), sliding feet without tangential force; 4: with kinetic friction."""
        self._chk(self.L.ilqr_hip_set_contact_mode(self.h, int(mode), C.c_double(softness)))
        self.contact_mode = int(mode)

    def set_friction(self, mu):
        """Sliding friction coefficient of contact modes 3 / 4 (unilateral stance + Coulomb limit)."""
        self._chk(self.L.ilqr_hip_set_friction(self.h, C.c_double(mu)))

    def set_joint_limits(self, on=True):
        """Joint-limit rows of the plant (include/ilqr_hip.h): a hinge past its range that the step would still move outward is stopped."""
        self._chk(self.L.ilqr_hip_set_joint_limits(self.h, int(bool(on))))

    def set_joint_limit_stiffness(self, k):
        """Restoring stiffness of the joint-limit rows (include/ilqr_hip.h): qacc_i = -v_i / h - k r_i on a constrained hinge; 0 = the pure stop,
        1 / (2 h)^2 = MuJoCo's default solref time constant."""
        self._chk(self.L.ilqr_hip_set_joint_limit_stiffness(self.h, C.c_double(float(k))))

    # ---- device-resident plant (include/ilqr_hip.h "device-resident plant"): the closed loop without a host round trip per MPC step
    def plant_reset(self, x):
        """Upload the plant state [B,51]: every rollout alive, no pending kick, history cursor at 0."""
        x = _c64(x)
        if x.shape != (self.B, NX):
            raise ValueError("plant state must be [B, 51]")
        self._chk(self.L.ilqr_hip_plant_reset(self.h, _p(x)))

    def plant_configure(self, substeps=1, feedback_mode=0, contact_source="schedule"):
        """`substeps` plant steps of dt / substeps per MPC step; feedback_mode 0 holds u over the interval (the reference's loop), 1 re-evaluates
        u = ubar0 + K0 (x - xbar0) before every substep; contact_source "schedule" (row 0 of the current schedule) or "geometry" (foot hulls)."""
        code = {"schedule": 0, "geometry": 1}.get(contact_source)
        if code is None:
            raise ValueError("contact_source must be 'schedule' or 'geometry'")
        self._chk(self.L.ilqr_hip_plant_configure(self.h, int(substeps), int(feedback_mode), code))

    def plant_kick(self, dv):
        """Arm a one-shot velocity kick [B,25] (order of qvel) for the next advance."""
        dv = _c64(dv)
        if dv.shape != (self.B, NV):
            raise ValueError("kick must be [B, 25]")
        self._chk(self.L.ilqr_hip_plant_kick(self.h, _p(dv)))

    def plant_advance(self):
        """Enqueue one MPC interval of the plant under the policy of the last solve; does not synchronise."""
        self._chk(self.L.ilqr_hip_plant_advance(self.h))

    def plant_follow(self, first_knot, count):
        """Enqueue `count` MPC intervals of the plant in one kernel, under the knots first_knot .. first_knot + count - 1 of the policy of the
        last solve (schedule rows likewise); plant_follow(0, 1) is plant_advance.  Does not synchronise."""
        first_knot, count = int(first_knot), int(count)
        if first_knot < 0 or count < 1 or first_knot + count > self.N:
            raise ValueError("need first_knot >= 0, count >= 1, first_knot + count <= N")
        self._chk(self.L.ilqr_hip_plant_follow(self.h, first_knot, count))

    def initialize_warm_from_plant(self, shift=1):
        """initialize_warm_resident(shift=shift) with x0 taken from the plant state on the device; does not synchronise."""
        shift = self._check_shift(shift)
        if shift == 1:
            self._chk(self.L.ilqr_hip_initialize_warm_from_plant(self.h))
        else:
            self._chk(self.L.ilqr_hip_initialize_warm_from_plant_shifted(self.h, shift))

    def plant_set_history(self, steps):
        """Allocate (steps > 0) or free (0) the history ring of the plant."""
        self._chk(self.L.ilqr_hip_plant_set_history(self.h, int(steps)))
        self._plant_hist_rows = int(steps)

    def plant_history(self):
        """(x [rows,B,51], u [rows,B,19]) of the recorded advances, oldest first: the state each advance started from and the control it applied."""
        rows = getattr(self, "_plant_hist_rows", 0)
        x, u = np.zeros((rows, self.B, NX)), np.zeros((rows, self.B, NU))
        rec = C.c_int(0)
        self._chk(self.L.ilqr_hip_plant_get_history(self.h, _p(x), _p(u), C.byref(rec)))
        return x[:rec.value], u[:rec.value]

    def plant_state(self):
        return self._get("ilqr_hip_plant_get_state", (self.B, NX))

    def plant_control(self):
        return self._get("ilqr_hip_plant_get_control", (self.B, NU))

    def plant_stance(self):
        return self._get("ilqr_hip_plant_get_stance", (self.B, 2), np.int32)

    def plant_alive(self):
        return self._get("ilqr_hip_plant_get_alive", (self.B,), np.int32)

    def plant_state_device(self):
        """Device pointer of the plant state [B][51] (for kernels chained on `stream`)."""
        p = C.c_void_p()
        self._chk(self.L.ilqr_hip_plant_state_device(self.h, C.byref(p)))
        return p.value

    def plant_set_score(self, Q, R, upright=0.0, balance=0.0, joint_limits=0.0, control_limits=0.0):
        """Install the closed-loop score (ilqr_hip_plant_set_score): from now on every plant_advance / plant_follow adds the cost terms of its
        intervals, under THESE weights (Q [51], R [19] diagonals and the four scalars; independent of the solver's), to a record per rollout.
        Empties the record.  The history ring must hold at least the intervals of the largest plant call."""
        Q, R = _c64(Q), _c64(R)
        if Q.shape != (NX,) or R.shape != (NU,):
            raise ValueError("score weights: Q [51], R [19]")
        self._chk(self.L.ilqr_hip_plant_set_score(self.h, _p(Q), _p(R), *[C.c_double(float(v)) for v in (upright, balance, joint_limits, control_limits)]))

    def plant_clear_score(self):
        """Remove the score: the plant calls launch what they launch without it."""
        self._chk(self.L.ilqr_hip_plant_clear_score(self.h))

    def plant_set_task_score(self, tol=0.0):
        """Install the task score (ilqr_hip_plant_set_task_score): from now on every plant_advance / plant_follow scores the state rows it
        appends to the history ring against the task window the handle holds then (row 0 for an advance, first_knot + j for interval j of a
        follow; a foot's rows off where the schedule has it in stance) and folds the result into a record per rollout; `tol` (metres) is the
        threshold of the counts.  Empties the record.  The history ring must hold at least the intervals of the largest plant call, and a
        task family must be installed when the plant is called."""
        self._chk(self.L.ilqr_hip_plant_set_task_score(self.h, C.c_double(float(tol))))

    def plant_clear_task_score(self):
        """Remove the task score: the plant calls launch what they launch without it."""
        self._chk(self.L.ilqr_hip_plant_clear_task_score(self.h))

    def plant_set_model(self, contact_mode=None, joint_limits=None):
        """The plant's own contact mode (0..4) and joint-limit option (bool), each None to follow the solver's (the default): the plant kernels
        step with that model, the solve keeps the solver's (ilqr_hip_plant_set_model).  Launches nothing."""
        mode = -1 if contact_mode is None else int(contact_mode)
        lim = -1 if joint_limits is None else int(bool(joint_limits))
        if contact_mode is not None and not 0 <= mode <= 4:
            raise ValueError("contact_mode must be None or 0..4")
        self._chk(self.L.ilqr_hip_plant_set_model(self.h, mode, lim))

    def plant_set_params(self, params):
        """Install plant parameter sets [n_sets, 7] (columns PLANT_PARAMS; scenario.stack_plant_params builds them), n_sets 1 or B: rollout b's
        plant steps with its own gravity, friction, softness, joint-limit stiffness and torque gain (ilqr_hip_plant_set_params)."""
        params = _table(params, self.B, len(PLANT_PARAMS), "parameters")
        self._chk(self.L.ilqr_hip_plant_set_params(self.h, _p(params), int(params.shape[0])))

    def plant_clear_params(self):
        """Remove the parameter sets: the plant steps every rollout with the handle's values again."""
        self._chk(self.L.ilqr_hip_plant_clear_params(self.h))

    def plant_num_param_sets(self):
        return int(self.L.ilqr_hip_plant_num_param_sets(self.h))

    def plant_params(self):
        """[B, 7] (columns PLANT_PARAMS): the values the plant would step each rollout with now; without a table the handle's and gain 1."""
        return self._get("ilqr_hip_plant_get_params", (self.B, len(PLANT_PARAMS)))

    def plant_set_wrench(self, wrench):
        """Install external wrenches on the pelvis [n_sets, 11] (columns PLANT_WRENCH; scenario.stack_plant_wrench builds them), n_sets 1 or B:
        rollout b's plant steps under force, torque and point of application of its record in the plant intervals first <= i < end, counted
        from plant_reset (ilqr_hip_plant_set_wrench).  The solve does not know of it."""
        wrench = _table(wrench, self.B, len(PLANT_WRENCH), "wrenches")
        self._chk(self.L.ilqr_hip_plant_set_wrench(self.h, _p(wrench), int(wrench.shape[0])))

    def plant_clear_wrench(self):
        """Remove the wrenches: the plant calls launch what they launch without them."""
        self._chk(self.L.ilqr_hip_plant_clear_wrench(self.h))

    def plant_num_wrench_sets(self):
        return int(self.L.ilqr_hip_plant_num_wrench_sets(self.h))

    def plant_wrench(self):
        """[B, 11] (columns PLANT_WRENCH): the record of each rollout; zeros without a table."""
        return self._get("ilqr_hip_plant_get_wrench", (self.B, len(PLANT_WRENCH)))

    def plant_intervals(self):
        """Plant intervals run since the last plant_reset (plant_advance adds 1, plant_follow its count)."""
        fn = self.L.ilqr_hip_plant_intervals
        fn.restype = C.c_long
        return int(fn(self.h))

    def plant_set_payload(self, payload):
        """Install rigid payloads on the pelvis [n_sets, 10] (columns PLANT_PAYLOAD; scenario.stack_plant_payload builds them), n_sets 1 or B:
        rollout b's plant carries mass, centre of mass and rotational inertia of its record in every substep until plant_clear_payload
        (ilqr_hip_plant_set_payload).  The solve does not know of it."""
        payload = _table(payload, self.B, len(PLANT_PAYLOAD), "payloads")
        self._chk(self.L.ilqr_hip_plant_set_payload(self.h, _p(payload), int(payload.shape[0])))

    def plant_clear_payload(self):
        """Remove the payloads: the plant calls launch what they launch without them."""
        self._chk(self.L.ilqr_hip_plant_clear_payload(self.h))

    def plant_num_payload_sets(self):
        return int(self.L.ilqr_hip_plant_num_payload_sets(self.h))

    def plant_get_payload(self):
        """[B, 10] (columns PLANT_PAYLOAD): the record of each rollout; zeros without a table."""
        return self._get("ilqr_hip_plant_get_payload", (self.B, len(PLANT_PAYLOAD)))

    def plant_set_joints(self, joints):
        """Install joint records [n_sets, 76] (gain, range scale, damping, armature of the 19 joints; scenario.stack_plant_joints builds them),
        n_sets 1 or B: rollout b's plant steps with the joints of its record until plant_clear_joints (ilqr_hip_plant_set_joints).  None
        clears.  The solve does not know of it; the plant keeps reporting the commanded torque."""
        if joints is None:
            return self.plant_clear_joints()
        joints = _table(joints, self.B, PLANT_JOINTS, "joints")
        self._chk(self.L.ilqr_hip_plant_set_joints(self.h, _p(joints), int(joints.shape[0])))

    def plant_clear_joints(self):
        """Remove the joint records: the plant calls launch what they launch without them."""
        self._chk(self.L.ilqr_hip_plant_set_joints(self.h, None, 0))

    def plant_get_joints(self):
        """[B, 76]: the record of each rollout; the nominal record without a table."""
        return self._get("ilqr_hip_plant_get_joints", (self.B, PLANT_JOINTS))

    def plant_set_terrain(self, terrain):
        """Install floors [n_sets, 5] (columns PLANT_TERRAIN; scenario.stack_plant_terrain builds them), n_sets 1 or B: in the plant intervals
        first <= i < end rollout b's feet land and lift against a floor of height z_left / z_right where their ankle is at x >= edge_x, and
        against z = 0 elsewhere (ilqr_hip_plant_set_terrain).  None clears.  Needs the stance source "geometry" and a plant contact mode
        2-4: a plant call under another configuration raises.  The solve does not know of it."""
        if terrain is None:
            return self.plant_clear_terrain()
        terrain = _table(terrain, self.B, len(PLANT_TERRAIN), "terrain records")
        self._chk(self.L.ilqr_hip_plant_set_terrain(self.h, _p(terrain), int(terrain.shape[0])))

    def plant_clear_terrain(self):
        """Remove the floors: the plant calls launch what they launch without them."""
        self._chk(self.L.ilqr_hip_plant_clear_terrain(self.h))

    def plant_num_terrain_sets(self):
        return int(self.L.ilqr_hip_plant_num_terrain_sets(self.h))

    def plant_get_terrain(self):
        """[B, 5] (columns PLANT_TERRAIN): the record of each rollout; without a table heights 0, edge -inf and an empty window."""
        return self._get("ilqr_hip_plant_get_terrain", (self.B, len(PLANT_TERRAIN)))

    def plant_set_observation(self, observation, seed=0, stream0=0):
        """Install observation models [n_sets, 100] (bias[50], sigma[50] in tangent order; scenario.stack_plant_observation builds them),
        n_sets 1 or B: the warm starts and the plant's control law read rollout b's state with the error of its record, drawn once per plant
        interval from the counter-based generator under `seed`, rollout stream stream0 + b (ilqr_hip_plant_set_observation).  The plant's
        physics, the ring and the score stay on the true state."""
        observation = _table(observation, self.B, PLANT_OBSERVATION, "observation records")
        seed, stream0 = int(seed), int(stream0)
        if not (0 <= seed < 1 << 64 and 0 <= stream0 < 1 << 64):
            raise ValueError("seed and stream0 must fit 64 unsigned bits")
        self._chk(self.L.ilqr_hip_plant_set_observation(self.h, _p(observation), int(observation.shape[0]), C.c_ulonglong(seed), C.c_ulonglong(stream0)))

    def plant_clear_observation(self):
        """Remove the observation models: the plant calls and warm starts launch what they launch without them."""
        self._chk(self.L.ilqr_hip_plant_clear_observation(self.h))

    def plant_num_observation_sets(self):
        return int(self.L.ilqr_hip_plant_num_observation_sets(self.h))

    def plant_get_observation(self):
        """(records [B, 100], seed, stream0): the record of each rollout; zeros and 0, 0 without a table."""
        out = np.zeros((self.B, PLANT_OBSERVATION))
        seed, stream0 = C.c_ulonglong(0), C.c_ulonglong(0)
        self._chk(self.L.ilqr_hip_plant_get_observation(self.h, _p(out), C.byref(seed), C.byref(stream0)))
        return out, int(seed.value), int(stream0.value)

    def plant_observation_errors(self, interval0, count):
        """delta [count, B, 51]: the state-shaped observation errors of the plant intervals interval0 .. interval0 + count - 1, a pure
        function of table, seed, stream0 and interval (ilqr_hip_plant_observation_errors); 1 <= count <= N."""
        interval0, count = int(interval0), int(count)
        if interval0 < 0 or count < 1 or count > self.N:
            raise ValueError("plant_observation_errors: interval0 >= 0 and 1 <= count <= N")
        out = np.zeros((count, self.B, NX))
        self._chk(self.L.ilqr_hip_plant_observation_errors(self.h, C.c_long(interval0), count, _p(out)))
        return out

    def plant_get_observed(self):
        """[B, 51]: the plant state as the controller is told it now, x [+] delta(plant_intervals) -- what a warm start would hand the solve;
        the plant state itself without a table."""
        return self._get("ilqr_hip_plant_get_observed", (self.B, NX))

    def plant_set_actuator(self, actuator, seed=0, stream0=0):
        """Install actuator models [n_sets, 39] (delay in plant substeps, tau[19] s, sigma[19] N m; scenario.stack_plant_actuator builds
        them), n_sets 1 or B: the torque the plant's joints get is the law's command behind a delay line, a first-order lag and noise drawn
        once per plant interval under `seed`, rollout stream stream0 + b (ilqr_hip_plant_set_actuator).  What the plant reports -- control,
        ring, score -- stays the command."""
        actuator = _table(actuator, self.B, PLANT_ACTUATOR, "actuator records")
        seed, stream0 = int(seed), int(stream0)
        if not (0 <= seed < 1 << 64 and 0 <= stream0 < 1 << 64):
            raise ValueError("seed and stream0 must fit 64 unsigned bits")
        self._chk(self.L.ilqr_hip_plant_set_actuator(self.h, _p(actuator), int(actuator.shape[0]), C.c_ulonglong(seed), C.c_ulonglong(stream0)))

    def plant_clear_actuator(self):
        """Remove the actuator models: the plant calls launch what they launch without them."""
        self._chk(self.L.ilqr_hip_plant_clear_actuator(self.h))

    def plant_num_actuator_sets(self):
        return int(self.L.ilqr_hip_plant_num_actuator_sets(self.h))

    def plant_get_actuator(self):
        """(records [B, 39], seed, stream0): the record of each rollout; zeros and 0, 0 without a table."""
        out = np.zeros((self.B, PLANT_ACTUATOR))
        seed, stream0 = C.c_ulonglong(0), C.c_ulonglong(0)
        self._chk(self.L.ilqr_hip_plant_get_actuator(self.h, _p(out), C.byref(seed), C.byref(stream0)))
        return out, int(seed.value), int(stream0.value)

    def plant_actuator_blend(self):
        """beta [B, 19] = -expm1(-h / tau) as the plant kernel reads it, to the bit (1 where tau == 0: never used, the kernel selects)."""
        return self._get("ilqr_hip_plant_get_actuator_blend", (self.B, NU))

    def plant_actuator_draws(self, interval0, count):
        """z [count, B, 19]: the standard normals of the torque noise in the plant intervals interval0 .. interval0 + count - 1, a pure
        function of seed, stream0 and interval (ilqr_hip_plant_actuator_draws); 1 <= count <= N."""
        interval0, count = int(interval0), int(count)
        if interval0 < 0 or count < 1 or count > self.N:
            raise ValueError("plant_actuator_draws: interval0 >= 0 and 1 <= count <= N")
        out = np.zeros((count, self.B, NU))
        self._chk(self.L.ilqr_hip_plant_actuator_draws(self.h, C.c_long(interval0), count, _p(out)))
        return out

    def plant_get_applied(self):
        """[B, 19]: the torque of the last substep run under the actuator table, in front of the torque gain and the clamp; the reported
        control without a table."""
        return self._get("ilqr_hip_plant_get_applied", (self.B, NU))

    def plant_score(self):
        """The record [B, 8], columns PLANT_SCORE_TERMS: six summed cost terms, the minimum pelvis height, the number of intervals scored."""
        return self._get("ilqr_hip_plant_get_score", (self.B, len(PLANT_SCORE_TERMS)))

    def plant_task_score(self):
        """The record [B, 8], columns PLANT_TASK_SCORE_TERMS: per group the largest violation and the intervals above the tolerance, the sum of
        squared violations (NaN once an interval had a non-finite point), the number of intervals scored."""
        return self._get("ilqr_hip_plant_get_task_score", (self.B, len(PLANT_TASK_SCORE_TERMS)))

    def enable_profiling(self, on=True):
        self._chk(self.L.ilqr_hip_enable_profiling(self.h, int(bool(on))))

    STAGE_KEYS = ["iLQR_computeCost+forwardRollout", "iLQR_linearization", "iLQR_costQuadratics", "iLQR_backwardPass", "iLQR_lineSearch", "iLQR_control",
                  "iLQR_backwardPass_retry", "iLQR_lineSearch_retry"]

    def set_profiled_stages(self, keys=None):
        """Time only the given stages (keys of stage_ms()) while profiling is on; None = all."""
        mask = 0xFF if keys is None else sum(1 << self.STAGE_KEYS.index(k) for k in keys)
        self._chk(self.L.ilqr_hip_set_profiled_stages(self.h, C.c_uint(mask)))

    def adopt_mismatches(self):
        """Elements in which the concurrent nominal re-rollouts of the last solve differed from the trajectory they replaced."""
        n = C.c_ulonglong(0)
        self._chk(self.L.ilqr_hip_get_adopt_mismatches(self.h, C.byref(n)))
        return int(n.value)

    def iterations_enqueued(self):
        """Iterations the last solve launched (fewer than max_iterations once the whole batch has taken the convergence exit)."""
        return int(self.L.ilqr_hip_get_iterations_enqueued(self.h))

    def speculative_iterations(self):
        """Iterations of the last solve whose lambda retry ran beside the first pass (small passes; ILQR_SPEC=0 disables)."""
        return int(self.L.ilqr_hip_get_speculative_iterations(self.h))

    ORDER_NAMES = ("sequential", "twin", "dual-sequential", "dual-twin", "listed-spec")

    def set_listed_spec(self, on=True):
        """Let late iterations of a fixed-iteration solve run their two lambda passes side by side from their lists (on by default;
        ilqr_hip_set_listed_spec; ILQR_SPEC_LISTS=0 or ILQR_SPEC=0 switch it off as well)."""
        self._chk(self.L.ilqr_hip_set_listed_spec(self.h, int(bool(on))))

    def listed_spec_iterations(self):
        """Iterations of the last solve in which the device took the listed side-by-side order (ilqr_hip_get_listed_spec_iterations)."""
        n = int(self.L.ilqr_hip_get_listed_spec_iterations(self.h))
        if n < 0:
            raise ILQRError("ilqr_hip_get_listed_spec_iterations: %s" % self.L.ilqr_hip_last_error(self.h).decode())
        return n

    def iteration_orders(self):
        """One code per enqueued iteration of the last solve (ilqr_hip_get_iteration_orders; index into ORDER_NAMES)."""
        out = np.zeros(max(self.max_iter, 1), dtype=np.int32)
        n = int(self.L.ilqr_hip_get_iteration_orders(self.h, out.ctypes.data_as(C.c_void_p)))
        if n < 0:
            raise ILQRError("ilqr_hip_get_iteration_orders: %s" % self.L.ilqr_hip_last_error(self.h).decode())
        return [int(v) for v in out[:n]]

    def iteration_lists(self, it):
        """(chg, kr) of iteration `it` of the last solve as sorted int arrays (ilqr_hip_get_iteration_lists)."""
        chg, kr = np.zeros(self.B, dtype=np.int32), np.zeros(self.B, dtype=np.int32)
        cnt = np.zeros(2, dtype=np.int32)
        self._chk(self.L.ilqr_hip_get_iteration_lists(self.h, int(it), chg.ctypes.data_as(C.c_void_p), kr.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)))
        return np.sort(chg[:cnt[0]]), np.sort(kr[:cnt[1]])

    def split_iterations(self):
        """Iterations of the last solve whose concurrent region ran in two groups (early continuation; ILQR_SPLIT=0 disables)."""
        return int(self.L.ilqr_hip_get_split_iterations(self.h))

    def num_slices(self):
        """Batch slices a solve is enqueued as (ILQR_SLICES)."""
        return int(self.L.ilqr_hip_num_slices(self.h))

    def stage_ms(self):
        ms, n = np.zeros(8), np.zeros(8)
        self._chk(self.L.ilqr_hip_get_stage_ms(self.h, _p(ms), _p(n)))
        keys = ["iLQR_computeCost+forwardRollout", "iLQR_linearization", "iLQR_costQuadratics", "iLQR_backwardPass", "iLQR_lineSearch", "iLQR_control",
                "iLQR_backwardPass_retry", "iLQR_lineSearch_retry"]
        return dict(zip(keys, ms)), dict(zip(keys, n))

    # ---- solve groups: several starts per problem, the best one adopted on the device (include/ilqr_hip.h "solve groups")
    def set_groups(self, G):
        """Cut the batch into B / G groups of G consecutive rollouts that solve one problem from G starts; G = 1 switches groups off
        (ilqr_hip_set_groups).  Removes an installed perturbation."""
        G = int(G)
        if G < 1 or self.B % G:
            raise ValueError("G must be >= 1 and divide the batch")
        self._chk(self.L.ilqr_hip_set_groups(self.h, G))
        self.G = G

    def num_groups(self):
        """Groups of the handle, 0 while the feature is off."""
        return int(self.L.ilqr_hip_num_groups(self.h))

    def group_set_perturbation(self, sigma, hold=1, seed=0, stream0=0):
        """sigma [19] or [1, 19] (every member g >= 1) or [G, 19] (row g for member g, row 0 zeros; scenario.stack_group_sigma): the standard
        deviation per actuator of what group_perturb adds to the controls of the members g >= 1, one draw per `hold` knots
        (ilqr_hip_group_set_perturbation).  Sets the draw counter to 0."""
        sigma = np.atleast_2d(_c64(sigma))
        if sigma.ndim != 2 or sigma.shape[1] != NU:
            raise ValueError("sigma must be [19], [1, 19] or [G, 19]")
        self._chk(self.L.ilqr_hip_group_set_perturbation(self.h, int(sigma.shape[0]), _p(sigma), int(hold), C.c_ulonglong(int(seed)), C.c_ulonglong(int(stream0))))

    def group_clear_perturbation(self):
        self._chk(self.L.ilqr_hip_group_clear_perturbation(self.h))

    def group_draws(self):
        """group_perturb calls since the perturbation was installed: the draw the next call uses."""
        fn = self.L.ilqr_hip_group_draws
        fn.restype = C.c_long
        return int(fn(self.h))

    def group_perturb(self):
        """Enqueue the perturbation of the starts: ubar of every member g >= 1 gets sigma o z, member 0 keeps every bit (ilqr_hip_group_perturb)."""
        self._chk(self.L.ilqr_hip_group_perturb(self.h))

    def group_select(self, key=None):
        """Enqueue the selection: per group the member with the smallest finite key, ties to the lowest member.  key: None (the cost of the
        last solve), a torch tensor [B] of doubles on the handle's device, or a device pointer to such an array (ilqr_hip_group_select)."""
        if key is not None and hasattr(key, "data_ptr"):
            if str(key.dtype) != "torch.float64" or key.numel() != self.B or not key.is_contiguous() or not key.is_cuda:
                raise ValueError("key must be a contiguous float64 device tensor of B entries")
            key = key.data_ptr()
        self._chk(self.L.ilqr_hip_group_select(self.h, C.c_void_p(key)))

    def group_winners(self):
        """(winner [M] global rollout indices, rec [M, 4] columns GROUP_RECORD) of the last group_select; synchronises."""
        M = self.num_groups()
        winner, rec = np.zeros(M, dtype=np.int32), np.zeros((M, 4))
        self._chk(self.L.ilqr_hip_group_get_winners(self.h, winner.ctypes.data_as(_ip), _p(rec)))
        return winner, rec

    def group_winners_device(self):
        """Device pointers (winner [M] ints, rec [M][4] doubles), without synchronising."""
        w, r = C.c_void_p(), C.c_void_p()
        self._chk(self.L.ilqr_hip_group_winners_device(self.h, C.byref(w), C.byref(r)))
        return w.value, r.value

    def group_copy_winners_device(self, out_ptr):
        """Enqueue a copy of winner [M] into a caller-owned device array of M ints (a row of a per-step log); no synchronisation."""
        self._chk(self.L.ilqr_hip_group_copy_winners_device(self.h, C.c_void_p(out_ptr)))

    def group_adopt(self):
        """Enqueue the adoption: every member of a group receives the solution state of its group's winner, bit for bit (ilqr_hip_group_adopt)."""
        self._chk(self.L.ilqr_hip_group_adopt(self.h))

    @property
    def stream(self):
        return self.L.ilqr_hip_stream(self.h)


class BatchedMPC:
    """MPC::stepOnce for a batch (reference src/ilqr/mpc.cpp:40-127): window -> warm start -> solve ->
    u = ubar0 + K0 (x - xbar0).  `window(t_idx)` returns (x_ref, u_ref, com_ref) for the current step
    (RobotUtils::getReferenceWindow, robot_utils.cpp:422-443)."""

    def __init__(self, solver, window):
        self.ilqr, self.window = solver, window
        self.t_idx, self.has_prev = 0, False
        self.last_solve_cost = None

    def reset(self):
        self.t_idx, self.has_prev = 0, False

    def step_once(self, x_measured):
        x_ref, u_ref, com_ref = self.window(self.t_idx)
        self.ilqr.set_references(x_ref, u_ref, com_ref)
        if self.has_prev:
            self.ilqr.initialize_warm_resident(x_measured)
        else:
            self.ilqr.initialize(x_measured)
        self.last_solve_cost = self.ilqr.solve(x_measured)
        u = self.ilqr.compute_control(x_measured)
        self.has_prev = True
        self.t_idx += 1
        return u
