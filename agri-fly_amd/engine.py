"""ctypes binding of include/agrifly_engine.h (the C ABI of the HIP engine).

Mirrors the C entry points one to one; see the header for which reference
interface (agri-fly file:line) each call replaces.  Host arrays are numpy,
planar ``[components, count]``.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# AGRIFLY_ENGINE_LIB selects another build of the same library (kernel A/B runs)
_LIB = os.environ.get("AGRIFLY_ENGINE_LIB") or os.path.join(_HERE, "lib", "libagrifly_engine.so")

AFE_F32, AFE_F64 = 0, 1
AFE_SEED_REFERENCE, AFE_SEED_DECORRELATED, AFE_SEED_COUNTER = 0, 1, 2
AFE_STEP_LAUNCH, AFE_STEP_PERSISTENT, AFE_STEP_AUTO, AFE_STEP_RESIDENT = 0, 1, 2, 3

# every symbol include/agrifly_engine.h declares (checked by tests/test_abi.py)
ABI_FUNCTIONS = [
    "afe_params_from_type", "afe_type_from_id", "afe_create", "afe_create_host_visible", "afe_destroy",
    "afe_last_error", "afe_status_string", "afe_abi_version", "afe_set_stream",
    "afe_set_type_table", "afe_set_vehicle_types", "afe_set_logic_period",
    "afe_set_imu_noise", "afe_set_state", "afe_get_state", "afe_set_state_f32",
    "afe_get_state_f32", "afe_set_rng_state", "afe_get_rng_state",
    "afe_set_motor_cmds", "afe_set_external_force", "afe_set_external_torque",
    "afe_step", "afe_steps_until_tick", "afe_sync", "afe_time_us",
    "afe_logic_ticks", "afe_get_imu", "afe_plan_ticks", "afe_get_device_view",
    "afe_algorithmic_bytes_per_step", "afe_event_create", "afe_event_destroy",
    "afe_event_record", "afe_event_elapsed_ms", "afe_pack_positions",
    "afe_nearest_neighbour", "afe_selftest_normals", "afe_selftest_normals_f32",
    "afe_rates_logic_params_from_type", "afe_set_rates_logic", "afe_set_rates_commands",
    "afe_get_motor_cmds", "afe_checkpoint_size", "afe_save_checkpoint", "afe_load_checkpoint",
    "afe_radio_create_rates_command", "afe_radio_create_position_command",
    "afe_radio_create_acceleration_command", "afe_radio_create_simple_command", "afe_radio_decode",
    "afe_telemetry_encode", "afe_telemetry_decode", "afe_set_commands_from_radio",
    "afe_set_max_fused_steps", "afe_set_addressing", "afe_step_kernel_info", "afe_planner_default_config", "afe_planner_samples", "afe_rappids_plan",
    "afe_set_split_stepping", "afe_rappids_plan_device", "afe_planner_release_scratch", "afe_camera_default", "afe_camera_default_mount", "afe_scene_create",
    "afe_scene_destroy", "afe_scene_info", "afe_scene_set_walk", "afe_render_depth", "afe_render_depth_engine", "afe_render_depth_stats",
    "afe_device_alloc", "afe_device_free", "afe_device_download", "afe_scene_check_hierarchy",
    "afe_comm_unique_id", "afe_comm_create", "afe_comm_info", "afe_comm_destroy", "afe_comm_last_error",
    "afe_gather_positions", "afe_group_create", "afe_group_destroy", "afe_group_size", "afe_group_shard",
    "afe_group_step", "afe_group_sync", "afe_group_gather_positions", "afe_group_last_error", "afe_group_peer_access",
    "afe_nearest_neighbour_grid", "afe_neighbour_grid_info", "afe_set_neighbour_grid_refresh", "afe_set_neighbour_sort_reuse", "afe_nearest_neighbour_bruteforce",
    "afe_uwb_create", "afe_uwb_destroy", "afe_uwb_set_noise", "afe_uwb_draw", "afe_uwb_range",
    "afe_set_step_mode", "afe_steps_completed", "afe_persistent_running", "afe_stream_probe",
    "afe_set_noise_seed", "afe_set_gust_process", "afe_get_external_force", "afe_nearest_neighbour_async", "afe_query_sync",
    "afe_gather_exchange", "afe_set_cache_policy", "afe_grid_time", "afe_cache_policy_in_use", "afe_set_resident_queue",
    "afe_has_dev_hooks", "afe_persistent_kernarg_layout", "afe_group_set_staged_copies",
    "afe_clearance_map_create", "afe_clearance_map_destroy", "afe_clearance_map_info", "afe_clearance_check_hierarchy",
    "afe_clearance_query", "afe_clearance_query_stats", "afe_clearance_query_engine",
    "afe_path_sample_points", "afe_clearance_paths", "afe_clearance_paths_stats", "afe_clearance_plans_engine",
    "afe_contact_monitor_create", "afe_contact_monitor_update", "afe_contact_monitor_get", "afe_contact_monitor_reset",
    "afe_contact_monitor_destroy",
    "afe_clearance_segments", "afe_clearance_segments_stats", "afe_clearance_paths_swept", "afe_clearance_paths_swept_stats",
    "afe_clearance_plans_engine_swept", "afe_path_chord_deviation", "afe_contact_monitor_create_swept",
    "afe_stats_check_layout", "afe_stats_create", "afe_stats_destroy", "afe_stats_info", "afe_stats_set_reference",
    "afe_stats_set_histogram", "afe_stats_update", "afe_stats_get", "afe_stats_reset",
    "afe_image_truth_sample_times", "afe_image_truth_paths", "afe_image_truth_paths_stats", "afe_image_truth_plans",
    "afe_image_truth_candidates", "afe_device_upload",
    "afe_low_battery_threshold_from_type",
    "afe_raycast", "afe_raycast_stats", "afe_line_of_sight",
    "afe_range_sensor_create", "afe_range_sensor_update", "afe_range_sensor_info", "afe_range_sensor_destroy",
    "afe_get_rates_commands",
    "afe_follower_default_config", "afe_follower_ring_slots", "afe_follower_create", "afe_follower_destroy", "afe_follower_info",
    "afe_follower_set_hold", "afe_follower_set_goal", "afe_follower_set_plans", "afe_follower_get_plans",
    "afe_follower_planner_inputs", "afe_follower_plan", "afe_follower_tick", "afe_follower_get_reference",
    "afe_follower_get_command", "afe_follower_selftest_math",
    "afe_estimator_default_config", "afe_estimator_ring_slots", "afe_estimator_create", "afe_estimator_destroy", "afe_estimator_info",
    "afe_estimator_measure", "afe_estimator_predict", "afe_estimator_get_prediction", "afe_estimator_announce",
    "afe_estimator_get_state", "afe_estimator_reset", "afe_estimator_selftest_math", "afe_follower_attach_estimator",
    "afe_gps_estimator_default_config", "afe_gps_estimator_create", "afe_gps_estimator_destroy", "afe_gps_estimator_info",
    "afe_gps_estimator_imu", "afe_gps_estimator_measure", "afe_gps_estimator_get_state", "afe_gps_estimator_set_state",
    "afe_gps_estimator_reset", "afe_gps_estimator_selftest_math", "afe_follower_attach_gps_estimator",
    "afe_stages_default_config", "afe_stages_create", "afe_stages_destroy", "afe_stages_info", "afe_stages_set_desired_position",
    "afe_stages_set_desired_yaw", "afe_stages_set_centre", "afe_stages_set_unsafe", "afe_stages_request", "afe_stages_set_warnings",
    "afe_stages_tick", "afe_stages_get", "afe_stages_attach_gps_estimator", "afe_stages_selftest_math",
    "afe_onboard_default_config", "afe_onboard_create", "afe_onboard_destroy", "afe_onboard_info", "afe_onboard_set_battery",
    "afe_onboard_radio", "afe_onboard_tick", "afe_onboard_get", "afe_onboard_set_state", "afe_onboard_telemetry",
    "afe_onboard_selftest_math",
]


class AfeError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("agrifly_engine status %d: %s" % (status, message))
        self.status = status


class VehicleParams(C.Structure):
    """afe_vehicle_params == the Quadcopter_T constructor arguments
    (reference Components/Components/Simulation/Quadcopter_T.hpp:24-32)."""
    _fields_ = [
        ("mass", C.c_double),
        ("inertia", C.c_double * 9),
        ("arm_length", C.c_double),
        ("com_error", C.c_double * 3),
        ("motor_min_speed", C.c_double),
        ("motor_max_speed", C.c_double),
        ("prop_thrust_from_speed_sqr", C.c_double),
        ("prop_torque_from_speed_sqr", C.c_double),
        ("motor_time_const", C.c_double),
        ("motor_inertia", C.c_double),
        ("lin_drag_coeff_b", C.c_double * 3),
        ("imu_yaw", C.c_float),
        ("imu_pitch", C.c_float),
        ("imu_roll", C.c_float),
    ]

    def copy(self):
        other = VehicleParams()
        C.memmove(C.byref(other), C.byref(self), C.sizeof(VehicleParams))
        return other

    @property
    def hover_speed(self):
        """per-motor speed at which 4 k_f w^2 = m g"""
        return float(np.sqrt(self.mass * 9.81 / (4.0 * self.prop_thrust_from_speed_sqr)))


class RatesLogicParams(C.Structure):
    """afe_rates_logic_params: the rates-control slice of Onboard::QuadcopterLogic."""
    _fields_ = [
        ("mass", C.c_float), ("inertia", C.c_float * 9),
        ("ang_vel_time_const_xy", C.c_float), ("ang_vel_time_const_z", C.c_float),
        ("arm_length", C.c_float), ("prop_thrust_from_speed_sqr", C.c_float),
        ("prop_torque_from_thrust", C.c_float), ("prop0_spin_dir", C.c_int),
        ("max_thrust_per_propeller", C.c_float), ("min_thrust_per_propeller", C.c_float),
        ("max_cmd_total_thrust", C.c_float),
        ("imu_yaw", C.c_float), ("imu_pitch", C.c_float), ("imu_roll", C.c_float),
        ("gyro_lowpass_cutoff", C.c_float),
    ]


class RadioMessage(C.Structure):
    _fields_ = [("type", C.c_uint8), ("flags", C.c_uint8), ("floats", C.c_float * 10)]


class TelemetryPacket(C.Structure):
    _fields_ = [("type", C.c_uint8), ("packet_number", C.c_uint8), ("accel", C.c_float * 3),
                ("gyro", C.c_float * 3), ("motor_forces", C.c_float * 4), ("position", C.c_float * 3),
                ("batt_voltage", C.c_float), ("velocity", C.c_float * 3), ("attitude", C.c_float * 3),
                ("debug_vals", C.c_float * 6), ("panic_reason", C.c_uint8), ("warnings", C.c_uint8)]


RADIO_PACKET_SIZE, TELEMETRY_PACKET_SIZE = 23, 30


class PlannerConfig(C.Structure):
    """afe_planner_config (RAPPIDS depth-image planner)"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("depth_scale", C.c_double), ("focal_length", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("true_vehicle_radius", C.c_double),
                ("planning_vehicle_radius", C.c_double), ("min_checking_dist", C.c_double),
                ("min_thrust", C.c_double), ("max_thrust", C.c_double), ("max_ang_vel", C.c_double),
                ("max_velocity", C.c_double), ("min_section_time", C.c_double), ("max_pyramids", C.c_int),
                ("pixel_buffer", C.c_int), ("cost_type", C.c_int), ("cost_vec", C.c_double * 3)]


class PlanOutput(C.Structure):
    _fields_ = [("found", C.c_int), ("best_index", C.c_int), ("best_cost", C.c_double),
                ("coeffs", (C.c_double * 3) * 6), ("tf", C.c_double), ("n_generated", C.c_int),
                ("n_cost_checks", C.c_int), ("n_collision_checks", C.c_int), ("n_velocity_checks", C.c_int),
                ("n_collision_free", C.c_int), ("n_pyramids", C.c_int)]


# PlanOutput as a numpy record (same layout), for hosts that consume 10^4..10^5 plans per frame
PLAN_DTYPE = np.dtype([("found", np.int32), ("best_index", np.int32), ("best_cost", np.float64),
                       ("coeffs", np.float64, (6, 3)), ("tf", np.float64), ("n_generated", np.int32),
                       ("n_cost_checks", np.int32), ("n_collision_checks", np.int32), ("n_velocity_checks", np.int32),
                       ("n_collision_free", np.int32), ("n_pyramids", np.int32)])


def plans_as_array(out):
    """zero-copy numpy view of the PlanOutput array rappids_plan returns"""
    assert PLAN_DTYPE.itemsize == C.sizeof(PlanOutput)
    return np.frombuffer(out, dtype=PLAN_DTYPE)


class FollowerConfig(C.Structure):
    """afe_follower_config (set struct_bytes before handing one to the library; follower_default_config does)"""
    _fields_ = [("struct_bytes", C.c_size_t), ("period_us", C.c_uint64), ("delay_us", C.c_uint64),
                ("lookahead_s", C.c_double), ("omega_step_s", C.c_double), ("mount", C.c_double * 4),
                ("nat_freq", C.c_float), ("damping", C.c_float), ("att_time_const_xy", C.c_float),
                ("att_time_const_z", C.c_float), ("hover_thrust", C.c_double)]


class EstimatorConfig(C.Structure):
    """afe_estimator_config (estimator_default_config sets struct_bytes)"""
    _fields_ = [("struct_bytes", C.c_size_t), ("command_delay_s", C.c_double), ("rate_time_constant_s", C.c_double),
                ("gate", C.c_double), ("sigma_pos", C.c_double), ("sigma_att", C.c_double), ("sigma_acc", C.c_double),
                ("sigma_ang_acc", C.c_double), ("offboard_period_us", C.c_uint64), ("max_measure_gap_us", C.c_uint64)]


class GpsEstimatorConfig(C.Structure):
    """afe_gps_estimator_config (gps_estimator_default_config sets struct_bytes)"""
    _fields_ = [("struct_bytes", C.c_size_t), ("init_sigma_pos", C.c_double), ("init_sigma_vel", C.c_double),
                ("init_sigma_att", C.c_double), ("sigma_acc", C.c_double), ("sigma_gyro", C.c_double), ("sigma_pos", C.c_double),
                ("accel_lowpass_cutoff", C.c_float)]


class StagesConfig(C.Structure):
    """afe_stages_config (stages_default_config sets struct_bytes)"""
    _fields_ = [("struct_bytes", C.c_size_t), ("period_us", C.c_uint64), ("delay_us", C.c_uint64),
                ("nat_freq", C.c_float), ("damping", C.c_float), ("att_time_const_xy", C.c_float), ("att_time_const_z", C.c_float),
                ("min_corner", C.c_double * 3), ("max_corner", C.c_double * 3), ("min_normal_height", C.c_double),
                ("not_seen_timeout_s", C.c_double), ("spool_up_time_s", C.c_double), ("spool_up_thrust_by_weight", C.c_double),
                ("takeoff_time_s", C.c_double), ("get_into_action_time_s", C.c_double), ("landing_speed", C.c_double),
                ("traj_id", C.c_int)]


class StagesFields(C.Structure):
    """afe_stages_fields: where afe_stages_get writes (NULL: not read back)"""
    _fields_ = [("struct_bytes", C.c_size_t), ("stage", C.c_void_p), ("last_stage", C.c_void_p), ("t0_us", C.c_void_p),
                ("safety", C.c_void_p), ("ready", C.c_void_p), ("init_pos3", C.c_void_p), ("desired_pos3", C.c_void_p),
                ("last_pos3", C.c_void_p), ("last_vel3", C.c_void_p), ("last_acc3", C.c_void_p), ("cmd_yaw", C.c_void_p),
                ("computed4", C.c_void_p), ("sent4", C.c_void_p), ("msg_type", C.c_void_p)]


class OnboardConfig(C.Structure):
    """afe_onboard_config (onboard_default_config sets struct_bytes)"""
    _fields_ = [("struct_bytes", C.c_size_t), ("accel_lowpass_cutoff", C.c_float), ("batt_lowpass_cutoff", C.c_float),
                ("temp_lowpass_cutoff", C.c_float), ("main_loop_monitor_cutoff", C.c_float), ("cmd_rate_monitor_cutoff", C.c_float),
                ("att_time_const_xy", C.c_float), ("att_time_const_z", C.c_float), ("low_battery_threshold", C.c_float),
                ("radio_cmd_period", C.c_float)]


class OnboardFields(C.Structure):
    """afe_onboard_fields: where afe_onboard_get writes (NULL: not read back)"""
    _fields_ = [("struct_bytes", C.c_size_t), ("flight_state", C.c_void_p), ("panic_reason", C.c_void_p), ("warnings", C.c_void_p),
                ("est_att4", C.c_void_p), ("est_ang_vel3", C.c_void_p), ("acc_filtered3", C.c_void_p), ("batt_filtered", C.c_void_p),
                ("main_loop_dt", C.c_void_p), ("cmd_dt", C.c_void_p), ("motor_forces4", C.c_void_p), ("cycle_counter", C.c_void_p),
                ("last_radio_us", C.c_void_p), ("motors_running", C.c_void_p)]


class OnboardState(C.Structure):
    """afe_onboard_state: what afe_onboard_set_state writes (NULL: left as it is)"""
    _fields_ = [("struct_bytes", C.c_size_t), ("est_att4", C.c_void_p), ("est_ang_vel3", C.c_void_p), ("imu_initialized", C.c_void_p),
                ("lowpass20", C.c_void_p), ("flight_state", C.c_void_p), ("motors_running", C.c_void_p), ("last_radio_us", C.c_void_p)]


AFE_FS_UNINITIALIZED, AFE_FS_IDLE, AFE_FS_FULLY_AUTONOMOUS, AFE_FS_PANIC, AFE_FS_KILLED, AFE_FS_EXTERNAL_ACCELERATION_CONTROL, \
    AFE_FS_EXTERNAL_RATES_CONTROL = range(7)
AFE_PANIC_NO_PANIC, AFE_PANIC_ONBOARD_ESTIMATE_CRAZY, AFE_PANIC_UWB_TIMEOUT, AFE_PANIC_UPSIDE_DOWN, AFE_PANIC_RADIO_CMD_TIMEOUT, \
    AFE_PANIC_LOW_BATTERY, AFE_PANIC_KILLED_INTERNALLY, AFE_PANIC_KILLED_EXTERNALLY = range(8)
AFE_WARN_CMD_RATE, AFE_WARN_UWB_RESET, AFE_WARN_ONBOARD_FREQ, AFE_WARN_CMD_BATCH_DROP = 0x02, 0x04, 0x08, 0x10
AFE_RADIO_FLAG_DISABLE_SAFETY_CHECKS = 0x02
AFE_STAGE_WAIT_FOR_START, AFE_STAGE_SPOOL_UP, AFE_STAGE_TAKEOFF, AFE_STAGE_FLIGHT, AFE_STAGE_LANDING, AFE_STAGE_COMPLETE, \
    AFE_STAGE_EMERGENCY = range(7)
AFE_SAFETY_NOT_SEEN, AFE_SAFETY_UNSAFE_POSITION, AFE_SAFETY_UPSIDE_DOWN_AND_LOW, AFE_SAFETY_USER_UNSAFE = 1, 2, 4, 8
AFE_WARN_LOW_BATT = 0x01


class DeviceView(C.Structure):
    _fields_ = [
        ("struct_bytes", C.c_size_t), ("n_vehicles", C.c_int64), ("stride", C.c_int64), ("state_elem_size", C.c_int),
        ("pos", C.c_void_p), ("vel", C.c_void_p), ("att", C.c_void_p),
        ("ang_vel", C.c_void_p), ("motor_speed", C.c_void_p),
        ("ext_force", C.c_void_p), ("ext_torque", C.c_void_p),
        ("motor_cmd", C.c_void_p), ("gyro", C.c_void_p), ("acc", C.c_void_p),
        ("rng", C.c_void_p), ("type_index", C.c_void_p), ("pos_anchor_xy", C.c_void_p),
    ]


def stream_probe(n, n_read=24, n_write=17, launches=100, device=-1):
    """afe_stream_probe: microseconds per launch of a pure streaming kernel in the step kernel's launch shape"""
    us = C.c_float(0)
    rc = library().afe_stream_probe(int(device), int(n), int(n_read), int(n_write), int(launches), C.byref(us))
    if rc:
        raise AfeError(rc, "afe_stream_probe")
    return us.value


def library_path():
    return _LIB


def build_library(force=False):
    """hipcc --offload-arch=gfx950 build of csrc/ into lib/ (in-tree)."""
    src = os.path.join(_HERE, "csrc")
    if force and os.path.exists(_LIB):
        os.remove(_LIB)
    subprocess.check_call(["make", "-s", "-C", src])
    if not os.path.exists(_LIB):
        raise RuntimeError("engine build produced no " + _LIB)
    return _LIB


_AG = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)
_BC = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int)
_GR = C.CFUNCTYPE(C.c_int, C.c_void_p)


class GatherTransport(C.Structure):
    """afe_gather_transport: the collectives afe_gather_exchange runs on"""
    _fields_ = [("ctx", C.c_void_p), ("all_gather", _AG), ("broadcast", _BC), ("group_start", _GR), ("group_end", _GR)]


def gather_exchange(all_gather, broadcast, rank, n_ranks, counts, packed_xyz, xyz_all):
    """afe_gather_exchange over host arrays with Python collectives:
    all_gather(send: float32[count], recv: float32[n_ranks * count]); broadcast(send, recv: float32[count], root).
    packed_xyz float32 [3, n_local], xyz_all float32 [3, n_all] (both C-contiguous, written in place)."""
    def view(ptr, count):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_float)), shape=(int(count),))

    def ag(_, send, recv, count):
        try:
            all_gather(view(send, count), view(recv, count * n_ranks))
            return 0
        except Exception:      # noqa: BLE001  (an exception must not cross the C frame)
            return 1

    def bc(_, send, recv, count, root):
        try:
            broadcast(view(send, count), view(recv, count), int(root))
            return 0
        except Exception:      # noqa: BLE001
            return 1

    t = GatherTransport(None, _AG(ag), _BC(bc), _GR(), _GR())
    cnt = None if counts is None else np.ascontiguousarray(counts, dtype=np.int64)
    assert packed_xyz.dtype == np.float32 and xyz_all.dtype == np.float32 and packed_xyz.flags.c_contiguous and xyz_all.flags.c_contiguous
    rc = library().afe_gather_exchange(C.byref(t), int(rank), int(n_ranks), None if cnt is None else cnt.ctypes.data,
                                       int(packed_xyz.shape[1]), packed_xyz.ctypes.data, xyz_all.ctypes.data)
    if rc:
        raise AfeError(rc, "afe_gather_exchange")


class Camera(C.Structure):
    """afe_camera: the pinhole depth camera of Rappids_Simulator/main.cpp:120-122,360."""
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("focal_length", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
        ("depth_scale", C.c_double),
        ("max_count", C.c_int32), ("reserved", C.c_int32),
    ]


_lib = None


def library():
    """Load the engine library; fails loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise ImportError(
            "HIP engine library %s is missing: run `python -c \"import __graft_entry__ as g; "
            "g.build()\"` (hipcc, gfx950). There is no CPU fallback." % _LIB)
    L = C.CDLL(_LIB)
    i64, u64, vp, ci = C.c_int64, C.c_uint64, C.c_void_p, C.c_int
    eng = vp
    sig = {
        "afe_params_from_type": [ci, C.POINTER(VehicleParams)],
        "afe_type_from_id": [C.c_uint],
        "afe_low_battery_threshold_from_type": [ci, C.POINTER(C.c_float)],
        "afe_create": [C.POINTER(vp), i64, ci, ci, i64],
        "afe_create_host_visible": [C.POINTER(vp), i64, ci, ci, i64],
        "afe_destroy": [eng],
        "afe_abi_version": [],
        "afe_set_stream": [eng, vp],
        "afe_set_type_table": [eng, C.POINTER(VehicleParams), ci],
        "afe_set_vehicle_types": [eng, i64, i64, vp],
        "afe_set_logic_period": [eng, C.c_double],
        "afe_set_imu_noise": [eng, ci, C.c_double, C.c_double, ci],
        "afe_set_state": [eng, i64, i64, vp, vp, vp, vp, vp],
        "afe_get_state": [eng, i64, i64, vp, vp, vp, vp, vp],
        "afe_set_state_f32": [eng, i64, i64, vp, vp, vp, vp, vp],
        "afe_get_state_f32": [eng, i64, i64, vp, vp, vp, vp, vp],
        "afe_set_rng_state": [eng, i64, i64, vp],
        "afe_get_rng_state": [eng, i64, i64, vp],
        "afe_set_motor_cmds": [eng, i64, i64, vp],
        "afe_set_external_force": [eng, i64, i64, vp],
        "afe_set_external_torque": [eng, i64, i64, vp],
        "afe_step": [eng, u64, ci],
        "afe_steps_until_tick": [eng, u64, C.POINTER(ci)],
        "afe_sync": [eng],
        "afe_time_us": [eng, C.POINTER(u64)],
        "afe_logic_ticks": [eng, C.POINTER(u64)],
        "afe_get_imu": [eng, i64, i64, vp, vp],
        "afe_plan_ticks": [C.c_double, C.POINTER(u64), u64, ci, vp],
        "afe_get_device_view": [eng, C.POINTER(DeviceView)],
        "afe_algorithmic_bytes_per_step": [eng, ci, C.POINTER(C.c_double)],
        "afe_event_create": [C.POINTER(vp)],
        "afe_event_destroy": [vp],
        "afe_event_record": [eng, vp],
        "afe_event_elapsed_ms": [vp, vp, C.POINTER(C.c_float)],
        "afe_pack_positions": [eng, vp],
        "afe_nearest_neighbour": [eng, vp, i64, vp, vp],
        "afe_selftest_normals": [eng, vp, i64, vp, vp],
        "afe_selftest_normals_f32": [eng, vp, i64, vp, vp],
        "afe_rates_logic_params_from_type": [ci, C.POINTER(RatesLogicParams)],
        "afe_set_rates_logic": [eng, C.POINTER(RatesLogicParams), ci],
        "afe_set_rates_commands": [eng, i64, i64, vp, vp],
        "afe_get_motor_cmds": [eng, i64, i64, vp],
        "afe_radio_create_rates_command": [C.c_uint8, C.c_float, vp, vp],
        "afe_radio_create_position_command": [C.c_uint8, vp, vp, vp, vp],
        "afe_radio_create_acceleration_command": [C.c_uint8, vp, C.c_float, vp],
        "afe_radio_create_simple_command": [ci, C.c_uint8, vp],
        "afe_radio_decode": [vp, C.POINTER(RadioMessage)],
        "afe_telemetry_encode": [C.POINTER(TelemetryPacket), vp],
        "afe_telemetry_decode": [vp, C.POINTER(TelemetryPacket)],
        "afe_set_commands_from_radio": [eng, i64, i64, vp],
        "afe_set_max_fused_steps": [eng, ci],
        "afe_set_split_stepping": [eng, ci],
        "afe_set_step_mode": [eng, ci],
        "afe_nearest_neighbour_async": [eng, vp, i64, vp, vp],
        "afe_query_sync": [eng],
        "afe_gather_exchange": [C.POINTER(GatherTransport), ci, ci, vp, i64, vp, vp],
        "afe_set_noise_seed": [eng, u64],
        "afe_set_gust_process": [eng, ci, u64, C.c_double, u64, i64],
        "afe_get_external_force": [eng, i64, i64, vp],
        "afe_stream_probe": [ci, i64, ci, ci, ci, C.POINTER(C.c_float)],
        "afe_steps_completed": [eng, C.POINTER(u64)],
        "afe_persistent_running": [eng, C.POINTER(ci)],
        "afe_set_addressing": [eng, ci],
        "afe_step_kernel_info": [eng, C.POINTER(ci), C.POINTER(ci)],
        "afe_planner_default_config": [C.POINTER(PlannerConfig), ci, ci] + [C.c_double] * 5,
        "afe_planner_samples": [C.c_uint32, ci, ci, ci, vp],
        "afe_rappids_plan": [ci, C.POINTER(PlannerConfig), i64, vp, i64, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp,
                             C.POINTER(C.c_float)],
        "afe_planner_release_scratch": [],
        "afe_rappids_plan_device": [ci, C.POINTER(PlannerConfig), i64, vp, i64, vp, vp, vp, vp, vp, vp, ci, vp, ci, vp,
                                    vp, C.POINTER(C.c_float)],
        "afe_camera_default": [C.POINTER(Camera), ci, ci],
        "afe_camera_default_mount": [vp],
        "afe_scene_create": [ci, vp, i64, C.POINTER(vp)],
        "afe_scene_info": [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(ci), vp],
        "afe_scene_check_hierarchy": [vp, i64, C.POINTER(i64), C.POINTER(ci), C.POINTER(ci)],
        "afe_render_depth": [vp, C.POINTER(Camera), i64, vp, vp, vp, vp, C.POINTER(C.c_float)],
        "afe_render_depth_engine": [eng, vp, C.POINTER(Camera), i64, i64, vp, vp, ci, C.POINTER(C.c_float)],
        "afe_render_depth_stats": [vp, C.POINTER(Camera), i64, vp, vp, vp, vp, C.POINTER(C.c_float)],
        "afe_scene_set_walk": [vp, C.c_int],
        "afe_device_alloc": [ci, u64, C.POINTER(vp)],
        "afe_device_free": [vp],
        "afe_device_download": [vp, vp, u64],
        "afe_device_upload": [vp, vp, u64],
        "afe_checkpoint_size": [eng, C.POINTER(u64)],
        "afe_save_checkpoint": [eng, vp, u64],
        "afe_load_checkpoint": [eng, vp, u64],
        "afe_comm_unique_id": [vp],
        "afe_comm_create": [C.POINTER(vp), vp, ci, ci, ci],
        "afe_comm_info": [vp, C.POINTER(ci), C.POINTER(ci)],
        "afe_comm_destroy": [vp],
        "afe_gather_positions": [eng, vp, vp, vp],
        "afe_group_create": [C.POINTER(vp), i64, ci, vp, ci],
        "afe_group_peer_access": [vp, C.POINTER(ci)],
        "afe_set_cache_policy": [eng, ci],
        "afe_cache_policy_in_use": [eng, C.POINTER(ci)],
        "afe_has_dev_hooks": [],
        "afe_persistent_kernarg_layout": [ci, vp, vp, vp],
        "afe_group_set_staged_copies": [vp, ci],
        "afe_set_resident_queue": [eng, ci],
        "afe_grid_time": [eng, C.POINTER(u64), C.POINTER(u64)],
        "afe_group_destroy": [vp],
        "afe_group_size": [vp, C.POINTER(ci), C.POINTER(i64)],
        "afe_group_shard": [vp, ci, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64)],
        "afe_group_step": [vp, u64, ci],
        "afe_group_sync": [vp],
        "afe_group_gather_positions": [vp, vp],
        "afe_nearest_neighbour_grid": [eng, vp, i64, C.c_float, vp, vp],
        "afe_neighbour_grid_info": [eng, vp, C.POINTER(C.c_float), C.POINTER(i64), C.POINTER(i64)],
        "afe_nearest_neighbour_bruteforce": [eng, vp, i64, vp, i64, vp, vp],
        "afe_set_neighbour_grid_refresh": [eng, ci],
        "afe_set_neighbour_sort_reuse": [eng, ci],
        "afe_uwb_create": [C.POINTER(vp)],
        "afe_uwb_set_noise": [vp, C.c_double, C.c_double, C.c_double],
        "afe_uwb_draw": [vp, i64, vp, vp],
        "afe_uwb_range": [vp, eng, vp, i64, vp, vp, i64, vp, vp],
        "afe_clearance_map_create": [ci, vp, i64, C.POINTER(vp)],
        "afe_clearance_map_destroy": [vp],
        "afe_clearance_map_info": [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(ci), vp],
        "afe_clearance_check_hierarchy": [vp, i64, C.POINTER(i64), C.POINTER(ci), C.POINTER(ci)],
        "afe_clearance_query": [vp, i64, vp, C.c_double, vp, vp, vp, C.POINTER(C.c_float)],
        "afe_clearance_query_stats": [vp, i64, vp, C.c_double, vp, C.POINTER(C.c_float)],
        "afe_clearance_query_engine": [eng, vp, i64, i64, C.c_double, vp, vp, vp, ci, C.POINTER(C.c_float)],
        "afe_path_sample_points": [vp, C.c_double, C.c_double, vp, vp, ci, vp, vp],
        "afe_clearance_paths": [vp, i64, vp, vp, vp, vp, ci, C.c_double, C.c_double, vp, C.POINTER(i64), C.POINTER(C.c_float)],
        "afe_clearance_paths_stats": [vp, i64, vp, vp, vp, vp, ci, C.c_double, C.c_double, vp, C.POINTER(C.c_float)],
        "afe_clearance_plans_engine": [eng, vp, i64, i64, vp, vp, ci, C.c_double, C.c_double, vp, C.POINTER(i64), C.POINTER(C.c_float)],
        "afe_contact_monitor_create": [eng, vp, C.c_double, C.c_double, C.POINTER(vp)],
        "afe_contact_monitor_update": [vp, C.POINTER(i64), C.POINTER(i64)],
        "afe_contact_monitor_get": [vp, i64, i64, vp, vp, vp],
        "afe_contact_monitor_reset": [vp, i64, i64],
        "afe_contact_monitor_destroy": [vp],
        "afe_clearance_segments": [vp, i64, vp, vp, C.c_double, vp, C.POINTER(C.c_float)],
        "afe_clearance_segments_stats": [vp, i64, vp, vp, C.c_double, vp, C.POINTER(C.c_float)],
        "afe_clearance_paths_swept": [vp, i64, vp, vp, vp, vp, ci, C.c_double, C.c_double, vp, C.POINTER(i64), C.POINTER(C.c_float)],
        "afe_clearance_paths_swept_stats": [vp, i64, vp, vp, vp, vp, ci, C.c_double, C.c_double, vp, C.POINTER(C.c_float)],
        "afe_clearance_plans_engine_swept": [eng, vp, i64, i64, vp, vp, ci, C.c_double, C.c_double, vp, C.POINTER(i64), C.POINTER(C.c_float)],
        "afe_path_chord_deviation": [vp, C.c_double, C.c_double, vp, ci, C.POINTER(C.c_double)],
        "afe_contact_monitor_create_swept": [eng, vp, C.c_double, C.c_double, C.POINTER(vp)],
        "afe_stats_check_layout": [vp, ci, i64, C.POINTER(i64), C.POINTER(ci)],
        "afe_stats_create": [eng, vp, ci, C.POINTER(vp)],
        "afe_stats_destroy": [vp],
        "afe_stats_info": [vp, C.POINTER(ci), C.POINTER(i64), C.POINTER(ci), C.POINTER(u64)],
        "afe_stats_set_reference": [vp, i64, i64, vp],
        "afe_stats_set_histogram": [vp, vp, ci],
        "afe_stats_update": [vp, vp, vp],
        "afe_stats_get": [vp, i64, i64, vp, vp, vp, vp, vp, vp],
        "afe_stats_reset": [vp, i64, i64],
        "afe_image_truth_sample_times": [C.c_double, C.c_double, C.c_double, C.POINTER(ci), vp],
        "afe_image_truth_paths": [ci, C.POINTER(PlannerConfig), i64, vp, i64, ci, vp, vp, vp, C.c_double, vp, C.POINTER(i64), C.POINTER(C.c_float)],
        "afe_image_truth_paths_stats": [ci, C.POINTER(PlannerConfig), i64, vp, i64, ci, vp, vp, vp, C.c_double, vp, C.POINTER(C.c_float)],
        "afe_image_truth_plans": [ci, C.POINTER(PlannerConfig), i64, vp, i64, ci, vp, vp, C.c_double, vp, C.POINTER(i64), C.POINTER(C.c_float)],
        "afe_image_truth_candidates": [ci, C.POINTER(PlannerConfig), i64, vp, i64, ci, vp, vp, vp, vp, ci, vp, ci, vp, C.c_double, vp, vp, vp, vp,
                                       C.POINTER(C.c_float)],
        "afe_raycast": [vp, i64, vp, vp, vp, vp, vp, C.POINTER(C.c_float)],
        "afe_raycast_stats": [vp, i64, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_float)],
        "afe_line_of_sight": [vp, i64, vp, vp, vp, C.POINTER(C.c_float)],
        "afe_range_sensor_create": [eng, vp, vp, vp, ci, C.POINTER(vp)],
        "afe_range_sensor_update": [vp, i64, i64, vp, vp, ci, C.POINTER(C.c_float)],
        "afe_range_sensor_info": [vp, C.POINTER(ci), C.POINTER(i64)],
        "afe_range_sensor_destroy": [vp],
        "afe_get_rates_commands": [eng, i64, i64, vp, vp, vp],
        "afe_follower_default_config": [ci, C.POINTER(FollowerConfig)],
        "afe_follower_ring_slots": [u64, u64, C.POINTER(ci)],
        "afe_follower_create": [eng, C.POINTER(FollowerConfig), C.POINTER(vp)],
        "afe_follower_destroy": [vp],
        "afe_follower_info": [vp, C.POINTER(i64), C.POINTER(ci), C.POINTER(u64), C.POINTER(ci)],
        "afe_follower_set_hold": [vp, i64, i64, vp],
        "afe_follower_set_goal": [vp, i64, i64, vp],
        "afe_follower_set_plans": [vp, i64, i64, vp, vp, vp, vp, vp, vp, vp],
        "afe_follower_get_plans": [vp, i64, i64, vp, vp, vp, vp, vp, vp, vp],
        "afe_follower_planner_inputs": [vp, vp, vp, vp, vp],
        "afe_follower_plan": [vp, C.POINTER(PlannerConfig), vp, vp, ci, vp, vp, C.POINTER(i64), C.POINTER(C.c_float)],
        "afe_follower_tick": [vp, C.POINTER(i64)],
        "afe_follower_get_reference": [vp, i64, i64, vp],
        "afe_follower_get_command": [vp, i64, i64, vp, vp],
        "afe_follower_selftest_math": [ci, ci, i64, vp, vp],
        "afe_estimator_default_config": [C.POINTER(EstimatorConfig)],
        "afe_estimator_ring_slots": [C.POINTER(EstimatorConfig), C.POINTER(ci)],
        "afe_estimator_create": [eng, C.POINTER(EstimatorConfig), C.POINTER(vp)],
        "afe_estimator_destroy": [vp],
        "afe_estimator_info": [vp, C.POINTER(i64), C.POINTER(ci), C.POINTER(u64), C.POINTER(ci), C.POINTER(C.c_uint32)],
        "afe_estimator_measure": [vp, C.POINTER(i64)],
        "afe_estimator_predict": [vp, C.c_double],
        "afe_estimator_get_prediction": [vp, i64, i64, vp],
        "afe_estimator_announce": [vp, i64, i64, vp, vp],
        "afe_estimator_get_state": [vp, i64, i64, vp, vp, vp, vp, vp, vp],
        "afe_estimator_reset": [vp, i64, i64],
        "afe_estimator_selftest_math": [ci, ci, i64, vp, vp],
        "afe_follower_attach_estimator": [vp, vp],
        "afe_gps_estimator_default_config": [C.POINTER(GpsEstimatorConfig)],
        "afe_gps_estimator_create": [eng, C.POINTER(GpsEstimatorConfig), C.POINTER(vp)],
        "afe_gps_estimator_destroy": [vp],
        "afe_gps_estimator_info": [vp, C.POINTER(i64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)],
        "afe_gps_estimator_imu": [vp],
        "afe_gps_estimator_measure": [vp, C.POINTER(i64)],
        "afe_gps_estimator_get_state": [vp, i64, i64, vp, vp, vp, vp, vp, vp],
        "afe_gps_estimator_set_state": [vp, i64, i64, vp, vp, vp],
        "afe_gps_estimator_reset": [vp, i64, i64],
        "afe_gps_estimator_selftest_math": [ci, ci, i64, vp, vp],
        "afe_follower_attach_gps_estimator": [vp, vp],
        "afe_stages_default_config": [ci, C.POINTER(StagesConfig)],
        "afe_stages_create": [eng, C.POINTER(StagesConfig), C.POINTER(vp)],
        "afe_stages_destroy": [vp],
        "afe_stages_info": [vp, C.POINTER(i64), C.POINTER(ci), C.POINTER(u64), C.POINTER(ci)],
        "afe_stages_set_desired_position": [vp, i64, i64, vp],
        "afe_stages_set_desired_yaw": [vp, i64, i64, vp],
        "afe_stages_set_centre": [vp, i64, i64, vp],
        "afe_stages_set_unsafe": [vp, i64, i64],
        "afe_stages_request": [vp, i64, i64, ci, ci],
        "afe_stages_set_warnings": [vp, i64, i64, vp],
        "afe_stages_tick": [vp, ci, ci, vp],
        "afe_stages_get": [vp, i64, i64, C.POINTER(StagesFields)],
        "afe_stages_attach_gps_estimator": [vp, vp],
        "afe_stages_selftest_math": [ci, ci, i64, vp, vp],
        "afe_onboard_default_config": [ci, C.POINTER(OnboardConfig)],
        "afe_onboard_create": [eng, C.POINTER(OnboardConfig), ci, C.POINTER(vp)],
        "afe_onboard_destroy": [vp],
        "afe_onboard_info": [vp, C.POINTER(i64), C.POINTER(u64), C.POINTER(u64)],
        "afe_onboard_set_battery": [vp, i64, i64, vp],
        "afe_onboard_radio": [vp, i64, i64, vp],
        "afe_onboard_tick": [vp, vp],
        "afe_onboard_get": [vp, i64, i64, C.POINTER(OnboardFields)],
        "afe_onboard_set_state": [vp, i64, i64, C.POINTER(OnboardState)],
        "afe_onboard_telemetry": [vp, i64, i64, vp],
        "afe_onboard_selftest_math": [ci, ci, i64, vp, vp],
    }
    for name, args in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = ci
    L.afe_scene_destroy.argtypes = [vp]
    L.afe_scene_destroy.restype = None
    L.afe_uwb_destroy.argtypes = [vp]
    L.afe_uwb_destroy.restype = None
    for name in ("afe_comm_last_error", "afe_group_last_error"):
        getattr(L, name).argtypes = [vp]
        getattr(L, name).restype = C.c_char_p
    L.afe_last_error.argtypes = [eng]
    L.afe_last_error.restype = C.c_char_p
    L.afe_status_string.argtypes = [ci]
    L.afe_status_string.restype = C.c_char_p
    _lib = L
    return L


def params_from_type(quadcopter_type):
    p = VehicleParams()
    rc = library().afe_params_from_type(int(quadcopter_type), C.byref(p))
    if rc:
        raise AfeError(rc, "invalid quadcopter type %r" % (quadcopter_type,))
    return p


def rates_logic_params_from_type(quadcopter_type):
    p = RatesLogicParams()
    rc = library().afe_rates_logic_params_from_type(int(quadcopter_type), C.byref(p))
    if rc:
        raise AfeError(rc, "invalid quadcopter type %r" % (quadcopter_type,))
    return p


def low_battery_threshold_from_type(quadcopter_type):
    """QuadcopterConstants(type).lowBatteryThreshold [V] as a numpy float32; types 0..5"""
    v = C.c_float()
    rc = library().afe_low_battery_threshold_from_type(int(quadcopter_type), C.byref(v))
    if rc:
        raise AfeError(rc, "invalid quadcopter type %r" % (quadcopter_type,))
    return np.float32(v.value)


def radio_create_rates_command(flags, thrust, ang_vel):
    raw = np.zeros(RADIO_PACKET_SIZE, np.uint8)
    w = np.ascontiguousarray(ang_vel, dtype=np.float32)
    rc = library().afe_radio_create_rates_command(int(flags), float(thrust), w.ctypes.data, raw.ctypes.data)
    if rc:
        raise AfeError(rc, "afe_radio_create_rates_command")
    return raw


def radio_create_acceleration_command(flags, acc, yaw_rate):
    raw = np.zeros(RADIO_PACKET_SIZE, np.uint8)
    a = np.ascontiguousarray(acc, dtype=np.float32)
    rc = library().afe_radio_create_acceleration_command(int(flags), a.ctypes.data, float(yaw_rate), raw.ctypes.data)
    if rc:
        raise AfeError(rc, "afe_radio_create_acceleration_command")
    return raw


def radio_create_simple_command(msg_type, flags=0):
    """kill (2) or idle (6)"""
    raw = np.zeros(RADIO_PACKET_SIZE, np.uint8)
    rc = library().afe_radio_create_simple_command(int(msg_type), int(flags), raw.ctypes.data)
    if rc:
        raise AfeError(rc, "afe_radio_create_simple_command")
    return raw


def radio_decode(raw):
    r = np.ascontiguousarray(raw, dtype=np.uint8)
    m = RadioMessage()
    rc = library().afe_radio_decode(r.ctypes.data, C.byref(m))
    if rc:
        raise AfeError(rc, "afe_radio_decode")
    return m


def planner_default_config(width, height, depth_scale, focal_length, true_radius, planning_radius,
                           min_checking_dist):
    c = PlannerConfig()
    rc = library().afe_planner_default_config(C.byref(c), width, height, depth_scale, focal_length, true_radius,
                                              planning_radius, min_checking_dist)
    if rc:
        raise AfeError(rc, "afe_planner_default_config")
    return c


def planner_samples(seed, width, height, n_candidates):
    s = np.empty((n_candidates, 4))
    rc = library().afe_planner_samples(int(seed), width, height, n_candidates, s.ctypes.data)
    if rc:
        raise AfeError(rc, "afe_planner_samples")
    return s


def planner_release_scratch():
    """afe_planner_release_scratch: give back the device scratch the planner keeps between calls"""
    library().afe_planner_release_scratch()


def rappids_plan(cfg, depth_images, vel0, acc0, grav, samples, image_index=None, cost_vec=None,
                 sample_table=None, want_flags=False, device=-1):
    """Batched RAPPIDS plan.  depth_images uint16 [n_images, H, W] (or a DeviceBuffer holding them,
    e.g. filled by Scene.render_engine); vel0/acc0/grav [3, n];
    samples [n_tables, M, 4] (or [M, 4]).  Returns (PlanOutput array, flags or None, kernel_ms)."""
    on_device = isinstance(depth_images, DeviceBuffer)
    if not on_device:
        img = np.ascontiguousarray(depth_images, dtype=np.uint16)
        if img.ndim == 2:
            img = img[None]
    v = np.ascontiguousarray(vel0, dtype=np.float64)
    n = v.shape[1]
    a = np.ascontiguousarray(acc0, dtype=np.float64)
    g = np.ascontiguousarray(grav, dtype=np.float64)
    s = np.ascontiguousarray(samples, dtype=np.float64)
    if s.ndim == 2:
        s = s[None]
    assert v.shape == a.shape == g.shape == (3, n) and s.shape[2] == 4
    if on_device:
        n_images = depth_images.nbytes // (2 * cfg.height * cfg.width)
        img_ptr, fn = depth_images.ptr, library().afe_rappids_plan_device
    else:
        assert img.shape[1:] == (cfg.height, cfg.width)
        n_images, img_ptr, fn = img.shape[0], img.ctypes.data, library().afe_rappids_plan
    idx = None if image_index is None else np.ascontiguousarray(image_index, dtype=np.int32)
    cv = None if cost_vec is None else np.ascontiguousarray(cost_vec, dtype=np.float64)
    st = None if sample_table is None else np.ascontiguousarray(sample_table, dtype=np.int32)
    out = (PlanOutput * n)()
    flags = np.zeros((n, s.shape[1]), np.uint8) if want_flags else None
    ms = C.c_float(0)
    rc = fn(int(device), C.byref(cfg), n, img_ptr, n_images,
            None if idx is None else idx.ctypes.data, v.ctypes.data, a.ctypes.data,
            g.ctypes.data, None if cv is None else cv.ctypes.data, s.ctypes.data, s.shape[0],
            None if st is None else st.ctypes.data, s.shape[1], out,
            None if flags is None else flags.ctypes.data, C.byref(ms))
    if rc:
        raise AfeError(rc, library().afe_status_string(rc).decode())
    return out, flags, ms.value


def camera_default(width, height):
    cam = Camera()
    rc = library().afe_camera_default(C.byref(cam), int(width), int(height))
    if rc:
        raise AfeError(rc, "afe_camera_default")
    return cam


def camera_default_mount():
    """depthCamAtt (main.cpp:123-125) as (w, x, y, z)."""
    q = np.empty(4)
    rc = library().afe_camera_default_mount(q.ctypes.data)
    if rc:
        raise AfeError(rc, "afe_camera_default_mount")
    return q


class DeviceBuffer:
    """A raw HBM allocation (afe_device_alloc) for chaining render -> plan on the device."""

    def __init__(self, nbytes, device=-1):
        self.ptr = C.c_void_p()
        self.nbytes = int(nbytes)
        rc = library().afe_device_alloc(int(device), self.nbytes, C.byref(self.ptr))
        if rc:
            raise AfeError(rc, library().afe_status_string(rc).decode())

    def download(self, dtype, shape, offset_bytes=0):
        out = np.empty(shape, dtype)
        assert offset_bytes >= 0 and offset_bytes + out.nbytes <= self.nbytes
        rc = library().afe_device_download(out.ctypes.data, C.c_void_p(self.ptr.value + int(offset_bytes)), out.nbytes)
        if rc:
            raise AfeError(rc, library().afe_status_string(rc).decode())
        return out

    def upload(self, array, offset_bytes=0):
        a = np.ascontiguousarray(array)
        assert offset_bytes >= 0 and offset_bytes + a.nbytes <= self.nbytes
        rc = library().afe_device_upload(C.c_void_p(self.ptr.value + int(offset_bytes)), a.ctypes.data, a.nbytes)
        if rc:
            raise AfeError(rc, library().afe_status_string(rc).decode())

    def close(self):
        if self.ptr:
            library().afe_device_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Scene:
    """afe_scene: a static triangle mesh (world frame, metres) + its BVH in HBM."""

    def __init__(self, triangles, device=-1):
        t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
        self._h = C.c_void_p()
        rc = library().afe_scene_create(int(device), t.ctypes.data, t.shape[0], C.byref(self._h))
        if rc:
            raise AfeError(rc, library().afe_status_string(rc).decode())

    def close(self):
        if self._h:
            library().afe_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        nt, nn, d = C.c_int64(), C.c_int64(), C.c_int()
        b = np.empty(6)
        rc = library().afe_scene_info(self._h, C.byref(nt), C.byref(nn), C.byref(d), b.ctypes.data)
        if rc:
            raise AfeError(rc, "afe_scene_info")
        return {"n_tri": nt.value, "n_nodes": nn.value, "depth": d.value, "bounds": b}

    def render(self, cam, pos, att, mount=None):
        """pos [3, n], att [4, n] -> (uint16 [n, H, W], kernel_ms)."""
        p = np.ascontiguousarray(pos, dtype=np.float64)
        q = np.ascontiguousarray(att, dtype=np.float64)
        n = p.shape[1]
        assert p.shape == (3, n) and q.shape == (4, n)
        m = None if mount is None else np.ascontiguousarray(mount, dtype=np.float64)
        out = np.empty((n, cam.height, cam.width), np.uint16)
        ms = C.c_float(0)
        rc = library().afe_render_depth(self._h, C.byref(cam), n, p.ctypes.data, q.ctypes.data,
                                        None if m is None else m.ctypes.data, out.ctypes.data, C.byref(ms))
        if rc:
            raise AfeError(rc, library().afe_status_string(rc).decode())
        return out, ms.value

    def set_walk(self, plain_only):
        """False (default): ordered walk of the octant-mirrored trees where a tile allows it; True: the plain
        walk everywhere.  Same images -- a cross-check."""
        rc = library().afe_scene_set_walk(self._h, 1 if plain_only else 0)
        if rc:
            raise AfeError(rc, library().afe_status_string(rc).decode())

    def render_stats(self, cam, pos, att, mount=None):
        """traversal counters of one batch (counting build): dict + kernel_ms"""
        p = np.ascontiguousarray(pos, dtype=np.float64)
        q = np.ascontiguousarray(att, dtype=np.float64)
        n = p.shape[1]
        m = None if mount is None else np.ascontiguousarray(mount, dtype=np.float64)
        st = np.zeros(8, np.uint64)
        ms = C.c_float(0)
        rc = library().afe_render_depth_stats(self._h, C.byref(cam), n, p.ctypes.data, q.ctypes.data,
                                              None if m is None else m.ctypes.data, st.ctypes.data, C.byref(ms))
        if rc:
            raise AfeError(rc, library().afe_status_string(rc).decode())
        keys = ("nodes_per_wave", "tri_box_tests_per_wave", "tri_fp64_tests_per_wave", "tri_box_tests_per_ray",
                "tri_fp64_tests_per_ray", "rays", "waves", "visible_triangles_per_wave")
        return dict(zip(keys, (int(x) for x in st[:8]))), ms.value

    def render_engine(self, ensemble, cam, mount=None, first=0, count=None, out=None):
        """Depth images of vehicles [first, first+count) from the engine's device state.
        out: a DeviceBuffer to keep the images in HBM (returns kernel_ms only), or None to
        get (uint16 [count, H, W], kernel_ms) on the host."""
        count = ensemble.n - first if count is None else count
        m = None if mount is None else np.ascontiguousarray(mount, dtype=np.float64)
        ms = C.c_float(0)
        if out is None:
            img = np.empty((count, cam.height, cam.width), np.uint16)
            dst, is_dev = img.ctypes.data, 0
        else:
            assert out.nbytes >= count * cam.height * cam.width * 2
            img, dst, is_dev = None, out.ptr, 1
        rc = library().afe_render_depth_engine(ensemble.handle, self._h, C.byref(cam), first, count,
                                               None if m is None else m.ctypes.data, dst, is_dev, C.byref(ms))
        if rc:
            raise AfeError(rc, library().afe_status_string(rc).decode())
        return (img, ms.value) if out is None else ms.value


def scene_check_hierarchy(triangles):
    """Host-only: (n_nodes, depth, max_leaf) of the BVH for a mesh, after verifying its invariants."""
    t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
    nn, d, ml = C.c_int64(), C.c_int(), C.c_int()
    rc = library().afe_scene_check_hierarchy(t.ctypes.data, t.shape[0], C.byref(nn), C.byref(d), C.byref(ml))
    if rc:
        raise AfeError(rc, library().afe_status_string(rc).decode())
    return nn.value, d.value, ml.value


def _status(rc):
    if rc:
        raise AfeError(rc, library().afe_status_string(rc).decode())


class PathClearance(C.Structure):
    """afe_path_clearance: what one sampled path did against the mesh (8-byte members only, 96 bytes)."""
    _fields_ = [("min_dist2", C.c_double), ("closest", C.c_double * 3), ("t_min", C.c_double), ("t_first_hit", C.c_double),
                ("k_min", C.c_int64), ("tri_min", C.c_int64), ("k_first_hit", C.c_int64), ("tri_first_hit", C.c_int64),
                ("n_hit", C.c_int64), ("n_nonfinite", C.c_int64)]


PATH_CLEARANCE_DTYPE = np.dtype([("min_dist2", np.float64), ("closest", np.float64, (3,)), ("t_min", np.float64),
                                 ("t_first_hit", np.float64), ("k_min", np.int64), ("tri_min", np.int64),
                                 ("k_first_hit", np.int64), ("tri_first_hit", np.int64), ("n_hit", np.int64),
                                 ("n_nonfinite", np.int64)])


# afe_segment_clearance: one segment against the mesh (48 bytes); afe_path_sweep: afe_path_clearance over chords (112 bytes)
SEGMENT_CLEARANCE_DTYPE = np.dtype([("dist2", np.float64), ("s", np.float64), ("closest", np.float64, (3,)), ("tri", np.int32), ("kind", np.int32)])
PATH_SWEEP_DTYPE = np.dtype(PATH_CLEARANCE_DTYPE.descr + [("s_min", np.float64), ("s_first_hit", np.float64)])


def path_chord_deviation(coeffs, t_begin, t_end, rot=None, n_samples=64):
    """Host-only: an upper bound [m] on how far the quintic (coeffs [6, 3]) leaves the polyline of its n_samples sample points
    (crude: h^2/8 max|p''| by triangle inequalities; see the header)."""
    c = np.ascontiguousarray(coeffs, dtype=np.float64)
    assert c.shape == (6, 3)
    r = None if rot is None else np.ascontiguousarray(np.asarray(rot, np.float64).reshape(-1))
    assert r is None or r.shape == (9,)
    out = C.c_double(0)
    _status(library().afe_path_chord_deviation(c.ctypes.data, float(t_begin), float(t_end), None if r is None else r.ctypes.data,
                                               int(n_samples), C.byref(out)))
    return out.value


def _opt_f64(a, shape):
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.shape == shape, (a.shape, shape)
    return a, a.ctypes.data


def path_sample_points(coeffs, t_begin, t_end, origin=None, rot=None, n_samples=64):
    """Host-only: the sample times [K] and world points [3, K] of one path (coeffs [6, 3], t^5 .. t^0 per axis; origin [3]
    and row-major rot [9] or [3, 3] optional) by the definition's expressions (csrc/afe_clearance.hip)."""
    c = np.ascontiguousarray(coeffs, dtype=np.float64)
    assert c.shape == (6, 3)
    o, o_ptr = _opt_f64(origin, (3,))
    r, r_ptr = _opt_f64(None if rot is None else np.asarray(rot, np.float64).reshape(-1), (9,))
    k = max(int(n_samples), 0)
    t, xyz = np.empty(k), np.empty((3, k))
    _status(library().afe_path_sample_points(c.ctypes.data, float(t_begin), float(t_end), o_ptr, r_ptr, int(n_samples),
                                             t.ctypes.data, xyz.ctypes.data))
    return t, xyz


class ClearanceMap:
    """afe_clearance_map: a static triangle mesh (world frame, metres) + its own hierarchy in HBM, answering
    "how far is this point from the mesh" (squared distances; see the header)."""

    def __init__(self, triangles, device=-1):
        t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
        self._h = C.c_void_p()
        _status(library().afe_clearance_map_create(int(device), t.ctypes.data, t.shape[0], C.byref(self._h)))

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            library().afe_clearance_map_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        nt, nn, d = C.c_int64(), C.c_int64(), C.c_int()
        b = np.empty(6)
        _status(library().afe_clearance_map_info(self._h, C.byref(nt), C.byref(nn), C.byref(d), b.ctypes.data))
        return {"n_tri": nt.value, "n_nodes": nn.value, "depth": d.value, "bounds": b}

    def query(self, pos, max_dist=np.inf, want_closest=True):
        """pos [3, n] -> (dist2 [n], tri [n] int32, closest [3, n] or None, kernel_ms)."""
        p = np.ascontiguousarray(pos, dtype=np.float64)
        n = p.shape[1]
        assert p.shape == (3, n)
        d2, tri = np.empty(n), np.empty(n, np.int32)
        cl = np.empty((3, n)) if want_closest else None
        ms = C.c_float(0)
        _status(library().afe_clearance_query(self._h, n, p.ctypes.data, float(max_dist), d2.ctypes.data, tri.ctypes.data,
                                              None if cl is None else cl.ctypes.data, C.byref(ms)))
        return d2, tri, cl, ms.value

    def query_stats(self, pos, max_dist=np.inf):
        """traversal counters of one batch (counting build), summed over the points: dict + kernel_ms"""
        p = np.ascontiguousarray(pos, dtype=np.float64)
        st = np.zeros(4, np.uint64)
        ms = C.c_float(0)
        _status(library().afe_clearance_query_stats(self._h, p.shape[1], p.ctypes.data, float(max_dist), st.ctypes.data, C.byref(ms)))
        return dict(zip(("nodes", "tri_box_tests", "tri_fp64_evals", "points"), (int(x) for x in st))), ms.value

    def _segment_arrays(self, p0, p1):
        a, b = np.ascontiguousarray(p0, dtype=np.float64), np.ascontiguousarray(p1, dtype=np.float64)
        n = a.shape[1]
        assert a.shape == b.shape == (3, n)
        return n, a, b

    def segments(self, p0, p1, max_dist=np.inf):
        """n segments p0 -> p1 ([3, n] each) -> (records: SEGMENT_CLEARANCE_DTYPE [n], kernel_ms): the exact squared distance
        between each segment and the mesh (see the header, swept clearance)."""
        n, a, b = self._segment_arrays(p0, p1)
        out = np.empty(n, SEGMENT_CLEARANCE_DTYPE)
        ms = C.c_float(0)
        _status(library().afe_clearance_segments(self._h, n, a.ctypes.data, b.ctypes.data, float(max_dist), out.ctypes.data, C.byref(ms)))
        return out, ms.value

    def segments_stats(self, p0, p1, max_dist=np.inf):
        """traversal counters of such a batch (counting build), summed over the segments: dict + kernel_ms"""
        n, a, b = self._segment_arrays(p0, p1)
        st = np.zeros(4, np.uint64)
        ms = C.c_float(0)
        _status(library().afe_clearance_segments_stats(self._h, n, a.ctypes.data, b.ctypes.data, float(max_dist), st.ctypes.data, C.byref(ms)))
        return dict(zip(("nodes", "tri_box_tests", "tri_fp64_evals", "segments"), (int(x) for x in st))), ms.value

    def _ray_arrays(self, origin, dir, t_max):
        n, o, d = self._segment_arrays(origin, dir)
        tm = None if t_max is None else np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, dtype=np.float64), (n,)))
        return n, o, d, tm

    def raycast(self, origin, dir, t_max=None, want_ms=False):
        """n rays ([3, n] origins and directions, neither normalised; t_max None, a scalar or [n]) -> (t [n], tri [n] int32):
        the first triangle each ray hits and its ray parameter (metres for unit directions); no hit: (+inf, -1).
        See the header, range beams.  want_ms: (t, tri, kernel_ms)."""
        n, o, d, tm = self._ray_arrays(origin, dir, t_max)
        t, tri = np.empty(n), np.empty(n, np.int32)
        ms = C.c_float(0)
        _status(library().afe_raycast(self._h, n, o.ctypes.data, d.ctypes.data, None if tm is None else tm.ctypes.data, t.ctypes.data,
                                      tri.ctypes.data, C.byref(ms)))
        return (t, tri, ms.value) if want_ms else (t, tri)

    def raycast_stats(self, origin, dir, t_max=None, want_answers=False):
        """traversal counters of such a batch (counting build), summed over the rays: dict + kernel_ms; want_answers: and
        the counting build's own (t, tri)"""
        n, o, d, tm = self._ray_arrays(origin, dir, t_max)
        st = np.zeros(4, np.uint64)
        t, tri = np.empty(n), np.empty(n, np.int32)
        ms = C.c_float(0)
        _status(library().afe_raycast_stats(self._h, n, o.ctypes.data, d.ctypes.data, None if tm is None else tm.ctypes.data,
                                            t.ctypes.data if want_answers else None, tri.ctypes.data if want_answers else None,
                                            st.ctypes.data, C.byref(ms)))
        counts = dict(zip(("nodes", "tri_box_tests", "tri_fp64_tests", "rays"), (int(x) for x in st)))
        return (counts, ms.value, t, tri) if want_answers else (counts, ms.value)

    def line_of_sight(self, p0, p1, want_ms=False):
        """n pairs ([3, n] each) -> blocked [n] uint8: 1 where a triangle lies between p0 and p1 (a hit with 0 < t <= 1 of
        the ray p0 + t (p1 - p0)), else 0.  want_ms: (blocked, kernel_ms)."""
        n, a, b = self._segment_arrays(p0, p1)
        out = np.empty(n, np.uint8)
        ms = C.c_float(0)
        _status(library().afe_line_of_sight(self._h, n, a.ctypes.data, b.ctypes.data, out.ctypes.data, C.byref(ms)))
        return (out, ms.value) if want_ms else out

    def query_engine(self, ensemble, max_dist, first=0, count=None, out=None):
        """The same for vehicles [first, first+count) from the engine's device state.  out: None to get
        (dist2, tri, closest, kernel_ms) on the host, or a (dist2, tri, closest) tuple of DeviceBuffers (closest may
        be None) to keep the answers in HBM (returns kernel_ms only)."""
        count = ensemble.n - first if count is None else count
        ms = C.c_float(0)
        if out is None:
            d2, tri, cl = np.empty(max(count, 0)), np.empty(max(count, 0), np.int32), np.empty((3, max(count, 0)))
            args, is_dev = (d2.ctypes.data, tri.ctypes.data, cl.ctypes.data), 0
        else:
            b_d2, b_tri, b_cl = out
            assert b_d2.nbytes >= count * 8 and b_tri.nbytes >= count * 4 and (b_cl is None or b_cl.nbytes >= count * 24)
            args, is_dev = (b_d2.ptr, b_tri.ptr, None if b_cl is None else b_cl.ptr), 1
        _status(library().afe_clearance_query_engine(ensemble.handle, self._h, int(first), int(count), float(max_dist),
                                                     args[0], args[1], args[2], is_dev, C.byref(ms)))
        return (d2, tri, cl, ms.value) if out is None else ms.value

    @staticmethod
    def _path_arrays(coeffs, t_range, origin, rot):
        c = np.ascontiguousarray(coeffs, dtype=np.float64)
        n = c.shape[0]
        assert c.shape == (n, 6, 3)
        tr = np.ascontiguousarray(t_range, dtype=np.float64)
        assert tr.shape == (2, n)
        o, o_ptr = _opt_f64(origin, (3, n))
        r, r_ptr = _opt_f64(rot, (9, n))
        return n, (c, tr, o, r), (c.ctypes.data, tr.ctypes.data, o_ptr, r_ptr)      # (the arrays: alive while the pointers are used)

    def paths(self, coeffs, t_range, origin=None, rot=None, n_samples=64, radius=0.116, max_dist=np.inf):
        """n explicit paths sampled at n_samples times each: coeffs [n, 6, 3] (t^5 .. t^0 per axis), t_range [2, n], origin
        [3, n] or None, rot [9, n] (row-major, planar) or None -> (records: PATH_CLEARANCE_DTYPE [n], n_colliding, kernel_ms).
        radius defaults to the reference vehicle's 0.116 m."""
        n, _arrays, ptrs = self._path_arrays(coeffs, t_range, origin, rot)
        out = np.empty(n, PATH_CLEARANCE_DTYPE)
        nc, ms = C.c_int64(0), C.c_float(0)
        _status(library().afe_clearance_paths(self._h, n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], int(n_samples), float(radius), float(max_dist),
                                              out.ctypes.data, C.byref(nc), C.byref(ms)))
        return out, nc.value, ms.value

    def paths_stats(self, coeffs, t_range, origin=None, rot=None, n_samples=64, radius=0.116, max_dist=np.inf):
        """traversal counters of such a batch (counting build), summed over the samples: dict + kernel_ms"""
        n, _arrays, ptrs = self._path_arrays(coeffs, t_range, origin, rot)
        st = np.zeros(4, np.uint64)
        ms = C.c_float(0)
        _status(library().afe_clearance_paths_stats(self._h, n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], int(n_samples), float(radius),
                                                    float(max_dist), st.ctypes.data, C.byref(ms)))
        return dict(zip(("nodes", "tri_box_tests", "tri_fp64_evals", "samples"), (int(x) for x in st))), ms.value

    def paths_swept(self, coeffs, t_range, origin=None, rot=None, n_samples=64, radius=0.116, max_dist=np.inf):
        """paths() over the n_samples - 1 chords between the sample points -> (records: PATH_SWEEP_DTYPE [n], n_colliding, kernel_ms)"""
        n, _arrays, ptrs = self._path_arrays(coeffs, t_range, origin, rot)
        out = np.empty(n, PATH_SWEEP_DTYPE)
        nc, ms = C.c_int64(0), C.c_float(0)
        _status(library().afe_clearance_paths_swept(self._h, n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], int(n_samples), float(radius),
                                                    float(max_dist), out.ctypes.data, C.byref(nc), C.byref(ms)))
        return out, nc.value, ms.value

    def paths_swept_stats(self, coeffs, t_range, origin=None, rot=None, n_samples=64, radius=0.116, max_dist=np.inf):
        """traversal counters of such a batch (counting build), summed over the chords: dict + kernel_ms"""
        n, _arrays, ptrs = self._path_arrays(coeffs, t_range, origin, rot)
        st = np.zeros(4, np.uint64)
        ms = C.c_float(0)
        _status(library().afe_clearance_paths_swept_stats(self._h, n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], int(n_samples), float(radius),
                                                          float(max_dist), st.ctypes.data, C.byref(ms)))
        return dict(zip(("nodes", "tri_box_tests", "tri_fp64_evals", "chords"), (int(x) for x in st))), ms.value

    def plans_engine_swept(self, ensemble, plans, mount=None, first=0, count=None, n_samples=64, radius=0.116, max_dist=np.inf):
        """plans_engine() over chords -> (records: PATH_SWEEP_DTYPE [count], n_colliding, kernel_ms)"""
        return self._plans_engine(library().afe_clearance_plans_engine_swept, PATH_SWEEP_DTYPE, ensemble, plans, mount, first, count,
                                  n_samples, radius, max_dist)

    def plans_engine(self, ensemble, plans, mount=None, first=0, count=None, n_samples=64, radius=0.116, max_dist=np.inf):
        """The plans of vehicles [first, first+count) as rappids_plan returned them (a PlanOutput array or a PLAN_DTYPE
        array, plans[i] for vehicle first + i), placed by each vehicle's pose on the device ->
        (records: PATH_CLEARANCE_DTYPE [count], n_colliding, kernel_ms)."""
        return self._plans_engine(library().afe_clearance_plans_engine, PATH_CLEARANCE_DTYPE, ensemble, plans, mount, first, count,
                                  n_samples, radius, max_dist)

    def _plans_engine(self, entry, dtype, ensemble, plans, mount, first, count, n_samples, radius, max_dist):
        """plans_engine and plans_engine_swept: the C entry and the dtype of its records"""
        count = ensemble.n - first if count is None else count
        if isinstance(plans, np.ndarray):
            assert plans.dtype == PLAN_DTYPE
            p = np.ascontiguousarray(plans)
            assert p.size >= count
            p_ptr = p.ctypes.data
        else:
            assert len(plans) >= count
            p, p_ptr = plans, C.cast(plans, C.c_void_p)
        m = None if mount is None else np.ascontiguousarray(mount, dtype=np.float64)
        out = np.empty(max(count, 0), dtype)
        nc, ms = C.c_int64(0), C.c_float(0)
        _status(entry(ensemble.handle, self._h, int(first), int(count), None if m is None else m.ctypes.data,
                      p_ptr, int(n_samples), float(radius), float(max_dist), out.ctypes.data, C.byref(nc), C.byref(ms)))
        return out, nc.value, ms.value


# afe_image_truth: what one sampled path did against the depth image (8-byte members only, 64 bytes)
IMAGE_TRUTH_DTYPE = np.dtype([("verdict", np.int64), ("k_fov", np.int64), ("t_fov", np.float64), ("k_hit", np.int64),
                              ("t_hit", np.float64), ("pixel_hit", np.int64), ("n_samples", np.int64), ("n_checked", np.int64)])
# afe_conservativeness: MeasureConservativeness' tally
CONSERVATIVENESS_DTYPE = np.dtype([(k, np.int64) for k in ("n_checked", "n_planner_free", "n_correct_in_collision",
                                                           "n_incorrect_in_collision", "n_free_but_out_of_view", "n_free_but_occluded")])


def image_truth_sample_times(t_begin, t_end, timestep=0.1):
    """Host-only: the ground truth's sample times over [t_begin, t_end), the running sum t_{k+1} = t_k + timestep."""
    k = C.c_int(0)
    _status(library().afe_image_truth_sample_times(float(t_begin), float(t_end), float(timestep), C.byref(k), None))
    t = np.empty(k.value)
    _status(library().afe_image_truth_sample_times(float(t_begin), float(t_end), float(timestep), C.byref(k), t.ctypes.data))
    return t


def _truth_images(cfg, depth_images, image_index, n_owners):
    """(keep-alive, pointer, n_images, on_device, index keep-alive, index pointer) of the image arguments"""
    if isinstance(depth_images, DeviceBuffer):
        img, ptr, n_images, on_device = depth_images, depth_images.ptr, depth_images.nbytes // (2 * cfg.height * cfg.width), 1
    else:
        img = np.ascontiguousarray(depth_images, dtype=np.uint16)
        if img.ndim == 2:
            img = img[None]
        assert img.shape[1:] == (cfg.height, cfg.width), (img.shape, cfg.height, cfg.width)
        ptr, n_images, on_device = img.ctypes.data, img.shape[0], 0
    idx = None if image_index is None else np.ascontiguousarray(image_index, dtype=np.int32)
    assert idx is None or idx.shape == (n_owners,)
    return img, ptr, n_images, on_device, idx, None if idx is None else idx.ctypes.data


def image_truth_paths(cfg, depth_images, coeffs, t_range, image_index=None, timestep=0.1, device=-1, want_stats=False):
    """The reference's IsCollisionFreeGroundTruth for n explicit camera-frame paths: depth_images uint16 [n_images, H, W] or a
    DeviceBuffer holding them, coeffs [n, 6, 3] (t^5 .. t^0 per axis), t_range [2, n] = [t_begin, t_end) ->
    (records: IMAGE_TRUTH_DTYPE [n], n_free, kernel_ms); verdict 0 free, 1 out of view, 2 occluded.
    want_stats: the scan's counters instead (counting build): (dict, kernel_ms)."""
    c = np.ascontiguousarray(coeffs, dtype=np.float64)
    n = c.shape[0]
    assert c.shape == (n, 6, 3)
    tr = np.ascontiguousarray(t_range, dtype=np.float64)
    assert tr.shape == (2, n)
    _img, ptr, n_images, on_device, _idx, idx_ptr = _truth_images(cfg, depth_images, image_index, n)
    ms = C.c_float(0)
    if want_stats:
        st = np.zeros(4, np.uint64)
        _status(library().afe_image_truth_paths_stats(int(device), C.byref(cfg), n, ptr, n_images, on_device, idx_ptr, c.ctypes.data,
                                                      tr.ctypes.data, float(timestep), st.ctypes.data, C.byref(ms)))
        return dict(zip(("samples", "pixels_tested", "pixels_meeting_sphere", "pixels_brute_force"), (int(x) for x in st))), ms.value
    out = np.empty(n, IMAGE_TRUTH_DTYPE)
    nf = C.c_int64(0)
    _status(library().afe_image_truth_paths(int(device), C.byref(cfg), n, ptr, n_images, on_device, idx_ptr, c.ctypes.data, tr.ctypes.data,
                                            float(timestep), out.ctypes.data, C.byref(nf), C.byref(ms)))
    return out, nf.value, ms.value


def image_truth_plans(cfg, depth_images, plans, image_index=None, timestep=0.1, device=-1):
    """The same for the plans rappids_plan returned (a PlanOutput array or a PLAN_DTYPE array), each over [0, tf); a plan with
    found == 0 gets the empty record (verdict -1) -> (records: IMAGE_TRUTH_DTYPE [n], n_free, kernel_ms)."""
    if isinstance(plans, np.ndarray):
        assert plans.dtype == PLAN_DTYPE
        p = np.ascontiguousarray(plans)
        n, p_ptr = p.size, p.ctypes.data
    else:
        p, n, p_ptr = plans, len(plans), C.cast(plans, C.c_void_p)
    _img, ptr, n_images, on_device, _idx, idx_ptr = _truth_images(cfg, depth_images, image_index, n)
    out = np.empty(n, IMAGE_TRUTH_DTYPE)
    nf, ms = C.c_int64(0), C.c_float(0)
    _status(library().afe_image_truth_plans(int(device), C.byref(cfg), n, ptr, n_images, on_device, idx_ptr, p_ptr, float(timestep),
                                            out.ctypes.data, C.byref(nf), C.byref(ms)))
    return out, nf.value, ms.value


def image_truth_candidates(cfg, depth_images, vel0, acc0, samples, flags, image_index=None, sample_table=None, timestep=0.1,
                           want_coeffs=False, want_per_planner=False, device=-1):
    """The reference's MeasureConservativeness for n planners x M candidates: the arguments of rappids_plan and the flags [n, M]
    it returned -> (verdicts uint8 [n, M], coeffs [n, M, 6, 3] or None, tally: CONSERVATIVENESS_DTYPE scalar,
    per_planner: CONSERVATIVENESS_DTYPE [n] or None, kernel_ms).  Every candidate gets a verdict; only those the planner
    collision-checked (flag bit 4) are tallied."""
    v = np.ascontiguousarray(vel0, dtype=np.float64)
    n = v.shape[1]
    a = np.ascontiguousarray(acc0, dtype=np.float64)
    s = np.ascontiguousarray(samples, dtype=np.float64)
    if s.ndim == 2:
        s = s[None]
    m = s.shape[1]
    fl = np.ascontiguousarray(flags, dtype=np.uint8)
    assert v.shape == a.shape == (3, n) and s.shape[2] == 4 and fl.shape == (n, m)
    _img, ptr, n_images, on_device, _idx, idx_ptr = _truth_images(cfg, depth_images, image_index, n)
    st = None if sample_table is None else np.ascontiguousarray(sample_table, dtype=np.int32)
    verdict = np.empty((n, m), np.uint8)
    co = np.empty((n, m, 6, 3)) if want_coeffs else None
    tally = np.zeros(1, CONSERVATIVENESS_DTYPE)
    per = np.zeros(n, CONSERVATIVENESS_DTYPE) if want_per_planner else None
    ms = C.c_float(0)
    _status(library().afe_image_truth_candidates(int(device), C.byref(cfg), n, ptr, n_images, on_device, idx_ptr, v.ctypes.data, a.ctypes.data,
                                                 s.ctypes.data, s.shape[0], None if st is None else st.ctypes.data, m, fl.ctypes.data,
                                                 float(timestep), verdict.ctypes.data, None if co is None else co.ctypes.data,
                                                 tally.ctypes.data, None if per is None else per.ctypes.data, C.byref(ms)))
    return verdict, co, tally[0], per, ms.value


def clearance_check_hierarchy(triangles):
    """Host-only: (n_nodes, depth, max_leaf) of the clearance hierarchy for a mesh, after verifying its invariants."""
    t = np.ascontiguousarray(triangles, dtype=np.float32).reshape(-1, 9)
    nn, d, ml = C.c_int64(), C.c_int(), C.c_int()
    _status(library().afe_clearance_check_hierarchy(t.ctypes.data, t.shape[0], C.byref(nn), C.byref(d), C.byref(ml)))
    return nn.value, d.value, ml.value


class ContactMonitor:
    """afe_contact_monitor: per-vehicle closest approach and first contact, latched on the device.  Borrows the
    ensemble and the map: close it before either of them.  swept=True: every update measures the segment from the vehicle's
    position at its last update to the current one (afe_contact_monitor_create_swept); reset() the vehicles you move with
    set_state."""

    NEVER = np.uint64(0xffffffffffffffff)

    def __init__(self, ensemble, cmap, contact_radius, search_radius, swept=False):
        self._h = C.c_void_p()
        self.n = ensemble.n
        self.swept = bool(swept)
        self._keep = (ensemble, cmap)
        create = library().afe_contact_monitor_create_swept if swept else library().afe_contact_monitor_create
        _status(create(ensemble.handle, cmap.handle, float(contact_radius), float(search_radius), C.byref(self._h)))

    def update(self):
        """-> (vehicles in contact now, vehicles ever in contact)"""
        now, ever = C.c_int64(), C.c_int64()
        _status(library().afe_contact_monitor_update(self._h, C.byref(now), C.byref(ever)))
        return now.value, ever.value

    def get(self, first=0, count=None):
        """-> dict(min_dist2 [count], first_contact_us [count] uint64 (NEVER: none), first_contact_tri [count] int32 (-1))"""
        count = self.n - first if count is None else count
        out = dict(min_dist2=np.empty(count), first_contact_us=np.empty(count, np.uint64), first_contact_tri=np.empty(count, np.int32))
        _status(library().afe_contact_monitor_get(self._h, int(first), int(count), out["min_dist2"].ctypes.data,
                                                  out["first_contact_us"].ctypes.data, out["first_contact_tri"].ctypes.data))
        return out

    def reset(self, first=0, count=None):
        count = self.n - first if count is None else count
        _status(library().afe_contact_monitor_reset(self._h, int(first), int(count)))

    def close(self):
        if getattr(self, "_h", None):
            library().afe_contact_monitor_destroy(self._h)
            self._h = C.c_void_p()
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# afe_range_beam: one beam of a range sensor (64 bytes)
RANGE_BEAM_DTYPE = np.dtype([("off", np.float64, 3), ("dir", np.float64, 3), ("t_max", np.float64), ("frame", np.int32), ("reserved", np.int32)])
RANGE_FRAME_SENSOR, RANGE_FRAME_WORLD = 0, 1


def range_beam(dir, off=(0.0, 0.0, 0.0), t_max=np.inf, frame=RANGE_FRAME_SENSOR):
    """One RANGE_BEAM_DTYPE record."""
    b = np.zeros((), RANGE_BEAM_DTYPE)
    b["off"], b["dir"], b["t_max"], b["frame"] = off, dir, t_max, frame
    return b


def crazyflie_range_beams(t_max=4.0):
    """The six beams of a Crazyflie's multi-ranger and z-ranger decks: +x, -x, +y, -y, +z, -z of the sensor frame from its
    origin, t_max metres each (the decks' VL53L1x reaches about 4 m) -> RANGE_BEAM_DTYPE [6]."""
    dirs = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
    return np.array([range_beam(np.array(d, np.float64), t_max=t_max) for d in dirs], RANGE_BEAM_DTYPE)


class RangeSensor:
    """afe_range_sensor: beams mounted on every vehicle of an ensemble, answered from the engine's device state against a
    ClearanceMap (see the header, range beams).  beams: RANGE_BEAM_DTYPE [1 .. 32]; mount: quaternion of the sensor frame
    in the body frame (None: identity).  Borrows the ensemble and the map: close it before either of them."""

    def __init__(self, ensemble, cmap, beams, mount=None):
        self._h = C.c_void_p()
        self.n = ensemble.n
        self._keep = (ensemble, cmap)
        b = np.ascontiguousarray(beams, dtype=RANGE_BEAM_DTYPE).reshape(-1)
        m = None if mount is None else np.ascontiguousarray(mount, dtype=np.float64)
        assert m is None or m.shape == (4,)
        self.n_beams = b.size
        _status(library().afe_range_sensor_create(ensemble.handle, cmap.handle, None if m is None else m.ctypes.data, b.ctypes.data,
                                                  b.size, C.byref(self._h)))

    def update(self, first=0, count=None, out=None, want_ms=True):
        """Vehicles [first, first+count) now.  out: None to get (t [n_beams, count], tri [n_beams, count] int32, kernel_ms) on
        the host, or a (t, tri) tuple of DeviceBuffers (tri may be None) to keep the readings in HBM (returns kernel_ms, or
        None without waiting if want_ms is false)."""
        count = self.n - first if count is None else count
        ms = C.c_float(0)
        ms_ptr = C.byref(ms) if want_ms else None
        if out is None:
            t, tri = np.empty((self.n_beams, max(count, 0))), np.empty((self.n_beams, max(count, 0)), np.int32)
            _status(library().afe_range_sensor_update(self._h, int(first), int(count), t.ctypes.data, tri.ctypes.data, 0, ms_ptr))
            return t, tri, ms.value
        b_t, b_tri = out
        assert b_t.nbytes >= self.n_beams * count * 8 and (b_tri is None or b_tri.nbytes >= self.n_beams * count * 4)
        _status(library().afe_range_sensor_update(self._h, int(first), int(count), b_t.ptr, None if b_tri is None else b_tri.ptr, 1, ms_ptr))
        return ms.value if want_ms else None

    def info(self):
        nb, nv = C.c_int(), C.c_int64()
        _status(library().afe_range_sensor_info(self._h, C.byref(nb), C.byref(nv)))
        return {"n_beams": nb.value, "n_vehicles": nv.value}

    def close(self):
        if getattr(self, "_h", None):
            library().afe_range_sensor_destroy(self._h)
            self._h = C.c_void_p()
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GroupStats(C.Structure):
    """afe_group_stats: one record per group of a StatsMonitor update (8-byte members only)."""
    _fields_ = ([(k, C.c_int64) for k in ("count", "n_invalid", "n_grounded", "n_ever_invalid", "n_ever_grounded", "sum_n_valid",
                                          "argmax_h2", "argmax_peak_h2")] +
                [(k, C.c_double) for k in ("sum_h2", "sum_dz", "sum_dz2", "sum_v2", "sum_w2", "max_h2", "min_dz", "max_dz", "max_v2",
                                           "max_w2", "min_up", "sum_peak_h2", "sum_acc_h2", "max_peak_h2", "min_min_up")])


GROUP_STATS_DTYPE = np.dtype([(k, np.int64 if t is C.c_int64 else np.float64) for k, t in GroupStats._fields_])


def stats_check_layout(edges, n_vehicles):
    """Host-only: (n_chunks, levels) of the statistics layout for group edges over n_vehicles, after validating them."""
    ed = np.ascontiguousarray(edges, dtype=np.int64)
    nc, lv = C.c_int64(), C.c_int()
    _status(library().afe_stats_check_layout(ed.ctypes.data, ed.size - 1, int(n_vehicles), C.byref(nc), C.byref(lv)))
    return nc.value, lv.value


class StatsMonitor:
    """afe_stats_monitor: per-group statistics of the ensemble's state and per-vehicle latches, computed and kept on
    the device (see the header).  Groups are [edges[g], edges[g+1]).  Borrows the ensemble: close it first."""

    NEVER = np.uint64(0xffffffffffffffff)

    def __init__(self, ensemble, edges):
        ed = np.ascontiguousarray(edges, dtype=np.int64)
        self._h = C.c_void_p()
        self.n = ensemble.n
        self.n_groups = ed.size - 1
        self.n_hist_edges = 0
        self._keep = ensemble
        _status(library().afe_stats_create(ensemble.handle, ed.ctypes.data, self.n_groups, C.byref(self._h)))

    def mark(self, first=0, count=None):
        """reference of vehicles [first, first+count) = where they are now (formed on the device)"""
        count = self.n - first if count is None else count
        _status(library().afe_stats_set_reference(self._h, int(first), int(count), None))

    def set_reference(self, pos3, first=0):
        """explicit reference points, planar [3, count], for vehicles [first, first+count)"""
        p = np.ascontiguousarray(pos3, dtype=np.float64)
        assert p.ndim == 2 and p.shape[0] == 3
        _status(library().afe_stats_set_reference(self._h, int(first), p.shape[1], p.ctypes.data))

    def set_histogram(self, edges_m=None):
        """ascending edges in metres for the histogram of the horizontal deviation; None or empty: off"""
        ed = np.ascontiguousarray([] if edges_m is None else edges_m, dtype=np.float64).ravel()
        _status(library().afe_stats_set_histogram(self._h, ed.ctypes.data if ed.size else None, ed.size))
        self.n_hist_edges = ed.size

    def update(self):
        """-> (records: structured array [n_groups] of GROUP_STATS_DTYPE, histogram int64 [n_groups, n_edges+1] or None)"""
        rec = np.empty(self.n_groups, GROUP_STATS_DTYPE)
        hist = np.empty((self.n_groups, self.n_hist_edges + 1), np.int64) if self.n_hist_edges else None
        _status(library().afe_stats_update(self._h, rec.ctypes.data, None if hist is None else hist.ctypes.data))
        return rec, hist

    def latches(self, first=0, count=None):
        """-> dict(peak_h2, min_up, acc_h2 [count] float64, n_valid [count] int64, first_grounded_us, first_invalid_us
        [count] uint64 (NEVER: none))"""
        count = self.n - first if count is None else count
        out = dict(peak_h2=np.empty(count), min_up=np.empty(count), acc_h2=np.empty(count), n_valid=np.empty(count, np.int64),
                   first_grounded_us=np.empty(count, np.uint64), first_invalid_us=np.empty(count, np.uint64))
        _status(library().afe_stats_get(self._h, int(first), int(count), *[a.ctypes.data for a in out.values()]))
        return out

    def reset(self, first=0, count=None):
        count = self.n - first if count is None else count
        _status(library().afe_stats_reset(self._h, int(first), int(count)))

    def info(self):
        ng, nv, ne, nu = C.c_int(), C.c_int64(), C.c_int(), C.c_uint64()
        _status(library().afe_stats_info(self._h, C.byref(ng), C.byref(nv), C.byref(ne), C.byref(nu)))
        return {"n_groups": ng.value, "n_vehicles": nv.value, "n_hist_edges": ne.value, "n_updates": nu.value}

    def close(self):
        if getattr(self, "_h", None):
            library().afe_stats_destroy(self._h)
            self._h = C.c_void_p()
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def follower_default_config(quadcopter_type):
    """afe_follower_default_config: the tracking controller's tuning for the type and the loop's constants.  Pure host."""
    c = FollowerConfig()
    _status(library().afe_follower_default_config(int(quadcopter_type), C.byref(c)))
    return c


def follower_ring_slots(period_us, delay_us):
    """afe_follower_ring_slots: slots of the delay ring.  Pure host."""
    k = C.c_int()
    _status(library().afe_follower_ring_slots(int(period_us), int(delay_us), C.byref(k)))
    return k.value


FOLLOWER_MATH_OPS = {"sinf": 0, "cosf": 1, "asinf": 2, "acosf": 3, "acos": 4}


def follower_selftest_math(op, x, device=-1):
    """afe_follower_selftest_math: the device library's sinf / cosf / asinf / acosf (float32) or acos (float64) of x, as
    the follower's kernels call them; op is a name or 0..4"""
    op = FOLLOWER_MATH_OPS.get(op, op)
    a = np.ascontiguousarray(x, dtype=np.float64 if op == 4 else np.float32)
    y = np.empty_like(a)
    _status(library().afe_follower_selftest_math(int(device), int(op), a.size, a.ctypes.data, y.ctypes.data))
    return y


class Follower:
    """afe_follower: plan adoption, tracking reference, tracking controller, radio codec and delay line for every vehicle
    of an ensemble, on the device (see the header).  Borrows the ensemble: close the follower first."""

    def __init__(self, ensemble, cfg=None, quadcopter_type=5):
        self.cfg = follower_default_config(quadcopter_type) if cfg is None else cfg
        self._h = C.c_void_p()
        self.n = ensemble.n
        self._keep = ensemble
        _status(library().afe_follower_create(ensemble.handle, C.byref(self.cfg), C.byref(self._h)))

    def _range(self, first, count):
        return int(first), int(self.n - first if count is None else count)

    def set_hold(self, pos3, first=0):
        p = np.ascontiguousarray(pos3, dtype=np.float64)
        assert p.ndim == 2 and p.shape[0] == 3
        _status(library().afe_follower_set_hold(self._h, int(first), p.shape[1], p.ctypes.data))

    def set_goal(self, pos3, first=0):
        p = np.ascontiguousarray(pos3, dtype=np.float64)
        assert p.ndim == 2 and p.shape[0] == 3
        _status(library().afe_follower_set_goal(self._h, int(first), p.shape[1], p.ctypes.data))

    _PLAN_FIELDS = (("planned", np.uint8, 0), ("coeffs", np.float64, 18), ("tf", np.float64, 0), ("t_plan_us", np.uint64, 0),
                    ("traj_att", np.float64, 4), ("offset", np.float64, 3), ("grav", np.float64, 3))

    def set_plans(self, first=0, count=None, **fields):
        """planned uint8 [count], coeffs [18, count] (row k = coeffs[k // 3][k % 3]), tf [count], t_plan_us uint64 [count],
        traj_att [4, count], offset [3, count], grav [3, count]; what is not given stays as it is"""
        first, count = self._range(first, count)
        unknown = set(fields) - {k for k, _, _ in self._PLAN_FIELDS}
        if unknown:
            raise ValueError("unknown plan fields %r" % sorted(unknown))
        keep, ptrs = [], []
        for name, dtype, comps in self._PLAN_FIELDS:
            if fields.get(name) is None:
                ptrs.append(None)
                continue
            a = np.ascontiguousarray(fields[name], dtype=dtype)
            if a.shape != ((comps, count) if comps else (count,)):
                raise ValueError("%s must have shape %r" % (name, (comps, count) if comps else (count,)))
            keep.append(a)
            ptrs.append(a.ctypes.data)
        _status(library().afe_follower_set_plans(self._h, first, count, *ptrs))

    def get_plans(self, first=0, count=None):
        first, count = self._range(first, count)
        out = {name: np.empty((comps, count) if comps else (count,), dtype) for name, dtype, comps in self._PLAN_FIELDS}
        _status(library().afe_follower_get_plans(self._h, first, count, *[out[name].ctypes.data for name, _, _ in self._PLAN_FIELDS]))
        return out

    def planner_inputs(self):
        """-> dict(vel0, acc0, grav, cost_vec), [3, n] each, formed on the device from the slabs"""
        out = {k: np.empty((3, self.n)) for k in ("vel0", "acc0", "grav", "cost_vec")}
        _status(library().afe_follower_planner_inputs(self._h, *[a.ctypes.data for a in out.values()]))
        return out

    def plan(self, cfg, depth_images, samples, want_out=False, want_flags=False):
        """depth_images: a DeviceBuffer holding one image per vehicle (Scene.render_engine's).  -> (n_found, PlanOutput array
        or None, flags or None, kernel_ms)"""
        s = np.ascontiguousarray(samples, dtype=np.float64)
        assert s.ndim == 2 and s.shape[1] == 4
        out = (PlanOutput * self.n)() if want_out else None
        flags = np.zeros((self.n, s.shape[0]), np.uint8) if want_flags else None
        n_found, ms = C.c_int64(), C.c_float()
        ptr = depth_images.ptr if isinstance(depth_images, DeviceBuffer) else depth_images
        _status(library().afe_follower_plan(self._h, C.byref(cfg), ptr, s.ctypes.data, s.shape[0],
                                            None if out is None else C.cast(out, C.c_void_p),
                                            None if flags is None else flags.ctypes.data, C.byref(n_found), C.byref(ms)))
        return n_found.value, out, flags, ms.value

    def tick(self, count_tracking=False):
        """one offboard period; -> vehicles on a running plan (count_tracking) or None (then nothing is downloaded)"""
        if not count_tracking:
            _status(library().afe_follower_tick(self._h, None))
            return None
        k = C.c_int64()
        _status(library().afe_follower_tick(self._h, C.byref(k)))
        return k.value

    def get_reference(self, first=0, count=None):
        """-> [14, count]: position 3, velocity 3, acceleration 3, thrust, body rates 3, running"""
        first, count = self._range(first, count)
        out = np.empty((14, count))
        _status(library().afe_follower_get_reference(self._h, first, count, out.ctypes.data))
        return out

    def get_command(self, first=0, count=None):
        """-> (computed [4, count], sent [4, count]) float32: thrust and body rates before and after the radio codec"""
        first, count = self._range(first, count)
        computed, sent = np.empty((4, count), np.float32), np.empty((4, count), np.float32)
        _status(library().afe_follower_get_command(self._h, first, count, computed.ctypes.data, sent.ctypes.data))
        return computed, sent

    def info(self):
        nv, sl, nt, fl = C.c_int64(), C.c_int(), C.c_uint64(), C.c_int()
        _status(library().afe_follower_info(self._h, C.byref(nv), C.byref(sl), C.byref(nt), C.byref(fl)))
        return {"n_vehicles": nv.value, "slots": sl.value, "n_ticks": nt.value, "in_flight": fl.value}

    def attach_estimator(self, est):
        """afe_follower_attach_estimator: plan, planner_inputs and tick read the estimator's prediction in place of the
        truth, and a tick announces its command to it; None detaches.  Close the follower before the estimator."""
        _status(library().afe_follower_attach_estimator(self._h, None if est is None else est._h))
        self._est = est

    def attach_gps_estimator(self, gps):
        """afe_follower_attach_gps_estimator: plan, planner_inputs and tick read the GPS + IMU estimator's current estimate
        in place of the truth and announce nothing; None detaches.  Close the follower before the estimator."""
        _status(library().afe_follower_attach_gps_estimator(self._h, None if gps is None else gps._h))
        self._gps = gps

    def close(self):
        if getattr(self, "_h", None):
            library().afe_follower_destroy(self._h)
            self._h = C.c_void_p()
            self._keep = None
            self._est = None
            self._gps = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stages_default_config(quadcopter_type):
    """afe_stages_default_config: the field node's mission constants and the controller's tuning for the type.  Pure host."""
    c = StagesConfig()
    _status(library().afe_stages_default_config(int(quadcopter_type), C.byref(c)))
    return c


STAGES_MATH_OPS = {"sin": 0, "cos": 1, "sinf": 2, "cosf": 3, "asinf": 4, "acosf": 5}


def stages_selftest_math(op, x, device=-1):
    """afe_stages_selftest_math: the device library's sin / cos (float64) or sinf / cosf / asinf / acosf (float32) of x, as
    the stage machine's kernel calls them; op is a name or 0..5"""
    op = STAGES_MATH_OPS.get(op, op)
    a = np.ascontiguousarray(x, dtype=np.float64 if op < 2 else np.float32)
    y = np.empty_like(a)
    _status(library().afe_stages_selftest_math(int(device), int(op), a.size, a.ctypes.data, y.ctypes.data))
    return y


class FlightStages:
    """afe_stages: the field node's mission -- wait, spool up, take off, fly, land, idle -- with its safety net, position
    controller, radio codec and delay line for every vehicle of an ensemble, on the device (see the header).  Borrows the
    ensemble and an attached estimator: close the stage machine first."""

    _FIELDS = (("stage", np.uint8, 0), ("last_stage", np.uint8, 0), ("t0_us", np.uint64, 0), ("safety", np.uint8, 0),
               ("ready", np.uint8, 0), ("init_pos", np.float64, 3), ("desired_pos", np.float64, 3), ("last_pos", np.float64, 3),
               ("last_vel", np.float64, 3), ("last_acc", np.float64, 3), ("cmd_yaw", np.float64, 0), ("computed", np.float32, 4),
               ("sent", np.float32, 4), ("msg_type", np.uint8, 0))

    def __init__(self, ensemble, cfg=None, quadcopter_type=5):
        self.cfg = stages_default_config(quadcopter_type) if cfg is None else cfg
        self._h = C.c_void_p()
        self.n = ensemble.n
        self._keep = ensemble
        self._gps = None
        _status(library().afe_stages_create(ensemble.handle, C.byref(self.cfg), C.byref(self._h)))

    def _rows(self, a, comps, first):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape[:-1] == ((comps,) if comps else ())
        return a, int(first), a.shape[-1]

    def set_desired_position(self, pos3, first=0):
        a, first, count = self._rows(pos3, 3, first)
        _status(library().afe_stages_set_desired_position(self._h, first, count, a.ctypes.data))

    def set_desired_yaw(self, yaw, first=0):
        a, first, count = self._rows(yaw, 0, first)
        _status(library().afe_stages_set_desired_yaw(self._h, first, count, a.ctypes.data))

    def set_centre(self, xy2, first=0):
        a, first, count = self._rows(xy2, 2, first)
        _status(library().afe_stages_set_centre(self._h, first, count, a.ctypes.data))

    def set_unsafe(self, first=0, count=None):
        """SetExternalPanic for vehicles [first, first + count): userUnsafe, for good"""
        _status(library().afe_stages_set_unsafe(self._h, int(first), int(self.n - first if count is None else count)))

    def request(self, start=False, stop=False, first=0, count=None):
        """the per-vehicle start / stop request that is OR-ed with a tick's arguments; it stays until changed"""
        _status(library().afe_stages_request(self._h, int(first), int(self.n - first if count is None else count), int(bool(start)), int(bool(stop))))

    def set_warnings(self, warnings, first=0):
        w = np.ascontiguousarray(warnings, dtype=np.uint8)
        assert w.ndim == 1
        _status(library().afe_stages_set_warnings(self._h, int(first), w.size, w.ctypes.data))

    def tick(self, should_start=False, should_stop=False, count=False):
        """one period of Run(shouldStart, shouldStop); -> int64 [8]: vehicles per stage and the ready ones (count), or None
        (then nothing is downloaded and the call does not wait)"""
        if not count:
            _status(library().afe_stages_tick(self._h, int(bool(should_start)), int(bool(should_stop)), None))
            return None
        c = np.zeros(8, np.int64)
        _status(library().afe_stages_tick(self._h, int(bool(should_start)), int(bool(should_stop)), c.ctypes.data))
        return c

    def get(self, first=0, count=None, fields=None):
        """-> dict of the machine's per-vehicle state (all of _FIELDS, or those named), planar [comps, count]"""
        first = int(first)
        count = int(self.n - first if count is None else count)
        names = [f[0] for f in self._FIELDS] if fields is None else list(fields)
        out, req = {}, StagesFields()
        req.struct_bytes = C.sizeof(StagesFields)
        for name, dtype, comps in self._FIELDS:
            if name in names:
                out[name] = np.empty((comps, count) if comps else (count,), dtype)
                setattr(req, name + ("3" if comps == 3 else "4" if comps == 4 else ""), out[name].ctypes.data)
        if len(out) != len(names):
            raise ValueError("unknown fields %r" % sorted(set(names) - set(out)))
        _status(library().afe_stages_get(self._h, first, count, C.byref(req)))
        return out

    def info(self):
        nv, sl, nt, fl = C.c_int64(), C.c_int(), C.c_uint64(), C.c_int()
        _status(library().afe_stages_info(self._h, C.byref(nv), C.byref(sl), C.byref(nt), C.byref(fl)))
        return {"n_vehicles": nv.value, "slots": sl.value, "n_ticks": nt.value, "in_flight": fl.value}

    def attach_gps_estimator(self, gps):
        """afe_stages_attach_gps_estimator: a tick reads the GPS + IMU estimator's current estimate in place of the truth, and
        the safety net its time since the last good measurement; None detaches.  Close the stage machine before the estimator."""
        _status(library().afe_stages_attach_gps_estimator(self._h, None if gps is None else gps._h))
        self._gps = gps

    def close(self):
        if getattr(self, "_h", None):
            library().afe_stages_destroy(self._h)
            self._h = C.c_void_p()
            self._keep = None
            self._gps = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def onboard_default_config(quadcopter_type):
    """afe_onboard_default_config: QuadcopterLogic::Initialise's cut-offs, the attitude controller's time constants, the battery
    threshold and the radio period for the type.  Pure host."""
    c = OnboardConfig()
    _status(library().afe_onboard_default_config(int(quadcopter_type), C.byref(c)))
    return c


ONBOARD_MATH_OPS = {"sinf": 0, "cosf": 1, "acosf": 2, "asinf": 3, "atan2f": 4}


def onboard_selftest_math(op, x, x2=None, device=-1):
    """afe_onboard_selftest_math: the device library's sinf / cosf / acosf / asinf of x, or atan2f(x, x2), as the onboard
    computer's kernel calls them; op is a name or 0..4"""
    op = ONBOARD_MATH_OPS.get(op, op)
    a = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty_like(a)
    if op == 4:
        arg = np.ascontiguousarray(np.stack([a.ravel(), np.ascontiguousarray(x2, dtype=np.float32).ravel()]))
    else:
        arg = a
    _status(library().afe_onboard_selftest_math(int(device), int(op), a.size, arg.ctypes.data, y.ctypes.data))
    return y


class Onboard:
    """afe_onboard: the vehicle's own flight computer -- attitude estimate, radio parsing with sticky PANIC / KILLED, telemetry
    warnings, panic checks, the external-acceleration controller and the telemetry packets -- for every vehicle of an ensemble,
    on the device (see the header).  cfgs: one OnboardConfig per type record (default: quadcopter_type's for every record).
    Borrows the ensemble: close the onboard computer first."""

    _FIELDS = (("flight_state", np.uint8, 0), ("panic_reason", np.uint8, 0), ("warnings", np.uint8, 0), ("est_att", np.float32, 4),
               ("est_ang_vel", np.float32, 3), ("acc_filtered", np.float32, 3), ("batt_filtered", np.float32, 0),
               ("main_loop_dt", np.float32, 0), ("cmd_dt", np.float32, 0), ("motor_forces", np.float32, 4),
               ("cycle_counter", np.uint32, 0), ("last_radio_us", np.uint64, 0), ("motors_running", np.uint8, 0))
    _STATE = (("est_att4", np.float32, 4), ("est_ang_vel3", np.float32, 3), ("imu_initialized", np.uint8, 0), ("lowpass20", np.float32, 20),
              ("flight_state", np.uint8, 0), ("motors_running", np.uint8, 0), ("last_radio_us", np.uint64, 0))

    def __init__(self, ensemble, cfgs=None, quadcopter_type=5, n_types=1):
        if cfgs is None:
            cfgs = [onboard_default_config(quadcopter_type) for _ in range(n_types)]
        self.cfgs = list(cfgs)
        table = (OnboardConfig * len(self.cfgs))(*self.cfgs)
        self._h = C.c_void_p()
        self.n = ensemble.n
        self._keep = ensemble
        _status(library().afe_onboard_create(ensemble.handle, table, len(self.cfgs), C.byref(self._h)))

    def _range(self, first, count):
        first = int(first)
        return first, int(self.n - first if count is None else count)

    def set_battery(self, volts, first=0):
        a = np.ascontiguousarray(volts, dtype=np.float32)
        assert a.ndim == 1
        _status(library().afe_onboard_set_battery(self._h, int(first), a.size, a.ctypes.data))

    def radio(self, raw_packets, first=0):
        """SetCommandRadioMsg: raw_packets uint8 [count, RADIO_PACKET_SIZE]; types 2, 4, 5, 6"""
        a = np.ascontiguousarray(raw_packets, dtype=np.uint8)
        assert a.ndim == 2 and a.shape[1] == RADIO_PACKET_SIZE
        _status(library().afe_onboard_radio(self._h, int(first), a.shape[0], a.ctypes.data))

    def tick(self, count=False):
        """one Run() behind the step that fired the logic tick; -> int64 [16]: vehicles per flight state [0..6], per first panic
        reason [7..14], with any warning [15] (count), or None (then nothing is downloaded and the call does not wait)"""
        if not count:
            _status(library().afe_onboard_tick(self._h, None))
            return None
        c = np.zeros(16, np.int64)
        _status(library().afe_onboard_tick(self._h, c.ctypes.data))
        return c

    def get(self, first=0, count=None, fields=None):
        """-> dict of the computer's per-vehicle state (all of _FIELDS, or those named), planar [comps, count]"""
        first, count = self._range(first, count)
        names = [f[0] for f in self._FIELDS] if fields is None else list(fields)
        out, req = {}, OnboardFields()
        req.struct_bytes = C.sizeof(OnboardFields)
        for name, dtype, comps in self._FIELDS:
            if name in names:
                out[name] = np.empty((comps, count) if comps else (count,), dtype)
                setattr(req, name + (str(comps) if comps else ""), out[name].ctypes.data)
        if len(out) != len(names):
            raise ValueError("unknown fields %r" % sorted(set(names) - set(out)))
        _status(library().afe_onboard_get(self._h, first, count, C.byref(req)))
        return out

    def set_state(self, first=0, **fields):
        """afe_onboard_set_state: est_att4, est_ang_vel3, imu_initialized, lowpass20, flight_state, motors_running, last_radio_us;
        planar [comps, count], what is not named is left as it is"""
        req, keep, count = OnboardState(), [], None
        req.struct_bytes = C.sizeof(OnboardState)
        for name, dtype, comps in self._STATE:
            if name in fields:
                a = np.ascontiguousarray(fields.pop(name), dtype=dtype)
                assert a.shape[:-1] == ((comps,) if comps else ()) and count in (None, a.shape[-1])
                count = a.shape[-1]
                keep.append(a)
                setattr(req, name, a.ctypes.data)
        if fields:
            raise ValueError("unknown fields %r" % sorted(fields))
        _status(library().afe_onboard_set_state(self._h, int(first), int(count or 0), C.byref(req)))

    def telemetry(self, first=0, count=None):
        """GetTelemetryDataPackets -> uint8 [count, 2, TELEMETRY_PACKET_SIZE]; the range's packet counters advance and its
        warnings are cleared"""
        first, count = self._range(first, count)
        out = np.zeros((count, 2, TELEMETRY_PACKET_SIZE), np.uint8)
        _status(library().afe_onboard_telemetry(self._h, first, count, out.ctypes.data))
        return out

    def info(self):
        nv, nt, lt = C.c_int64(), C.c_uint64(), C.c_uint64()
        _status(library().afe_onboard_info(self._h, C.byref(nv), C.byref(nt), C.byref(lt)))
        return {"n_vehicles": nv.value, "n_ticks": nt.value, "last_tick": lt.value}

    def close(self):
        """afe_onboard_destroy withdraws the mailbox from the engine: if the ensemble was closed first (the wrong order) the
        engine is gone and the handle is dropped without the call (its device memory went with the engine's context)"""
        if getattr(self, "_h", None):
            if self._keep is not None and getattr(self._keep, "_h", None):
                library().afe_onboard_destroy(self._h)
            self._h = C.c_void_p()
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def estimator_default_config():
    """afe_estimator_default_config: MocapStateEstimator's statistics and the loop's cadences.  Pure host."""
    c = EstimatorConfig()
    _status(library().afe_estimator_default_config(C.byref(c)))
    return c


def estimator_ring_slots(cfg):
    """afe_estimator_ring_slots: slots of the command ring for a configuration.  Pure host."""
    k = C.c_int()
    _status(library().afe_estimator_ring_slots(C.byref(cfg), C.byref(k)))
    return k.value


ESTIMATOR_MATH_OPS = {"sin": 0, "cos": 1, "asin": 2, "acos": 3, "exp": 4}


def estimator_selftest_math(op, x, device=-1):
    """afe_estimator_selftest_math: the device library's sin / cos / asin / acos / exp (float64) of x, as the estimator's
    kernels call them; op is a name or 0..4"""
    op = ESTIMATOR_MATH_OPS.get(op, op)
    a = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(a)
    _status(library().afe_estimator_selftest_math(int(device), int(op), a.size, a.ctypes.data, y.ctypes.data))
    return y


class Estimator:
    """afe_estimator: Offboard::MocapStateEstimator and its PredictionPipe for every vehicle of an ensemble, on the device
    (see the header).  Borrows the ensemble: close a follower it is attached to first, then the estimator."""

    def __init__(self, ensemble, cfg=None):
        self.cfg = estimator_default_config() if cfg is None else cfg
        self._h = C.c_void_p()
        self.n = ensemble.n
        self._keep = ensemble
        _status(library().afe_estimator_create(ensemble.handle, C.byref(self.cfg), C.byref(self._h)))

    def _range(self, first, count):
        return int(first), int(self.n - first if count is None else count)

    def measure(self, count_rejected=False):
        """UpdateWithMeasurement(the engine's pose now); -> measurements rejected by this call (count_rejected) or None
        (then nothing is downloaded and the call does not wait)"""
        if not count_rejected:
            _status(library().afe_estimator_measure(self._h, None))
            return None
        k = C.c_int64()
        _status(library().afe_estimator_measure(self._h, C.byref(k)))
        return k.value

    def predict(self, ahead=0.03):
        """GetPrediction(ahead) into the prediction buffer, stamped with the engine's time"""
        _status(library().afe_estimator_predict(self._h, float(ahead)))

    def prediction(self, first=0, count=None):
        """-> [13, count]: position 3, velocity 3, attitude 4, body rates 3 of the last predict"""
        first, count = self._range(first, count)
        out = np.empty((13, count))
        _status(library().afe_estimator_get_prediction(self._h, first, count, out.ctypes.data))
        return out

    def announce(self, ang_vel, acc, first=0):
        """SetPredictedValues(ang_vel [3, count], acc [3, count]): one new message for the whole ensemble"""
        w = np.ascontiguousarray(ang_vel, dtype=np.float64)
        a = np.ascontiguousarray(acc, dtype=np.float64)
        assert w.ndim == 2 and w.shape[0] == 3 and a.shape == w.shape
        _status(library().afe_estimator_announce(self._h, int(first), w.shape[1], w.ctypes.data, a.ctypes.data))

    def state(self, first=0, count=None):
        """-> dict(est [13, count], cov [6, count] (P.vv, P.vr, P.rr, A.vv, A.vr, A.rr), valid_at_us, started,
        rejected_in_a_row, rejected)"""
        first, count = self._range(first, count)
        out = {"est": np.empty((13, count)), "cov": np.empty((6, count)), "valid_at_us": np.empty(count, np.uint64),
               "started": np.empty(count, np.uint8), "rejected_in_a_row": np.empty(count, np.uint32),
               "rejected": np.empty(count, np.uint32)}
        _status(library().afe_estimator_get_state(self._h, first, count, *[a.ctypes.data for a in out.values()]))
        return out

    def reset(self, first=0, count=None):
        first, count = self._range(first, count)
        _status(library().afe_estimator_reset(self._h, first, count))

    def info(self):
        nv, sl, nm, ng, er = C.c_int64(), C.c_int(), C.c_uint64(), C.c_int(), C.c_uint32()
        _status(library().afe_estimator_info(self._h, C.byref(nv), C.byref(sl), C.byref(nm), C.byref(ng), C.byref(er)))
        return {"n_vehicles": nv.value, "slots": sl.value, "n_measures": nm.value, "n_messages": ng.value, "error": er.value}

    def close(self):
        if getattr(self, "_h", None):
            library().afe_estimator_destroy(self._h)
            self._h = C.c_void_p()
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gps_estimator_default_config():
    """afe_gps_estimator_default_config: GPSIMUStateEstimator's statistics and the logic's accelerometer cutoff.  Pure host."""
    c = GpsEstimatorConfig()
    _status(library().afe_gps_estimator_default_config(C.byref(c)))
    return c


GPS_ESTIMATOR_MATH_OPS = {"sin": 0, "cos": 1, "acosf": 2}


def gps_estimator_selftest_math(op, x, device=-1):
    """afe_gps_estimator_selftest_math: the device library's sin / cos (float64) and acosf (x narrowed to float32, the result
    widened) as the GPS + IMU estimator's kernels call them; op is a name or 0..2"""
    op = GPS_ESTIMATOR_MATH_OPS.get(op, op)
    a = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(a)
    _status(library().afe_gps_estimator_selftest_math(int(device), int(op), a.size, a.ctypes.data, y.ctypes.data))
    return y


class GpsEstimator:
    """afe_gps_estimator: Offboard::GPSIMUStateEstimator for every vehicle of an ensemble, on the device (see the header).
    Borrows the ensemble, which needs set_rates_logic: close a follower it is attached to first, then the estimator."""

    def __init__(self, ensemble, cfg=None):
        self.cfg = gps_estimator_default_config() if cfg is None else cfg
        self._h = C.c_void_p()
        self.n = ensemble.n
        self._keep = ensemble
        _status(library().afe_gps_estimator_create(ensemble.handle, C.byref(self.cfg), C.byref(self._h)))

    def _range(self, first, count):
        return int(first), int(self.n - first if count is None else count)

    def imu(self):
        """Predict(acc, gyro) with the sample of the latest logic tick: once per tick, right behind it.  Does not wait."""
        _status(library().afe_gps_estimator_imu(self._h))

    def measure(self, count_reinitialised=False):
        """UpdateWithMeasurement(the engine's position now); -> vehicles that took the singular branch in this call
        (count_reinitialised) or None (then nothing is downloaded and the call does not wait)"""
        if not count_reinitialised:
            _status(library().afe_gps_estimator_measure(self._h, None))
            return None
        k = C.c_int64()
        _status(library().afe_gps_estimator_measure(self._h, C.byref(k)))
        return k.value

    def state(self, first=0, count=None):
        """-> dict(est [13, count], cov [81, count] row major, last_predict_us, last_update_us, initialized, num_resets)"""
        first, count = self._range(first, count)
        out = {"est": np.empty((13, count)), "cov": np.empty((81, count)), "last_predict_us": np.empty(count, np.uint64),
               "last_update_us": np.empty(count, np.uint64), "initialized": np.empty(count, np.uint8),
               "num_resets": np.empty(count, np.uint32)}
        _status(library().afe_gps_estimator_get_state(self._h, first, count, *[a.ctypes.data for a in out.values()]))
        return out

    def set_state(self, est=None, cov=None, corr=None, first=0):
        """est [13, count], cov [81, count], corr [3, count] (_lastMeasUpdateAttCorrection); None leaves a part as it is.
        The vehicles are marked initialised."""
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (est, cov, corr)]
        count = next(a.shape[1] for a in arrs if a is not None)
        for a, comps in zip(arrs, (13, 81, 3)):
            assert a is None or a.shape == (comps, count)
        _status(library().afe_gps_estimator_set_state(self._h, int(first), count, *[None if a is None else a.ctypes.data for a in arrs]))

    def reset(self, first=0, count=None):
        first, count = self._range(first, count)
        _status(library().afe_gps_estimator_reset(self._h, first, count))

    def info(self):
        nv, ni, nm, lt = C.c_int64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        _status(library().afe_gps_estimator_info(self._h, C.byref(nv), C.byref(ni), C.byref(nm), C.byref(lt)))
        return {"n_vehicles": nv.value, "n_imu": ni.value, "n_measures": nm.value, "last_tick": lt.value}

    def close(self):
        if getattr(self, "_h", None):
            library().afe_gps_estimator_destroy(self._h)
            self._h = C.c_void_p()
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def type_from_id(vehicle_id):
    return library().afe_type_from_id(int(vehicle_id))


def plan_ticks(logic_period, elapsed_us, dt_us, n_steps):
    """(ticks[n_steps], new elapsed_us): pure host, no GPU needed."""
    el = C.c_uint64(int(elapsed_us))
    out = np.zeros(n_steps, np.uint8)
    rc = library().afe_plan_ticks(float(logic_period), C.byref(el), int(dt_us), int(n_steps),
                                  out.ctypes.data)
    if rc:
        raise AfeError(rc, "afe_plan_ticks")
    return out, el.value


def _planar(a, comps, count, dtype):
    if a is None:
        return None, None
    arr = np.ascontiguousarray(a, dtype=dtype)
    if arr.shape != (comps, count):
        raise ValueError("expected planar array of shape (%d, %d), got %r" % (comps, count, arr.shape))
    return arr, arr.ctypes.data


class Ensemble:
    """One engine = one vehicle ensemble (or one rank's shard of it) on one GPU."""

    def __init__(self, n_vehicles, precision=AFE_F32, device=-1, first_global_index=0, _borrowed=None, host_visible=False):
        """host_visible: afe_create_host_visible -- the state arena in pinned host memory (small ensembles with the host in
        the loop of every step: getters and setters become host copies and leave a resident grid where it is)."""
        self._L = library()
        self._owned = _borrowed is None
        if _borrowed is not None:   # a shard of a Group: the group owns the engine
            self._h = _borrowed
            self.n = int(n_vehicles)
            self.precision = precision
            self.first_global_index = int(first_global_index)
            return
        self._h = C.c_void_p()
        create = self._L.afe_create_host_visible if host_visible else self._L.afe_create
        rc = create(C.byref(self._h), int(n_vehicles), int(precision), int(device), int(first_global_index))
        if rc:
            self._h = None
            raise AfeError(rc, self._L.afe_status_string(rc).decode() +
                           " (the HIP engine needs an MI355X / gfx950 device; there is no CPU fallback)")
        self.n = int(n_vehicles)
        self.precision = precision
        self.first_global_index = int(first_global_index)

    # -- plumbing ---------------------------------------------------------
    def _ck(self, rc):
        if rc:
            raise AfeError(rc, self._L.afe_last_error(self._h).decode() or
                           self._L.afe_status_string(rc).decode())

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                self._L.afe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    def _range(self, first, count):
        first = int(first)
        count = self.n - first if count is None else int(count)
        return first, count

    # -- configuration ----------------------------------------------------
    def set_type_table(self, params_list):
        arr = (VehicleParams * len(params_list))()
        for i, p in enumerate(params_list):
            C.memmove(C.byref(arr[i]), C.byref(p), C.sizeof(VehicleParams))
        self._ck(self._L.afe_set_type_table(self._h, arr, len(params_list)))

    def set_vehicle_types(self, type_index, first=0):
        t = np.ascontiguousarray(type_index, dtype=np.uint8)
        self._ck(self._L.afe_set_vehicle_types(self._h, int(first), t.size, t.ctypes.data))

    def set_logic_period(self, seconds):
        self._ck(self._L.afe_set_logic_period(self._h, float(seconds)))

    def set_imu_noise(self, enabled=True, sigma_gyro=0.1, sigma_acc=0.2,
                      seed_policy=AFE_SEED_REFERENCE):
        self._ck(self._L.afe_set_imu_noise(self._h, int(bool(enabled)), float(sigma_gyro),
                                           float(sigma_acc), int(seed_policy)))

    def set_stream(self, hip_stream):
        """afe_set_stream: all engine work goes to the caller's HIP stream `hip_stream` (an integer handle, e.g.
        torch.cuda.Stream().cuda_stream), which must stay alive until the engine is closed or taken off it again.
        None or 0 restores the engine's OWN stream -- torch's default stream has handle 0 and is NOT meant by it.  The
        default stream is not supported as a caller's stream (HIP's reserved handles 1 and 2 are refused): queue the
        host's work on a torch.cuda.Stream() of its own.  See the header for what is ordered."""
        self._ck(self._L.afe_set_stream(self._h, C.c_void_p(int(hip_stream) if hip_stream else None)))

    # -- state ------------------------------------------------------------
    def set_state(self, pos=None, vel=None, att=None, ang_vel=None, motor_speed=None,
                  first=0, count=None, dtype=np.float64):
        first, count = self._range(first, count)
        fn = self._L.afe_set_state if dtype == np.float64 else self._L.afe_set_state_f32
        keep = [_planar(a, c, count, dtype) for a, c in
                ((pos, 3), (vel, 3), (att, 4), (ang_vel, 3), (motor_speed, 4))]
        self._ck(fn(self._h, first, count, *[k[1] for k in keep]))

    def get_state(self, first=0, count=None, dtype=np.float64):
        first, count = self._range(first, count)
        fn = self._L.afe_get_state if dtype == np.float64 else self._L.afe_get_state_f32
        out = dict(pos=np.empty((3, count), dtype), vel=np.empty((3, count), dtype),
                   att=np.empty((4, count), dtype), ang_vel=np.empty((3, count), dtype),
                   motor_speed=np.empty((4, count), dtype))
        self._ck(fn(self._h, first, count, out["pos"].ctypes.data, out["vel"].ctypes.data,
                    out["att"].ctypes.data, out["ang_vel"].ctypes.data,
                    out["motor_speed"].ctypes.data))
        return out

    def set_rng_state(self, state, first=0):
        s = np.ascontiguousarray(state, dtype=np.uint32)
        self._ck(self._L.afe_set_rng_state(self._h, int(first), s.size, s.ctypes.data))

    def get_rng_state(self, first=0, count=None):
        first, count = self._range(first, count)
        s = np.empty(count, np.uint32)
        self._ck(self._L.afe_get_rng_state(self._h, first, count, s.ctypes.data))
        return s

    # -- inputs -----------------------------------------------------------
    def set_motor_cmds(self, cmd4, first=0, count=None):
        first, count = self._range(first, count)
        arr, ptr = _planar(cmd4, 4, count, np.float32)
        self._ck(self._L.afe_set_motor_cmds(self._h, first, count, ptr))

    def set_external_force(self, force3, first=0, count=None):
        first, count = self._range(first, count)
        arr, ptr = _planar(force3, 3, count, np.float64)
        self._ck(self._L.afe_set_external_force(self._h, first, count, ptr))

    def set_external_torque(self, torque3, first=0, count=None):
        first, count = self._range(first, count)
        arr, ptr = _planar(torque3, 3, count, np.float64)
        self._ck(self._L.afe_set_external_torque(self._h, first, count, ptr))

    # -- on-device onboard rates logic (f1) ---------------------------------
    def set_rates_logic(self, params_list):
        """enable (list of RatesLogicParams, one per vehicle type) or disable (None)"""
        if params_list is None:
            self._ck(self._L.afe_set_rates_logic(self._h, None, 0))
            return
        arr = (RatesLogicParams * len(params_list))()
        for i, p in enumerate(params_list):
            C.memmove(C.byref(arr[i]), C.byref(p), C.sizeof(RatesLogicParams))
        self._ck(self._L.afe_set_rates_logic(self._h, arr, len(params_list)))

    def set_rates_commands(self, thrust_norm, ang_vel3, first=0, count=None):
        first, count = self._range(first, count)
        t = np.ascontiguousarray(thrust_norm, dtype=np.float32)
        if t.shape != (count,):
            raise ValueError("thrust_norm must have shape (%d,)" % count)
        w, wp = _planar(ang_vel3, 3, count, np.float32)
        self._ck(self._L.afe_set_rates_commands(self._h, first, count, t.ctypes.data, wp))

    def get_rates_commands(self, first=0, count=None):
        """-> (thrust_norm [count], ang_vel [3, count]) float32, have [count] uint8: the rates command in force"""
        first, count = self._range(first, count)
        t, w, h = np.empty(count, np.float32), np.empty((3, count), np.float32), np.empty(count, np.uint8)
        self._ck(self._L.afe_get_rates_commands(self._h, first, count, t.ctypes.data, w.ctypes.data, h.ctypes.data))
        return t, w, h

    def set_commands_from_radio(self, raw_packets, first=0):
        """raw_packets: uint8 [count, 23]"""
        r = np.ascontiguousarray(raw_packets, dtype=np.uint8)
        if r.ndim != 2 or r.shape[1] != RADIO_PACKET_SIZE:
            raise ValueError("raw_packets must have shape (count, 23)")
        self._ck(self._L.afe_set_commands_from_radio(self._h, int(first), r.shape[0], r.ctypes.data))

    def get_motor_cmds(self, first=0, count=None):
        first, count = self._range(first, count)
        out = np.empty((4, count), np.float32)
        self._ck(self._L.afe_get_motor_cmds(self._h, first, count, out.ctypes.data))
        return out

    # -- stepping ---------------------------------------------------------
    def step(self, dt_us, n_steps=1):
        self._ck(self._L.afe_step(self._h, int(dt_us), int(n_steps)))

    def set_addressing(self, force_global):
        """False (default): buffer resources when the arenas fit 32-bit offsets; True: global addresses always"""
        self._ck(self._L.afe_set_addressing(self._h, 1 if force_global else 0))

    def step_kernel_info(self):
        """(record path, addressing): ("kernel arguments" | "per-wave scalar loads" | "LDS table", "buffer" | "global")"""
        a, b = C.c_int(0), C.c_int(0)
        self._ck(self._L.afe_step_kernel_info(self._h, C.byref(a), C.byref(b)))
        return ("kernel arguments", "per-wave scalar loads", "LDS table")[a.value], ("buffer", "global")[b.value]

    def set_max_fused_steps(self, k):
        self._ck(self._L.afe_set_max_fused_steps(self._h, int(k)))

    def set_split_stepping(self, parts):
        """afe_set_split_stepping: 0 automatic (default), 1 off, 2 = the two halves of the ensemble step on two streams (see the header)"""
        self._ck(self._L.afe_set_split_stepping(self._h, int(parts)))

    def set_noise_seed(self, seed):
        self._ck(self._L.afe_set_noise_seed(self._h, int(seed)))

    def set_gust_process(self, enabled, seed=0, sigma_max=0.5, period_us=100000, n_global=0):
        """afe_set_gust_process: per-vehicle piecewise-constant wind gusts resampled on the device (BASELINE config 4)"""
        self._ck(self._L.afe_set_gust_process(self._h, int(bool(enabled)), int(seed), float(sigma_max), int(period_us), int(n_global)))

    def get_external_force(self, first=0, count=None):
        count = self.n - first if count is None else count
        out = np.empty((3, count), np.float64)
        self._ck(self._L.afe_get_external_force(self._h, int(first), int(count), out.ctypes.data))
        return out

    def set_step_mode(self, mode):
        """afe_set_step_mode: AFE_STEP_LAUNCH (0), AFE_STEP_PERSISTENT (1: one resident grid, afe_step only authorises steps), AFE_STEP_AUTO (2)"""
        self._ck(self._L.afe_set_step_mode(self._h, int(mode)))

    @property
    def steps_completed(self):
        """steps every vehicle has been advanced through (the resident grid's completion word; steps issued in launch mode)"""
        n = C.c_uint64(0)
        self._ck(self._L.afe_steps_completed(self._h, C.byref(n)))
        return n.value

    @property
    def persistent_running(self):
        r = C.c_int(0)
        self._ck(self._L.afe_persistent_running(self._h, C.byref(r)))
        return bool(r.value)

    def steps_until_tick(self, dt_us):
        n = C.c_int(0)
        self._ck(self._L.afe_steps_until_tick(self._h, int(dt_us), C.byref(n)))
        return n.value

    def sync(self):
        self._ck(self._L.afe_sync(self._h))

    @property
    def time_us(self):
        t = C.c_uint64(0)
        self._ck(self._L.afe_time_us(self._h, C.byref(t)))
        return t.value

    @property
    def logic_ticks(self):
        t = C.c_uint64(0)
        self._ck(self._L.afe_logic_ticks(self._h, C.byref(t)))
        return t.value

    def get_imu(self, first=0, count=None):
        first, count = self._range(first, count)
        gyro = np.empty((3, count), np.float32)
        acc = np.empty((3, count), np.float32)
        self._ck(self._L.afe_get_imu(self._h, first, count, gyro.ctypes.data, acc.ctypes.data))
        return gyro, acc

    def device_view(self):
        v = DeviceView()
        v.struct_bytes = C.sizeof(DeviceView)
        self._ck(self._L.afe_get_device_view(self._h, C.byref(v)))
        return v

    def grid_time(self):
        """(device seconds, steps) of the resident grids since the last call; ends the grid now resident"""
        ns, steps = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.afe_grid_time(self._h, C.byref(ns), C.byref(steps)))
        return ns.value * 1e-9, steps.value

    def set_cache_policy(self, policy):
        """-1 automatic, 0 default, 1 inputs / outputs nt, 2 everything nt, 3 everything nt + one range per XCD"""
        self._ck(self._L.afe_set_cache_policy(self._h, int(policy)))

    def set_resident_queue(self, mode):
        """-1 automatic (own queue up to 262 144 vehicles), 0 the HIP stream, 1 the engine's own queue"""
        self._ck(self._L.afe_set_resident_queue(self._h, int(mode)))

    @property
    def cache_policy_in_use(self):
        p = C.c_int(0)
        self._ck(self._L.afe_cache_policy_in_use(self._h, C.byref(p)))
        return p.value

    def algorithmic_bytes_per_step(self, imu_tick):
        b = C.c_double(0)
        self._ck(self._L.afe_algorithmic_bytes_per_step(self._h, int(bool(imu_tick)), C.byref(b)))
        return b.value

    # -- checkpoint / resume --------------------------------------------------
    CHECKPOINT_HEADER_BYTES = 27 * 8    # CheckpointHeader (afe_engine.cpp): 17 x uint64, 3 x double, 6 x uint64, 1 x double; the arena follows

    def save_checkpoint(self):
        n = C.c_uint64(0)
        self._ck(self._L.afe_checkpoint_size(self._h, C.byref(n)))
        buf = np.empty(n.value, np.uint8)
        self._ck(self._L.afe_save_checkpoint(self._h, buf.ctypes.data, n.value))
        return buf

    def load_checkpoint(self, buf):
        b = np.ascontiguousarray(buf, dtype=np.uint8)
        self._ck(self._L.afe_load_checkpoint(self._h, b.ctypes.data, b.size))

    # -- HIP events on the engine stream ------------------------------------
    def event(self):
        ev = C.c_void_p()
        rc = self._L.afe_event_create(C.byref(ev))
        if rc:
            raise AfeError(rc, "afe_event_create")
        return ev

    def record(self, ev):
        self._ck(self._L.afe_event_record(self._h, ev))

    def elapsed_ms(self, start, stop):
        ms = C.c_float(0)
        rc = self._L.afe_event_elapsed_ms(start, stop, C.byref(ms))
        if rc:
            raise AfeError(rc, "afe_event_elapsed_ms")
        return ms.value

    def destroy_event(self, ev):
        self._L.afe_event_destroy(ev)

    def selftest_normals(self, seeds, dtype=np.float64):
        """(normals[n, 6], state_after[n] uint32) from the device generator: float64 = the AFE_F64
        engine's (libstdc++'s doubles), float32 = the AFE_F32 engine's (float multiplier)"""
        s = np.ascontiguousarray(seeds, dtype=np.uint32)
        out = np.empty((s.size, 6), dtype)
        st = np.empty(s.size, np.uint32)
        fn = self._L.afe_selftest_normals if dtype == np.float64 else self._L.afe_selftest_normals_f32
        self._ck(fn(self._h, s.ctypes.data, s.size, out.ctypes.data, st.ctypes.data))
        return out, st

    # -- shared-world exchange and queries ------------------------------------
    def pack_positions(self, device_ptr):
        self._ck(self._L.afe_pack_positions(self._h, C.c_void_p(int(device_ptr))))

    def gather_positions(self, comm, out_ptr, counts=None):
        """pack + RCCL all-gather on the engine's stream into a device buffer of 3*n_all floats"""
        cnt = None if counts is None else np.ascontiguousarray(counts, dtype=np.int64)
        rc = self._L.afe_gather_positions(self._h, comm.handle, None if cnt is None else cnt.ctypes.data,
                                          C.c_void_p(int(out_ptr)))
        if rc:
            raise AfeError(rc, (self._L.afe_comm_last_error(comm.handle) or b"").decode() or
                           self._L.afe_status_string(rc).decode())

    def nearest_neighbour(self, all_xyz_ptr, n_all, dist2_ptr, index_ptr, cell_size=0.0):
        self._ck(self._L.afe_nearest_neighbour_grid(self._h, C.c_void_p(int(all_xyz_ptr)), int(n_all), float(cell_size),
                                                    C.c_void_p(int(dist2_ptr)), C.c_void_p(int(index_ptr))))

    def nearest_neighbour_async(self, all_xyz_ptr, n_all, dist2_ptr, index_ptr):
        """afe_nearest_neighbour_async: the query on its own stream behind the gather; later steps are not ordered behind it"""
        self._ck(self._L.afe_nearest_neighbour_async(self._h, C.c_void_p(int(all_xyz_ptr)), int(n_all),
                                                     C.c_void_p(int(dist2_ptr)), C.c_void_p(int(index_ptr))))

    def query_sync(self):
        self._ck(self._L.afe_query_sync(self._h))

    def nearest_neighbour_bruteforce(self, all_xyz_ptr, n_all, queries_ptr, n_queries, dist2_ptr, index_ptr):
        self._ck(self._L.afe_nearest_neighbour_bruteforce(self._h, C.c_void_p(int(all_xyz_ptr)), int(n_all),
                                                          C.c_void_p(int(queries_ptr)), int(n_queries),
                                                          C.c_void_p(int(dist2_ptr)), C.c_void_p(int(index_ptr))))

    def set_neighbour_grid_refresh(self, every_n_queries):
        self._ck(self._L.afe_set_neighbour_grid_refresh(self._h, int(every_n_queries)))

    def set_neighbour_sort_reuse(self, every_n_queries):
        """sort the vehicles into the grid's cells every n-th query only; in between the order is kept and the positions
        refreshed (exact all the same: the device bounds the movement since the sort)"""
        self._ck(self._L.afe_set_neighbour_sort_reuse(self._h, int(every_n_queries)))

    def neighbour_grid_info(self):
        dims = (C.c_int * 3)()
        h, nc, nb = C.c_float(0), C.c_int64(0), C.c_int64(0)
        self._ck(self._L.afe_neighbour_grid_info(self._h, dims, C.byref(h), C.byref(nc), C.byref(nb)))
        return {"dims": tuple(dims), "cell_size": h.value, "n_cells": nc.value, "n_bruteforce": nb.value}


class Comm:
    """afe_comm: an RCCL communicator for the one-process-per-GPU layout."""

    @staticmethod
    def unique_id():
        uid = np.zeros(128, np.uint8)
        rc = library().afe_comm_unique_id(uid.ctypes.data)
        if rc:
            raise AfeError(rc, "afe_comm_unique_id (is RCCL loadable?)")
        return uid

    def __init__(self, unique_id, rank, n_ranks, device=-1):
        self._h = C.c_void_p()
        uid = np.ascontiguousarray(unique_id, dtype=np.uint8)
        assert uid.size == 128
        rc = library().afe_comm_create(C.byref(self._h), uid.ctypes.data, int(rank), int(n_ranks), int(device))
        if rc:
            self._h = None
            raise AfeError(rc, "afe_comm_create: " + library().afe_status_string(rc).decode())

    @property
    def handle(self):
        return self._h

    def info(self):
        r, n = C.c_int(0), C.c_int(0)
        rc = library().afe_comm_info(self._h, C.byref(r), C.byref(n))
        if rc:
            raise AfeError(rc, "afe_comm_info")
        return r.value, n.value

    def close(self):
        if getattr(self, "_h", None):
            library().afe_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Group:
    """afe_group: one process, several devices (or logical shards of one device)."""

    def __init__(self, n_vehicles, precision=AFE_F32, devices=(0,)):
        self._L = library()
        self._h = C.c_void_p()
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        rc = self._L.afe_group_create(C.byref(self._h), int(n_vehicles), int(precision), dev.ctypes.data, dev.size)
        if rc:
            self._h = None
            raise AfeError(rc, self._L.afe_status_string(rc).decode())
        self.n = int(n_vehicles)
        self.shards = []
        for k in range(dev.size):
            e, first, count = C.c_void_p(), C.c_int64(0), C.c_int64(0)
            self._ck(self._L.afe_group_shard(self._h, k, C.byref(e), C.byref(first), C.byref(count)))
            self.shards.append(Ensemble(count.value, precision, first_global_index=first.value, _borrowed=e))

    def _ck(self, rc):
        if rc:
            raise AfeError(rc, (self._L.afe_group_last_error(self._h) or b"").decode() or
                           self._L.afe_status_string(rc).decode())

    def ranges(self):
        return [(s.first_global_index, s.n) for s in self.shards]

    def peer_access(self):
        """True if every pair of the group's devices reads the other's memory directly"""
        ok = C.c_int(0)
        self._ck(self._L.afe_group_peer_access(self._h, C.byref(ok)))
        return bool(ok.value)

    def set_staged_copies(self, staged):
        """the gather's staged path (hipMemcpyPeerAsync row by row) even between peers; False: direct copies again"""
        self._ck(self._L.afe_group_set_staged_copies(self._h, 1 if staged else 0))

    def step(self, dt_us, n_steps=1):
        self._ck(self._L.afe_group_step(self._h, int(dt_us), int(n_steps)))

    def sync(self):
        self._ck(self._L.afe_group_sync(self._h))

    def gather_positions(self):
        """device pointers (one per shard) of the planar fp32 [3][n] gathered positions"""
        ptrs = (C.c_void_p * len(self.shards))()
        self._ck(self._L.afe_group_gather_positions(self._h, ptrs))
        return [int(p) for p in ptrs]

    def close(self):
        if getattr(self, "_h", None):
            for s in self.shards:
                s.close()
            self._L.afe_group_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class UwbNetwork:
    """afe_uwb_network == Simulation::UWBNetwork (UWBNetwork.cpp:8-89), batched."""

    def __init__(self, noise_std=0.0, outlier_prob=0.0, outlier_std=0.0):
        self._h = C.c_void_p()
        rc = library().afe_uwb_create(C.byref(self._h))
        if rc:
            raise AfeError(rc, "afe_uwb_create")
        library().afe_uwb_set_noise(self._h, float(noise_std), float(outlier_prob), float(outlier_std))

    def set_noise(self, noise_std, outlier_prob, outlier_std):
        library().afe_uwb_set_noise(self._h, float(noise_std), float(outlier_prob), float(outlier_std))

    def draw(self, n_pairs):
        """the stream alone: (noise_term float64[n], is_outlier uint8[n]); host only"""
        noise = np.empty(n_pairs, np.float64)
        out = np.empty(n_pairs, np.uint8)
        rc = library().afe_uwb_draw(self._h, int(n_pairs), noise.ctypes.data, out.ctypes.data)
        if rc:
            raise AfeError(rc, "afe_uwb_draw")
        return noise, out

    def range(self, ensemble, all_xyz_ptr, n_all, requester, responder):
        req = np.ascontiguousarray(requester, dtype=np.int32)
        res = np.ascontiguousarray(responder, dtype=np.int32)
        assert req.shape == res.shape and req.ndim == 1
        rng = np.empty(req.size, np.float32)
        out = np.empty(req.size, np.uint8)
        rc = library().afe_uwb_range(self._h, ensemble.handle, C.c_void_p(int(all_xyz_ptr)), int(n_all), req.ctypes.data,
                                     res.ctypes.data, req.size, rng.ctypes.data, out.ctypes.data)
        if rc:
            raise AfeError(rc, library().afe_status_string(rc).decode())
        return rng, out

    def close(self):
        if getattr(self, "_h", None):
            library().afe_uwb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
